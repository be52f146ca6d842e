"""numpy restatement of event-based (collar) scoring (include/eat_event_score.h, efficientat_amd/sed.py: evaluate_events):
the estimated events of a timeline by `detect_ref.timeline_events`, their conversion to samples with the clip to the
recording's length, the offset tolerance rule and sed_eval's reference-outer greedy matching.  Plain loops over Python
integers; nothing here shares code with the package.

A recording table `rec` is a list of rows (first window, window count, goff, G); reference rows are (class, onset, offset)
in samples, recording i owning rows [ro[i], ro[i + 1]) sorted by (class, onset)."""
import math

import numpy as np

from tests.detect_ref import timeline_events


def tolerances(events, c, pct):
    """Offset tolerance of every reference row: max(c, floor(pct * (offset - onset))), the product in fp64 -> list of int."""
    return [max(int(c), int(math.floor(float(pct) * float(int(off) - int(on))))) for _, on, off in np.asarray(events).tolist()]


def to_samples(frames, R, n):
    """[(on, off)] in frames -> [(on R, min(off R, n))] in samples (Python integers: no width to overflow)."""
    return [(int(on) * int(R), min(int(off) * int(R), int(n))) for on, off in frames]


def compatible(r, tol, e, c):
    return abs(r[0] - e[0]) <= c and abs(r[1] - e[1]) <= tol


def match_ref_outer(refs, tols, ests, c):
    """sed_eval's EventBasedMetrics: for each reference in row order, the first estimate in onset order that is compatible
    and not yet taken -> [(reference index, estimate index)]."""
    taken, pairs = set(), []
    for i, (r, tol) in enumerate(zip(refs, tols)):
        for j, e in enumerate(ests):
            if j not in taken and compatible(r, tol, e, c):
                taken.add(j)
                pairs.append((i, j))
                break
    return pairs


def match_est_outer(refs, tols, ests, c):
    """The other serial order: for each estimate in onset order, the first compatible reference not yet taken."""
    taken, pairs = set(), []
    for j, e in enumerate(ests):
        for i, (r, tol) in enumerate(zip(refs, tols)):
            if i not in taken and compatible(r, tol, e, c):
                taken.add(i)
                pairs.append((i, j))
                break
    return pairs


def class_rows(ref, ro, i, k):
    """Indices of recording i's reference rows of class k, in row order."""
    return [e for e in range(int(ro[i]), int(ro[i + 1])) if int(ref[e][0]) == k]


def score_ref(filt, rec, nsamp, R, ref, tol, ro, c, hi, lo, max_gap=0, min_len=0):
    """filt (K, G_total) float32 -> counts (n_rec, K, V, 2) int64 holding (tp, n_est) of every recording, class and
    threshold pair (hi[v], lo[v]), compared as float32."""
    filt = np.asarray(filt, dtype=np.float32)
    hi, lo = np.asarray(hi, dtype=np.float32).reshape(-1), np.asarray(lo, dtype=np.float32).reshape(-1)
    ref = np.asarray(ref).reshape(-1, 3).tolist()
    tol = [int(t) for t in np.asarray(tol).reshape(-1)]
    K, V = filt.shape[0], hi.shape[0]
    out = np.zeros((len(rec), K, V, 2), dtype=np.int64)
    for i, (_, _, goff, G) in enumerate(rec):
        for k in range(K):
            rows = class_rows(ref, ro, i, k)
            refs, tols = [(ref[e][1], ref[e][2]) for e in rows], [tol[e] for e in rows]
            x = filt[k, goff:goff + G]
            for v in range(V):
                ests = to_samples(timeline_events(x, hi[v], lo[v], max_gap, min_len), R, nsamp[i])
                out[i, k, v] = (len(match_ref_outer(refs, tols, ests, int(c))), len(ests))
    return out
