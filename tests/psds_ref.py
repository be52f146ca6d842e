"""numpy restatement of PSDS (include/eat_psds.h, efficientat_amd/sed.py: evaluate_psds, psds_from_counts): the detections
of a timeline by `detect_ref.timeline_events`, their conversion to samples with the clip to the recording's length, the three
intersection criteria in per-mille integers, and the curve with its integral.  Plain loops over Python integers and floats;
nothing here shares code with the package.

A recording table `rec` is a list of rows (first window, window count, goff, G); reference rows are (class, onset, offset)
in samples, recording i owning rows [ro[i], ro[i + 1]) sorted by (class, onset)."""
import math

import numpy as np

from tests.detect_ref import timeline_events
from tests.event_score_ref import class_rows, to_samples


def inter(d, r):
    """I(d, r) of two sample intervals (on, off)."""
    return max(0, min(d[1], r[1]) - max(d[0], r[0]))


def judge_timeline(dets, own, others, dtc_pm, gtc_pm, cttc_pm):
    """Detections [(on, off)] of one (recording, class, threshold) against the rows `own` [(on, off)] of its class and
    `others` {class: [(on, off)]} of the recording's other classes -> (tp, n_det, fp, [cross-triggered classes, one entry
    per cross-trigger])."""
    cover = [0] * len(own)
    fp, crossed = 0, []
    for d in dets:
        L = d[1] - d[0]
        S = sum(inter(d, r) for r in own)
        if L > 0 and 1000 * S >= dtc_pm * L:
            for j, r in enumerate(own):
                cover[j] += inter(d, r)
            continue
        fp += 1
        if cttc_pm > 0 and L > 0:
            for c in sorted(others):
                if 1000 * sum(inter(d, r) for r in others[c]) >= cttc_pm * L:
                    crossed.append(c)
    tp = sum(1 for r, C in zip(own, cover) if r[1] - r[0] > 0 and 1000 * C >= gtc_pm * (r[1] - r[0]))
    return tp, len(dets), fp, crossed


def count_ref(filt, rec, nsamp, R, ref, ro, dtc_pm, gtc_pm, cttc_pm, hi, lo, max_gap=0, min_len=0):
    """filt (K, G_total) float32 -> (counts (n_rec, K, V, 4) int64 holding (tp, n_det, fp, n_ct), ct (V, K, K) int64 indexed
    [v, detection class, reference class]); thresholds compared as float32."""
    filt = np.asarray(filt, dtype=np.float32)
    hi, lo = np.asarray(hi, dtype=np.float32).reshape(-1), np.asarray(lo, dtype=np.float32).reshape(-1)
    ref = np.asarray(ref).reshape(-1, 3).tolist()
    K, V = filt.shape[0], hi.shape[0]
    counts = np.zeros((len(rec), K, V, 4), dtype=np.int64)
    ct = np.zeros((V, K, K), dtype=np.int64)
    for i, (_, _, goff, G) in enumerate(rec):
        rows = {k: [(ref[e][1], ref[e][2]) for e in class_rows(ref, ro, i, k)] for k in range(K)}
        for k in range(K):
            others = {c: r for c, r in rows.items() if c != k and r}
            x = filt[k, goff:goff + G]
            for v in range(V):
                dets = to_samples(timeline_events(x, hi[v], lo[v], max_gap, min_len), R, nsamp[i])
                tp, n_det, fp, crossed = judge_timeline(dets, rows[k], others, dtc_pm, gtc_pm, cttc_pm)
                counts[i, k, v] = (tp, n_det, fp, len(crossed))
                for c in crossed:
                    ct[v, k, c] += 1
    return counts, ct


def curve_ref(tp, fp, ct, n_ref, ref_seconds, total_seconds, alpha_ct, alpha_st, e_max=100.0):
    """The PSDS of integer counts tp, fp (V, K), ct (V, K, K) -> (psds, breakpoints, eTPR on the interval from each), with
    Python floats (fp64) throughout.  No class with references: (nan, [], [])."""
    tp, fp, ct = np.asarray(tp).tolist(), np.asarray(fp).tolist(), np.asarray(ct).tolist()
    V, K = len(tp), len(tp[0])
    hours = float(total_seconds) / 3600.0
    curves = []
    for c in range(K):
        if n_ref[c] <= 0:
            continue
        pts = {}
        for v in range(V):
            x = fp[v][c] / hours
            if K > 1:
                cross = 0.0
                for o in range(K):
                    if o != c and ref_seconds[o] > 0:
                        cross += ct[v][c][o] / (float(ref_seconds[o]) / 3600.0)
                x += float(alpha_ct) * cross / (K - 1)
            y = tp[v][c] / float(n_ref[c])
            pts[x] = max(pts.get(x, 0.0), y)
        xs, ys, top = sorted(pts), [], 0.0
        for x in xs:
            top = max(top, pts[x])
            ys.append(top)
        curves.append((xs, ys))
    if not curves:
        return float("nan"), [], []
    e_max = float(e_max)
    bx = sorted({0.0, e_max} | {x for xs, _ in curves for x in xs if 0.0 <= x <= e_max})
    etpr = []
    for b in bx:
        f = []
        for xs, ys in curves:
            val = 0.0
            for x, y in zip(xs, ys):
                if x <= b:
                    val = y
            f.append(val)
        mean = math.fsum(f) / len(f)
        std = math.sqrt(math.fsum((a - mean) ** 2 for a in f) / len(f))
        etpr.append(mean - float(alpha_st) * std)
    area = math.fsum(etpr[j] * (bx[j + 1] - bx[j]) for j in range(len(bx) - 1))
    return area / e_max, bx, etpr
