"""Wall time of event-based (collar) scoring over a grid of thresholds, a host loop against the scoring kernel (GPU diagnostic):

    python tools/prof_event_score.py [--clips 1000] [--repeats 5] [--out profiles/event_score.json]

Workload: synthetic median-filtered timelines of a strong-label split - `--clips` clips of 10 s (32 frames of 10240 samples
at 32 kHz), about three reference events per clip, a probability plateau under most of them and some plateaus without one -
at two shapes: K = 10 classes (DESED-like) and K = 527 (AudioSet-strong-like), V = 49 thresholds k / 50, low threshold =
0.8 threshold, collar 200 ms / 20 %.  From the timelines on the device to the (V, K, 3) counts on the host:
  (a) host    per threshold: ops.detect_events (two launches, a cumsum and one host read), one copy of the event list,
              and sed_eval's greedy matching on the host (tests/event_score_ref.py per timeline that has estimates and
              references; timelines are grouped with numpy)
  (b) device  one ops.event_score for all thresholds, torch's integer sum over the recordings, one copy of (K, V, 2)
Both are warmed up, then run alternately in one process; each time is a host clock around work that ends in a device
synchronise.  The two legs must give the same counts (`same_counts`).  The kernel alone is a host clock around 20
back-to-back launches, divided by 20.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from efficientat_amd import ops, sed  # noqa: E402
from tests import event_score_ref as R  # noqa: E402

SR, RS, G = 32000, 10240, 32


def workload(n_clips, K, seed):
    """-> (filt (K, n_clips G) float32, table rows, nsamp, ref (E, 3) int32, ro)."""
    rng = np.random.default_rng(seed)
    n = 10 * SR
    filt = (0.02 + 0.1 * rng.random((K, n_clips * G))).astype(np.float32)
    rows, ro = [], [0]
    for i in range(n_clips):
        mine = []
        for _ in range(int(rng.integers(1, 6))):
            k, on_f = int(rng.integers(K)), int(rng.integers(0, G - 2))
            off_f = int(min(G, on_f + rng.integers(1, 12)))
            if rng.random() < 0.85:                                           # the detector sees it (at some thresholds)
                filt[k, i * G + on_f:i * G + off_f] = rng.uniform(0.2, 0.98) * (0.8 + 0.2 * rng.random(off_f - on_f))
            if rng.random() < 0.85:                                           # it is annotated, a little off the frame grid
                on = min(max(on_f * RS + int(rng.integers(-8000, 8001)), 0), n - 1)
                mine.append((k, on, min(max(off_f * RS + int(rng.integers(-8000, 8001)), on + 1), n)))
        rows.extend(sorted(mine))
        ro.append(len(rows))
    rec = [(i, 1, i * G, G) for i in range(n_clips)]
    return filt, rec, [n] * n_clips, np.asarray(rows, dtype=np.int32).reshape(-1, 3), np.asarray(ro, dtype=np.int64)


def host_counts(ev_i, ref, tol, ro, nsamp, K, c):
    """Event list (E, 4) of `ops.detect_events` on the host -> (K, 2) (tp, n_est): the matching of tests/event_score_ref.py on
    every timeline that has both estimates and references."""
    out = np.zeros((K, 2), dtype=np.int64)
    np.add.at(out[:, 1], ev_i[:, 1], 1)
    if len(ev_i) == 0 or len(ref) == 0:
        return out
    rec_of_ref = np.repeat(np.arange(len(ro) - 1), np.diff(ro))
    ref_key = rec_of_ref * K + ref[:, 0]
    est_key = ev_i[:, 0].astype(np.int64) * K + ev_i[:, 1]
    both = np.intersect1d(ref_key, est_key)
    r0, r1 = np.searchsorted(ref_key, both, "left"), np.searchsorted(ref_key, both, "right")
    e0, e1 = np.searchsorted(est_key, both, "left"), np.searchsorted(est_key, both, "right")
    for key, a, b, p, q in zip(both.tolist(), r0.tolist(), r1.tolist(), e0.tolist(), e1.tolist()):
        i, k = divmod(key, K)
        ests = R.to_samples(ev_i[p:q, 2:4].tolist(), RS, nsamp[i])
        out[k, 0] += len(R.match_ref_outer(ref[a:b, 1:3].tolist(), tol[a:b].tolist(), ests, c))
    return out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def summary(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "all_s": [round(x, 5) for x in ts]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prof_event_score needs a GPU"
    dev = torch.device("cuda:0")
    hi, lo = sed.threshold_grid(None, 0.8)
    V, c = hi.size, sed.collar_samples(200, SR)
    d_hi, d_lo = torch.from_numpy(hi).to(dev), torch.from_numpy(lo).to(dev)
    result = {"workload": {"clips": args.clips, "frames_per_clip": G, "samples_per_frame": RS, "thresholds": int(V),
                           "low_ratio": 0.8, "collar_samples": c, "offset_pct": 0.2}}
    for name, K, reps in (("K10", 10, args.repeats), ("K527", 527, max(1, args.repeats // 2))):
        filt, rec, nsamp, ref, ro = workload(args.clips, K, seed=K)
        tol = sed.event_tolerances(ref, c, 0.2)
        d_filt = torch.from_numpy(filt).to(dev)
        table = ops.detect_table(np.asarray(rec, dtype=np.int64))
        refs = ops.event_refs(ref, tol, ro, K)
        d_n = torch.tensor(nsamp, device=dev, dtype=torch.int64)
        n_ref = np.bincount(ref[:, 0], minlength=K)

        def host():
            out = np.zeros((V, K, 2), dtype=np.int64)
            for v in range(V):
                ev_i, _ = ops.detect_events(d_filt, table, d_hi[v].expand(K).contiguous(), d_lo[v].expand(K).contiguous(), 0, 0)
                out[v] = host_counts(ev_i.cpu().numpy(), ref, tol, ro, nsamp, K, c)
            return out

        def device():
            cnt = ops.event_score(d_filt, table, d_n, RS, refs, c, d_hi, d_lo, 0, 0)
            return cnt.sum(dim=0, dtype=torch.int64).cpu().numpy().transpose(1, 0, 2)

        ra, rb = host(), device()                                             # warm-up of both, and what they return
        times = {"host": [], "device": []}
        for _ in range(reps):
            times["host"].append(timed(host)[0])
            times["device"].append(timed(device)[0])
        out = torch.empty((args.clips, K, V, 2), device=dev, dtype=torch.int32)
        kernel = timed(lambda: [ops.event_score(d_filt, table, d_n, RS, refs, c, d_hi, d_lo, 0, 0, out=out) for _ in range(20)])[0] / 20
        tp = rb[:, :, 0]
        f1 = [sed.segment_scores(np.stack([tp[v], rb[v, :, 1] - tp[v], n_ref - tp[v]], 1))["micro_f1"] for v in range(V)]
        result[name] = {"classes": K, "timelines": args.clips * K, "reference_events": int(len(ref)),
                        "estimated_events_at_0.5": int(rb[24, :, 1].sum()), "tp_at_0.5": int(tp[24].sum()),
                        "best_micro_f1": float(np.nanmax(f1)), "same_counts": bool(np.array_equal(ra, rb)),
                        "host": summary(times["host"]), "device": summary(times["device"]), "kernel_s": kernel,
                        "counts_bytes": int(out.numel() * 4), "timeline_bytes": int(d_filt.numel() * 4)}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
