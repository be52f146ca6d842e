"""Wall time of scoring a grid of median widths, one median launch per width against the width-bank kernel (GPU diagnostic):

    python tools/prof_tune.py [--clips 1000] [--repeats 7] [--out profiles/tune.json]

Workload: the timelines of tools/prof_event_score.py taken as stitched probabilities - `--clips` clips of 10 s (32 frames of
10240 samples at 32 kHz), about three reference events per clip - at K = 10 classes (DESED-like) and K = 527
(AudioSet-strong-like), the 8 odd median widths 1 .. 15 frames, V = 49 thresholds k / 50, low threshold = 0.8 threshold.  From
the probabilities on the device to the (8, K, V, 2) int64 sums over the clips on the device:
  (a) per_width  per width one ops.detect_median (none at width 1) and one ops.event_score
  (b) bank       one ops.detect_median_bank for the 8 widths and 8 ops.event_score on its slices (sed._sweep_timelines)
Both are warmed up, then run alternately in one process; each time is a host clock around work that ends in a device
synchronise.  The two legs must give the same counts (`same_counts`).  The median alone: a host clock around 20 rounds of 8
ops.detect_median launches (width 1 included, as a copy) against 20 ops.detect_median_bank launches, each into a preallocated
output, divided by 20.  The trunk forward that a walk of a real split repeats per width in leg (a) is not part of either leg.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from efficientat_amd import ops, sed  # noqa: E402
from tools.prof_event_score import G, RS, SR, summary, timed, workload  # noqa: E402

WIDTHS = list(range(1, 16, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prof_tune needs a GPU"
    dev = torch.device("cuda:0")
    hi, lo = sed.threshold_grid(None, 0.8)
    V, c, Mw = hi.size, sed.collar_samples(200, SR), len(WIDTHS)
    d_hi, d_lo = torch.from_numpy(hi).to(dev), torch.from_numpy(lo).to(dev)
    result = {"workload": {"clips": args.clips, "frames_per_clip": G, "samples_per_frame": RS, "thresholds": int(V),
                           "low_ratio": 0.8, "collar_samples": c, "offset_pct": 0.2, "median_frames": WIDTHS}}
    for name, K in (("K10", 10), ("K527", 527)):
        prob, rec, nsamp, ref, ro = workload(args.clips, K, seed=K)
        d_prob = torch.from_numpy(prob).to(dev)
        table = ops.detect_table(np.asarray(rec, dtype=np.int64))
        refs = ops.event_refs(ref, sed.event_tolerances(ref, c, 0.2), ro, K)
        d_n = torch.tensor(nsamp, device=dev, dtype=torch.int64)
        widths = ops.median_width_table(np.repeat(np.asarray(WIDTHS)[:, None], K, axis=1), K)
        widths.dev(dev)

        def per_width():
            out = []
            for m in WIDTHS:
                filt = ops.detect_median(d_prob, table, m) if m != 1 else d_prob
                out.append(ops.event_score(filt, table, d_n, RS, refs, c, d_hi, d_lo, 0, 0).sum(dim=0, dtype=torch.int64))
            return torch.stack(out)

        def bank():
            return sed._sweep_timelines(d_prob, table, d_n, RS, refs, c, widths, d_hi, d_lo, 0, 0)

        ra, rb = per_width(), bank()                                          # warm-up of both, and what they return
        times = {"per_width": [], "bank": []}
        for _ in range(args.repeats):
            times["per_width"].append(timed(per_width)[0])
            times["bank"].append(timed(bank)[0])
        one = torch.empty((K, table.G_total), device=dev)
        many = torch.empty((Mw, K, table.G_total), device=dev)
        med = {"eight_launches": [], "bank_launch": []}
        for _ in range(args.repeats):
            med["eight_launches"].append(timed(lambda: [ops.detect_median(d_prob, table, m, out=one) for _ in range(20)
                                                        for m in WIDTHS])[0] / 20)
            med["bank_launch"].append(timed(lambda: [ops.detect_median_bank(d_prob, table, widths, out=many)
                                                     for _ in range(20)])[0] / 20)
        result[name] = {"classes": K, "timelines": args.clips * K, "reference_events": int(len(ref)),
                        "estimated_events_at_0.5_per_width": rb[:, :, 24, 1].sum(dim=1).tolist(),
                        "same_counts": bool(torch.equal(ra, rb)), "per_width": summary(times["per_width"]),
                        "bank": summary(times["bank"]), "median_eight_launches": summary(med["eight_launches"]),
                        "median_bank_launch": summary(med["bank_launch"]), "timeline_bytes": int(d_prob.numel() * 4),
                        "filtered_bytes": int(many.numel() * 4)}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
