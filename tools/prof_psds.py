"""Wall time of PSDS counting over a grid of thresholds, a host loop against the counting kernel (GPU diagnostic):

    python tools/prof_psds.py [--clips 1000] [--repeats 5] [--out profiles/psds.json]

Workload: that of tools/prof_event_score.py - synthetic median-filtered timelines of a strong-label split, `--clips` clips
of 10 s (32 frames of 10240 samples at 32 kHz), about three reference events per clip - at K = 10 classes (DESED-like) and
K = 527 (AudioSet-strong-like), V = 49 thresholds k / 50, low threshold = 0.8 threshold, the criteria of scenario 2 (dtc =
gtc = 0.1, cttc = 0.3).  From the timelines on the device to the (V, K, 4) counts and the (V, K, K) cross-triggers on the host:
  (a) host    per threshold: ops.detect_events (two launches, a cumsum and one host read), one copy of the event list, and
              the three criteria on the host (tests/psds_ref.py per timeline that has detections; grouped with numpy)
  (b) device  one ops.psds_count for all thresholds, torch's integer sum over the recordings, one copy of counts and
              cross-triggers in one buffer
Both are warmed up, then run alternately in one process; each time is a host clock around work that ends in a device
synchronise.  The two legs must give the same counts (`same_counts`).  The kernel alone is a host clock around 20
back-to-back launches, divided by 20.  PSDS itself (sed.psds_from_counts on the counts) is reported for the record.
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
from tests import psds_ref as P  # noqa: E402
from tests.event_score_ref import to_samples  # noqa: E402
from tools.prof_event_score import G, RS, SR, summary, timed, workload  # noqa: E402


def host_counts(ev_i, ref, ro, nsamp, K, crit):
    """Event list (E, 4) of `ops.detect_events` on the host -> ((K, 4) (tp, n_det, fp, n_ct), (K, K) cross-triggers): the
    criteria of tests/psds_ref.py on every timeline that has detections."""
    out, ct = np.zeros((K, 4), dtype=np.int64), np.zeros((K, K), dtype=np.int64)
    if len(ev_i) == 0:
        return out, ct
    key = ev_i[:, 0].astype(np.int64) * K + ev_i[:, 1]
    uniq, start = np.unique(key, return_index=True)
    end = np.append(start[1:], len(key))
    for u, p, q in zip(uniq.tolist(), start.tolist(), end.tolist()):
        i, k = divmod(u, K)
        rows = {}
        for c, on, off in ref[ro[i]:ro[i + 1]].tolist():
            rows.setdefault(c, []).append((on, off))
        dets = to_samples(ev_i[p:q, 2:4].tolist(), RS, nsamp[i])
        tp, n_det, fp, crossed = P.judge_timeline(dets, rows.pop(k, []), rows, *crit)
        out[k] += (tp, n_det, fp, len(crossed))
        for c in crossed:
            ct[k, c] += 1
    return out, ct


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prof_psds needs a GPU"
    dev = torch.device("cuda:0")
    hi, lo = sed.threshold_grid(None, 0.8)
    V = hi.size
    sc = sed.PSDS_SCENARIOS[2]
    crit = tuple(ops.per_mille(k, sc[k], 0) for k in ("dtc", "gtc", "cttc"))
    d_hi, d_lo = torch.from_numpy(hi).to(dev), torch.from_numpy(lo).to(dev)
    result = {"workload": {"clips": args.clips, "frames_per_clip": G, "samples_per_frame": RS, "thresholds": int(V),
                           "low_ratio": 0.8, "scenario": 2, "per_mille": list(crit)}}
    for name, K, reps in (("K10", 10, args.repeats), ("K527", 527, max(1, args.repeats // 2))):
        filt, rec, nsamp, ref, ro = workload(args.clips, K, seed=K)
        d_filt = torch.from_numpy(filt).to(dev)
        table = ops.detect_table(np.asarray(rec, dtype=np.int64))
        refs = ops.event_refs(ref, np.zeros(len(ref), dtype=np.int32), ro, K)
        d_n = torch.tensor(nsamp, device=dev, dtype=torch.int64)

        def host():
            out, ct = np.zeros((V, K, 4), dtype=np.int64), np.zeros((V, K, K), dtype=np.int64)
            for v in range(V):
                ev_i, _ = ops.detect_events(d_filt, table, d_hi[v].expand(K).contiguous(), d_lo[v].expand(K).contiguous(), 0, 0)
                out[v], ct[v] = host_counts(ev_i.cpu().numpy(), ref, ro, nsamp, K, crit)
            return out, ct

        def device():
            cnt, ct = ops.psds_count(d_filt, table, d_n, RS, refs, sc["dtc"], sc["gtc"], sc["cttc"], d_hi, d_lo, 0, 0)
            both = torch.cat([cnt.sum(dim=0, dtype=torch.int64).flatten(), ct.flatten().to(torch.int64)]).cpu().numpy()
            return both[:K * V * 4].reshape(K, V, 4).transpose(1, 0, 2), both[K * V * 4:].reshape(V, K, K)

        ra, rb = host(), device()                                             # warm-up of both, and what they return
        times = {"host": [], "device": []}
        for _ in range(reps):
            times["host"].append(timed(host)[0])
            times["device"].append(timed(device)[0])
        out = torch.empty((args.clips, K, V, 4), device=dev, dtype=torch.int32)
        ct = torch.zeros((V, K, K), device=dev, dtype=torch.int32)
        kernel = timed(lambda: [ops.psds_count(d_filt, table, d_n, RS, refs, sc["dtc"], sc["gtc"], sc["cttc"], d_hi, d_lo, 0, 0,
                                               out=out, ct=ct) for _ in range(20)])[0] / 20
        ev = ref.astype(np.int64)
        curve = sed.psds_from_counts(rb[0][:, :, 0], rb[0][:, :, 2], rb[1], np.bincount(ev[:, 0], minlength=K),
                                     np.bincount(ev[:, 0], weights=(ev[:, 2] - ev[:, 1]).astype(np.float64), minlength=K) / SR,
                                     sum(nsamp) / SR, sc["alpha_ct"], sc["alpha_st"], sc["e_max"])
        result[name] = {"classes": K, "timelines": args.clips * K, "reference_events": int(len(ref)),
                        "detections_at_0.5": int(rb[0][24, :, 1].sum()), "tp_at_0.5": int(rb[0][24, :, 0].sum()),
                        "cross_triggers_at_0.5": int(rb[1][24].sum()), "psds": curve["psds"],
                        "same_counts": bool(np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1])),
                        "host": summary(times["host"]), "device": summary(times["device"]), "kernel_s": kernel,
                        "counts_bytes": int(out.numel() * 4 + ct.numel() * 4), "timeline_bytes": int(d_filt.numel() * 4)}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
