"""Wall time of the post-processing of sound event detection, host restatement against the device kernels (GPU diagnostic):

    python tools/prof_detect.py [--minutes 60] [--repeats 5] [--out profiles/detect.json]

Workload: one synthetic 32 kHz recording, mn10 with synthetic weights, EADetector at its default settings (windows of
10.24 s every 5.12 s, triangle taper, median 960 ms, threshold 0.5).  The frame logits (N_w, K, Tp) of all windows are
computed once; then, from those logits on the device to the event list on the host:
  (a) host    copy the logits to the host and run tests/detect_ref.py: stitch_ref, median_ref, events_ref (numpy, fp64
              sigmoid, np.sort, a Python state machine per class)
  (b) device  ops.detect_stitch, ops.detect_median, ops.detect_events and the copy of the event list
Both are warmed up, then run alternately in one process; each time is a host clock around work that ends in a device
synchronise.  (b) is also run stage by stage with a synchronise after each.  The same pair is measured a second time with
per-class thresholds at the 90th / 80th percentile of each class's own probabilities, so that every class has events.
`forward` is mel + trunk + frame head of all windows, `to_event_arrays` a whole `detect` up to the event arrays on the host
(their ratio is the share the forward takes), `event_lists_host` the Python tuples `detect` builds from them.  The stitch
and median stages are a host clock around 20 back-to-back launches, divided by 20.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from efficientat_amd import detection, ops  # noqa: E402
from efficientat_amd.mn import get_model  # noqa: E402
from oracle import eat_oracle as O  # noqa: E402
from oracle import synth  # noqa: E402
from tests import detect_ref as R  # noqa: E402

SR = 32000


def recording(minutes, dev, seed=0):
    """A slow frequency sweep with bursts of noise, generated on the device."""
    n = int(minutes * 60 * SR)
    g = torch.Generator(device=dev).manual_seed(seed)
    t = torch.arange(n, device=dev, dtype=torch.float32) / SR
    x = 0.2 * torch.sin(2 * np.pi * (200.0 + 40.0 * torch.sin(2 * np.pi * 0.05 * t)) * t)
    burst = (torch.sin(2 * np.pi * t / 7.3) > 0.6).float()
    return x + 0.05 * (1.0 + 3.0 * burst) * torch.randn(n, device=dev, generator=g)


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
    ap.add_argument("--minutes", type=float, default=60.0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prof_detect needs a GPU"
    dev = torch.device("cuda:0")
    with contextlib.redirect_stdout(io.StringIO()):
        model = get_model(width_mult=1.0)
    x_cal = O.mel_forward(synth.parity_clips(64000, seed=3)).unsqueeze(1)         # running statistics as __graft_entry__.smoke
    model.load_state_dict(synth.calibrate(synth.synth_state(synth.mn_shapes(1.0), seed=0), O.mn_forward, x_cal))
    model.to(dev).eval()
    det = detection.EADetector(model=model)
    geo, K = det.geometry, det.num_classes
    wave = recording(args.minutes, dev)
    lengths = [int(wave.numel())]
    starts, valids, table = det.plan(lengths)
    rec = table.cpu.tolist()
    m = detection.median_frames(960, geo.frame_s)
    wt64 = ops.detect_weights(geo.T, det.taper)

    det.window_logits(wave, starts, valids)                                        # warm-up of the forward
    t_fwd = [timed(lambda: det.window_logits(wave, starts, valids))[0] for _ in range(3)]
    P = det.window_logits(wave, starts, valids)
    half = torch.full((K,), 0.5, device=dev)

    def to_arrays():                                           # `detect` up to the event list's arrays on the host
        _, filt, tab, _ = det.timelines([wave], m)
        ev_i, ev_f = ops.detect_events(filt, tab, half, half, 0, 0)
        return ev_i.cpu().numpy(), ev_f.cpu().numpy()

    ev = to_arrays()
    t_arrays = [timed(to_arrays)[0] for _ in range(3)]
    t_lists = [timed(lambda: det.event_lists(ev[0], ev[1], lengths))[0] for _ in range(3)]   # the Python tuples per event
    prob0 = ops.detect_stitch(P, table, geo.Hf, geo.T, det._wt)

    def host(hi, lo):
        p = P.cpu().numpy()
        filt = R.median_ref(R.stitch_ref(p, rec, geo.Hf, geo.T, wt64).astype(np.float32), rec, m)
        return R.events_ref(filt, rec, hi, lo, 0, 0)

    def device(d_hi, d_lo):
        filt = ops.detect_median(ops.detect_stitch(P, table, geo.Hf, geo.T, det._wt), table, m)
        ev_i, ev_f = ops.detect_events(filt, table, d_hi, d_lo, 0, 0)
        return ev_i.cpu().numpy(), ev_f.cpu().numpy()

    def staged(d_hi, d_lo):
        out = {}
        prob, filt = torch.empty((K, table.G_total), device=dev), torch.empty((K, table.G_total), device=dev)
        out["stitch"] = timed(lambda: [ops.detect_stitch(P, table, geo.Hf, geo.T, det._wt, out=prob) for _ in range(20)])[0] / 20
        out["median"] = timed(lambda: [ops.detect_median(prob, table, m, out=filt) for _ in range(20)])[0] / 20
        out["events"], ev = timed(lambda: ops.detect_events(filt, table, d_hi, d_lo, 0, 0))
        out["copy"], _ = timed(lambda: (ev[0].cpu(), ev[1].cpu()))
        return out

    result = {"workload": {"minutes": args.minutes, "rate": SR, "samples": lengths[0], "windows": int(P.shape[0]), "classes": K,
                           "frames": table.G_total, "frame_s": geo.frame_s, "median_frames": m, "taper": det.taper,
                           "batch_windows": det.batch_windows},
              "forward": summary(t_fwd), "to_event_arrays": summary(t_arrays), "event_lists_host": summary(t_lists),
              "events_default": int(len(ev[0]))}
    q = torch.quantile(prob0, torch.tensor([0.8, 0.9], device=dev), dim=1).clamp(1e-6, 1.0).cpu().numpy().astype(np.float32)
    for name, hi, lo, reps in (("default_thresholds", np.full(K, 0.5, np.float32), np.full(K, 0.5, np.float32), args.repeats),
                               ("percentile_thresholds", q[1], q[0], max(1, args.repeats // 2))):
        d_hi, d_lo = torch.from_numpy(hi).to(dev), torch.from_numpy(lo).to(dev)
        ra, rb = host(hi, lo), device(d_hi, d_lo)                                  # warm-up of both, and what they return
        times = {"host": [], "device": []}
        for _ in range(reps):
            times["host"].append(timed(lambda: host(hi, lo))[0])
            times["device"].append(timed(lambda: device(d_hi, d_lo))[0])
        stages = [staged(d_hi, d_lo) for _ in range(3)]
        st = {k: statistics.median(s[k] for s in stages) for k in stages[0]}
        n_valid = sum(min(geo.T, r[3] - qq * geo.Hf) for r in rec for qq in range(r[1]))
        traffic = {"stitch_bytes": 4 * K * (n_valid + table.G_total), "median_bytes": 8 * K * table.G_total}
        traffic["stitch_GBps"] = traffic["stitch_bytes"] / st["stitch"] / 1e9
        traffic["median_GBps"] = traffic["median_bytes"] / st["median"] / 1e9
        result[name] = {"events": int(len(rb[0])), "same_events": bool(np.array_equal(ra[0], rb[0])),
                        "peak_max_diff": float(np.abs(ra[1] - rb[1][:, 0]).max()) if len(rb[0]) == len(ra[0]) > 0 else None,
                        "host": summary(times["host"]), "device": summary(times["device"]), "device_stages_s": st, **traffic}
    result["forward_share_of_to_event_arrays"] = result["forward"]["median_s"] / result["to_event_arrays"]["median_s"]
    result["post_share_of_to_event_arrays"] = result["default_thresholds"]["device"]["median_s"] / result["to_event_arrays"]["median_s"]
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
