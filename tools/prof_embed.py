"""Time of pooling one chunk's feature maps into embeddings, the torch formulation against eat_embed_pool (GPU diagnostic):

    python tools/prof_embed.py [--windows 64] [--repeats 5] [--inner 20] [--out prof_embed.json]

Workload: mn10 with seeded random weights, `windows` windows of 10 s (128 mels x 1000 frames), the 17 feature maps of
one eval forward with return_fmaps=True.  Two modes, scene and timestamps at (hop 50 ms, width 160 ms), two legs each:
  (a) torch  scene: 17 `mean((2, 3))` calls and a `cat`;  timestamps: per map the column sums over f, their `cumsum`
             along t, gathered at hi and lo, divided by F (hi - lo), then a `cat` (index tensors built beforehand)
  (b) hip    ops.embed_pool: one launch
Both are warmed up, then run alternately `repeats` times; each time is a host clock around `inner` back-to-back calls that
end in a device synchronise, divided by `inner`.  For (b) the bytes read (every map once) and written (the embeddings),
computed from the shapes, are set against its median time.
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

from efficientat_amd import embeddings, ops  # noqa: E402
from efficientat_amd.mn import get_model  # noqa: E402

COPY_TBS = 6.29          # what a device-to-device copy reaches on this part (VERDICT, "What's weak" #6)


def torch_scene(fmaps):
    return torch.cat([m.mean((2, 3)) for m in fmaps], dim=1).unsqueeze(1)


def torch_timestamps(fmaps, lo_d, hi_d, inv_d):
    out = []
    for m, lo, hi, inv in zip(fmaps, lo_d, hi_d, inv_d):
        cs = torch.nn.functional.pad(m.sum(2).cumsum(2), (1, 0))                    # (B, C, T + 1), cs[..., t] = sum of columns < t
        out.append(((cs[:, :, hi] - cs[:, :, lo]) * inv).transpose(1, 2))           # (B, n, C)
    return torch.cat(out, dim=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prof_embed needs a GPU"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        model = get_model(width_mult=1.0).to(dev).eval()
    _, strides = embeddings.model_maps(model)
    with torch.no_grad():
        spec = torch.randn((args.windows, 1, 128, 1000), device=dev)
        fmaps = [m.contiguous() for m in model._forward_impl(spec, return_fmaps=True)[1]]
    del spec
    widths = [m.shape[3] for m in fmaps]
    D = sum(m.shape[1] for m in fmaps)
    plans = {"scene": (np.zeros((17, 1), dtype=np.int32), np.asarray(widths, dtype=np.int32).reshape(-1, 1)),
             "timestamps": embeddings.segment_plan(1000, widths, strides, 10.0, 50.0, 160.0)[:2]}
    result = {"workload": {"model": "mn10", "windows": args.windows, "frames": 1000, "maps": [list(m.shape[1:]) for m in fmaps],
                           "D": D, "repeats": args.repeats, "inner": args.inner}, "copy_TBs": COPY_TBS}
    for mode, (lo, hi) in plans.items():
        n_seg = lo.shape[1]
        if mode == "scene":
            a = lambda: torch_scene(fmaps)
        else:
            lo_d = [torch.from_numpy(lo[l].astype(np.int64)).to(dev) for l in range(17)]
            hi_d = [torch.from_numpy(hi[l].astype(np.int64)).to(dev) for l in range(17)]
            inv_d = [torch.from_numpy((1.0 / (m.shape[2] * (hi[l] - lo[l]))).astype(np.float32)).to(dev)
                     for l, m in enumerate(fmaps)]
            a = lambda: torch_timestamps(fmaps, lo_d, hi_d, inv_d)
        b = lambda: ops.embed_pool(fmaps, lo, hi)
        ra, rb = a(), b()                                  # warm-up of both, and how far apart they are
        diff = float((ra - rb).abs().max())
        scale = float(ra.abs().mean())
        del ra, rb
        times = {"torch": [], "hip": []}
        for _ in range(args.repeats):
            for name, fn in (("torch", a), ("hip", b)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.inner):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / args.inner)
        r = {"n_seg": n_seg, "max_abs_diff": diff, "mean_abs": scale}
        for name, ts in times.items():
            r[name] = {"median_us": 1e6 * statistics.median(ts), "min_us": 1e6 * min(ts), "max_us": 1e6 * max(ts),
                       "all_us": [round(1e6 * x, 1) for x in ts]}
        r["speedup_median"] = r["torch"]["median_us"] / r["hip"]["median_us"]
        read = 4 * sum(m.numel() for m in fmaps)
        written = 4 * args.windows * n_seg * D
        r["hip_bytes"] = {"read": read, "written": written,
                          "TBs": (read + written) / (1e-6 * r["hip"]["median_us"]) / 1e12}
        r["hip_bytes"]["of_copy"] = r["hip_bytes"]["TBs"] / COPY_TBS
        result[mode] = r
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
