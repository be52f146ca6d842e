"""Kernel times of the wave-augmentation gathers at B = 64, L = 320000 (profiles/fsd50k_ragged_kernel_times.json).

    for m in rect equal long; do rocprofv3 --kernel-trace --stats --output-format csv -d OUT/prof_$m -- python tools/prof_ragged.py $m; done
    python tools/prof_ragged.py reduce OUT

One case per process, so that rocprofv3's per-kernel statistics do not merge them: `rect` = eat_wave_augment on a rectangle
of clips of exactly L; `equal` = eat_wave_augment_ragged on the same bytes; `long` = clips of 2L - 3L with random crops.  Seven
eager calls each (2 warm-up + 5 repeats); `reduce` reads the per-call durations of the last five from the kernel traces."""
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def reduce(root):
    res = {}
    for mode in ("rect", "equal", "long"):
        for f in glob.glob(os.path.join(root, f"prof_{mode}", "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                for key in ("wave_augment_kernel", "ragged_mean_kernel", "ragged_gather_kernel"):
                    if key in r["Kernel_Name"]:
                        t0, t1 = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
                        res.setdefault(f"{mode}:{key}", []).append((t0, (t1 - t0) / 1e3))
    out = {}
    for k, v in res.items():
        us = [d for _, d in sorted(v)][-5:]
        out[k] = {"us": [round(x, 2) for x in us], "min": round(min(us), 2), "max": round(max(us), 2),
                  "mean": round(sum(us) / len(us), 2)}
    print(json.dumps(out, indent=1))


def run(mode):
    import numpy as np
    import torch
    from efficientat_amd import ops


    dev = torch.device("cuda:0")
    B, L, N = 64, 320000, 128
    g = torch.Generator().manual_seed(0)
    rng = np.random.default_rng(0)
    idx = torch.full((2 * B,), -1, dtype=torch.int32)
    idx[0::2] = torch.randperm(N, generator=g)[:B].to(torch.int32)
    mixed = torch.arange(B) % 2 == 1
    idx[1::2][mixed] = torch.randint(N, (int(mixed.sum()),), generator=g).to(torch.int32)
    shift = torch.randint(-4000, 4001, (2 * B,), generator=g).to(torch.int32)
    amp = torch.tensor(10 ** (rng.integers(-12, 12, 2 * B) / 20), dtype=torch.float32)
    lm = torch.tensor(rng.beta(2, 2, B), dtype=torch.float32)
    mix = torch.where(mixed, torch.maximum(lm, 1 - lm), torch.ones(B))
    out = torch.empty(B, L, device=dev)
    if mode == "rect":
        bank = torch.randn(N, L, device=dev) * 0.1
        mean = bank.double().mean(1)
        t = [x.to(dev) for x in (idx, shift, amp, mix)]
        call = lambda: ops.wave_augment(bank, mean, None, *t, 0, out=out)
    else:
        lens = torch.full((N,), L, dtype=torch.int64) if mode == "equal" else torch.randint(2 * L, 3 * L + 1, (N,), generator=g)
        offs = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)[:-1]])
        waves = torch.randn(int(lens.sum()), device=dev) * 0.1
        csum = torch.stack([waves[o:o + n].double().sum() for o, n in zip(offs.tolist(), lens.tolist())])
        rb = dict(waves=waves, offsets=offs.to(dev), lengths=lens.to(torch.int32).to(dev), clip_sum=csum,
                  bank_y=torch.zeros(N, 200, device=dev), lengths_cpu=lens)
        start = torch.zeros(2 * B, dtype=torch.int32)
        if mode == "long":
            u = torch.rand(2 * B, generator=g)
            room = torch.where(idx >= 0, lens[idx.clamp(min=0).long()] - L, 0)
            start = (u * (room + 1)).long().clamp(max=room).to(torch.int32)
        ops.check_ragged_draws(idx, start, shift, lens, L)
        t = [x.to(dev) for x in (idx, start, shift, amp, mix)]
        wm = torch.empty(2 * B, device=dev, dtype=torch.float64)
        yy = torch.empty(B, 400, device=dev)
        call = lambda: ops.wave_augment_ragged(rb, *t, L, out=out, yy=yy, win_mean=wm)
    for _ in range(7):                       # 2 warm-up calls + 5 repeats
        call()
        torch.cuda.synchronize()
    print(mode, "done", float(out.abs().mean()))


if __name__ == "__main__":
    if sys.argv[1] == "reduce":
        reduce(sys.argv[2])
    else:
        run(sys.argv[1])
