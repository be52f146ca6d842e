"""Wall time of strong-label SED training and scoring (GPU diagnostic):

    python tools/prof_sed.py [--batch 64] [--clips 96] [--classes 10] [--steps 10] [--repeats 5] [--out profiles/sed.json]

Workload: a synthetic strong-label bank (tests/sed_ref.synth_bank: clips of 4 - 14 s, up to 4 events each), mn10 with
random weights and `--classes` classes, clips of 327680 samples (32 frames), fp32 log-mel, train_precision 'auto'.
  (a) eager   sed.FrameBCETrainer.step
  (b) graph   sed.GraphedFrameBCETrainer.step (one replay per step)
  (c) weak_graph  sed.GraphedWeakFrameTrainer.step on the same clips with every third marked weak (strong.npy), weak_weight 1
Both are warmed up, then run alternately in one process, `--steps` steps per leg and `--repeats` legs each; each time is a
host clock around work that ends in a device synchronise, divided by the steps.  `clip_level_graph` is
finetune.GraphedBCETrainer on the same bank (the weak labels) for the cost of the frame path over the clip-level one.
The glue kernels are a host clock around 20 back-to-back launches, divided by 20, at the AudioSet shape (B, 527, 32):
eat_sed_targets, eat_frame_bce_fwd_bwd (loss + gradient), eat_frame_grad_pad, eat_frame_hidden_fwd / _bwd at H = 1280,
eat_sed_clip_targets and eat_weak_frame_bce_fwd_bwd (loss + gradient) at the same shape and at K = 10.
`evaluate_frames` scores the whole bank."""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from efficientat_amd import ops, sed  # noqa: E402
from efficientat_amd.finetune import GraphedBCETrainer  # noqa: E402
from efficientat_amd.mn import get_model  # noqa: E402
from efficientat_amd.optim import FusedAdam  # noqa: E402
from efficientat_amd.preprocess import AugmentMelSTFT  # noqa: E402
from tests import sed_ref as R  # noqa: E402
from tests import weak_sed_ref as W  # noqa: E402


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def summary(ts):
    return {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "all_s": [round(x, 6) for x in ts]}


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--clips", type=int, default=96)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prof_sed needs a GPU"
    dev = torch.device("cuda:0")
    B, K, L = args.batch, args.classes, sed.CLIP_SAMPLES
    with tempfile.TemporaryDirectory() as d:
        R.synth_bank(d, n_clips=args.clips, K=K, seed=1, lo_s=4.0, hi_s=14.0)
        bank = sed.load_bank(d, device=dev)
        W.weaken_bank(d)
        weak_bank = sed.load_bank(d, device=dev)

    def trainer(kind):
        torch.manual_seed(0)
        m = quiet(get_model, num_classes=K, width_mult=1.0).to(dev).train()
        mel = quiet(AugmentMelSTFT, freqm=0, timem=0).to(dev).train()
        opt = FusedAdam(m.parameters(), lr=torch.tensor(1e-4, device=dev), capturable=True)
        if kind == "eager":
            return sed.FrameBCETrainer(m, mel, opt, bank, clip_samples=L)
        if kind == "graph":
            return sed.GraphedFrameBCETrainer(m, mel, opt, bank, B, clip_samples=L)
        if kind == "weak_graph":
            return sed.GraphedWeakFrameTrainer(m, mel, opt, weak_bank, B, clip_samples=L, weak_weight=1.0)
        return GraphedBCETrainer(m, mel, opt, bank, B, clip_samples=L)

    legs = {k: trainer(k) for k in ("eager", "graph", "weak_graph", "clip_level_graph")}
    rng = np.random.RandomState(0)

    def run(tr):
        for _ in range(args.steps):
            tr.step(rng.randint(0, args.clips, size=B).tolist())

    for tr in legs.values():                                                  # warm-up of every leg
        run(tr)
    times = {k: [] for k in legs}
    for _ in range(args.repeats):
        for k, tr in legs.items():
            times[k].append(timed(lambda: run(tr))[0] / args.steps)
    result = {"workload": {"batch": B, "clips": args.clips, "classes": K, "clip_samples": L, "frames": 32,
                           "steps_per_leg": args.steps, "bank_seconds": bank["waves"].numel() / 32000.0,
                           "weak_clips": sed.n_weak(weak_bank)},
              "step": {k: summary(v) for k, v in times.items()}}
    result["graph_over_eager"] = result["step"]["graph"]["median_s"] / result["step"]["eager"]["median_s"]
    result["weak_over_strong_graph"] = result["step"]["weak_graph"]["median_s"] / result["step"]["graph"]["median_s"]
    result["frame_over_clip_level"] = result["step"]["graph"]["median_s"] / result["step"]["clip_level_graph"]["median_s"]

    ev = legs["graph"]
    timed(lambda: sed.evaluate_frames(ev.model, ev.mel, bank, clip_samples=L))
    t_ev = [timed(lambda: sed.evaluate_frames(ev.model, ev.mel, bank, clip_samples=L)) for _ in range(3)]
    result["evaluate_frames"] = dict(summary([t for t, _ in t_ev]), n_frames=t_ev[0][1]["n_frames"],
                                     windows=int(sum(-(-int(n) // L) for n in bank["lengths_cpu"].tolist())))

    # the glue kernels at the AudioSet shape
    Kb, T = 527, 32
    big = dict(bank, classes=[str(c) for c in range(Kb)])
    draws = sed.draw_augment(rng.randint(0, args.clips, size=B).tolist(), bank["lengths_cpu"], L)
    idx, start, shift = (t.to(dev, torch.int32) for t in draws[:3])
    mix = draws[4].to(dev)
    y = torch.empty((B, Kb, T), device=dev)
    z = torch.randn(B, Kb, T, device=dev)
    z1 = torch.randn(B, 1280, T, device=dev)
    keep = torch.ones(B, 1280, device=dev)
    step = torch.zeros(1, device=dev)
    big_weak = dict(weak_bank, classes=big["classes"])
    w, framed = ops.sed_clip_targets(big_weak, idx, start, mix, L)
    step3 = torch.zeros(3, device=dev)
    z10, y10, w10 = z[:, :10].contiguous(), torch.zeros((B, 10, T), device=dev), w[:, :10].contiguous()
    glue = {
        "sed_targets": lambda: ops.sed_targets(big, idx, start, shift, mix, L, L // T, T, T, out=y),
        "frame_bce_fwd_bwd": lambda: ops.frame_bce_fwd_bwd(z, y, T, sums=step),
        "frame_grad_pad": lambda: ops.frame_grad_pad(z, T, 528),
        "frame_hidden_fwd": lambda: ops.frame_hidden_fwd(z1, keep),
        "frame_hidden_bwd": lambda: ops.frame_hidden_bwd(z1, z1, keep, 1280, T),
        "sed_clip_targets": lambda: ops.sed_clip_targets(big_weak, idx, start, mix, L, out=w, framed_out=framed),
        "weak_frame_bce_fwd_bwd": lambda: ops.weak_frame_bce_fwd_bwd(z, y, w, framed, T, sums=step3),
        "frame_bce_fwd_bwd_K10": lambda: ops.frame_bce_fwd_bwd(z10, y10, T, sums=step),
        "weak_frame_bce_fwd_bwd_K10": lambda: ops.weak_frame_bce_fwd_bwd(z10, y10, w10, framed, T, sums=step3),
    }
    result["glue_s"] = {}
    for name, fn in glue.items():
        fn()
        ts = [timed(lambda: [fn() for _ in range(20)])[0] / 20 for _ in range(3)]
        result["glue_s"][name] = statistics.median(ts)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
