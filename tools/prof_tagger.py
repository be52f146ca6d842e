"""Wall time of tagging one long recording, the per-window host loop against the batched tagger (GPU diagnostic):

    python tools/prof_tagger.py [--minutes 10] [--repeats 5] [--out prof_tagger.json]

Workload: a synthetic 44.1 kHz stereo int16 WAV, window 10 s, hop 2.5 s, mn10 with synthetic weights.
  (a) loop     audio_io.load_audio (scipy decode + down-mix + resample_poly on the host), then the loop of
               tests/callpaths/driver.py::windowed: zero-pad, and per window one mel call, one forward at batch 1, one
               sigmoid, one device->host copy, one numpy argsort (fp32, without the driver's autocast, as (b))
  (b) batched  EATagger.tag_audio_window
Both are warmed up, then run alternately; each time is a host clock around work that ends in a device synchronise.  (b) is
also run once more stage by stage, a synchronise after each stage: decode, upload, resample, mel, forward, top-k + copy.
"""
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

from efficientat_amd import audio_io, ops, tagger  # noqa: E402
from efficientat_amd.mn import get_model  # noqa: E402
from efficientat_amd.preprocess import AugmentMelSTFT  # noqa: E402
from oracle import eat_oracle as O  # noqa: E402
from oracle import synth  # noqa: E402

SR = 32000


def write_recording(path, minutes, rate=44100, seed=0):
    from scipy.io import wavfile
    n = int(minutes * 60 * rate)
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    x = np.stack([0.2 * np.sin(2 * np.pi * (200.0 + 40.0 * np.sin(2 * np.pi * 0.05 * t)) * t * (c + 1))
                  + 0.05 * rng.standard_normal(n) for c in range(2)], axis=1)
    wavfile.write(path, rate, np.clip(x * 32768.0, -32768, 32767).astype(np.int16))


def loop_tagger(model, mel, path, window_s, hop_s, dev):
    """The parent commit's only way (the reference's loop on the drop-in modules)."""
    waveform, _ = audio_io.load_audio(path, sr=SR, mono=True)
    waveform = torch.from_numpy(waveform[None, :]).to(dev)
    win, hop = int(window_s * SR), int(hop_s * SR)
    n_windows = int(np.ceil((waveform.shape[1] - win) / hop)) + 1
    waveform = torch.nn.functional.pad(waveform, (0, n_windows * hop + win - waveform.shape[1]))
    tags = []
    with torch.no_grad():
        for i in range(n_windows):
            spec = mel(waveform[:, i * hop:i * hop + win])
            preds, _ = model(spec.unsqueeze(0))
            p = torch.sigmoid(preds.float()).squeeze().cpu().numpy()
            order = np.argsort(p)[::-1]
            tags.append({"start": i * hop / SR, "end": (i * hop + win) / SR,
                         "tags": [{"tag": int(order[k]), "probability": p[order[k]]} for k in range(10)]})
    torch.cuda.synchronize()
    return tags


def staged(t, path, window_s, hop_s):
    """(b) stage by stage, a device synchronise after each -> {stage: seconds}."""
    from scipy.io import wavfile
    out = {}

    def lap(name, t0):
        torch.cuda.synchronize()
        out[name] = time.perf_counter() - t0
        return time.perf_counter()

    t0 = time.perf_counter()
    src_sr, data = wavfile.read(path)
    t0 = lap("decode", t0)
    frames = torch.from_numpy(np.ascontiguousarray(data)).to(t.device)
    t0 = lap("upload", t0)
    up, down, taps = tagger.resample_plan(src_sr, t.sample_rate)
    wave = ops.resample_mono(frames, up, down, taps.to(t.device))
    t0 = lap("resample", t0)
    starts, valids, W = t.window_plan(wave.numel(), window_s, hop_s)
    ds, dv = (x.to(t.device) for x in ops.check_windows(starts, valids, W, wave.numel()))
    specs = []
    with torch.no_grad():
        for lo in range(0, len(starts), t.batch_windows):
            specs.append(t.mel.forward_windows(wave, ds[lo:lo + t.batch_windows], dv[lo:lo + t.batch_windows], W))
        t0 = lap("mel", t0)
        logits = torch.cat([t.model(s.unsqueeze(1))[0] for s in specs])
        t0 = lap("forward", t0)
        prob, index = ops.tag_topk(logits, 10)
        prob, index = prob.cpu(), index.cpu()
    lap("topk_copy", t0)
    out["windows"] = len(starts)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=10.0)
    ap.add_argument("--window_size", type=float, default=10.0)
    ap.add_argument("--hop_length", type=float, default=2.5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batch_windows", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "prof_tagger needs a GPU"
    dev = torch.device("cuda:0")
    with contextlib.redirect_stdout(io.StringIO()):
        model = get_model(width_mult=1.0)
        mel = AugmentMelSTFT(n_mels=128, sr=SR, win_length=800, hopsize=320).to(dev).eval()
    x_cal = O.mel_forward(synth.parity_clips(64000, seed=3)).unsqueeze(1)         # running statistics as __graft_entry__.smoke
    model.load_state_dict(synth.calibrate(synth.synth_state(synth.mn_shapes(1.0), seed=0), O.mn_forward, x_cal))
    model.to(dev).eval()
    t = tagger.EATagger(model=model, batch_windows=args.batch_windows)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "recording.wav")
        write_recording(path, args.minutes)
        a = lambda: loop_tagger(model, mel, path, args.window_size, args.hop_length, dev)
        b = lambda: t.tag_audio_window(path, window_size=args.window_size, hop_length=args.hop_length)
        ra, rb = a(), b()                                  # warm-up of both (and a look at what they return)
        agree = sum(x["tags"][0]["tag"] == y["tags"][0]["tag"] for x, y in zip(ra, rb))
        dp = max(abs(float(x["tags"][0]["probability"]) - float(y["tags"][0]["probability"])) for x, y in zip(ra, rb))
        times = {"loop": [], "batched": []}
        for _ in range(args.repeats):
            for name, fn in (("loop", a), ("batched", b)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
        stages = staged(t, path, args.window_size, args.hop_length)
    result = {"workload": {"minutes": args.minutes, "rate": 44100, "channels": 2, "window_s": args.window_size,
                           "hop_s": args.hop_length, "windows": len(rb), "batch_windows": args.batch_windows},
              "top1_agree": f"{agree}/{len(rb)}", "top1_prob_max_diff": dp, "stages_batched_s": stages}
    for name, ts in times.items():
        result[name] = {"median_s": statistics.median(ts), "min_s": min(ts), "max_s": max(ts), "all_s": [round(x, 4) for x in ts]}
    result["speedup_median"] = result["loop"]["median_s"] / result["batched"]["median_s"]
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
