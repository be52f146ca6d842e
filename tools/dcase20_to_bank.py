"""TAU Urban Acoustic Scenes 2020 Mobile (the reference's datasets/dcase20.py layout: meta.csv, evaluation_setup/, audio/) ->
a decoded bank directory of one split (waves.npy, labels.npy, names.txt, classes.json: efficientat_amd/dcase20.py).

    python tools/dcase20_to_bank.py DATA_DIR OUT_DIR --split train|test [--resample_rate 32000] [--float32] [--clip_seconds 10]

Every wav of the split (fold1_train.csv / fold1_evaluate.csv, in meta order) is decoded with `audio_io.load_audio` (mono,
resampled - the contract of the reference's librosa.load) and written through a memory map, so the host never holds the
split.  Each clip is padded with zeros or truncated to --clip_seconds.  The reference does NEITHER: every TAU clip is 10 s
long, and its default collate would fail on clips of different lengths; padding / truncating here only makes a damaged or
foreign file an (N, L) row instead of an error.  Labels are encoded over the whole meta.csv (dcase20.read_meta)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def convert(data_dir, out, split="train", resample_rate=32000, float32=False, clip_seconds=10):
    from numpy.lib.format import open_memmap

    from efficientat_amd.audio_io import load_audio
    from efficientat_amd.dcase20 import KINDS, split_rows
    if split not in ("train", "test"):
        raise ValueError("--split must be train or test")
    rows, encoders = split_rows(data_dir, split == "train")
    if not rows:
        raise ValueError(f"DCASE20 at {data_dir}: the {split} split lists no clip of meta.csv")
    L = int(clip_seconds * resample_rate)
    os.makedirs(out, exist_ok=True)
    waves = open_memmap(os.path.join(out, "waves.npy"), mode="w+", dtype=np.float32 if float32 else np.int16,
                        shape=(len(rows), L))
    for i, r in enumerate(rows):
        x, _ = load_audio(os.path.join(data_dir, r[0]), sr=resample_rate, mono=True)
        x = np.asarray(x, dtype=np.float32)[:L]
        x = np.concatenate((x, np.zeros(L - len(x), dtype=np.float32)))
        waves[i] = x if float32 else np.rint(np.clip(x, -1.0, 1.0) * 32767.0).astype(np.int16)
    waves.flush()
    del waves
    np.save(os.path.join(out, "labels.npy"), np.array([r[1:] for r in rows], dtype=np.int32))
    with open(os.path.join(out, "names.txt"), "w") as g:
        g.write("\n".join(r[0] for r in rows) + "\n")
    with open(os.path.join(out, "classes.json"), "w") as g:
        json.dump({k: encoders[k] for k in KINDS}, g)
    return len(rows)


if __name__ == "__main__":
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("data_dir")
    p.add_argument("out")
    p.add_argument("--split", choices=("train", "test"), required=True)
    p.add_argument("--resample_rate", type=int, default=32000)
    p.add_argument("--float32", action="store_true", help="store fp32 waveforms (default: int16)")
    p.add_argument("--clip_seconds", type=float, default=10)
    a = p.parse_args()
    print(f"{convert(a.data_dir, a.out, a.split, a.resample_rate, a.float32, a.clip_seconds)} clips -> {a.out}")
