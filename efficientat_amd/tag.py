"""Command line of the long-recording tagger (the reference's ``python windowed_inference.py``):

    python -m efficientat_amd.tag --audio_path A.wav [B.wav ...] --model mn10_as | --checkpoint F.pt [--width 1.0]
                                  [--window_size 10 --hop_length 2.5] [--labels_csv class_labels_indices.csv] [--json]

Prints, per window, what windowed_inference.py:143-148 prints (the top 5 tags), or with --json one line per file:
{"audio_path": ..., "windows": [{"start", "end", "tags": [{"tag", "probability"} x 10]}]}.
"""
import argparse
import contextlib
import csv
import io
import json
import sys

import torch

from .mn import get_model
from .tagger import EATagger
from .utils import NAME_TO_WIDTH


def read_labels(path):
    """display_name column of an AudioSet-style `index,mid,display_name` CSV (the reference's metadata file)."""
    with open(path, "r", newline="") as f:
        rows = list(csv.reader(f))
    return [r[2] for r in rows[1:]]


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--model", type=str, default="mn10_as", help="released model name")
    p.add_argument("--checkpoint", type=str, default=None, help="state dict of an MN model, instead of --model")
    p.add_argument("--width", type=float, default=None, help="width multiplier of --checkpoint (default: from --model)")
    p.add_argument("--audio_path", type=str, nargs="+", required=True, help="WAV files")
    p.add_argument("--window_size", type=float, default=10.0, help="window size in seconds")
    p.add_argument("--hop_length", type=float, default=2.5, help="hop length in seconds")
    p.add_argument("--labels_csv", type=str, default=None, help="index,mid,display_name CSV; default: class indices")
    p.add_argument("--batch_windows", type=int, default=64)
    p.add_argument("--json", action="store_true", help="one JSON line per file")
    args = p.parse_args(argv)

    labels = read_labels(args.labels_csv) if args.labels_csv else None
    if args.checkpoint:
        sd = torch.load(args.checkpoint, map_location="cpu")
        width = args.width if args.width is not None else NAME_TO_WIDTH(args.model)
        with contextlib.redirect_stdout(io.StringIO()):
            model = get_model(width_mult=width, num_classes=sd["classifier.5.weight"].shape[0])
        model.load_state_dict(sd)
        tagger = EATagger(model=model, labels=labels, batch_windows=args.batch_windows)
    else:
        tagger = EATagger(model_name=args.model, labels=labels, batch_windows=args.batch_windows)

    for path in args.audio_path:
        tags = tagger.tag_audio_window(path, window_size=args.window_size, hop_length=args.hop_length)
        if args.json:
            for w in tags:
                for t in w["tags"]:
                    t["probability"] = float(t["probability"])
            print(json.dumps({"audio_path": path, "windows": tags}))
            continue
        for window in tags:
            print(f'Window: {window["start"]:.2f} - {window["end"]:.2f}')
            for tag in window["tags"][:5]:
                print(f'\t{tag["tag"]}: {tag["probability"]:.2f}')
            print()
    return 0


if __name__ == "__main__":
    sys.exit(main())
