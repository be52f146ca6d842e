"""Command line of sound event detection (efficientat_amd/detection.py):

    python -m efficientat_amd.detect --audio_path A.wav [B.wav ...] --model mn10_as | --checkpoint F.pt [--width 1.0]
                                     [--labels_csv class_labels_indices.csv] [--window_size 10.24 --hop_length 5.12]
                                     [--median_ms 960 --threshold 0.5 --low_threshold 0.3 --min_duration_ms 0 --max_gap_ms 0]
                                     [--thresholds_file ops.json] [--json | --out events.tsv]

Prints one line per event (file, onset and offset in seconds, label, peak and mean probability); with --json one line per
file: {"audio_path": ..., "events": [{"label", "onset", "offset", "peak", "mean"}]}; with --out writes the DCASE
tab-separated columns `filename onset offset event_label`, sorted by file, onset, offset and label.
--thresholds_file takes the per-class operating points that `finetune_sed --save_thresholds` / `score_sed` write
(sed.load_operating_points): its thresholds, post-processing values (the per-class median widths `class_median_ms` when it
has them) and labels become this run's defaults; a flag given on the command line still wins, --median_ms for every class.
"""
import argparse
import contextlib
import io
import json
import os
import sys

import torch

from .detection import EADetector
from .mn import get_model
from .tag import read_labels
from .utils import NAME_TO_WIDTH


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--model", type=str, default="mn10_as", help="released model name")
    p.add_argument("--checkpoint", type=str, default=None, help="state dict of an MN model, instead of --model")
    p.add_argument("--width", type=float, default=None, help="width multiplier of --checkpoint (default: from --model)")
    p.add_argument("--audio_path", type=str, nargs="+", required=True, help="WAV files")
    p.add_argument("--window_size", type=float, default=None, help="window size in seconds (a multiple of 0.32; default 10.24)")
    p.add_argument("--hop_length", type=float, default=None, help="window hop in seconds (a multiple of 0.32; default 5.12)")
    p.add_argument("--median_ms", type=float, default=None, help="width of the median filter (default 960)")
    p.add_argument("--threshold", type=float, default=None, help="a run of frames must reach it to be an event (default 0.5)")
    p.add_argument("--low_threshold", type=float, default=None, help="a run lasts while frames stay at or above it")
    p.add_argument("--min_duration_ms", type=float, default=None, help="shorter events are dropped (default 0)")
    p.add_argument("--max_gap_ms", type=float, default=None, help="events at most this far apart are merged (default 0)")
    p.add_argument("--taper", type=str, default=None, choices=["triangle", "uniform"], help="default triangle")
    p.add_argument("--thresholds_file", type=str, default=None,
                   help="per-class operating points (sed.save_operating_points): the defaults of this run")
    p.add_argument("--labels_csv", type=str, default=None, help="index,mid,display_name CSV; default: class indices")
    p.add_argument("--batch_windows", type=int, default=64)
    p.add_argument("--json", action="store_true", help="one JSON line per file")
    p.add_argument("--out", type=str, default=None, help="write the DCASE columns filename onset offset event_label here")
    args = p.parse_args(argv)
    points = None
    if args.thresholds_file:
        from .sed import load_operating_points
        points = load_operating_points(args.thresholds_file)
    defaults = dict(window_size=10.24, hop_length=5.12, median_ms=960.0, threshold=0.5, min_duration_ms=0.0, max_gap_ms=0.0,
                    taper="triangle")
    median_given = args.median_ms is not None
    file_low = args.low_threshold is None and args.threshold is None and points is not None
    for name, value in defaults.items():                     # a flag, else the file's value, else the default
        if getattr(args, name) is None:
            setattr(args, name, value if points is None else points[name])
    if points is not None and not median_given and points.get("class_median_ms") is not None:
        args.median_ms = points["class_median_ms"]           # the file's per-class widths; an explicit --median_ms wins
    if file_low:                                             # (an explicit --threshold alone means low = high, as without a file)
        args.low_threshold = points["low_threshold"]

    labels = read_labels(args.labels_csv) if args.labels_csv else None
    kw = dict(labels=labels, batch_windows=args.batch_windows, clip_seconds=args.window_size, hop_seconds=args.hop_length,
              taper=args.taper)
    if args.checkpoint:
        sd = torch.load(args.checkpoint, map_location="cpu")
        width = args.width if args.width is not None else NAME_TO_WIDTH(args.model)
        with contextlib.redirect_stdout(io.StringIO()):
            model = get_model(width_mult=width, num_classes=sd["classifier.5.weight"].shape[0])
        model.load_state_dict(sd)
        detector = EADetector(model=model.eval(), **kw)
    else:
        detector = EADetector(model_name=args.model, **kw)
    if points is not None and len(points["classes"]) != detector.num_classes:
        raise SystemExit(f"detect: {args.thresholds_file} holds {len(points['classes'])} classes, the model "
                         f"{detector.num_classes}")
    if points is not None and labels is None:
        detector.labels = list(points["classes"])

    waves = [detector.load_waveform(path) for path in args.audio_path]
    found = detector.detect(waves, threshold=args.threshold, low_threshold=args.low_threshold, median_ms=args.median_ms,
                            min_duration_ms=args.min_duration_ms, max_gap_ms=args.max_gap_ms)
    rows = []
    for path, events in zip(args.audio_path, found):
        if args.json:
            print(json.dumps({"audio_path": path, "events": [
                {"label": label, "onset": on, "offset": off, "peak": peak, "mean": mean} for label, on, off, peak, mean in events]}))
        for label, on, off, peak, mean in sorted(events, key=lambda e: (e[1], e[2], str(e[0]))):
            rows.append((os.path.basename(path), on, off, label))
            if not args.json and not args.out:
                print(f"{path}\t{on:.2f}\t{off:.2f}\t{label}\t{peak:.3f}\t{mean:.3f}")
    if args.out:
        with open(args.out, "w") as f:
            f.write("filename\tonset\toffset\tevent_label\n")
            for name, on, off, label in rows:
                f.write(f"{name}\t{on:.3f}\t{off:.3f}\t{label}\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
