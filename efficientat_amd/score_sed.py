"""Score an existing strong-label SED checkpoint event by event, without training:

    python -m efficientat_amd.score_sed --checkpoint sed.pt --bank DIR [--model mn10_as | --width 1.0]
                                        [--collar_ms 200 --offset_pct 0.2 --median_ms 960 --min_duration_ms 0 --max_gap_ms 0
                                         --low_ratio 1.0 --threshold 0.5] [--save_thresholds ops.json] [--json]
                                        [--tune_median [--median_grid_ms a,b,c]] [--operating_points ops.json]
                                        [--psds 1,2] [--dtc --gtc --cttc --alpha_ct --alpha_st --e_max]

DIR is a decoded strong-label split (sed.load_bank), the checkpoint a state dict of an mlp-head MN with the bank's classes
(what `finetune_sed --save` writes).  `sed.evaluate_events` runs the detector of `detect` over every clip and scores its
events with onset / offset collars at the 49 thresholds k / 50 in one kernel launch per chunk of clips.  Prints micro / macro
F1, precision and recall at `--threshold`, and macro F1 at the per-class best thresholds (tuned on this very split);
`--save_thresholds` writes those operating points for `detect --thresholds_file`; `--json` prints one JSON line.
`--tune_median` also tries a grid of median widths in the same walk (sed.tune_postprocessing), prints macro F1 with the width
and threshold tuned per class next to the best single width, and `--save_thresholds` then writes `class_median_ms` too.
`--operating_points FILE` scores such a file as it stands on `--bank` (sed.score_operating_points: a file tuned on another
split is judged on this one) under `*_at_ops` keys, and PSDS then runs at the file's per-class widths.
`--psds` adds PSDS (sed.evaluate_psds) of the same detector over the same grid for scenario 1 and / or 2 of DCASE Task 4, as
`psds_scenario1` / `psds_scenario2`; explicit criteria override the scenario's, and without `--psds` they score under `psds`.
"""
import argparse
import contextlib
import io
import json
import sys

import torch

from .finetune_sed import add_event_args, add_psds_args, event_eval, psds_eval, psds_scenarios, tuned_text
from .utils import NAME_TO_WIDTH


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="event-based (collar) scoring of a strong-label SED checkpoint")
    p.add_argument("--checkpoint", required=True, help="state dict of an mlp-head MN (finetune_sed --save)")
    p.add_argument("--bank", required=True, help="decoded strong-label split to score (sed.load_bank)")
    p.add_argument("--model", type=str, default="mn10_as", help="released model name that fixes the width")
    p.add_argument("--width", type=float, default=None, help="width multiplier of --checkpoint (default: from --model)")
    p.add_argument("--threshold", type=float, default=0.5, help="threshold whose scores are reported")
    p.add_argument("--batch_windows", type=int, default=64, help="windows per forward chunk")
    p.add_argument("--window_size", type=int, default=800)
    p.add_argument("--hop_size", type=int, default=320)
    p.add_argument("--n_fft", type=int, default=1024)
    p.add_argument("--n_mels", type=int, default=128)
    p.add_argument("--json", action="store_true", help="print one JSON line with the results")
    p.add_argument("--operating_points", default=None,
                   help="operating-point file to score as it stands on --bank (sed.score_operating_points)")
    add_event_args(p)
    add_psds_args(p)
    args = p.parse_args(argv)
    if args.median_grid_ms and not args.tune_median:
        p.error("--median_grid_ms needs --tune_median")
    return args


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("efficientat_amd.score_sed needs a GPU: the package has no CPU path")
    from . import sed
    from .mn import get_model
    from .preprocess import AugmentMelSTFT

    dev = torch.device("cuda", torch.cuda.current_device())
    bank = sed.load_bank(args.bank, device=dev)
    K = len(bank["classes"])
    sd = torch.load(args.checkpoint, map_location="cpu")
    if sd["classifier.5.weight"].shape[0] != K:
        raise SystemExit(f"score_sed: the checkpoint has {sd['classifier.5.weight'].shape[0]} classes, the bank {K}")
    width = args.width if args.width is not None else NAME_TO_WIDTH(args.model)
    with contextlib.redirect_stdout(io.StringIO()):
        model = get_model(width_mult=width, num_classes=K)
        mel = AugmentMelSTFT(n_mels=args.n_mels, sr=32000, win_length=args.window_size, hopsize=args.hop_size, n_fft=args.n_fft,
                             freqm=0, timem=0)
    model.load_state_dict(sd)
    model.to(dev).eval()
    mel.to(dev).eval()
    ev, keys = event_eval(args, model, mel, bank)
    if args.save_thresholds:
        sed.save_operating_points(args.save_thresholds, ev, bank["classes"])
    print(f"[score_sed] {ev['n_clips']} clips, {ev['n_ref']} reference events, {K} classes; at threshold {ev['threshold']:.2f}: "
          f"micro F1 {ev['micro_f1']:.4f}, macro F1 {ev['macro_f1']:.4f}; macro F1 at the per-class best thresholds (tuned on "
          f"this split) {ev['macro_f1_best']:.4f} ({ev['eval_s']:.2f} s)", file=sys.stderr, flush=True)
    if args.tune_median:
        print("[score_sed] " + tuned_text(ev), file=sys.stderr, flush=True)
    ops_keys, points = {}, None
    if args.operating_points:
        points = sed.load_operating_points(args.operating_points, classes=bank["classes"])
        at = sed.score_operating_points(model, mel, bank, points, batch_windows=args.batch_windows)
        ops_keys = {k + "_at_ops": at[k] for k in sed.SCORE_NAMES}
        ops_keys.update({"operating_points": args.operating_points, "eval_s_at_ops": round(at["eval_s"], 3)})
        print(f"[score_sed] at the operating points of {args.operating_points}: micro F1 {at['micro_f1']:.4f}, macro F1 "
              f"{at['macro_f1']:.4f} ({at['eval_s']:.2f} s)", file=sys.stderr, flush=True)
    scenarios = psds_scenarios(args)
    ps_keys = {}
    if scenarios:
        file_ms = None if points is None else points.get("class_median_ms")
        ps_keys = psds_eval(args, model, mel, bank, scenarios, median_ms=file_ms)
        print("[score_sed] " + ", ".join(f"{k} {v:.4f}" for k, v in ps_keys.items() if k != "psds_eval_s")
              + f" ({ps_keys['psds_eval_s']:.2f} s)", file=sys.stderr, flush=True)
    if args.json:
        line = {"what": "efficientat_amd.score_sed", "checkpoint": args.checkpoint, "classes": K, "n_clips": ev["n_clips"],
                "n_ref": ev["n_ref"]}
        line.update(keys)
        line.update(ops_keys)
        line.update(ps_keys)
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
