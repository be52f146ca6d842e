"""Fine-tune an MN on strongly labelled sound events on the HIP path: frame-level training of what `detect` runs.

    python -m efficientat_amd.finetune_sed --train_bank DIR --valid_bank DIR [--init_checkpoint mn10_as.pt] [--save sed.pt]

Each DIR is a decoded strong-label split (sed.load_bank: waves.npy, lengths.npy, names.txt, classes.txt, events.npy,
event_offsets.npy; tools/strong_to_bank.py writes one from WAV files and a `filename onset offset event_label` table).  Each
step is one hipGraph replay of crop / pad + wave augmentation + frame targets -> mel -> mix-up -> trunk -> frame head ->
frame BCE -> backward -> FusedAdam (sed.GraphedFrameBCETrainer; `--no_graph`: the eager FrameBCETrainer).  After every epoch
the validation split is scored frame by frame (sed.evaluate_frames: frame mAP / ROC, segment-based F1 at `--threshold`,
val_loss); with `--event_eval` also event by event (sed.evaluate_events: collar-based F1 at a grid of thresholds, the
post-processing of `detect` given by `--median_ms --min_duration_ms --max_gap_ms --low_ratio`), and `--save_thresholds FILE`
writes the per-class operating points of the last validation for `detect --thresholds_file` (`--tune_median
[--median_grid_ms a,b,c]` also tunes the median width per class, sed.tune_postprocessing); with `--psds_eval` also with
PSDS (sed.evaluate_psds: the scenarios of `--psds`, default both, criteria `--dtc --gtc --cttc --alpha_ct --alpha_st --e_max`).
A training bank may hold weakly labelled clips (strong.npy: clip-level tags only, e.g. DESED's weak.tsv through
`tools/strong_to_bank.py --weak_tsv`): `--weak_weight W` with W > 0 trains on strong and weak clips in the same batches
(sed.GraphedWeakFrameTrainer / WeakFrameTrainer: the frame BCE over the clips with frame truth + W times a clip-level BCE
behind linear-softmax pooling of the frame probabilities, one kernel).  The validation bank must be all strong.
`--save` writes the final plain state dict: an mlp-head MN with K = the bank's classes, which
`detection.EADetector(model=...)` and `python -m efficientat_amd.detect --checkpoint` accept.  `--init_checkpoint` loads a
local state dict and drops its output layer when the class count differs (finetune.load_init_checkpoint).

Augmentation arguments and the schedule are finetune_fsd50k's.  Only MN models with the mlp head, at 32 kHz.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

from .finetune_esc50 import build
from .utils import exp_warmup_linear_down

METRICS = ("frame_mAP", "frame_ROC", "micro_f1", "micro_precision", "micro_recall", "macro_f1", "macro_precision",
           "macro_recall", "val_loss")


EVENT_KEYS = ("event_threshold", "event_micro_f1", "event_micro_precision", "event_micro_recall", "event_macro_f1",
              "event_macro_precision", "event_macro_recall", "event_macro_f1_best", "event_best_threshold", "event_collar_ms",
              "event_offset_pct", "event_eval_s", "thresholds_file")


def add_event_args(p):
    """The arguments of event-based scoring (sed.evaluate_events), shared with score_sed."""
    p.add_argument("--collar_ms", type=float, default=200.0, help="onset collar, and the floor of the offset collar")
    p.add_argument("--offset_pct", type=float, default=0.2, help="offset collar as a fraction of the reference's length")
    p.add_argument("--median_ms", type=float, default=960.0, help="median filter of the scored detector")
    p.add_argument("--min_duration_ms", type=float, default=0.0, help="its minimum event length")
    p.add_argument("--max_gap_ms", type=float, default=0.0, help="its merge gap")
    p.add_argument("--low_ratio", type=float, default=1.0, help="low threshold as a fraction of the threshold")
    p.add_argument("--save_thresholds", default=None, help="file for the per-class operating points (detect --thresholds_file)")
    p.add_argument("--tune_median", action="store_true",
                   help="also tune the median width per class over --median_grid_ms (sed.tune_postprocessing)")
    p.add_argument("--median_grid_ms", type=_grid_ms, default=None, metavar="a,b,c",
                   help="median widths to try with --tune_median, in ms (default: the odd widths 1 .. 15 frames)")


def _grid_ms(text):
    """`--median_grid_ms` values: "0,960,2240" -> [float]."""
    try:
        out = [float(t) for t in str(text).split(",") if t.strip()]
    except ValueError:
        out = []
    if not out:
        raise argparse.ArgumentTypeError(f"--median_grid_ms takes a comma-separated list of ms (got {text!r})")
    return out


def tuned_text(ev):
    """What the programs print about a `sed.tune_postprocessing` result, next to the scores at the reference width."""
    return (f"median tuned per class (on this split): macro F1 {ev['macro_f1_tuned']:.4f}; best single width "
            f"{ev['best_single_median_ms']:.0f} ms: {ev['macro_f1_best_single']:.4f}")


def event_eval(args, model, mel, bank):
    """`sed.evaluate_events` - with --tune_median `sed.tune_postprocessing` - with the command line's settings -> (its result,
    the JSON line's keys)."""
    from . import sed
    kw = dict(low_ratio=args.low_ratio, median_ms=args.median_ms, min_duration_ms=args.min_duration_ms,
              max_gap_ms=args.max_gap_ms, collar_ms=args.collar_ms, offset_pct=args.offset_pct, threshold=args.threshold,
              batch_windows=args.batch_windows)
    if args.tune_median:
        ev = sed.tune_postprocessing(model, mel, bank, median_grid_ms=args.median_grid_ms, **kw)
    else:
        ev = sed.evaluate_events(model, mel, bank, **kw)
    keys = {"event_threshold": ev["threshold"]}
    keys.update({"event_" + k: ev[k] for k in sed.SCORE_NAMES})
    keys.update({"event_macro_f1_best": ev["macro_f1_best"], "event_best_threshold": [float(v) for v in ev["best_threshold"]],
                 "event_collar_ms": args.collar_ms, "event_offset_pct": args.offset_pct, "event_eval_s": round(ev["eval_s"], 3),
                 "thresholds_file": args.save_thresholds})
    if args.tune_median:
        keys.update({"macro_f1_tuned": ev["macro_f1_tuned"], "macro_f1_best_single": ev["macro_f1_best_single"],
                     "best_single_median_ms": ev["best_single_median_ms"],
                     "best_median_ms": [float(v) for v in ev["best_median_ms"]]})
    return ev, keys


def _scenarios(text):
    """`--psds` values: "1", "2" or "1,2" -> [int]."""
    try:
        out = [int(t) for t in str(text).split(",") if t.strip()]
    except ValueError:
        out = []
    if not out or any(v not in (1, 2) for v in out):
        raise argparse.ArgumentTypeError(f"--psds takes 1, 2 or 1,2 (got {text!r})")
    return out


def add_psds_args(p):
    """The arguments of PSDS scoring (sed.evaluate_psds), shared with score_sed."""
    p.add_argument("--psds", type=_scenarios, action="append", default=None, metavar="{1,2}",
                   help="PSDS scenario(s) of DCASE Task 4 to score: repeatable or comma-separated")
    for name, what in (("dtc", "detection tolerance criterion"), ("gtc", "ground-truth intersection criterion"),
                       ("cttc", "cross-trigger tolerance criterion"), ("alpha_ct", "weight of the cross-trigger rate"),
                       ("alpha_st", "weight of the spread over classes")):
        p.add_argument("--" + name, type=float, default=None, help=f"PSDS: {what} (default: the scenario's)")
    p.add_argument("--e_max", type=float, default=100.0, help="PSDS: largest effective false positives per hour")


def psds_scenarios(args, default=()):
    """The scenarios the command line asks for, in first-mention order: those of --psds, else `default`, else scenario 1 as
    the base of explicit criteria (then under the plain key "psds") -> [(scenario, key of the JSON line)]."""
    asked = list(dict.fromkeys(v for group in (args.psds or []) for v in group)) or list(default)
    if asked:
        return [(v, f"psds_scenario{v}") for v in asked]
    explicit = any(getattr(args, k) is not None for k in ("dtc", "gtc", "cttc", "alpha_ct", "alpha_st")) or args.e_max != 100.0
    return [(1, "psds")] if explicit else []


def psds_eval(args, model, mel, bank, scenarios, median_ms=None):
    """`sed.evaluate_psds` per scenario with the command line's settings -> the JSON line's keys.  median_ms: per-class
    widths to use in place of --median_ms."""
    from . import sed
    keys, seconds = {}, 0.0
    for scenario, key in scenarios:
        ev = sed.evaluate_psds(model, mel, bank, scenario=scenario, dtc=args.dtc, gtc=args.gtc, cttc=args.cttc,
                               alpha_ct=args.alpha_ct, alpha_st=args.alpha_st, e_max=args.e_max, low_ratio=args.low_ratio,
                               median_ms=args.median_ms if median_ms is None else median_ms,
                               min_duration_ms=args.min_duration_ms, max_gap_ms=args.max_gap_ms,
                               batch_windows=args.batch_windows)
        keys[key] = ev["psds"]
        seconds += ev["eval_s"]
    keys["psds_eval_s"] = round(seconds, 3)
    return keys


def check_weak_banks(args, n_weak_train, n_weak_valid):
    """The rules of weakly labelled clips, as argument errors: a training bank that holds some needs --weak_weight > 0, a
    validation bank must hold none."""
    error = argparse.ArgumentParser(prog="finetune_sed", add_help=False).error     # (exit status 2, as parse_args' own)
    if n_weak_train and not args.weak_weight > 0:
        error(f"--train_bank holds {n_weak_train} weakly labelled clips (strong.npy): set --weak_weight W > 0 to train on them")
    if n_weak_valid:
        error(f"--valid_bank holds {n_weak_valid} weakly labelled clips (strong.npy): scoring needs onset / offset truth")


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="strong-label SED fine-tuning on the HIP path")
    p.add_argument("--train_bank", required=True, help="decoded training split (sed.load_bank)")
    p.add_argument("--valid_bank", required=True, help="decoded validation split, scored after every epoch")
    p.add_argument("--init_checkpoint", default=None, help="state dict to start from (its output layer is re-sized)")
    p.add_argument("--save", default=None, help="file for the final state dict (loads into EADetector / detect --checkpoint)")
    p.add_argument("--threshold", type=float, default=0.5, help="probability at which a frame counts as active in the F1")
    p.add_argument("--json", action="store_true", help="print one JSON line with the run's results at the end")
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--batch_windows", type=int, default=64, help="windows per evaluation chunk")
    p.add_argument("--model_name", type=str, default="mn10_as")
    p.add_argument("--model_width", type=float, default=1.0)
    p.add_argument("--se_dims", type=str, default="c")
    p.add_argument("--n_epochs", type=int, default=80)
    p.add_argument("--mixup_alpha", type=float, default=0.3)
    p.add_argument("--no_roll", action="store_true", default=False)
    p.add_argument("--no_wavmix", action="store_true", default=False)
    p.add_argument("--gain_augment", type=int, default=12)
    p.add_argument("--weight_decay", type=float, default=0.0)
    p.add_argument("--lr", type=float, default=7e-5)
    p.add_argument("--warm_up_len", type=int, default=10)
    p.add_argument("--ramp_down_start", type=int, default=10)
    p.add_argument("--ramp_down_len", type=int, default=65)
    p.add_argument("--last_lr_value", type=float, default=0.01)
    p.add_argument("--window_size", type=int, default=800)
    p.add_argument("--hop_size", type=int, default=320)
    p.add_argument("--n_fft", type=int, default=1024)
    p.add_argument("--n_mels", type=int, default=128)
    p.add_argument("--freqm", type=int, default=0)
    p.add_argument("--timem", type=int, default=0)
    p.add_argument("--fmin", type=int, default=0)
    p.add_argument("--fmax", type=int, default=None)
    p.add_argument("--fmin_aug_range", type=int, default=10)
    p.add_argument("--fmax_aug_range", type=int, default=2000)
    p.add_argument("--clip_frames", type=int, default=32, help="frames per training clip and evaluation window (32 = 10.24 s)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--no_graph", action="store_true", help="eager FrameBCETrainer instead of the captured step")
    p.add_argument("--weak_weight", type=float, default=0.0,
                   help="weight of the pooled clip-level BCE; > 0 trains on weakly labelled clips as well (strong.npy)")
    p.add_argument("--max_steps", type=int, default=0, help="stop after this many steps (benchmarks / tests); 0 = whole epochs")
    p.add_argument("--precision", default=None, help="model.train_precision (auto / fp32 / bf16)")
    add_event_args(p)
    p.add_argument("--event_eval", action="store_true", help="also score the validation split event by event (collar F1)")
    add_psds_args(p)
    p.add_argument("--psds_eval", action="store_true", help="also score the validation split with PSDS (--psds, default 1,2)")
    args = p.parse_args(argv)
    if psds_scenarios(args) and not args.psds_eval:
        p.error("--psds and its criteria need --psds_eval")
    if args.save_thresholds and not args.event_eval:
        p.error("--save_thresholds needs --event_eval")
    if (args.tune_median or args.median_grid_ms) and not args.event_eval:
        p.error("--tune_median and --median_grid_ms need --event_eval")
    if args.median_grid_ms and not args.tune_median:
        p.error("--median_grid_ms needs --tune_median")
    if args.model_name.startswith("dymn"):
        p.error("frame-level training covers the static MobileNets (mn*) only")
    if args.clip_frames < 1:
        p.error("--clip_frames must be >= 1")
    if not 0.0 <= args.weak_weight < float("inf"):
        p.error("--weak_weight must be finite and not negative")
    args.head_type, args.resample_rate, args.pretrain_final_temp = "mlp", 32000, 1.0
    return args


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("efficientat_amd.finetune_sed needs a GPU: the package has no CPU path")
    from . import detection, sed
    from .optim import FusedAdam

    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    t_load = time.perf_counter()
    train = sed.load_bank(args.train_bank, device=dev)
    valid = sed.load_bank(args.valid_bank, device=dev)
    t_load = time.perf_counter() - t_load
    if train["classes"] != valid["classes"]:
        raise SystemExit("finetune_sed: the two banks differ in classes.txt")
    check_weak_banks(args, sed.n_weak(train), sed.n_weak(valid))
    weak = args.weak_weight > 0
    n_train, K = train["lengths"].numel(), len(train["classes"])
    print(f"[finetune_sed] {n_train} training / {valid['lengths'].numel()} validation clips, {K} classes, "
          f"{train['events'].shape[0]} / {valid['events'].shape[0]} events resident on {dev} ({t_load:.1f} s to load)",
          file=sys.stderr, flush=True)
    model, mel = build(args, dev, K)
    L = args.clip_frames * detection.check_model(model)[1] * args.hop_size

    graphed = not args.no_graph
    lr = torch.tensor(args.lr, device=dev) if graphed else args.lr            # tensor lr: the schedule needs no re-capture
    opt = FusedAdam(model.parameters(), lr=lr, weight_decay=args.weight_decay, capturable=graphed)
    sched = torch.optim.lr_scheduler.LambdaLR(
        opt, exp_warmup_linear_down(args.warm_up_len, args.ramp_down_len, args.ramp_down_start, args.last_lr_value))
    model.train()
    mel.train()
    common = dict(clip_samples=L, mixup_alpha=args.mixup_alpha, gain_augment=args.gain_augment, roll=not args.no_roll,
                  wavmix=not args.no_wavmix)
    if weak:
        trainer = (sed.GraphedWeakFrameTrainer(model, mel, opt, train, args.batch_size, weak_weight=args.weak_weight, **common)
                   if graphed else sed.WeakFrameTrainer(model, mel, opt, train, weak_weight=args.weak_weight, **common))
    else:
        trainer = (sed.GraphedFrameBCETrainer(model, mel, opt, train, args.batch_size, **common) if graphed
                   else sed.FrameBCETrainer(model, mel, opt, train, **common))

    steps_total, clips_total, t_train = 0, 0, 0.0
    ev, stats, done = None, {"train_loss": float("nan")}, False
    ee, ee_keys, ps_keys = None, {}, {}
    for epoch in range(args.n_epochs):
        order = torch.randperm(n_train)                                       # shuffle, partial last batch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n_ep = 0
        for s in range(0, n_train, args.batch_size):
            batch = order[s:s + args.batch_size].tolist()
            trainer.step(batch)
            n_ep += 1
            clips_total += len(batch)
            if args.max_steps and steps_total + n_ep >= args.max_steps:
                done = True
                break
        sched.step()
        stats = trainer.epoch_stats()                                         # the one host sync of the epoch
        torch.cuda.synchronize()
        t_train += time.perf_counter() - t0
        steps_total += n_ep
        ev = sed.evaluate_frames(model, mel, valid, args.batch_windows, args.threshold, clip_samples=L)
        print(f"[finetune_sed] epoch {epoch + 1}/{args.n_epochs}: {n_ep} steps, train_loss {stats['train_loss']:.5f}, "
              f"frame mAP {ev['frame_mAP']:.4f}, ROC {ev['frame_ROC']:.4f}, micro F1 {ev['micro_f1']:.4f}, macro F1 "
              f"{ev['macro_f1']:.4f}, val_loss {ev['val_loss']:.5f}, lr {float(sched.get_last_lr()[0]):.2e}", file=sys.stderr,
              flush=True)
        if args.event_eval:
            ee, ee_keys = event_eval(args, model, mel, valid)
            print(f"[finetune_sed] events at {ee['threshold']:.2f}: micro F1 {ee['micro_f1']:.4f}, macro F1 {ee['macro_f1']:.4f}; "
                  f"macro F1 at the per-class best thresholds (tuned on this split) {ee['macro_f1_best']:.4f} "
                  f"({ee['eval_s']:.2f} s)", file=sys.stderr, flush=True)
            if args.tune_median:
                print("[finetune_sed] " + tuned_text(ee), file=sys.stderr, flush=True)
        if args.psds_eval:
            ps_keys = psds_eval(args, model, mel, valid, psds_scenarios(args, default=(1, 2)))
            print("[finetune_sed] " + ", ".join(f"{k} {v:.4f}" for k, v in ps_keys.items() if k != "psds_eval_s")
                  + f" ({ps_keys['psds_eval_s']:.2f} s)", file=sys.stderr, flush=True)
        if done:
            break
    if args.save_thresholds and ee is not None:
        sed.save_operating_points(args.save_thresholds, ee, valid["classes"])
    if args.save:
        os.makedirs(os.path.dirname(os.path.abspath(args.save)), exist_ok=True)
        torch.save(model.state_dict(), args.save)
    if args.json:
        line = {"what": "efficientat_amd.finetune_sed", "model": args.model_name, "classes": K, "steps": steps_total,
                "epochs": epoch + 1, "batch_size": args.batch_size, "clip_samples": L,
                "launch": "hipGraph replay" if graphed else "eager", "threshold": args.threshold,
                "train_loss": stats["train_loss"], "clips_per_s": round(clips_total / max(t_train, 1e-9), 1),
                "n_frames": ev["n_frames"], "eval_s": round(ev["eval_s"], 3), "checkpoint": args.save}
        if weak:
            line.update({"weak_weight": args.weak_weight, "n_weak": sed.n_weak(train),
                         "train_frame_loss": stats["train_frame_loss"], "train_clip_loss": stats["train_clip_loss"]})
        line.update({k: ev[k] for k in METRICS})
        line.update(ee_keys)
        line.update(ps_keys)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
