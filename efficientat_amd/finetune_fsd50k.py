"""Fine-tune or evaluate an MN / DyMN on FSD50K on the HIP path: ex_fsd50k.py with the data resident on the GPU.

    python -m efficientat_amd.finetune_fsd50k --train --train_bank DIR --valid_bank DIR [--init_checkpoint mn10_as.pt] [...]
    python -m efficientat_amd.finetune_fsd50k --eval_bank DIR --init_checkpoint mn10_fsd50k.pt [--variable_eval_length]

Each DIR is a decoded split (fsd50k.load_bank: waves.npy, lengths.npy, targets.npy, names.txt; tools/fsd50k_to_bank.py writes
one from the reference's FSD50K.{train,val,eval}_mp3.hdf).  The clips keep their own lengths (0.3 s - 30 s) in one flat buffer
in HBM.  `--train`: each step is one hipGraph replay of crop / pad + wave augmentation + label rows -> mel -> mix-up -> model
-> BCE -> backward -> FusedAdam (finetune.GraphedBCETrainer; `--no_graph`: the eager BCETrainer); after every epoch the
validation split is evaluated as the reference's `_test` (mAP and ROC on the logits, val_loss), at 10 s or - with
`--variable_eval_length` - clip by clip at each clip's own length, and with `--out` only the latest state dict is kept under
the reference's name `mn{width}_fsd50k_epoch_{e}_mAP_{round(mAP * 1000)}.pt`.  Without `--train` the program is the
reference's `evaluate()`: it scores `--eval_bank` and prints mAP / ROC.

Arguments and defaults are ex_fsd50k.py's (:245-289), minus wandb / --cuda / --num_workers / --pretrained (the download);
`--init_checkpoint` loads a local state dict instead (finetune.load_init_checkpoint).  Only --resample_rate 32000 is
supported (fsd50k.py).  Like ex_fsd50k.py, the DyMN temperature is not scheduled here.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

from .finetune_esc50 import _width, build          # the model and the mel front-end: ex_fsd50k.py:33-60 = ex_esc50.py:31-58
from .utils import exp_warmup_linear_down


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="FSD50K fine-tuning / evaluation on the HIP path (ex_fsd50k.py's arguments)")
    p.add_argument("--train_bank", default=None, help="decoded training split: waves.npy, lengths.npy, targets.npy, names.txt")
    p.add_argument("--valid_bank", default=None, help="decoded validation split (evaluated after every epoch of --train)")
    p.add_argument("--eval_bank", default=None, help="decoded evaluation split (scored without --train)")
    p.add_argument("--experiment_name", type=str, default="FSD50K")
    p.add_argument("--train", action="store_true", default=False)
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--variable_eval_length", action="store_true", default=False)
    p.add_argument("--model_name", type=str, default="mn10_as")
    p.add_argument("--pretrain_final_temp", type=float, default=1.0)
    p.add_argument("--model_width", type=float, default=1.0)
    p.add_argument("--head_type", type=str, default="mlp")
    p.add_argument("--se_dims", type=str, default="c")
    p.add_argument("--n_epochs", type=int, default=80)
    p.add_argument("--mixup_alpha", type=float, default=0.3)
    p.add_argument("--no_roll", action="store_true", default=False)
    p.add_argument("--no_wavmix", action="store_true", default=False)
    p.add_argument("--gain_augment", type=int, default=12)
    p.add_argument("--weight_decay", type=int, default=0.0)
    p.add_argument("--lr", type=float, default=7e-5)
    p.add_argument("--warm_up_len", type=int, default=10)
    p.add_argument("--ramp_down_start", type=int, default=10)
    p.add_argument("--ramp_down_len", type=int, default=65)
    p.add_argument("--last_lr_value", type=float, default=0.01)
    p.add_argument("--resample_rate", type=int, default=32000)
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
    # this package's additions
    p.add_argument("--clip_seconds", type=float, default=10.0, help="the reference's clip_length (10 s); shorter for tests")
    p.add_argument("--init_checkpoint", default=None, help="state dict to start from (AudioSet for --train, FSD50K to evaluate)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--no_graph", action="store_true", help="eager BCETrainer instead of the captured step")
    p.add_argument("--max_steps", type=int, default=0, help="stop after this many steps (benchmarks / tests); 0 = whole epochs")
    p.add_argument("--precision", default=None, help="model.train_precision (auto / fp32 / bf16)")
    p.add_argument("--out", default=None, help="directory for the latest state dict (the reference keeps only the latest)")
    p.add_argument("--eval_dump", default=None, help="directory: the last evaluation's logits.npy / targets.npy (bank order)")
    p.add_argument("--json", action="store_true", help="print one JSON line with the run's results at the end")
    args = p.parse_args(argv)
    if args.resample_rate != 32000:
        p.error("only --resample_rate 32000 is supported: the reference decimates after cropping 10 s of 32 kHz audio, "
                "which the resident bank does not reproduce")
    if args.train and not (args.train_bank and args.valid_bank):
        p.error("--train needs --train_bank and --valid_bank")
    if not args.train and not args.eval_bank:
        p.error("evaluation (no --train) needs --eval_bank")
    return args


def _dump(args, ev):
    if args.eval_dump:
        os.makedirs(args.eval_dump, exist_ok=True)
        np.save(os.path.join(args.eval_dump, "logits.npy"), ev["logits"].cpu().numpy())
        np.save(os.path.join(args.eval_dump, "targets.npy"), ev["targets"].cpu().numpy())


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("efficientat_amd.finetune_fsd50k needs a GPU: the package has no CPU path")
    from .finetune import BCETrainer, GraphedBCETrainer, evaluate_multilabel
    from .fsd50k import N_CLASSES, load_bank
    from .optim import FusedAdam

    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    L = int(round(args.clip_seconds * args.resample_rate))
    ev_kw = dict(clip_samples=L, variable_length=args.variable_eval_length, keep_outputs=bool(args.eval_dump))
    eval_mode = "variable length" if args.variable_eval_length else f"{args.clip_seconds:g} s"

    if not args.train:                                                        # ex_fsd50k.py:181-241
        bank = load_bank(args.eval_bank, device=dev)
        model, mel = build(args, dev, N_CLASSES)
        print(f"Running FSD50K evaluation for model '{args.model_name}' on device '{dev}' ({bank['lengths'].numel()} clips, "
              f"{eval_mode})", file=sys.stderr, flush=True)
        ev = evaluate_multilabel(model, mel, bank, args.batch_size, **ev_kw)
        print(f"Results on FSD50K evaluation split for loaded model: {args.model_name}")
        print("  mAP: {:.3f}".format(ev["mAP"]))
        print("  ROC: {:.3f}".format(ev["ROC"]))
        _dump(args, ev)
        if args.json:
            print(json.dumps({"what": "efficientat_amd.finetune_fsd50k", "mode": "evaluate", "model": args.model_name,
                              "eval": eval_mode, "mAP": ev["mAP"], "ROC": ev["ROC"], "val_loss": ev["val_loss"],
                              "n_clips": ev["n_clips"], "eval_clips_per_s": round(ev["clips_per_s"], 1)}), flush=True)
        return

    t_load = time.perf_counter()
    train = load_bank(args.train_bank, device=dev)
    valid = load_bank(args.valid_bank, device=dev)
    t_load = time.perf_counter() - t_load
    n_train = train["lengths"].numel()
    print(f"[finetune_fsd50k] {n_train} training / {valid['lengths'].numel()} validation clips "
          f"({train['waves'].numel() / args.resample_rate / 3600:.2f} h / {valid['waves'].numel() / args.resample_rate / 3600:.2f} h) "
          f"resident on {dev} ({t_load:.1f} s to load)", file=sys.stderr, flush=True)
    model, mel = build(args, dev, N_CLASSES)

    graphed = not args.no_graph
    lr = torch.tensor(args.lr, device=dev) if graphed else args.lr            # tensor lr: the schedule needs no re-capture
    opt = FusedAdam(model.parameters(), lr=lr, weight_decay=args.weight_decay, capturable=graphed)
    sched = torch.optim.lr_scheduler.LambdaLR(
        opt, exp_warmup_linear_down(args.warm_up_len, args.ramp_down_len, args.ramp_down_start, args.last_lr_value))
    model.train()
    mel.train()
    common = dict(clip_samples=L, mixup_alpha=args.mixup_alpha, gain_augment=args.gain_augment, roll=not args.no_roll,
                  wavmix=not args.no_wavmix)
    trainer = (GraphedBCETrainer(model, mel, opt, train, args.batch_size, **common) if graphed
               else BCETrainer(model, mel, opt, train, **common))

    steps_total, clips_total, t_train = 0, 0, 0.0
    name, ev, stats, done = None, None, {"train_loss": float("nan")}, False
    width = _width(args)
    for epoch in range(args.n_epochs):
        order = torch.randperm(n_train)                                       # DataLoader(shuffle=True), partial last batch
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
        dt = time.perf_counter() - t0
        t_train += dt
        steps_total += n_ep
        ev = evaluate_multilabel(model, mel, valid, args.batch_size, **ev_kw)
        print(f"[finetune_fsd50k] epoch {epoch + 1}/{args.n_epochs}: {n_ep} steps, train_loss {stats['train_loss']:.5f}, "
              f"mAP {ev['mAP']:.4f}, ROC {ev['ROC']:.4f}, val_loss {ev['val_loss']:.5f} ({eval_mode}), "
              f"lr {float(sched.get_last_lr()[0]):.2e}", file=sys.stderr, flush=True)
        if args.out:                                                          # ex_fsd50k.py:138-142: keep the latest only
            os.makedirs(args.out, exist_ok=True)
            if name is not None:
                os.remove(os.path.join(args.out, name))
            name = f"mn{str(width).replace('.', '')}_fsd50k_epoch_{epoch}_mAP_{int(round(ev['mAP'] * 1000))}.pt"
            torch.save(model.state_dict(), os.path.join(args.out, name))
        if done:
            break
    _dump(args, ev)
    if args.json:
        line = {"what": "efficientat_amd.finetune_fsd50k", "mode": "train", "model": args.model_name, "steps": steps_total,
                "epochs": epoch + 1, "batch_size": args.batch_size, "launch": "hipGraph replay" if graphed else "eager",
                "eval": eval_mode, "mAP": ev["mAP"], "ROC": ev["ROC"], "val_loss": ev["val_loss"],
                "train_loss": stats["train_loss"], "clips_per_s": round(clips_total / max(t_train, 1e-9), 1),
                "eval_clips_per_s": round(ev["clips_per_s"], 1), "checkpoint": name}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
