"""Fine-tune an MN / DyMN on ESC-50 on the HIP path: ex_esc50.py's training program with the data resident on the GPU.

    python -m efficientat_amd.finetune_esc50 --data DIR [--fold 1] [--init_checkpoint mn10_as.pt] [--json] [...]

DIR holds the official layout: meta/esc50.csv plus audio_32k/ (the reference's copy) or audio/ (the 44.1 kHz release,
resampled on load).  The training split (the other four folds) and the test fold are decoded once and kept in HBM
(esc50.load_split); each step is one hipGraph replay of wave augmentation -> mel -> mix-up -> model -> cross-entropy ->
backward -> FusedAdam (finetune.GraphedCETrainer; `--no_graph`: the eager CETrainer).  After every epoch the test fold is
evaluated as the reference's `_test` (accuracy, val_loss = mean of per-batch mean CE), and with `--out` only the latest
state dict is kept under the reference's name `mn{width}_esc50_epoch_{e}_acc_{round(acc * 1000)}.pt`.

Arguments and defaults are ex_esc50.py's (:183-229), minus wandb / --cuda / --num_workers / --pretrained (the download);
`--init_checkpoint` loads a local AudioSet state dict instead (finetune.load_init_checkpoint).  Like ex_esc50.py, the
DyMN temperature is not scheduled here: it stays at T_max (= --pretrain_final_temp with --init_checkpoint).
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

from .utils import NAME_TO_WIDTH, exp_warmup_linear_down


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="ESC-50 fine-tuning on the HIP path (ex_esc50.py's arguments)")
    p.add_argument("--data", required=True, help="ESC-50 directory: meta/esc50.csv + audio_32k/ or audio/")
    p.add_argument("--experiment_name", type=str, default="ESC50")
    p.add_argument("--batch_size", type=int, default=128)
    p.add_argument("--fold", type=int, default=1)
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
    p.add_argument("--lr", type=float, default=6e-5)
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
    p.add_argument("--init_checkpoint", default=None, help="AudioSet state dict to start from (e.g. written by train_dp --out)")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--no_graph", action="store_true", help="eager CETrainer instead of the captured step")
    p.add_argument("--max_steps", type=int, default=0, help="stop after this many steps (benchmarks / tests); 0 = whole epochs")
    p.add_argument("--precision", default=None, help="model.train_precision (auto / fp32 / bf16)")
    p.add_argument("--out", default=None, help="directory for the latest state dict (the reference keeps only the latest)")
    p.add_argument("--eval_dump", default=None, help="directory: the last evaluation's logits.npy / targets.npy (fold order)")
    p.add_argument("--json", action="store_true", help="print one JSON line with the run's results at the end")
    return p.parse_args(argv)


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _width(args):
    """ex_esc50.py:45-47: the width of --model_name when starting from pre-trained weights, else --model_width."""
    return NAME_TO_WIDTH(args.model_name) if args.init_checkpoint else args.model_width


def build(args, dev, n_classes):
    """The model of ex_esc50.py:43-58 (width --model_width; DyMN's T_max = --pretrain_final_temp when it starts from a
    checkpoint, as pretrained_name does in models/dymn/model.py) and the mel front-end of :31-41."""
    from .preprocess import AugmentMelSTFT
    width = _width(args)
    if args.model_name.startswith("dymn"):
        from .dymn import get_model
        kw = dict(T_max=args.pretrain_final_temp) if args.init_checkpoint else {}
        model = _quiet(get_model, width_mult=width, num_classes=n_classes, **kw)
    else:
        from .mn import get_model
        model = _quiet(get_model, width_mult=width, head_type=args.head_type, se_dims=args.se_dims, num_classes=n_classes)
    if args.init_checkpoint:
        from .finetune import load_init_checkpoint
        load_init_checkpoint(model, args.init_checkpoint)
    model.to(dev)
    if args.precision:
        model.train_precision = args.precision
    mel = _quiet(AugmentMelSTFT, n_mels=args.n_mels, sr=args.resample_rate, win_length=args.window_size,
                 hopsize=args.hop_size, n_fft=args.n_fft, freqm=args.freqm, timem=args.timem, fmin=args.fmin, fmax=args.fmax,
                 fmin_aug_range=args.fmin_aug_range, fmax_aug_range=args.fmax_aug_range).to(dev)
    return model, mel


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("efficientat_amd.finetune_esc50 needs a GPU: the package has no CPU path")
    from .esc50 import N_CLASSES, load_split
    from .finetune import CETrainer, GraphedCETrainer, evaluate_accuracy
    from .optim import FusedAdam

    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    t_load = time.perf_counter()
    train = load_split(args.data, args.fold, True, sr=args.resample_rate, device=dev)
    test = load_split(args.data, args.fold, False, sr=args.resample_rate, device=dev)
    t_load = time.perf_counter() - t_load
    print(f"[finetune_esc50] fold {args.fold}: {train['bank'].shape[0]} training / {test['bank'].shape[0]} test clips resident "
          f"on {dev} ({t_load:.1f} s to decode)", file=sys.stderr, flush=True)
    model, mel = build(args, dev, N_CLASSES)

    graphed = not args.no_graph
    lr = torch.tensor(args.lr, device=dev) if graphed else args.lr            # tensor lr: the schedule needs no re-capture
    opt = FusedAdam(model.parameters(), lr=lr, weight_decay=args.weight_decay, capturable=graphed)
    sched = torch.optim.lr_scheduler.LambdaLR(
        opt, exp_warmup_linear_down(args.warm_up_len, args.ramp_down_len, args.ramp_down_start, args.last_lr_value))
    model.train()
    mel.train()
    common = dict(n_classes=N_CLASSES, mixup_alpha=args.mixup_alpha, gain_augment=args.gain_augment, roll=not args.no_roll,
                  wavmix=not args.no_wavmix)
    bank = (train["bank"], train["bank_mean"], train["bank_cls"])
    trainer = (GraphedCETrainer(model, mel, opt, *bank, args.batch_size, **common) if graphed
               else CETrainer(model, mel, opt, *bank, **common))

    n_train = train["bank"].shape[0]
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
        ev = evaluate_accuracy(model, mel, test["bank"], test["bank_cls"], args.batch_size, N_CLASSES,
                               keep_outputs=bool(args.eval_dump))
        print(f"[finetune_esc50] epoch {epoch + 1}/{args.n_epochs}: {n_ep} steps, train_loss {stats['train_loss']:.5f}, "
              f"accuracy {ev['accuracy']:.4f}, val_loss {ev['val_loss']:.5f}, lr {float(sched.get_last_lr()[0]):.2e}",
              file=sys.stderr, flush=True)
        if args.out:                                                          # ex_esc50.py:128-132: keep the latest only
            os.makedirs(args.out, exist_ok=True)
            if name is not None:
                os.remove(os.path.join(args.out, name))
            name = f"mn{str(width).replace('.', '')}_esc50_epoch_{epoch}_acc_{int(round(ev['accuracy'] * 1000))}.pt"
            torch.save(model.state_dict(), os.path.join(args.out, name))
        if done:
            break
    if args.eval_dump:
        os.makedirs(args.eval_dump, exist_ok=True)
        np.save(os.path.join(args.eval_dump, "logits.npy"), ev["logits"].cpu().numpy())
        np.save(os.path.join(args.eval_dump, "targets.npy"), ev["targets"].cpu().numpy())
    if args.json:
        line = {"what": "efficientat_amd.finetune_esc50", "model": args.model_name, "fold": args.fold, "steps": steps_total,
                "epochs": epoch + 1, "batch_size": args.batch_size, "launch": "hipGraph replay" if graphed else "eager",
                "accuracy": ev["accuracy"], "val_loss": ev["val_loss"], "train_loss": stats["train_loss"],
                "clips_per_s": round(clips_total / max(t_train, 1e-9), 1), "eval_clips_per_s": round(ev["clips_per_s"], 1),
                "checkpoint": name}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
