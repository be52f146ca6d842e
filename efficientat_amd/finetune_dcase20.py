"""Fine-tune an MN / DyMN on TAU Urban Acoustic Scenes 2020 Mobile (DCASE20 task 1A) on the HIP path: ex_dcase20.py's
training program with the data resident on the GPU.

    python -m efficientat_amd.finetune_dcase20 --train_bank DIR --test_bank DIR [--mixstyle_p 0.4] [--init_checkpoint mn10_as.pt]
                                               [--json] [...]

The two DIRs are decoded splits written by tools/dcase20_to_bank.py (dcase20.load_bank: waves.npy, labels.npy, names.txt,
classes.json).  Both are kept in HBM; each step is one hipGraph replay of wave augmentation -> mel -> frequency-wise MixStyle
or mix-up -> model -> cross-entropy -> backward -> FusedAdam (finetune.GraphedSceneCETrainer; `--no_graph`: the eager
SceneCETrainer).  After every epoch the test split is evaluated as the reference's `_test` (accuracy, val_loss = mean of
per-batch mean CE) plus the accuracy per recording device, and with `--out` only the latest state dict is kept under the
reference's name `mn{width}_dcase_epoch_{e}_acc_{round(acc * 1000)}.pt`.

Arguments and defaults are ex_dcase20.py's (:187-230), minus wandb / --cuda / --num_workers / --pretrained (the download) /
--cache_path (the banks are the cache); `--init_checkpoint` loads a local AudioSet state dict instead
(finetune.load_init_checkpoint).  Like ex_dcase20.py, the DyMN temperature is not scheduled here.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

from .finetune_esc50 import _quiet, _width, build  # noqa: F401  (the model / mel construction is ex_esc50.py's, line for line)
from .utils import exp_warmup_linear_down


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="DCASE20 fine-tuning on the HIP path (ex_dcase20.py's arguments)")
    p.add_argument("--train_bank", required=True, help="decoded training split (tools/dcase20_to_bank.py --split train)")
    p.add_argument("--test_bank", required=True, help="decoded test split (tools/dcase20_to_bank.py --split test)")
    p.add_argument("--experiment_name", type=str, default="DCASE20")
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--model_name", type=str, default="mn10_as")
    p.add_argument("--pretrain_final_temp", type=float, default=1.0)
    p.add_argument("--model_width", type=float, default=1.0)
    p.add_argument("--head_type", type=str, default="mlp")
    p.add_argument("--se_dims", type=str, default="c")
    p.add_argument("--n_epochs", type=int, default=80)
    p.add_argument("--mixup_alpha", type=float, default=0.3)
    p.add_argument("--mixstyle_p", type=float, default=0.0)
    p.add_argument("--mixstyle_alpha", type=float, default=0.4)
    p.add_argument("--no_roll", action="store_true", default=False)
    p.add_argument("--no_wavmix", action="store_true", default=False)
    p.add_argument("--gain_augment", type=int, default=12)
    p.add_argument("--weight_decay", type=int, default=0.0)
    p.add_argument("--lr", type=float, default=8e-4)
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
    p.add_argument("--no_graph", action="store_true", help="eager SceneCETrainer instead of the captured step")
    p.add_argument("--max_steps", type=int, default=0, help="stop after this many steps (benchmarks / tests); 0 = whole epochs")
    p.add_argument("--precision", default=None, help="model.train_precision (auto / fp32 / bf16)")
    p.add_argument("--out", default=None, help="directory for the latest state dict (the reference keeps only the latest)")
    p.add_argument("--eval_dump", default=None,
                   help="directory: the last evaluation's logits.npy / targets.npy / devices.npy (bank order)")
    p.add_argument("--json", action="store_true", help="print one JSON line with the run's results at the end")
    return p.parse_args(argv)


def main(argv=None):
    args = parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("efficientat_amd.finetune_dcase20 needs a GPU: the package has no CPU path")
    from .dcase20 import N_CLASSES, load_bank
    from .finetune import GraphedSceneCETrainer, SceneCETrainer, evaluate_accuracy
    from .optim import FusedAdam

    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    t_load = time.perf_counter()
    train = load_bank(args.train_bank, device=dev)
    test = load_bank(args.test_bank, device=dev)
    t_load = time.perf_counter() - t_load
    if train["bank"].shape[1] != test["bank"].shape[1]:
        raise SystemExit(f"the banks hold clips of {train['bank'].shape[1]} and {test['bank'].shape[1]} samples")
    devices = test["classes"]["device"]
    print(f"[finetune_dcase20] {train['bank'].shape[0]} training / {test['bank'].shape[0]} test clips of "
          f"{train['bank'].shape[1]} samples resident on {dev} ({t_load:.1f} s to load), test devices {devices}",
          file=sys.stderr, flush=True)
    model, mel = build(args, dev, N_CLASSES)

    graphed = not args.no_graph
    lr = torch.tensor(args.lr, device=dev) if graphed else args.lr            # tensor lr: the schedule needs no re-capture
    opt = FusedAdam(model.parameters(), lr=lr, weight_decay=args.weight_decay, capturable=graphed)
    sched = torch.optim.lr_scheduler.LambdaLR(
        opt, exp_warmup_linear_down(args.warm_up_len, args.ramp_down_len, args.ramp_down_start, args.last_lr_value))
    model.train()
    mel.train()
    common = dict(n_classes=N_CLASSES, mixup_alpha=args.mixup_alpha, mixstyle_p=args.mixstyle_p,
                  mixstyle_alpha=args.mixstyle_alpha, gain_augment=args.gain_augment, roll=not args.no_roll,
                  wavmix=not args.no_wavmix)
    bank = (train["bank"], train["bank_mean"], train["bank_cls"])
    trainer = (GraphedSceneCETrainer(model, mel, opt, *bank, args.batch_size, **common) if graphed
               else SceneCETrainer(model, mel, opt, *bank, **common))

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
                               keep_outputs=bool(args.eval_dump), groups=(test["bank_dev"], len(devices)))
        by_dev = dict(zip(devices, ev["accuracy_by_group"]))
        print(f"[finetune_dcase20] epoch {epoch + 1}/{args.n_epochs}: {n_ep} steps, train_loss {stats['train_loss']:.5f}, "
              f"accuracy {ev['accuracy']:.4f}, val_loss {ev['val_loss']:.5f}, lr {float(sched.get_last_lr()[0]):.2e}, "
              + " ".join(f"{k} {v:.3f}" for k, v in by_dev.items()), file=sys.stderr, flush=True)
        if args.out:                                                          # ex_dcase20.py:144-148: keep the latest only
            os.makedirs(args.out, exist_ok=True)
            if name is not None:
                os.remove(os.path.join(args.out, name))
            name = f"mn{str(width).replace('.', '')}_dcase_epoch_{epoch}_acc_{int(round(ev['accuracy'] * 1000))}.pt"
            torch.save(model.state_dict(), os.path.join(args.out, name))
        if done:
            break
    if args.eval_dump:
        os.makedirs(args.eval_dump, exist_ok=True)
        np.save(os.path.join(args.eval_dump, "logits.npy"), ev["logits"].cpu().numpy())
        np.save(os.path.join(args.eval_dump, "targets.npy"), ev["targets"].cpu().numpy())
        np.save(os.path.join(args.eval_dump, "devices.npy"), test["bank_dev"].cpu().numpy())
    if args.json:
        line = {"what": "efficientat_amd.finetune_dcase20", "model": args.model_name, "steps": steps_total,
                "epochs": epoch + 1, "batch_size": args.batch_size, "launch": "hipGraph replay" if graphed else "eager",
                "accuracy": ev["accuracy"], "accuracy_by_device": by_dev, "val_loss": ev["val_loss"],
                "train_loss": stats["train_loss"], "clips_per_s": round(clips_total / max(t_train, 1e-9), 1),
                "eval_clips_per_s": round(ev["clips_per_s"], 1), "checkpoint": name, "mixstyle_p": args.mixstyle_p}
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
