"""Validation pass of the AudioSet training program: sharded eval forward, gather, mAP / ROC AUC on the device.

What it must equal: the reference's `_test` (ex_audioset.py:231-256) after every epoch (:203-216), and its multi-GPU form
(ex_pl_audioset.py:215-247: every rank evaluates a shard, the predictions are all_gathered, the metric runs over the whole
eval split).  The metric is efficientat_amd.metrics.ap_auc (HIP, no sklearn, no host copy of the logits).
"""
import time

import torch
import torch.distributed as dist
import torch.nn.functional as F

from .metrics import ap_auc


def _shard_len(n, rank, world):
    return (n - rank + world - 1) // world if rank < n else 0


def evaluate(model, mel, dataset, batch_size, rank, world, device, num_workers=0, keep_outputs=False):
    """Evaluate `model` on every clip of `dataset` ((wave, name, target) items) -> {"mAP", "ROC", "val_loss", "n_clips",
    "eval_s", "clips_per_s"} on every rank (plus "logits" / "targets" (N, C) device tensors in dataset order with
    keep_outputs=True).

    Rank r forwards clips r, r + world, ... in eval mode under no_grad; each rank fills a preallocated (ceil(N / world), C)
    buffer and the buffers are all_gathered (RCCL or gloo), then interleaved back into dataset order; the padding rows of
    the short shards are dropped, so every clip counts exactly once.  mAP / ROC are the plain means of the per-class AP /
    ROC AUC (the reference's `.mean()`: a class with one label value only makes ROC NaN).  val_loss is the BCE-with-logits
    mean over all clips and classes; the reference averages per-batch means (`losses.mean()`), which is the same number
    when every batch is full.

    Evaluation does not perturb training: the eval loader has its own torch.Generator, the host RNG draws of the mel
    front-end happen inside a forked torch RNG, np.random is not touched, and eval-mode BatchNorm leaves the running
    statistics alone.  Both modules get their previous train / eval mode back."""
    n = len(dataset)
    if n == 0:
        raise ValueError("evaluate: the dataset is empty")
    m = (n + world - 1) // world
    mine = list(range(rank, n, world))
    assert len(mine) == _shard_len(n, rank, world)
    was_training = (model.training, mel.training)
    model.eval()
    mel.eval()
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    try:
        with torch.random.fork_rng(devices=[]), torch.no_grad():
            dl = torch.utils.data.DataLoader(torch.utils.data.Subset(dataset, mine), batch_size=batch_size, shuffle=False,
                                             num_workers=num_workers, pin_memory=True, generator=torch.Generator())
            logits = targets = None
            row = 0
            for batch in dl:
                x, y = batch[0], batch[2]
                bs = x.shape[0]
                x = x.to(device, non_blocking=True).reshape(bs, -1)
                y_hat, _ = model(mel(x).unsqueeze(1))                     # _mel_forward + model (ex_audioset.py:246-247)
                if logits is None:
                    logits = torch.zeros((m, y_hat.shape[1]), device=device, dtype=torch.float32)
                    targets = torch.zeros((m, y.shape[1]), device=device, dtype=torch.float32)
                logits[row:row + bs].copy_(y_hat)
                targets[row:row + bs].copy_(y, non_blocking=True)
                row += bs
            if logits is None:                                            # (an empty shard: world > n; shapes from clip 0)
                c = int(torch.as_tensor(dataset[0][2]).numel())
                logits = torch.zeros((m, c), device=device)
                targets = torch.zeros((m, c), device=device)
            if world > 1:
                parts_l = [torch.empty_like(logits) for _ in range(world)]
                parts_t = [torch.empty_like(targets) for _ in range(world)]
                dist.all_gather(parts_l, logits)
                dist.all_gather(parts_t, targets)
                # rank r's row j is clip j * world + r: interleave, then drop the padding rows at the end
                logits = torch.stack(parts_l, 1).reshape(m * world, -1)[:n]
                targets = torch.stack(parts_t, 1).reshape(m * world, -1)[:n]
            else:
                logits, targets = logits[:n], targets[:n]
            ap, auc = ap_auc(logits, targets)
            val_loss = F.binary_cross_entropy_with_logits(logits, targets)
            res = torch.stack([ap.mean(), auc.mean(), val_loss.double()]).cpu().tolist()
    finally:
        model.train(was_training[0])
        mel.train(was_training[1])
    eval_s = time.perf_counter() - t0
    out = {"mAP": res[0], "ROC": res[1], "val_loss": res[2], "n_clips": n, "eval_s": eval_s,
           "clips_per_s": n / max(eval_s, 1e-9)}
    if keep_outputs:
        out["logits"], out["targets"] = logits, targets
    return out
