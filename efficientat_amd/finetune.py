"""Single-label fine-tuning (ex_esc50.py:95-178) as a device-resident engine: the clip bank lives in HBM, the augmentation and
the loss are HIP kernels, and a captured step is one hipGraph replay.

Per step the reference does: DataLoader workers decode, gain, pad, roll and wave-mix each clip on the host (datasets/esc50.py,
datasets/helpers/audiodatasets.py) -> blocking copy -> mel -> log-mel mix-up -> model -> two F.cross_entropy terms weighted by
the mix-up lambda -> a `.cpu()` read of the loss (a device sync) -> backward -> Adam.  Here:

  * the batch is built on the device from the resident bank by `eat_wave_augment` (ops.wave_augment) from host draws made in
    MixupDataset's order (esc50.draw_augment) - a few hundred bytes per step cross PCIe, no waveform does;
  * `eat_softmax_ce_fwd_bwd` computes the soft-target cross-entropy of the mixed targets and d loss / d logits in one pass;
    the loss is accumulated on the device and read once per epoch (`epoch_stats`);
  * evaluation (`evaluate_accuracy`) takes argmax and per-row loss from the same kernel.

Host RNG order of a step: the augmentation draws (torch, numpy), the mel's (fmin, fmax) draw, then `mixup` (torch.randperm,
numpy beta) - the reference's order within the main process, with the DataLoader's draws moved in front of the step.

Multi-label fine-tuning with partially observed labels (ex_openmic.py:96-206) has the same shape: `MaskedBCETrainer` /
`GraphedMaskedBCETrainer` build the batch with `eat_wave_augment` (waveforms) and `eat_openmic_targets` (label | mask rows,
openmic.draw_augment's order), the loss is `eat_masked_bce_fwd_bwd`, and `evaluate_masked` takes the probabilities from the
same kernel and the masked mAP / ROC from `metrics.ap_auc(..., sample_weight=mask)`.

Multi-label fine-tuning on clips of any length (ex_fsd50k.py:89-178): `BCETrainer` / `GraphedBCETrainer` build the batch and
its mixed soft labels from a ragged bank (fsd50k.load_bank) with `eat_wave_augment_ragged` (fsd50k.draw_augment's order: the
crop of a long clip is redrawn on every fetch), the loss is `eat_masked_bce_fwd_bwd` with soft labels and a mask of ones, and
`evaluate_multilabel` ranks the logits at a fixed length or at every clip's own.

Acoustic scene classification (ex_dcase20.py:91-183): `SceneCETrainer` / `GraphedSceneCETrainer` are the single-label
trainers with DCASE20's draw order (dcase20.draw_augment) and the reference's three-way branch on the log-mel: frequency-wise
MixStyle (`eat_freq_mixstyle`, ops.freq_mixstyle) when --mixstyle_p > 0, else the mix-up, else nothing.  In the captured
step the MixStyle coin of a step is a device flag, so applied and unapplied steps replay the same graph.
`evaluate_accuracy(..., groups=)` adds the per-recording-device accuracy.
"""
import time

import torch

from . import dcase20, fsd50k, metrics, openmic, ops
from .esc50 import draw_augment
from .graphs import HostRing
from .train_loop import FusedLoss, GraphedTrainer, Trainer


def ce_loss(logits, y, perm=None, lam=None, sums=None):
    """mean_b [lam CE(z, y) + (1 - lam) CE(z, y[perm])] (ex_esc50.py:102-118) as a device scalar that supports .backward();
    `sums` (1,) accumulates it across calls."""
    if sums is None:
        sums = torch.zeros(1, device=logits.device, dtype=torch.float64)
    y = y.contiguous().float()
    # (row_loss lets the kernel's second launch read the row losses instead of recomputing every row in one block)
    return FusedLoss.apply(logits, sums, 1, lambda z, step: ops.softmax_ce_fwd_bwd(
        z, y, perm, lam, sums=step, row_loss=torch.empty(z.shape[0], device=z.device, dtype=torch.float32)))


class CETrainer(Trainer):
    """step(batch) = one iteration of ex_esc50.py's training loop (:95-121) on the bank rows `batch` (host indices).

    bank (N, L) fp32, bank_mean (N) fp64, bank_cls (N) int32: the resident training split (esc50.load_split); model / mel:
    the HIP-backed modules; optimizer: e.g. optim.FusedAdam.  gain_augment / roll / wavmix: ex_esc50.py's --gain_augment,
    not --no_roll, not --no_wavmix."""

    STATS = ("train_loss",)

    def __init__(self, model, mel, optimizer, bank, bank_mean, bank_cls, n_classes=50, mixup_alpha=0.3, gain_augment=12,
                 roll=True, wavmix=True):
        self.model, self.mel, self.opt = model, mel, optimizer
        self.bank, self.bank_mean, self.bank_cls = bank, bank_mean, bank_cls.to(torch.int32).contiguous()
        if bank.dim() != 2 or bank_mean.numel() != bank.shape[0] or self.bank_cls.numel() != bank.shape[0]:
            raise ValueError("CETrainer: bank (N, L), bank_mean (N) and bank_cls (N) do not match")
        self.n_classes, self.mixup_alpha = int(n_classes), mixup_alpha
        self.gain_augment, self.roll, self.wavmix = int(gain_augment), bool(roll), bool(wavmix)
        dev = next(model.parameters()).device
        self.sums = torch.zeros(1, device=dev, dtype=torch.float64)
        self.steps = 0

    def draw(self, batch):
        idx, shift, amp, mix = draw_augment(batch, self.bank.shape[0], self.gain_augment, self.roll, self.wavmix)
        ops.check_augment_draws(idx, shift, self.bank.shape[0], self.bank.shape[1])
        return idx, shift, amp, mix

    def loss_and_backward(self, batch):
        """augment -> mel -> log-mel mix-up -> model -> CE -> backward; leaves the gradients in `.grad`."""
        draws = self.draw(batch)
        x, y = ops.wave_augment(self.bank, self.bank_mean, self.bank_cls, *draws, self.n_classes)
        spec = self.mel(x).unsqueeze(1)                                       # _mel_forward, ex_esc50.py:143-148
        spec, perm, lam = self._mixup(spec)                                   # host draws, reference order
        y_hat, _ = self.model(spec)
        loss = ce_loss(y_hat, y, perm, lam, self.sums)
        loss.backward()
        return loss.detach()


class GraphedCETrainer(GraphedTrainer, CETrainer):
    """`CETrainer` with the whole iteration - wave augmentation, log-mel, mix-up, forward, CE, backward, optimizer - captured
    ONCE into a hipGraph and replayed with one host call per step.  What changes per step enters through static buffers:

        idx / shift (2B) int32, amp (2B), mix (B)   the augmentation draws (validated on the host before staging);
        perm (B) int32, lam (B)                     the log-mel mix-up draw;
        the mel basis                               band table of the step's (fmin, fmax) jitter (`AugmentMelSTFT.static_tables`).

    Host RNG order as `CETrainer.step`.  SpecAugment masks (freqm / timem != 0) are launch arguments of the mel kernel: the
    augmentation and the mel then run eagerly in front of the graph.  The optimizer must be capturable (FusedAdam(...,
    capturable=True) with a tensor lr, so that a scheduler needs no re-capture).  DyMN: call `recapture()` after
    `model.update_params(epoch)` (the temperatures are launch constants).  A batch of another size (the last, partial batch
    of an epoch) takes the eager step."""

    def __init__(self, model, mel, optimizer, bank, bank_mean, bank_cls, batch_size, n_classes=50, mixup_alpha=0.3,
                 gain_augment=12, roll=True, wavmix=True, warmup=2):
        CETrainer.__init__(self, model, mel, optimizer, bank, bank_mean, bank_cls, n_classes, mixup_alpha, gain_augment, roll,
                           wavmix)
        dev, B = bank.device, int(batch_size)
        first = torch.full((2 * B,), -1, device=dev, dtype=torch.int32)
        first[0::2] = 0                                                       # (bank row 0, no wave-mix: the warm-up batch)
        self._idx = HostRing(first)
        self._shift = HostRing(torch.zeros(2 * B, device=dev, dtype=torch.int32))
        self._amp = HostRing(torch.ones(2 * B, device=dev))
        self._mix = HostRing(torch.ones(B, device=dev))
        self._setup_graph(B, bank.shape[1], self.n_classes, warmup)

    def _front(self, fmask=(0, 0), tmask=(0, 0)):
        ops.wave_augment(self.bank, self.bank_mean, self.bank_cls, self._idx.dev, self._shift.dev, self._amp.dev, self._mix.dev,
                         self.n_classes, out=self.wave, y=self.y)
        super()._front(fmask, tmask)

    def _graph_loss(self, y_hat, perm, lam):
        return ce_loss(y_hat, self.y, perm, lam, self.sums)

    def _fits(self, batch):
        return len(batch) == self.B

    def _stage(self, batch):
        idx, shift, amp, mix = self.draw(batch)          # host draws, reference order: augmentation, then the mel's, mix-up
        self._idx.put(idx)
        self._shift.put(shift)
        self._amp.put(amp)
        self._mix.put(mix)


class SceneCETrainer(CETrainer):
    """step(batch) = one iteration of ex_dcase20.py's training loop (:98-131) on the bank rows `batch` (host indices).

    The arguments of `CETrainer` on a bank of dcase20.load_bank, plus mixstyle_p / mixstyle_alpha = --mixstyle_p /
    --mixstyle_alpha.  The reference's branch (:104-120): with mixstyle_p > 0 the log-mel goes through frequency-wise MixStyle
    and the loss is the plain soft-target cross-entropy - NO mix-up and none of its draws, also on a step whose coin says
    "not applied" (`mixup_alpha` then reads 0 on the trainer); otherwise the mix-up when mixup_alpha is non-zero; otherwise
    neither.  Host RNG order of a step: the augmentation draws in DCASE20's order (dcase20.draw_augment), the mel's draw,
    then dcase20.draw_mixstyle or `mixup`."""

    def __init__(self, model, mel, optimizer, bank, bank_mean, bank_cls, n_classes=10, mixup_alpha=0.3, mixstyle_p=0.0,
                 mixstyle_alpha=0.4, gain_augment=12, roll=True, wavmix=True):
        self.mixstyle_p, self.mixstyle_alpha = float(mixstyle_p), float(mixstyle_alpha)
        CETrainer.__init__(self, model, mel, optimizer, bank, bank_mean, bank_cls, n_classes,
                           0.0 if self.mixstyle_p > 0 else mixup_alpha, gain_augment, roll, wavmix)

    def draw(self, batch):
        idx, shift, amp, mix = dcase20.draw_augment(batch, self.bank.shape[0], self.gain_augment, self.roll, self.wavmix)
        ops.check_augment_draws(idx, shift, self.bank.shape[0], self.bank.shape[1])
        return idx, shift, amp, mix

    def loss_and_backward(self, batch):
        """augment -> mel -> MixStyle or mix-up -> model -> CE -> backward; leaves the gradients in `.grad`."""
        draws = self.draw(batch)
        x, y = ops.wave_augment(self.bank, self.bank_mean, self.bank_cls, *draws, self.n_classes)
        spec = self.mel(x).unsqueeze(1)                                       # _mel_forward, ex_dcase20.py:151-156
        perm = lam = None
        if self.mixstyle_p > 0:
            on, ms_perm, ms_lam = dcase20.draw_mixstyle(spec.shape[0], self.mixstyle_p, self.mixstyle_alpha)
            if on:
                spec = ops.freq_mixstyle(spec, ms_perm, ms_lam)
        else:
            spec, perm, lam = self._mixup(spec)                               # host draws, reference order
        y_hat, _ = self.model(spec)
        loss = ce_loss(y_hat, y, perm, lam, self.sums)
        loss.backward()
        return loss.detach()


class GraphedSceneCETrainer(GraphedCETrainer, SceneCETrainer):
    """`SceneCETrainer` as `GraphedCETrainer`'s captured step.  With mixstyle_p > 0 MixStyle runs inside the graph on static
    buffers of its own: rings for perm (B) int32 and lam (B), a one-element int32 ring for the step's coin (`apply`: read by the
    kernel, 0 = the spec passes through bit for bit), the (B, n_mels, 2) statistics workspace and the output spec.  Applied
    and unapplied steps replay the same graph: nothing is captured again.  Everything said on `GraphedCETrainer` about the
    optimizer, SpecAugment masks, DyMN `recapture()` and partial batches holds here."""

    def __init__(self, model, mel, optimizer, bank, bank_mean, bank_cls, batch_size, n_classes=10, mixup_alpha=0.3,
                 mixstyle_p=0.0, mixstyle_alpha=0.4, gain_augment=12, roll=True, wavmix=True, warmup=2):
        self.mixstyle_p, self.mixstyle_alpha = float(mixstyle_p), float(mixstyle_alpha)
        if self.mixstyle_p > 0:
            dev, B = bank.device, int(batch_size)
            self._ms_perm = HostRing(torch.arange(B, device=dev, dtype=torch.int32))
            self._ms_lam = HostRing(torch.ones(B, device=dev))
            self._ms_apply = HostRing(torch.ones(1, device=dev, dtype=torch.int32))    # (the warm-up batch: applied)
            self._ms_stats = torch.zeros((B, mel.n_mels, 2), device=dev)
            self._ms_out = None                                               # (shaped like the spec: made by the first issue)
        GraphedCETrainer.__init__(self, model, mel, optimizer, bank, bank_mean, bank_cls, batch_size, n_classes,
                                  0.0 if self.mixstyle_p > 0 else mixup_alpha, gain_augment, roll, wavmix, warmup)

    def _stage_mix(self):
        if self.mixstyle_p <= 0:
            return super()._stage_mix()
        on, perm, lam = dcase20.draw_mixstyle(self.B, self.mixstyle_p, self.mixstyle_alpha)
        self._ms_apply.put(torch.tensor([int(on)], dtype=torch.int32))
        if on:
            ops.check_mixstyle_perm(perm, self.B)                             # validated before it is staged
            self._ms_perm.put(perm.to(torch.int32))
            self._ms_lam.put(lam)

    def _mix_spec(self, spec):
        if self.mixstyle_p <= 0:
            return super()._mix_spec(spec)
        if self._ms_out is None:
            self._ms_out = torch.empty_like(spec)
        ops.freq_mixstyle(spec, self._ms_perm.dev, self._ms_lam.dev, apply=self._ms_apply.dev, out=self._ms_out,
                          stats=self._ms_stats)
        return self._ms_out, None, None


def evaluate_accuracy(model, mel, bank, bank_cls, batch_size, n_classes=None, keep_outputs=False, groups=None):
    """The reference's `_test` (ex_esc50.py:154-178) on a resident split -> {"accuracy", "val_loss", "n_clips", "eval_s",
    "clips_per_s"} (+ "logits" / "targets" (N, C) device tensors with keep_outputs=True).

    accuracy: argmax(logits) == class over every clip; val_loss: the MEAN OF THE PER-BATCH MEAN cross-entropies at
    `batch_size` (the reference's `losses.mean()`; the last batch of a fold may be short, so this is not the clip mean).
    Both come from `eat_softmax_ce_fwd_bwd` (row argmax, per-batch sums); one host sync at the end.  Runs in eval mode under
    no_grad inside a forked torch RNG (the mel draws its jitter even in eval); both modules get their previous mode back.
    groups = (g, n_groups), g an (N) integer tensor with values in [0, n_groups) (e.g. DCASE20's recording device of every
    clip): the result also holds "accuracy_by_group", a list of n_groups accuracies (NaN for a group without clips), counted
    on the device and read in the same single host sync.  Nothing else changes."""
    n = bank.shape[0]
    if n == 0:
        raise ValueError("evaluate_accuracy: the split is empty")
    dev = bank.device
    cls = bank_cls.to(device=dev, dtype=torch.int64)
    if groups is not None:
        g, n_groups = groups
        n_groups = int(n_groups)
        if g.numel() != n or n_groups < 1 or g.is_floating_point():
            raise ValueError(f"evaluate_accuracy: groups must be ({n} integers, a group count >= 1)")
        if not g.is_cuda and bool(((g < 0) | (g >= n_groups)).any()):
            raise ValueError(f"evaluate_accuracy: a group lies outside [0, {n_groups})")
        g = g.reshape(-1).to(device=dev, dtype=torch.int64)
    n_batches = (n + batch_size - 1) // batch_size
    was_training = (model.training, mel.training)
    model.eval()
    mel.eval()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    try:
        with torch.random.fork_rng(devices=[]), torch.no_grad():
            amax = torch.empty(n, device=dev, dtype=torch.int32)
            rloss = torch.empty(n, device=dev, dtype=torch.float32)
            bsum = torch.zeros(n_batches, device=dev, dtype=torch.float32)
            logits = targets = None
            for k in range(n_batches):
                s, e = k * batch_size, min(n, (k + 1) * batch_size)
                y_hat, _ = model(mel(bank[s:e]).unsqueeze(1))                 # _mel_forward + model (ex_esc50.py:163-165)
                y_hat = y_hat.reshape(e - s, -1).float().contiguous()
                C = y_hat.shape[1]
                y = torch.nn.functional.one_hot(cls[s:e], n_classes or C).float()
                ops.softmax_ce_fwd_bwd(y_hat, y, sums=bsum[k:k + 1], grad=False, row_loss=rloss[s:e], row_argmax=amax[s:e])
                if keep_outputs:
                    if logits is None:
                        logits = torch.empty((n, C), device=dev)
                        targets = torch.empty((n, y.shape[1]), device=dev)
                    logits[s:e].copy_(y_hat)
                    targets[s:e].copy_(y)
            hit = (amax.long() == cls).double()
            res = torch.stack([hit.mean(), bsum.double().mean()])
            if groups is not None:                                            # (sums of 0 / 1 in fp64: exact in any order)
                hits = torch.zeros(n_groups, device=dev, dtype=torch.float64).index_add_(0, g, hit)
                count = torch.zeros(n_groups, device=dev, dtype=torch.float64).index_add_(0, g, torch.ones_like(hit))
                res = torch.cat([res, hits / count])
            res = res.cpu().tolist()
    finally:
        model.train(was_training[0])
        mel.train(was_training[1])
    eval_s = time.perf_counter() - t0
    out = {"accuracy": res[0], "val_loss": res[1], "n_clips": n, "eval_s": eval_s, "clips_per_s": n / max(eval_s, 1e-9)}
    if groups is not None:
        out["accuracy_by_group"] = res[2:]
    if keep_outputs:
        out["logits"], out["targets"] = logits, targets
    return out


def masked_bce_loss(logits, yy, perm=None, lam=None, sums=None, binarize=True):
    """mean_bc mask * BCE-with-logits(z, lam y + (1 - lam) y[perm]), y = labels > 0.5 (ex_openmic.py:102-121) as a device
    scalar that supports .backward(); yy (B, 2C) = [labels | mask]; `sums` (1,) accumulates it across calls.
    binarize=False: y = the labels as they are (the soft labels of ex_fsd50k.py:102-115)."""
    if sums is None:
        sums = torch.zeros(1, device=logits.device, dtype=torch.float64)
    yy = yy.contiguous().float()
    return FusedLoss.apply(logits, sums, 1, lambda z, step: ops.masked_bce_fwd_bwd(
        z, yy, perm, lam, sums=step, row_loss=torch.empty(z.shape[0], device=z.device, dtype=torch.float32),
        binarize=binarize))


class MaskedBCETrainer(Trainer):
    """step(batch) = one iteration of ex_openmic.py's training loop (:96-129) on the bank rows `batch` (host indices).

    bank (N, L) fp32, bank_mean (N) fp64, bank_y (N, 2C) fp32 = [labels | mask]: the resident training split
    (openmic.load_bank); the other arguments as `CETrainer`."""

    STATS = ("train_loss",)

    def __init__(self, model, mel, optimizer, bank, bank_mean, bank_y, mixup_alpha=0.3, gain_augment=12, roll=True,
                 wavmix=True):
        self.model, self.mel, self.opt = model, mel, optimizer
        self.bank, self.bank_mean, self.bank_y = bank, bank_mean, bank_y.float().contiguous()
        if (bank.dim() != 2 or bank_mean.numel() != bank.shape[0] or self.bank_y.dim() != 2
                or self.bank_y.shape[0] != bank.shape[0] or self.bank_y.shape[1] % 2):
            raise ValueError("MaskedBCETrainer: bank (N, L), bank_mean (N) and bank_y (N, 2C) do not match")
        self.mixup_alpha = mixup_alpha
        self.gain_augment, self.roll, self.wavmix = int(gain_augment), bool(roll), bool(wavmix)
        dev = next(model.parameters()).device
        self.sums = torch.zeros(1, device=dev, dtype=torch.float64)
        self.steps = 0

    def draw(self, batch):
        idx, shift, amp, mix = openmic.draw_augment(batch, self.bank.shape[0], self.gain_augment, self.roll, self.wavmix)
        ops.check_augment_draws(idx, shift, self.bank.shape[0], self.bank.shape[1])
        return idx, shift, amp, mix

    def loss_and_backward(self, batch):
        """augment -> mel -> log-mel mix-up -> model -> masked BCE -> backward; leaves the gradients in `.grad`."""
        dev = self.bank.device
        idx, shift, amp, mix = (t.to(dev, non_blocking=True) for t in self.draw(batch))    # validated: uploaded once for both
        x, _ = ops.wave_augment(self.bank, self.bank_mean, None, idx, shift, amp, mix, 0)
        yy = ops.openmic_targets(self.bank_y, idx, mix)
        spec = self.mel(x).unsqueeze(1)                                       # _mel_forward, ex_openmic.py:152-157
        spec, perm, lam = self._mixup(spec)                                   # host draws, reference order
        y_hat, _ = self.model(spec)
        loss = masked_bce_loss(y_hat, yy, perm, lam, self.sums)
        loss.backward()
        return loss.detach()


class GraphedMaskedBCETrainer(GraphedTrainer, MaskedBCETrainer):
    """`MaskedBCETrainer` with the whole iteration captured once and replayed, on `GraphedCETrainer`'s static-buffer scheme
    (the same rings for idx / shift / amp / mix, perm / lam and the mel basis); `self.y` holds the (B, 2C) label | mask rows
    that `eat_openmic_targets` writes inside the graph.  Everything said there about the optimizer, SpecAugment masks, DyMN
    and partial batches holds here."""

    def __init__(self, model, mel, optimizer, bank, bank_mean, bank_y, batch_size, mixup_alpha=0.3, gain_augment=12,
                 roll=True, wavmix=True, warmup=2):
        MaskedBCETrainer.__init__(self, model, mel, optimizer, bank, bank_mean, bank_y, mixup_alpha, gain_augment, roll, wavmix)
        dev, B = bank.device, int(batch_size)
        first = torch.full((2 * B,), -1, device=dev, dtype=torch.int32)
        first[0::2] = 0                                                       # (bank row 0, no wave-mix: the warm-up batch)
        self._idx = HostRing(first)
        self._shift = HostRing(torch.zeros(2 * B, device=dev, dtype=torch.int32))
        self._amp = HostRing(torch.ones(2 * B, device=dev))
        self._mix = HostRing(torch.ones(B, device=dev))
        self._setup_graph(B, bank.shape[1], self.bank_y.shape[1], warmup)     # (y is as wide as a packed row: 2C)

    def _front(self, fmask=(0, 0), tmask=(0, 0)):
        ops.wave_augment(self.bank, self.bank_mean, None, self._idx.dev, self._shift.dev, self._amp.dev, self._mix.dev, 0,
                         out=self.wave)
        ops.openmic_targets(self.bank_y, self._idx.dev, self._mix.dev, out=self.y)
        super()._front(fmask, tmask)

    def _graph_loss(self, y_hat, perm, lam):
        return masked_bce_loss(y_hat, self.y, perm, lam, self.sums)

    def _fits(self, batch):
        return len(batch) == self.B

    def _stage(self, batch):
        idx, shift, amp, mix = self.draw(batch)          # host draws, reference order: augmentation, then the mel's, mix-up
        self._idx.put(idx)
        self._shift.put(shift)
        self._amp.put(amp)
        self._mix.put(mix)


def evaluate_masked(model, mel, bank, bank_y, batch_size, keep_outputs=False):
    """The reference's `_test` (ex_openmic.py:160-206) on a resident split -> {"mAP", "ROC", "val_loss", "n_clips", "eval_s",
    "clips_per_s"} (+ "probs" (N, C) and "targets" (N, 2C) = [labels > 0.5 | mask] device tensors with keep_outputs=True).

    val_loss: the MEAN OF THE PER-BATCH MEAN masked losses at `batch_size` (the reference's `losses.mean()`; the last batch
    may be short).  `eat_masked_bce_fwd_bwd` writes sigmoid(logits) of every batch into its rows of one (N, C) matrix; mAP /
    ROC are the plain means over the classes of `metrics.ap_auc(probs, labels > 0.5, sample_weight=mask)`, so a class
    without weighted positives and negatives makes ROC NaN, and input sklearn refuses with a ValueError (a non-finite
    probability, a mask entry other than 0 / 1) makes both NaN - the reference's `except ValueError`.  The host waits once, at
    the end (the metrics' status word, then the three results).  Mode restore and forked RNG as `evaluate_accuracy`."""
    n = bank.shape[0]
    if n == 0:
        raise ValueError("evaluate_masked: the split is empty")
    dev = bank.device
    yy = bank_y.to(device=dev, dtype=torch.float32).contiguous()
    C = yy.shape[1] // 2
    n_batches = (n + batch_size - 1) // batch_size
    was_training = (model.training, mel.training)
    model.eval()
    mel.eval()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    try:
        with torch.random.fork_rng(devices=[]), torch.no_grad():
            probs = torch.empty((n, C), device=dev, dtype=torch.float32)
            bsum = torch.zeros(n_batches, device=dev, dtype=torch.float32)
            for k in range(n_batches):
                s, e = k * batch_size, min(n, (k + 1) * batch_size)
                y_hat, _ = model(mel(bank[s:e]).unsqueeze(1))                 # _mel_forward + model (ex_openmic.py:177-179)
                y_hat = y_hat.reshape(e - s, -1).float().contiguous()
                ops.masked_bce_fwd_bwd(y_hat, yy[s:e], sums=bsum[k:k + 1], grad=False, probs=probs[s:e])
            labels, mask = (yy[:, :C] > 0.5).float(), yy[:, C:]
            nan = torch.full((), float("nan"), device=dev, dtype=torch.float64)
            try:
                ap, auc = metrics.ap_auc(probs, labels, sample_weight=mask)
                m_ap, m_auc = ap.mean(), auc.mean()
            except ValueError:
                m_ap = m_auc = nan
            res = torch.stack([m_ap, m_auc, bsum.double().mean()]).cpu().tolist()
    finally:
        model.train(was_training[0])
        mel.train(was_training[1])
    eval_s = time.perf_counter() - t0
    out = {"mAP": res[0], "ROC": res[1], "val_loss": res[2], "n_clips": n, "eval_s": eval_s,
           "clips_per_s": n / max(eval_s, 1e-9)}
    if keep_outputs:
        out["probs"], out["targets"] = probs, torch.cat([labels, mask], 1)
    return out


class BCETrainer(Trainer):
    """step(batch) = one iteration of ex_fsd50k.py's training loop (:96-123) on the bank clips `batch` (host indices).

    bank: the resident training split, the dict of `fsd50k.load_bank` (ragged: waves, offsets, lengths, clip_sum, bank_y,
    lengths_cpu); clip_samples: the length every clip is padded or cropped to (10 s); the other arguments as `CETrainer`."""

    STATS = ("train_loss",)

    def __init__(self, model, mel, optimizer, bank, clip_samples=320000, mixup_alpha=0.3, gain_augment=12, roll=True,
                 wavmix=True):
        self.model, self.mel, self.opt = model, mel, optimizer
        self.bank, self.L = bank, int(clip_samples)
        n = bank["lengths"].numel()
        if (bank["waves"].dim() != 1 or bank["offsets"].numel() != n or bank["clip_sum"].numel() != n
                or bank["bank_y"].dim() != 2 or bank["bank_y"].shape[0] != n or len(bank["lengths_cpu"]) != n or self.L < 1):
            raise ValueError("BCETrainer: waves (S), offsets / lengths / clip_sum (N), bank_y (N, C) and lengths_cpu (N) do not match")
        self.mixup_alpha = mixup_alpha
        self.gain_augment, self.roll, self.wavmix = int(gain_augment), bool(roll), bool(wavmix)
        dev = next(model.parameters()).device
        self.sums = torch.zeros(1, device=dev, dtype=torch.float64)
        self.steps = 0

    def draw(self, batch):
        idx, start, shift, amp, mix = fsd50k.draw_augment(batch, self.bank["lengths_cpu"], self.L, self.gain_augment, self.roll,
                                                          self.wavmix)
        ops.check_ragged_draws(idx, start, shift, self.bank["lengths_cpu"], self.L)
        return idx, start, shift, amp, mix

    def loss_and_backward(self, batch):
        """crop / pad + augment + labels -> mel -> log-mel mix-up -> model -> BCE -> backward; leaves the gradients in `.grad`."""
        x, yy = ops.wave_augment_ragged(self.bank, *self.draw(batch), self.L)
        spec = self.mel(x).unsqueeze(1)                                       # _mel_forward, ex_fsd50k.py:145-150
        spec, perm, lam = self._mixup(spec)                                   # host draws, reference order
        y_hat, _ = self.model(spec)
        loss = masked_bce_loss(y_hat, yy, perm, lam, self.sums, binarize=False)
        loss.backward()
        return loss.detach()


class GraphedBCETrainer(GraphedTrainer, BCETrainer):
    """`BCETrainer` with the whole iteration captured once and replayed, on `GraphedCETrainer`'s static-buffer scheme: rings
    for idx / start / shift / amp / mix, perm / lam and the mel basis; `eat_wave_augment_ragged` runs inside the graph and
    writes `self.wave` and the (B, 2C) label | ones rows `self.y`, with its window-mean workspace as one more static buffer.
    Everything said there about the optimizer, SpecAugment masks, DyMN and partial batches holds here."""

    def __init__(self, model, mel, optimizer, bank, batch_size, clip_samples=320000, mixup_alpha=0.3, gain_augment=12,
                 roll=True, wavmix=True, warmup=2):
        BCETrainer.__init__(self, model, mel, optimizer, bank, clip_samples, mixup_alpha, gain_augment, roll, wavmix)
        dev, B = bank["waves"].device, int(batch_size)
        first = torch.full((2 * B,), -1, device=dev, dtype=torch.int32)
        first[0::2] = 0                                                       # (clip 0 from its start, no wave-mix: the warm-up batch)
        self._idx = HostRing(first)
        self._start = HostRing(torch.zeros(2 * B, device=dev, dtype=torch.int32))
        self._shift = HostRing(torch.zeros(2 * B, device=dev, dtype=torch.int32))
        self._amp = HostRing(torch.ones(2 * B, device=dev))
        self._mix = HostRing(torch.ones(B, device=dev))
        self._win_mean = torch.zeros(2 * B, device=dev, dtype=torch.float64)
        self._setup_graph(B, self.L, 2 * bank["bank_y"].shape[1], warmup)     # (y is as wide as a packed row: 2C)

    def _front(self, fmask=(0, 0), tmask=(0, 0)):
        ops.wave_augment_ragged(self.bank, self._idx.dev, self._start.dev, self._shift.dev, self._amp.dev, self._mix.dev, self.L,
                                out=self.wave, yy=self.y, win_mean=self._win_mean)
        super()._front(fmask, tmask)

    def _graph_loss(self, y_hat, perm, lam):
        return masked_bce_loss(y_hat, self.y, perm, lam, self.sums, binarize=False)

    def _fits(self, batch):
        return len(batch) == self.B

    def _stage(self, batch):
        idx, start, shift, amp, mix = self.draw(batch)   # host draws, reference order: augmentation, then the mel's, mix-up
        self._idx.put(idx)
        self._start.put(start)
        self._shift.put(shift)
        self._amp.put(amp)
        self._mix.put(mix)


def evaluate_multilabel(model, mel, bank, batch_size, clip_samples=320000, variable_length=False, keep_outputs=False):
    """The reference's `_test` (ex_fsd50k.py:153-178) on a resident ragged split -> {"mAP", "ROC", "val_loss", "n_clips",
    "eval_s", "clips_per_s"} (+ "logits" (N, C) and "targets" (N, C) device tensors with keep_outputs=True).

    Fixed length (the default): batches of `batch_size` clips padded or cropped to `clip_samples` by `eat_wave_augment_ragged`
    (gain 1, no roll, no wave-mix).  The reference crops a long clip at random in evaluation too; those offsets are
    `fsd50k.draw_eval_crops`, drawn first inside the forked RNG.  val_loss: the MEAN OF THE PER-BATCH MEAN losses (the
    reference's `losses.mean()`; the last batch may be short).
    variable_length (--variable_eval_length): every clip at its own length, one by one (the reference's batch size 1), as a
    view of the flat buffer - nothing is copied; val_loss is then the mean over the clips.
    mAP / ROC: the plain means over the classes of `metrics.ap_auc` on the LOGITS, as `_test` hands y_hat to sklearn (sigmoid
    values would tie where fp32 saturates).  A class with one label value only makes ROC NaN where the reference's
    roc_auc_score raises ValueError; non-finite logits make both NaN.  One host wait at the end.  Mode restore and forked RNG
    as `evaluate_accuracy`."""
    n = bank["lengths"].numel()
    if n == 0:
        raise ValueError("evaluate_multilabel: the split is empty")
    dev = bank["waves"].device
    L = int(clip_samples)
    y = bank["bank_y"].to(device=dev, dtype=torch.float32).contiguous()
    C = y.shape[1]
    yy = torch.cat([y, torch.ones_like(y)], 1)                                # packed rows: a mask of ones
    lengths, offsets = bank["lengths_cpu"].tolist(), bank["offsets"].cpu().tolist()
    n_batches = n if variable_length else (n + batch_size - 1) // batch_size
    was_training = (model.training, mel.training)
    model.eval()
    mel.eval()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    try:
        with torch.random.fork_rng(devices=[]), torch.no_grad():
            logits = torch.empty((n, C), device=dev, dtype=torch.float32)
            bsum = torch.zeros(n_batches, device=dev, dtype=torch.float32)
            if variable_length:
                for k in range(n):
                    x = bank["waves"][offsets[k]:offsets[k] + lengths[k]].unsqueeze(0)
                    y_hat, _ = model(mel(x).unsqueeze(1))                     # _mel_forward + model (ex_fsd50k.py:167-168)
                    logits[k:k + 1].copy_(y_hat.reshape(1, -1).float())
                    ops.masked_bce_fwd_bwd(logits[k:k + 1], yy[k:k + 1], sums=bsum[k:k + 1], grad=False, binarize=False)
            else:
                crops = fsd50k.draw_eval_crops(bank["lengths_cpu"], L)
                for k in range(n_batches):
                    s, e = k * batch_size, min(n, (k + 1) * batch_size)
                    idx = torch.full((2 * (e - s),), -1, dtype=torch.int32)
                    idx[0::2] = torch.arange(s, e, dtype=torch.int32)
                    start = torch.zeros(2 * (e - s), dtype=torch.int32)
                    start[0::2] = crops[s:e]
                    x, _ = ops.wave_augment_ragged(bank, idx, start, torch.zeros_like(idx), torch.ones(2 * (e - s)),
                                                   torch.ones(e - s), L, labels=False)
                    y_hat, _ = model(mel(x).unsqueeze(1))
                    logits[s:e].copy_(y_hat.reshape(e - s, -1).float())
                    ops.masked_bce_fwd_bwd(logits[s:e], yy[s:e], sums=bsum[k:k + 1], grad=False, binarize=False)
            nan = torch.full((), float("nan"), device=dev, dtype=torch.float64)
            try:
                ap, auc = metrics.ap_auc(logits, y)
                m_ap, m_auc = ap.mean(), auc.mean()
            except ValueError:
                m_ap = m_auc = nan
            res = torch.stack([m_ap, m_auc, bsum.double().mean()]).cpu().tolist()
    finally:
        model.train(was_training[0])
        mel.train(was_training[1])
    eval_s = time.perf_counter() - t0
    out = {"mAP": res[0], "ROC": res[1], "val_loss": res[2], "n_clips": n, "eval_s": eval_s,
           "clips_per_s": n / max(eval_s, 1e-9)}
    if keep_outputs:
        out["logits"], out["targets"] = logits, y
    return out


def _out_layer(model, sd):
    """-> (keys of the output layer, classes of the checkpoint, classes of the model) for the heads the reference re-sizes
    (models/mn/model.py:285-304), None for any other head."""
    head = getattr(model, "head_type", None)
    if head == "mlp":
        return ["classifier.5.weight", "classifier.5.bias"], sd["classifier.5.bias"].shape[0], model.classifier[5].out_features
    if head == "fully_convolutional":
        keys = ["classifier.0.weight"] + [k for k in sd if k.startswith("classifier.1.")]
        return keys, sd["classifier.1.bias"].shape[0], model.classifier[0].out_channels
    return None


def load_init_checkpoint(model, path):
    """Initialise `model` from a local AudioSet state dict (e.g. one written by `train_dp --out`) - what the reference's
    `pretrained_name` does from its download.  When the class count differs, the output layer is dropped (classifier.5.* for
    the mlp head, classifier.0.weight + classifier.1.* for the fully-convolutional one) with the reference's note, and the
    rest is loaded strictly; a mismatch on any other head raises ValueError.  An attention-pooling model takes the trunk of a
    checkpoint of another head (one without `classifier.subspace_proj.weight`): the reference's note, every `classifier.*`
    key of the checkpoint dropped, the head keeps its fresh initialisation.  -> the list of dropped keys."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    msd = model.state_dict()
    mismatch = sorted(k for k in sd if k in msd and tuple(sd[k].shape) != tuple(msd[k].shape))
    out = _out_layer(model, sd) if mismatch else None
    if mismatch and out is None:
        raise ValueError(f"load_init_checkpoint: {path} does not fit head '{getattr(model, 'head_type', None)}' "
                         f"(shape mismatch at {mismatch[:4]}); only the mlp and fully_convolutional heads can be re-sized")
    dropped = []
    if (not mismatch and getattr(model, "head_type", None) == "multihead_attention_pooling"
            and "classifier.subspace_proj.weight" not in sd):
        # a checkpoint of another head (every released one carries the mlp head): the trunk is loaded, the attention head
        # keeps its fresh initialisation (models/mn/model.py:289-310 prints this note and loads non-strictly)
        dropped = [k for k in sd if k.startswith("classifier.")]
        own = sorted(k for k in msd if k.startswith("classifier."))
        rest = {k for k in sd if not k.startswith("classifier.")}
        missing, unexpected = sorted(set(msd) - rest), sorted(rest - set(msd))
        if missing != own or unexpected:
            raise ValueError(f"load_init_checkpoint: {path} does not hold the model's other tensors "
                             f"(missing {[k for k in missing if k not in own][:4]}, unexpected {unexpected[:4]})")
        print("Loading weights for classifier only implemented for head types 'mlp' and 'fully_convolutional'")
        for k in dropped:
            sd.pop(k)
        model.load_state_dict(sd, strict=False)
        return dropped
    if out is not None:
        keys, n_ckpt, n_model = out
        stray = [k for k in mismatch if k not in keys]
        if n_ckpt == n_model or stray:
            raise ValueError(f"load_init_checkpoint: {path} mismatches outside the output layer: {(stray or mismatch)[:4]}")
        print(f"Number of classes defined: {n_model}, but try to load pre-trained layer with logits: {n_ckpt}\n"
              "Dropping last layer.")
        for k in keys:
            sd.pop(k)
        dropped = keys
    res = model.load_state_dict(sd, strict=not dropped)
    if dropped and (sorted(res.missing_keys) != sorted(dropped) or res.unexpected_keys):
        raise ValueError(f"load_init_checkpoint: {path} does not hold the model's other tensors "
                         f"(missing {res.missing_keys[:4]}, unexpected {res.unexpected_keys[:4]})")
    return dropped
