"""The KD training step of the reference's `ex_audioset.py` (lines 139-199) as one device-resident engine.

What the reference does per step on the host thread: mel -> mixup of the log-mel and the labels (~8 torch ops) ->
model -> BCE on mixed labels + knowledge-distillation BCE against gathered, mixed teacher probabilities (~20 torch ops
incl. a CPU-side index lookup and a host->device copy of the gathered rows) -> three `.cpu()` scalar reads (each a full
device sync) -> backward -> Adam.  Here:

  * the teacher table lives on the GPU; the file-name -> row lookup stays a host dict (names are Python strings) but only
    the (B,) int64 index vector travels;
  * mixup of the log-mel is one kernel (`eat_mixup_fwd`), the label / teacher mixing is folded into the loss kernel;
  * `eat_kd_loss_fwd_bwd` computes the loss terms AND d loss / d logits in one pass over the (B, 527) logits; the three
    statistics are accumulated in a device buffer and read ONCE per epoch (`epoch_stats`);
  * forward / backward are the HIP plans of mn_train.py / dymn_train.py; with `enable_data_parallel` the gradients are
    reduced in buckets while backward runs; the optimizer is whatever the caller built (fused Adam recommended).

Host RNG draws (`mixup`: torch.randperm, then numpy beta) happen in the reference's order, so a seeded run mixes the same
pairs with the same lambdas as the reference loop.
"""
import numpy as np
import torch

from . import ops
from .graphs import HostRing, capture, keep_state, replay_step
from .input_pipeline import I16_SCALE


def mixup(size, alpha):
    """helpers/utils.py:90-95: permutation + per-sample lambda = max(l, 1 - l), l ~ Beta(alpha, alpha)."""
    perm = torch.randperm(size)
    lam = np.random.beta(alpha, alpha, size).astype(np.float32)
    return perm, torch.from_numpy(np.maximum(lam, 1.0 - lam))


class FusedLoss(torch.autograd.Function):
    """Loss scalar (device) of a fused loss kernel: `kernel(logits, step)` writes the step's `n_terms` loss terms into `step`
    and returns d loss / d logits, which backward hands to the network's backward.  `sums` (fp64) accumulates the terms."""

    @staticmethod
    def forward(ctx, logits, sums, n_terms, kernel):
        # the step's terms go to their own zeroed buffer (the epoch accumulator grows to the hundreds: a difference of two
        # such fp32 numbers would lose 3-4 digits of the step loss); the accumulator is updated from it
        step = torch.zeros(n_terms, device=logits.device, dtype=torch.float32)
        ctx.save_for_backward(kernel(logits.contiguous(), step))
        sums += step.to(sums.dtype)
        return step[0]

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return dlogits * g, None, None, None


def kd_loss(logits, y, perm=None, lam=None, teacher=None, teacher_idx=None, kd_lambda=1.0, sums=None):
    """Fused loss of ex_audioset.py:149-189 (see include/eat_hip.h: eat_kd_loss_fwd_bwd).  Returns the scalar loss as a
    device tensor that supports .backward(); `sums` (3,) accumulates (loss, label part, KD part) across calls."""
    if sums is None:
        sums = torch.zeros(3, device=logits.device, dtype=torch.float64)
    y, kd_lambda = y.contiguous().float(), float(kd_lambda)
    return FusedLoss.apply(logits, sums, 3,
                           lambda z, step: ops.kd_loss_fwd_bwd(z, y, perm, lam, teacher, teacher_idx, kd_lambda, step))


class Trainer:
    """What the eager trainers share: `step(*batch)` = `loss_and_backward(*batch)` + optimizer step, and the loss terms
    accumulated in the device buffer `sums`, named by `STATS` and read once per epoch (`epoch_stats`)."""

    STATS = ()

    def step(self, *batch):
        loss = self.loss_and_backward(*batch)
        self.opt.step()
        self.opt.zero_grad()
        self.steps += 1
        return loss                                                            # device scalar: no sync

    def epoch_stats(self):
        """Mean of each loss term since the last call: the ONE host sync of the epoch."""
        s = (self.sums / max(1, self.steps)).cpu().tolist()
        self.sums.zero_()
        self.steps = 0
        return dict(zip(self.STATS, s))

    def _mixup(self, spec):
        """-> (mixed spec, perm, lam) from a host mix-up draw (reference order), or (spec, None, None) without mix-up."""
        if not self.mixup_alpha:
            return spec, None, None
        rn, lm = mixup(spec.shape[0], self.mixup_alpha)
        perm, lam = rn.to(spec.device, torch.int32, non_blocking=True), lm.to(spec.device, non_blocking=True)
        return ops.mixup_fwd(spec, perm, lam), perm, lam


class KDTrainer(Trainer):
    """step(wave, names, y) = one iteration of the reference's training loop (ex_audioset.py:139-199) without host syncs.

    model / mel: the HIP-backed modules; optimizer: e.g. torch.optim.Adam(model.parameters(), lr, fused=True);
    teacher_preds: (N, 527) tensor of teacher LOGITS (as stored in passt_enemble_logits_mAP_495.npy) or None;
    fname_to_index: dict file name -> row of teacher_preds."""

    STATS = ("train_loss", "label_loss", "distillation_loss")

    def __init__(self, model, mel, optimizer, teacher_preds=None, fname_to_index=None, kd_lambda=0.1, temperature=1.0,
                 mixup_alpha=0.3):
        assert 0 <= kd_lambda <= 1, "Lambda for Knowledge Distillation must be between 0 and 1."
        self.model, self.mel, self.opt = model, mel, optimizer
        self.kd_lambda, self.mixup_alpha = float(kd_lambda), mixup_alpha
        dev = next(model.parameters()).device
        self.teacher = None
        if teacher_preds is not None and kd_lambda > 0:
            self.teacher = torch.sigmoid(torch.as_tensor(teacher_preds).float() / temperature).to(dev).contiguous()
        self.fname_to_index = fname_to_index or {}
        if self.teacher is not None and self.fname_to_index:
            # validated once on the host: the loss kernel gathers teacher rows by these indices on the device
            bad = [(f, i) for f, i in self.fname_to_index.items() if not (-1 <= int(i) < self.teacher.shape[0])]
            if bad:
                raise ValueError(f"fname_to_index holds {len(bad)} indices outside the teacher table of {self.teacher.shape[0]} "
                                 f"rows, e.g. {bad[0]}")
        self.sums = torch.zeros(3, device=dev, dtype=torch.float64)
        self.steps = 0

    def _teacher_rows(self, names):
        return torch.tensor([self.fname_to_index.get(f, -1) for f in names], dtype=torch.int64)

    def _loss(self, y_hat, y, perm, lam, tidx):
        # (the reference's kd_lambda == 0 branch skips the KD term, i.e. loss = hard-label BCE: lambda 1 here)
        return kd_loss(y_hat, y, perm, lam, self.teacher, tidx, self.kd_lambda if self.teacher is not None else 1.0, self.sums)

    def loss_and_backward(self, x, names, y):
        """mel -> mixup -> model -> KD loss -> backward (ex_audioset.py:139-196): leaves the gradients in `.grad` (averaged
        over the ranks when the model was handed to `enable_data_parallel`) and returns the loss as a device scalar.
        x (B, 1, L) or (B, L) waveforms and y (B, 527) targets on the device; names: the B file names."""
        bs = x.size(0)
        if x.dtype == torch.int16:                                             # 16-bit transport (input_pipeline.py)
            x = ops.wave_i16_to_f32(x.reshape(bs, -1).contiguous(), scale=1.0 / I16_SCALE)
        spec = self.mel(x.reshape(bs, -1)).unsqueeze(1)                        # _mel_forward, ex_audioset.py:223-228
        spec, perm, lam = self._mixup(spec)                                    # host draws, reference order
        tidx = None
        if self.teacher is not None:
            tidx = self._teacher_rows(names).to(x.device, non_blocking=True)
        y_hat, _ = self.model(spec)
        loss = self._loss(y_hat, y, perm, lam, tidx)
        loss.backward()
        return loss.detach()


class GraphedTrainer(Trainer):
    """What the captured trainers share: static buffers of a (B, L) batch - `wave`, its targets `y`, the log-mel `spec`, the
    mix-up rings and the mel basis (`AugmentMelSTFT.static_tables`) - the captured iteration (`_issue`), its capture
    (`recapture`, inside `keep_state`) and the replayed step.  A subclass stages its batch (`_stage`, which may make host
    draws of its own in front of the mel's) and supplies the loss; `_front` is the part of the iteration in front of the
    mix-up, run eagerly before the replay when SpecAugment masks are set (they are scalar launch arguments of the mel)."""

    def _setup_graph(self, batch_size, clip_samples, n_classes, warmup):
        dev = self.sums.device
        self.B, self.L = int(batch_size), int(clip_samples)
        self._perm = HostRing(torch.arange(self.B, device=dev, dtype=torch.int32)) if self.mixup_alpha else None
        self._lam = HostRing(torch.ones(self.B, device=dev)) if self.mixup_alpha else None
        self.wave = torch.zeros((self.B, self.L), device=dev)
        self.y = torch.zeros((self.B, n_classes), device=dev)
        self.mel_in_graph = not (self.mel.freqm or self.mel.timem)
        T = 1 + (self.L - 1) // self.mel.hopsize
        self.spec = torch.empty((self.B, 1, self.mel.n_mels, T), device=dev)
        self.mel.static_tables(dev)
        self.mel.stage_tables(self.mel.fmin, self.mel.fmax)
        self.warmup = warmup
        self.recapture()

    def _front(self, fmask=(0, 0), tmask=(0, 0)):
        self.mel.forward_static(self.wave, out=self.spec, fmask=fmask, tmask=tmask)

    # How the step mixes the log-mel, as a pair a subclass overrides together: `_stage_mix` makes the host draws (after the
    # mel's) and stages them, `_mix_spec` is the matching part of the captured sequence.  Here: the mix-up.
    def _stage_mix(self):
        if self._perm is not None:
            rn, lm = mixup(self.B, self.mixup_alpha)
            self._perm.put(rn.to(torch.int32))
            self._lam.put(lm)

    def _mix_spec(self, spec):
        """-> (the spec the model sees, perm, lam as `_graph_loss` takes them)."""
        if self._perm is None:
            return spec, None, None
        perm, lam = self._perm.dev, self._lam.dev
        return ops.mixup_fwd(spec, perm, lam), perm, lam

    # the captured sequence (everything reads / writes static buffers)
    def _issue(self):
        if self.mel_in_graph:
            self._front()
        spec, perm, lam = self._mix_spec(self.spec)
        y_hat, _ = self.model(spec)
        loss = self._graph_loss(y_hat, perm, lam)
        loss.backward()
        self.opt.step()
        return loss.detach()

    def recapture(self):
        if not self.mel_in_graph:
            self._front()
        # the warm-up steps train on the static batch: parameters, BatchNorm buffers, optimizer state and the sums are put back
        with keep_state(self.model, self.opt, self.sums):
            self.graph, self.loss = capture(self._issue, self.warmup, self.opt)

    def step(self, *batch):
        if not self._fits(*batch):
            return Trainer.step(self, *batch)            # e.g. the last, partial batch of an epoch
        self._stage(*batch)
        fmin, fmax, fmask, tmask = self.mel.draw(self.L)
        self.mel.stage_tables(fmin, fmax)
        if not self.mel_in_graph:
            self._front(fmask, tmask)
        self._stage_mix()
        replay_step(self)
        self.steps += 1
        return self.loss


class GraphedKDTrainer(GraphedTrainer, KDTrainer):
    """`KDTrainer` with the whole iteration - log-mel, mixup, forward, KD loss, backward, [bucketed RCCL all-reduce], optimizer -
    captured ONCE into a hipGraph and replayed with one host call per step (the eager loop issues ~450 launches per step
    from the reference's single host thread and is launch-bound).  What changes from step to step enters the graph through
    static device buffers, refreshed before each replay:

        wave (B, L) / y (B, 527)      the batch (device-to-device copy from the prefetcher's slot, or the int16 -> fp32
                                      conversion of a 16-bit batch written straight into the buffer);
        perm (B) int32, lam (B)       the mixup draw (helpers/utils.py:90-95), drawn on the host in the reference's order;
        tidx (B) int64                rows of the teacher table (the file-name lookup stays a host dict);
        the mel basis                 band table of the step's (fmin, fmax) jitter (models/preprocess.py:45-55), fixed shape
                                      (`AugmentMelSTFT.static_tables`).

    Host RNG: mel draws, then the mixup draws - the order of `KDTrainer.step` and of ex_audioset.py:139-146, so a seeded
    run replays the same augmentation as the eager trainer.  SpecAugment masks (freqm / timem != 0) are scalar launch
    arguments of the mel kernel: the mel then runs eagerly in front of the graph, writing the graph's input buffer.

    The optimizer must be capturable (torch.optim.Adam(..., capturable=True[, fused=True]); a tensor `lr` lets a scheduler
    change the rate without re-capturing).  DyMN: `model.update_params(epoch)` changes Python-side temperatures that are
    launch constants - call `recapture()` after it.  Batches of another size (a last partial batch) fall back to the eager
    step."""

    def __init__(self, model, mel, optimizer, batch_size, clip_samples, n_classes=527, teacher_preds=None,
                 fname_to_index=None, kd_lambda=0.1, temperature=1.0, mixup_alpha=0.3, warmup=2):
        KDTrainer.__init__(self, model, mel, optimizer, teacher_preds, fname_to_index, kd_lambda, temperature, mixup_alpha)
        self._tidx = (HostRing(torch.full((int(batch_size),), -1, device=self.sums.device, dtype=torch.int64))
                      if self.teacher is not None else None)
        self._setup_graph(batch_size, clip_samples, n_classes, warmup)

    def _graph_loss(self, y_hat, perm, lam):
        return self._loss(y_hat, self.y, perm, lam, None if self._tidx is None else self._tidx.dev)

    def _fits(self, x, names, y):
        return x.size(0) == self.B and x.numel() == self.B * self.L

    def _stage(self, x, names, y):
        if x.dtype == torch.int16:                                           # 16-bit transport (input_pipeline.py)
            ops.wave_i16_to_f32(x.reshape(self.B, -1).contiguous(), out=self.wave, scale=1.0 / I16_SCALE)
        else:
            self.wave.copy_(x.reshape(self.B, -1), non_blocking=True)
        self.y.copy_(y, non_blocking=True)
        if self._tidx is not None:
            self._tidx.put(self._teacher_rows(names))
