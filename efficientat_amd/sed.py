"""Strong-label sound event detection on the device: train and score the frame-level path that `detection.EADetector` runs.

A strongly labelled split (DESED, AudioSet-strong, TAU urban SED: `file, onset, offset, label`) is decoded once
(tools/strong_to_bank.py) into a directory in the format of the FSD50K bank (fsd50k.py) with the events in place of the
clip labels

    waves.npy          (S,) int16 (input_pipeline.I16_SCALE = 32767 per unit) or float32: the clips back to back, at 32 kHz
    lengths.npy        (N,) integer samples per clip, sum = S
    names.txt          N lines
    classes.txt        K lines, the class names in index order
    events.npy         (E, 3) int32 rows (class, onset sample, offset sample)
    event_offsets.npy  (N + 1,) int64: clip i owns the event rows [eo[i], eo[i + 1]), sorted by (class, onset), with
                       0 <= onset < offset <= lengths[i] and 0 <= class < K; a clip may have none
    strong.npy         optional, (N,) uint8 in {0, 1}: 0 marks a WEAKLY labelled clip, one with clip-level tags only; its
                       tags are stored as events that span the whole clip, (class, 0, lengths[i]).  Absent: all ones

and kept on the GPU (`load_bank`) as the ragged bank `ops.wave_augment_ragged` takes, plus the event table.  A training
step draws the FSD50K augmentation (`draw_augment` IS `fsd50k.draw_augment`), builds the waveforms with
`ops.wave_augment_ragged` and - from the same tables - the frame targets with `ops.sed_targets`, so an event follows its
clip through crop, pad, roll and wave-mix; the model's frame logits (`mn_train.forward_train_frames`) meet them in the fused
frame BCE (`frame_bce_loss`).  One frame is one column of the trunk's last feature map: R = r hopsize samples (10240 =
0.32 s at the default geometry), frame t of a window owns its samples [t R, (t + 1) R).  A clip is L = T R samples, a whole
number of frames; the default 327680 is `EADetector`'s 10.24 s window, 32 frames.

`evaluate_frames` tiles every clip of a split with non-overlapping windows and scores the eval frame logits
(`detection.frame_logits`) against the events: frame-level mAP / ROC and segment-based F1 with one frame as the segment.
`evaluate_events` scores what `EADetector.detect` lists: event-based F1 with onset / offset collars (sed_eval's
EventBasedMetrics in integer samples) at a whole grid of thresholds in one kernel launch per chunk of clips
(`ops.event_score`, include/eat_event_score.h), and picks a threshold per class; `save_operating_points` /
`load_operating_points` carry them to `detect --thresholds_file`.  `evaluate_psds` scores the same event lists with PSDS, the
intersection-based score of DCASE Task 4, over the same grid (`ops.psds_count`, include/eat_psds.h; `psds_from_counts`).
A bank with weakly labelled clips (strong.npy) trains with `WeakFrameTrainer` / `GraphedWeakFrameTrainer`: the frame BCE
over the samples whose clips carry frame truth plus a clip-level BCE behind linear-softmax pooling of the frame
probabilities, P = sum_t p_t^2 / sum_t p_t (Wang et al., ICASSP 2019), in one kernel (`weak_frame_loss`,
include/eat_weak_sed.h); the pooling has no parameters, so the checkpoint stays what it was.  The evaluators need onset /
offset truth and refuse such a bank.
The fine-tuned model keeps the reference's state-dict layout (an mlp-head MN with K classes), so its checkpoint loads
straight into `EADetector(model=...)` and `detect --checkpoint`.  Only MN models with the mlp head on the monolithic plan.
"""
import json
import os
import time

import numpy as np
import torch

from . import detection, fsd50k, metrics, ops
from .graphs import HostRing
from .mn_train import _frame_scope, forward_train_frames
from .train_loop import FusedLoss, GraphedTrainer, Trainer

CLIP_SAMPLES = 327680                     # 32 frames of 10240 samples: the 10.24 s window of `detection.EADetector`

draw_augment = fsd50k.draw_augment        # same host RNG order, same tables


def _read_lines(path):
    with open(path) as f:
        return f.read().splitlines()


def load_bank(path, device=None):
    """A decoded strong-label split (see the module header) -> the dict of `fsd50k.load_bank` (waves (S) fp32, offsets (N)
    int64, lengths (N) int32, clip_sum (N) fp64, bank_y (N, K) fp32 on `device` when given, else on the CPU; lengths_cpu,
    names) with bank_y the WEAK labels (the class has at least one event in the clip), plus events (E, 3) int32 and
    event_offsets (N + 1) int64 on the device, classes (K names), strong (N) uint8 on the device (strong.npy; all ones
    without the file) and n_weak, the host count of its zeros.  Every violation of the format is a ValueError naming the file."""
    what = f"SED bank at {path}"
    waves, lengths = fsd50k.read_waves(path, what)
    n = lengths.shape[0]
    events = np.load(os.path.join(path, "events.npy"))
    eo = np.load(os.path.join(path, "event_offsets.npy"))
    names = _read_lines(os.path.join(path, "names.txt"))
    classes = _read_lines(os.path.join(path, "classes.txt"))
    if len(names) != n:
        raise ValueError(f"{what}: names.txt holds {len(names)} lines for {n} clips")
    K = len(classes)
    if K < 1 or any(not c.strip() for c in classes) or len(set(classes)) != K:
        raise ValueError(f"{what}: classes.txt must hold K >= 1 distinct, non-empty names, one per line (got {K} lines)")
    if events.ndim != 2 or events.shape[1] != 3 or events.dtype != np.int32:
        raise ValueError(f"{what}: events.npy must be (E, 3) int32 rows (class, onset, offset), got {events.dtype} {events.shape}")
    E = events.shape[0]
    if eo.ndim != 1 or eo.shape[0] != n + 1 or eo.dtype != np.int64:
        raise ValueError(f"{what}: event_offsets.npy must be (N + 1,) = ({n + 1},) int64, got {eo.dtype} {eo.shape}")
    if eo[0] != 0 or eo[-1] != E or bool((np.diff(eo) < 0).any()):
        raise ValueError(f"{what}: event_offsets.npy must rise from 0 to E = {E} (got {int(eo[0])} .. {int(eo[-1])})")
    clip = np.repeat(np.arange(n), np.diff(eo))                               # the clip of every event row
    cls, on, off = (events[:, j].astype(np.int64) for j in range(3))
    if E and (cls.min() < 0 or cls.max() >= K):
        raise ValueError(f"{what}: events.npy names a class outside [0, {K})")
    bad = (on < 0) | (on >= off) | (off > lengths[clip])
    if bool(bad.any()):
        e = int(np.flatnonzero(bad)[0])
        raise ValueError(f"{what}: events.npy row {e} = {events[e].tolist()} breaks 0 <= onset < offset <= length "
                         f"{int(lengths[clip[e]])} of clip {int(clip[e])}")
    same = clip[1:] == clip[:-1]
    order = (cls[1:] > cls[:-1]) | ((cls[1:] == cls[:-1]) & (on[1:] >= on[:-1]))
    if bool((same & ~order).any()):
        e = int(np.flatnonzero(same & ~order)[0]) + 1
        raise ValueError(f"{what}: events.npy row {e} is out of order: a clip's events are sorted by (class, onset)")
    weak = np.zeros((n, K), dtype=np.float32)
    weak[clip, cls] = 1.0
    strong = np.ones(n, dtype=np.uint8)
    if os.path.exists(os.path.join(path, "strong.npy")):
        strong = np.load(os.path.join(path, "strong.npy"))
        if strong.shape != (n,) or strong.dtype != np.uint8:
            raise ValueError(f"{what}: strong.npy must be (N,) = ({n},) uint8, got {strong.dtype} {strong.shape}")
        if bool((strong > 1).any()):
            raise ValueError(f"{what}: strong.npy holds a value outside {{0, 1}}")
        bad = (strong[clip] == 0) & ((on != 0) | (off != lengths[clip]))
        if bool(bad.any()):
            e = int(np.flatnonzero(bad)[0])
            raise ValueError(f"{what}: strong.npy marks clip {int(clip[e])} weak, but events.npy row {e} = {events[e].tolist()} "
                             f"does not span the whole clip (0, {int(lengths[clip[e]])})")

    dev = torch.device("cpu") if device is None else device
    return dict(fsd50k.resident_waves(waves, lengths, dev), bank_y=torch.from_numpy(weak).to(dev), names=names, classes=classes,
                events=torch.from_numpy(np.ascontiguousarray(events)).to(dev), event_offsets=torch.from_numpy(eo).to(dev),
                strong=torch.from_numpy(np.ascontiguousarray(strong)).to(dev), n_weak=int((strong == 0).sum()))


def n_weak(bank):
    """The number of weakly labelled clips of a bank: the host count `load_bank` took, else read off its "strong" vector
    (0 without one)."""
    if "n_weak" in bank:
        return int(bank["n_weak"])
    strong = bank.get("strong")
    return 0 if strong is None else int((strong == 0).sum())


def _refuse_weak(fn, bank):
    n = n_weak(bank)
    if n:
        raise ValueError(f"{fn}: strong.npy marks {n} of the bank's clips weakly labelled; scoring needs onset / offset truth "
                         f"for every clip")


def frame_bce_loss(logits, y, T, perm=None, lam=None, sums=None):
    """Mean over (b, c, t < T) of BCE-with-logits(z, lam y + (1 - lam) y[perm]) of frame logits (B, K, Tp) against frame
    targets y (B, K, Tp), as a device scalar that supports .backward() (include/eat_sed.h: eat_frame_bce_fwd_bwd); `sums`
    (1,) accumulates it across calls."""
    if sums is None:
        sums = torch.zeros(1, device=logits.device, dtype=torch.float64)
    y = y.contiguous().float()
    return FusedLoss.apply(logits, sums, 1, lambda z, step: ops.frame_bce_fwd_bwd(z, y, T, perm, lam, sums=step)[0])


def weak_frame_loss(logits, y, w, framed, T, perm=None, lam=None, weak_weight=1.0, sums=None):
    """Frame BCE of frame logits (B, K, Tp) against y (B, K, Tp) over the samples with framed (B) int32 != 0, plus
    `weak_weight` times the clip-level BCE of their linear-softmax pooling against the clip targets w (B, K), the mix-up
    (perm, lam) folded into both targets, as a device scalar that supports .backward() (include/eat_weak_sed.h:
    eat_weak_frame_bce_fwd_bwd); `sums` (3,) accumulates (loss, frame term, clip term) across calls."""
    if sums is None:
        sums = torch.zeros(3, device=logits.device, dtype=torch.float64)
    y, w, weak_weight = y.contiguous().float(), w.contiguous().float(), float(weak_weight)
    return FusedLoss.apply(logits, sums, 3, lambda z, step: ops.weak_frame_bce_fwd_bwd(z, y, w, framed, T, perm, lam, weak_weight,
                                                                                     sums=step)[0])


def frame_geometry(model, mel, clip_samples):
    """-> (R samples per frame, T frames per clip, K classes) of `model` behind `mel` on clips of `clip_samples`, which must
    be a whole number of frames.  ValueError for a model outside `mn_train.forward_train_frames`' scope."""
    _frame_scope(model)
    _, r, K = detection.check_model(model)
    R, L = int(r) * int(mel.hopsize), int(clip_samples)
    if L < R or L % R:
        raise ValueError(f"clip_samples={L} must be a positive multiple of R = {R} samples (one frame of the last feature map)")
    return R, L // R, K


class FrameBCETrainer(Trainer):
    """step(batch) = one strong-label training iteration on the bank clips `batch` (host indices): the FSD50K augmentation
    of the waveforms (`ops.wave_augment_ragged`), the frame targets from the same tables (`ops.sed_targets`), mel, log-mel
    mix-up, `forward_train_frames`, the fused frame BCE, backward.

    bank: the dict of `load_bank`; clip_samples: L = T R, a whole number of frames; the other arguments as
    `finetune.BCETrainer`."""

    STATS = ("train_loss",)

    def __init__(self, model, mel, optimizer, bank, clip_samples=CLIP_SAMPLES, mixup_alpha=0.3, gain_augment=12, roll=True,
                 wavmix=True):
        self.model, self.mel, self.opt = model, mel, optimizer
        self.bank, self.L = bank, int(clip_samples)
        self.R, self.T, self.K = frame_geometry(model, mel, clip_samples)
        self.Tp = ops.pitch4(self.T)
        n = bank["lengths"].numel()
        if (bank["waves"].dim() != 1 or bank["offsets"].numel() != n or bank["clip_sum"].numel() != n
                or len(bank["lengths_cpu"]) != n or bank["event_offsets"].numel() != n + 1):
            raise ValueError("FrameBCETrainer: waves (S), offsets / lengths / clip_sum (N), event_offsets (N + 1) and "
                             "lengths_cpu (N) do not match")
        if len(bank["classes"]) != self.K:
            raise ValueError(f"FrameBCETrainer: the bank has {len(bank['classes'])} classes, the model {self.K}")
        self.mixup_alpha = mixup_alpha
        self.gain_augment, self.roll, self.wavmix = int(gain_augment), bool(roll), bool(wavmix)
        dev = next(model.parameters()).device
        self.sums = torch.zeros(1, device=dev, dtype=torch.float64)
        self.steps = 0

    def draw(self, batch):
        idx, start, shift, amp, mix = draw_augment(batch, self.bank["lengths_cpu"], self.L, self.gain_augment, self.roll,
                                                   self.wavmix)
        ops.check_ragged_draws(idx, start, shift, self.bank["lengths_cpu"], self.L)
        return idx, start, shift, amp, mix

    def _frames(self, spec):
        z = forward_train_frames(self.model, spec)
        if z.shape[2] != self.Tp:
            raise RuntimeError(f"the model's last feature map of a {self.L}-sample clip gives rows of {z.shape[2]} frames, the "
                               f"frame plan promises pitch4(T = {self.T})")
        return z

    def loss_and_backward(self, batch):
        """augment + frame targets -> mel -> log-mel mix-up -> frame logits -> frame BCE -> backward."""
        dev = self.bank["waves"].device
        idx, start, shift, amp, mix = self.draw(batch)                        # validated: uploaded once for both kernels
        idx, start, shift = (t.to(dev, torch.int32, non_blocking=True) for t in (idx, start, shift))
        amp, mix = (t.to(dev, torch.float32, non_blocking=True) for t in (amp, mix))
        x, _ = ops.wave_augment_ragged(self.bank, idx, start, shift, amp, mix, self.L, labels=False)
        y = ops.sed_targets(self.bank, idx, start, shift, mix, self.L, self.R, self.T, self.Tp)
        spec = self.mel(x).unsqueeze(1)
        spec, perm, lam = self._mixup(spec)                                   # host draws, reference order
        loss = frame_bce_loss(self._frames(spec), y, self.T, perm, lam, self.sums)
        loss.backward()
        return loss.detach()


class GraphedFrameBCETrainer(GraphedTrainer, FrameBCETrainer):
    """`FrameBCETrainer` with the whole iteration captured once and replayed, on `finetune.GraphedBCETrainer`'s
    static-buffer scheme: rings for idx / start / shift / amp / mix, perm / lam and the mel basis;
    `eat_wave_augment_ragged` and `eat_sed_targets` run inside the graph and write `self.wave` and the static (B, K, Tp)
    target buffer.  Everything said there about the optimizer, SpecAugment masks and partial batches holds here."""

    def __init__(self, model, mel, optimizer, bank, batch_size, clip_samples=CLIP_SAMPLES, mixup_alpha=0.3, gain_augment=12,
                 roll=True, wavmix=True, warmup=2):
        FrameBCETrainer.__init__(self, model, mel, optimizer, bank, clip_samples, mixup_alpha, gain_augment, roll, wavmix)
        self._setup_rings(int(batch_size), warmup)

    def _setup_rings(self, B, warmup):
        dev = self.bank["waves"].device
        first = torch.full((2 * B,), -1, device=dev, dtype=torch.int32)
        first[0::2] = 0                                                       # (clip 0 from its start, no wave-mix: the warm-up batch)
        self._idx = HostRing(first)
        self._start = HostRing(torch.zeros(2 * B, device=dev, dtype=torch.int32))
        self._shift = HostRing(torch.zeros(2 * B, device=dev, dtype=torch.int32))
        self._amp = HostRing(torch.ones(2 * B, device=dev))
        self._mix = HostRing(torch.ones(B, device=dev))
        self._win_mean = torch.zeros(2 * B, device=dev, dtype=torch.float64)
        self._setup_graph(B, self.L, self.K * self.Tp, warmup)                # (y: the (B, K, Tp) targets, flat per sample)

    def _front(self, fmask=(0, 0), tmask=(0, 0)):
        tables = (self._idx.dev, self._start.dev, self._shift.dev)
        ops.wave_augment_ragged(self.bank, *tables, self._amp.dev, self._mix.dev, self.L, out=self.wave,
                                win_mean=self._win_mean, labels=False)
        ops.sed_targets(self.bank, *tables, self._mix.dev, self.L, self.R, self.T, self.Tp, out=self.y)
        super()._front(fmask, tmask)

    # the captured sequence: `GraphedTrainer._issue` with the frame logits in place of `self.model(spec)`
    def _issue(self):
        if self.mel_in_graph:
            self._front()
        spec, perm, lam = self._mix_spec(self.spec)
        loss = self._graph_loss(self._frames(spec), perm, lam)
        loss.backward()
        self.opt.step()
        return loss.detach()

    def _graph_loss(self, z, perm, lam):
        return frame_bce_loss(z, self.y.view(self.B, self.K, self.Tp), self.T, perm, lam, self.sums)

    def _fits(self, batch):
        return len(batch) == self.B

    def _stage(self, batch):
        idx, start, shift, amp, mix = self.draw(batch)   # host draws, reference order: augmentation, then the mel's, mix-up
        self._idx.put(idx)
        self._start.put(start)
        self._shift.put(shift)
        self._amp.put(amp)
        self._mix.put(mix)


class WeakFrameTrainer(FrameBCETrainer):
    """`FrameBCETrainer` on a bank that mixes strongly and weakly labelled clips (`bank["strong"]`): the strong step plus
    the clip targets and the frame-truth flag from the same uploaded tables (`ops.sed_clip_targets`), and `weak_frame_loss`
    - the frame BCE over the samples whose clips all carry frame truth plus `weak_weight` times the pooled clip BCE over
    every sample - in place of `frame_bce_loss`.  Batches are drawn from the whole bank; nothing is stratified."""

    STATS = ("train_loss", "train_frame_loss", "train_clip_loss")

    def __init__(self, model, mel, optimizer, bank, clip_samples=CLIP_SAMPLES, mixup_alpha=0.3, gain_augment=12, roll=True,
                 wavmix=True, weak_weight=1.0):
        FrameBCETrainer.__init__(self, model, mel, optimizer, bank, clip_samples, mixup_alpha, gain_augment, roll, wavmix)
        self._weak_setup(weak_weight)

    def _weak_setup(self, weak_weight):
        self.weak_weight = float(weak_weight)
        if not 0.0 <= self.weak_weight < float("inf"):
            raise ValueError(f"weak_weight must be finite and not negative (got {weak_weight})")
        n = self.bank["lengths"].numel()
        strong = self.bank.get("strong")
        if strong is None or strong.dtype != torch.uint8 or strong.numel() != n or strong.device != self.bank["lengths"].device:
            raise ValueError("WeakFrameTrainer: the bank needs strong (N) uint8 next to its lengths (sed.load_bank)")
        self.sums = torch.zeros(3, device=self.sums.device, dtype=torch.float64)

    def loss_and_backward(self, batch):
        """augment + frame and clip targets -> mel -> log-mel mix-up -> frame logits -> fused frame + clip BCE -> backward."""
        dev = self.bank["waves"].device
        idx, start, shift, amp, mix = self.draw(batch)                        # validated: uploaded once for the three kernels
        idx, start, shift = (t.to(dev, torch.int32, non_blocking=True) for t in (idx, start, shift))
        amp, mix = (t.to(dev, torch.float32, non_blocking=True) for t in (amp, mix))
        x, _ = ops.wave_augment_ragged(self.bank, idx, start, shift, amp, mix, self.L, labels=False)
        y = ops.sed_targets(self.bank, idx, start, shift, mix, self.L, self.R, self.T, self.Tp)
        w, framed = ops.sed_clip_targets(self.bank, idx, start, mix, self.L)
        spec = self.mel(x).unsqueeze(1)
        spec, perm, lam = self._mixup(spec)                                   # host draws, reference order
        loss = weak_frame_loss(self._frames(spec), y, w, framed, self.T, perm, lam, self.weak_weight, self.sums)
        loss.backward()
        return loss.detach()


class GraphedWeakFrameTrainer(GraphedFrameBCETrainer, WeakFrameTrainer):
    """`WeakFrameTrainer` captured once and replayed, on `GraphedFrameBCETrainer`'s scheme: `eat_sed_clip_targets` runs
    inside the graph next to `eat_sed_targets` and fills the static (B, K) clip targets and (B) frame-truth flags.  The loss
    kernel counts the framed samples on the device, so the one graph serves every mixture of strong and weak clips, a batch
    without any frame truth included."""

    def __init__(self, model, mel, optimizer, bank, batch_size, clip_samples=CLIP_SAMPLES, mixup_alpha=0.3, gain_augment=12,
                 roll=True, wavmix=True, warmup=2, weak_weight=1.0):
        FrameBCETrainer.__init__(self, model, mel, optimizer, bank, clip_samples, mixup_alpha, gain_augment, roll, wavmix)
        self._weak_setup(weak_weight)
        dev, B = bank["waves"].device, int(batch_size)
        self.w = torch.zeros((B, self.K), device=dev)
        self.framed = torch.zeros((B,), device=dev, dtype=torch.int32)
        self._setup_rings(B, warmup)

    def _front(self, fmask=(0, 0), tmask=(0, 0)):
        ops.sed_clip_targets(self.bank, self._idx.dev, self._start.dev, self._mix.dev, self.L, out=self.w, framed_out=self.framed)
        super()._front(fmask, tmask)

    def _graph_loss(self, z, perm, lam):
        return weak_frame_loss(z, self.y.view(self.B, self.K, self.Tp), self.w, self.framed, self.T, perm, lam, self.weak_weight,
                               self.sums)


def eval_windows(lengths, L):
    """The non-overlapping windows of L samples that tile every clip -> (clip (W,), q (W,), valid (W,)) int64 numpy arrays:
    window q of clip i starts at its sample q L and holds valid = min(L, length - q L) samples."""
    lengths = np.asarray(lengths, dtype=np.int64)
    n_w = -(-lengths // L)
    clip = np.repeat(np.arange(lengths.shape[0], dtype=np.int64), n_w)
    q = np.arange(int(n_w.sum()), dtype=np.int64) - np.repeat(np.cumsum(n_w) - n_w, n_w)
    return clip, q, np.minimum(L, lengths[clip] - q * L)


def segment_scores(counts):
    """(K, 3) (tp, fp, fn) per class -> segment-based micro / macro F1, precision and recall.  Micro: from the summed counts.
    Macro: the mean over the classes that have a reference or a predicted segment (2 tp + fp + fn > 0) of the per-class
    value, a ratio with an empty denominator counting as 0.  Nothing to average: NaN."""
    c = np.asarray(counts, dtype=np.float64).reshape(-1, 3)

    def ratios(tp, fp, fn):
        with np.errstate(divide="ignore", invalid="ignore"):
            p = np.where(tp + fp > 0, tp / (tp + fp), 0.0)
            r = np.where(tp + fn > 0, tp / (tp + fn), 0.0)
            f = np.where(2 * tp + fp + fn > 0, 2 * tp / (2 * tp + fp + fn), np.nan)
        return f, p, r

    tp, fp, fn = c.sum(0)
    f, p, r = (float(v) for v in ratios(tp, fp, fn))
    if np.isnan(f):
        p = r = float("nan")
    out = {"micro_f1": f, "micro_precision": p, "micro_recall": r}
    fk, pk, rk = ratios(c[:, 0], c[:, 1], c[:, 2])
    live = ~np.isnan(fk)
    for name, v in (("macro_f1", fk), ("macro_precision", pk), ("macro_recall", rk)):
        out[name] = float(v[live].mean()) if live.any() else float("nan")
    return out


def evaluate_frames(model, mel, bank, batch_windows=64, threshold=0.5, clip_samples=CLIP_SAMPLES, keep_outputs=False):
    """Frame-level scores of `model` on a resident strong-label split -> {"frame_mAP", "frame_ROC", "micro_f1",
    "micro_precision", "micro_recall", "macro_f1", "macro_precision", "macro_recall", "val_loss", "n_clips", "n_frames",
    "eval_s"} (+ "rows", "truth", "weight" (W T, K) device tensors and "counts" (K, 3) with keep_outputs=True).

    Every clip is tiled by non-overlapping windows of L = clip_samples (`eval_windows`), read straight from the flat bank
    buffer by `AugmentMelSTFT.forward_windows` (a window's tail beyond its clip reads as zeros; nothing is copied), in chunks
    of `batch_windows`: eval forward, `detection.frame_logits`, the targets from `ops.sed_targets` (shift 0, no mix), and one
    `eat_frame_bce_fwd_bwd` per chunk for loss, counts and score rows over the window's ceil(valid / R) frames.
    frame_mAP / frame_ROC: the plain means over the classes of `metrics.ap_auc` on the frame LOGITS with the frame validity as
    sample_weight (a class without a positive frame has AP 0 and makes ROC NaN, as in `evaluate_multilabel`).  F1, precision,
    recall: segment-based with one frame of R samples as the segment (`segment_scores`), a frame predicted where
    sigmoid(logit) >= threshold (a scalar or one value per class) - what `EADetector` binarises without median filter.
    val_loss: the mean BCE over all valid (frame, class) pairs.  One host wait at the end; mode restore and forked RNG as
    `finetune.evaluate_multilabel`."""
    _refuse_weak("evaluate_frames", bank)
    n = bank["lengths"].numel()
    if n == 0:
        raise ValueError("evaluate_frames: the split is empty")
    if not 1 <= int(batch_windows) <= 65535:
        raise ValueError(f"batch_windows must lie in [1, 65535] (got {batch_windows})")
    R, T, K = frame_geometry(model, mel, clip_samples)
    if len(bank["classes"]) != K:
        raise ValueError(f"evaluate_frames: the bank has {len(bank['classes'])} classes, the model {K}")
    L, Tp, bw = int(clip_samples), ops.pitch4(T), int(batch_windows)
    dev = bank["waves"].device
    hi, _ = detection.thresholds(threshold, None, K)
    clip, q, valid = eval_windows(bank["lengths_cpu"].numpy(), L)
    W = clip.shape[0]
    starts = bank["offsets"].cpu().numpy()[clip] + q * L
    nframes = -(-valid // R)
    chunk_frames = np.add.reduceat(nframes, np.arange(0, W, bw)).astype(np.float64)
    was_training = (model.training, mel.training)
    model.eval()
    mel.eval()
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    try:
        with torch.random.fork_rng(devices=[]), torch.no_grad():
            thr = torch.from_numpy(hi).to(dev)
            d_start, d_valid = (t.to(dev) for t in ops.check_windows(starts, valid, L, bank["waves"].numel()))
            d_nf = torch.from_numpy(nframes.astype(np.int32)).to(dev)
            idx = torch.full((2 * W,), -1, dtype=torch.int32)
            idx[0::2] = torch.from_numpy(clip.astype(np.int32))
            st = torch.zeros(2 * W, dtype=torch.int32)
            st[0::2] = torch.from_numpy((q * L).astype(np.int32))
            ops.check_eval_draws(idx, st, bank["lengths_cpu"])
            d_idx, d_st = idx.to(dev), st.to(dev)
            d_shift, d_mix = torch.zeros(2 * W, device=dev, dtype=torch.int32), torch.ones(W, device=dev)
            rows = torch.empty((W * T, K), device=dev, dtype=torch.float32)
            truth = torch.empty((W, T, K), device=dev, dtype=torch.float32)
            counts = torch.zeros((K, 3), device=dev, dtype=torch.int64)
            bsum = torch.zeros(len(chunk_frames), device=dev, dtype=torch.float32)
            for k, w0 in enumerate(range(0, W, bw)):
                w1 = min(w0 + bw, W)
                spec = mel.forward_windows(bank["waves"], d_start[w0:w1], d_valid[w0:w1], L)
                ymap = model._forward_impl(spec.unsqueeze(1), return_fmaps=True)[1][-1]
                if ymap.shape[3] != T:
                    raise RuntimeError(f"the model's last feature map of a {L}-sample window is {ymap.shape[3]} columns wide, "
                                       f"the frame plan promises T = {T}")
                z = detection.frame_logits(model, ymap)
                y = ops.sed_targets(bank, d_idx[2 * w0:2 * w1], d_st[2 * w0:2 * w1], d_shift[2 * w0:2 * w1], d_mix[w0:w1], L, R,
                                    T, Tp)
                ops.frame_bce_fwd_bwd(z, y, T, nframes=d_nf[w0:w1], sums=bsum[k:k + 1], grad=False, counts=counts, thr=thr,
                                      rows=rows[w0 * T:w1 * T])
                truth[w0:w1].copy_(y[:, :, :T].transpose(1, 2))
            truth = (truth.view(W * T, K) > 0.5).float()
            weight = (torch.arange(T, device=dev).view(1, T) < d_nf.view(W, 1)).float().view(W * T, 1).expand(W * T, K).contiguous()
            nan = torch.full((), float("nan"), device=dev, dtype=torch.float64)
            try:
                ap, auc = metrics.ap_auc(rows, truth, sample_weight=weight)
                m_ap, m_auc = ap.mean(), auc.mean()
            except ValueError:
                m_ap = m_auc = nan
            cf = torch.from_numpy(chunk_frames).to(dev)
            loss = (bsum.double() * cf).sum() / cf.sum()
            res = torch.cat([torch.stack([m_ap, m_auc, loss]), counts.double().flatten()]).cpu().numpy()
    finally:
        model.train(was_training[0])
        mel.train(was_training[1])
    eval_s = time.perf_counter() - t0
    cnt = np.rint(res[3:]).astype(np.int64).reshape(K, 3)
    out = {"frame_mAP": float(res[0]), "frame_ROC": float(res[1])}
    out.update(segment_scores(cnt))
    out.update({"val_loss": float(res[2]), "n_clips": n, "n_frames": int(nframes.sum()), "eval_s": eval_s})
    if keep_outputs:
        out.update(rows=rows, truth=truth, weight=weight, counts=cnt)
    return out


# ---------------------------------------------------------------------------------------------------- event-based scoring
SCORE_NAMES = ("micro_f1", "micro_precision", "micro_recall", "macro_f1", "macro_precision", "macro_recall")
_TINY = np.finfo(np.float32).tiny                                             # the smallest positive normal fp32


def collar_samples(collar_ms, sample_rate):
    """The onset collar c = round(collar_ms sample_rate / 1000) in samples."""
    c = float(collar_ms) * int(sample_rate) / 1000.0
    if not np.isfinite(c) or c < 0 or c >= 2 ** 31:
        raise ValueError(f"collar_ms={collar_ms} must be finite, not negative and below 2^31 samples")
    return int(round(c))


def event_tolerances(events, collar_samples, pct):
    """Offset tolerance of every reference row of events (E, 3) (class, onset, offset) in samples -> (E,) int32 numpy:
    max(collar_samples, floor(pct (offset - onset))), the product taken in fp64."""
    ev = np.asarray(events.cpu() if torch.is_tensor(events) else events)
    if ev.ndim != 2 or ev.shape[1] != 3:
        raise ValueError(f"event_tolerances: events must be (E, 3) rows (class, onset, offset), got {ev.shape}")
    c, pct = int(collar_samples), float(pct)
    if c < 0 or not np.isfinite(pct) or pct < 0:
        raise ValueError(f"event_tolerances: collar_samples and pct must not be negative (got {collar_samples}, {pct})")
    length = ev[:, 2].astype(np.int64) - ev[:, 1].astype(np.int64)
    tol = np.maximum(np.int64(c), np.floor(np.float64(pct) * length.astype(np.float64)).astype(np.int64))
    if tol.size and tol.max() >= 2 ** 31:
        raise ValueError("event_tolerances: a tolerance of 2^31 samples or more")
    return tol.astype(np.int32)


def threshold_grid(thresholds=None, low_ratio=1.0):
    """-> (hi (V,), lo (V,)) float32: `thresholds` (default the 49 values k / 50, k = 1 .. 49) and
    lo = max(low_ratio hi, smallest positive normal fp32) with the product taken in fp32, so lo <= hi."""
    low_ratio = float(low_ratio)
    if not 0.0 <= low_ratio <= 1.0:
        raise ValueError(f"low_ratio must lie in [0, 1] (got {low_ratio})")
    hi = (np.arange(1, 50, dtype=np.float64) / 50.0).astype(np.float32) if thresholds is None else \
        np.ascontiguousarray(np.asarray(thresholds, dtype=np.float32).reshape(-1))
    if hi.size < 1 or not bool(((hi > 0) & (hi <= 1)).all()):
        raise ValueError("thresholds must hold V >= 1 values in (0, 1]")
    lo = np.maximum(np.float32(low_ratio) * hi, _TINY).astype(np.float32)
    return hi, np.minimum(lo, hi)


def class_f1(counts):
    """(..., 3) (tp, fp, fn) -> F1 = 2 tp / (2 tp + fp + fn) in fp64, NaN where there is nothing to score."""
    c = np.asarray(counts, dtype=np.float64)
    den = 2 * c[..., 0] + c[..., 1] + c[..., 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, 2 * c[..., 0] / den, np.nan)


def pick_thresholds(counts, hi, lo, threshold, low_ratio=1.0):
    """counts (V, K, 3), the grid (hi, lo) -> (index of the grid value nearest `threshold` (the first of equals), best
    index (K,) or -1, best_threshold (K,), best_low_threshold (K,) float32).  Per class the FIRST grid value of maximal F1,
    a threshold without anything to score ranking below every F1; a class with nothing to score at any threshold keeps
    `threshold` (index -1)."""
    f = class_f1(counts)                                                     # (V, K)
    at = int(np.argmin(np.abs(hi.astype(np.float64) - float(np.float32(threshold)))))
    best = np.argmax(np.where(np.isnan(f), -1.0, f), axis=0)
    best = np.where(np.isnan(f).all(axis=0), -1, best)
    keep_hi = np.float32(threshold)
    keep_lo = np.minimum(np.maximum(np.float32(low_ratio) * keep_hi, _TINY), keep_hi).astype(np.float32)
    b_hi = np.where(best >= 0, hi[np.maximum(best, 0)], keep_hi).astype(np.float32)
    b_lo = np.where(best >= 0, lo[np.maximum(best, 0)], keep_lo).astype(np.float32)
    return at, best, b_hi, b_lo


def _walk_chunks(fn, model, mel, bank, hi, lo, n_acc, score, finish=None, median_ms=960, min_duration_ms=0, max_gap_ms=0,
                 batch_clips=256, taper="triangle", clip_seconds=10.24, hop_seconds=5.12, batch_windows=64, unfiltered=False):
    """The chunk walk `evaluate_events`, `evaluate_psds`, `tune_postprocessing` and `score_operating_points` share.  The
    bank's clips are walked in contiguous chunks of `batch_clips` of the resident flat buffer (no waveform is copied):
    `detector.plan` on the chunk's lengths, `window_logits` on the slice (through `mel`), `ops.detect_stitch`, the median,
    then `score(acc, filt, table, nsamp, R, d_hi, d_lo, max_gap, min_len, first)`, which adds the chunk's counts to acc, a
    flat int64 device buffer of n_acc zeros; `finish(acc)` runs after the last chunk; then the one host wait.  The median:
    median_ms is a scalar or one value per class (`detection.median_frames_per_class`); frame widths that are the same in
    every class run `ops.detect_median` (nothing at width 1), widths that differ one `ops.detect_median_bank` of one slice.
    unfiltered = True hands `score` the stitched probabilities instead, for a caller that filters them itself (median_ms is
    still checked).  Model and mel are put in eval mode and restored, the RNG is forked.
    -> (acc on the host, seconds, K, the (K,) frame widths)."""
    n = bank["lengths"].numel()
    if n == 0:
        raise ValueError(f"{fn}: the split is empty")
    if int(batch_clips) < 1:
        raise ValueError(f"batch_clips must be >= 1 (got {batch_clips})")
    _, _, K = detection.check_model(model)
    if len(bank["classes"]) != K:
        raise ValueError(f"{fn}: the bank has {len(bank['classes'])} classes, the model {K}")
    dev = bank["waves"].device
    lengths = bank["lengths_cpu"].numpy().astype(np.int64)
    offsets = np.cumsum(lengths) - lengths
    was_training = (model.training, mel.training)
    model.eval()
    mel.eval()
    try:
        det = detection.EADetector(model=model, device=dev, sample_rate=mel.sr, window_size=mel.win_length, hop_size=mel.hopsize,
                                   n_mels=mel.n_mels, batch_windows=batch_windows, clip_seconds=clip_seconds,
                                   hop_seconds=hop_seconds, taper=taper)
        det.mel = mel                                                         # the caller's front end, not a default one
        geo = det.geometry
        m_k = detection.median_frames_per_class(median_ms, geo.frame_s, K)
        m = int(m_k[0])
        widths = None if bool((m_k == m).all()) else ops.median_width_table(m_k, K)
        min_len, max_gap = detection.ms_to_frames(min_duration_ms, geo.frame_s), detection.ms_to_frames(max_gap_ms, geo.frame_s)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        with torch.random.fork_rng(devices=[]), torch.no_grad():
            d_hi, d_lo = (t.to(dev) for t in ops.check_threshold_grid(hi, lo))
            d_n = torch.from_numpy(lengths).to(dev)
            acc = torch.zeros((int(n_acc),), device=dev, dtype=torch.int64)
            for i0 in range(0, n, int(batch_clips)):
                i1 = min(i0 + int(batch_clips), n)
                starts, valids, table = det.plan(lengths[i0:i1].tolist())
                flat = bank["waves"][int(offsets[i0]):int(offsets[i1 - 1] + lengths[i1 - 1])]
                P = det.window_logits(flat, starts, valids)
                prob = ops.detect_stitch(P, table, geo.Hf, geo.T, det._wt)
                if unfiltered:
                    filt = prob
                elif widths is not None:
                    filt = ops.detect_median_bank(prob, table, widths)[0]
                else:
                    filt = ops.detect_median(prob, table, m) if m != 1 else prob
                score(acc, filt, table, d_n[i0:i1], geo.R, d_hi, d_lo, max_gap, min_len, i0)
            if finish is not None:
                finish(acc)
            res = acc.cpu().numpy()                                           # the one host wait
    finally:
        model.train(was_training[0])
        mel.train(was_training[1])
    return res, time.perf_counter() - t0, K, m_k


def _median_settings(median_ms):
    """The settings entries of a median given as a scalar ({"median_ms"}) or per class ({"median_ms": the first class's
    value, "class_median_ms": the K values})."""
    if np.ndim(median_ms) == 0:
        return {"median_ms": float(median_ms)}
    ms = [float(v) for v in np.asarray(median_ms, dtype=np.float64).reshape(-1)]
    return {"median_ms": ms[0], "class_median_ms": ms}


def _event_refs(bank, mel, collar_ms, offset_pct):
    """The reference events of a strong-label bank for `ops.event_score` -> (EventRefs, collar in samples, n_ref (K,))."""
    c = collar_samples(collar_ms, mel.sr)
    K = len(bank["classes"])
    events_cpu = bank["events"].cpu()
    refs = ops.event_refs(events_cpu, torch.from_numpy(event_tolerances(events_cpu, c, offset_pct)),
                          bank["event_offsets"].cpu(), K)
    return refs, c, np.bincount(events_cpu[:, 0].numpy(), minlength=K).astype(np.int64)


def evaluate_events(model, mel, bank, thresholds=None, low_ratio=1.0, median_ms=960, min_duration_ms=0, max_gap_ms=0,
                    collar_ms=200, offset_pct=0.2, threshold=0.5, batch_clips=256, taper="triangle", clip_seconds=10.24,
                    hop_seconds=5.12, batch_windows=64):
    """Event-based (collar) scores of what `detection.EADetector(model=model).detect` lists on a resident strong-label
    split, at a whole grid of thresholds at once.

    The bank's clips are walked in contiguous chunks of `batch_clips` of the resident flat buffer (`_walk_chunks`): stitch,
    median, then ONE `ops.event_score` for all thresholds; int64 counts accumulate on the device, with one
    host wait at the end.  Grid: `threshold_grid(thresholds, low_ratio)`.  An estimated event of frames [on, off) spans the
    samples [on R, min(off R, n)); it matches a reference of its clip and class iff the onsets are at most
    c = round(collar_ms sample_rate / 1000) samples apart and the offsets at most max(c, floor(offset_pct length)) of the
    reference (`event_tolerances`); greedy in reference order as sed_eval's EventBasedMetrics (integer samples: a float-
    second sed_eval run may differ only where a distance sits exactly on a collar).

    -> {"thresholds", "low_thresholds" (V,) float32; "counts" (V, K, 3) int64 (tp, fp, fn); "grid": {name: (V,) float64} for
    micro / macro F1, precision, recall (`segment_scores` per threshold); "class_f1" (V, K); "threshold": the grid value
    nearest the argument (itself when it is on the grid), "threshold_index", and the six scores at it under their plain
    names; "best_threshold", "best_low_threshold" (K,) float32 and "best_index" (K,) (`pick_thresholds`); "macro_f1_best":
    macro F1 with those per-class values - TUNED ON THE SCORED SPLIT, an upper bound for any other; "n_clips", "n_ref",
    "eval_s", "settings"}.  median_ms is a scalar or one value per class; given per class, settings gains "class_median_ms"
    (the K values) and settings["median_ms"] holds the first class's value.  Mode restore and forked RNG as
    `evaluate_frames`."""
    _refuse_weak("evaluate_events", bank)
    n = bank["lengths"].numel()
    if n == 0:
        raise ValueError("evaluate_events: the split is empty")
    hi, lo = threshold_grid(thresholds, low_ratio)
    K = len(bank["classes"])
    refs, c, n_ref = _event_refs(bank, mel, collar_ms, offset_pct)

    def score(acc, filt, table, nsamp, R, d_hi, d_lo, max_gap, min_len, first):
        cnt = ops.event_score(filt, table, nsamp, R, refs, c, d_hi, d_lo, max_gap, min_len, first=first)
        acc += cnt.sum(dim=0, dtype=torch.int64).flatten()

    res, eval_s, K, _ = _walk_chunks("evaluate_events", model, mel, bank, hi, lo, K * hi.size * 2, score, None, median_ms,
                                     min_duration_ms, max_gap_ms, batch_clips, taper, clip_seconds, hop_seconds, batch_windows)
    settings = _median_settings(median_ms)
    settings.update({"min_duration_ms": float(min_duration_ms), "max_gap_ms": float(max_gap_ms), "taper": taper,
                     "window_size": float(clip_seconds), "hop_length": float(hop_seconds), "collar_ms": float(collar_ms),
                     "offset_pct": float(offset_pct), "low_ratio": float(low_ratio)})
    return _event_result(_event_counts(res.reshape(K, hi.size, 2), n_ref), hi, lo, threshold, low_ratio, n, n_ref, eval_s,
                         settings)


def _event_counts(res, n_ref):
    """(K, V, 2) sums of `ops.event_score`'s (tp, n_est) over a split -> counts (V, K, 3) int64 (tp, fp, fn)."""
    tp, n_est = res[:, :, 0].T, res[:, :, 1].T                                # (V, K)
    return np.stack([tp, n_est - tp, n_ref[None, :] - tp], axis=2).astype(np.int64)


def _event_result(counts, hi, lo, threshold, low_ratio, n, n_ref, eval_s, settings):
    """The result dict of `evaluate_events` from the counts (V, K, 3) of one median setting."""
    K = counts.shape[1]
    rows = [segment_scores(counts[v]) for v in range(hi.size)]
    at, best, b_hi, b_lo = pick_thresholds(counts, hi, lo, threshold, low_ratio)
    at_best = np.where(best >= 0, best, at)
    out = {"thresholds": hi, "low_thresholds": lo, "counts": counts,
           "grid": {k: np.asarray([r[k] for r in rows], dtype=np.float64) for k in SCORE_NAMES}, "class_f1": class_f1(counts),
           "threshold": float(hi[at]), "threshold_index": at}
    out.update(rows[at])
    out.update({"best_threshold": b_hi, "best_low_threshold": b_lo, "best_index": best,
                "macro_f1_best": segment_scores(counts[at_best, np.arange(K)])["macro_f1"], "n_clips": n,
                "n_ref": int(n_ref.sum()), "eval_s": eval_s, "settings": settings})
    return out


# ---- the median width per class: one trunk pass per chunk, all candidate widths from one `ops.detect_median_bank`
def pick_operating_points(counts_grid, hi, lo, threshold, ref_index, low_ratio=1.0):
    """counts_grid (Mw, V, K, 3) (tp, fp, fn) per median width (ascending), threshold pair and class; the grid (hi, lo) ->
    (index of the grid value nearest `threshold`, best width index (K,), best threshold index (K,) or -1, best_threshold
    (K,), best_low_threshold (K,) float32).  Per class the FIRST maximum of F1 over the (Mw, V) grid in width-major order:
    the narrowest width, then the lowest threshold; a point without anything to score ranks below every F1.  A class with
    nothing to score anywhere keeps width `ref_index` and `threshold` (threshold index -1): the rule of `pick_thresholds`."""
    counts_grid = np.asarray(counts_grid)
    if counts_grid.ndim != 4 or counts_grid.shape[3] != 3 or counts_grid.shape[1] != hi.size:
        raise ValueError(f"pick_operating_points: counts_grid must be (Mw, V = {hi.size}, K, 3) (got {counts_grid.shape})")
    Mw, V, K, _ = counts_grid.shape
    if not 0 <= int(ref_index) < Mw:
        raise ValueError(f"pick_operating_points: ref_index={ref_index} lies outside the {Mw} widths")
    f = class_f1(counts_grid)                                                 # (Mw, V, K)
    at = int(np.argmin(np.abs(hi.astype(np.float64) - float(np.float32(threshold)))))
    first = np.argmax(np.where(np.isnan(f), -1.0, f).reshape(Mw * V, K), axis=0)
    none = np.isnan(f).all(axis=(0, 1))
    best_j = np.where(none, int(ref_index), first // V)
    best_v = np.where(none, -1, first % V)
    keep_hi = np.float32(threshold)
    keep_lo = np.minimum(np.maximum(np.float32(low_ratio) * keep_hi, _TINY), keep_hi).astype(np.float32)
    b_hi = np.where(best_v >= 0, hi[np.maximum(best_v, 0)], keep_hi).astype(np.float32)
    b_lo = np.where(best_v >= 0, lo[np.maximum(best_v, 0)], keep_lo).astype(np.float32)
    return at, best_j, best_v, b_hi, b_lo


def _sweep_timelines(prob, table, nsamp, R, refs, c, width_table, hi, lo, max_gap, min_len, first=0):
    """Event counts of stitched probabilities prob (K, G_total) at every median width of `width_table` (Mw, K) and every
    threshold pair -> (Mw, K, V, 2) int64 on the device, (tp, n_est) summed over the recordings of `table`: ONE
    `ops.detect_median_bank`, then one `ops.event_score` per slice on the contiguous filt[j].  The other operands are
    `ops.event_score`'s.  No host wait."""
    filt = ops.detect_median_bank(prob, table, width_table)
    return torch.stack([ops.event_score(filt[j], table, nsamp, R, refs, c, hi, lo, max_gap, min_len, first=first)
                        .sum(dim=0, dtype=torch.int64) for j in range(filt.shape[0])])


def tune_postprocessing(model, mel, bank, median_grid_ms=None, median_ms=960, thresholds=None, low_ratio=1.0,
                        min_duration_ms=0, max_gap_ms=0, collar_ms=200, offset_pct=0.2, threshold=0.5, batch_clips=256,
                        taper="triangle", clip_seconds=10.24, hop_seconds=5.12, batch_windows=64):
    """`evaluate_events` at a whole grid of median widths in one walk of the split, and the width and threshold that suit
    each class.  The widths in frames are `detection.median_frames` of every entry of median_grid_ms (default: the odd
    widths 1 .. 15 frames) plus that of median_ms (a scalar: the reference width), without repeats, ascending.  Per chunk
    of clips ONE trunk pass and stitch (`_walk_chunks`), then `_sweep_timelines`: one `ops.detect_median_bank` whose slice
    j holds width j in every class and one `ops.event_score` per slice; int64 counts accumulate on the device with one host
    wait at the end.  The remaining arguments are `evaluate_events`'s.

    -> every key of `evaluate_events(median_ms=median_ms)` (counts, grid, scores, "macro_f1_best", settings: all at the
    reference width), and: "median_frames" (Mw,) int32, "median_ms_grid" (Mw,) float64 (frames times the frame length);
    "counts_grid" (Mw, V, K, 3) int64, "class_f1_grid" (Mw, V, K); "best_median_index", "best_median_frames",
    "best_median_ms" (K,) (`pick_operating_points`); "best_threshold", "best_low_threshold", "best_index" are taken AT THE
    CHOSEN WIDTH; "macro_f1_tuned": macro F1 with each class at its width and threshold; "macro_f1_best_single" with
    "best_single_median_ms": the best macro F1 one shared width reaches with per-class thresholds (`pick_thresholds` per
    width, the narrowest of equals).  Both figures are TUNED ON THE SCORED SPLIT, an upper bound for any other, as
    "macro_f1_best" is; `score_operating_points` judges a saved choice on another split.  settings gains "frame_ms"."""
    _refuse_weak("tune_postprocessing", bank)
    n = bank["lengths"].numel()
    if n == 0:
        raise ValueError("tune_postprocessing: the split is empty")
    if np.ndim(median_ms) != 0:
        raise ValueError("tune_postprocessing: median_ms is the scalar reference width; the grid goes in median_grid_ms")
    hi, lo = threshold_grid(thresholds, low_ratio)
    V, K = hi.size, len(bank["classes"])
    refs, c, n_ref = _event_refs(bank, mel, collar_ms, offset_pct)
    frame_s = detection.frame_geometry(detection.check_model(model)[1], mel.hopsize, mel.sr, clip_seconds, hop_seconds).frame_s
    m_ref = detection.median_frames(median_ms, frame_s)
    if median_grid_ms is None:
        grid = list(range(1, 16, 2))
    else:
        grid = [detection.median_frames(v, frame_s) for v in np.asarray(median_grid_ms, dtype=np.float64).reshape(-1)]
    frames = np.asarray(sorted(set(grid + [m_ref])), dtype=np.int32)
    Mw, ref_index = frames.size, int(np.flatnonzero(frames == m_ref)[0])
    width_table = ops.median_width_table(np.repeat(frames[:, None], K, axis=1), K)

    def score(acc, prob, table, nsamp, R, d_hi, d_lo, max_gap, min_len, first):
        acc += _sweep_timelines(prob, table, nsamp, R, refs, c, width_table, d_hi, d_lo, max_gap, min_len, first).flatten()

    res, eval_s, K, _ = _walk_chunks("tune_postprocessing", model, mel, bank, hi, lo, Mw * K * V * 2, score, None, median_ms,
                                     min_duration_ms, max_gap_ms, batch_clips, taper, clip_seconds, hop_seconds, batch_windows,
                                     unfiltered=True)
    res = res.reshape(Mw, K, V, 2)
    counts_grid = np.stack([_event_counts(res[j], n_ref) for j in range(Mw)])                  # (Mw, V, K, 3)
    settings = {"median_ms": float(median_ms), "min_duration_ms": float(min_duration_ms), "max_gap_ms": float(max_gap_ms),
                "taper": taper, "window_size": float(clip_seconds), "hop_length": float(hop_seconds),
                "collar_ms": float(collar_ms), "offset_pct": float(offset_pct), "low_ratio": float(low_ratio),
                "frame_ms": 1000.0 * frame_s}
    out = _event_result(counts_grid[ref_index], hi, lo, threshold, low_ratio, n, n_ref, eval_s, settings)
    ms_grid = frames.astype(np.float64) * (1000.0 * frame_s)
    tuned = tuned_scores(counts_grid, hi, lo, threshold, ref_index, low_ratio)
    best_j, j_single = tuned["best_median_index"], tuned.pop("best_single_index")
    out.update(tuned)
    out.update({"median_frames": frames, "median_ms_grid": ms_grid, "counts_grid": counts_grid,
                "class_f1_grid": class_f1(counts_grid), "best_median_frames": frames[best_j], "best_median_ms": ms_grid[best_j],
                "best_single_median_ms": float(ms_grid[j_single])})
    return out


def tuned_scores(counts_grid, hi, lo, threshold, ref_index, low_ratio=1.0):
    """The choices and figures `tune_postprocessing` derives from counts_grid (Mw, V, K, 3), pure numpy -> {"best_median_index",
    "best_index" (K,), "best_threshold", "best_low_threshold" (K,) float32 (`pick_operating_points`); "macro_f1_tuned":
    macro F1 of the classes' counts at their chosen points (a class that keeps the reference: at the reference width and the
    grid value nearest `threshold`); "macro_f1_best_single", "best_single_index": the largest macro F1 one width reaches
    with per-class thresholds (`pick_thresholds` per width), and the narrowest width that reaches it}."""
    at, best_j, best_v, b_hi, b_lo = pick_operating_points(counts_grid, hi, lo, threshold, ref_index, low_ratio)
    counts_grid = np.asarray(counts_grid)
    cls = np.arange(counts_grid.shape[2])
    single = []
    for j in range(counts_grid.shape[0]):
        _, best, _, _ = pick_thresholds(counts_grid[j], hi, lo, threshold, low_ratio)
        single.append(segment_scores(counts_grid[j][np.where(best >= 0, best, at), cls])["macro_f1"])
    single = np.asarray(single, dtype=np.float64)
    j_single = int(np.argmax(np.where(np.isnan(single), -1.0, single)))
    return {"best_median_index": best_j, "best_index": best_v, "best_threshold": b_hi, "best_low_threshold": b_lo,
            "macro_f1_tuned": segment_scores(counts_grid[best_j, np.where(best_v >= 0, best_v, at), cls])["macro_f1"],
            "macro_f1_best_single": float(single[j_single]), "best_single_index": j_single}


def score_operating_points(model, mel, bank, doc, batch_clips=256, batch_windows=64):
    """Score a loaded operating-point file (`load_operating_points`) on a resident strong-label split: the event-based
    scores of `detect --thresholds_file` with that file, so that a choice tuned on one split can be judged on another.
    The detector's post-processing, collars and per-class thresholds are the file's; its "class_median_ms" (else its
    "median_ms") gives the widths, filtered as in `_walk_chunks` (unequal widths: one `ops.detect_median_bank` of one
    slice).  The K pairs (threshold[k], low_threshold[k]) are the grid of ONE `ops.event_score` per chunk; class k's counts
    are read at pair k.
    -> {"counts" (K, 3) int64 (tp, fp, fn), the six `segment_scores`, "n_clips", "n_ref", "eval_s"}.  On the split the
    file was tuned on, "macro_f1" is `tune_postprocessing`'s "macro_f1_tuned" exactly."""
    _refuse_weak("score_operating_points", bank)
    n = bank["lengths"].numel()
    if n == 0:
        raise ValueError("score_operating_points: the split is empty")
    K = len(bank["classes"])
    if list(doc["classes"]) != list(bank["classes"]):
        raise ValueError("score_operating_points: the operating points and the bank differ in their classes")
    scoring = doc.get("scoring") or {}
    refs, c, n_ref = _event_refs(bank, mel, scoring.get("collar_ms", 200.0), scoring.get("offset_pct", 0.2))
    median = doc["class_median_ms"] if doc.get("class_median_ms") is not None else doc["median_ms"]

    def score(acc, filt, table, nsamp, R, d_hi, d_lo, max_gap, min_len, first):
        cnt = ops.event_score(filt, table, nsamp, R, refs, c, d_hi, d_lo, max_gap, min_len, first=first)       # V = K pairs
        acc += cnt.sum(dim=0, dtype=torch.int64).diagonal(dim1=0, dim2=1).t().flatten()                       # [k, pair k]

    res, eval_s, K, _ = _walk_chunks("score_operating_points", model, mel, bank, doc["threshold"], doc["low_threshold"], K * 2,
                                     score, None, median, doc["min_duration_ms"], doc["max_gap_ms"], batch_clips, doc["taper"],
                                     doc["window_size"], doc["hop_length"], batch_windows)
    counts = _event_counts(res.reshape(K, 1, 2), n_ref)[0]
    out = {"counts": counts}
    out.update(segment_scores(counts))
    out.update({"n_clips": n, "n_ref": int(n_ref.sum()), "eval_s": eval_s})
    return out


# ---------------------------------------------------------------------------------------------------- PSDS
# The polyphonic sound detection score of Bilen et al. (ICASSP 2020), the ranking metric of DCASE Task 4: the two scenarios
# of that task as (dtc, gtc, cttc, alpha_ct, alpha_st, e_max).
PSDS_SCENARIOS = {1: {"dtc": 0.7, "gtc": 0.7, "cttc": 0.0, "alpha_ct": 0.0, "alpha_st": 1.0, "e_max": 100.0},
                  2: {"dtc": 0.1, "gtc": 0.1, "cttc": 0.3, "alpha_ct": 0.5, "alpha_st": 1.0, "e_max": 100.0}}


def psds_from_counts(tp, fp, ct, n_ref, ref_seconds, total_seconds, alpha_ct, alpha_st, e_max=100.0):
    """The PSDS curve and its integral from integer counts, in fp64 on the host.  tp, fp (V, K) per threshold and class,
    ct (V, K, K) cross-triggers [v, detection class, reference class] (None: none), n_ref (K) reference events and
    ref_seconds (K) their summed length per class, total_seconds the length of the split.

    TPR = tp / n_ref; FPR = fp per hour of the split; CTR[v, c, c'] = ct per hour of class c' references (0 where it has
    none); eFPR = FPR + alpha_ct mean over c' != c of CTR (no such term for K = 1).  Per class with references, the points
    (eFPR, TPR) sorted by eFPR, the largest TPR among equal eFPR, then the running maximum, read as a step function f_c
    (0 before the first point).  eTPR(x) = mean_c f_c(x) - alpha_st std_c f_c(x) (population std over the classes with
    references, not clipped); PSDS is the exact integral of that step function over [0, e_max], divided by e_max.  No class
    with references: NaN.
    -> {"psds", "efpr" (V, K), "tpr" (V, K) (NaN without references), "etpr_x": the breakpoints from 0 to e_max,
    "etpr_y": eTPR on the interval that starts at each}."""
    tp, fp = np.asarray(tp, dtype=np.float64), np.asarray(fp, dtype=np.float64)
    if tp.ndim != 2 or fp.shape != tp.shape:
        raise ValueError(f"psds_from_counts: tp and fp must be (V, K) (got {tp.shape}, {fp.shape})")
    V, K = tp.shape
    ct = np.zeros((V, K, K)) if ct is None else np.asarray(ct, dtype=np.float64)
    n_ref, ref_seconds = np.asarray(n_ref, dtype=np.float64), np.asarray(ref_seconds, dtype=np.float64)
    if ct.shape != (V, K, K) or n_ref.shape != (K,) or ref_seconds.shape != (K,):
        raise ValueError(f"psds_from_counts: need ct (V, K, K), n_ref (K), ref_seconds (K) for V = {V}, K = {K} "
                         f"(got {ct.shape}, {n_ref.shape}, {ref_seconds.shape})")
    total_seconds, e_max = float(total_seconds), float(e_max)
    if not total_seconds > 0 or not e_max > 0:
        raise ValueError(f"psds_from_counts: total_seconds and e_max must be positive (got {total_seconds}, {e_max})")
    with np.errstate(divide="ignore", invalid="ignore"):
        tpr = np.where(n_ref > 0, tp / n_ref, np.nan)
        ctr = np.where(ref_seconds > 0, ct / (ref_seconds / 3600.0), 0.0)     # (V, K, K'), by reference class
    efpr = fp / (total_seconds / 3600.0)
    if K > 1:
        cross = ctr.sum(axis=2) - ctr[:, np.arange(K), np.arange(K)]
        efpr = efpr + float(alpha_ct) * cross / (K - 1)
    out = {"psds": float("nan"), "efpr": efpr, "tpr": tpr, "etpr_x": np.zeros(0), "etpr_y": np.zeros(0)}
    scored = np.flatnonzero(n_ref > 0)
    if scored.size == 0:
        return out
    curves = []
    for c in scored:
        order = np.lexsort((-tpr[:, c], efpr[:, c]))                          # by x, the largest y of equal x first
        x, y = efpr[order, c], tpr[order, c]
        first = np.concatenate([[True], x[1:] != x[:-1]])
        curves.append((x[first], np.maximum.accumulate(y[first])))
    inside = [x[(x >= 0) & (x <= e_max)] for x, _ in curves]
    bx = np.unique(np.concatenate(inside + [np.asarray([0.0, e_max])]))
    f = np.zeros((len(curves), bx.size))
    for j, (x, y) in enumerate(curves):
        at = np.searchsorted(x, bx, side="right") - 1                         # the last point with x_j <= x
        f[j] = np.where(at >= 0, y[np.maximum(at, 0)], 0.0)
    etpr = f.mean(axis=0) - float(alpha_st) * f.std(axis=0)
    out.update(psds=float(np.sum(etpr[:-1] * np.diff(bx)) / e_max), etpr_x=bx, etpr_y=etpr)
    return out


def evaluate_psds(model, mel, bank, scenario=1, dtc=None, gtc=None, cttc=None, alpha_ct=None, alpha_st=None, e_max=100.0,
                  thresholds=None, low_ratio=1.0, median_ms=960, min_duration_ms=0, max_gap_ms=0, batch_clips=256,
                  taper="triangle", clip_seconds=10.24, hop_seconds=5.12, batch_windows=64):
    """PSDS of what `detection.EADetector(model=model).detect` lists on a resident strong-label split: the operating points
    are the grid `threshold_grid(thresholds, low_ratio)`, all counted at once.

    The chunk walk of `evaluate_events` (`_walk_chunks`) with ONE `ops.psds_count` per chunk (include/eat_psds.h: detection
    and ground-truth intersection criteria dtc / gtc, cross-trigger criterion cttc); int64 counts accumulate on the device,
    the cross-triggers in the same buffer, with one host wait at the end; `psds_from_counts` then integrates the curve.
    `scenario` (1 or 2) picks a row of `PSDS_SCENARIOS`; dtc, gtc, cttc, alpha_ct, alpha_st given explicitly override it
    (e_max is the argument's).  This restates the definitions of the psds_eval package in integer samples; no run of that
    package stands behind it.

    -> {"thresholds", "low_thresholds" (V,) float32; "counts" (V, K, 3) int64 (tp, fp, fn); "n_det" (V, K); "ct" (V, K, K)
    int64; "psds", "efpr", "tpr", "etpr_x", "etpr_y" of `psds_from_counts`; "n_ref", "ref_seconds" (K,); "total_seconds";
    "n_clips", "eval_s", "settings"}.  median_ms is a scalar or one value per class, with the settings entries of
    `evaluate_events`."""
    if scenario not in PSDS_SCENARIOS:
        raise ValueError(f"evaluate_psds: scenario must be one of {sorted(PSDS_SCENARIOS)} (got {scenario!r})")
    st = dict(PSDS_SCENARIOS[scenario])
    st["e_max"] = float(e_max)
    for name, val in (("dtc", dtc), ("gtc", gtc), ("cttc", cttc), ("alpha_ct", alpha_ct), ("alpha_st", alpha_st)):
        if val is not None:
            st[name] = float(val)
    for name in ("dtc", "gtc", "cttc"):
        ops.per_mille(name, st[name], 0 if name == "cttc" else 1)
    _refuse_weak("evaluate_psds", bank)
    n = bank["lengths"].numel()
    if n == 0:
        raise ValueError("evaluate_psds: the split is empty")
    hi, lo = threshold_grid(thresholds, low_ratio)
    V, K = hi.size, len(bank["classes"])
    events_cpu = bank["events"].cpu()
    refs = ops.event_refs(events_cpu, torch.zeros(events_cpu.shape[0], dtype=torch.int32), bank["event_offsets"].cpu(), K)
    ev = events_cpu.numpy().astype(np.int64)
    n_ref = np.bincount(ev[:, 0], minlength=K).astype(np.int64)
    ref_seconds = np.bincount(ev[:, 0], weights=(ev[:, 2] - ev[:, 1]).astype(np.float64), minlength=K) / float(mel.sr)
    total_seconds = float(bank["lengths_cpu"].to(torch.int64).sum()) / float(mel.sr)
    cross = [None]                                                            # (V, K, K) int32, added to by every chunk

    def score(acc, filt, table, nsamp, R, d_hi, d_lo, max_gap, min_len, first):
        cnt, cross[0] = ops.psds_count(filt, table, nsamp, R, refs, st["dtc"], st["gtc"], st["cttc"], d_hi, d_lo, max_gap,
                                       min_len, first=first, ct=cross[0])
        acc[:K * V * 4] += cnt.sum(dim=0, dtype=torch.int64).flatten()

    def finish(acc):
        if cross[0] is not None:
            acc[K * V * 4:] = cross[0].flatten()

    res, eval_s, K, _ = _walk_chunks("evaluate_psds", model, mel, bank, hi, lo, K * V * 4 + V * K * K, score, finish, median_ms,
                                     min_duration_ms, max_gap_ms, batch_clips, taper, clip_seconds, hop_seconds, batch_windows)
    per = res[:K * V * 4].reshape(K, V, 4).transpose(1, 0, 2)                 # (V, K, 4): tp, n_det, fp, n_ct
    ct = res[K * V * 4:].reshape(V, K, K).astype(np.int64)
    tp, fp = per[:, :, 0], per[:, :, 2]
    out = {"thresholds": hi, "low_thresholds": lo,
           "counts": np.stack([tp, fp, n_ref[None, :] - tp], axis=2).astype(np.int64), "n_det": per[:, :, 1].astype(np.int64),
           "ct": ct}
    out.update(psds_from_counts(tp, fp, ct, n_ref, ref_seconds, total_seconds, st["alpha_ct"], st["alpha_st"], st["e_max"]))
    settings = {"scenario": scenario}
    settings.update(_median_settings(median_ms))
    settings.update({"min_duration_ms": float(min_duration_ms), "max_gap_ms": float(max_gap_ms), "taper": taper,
                     "window_size": float(clip_seconds), "hop_length": float(hop_seconds), "low_ratio": float(low_ratio)})
    settings.update(st)
    out.update({"n_ref": n_ref, "ref_seconds": ref_seconds, "total_seconds": total_seconds, "n_clips": n, "eval_s": eval_s,
                "settings": settings})
    return out


# ---- operating points: the per-class thresholds and the post-processing they were tuned with, for `detect --thresholds_file`
_OP_POST = ("median_ms", "min_duration_ms", "max_gap_ms", "taper", "window_size", "hop_length")


def save_operating_points(path, result, classes):
    """Write the per-class operating points of an `evaluate_events` result as JSON: classes, threshold (K), low_threshold (K),
    median_ms, min_duration_ms, max_gap_ms, taper, window_size, hop_length (seconds, `detect`'s flags), and under "scoring" /
    "scores" the settings and the scores they came from.  A `tune_postprocessing` result (one with "best_median_ms") also
    writes class_median_ms (K floats: the chosen width per class, which `detect` prefers to median_ms), frame_ms and the
    tuned scores."""
    classes = list(classes)
    hi, lo = np.asarray(result["best_threshold"], dtype=np.float32), np.asarray(result["best_low_threshold"], dtype=np.float32)
    if hi.shape != (len(classes),) or lo.shape != hi.shape:
        raise ValueError(f"save_operating_points: {len(classes)} classes, thresholds of shape {hi.shape} / {lo.shape}")
    st = result["settings"]
    doc = {"classes": classes, "threshold": [float(v) for v in hi], "low_threshold": [float(v) for v in lo]}
    doc.update({k: st[k] for k in _OP_POST})
    doc["scoring"] = {"collar_ms": st["collar_ms"], "offset_pct": st["offset_pct"], "low_ratio": st["low_ratio"],
                      "reference_threshold": result["threshold"], "n_clips": result["n_clips"], "n_ref": result["n_ref"],
                      "grid": [float(v) for v in result["thresholds"]]}
    doc["scores"] = {"macro_f1_best": result["macro_f1_best"]}
    doc["scores"].update({k: result[k] for k in SCORE_NAMES})
    if "best_median_ms" in result:
        ms = np.asarray(result["best_median_ms"], dtype=np.float64)
        if ms.shape != (len(classes),):
            raise ValueError(f"save_operating_points: {len(classes)} classes, best_median_ms of shape {ms.shape}")
        doc["class_median_ms"] = [float(v) for v in ms]
        doc["frame_ms"] = st["frame_ms"]
        doc["scores"].update({k: result[k] for k in ("macro_f1_tuned", "macro_f1_best_single", "best_single_median_ms")})
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return doc


def load_operating_points(path, classes=None, n_classes=None):
    """Read an operating-point file -> its dict with threshold / low_threshold as (K,) float32 arrays.  classes: the class
    names, in order, that the file must hold; n_classes: the class count it must hold.  A missing field, a wrong length,
    another class order, thresholds outside 0 < low_threshold <= threshold <= 1 or an unknown taper: ValueError naming the
    file.  class_median_ms is optional: a file without it loads as ever; with it, it comes back as a (K,) float64 array and
    must hold K finite values that are each a legal median width in frames of the file's frame_ms (320 when absent)."""
    what = f"operating points at {path}"
    try:
        with open(path) as f:
            doc = json.load(f)
    except (OSError, ValueError) as e:
        raise ValueError(f"{what}: not readable as JSON ({e})") from None
    if not isinstance(doc, dict):
        raise ValueError(f"{what}: the file must hold one JSON object")
    missing = [k for k in ("classes", "threshold", "low_threshold") + _OP_POST if k not in doc]
    if missing:
        raise ValueError(f"{what}: missing {', '.join(missing)}")
    names = doc["classes"]
    if not isinstance(names, list) or len(names) < 1 or not all(isinstance(c, str) for c in names):
        raise ValueError(f"{what}: classes must be a list of K >= 1 names")
    K = len(names)
    if n_classes is not None and K != int(n_classes):
        raise ValueError(f"{what}: the file holds {K} classes, {int(n_classes)} are expected")
    if classes is not None and list(classes) != names:
        raise ValueError(f"{what}: the file's classes {names[:4]}{'...' if K > 4 else ''} are not the expected names in "
                         f"their order")
    try:
        hi, lo = (np.asarray(doc[k], dtype=np.float32) for k in ("threshold", "low_threshold"))
        post = {k: float(doc[k]) for k in _OP_POST if k != "taper"}
    except (TypeError, ValueError):
        raise ValueError(f"{what}: thresholds and post-processing values must be numbers") from None
    if hi.shape != (K,) or lo.shape != (K,):
        raise ValueError(f"{what}: threshold and low_threshold must hold K = {K} values (got {hi.shape}, {lo.shape})")
    if not bool(((lo > 0) & (lo <= hi) & (hi <= 1)).all()):
        raise ValueError(f"{what}: thresholds need 0 < low_threshold <= threshold <= 1 in every class")
    if doc["taper"] not in ("triangle", "uniform"):
        raise ValueError(f"{what}: taper must be 'triangle' or 'uniform' (got {doc['taper']!r})")
    if not all(np.isfinite(v) and v >= 0 for v in post.values()):
        raise ValueError(f"{what}: post-processing values must be finite and not negative")
    out = dict(doc)
    out.update(post)
    out.update(threshold=hi, low_threshold=lo)
    if "class_median_ms" in doc:                             # optional: the per-class widths of `tune_postprocessing`
        try:
            ms = np.asarray(doc["class_median_ms"], dtype=np.float64)
            frame_ms = float(doc.get("frame_ms", 320.0))
        except (TypeError, ValueError):
            raise ValueError(f"{what}: class_median_ms and frame_ms must be numbers") from None
        if ms.shape != (K,):
            raise ValueError(f"{what}: class_median_ms must hold K = {K} values (got shape {ms.shape})")
        if not np.isfinite(frame_ms) or frame_ms <= 0:
            raise ValueError(f"{what}: frame_ms must be finite and positive")
        try:
            detection.median_frames_per_class(ms, frame_ms / 1000.0, K)
        except ValueError as e:
            raise ValueError(f"{what}: class_median_ms: {e}") from None
        out.update(class_median_ms=ms, frame_ms=frame_ms)
    return out
