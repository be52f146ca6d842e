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

and kept on the GPU (`load_bank`) as the ragged bank `ops.wave_augment_ragged` takes, plus the event table.  A training
step draws the FSD50K augmentation (`draw_augment` IS `fsd50k.draw_augment`), builds the waveforms with
`ops.wave_augment_ragged` and - from the same tables - the frame targets with `ops.sed_targets`, so an event follows its
clip through crop, pad, roll and wave-mix; the model's frame logits (`mn_train.forward_train_frames`) meet them in the fused
frame BCE (`frame_bce_loss`).  One frame is one column of the trunk's last feature map: R = r hopsize samples (10240 =
0.32 s at the default geometry), frame t of a window owns its samples [t R, (t + 1) R).  A clip is L = T R samples, a whole
number of frames; the default 327680 is `EADetector`'s 10.24 s window, 32 frames.

`evaluate_frames` tiles every clip of a split with non-overlapping windows and scores the eval frame logits
(`detection.frame_logits`) against the events: frame-level mAP / ROC and segment-based F1 with one frame as the segment.
The fine-tuned model keeps the reference's state-dict layout (an mlp-head MN with K classes), so its checkpoint loads
straight into `EADetector(model=...)` and `detect --checkpoint`.  Only MN models with the mlp head on the monolithic plan.
"""
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
    event_offsets (N + 1) int64 on the device and classes (K names).  Every violation of the format is a ValueError naming
    the file."""
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

    dev = torch.device("cpu") if device is None else device
    return dict(fsd50k.resident_waves(waves, lengths, dev), bank_y=torch.from_numpy(weak).to(dev), names=names, classes=classes,
                events=torch.from_numpy(np.ascontiguousarray(events)).to(dev), event_offsets=torch.from_numpy(eo).to(dev))


def frame_bce_loss(logits, y, T, perm=None, lam=None, sums=None):
    """Mean over (b, c, t < T) of BCE-with-logits(z, lam y + (1 - lam) y[perm]) of frame logits (B, K, Tp) against frame
    targets y (B, K, Tp), as a device scalar that supports .backward() (include/eat_sed.h: eat_frame_bce_fwd_bwd); `sums`
    (1,) accumulates it across calls."""
    if sums is None:
        sums = torch.zeros(1, device=logits.device, dtype=torch.float64)
    y = y.contiguous().float()
    return FusedLoss.apply(logits, sums, 1, lambda z, step: ops.frame_bce_fwd_bwd(z, y, T, perm, lam, sums=step)[0])


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
        dev, B = bank["waves"].device, int(batch_size)
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
