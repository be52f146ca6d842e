"""ESC-50 on the device: the reader of `datasets/esc50.py` as a resident clip bank, and the host draws of its augmentations.

The reference reads `meta/esc50.csv` (filename, fold, target) with pandas, decodes `audio_32k/<filename>` with librosa per
item in DataLoader workers, applies the gain, pads / truncates to 5 s, rolls (datasets/helpers/audiodatasets.py) and mixes
waveforms (`MixupDataset`).  Here the whole split is decoded once (`audio_io.load_audio`: the same decode + resample
contract), padded / truncated, and kept on the GPU as `(bank, bank_mean, bank_cls)`; the augmentation runs on the device
(`ops.wave_augment`) from a few hundred bytes of host draws per batch made by `draw_augment` in the reference's order.
"""
import csv
import os

import numpy as np
import torch

N_CLASSES = 50
CLIP_SECONDS = 5


def read_meta(data_dir):
    """meta/esc50.csv -> list of (filename, fold, target)."""
    with open(os.path.join(data_dir, "meta", "esc50.csv"), newline="") as f:
        return [(r["filename"], int(r["fold"]), int(r["target"])) for r in csv.DictReader(f)]


def audio_dir(data_dir):
    """`audio_32k/` (the reference's pre-resampled copy) if present, else the 44.1 kHz release's `audio/`."""
    for sub in ("audio_32k", "audio"):
        p = os.path.join(data_dir, sub)
        if os.path.isdir(p):
            return p
    raise FileNotFoundError(f"{data_dir} holds neither audio_32k/ nor audio/")


def pad_or_truncate(x, length):
    """datasets/esc50.py:35-40."""
    if len(x) <= length:
        return np.concatenate((x, np.zeros(length - len(x), dtype=np.float32)), axis=0)
    return x[:length]


def load_split(data_dir, fold, train, sr=32000, clip_seconds=CLIP_SECONDS, device=None, n_classes=N_CLASSES):
    """The clips of one split (train: every fold but `fold`; test: `fold`, datasets/esc50.py:72-80) in csv order ->
    dict(bank (N, L) fp32, bank_mean (N) fp64, bank_cls (N) int32, names).  On `device` when given, else on the CPU."""
    from .audio_io import load_audio
    meta = read_meta(data_dir)
    rows = [r for r in meta if (r[1] != fold) == bool(train)]
    if not rows:
        raise ValueError(f"ESC-50 at {data_dir}: no clips for fold {fold} ({'train' if train else 'test'} split)")
    adir = audio_dir(data_dir)
    L = int(clip_seconds * sr)
    bank = np.empty((len(rows), L), dtype=np.float32)
    for i, (name, _, _) in enumerate(rows):
        wave, _ = load_audio(os.path.join(adir, name), sr=sr, mono=True)
        bank[i] = pad_or_truncate(wave, L)
    cls = np.array([r[2] for r in rows], dtype=np.int32)
    if cls.min() < 0 or cls.max() >= n_classes:
        raise ValueError(f"ESC-50 at {data_dir}: a target lies outside [0, {n_classes})")
    out = dict(bank=torch.from_numpy(bank), bank_mean=torch.from_numpy(bank.astype(np.float64).mean(axis=1)),
               bank_cls=torch.from_numpy(cls), names=[r[0] for r in rows])
    if device is not None:
        for k in ("bank", "bank_mean", "bank_cls"):
            out[k] = out[k].to(device)
    return out


def _gain_and_roll(gain_augment, roll, shift_range):
    """One clip's draws in the reference's order: gain in the base dataset (datasets/esc50.py:43-48, torch), then the roll of
    PreprocessDataset (audiodatasets.py:29-37, numpy: randint(-r, r + 1) is the deprecated random_integers(-r, r))."""
    amp = 1.0
    if gain_augment:
        gain = torch.randint(gain_augment * 2, (1,)).item() - gain_augment
        amp = 10 ** (gain / 20)
    shift = int(np.random.randint(-shift_range, shift_range + 1)) if roll else 0
    return amp, shift


def draw_augment(indices, n_bank, gain_augment=12, roll=True, wavmix=True, shift_range=4000, beta=2.0, rate=0.5):
    """Host draws of one batch, per sample in MixupDataset.__getitem__'s order (datasets/esc50.py:58-71): torch.rand(1) < rate
    decides wave-mix; the clip's gain and shift; for a mixed sample the partner torch.randint(n_bank), its gain and shift, then
    l = max(b, 1 - b), b ~ np.random.beta(beta, beta).  -> (idx (2B) int32, shift (2B) int32, amp (2B) fp32, mix (B) fp32)
    CPU tensors, the tables of `ops.wave_augment` (idx[2i + 1] = -1: no wave-mix)."""
    indices = [int(i) for i in indices]
    B = len(indices)
    idx = torch.full((2 * B,), -1, dtype=torch.int32)
    shift = torch.zeros(2 * B, dtype=torch.int32)
    amp = torch.ones(2 * B, dtype=torch.float32)
    mix = torch.ones(B, dtype=torch.float32)
    for i, index in enumerate(indices):
        mixing = bool(torch.rand(1) < rate) if wavmix else False
        idx[2 * i] = index
        amp[2 * i], shift[2 * i] = _gain_and_roll(gain_augment, roll, shift_range)
        if mixing:
            idx[2 * i + 1] = torch.randint(n_bank, (1,)).item()
            amp[2 * i + 1], shift[2 * i + 1] = _gain_and_roll(gain_augment, roll, shift_range)
            b = np.random.beta(beta, beta)
            mix[i] = max(b, 1.0 - b)
    return idx, shift, amp, mix
