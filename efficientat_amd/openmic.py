"""OpenMIC-2018 on the device: a decoded split as a resident clip bank, and the host draws of its augmentations.

The reference (datasets/openmic.py) keeps each split in an HDF5 file of mp3 bytes and decodes a clip per item in DataLoader
workers: gain, pad / truncate to 10 s, roll (datasets/helpers/audiodatasets.py) and `MixupDataset`'s wave-mix.  Every clip
carries 40 numbers: 20 instrument labels, then 20 "this label was annotated" mask entries.  Here a split is decoded once
(tools/openmic_to_bank.py) into a directory

    waves.npy    (N, L) int16 (input_pipeline.I16_SCALE = 32767 per unit) or float32, clips padded / truncated to L samples
    targets.npy  (N, 40) float32, as stored in the HDF5 `target` rows
    names.txt    N lines, the `audio_name` rows

and kept on the GPU (`load_bank`); the augmentation runs on the device (`ops.wave_augment` for the waveforms,
`ops.openmic_targets` for the label rows) from a few hundred bytes of host draws per batch, made by `draw_augment` in the
reference's order - which is not ESC-50's.
"""
import os

import numpy as np
import torch

from .esc50 import _gain_and_roll
from .input_pipeline import I16_SCALE

N_CLASSES = 20
CLIP_SECONDS = 10


def load_bank(path, device=None):
    """A decoded split (see the module header) -> dict(bank (N, L) fp32, bank_mean (N) fp64, bank_y (N, 40) fp32, names).
    On `device` when given, else on the CPU.  waves.npy is memory-mapped while loading and converted in slices, so the host
    never holds a second fp32 copy.  The training split (14 915 clips of 10 s at 32 kHz) is about 19 GB as fp32, which fits in
    HBM next to the model; int16 on disk halves the file, not the resident bank."""
    waves = np.load(os.path.join(path, "waves.npy"), mmap_mode="r")
    targets = np.load(os.path.join(path, "targets.npy"))
    with open(os.path.join(path, "names.txt")) as f:
        names = f.read().splitlines()
    if waves.ndim != 2 or waves.dtype not in (np.int16, np.float32):
        raise ValueError(f"OpenMIC bank at {path}: waves.npy must be (N, L) int16 or float32, got {waves.dtype} {waves.shape}")
    n = waves.shape[0]
    if targets.ndim != 2 or targets.shape[1] != 2 * N_CLASSES:
        raise ValueError(f"OpenMIC bank at {path}: targets.npy must be (N, {2 * N_CLASSES}), got {targets.shape}")
    if targets.shape[0] != n or len(names) != n or n == 0:
        raise ValueError(f"OpenMIC bank at {path}: {n} waveforms, {targets.shape[0]} target rows and {len(names)} names")
    dev = torch.device("cpu") if device is None else device
    bank = torch.empty(waves.shape, dtype=torch.float32, device=dev)
    mean = torch.empty(n, dtype=torch.float64, device=dev)
    rows = max(1, (1 << 26) // waves.shape[1])                                 # 256 MB of fp32 per slice
    for s in range(0, n, rows):
        x = torch.from_numpy(np.array(waves[s:s + rows]))                      # (a copy: the map is read-only)
        x = x.float() / I16_SCALE if x.dtype == torch.int16 else x
        bank[s:s + rows] = x
        mean[s:s + rows] = x.double().mean(1)
    return dict(bank=bank, bank_mean=mean, bank_y=torch.from_numpy(targets.astype(np.float32)).to(dev), names=names)


def draw_augment(indices, n_bank, gain_augment=12, roll=True, wavmix=True, shift_range=4000, beta=2.0, rate=0.5):
    """Host draws of one batch, per sample in the order of OpenMIC's MixupDataset.__getitem__ (datasets/openmic.py:74-81): the
    clip is fetched FIRST - its gain (torch) and its roll (numpy) - and only then torch.rand(1) < rate decides the wave-mix;
    a mixed sample goes on with the partner torch.randint(n_bank), its gain and roll, and l = max(b, 1 - b), b ~
    np.random.beta(beta, beta).  (ESC-50's MixupDataset draws torch.rand first: esc50.draw_augment.)  -> the four tables of
    `esc50.draw_augment`: (idx (2B) int32, shift (2B) int32, amp (2B) fp32, mix (B) fp32) CPU tensors."""
    indices = [int(i) for i in indices]
    B = len(indices)
    idx = torch.full((2 * B,), -1, dtype=torch.int32)
    shift = torch.zeros(2 * B, dtype=torch.int32)
    amp = torch.ones(2 * B, dtype=torch.float32)
    mix = torch.ones(B, dtype=torch.float32)
    for i, index in enumerate(indices):
        idx[2 * i] = index
        amp[2 * i], shift[2 * i] = _gain_and_roll(gain_augment, roll, shift_range)
        if wavmix and bool(torch.rand(1) < rate):
            idx[2 * i + 1] = torch.randint(n_bank, (1,)).item()
            amp[2 * i + 1], shift[2 * i + 1] = _gain_and_roll(gain_augment, roll, shift_range)
            b = np.random.beta(beta, beta)
            mix[i] = max(b, 1.0 - b)
    return idx, shift, amp, mix
