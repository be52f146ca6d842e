"""FSD50K on the device: a decoded split as a RAGGED resident clip bank, and the host draws of its augmentations.

The reference (datasets/fsd50k.py) keeps each split in an HDF5 file of mp3 bytes and decodes a clip per item in DataLoader
workers: gain, then pad to 10 s or - for a longer clip - a random 10 s window redrawn on every fetch, roll
(datasets/helpers/audiodatasets.py) and `MixupDataset`'s wave-mix, which subtracts the mean of that window.  Clips run from
0.3 s to 30 s, so a rectangle of padded rows would hold mostly zeros (and a rectangle of cut rows would freeze the crop).
Here a split is decoded once (tools/fsd50k_to_bank.py) into a directory

    waves.npy    (S,) int16 (input_pipeline.I16_SCALE = 32767 per unit) or float32: the clips back to back, at 32 kHz
    lengths.npy  (N,) int64 samples per clip, sum = S
    targets.npy  (N, 200) uint8 or float32 multi-hot labels
    names.txt    N lines, the `audio_name` rows

and kept on the GPU (`load_bank`) as one flat buffer plus offsets and lengths; `ops.wave_augment_ragged` builds a training
batch from it on the device from a few hundred bytes of host draws, made by `draw_augment` in the reference's order.  Only
32 kHz is supported: at 16 / 8 kHz the reference decimates AFTER cropping 10 s of 32 kHz audio, which is not reproduced.
"""
import os

import numpy as np
import torch

from .input_pipeline import I16_SCALE

N_CLASSES = 200
CLIP_SECONDS = 10
SAMPLE_RATE = 32000


def read_waves(path, what):
    """waves.npy (memory-mapped) and lengths.npy of a bank directory, checked -> (waves (S,) int16 / float32, lengths (N,)
    int64); `what` names the bank in the ValueError of a violation."""
    waves = np.load(os.path.join(path, "waves.npy"), mmap_mode="r")
    lengths = np.load(os.path.join(path, "lengths.npy"))
    if waves.ndim != 1 or waves.dtype not in (np.int16, np.float32):
        raise ValueError(f"{what}: waves.npy must be (S,) int16 or float32, got {waves.dtype} {waves.shape}")
    if lengths.ndim != 1 or lengths.dtype.kind not in "iu":
        raise ValueError(f"{what}: lengths.npy must be (N,) integers, got {lengths.dtype} {lengths.shape}")
    n = lengths.shape[0]
    lengths = lengths.astype(np.int64)
    if n == 0 or lengths.min() < 1 or lengths.max() >= 2 ** 31 or int(lengths.sum()) != waves.shape[0]:
        raise ValueError(f"{what}: lengths.npy holds {n} lengths (each must be in [1, 2^31)) summing to "
                         f"{int(lengths.sum()) if n else 0} for {waves.shape[0]} samples")
    return waves, lengths


def resident_waves(waves, lengths, dev):
    """The sample side of a ragged bank on `dev` from `read_waves`' pair -> dict(waves (S) fp32, offsets (N) int64, lengths (N)
    int32, clip_sum (N) fp64 on `dev`, lengths_cpu (N) int64)."""
    n = lengths.shape[0]
    offsets = np.concatenate(([0], np.cumsum(lengths)[:-1])).astype(np.int64)
    S = waves.shape[0]
    flat = torch.empty(S, dtype=torch.float32, device=dev)
    # per-clip fp64 sums from the slices: the prefix sum of a slice, differenced at the clip boundaries that fall inside it,
    # would lose digits on 8e9 samples - each clip is summed on its own instead, piece by piece where it straddles slices
    clip_sum = np.zeros(n, dtype=np.float64)
    step = 1 << 26                                                             # 256 MB of fp32 per slice
    ends = offsets + lengths
    for s in range(0, S, step):
        e = min(S, s + step)
        x = torch.from_numpy(np.array(waves[s:e]))                             # (a copy: the map is read-only)
        x = x.float() / I16_SCALE if x.dtype == torch.int16 else x
        flat[s:e] = x
        xd = x.double()
        first = int(np.searchsorted(ends, s, side="right"))
        last = int(np.searchsorted(offsets, e, side="left"))
        for i in range(first, last):
            clip_sum[i] += float(xd[max(offsets[i], s) - s:min(ends[i], e) - s].sum())
    return dict(waves=flat, offsets=torch.from_numpy(offsets).to(dev), lengths=torch.from_numpy(lengths.astype(np.int32)).to(dev),
                clip_sum=torch.from_numpy(clip_sum).to(dev), lengths_cpu=torch.from_numpy(lengths))


def load_bank(path, device=None):
    """A decoded split (see the module header) -> dict(waves (S) fp32, offsets (N) int64, lengths (N) int32, clip_sum (N)
    fp64, bank_y (N, 200) fp32 on `device` when given, else on the CPU; lengths_cpu (N) int64 CPU, names).  offsets =
    the exclusive cumulative sum of lengths; clip_sum[i] = the fp64 sum of clip i's fp32 samples.  waves.npy is memory-mapped
    while loading and converted in slices, so the host never holds a second fp32 copy.  The training split (about 37 k clips,
    8e9 samples) is about 32 GB as fp32; int16 on disk halves the file, not the resident bank."""
    waves, lengths = read_waves(path, f"FSD50K bank at {path}")
    n = lengths.shape[0]
    targets = np.load(os.path.join(path, "targets.npy"))
    with open(os.path.join(path, "names.txt")) as f:
        names = f.read().splitlines()
    if targets.ndim != 2 or targets.shape[1] != N_CLASSES or targets.dtype not in (np.uint8, np.float32):
        raise ValueError(f"FSD50K bank at {path}: targets.npy must be (N, {N_CLASSES}) uint8 or float32, got {targets.dtype} "
                         f"{targets.shape}")
    if targets.shape[0] != n or len(names) != n:
        raise ValueError(f"FSD50K bank at {path}: {n} lengths, {targets.shape[0]} target rows and {len(names)} names")
    dev = torch.device("cpu") if device is None else device
    return dict(resident_waves(waves, lengths, dev), bank_y=torch.from_numpy(targets.astype(np.float32)).to(dev), names=names)


def _fetch(length, L, gain_augment, roll, shift_range):
    """One clip's draws in the order of AudioSetDataset.__getitem__ (datasets/fsd50k.py:147-149) under PreprocessDataset:
    the gain (torch.randint(2 g), only if g), the crop offset (torch.randint(0, len - L + 1), ONLY for a clip longer than L:
    pad_or_truncate draws nothing for one that fits), then the roll (numpy) -> (amp, start, shift)."""
    amp = 1.0
    if gain_augment:
        gain = torch.randint(gain_augment * 2, (1,)).item() - gain_augment
        amp = 10 ** (gain / 20)
    start = torch.randint(0, length - L + 1, (1,)).item() if length > L else 0
    shift = int(np.random.randint(-shift_range, shift_range + 1)) if roll else 0
    return amp, start, shift


def draw_augment(indices, lengths_cpu, L, gain_augment=12, roll=True, wavmix=True, shift_range=4000, beta=2.0, rate=0.5):
    """Host draws of one batch, per sample in the order of FSD50K's MixupDataset.__getitem__ (datasets/fsd50k.py:80-92):
    torch.rand(1) < rate FIRST (ESC-50's order, not OpenMIC's), the clip's fetch (`_fetch`: gain, crop, roll), and for a mixed
    sample the partner torch.randint(N), its fetch, then l = max(b, 1 - b), b ~ np.random.beta(beta, beta).
    -> (idx (2B) int32, start (2B) int32, shift (2B) int32, amp (2B) fp32, mix (B) fp32) CPU tensors, the tables of
    `ops.wave_augment_ragged` (idx[2i + 1] = -1: no wave-mix)."""
    indices = [int(i) for i in indices]
    lengths = [int(v) for v in torch.as_tensor(lengths_cpu).tolist()]
    B, n_bank = len(indices), len(lengths)
    idx = torch.full((2 * B,), -1, dtype=torch.int32)
    start = torch.zeros(2 * B, dtype=torch.int32)
    shift = torch.zeros(2 * B, dtype=torch.int32)
    amp = torch.ones(2 * B, dtype=torch.float32)
    mix = torch.ones(B, dtype=torch.float32)
    for i, index in enumerate(indices):
        mixing = bool(torch.rand(1) < rate) if wavmix else False
        idx[2 * i] = index
        amp[2 * i], start[2 * i], shift[2 * i] = _fetch(lengths[index], L, gain_augment, roll, shift_range)
        if mixing:
            j = torch.randint(n_bank, (1,)).item()
            idx[2 * i + 1] = j
            amp[2 * i + 1], start[2 * i + 1], shift[2 * i + 1] = _fetch(lengths[j], L, gain_augment, roll, shift_range)
            b = np.random.beta(beta, beta)
            mix[i] = max(b, 1.0 - b)
    return idx, start, shift, amp, mix


def draw_eval_crops(lengths_cpu, L):
    """The crop offsets of a fixed-length evaluation pass: the reference's validation / evaluation sets keep clip_length = 10
    (get_base_valid_set), so pad_or_truncate crops a long clip at RANDOM there too - torch.randint(0, len - L + 1) per long
    clip, in bank order (a sequential DataLoader without workers) -> start (N) int32, 0 for a clip that fits."""
    lengths = [int(v) for v in torch.as_tensor(lengths_cpu).tolist()]
    return torch.tensor([torch.randint(0, n - L + 1, (1,)).item() if n > L else 0 for n in lengths], dtype=torch.int32)
