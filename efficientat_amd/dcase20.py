"""TAU Urban Acoustic Scenes 2020 Mobile (DCASE20 task 1A) on the device: the reader of `datasets/dcase20.py`, a decoded
split as a resident clip bank, and the host draws of its augmentations.

The reference reads `meta.csv` (tab-separated: filename, scene_label, identifier, source_label) with pandas, encodes scene,
recording device (source_label) and city (the identifier up to its first "-") with sklearn's LabelEncoder over the WHOLE
file, selects the rows of `evaluation_setup/fold1_train.csv` / `fold1_evaluate.csv` in meta order, and decodes a clip per
item in DataLoader workers: roll, gain (datasets/helpers/audiodatasets.py) and `MixupDataset`'s wave-mix.  Here a split is
decoded once (tools/dcase20_to_bank.py) into a directory

    waves.npy     (N, L) int16 (input_pipeline.I16_SCALE = 32767 per unit) or float32, 10 s clips
    labels.npy    (N, 3) int32: scene, device, city, encoded as above
    names.txt     N lines, the `filename` column
    classes.json  {"scene": [...], "device": [...], "city": [...]}: the three label lists, index = code

and kept on the GPU (`load_bank`); the augmentation runs on the device (`ops.wave_augment`, then `ops.freq_mixstyle` on the
log-mel) from a few hundred bytes of host draws per batch, made by `draw_augment` / `draw_mixstyle` in the reference's
order - which is neither ESC-50's nor OpenMIC's.
"""
import csv
import json
import os

import numpy as np
import torch

from .input_pipeline import I16_SCALE

N_CLASSES = 10
CLIP_SECONDS = 10
KINDS = ("scene", "device", "city")


def read_meta(data_dir):
    """meta.csv -> (rows, encoders): rows = list of (filename, scene, device, city) codes in file order; encoders = {"scene",
    "device", "city"} -> the sorted unique labels of the whole file (LabelEncoder.fit_transform, datasets/dcase20.py:36-40)."""
    with open(os.path.join(data_dir, "meta.csv"), newline="") as f:
        raw = [(r["filename"], r["scene_label"], r["source_label"], r["identifier"].split("-")[0])
               for r in csv.DictReader(f, delimiter="\t")]
    if not raw:
        raise ValueError(f"DCASE20 at {data_dir}: meta.csv lists no clip")
    encoders = {k: sorted({r[1 + i] for r in raw}) for i, k in enumerate(KINDS)}
    code = {k: {name: j for j, name in enumerate(v)} for k, v in encoders.items()}
    rows = [(r[0], code["scene"][r[1]], code["device"][r[2]], code["city"][r[3]]) for r in raw]
    return rows, encoders


def split_rows(data_dir, train):
    """The meta rows of one split IN META ORDER (meta[meta.filename.isin(files)].index, datasets/dcase20.py:140-159) ->
    (rows, encoders) as `read_meta`."""
    rows, encoders = read_meta(data_dir)
    name = "fold1_train.csv" if train else "fold1_evaluate.csv"
    with open(os.path.join(data_dir, "evaluation_setup", name), newline="") as f:
        files = {r["filename"] for r in csv.DictReader(f, delimiter="\t")}
    return [r for r in rows if r[0] in files], encoders


def load_bank(path, device=None):
    """A decoded split (see the module header) -> dict(bank (N, L) fp32, bank_mean (N) fp64, bank_cls / bank_dev / bank_city (N)
    int32, names, classes).  On `device` when given, else on the CPU.  waves.npy is memory-mapped while loading and converted
    in slices, so the host never holds a second fp32 copy.  The training split (13 965 clips of 10 s at 32 kHz) is about
    18 GB as fp32, which fits in HBM next to the model; int16 on disk halves the file, not the resident bank."""
    waves = np.load(os.path.join(path, "waves.npy"), mmap_mode="r")
    labels = np.load(os.path.join(path, "labels.npy"))
    with open(os.path.join(path, "names.txt")) as f:
        names = f.read().splitlines()
    with open(os.path.join(path, "classes.json")) as f:
        classes = json.load(f)
    if waves.ndim != 2 or waves.dtype not in (np.int16, np.float32):
        raise ValueError(f"DCASE20 bank at {path}: waves.npy must be (N, L) int16 or float32, got {waves.dtype} {waves.shape}")
    n = waves.shape[0]
    if labels.ndim != 2 or labels.shape[1] != 3 or labels.dtype.kind not in "iu":
        raise ValueError(f"DCASE20 bank at {path}: labels.npy must be (N, 3) integers, got {labels.dtype} {labels.shape}")
    if labels.shape[0] != n or len(names) != n or n == 0:
        raise ValueError(f"DCASE20 bank at {path}: {n} waveforms, {labels.shape[0]} label rows and {len(names)} names")
    if not isinstance(classes, dict) or any(not isinstance(classes.get(k), list) for k in KINDS):
        raise ValueError(f"DCASE20 bank at {path}: classes.json must hold the lists {KINDS}")
    for i, k in enumerate(KINDS):
        if labels[:, i].min() < 0 or labels[:, i].max() >= len(classes[k]):
            raise ValueError(f"DCASE20 bank at {path}: a {k} label lies outside its list of {len(classes[k])}")
    if len(classes["scene"]) > N_CLASSES:
        raise ValueError(f"DCASE20 bank at {path}: {len(classes['scene'])} scenes, the task has {N_CLASSES}")
    dev = torch.device("cpu") if device is None else device
    bank = torch.empty(waves.shape, dtype=torch.float32, device=dev)
    mean = torch.empty(n, dtype=torch.float64, device=dev)
    rows = max(1, (1 << 26) // waves.shape[1])                                 # 256 MB of fp32 per slice
    for s in range(0, n, rows):
        x = torch.from_numpy(np.array(waves[s:s + rows]))                      # (a copy: the map is read-only)
        x = x.float() / I16_SCALE if x.dtype == torch.int16 else x
        bank[s:s + rows] = x
        mean[s:s + rows] = x.double().mean(1)
    lab = torch.from_numpy(labels.astype(np.int32)).to(dev)
    return dict(bank=bank, bank_mean=mean, bank_cls=lab[:, 0].contiguous(), bank_dev=lab[:, 1].contiguous(),
                bank_city=lab[:, 2].contiguous(), names=names, classes=classes)


def _roll_and_gain(gain_augment, roll, shift_range):
    """One clip's draws in this dataset's order (datasets/dcase20.py:125-137): the gain dataset wraps the roll dataset, so the
    roll (audiodatasets.py:31-38, numpy: randint(-r, r + 1) is the deprecated random_integers(-r, r)) is drawn before the
    gain (audiodatasets.py:45-51, torch).  -> (amp, shift)."""
    shift = int(np.random.randint(-shift_range, shift_range + 1)) if roll else 0
    amp = 1.0
    if gain_augment:
        gain = torch.randint(gain_augment * 2, (1,)).item() - gain_augment
        amp = 10 ** (gain / 20)
    return amp, shift


def draw_augment(indices, n_bank, gain_augment=12, roll=True, wavmix=True, shift_range=4000, beta=2.0, rate=0.5):
    """Host draws of one batch, per sample in the order of DCASE20's MixupDataset.__getitem__ (datasets/dcase20.py:100-118):
    the clip is fetched FIRST - its roll (numpy), then its gain (torch) - and only then torch.rand(1) < rate decides the
    wave-mix; a mixed sample goes on with the partner torch.randint(n_bank), its roll and gain, and l = max(b, 1 - b), b ~
    np.random.beta(beta, beta).  (ESC-50 draws the coin first, and both ESC-50 and OpenMIC draw the gain before the roll.)
    -> the four tables of `esc50.draw_augment`: (idx (2B) int32, shift (2B) int32, amp (2B) fp32, mix (B) fp32) CPU tensors."""
    indices = [int(i) for i in indices]
    B = len(indices)
    idx = torch.full((2 * B,), -1, dtype=torch.int32)
    shift = torch.zeros(2 * B, dtype=torch.int32)
    amp = torch.ones(2 * B, dtype=torch.float32)
    mix = torch.ones(B, dtype=torch.float32)
    for i, index in enumerate(indices):
        idx[2 * i] = index
        amp[2 * i], shift[2 * i] = _roll_and_gain(gain_augment, roll, shift_range)
        if wavmix and bool(torch.rand(1) < rate):
            idx[2 * i + 1] = torch.randint(n_bank, (1,)).item()
            amp[2 * i + 1], shift[2 * i + 1] = _roll_and_gain(gain_augment, roll, shift_range)
            b = np.random.beta(beta, beta)
            mix[i] = max(b, 1.0 - b)
    return idx, shift, amp, mix


def draw_mixstyle(batch_size, p, alpha):
    """The host draws of helpers/utils.py `mixstyle`, in its order: np.random.rand() > p - not applied, NOTHING further is
    drawn; else lambda ~ Beta(alpha, alpha).sample((B, 1, 1, 1)) (torch), then torch.randperm(B).
    -> (apply, perm (B) int64 or None, lam (B) fp32 or None)."""
    if np.random.rand() > p:
        return False, None, None
    lam = torch.distributions.beta.Beta(alpha, alpha).sample((batch_size, 1, 1, 1))
    perm = torch.randperm(batch_size)
    return True, perm, lam.reshape(batch_size).float()
