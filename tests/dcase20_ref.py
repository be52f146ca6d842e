"""float64 references of the DCASE20 additions, in numpy, written from the contract in include/eat_hip.h (eat_freq_mixstyle)
and from the order of the nested datasets described in efficientat_amd/dcase20.py."""
import numpy as np
import torch


def freq_mixstyle_ref(x, perm, lam, eps=1e-6):
    """x (B, C, F, T) fp32, perm (B) int, lam (B) fp32 -> dict(out, mu (B, F), sig (B, F), scale) in float64.  eps is the
    fp32 number the kernel receives.  scale (same shape as out) is the per-element size the output error is measured in:
    |x - mu| / sig * sig_mix + |mu_mix| + |mu| sig_mix / sig - the last term is the rounding of mu to fp32 (the statistics are
    fp32 in the kernel's workspace and in torch alike), amplified by sig_mix / sig where sig is tiny."""
    x = np.asarray(x, dtype=np.float64)
    perm = np.asarray(perm, dtype=np.int64)
    l = np.asarray(lam, dtype=np.float64).reshape(-1, 1, 1, 1)
    n = x.shape[1] * x.shape[3]
    mu = x.mean(axis=(1, 3), keepdims=True)
    var = ((x - mu) ** 2).sum(axis=(1, 3), keepdims=True) / (n - 1)
    sig = np.sqrt(var + float(np.float32(eps)))
    sig_mix = l * sig + (1.0 - l) * sig[perm]
    mu_mix = l * mu + (1.0 - l) * mu[perm]
    out = (x - mu) / sig * sig_mix + mu_mix
    scale = np.abs(x - mu) / sig * sig_mix + np.abs(mu_mix) + np.abs(mu) * sig_mix / sig
    return dict(out=out, mu=mu[:, 0, :, 0], sig=sig[:, 0, :, 0], scale=scale)


def freq_mixstyle_torch_fp32(x, perm, lam, eps=1e-6):
    """The arithmetic of dropin/helpers/utils.py `mixstyle` in fp32 torch ops on the CPU, with the draws passed in
    -> (out, mu (B, F), sig (B, F)) fp32 tensors.  The yardstick the kernel's tolerance is taken from."""
    lmda = lam.reshape(-1, 1, 1, 1).float()
    mu = x.mean(dim=[1, 3], keepdim=True)
    sig = (x.var(dim=[1, 3], keepdim=True) + eps).sqrt()
    out = (x - mu) / sig * (sig * lmda + sig[perm] * (1 - lmda)) + (mu * lmda + mu[perm] * (1 - lmda))
    return out, mu[:, 0, :, 0], sig[:, 0, :, 0]


def mixstyle_errors(out, mu, sig, ref, x):
    """-> (worst scaled output error, worst |mu - ref| / max |x_row|, worst |sig - ref| / ref) of fp32 results against
    `freq_mixstyle_ref`'s dict; x: the fp32 input."""
    out, mu, sig = (np.asarray(t, dtype=np.float64) for t in (out, mu, sig))
    xmax = np.abs(np.asarray(x, dtype=np.float64)).max(axis=(1, 3))
    e_out = float((np.abs(out - ref["out"]) / ref["scale"]).max())
    e_mu = float((np.abs(mu - ref["mu"]) / np.maximum(xmax, 1e-300)).max())
    e_sig = float((np.abs(sig - ref["sig"]) / ref["sig"]).max())
    return e_out, e_mu, e_sig


def nested_dataset_draws(indices, n_bank, gain_augment=12, roll=True, wavmix=True, shift_range=4000, beta=2.0, rate=0.5):
    """The draws of one batch written as the nested datasets make them (datasets/dcase20.py:100-137): MixupDataset(
    GainDataset(RollDataset(base))).  Each class below draws exactly what its reference counterpart draws, in __getitem__
    order -> (idx, shift, amp, mix) lists in the layout of ops.wave_augment."""
    class Base:
        def get(self, i):
            return dict(i=i, shift=0, amp=1.0)

    class Roll:
        def __init__(self, ds):
            self.ds = ds

        def get(self, i):
            item = self.ds.get(i)
            item["shift"] = int(np.random.randint(-shift_range, shift_range + 1))
            return item

    class Gain:
        def __init__(self, ds):
            self.ds = ds

        def get(self, i):
            item = self.ds.get(i)
            gain = torch.randint(gain_augment * 2, (1,)).item() - gain_augment
            item["amp"] = 10 ** (gain / 20)
            return item

    ds = Base()
    if roll:
        ds = Roll(ds)
    if gain_augment:
        ds = Gain(ds)
    idx, shift, amp, mix = [], [], [], []
    for i in indices:
        a = ds.get(int(i))
        b, l = dict(i=-1, shift=0, amp=1.0), 1.0
        if wavmix and bool(torch.rand(1) < rate):
            b = ds.get(torch.randint(n_bank, (1,)).item())
            l = np.random.beta(beta, beta)
            l = max(l, 1.0 - l)
        idx += [a["i"], b["i"]]
        shift += [a["shift"], b["shift"]]
        amp += [a["amp"], b["amp"]]
        mix.append(l)
    return idx, shift, amp, mix
