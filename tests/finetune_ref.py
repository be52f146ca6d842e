"""float64 references of the fine-tuning kernels (efficientat_amd/csrc/finetune.hip), in numpy.

softmax_ce_ref: F.cross_entropy with probability targets (ex_esc50.py:102-118), the mix-up folded into the target.
wave_augment_ref: gain, roll and MixupDataset's wave-mix of clips taken from a bank of padded rows (datasets/esc50.py)."""
import numpy as np


def mixed_targets(y, perm=None, lam=None):
    y = np.asarray(y, dtype=np.float64)
    if perm is None:
        return y
    lam = np.asarray(lam, dtype=np.float32).astype(np.float64)[:, None]
    return lam * y + (1.0 - lam) * y[np.asarray(perm)]


def softmax_ce_ref(z, y, perm=None, lam=None):
    """-> dict(loss, row_loss (B), dlogits (B, C), argmax (B), S (B)); z, y (B, C) as float32 arrays."""
    z = np.asarray(z, dtype=np.float32).astype(np.float64)
    t = mixed_targets(y, perm, lam)
    B = z.shape[0]
    S = t.sum(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        m = z.max(axis=1, keepdims=True)
        lse = m + np.log(np.exp(z - m).sum(axis=1, keepdims=True))
        ce = (t * (lse - z)).sum(axis=1)
        d = (S[:, None] * np.exp(z - lse) - t) / B
    return dict(loss=ce.mean(), row_loss=ce, dlogits=d, argmax=z.argmax(axis=1), S=S)


def wave_augment_ref(bank, bank_cls, idx, shift, amp, mix, n_classes):
    """-> (out (B, L), y (B, C)) float64.  x_k = amp_k * roll(bank[idx_k], shift_k); wave-mix (idx[2b+1] >= 0):
    l (x_0 - mean x_0) + (1 - l) (x_1 - mean x_1), y = l onehot(cls_0) + (1 - l) onehot(cls_1)."""
    bank = np.asarray(bank, dtype=np.float32).astype(np.float64)
    idx, shift = np.asarray(idx), np.asarray(shift)
    amp = np.asarray(amp, dtype=np.float32).astype(np.float64)
    mix = np.asarray(mix, dtype=np.float32).astype(np.float64)
    B = len(mix)
    out = np.zeros((B, bank.shape[1]))
    y = np.zeros((B, n_classes))
    for b in range(B):
        i0, i1 = int(idx[2 * b]), int(idx[2 * b + 1])
        x0 = amp[2 * b] * np.roll(bank[i0], int(shift[2 * b]))
        if i1 < 0:
            out[b] = x0
            y[b, bank_cls[i0]] = 1.0
            continue
        x1 = amp[2 * b + 1] * np.roll(bank[i1], int(shift[2 * b + 1]))
        lm = mix[b]
        out[b] = lm * (x0 - x0.mean()) + (1.0 - lm) * (x1 - x1.mean())
        y[b, bank_cls[i0]] += lm
        y[b, bank_cls[i1]] += 1.0 - lm
    return out, y
