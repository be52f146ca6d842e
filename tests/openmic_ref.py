"""float64 references of the OpenMIC kernels (a helper, not a test module), in numpy, written from the contract in
include/eat_hip.h.

masked_bce_ref: ex_openmic.py:102-121 - BCE-with-logits on binarized, mixed labels times the annotation mask.
openmic_targets_ref: the label rule of OpenMIC's MixupDataset.__getitem__ (datasets/openmic.py:74-95).
masked_ap_auc: tests/rank_metrics_ref.ap_auc_column on the rows of weight 1."""
import numpy as np

from tests import rank_metrics_ref as R


def masked_bce_ref(z, yy, perm=None, lam=None, binarize=True):
    """-> dict(loss, row_loss (B), dlogits (B, C), probs (B, C)); z (B, C), yy (B, 2C) = [labels | mask] as float32 arrays.
    A perm entry outside [0, B) makes its row NaN."""
    z = np.asarray(z, dtype=np.float32).astype(np.float64)
    yy = np.asarray(yy, dtype=np.float32)
    B, C = z.shape
    t = (yy[:, :C] > 0.5).astype(np.float64) if binarize else yy[:, :C].astype(np.float64)
    m = yy[:, C:].astype(np.float64)
    if perm is not None:
        perm = np.asarray(perm)
        l = np.asarray(lam, dtype=np.float32).astype(np.float64)[:, None]
        bad = (perm < 0) | (perm >= B)
        l = np.where(bad[:, None], np.nan, l)
        t = l * t + (1.0 - l) * t[np.where(bad, np.arange(B), perm)]
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(-np.abs(z))
        elem = m * (np.maximum(z, 0.0) - z * t + np.log1p(e))
        sg = np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        sg = np.where(np.isnan(z), np.nan, sg)
        d = m * (sg - t) / (B * C)
    row = elem.sum(axis=1) / C
    return dict(loss=row.mean(), row_loss=row, dlogits=d, probs=sg)


def openmic_targets_ref(bank_y, idx, mix):
    """-> yy (B, 2C) float64: row idx[2b] copied unchanged when idx[2b + 1] < 0, else labels l y1 m1 + (1 - l) y2 m2 and mask
    max(m1, m2) with m_k = (mask_k > 0.5); an index outside the bank gives a NaN row."""
    bank_y = np.asarray(bank_y, dtype=np.float32).astype(np.float64)
    n, C = bank_y.shape[0], bank_y.shape[1] // 2
    mix = np.asarray(mix, dtype=np.float32).astype(np.float64)
    out = np.empty((len(mix), 2 * C))
    for b in range(len(mix)):
        i0, i1 = int(idx[2 * b]), int(idx[2 * b + 1])
        if not (0 <= i0 < n and -1 <= i1 < n):
            out[b] = np.nan
        elif i1 < 0:
            out[b] = bank_y[i0]
        else:
            y1, y2, l = bank_y[i0], bank_y[i1], mix[b]
            m1, m2 = (y1[C:] > 0.5).astype(np.float64), (y2[C:] > 0.5).astype(np.float64)
            out[b, :C] = l * (y1[:C] * m1) + (1.0 - l) * (y2[:C] * m2)
            out[b, C:] = np.maximum(m1, m2)
    return out


def masked_ap_auc(scores, targets, weights):
    """(N, C) arrays -> (ap, auc) float64 (C,): the unweighted oracle on the rows whose weight is 1.  A column without any
    weighted row follows the rule for "no positives" (AP 0.0, AUC NaN; the oracle itself cannot take an empty column)."""
    s, y, w = (np.asarray(a) for a in (scores, targets, weights))
    if s.ndim == 1:
        s, y, w = s[:, None], y[:, None], w[:, None]
    ap, auc = np.empty(s.shape[1]), np.empty(s.shape[1])
    for c in range(s.shape[1]):
        keep = w[:, c] == 1
        ap[c], auc[c] = R.ap_auc_column(s[keep, c], y[keep, c]) if keep.any() else (0.0, float("nan"))
    return ap, auc
