"""fp64 numpy average precision / ROC AUC per class: the oracle of efficientat_amd.metrics (a helper, not a test module).

The definitions of sklearn 1.7's average_precision_score / roc_auc_score with average=None (what the reference's `_test`
calls, ex_audioset.py:253-254), written out with a stable descending sort and explicit tie groups:
  * two scores tie iff they are equal as fp32 values (-0.0 == +0.0);
  * AP  = sum over distinct thresholds t, descending, of (R(t) - R(t_prev)) * P(t), R = TP / n_pos, P = TP / count;
  * AUC = trapezoid area of the ROC curve (Mann-Whitney U with ties counted 1/2);
  * no positives: AP = 0.0; only positives: AP = 1.0; one class only: AUC = NaN (sklearn warns; this returns NaN quietly).
"""
import numpy as np


def ap_auc_column(scores, targets):
    s = np.asarray(scores, dtype=np.float32).astype(np.float64)
    y = np.asarray(targets, dtype=np.float64)
    n = s.shape[0]
    n_pos = int(y.sum())
    n_neg = n - n_pos
    order = np.argsort(-s, kind="stable")
    s, y = s[order], y[order]
    ends = np.flatnonzero(np.r_[s[1:] != s[:-1], True])          # last index of every tie group (-0.0 == 0.0 in fp64 too)
    tp = np.cumsum(y)[ends]
    cnt = (ends + 1).astype(np.float64)
    fp = cnt - tp
    tp_prev = np.r_[0.0, tp[:-1]]
    fp_prev = np.r_[0.0, fp[:-1]]
    if n_pos == 0:
        ap = 0.0
    elif n_neg == 0:
        ap = 1.0
    else:
        ap = float(np.sum((tp - tp_prev) / n_pos * (tp / cnt)))
    if n_pos == 0 or n_neg == 0:
        auc = float("nan")
    else:
        auc = float(np.sum((fp - fp_prev) * (tp + tp_prev)) / (2.0 * n_pos * n_neg))
    return ap, auc


def ap_auc(scores, targets):
    """scores, targets: (N, C) or (N,) -> (ap, auc) float64 arrays of shape (C,)."""
    s = np.asarray(scores, dtype=np.float32)
    y = np.asarray(targets, dtype=np.float64)
    if s.ndim == 1:
        s, y = s[:, None], y[:, None]
    res = np.array([ap_auc_column(s[:, c], y[:, c]) for c in range(s.shape[1])], dtype=np.float64).reshape(-1, 2)
    return res[:, 0].copy(), res[:, 1].copy()
