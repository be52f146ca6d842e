"""Ranking metrics of the AudioSet evaluation on the GPU: per-class average precision and ROC AUC.

What it must equal: the reference's `_test` (ex_audioset.py:231-256; ex_pl_audioset.py:215-247 after gathering every rank's
predictions), i.e. sklearn 1.7's `average_precision_score` / `roc_auc_score` with `average=None`, ties included (scores
tie iff equal as fp32, so -0.0 ties +0.0).  Degenerate columns as sklearn: no positives -> AP 0.0, only positives -> AP 1.0,
one class only -> AUC NaN (without sklearn's warning).  A non-finite score or a target other than 0 / 1 raises ValueError,
as sklearn does.  The work is eat_rank_metrics (csrc/metrics.hip): key build, a per-class radix sort and one scan, all on
the device with fp64 sums in a fixed order - repeated calls are bit-identical.  There is no CPU path and no sklearn.
"""
import torch

from . import _lib
from .ops import _stream

_BAD_SCORE, _BAD_TARGET, _BAD_WEIGHT = 1, 2, 4


def _as_matrix(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise _lib.EatHipError(f"{name} must live on the GPU: efficientat_amd has no CPU path (got device {t.device})")
    if t.dim() == 1:
        t = t.unsqueeze(1)
    if t.dim() != 2:
        raise ValueError(f"{name} must be (N, C) or (N,), got shape {tuple(t.shape)}")
    return t


def ap_auc(scores, targets, sample_weight=None):
    """scores (N, C) or (N,) fp32 / bf16 / fp16, targets of the same shape (0 / 1) -> (ap, auc): float64 device tensors of
    shape (C,).  One launch sequence and one read of the status word (a host sync).  sample_weight: a 0 / 1 matrix of the same
    shape (ex_openmic.py:194-204, sklearn's `sample_weight`): an item of weight 0 is left out of its column, and the
    degenerate rules apply to what is left (no weighted item at all: AP 0.0, AUC NaN)."""
    s = _as_matrix(scores, "scores")
    y = _as_matrix(targets, "targets")
    if s.shape != y.shape:
        raise ValueError(f"scores {tuple(s.shape)} and targets {tuple(y.shape)} differ in shape")
    if s.device != y.device:
        raise ValueError(f"scores on {s.device}, targets on {y.device}")
    w = None
    if sample_weight is not None:
        w = _as_matrix(sample_weight, "sample_weight")
        if w.shape != s.shape:
            raise ValueError(f"scores {tuple(s.shape)} and sample_weight {tuple(w.shape)} differ in shape")
        if w.device != s.device:
            raise ValueError(f"scores on {s.device}, sample_weight on {w.device}")
        w = w.to(torch.float32).contiguous()
    if s.dtype not in (torch.float32, torch.bfloat16):
        s = s.float()                                   # fp16 (and anything else) is widened to fp32
    s = s.contiguous()
    y = y.to(torch.float32).contiguous()
    N, C = s.shape
    h = _lib.lib()
    ws_bytes = h.eat_rank_metrics_ws_bytes(N, C)
    if ws_bytes < 0:
        raise _lib.EatHipError(f"eat_rank_metrics_ws_bytes failed ({ws_bytes}): {h.eat_last_error_string().decode()}")
    with torch.cuda.device(s.device):
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=s.device)
        ap = torch.empty(C, dtype=torch.float64, device=s.device)
        auc = torch.empty(C, dtype=torch.float64, device=s.device)
        n_pos = torch.empty(C, dtype=torch.int32, device=s.device)
        status = torch.empty(1, dtype=torch.int32, device=s.device)
        out = (N, C, ws.data_ptr(), ap.data_ptr(), auc.data_ptr(), n_pos.data_ptr(), status.data_ptr(), _stream())
        if w is None:
            _lib.call("eat_rank_metrics", s.data_ptr(), int(s.dtype == torch.bfloat16), y.data_ptr(), *out)
        else:
            _lib.call("eat_rank_metrics_masked", s.data_ptr(), int(s.dtype == torch.bfloat16), y.data_ptr(), w.data_ptr(), *out)
        st = int(status.item())
    if st & _BAD_SCORE:
        raise ValueError("scores contain NaN or infinity")
    if st & _BAD_TARGET:
        raise ValueError("targets must be exactly 0 or 1")
    if st & _BAD_WEIGHT:
        raise ValueError("sample_weight must be exactly 0 or 1")
    return ap, auc


def _reduce(v, average):
    if average is None:
        return v
    if average == "macro":
        return v.mean()             # the reference's `.mean()`: a NaN column makes the mean NaN
    raise ValueError(f"average must be None or 'macro', got {average!r}")


def average_precision(scores, targets, average=None, sample_weight=None):
    """Per-class AP (average=None) or its plain mean ("macro"): sklearn's average_precision_score."""
    return _reduce(ap_auc(scores, targets, sample_weight)[0], average)


def roc_auc(scores, targets, average=None, sample_weight=None):
    """Per-class ROC AUC (average=None) or its plain mean ("macro"): sklearn's roc_auc_score."""
    return _reduce(ap_auc(scores, targets, sample_weight)[1], average)
