"""efficientat_amd.metrics (eat_rank_metrics, csrc/metrics.hip) against the fp64 numpy oracle tests/rank_metrics_ref.py:
per-class AP / ROC AUC at sizes that cross the tile and sort edges, fp32 / bf16 / fp16 and non-contiguous scores, ties,
+-0.0, huge finite scores, degenerate columns, invalid input, determinism, and the time of a 20 000 x 527 evaluation."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import rank_metrics_ref as R

from efficientat_amd import metrics  # noqa: E402
from efficientat_amd._lib import EatHipError  # noqa: E402

DEV = torch.device("cuda:0")
ATOL = 1e-9


def _data(n, c, seed, p=0.1):
    """Scores with a few kinds of column: continuous, quantised to 1-8 levels (ties), and +-0.0 mixes."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(n, c, generator=g)
    levels = torch.randint(1, 9, (c,), generator=g)
    q = torch.floor(torch.rand(n, c, generator=g) * levels) - 2.0
    kind = torch.arange(c) % 3
    s = torch.where(kind == 1, q, s)
    z = torch.where(torch.rand(n, c, generator=g) < 0.5, torch.tensor(-0.0), torch.tensor(0.0))
    s = torch.where((kind == 2) & (torch.rand(n, c, generator=g) < 0.5), z, s)
    y = (torch.rand(n, c, generator=g) < p).float()
    return s, y


def _check(s, y, scores_dev=None):
    ap, auc = metrics.ap_auc(scores_dev if scores_dev is not None else s.to(DEV), y.to(DEV))
    assert ap.dtype == torch.float64 and ap.shape == (s.shape[1] if s.dim() == 2 else 1,)
    ap_r, auc_r = R.ap_auc(s.float().numpy(), y.numpy())
    np.testing.assert_allclose(ap.cpu().numpy(), ap_r, rtol=0, atol=ATOL)
    np.testing.assert_allclose(auc.cpu().numpy(), auc_r, rtol=0, atol=ATOL, equal_nan=True)
    assert np.array_equal(np.isnan(auc.cpu().numpy()), np.isnan(auc_r))


SIZES = [(n, c) for n in (1, 2, 63, 64, 65, 1024, 1025, 20480, 20481) for c in (1, 7, 50, 527)] + \
        [(100003, 1), (100003, 7), (100003, 50), ((1 << 20) + 3, 1), ((1 << 20) + 3, 7)]


@pytest.mark.parametrize("n,c", SIZES)
def test_ap_auc_matches_fp64_oracle(n, c):
    s, y = _data(n, c, seed=n * 1000 + c, p=0.3 if n < 100 else 0.05)
    _check(s, y)


@pytest.mark.parametrize("n,c", [(65, 7), (1025, 50), (20481, 7)])
def test_bf16_and_fp16_scores(n, c):
    s, y = _data(n, c, seed=7 + n)
    sb = s.to(torch.bfloat16)
    _check(sb.float(), y, scores_dev=sb.to(DEV))                 # the oracle gets the bf16 values widened to fp32
    sh = s.to(torch.float16)
    _check(sh.float(), y, scores_dev=sh.to(DEV))


def test_non_contiguous_and_1d_inputs():
    s, y = _data(1025, 9, seed=3)
    st, yt = s.t().contiguous().to(DEV).t(), y.t().contiguous().to(DEV).t()     # (N, C) views of column-major memory
    assert not st.is_contiguous()
    ap, auc = metrics.ap_auc(st, yt)
    ap_r, auc_r = R.ap_auc(s.numpy(), y.numpy())
    np.testing.assert_allclose(ap.cpu().numpy(), ap_r, atol=ATOL)
    np.testing.assert_allclose(auc.cpu().numpy(), auc_r, atol=ATOL, equal_nan=True)
    ap1, auc1 = metrics.ap_auc(s[:, 4].to(DEV), y[:, 4].to(DEV))                  # (N,) = one class
    assert ap1.shape == (1,) and abs(float(ap1[0]) - ap_r[4]) < ATOL and abs(float(auc1[0]) - auc_r[4]) < ATOL
    sb = s.to(torch.bfloat16).t().contiguous().to(DEV).t()
    ap2, _ = metrics.ap_auc(sb, yt)
    np.testing.assert_allclose(ap2.cpu().numpy(), R.ap_auc(s.to(torch.bfloat16).float().numpy(), y.numpy())[0], atol=ATOL)


def test_ties_zeros_huge_scores_and_degenerate_columns():
    rng = np.random.default_rng(5)
    n = 3000
    cols = [rng.choice(np.array([-0.0, 0.0]), n),                                  # only zeros of both signs: one tie group
            rng.choice(np.array([-0.0, 0.0, 1.0, -1.0]), n),
            rng.choice(np.array([-3e38, 3e38, 1e38, -1e-38, 0.0]), n),
            np.full(n, 0.25),                                                       # all equal
            rng.integers(0, 2, n).astype(np.float64),
            rng.standard_normal(n),
            rng.standard_normal(n)]
    s = torch.tensor(np.stack(cols, 1), dtype=torch.float32)
    y = torch.tensor(rng.random((n, len(cols))) < 0.2, dtype=torch.float32)
    y[:, 5] = 0.0                                                                   # no positives: AP 0, AUC NaN
    y[:, 6] = 1.0                                                                   # only positives: AP 1, AUC NaN
    _check(s, y)
    ap, auc = metrics.ap_auc(s.to(DEV), y.to(DEV))
    assert float(ap[5]) == 0.0 and float(ap[6]) == 1.0 and torch.isnan(auc[5:7]).all()
    assert float(auc[0]) == 0.5 and float(auc[3]) == 0.5                         # a single tie group: area 1/2
    # N = 1
    ap, auc = metrics.ap_auc(torch.tensor([[2.0, -1.0]], device=DEV), torch.tensor([[1.0, 0.0]], device=DEV))
    assert ap.tolist() == [1.0, 0.0] and torch.isnan(auc).all()


def test_averages():
    s, y = _data(1025, 50, seed=11)
    s, y = s.to(DEV), y.to(DEV)
    ap, auc = metrics.ap_auc(s, y)
    assert torch.equal(metrics.average_precision(s, y), ap)
    assert float(metrics.average_precision(s, y, average="macro")) == float(ap.mean())
    assert float(metrics.roc_auc(s, y, average="macro")) == float(auc.mean())
    y[:, 3] = 0.0
    assert torch.isnan(metrics.roc_auc(s, y, average="macro"))                   # the reference's .mean(): NaN propagates
    with pytest.raises(ValueError):
        metrics.roc_auc(s, y, average="micro")


@pytest.mark.parametrize("bad", ["nan", "inf", "-inf", "half_target", "nan_target"])
def test_invalid_input_raises_value_error(bad):
    s, y = _data(200, 5, seed=2)
    if bad == "nan":
        s[17, 3] = float("nan")
    elif bad == "inf":
        s[199, 0] = float("inf")
    elif bad == "-inf":
        s[0, 4] = float("-inf")
    elif bad == "half_target":
        y[5, 2] = 0.5
    else:
        y[5, 2] = float("nan")
    with pytest.raises(ValueError):
        metrics.ap_auc(s.to(DEV), y.to(DEV))
    metrics.ap_auc(_data(200, 5, seed=2)[0].to(DEV), _data(200, 5, seed=2)[1].to(DEV))   # the next call is clean again


def test_bad_shapes_and_cpu_tensors():
    with pytest.raises(EatHipError):
        metrics.ap_auc(torch.zeros(4, 2), torch.zeros(4, 2))
    with pytest.raises(EatHipError):                                                # N = 0: EAT_EINVAL
        metrics.ap_auc(torch.zeros(0, 2, device=DEV), torch.zeros(0, 2, device=DEV))
    with pytest.raises(ValueError):
        metrics.ap_auc(torch.zeros(4, 2, device=DEV), torch.zeros(4, 3, device=DEV))
    from efficientat_amd._lib import lib
    h = lib()
    assert h.eat_rank_metrics_ws_bytes(20000, 527) == 16 * 20000 * 527
    assert h.eat_rank_metrics_ws_bytes((1 << 22) + 1, 1) < 0
    assert h.eat_rank_metrics_ws_bytes(1, (1 << 16) + 1) < 0
    assert h.eat_rank_metrics_ws_bytes(1 << 22, 1 << 10) < 0                       # N * C >= 2^31
    assert h.eat_rank_metrics_ws_bytes(1 << 22, 511) == 16 * (1 << 22) * 511


def test_two_calls_are_bit_identical():
    s, y = _data(20480, 64, seed=9)
    s, y = s.to(DEV), y.to(DEV)
    a1, u1 = metrics.ap_auc(s, y)
    a2, u2 = metrics.ap_auc(s, y)
    assert torch.equal(a1, a2) and torch.equal(torch.nan_to_num(u1), torch.nan_to_num(u2))


def test_time_of_audioset_eval_size():
    """20 000 x 527 (the AudioSet eval split): time per call with HIP events, printed; no bound asserted."""
    g = torch.Generator(device=DEV).manual_seed(0)
    s = torch.randn(20000, 527, device=DEV, generator=g)
    y = (torch.rand(20000, 527, device=DEV, generator=g) < 0.01).float()
    y[0] = 1.0
    for _ in range(2):
        metrics.ap_auc(s, y)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps = 5
    e0.record()
    for _ in range(reps):
        ap, _ = metrics.ap_auc(s, y)                     # (each call reads the status word: a host sync included)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    print(f"\nap_auc 20000 x 527 fp32: {ms:.3f} ms per call")
    ap_r, _ = R.ap_auc(s[:, :16].cpu().numpy(), y[:, :16].cpu().numpy())
    np.testing.assert_allclose(ap[:16].cpu().numpy(), ap_r, atol=ATOL)
