"""tests/rank_metrics_ref.py (the fp64 oracle of the GPU ranking metrics) against sklearn.metrics, on the CPU."""
import warnings

import numpy as np
import pytest

from tests import rank_metrics_ref as R


def _cases():
    """(scores float32 (N, C), targets float (N, C)) - random, heavy ties, +-0.0, huge finite scores, degenerate columns."""
    rng = np.random.default_rng(0)
    out = []
    for k in range(240):
        n = int(rng.choice([1, 2, 3, 5, 17, 64, 65, 200]))
        c = int(rng.integers(1, 6))
        kind = k % 6
        if kind == 0:
            s = rng.standard_normal((n, c))
        elif kind == 1:                                           # quantised to 1 - 8 levels: ties everywhere
            s = rng.integers(0, int(rng.integers(1, 9)), (n, c)) * 0.25 - 1.0
        elif kind == 2:                                           # a mix of -0.0 / +0.0 and a few other values
            s = rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 1.0, -1.0]), (n, c))
        elif kind == 3:                                           # very large finite scores
            s = rng.choice(np.array([-3e38, 3e38, 1e38, -1e-38, 0.0]), (n, c))
        elif kind == 4:                                           # all scores equal
            s = np.full((n, c), float(rng.standard_normal()))
        else:
            s = rng.standard_normal((n, c)) * 1e3
        y = (rng.random((n, c)) < rng.uniform(0.05, 0.6)).astype(np.float64)
        if c > 1:
            y[:, 0] = 0.0                                         # a column without positives ...
        if c > 2:
            y[:, 1] = 1.0                                         # ... and one with positives only
        out.append((s.astype(np.float32), y))
    return out


def test_ties_and_degenerate_columns_by_hand():
    # 4 clips, scores 0.9, 0.5 (pos), 0.5 (neg), 0.1 (pos): thresholds 0.9 / 0.5 / 0.1
    ap, auc = R.ap_auc_column([0.9, 0.5, 0.5, 0.1], [0, 1, 0, 1])
    assert ap == pytest.approx(0.5 * (1 / 3) + 0.5 * 0.5)       # tied positive shares precision 1/3; the last one 2/4
    assert auc == pytest.approx(0.5 / 4)                         # 4 (pos, neg) pairs: only pos@0.5 vs neg@0.5 counts, 1/2
    assert R.ap_auc_column([-0.0, 0.0], [1, 0]) == (0.5, 0.5)    # -0.0 ties +0.0
    ap, auc = R.ap_auc_column([1.0, 2.0], [0, 0])
    assert ap == 0.0 and np.isnan(auc)
    ap, auc = R.ap_auc_column([1.0, 2.0], [1, 1])
    assert ap == 1.0 and np.isnan(auc)
    ap, auc = R.ap_auc_column([3.0], [1])
    assert ap == 1.0 and np.isnan(auc)


def test_reference_helper_matches_sklearn():
    metrics = pytest.importorskip("sklearn.metrics")
    n_checked = 0
    for s, y in _cases():
        ap, auc = R.ap_auc(s, y)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ap_sk = metrics.average_precision_score(y, s, average=None)
            ap_sk = np.atleast_1d(ap_sk)
            if s.shape[1] == 1:                                   # a single column is "binary" to sklearn
                ap_sk = np.array([metrics.average_precision_score(y[:, 0], s[:, 0])])
            auc_sk = np.array([metrics.roc_auc_score(y[:, j], s[:, j]) if 0 < y[:, j].sum() < len(y) else np.nan
                               for j in range(s.shape[1])])
        np.testing.assert_allclose(ap, ap_sk, rtol=0, atol=1e-12)
        np.testing.assert_allclose(auc, auc_sk, rtol=0, atol=1e-12, equal_nan=True)
        assert np.array_equal(np.isnan(auc), np.isnan(auc_sk))
        n_checked += 1
    assert n_checked >= 200


def test_sklearn_one_class_auc_is_nan_and_ours_too():
    metrics = pytest.importorskip("sklearn.metrics")
    y = np.array([[0, 1, 1], [0, 1, 0], [0, 1, 1.0]])
    s = np.array([[0.1, 0.2, 0.3], [0.2, 0.1, 0.3], [0.0, -0.0, 0.5]], dtype=np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        auc_sk = metrics.roc_auc_score(y, s, average=None)
        ap_sk = metrics.average_precision_score(y, s, average=None)
    ap, auc = R.ap_auc(s, y)
    np.testing.assert_allclose(auc, auc_sk, atol=1e-12, equal_nan=True)
    np.testing.assert_allclose(ap, ap_sk, atol=1e-12)
