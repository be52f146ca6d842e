"""fp64 numpy reference of query-by-example search (include/eat_search.h, efficientat_amd/retrieval.py), and the ranking
check that the GPU tests share.

score[q, n] = sum_d qn[q, d] bank[n, d] in fp64; a row is eligible unless skip[q, 0] <= n < skip[q, 1] (bounds clamped into
[0, N]); the result is the k eligible rows in (score descending, index ascending) order - np.lexsort on (index, -score) -
padded with index -1 and score -inf."""
import numpy as np


def normalize_ref(x):
    """x / sqrt(sum x^2) per row in fp64; a row whose sum of squares is 0 becomes zeros."""
    x = np.asarray(x, dtype=np.float64)
    ss = (x * x).sum(axis=1, keepdims=True)
    return np.where(ss > 0, x / np.sqrt(np.where(ss > 0, ss, 1.0)), 0.0)


def eligible_ref(N, Q, skip=None):
    """(Q, N) bool."""
    ok = np.ones((Q, N), dtype=bool)
    if skip is not None:
        rows = np.arange(N)
        for q, (lo, hi) in enumerate(np.asarray(skip, dtype=np.int64).reshape(Q, 2)):
            lo, hi = min(max(int(lo), 0), N), min(max(int(hi), 0), N)
            ok[q] = ~((rows >= lo) & (rows < hi))
    return ok


def scores_ref(bank, queries, normalize=True):
    """(Q, N) fp64 scores; normalize=False: both operands are taken as they are (the C entry point's contract)."""
    b, q = np.asarray(bank, dtype=np.float64), np.asarray(queries, dtype=np.float64)
    if normalize:
        b, q = normalize_ref(b), normalize_ref(q)
    # one row-wise sum per query, not a BLAS product: identical rows then score identically, wherever they stand
    return np.stack([(b * vec).sum(axis=1) for vec in q])


def topk_ref(scores, k, skip=None):
    """scores (Q, N) fp64 -> (score (Q, k) fp64, index (Q, k) int64)."""
    Q, N = scores.shape
    ok = eligible_ref(N, Q, skip)
    out_s = np.full((Q, k), -np.inf)
    out_i = np.full((Q, k), -1, dtype=np.int64)
    for q in range(Q):
        rows = np.flatnonzero(ok[q])
        order = rows[np.lexsort((rows, -scores[q, rows]))][:k]
        out_s[q, :len(order)] = scores[q, order]
        out_i[q, :len(order)] = order
    return out_s, out_i


def search_ref(bank, queries, k, skip=None, normalize=True):
    return topk_ref(scores_ref(bank, queries, normalize), k, skip)


def check_ranking(score, index, ref, k, skip=None, bar=2e-5, slack=4e-5, tag=""):
    """What every search result must satisfy, given the fp64 scores ref (Q, N); needs no index equality, so near-ties
    cannot make it flaky.  Prints the largest score error and returns it.
    - returned indices are distinct, eligible, and in (score desc, index asc) order by the returned fp32 scores;
    - |score - ref at the returned index| <= bar;
    - every eligible row not returned has ref <= the last returned row's ref + slack;
    - exactly max(0, k - eligible) slots hold (-inf, -1), and they come last."""
    score, index = np.asarray(score), np.asarray(index)
    Q, N = ref.shape
    assert score.shape == (Q, k) and index.shape == (Q, k), (score.shape, index.shape, (Q, k))
    assert score.dtype == np.float32 and index.dtype == np.int32
    ok = eligible_ref(N, Q, skip)
    worst = 0.0
    for q in range(Q):
        n_el = int(ok[q].sum())
        n_ret = min(k, n_el)
        idx, s = index[q].astype(np.int64), score[q]
        assert bool((idx[n_ret:] == -1).all()) and bool(np.isneginf(s[n_ret:]).all()), (tag, q, "padding", idx, s)
        idx, s = idx[:n_ret], s[:n_ret]
        assert bool(((idx >= 0) & (idx < N)).all()), (tag, q, "index out of range", idx)
        assert len(set(idx.tolist())) == n_ret, (tag, q, "an index twice", idx)
        assert bool(ok[q, idx].all()), (tag, q, "an excluded row was returned", idx)
        assert not bool(np.isnan(s).any()), (tag, q, "NaN score")
        for a in range(n_ret - 1):
            assert s[a] > s[a + 1] or (s[a] == s[a + 1] and idx[a] < idx[a + 1]), (tag, q, a, "order", s[a:a + 2], idx[a:a + 2])
        err = np.abs(s.astype(np.float64) - ref[q, idx])
        if n_ret:
            worst = max(worst, float(err.max()))
            assert bool((err <= bar).all()), (tag, q, "score error", float(err.max()))
            left = ok[q].copy()
            left[idx] = False
            if bool(left.any()):
                assert float(ref[q, left].max()) <= float(ref[q, idx[-1]]) + slack, (tag, q, "a better row was left out",
                                                                                    float(ref[q, left].max()), float(ref[q, idx[-1]]))
    print(f"SEARCH {tag}: max |score - ref| = {worst:.3e} over {Q} x {k} (bar {bar:.0e})")
    return worst
