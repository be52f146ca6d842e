"""numpy reference of occurrence search (include/eat_match.h, efficientat_amd/retrieval.py: EmbeddingIndex.find).

`match_ref` takes the row scores S (L, N) - S[j, n] = the score of query row j and bank row n - and implements the
definition in the dtype of S.  In float32 it performs the additions one at a time in ascending j and the IEEE division by
float32(L): given the bits of `eat_embed_search` in S it predicts the bits of `eat_embed_match`.  In float64 it is the
reference.  The peak rule is vectorised; `match_brute` in tests/test_match_cpu.py reads the definition literally."""
import numpy as np


def window_means(S):
    """m (N,) in S's dtype: m[n] = ((S[0, n] + S[1, n + 1]) + ...) / L where the window fits the BANK (n + L <= N), NaN
    elsewhere.  Whether it fits the row's file is `starts_ref`'s business."""
    S = np.asarray(S)
    L, N = S.shape
    m = np.full(N, np.nan, dtype=S.dtype)
    if N >= L:
        n = N - L + 1
        acc = S[0, :n].copy()
        for j in range(1, L):
            acc = acc + S[j, j:j + n]                      # one rounding per addition, in S's dtype
        m[:n] = acc / S.dtype.type(L)
    return m


def starts_ref(seg, N, L, skip=None):
    """(file of each row (N,), candidate (N,) bool): valid - the window fits the row's file - and outside `skip`."""
    seg = np.asarray(seg, dtype=np.int64)
    assert seg[0] == 0 and seg[-1] == N and bool((np.diff(seg) > 0).all())
    rows = np.arange(N)
    file = np.searchsorted(seg, rows, side="right") - 1
    cand = rows + L <= seg[file + 1]
    if skip is not None:
        lo, hi = (min(max(int(v), 0), N) for v in skip)
        cand &= ~((rows >= lo) & (rows < hi))
    return file, cand


def peaks_ref(m, file, cand, sep):
    """(N,) bool: candidates better than every other candidate of their file within sep rows (better: larger m, equal m
    by lower row).  Local maxima, not greedy suppression."""
    N = len(m)
    peak = cand.copy()
    rows = np.arange(N)
    with np.errstate(invalid="ignore"):
        for d in range(1, min(int(sep), N - 1) + 1):
            a, b = rows[:-d], rows[d:]                         # a < b, |a - b| = d
            both = cand[a] & cand[b] & (file[a] == file[b])
            peak[b[both & (m[a] >= m[b])]] = False             # a is better than b on a tie: the lower row
            peak[a[both & (m[b] > m[a])]] = False
    return peak


def match_ref(S, seg, k, sep, min_score=-np.inf, skip=None):
    """-> (score (k,) in S's dtype, index (k,) int64): the k peaks with m >= min_score in descending m, equal m by
    ascending row, padded with (-inf, -1)."""
    S = np.asarray(S)
    L, N = S.shape
    m = window_means(S)
    file, cand = starts_ref(seg, N, L, skip)
    peak = peaks_ref(m, file, cand, sep)
    with np.errstate(invalid="ignore"):
        rows = np.flatnonzero(peak & (m >= S.dtype.type(min_score)))
    order = rows[np.lexsort((rows, -m[rows]))][:k]
    score = np.full(k, -np.inf, dtype=S.dtype)
    index = np.full(k, -1, dtype=np.int64)
    score[:len(order)] = m[order]
    index[:len(order)] = order
    return score, index
