"""numpy emulation of the 8-bit search index (include/eat_search_q8.h), exact on both sides: the GPU tests demand equal
score bits and equal indices, not tolerances.

Quantiser, in float32 throughout: amax = max |x|, scale = amax / 127, code = rint(x / scale) (IEEE division, half to
even); a row with amax == 0 has scale 0 and zero codes.  normalize=True first divides each row by its norm with the very
operations of eat_rows_normalize: lane l of 64 adds the squares of elements 4 l + 256 i .. + 3 in ascending order with one
fused multiply-add each, a butterfly adds the lanes, then sqrt and one division per element.

Score: acc = sum_d cq cn in integers, s = float32(acc) * (sq * sn) in float32.  Top-k: np.lexsort on (n, -s) over the
eligible rows (tests/search_ref.py: eligible_ref), padded with (-inf, -1)."""
import numpy as np

from tests.search_ref import eligible_ref

F32, F64 = np.float32, np.float64


def fma_f32(a, b, c):
    """fl32(a * b + c) of float32 arrays with ONE rounding.  The product is exact in float64; the float64 sum is rounded to
    odd (its error term, from two-sum, decides), after which the rounding to float32 is the correct one: 53 >= 2 * 24 + 2."""
    p = a.astype(F64) * b.astype(F64)
    c = c.astype(F64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(e > 0, np.inf, -np.inf)
    s = np.where((e != 0) & even, np.nextafter(s, toward), s)
    return s.astype(F32)


def normalize_f32(x):
    """eat_rows_normalize bit for bit: (N, D) float32 -> (N, D) float32."""
    x = np.ascontiguousarray(x, dtype=F32)
    N, D = x.shape
    chunks = (D + 255) // 256
    padded = np.zeros((N, chunks * 256), dtype=F32)                   # fma(0, 0, ss) = ss: the pad changes nothing
    padded[:, :D] = x
    lanes = padded.reshape(N, chunks, 64, 4)
    ss = np.zeros((N, 64), dtype=F32)
    for i in range(chunks):
        for j in range(4):
            ss = fma_f32(lanes[:, i, :, j], lanes[:, i, :, j], ss)
    for o in (32, 16, 8, 4, 2, 1):
        ss = ss + ss[:, np.arange(64) ^ o]
    ss = ss[:, :1]
    with np.errstate(divide="ignore", invalid="ignore"):
        out = x / np.sqrt(ss)
    return np.where(ss > 0, out, F32(0)).astype(F32)


def quantize_ref(x, normalize=False):
    """(N, D) float32 -> (codes (N, D) int8, scale (N,) float32)."""
    x = normalize_f32(x) if normalize else np.ascontiguousarray(x, dtype=F32)
    amax = np.abs(x).max(axis=1)
    scale = (amax / F32(127.0)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        codes = np.rint(x / scale[:, None])
    codes = np.where(amax[:, None] > 0, codes, F32(0))
    assert bool((np.abs(codes) <= 127).all())
    return codes.astype(np.int8), scale


def padded(codes, ld=None, fill=0):
    """(N, D) int8 -> (N, ld) int8 with `fill` from column D on; ld: D rounded up to 16."""
    N, D = codes.shape
    ld = (D + 15) // 16 * 16 if ld is None else ld
    out = np.full((N, ld), fill, dtype=np.int8)
    out[:, :D] = codes
    return out


def acc_ref(codes, qcodes):
    """(Q, N) int64 dot products of the codes."""
    return qcodes.astype(np.int64) @ codes.astype(np.int64).T


def scores_q8_ref(codes, scale, qcodes, qscale):
    """(Q, N) float32: float32(acc) * (sq * sn)."""
    acc = acc_ref(codes, qcodes)
    assert int(np.abs(acc).max(initial=0)) < 2 ** 31
    both = (np.asarray(qscale, dtype=F32)[:, None] * np.asarray(scale, dtype=F32)[None, :]).astype(F32)
    return (acc.astype(F32) * both).astype(F32)


def topk_q8_ref(scores, k, skip=None):
    """scores (Q, N) float32 -> (score (Q, k) float32, index (Q, k) int32)."""
    Q, N = scores.shape
    ok = eligible_ref(N, Q, skip)
    out_s = np.full((Q, k), -np.inf, dtype=F32)
    out_i = np.full((Q, k), -1, dtype=np.int32)
    for q in range(Q):
        rows = np.flatnonzero(ok[q])
        order = rows[np.lexsort((rows, -scores[q, rows]))][:k]
        out_s[q, :len(order)] = scores[q, order]
        out_i[q, :len(order)] = order
    return out_s, out_i


def search_q8_ref(codes, scale, qcodes, qscale, k, skip=None):
    return topk_q8_ref(scores_q8_ref(codes, scale, qcodes, qscale), k, skip)
