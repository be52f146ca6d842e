"""eat_rows_quantize_q8 and eat_embed_search_q8 (csrc/search_q8.hip, include/eat_search_q8.h) alone against the emulation of
tests/search_q8_ref.py, through the raw C ABI and through the `ops` wrappers.

Both sides are exact - float32 divisions and an integer dot product - so every comparison is of bits: equal codes, equal
scale bits, equal score bits, equal indices.  No tolerance appears except in the one test that compares the quantised score
with the unquantised cosine, whose bound is derived there.

Codes are views into larger buffers filled with the byte 0x55, which also fills the bytes [D, ld) of every row handed to the
search (the kernel masks d >= D): a read outside a row's D values moves the integer sum.  Scales lie between NaNs.  `score`,
`index`, the workspace and the quantiser's outputs lie inside guard bands that must be intact afterwards, while every
element of the outputs must have been written; a second call must give the same bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, ops  # noqa: E402
from tests import search_q8_ref as R8  # noqa: E402
from tests import search_ref as R  # noqa: E402

DEV = torch.device("cuda:0")
GUARD = 67            # floats / ints around the fp32 and int32 buffers; odd: the view behind it starts on an odd word
BAND = 64             # bytes around the int8 buffers: the codes stay 16-byte aligned
FILL = 0x55           # what the int8 buffers hold where no code was put
SENTINEL = -7         # no index is ever -7
GROUP, TILE, BLOCKS = ops.SEARCH_Q8_GROUP, ops.SEARCH_Q8_TILE_ROWS, ops.SEARCH_Q8_BLOCKS
THREE_TILES = 2 * BLOCKS * TILE + 5          # block 0 of the fixed grid takes three tiles, every other block two


def _values(n, D, seed):
    return np.clip(0.75 + np.random.default_rng(seed).standard_normal((n, D)), 0, None).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _guarded_f32(x, word=1):
    """x (numpy fp32) as a device view that starts `word` 4-byte words into a NaN buffer, NaN right behind it."""
    buf = torch.full((word + x.size + GUARD,), float("nan"), device=DEV, dtype=torch.float32)
    view = buf[word:word + x.size].view(x.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    assert view.data_ptr() % 16 == (4 * word) % 16
    return view


def _guarded_codes(codes, ld=None):
    """codes (n, D) int8 -> a 16-byte aligned (n, ld) device view inside a buffer of FILL bytes, FILL from column D on."""
    rows = R8.padded(codes, ld, fill=FILL)
    buf = torch.full((BAND + rows.size + BAND,), FILL, device=DEV, dtype=torch.int8)
    view = buf[BAND:BAND + rows.size].view(rows.shape)
    view.copy_(torch.from_numpy(rows))
    assert view.data_ptr() % 16 == 0
    return view


def _search(codes, scale, qcodes, qscale, k, skip=None, ld=None):
    """codes (N, D), qcodes (Q, D) int8 and their scales, numpy -> (score, index) numpy, straight through the C ABI with
    `skip` as it is.  Checks the guard bands, that every output was written, that a second call gives the same bits and that
    ops.embed_search_q8 gives them too."""
    (N, D), Q = codes.shape, qcodes.shape[0]
    b, q = _guarded_codes(codes, ld), _guarded_codes(qcodes)
    sn, sq = _guarded_f32(np.asarray(scale, dtype=np.float32)), _guarded_f32(np.asarray(qscale, dtype=np.float32))
    need = _lib.lib().eat_embed_search_q8_ws_bytes(Q, k)
    assert need > 0
    skip_d = None if skip is None else torch.tensor(skip, dtype=torch.int32).reshape(Q, 2).to(DEV)
    outs = []
    for _ in range(2):
        sbuf = torch.full((GUARD + Q * k + GUARD,), float("nan"), device=DEV, dtype=torch.float32)
        ibuf = torch.full((GUARD + Q * k + GUARD,), SENTINEL, device=DEV, dtype=torch.int32)
        ws = torch.full((need + 64,), 0xA5, device=DEV, dtype=torch.uint8)
        score, index = sbuf[GUARD:GUARD + Q * k].view(Q, k), ibuf[GUARD:GUARD + Q * k].view(Q, k)
        _lib.call("eat_embed_search_q8", b.data_ptr(), b.shape[1], sn.data_ptr(), N, D, q.data_ptr(), q.shape[1], sq.data_ptr(), Q, k,
                  None if skip_d is None else skip_d.data_ptr(), ws.data_ptr(), need, score.data_ptr(), index.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool(torch.isnan(sbuf[:GUARD]).all()) and bool(torch.isnan(sbuf[GUARD + Q * k:]).all()), "a guard of score was written"
        assert bool((ibuf[:GUARD] == SENTINEL).all()) and bool((ibuf[GUARD + Q * k:] == SENTINEL).all()), "a guard of index was written"
        assert bool((ws[need:] == 0xA5).all()), "the workspace was overrun"
        assert not bool(torch.isnan(score).any()), "an element of score was not written, or a scale was read outside its vector"
        assert not bool((index == SENTINEL).any()), "an element of index was not written"
        outs.append((score.clone(), index.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "two calls, two results"
    if skip is None or all(-2 ** 31 <= int(v) < 2 ** 31 for v in np.asarray(skip).reshape(-1)):
        s2, i2 = ops.embed_search_q8(b, sn, D, q, sq, k, skip)
        assert s2.shape == (Q, k) and s2.dtype == torch.float32 and i2.dtype == torch.int32
        assert torch.equal(s2, outs[0][0]) and torch.equal(i2, outs[0][1]), "ops.embed_search_q8 and the C ABI differ"
    return outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy()


def _check(tag, codes, scale, qcodes, qscale, k, skip=None, ld=None):
    """Equal score bits and equal indices, or the first place where they differ."""
    score, index = _search(codes, scale, qcodes, qscale, k, skip, ld)
    ref_s, ref_i = R8.search_q8_ref(codes, scale, qcodes, qscale, k, skip)
    wrong = np.argwhere((index != ref_i) | (_bits(score) != _bits(ref_s)))
    print(f"SEARCH_Q8 {tag}: {len(wrong)} of {index.size} results differ from the emulation")
    if len(wrong):
        q, j = wrong[0]
        raise AssertionError((tag, "first difference at", (int(q), int(j)), "got", (float(score[q, j]), int(index[q, j])),
                              "want", (float(ref_s[q, j]), int(ref_i[q, j]))))
    return score, index


def _quantized(n, D, seed):
    """Rows of clip(0.75 + N(0, 1), 0), normalised and quantised by the emulation."""
    return R8.quantize_ref(_values(n, D, seed), normalize=True)


# ---------------------------------------------------------------------------------------------------------------- quantiser
def _quantize(x, normalize, word, ld=None):
    """x numpy (N, D) -> (codes (N, ld), scale (N,)) numpy through the C ABI, from a base `word` words into a NaN buffer."""
    N, D = x.shape
    ld = ops.q8_ld(D) if ld is None else ld
    xv = _guarded_f32(x, word)
    cbuf = torch.full((BAND + N * ld + BAND,), FILL, device=DEV, dtype=torch.int8)
    sbuf = torch.full((GUARD + N + GUARD,), float("nan"), device=DEV, dtype=torch.float32)
    codes, scale = cbuf[BAND:BAND + N * ld].view(N, ld), sbuf[GUARD:GUARD + N]
    outs = []
    for _ in range(2):
        codes.fill_(FILL)
        scale.fill_(float("nan"))
        _lib.call("eat_rows_quantize_q8", xv.data_ptr(), N, D, normalize, codes.data_ptr(), ld, scale.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool((cbuf[:BAND] == FILL).all()) and bool((cbuf[BAND + N * ld:] == FILL).all()), "a guard of codes was written"
        assert bool(torch.isnan(sbuf[:GUARD]).all()) and bool(torch.isnan(sbuf[GUARD + N:]).all()), "a guard of scale was written"
        assert not bool(torch.isnan(scale).any()), "an element of scale was not written"
        assert not bool(codes[:, D:].any()), "a pad byte is not zero"
        outs.append((codes.clone(), scale.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "two calls, two results"
    if ld == ops.q8_ld(D):
        c2, s2 = ops.rows_quantize_q8(xv, normalize=bool(normalize))
        assert c2.shape == (N, ld) and c2.dtype == torch.int8 and s2.dtype == torch.float32
        assert torch.equal(c2, outs[0][0]) and torch.equal(s2, outs[0][1]), "ops.rows_quantize_q8 and the C ABI differ"
    return outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy(), xv


_QSEEN = {}


@pytest.mark.parametrize("word", [1, 0], ids=["odd_word", "aligned"])
@pytest.mark.parametrize("D", [1, 7, 16, 17, 130, 2184])
def test_quantiser_equals_the_emulation_bit_for_bit(D, word):
    N = 37                                                  # ten blocks of four rows, the last one ragged
    x = (3.0 * np.random.default_rng(D).standard_normal((N, D))).astype(np.float32)
    x[5] = 0.0                                              # a zero row: scale 0, zero codes
    x[6, D // 2] = -100.0                                   # the largest element is negative: it reaches -127
    x[7] = np.abs(x[7]) * np.float32(1e-15)                 # small values: the scale is relative
    for normalize in (0, 1):
        codes, scale, xv = _quantize(x, normalize, word)
        ref_c, ref_s = R8.quantize_ref(x, normalize=bool(normalize))
        bad_c, bad_s = int((codes[:, :D] != ref_c).sum()), int((_bits(scale) != _bits(ref_s)).sum())
        print(f"QUANTIZE D={D} word={word} normalize={normalize}: {bad_c} codes and {bad_s} scales differ from the emulation")
        assert bad_c == 0 and bad_s == 0
        assert scale[5] == 0.0 and not codes[5].any()
        assert codes[6, D // 2] == -127 and int(codes.min()) >= -127 and int(np.abs(codes[np.arange(N) != 5]).max(axis=1).min()) == 127
        # the bits do not depend on the alignment, nor on the load width it selects
        other = _QSEEN.setdefault((D, normalize), (codes, scale))
        assert np.array_equal(other[0], codes) and np.array_equal(_bits(other[1]), _bits(scale))
    # normalising in the same launch = quantising what eat_rows_normalize gives
    unit = ops.rows_normalize(xv)
    c0, s0 = ops.rows_quantize_q8(unit, normalize=False)
    assert np.array_equal(c0.cpu().numpy(), codes) and np.array_equal(_bits(s0.cpu().numpy()), _bits(scale))
    # a wider row stride: the same codes, zeros up to ld
    wide, wide_s, _ = _quantize(x, 1, word, ld=ops.q8_ld(D) + 32)
    assert np.array_equal(wide[:, :D], codes[:, :D]) and not wide[:, D:].any() and np.array_equal(_bits(wide_s), _bits(scale))


# ---------------------------------------------------------------------------------------------------------- fragment layout
@pytest.mark.parametrize("D", [64, 128, 200])
def test_fragment_layout_with_codes_asymmetric_in_row_query_and_k(D):
    """Codes fed directly, different along n, q and d, with scales that differ per row and per query: a lane map that swaps
    row and query, permutes the rows of a tile or the accumulator registers, or takes the two operands from different k
    gives other sums."""
    N, Q, k = 40, 19, 40
    n, q, d = np.arange(N)[:, None], np.arange(Q)[:, None], np.arange(D)[None, :]
    codes = (((7 * n + 3 * d) % 255) - 127).astype(np.int8)
    qcodes = (((5 * q + 11 * d) % 255) - 127).astype(np.int8)
    scale = (1 + np.arange(N) / 8).astype(np.float32)
    qscale = (1 + np.arange(Q) / 4).astype(np.float32)
    _check(f"layout D={D}", codes, scale, qcodes, qscale, k)


# ------------------------------------------------------------------------------------------------------------------- shapes
SHAPES = [(1, 1, 1, 1), (5, 7, 3, 5),
          (3, 7, 2, 5),                                   # k > N: padding
          (257, 33, 9, 16), (4099, 2184, 2, 128)]
SHAPES += [(100, D, 3, 8) for D in (15, 16, 17, 63, 64, 65, 127, 129)]        # the edges of a 16-byte piece and of a k-step
SHAPES += [(300, 36, Q, 8) for Q in (GROUP, GROUP + 1, 2 * GROUP + 1)]        # a full group; and one more; two and one more
SHAPES += [(THREE_TILES, 4, 1, 8), (THREE_TILES, 4, GROUP, 8)]                # more than one tile per block, alone and in a full group
SHAPES += [(150, 4000, GROUP, 8),                         # 64 x 4000 bytes of queries exceed the LDS: the group is halved
           (140, 1300, GROUP + 3, 128),                   # so do 64 lists of 128 entries beside 64 x 1328 bytes
           (6, 41004, 2, 3)]                              # a long row: not even 4 queries fit


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_search_equals_the_emulation(shape):
    N, D, Q, k = shape
    codes, scale = _quantized(N, D, seed=N + D)
    qcodes, qscale = _quantized(Q, D, seed=N + D + 1)
    score, index = _check(f"{shape}", codes, scale, qcodes, qscale, k)
    if shape == (3, 7, 2, 5):
        assert bool((index[:, 3:] == -1).all()) and bool((index[:, :3] >= 0).all()) and bool(np.isneginf(score[:, 3:]).all())


def test_a_wider_row_stride_gives_the_same_bits():
    N, D, Q, k = 200, 33, 3, 8
    codes, scale = _quantized(N, D, seed=1)
    qcodes, qscale = _quantized(Q, D, seed=2)
    narrow = _check("ld = 48", codes, scale, qcodes, qscale, k)
    wide = _check("ld = 112", codes, scale, qcodes, qscale, k, ld=112)
    assert np.array_equal(_bits(narrow[0]), _bits(wide[0])) and np.array_equal(narrow[1], wide[1])


# -------------------------------------------------------------------------------------------------------------------- range
def test_the_largest_sums_come_back_exact():
    """D = 131072 with every code at +-127: acc = +-127^2 x 131072 = +-2 114 060 288, 33 423 360 below 2^31."""
    D, k = 131072, 3
    codes = np.stack([np.full(D, 127), np.full(D, -127), np.where(np.arange(D) % 2, -127, 127)]).astype(np.int8)
    qcodes = codes[:2].copy()
    scale, qscale = np.ones(3, dtype=np.float32), np.ones(2, dtype=np.float32)
    acc = R8.acc_ref(codes, qcodes)
    assert acc.tolist() == [[2114060288, -2114060288, 0], [-2114060288, 2114060288, 0]]
    score, index = _check("range", codes, scale, qcodes, qscale, k)
    assert index.tolist() == [[0, 2, 1], [1, 2, 0]]
    assert score.tolist() == [[2114060288.0, 0.0, -2114060288.0]] * 2 and np.float32(2114060288) == 2114060288


# ------------------------------------------------------------------------------------------------------- ties and ordering
def test_identical_rows_tie_exactly_in_ascending_index():
    """Copies of one row at the first row, at the last row of a tile and at the last row of the bank: whatever block,
    wavefront and lane meets them, their scores are bit-equal for every query."""
    Q, D, k = 9, 36, 128
    N = TILE + 37                                          # two tiles, two blocks
    x, xq = _values(N, D, seed=1), _values(Q, D, seed=2)
    twins = [0, TILE - 1, N - 1]
    x[twins] = xq[0]                                       # the best rows of query 0; anywhere in the order of the others
    codes, scale = R8.quantize_ref(x, normalize=True)
    qcodes, qscale = R8.quantize_ref(xq, normalize=True)
    score, index = _check("twins", codes, scale, qcodes, qscale, k)
    assert index[0, :3].tolist() == twins and score[0, 0] == score[0, 1] == score[0, 2]
    for q in range(Q):
        at = [int(np.flatnonzero(index[q] == t)[0]) for t in twins if t in index[q]]      # those inside the first k: the lower rows
        assert at == list(range(at[0], at[0] + len(at))), (q, at)
        assert len(set(_bits(score[q, at]).tolist())) == 1


@pytest.mark.parametrize("shape", [(700, 33, 2, 128), (THREE_TILES, 4, 2, 128)], ids=lambda s: "x".join(map(str, s)))
def test_a_bank_of_one_repeated_row_returns_the_first_k_rows(shape):
    N, D, Q, k = shape
    row, row_s = _quantized(1, D, seed=3)
    qcodes, qscale = _quantized(Q, D, seed=4)
    score, index = _check(f"repeated {shape}", np.repeat(row, N, axis=0), np.repeat(row_s, N), qcodes, qscale, k)
    assert np.array_equal(index, np.tile(np.arange(k, dtype=np.int32), (Q, 1)))
    assert bool((score == score[:, :1]).all())


def test_exclusion_ranges():
    Q, D, k = 7, 33, 12
    N = 3 * TILE + 7
    x, xq = _values(N, D, seed=7), _values(Q, D, seed=8)
    x[40:45] = xq[3]                                       # the true top rows of query 3 ...
    big = 2 ** 31 - 1
    skip = [[0, 0],                                        # empty
            [50, 20],                                      # lo > hi: nothing
            [0, N],                                        # the whole bank: all -1
            [40, 45],                                      # ... hidden
            [TILE - 3, TILE + 4],                          # straddles a tile edge
            [-5, 10],                                      # clamped below
            [N - 4, big]]                                  # clamped above
    codes, scale = R8.quantize_ref(x, normalize=True)
    qcodes, qscale = R8.quantize_ref(xq, normalize=True)
    free, free_i = _check("no exclusion", codes, scale, qcodes, qscale, k)
    score, index = _check("exclusion", codes, scale, qcodes, qscale, k, skip)
    assert np.array_equal(index[:2], free_i[:2]) and np.array_equal(score[:2], free[:2])
    assert bool((index[2] == -1).all()) and bool(np.isneginf(score[2]).all())
    assert sorted(free_i[3, :5].tolist()) == [40, 41, 42, 43, 44] and not set(index[3].tolist()) & {40, 41, 42, 43, 44}
    assert not set(index[4].tolist()) & set(range(TILE - 3, TILE + 4))
    assert int(index[5].min()) >= 10 and int(index[6].max()) < N - 4
    with pytest.raises(_lib.EatHipError, match="must fit int32"):
        ops.embed_search_q8(_guarded_codes(codes), _guarded_f32(scale), D, _guarded_codes(qcodes), _guarded_f32(qscale), k,
                            [[0, 2 ** 31]] * Q)
    # k larger than what is left: all rows but the first five hidden
    score, index = _check("exclusion and padding", codes, scale, qcodes, qscale, 100, [[5, N]] * Q)
    assert bool((index[:, 5:] == -1).all()) and sorted(index[0, :5].tolist()) == [0, 1, 2, 3, 4]


def test_zero_rows_score_zero_and_nothing_is_nan():
    N, D, Q, k = 70, 19, 3, 70
    x, xq = _values(N, D, seed=9), _values(Q, D, seed=10)
    x[3] = 0.0
    x[N - 1] = 0.0
    xq[1] = 0.0
    codes, scale = (t.cpu().numpy() for t in ops.rows_quantize_q8(_guarded_f32(x)))
    qcodes, qscale = (t.cpu().numpy() for t in ops.rows_quantize_q8(_guarded_f32(xq)))
    assert scale[3] == 0 and scale[N - 1] == 0 and qscale[1] == 0 and not codes[3].any() and not qcodes[1].any()
    score, index = _check("zero rows", codes[:, :D], scale, qcodes[:, :D], qscale, k)
    assert not bool(np.isnan(score).any())
    assert bool((_bits(score[1]) == 0).all()) and index[1].tolist() == list(range(N))       # a zero query: every score +0.0, by row
    for q in (0, 2):                                                                       # zero rows: the last two, by row
        assert index[q, -2:].tolist() == [3, N - 1] and bool((score[q, -2:] == 0.0).all()) and float(score[q, -3]) > 0


# --------------------------------------------------------------------------------------------- against the unquantised score
@pytest.mark.parametrize("D", [130, 2184])
def test_the_score_lies_within_the_quantisation_bound_of_the_cosine(D):
    """x = scale (code + e) with |e| <= 0.5 per element, so the quantised dot product differs from the true one by
    sq sn sum (cq en + cn eq + eq en), at most sq sn (0.5 sum |cq| + 0.5 sum |cn| + 0.25 D).  The 2e-5 on top is the
    project's fp32 bar: the rounding of the scales, of the final multiplies and of the conversion of the sum."""
    N, Q, k = 1000, 5, 10
    bank = R.normalize_ref(_values(N, D, seed=D)).astype(np.float32)
    queries = R.normalize_ref(_values(Q, D, seed=D + 1)).astype(np.float32)
    c, sn = ops.rows_quantize_q8(_guarded_f32(bank), normalize=False)
    cq, sq = ops.rows_quantize_q8(_guarded_f32(queries), normalize=False)
    score, index = (t.cpu().numpy() for t in ops.embed_search_q8(c, sn, D, cq, sq, k))
    c, sn, cq, sq = (t.cpu().numpy().astype(np.float64) for t in (c, sn, cq, sq))
    s64 = R.scores_ref(bank, queries, normalize=False)
    worst = 0.0
    for q in range(Q):
        for j in range(k):
            n = int(index[q, j])
            assert 0 <= n < N
            bound = sq[q] * sn[n] * (0.5 * np.abs(cq[q]).sum() + 0.5 * np.abs(c[n]).sum() + 0.25 * D) + 2e-5
            err = abs(float(score[q, j]) - s64[q, n])
            worst = max(worst, err / bound)
            assert err <= bound, (q, j, n, err, bound)
    print(f"SEARCH_Q8 D={D}: largest |score - cosine| / bound = {worst:.3f}; "
          f"largest |score - cosine| = {float(np.abs(score - np.take_along_axis(s64, index.astype(np.int64), 1)).max()):.3e}")


# -------------------------------------------------------------------------------------------------- offsets beyond 2^31 bytes
def test_offsets_beyond_2_to_the_31_bytes():
    """A zero bank of (2^20 + 8) rows of 2048 bytes, 2.1 GB: rows from 2^20 on start past byte 2^31.  Query codes are
    planted there; every other row scores exactly 0.0 and ties resolve by index, so the reference needs the planted rows alone."""
    N, D, Q, k = 2 ** 20 + 8, 2048, 3, 8
    assert N * D > 2 ** 31 and (N - 9) * D < 2 ** 31
    qcodes, qscale = _quantized(Q, D, seed=11)
    planted = {2 ** 20 + 1: 0, 2 ** 20 + 4: 1, 2 ** 20 + 7: 2, 2 ** 20 - 1: 2}
    rows = np.array(sorted(planted))
    scale_rows = np.array([0.5, 1.0, 0.25, 2.0], dtype=np.float32) / 127
    bank = torch.zeros((N, D), device=DEV, dtype=torch.int8)
    scale = torch.full((N,), 1.0 / 127, device=DEV, dtype=torch.float32)
    try:
        for row, s in zip(rows, scale_rows):
            bank[row] = torch.from_numpy(qcodes[planted[int(row)]]).to(DEV)
            scale[row] = float(s)
        score, index = (t.cpu().numpy() for t in ops.embed_search_q8(bank, scale, D, torch.from_numpy(qcodes).to(DEV),
                                                                    torch.from_numpy(qscale).to(DEV), k))
    finally:
        del bank
        torch.cuda.empty_cache()
    ref = R8.scores_q8_ref(np.stack([qcodes[planted[int(r)]] for r in rows]), scale_rows, qcodes, qscale)       # (Q, 4), all > 0
    assert bool((ref > 0).all())
    for q in range(Q):
        order = np.lexsort((rows, -ref[q]))
        assert index[q].tolist() == rows[order].tolist() + [0, 1, 2, 3], (q, index[q])
        assert np.array_equal(_bits(score[q, :4]), _bits(ref[q, order])) and bool((_bits(score[q, 4:]) == 0).all())


def test_wrappers_refuse_bad_operands():
    codes, scale = torch.zeros((5, 16), device=DEV, dtype=torch.int8), torch.zeros(5, device=DEV)
    q, qs = torch.zeros((2, 16), device=DEV, dtype=torch.int8), torch.zeros(2, device=DEV)
    with pytest.raises(_lib.EatHipError, match="bank codes must be a contiguous"):
        ops.embed_search_q8(codes.float(), scale, 8, q, qs, 3)
    with pytest.raises(_lib.EatHipError, match="query codes need a 16-byte aligned base and a row stride"):
        ops.embed_search_q8(codes, scale, 8, torch.zeros((2, 8), device=DEV, dtype=torch.int8), qs, 3)
    with pytest.raises(_lib.EatHipError, match="at least D = 17"):
        ops.embed_search_q8(codes, scale, 17, q, qs, 3)
    with pytest.raises(_lib.EatHipError, match=r"bank scale must be \(5,\)"):
        ops.embed_search_q8(codes, scale[:4], 8, q, qs, 3)
    with pytest.raises(_lib.EatHipError, match="need 1 <= k <= 128"):
        ops.embed_search_q8(codes, scale, 8, q, qs, 129)
    with pytest.raises(_lib.EatHipError, match="need 1 <= D <= 131072"):
        ops.embed_search_q8(codes, scale, 0, q, qs, 3)
    with pytest.raises(_lib.EatHipError, match=r"skip must be \(2, 2\)"):
        ops.embed_search_q8(codes, scale, 8, q, qs, 3, [[0, 1]])
    with pytest.raises(_lib.EatHipError, match=r"x must be \(N, 1 <= D <= 131072\)"):
        ops.rows_quantize_q8(torch.zeros(8, device=DEV))
    with pytest.raises(_lib.EatHipError, match="codes must have 5 rows"):
        ops.rows_quantize_q8(torch.zeros((5, 8), device=DEV), codes=torch.zeros((4, 16), device=DEV, dtype=torch.int8))
    score, index = ops.embed_search_q8(codes, scale, 8, q, qs, 3)
    assert index.tolist() == [[0, 1, 2]] * 2 and bool((score == 0).all())
