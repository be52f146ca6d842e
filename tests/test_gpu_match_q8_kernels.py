"""eat_embed_match_q8 (csrc/match_q8.hip, include/eat_match_q8.h) alone, through the raw C ABI and through
`ops.embed_match_q8`, with the harness of tests/test_gpu_match_kernels.py and the operands of
tests/test_gpu_search_q8_kernels.py: codes are 16-byte aligned views into buffers of the byte 0x55, which also fills the bytes
[D, ld) of every bank and query row (the kernel masks d >= D), scales lie between NaNs, `score`, `index` and the workspace
lie inside guard bands that must be intact afterwards, every element of both outputs must have been written, and a second
call must give the same bits.

Where the expected bits come from: the numpy emulation alone.  tests/search_q8_ref.py gives the row scores
S[j, n] = float32(integer dot product) * (sq[j] * sn[n]) exactly, and tests/match_ref.py in float32 - sequential additions in
ascending j, one IEEE division - turns them into the score bits and the indices of eat_embed_match_q8.  Every comparison
demands EQUALITY of bits and indices; no tolerance appears.  S is computed once per case and shared."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, ops  # noqa: E402
from tests import match_ref as M  # noqa: E402
from tests import search_q8_ref as R8  # noqa: E402
from tests.test_gpu_search_q8_kernels import (BLOCKS, DEV, GUARD, SENTINEL, TILE, _bits, _guarded_codes, _guarded_f32,  # noqa: E402
                                               _values)

BIG = 2 ** 31 - 1
MANY = 2 * BLOCKS * TILE + 5              # block 0 of the fixed grid takes three tiles; the last tile holds 5 rows
SEPS, KS = (0, 1, 5, None, 4096), (1, 10, 128)          # None: L


class Case:
    """A q8 bank, its files and a quantised clip on the device, and the emulation's row scores S (L, N)."""

    def __init__(self, codes, scale, seg, qcodes, qscale, ld=None, qld=None):
        (self.N, self.D), self.L = codes.shape, qcodes.shape[0]
        self.seg = [int(v) for v in seg]
        assert self.seg[0] == 0 and self.seg[-1] == self.N
        self.b, self.q = _guarded_codes(codes, ld), _guarded_codes(qcodes, qld)
        self.sn = _guarded_f32(np.asarray(scale, dtype=np.float32))
        self.sq = _guarded_f32(np.asarray(qscale, dtype=np.float32))
        self.seg_d = torch.tensor(self.seg, dtype=torch.int32, device=DEV)
        self.S = R8.scores_q8_ref(codes, scale, qcodes, qscale)
        assert self.S.dtype == np.float32 and self.S.shape == (self.L, self.N)

    def match(self, k, sep, min_score=-np.inf, skip=None, wrapper=True):
        """-> (score, index) numpy, straight through the C ABI; checks the guard bands, that every output was written, that
        a second call gives the same bits and that ops.embed_match_q8 gives them too."""
        need = _lib.lib().eat_embed_match_q8_ws_bytes(self.N, self.L, k)
        assert need > 0
        lo, hi = (0, 0) if skip is None else skip
        outs = []
        for _ in range(2):
            sbuf = torch.full((GUARD + k + GUARD,), float("nan"), device=DEV, dtype=torch.float32)
            ibuf = torch.full((GUARD + k + GUARD,), SENTINEL, device=DEV, dtype=torch.int32)
            ws = torch.full((need + 64,), 0xA5, device=DEV, dtype=torch.uint8)
            score, index = sbuf[GUARD:GUARD + k], ibuf[GUARD:GUARD + k]
            _lib.call("eat_embed_match_q8", self.b.data_ptr(), self.b.shape[1], self.sn.data_ptr(), self.N, self.D, self.seg_d.data_ptr(),
                      len(self.seg) - 1, self.q.data_ptr(), self.q.shape[1], self.sq.data_ptr(), self.L, k, sep, float(min_score), lo, hi,
                      ws.data_ptr(), need, score.data_ptr(), index.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert bool(torch.isnan(sbuf[:GUARD]).all()) and bool(torch.isnan(sbuf[GUARD + k:]).all()), "a guard of score was written"
            assert bool((ibuf[:GUARD] == SENTINEL).all()) and bool((ibuf[GUARD + k:] == SENTINEL).all()), "a guard of index was written"
            assert bool((ws[need:] == 0xA5).all()), "the workspace was overrun"
            assert not bool(torch.isnan(score).any()), "an element of score was not written, or a sum read outside its row"
            assert not bool((index == SENTINEL).any()), "an element of index was not written"
            outs.append((score.clone(), index.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "two calls, two results"
        if wrapper:
            s2, i2 = ops.embed_match_q8(self.b, self.sn, self.D, self.seg_d, self.q, self.sq, k, sep, min_score, skip)
            assert s2.shape == (k,) and s2.dtype == torch.float32 and i2.dtype == torch.int32
            assert torch.equal(s2, outs[0][0]) and torch.equal(i2, outs[0][1]), "ops.embed_match_q8 and the C ABI differ"
        return outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy()

    def check(self, k, sep, min_score=-np.inf, skip=None, wrapper=True):
        """The kernel's result must be match_ref's on S in float32, bit for bit."""
        score, index = self.match(k, sep, min_score, skip, wrapper)
        want_s, want_i = M.match_ref(self.S, self.seg, k, sep, min_score, skip)
        assert want_s.dtype == np.float32
        tag = (self.N, self.D, self.L, k, sep, min_score, skip)
        assert np.array_equal(index, want_i.astype(np.int32)), (tag, index, want_i)
        assert np.array_equal(_bits(score), _bits(want_s)), (tag, score, want_s)
        return score, index


def _segments(lengths):
    return [0] + np.cumsum(lengths).tolist()


def _ragged(N_about, L, seed, exact=None):
    """File bounds with lengths drawn from around L and around the tile of 128 rows; exact: the total to end on."""
    rng = np.random.default_rng(seed)
    choices = sorted(v for v in {1, L - 1, L, L + 1, 127, 128, 129, 260} if v >= 1)
    lengths = []
    while sum(lengths) < N_about:
        lengths.append(int(rng.choice(choices)))
    if exact is not None:
        lengths[-1] -= sum(lengths) - exact
        assert lengths[-1] >= 1
    return _segments(lengths)


def _random_case(N_about, D, L, seed, exact=None, **strides):
    seg = _ragged(N_about, L, seed, exact)
    codes, scale = R8.quantize_ref(_values(seg[-1], D, seed), normalize=True)
    qcodes, qscale = R8.quantize_ref(_values(L, D, seed + 1), normalize=True)
    return Case(codes, scale, seg, qcodes, qscale, **strides)


def _skips(case):
    N, seg = case.N, case.seg
    f = max(range(len(seg) - 1), key=lambda j: (seg[j + 1] - seg[j] >= 64, -abs(seg[j] - N // 2)))      # a long file near the middle
    if N < 180:                                            # a few rows: the same four forms, scaled down so that rows stay eligible
        return [None, (seg[f], min(seg[f + 1], seg[f] + 1 + N // 3)), (-5, N // 3), (N - N // 3, BIG)]
    return [None, (seg[f], seg[f + 1]), (-5, 70), (N - 90, BIG)]


def _cross(case, full):
    """Every sep with every skip form; full: with every k as well, else k = 10."""
    first = True
    for sep in SEPS:
        sep = case.L if sep is None else sep
        for k in (KS if full else (10,)):
            for skip in _skips(case):
                case.check(k, sep, skip=skip, wrapper=first or (full and k == 10 and skip is None))
                first = False


# D = 130: the tail-only k path, no multiple of 16; D = 600: one full batch of 8 k-steps and a ragged tail.
# L = 65 and 130 take two and three groups of query rows, the last one on a smaller instance.
@pytest.mark.parametrize("D", [130, 600])
@pytest.mark.parametrize("L", [1, 2, 15, 16, 17, 63, 64, 65, 130])
def test_group_and_tile_edges(L, D):
    case = _random_case(700, D, L, seed=10 * L + D)
    _cross(case, full=(L, D) in ((17, 130), (65, 600)))
    # a threshold between two returned scores cuts the list there
    free = case.check(10, L)
    cuts = [a for a in range(9) if free[0][a] > free[0][a + 1] > -np.inf]
    if cuts:
        cut = cuts[0]
        min_score = np.float32(0.5) * (free[0][cut] + free[0][cut + 1])
        if not free[0][cut] > min_score > free[0][cut + 1]:                 # neighbours in fp32: the upper one itself
            min_score = free[0][cut]
        score, index = case.check(10, L, min_score=float(min_score))
        assert index[:cut + 1].tolist() == free[1][:cut + 1].tolist() and bool((index[cut + 1:] == -1).all())
        assert bool(np.isneginf(score[cut + 1:]).all())


@pytest.mark.parametrize("shape", [(300, 4000, 40),        # 64 rows of 4000 bytes exceed the LDS: groups of 32 + 8
                                   (6, 41004, 3)],         # a long row: groups of 2, then 1
                         ids=lambda s: "x".join(map(str, s)))
def test_groups_that_the_lds_halves(shape):
    N, D, L = shape
    seg = [0, N] if N < 10 else _ragged(N, L, seed=N, exact=N)
    codes, scale = R8.quantize_ref(_values(N, D, N + D), normalize=True)
    qcodes, qscale = R8.quantize_ref(_values(L, D, N + D + 1), normalize=True)
    _cross(Case(codes, scale, seg, qcodes, qscale), full=False)


def test_the_largest_sums_come_back_exact():
    """D = 131072 with every code at +-127: acc = +-127^2 x 131072 = +-2 114 060 288 per row, and a window adds two of them."""
    N, D, L = 40, 131072, 2
    kinds = np.stack([np.full(D, 127), np.full(D, -127), np.where(np.arange(D) % 2, -127, 127)]).astype(np.int8)
    which = np.arange(N) % 3
    codes = kinds[which]
    qcodes = kinds[:2].copy()
    case = Case(codes, np.ones(N, dtype=np.float32), [0, 13, 14, N], qcodes, np.ones(L, dtype=np.float32))
    assert float(np.abs(case.S).max()) == 2114060288.0
    score, index = case.check(128, 0)
    pairs = [n for n in range(N - 1) if which[n] == 0 and which[n + 1] == 1 and n + L <= (13 if n < 13 else 14 if n < 14 else N)]
    assert pairs and index[:len(pairs)].tolist() == pairs and bool((score[:len(pairs)] == np.float32(2114060288.0)).all())
    for sep in (1, 5, 4096):
        case.check(10, sep)


@pytest.mark.parametrize("L", [3, 64])
def test_more_tiles_than_blocks_and_a_tail_tile_of_five_rows(L):
    D = 20
    case = _random_case(MANY, D, L, seed=17 + L, exact=MANY)
    assert case.N == MANY and (case.N % TILE) == 5
    _, index = case.check(128, 3)
    assert int(index.min()) >= 0
    case.check(10, 5, skip=(MANY // 2, MANY // 2 + 5000))
    last = case.seg[-2]
    case.check(10, 0, skip=(0, last))                       # what is left lies in the last file, next to the tail tile


@pytest.mark.parametrize("D", [64, 200])
def test_fragment_layout_with_codes_asymmetric_in_row_query_and_k(D):
    """Codes fed directly, different along n, j and d, with scales that differ per row and per query row: a store path that
    swaps row and query row, permutes the rows of a tile or the accumulator registers gives other means."""
    N, L = 40, 19
    n, j, d = np.arange(N)[:, None], np.arange(L)[:, None], np.arange(D)[None, :]
    codes = (((7 * n + 3 * d) % 255) - 127).astype(np.int8)
    qcodes = (((5 * j + 11 * d) % 255) - 127).astype(np.int8)
    scale = (1 + np.arange(N) / 8).astype(np.float32)
    qscale = (1 + np.arange(L) / 4).astype(np.float32)
    for seg in ([0, N], [0, L, N]):
        case = Case(codes, scale, seg, qcodes, qscale)
        score, index = case.check(128, 0)
        assert int((index >= 0).sum()) == sum(max(0, b - a - L + 1) for a, b in zip(seg, seg[1:]))
        case.check(10, 3)
    # every row score on its own: L = 1 windows of each query row return S[j] itself
    for jj in (0, 7, 18):
        one = Case(codes, scale, [0, N], qcodes[jj:jj + 1], qscale[jj:jj + 1])
        score, index = one.check(N, 0)
        assert np.array_equal(_bits(np.sort(score)), _bits(np.sort(case.S[jj])))


def test_a_wider_row_stride_gives_the_same_bits():
    L, D = 5, 33
    seg = _ragged(300, L, seed=3)
    codes, scale = R8.quantize_ref(_values(seg[-1], D, 1), normalize=True)
    qcodes, qscale = R8.quantize_ref(_values(L, D, 2), normalize=True)
    narrow = Case(codes, scale, seg, qcodes, qscale).check(10, L)
    wide = Case(codes, scale, seg, qcodes, qscale, ld=112, qld=80).check(10, L)
    assert np.array_equal(_bits(narrow[0]), _bits(wide[0])) and np.array_equal(narrow[1], wide[1])


def test_a_file_stored_twice_ties_exactly():
    """One file's rows at rows 60 .. 99 and again at 500 .. 539 (another position within the tile, another block): the means
    of corresponding start rows are bit-equal, so both are returned next to each other, the lower row first."""
    D, L = 36, 5
    x = _values(700, D, seed=21)
    x[60:100] = x[60] + 0.1 * x[60:100]                         # rows of one sound: every start row of the file outscores the rest
    x[500:540] = x[60:100]
    seg = [0, 60, 100, 333, 500, 540, 700]
    codes, scale = R8.quantize_ref(x, normalize=True)
    case = Case(codes, scale, seg, codes[70:75].copy(), scale[70:75].copy())       # the clip is rows 70 .. 74 of the file
    score, index = case.check(10, 4)
    assert index[:2].tolist() == [70, 510] and score[0] == score[1]
    score, index = case.check(128, 0)
    at = {int(n): j for j, n in enumerate(index) if n >= 0}
    twins = list(range(60, 100 - L + 1))
    assert sorted(at[n] for n in twins) == list(range(0, 2 * len(twins), 2))       # the best 72 places are the 36 pairs
    for n in twins:
        assert at[n + 440] == at[n] + 1 and score[at[n]] == score[at[n] + 1], n


def test_a_file_of_identical_rows_keeps_what_the_reference_names():
    D, L = 33, 4
    x = _values(300, D, seed=22)
    x[100:150] = x[100]
    queries = x[100] + 0.1 * _values(L, D, seed=23)             # near the repeated row: its file's start rows outscore the rest
    codes, scale = R8.quantize_ref(x, normalize=True)
    qcodes, qscale = R8.quantize_ref(queries, normalize=True)
    case = Case(codes, scale, [0, 100, 150, 300], qcodes, qscale)
    for sep in (0, 7, 49):
        _, index = case.check(128, sep)
        inside = sorted(int(n) for n in index if 100 <= n < 150)
        # every start row of the file ties: within sep the lower row is better, and a row dropped still drops its neighbours
        assert inside == (list(range(100, 147)) if sep == 0 else [100]), (sep, inside)


def test_no_file_as_long_as_the_clip_and_everything_excluded():
    L, D = 5, 19
    rng = np.random.default_rng(32)
    seg = _segments([int(v) for v in rng.choice([1, 2, 3, 4], size=80)])
    codes, scale = R8.quantize_ref(_values(seg[-1], D, 32), normalize=True)
    qcodes, qscale = R8.quantize_ref(_values(L, D, 33), normalize=True)
    short = Case(codes, scale, seg, qcodes, qscale)
    for sep in (0, 3):
        score, index = short.check(7, sep)
        assert bool((index == -1).all()) and bool(np.isneginf(score).all())
    one_file = Case(codes, scale, [0, seg[-1]], qcodes, qscale)
    score, index = one_file.check(128, 10)
    found = int((index >= 0).sum())
    assert 1 <= found < 128 and bool((index[found:] == -1).all()) and bool(np.isneginf(score[found:]).all())
    score, index = one_file.check(5, 2, skip=(-1, BIG))
    assert bool((index == -1).all()) and bool(np.isneginf(score).all())


def test_zero_rows_score_zero_and_nothing_is_nan():
    N, D, L = 70, 19, 3
    x, xq = _values(N, D, seed=9), _values(L, D, seed=10)
    x[3] = 0.0
    x[20:26] = 0.0
    x[N - 1] = 0.0
    xq[1] = 0.0
    codes, scale = (t.cpu().numpy() for t in ops.rows_quantize_q8(_guarded_f32(x)))
    qcodes, qscale = (t.cpu().numpy() for t in ops.rows_quantize_q8(_guarded_f32(xq)))
    assert scale[3] == 0 and scale[N - 1] == 0 and qscale[1] == 0 and not codes[3].any() and not qcodes[1].any()
    case = Case(codes[:, :D], scale, [0, 30, N], qcodes[:, :D], qscale)
    score, index = case.check(N, 0)
    assert not bool(np.isnan(score).any())
    at = {int(n): float(s) for s, n in zip(score, index) if n >= 0}
    assert all(at[n] == 0.0 for n in (20, 21, 22, 23)) and min(at.values()) == 0.0
    zero = Case(codes[:, :D], scale, [0, 30, N], np.zeros((L, D), dtype=np.int8), np.zeros(L, dtype=np.float32))
    score, index = zero.check(10, 2)
    assert bool((_bits(score[index >= 0]) == 0).all()) and index.tolist() == [0, 30] + [-1] * 8      # all tie: the first row of a file


@pytest.mark.parametrize("shape", [(200, 130, 10), (MANY, 20, 128)], ids=lambda s: "x".join(map(str, s)))
def test_one_row_no_separation_one_file_is_plain_search(shape):
    N, D, k = shape
    codes, scale = R8.quantize_ref(_values(N, D, N), normalize=True)
    qcodes, qscale = R8.quantize_ref(_values(1, D, N + 1), normalize=True)
    case = Case(codes, scale, [0, N], qcodes, qscale)
    score, index = case.check(k, 0)
    s, i = ops.embed_search_q8(case.b, case.sn, D, case.q, case.sq, k)
    assert np.array_equal(index, i[0].cpu().numpy()) and np.array_equal(_bits(score), _bits(s[0].cpu().numpy()))


def test_offsets_beyond_2_to_the_31_bytes():
    """The zero bank of tests/test_gpu_search_q8_kernels.py: (2^20 + 8) rows of 2048 bytes, so row 2^20 starts at byte 2^31.
    A 3-row clip is planted across that byte, once more past it across a file boundary (no place) and once the wrong way
    round; every other row scores exactly 0.0 and ties resolve by row, so the emulation needs the planted columns alone."""
    N, D, L, k, sep = 2 ** 20 + 8, 2048, 3, 8, 3
    assert N * D > 2 ** 31 and (2 ** 20 - 1) * D < 2 ** 31 == 2 ** 20 * D
    qcodes, qscale = R8.quantize_ref(_values(L, D, seed=61), normalize=True)
    seg = [0, 1000, 2 ** 20 + 4, N]
    planted = {2 ** 20 - 1: 0, 2 ** 20: 1, 2 ** 20 + 1: 2,             # the clip, in order, across byte 2^31
               2 ** 20 + 2: 0, 2 ** 20 + 3: 1, 2 ** 20 + 4: 2,         # across the file boundary: no place
               2 ** 20 + 7: 0, 2 ** 20 + 6: 1, 2 ** 20 + 5: 2}         # the wrong way round
    rows = sorted(planted)
    scale_rows = (np.array([2.0, 1.5, 1.75, 0.5, 1.0, 0.25, 0.75, 1.0, 0.5], dtype=np.float32) / 127).astype(np.float32)
    bank = torch.zeros((N, D), device=DEV, dtype=torch.int8)
    scale = torch.full((N,), 1.0 / 127, device=DEV, dtype=torch.float32)
    try:
        for row, s in zip(rows, scale_rows):
            bank[row] = torch.from_numpy(qcodes[planted[row]]).to(DEV)
            scale[row] = float(s)
        score, index = (t.cpu().numpy() for t in ops.embed_match_q8(bank, scale, D, torch.tensor(seg, dtype=torch.int32, device=DEV),
                                                                   torch.from_numpy(qcodes).to(DEV), torch.from_numpy(qscale).to(DEV),
                                                                   k, sep))
    finally:
        del bank
        torch.cuda.empty_cache()
    S = np.zeros((L, N), dtype=np.float32)
    S[:, rows] = R8.scores_q8_ref(np.stack([qcodes[planted[r]] for r in rows]), scale_rows, qcodes, qscale)
    want_s, want_i = M.match_ref(S, seg, k, sep)
    assert want_i[0] == 2 ** 20 - 1 and int((want_i >= 2 ** 20).sum()) >= 1 and want_s.dtype == np.float32
    assert index.tolist() == want_i.tolist(), (index, want_i)
    assert np.array_equal(_bits(score), _bits(want_s)), (score, want_s)


def test_every_limit_is_refused_with_nothing_written():
    N, D, L, k = 40, 20, 3, 5
    codes, scale = R8.quantize_ref(_values(N, D, 51), normalize=True)
    qcodes, qscale = R8.quantize_ref(_values(L, D, 52), normalize=True)
    case = Case(codes, scale, [0, 10, N], qcodes, qscale)
    need = _lib.lib().eat_embed_match_q8_ws_bytes(N, L, k)
    ok = dict(N=N, D=D, F=2, L=L, k=k, sep=4, min_score=0.0, ws=need, ld=32, qld=32, off=0)
    for change in (dict(L=0), dict(L=1025), dict(k=0), dict(k=129), dict(sep=-1), dict(sep=4097), dict(N=0), dict(N=2 ** 31),
                   dict(F=0), dict(D=0), dict(D=131073), dict(D=33), dict(min_score=float("nan")), dict(ws=need - 1), dict(ld=16),
                   dict(qld=16), dict(ld=40), dict(qld=24), dict(off=4)):
        a = dict(ok, **change)
        score = torch.full((128,), float("nan"), device=DEV, dtype=torch.float32)
        index = torch.full((128,), SENTINEL, device=DEV, dtype=torch.int32)
        ws = torch.full((need,), 0xA5, device=DEV, dtype=torch.uint8)
        with pytest.raises(_lib.EatHipError, match=r"eat_embed_match_q8 failed \(-\d+\)"):
            _lib.call("eat_embed_match_q8", case.b.data_ptr() + a["off"], a["ld"], case.sn.data_ptr(), a["N"], a["D"], case.seg_d.data_ptr(),
                      a["F"], case.q.data_ptr(), a["qld"], case.sq.data_ptr(), a["L"], a["k"], a["sep"], a["min_score"], 0, 0,
                      ws.data_ptr(), a["ws"], score.data_ptr(), index.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool(torch.isnan(score).all()) and bool((index == SENTINEL).all()) and bool((ws == 0xA5).all()), change
    with pytest.raises(_lib.EatHipError, match="need 1 <= k <= 128, 1 <= L <= 1024, 0 <= sep <= 4096"):
        ops.embed_match_q8(case.b, case.sn, D, case.seg_d, case.q, case.sq, k, 4097)
    with pytest.raises(_lib.EatHipError, match="min_score is NaN"):
        ops.embed_match_q8(case.b, case.sn, D, case.seg_d, case.q, case.sq, k, 4, float("nan"))
    with pytest.raises(_lib.EatHipError, match="seg must be a contiguous int32 vector"):
        ops.embed_match_q8(case.b, case.sn, D, case.seg_d.long(), case.q, case.sq, k, 4)
    with pytest.raises(_lib.EatHipError, match="at least D = 33"):
        ops.embed_match_q8(case.b, case.sn, 33, case.seg_d, case.q, case.sq, k, 4)
    with pytest.raises(_lib.EatHipError, match=r"query scale must be \(3,\)"):
        ops.embed_match_q8(case.b, case.sn, D, case.seg_d, case.q, case.sq[:2], k, 4)
    case.check(k, 4)                                                   # and the call is fine when nothing is wrong
