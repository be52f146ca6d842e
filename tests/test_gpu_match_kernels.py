"""eat_embed_match (csrc/match.hip, include/eat_match.h) alone, through the raw C ABI and through `ops.embed_match`, with
the harness of tests/test_gpu_search_kernels.py: bank and queries are views into NaN-filled buffers that start on an odd
4-byte word (or, aligned, on a 16-byte boundary), `score`, `index` and the workspace lie inside guard bands that must be
intact afterwards, every element of both outputs must have been written, and a second call must give the same bits.

Where the expected bits come from.  The score s[j, n] of query row j and bank row n is that of eat_embed_search, whose
bits depend on the two rows' contents and on D alone.  So eat_embed_search on slices of at most 128 bank rows with k = the
slice's length returns every s[j, n] exactly; scattered into S (L, N), tests/match_ref.py in float32 - sequential
additions in ascending j, one IEEE division - predicts the score bits and the indices of eat_embed_match.  These tests
demand EQUALITY, not a tolerance, so near-ties cannot make them flaky.  S is computed once per bank and shared.

The fp64 test has a bar instead: |m - m64| <= 2e-5 at the returned rows, the project's per-op bar (a fully serial fp32
emulation lies 2.4e-7 from fp64 at D = 2184, L = 64 and 3.4e-7 at D = 130, L = 200)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, ops  # noqa: E402
from tests import match_ref as M  # noqa: E402
from tests import search_ref as R  # noqa: E402
from tests.test_gpu_search_kernels import GUARD, SENTINEL, _guarded, _unit, _values  # noqa: E402

DEV = torch.device("cuda:0")
BAR = 2e-5
BIG = 2 ** 31 - 1
MANY = 2 * ops.SEARCH_BLOCKS * ops.search_tile_rows(1) + 5            # block 0 of the fixed grid takes three tiles


class Case:
    """A bank, its files and a query clip on the device, and the exact row scores S (L, N) of eat_embed_search."""

    def __init__(self, bank, seg, queries, word=1):
        self.N, self.D = bank.shape
        self.L = queries.shape[0]
        self.seg = [int(v) for v in seg]
        assert self.seg[0] == 0 and self.seg[-1] == self.N
        self.b, self.q = _guarded(bank, word), _guarded(queries, word)
        self.seg_d = torch.tensor(self.seg, dtype=torch.int32, device=DEV)
        S = torch.full((self.L, self.N), float("nan"), device=DEV)
        for lo in range(0, self.N, 128):
            hi = min(lo + 128, self.N)
            s, i = ops.embed_search(self.b[lo:hi], self.q, hi - lo)
            S[:, lo:hi].scatter_(1, i.long(), s)
        self.S = S.cpu().numpy()
        assert not bool(np.isnan(self.S).any())

    def other(self, word):
        """The same rows at another alignment; S is shared: its bits do not depend on where the rows lie."""
        twin = object.__new__(Case)
        twin.__dict__.update(self.__dict__)
        twin.b, twin.q = _guarded(self.b.cpu().numpy(), word), _guarded(self.q.cpu().numpy(), word)
        return twin

    def match(self, k, sep, min_score=-np.inf, skip=None, wrapper=True):
        """-> (score, index) numpy, straight through the C ABI; checks the guard bands, that every output was written, that
        a second call gives the same bits and that ops.embed_match gives them too."""
        need = _lib.lib().eat_embed_match_ws_bytes(self.N, self.L, k)
        assert need > 0
        lo, hi = (0, 0) if skip is None else skip
        outs = []
        for _ in range(2):
            sbuf = torch.full((GUARD + k + GUARD,), float("nan"), device=DEV, dtype=torch.float32)
            ibuf = torch.full((GUARD + k + GUARD,), SENTINEL, device=DEV, dtype=torch.int32)
            ws = torch.full((need + 64,), 0xA5, device=DEV, dtype=torch.uint8)
            score, index = sbuf[GUARD:GUARD + k], ibuf[GUARD:GUARD + k]
            _lib.call("eat_embed_match", self.b.data_ptr(), self.N, self.D, self.seg_d.data_ptr(), len(self.seg) - 1, self.q.data_ptr(),
                      self.L, k, sep, float(min_score), lo, hi, ws.data_ptr(), need, score.data_ptr(), index.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert bool(torch.isnan(sbuf[:GUARD]).all()) and bool(torch.isnan(sbuf[GUARD + k:]).all()), "a guard of score was written"
            assert bool((ibuf[:GUARD] == SENTINEL).all()) and bool((ibuf[GUARD + k:] == SENTINEL).all()), "a guard of index was written"
            assert bool((ws[need:] == 0xA5).all()), "the workspace was overrun"
            assert not bool(torch.isnan(score).any()), "an element of score was not written, or a sum read outside its row"
            assert not bool((index == SENTINEL).any()), "an element of index was not written"
            outs.append((score.clone(), index.clone()))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "two calls, two results"
        if wrapper:
            s2, i2 = ops.embed_match(self.b, self.seg_d, self.q, k, sep, min_score, skip)
            assert s2.shape == (k,) and s2.dtype == torch.float32 and i2.dtype == torch.int32
            assert torch.equal(s2, outs[0][0]) and torch.equal(i2, outs[0][1]), "ops.embed_match and the C ABI differ"
        return outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy()

    def check(self, k, sep, min_score=-np.inf, skip=None, wrapper=True):
        """The kernel's result must be match_ref's on S in float32, bit for bit."""
        score, index = self.match(k, sep, min_score, skip, wrapper)
        want_s, want_i = M.match_ref(self.S, self.seg, k, sep, min_score, skip)
        assert want_s.dtype == np.float32
        tag = (self.N, self.D, self.L, k, sep, min_score, skip)
        assert np.array_equal(index, want_i.astype(np.int32)), (tag, index, want_i)
        assert np.array_equal(score.view(np.int32), want_s.view(np.int32)), (tag, score, want_s)
        return score, index


def _segments(lengths):
    return [0] + np.cumsum(lengths).tolist()


def _random_case(N_about, D, L, choices, seed, word=1):
    rng = np.random.default_rng(seed)
    lengths = []
    while sum(lengths) < N_about:
        lengths.append(int(rng.choice(choices)))
    seg = _segments(lengths)
    return Case(_unit(_values(seg[-1], D, seed)), seg, _unit(_values(L, D, seed + 1)), word)


@pytest.mark.parametrize("shape", [(200, 130, 10), (MANY, 20, 128)], ids=lambda s: "x".join(map(str, s)))
def test_one_row_no_separation_one_file_is_plain_search(shape):
    N, D, k = shape
    case = Case(_unit(_values(N, D, seed=N)), [0, N], _unit(_values(1, D, seed=N + 1)))
    score, index = case.check(k, 0)
    s, i = ops.embed_search(case.b, case.q, k)
    assert np.array_equal(index, i[0].cpu().numpy()) and np.array_equal(score.view(np.int32), s[0].cpu().numpy().view(np.int32))


@pytest.mark.parametrize("D", [130, 132], ids=["D130_4byte_path", "D132_aligned_path"])
@pytest.mark.parametrize("L", [1, 2, 15, 16, 17, 33])
def test_group_and_tile_edges(L, D):
    """File lengths around L and around the tile of 64 rows: windows cross multiples of 64, file ends fall inside tiles,
    files shorter than L have no start row; L = 17 and 33 take more than one group of query rows."""
    choices = [v for v in {1, L - 1, L, L + 1, 63, 64, 65, 130} if v >= 1]
    case = _random_case(700, D, L, sorted(choices), seed=10 * L + D, word=0 if D == 132 else 1)
    N, seg = case.N, case.seg
    f = max(range(len(seg) - 1), key=lambda j: (seg[j + 1] - seg[j] >= 64, -abs(seg[j] - N // 2)))      # a long file near the middle
    skips = [None, (seg[f], seg[f + 1]), (-5, 70), (N - 90, BIG)]
    first = True
    for sep in (0, 1, 5, L, 4096):
        for k in (1, 10, 128):
            for skip in skips:
                case.check(k, sep, skip=skip, wrapper=first or k == 10)
                first = False
    # the bits do not depend on the alignment, nor on the load width it selects
    free = case.check(10, L)
    twin = case.other(1 if D == 132 else 0).check(10, L)
    assert np.array_equal(free[0].view(np.int32), twin[0].view(np.int32)) and np.array_equal(free[1], twin[1])
    # a threshold between two returned scores cuts the list there
    cut = next(a for a in range(9) if free[0][a] > free[0][a + 1])
    min_score = np.float32(0.5) * (free[0][cut] + free[0][cut + 1])
    if not free[0][cut] > min_score > free[0][cut + 1]:                 # neighbours in fp32: the upper one itself
        min_score = free[0][cut]
    score, index = case.check(10, L, min_score=float(min_score))
    assert index[:cut + 1].tolist() == free[1][:cut + 1].tolist() and bool((index[cut + 1:] == -1).all())
    assert bool(np.isneginf(score[cut + 1:]).all())


_MANY = {}


@pytest.mark.parametrize("sep", [3, 100])
def test_many_blocks(sep):
    """More tiles than blocks, for the scan and for the peak kernel; neighbours within sep live in other tiles and blocks."""
    if "case" not in _MANY:
        rng = np.random.default_rng(17)
        lengths = []
        while sum(lengths) < MANY:
            lengths.append(int(rng.integers(1, 201)))
        lengths[-1] -= sum(lengths) - MANY
        seg = _segments(lengths)
        _MANY["case"] = Case(_unit(_values(MANY, 20, seed=17)), seg, _unit(_values(17, 20, seed=18)))
    case = _MANY["case"]
    assert case.N == MANY
    _, index = case.check(128, sep)
    assert int(index.min()) >= 0
    case.check(10, sep, skip=(MANY // 2, MANY // 2 + 5000))


def test_a_file_stored_twice_ties_exactly():
    """One file's rows at rows 60 .. 99 and again at 500 .. 539 (another position within the tile, other blocks): the means
    of corresponding start rows are bit-equal, so both are returned next to each other, the lower row first."""
    D, L = 36, 5
    x = _values(700, D, seed=21)
    x[60:100] = x[60] + 0.1 * x[60:100]                         # rows of one sound: every start row of the file outscores the rest
    x[500:540] = x[60:100]
    seg = [0, 60, 100, 333, 500, 540, 700]
    bank = _unit(x)
    case = Case(bank, seg, bank[70:75].copy())                  # the clip is rows 70 .. 74 of the file
    score, index = case.check(10, 4)
    assert index[:2].tolist() == [70, 510] and score[0] == score[1] and abs(float(score[0]) - 1.0) <= BAR
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
    case = Case(_unit(x), [0, 100, 150, 300], _unit(queries))
    for sep in (0, 7, 49):
        _, index = case.check(128, sep)
        inside = sorted(int(n) for n in index if 100 <= n < 150)
        # every start row of the file ties: within sep the lower row is better, and a row dropped still drops its neighbours
        assert inside == (list(range(100, 147)) if sep == 0 else [100]), (sep, inside)


def test_fewer_peaks_than_k_and_no_candidate_at_all():
    case = _random_case(50, 19, 3, [4, 9], seed=31)
    score, index = case.check(128, 10)
    found = int((index >= 0).sum())
    assert 1 <= found < 128 and bool((index[found:] == -1).all()) and bool(np.isneginf(score[found:]).all())
    short = _random_case(200, 19, 5, [1, 2, 3, 4], seed=32)             # every file is shorter than L
    for sep in (0, 3):
        score, index = short.check(7, sep)
        assert bool((index == -1).all()) and bool(np.isneginf(score).all())
    # everything excluded
    score, index = case.check(5, 2, skip=(-1, BIG))
    assert bool((index == -1).all()) and bool(np.isneginf(score).all())


def test_one_row():
    D = 7
    bank = _unit(_values(1, D, seed=41))
    one = Case(bank, [0, 1], _unit(_values(1, D, seed=42)))
    score, index = one.check(3, 5)
    assert index.tolist() == [0, -1, -1] and score[0] == one.S[0, 0]
    two = Case(bank, [0, 1], _unit(_values(2, D, seed=43)))
    assert two.check(3, 0)[1].tolist() == [-1, -1, -1]


@pytest.mark.parametrize("shape", [(400, 2184, 64), (400, 130, 200)], ids=lambda s: "x".join(map(str, s)))
def test_against_fp64(shape):
    N, D, L = shape
    bank, queries = _unit(_values(N, D, seed=D)), _unit(_values(L, D, seed=D + 1))
    seg = [0, N // 4, N]
    case = Case(bank, seg, queries)
    k = 10
    score, index = case.check(k, L)
    m64 = M.window_means(R.scores_ref(bank, queries, normalize=False))
    found = index[index >= 0]
    assert len(found) >= 1
    err = np.abs(score[:len(found)].astype(np.float64) - m64[found])
    print(f"MATCH {shape}: max |m - m64| = {float(err.max()):.3e} over {len(found)} places (bar {BAR:.0e})")
    assert bool((err <= BAR).all())


def test_offsets_beyond_2_to_the_31_elements():
    """A zero bank of (2^20 + 8) x 2048 floats, 8.6 GB: rows from 2^20 on start past element 2^31.  The clip's two rows are
    planted there, in order, across a file boundary and the wrong way round; every other row scores exactly 0.0 and ties
    resolve by row, so the fp64 reference needs the planted columns of S alone."""
    N, D, L, k, sep = 2 ** 20 + 8, 2048, 2, 8, 3
    queries = _unit(_values(L, D, seed=61))
    seg = [0, 1000, 2 ** 20 + 4, N]
    planted = {2 ** 20 + 1: queries[0], 2 ** 20 + 2: queries[1],       # the clip, in order
               2 ** 20 + 3: queries[0], 2 ** 20 + 4: queries[1],       # across the file boundary: no place
               2 ** 20 + 7: queries[0], 2 ** 20 + 6: queries[1]}       # the wrong way round
    bank = torch.zeros((N, D), device=DEV, dtype=torch.float32)
    try:
        for row, vec in planted.items():
            bank[row] = torch.from_numpy(vec).to(DEV)
        score, index = (t.cpu().numpy() for t in ops.embed_match(bank, torch.tensor(seg, dtype=torch.int32, device=DEV),
                                                                 torch.from_numpy(queries).to(DEV), k, sep))
    finally:
        del bank
        torch.cuda.empty_cache()
    S = np.zeros((L, N))
    rows = sorted(planted)
    S[:, rows] = R.scores_ref(np.stack([planted[r] for r in rows]), queries, normalize=False)
    want_s, want_i = M.match_ref(S, seg, k, sep)
    assert want_i[0] == 2 ** 20 + 1 and abs(want_s[0] - 1.0) <= BAR and int((want_i >= 2 ** 20).sum()) >= 2
    assert index.tolist() == want_i.tolist(), (index, want_i)
    found = want_i >= 0
    assert bool((np.abs(score[found] - want_s[found]) <= BAR).all()) and bool(np.isneginf(score[~found]).all())
    assert bool((score[want_s == 0.0] == 0.0).all())


def test_every_limit_is_refused_with_nothing_written():
    N, D, L, k = 40, 8, 3, 5
    case = Case(_unit(_values(N, D, seed=51)), [0, 10, 40], _unit(_values(L, D, seed=52)))
    need = _lib.lib().eat_embed_match_ws_bytes(N, L, k)
    ok = dict(N=N, D=D, F=2, L=L, k=k, sep=4, min_score=0.0, ws=need)
    for change in (dict(L=0), dict(L=1025), dict(k=0), dict(k=129), dict(sep=-1), dict(sep=4097), dict(N=0), dict(N=2 ** 31),
                   dict(F=0), dict(D=0), dict(min_score=float("nan")), dict(ws=need - 1)):
        a = dict(ok, **change)
        score = torch.full((128,), float("nan"), device=DEV, dtype=torch.float32)
        index = torch.full((128,), SENTINEL, device=DEV, dtype=torch.int32)
        ws = torch.full((need,), 0xA5, device=DEV, dtype=torch.uint8)
        with pytest.raises(_lib.EatHipError, match=r"eat_embed_match failed \(-\d+\)"):
            _lib.call("eat_embed_match", case.b.data_ptr(), a["N"], a["D"], case.seg_d.data_ptr(), a["F"], case.q.data_ptr(), a["L"],
                      a["k"], a["sep"], a["min_score"], 0, 0, ws.data_ptr(), a["ws"], score.data_ptr(), index.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool(torch.isnan(score).all()) and bool((index == SENTINEL).all()) and bool((ws == 0xA5).all()), change
    with pytest.raises(_lib.EatHipError, match="need 1 <= k <= 128, 1 <= L <= 1024, 0 <= sep <= 4096"):
        ops.embed_match(case.b, case.seg_d, case.q, k, 4097)
    with pytest.raises(_lib.EatHipError, match="min_score is NaN"):
        ops.embed_match(case.b, case.seg_d, case.q, k, 4, float("nan"))
    with pytest.raises(_lib.EatHipError, match="seg must be a contiguous int32 vector"):
        ops.embed_match(case.b, case.seg_d.long(), case.q, k, 4)
    with pytest.raises(_lib.EatHipError, match="must share D"):
        ops.embed_match(case.b, case.seg_d, case.q[:, :-1].contiguous(), k, 4)
    case.check(k, 4)                                                   # and the call is fine when nothing is wrong
