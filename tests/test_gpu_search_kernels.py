"""eat_rows_normalize and eat_embed_search (csrc/search.hip, include/eat_search.h) alone against the fp64 reference of
tests/search_ref.py, through the raw C ABI and through the `ops` wrappers.

Bank and queries are views into larger NaN-filled buffers, by default starting on an odd 4-byte word, with NaN directly
behind their last element: a read outside them turns a score into NaN.  `score`, `index` and the workspace lie inside guard
bands that must be intact afterwards, while every element of `score` and `index` must have been written; a second call must
give the same bits.  Values are clip(0.75 + N(0, 1), 0): cosines sit near 0.5 with no cancellation.

Score bar: |score - fp64 score of the returned row| <= 2e-5, the project's per-op bar.  A fully serial fp32 accumulation
of such data at D = 2184 lies 1.5e-6 from fp64, so any sane order passes; at the small D used here a dropped element moves a
score by far more.  The ranking check (search_ref.check_ranking) needs no index equality: near-ties cannot make it flaky.

The entry point takes rows that are normalised already; the tests normalise in fp64 on the host, round to fp32 and take
the fp64 dot products of those fp32 rows as the reference, except where they say that `ops.rows_normalize` does it.

Shapes beyond the issue's list, one per path of the kernel: the same cases on a 16-byte aligned bank (16-byte loads where
D % 4 == 0) - whose bits must equal the unaligned run's, the scores being functions of the rows' contents alone - and a D so
large that not even one query fits the LDS (the queries are then read from global memory)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, ops  # noqa: E402
from tests import search_ref as R  # noqa: E402

DEV = torch.device("cuda:0")
BAR = 2e-5
GUARD = 67            # odd: the view behind it starts on an odd word
SENTINEL = -7         # no index is ever -7
_SEEN = {}            # (case) -> (score, index) of the unaligned run, for the aligned one to equal


def _group(Q):
    """Queries resident in the first pass: the smallest power of two that holds min(Q, 16) (search.hip: eat_embed_search)."""
    g = 1
    while g < min(Q, ops.SEARCH_GROUP):
        g *= 2
    return g


def _tile(Q):
    return ops.search_tile_rows(_group(Q))


# a bank on which block 0 of the fixed grid takes three tiles and every other block two, from the kernel's grid constants
def _three_tiles(Q):
    return 2 * ops.SEARCH_BLOCKS * _tile(Q) + 5


def _values(n, D, seed):
    return np.clip(0.75 + np.random.default_rng(seed).standard_normal((n, D)), 0, None)


def _unit(x):
    """fp64 normalisation on the host, rounded to fp32: what the C entry point is handed."""
    return R.normalize_ref(x).astype(np.float32)


def _guarded(x, word=1):
    """x (numpy fp32) as a device view that starts `word` 4-byte words into a NaN buffer, NaN right behind it."""
    buf = torch.full((word + x.size + GUARD,), float("nan"), device=DEV, dtype=torch.float32)
    view = buf[word:word + x.size].view(x.shape)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == (4 * word) % 16 and bool(torch.isnan(buf[word + x.size:]).all())
    return view


def _search(bank, queries, k, skip=None, word=1):
    """bank, queries: normalised numpy fp32 -> (score, index) numpy, straight through the C ABI with `skip` as it is.
    Checks the guard bands, that every output was written, that a second call gives the same bits and that
    ops.embed_search gives them too."""
    b, q = _guarded(bank, word), _guarded(queries, word)
    (N, D), Q = bank.shape, queries.shape[0]
    need = _lib.lib().eat_embed_search_ws_bytes(Q, k)
    assert need > 0
    skip_d = None if skip is None else torch.tensor(skip, dtype=torch.int32).reshape(Q, 2).to(DEV)
    outs = []
    for _ in range(2):
        sbuf = torch.full((GUARD + Q * k + GUARD,), float("nan"), device=DEV, dtype=torch.float32)
        ibuf = torch.full((GUARD + Q * k + GUARD,), SENTINEL, device=DEV, dtype=torch.int32)
        ws = torch.full((need + 64,), 0xA5, device=DEV, dtype=torch.uint8)
        score, index = sbuf[GUARD:GUARD + Q * k].view(Q, k), ibuf[GUARD:GUARD + Q * k].view(Q, k)
        _lib.call("eat_embed_search", b.data_ptr(), N, D, q.data_ptr(), Q, k, None if skip_d is None else skip_d.data_ptr(),
                  ws.data_ptr(), need, score.data_ptr(), index.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert bool(torch.isnan(sbuf[:GUARD]).all()) and bool(torch.isnan(sbuf[GUARD + Q * k:]).all()), "a guard of score was written"
        assert bool((ibuf[:GUARD] == SENTINEL).all()) and bool((ibuf[GUARD + Q * k:] == SENTINEL).all()), "a guard of index was written"
        assert bool((ws[need:] == 0xA5).all()), "the workspace was overrun"
        assert not bool(torch.isnan(score).any()), "an element of score was not written, or a sum read outside its row"
        assert not bool((index == SENTINEL).any()), "an element of index was not written"
        outs.append((score.clone(), index.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "two calls, two results"
    if skip is None or all(-2 ** 31 <= int(v) < 2 ** 31 for v in np.asarray(skip).reshape(-1)):
        s2, i2 = ops.embed_search(b, q, k, skip)
        assert s2.shape == (Q, k) and s2.dtype == torch.float32 and i2.dtype == torch.int32
        assert torch.equal(s2, outs[0][0]) and torch.equal(i2, outs[0][1]), "ops.embed_search and the C ABI differ"
    return outs[0][0].cpu().numpy(), outs[0][1].cpu().numpy()


def _check(tag, bank, queries, k, skip=None, word=1):
    score, index = _search(bank, queries, k, skip, word)
    ref = R.scores_ref(bank, queries, normalize=False)
    R.check_ranking(score, index, ref, k, skip, bar=BAR, slack=2 * BAR, tag=tag)
    return score, index, ref


SHAPES = [(1, 1, 1, 1), (5, 7, 3, 5),
          (3, 7, 2, 5),                                   # k > N: padding
          (257, 33, 9, 16), (1000, 130, 17, 64),          # Q = 17: one full group of 16 and a group of one
          (4099, 2184, 2, 128),
          (300, 36, 17, 8),                               # one group + 1 again, D % 4 == 0
          (_three_tiles(1), 4, 1, 8), (_three_tiles(16), 4, 16, 8),      # more than one tile per block, alone and in a full group
          (6, 41004, 2, 3)]                               # 4 x 41216 bytes of one padded query exceed the 160 KB of LDS


@pytest.mark.parametrize("word", [1, 0], ids=["odd_word", "aligned"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_search_against_fp64(shape, word):
    N, D, Q, k = shape
    bank, queries = _unit(_values(N, D, seed=N + D)), _unit(_values(Q, D, seed=N + D + 1))
    score, index, _ = _check(f"{shape} word={word}", bank, queries, k, word=word)
    if shape == (3, 7, 2, 5):
        assert bool((index[:, 3:] == -1).all()) and bool((index[:, :3] >= 0).all())
    # the bits of a score depend on the rows' contents alone: not on the alignment, nor on the load width it selects
    other = _SEEN.setdefault(shape, (score, index))
    assert np.array_equal(other[0], score) and np.array_equal(other[1], index)


def test_identical_rows_tie_exactly_in_ascending_index():
    """Copies of one row at the first row, at the last row of a tile and at the last row of the bank: whatever block and
    slot meets them, their scores are bit-equal for every query, so they stand next to each other in ascending index."""
    Q, D = 9, 36
    tile = _tile(Q)
    N = tile + 37                                          # two tiles, two blocks; k = N gives the whole order
    assert tile - 1 < N - 1 and N <= ops.SEARCH_MAX_K
    x = _values(N, D, seed=1)
    twins = [0, tile - 1, N - 1]
    queries = _values(Q, D, seed=2)
    x[twins] = queries[0]                                  # the best rows of query 0; anywhere in the order of the others
    for word in (1, 0):
        score, index, _ = _check(f"twins word={word}", _unit(x), _unit(queries), N, word=word)
        for q in range(Q):
            at = [int(np.flatnonzero(index[q] == t)[0]) for t in twins]
            assert at == [at[0], at[0] + 1, at[0] + 2], (q, at)
            assert score[q, at[0]] == score[q, at[1]] == score[q, at[2]]
        assert index[0, :3].tolist() == twins and abs(float(score[0, 0]) - 1.0) <= BAR


@pytest.mark.parametrize("shape", [(700, 33, 2, 128), (_three_tiles(2), 4, 2, 128)], ids=lambda s: "x".join(map(str, s)))
def test_a_bank_of_one_repeated_row_returns_the_first_k_rows(shape):
    N, D, Q, k = shape
    bank = np.repeat(_unit(_values(1, D, seed=3)), N, axis=0)
    score, index, _ = _check(f"repeated {shape}", bank, _unit(_values(Q, D, seed=4)), k)
    assert np.array_equal(index, np.tile(np.arange(k, dtype=np.int32), (Q, 1)))
    assert bool((score == score[:, :1]).all())


def test_planted_neighbours_take_the_top_ranks():
    """Copies of each query scaled by positive constants - at row 0, at row N - 1, on both sides of a tile edge - through
    ops.rows_normalize: they are the query's direction again, score 1."""
    Q, D, k = 3, 40, 5
    tile = _tile(Q)
    N = 3 * tile + 7
    x, queries = _values(N, D, seed=5), _values(Q, D, seed=6)
    planted = [[0, tile - 1, N - 1], [1, tile, N - 2], [2, 2 * tile - 1, 2 * tile]]
    for q, rows in enumerate(planted):
        for row, scale in zip(rows, (0.5, 2.0, 3.7)):
            x[row] = scale * queries[q]
    bank = ops.rows_normalize(_guarded(x.astype(np.float32)))
    qn = ops.rows_normalize(_guarded(queries.astype(np.float32)))
    score, index = (t.cpu().numpy() for t in ops.embed_search(bank, qn, k))
    ref = R.scores_ref(x.astype(np.float32), queries.astype(np.float32))
    R.check_ranking(score, index, ref, k, bar=BAR, slack=2 * BAR, tag="planted")
    for q, rows in enumerate(planted):
        assert sorted(index[q, :3].tolist()) == rows, (q, index[q])
        assert bool((np.abs(score[q, :3].astype(np.float64) - 1.0) <= BAR).all()) and float(score[q, 3]) < 0.99


def test_exclusion_ranges():
    Q, D, k = 7, 33, 12
    tile = _tile(Q)
    N = 3 * tile + 7
    x, queries = _values(N, D, seed=7), _values(Q, D, seed=8)
    x[40:45] = queries[3]                                  # the true top rows of query 3 ...
    big = 2 ** 31 - 1
    skip = [[0, 0],                                        # empty
            [50, 20],                                      # lo > hi: nothing
            [0, N],                                        # the whole bank: all -1
            [40, 45],                                      # ... hidden
            [tile - 3, tile + 4],                          # straddles a tile edge
            [-5, 10],                                      # clamped below
            [N - 4, big]]                                  # clamped above
    bank, qn = _unit(x), _unit(queries)
    for word in (1, 0):
        free, free_i, _ = _check(f"no exclusion word={word}", bank, qn, k, word=word)
        score, index, _ = _check(f"exclusion word={word}", bank, qn, k, skip, word=word)
        assert np.array_equal(index[:2], free_i[:2]) and np.array_equal(score[:2], free[:2])
        assert bool((index[2] == -1).all()) and bool(np.isneginf(score[2]).all())
        assert sorted(free_i[3, :5].tolist()) == [40, 41, 42, 43, 44] and not set(index[3].tolist()) & {40, 41, 42, 43, 44}
        assert not set(index[4].tolist()) & set(range(tile - 3, tile + 4))
        assert int(index[5].min()) >= 10 and int(index[6].max()) < N - 4
    # beyond int32 nothing is representable: the raw table of the C ABI is int32, and the wrapper says so
    with pytest.raises(_lib.EatHipError, match="must fit int32"):
        ops.embed_search(_guarded(bank), _guarded(qn), k, [[0, 2 ** 31]] * Q)
    # k larger than what is left: all rows but the first five hidden
    score, index, _ = _check("exclusion and padding", bank, qn, 100, [[5, N]] * Q)
    assert bool((index[:, 5:] == -1).all()) and sorted(index[0, :5].tolist()) == [0, 1, 2, 3, 4]


def test_zero_rows_score_zero_and_nothing_is_nan():
    N, D, Q, k = 70, 19, 3, 70
    x, queries = _values(N, D, seed=9), _values(Q, D, seed=10)
    x[3] = 0.0
    x[N - 1] = 0.0
    queries[1] = 0.0
    bank = ops.rows_normalize(_guarded(x.astype(np.float32)))
    qn = ops.rows_normalize(_guarded(queries.astype(np.float32)))
    assert bool((bank[3] == 0).all()) and bool((bank[N - 1] == 0).all()) and bool((qn[1] == 0).all())
    assert not bool(torch.isnan(bank).any()) and not bool(torch.isnan(qn).any())
    score, index = (t.cpu().numpy() for t in ops.embed_search(bank, qn, k))
    R.check_ranking(score, index, R.scores_ref(x.astype(np.float32), queries.astype(np.float32)), k, bar=BAR, slack=2 * BAR, tag="zero rows")
    assert bool((score[1] == 0.0).all()) and index[1].tolist() == list(range(N))          # a zero query: every score 0.0, by row
    for q in (0, 2):                                                                       # zero rows: the last two, by row
        assert index[q, -2:].tolist() == [3, N - 1] and bool((score[q, -2:] == 0.0).all()) and float(score[q, -3]) > 0


@pytest.mark.parametrize("word", [1, 0], ids=["odd_word", "aligned"])
@pytest.mark.parametrize("D", [1, 7, 130, 2184])
def test_rows_normalize(D, word):
    N = 37                                                  # ten blocks of four rows, the last one ragged
    x = (3.0 * np.random.default_rng(D).standard_normal((N, D))).astype(np.float32)
    x[5] = 0.0
    xv = _guarded(x, word)
    front = 64 + word                                       # out starts on a 16-byte boundary exactly when x does
    buf = torch.full((front + N * D + GUARD,), float("nan"), device=DEV, dtype=torch.float32)
    out = buf[front:front + N * D].view(N, D)
    assert out.data_ptr() % 16 == xv.data_ptr() % 16
    assert ops.rows_normalize(xv, out=out) is out
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[:front]).all()) and bool(torch.isnan(buf[front + N * D:]).all()), "a guard of out was written"
    assert not bool(torch.isnan(out).any()), "an element of out was not written"
    got = out.cpu().numpy().astype(np.float64)
    ref = R.normalize_ref(x)
    norms = np.sqrt((got * got).sum(axis=1))
    keep = np.arange(N) != 5
    print(f"NORMALIZE D={D} word={word}: max |norm - 1| = {float(np.abs(norms[keep] - 1).max()):.3e}, "
          f"max |out - ref| = {float(np.abs(got - ref).max()):.3e} (bars 2e-6)")
    assert bool((np.abs(norms[keep] - 1.0) <= 2e-6).all()) and bool((got[5] == 0.0).all())
    # direction: every component within 2e-6 of the fp64 quotient (components are at most 1; fp32 rounds at 6e-8)
    assert bool((np.abs(got - ref) <= 2e-6).all())
    fresh = ops.rows_normalize(xv)
    assert torch.equal(fresh, out)
    assert ops.rows_normalize(xv, out=xv) is xv and torch.equal(xv, out)                   # in place: the same bits


def test_offsets_beyond_2_to_the_31_elements():
    """A zero bank of (2^20 + 8) x 2048 floats, 8.6 GB: rows from 2^20 on start past element 2^31.  Unit rows are planted
    there; every other row scores exactly 0.0 and ties resolve by index, so the reference needs the planted rows alone."""
    N, D, Q, k = 2 ** 20 + 8, 2048, 3, 8
    queries = _unit(_values(Q, D, seed=11))
    planted = {2 ** 20 + 1: queries[0], 2 ** 20 + 4: queries[1], 2 ** 20 + 7: queries[2], 2 ** 20 - 1: queries[2]}
    bank = torch.zeros((N, D), device=DEV, dtype=torch.float32)
    try:
        for row, vec in planted.items():
            bank[row] = torch.from_numpy(vec).to(DEV)
        score, index = (t.cpu().numpy() for t in ops.embed_search(bank, torch.from_numpy(queries).to(DEV), k))
    finally:
        del bank
        torch.cuda.empty_cache()
    rows = np.array(sorted(planted))
    ref = R.scores_ref(np.stack([planted[r] for r in rows]), queries, normalize=False)       # (Q, 4), all > 0
    for q in range(Q):
        order = rows[np.lexsort((rows, -ref[q]))]
        assert index[q].tolist() == order.tolist() + [0, 1, 2, 3], (q, index[q])
        want = np.concatenate((np.sort(ref[q])[::-1], np.zeros(4)))
        assert bool((np.abs(score[q] - want) <= BAR).all()) and bool((score[q, 4:] == 0.0).all())


def test_wrappers_refuse_bad_operands():
    bank, q = torch.zeros((5, 8), device=DEV), torch.zeros((2, 8), device=DEV)
    with pytest.raises(_lib.EatHipError, match="must share D"):
        ops.embed_search(bank, torch.zeros((2, 7), device=DEV), 3)
    with pytest.raises(_lib.EatHipError, match="contiguous float32"):
        ops.embed_search(bank.t().contiguous().t(), q, 3)
    with pytest.raises(_lib.EatHipError, match="must live on the GPU"):
        ops.embed_search(bank, q.cpu(), 3)
    with pytest.raises(_lib.EatHipError, match="need 1 <= k <= 128"):
        ops.embed_search(bank, q, 129)
    with pytest.raises(_lib.EatHipError, match=r"skip must be \(2, 2\)"):
        ops.embed_search(bank, q, 3, [[0, 1]])
    with pytest.raises(_lib.EatHipError, match=r"x must be \(N, D >= 1\)"):
        ops.rows_normalize(torch.zeros(8, device=DEV))
    with pytest.raises(_lib.EatHipError, match="out must be"):
        ops.rows_normalize(bank, out=torch.zeros((5, 7), device=DEV))
    score, index = ops.embed_search(bank, q, 3)
    assert index.tolist() == [[0, 1, 2]] * 2 and bool((score == 0).all())
