"""eat_embed_pool (csrc/embed.hip, include/eat_embed.h) alone against the fp64 `embed_pool_ref`.

Every map is a view into a larger NaN-filled buffer, by default starting on an odd 4-byte word, with NaN directly after its
last element: a read outside the map turns a sum into NaN.  `out` is NaN-filled and lies inside a larger NaN buffer whose
guard elements must still be NaN afterwards, while every element of `out` itself must have been written.  Values are
0.75 + N(0, 1) plus a ramp of 0.05 per column: a wrong divisor shows through the non-zero mean, an off-by-one bound through
the ramp (neighbouring column means differ by 0.05, far above the bar).

Bar: |got - ref| <= 2e-5 mean|x| over the segment, the project's per-op bar.  A 64-lane-serial-then-tree fp32 sum over a
64 x 500 plane lies at 6.4e-8 relative and a fully serial one at 2e-6, so the bar holds for any sane summation order;
an indexing error lies above 1e-3.

Shapes beyond the issue's list, one per path of the kernel: 16-byte and 8-byte aligned maps (vector loads, with fewer and
with more column groups than lanes), T = 1024 (the widest plane whose column sums are kept on chip) and T > 1024
(per-segment sums straight from the map)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, embeddings, ops  # noqa: E402
from tests import embed_ref as R  # noqa: E402

DEV = torch.device("cuda:0")
BAR = 2e-5
GUARD = 67            # odd: the view behind it starts on an odd word

SHAPES = [(1, 1, 1), (3, 1, 5), (5, 4, 32), (7, 8, 63), (2, 16, 125), (2, 32, 251), (2, 64, 500), (130, 2, 3)]


def _values(B, C, F, T, seed):
    rng = np.random.default_rng(seed)
    x = 0.75 + rng.standard_normal((B, C, F, T)) + 0.05 * np.arange(T)
    return x.astype(np.float32)


def _guarded(x, word=1):
    """x (numpy fp32) as a device view that starts `word` 4-byte words into a NaN buffer, NaN right behind it."""
    buf = torch.full((word + x.size + GUARD,), float("nan"), device=DEV, dtype=torch.float32)
    view = buf[word:word + x.size].view(x.shape)
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == (4 * word) % 16 and bool(torch.isnan(buf[word + x.size:]).all())
    return view


def _run(xs, lo, hi, raw=False, word=1):
    """xs: numpy maps -> out (B, n_seg, D) numpy, through ops.embed_pool or (raw) straight through the C ABI with the
    tables as they are.  Checks the guards of `out` and that a second call gives the same bits."""
    maps = [_guarded(x, word) for x in xs]
    B, n_seg, D = xs[0].shape[0], np.asarray(lo).shape[1], sum(x.shape[1] for x in xs)
    outs = []
    for _ in range(2):
        buf = torch.full((GUARD + B * n_seg * D + GUARD,), float("nan"), device=DEV, dtype=torch.float32)
        out = buf[GUARD:GUARD + B * n_seg * D].view(B, n_seg, D)
        if raw:
            offs = np.concatenate(([0], np.cumsum([x.shape[1] for x in xs])[:-1]))
            dims = torch.tensor([[x.shape[1], x.shape[2], x.shape[3], int(o)] for x, o in zip(xs, offs)], dtype=torch.int32).to(DEV)
            seg = torch.from_numpy(np.stack((np.asarray(lo), np.asarray(hi)), axis=2).astype(np.int32)).contiguous().to(DEV)
            addr = torch.tensor([m.data_ptr() for m in maps], dtype=torch.int64).to(DEV)
            _lib.call("eat_embed_pool", addr.data_ptr(), dims.data_ptr(), seg.data_ptr(), len(xs), B, n_seg, D, out.data_ptr(),
                      torch.cuda.current_stream().cuda_stream)
        else:
            assert ops.embed_pool(maps, lo, hi, out=out) is out
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + B * n_seg * D:]).all()), "a guard of out was written"
        assert not bool(torch.isnan(out).any()), "an element of out was not written, or a sum read outside its map"
        outs.append(out.clone())
    assert torch.equal(outs[0], outs[1])
    return outs[0].cpu().numpy()


def _check(tag, got, xs, lo, hi):
    ref = R.embed_pool_ref(xs, lo, hi)
    scale = R.segment_abs_mean_ref(xs, lo, hi)
    err = np.abs(got.astype(np.float64) - ref)
    rel = float((err[scale > 0] / scale[scale > 0]).max()) if bool((scale > 0).any()) else 0.0
    print(f"EMBK {tag}: max |got - ref| / mean|x| = {rel:.3e} over {got.size} values (bar {BAR:.0e})")
    assert got.shape == ref.shape
    assert bool((err <= BAR * scale).all()), rel


def _tables(T, kind):
    """(1, n_seg) segment tables of one map of width T."""
    if kind == "scene":
        segs = [(0, T)]
    elif kind == "edges":          # single columns at 0 and T - 1, the whole plane twice
        segs = [(0, 1), (T - 1, T), (0, T), (0, T)]
    elif kind == "tiling":         # non-overlapping, width 7, the last one ragged
        segs = [(a, min(a + 7, T)) for a in range(0, T, 7)]
    else:                          # every single column
        segs = [(t, t + 1) for t in range(T)]
    return np.array([[s[0] for s in segs]], dtype=np.int32), np.array([[s[1] for s in segs]], dtype=np.int32)


@pytest.mark.parametrize("kind", ["scene", "edges", "tiling", "columns"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_one_map(shape, B, kind):
    C, F, T = shape
    xs = [_values(B, C, F, T, seed=C * 1000 + T)]
    lo, hi = _tables(T, kind)
    _check(f"{shape} B={B} {kind}", _run(xs, lo, hi), xs, lo, hi)


# one shape per load width and per branch of the column sums; word 0 / 2 / 1 = 16- / 8- / 4-byte aligned maps
@pytest.mark.parametrize("word", [0, 2, 1])
@pytest.mark.parametrize("shape", [(2, 64, 500), (2, 32, 250), (1, 3, 1024), (1, 3, 1028), (2, 2, 4100), (3, 5, 36)],
                         ids=lambda s: "x".join(map(str, s)))
def test_alignments_and_wide_maps(shape, word):
    C, F, T = shape
    xs = [_values(2, C, F, T, seed=T + word)]
    for kind in ("scene", "tiling"):
        lo, hi = _tables(T, kind)
        _check(f"{shape} word={word} {kind}", _run(xs, lo, hi, word=word), xs, lo, hi)


@pytest.mark.parametrize("B", [1, 3])
def test_seventeen_maps_of_every_kind(B):
    """All the shapes above and nine more in one call, off_l = 0, 1, 4, 9, 16, 18, 20, 22, 152, ...: not multiples of 4."""
    shapes = SHAPES + [(3, 2, 17), (1, 64, 500), (5, 1, 1), (2, 3, 300), (9, 16, 125), (1, 8, 63), (6, 4, 32), (3, 32, 250), (2, 1, 2)]
    assert len(shapes) == 17
    xs = [_values(B, C, F, T, seed=i) for i, (C, F, T) in enumerate(shapes)]
    offs = np.cumsum([0] + [s[0] for s in shapes])
    assert sum(int(o) % 4 != 0 for o in offs[1:-1]) >= 8
    lo = np.array([[0, 0, T - 1, 0, 0, T // 2] for _, _, T in shapes], dtype=np.int32)
    hi = np.array([[T, 1, T, T, max(1, (T + 1) // 2), T] for _, _, T in shapes], dtype=np.int32)
    _check(f"17 maps B={B}", _run(xs, lo, hi), xs, lo, hi)


def test_the_default_timestamp_plan_of_a_ten_second_window():
    """(hop 50 ms, width 160 ms) on the map widths of a 1000-frame window: 200 overlapping segments per map, single
    nearest columns on the stride-32 maps."""
    T_l = R.mn_widths(1000)
    lo, hi, t = embeddings.segment_plan(1000, T_l, R.MN_STRIDES, 10.0, 50.0, 160.0)
    assert lo.shape == (17, 200) and bool((lo[0, 1:] < hi[0, :-1]).all()) and bool((hi[13:] - lo[13:] == 1).all())
    channels = [1, 3, 2, 1, 5, 2, 3, 7, 1, 2, 3, 1, 2, 9, 2, 3, 6]
    xs = [_values(2, C, 2048 // (4 * r), T, seed=100 + i) for i, (C, T, r) in enumerate(zip(channels, T_l, R.MN_STRIDES))]
    assert xs[0].shape == (2, 1, 256, 500) and xs[-1].shape == (2, 6, 16, 32)
    _check("plan(50, 160)", _run(xs, lo, hi), xs, lo, hi)


@pytest.mark.parametrize("shape", [(7, 8, 63), (2, 64, 500), (2, 2, 4100)], ids=lambda s: "x".join(map(str, s)))
def test_unvalidated_tables_are_clamped(shape):
    """Straight through the C ABI: hi > T_l and lo < 0 are clamped, lo >= hi (before or after clamping) gives exactly 0.0."""
    C, F, T = shape
    xs = [_values(2, C, F, T, seed=T)]
    big = 2 ** 31 - 1
    segs = [(0, T + 5), (3, 3), (5, 2), (-4, 2), (T, T + 9), (-7, -1), (T - 1, big), (-big, big), (big, -big), (T + 1, T + 2)]
    lo = np.array([[s[0] for s in segs]], dtype=np.int64)
    hi = np.array([[s[1] for s in segs]], dtype=np.int64)
    with pytest.raises(_lib.EatHipError, match="need 0 <= lo < hi"):
        ops.check_segments(lo, hi, [T])
    got = _run(xs, lo, hi, raw=True)
    for s in (1, 2, 4, 5, 8, 9):
        assert bool((got[:, s, :] == 0.0).all()), s
    assert np.array_equal(got[:, 0, :], got[:, 7, :])                # both are the whole plane after clamping
    _check(f"{shape} unvalidated", got, xs, lo, hi)


def test_wrapper_refuses_bad_operands():
    x = torch.zeros((2, 3, 4, 5), device=DEV)
    lo, hi = _tables(5, "scene")
    with pytest.raises(_lib.EatHipError, match="1 to 64 feature maps"):
        ops.embed_pool([], lo, hi)
    with pytest.raises(_lib.EatHipError, match="one B"):
        ops.embed_pool([x, x[:1]], np.repeat(lo, 2, 0), np.repeat(hi, 2, 0))
    with pytest.raises(_lib.EatHipError, match="contiguous float32"):
        ops.embed_pool([x.transpose(2, 3)], lo, hi)
    with pytest.raises(_lib.EatHipError, match="ragged"):
        ops.embed_pool([x, x], lo, hi)
    with pytest.raises(_lib.EatHipError, match="out must be"):
        ops.embed_pool([x], lo, hi, out=torch.empty((2, 1, 4), device=DEV))
    assert ops.embed_pool([x], lo, hi).shape == (2, 1, 3)
