"""The kernels of csrc/detect.hip alone against the restatements of tests/detect_ref.py: stitch within 1e-6 of the fp64
weighted mean (the bar tests/test_gpu_tagger_kernels.py gives the same fp32 sigmoid; a convex combination adds a few
6e-8 roundings), the median bit for bit, the event list exactly with the mean within one fp32 ulp.  Outputs are pre-filled
with NaN, so are the pad columns of p and the columns past a recording's end; every output element must come back finite,
and two calls must agree bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import ops  # noqa: E402
from efficientat_amd._lib import EatHipError  # noqa: E402
from tests import detect_ref as R  # noqa: E402

DEV = torch.device("cuda:0")


def _rec(rows):
    """[(window count, G)] -> table rows (first, count, goff, G)."""
    out, first, goff = [], 0, 0
    for count, G in rows:
        out.append((first, count, goff, G))
        first, goff = first + count, goff + G
    return out


# ------------------------------------------------------------------------------------------------ stitch
@pytest.mark.parametrize("taper", ["uniform", "triangle"])
@pytest.mark.parametrize("K,T,Hf,n_w", [(1, 1, 1, 1), (3, 10, 10, 3), (3, 10, 1, 12), (527, 32, 16, 5), (5, 32, 7, 4)])
def test_stitch(K, T, Hf, n_w, taper):
    """Two recordings back to back: A with n_w windows whose last one has a single valid frame, B shorter than a window."""
    Tp = ops.pitch4(T)
    rec = _rec([(n_w, (n_w - 1) * Hf + 1), (1, max(1, T // 2))])
    N = n_w + 1
    g = torch.Generator().manual_seed(K * 1000 + T * 10 + Hf)
    p = 3.0 * torch.randn((N, K, Tp), generator=g)
    flat = p.view(-1)
    where = torch.randperm(flat.numel(), generator=g)[:max(2, flat.numel() // 50)]
    flat[where[::2]] = 100.0
    flat[where[1::2]] = -100.0
    p[:, :, T:] = float("nan")                                 # pad columns
    for first, count, _, G in rec:
        for q in range(count):
            p[first + q, :, max(0, min(T, G - q * Hf)):] = float("nan")       # columns whose frame is >= G
    wt = ops.detect_weights(T, taper)
    table = ops.detect_table(rec)
    d_p, d_wt = p.to(DEV), torch.from_numpy(wt.astype(np.float32)).to(DEV)
    out = torch.full((K, table.G_total), float("nan"), device=DEV)
    got = ops.detect_stitch(d_p, table, Hf, T, d_wt, out=out)
    assert got.data_ptr() == out.data_ptr() and got.shape == (K, table.G_total)
    again = ops.detect_stitch(d_p, table, Hf, T, d_wt)
    want = R.stitch_ref(p.numpy(), rec, Hf, T, wt)
    assert np.isfinite(want).all()
    err = float(np.abs(got.double().cpu().numpy() - want).max())
    print(f"stitch K={K} T={T} Hf={Hf} n_w={n_w} {taper}: max |prob - ref| = {err:.3e} over {want.size} elements")
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, again)
    assert err <= 1e-6
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0


# ------------------------------------------------------------------------------------------------ median
LENGTHS = [1, 2, 15, 16, 31, 64, 65, 1000]


def _tenths(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 11, shape, generator=g).float() / 10.0


def _median_case(x, rec, m):
    table = ops.detect_table(rec)
    d_x = x.to(DEV)
    out = torch.full(tuple(x.shape), float("nan"), device=DEV)
    got = ops.detect_median(d_x, table, m, out=out)
    again = ops.detect_median(d_x, table, m)
    want = torch.from_numpy(R.median_ref(d_x.cpu().numpy(), rec, m))
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, again)
    return got.cpu(), want


@pytest.mark.parametrize("K", [1, 527])
@pytest.mark.parametrize("m", [1, 3, 5, 31])
def test_median_all_lengths_side_by_side(m, K):
    """Recordings of every length in one table (tiles that hold several recordings, recordings that span several tiles), then
    two neighbours at the levels 0.1 and 0.9: a read across their boundary would show in either."""
    rec = _rec([(1, G) for G in LENGTHS] + [(1, 20), (1, 20)])
    x = _tenths((K, sum(r[3] for r in rec)), seed=m * 7 + K)
    lo0 = rec[-2][2]
    x[:, lo0:lo0 + 20] = 0.1
    x[:, lo0 + 20:] = 0.9
    got, want = _median_case(x, rec, m)
    bad = int((got != want).sum())
    print(f"median m={m} K={K}: {bad} of {want.numel()} elements differ from median_ref")
    assert torch.equal(got, want)
    assert torch.equal(got[:, lo0:], x[:, lo0:])               # constant recordings stay what they are
    if m == 1:
        assert torch.equal(got, x)


@pytest.mark.parametrize("G", LENGTHS)
def test_median_one_recording(G):
    for m in (3, 5, 31):
        got, want = _median_case(_tenths((3, G), seed=G + m), [(0, 1, 0, G)], m)
        print(f"median G={G} m={m}: {int((got != want).sum())} of {want.numel()} elements differ")
        assert torch.equal(got, want)


def test_median_refuses_aliasing_and_bad_widths():
    x = _tenths((2, 40), seed=1).to(DEV)
    table = ops.detect_table([(0, 1, 0, 40)])
    with pytest.raises(EatHipError, match="out must not overlap prob"):
        ops.detect_median(x, table, 3, out=x)
    buf = torch.zeros(120, device=DEV)
    with pytest.raises(EatHipError, match="out must not overlap prob"):
        ops.detect_median(buf[:80].view(2, 40), table, 3, out=buf[40:].view(2, 40))
    for m in (0, 2, 33):
        with pytest.raises(EatHipError, match="odd integer in"):
            ops.detect_median(x, table, m)


def test_stitch_and_median_index_past_2_to_31():
    """K G_total > 2^31 elements in p, prob and filt: the last class row lies wholly beyond a 32-bit element index."""
    K, T, n_w_a, G_b = 33, 4, 2 ** 24, 37
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < 30 * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GB of device memory free: three 8.9 GB buffers need 30")
    rec = _rec([(n_w_a, n_w_a * T), ((G_b + T - 1) // T, G_b)])
    table = ops.detect_table(rec)
    N = rec[1][0] + rec[1][1]
    assert K * table.G_total > 2 ** 31 and N * K * T > 2 ** 31
    p = torch.empty((N, K, T), device=DEV)
    p.normal_(generator=torch.Generator(device=DEV).manual_seed(3))
    wt = torch.ones(T, device=DEV)
    prob = ops.detect_stitch(p, table, T, T, wt)
    # windows do not overlap: prob[k, 4 q + j] = sigmoid(p[q, k, j])
    for k in (0, K - 1):
        for q0, q1 in ((0, 512), (n_w_a - 512, n_w_a)):
            want = 1.0 / (1.0 + torch.exp(-p[q0:q1, k, :].double())).reshape(-1)
            err = float((prob[k, q0 * T:q1 * T].double() - want).abs().max())
            print(f"stitch past 2^31: class {k}, windows [{q0}, {q1}): max err {err:.3e}")
            assert err <= 1e-6
    tail = 1.0 / (1.0 + torch.exp(-p[n_w_a:, K - 1, :].double())).reshape(-1)[:G_b]
    assert float((prob[K - 1, n_w_a * T:].double() - tail).abs().max()) <= 1e-6
    del p
    filt = ops.detect_median(prob, table, 5)
    G_a = n_w_a * T
    for k in (0, K - 1):
        end = prob[k, G_a - 300:G_a].cpu().numpy()[None, :]    # the end of recording A: its left context is inside the slice
        want = R.median_ref(end, [(0, 1, 0, 300)], 5)[0, 100:]
        assert np.array_equal(filt[k, G_a - 200:G_a].cpu().numpy(), want)
        last = prob[k, G_a:].cpu().numpy()[None, :]
        assert np.array_equal(filt[k, G_a:].cpu().numpy(), R.median_ref(last, [(0, 1, 0, G_b)], 5)[0])
        head = prob[k, :300].cpu().numpy()[None, :]
        assert np.array_equal(filt[k, :200].cpu().numpy(), R.median_ref(head, [(0, 1, 0, 300)], 5)[0, :200])
    del prob, filt
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ events
def _events_case(name, filt, rec, hi, lo, max_gap=0, min_len=0):
    filt = np.asarray(filt, dtype=np.float32)
    table = ops.detect_table(rec)
    d = torch.from_numpy(filt).to(DEV)
    ev_i, ev_f = ops.detect_events(d, table, hi, lo, max_gap, min_len)
    ev_i2, ev_f2 = ops.detect_events(d, table, hi, lo, max_gap, min_len)
    want_i, want_peak, want_mean = R.events_ref(filt, rec, hi, lo, max_gap, min_len)
    assert ev_i.dtype == torch.int32 and ev_f.dtype == torch.float32 and ev_i.is_cuda and ev_f.is_cuda
    assert ev_i.shape == (len(want_i), 4) and ev_f.shape == (len(want_i), 2), (name, tuple(ev_i.shape), len(want_i))
    assert torch.equal(ev_i, ev_i2) and torch.equal(ev_f, ev_f2)
    got_i, got_f = ev_i.cpu().numpy(), ev_f.cpu().numpy()
    m32 = want_mean.astype(np.float32)
    ulps = np.abs(got_f[:, 1].astype(np.float64) - m32.astype(np.float64)) / np.spacing(m32).astype(np.float64) if len(m32) else np.zeros(0)
    print(f"events {name}: {len(want_i)} events, ints equal {np.array_equal(got_i, want_i)}, peak equal "
          f"{np.array_equal(got_f[:, 0], want_peak)}, mean off by at most {float(ulps.max()) if len(ulps) else 0.0:.2f} ulp")
    assert np.array_equal(got_i, want_i), name
    assert np.array_equal(got_f[:, 0], want_peak), name
    assert bool((ulps <= 1.0).all()), name
    assert bool(np.isfinite(got_f).all())
    return got_i


def _line(G, spans, level=0.6, floor=0.1):
    v = np.full(G, floor, dtype=np.float32)
    for a, b in spans:
        v[a:b] = level
    return v


A_, B_, Z_ = 0.6, 0.4, 0.1


def test_events_hand_cases():
    one = lambda v: (np.asarray(v, dtype=np.float32)[None, :], [(0, 1, 0, len(v))])
    got = _events_case("first and last frame", *one([A_, Z_, Z_, A_]), 0.5, 0.3)
    assert got.tolist() == [[0, 0, 0, 1], [0, 0, 3, 4]]
    assert len(_events_case("never reaches hi", *one([Z_, B_, B_, Z_]), 0.5, 0.3)) == 0
    assert _events_case("run is the event", *one([Z_, B_, A_, B_, Z_]), 0.5, 0.3).tolist() == [[0, 0, 1, 4]]
    assert _events_case("lo == hi", *one([Z_, B_, A_, B_, Z_]), 0.5, 0.5).tolist() == [[0, 0, 2, 3]]
    v = _line(300, [(60, 71)])
    v[65] = 0.4                                                # reaches hi on either side of the 64-frame step
    assert _events_case("frames 60-70", v[None, :], [(0, 1, 0, 300)], 0.5, 0.3).tolist() == [[0, 0, 60, 71]]
    v = _line(300, [(60, 71)], level=0.4)
    v[64] = 0.6                                                # reaches hi only after the step boundary
    assert _events_case("frames 60-70, hi at 64", v[None, :], [(0, 1, 0, 300)], 0.5, 0.3).tolist() == [[0, 0, 60, 71]]
    v[64] = 0.4
    v[63] = 0.6                                                # ... only before it
    assert _events_case("frames 60-70, hi at 63", v[None, :], [(0, 1, 0, 300)], 0.5, 0.3).tolist() == [[0, 0, 60, 71]]
    ramp = (0.55 + 0.4 * np.arange(201) / 200).astype(np.float32)
    v = _line(300, [])
    v[:201] = ramp
    assert _events_case("frames 0-200", v[None, :], [(0, 1, 0, 300)], 0.5, 0.3).tolist() == [[0, 0, 0, 201]]
    assert _events_case("run ends at 64", _line(128, [(10, 64)])[None, :], [(0, 1, 0, 128)], 0.5, 0.3).tolist() == [[0, 0, 10, 64]]
    assert _events_case("run starts at 64", _line(128, [(64, 128)])[None, :], [(0, 1, 0, 128)], 0.5, 0.3).tolist() == [[0, 0, 64, 128]]
    assert _events_case("G = 64, all active", _line(64, [(0, 64)])[None, :], [(0, 1, 0, 64)], 0.5, 0.3).tolist() == [[0, 0, 0, 64]]
    assert _events_case("gap == max_gap", *one([A_, Z_, Z_, A_]), 0.5, 0.3, 2).tolist() == [[0, 0, 0, 4]]
    assert _events_case("gap == max_gap + 1", *one([A_, Z_, Z_, Z_, A_]), 0.5, 0.3, 2).tolist() == [[0, 0, 0, 1], [0, 0, 4, 5]]
    v = _line(200, [(50, 62), (70, 80)])                       # a gap of 8 frames across the step boundary
    assert _events_case("gap across a step", v[None, :], [(0, 1, 0, 200)], 0.5, 0.3, 8).tolist() == [[0, 0, 50, 80]]
    assert len(_events_case("gap across a step + 1", v[None, :], [(0, 1, 0, 200)], 0.5, 0.3, 7)) == 2
    assert _events_case("min_len and one less", *one([A_, A_, Z_, A_]), 0.5, 0.3, 0, 2).tolist() == [[0, 0, 0, 2]]
    assert _events_case("merge, then drop", *one([A_, Z_, A_, Z_, Z_, Z_, A_]), 0.5, 0.3, 1, 3).tolist() == [[0, 0, 0, 3]]
    assert len(_events_case("no merge: both too short", *one([A_, Z_, A_]), 0.5, 0.3, 0, 2)) == 0
    assert _events_case("a run that does not count lies in the gap", *one([A_, Z_, B_, Z_, A_]), 0.5, 0.3, 3).tolist() == [[0, 0, 0, 5]]
    assert _events_case("all active", *one([A_] * 130), 0.5, 0.3).tolist() == [[0, 0, 0, 130]]
    got_i = _events_case("none active", *one([Z_] * 130), 0.5, 0.3, 5, 0)
    assert got_i.shape == (0, 4)
    filt = np.array([[A_, A_, Z_, A_, B_], [Z_, A_, A_, Z_, Z_]], dtype=np.float32)
    assert _events_case("per-class thresholds", filt, [(0, 1, 0, 5)], [0.5, 0.7], [0.3, 0.3]).tolist() == [[0, 0, 0, 2], [0, 0, 3, 5]]
    assert _events_case("per-class lo", filt, [(0, 1, 0, 5)], [0.5, 0.5], [0.3, 0.5]).tolist() == \
        [[0, 0, 0, 2], [0, 0, 3, 5], [0, 1, 1, 3]]
    filt = np.array([[Z_, A_, A_, A_, A_, Z_]], dtype=np.float32)
    got = _events_case("A ends active, B starts active", filt, [(0, 1, 0, 3), (1, 1, 3, 3)], 0.5, 0.3, 5)
    assert got.tolist() == [[0, 0, 1, 3], [1, 0, 0, 2]]


@pytest.mark.parametrize("max_gap,min_len", [(0, 0), (2, 0), (0, 3), (3, 5), (400, 0), (1, 400)])
def test_events_random_timelines(max_gap, min_len):
    rng = np.random.default_rng(17)
    rec = _rec([(1, 300), (1, 65), (1, 129)])
    K = 17
    # tenths with some persistence, so that runs of several lengths occur
    walk = np.cumsum(rng.integers(-1, 2, size=(K, rec[-1][2] + rec[-1][3])), axis=1)
    filt = (np.abs(walk + rng.integers(0, 11, size=(K, 1))) % 11 / 10.0).astype(np.float32)
    hi = (rng.integers(4, 9, size=K) / 10.0).astype(np.float32)
    lo = np.minimum(hi, (rng.integers(1, 6, size=K) / 10.0).astype(np.float32))
    got = _events_case(f"random gap={max_gap} len={min_len}", filt, rec, hi, lo, max_gap, min_len)
    if (max_gap, min_len) == (0, 0):
        assert len(got) > 50
    order = [tuple(r[:3]) for r in got.tolist()]
    assert order == sorted(order)
