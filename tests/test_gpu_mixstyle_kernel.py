"""eat_freq_mixstyle (csrc/mixstyle.hip) against the float64 reference of tests/dcase20_ref.py.

The tolerance is not a constant: the same cases go through the fp32 torch restatement of helpers/utils.py `mixstyle` on the
CPU, its worst error against fp64 over ALL cases is taken per quantity (output, mu, sig), and the kernel is allowed 4x that
(its sums run in another order).  The statistics are checked on their own because the variance's divisor cancels in the
output (every row has the same n): only the sig check can tell n - 1 from n.  At n = 1000 that gap is 5e-4 relative, and
the sig bound must stay below it."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, ops  # noqa: E402
from tests.dcase20_ref import freq_mixstyle_ref, freq_mixstyle_torch_fp32, mixstyle_errors  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [(1, 1, 1, 2), (3, 1, 7, 2), (6, 1, 3, 63), (2, 1, 5, 64), (4, 3, 40, 65), (5, 1, 128, 1000), (2, 1, 128, 1001),
          (2, 1, 4, 4099)]                                                     # (the last: C T > 1024, the re-reading kernel)
DRAWS = ("identity", "fixed_point", "random")
CASES = [(s, d) for s in SHAPES for d in DRAWS]
BIASED_GAP = 5e-4                                                              # sqrt(1000 / 999) - 1


def _input(shape, seed):
    """Log-mel-like rows (every (b, f) row its own level and spread); when there are at least four rows, rows 0..2 are the
    probes: a constant row, a row of mean 8 and std 0.01 (cancellation), a row scaled by 1e-4."""
    B, C, F, T = shape
    g = torch.Generator().manual_seed(seed)
    level = torch.randn(B, 1, F, 1, generator=g) * 3
    spread = torch.rand(B, 1, F, 1, generator=g) * 2 + 0.1
    x = (torch.randn(B, C, F, T, generator=g) * spread + level).float()
    if B * F >= 4:
        rows = [(r // F, r % F) for r in range(3)]
        x[rows[0][0], :, rows[0][1], :] = 2.5
        x[rows[1][0], :, rows[1][1], :] = 8.0 + 0.01 * torch.randn(C, T, generator=g)
        x[rows[2][0], :, rows[2][1], :] *= 1e-4
    return x


def _draws(B, kind, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    lam = torch.rand(B, generator=g)
    if kind == "identity":
        perm = torch.arange(B)
    elif kind == "fixed_point":
        perm = torch.roll(torch.arange(B), 1)
        perm[0] = 0                                                            # perm[0] = 0: a sample mixed with itself
    else:
        perm = torch.randperm(B, generator=g)
        lam[0] = 0.0                                                           # lam holds exact 0 and (B > 1) exact 1
        if B > 1:
            lam[1] = 1.0
    return perm, lam.float()


@pytest.fixture(scope="module")
def cases():
    """Per case: input, draws, fp64 reference, the restatement's errors.  Computed once; never modified."""
    out = {}
    for k, (shape, kind) in enumerate(CASES):
        x = _input(shape, k)
        perm, lam = _draws(shape[0], kind, k)
        ref = freq_mixstyle_ref(x.numpy(), perm.numpy(), lam.numpy())
        t_out, t_mu, t_sig = freq_mixstyle_torch_fp32(x, perm, lam)
        out[(shape, kind)] = dict(x=x, perm=perm, lam=lam, ref=ref,
                                  torch_err=mixstyle_errors(t_out.numpy(), t_mu.numpy(), t_sig.numpy(), ref, x.numpy()))
    return out


@pytest.fixture(scope="module")
def bounds(cases):
    worst = np.max(np.array([c["torch_err"] for c in cases.values()]), axis=0)
    b = 4.0 * worst
    print(f"fp32 torch restatement, worst over {len(cases)} cases: out {worst[0]:.2e}, mu {worst[1]:.2e}, sig {worst[2]:.2e}")
    assert b[2] < BIASED_GAP, f"the sig bound {b[2]:.2e} could not tell the biased variance: the test is wrong"
    return b


def _run(x, perm, lam, apply=None, out=None, stats=None):
    xd = x.to(DEV) if not x.is_cuda else x
    if stats is None:
        stats = torch.full((x.shape[0], x.shape[2], 2), float("nan"), device=DEV)
    out = ops.freq_mixstyle(xd, perm, lam, apply=apply, out=out, stats=stats)
    torch.cuda.synchronize()
    return out, stats


@pytest.mark.parametrize("shape,kind", CASES, ids=[f"{'x'.join(map(str, s))}-{d}" for s, d in CASES])
def test_freq_mixstyle_against_fp64(shape, kind, cases, bounds):
    c = cases[(shape, kind)]
    out, stats = _run(c["x"], c["perm"], c["lam"])
    got = out.cpu().numpy()
    st = stats.cpu().numpy()
    assert np.isfinite(got).all() and np.isfinite(st).all()
    e = mixstyle_errors(got, st[:, :, 0], st[:, :, 1], c["ref"], c["x"].numpy())
    t = c["torch_err"]
    print(f"{shape} {kind}: scaled out err {e[0]:.2e} (torch fp32 {t[0]:.2e}), mu {e[1]:.2e} ({t[1]:.2e}), "
          f"sig {e[2]:.2e} ({t[2]:.2e}); bounds {bounds[0]:.2e} {bounds[1]:.2e} {bounds[2]:.2e}")
    assert e[0] <= bounds[0] and e[1] <= bounds[1] and e[2] <= bounds[2], (e, tuple(bounds))
    # device draw tables (the captured step's path) and a second call: the same bits
    out2, stats2 = _run(c["x"], c["perm"].to(DEV, torch.int32), c["lam"].to(DEV))
    assert torch.equal(out2, out) and torch.equal(stats2, stats)
    out3, stats3 = _run(c["x"], c["perm"], c["lam"])
    assert torch.equal(out3, out) and torch.equal(stats3, stats)


@pytest.mark.parametrize("shape", [(2, 1, 128, 1001), (4, 3, 40, 65)])
@pytest.mark.parametrize("x_off,out_off", [(0, 1), (1, 1), (1, 0)])
def test_freq_mixstyle_unaligned_views(shape, x_off, out_off, cases, bounds):
    """Views off by one float: out alone (x is then read value by value), both (rows start with a scalar head), x alone."""
    c = cases[(shape, "random")]
    n = c["x"].numel()
    xbuf = torch.zeros(n + 1, device=DEV)
    xv = xbuf[x_off:x_off + n].view(shape)
    xv.copy_(c["x"])
    obuf = torch.full((n + 2,), float("nan"), device=DEV)
    ov = obuf[out_off:out_off + n].view(shape)
    out, stats = _run(xv, c["perm"], c["lam"], out=ov)
    assert out.data_ptr() == ov.data_ptr()
    e = mixstyle_errors(ov.cpu().numpy(), stats[:, :, 0].cpu().numpy(), stats[:, :, 1].cpu().numpy(), c["ref"], c["x"].numpy())
    print(f"{shape} x+{x_off} out+{out_off}: scaled out err {e[0]:.2e}, mu {e[1]:.2e}, sig {e[2]:.2e}")
    assert e[0] <= bounds[0] and e[1] <= bounds[1] and e[2] <= bounds[2], (e, tuple(bounds))
    tail = obuf[out_off + n:].cpu()
    assert torch.isnan(tail).all() and (out_off == 0 or torch.isnan(obuf[0]).item())   # nothing written around the view
    # the aligned call gives the same bits: the result does not depend on how a row is cut into head, body and tail
    ref_out, _ = _run(c["x"], c["perm"], c["lam"])
    assert torch.equal(ov, ref_out)


def test_apply_flag():
    """Flag 0: out is x bit for bit and the workspace keeps its poison; flag 1 and NULL give the same bits."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, 2, 9, 37, generator=g)
    x[0, 0, 0, :3] = torch.tensor([float("inf"), -0.0, 1e-42])                 # a copy keeps what arithmetic would not
    perm, lam = torch.tensor([2, 0, 1]), torch.tensor([0.3, 0.9, 0.5])
    zero = torch.zeros(1, device=DEV, dtype=torch.int32)
    one = torch.ones(1, device=DEV, dtype=torch.int32)
    out0, stats0 = _run(x, perm, lam, apply=zero)
    assert torch.equal(out0.cpu().view(torch.int32), x.view(torch.int32)) and torch.isnan(stats0).all()
    x[0, 0, 0, :3] = 0.25
    out1, stats1 = _run(x, perm, lam, apply=one)
    outn, statsn = _run(x, perm, lam)
    assert torch.equal(out1, outn) and torch.equal(stats1, statsn) and not torch.equal(out1.cpu(), x)
    # the flag is read on the device at run time: the same call, the flag flipped in place
    one.zero_()
    out2, _ = _run(x, perm, lam, apply=one)
    assert torch.equal(out2.cpu(), x)


def test_freq_mixstyle_rejects_bad_arguments():
    h = _lib.lib()
    x = torch.zeros(2, 1, 4, 8, device=DEV)
    out = torch.full_like(x, float("nan"))
    stats = torch.full((2, 4, 2), float("nan"), device=DEV)
    perm = torch.arange(2, device=DEV, dtype=torch.int32)
    lam = torch.ones(2, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    px, pp, pl, po, ps = (t.data_ptr() for t in (x, perm, lam, out, stats))
    eps = ctypes.c_float(1e-6)

    def rc(x_=px, perm_=pp, lam_=pl, out_=po, stats_=ps, shape=(2, 1, 4, 8)):
        return ctypes.c_int(h.eat_freq_mixstyle(x_, perm_, lam_, None, out_, stats_, *shape, eps, st)).value

    assert rc() == 0
    torch.cuda.synchronize()
    out.fill_(float("nan"))
    stats.fill_(float("nan"))
    for shape in [(0, 1, 4, 8), (2, 0, 4, 8), (2, 1, 0, 8), (2, 1, 4, 0), (-1, 1, 4, 8), (2, 1, 4, -8),
                  (2, 1, 4, 1),                                                # C T < 2: no unbiased variance
                  (65536, 1, 128, 1000)]:                                      # beyond int32 indexing
        assert rc(shape=shape) == -1, shape
    assert rc(x_=None) == -1 and rc(perm_=None) == -1 and rc(lam_=None) == -1 and rc(out_=None) == -1
    assert rc(stats_=None) == -1
    assert rc(out_=px) == -1                                                   # in place
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(stats).all() and not x.any()   # nothing was launched
    with pytest.raises(ValueError):
        ops.freq_mixstyle(x, torch.tensor([0, 2]), torch.ones(2), out=out, stats=stats)
    with pytest.raises(ValueError):
        ops.freq_mixstyle(x, torch.tensor([-1, 0]), torch.ones(2), out=out, stats=stats)
    with pytest.raises(ValueError):
        ops.freq_mixstyle(x, torch.tensor([0, 1, 0]), torch.ones(2), out=out, stats=stats)
    ok = torch.tensor([1, 0])
    for bad in (lambda: ops.freq_mixstyle(x.cpu(), ok, torch.ones(2)),                      # no CPU path
                lambda: ops.freq_mixstyle(x.double(), ok, torch.ones(2)),
                lambda: ops.freq_mixstyle(x[0], ok, torch.ones(2)),                         # not (B, C, F, T)
                lambda: ops.freq_mixstyle(x, ok, torch.ones(3)),
                lambda: ops.freq_mixstyle(x, ok, torch.ones(2), out=x),
                lambda: ops.freq_mixstyle(x, ok, torch.ones(2), out=out[:1]),
                lambda: ops.freq_mixstyle(x, ok, torch.ones(2), stats=stats[:1]),
                lambda: ops.freq_mixstyle(x, perm.long(), lam),                             # device perm must be int32
                lambda: ops.freq_mixstyle(x, ok, torch.ones(2), apply=torch.ones(1, device=DEV)),
                lambda: ops.freq_mixstyle(torch.zeros(2, 1, 4, 1, device=DEV), ok, torch.ones(2))):
        with pytest.raises(_lib.EatHipError):
            bad()
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(stats).all()
