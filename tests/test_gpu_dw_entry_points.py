"""GPU tests of the host layer behind the eight depthwise training entry points that share one validation each
(csrc/conv_spatial.hip: eat_dw_conv[_dyn]_fwd_stats[_b16]; csrc/dw_grad.hip: eat_dw_conv[_dyn]_bwd_bn_g[_b16]):
  * arguments that are refused before any launch answer EAT_EINVAL with a message that names the entry point called;
  * one accepted call per entry point and covered geometry lands every operand in its own role - gscale / gadd, res,
    gpart / gzpart - against the fp64 references and the fp32 twins of tests/test_gpu_train_fuse.py,
    tests/test_gpu_dymn.py, tests/test_gpu_bf16_store.py and tests/test_gpu_dymn_bf16.py (their helpers and tolerances).
Planes of 4 x 32 (whole rows per lane group) and 16 x 130 (tiles), 3x3 / stride 1 and 5x5 / stride 2."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, ops  # noqa: E402
from tests import test_gpu_bf16_store as S16  # noqa: E402
from tests import test_gpu_dymn_bf16 as D16  # noqa: E402

DEV = torch.device("cuda:0")
BF = torch.bfloat16
EAT_EINVAL = -1
_rand, _rel = S16._rand, S16._rel
ACTS = [lambda t: t, F.relu, F.hardswish]

B, C = 2, 8
GEOMS = [(4, 32, 3, 1), (4, 32, 5, 2), (16, 130, 3, 1), (16, 130, 5, 2)]
# the bf16-storage forward has register-resident kernels only: of the four, the tiled planes (T > 128)
GEOMS_FWD16 = [g for g in GEOMS if g[1] > 128]


def _out(n, k, s):
    return (n + 2 * ((k - 1) // 2) - k) // s + 1


def _uni(*shape, seed, lo=0.5):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) + lo


# ------------------------------------------------------------------ refused before any launch
FWD = ["eat_dw_conv_fwd_stats", "eat_dw_conv_fwd_stats_b16", "eat_dw_conv_dyn_fwd_stats", "eat_dw_conv_dyn_fwd_stats_b16"]
BWD = ["eat_dw_conv_bwd_bn_g", "eat_dw_conv_bwd_bn_g_b16", "eat_dw_conv_dyn_bwd_bn_g", "eat_dw_conv_dyn_bwd_bn_g_b16"]
ORDER = {
    "fwd": ["x", "x_b16", "in_a", "in_b", "in_act", "w", "y", "part", "inner_cap", "h_inner"],
    "bwd": ["dy", "z", "bn_a", "bn_b", "bn_mean", "bn_invstd", "gscale", "gadd", "sums", "bn_act", "frozen", "x", "x_b16", "in_a",
            "in_b", "in_act", "w", "g", "dw", "gpart", "inner_cap", "h_inner"],
    "dyn_bwd": ["dy", "z", "bn_a", "bn_b", "bn_mean", "bn_invstd", "sums", "bn_act", "frozen", "x", "x_b16", "in_a", "in_b", "in_act",
                "w", "res", "g", "dw", "gpart", "gzpart", "inner_cap", "h_inner"],
}
GEOM_ARGS = ["B", "C", "F", "T", "Fo", "To", "k", "stride"]


class _Call:
    """A valid call of one entry point at 4 x 32 planes, 5x5 / stride 1 (all eight have a kernel there), with every buffer
    large enough for the geometries the cases below ask for instead (so that a call that slipped through the validation would
    still stay in bounds)."""

    def __init__(self, name):
        self.name = name
        self.fwd, self.b16, self.dyn = name in FWD, name.endswith("_b16"), "_dyn_" in name
        wide = lambda: torch.zeros(B * C * 8 * 40, device=DEV)             # fp32 or bf16 planes of up to 8 x 40
        chan = lambda: torch.ones(B * C * 25, device=DEV)                  # per-channel vectors, taps, per-plane factors
        self.keep = {n: wide() for n in ("x", "y", "dy", "z", "g", "res", "part", "gpart", "gzpart")}
        self.keep.update({n: chan() for n in ("in_a", "in_b", "w", "dw", "bn_a", "bn_b", "bn_mean", "bn_invstd", "gscale", "gadd")})
        self.keep["sums"] = torch.zeros(2 * C, device=DEV, dtype=torch.float64)
        self.inner = ctypes.c_int(0)
        self.v = {n: t.data_ptr() for n, t in self.keep.items()}
        self.v.update(x_b16=1, in_act=1, bn_act=2, frozen=0, inner_cap=1, h_inner=ctypes.addressof(self.inner), res=None,
                      B=B, C=C, F=4, T=32, Fo=4, To=32, k=5, stride=1)

    def run(self, **change):
        v = dict(self.v, **change)
        order = ORDER["fwd" if self.fwd else ("dyn_bwd" if self.dyn else "bwd")]
        args = [v[n] for n in order if n != "x_b16" or self.b16] + [v[n] for n in GEOM_ARGS] + [ops._stream()]
        h = _lib.lib()
        rc = getattr(h, self.name)(*args)
        return rc, h.eat_last_error_string().decode()


def _refused(name, word, **change):
    rc, msg = _Call(name).run(**change)
    assert rc == EAT_EINVAL and msg.startswith(name + ":") and word in msg, (rc, msg)


@pytest.mark.parametrize("name", FWD + BWD)
def test_the_unchanged_call_is_accepted(name):
    """(so that each refusal below is owed to the one argument it changes)"""
    c = _Call(name)
    rc, msg = c.run()
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert c.inner.value == 1


@pytest.mark.parametrize("name,missing", [(n, p) for n in FWD for p in ("x", "w", "y", "part", "h_inner")] +
                         [(n, p) for n in BWD for p in ("dy", "z", "bn_a", "sums", "x", "in_b", "w", "g", "dw")])
def test_missing_required_pointer_is_refused(name, missing):
    _refused(name, "partial buffer" if missing in ("part", "h_inner") else "missing operand", **{missing: None})


@pytest.mark.parametrize("name", FWD + BWD)
def test_bad_activation_code_is_refused(name):
    _refused(name, "act", in_act=3)


@pytest.mark.parametrize("name", FWD + BWD)
def test_partial_buffer_one_slot_short_is_refused(name):
    h = _lib.lib()
    geom = dict(F=8, T=40, Fo=8, To=40, k=3, stride=1)
    need = h.eat_dw_partials_inner(8, 40, 8, 40, 3, 1, 0) if name in FWD else h.eat_dw_bwd_partials_inner(8, 40, 8, 40, 3, 1)
    assert need >= 1
    _refused(name, "partial buffer too small", inner_cap=need - 1, **geom)


@pytest.mark.parametrize("name", [n for n in FWD + BWD if n.endswith("_b16")])
def test_odd_plane_size_is_refused_by_the_bf16_variants(name):
    _refused(name, "even number" if name in FWD else "geometry not covered", F=3, T=33, Fo=3, To=33)


def test_skip_gradient_with_bf16_g_is_refused():
    c = _Call("eat_dw_conv_dyn_bwd_bn_g_b16")
    rc, msg = c.run(res=c.keep["res"].data_ptr(), x_b16=1)
    assert rc == EAT_EINVAL and msg.startswith("eat_dw_conv_dyn_bwd_bn_g_b16:") and "skip gradient" in msg, (rc, msg)


@pytest.mark.parametrize("name", FWD + BWD)
def test_stride_1_with_another_output_height_is_refused(name):
    _refused(name, "inconsistent" if name in FWD else "geometry not covered", Fo=5)


# ------------------------------------------------------------------ accepted calls: forward + statistics
def _fwd_inputs(Fq, T, k, dyn):
    x = _rand(B, C, Fq, T, seed=1, scale=1.5) + _rand(1, C, 1, 1, seed=2)
    w = _rand(B, C * k * k, seed=3, scale=0.3) if dyn else _rand(C, k * k, seed=3, scale=0.3)
    return x, w, _uni(C, seed=4), _rand(C, seed=5, scale=0.3)


def _conv64(xin, w, k, s, dyn):
    if not dyn:
        return F.conv2d(xin, w.double().reshape(C, 1, k, k), None, s, (k - 1) // 2, 1, C)
    y = F.conv2d(xin.reshape(1, B * C, *xin.shape[2:]), w.double().reshape(B * C, 1, k, k), None, s, (k - 1) // 2, 1, B * C)
    return y.reshape(B, C, *y.shape[2:])


def _stat_sums(parts):
    part, outer, inner = parts
    return part[:outer * 2 * C * inner].view(outer, 2, C, inner).double().sum((0, 3)).cpu()


@pytest.mark.parametrize("Fq,T,k,s", GEOMS)
@pytest.mark.parametrize("dyn", [False, True], ids=["static", "dyn"])
def test_forward_statistics_fp32(Fq, T, k, s, dyn):
    x, w, ia, ib = _fwd_inputs(Fq, T, k, dyn)
    act = ops.ACT_HSWISH
    y_ref = _conv64(ACTS[act](x.double() * ia.double()[None, :, None, None] + ib.double()[None, :, None, None]), w, k, s, dyn)
    fn = ops.dw_conv_dyn_stats if dyn else ops.dw_conv_stats
    y, parts = fn(x.to(DEV), w.to(DEV), k, s, tf=(ia.to(DEV), ib.to(DEV), act))
    assert _rel(y, y_ref) < (5e-6 if dyn else 3e-6)
    st, yd = _stat_sums(parts), y.double().cpu()
    assert _rel(st[0], yd.sum((0, 2, 3))) < 1e-5 and _rel(st[1], (yd ** 2).sum((0, 2, 3))) < 1e-5


@pytest.mark.parametrize("Fq,T,k,s", GEOMS_FWD16)
@pytest.mark.parametrize("dyn", [False, True], ids=["static", "dyn"])
@pytest.mark.parametrize("x16", [True, False], ids=["x_bf16", "x_fp32"])
def test_forward_statistics_bf16_storage(Fq, T, k, s, dyn, x16):
    x, w, ia, ib = _fwd_inputs(Fq, T, k, dyn)
    fn = ops.dw_conv_dyn_stats if dyn else ops.dw_conv_stats
    tf = (ia.to(DEV), ib.to(DEV), ops.ACT_RELU) if x16 else None               # (x fp32: the block without expand conv)
    xd = x.to(DEV).to(BF) if x16 else x.to(DEV)
    y16, parts = fn(xd, w.to(DEV), k, s, tf=tf, out_b16=True)
    y32, _ = fn(xd.float(), w.to(DEV), k, s, tf=tf)
    if dyn:
        assert y16.dtype == BF
        D16._same_after_rounding(y16.cpu(), y32.cpu())
    else:
        S16._assert_is_rounding_of(y16, y32, "dw conv")
    st, yd = _stat_sums(parts), y16.double().cpu()                              # of the STORED values
    assert _rel(st[0], yd.sum((0, 2, 3))) < 1e-5 and _rel(st[1], (yd ** 2).sum((0, 2, 3))) < 1e-5


# ------------------------------------------------------------------ accepted calls: merged backward, static taps
def _bn_state(z64, gamma, beta):
    mean = z64.mean((0, 2, 3))
    invstd = (z64.var((0, 2, 3), unbiased=False) + 1e-3).rsqrt()
    a, b = gamma.double() * invstd, beta.double() - mean * gamma.double() * invstd
    return tuple(t.float().to(DEV) for t in (a, b, mean, invstd))


@pytest.mark.parametrize("Fq,T,k,s", GEOMS)
def test_backward_fp32_gscale_and_gadd_each_in_its_role(Fq, T, k, s):
    """eat_dw_conv_bwd_bn_g against fp64 autograd of act(BN_train(dwconv(act(a x + b)))) * gs + ga (the `se` variant of
    test_gpu_train_fuse.test_dw_conv_backward_with_its_batchnorm_backward_on_load); the result must be the one of
    (gscale, gadd) in this order - the reference of the swapped pair is far away."""
    act, p = ops.ACT_HSWISH, (k - 1) // 2
    x, w = _rand(B, C, Fq, T, seed=1, scale=2.5), _rand(C, 1, k, k, seed=2, scale=0.3)
    ia, ib = _uni(C, seed=5), _rand(C, seed=6, scale=0.3)
    gamma, beta = _uni(C, seed=7), _rand(C, seed=8, scale=0.3)
    gs, ga = _uni(B, C, seed=9, lo=0.2), _rand(B, C, seed=10, scale=0.05)

    def reference(gs_, ga_, dy_):
        xr, wr = x.double().requires_grad_(True), w.double().requires_grad_(True)
        z = F.conv2d(ACTS[act](xr * ia.double()[None, :, None, None] + ib.double()[None, :, None, None]), wr, None, s, p, 1, C)
        u = F.batch_norm(z, None, None, gamma.double(), beta.double(), True, 0.01, 1e-3)
        (ACTS[act](u) * (dy_.double() * gs_.double()[:, :, None, None] + ga_.double()[:, :, None, None])).sum().backward()
        return z.detach(), u.detach(), xr.grad / ia.double()[None, :, None, None], wr.grad.reshape(C, k * k)

    dy = _rand(B, C, _out(Fq, k, s), _out(T, k, s), seed=3)
    z_ref, u_ref, _, _ = reference(gs, ga, dy)
    dy = dy * (~((u_ref.abs() - 3.0).abs() < 2e-3)).float()                     # away from the kinks of the activation
    _, _, g_ref, dw_ref = reference(gs, ga, dy)
    _, _, g_swapped, _ = reference(ga, gs, dy)
    st = _bn_state(z_ref, gamma, beta)
    zd, dyd = z_ref.float().to(DEV), dy.to(DEV)
    sums, _, _ = ops.bn_act_bwd_sums(dyd, zd, *st, act, gscale=gs.to(DEV), gadd=ga.to(DEV))
    g, gparts, dw = ops.dw_conv_bwd_bn_g(dyd, zd, st, act, sums, w.reshape(C, k * k).contiguous().to(DEV), x.to(DEV), ia.to(DEV),
                                         ib.to(DEV), act, k, s, gscale=gs.to(DEV), gadd=ga.to(DEV))
    assert _rel(g, g_ref) < 1e-5, _rel(g, g_ref)
    assert _rel(g, g_swapped) > 0.1
    assert _rel(dw, dw_ref) < 5e-5, _rel(dw, dw_ref)
    gpart, outer, inner = gparts
    sums_g, ref_s = gpart[:B * C * inner].view(B, C, inner).sum(2).cpu().double(), g_ref.sum((2, 3))
    assert float((sums_g - ref_s).abs().max()) < 2e-4 * max(1.0, float(ref_s.abs().max()))


@pytest.mark.parametrize("Fq,T,k,s", GEOMS)
@pytest.mark.parametrize("x16", [True, False], ids=["x_bf16", "x_fp32"])
def test_backward_bf16_storage_gscale_and_gadd_each_in_its_role(Fq, T, k, s, x16):
    """eat_dw_conv_bwd_bn_g_b16 against its fp32 twin on the same rounded tensors (the `se` / `first_block` variants of
    test_gpu_bf16_store.test_dw_conv_backward_bf16_storage); the twin with (gscale, gadd) swapped is far away."""
    act = ops.ACT_HSWISH
    Fo, To = _out(Fq, k, s), _out(T, k, s)
    x = _rand(B, C, Fq, T, seed=1, scale=2.5).to(DEV).to(BF)
    if not x16:
        x = x.float() + 2.0 ** -12 * _rand(B, C, Fq, T, seed=21).to(DEV)        # an fp32 tensor that is not bf16-representable
    z16 = (_rand(B, C, Fo, To, seed=2, scale=1.5) + _rand(1, C, 1, 1, seed=3)).to(DEV).to(BF)
    dy16 = _rand(B, C, Fo, To, seed=4).to(DEV).to(BF)
    ia, ib, w = _uni(C, seed=5).to(DEV), _rand(C, seed=6, scale=0.3).to(DEV), _rand(C, k * k, seed=7, scale=0.3).to(DEV)
    st = (_uni(C, seed=8).to(DEV), _rand(C, seed=9, scale=0.3).to(DEV), _rand(C, seed=10, scale=0.2).to(DEV), _uni(C, seed=11).to(DEV))
    gs, ga = _uni(B, C, seed=12, lo=0.2).to(DEV), _rand(B, C, seed=13, scale=0.05).to(DEV)
    sums, _, _ = ops.bn_act_bwd_sums(dy16, z16, *st, act, gscale=gs, gadd=ga)
    g16, gp16, dw16 = ops.dw_conv_bwd_bn_g(dy16, z16, st, act, sums, w, x, ia, ib, act, k, s, gscale=gs, gadd=ga)
    g32, _, dw32 = ops.dw_conv_bwd_bn_g(dy16.float(), z16.float(), st, act, sums, w, x.float(), ia, ib, act, k, s, gscale=gs, gadd=ga)
    g_swapped, _, _ = ops.dw_conv_bwd_bn_g(dy16.float(), z16.float(), st, act, sums, w, x.float(), ia, ib, act, k, s, gscale=ga, gadd=gs)
    if x16:
        S16._assert_is_rounding_of(g16, g32, "merged dw backward g")
    else:
        assert g16.dtype == torch.float32 and _rel(g16, g32) < 2e-6, _rel(g16, g32)
    assert _rel(g16, g_swapped) > 0.1
    assert _rel(dw16, dw32) < 2e-5, _rel(dw16, dw32)
    gpart, outer, inner = gp16
    sums_g, ref_s = gpart[:B * C * inner].view(B, C, inner).double().sum(2).cpu(), g16.double().sum((2, 3)).cpu()
    assert float((sums_g - ref_s).abs().max()) < 2e-4 * max(1.0, float(ref_s.abs().max()))


# ------------------------------------------------------------------ accepted calls: merged backward, per-plane taps
def _plane_sums(p, inner):
    return p[:B * C * inner].view(B, C, inner).double().sum(2).cpu()


@pytest.mark.parametrize("Fq,T,k,s", GEOMS)
def test_dyn_backward_fp32_res_and_both_partials_each_in_its_role(Fq, T, k, s):
    """eat_dw_conv_dyn_bwd_bn_g with res AND gpart AND gzpart against fp64 autograd of BN_batch(conv_bc(x)) (the block without
    expand conv of test_gpu_dymn.test_dynamic_depthwise_train_kernels): res is added to g only, after the sums; gpart holds
    the plane sums of dx, gzpart those of dx * x."""
    x, taps = _rand(B, C, Fq, T, seed=1), _rand(B, C * k * k, seed=2, scale=0.3)
    gam, res = _rand(C, seed=5).abs() + 0.5, _rand(B, C, Fq, T, seed=8)
    xr = x.double().requires_grad_(True)
    zd = _conv64(xr, taps, k, s, True)
    mu, var = zd.mean((0, 2, 3)), zd.var((0, 2, 3), unbiased=False)
    dv = _rand(*zd.shape, seed=7)
    ((zd - mu.view(1, C, 1, 1)) * (gam.double() / torch.sqrt(var + 1e-3)).view(1, C, 1, 1)).backward(dv.double())
    dx_ref = xr.grad
    z_dev, parts = ops.dw_conv_dyn_stats(x.to(DEV), taps.to(DEV), k, s)
    bn = torch.nn.BatchNorm2d(C, eps=1e-3, momentum=0.01).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(gam)
    st = ops.bn_state_from_partials(parts, bn, zd.numel() // C)
    xhat = ((zd - mu.view(1, C, 1, 1)) / torch.sqrt(var + 1e-3).view(1, C, 1, 1)).detach()
    sums = torch.cat([dv.double().sum((0, 2, 3)), (dv.double() * xhat).sum((0, 2, 3))]).to(DEV)
    one, zero = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    g, dw, (gpart, gzpart, inner) = ops.dw_conv_dyn_bwd_bn_g(dv.to(DEV), z_dev, st, ops.ACT_NONE, sums, taps.to(DEV), x.to(DEV), one,
                                                             zero, ops.ACT_NONE, k, s, res=res.to(DEV))
    assert _rel(g, dx_ref + res.double()) < 3e-5
    assert _rel(g, dx_ref) > 0.1                                                 # (res is of the size of dx: it did arrive)
    ref_g, ref_gz = dx_ref.sum((2, 3)), (dx_ref * x.double()).sum((2, 3))
    got_g, got_gz = _plane_sums(gpart, inner), _plane_sums(gzpart, inner)
    assert float((got_g - ref_g).abs().max()) < 2e-4 * max(1.0, float(ref_g.abs().max()))
    assert float((got_gz - ref_gz).abs().max()) < 2e-4 * max(1.0, float(ref_gz.abs().max()))
    assert _rel(got_g, ref_gz) > 0.1 and _rel(got_gz, ref_g) > 0.1


# (x bf16: every geometry; x fp32 - the block without expand conv, with its skip gradient - has the 3x3 / stride-1 tile instance)
@pytest.mark.parametrize("Fq,T,k,s,x16", [g + (True,) for g in GEOMS] + [(16, 130, 3, 1, False)])
def test_dyn_backward_bf16_storage_res_and_both_partials_each_in_its_role(Fq, T, k, s, x16):
    """eat_dw_conv_dyn_bwd_bn_g_b16 against its fp32 twin on the same bf16-representable tensors
    (test_gpu_dymn_bf16.test_dynamic_depthwise_train_kernels_b16)."""
    act = ops.ACT_HSWISH
    x = D16._r16(_rand(B, C, Fq, T, seed=1))
    taps = _rand(B, C * k * k, seed=2, scale=0.3).to(DEV)
    tf = (_uni(C, seed=3).to(DEV), _rand(C, seed=4, scale=0.2).to(DEV), act) if x16 else None
    xd32 = x.to(DEV)
    xd = xd32.to(BF) if x16 else xd32
    z = ops.dw_conv_dyn_stats(xd32, taps, k, s, tf=tf)[0].to(BF)                  # (the bf16 forward covers fewer geometries)
    zf = z.float()
    mean, invstd = zf.mean(dim=(0, 2, 3)), torch.rsqrt(zf.var(dim=(0, 2, 3), unbiased=False) + 1e-3)
    gam = _uni(C, seed=6).to(DEV)
    st = ((gam * invstd).contiguous(), (0.1 - mean * gam * invstd).contiguous(), mean.contiguous(), invstd.contiguous())
    dv = D16._r16(_rand(*z.shape, seed=5)).to(DEV)
    xhat = (zf - mean[None, :, None, None]) * invstd[None, :, None, None]
    sums = torch.cat([dv.double().sum(dim=(0, 2, 3)), (dv.double() * xhat.double()).sum(dim=(0, 2, 3))]).contiguous()
    one, zero = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    ia, ib, iact = (tf[0], tf[1], act) if x16 else (one, zero, ops.ACT_NONE)
    res = None if x16 else _rand(B, C, Fq, T, seed=8).to(DEV)
    g32, dw32, _ = ops.dw_conv_dyn_bwd_bn_g(dv, zf.contiguous(), st, ops.ACT_NONE, sums, taps, xd32, ia, ib, iact, k, s, res=res)
    g16, dw16, p16 = ops.dw_conv_dyn_bwd_bn_g(dv.to(BF), z, st, ops.ACT_NONE, sums, taps, xd, ia, ib, iact, k, s, res=res)
    assert g16.dtype == (BF if x16 else torch.float32)
    if x16:
        D16._same_after_rounding(g16.cpu(), g32.cpu())
    else:
        assert _rel(g16, g32) < 1e-6
    assert _rel(dw16, dw32) < 1e-5
    gs = g16.double() if x16 else g16.double() - res.double()                   # of g as stored, before the skip gradient
    s0, s1 = _plane_sums(p16[0], p16[2]).sum(0), _plane_sums(p16[1], p16[2]).sum(0)
    ref0, ref1 = gs.sum(dim=(0, 2, 3)).cpu(), (gs * xd32.double()).sum(dim=(0, 2, 3)).cpu()
    assert _rel(s0, ref0) < 1e-4 and _rel(s1, ref1) < 1e-4
    assert _rel(s0, ref1) > 0.1 and _rel(s1, ref0) > 0.1
    if res is not None:
        assert _rel(g16, g32 - res) > 0.1
