"""The generic dilated depthwise kernels (csrc/conv_spatial.hip: eat_dw_conv_dilated_fwd / _dgrad / _wgrad) and their
callers in ops.py against torch on the CPU in float64, at the shapes where their launch and index arithmetic can go wrong:
pad >= F, every k and dilation, stride 2 over odd and even extents, planes of less than a wave / exactly one block / one
block + 1 / more than the 32-block grid-stride loop covers in one pass, and B * C beyond the 65535 planes of one launch
(static form and per-sample-taps form, whose batch ranges come from ops._plane_chunks).

Bars: forward and dx max-abs <= 2e-6 of the reference's max-abs and pool sums 2e-5 (the bars of test_dw_conv); weight
gradients and G rel-L2 <= 2e-5, forward and dx also rel-L2 <= 1e-5 (the bars of the dilated test this module replaces).
Sums much longer than those (LONG_SUMS) are held to 3x the error of the same op evaluated in fp32 by torch on the CPU, with
the small-sum bar as a floor (the form of test_mel_matches_oracle)."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, ops  # noqa: E402
from efficientat_amd.dymn_train import DwConv, DynDwConv  # noqa: E402

DEV = torch.device("cuda:0")

CROSSING = (70, 960, 2, 3, 5, 1, 2)     # 67200 planes of 6 elements: two batch ranges, [0, 68) and [68, 70)
BIG_PLANE = (2, 3, 9, 1000, 5, 1, 2)    # 9000 elements: the 32 x 256 grid-stride loop wraps, ragged second pass
# (B, C, F, T, k, stride, dilation)
CASES = [
    # pad >= F: only some tap rows ever land inside (40-mel tails have F = 3)
    (2, 5, 3, 20, 5, 1, 2), (1, 3, 1, 9, 5, 1, 2), (2, 4, 2, 7, 7, 1, 3),
    # k of 1, 3, 5, 7; dilation of 1, 2, 3, 4
    (2, 6, 9, 20, 1, 1, 2), (2, 6, 9, 20, 3, 1, 4), (1, 4, 12, 33, 7, 1, 2), (2, 6, 9, 20, 5, 1, 1),
    # stride 2 with dilation, odd and even extents
    (2, 8, 12, 33, 3, 2, 2), (2, 8, 11, 32, 5, 2, 2), (1, 3, 7, 8, 5, 2, 3),
    # Fo * To below one wave, exactly 256, 257
    (3, 5, 2, 5, 3, 1, 2), (1, 3, 8, 32, 5, 1, 2), (1, 3, 1, 257, 3, 1, 2),
    BIG_PLANE,
    # the real tail geometry
    (3, 24, 8, 63, 5, 1, 2),
    # the shapes of the former test_gpu_train.py::test_dilated_depthwise_conv_gradients ((2, 8, 12, 33, 3, 2, 2) is above)
    (2, 24, 8, 31, 5, 1, 2), (3, 16, 9, 20, 3, 1, 2), (1, 12, 7, 15, 5, 1, 3),
    CROSSING,
]
# Sums much longer than the ~500-element ones the 2e-5 bars were set on.  Error of the same op in fp32 by torch on the CPU
# against fp64, as measured (the tests recompute it, it moves a little with the CPU's thread count):
#   BIG_PLANE  pool, 9000 elements per plane, max-abs over the largest |sum|: none 2.2e-7, relu 4.9e-8, hardswish 7.4e-8
#   BIG_PLANE  dw, 18000 elements per tap: rel-L2 6.2e-7;   G, 9000 elements per tap: rel-L2 5.7e-7
#   CROSSING   dw, 420 elements per tap over 70 samples: rel-L2 2.1e-7
# Each of these bars is 3 x that error + the small-sum bar: 2.07e-5 / 2.01e-5 / 2.02e-5 (pool), 2.19e-5 (dw), 2.17e-5 (G)
# and 2.06e-5 (dw of CROSSING).
LONG_SUMS = {"pool": (BIG_PLANE,), "dw": (BIG_PLANE, CROSSING), "G": (BIG_PLANE,)}
ACTS = [lambda t: t, F.relu, F.hardswish]


def _id(case):
    return "x".join(map(str, case))


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _maxabs_err(got, ref):
    return float((got.detach().cpu().double() - ref.double()).abs().max())


def _rel(got, ref):
    got = got.detach().cpu().double().reshape(-1)
    ref = ref.detach().double().reshape(-1)
    return float((got - ref).norm() / max(1e-30, float(ref.norm())))


def _close(got, ref, rel, what, extra=0.0):
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    scale = max(1e-6, float(ref.abs().max()))
    err = _maxabs_err(got, ref)
    assert err <= rel * scale + extra, f"{what}: max-abs err {err:.3e} vs scale {scale:.3e} (rel tol {rel}, + {extra:.3e})"


def _conv(x, w, s, k, dil, groups):
    return F.conv2d(x, w, None, s, (k - 1) // 2 * dil, dil, groups)


def _static(case, dtype):
    B, C, F_, T, k, s, dil = case
    x, w, b = _rand(B, C, F_, T, seed=1), _rand(C, 1, k, k, seed=2, scale=0.3), _rand(C, seed=3, scale=0.1)
    xr, wr = x.to(dtype).requires_grad_(True), w.to(dtype).requires_grad_(True)
    z = _conv(xr, wr, s, k, dil, C)
    dz = _rand(*z.shape, seed=4)
    z.backward(dz.to(dtype))
    pre = z.detach() + b.to(dtype).view(1, C, 1, 1)
    return dict(x=x, w=w, b=b, dz=dz, pre=pre, dx=xr.grad, dw=wr.grad.reshape(C, k * k))


def _dyn(case, dtype):
    """Per-sample taps: the B * C planes folded into the groups of one conv."""
    B, C, F_, T, k, s, dil = case
    x, taps = _rand(B, C, F_, T, seed=1), _rand(B, C * k * k, seed=2, scale=0.3)
    xr = x.to(dtype).reshape(1, B * C, F_, T).requires_grad_(True)
    tr = taps.to(dtype).reshape(B * C, 1, k, k).requires_grad_(True)
    z = _conv(xr, tr, s, k, dil, B * C)
    dz = _rand(B, C, *z.shape[2:], seed=4)
    z.backward(dz.to(dtype).reshape(z.shape))
    return dict(x=x, taps=taps, dz=dz, y=z.detach().reshape(dz.shape), dx=xr.grad.reshape(x.shape),
                G=tr.grad.reshape(B, C * k * k))


@functools.lru_cache(maxsize=None)
def _ref(case, form="static", dtype=torch.float64):
    """Inputs (fp32) and reference results of one case, computed once and shared by the tests (read-only)."""
    return (_static if form == "static" else _dyn)(case, dtype)


def _long_sum_extra(case, form, what, err_fn):
    """0 for an ordinary case; for a LONG_SUMS case 3 x the error of the fp32 torch-CPU evaluation against fp64."""
    if case not in LONG_SUMS[what]:
        return 0.0
    return 3.0 * err_fn(_ref(case, form, torch.float32)[what], _ref(case, form)[what])


def _tail_samples(case):
    """Samples whose planes lie around the boundary of the batch ranges (asserted on their own, not averaged away)."""
    return (67, 68, 69) if case == CROSSING else ()


# ------------------------------------------------------------------------------------------------ static taps
@pytest.mark.parametrize("act", [ops.ACT_NONE, ops.ACT_RELU, ops.ACT_HSWISH])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_dilated_forward_bias_act_pool(case, act):
    B, C, F_, T, k, s, dil = case
    r = _ref(case)
    ref = ACTS[act](r["pre"])
    ref_pool = ref.sum(dim=(2, 3))
    x, b = r["x"].to(DEV), r["b"].to(DEV)
    w2 = r["w"].reshape(C, k * k).contiguous().to(DEV)
    pool = torch.zeros(B, C, device=DEV)
    got = ops.dw_conv_dilated(x, w2, b, k, s, dil, act, pool)
    assert got.shape == ref.shape == (B, C, *ops.dilated_out(F_, T, k, s, dil))
    pool_extra = 0.0
    if case in LONG_SUMS["pool"]:
        pre32 = _ref(case, "static", torch.float32)["pre"]
        pool_extra = 3.0 * _maxabs_err(ACTS[act](pre32).sum(dim=(2, 3)), ref_pool)
    _close(got, ref, 2e-6, "forward")
    assert _rel(got, ref) < 1e-5
    _close(pool, ref_pool, 2e-5, "pool", pool_extra)
    for i in _tail_samples(case):
        _close(got[i], ref[i], 2e-6, f"forward, sample {i}")
        _close(pool[i], ref_pool[i], 2e-5, f"pool, sample {i}")
    _close(ops.dw_conv_dilated(x, w2, b, k, s, dil, act, None), ref, 2e-6, "forward without pool")
    if dil == 1:
        # the same operation as ops.dw_conv: one reference (padding (k-1)//2, no dilation) serves both
        plain = ACTS[act](F.conv2d(r["x"].double(), r["w"].double(), r["b"].double(), s, (k - 1) // 2, 1, C))
        _close(got, plain, 2e-6, "forward vs the undilated reference")
        _close(ops.dw_conv(x, w2, b, k, s, act), plain, 2e-6, "dw_conv vs the undilated reference")


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_dilated_data_and_weight_gradient(case):
    B, C, F_, T, k, s, dil = case
    r = _ref(case)
    dz = r["dz"].to(DEV)
    w2 = r["w"].reshape(C, k * k).contiguous().to(DEV)
    dx = ops.dw_conv_dilated_dgrad(dz, w2, (B, C, F_, T), k, s, dil)
    _close(dx, r["dx"], 2e-6, "dx")
    assert _rel(dx, r["dx"]) < 1e-5
    for i in _tail_samples(case):
        _close(dx[i], r["dx"][i], 2e-6, f"dx, sample {i}")
    dw = ops.dw_conv_dilated_wgrad(dz, r["x"].to(DEV), k, s, dil)
    assert dw.shape == (C, k * k)
    assert _rel(dw, r["dw"]) <= 2e-5 + _long_sum_extra(case, "static", "dw", _rel)


# ------------------------------------------------------------------------------------------------ per-sample taps
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_dilated_per_sample_taps_forward_backward(case):
    B, C, F_, T, k, s, dil = case
    r = _ref(case, "dyn")
    x, taps, dz = r["x"].to(DEV), r["taps"].to(DEV), r["dz"].to(DEV)
    y = ops.dw_conv_dyn_dilated(x, taps, k, s, dil)
    _close(y, r["y"], 2e-6, "forward")
    assert _rel(y, r["y"]) < 1e-5
    dx, G = ops.dw_conv_dyn_dilated_bwd(dz, x, taps, k, s, dil)
    _close(dx, r["dx"], 2e-6, "dx")
    assert _rel(dx, r["dx"]) < 1e-5
    assert G.shape == (B, C * k * k)
    assert _rel(G, r["G"]) <= 2e-5 + _long_sum_extra(case, "dyn", "G", _rel)
    for i in _tail_samples(case):
        _close(y[i], r["y"][i], 2e-6, f"forward, sample {i}")
        _close(dx[i], r["dx"][i], 2e-6, f"dx, sample {i}")
        assert _rel(G[i], r["G"][i]) <= 2e-5, f"G, sample {i}"


# ------------------------------------------------------------------------------------------------ autograd Functions
FN_CASES = [(2, 5, 3, 20, 5, 1, 2), (2, 8, 12, 33, 3, 2, 2), (3, 24, 8, 63, 5, 1, 2),      # dilation 2
            (2, 4, 2, 7, 7, 1, 3), (1, 3, 7, 8, 5, 2, 3), (1, 12, 7, 15, 5, 1, 3)]         # dilation 3


@pytest.mark.parametrize("case", FN_CASES, ids=_id)
def test_dwconv_function_dilated(case):
    B, C, F_, T, k, s, dil = case
    r = _ref(case)
    xd, wd = (r[n].to(DEV).requires_grad_(True) for n in ("x", "w"))
    out = DwConv.apply(xd, wd, k, s, dil)
    out.backward(r["dz"].to(DEV))
    ref = r["pre"] - r["b"].double().view(1, C, 1, 1)          # the Function has no bias
    _close(out, ref, 2e-6, "forward")
    _close(xd.grad, r["dx"], 2e-6, "dx")
    assert wd.grad.shape == wd.shape and _rel(wd.grad, r["dw"]) <= 2e-5


@pytest.mark.parametrize("case", FN_CASES, ids=_id)
def test_dyndwconv_function_dilated(case):
    B, C, F_, T, k, s, dil = case
    K = 4
    x, bank = _rand(B, C, F_, T, seed=1), _rand(1, 1, K, C * k * k, seed=2, scale=0.3)
    att = torch.softmax(_rand(B, K, seed=3), dim=-1)
    xr, wr, ar = (t.double().requires_grad_(True) for t in (x, bank, att))
    y = _conv(xr.reshape(1, B * C, F_, T), (ar @ wr[0, 0]).reshape(B * C, 1, k, k), s, k, dil, B * C)
    y = y.reshape(B, C, *y.shape[2:])
    dz = _rand(*y.shape, seed=4)
    y.backward(dz.double())
    xd, wd, ad = (t.to(DEV).requires_grad_(True) for t in (x, bank, att))
    out = DynDwConv.apply(xd, wd, ad, k, s, dil)
    out.backward(dz.to(DEV))
    _close(out, y.detach(), 2e-6, "forward")
    _close(xd.grad, xr.grad, 2e-6, "dx")
    assert wd.grad.shape == wd.shape and ad.grad.shape == ad.shape
    assert _rel(wd.grad, wr.grad) <= 2e-5 and _rel(ad.grad, ar.grad) <= 2e-5


# ------------------------------------------------------------------------------------------------ refusals
def test_more_channels_than_one_launch_holds_is_refused():
    C = 65536
    x, w, b = torch.zeros(1, C, 1, 1, device=DEV), torch.zeros(C, 9, device=DEV), torch.zeros(C, device=DEV)
    with pytest.raises(_lib.EatHipError, match="channels"):
        ops.dw_conv_dilated(x, w, b, 3, 1, 2, ops.ACT_NONE)
    with pytest.raises(_lib.EatHipError, match="channels"):
        ops.dw_conv_dilated_dgrad(x, w, (1, C, 1, 1), 3, 1, 2)
    with pytest.raises(_lib.EatHipError, match="channels"):
        ops.dw_conv_dilated_wgrad(x, x, 3, 1, 2)
    with pytest.raises(_lib.EatHipError, match="channels"):
        ops.dw_conv_dyn_dilated(x, w.view(1, C * 9), 3, 1, 2)
    with pytest.raises(_lib.EatHipError, match="channels"):
        ops.dw_conv_dyn_dilated_bwd(x, x, w.view(1, C * 9), 3, 1, 2)
