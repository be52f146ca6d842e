"""GPU tests of the depthwise training kernels at the shapes where the BATCH picks the work decomposition: the loop of a wave
over G sample groups, its ragged tail, the lane groups without a sample in a group that is not the first
(csrc/dw_plane.hip: dw_bwd_tile_kernel, dw_tile_wgrad_kernel, dw_plane_wgrad_kernel), the second and later batch slices of
the column-walking weight gradient and the row chunks of the stem's (csrc/dw_grad.hip).  The cases and the branch each one
claims are in tests/dw_split_cases.py; every case first asserts its branch through the library's own split
(eat_dw_bwd_split / eat_dw_wgrad_split, which the launchers call) and then compares with fp64 on the CPU, built as the
existing test of the same entry point builds it, under that test's tolerances:
  merged backward with BatchNorm on load   test_gpu_train_fuse.test_dw_conv_backward_with_its_batchnorm_backward_on_load
  merged backward without BatchNorm        test_gpu_train_fuse.test_dw_conv_backward_merged_kernel
  per-sample taps, fp32 and bf16 storage   test_gpu_dw_entry_points.test_dyn_backward_* (g), test_gpu_dymn (the tap gradient)
  stand-alone weight gradients, stem       test_gpu_train.test_dw_conv_gradients / test_dw_conv_with_input_transform /
                                           test_stem_weight_gradient
No case reduces over more terms per channel (B * Fo * To <= 8864) than the cases those tolerances were set on (64 000).
Every case prints its measured errors."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, ops  # noqa: E402
from tests import dw_split_cases as K  # noqa: E402
from tests import test_gpu_dymn_bf16 as D16  # noqa: E402

DEV = torch.device("cuda:0")
BF = torch.bfloat16
ACTS = [lambda t: t, F.relu, F.hardswish]


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _uni(*shape, seed, lo=0.5):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) + lo


def _rel(got, ref):
    got = got.detach().cpu().double().reshape(-1)
    ref = ref.detach().cpu().double().reshape(-1)
    return float((got - ref).norm() / max(1e-30, float(ref.norm())))


def _sum_err(part, B, C, inner, ref_s):
    """Largest error of the plane sums of a partials buffer [B][C][inner], relative to max(1, largest reference sum)."""
    sums = part[:B * C * inner].view(B, C, inner).double().sum(2).cpu()
    return float((sums - ref_s).abs().max()) / max(1.0, float(ref_s.abs().max()))


def _report(what, shape, **errs):
    print(f"[dw-batch-splits] {what} {K.case_id(shape)}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))


# ------------------------------------------------------------------ merged backward with BatchNorm on load
@functools.lru_cache(maxsize=1)
def _bn_forward(shape, act, train, expand):
    """The fp64 graph of act(BN(dwconv(act_in(a x + b)))) for one row: shared by the variants that differ in the incoming
    gradient only (`plain`, `se`)."""
    B, C, F_, T, k, s = shape
    p = (k - 1) // 2
    x = _rand(B, C, F_, T, seed=1, scale=2.5)
    ia, ib = torch.rand(C, generator=torch.Generator().manual_seed(5)) + 0.5, _rand(C, seed=6, scale=0.3)
    in_act = act
    if not expand:
        ia, ib, in_act = torch.ones(C), torch.zeros(C), 0
    w = _rand(C, 1, k, k, seed=2, scale=0.3)
    gamma, beta = torch.rand(C, generator=torch.Generator().manual_seed(7)) + 0.5, _rand(C, seed=8, scale=0.3)
    xr = x.double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y_in = ACTS[in_act](xr * ia.double()[None, :, None, None] + ib.double()[None, :, None, None])
    z_ref = F.conv2d(y_in, wr, None, s, p, 1, C)
    rm, rv = torch.zeros(C).double() + 0.1, torch.ones(C).double() * 1.3
    u_ref = F.batch_norm(z_ref, rm.clone(), rv.clone(), gr, br, train, 0.01, 1e-3)
    dy = _rand(*z_ref.shape, seed=3)
    near = (u_ref.detach().abs() < 2e-3) if act == 1 else ((u_ref.detach().abs() - 3.0).abs() < 2e-3)
    dy = dy * (~near).float()
    return dict(x=x, ia=ia, ib=ib, in_act=in_act, w=w, gamma=gamma, beta=beta, xr=xr, wr=wr, gr=gr, br=br, z_ref=z_ref, rm=rm, rv=rv,
                out=ACTS[act](u_ref), dy=dy)


BN_CASES = ([(row, v) for row in K.BN_ROWS for v in ("plain", "se")]
            + [(row, v) for row in K.BN_ROWS_ALL_VARIANTS for v in ("frozen", "no_expand")])


@pytest.mark.parametrize("row,variant", BN_CASES, ids=[f"{K.case_id(r[0])}-{v}" for r, v in BN_CASES])
def test_merged_backward_with_batchnorm_on_load(row, variant):
    """eat_dw_conv_bwd_bn_g where a wave walks G > 1 sample groups and the batch is no multiple of what a wave walks."""
    shape, act, claim = row
    B, C, F_, T, k, s = shape
    split = K.bwd_split(shape, True)
    assert split == claim and split["G"] > 1 and K.ragged_bwd(shape, split)
    train = variant != "frozen"
    f = _bn_forward(shape, act, train, variant != "no_expand")
    gs = ga = None
    if variant == "se":
        gs = torch.rand(B, C, generator=torch.Generator().manual_seed(9)) + 0.2
        ga = _rand(B, C, seed=10, scale=0.05)
        d_eff = f["dy"].double() * gs.double()[:, :, None, None] + ga.double()[:, :, None, None]
    else:
        d_eff = f["dy"].double()
    x_grad, w_grad, gam_grad, bet_grad = torch.autograd.grad((f["out"] * d_eff).sum(), [f["xr"], f["wr"], f["gr"], f["br"]],
                                                             retain_graph=True)

    # forward state on the device (the statistics kernels have their own tests)
    z_ref = f["z_ref"].detach()
    zd = z_ref.float().to(DEV)
    if train:
        mean = z_ref.mean((0, 2, 3))
        invstd = (z_ref.var((0, 2, 3), unbiased=False) + 1e-3).rsqrt()
    else:
        mean, invstd = f["rm"], (f["rv"] + 1e-3).rsqrt()
    a = (f["gamma"].double() * invstd).float().to(DEV)
    b = (f["beta"].double() - mean * f["gamma"].double() * invstd).float().to(DEV)
    mean_d, invstd_d = mean.float().to(DEV), invstd.float().to(DEV)
    if not train:
        mean_d._eat_frozen = True
    st = (a, b, mean_d, invstd_d)
    dyd = f["dy"].to(DEV)
    gsd, gad = (None, None) if gs is None else (gs.to(DEV), ga.to(DEV))
    sums, dgam, dbet = ops.bn_act_bwd_sums(dyd, zd, *st, act, gscale=gsd, gadd=gad)
    g, gparts, dw = ops.dw_conv_bwd_bn_g(dyd, zd, st, act, sums, f["w"].reshape(C, k * k).contiguous().to(DEV), f["x"].to(DEV),
                                         f["ia"].to(DEV), f["ib"].to(DEV), f["in_act"], k, s, gscale=gsd, gadd=gad,
                                         want_gsum=variant != "no_expand")
    g_ref = x_grad / f["ia"].double()[None, :, None, None]                   # gradient w.r.t. u = a x + b
    errs = dict(g=_rel(g, g_ref), dw=_rel(dw, w_grad.reshape(C, k * k)), dgamma=_rel(dgam, gam_grad), dbeta=_rel(dbet, bet_grad))
    if gparts is not None:
        gpart, outer, inner = gparts
        assert inner == split["inner"]
        errs["sums"] = _sum_err(gpart, B, C, inner, g_ref.sum((2, 3)))
    _report(f"bwd_bn_g {variant} G={split['G']} lanes={split['lane_group']}", shape, **errs)
    assert errs["dgamma"] < 2e-5 and errs["dbeta"] < 2e-5
    assert errs["g"] < 1e-5
    assert errs["dw"] < 5e-5
    assert errs.get("sums", 0.0) < 2e-4


# ------------------------------------------------------------------ merged backward without BatchNorm
@pytest.mark.parametrize("row", K.PLAIN_ROWS, ids=lambda r: K.case_id(r[0]))
def test_merged_backward_without_batchnorm(row):
    """eat_dw_conv_bwd_g (planes of more than 128 columns: strips) with G = 2, 4, 8 and a ragged last wave."""
    shape, act, claim = row
    B, C, F_, T, k, s = shape
    split = K.bwd_split(shape, False)
    assert split == claim and split["G"] > 1 and K.ragged_bwd(shape, split)
    p = (k - 1) // 2
    Fo, To = K.out(F_, k, s), K.out(T, k, s)
    x = _rand(B, C, F_, T, seed=1, scale=2.5)                              # pre-BN expand output (spans the kinks)
    ia, ib = torch.rand(C, generator=torch.Generator().manual_seed(5)) + 0.5, _rand(C, seed=6, scale=0.3)
    w = _rand(C, 1, k, k, seed=2, scale=0.3)
    dz = _rand(B, C, Fo, To, seed=3)
    u = (x.double() * ia.double()[None, :, None, None] + ib.double()[None, :, None, None]).requires_grad_(True)
    wr = w.double().requires_grad_(True)
    F.conv2d(ACTS[act](u), wr, None, s, p, 1, C).backward(dz.double())
    g_ref = u.grad                                                          # = dgrad(dz) * act'(u)
    g, (gpart, outer, inner), dw = ops.dw_conv_bwd_g(dz.to(DEV), w.reshape(C, k * k).contiguous().to(DEV), x.to(DEV),
                                                     ia.to(DEV), ib.to(DEV), act, k, s)
    assert inner == split["inner"]
    errs = dict(g=_rel(g, g_ref), dw=_rel(dw, wr.grad.reshape(C, k * k)), sums=_sum_err(gpart, B, C, inner, g_ref.sum((2, 3))))
    _report(f"bwd_g G={split['G']}", shape, **errs)
    assert errs["g"] < 3e-6
    assert errs["dw"] < 2e-5
    assert errs["sums"] < 1e-4


# ------------------------------------------------------------------ merged backward, per-sample taps
def _conv_bc(xin, taps, k, s):
    B, C = xin.shape[0], xin.shape[1]
    y = F.conv2d(xin.reshape(1, B * C, *xin.shape[2:]), taps.reshape(B * C, 1, k, k), None, s, (k - 1) // 2, 1, B * C)
    return y.reshape(B, C, *y.shape[2:])


def _dyn_bwd(dy, z, st, sums, taps, x, in_a, in_b, in_act, k, s, res, dw):
    """ops.dw_conv_dyn_bwd_bn_g (fp32 storage) into the caller's tap-gradient buffer `dw` (B, C*k*k)."""
    B, C, Fq, T = x.shape
    Fo, To = z.shape[2], z.shape[3]
    cap = int(_lib.lib().eat_dw_bwd_partials_inner(Fq, T, Fo, To, k, s))
    g = torch.empty((B, C, Fq, T), device=DEV, dtype=torch.float32)
    parts = torch.empty((2, B * C * cap), device=DEV, dtype=torch.float32)
    inner = ctypes.c_int(0)
    _lib.call("eat_dw_conv_dyn_bwd_bn_g", dy.data_ptr(), z.data_ptr(), st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(),
              st[3].data_ptr(), sums.data_ptr(), ops.ACT_NONE, 0, x.data_ptr(), in_a.data_ptr(), in_b.data_ptr(), in_act,
              taps.data_ptr(), None if res is None else res.data_ptr(), g.data_ptr(), dw.data_ptr(), parts[0].data_ptr(),
              parts[1].data_ptr(), cap, ctypes.addressof(inner), B, C, Fq, T, Fo, To, k, s, torch.cuda.current_stream().cuda_stream)
    return g, parts[0], parts[1], inner.value


@pytest.mark.parametrize("row", K.DYN_ROWS, ids=lambda r: K.case_id(r[0]))
def test_merged_backward_per_sample_taps(row):
    """eat_dw_conv_dyn_bwd_bn_g with res, gpart and gzpart against fp64 autograd of BN_batch(conv_bc(x)) (the block without
    expand conv).  A plane of one tile has its tap gradient STORED: the buffer starts NaN-filled (a lane group without a sample
    must not write, every plane must be written) and a second call gives the same bits; planes of several tiles are added
    into a zeroed buffer."""
    shape, _, claim = row
    B, C, Fq, T, k, s = shape
    KK = k * k
    split = K.bwd_split(shape, True)
    assert split == claim and split["G"] > 1 and K.ragged_bwd(shape, split)
    x, taps = _rand(B, C, Fq, T, seed=1), _rand(B, C * KK, seed=2, scale=0.3)
    gam, res = _rand(C, seed=5).abs() + 0.5, _rand(B, C, Fq, T, seed=8)
    xr, tr = x.double().requires_grad_(True), taps.double().requires_grad_(True)
    zd = _conv_bc(xr, tr, k, s)
    mu, var = zd.mean((0, 2, 3)), zd.var((0, 2, 3), unbiased=False)
    dv = _rand(*zd.shape, seed=7)
    ((zd - mu.view(1, C, 1, 1)) * (gam.double() / torch.sqrt(var + 1e-3)).view(1, C, 1, 1)).backward(dv.double())
    dx_ref = xr.grad
    xd, tapd = x.to(DEV), taps.to(DEV)
    z_dev, parts = ops.dw_conv_dyn_stats(xd, tapd, k, s)
    bn = torch.nn.BatchNorm2d(C, eps=1e-3, momentum=0.01).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(gam)
    st = ops.bn_state_from_partials(parts, bn, zd.numel() // C)
    xhat = ((zd - mu.view(1, C, 1, 1)) / torch.sqrt(var + 1e-3).view(1, C, 1, 1)).detach()
    sums = torch.cat([dv.double().sum((0, 2, 3)), (dv.double() * xhat).sum((0, 2, 3))]).to(DEV)
    one, zero = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    stores = split["inner"] == 1
    fill = float("nan") if stores else 0.0
    dvd, resd = dv.to(DEV), res.to(DEV)
    dw = torch.full((B, C * KK), fill, device=DEV)
    g, gpart, gzpart, inner = _dyn_bwd(dvd, z_dev, st, sums, tapd, xd, one, zero, ops.ACT_NONE, k, s, resd, dw)
    assert inner == split["inner"]
    assert bool(torch.isfinite(dw).all())
    ref_g, ref_gz = dx_ref.sum((2, 3)), (dx_ref * x.double()).sum((2, 3))
    errs = dict(g=_rel(g, dx_ref + res.double()), dw=_rel(dw, tr.grad), gpart=_sum_err(gpart, B, C, inner, ref_g),
                gzpart=_sum_err(gzpart, B, C, inner, ref_gz))
    _report(f"dyn_bwd_bn_g G={split['G']} lanes={split['lane_group']} {'stored' if stores else 'added'}", shape, **errs)
    assert errs["g"] < 3e-5
    assert _rel(g, dx_ref) > 0.1                                                 # (res is of the size of dx: it did arrive)
    assert errs["dw"] < 3e-5
    assert errs["gpart"] < 2e-4 and errs["gzpart"] < 2e-4
    if stores:
        dw2 = torch.full((B, C * KK), fill, device=DEV)
        g2, gpart2, gzpart2, _ = _dyn_bwd(dvd, z_dev, st, sums, tapd, xd, one, zero, ops.ACT_NONE, k, s, resd, dw2)
        assert torch.equal(dw2, dw) and torch.equal(g2, g)
        assert torch.equal(gpart2[:B * C * inner], gpart[:B * C * inner]) and torch.equal(gzpart2[:B * C * inner], gzpart[:B * C * inner])


# (x bf16: every row; x fp32 - the block without expand conv, with its skip gradient - has the 3x3 / stride-1 strip instance)
DYN16_CASES = [(row, True) for row in K.DYN_ROWS] + [(K.DYN_ROWS[1], False)]


@pytest.mark.parametrize("row,x16", DYN16_CASES, ids=[f"{K.case_id(r[0])}-{'x_bf16' if x else 'x_fp32'}" for r, x in DYN16_CASES])
def test_merged_backward_per_sample_taps_bf16_storage(row, x16):
    """eat_dw_conv_dyn_bwd_bn_g_b16 against its fp32 twin on the same bf16-representable tensors, where the bf16 entry points
    cover the geometry (eat_dw_conv_b16_ok); where they do not, that answer is the assertion."""
    shape, _, claim = row
    B, C, Fq, T, k, s = shape
    split = K.bwd_split(shape, True)
    assert split == claim and split["G"] > 1 and K.ragged_bwd(shape, split)
    covered = bool(_lib.lib().eat_dw_conv_b16_ok(*K.geom(shape)))
    assert covered == (shape in ((5, 1366, 2, 130, 3, 1), (17, 2731, 4, 8, 5, 1)))
    if not covered:
        return
    act = ops.ACT_HSWISH
    x = D16._r16(_rand(B, C, Fq, T, seed=1))
    taps = _rand(B, C * k * k, seed=2, scale=0.3).to(DEV)
    tf = (_uni(C, seed=3).to(DEV), _rand(C, seed=4, scale=0.2).to(DEV), act) if x16 else None
    xd32 = x.to(DEV)
    xd = xd32.to(BF) if x16 else xd32
    z = ops.dw_conv_dyn_stats(xd32, taps, k, s, tf=tf)[0].to(BF)
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
    gs = g16.double() if x16 else g16.double() - res.double()                   # of g as stored, before the skip gradient
    inner = p16[2]
    assert inner == split["inner"]
    s0 = p16[0][:B * C * inner].view(B, C, inner).double().sum(2).cpu().sum(0)
    s1 = p16[1][:B * C * inner].view(B, C, inner).double().sum(2).cpu().sum(0)
    ref0, ref1 = gs.sum(dim=(0, 2, 3)).cpu(), (gs * xd32.double()).sum(dim=(0, 2, 3)).cpu()
    errs = dict(g=_rel(g16, g32), dw=_rel(dw16, dw32), gpart=_rel(s0, ref0), gzpart=_rel(s1, ref1))
    _report(f"dyn_bwd_bn_g_b16 {'x_bf16' if x16 else 'x_fp32'} G={split['G']} lanes={split['lane_group']}", shape, **errs)
    if not x16:
        assert errs["g"] < 1e-6
        assert _rel(g16, g32 - res) > 0.1
    assert errs["dw"] < 1e-5
    assert errs["gpart"] < 1e-4 and errs["gzpart"] < 1e-4


# ------------------------------------------------------------------ stand-alone weight gradients
@pytest.mark.parametrize("row", K.WGRAD_ROWS, ids=lambda r: K.case_id(r[0]) + ("-tf" if r[1] else ""))
def test_weight_gradient_kernels(row):
    """eat_dw_conv_wgrad / eat_dw_conv_wgrad_tf on the tile kernel (G = 2, 4, 8), the five whole-plane instances (G >= 2, one and
    two planes per wave), and the column-walking kernel with two and three batch slices, the last one short."""
    shape, tf, claim = row
    B, C, F_, T, k, s = shape
    split = K.wgrad_split(shape)
    assert split == claim
    assert split["parts"] == 1 if shape in K.CONTROLS else (split["split"] > 1 and split["parts"] > 1 and K.ragged_wgrad(shape, split))
    x, w = _rand(B, C, F_, T, seed=1), _rand(C, 1, k, k, seed=2, scale=0.3).double().requires_grad_(True)
    xin = x.double()
    if tf:
        act = 2 if k == 5 else 1
        a, b = torch.rand(C, generator=torch.Generator().manual_seed(3)) + 0.5, _rand(C, seed=4, scale=0.5)
        xin = ACTS[act](x.double() * a.double().view(1, C, 1, 1) + b.double().view(1, C, 1, 1))
    y = F.conv2d(xin, w, None, s, (k - 1) // 2, 1, C)
    dz = _rand(*y.shape, seed=3)
    y.backward(dz.double())
    ref = w.grad.reshape(C, k * k)
    if tf:
        dw = ops.dw_conv_wgrad_tf(dz.to(DEV), x.to(DEV), a.to(DEV), b.to(DEV), act, k, s)
    else:
        dw = ops.dw_conv_wgrad(dz.to(DEV), x.to(DEV), k, s)
    errs = dict(dw=_rel(dw, ref), dw_max=float((dw.cpu().double() - ref).abs().max()) / float(ref.abs().max()))
    _report(f"wgrad{'_tf' if tf else ''} {split['kernel']} split={split['split']} parts={split['parts']}", shape, **errs)
    assert errs["dw"] < 2e-5
    if tf:                                                  # (test_dw_conv_with_input_transform's measure)
        assert errs["dw_max"] < 2e-5


@pytest.mark.parametrize("row", K.STEM_ROWS, ids=lambda r: "x".join(str(v) for v in r[0]))
def test_stem_weight_gradient_row_chunks(row):
    """The stem's weight gradient (one input channel) with 3 and 2 output rows per block, the last chunk one row."""
    (B, F_, T), claim = row
    split = K.stem_split(row[0])
    assert split == claim and split["split"] > 1 and K.out(F_, 3, 2) % split["split"] != 0
    x, w = _rand(B, 1, F_, T, seed=1), _rand(K.STEM_C, 1, 3, 3, seed=2).double().requires_grad_(True)
    y = F.conv2d(x.double(), w, None, 2, 1)
    dz = _rand(*y.shape, seed=3)
    y.backward(dz.double())
    err = _rel(ops.dw_conv_wgrad(dz.to(DEV), x.to(DEV), 3, 2), w.grad.reshape(K.STEM_C, 9))
    print(f"[dw-batch-splits] stem wgrad {B}x{F_}x{T} rows/block={split['split']} chunks={split['parts']}: dw {err:.2e}")
    assert err < 2e-5
