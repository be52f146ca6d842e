"""MN and DyMN at the other released widths (mn01 mn02 mn04 mn05 mn20 mn30, dymn04), against the float64 oracle.

Every other whole-network comparison builds width 1.0 / 4.0 (MN) or 1.0 / 2.0 (DyMN).  Width changes what the launch plans
decide: 8 / 32 / 48 stem channels (no fused front), blocks without expand conv beyond block 0 and a residual one on the separate
depthwise-backward passes (width 0.1), channel counts the MFMA tilings see nowhere else (8, 104, 136 = 8 x 17, 272, 336, 368,
2016, 2880 ...), SE squeeze widths from 8 to 720, DyMN context dimensions 16 / 24 / 48.  The cases, their cached oracle steps and
the tables of literals that pin each case's kernels are in tests/widths_case.py; what each width is, in tests/test_widths_cpu.py.
The reference is fp64 (autograd over) the oracle, which tests/test_oracle_golden.py pins on the unmodified reference at
these widths.  The oracle's own fp32 evaluation sits within: gradient rel-L2 median 3.6e-5, maximum 1.1e-3, logits 2.9e-5 of
its fp64 one on these inputs (16 CPU threads; with another summation order it, too, puts single activations on the other side
of a kink - see test_mn_train_step_at_released_widths_matches_fp64_oracle): at least 45x inside the bars."""
import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import eat_oracle as O
from tests import widths_case as W

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import mn as mn_mod  # noqa: E402
from efficientat_amd import ops  # noqa: E402
from efficientat_amd.dymn import get_model as get_dymn  # noqa: E402
from efficientat_amd.mn import get_model as get_mn  # noqa: E402
from tests.test_gpu_mn_geometry import _Calls, _is_project_bn_bias  # noqa: E402

DEV = torch.device("cuda:0")
B, N_BLOCKS = W.B, W.N_BLOCKS


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


class _WidthCalls(_Calls):
    """_Calls plus the columns the widths add: `separate` = blocks whose depthwise backward ran as separate passes (a block
    without expand conv: one eat_dw_conv_wgrad and one eat_dw_conv_dgrad), and the eval plan's counts."""

    def plan(self):
        n = self.n
        assert n["eat_dw_conv_wgrad"] == n["eat_dw_conv_dgrad"], dict(n)
        return dict(super().plan(), separate=n["eat_dw_conv_dgrad"])

    def eval_plan(self):
        n = self.n
        return dict(front=n["eat_front_fwd"], fused=n["eat_mbconv_fwd"] + n["eat_fused_expand_dw_fwd"],
                    expand_dw=n["eat_expand_dw_bf16_fwd"], dw=n["eat_dw_conv_fwd"])


def _check_plan(case, calls, want):
    """`want`: a row of W.PLAN_F32 / W.PLAN_B16 (forms it does not name: no call; the on-load weight gradients as the convs)."""
    full = dict(cat16=0, on_load16=0, merged16=0, stats16=0)
    full.update(want)
    full["on_load_wgrad"], full["on_load_wgrad16"] = full["on_load"], full["on_load16"]
    got = calls.plan()
    assert got == full, (case, got, full)
    # one depthwise forward per block; every block's depthwise backward on exactly one of the three forms
    assert calls.n["eat_dw_conv_fwd_stats"] + calls.n["eat_dw_conv_fwd_stats_b16"] == N_BLOCKS, (case, dict(calls.n))
    assert got["merged"] + got["merged16"] + got["separate"] == N_BLOCKS, (case, got)
    assert calls.n["eat_front_fwd"] == 0 and calls.n["eat_mbconv_fwd"] == 0 and calls.n["eat_fused_expand_dw_fwd"] == 0


# ------------------------------------------------------------------------------------------------------------ MN, eval
def _mn_model(width, geo, sd):
    m = _quiet(get_mn, width_mult=width, input_dim_t=W.GEOMETRIES[geo] // 320)
    m.load_state_dict(sd, strict=True)
    return m.to(DEV)


def _check_mn_eval(width, pw_mode, batch, monkeypatch):
    monkeypatch.setattr(mn_mod, "_PW_MODE", pw_mode)
    ftol = 1e-3 if pw_mode == "fp32" else 1e-2
    x, sd = W.mn_case(width, "3s")
    ref_logits, ref_fmaps = W.mn_eval_ref(width, "3s", batch)
    model = _mn_model(width, "3s", sd).eval()
    xd = x[:batch].to(DEV)
    plans = []
    with torch.no_grad():
        for kw in (dict(return_fmaps=True), {}):                     # with the feature maps, and as model(x) runs it
            with _WidthCalls() as calls:
                out = model._forward_impl(xd, **kw)
                torch.cuda.synchronize()
            plans.append((calls.eval_plan(), out))
    (_, (logits, fmaps)), (_, (logits2, _)) = plans
    want = dict(W.EVAL_PLAN[width], front=0)
    if pw_mode == "fp32":
        want["expand_dw"] = 0
    want["dw"] = N_BLOCKS - want["expand_dw"]                        # one depthwise forward per block
    for got, _ in plans:
        assert got == want, (width, pw_mode, got, want)
    assert len(fmaps) == len(ref_fmaps) == 17
    scale = max(1.0, float(ref_logits.abs().max()))
    el = max(float((l.cpu().double() - ref_logits).abs().max()) for l in (logits, logits2))
    worst = (0.0, None)
    for i, (a, b) in enumerate(zip(fmaps, ref_fmaps)):
        assert a.shape == b.shape, i
        e = float((a.cpu().double() - b).abs().max()) / max(1.0, float(b.std()))
        worst = max(worst, (e, i))
    print(f"eval mn width {width} B {batch} {pw_mode}: logits max abs {el:.2e} (|logits| <= {scale:.1f}), fmap max abs / max(1, std) "
          f"{worst[0]:.2e} (fmap {worst[1]}), plan {plans[0][0]}")
    assert el < 1e-3 * scale, (el, scale)
    assert worst[0] < ftol, worst


@pytest.mark.parametrize("pw_mode", ["fp32", "auto"])
@pytest.mark.parametrize("width", W.MN_WIDTHS)
def test_mn_eval_at_released_widths_matches_fp64_oracle(width, pw_mode, monkeypatch):
    """Logits and all 17 feature maps against the fp64 oracle, the bars of test_mn10_eval_logits_and_fmaps: logits 1e-3 x
    max(1, |logits|), feature maps max-abs below ftol x max(1, std) with ftol 1e-3 (fp32) / 1e-2 (auto); W.EVAL_PLAN pins the
    unfused front and blocks."""
    _check_mn_eval(width, pw_mode, B, monkeypatch)


@pytest.mark.parametrize("pw_mode", ["fp32", "auto"])
def test_mn01_eval_of_one_clip_matches_fp64_oracle(pw_mode, monkeypatch):
    """B = 1 at width 0.1: 8 channels x one sample - the smallest operands the 1x1 routes see."""
    _check_mn_eval(0.1, pw_mode, 1, monkeypatch)


# ---------------------------------------------------------------------------------------------------- MN, one train step
def _train_model(width, geo, sd, prec, storage="fp32"):
    m = _mn_model(width, geo, sd).train()
    m.train_precision, m.act_storage = prec, storage
    return m


def _hip_step(model, x, y, keep):
    model._drop_mask_override = keep.to(DEV)
    with _WidthCalls() as calls:
        logits, _ = model(x.to(DEV))
        loss = F.binary_cross_entropy_with_logits(logits, y.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
    return loss.item(), logits.detach().cpu(), calls


@pytest.mark.parametrize("prec", ["fp32", "auto"])
@pytest.mark.parametrize("width", W.MN_WIDTHS)
def test_mn_train_step_at_released_widths_matches_fp64_oracle(width, prec):
    """Loss, logits, every parameter gradient, every BatchNorm running buffer and num_batches_tracked of one step (a fixed
    drop mask) against fp64 autograd over the oracle, by the bars of test_mn_train_step_off_grid_matches_fp64_oracle: loss
    1e-4, logits 1e-3 of their scale, running buffers 1e-4, gradients rel-L2 5e-2 per tensor and 1e-2 (fp32) / 1.5e-2 (auto)
    in the median.  Tensors are compared when their fp64 norm is at least 1e-4 of the largest; only project-BatchNorm biases
    (true gradient zero) may fall below, at most 15 (the oracle alone: 12 at width 0.1, 15 elsewhere).
    Measured on MI355X, gradient median / maximum (fp32 | auto): 0.1 7.5e-6 / 2.3e-5 | 2.3e-5 / 5.6e-5;  0.2 2.2e-5 / 7.5e-5 |
    3.7e-3 / 7.3e-3;  0.4 1.2e-5 / 3.6e-5 | 5.4e-5 / 1.4e-4;  0.5 1.4e-5 / 4.0e-5 | 2.5e-3 / 7.3e-3;  2.0 3.1e-3 / 7.0e-3 | 4.7e-3 /
    1.1e-2;  3.0 1.2e-5 / 6.5e-3 | 4.8e-3 / 1.4e-2; logits at most 9.0e-5.  The medians of 2e-3 ... 5e-3 are single activations on
    the other side of a Hardswish kink, not kernel error: the per-tensor errors are round-off down to one layer and one level
    from there to the stem (2.0 fp32: from features.16, whose fp64 pre-activations come within 4e-5 of 3; 0.2 auto: from block
    12's depthwise output), on 4 x 10 and 8 x 19 planes one element carries 1 / sqrt(elements) ~ 0.4 % of a tensor's norm, and the
    oracle's own fp32 evaluation shows the same step of 3.3e-3 at width 3.0 on the same machine."""
    x, sd = W.mn_case(width, "3s")
    y, keep = W.labels_and_mask(width)
    sdr, stats, logits_ref, loss_ref = W.mn_fp64_step(width, "3s")
    model = _train_model(width, "3s", sd, prec)
    loss, logits, calls = _hip_step(model, x, y, keep)
    _check_plan((width, prec), calls, W.PLAN_F32[width])
    scale = max(1.0, float(logits_ref.abs().max()))
    el = float((logits.double() - logits_ref).abs().max())
    gmax = max(float(v.grad.norm()) for v in sdr.values() if getattr(v, "grad", None) is not None)
    rels, bad, skipped = [], [], []
    for name, p in model.named_parameters():
        ref = sdr[name].grad
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        assert ref is not None, name
        if float(ref.norm()) < 1e-4 * gmax:
            skipped.append(name)
            continue
        r = W.rel(p.grad, ref)
        rels.append((r, name))
        if r >= 5e-2:
            bad.append((name, r))
    msd = model.state_dict()
    assert stats and all(k.endswith(("running_mean", "running_var")) for k in stats)
    bn = max((W.rel(msd[k], v), k) for k, v in stats.items())
    med = float(np.median([r for r, _ in rels]))
    print(f"train mn width {width} {prec}: loss {abs(loss - float(loss_ref)):.2e}, logits {el:.2e} (|logits| <= {scale:.1f}), gradient "
          f"rel-L2 median {med:.2e} max {max(rels)[0]:.2e} ({max(rels)[1]}) over {len(rels)} tensors ({len(skipped)} under the floor), "
          f"running buffers {bn[0]:.2e} ({bn[1]})")
    assert all(_is_project_bn_bias(n, model) for n in skipped) and len(skipped) <= N_BLOCKS, skipped
    assert abs(loss - float(loss_ref)) < 1e-4 * max(1.0, abs(float(loss_ref))), (loss, float(loss_ref))
    assert el < 1e-3 * scale, (el, scale)
    assert not bad, bad[:8]
    assert med < (1e-2 if prec == "fp32" else 1.5e-2), med
    assert bn[0] < 1e-4, bn
    tracked = [k for k in msd if k.endswith("num_batches_tracked")]
    assert len(tracked) == len(stats) // 2 and all(int(msd[k]) == 1 for k in tracked)


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("width", W.MN_B16_WIDTHS)
def test_mn_train_step_bf16_at_released_widths_tracks_oracle(width, storage):
    """train_precision = 'bf16' on 7 s clips, on fp32 storage and on the bf16 storage plan (W.B16_BLOCKS: every block, at width
    0.1 every block but the residual expand-less block 2), by the two criteria of test_mn_train_step_bf16_off_grid_tracks_oracle:
    (a) the same arithmetic as the oracle's emulation - which stores in bf16 exactly the blocks the plan stores - and (b) no
    further from the fp32 oracle than that emulation is (gradient median x 1.25 + 1 %, logits x 1.5 + 1 %).

    Measured on MI355X (logits hip-emu against the bar 2e-2 x scale | hip-fp32 / emu-fp32 | gradient medians hip-emu / hip-fp32 /
    emu-fp32):
        0.1 fp32 storage 1.30e-2 < 4.4e-2 | 3.95e-2 / 4.52e-2 | 0.060 / 0.177 / 0.181;  bf16 2.05e-2 | 1.12e-1 / 1.05e-1 | 0.127 / 0.278 / 0.284
        0.5 fp32 storage 2.42e-2 < 4.9e-2 | 7.84e-2 / 6.59e-2 | 0.152 / 0.273 / 0.270;  bf16 4.42e-2 | 9.69e-2 / 8.31e-2 | 0.232 / 0.323 / 0.328
        2.0 fp32 storage 1.51e-2 < 4.8e-2 | 3.12e-2 / 3.11e-2 | 0.100 / 0.157 / 0.152;  bf16 3.65e-2 | 5.13e-2 / 6.12e-2 | 0.143 / 0.196 / 0.191
    [0.5-bf16] is the case that found mn_train._expand_weights: with the expand BatchNorm's statistics (Gram matrix of the block
    input) and the backward's coefficients taken from the fp32 weights - the product W x, which the bf16 conv never forms - it sat
    6.09e-2 from the emulation against the bar of 2e-2 x 2.45 = 4.9e-2 (0.1: 2.89e-2, 2.0: 3.25e-2).  An emulation changed to take its
    statistics that way reproduced the distance on the CPU block by block (0.0048 after block 1, 0.103 at the last map; HIP 0.0047,
    0.103); two evaluations of the plain emulation whose inputs differ in the last fp32 bit sit 2.5e-2 apart at every width, which
    is the floor of this criterion."""
    x, sd = W.mn_case(width, "7s")
    y, keep = W.labels_and_mask(width)
    st16 = set(W.B16_BLOCKS[width]) if storage == "bf16" else set()
    if width == 0.1:
        assert 2 not in W.B16_BLOCKS[width]
    sdf, _, logits_f, loss_f = W.mn_fp32_step(width, "7s")
    sde = W.grad_state(sd)
    with O.emulate_bf16_pointwise(storage=st16 if storage == "bf16" else False):
        logits_e, _ = W.mn_fwd(width)(sde, x, train=True, stats={}, drop_mask=keep)
        loss_e = F.binary_cross_entropy_with_logits(logits_e, y)
        loss_e.backward()
    logits_e, loss_e = logits_e.detach(), loss_e.detach()
    model = _train_model(width, "7s", sd, "bf16", storage)
    loss, logits, calls = _hip_step(model, x, y, keep)
    _check_plan((width, storage), calls, W.PLAN_B16[width] if storage == "bf16" else W.PLAN_F32[width])
    assert set(calls.b16_blocks) == st16 and len(calls.b16_blocks) == len(st16), (width, calls.b16_blocks, sorted(st16))
    gmax = max(float(v.grad.norm()) for v in sdf.values() if getattr(v, "grad", None) is not None)
    names = [n for n, p in model.named_parameters() if sdf[n].grad is not None and float(sdf[n].grad.norm()) >= 1e-5 * gmax]
    gp = dict(model.named_parameters())
    for n in gp:
        assert gp[n].grad is not None and torch.isfinite(gp[n].grad).all(), n
    emu_vs_f = np.array([W.rel(sde[n].grad, sdf[n].grad) for n in names])
    hip_vs_e = np.array([W.rel(gp[n].grad, sde[n].grad) for n in names])
    hip_vs_f = np.array([W.rel(gp[n].grad, sdf[n].grad) for n in names])
    scale = float(logits_f.abs().max())
    e_he, e_hf, e_ef = (float((logits - logits_e).abs().max()), float((logits - logits_f).abs().max()),
                        float((logits_e - logits_f).abs().max()))
    print(f"bf16 mn width {width} storage {storage} (bf16-stored blocks {sorted(st16)}): loss hip {loss:.6f} emu {float(loss_e):.6f} "
          f"fp32 {float(loss_f):.6f}; logits hip-emu {e_he:.2e}, hip-fp32 {e_hf:.2e}, emu-fp32 {e_ef:.2e} (|logits| <= {scale:.1f}); "
          f"gradient medians hip-emu {np.median(hip_vs_e):.3f}, hip-fp32 {np.median(hip_vs_f):.3f}, emu-fp32 {np.median(emu_vs_f):.3f}")
    assert np.isfinite(hip_vs_e).all()
    # (a) the same arithmetic
    assert abs(loss - float(loss_e)) < 2e-3 * abs(float(loss_e)), (loss, float(loss_e))
    assert e_he < 2e-2 * scale, (e_he, scale)
    assert float(np.median(hip_vs_e)) < float(np.median(emu_vs_f)), (float(np.median(hip_vs_e)), float(np.median(emu_vs_f)))
    # (b) bf16 noise against the fp32 oracle: not larger than the emulated oracle's own
    assert abs(loss - float(loss_f)) < 2e-2 * abs(float(loss_f)), (loss, float(loss_f))
    assert float(np.median(hip_vs_f)) < 1.25 * float(np.median(emu_vs_f)) + 1e-2, (float(np.median(hip_vs_f)), float(np.median(emu_vs_f)))
    assert e_hf < 1.5 * e_ef + 1e-2 * scale, (e_hf, e_ef)


# ------------------------------------------------------------------------------------------------------------- DyMN 0.4
def _dymn_model(sd, temp, variant="all"):
    m = _quiet(get_dymn, width_mult=W.DYMN_WIDTH, **W.DYMN_VARIANTS[variant])
    m.load_state_dict(sd, strict=True)
    for mod in m.modules():
        if hasattr(mod, "temperature"):
            mod.temperature = temp
    return m.to(DEV)


def _dymn_blocks_plan(x, storage16):
    """Per dynamic block: (fused, bf16-stored) as dymn_train._block_train_fused decides them for input x."""
    blocks, _ = O.block_table(W.DYMN_WIDTH)
    f, t = (x.shape[2] - 1) // 2 + 1, (x.shape[3] - 1) // 2 + 1
    plan = []
    for c in blocks:
        fo, to = ops.conv_out(f, c["k"], c["stride"]), ops.conv_out(t, c["k"], c["stride"])
        fused = to <= 512 and ops.dw_bwd_merged_ok((B, c["cexp"], fo, to), (B, c["cexp"], f, t), c["k"], c["stride"])
        b16 = storage16 and fused and ops.dyn_b16_block_ok(B, c["cin"], c["cexp"], c["cout"], f, t, c["k"], c["stride"]) and \
            (c["cexp"] != c["cin"] or (t > 128 and c["k"] == 3 and c["stride"] == 1))
        plan.append((bool(fused), bool(b16)))
        f, t = fo, to
    return plan


def _check_dymn_paths(calls, stored):
    """All 15 blocks on the fused block step (none on the unfused path), `stored` of them on bf16 storage, no K-concat GEMM."""
    n = calls.n
    assert n["eat_dyrelu_ca_fwd"] == 0 and n["eat_dyrelu_ca_bwd"] == 0, dict(n)
    assert n["eat_dyrelu_ca_fwd2"] + n["eat_dyrelu_ca_fwd2_b16"] == N_BLOCKS, dict(n)
    assert n["eat_dyrelu_ca_fwd2_b16"] == len(stored) and n["eat_dyrelu_ca_bwd2_b16"] == len(stored), dict(n)
    assert n["eat_pw_conv_kcat_fwd"] == 0, dict(n)


@pytest.mark.parametrize("variant", list(W.DYMN_VARIANTS))
def test_dymn04_eval_matches_fp64_oracle(variant):
    x, sd = W.dymn_case("3s", variant)
    ref, ref_fmaps = W.dymn_eval_ref("3s", variant)
    model = _dymn_model(sd, 1.0, variant).eval()
    with torch.no_grad(), _WidthCalls() as calls:
        got, _ = model(x.to(DEV))
        _, fmaps = model(x.to(DEV), return_fmaps=True)
        torch.cuda.synchronize()
    assert calls.n["eat_pw_conv_kcat_fwd"] == 0 and calls.n["eat_front_fwd"] == 0, dict(calls.n)
    assert got.shape == ref.shape and len(fmaps) == len(ref_fmaps)
    for i, (a, b) in enumerate(zip(fmaps, ref_fmaps)):
        assert a.shape == b.shape, i
    errs = [W.rel(a, b) for a, b in zip(fmaps, ref_fmaps)]
    scale = max(1.0, float(ref.abs().max()))
    e = float((got.cpu().double() - ref).abs().max())
    print(f"eval dymn04 {variant}: logits max abs {e:.2e} (|logits| <= {scale:.1f}), fmap rel-L2 max {max(errs):.2e}")
    assert max(errs) < 2e-4, errs
    assert e < 1e-3 * scale, (e, scale)


def _dymn_hip_step(sd, x, y, keep, prec, storage="fp32"):
    model = _dymn_model(sd, 30.0).train()
    model.train_precision, model.act_storage = prec, storage
    model._drop_mask_override = keep.to(DEV)
    with _WidthCalls() as calls:
        logits, _ = model(x.to(DEV))
        loss = F.binary_cross_entropy_with_logits(logits, y.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
    return model, loss.item(), logits.detach().cpu(), calls


def _is_dymn_floor_class(name):
    return name.endswith("proj_norm.bias") or ".residuals.0." in name


@pytest.mark.parametrize("prec", ["fp32", "auto"])
def test_dymn04_train_step_matches_fp64_oracle(prec):
    """One step at temperature 30 (a fixed drop mask) against fp64 autograd over the oracle, the bars of
    test_dymn_train_step_off_grid_matches_fp64_oracle: loss 1e-4, logits 1e-3 of their scale, running buffers 1e-4, gradients
    5e-2 per tensor (`.residuals.0.` under 'auto': 1e-1), median 1e-2 / 2e-2.  Under the floor of 1e-4 of the largest norm lie
    only `proj_norm.bias` and `.residuals.0.` tensors, at most 56 (the oracle alone: 47) of the 365 parameters - 395 tensors of
    the oracle's state carry a gradient, the 30 DyReLU constants `lambdas` / `init_v` are buffers of the model."""
    x, sd = W.dymn_case("3s")
    y, keep = W.labels_and_mask(W.DYMN_WIDTH)
    sdr, stats, logits_ref, loss_ref = W.dymn_fp64_step("3s")
    plan = _dymn_blocks_plan(x, False)
    assert plan == [(True, False)] * N_BLOCKS, plan
    model, loss, logits, calls = _dymn_hip_step(sd, x, y, keep, prec)
    _check_dymn_paths(calls, ())
    scale = max(1.0, float(logits_ref.abs().max()))
    el = float((logits.double() - logits_ref).abs().max())
    gmax = max(float(v.grad.norm()) for v in sdr.values() if getattr(v, "grad", None) is not None)
    rels, bad, skipped = [], [], []
    params = list(model.named_parameters())
    assert len(params) == 365 and sum(getattr(v, "grad", None) is not None for v in sdr.values()) == 395
    for name, p in params:
        ref = sdr[name].grad
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
        assert ref is not None, name
        if float(ref.norm()) < 1e-4 * gmax:
            skipped.append(name)
            continue
        r = W.rel(p.grad, ref)
        rels.append((r, name))
        if r > (5e-2 if prec == "fp32" or ".residuals.0." not in name else 1e-1):
            bad.append((name, r))
    msd = model.state_dict()
    bn = max((W.rel(msd[k], v), k) for k, v in stats.items())
    med = float(np.median([r for r, _ in rels]))
    print(f"train dymn04 {prec}: loss {abs(loss - float(loss_ref)):.2e}, logits {el:.2e} (|logits| <= {scale:.1f}), gradient rel-L2 "
          f"median {med:.2e} max {max(rels)[0]:.2e} ({max(rels)[1]}) over {len(rels)} tensors ({len(skipped)} under the floor), "
          f"running buffers {bn[0]:.2e} ({bn[1]})")
    assert all(_is_dymn_floor_class(n) for n in skipped) and len(skipped) <= 56, skipped
    assert abs(loss - float(loss_ref)) < 1e-4 * max(1.0, abs(float(loss_ref)))
    assert el < 1e-3 * scale, (el, scale)
    assert not bad, bad[:8]
    assert med < (1e-2 if prec == "fp32" else 2e-2), med
    assert bn[0] < 1e-4, bn


def test_dymn04_train_step_bf16_storage_tracks_oracle():
    """act_storage = 'bf16' on 5 s clips, where the plan stores blocks 0, 1, 13, 14 (W.DYMN_B16_BLOCKS_5S) and keeps the others
    in fp32: against the oracle's emulation of the same block list and against the fp32 oracle, the two criteria of
    test_dymn_train_step_bf16_storage_off_grid_tracks_oracle."""
    x, sd = W.dymn_case("5s")
    y, keep = W.labels_and_mask(W.DYMN_WIDTH)
    plan = _dymn_blocks_plan(x, True)
    st16 = set(W.DYMN_B16_BLOCKS_5S)
    assert all(f for f, _ in plan) and {i for i, (_, b) in enumerate(plan) if b} == st16, plan
    sdf, _, logits_f, loss_f = W.dymn_fp32_step("5s")
    sde = W.grad_state(sd)
    with O.emulate_bf16_pointwise(storage=st16):
        logits_e, _ = W.dymn_fwd(temperature=30.0)(sde, x, train=True, stats={}, drop_mask=keep)
        loss_e = F.binary_cross_entropy_with_logits(logits_e, y)
        loss_e.backward()
    logits_e, loss_e = logits_e.detach(), loss_e.detach()
    model, loss, logits, calls = _dymn_hip_step(sd, x, y, keep, "bf16", "bf16")
    _check_dymn_paths(calls, st16)
    gmax = max(float(v.grad.norm()) for v in sdf.values() if getattr(v, "grad", None) is not None)
    names = [n for n, p in model.named_parameters() if sdf[n].grad is not None and float(sdf[n].grad.norm()) >= 1e-4 * gmax]
    gp = dict(model.named_parameters())
    for n in names:
        assert gp[n].grad is not None and torch.isfinite(gp[n].grad).all(), n
    emu_vs_f = np.array([W.rel(sde[n].grad, sdf[n].grad) for n in names])
    hip_vs_e = np.array([W.rel(gp[n].grad, sde[n].grad) for n in names])
    hip_vs_f = np.array([W.rel(gp[n].grad, sdf[n].grad) for n in names])
    scale = float(logits_f.abs().max())
    e_he, e_hf, e_ef = (float((logits - logits_e).abs().max()), float((logits - logits_f).abs().max()),
                        float((logits_e - logits_f).abs().max()))
    print(f"bf16 storage dymn04 5s (blocks {sorted(st16)}): logits hip-emu {e_he:.2e}, hip-fp32 {e_hf:.2e}, emu-fp32 {e_ef:.2e}; "
          f"gradient medians hip-emu {np.median(hip_vs_e):.3f}, hip-fp32 {np.median(hip_vs_f):.3f}, emu-fp32 {np.median(emu_vs_f):.3f}")
    # (a) the same arithmetic
    assert abs(loss - float(loss_e)) < 2e-3 * abs(float(loss_e)), (loss, float(loss_e))
    assert e_he < 2e-2 * scale, (e_he, scale)
    assert float(np.median(hip_vs_e)) < float(np.median(emu_vs_f))
    # (b) bf16 noise against the fp32 oracle: not larger than the emulated oracle's own
    assert abs(loss - float(loss_f)) < 2e-2 * abs(float(loss_f))
    assert float(np.median(hip_vs_f)) < 1.25 * float(np.median(emu_vs_f)) + 1e-2
    assert e_hf < 1.5 * e_ef + 1e-2 * scale, (e_hf, e_ef)
