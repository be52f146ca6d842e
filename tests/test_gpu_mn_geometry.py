"""The MN training step off the 128-mel / 10 s grid, against the float64 oracle.

The monolithic plan (efficientat_amd/mn_train.py) picks its kernels by geometry, block by block: the two-source data-gradient
GEMM (`cat`) where the block input has S % 4 == 0 (bf16 storage: C_exp % 32 == 0), the depthwise BatchNorm + activation on load
in the project conv and its weight gradient (`on_load`) where `ops.pw_tf_eligible` holds and - SE blocks - the depthwise
output has at least 2000 positions, bf16 storage (`b16`) only for the blocks `ops.b16_block_ok` admits, so that off the grid
`act_storage='bf16'` is a per-block mixture.  The depthwise instances, the generic 4-byte 1x1 kernel and the bf16 copies of
the narrow operands depend on the plane as well.  Every case below is a geometry no other training test reaches; the
reference is fp64 autograd over the oracle, and the call counts pin the branches each case was written for against tables of
literals (PLAN_F32, B16_BLOCKS, PLAN_B16) - a changed predicate turns the case red instead of moving it onto another path."""
import contextlib
import functools
import io
from collections import Counter

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import eat_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, ops  # noqa: E402
from efficientat_amd.mn import get_model  # noqa: E402

DEV = torch.device("cuda:0")
B = 3
N_BLOCKS = 15

# id: (mel bins, samples at 32 kHz; frames = samples / 320).  Planes P0 ... P4 (stem output, then after each stride-2 block):
#   0.3 s: 64x15, 32x8, 16x4, 8x2, 4x1;  1 s: 64x50, 32x25, 16x13, 8x7, 4x4;  5 s (ESC-50): 64x250, 32x125, 16x63, 8x32, 4x16;
#   7 s: 64x350, 32x175, 16x88, 8x44, 4x22 (the grid's plane-kernel instances at other widths: ragged lanes);
#   11 s: 64x550, 32x275, 16x138, 8x69, 4x35;  40 mels: 20x500, 10x250, 5x125, 3x63, 2x32;  64 mels: 32x485, 16x243, 8x122, 4x61, 2x31
GEOMETRIES = {"0.3s": (128, 9600), "1s": (128, 32000), "5s": (128, 160000), "7s": (128, 224000), "11s": (128, 352000),
              "40mels": (40, 320000), "64mels": (64, 310400)}

# Blocks (indices into features[1:-1]): expand conv in 1 ... 14; SE gate in 3, 4, 5, 10 ... 14; input planes P0: 0, 1;  P1: 2, 3;
# P2: 4, 5, 6;  P3: 7 ... 12;  P4: 13, 14;  depthwise output planes P0: 0;  P1: 1, 2;  P2: 3, 4, 5;  P3: 6 ... 11;  P4: 12, 13, 14.
#
# fp32 storage (train_precision fp32 / auto / bf16), per case:
#   cat      two-source data-gradient GEMMs (eat_pw_conv_cat_fwd): the blocks with expand conv whose INPUT plane is a multiple of 4
#   on_load  project convs AND project weight gradients that evaluate the depthwise BatchNorm + activation on load: the blocks
#            whose depthwise OUTPUT plane is a multiple of 4, SE blocks only from 2000 positions
#   merged   merged depthwise backward launches (eat_dw_conv_bwd_bn_g): every block at every size a test can afford
PLAN_F32 = {
    # P1 = 256, P2 = 64, P3 = 16, P4 = 4: every plane a multiple of 4, every SE plane below 2000
    "0.3s": dict(cat=14, on_load=7, merged=15),
    # P2 = 208, P3 = 56, P4 = 16
    "1s": dict(cat=14, on_load=7, merged=15),
    # P2 = 16 x 63 = 1008 < 2000: SE blocks 3 - 5 off the on-load path (at 10 s they sit on it: 16 x 125 = 2000)
    "5s": dict(cat=14, on_load=7, merged=15),
    # P2 = 16 x 88 = 1408 < 2000
    "7s": dict(cat=14, on_load=7, merged=15),
    # P2 = 16 x 138 = 2208 >= 2000: blocks 3, 4, 5 on load as well
    "11s": dict(cat=14, on_load=10, merged=15),
    # P2 = 5 x 125 = 625 and P3 = 3 x 63 = 189 are no multiples of 4: cat only in 1, 2, 3 (P0, P1) and 13, 14 (P4 = 64);
    # on load only in 0, 1, 2 (P0 = 10000, P1 = 2500; the SE blocks 12 - 14 at P4 = 64 are below 2000)
    "40mels": dict(cat=5, on_load=3, merged=15),
    # P0 = 15520, P1 = 3888, P2 = 976, P3 = 244 are multiples of 4; P4 = 2 x 31 = 62 is not: cat in 1 ... 12, on load in 0, 1, 2 and
    # the non-SE blocks 6 ... 9 at P3
    "64mels": dict(cat=12, on_load=7, merged=15),
}

# act_storage = 'bf16': the blocks that store their wide tensors in bf16 (eat_dw_conv_b16_ok: tile kernels for T > 128, plane
# kernels at F = 16 / 8 / 4 for 64 < T <= 128 / 32 < T <= 64 / T <= 32 and certain (k, stride); both planes multiples of 8)
B16_BLOCKS = {
    "0.3s": (),                           # P0 = 64 x 15: T <= 128 and F = 64; no plane kernel takes 32 x 8, 16 x 4, 8 x 2; 4 x 1 is no multiple of 8
    "1s": (13, 14),                       # 4 x 4 (k = 5, stride 1) only
    "5s": (0, 1, 13, 14),                 # 64 x 250 tiles; 32 x 125: T <= 128 and F = 32; 16 x 63, 8 x 32: T at the lower edge, excluded; 4 x 16
    "7s": tuple(range(N_BLOCKS)),         # 64 x 350, 32 x 175 tiles; 16 x 88, 8 x 44, 4 x 22 plane kernels
    "11s": (0, 1, 2, 3, 4, 5, 6),         # tiles down to 16 x 138; 8 x 69: T > 64 and F = 8; 4 x 35: T > 32
    "40mels": (0,),                       # block 1's output 10 x 250 = 2500 is no multiple of 8; 5 x 125 and 3 x 63 are odd; 2 x 32 has F = 2
    "64mels": (0, 1, 2, 3),               # tiles down to 16 x 243 (block 3: output 8 x 122 = 976); 8 x 122: T <= 128 and F = 8
}

# ... and the counts of the step under that plan: the fp32-storage kernels serve the other blocks
#   cat16 / on_load16 / merged16: the forms over bf16-stored tensors (eat_pw_conv_b16_fwd with x2 / with tf, eat_pw_conv_wgrad_b16
#   with tf, eat_dw_conv_bwd_bn_g_b16); stats16: eat_dw_conv_fwd_stats_b16.  cat16: the stored blocks with expand conv and
#   C_exp % 32 == 0 - 64 in block 1, 480, 672, 672, 960, 960 in 10 ... 14; the stored blocks with C_exp = 72, 120, 240, 200, 184
#   (2 ... 9) take the two single-source GEMMs, which neither column counts
PLAN_B16 = {
    # stored 0, 1, 13, 14: cat16 in 1, 13, 14, cat in 2 ... 12; on load: 0, 1 stored, 2, 6 ... 9 not
    "5s": dict(cat=11, cat16=3, on_load=5, on_load16=2, merged=11, merged16=4, stats16=4),
    # every block stored: cat16 in 1, 10 ... 14; on load 0, 1, 2, 6 ... 9
    "7s": dict(cat=0, cat16=6, on_load=0, on_load16=7, merged=0, merged16=15, stats16=15),
    # stored 0 ... 6: cat16 in 1 only, cat in 7 ... 14; on load: 0 ... 6 stored, 7, 8, 9 not
    "11s": dict(cat=8, cat16=1, on_load=3, on_load16=7, merged=8, merged16=7, stats16=7),
    # stored 0 ... 3: cat16 in 1, cat in 4 ... 12 (13, 14 read 2 x 31 planes); on load: 0, 1, 2 stored, 6 ... 9 not
    "64mels": dict(cat=9, cat16=1, on_load=4, on_load16=3, merged=11, merged16=4, stats16=4),
}


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / max(1e-30, float(b.norm())))


def _grad_state(sd, double=False):
    return {k: ((v.double() if double else v.clone()).requires_grad_(True) if v.is_floating_point() and "running" not in k
                else (v.double() if double and v.is_floating_point() else v.clone())) for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def _case(geo):
    """(x (B, 1, mels, frames) fp32, state calibrated on that input: running statistics = its batch statistics)."""
    n_mels, n = GEOMETRIES[geo]
    x = O.mel_forward(synth.parity_clips(n, seed=7)[:B], n_mels=n_mels).unsqueeze(1)
    assert x.shape == (B, 1, n_mels, n // 320)
    sd = synth.calibrate(synth.synth_state(synth.mn_shapes(1.0), seed=0), O.mn_forward, x)
    return x, sd


def _labels_and_mask():
    y = (torch.rand(B, 527, generator=torch.Generator().manual_seed(5)) < 0.01).float()
    keep = (torch.rand(B, 1280, generator=torch.Generator().manual_seed(6)) < 0.8).float()
    return y, keep


@functools.lru_cache(maxsize=None)
def _fp64_step(geo):
    """fp64 autograd over the oracle, once per geometry: (state with .grad, running buffers, logits, loss)."""
    x, sd = _case(geo)
    y, keep = _labels_and_mask()
    sdr = _grad_state(sd, double=True)
    stats = {}
    logits, _ = O.mn_forward(sdr, x.double(), train=True, stats=stats, drop_mask=keep.double())
    loss = F.binary_cross_entropy_with_logits(logits, y.double())
    loss.backward()
    return sdr, stats, logits.detach(), loss.detach()


@functools.lru_cache(maxsize=None)
def _fp32_step(geo):
    """The oracle as it stands (fp32), once per geometry: (state with .grad, logits, loss) - the anchor of the bf16 criteria."""
    x, sd = _case(geo)
    y, keep = _labels_and_mask()
    sdf = _grad_state(sd)
    logits, _ = O.mn_forward(sdf, x, train=True, stats={}, drop_mask=keep)
    loss = F.binary_cross_entropy_with_logits(logits, y)
    loss.backward()
    return sdf, logits.detach(), loss.detach()


def _model(geo, sd, prec, storage="fp32"):
    n_mels, n = GEOMETRIES[geo]
    m = _quiet(get_model, width_mult=1.0, input_dim_f=n_mels, input_dim_t=n // 320)
    m.load_state_dict(sd, strict=True)
    m.to(DEV).train()
    m.train_precision, m.act_storage = prec, storage
    return m


class _Calls:
    """with _Calls() as c: ...  ->  c.n[entry point] = calls made through efficientat_amd._lib (`call` and `call_rc`) inside the
    block; c.plan() = the counts that tell the plan's branches apart; c.b16_blocks = the blocks whose depthwise forward ran on
    the bf16-storage kernel (the plan calls one depthwise forward per block, in block order)."""

    def __enter__(self):
        self.n, self.tag, self.b16_blocks, self.saved = Counter(), Counter(), [], (_lib.call, _lib.call_rc)

        def note(name, a, rc):
            self.n[name] += 1
            if name == "eat_pw_conv_b16_fwd":                        # (x, x_b16, x2, C1, wp, bias, tf_a, ...)
                self.tag["cat16"] += a[2] is not None
                self.tag["tf_fwd16"] += a[6] is not None
            elif name == "eat_pw_conv_wgrad_b16":                    # (dz, dz_b16, x, x_b16, tf_a, ...)
                self.tag["tf_wgrad16"] += a[4] is not None
            elif name == "eat_pw_conv_stats_fwd":                    # (x, wp, wmode, per_sample, tf_a, ...); rc 1: declined
                self.tag["tf_fwd"] += a[4] is not None and rc == 0
            elif name == "eat_pw_conv_tf_fwd":
                self.tag["tf_fwd"] += 1
            elif name in ("eat_dw_conv_fwd_stats", "eat_dw_conv_fwd_stats_b16"):
                if name.endswith("_b16"):
                    self.b16_blocks.append(self.n["eat_dw_conv_fwd_stats"] + self.n["eat_dw_conv_fwd_stats_b16"] - 1)

        def call(name, *a):
            note(name, a, 0)
            return self.saved[0](name, *a)

        def call_rc(name, *a):
            rc = self.saved[1](name, *a)
            note(name, a, rc)
            return rc
        _lib.call, _lib.call_rc = call, call_rc
        return self

    def __exit__(self, *exc):
        _lib.call, _lib.call_rc = self.saved

    def plan(self):
        n, t = self.n, self.tag
        return dict(cat=n["eat_pw_conv_cat_fwd"], cat16=t["cat16"], on_load=t["tf_fwd"], on_load_wgrad=n["eat_pw_conv_wgrad_tf"],
                    on_load16=t["tf_fwd16"], on_load_wgrad16=t["tf_wgrad16"], merged=n["eat_dw_conv_bwd_bn_g"],
                    merged16=n["eat_dw_conv_bwd_bn_g_b16"], stats16=n["eat_dw_conv_fwd_stats_b16"])


def _check_plan(geo, calls, want):
    """`want`: a row of PLAN_F32 / PLAN_B16 (forms it does not name: no call; the on-load weight gradients as the convs)."""
    full = dict(cat16=0, on_load16=0, merged16=0, stats16=0)
    full.update(want)
    full["on_load_wgrad"], full["on_load_wgrad16"] = full["on_load"], full["on_load16"]
    got = calls.plan()
    assert got == full, (geo, got, full)
    assert calls.n["eat_dw_conv_fwd_stats"] + calls.n["eat_dw_conv_fwd_stats_b16"] == N_BLOCKS, (geo, dict(calls.n))


def _hip_step(model, x, y, keep):
    model._drop_mask_override = keep.to(DEV)
    with _Calls() as calls:
        logits, _ = model(x.to(DEV))
        loss = F.binary_cross_entropy_with_logits(logits, y.to(DEV))
        loss.backward()
        torch.cuda.synchronize()
    return loss.item(), logits.detach().cpu(), calls


def _is_project_bn_bias(name, model):
    """features.<i + 1>.block.<i_proj>.1.bias: the bias of a project BatchNorm.  The depthwise / expand BatchNorm of the next
    layer removes a per-channel constant... only where no residual or further conv mixes it; on this network its fp64
    gradient is round-off (below 1e-4 of the largest tensor) in all 15 blocks, and in no other tensor."""
    parts = name.split(".")
    if len(parts) != 6 or parts[0] != "features" or parts[2] != "block" or parts[4:] != ["1", "bias"]:
        return False
    blk = model.features[int(parts[1])]
    return int(parts[3]) == blk.i_proj


# ------------------------------------------------------------------------------------------------ one train step
@pytest.mark.parametrize("prec", ["fp32", "auto"])
@pytest.mark.parametrize("geo", list(GEOMETRIES))
def test_mn_train_step_off_grid_matches_fp64_oracle(geo, prec):
    """Loss, logits, every parameter gradient, every BatchNorm running buffer and num_batches_tracked of one step (a fixed
    drop mask) against fp64 autograd over the oracle.  Bars: loss 1e-4, logits 1e-3 of their scale, running buffers 1e-4,
    gradients rel-L2 5e-2 per tensor and 1e-2 (fp32) / 1.5e-2 (auto) in the median - the three-clip bars of
    test_mn10_other_mel_geometries_match_oracle and of the DyMN off-grid file; the oracle's own fp32 evaluation sits within
    7e-8 / 1.2e-5 / median 1.2e-5, maximum 5.3e-3 of its fp64 one on these inputs.  Tensors are compared when their fp64
    reference norm is at least 1e-4 of the largest; only the 15 project-BatchNorm biases (true gradient zero) may fall below."""
    x, sd = _case(geo)
    y, keep = _labels_and_mask()
    sdr, stats, logits_ref, loss_ref = _fp64_step(geo)
    model = _model(geo, sd, prec)
    loss, logits, calls = _hip_step(model, x, y, keep)
    _check_plan(geo, calls, PLAN_F32[geo])
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
        r = _rel(p.grad, ref)
        rels.append((r, name))
        if r >= 5e-2:
            bad.append((name, r))
    msd = model.state_dict()
    assert stats and all(k.endswith(("running_mean", "running_var")) for k in stats)
    bn = max((_rel(msd[k], v), k) for k, v in stats.items())
    med = float(np.median([r for r, _ in rels]))
    print(f"train {geo} {prec}: loss {abs(loss - float(loss_ref)):.2e}, logits {el:.2e} (|logits| <= {scale:.1f}), gradient rel-L2 median "
          f"{med:.2e} max {max(rels)[0]:.2e} ({max(rels)[1]}) over {len(rels)} tensors, running buffers {bn[0]:.2e} ({bn[1]})")
    assert all(_is_project_bn_bias(n, model) for n in skipped) and len(skipped) <= N_BLOCKS, skipped
    assert abs(loss - float(loss_ref)) < 1e-4 * max(1.0, abs(float(loss_ref))), (loss, float(loss_ref))
    assert el < 1e-3 * scale, (el, scale)
    assert not bad, bad[:8]
    assert med < (1e-2 if prec == "fp32" else 1.5e-2), med
    assert bn[0] < 1e-4, bn
    tracked = [k for k in msd if k.endswith("num_batches_tracked")]
    assert len(tracked) == len(stats) // 2 and all(int(msd[k]) == 1 for k in tracked)


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
@pytest.mark.parametrize("geo", ["5s", "7s", "11s", "64mels"])
def test_mn_train_step_bf16_off_grid_tracks_oracle(geo, storage):
    """train_precision = 'bf16' off the grid, on fp32 storage and on the per-block bf16 storage plan (B16_BLOCKS: a mixture
    at 5 s, 11 s and 64 mels, every block at 7 s), by the two criteria of test_mn40_train_step_bf16_tracks_oracle: (a) the same
    arithmetic as the oracle's emulation - which stores in bf16 exactly the blocks the plan stores - and (b) no further from the
    fp32 oracle than that emulation is (gradient median x 1.25 + 1 %, logits x 1.5 + 1 %)."""
    x, sd = _case(geo)
    y, keep = _labels_and_mask()
    st16 = set(B16_BLOCKS[geo]) if storage == "bf16" else set()
    if storage == "bf16":
        assert (len(st16) == N_BLOCKS) if geo == "7s" else (0 < len(st16) < N_BLOCKS), (geo, st16)
    sdf, logits_f, loss_f = _fp32_step(geo)
    sde = _grad_state(sd)
    with O.emulate_bf16_pointwise(storage=st16 if storage == "bf16" else False):
        logits_e, _ = O.mn_forward(sde, x, train=True, stats={}, drop_mask=keep)
        loss_e = F.binary_cross_entropy_with_logits(logits_e, y)
        loss_e.backward()
    logits_e, loss_e = logits_e.detach(), loss_e.detach()
    model = _model(geo, sd, "bf16", storage)
    loss, logits, calls = _hip_step(model, x, y, keep)
    _check_plan(geo, calls, PLAN_B16[geo] if storage == "bf16" else PLAN_F32[geo])
    assert set(calls.b16_blocks) == st16 and len(calls.b16_blocks) == len(st16), (geo, calls.b16_blocks, sorted(st16))
    gmax = max(float(v.grad.norm()) for v in sdf.values() if getattr(v, "grad", None) is not None)
    names = [n for n, p in model.named_parameters() if sdf[n].grad is not None and float(sdf[n].grad.norm()) >= 1e-5 * gmax]
    gp = dict(model.named_parameters())
    for n in gp:
        assert gp[n].grad is not None and torch.isfinite(gp[n].grad).all(), n
    emu_vs_f = np.array([_rel(sde[n].grad, sdf[n].grad) for n in names])
    hip_vs_e = np.array([_rel(gp[n].grad, sde[n].grad) for n in names])
    hip_vs_f = np.array([_rel(gp[n].grad, sdf[n].grad) for n in names])
    scale = float(logits_f.abs().max())
    e_he, e_hf, e_ef = (float((logits - logits_e).abs().max()), float((logits - logits_f).abs().max()),
                        float((logits_e - logits_f).abs().max()))
    print(f"bf16 {geo} storage {storage} (bf16-stored blocks {sorted(st16)}): loss hip {loss:.6f} emu {float(loss_e):.6f} fp32 "
          f"{float(loss_f):.6f}; logits hip-emu {e_he:.2e}, hip-fp32 {e_hf:.2e}, emu-fp32 {e_ef:.2e} (|logits| <= {scale:.1f}); gradient "
          f"medians hip-emu {np.median(hip_vs_e):.3f}, hip-fp32 {np.median(hip_vs_f):.3f}, emu-fp32 {np.median(emu_vs_f):.3f}")
    assert np.isfinite(hip_vs_e).all()
    # (a) the same arithmetic
    assert abs(loss - float(loss_e)) < 2e-3 * abs(float(loss_e)), (loss, float(loss_e))
    assert e_he < 2e-2 * scale, (e_he, scale)
    assert float(np.median(hip_vs_e)) < float(np.median(emu_vs_f)), (float(np.median(hip_vs_e)), float(np.median(emu_vs_f)))
    # (b) bf16 noise against the fp32 oracle: not larger than the emulated oracle's own
    assert abs(loss - float(loss_f)) < 2e-2 * abs(float(loss_f)), (loss, float(loss_f))
    assert float(np.median(hip_vs_f)) < 1.25 * float(np.median(emu_vs_f)) + 1e-2, (float(np.median(hip_vs_f)), float(np.median(emu_vs_f)))
    assert e_hf < 1.5 * e_ef + 1e-2 * scale, (e_hf, e_ef)


def test_mn_captured_step_off_grid_reproduces_its_gradients():
    """5 s clips on the mixed storage plan (blocks 0, 1, 13, 14 in bf16, the others in fp32): every replay of the captured step
    at learning rate 0 must reproduce the eager gradients - bar and structure of
    test_mn_captured_step_reproduces_its_gradients_on_every_replay (bf16 storage: 5e-2 over the tensors above 1e-3 of the largest)."""
    from efficientat_amd.graphs import GraphedTrainStep
    x, sd = _case("5s")
    y, keep = _labels_and_mask()
    x, y = x.to(DEV), y.to(DEV)

    def build():
        m = _model("5s", sd, "bf16", "bf16")
        m._drop_mask_override = keep.to(DEV)
        return m
    ref = build()
    with _Calls() as calls:
        logits, _ = ref(x)
        F.binary_cross_entropy_with_logits(logits, y).backward()
    _check_plan("5s", calls, PLAN_B16["5s"])
    ref_g = {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
    gmax = max(float(g.norm()) for g in ref_g.values())
    model = build()
    step = GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=0.0), F.binary_cross_entropy_with_logits, x, y)
    for r in range(4):
        step(step.x, step.y)
        torch.cuda.synchronize()
        worst = (0.0, None)
        for n, p in model.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), (r, n)
            if float(ref_g[n].norm()) < 1e-3 * gmax:
                continue
            e = float((p.grad - ref_g[n]).norm() / ref_g[n].norm())
            if e > worst[0]:
                worst = (e, n)
        print(f"captured 5s bf16 storage, replay {r}: worst gradient rel-L2 {worst[0]:.2e} ({worst[1]})")
        assert worst[0] < 5e-2, (r, worst)


def test_mn_train_step_5s_at_batch_48_reproduces_the_three_clip_step():
    """ESC-50's regime: many samples of small planes through the multi-sample reducers and the split-K weight gradients.  With
    the mean-reduced loss, 16 copies of the three 5 s clips have exactly the batch statistics, loss and parameter gradients of
    the three clips, whose step test_mn_train_step_off_grid_matches_fp64_oracle pins on the oracle (precision 'auto').
    Forward quantities must agree to round-off (loss 2e-5, logits and running buffers 2e-4); the gradients sum in different
    orders, so an activation at a kink may change side in all copies at once: per tensor 3e-2, median 5e-3 (the bars of
    test_gpu_configs.py::_check_tiled)."""
    reps, grad_tol, fwd_tol, med_tol = 16, 3e-2, 2e-5, 5e-3
    x, sd = _case("5s")
    y, keep = _labels_and_mask()
    runs, bufs = {}, {}
    for r in (1, reps):
        model = _model("5s", sd, "auto")
        loss, logits, calls = _hip_step(model, x.repeat(r, 1, 1, 1), y.repeat(r, 1), keep.repeat(r, 1))
        _check_plan("5s", calls, PLAN_F32["5s"])
        runs[r] = (loss, logits, {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()})
        bufs[r] = {k: v.detach().cpu() for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var"))}
        del model
    (loss_s, logits_s, g_s), (loss_l, logits_l, g_l) = runs[1], runs[reps]
    scale = max(1.0, float(logits_s.abs().max()))
    el = max(float((logits_l[c * B:(c + 1) * B] - logits_s).abs().max()) for c in (0, reps // 2, reps - 1))
    gmax = max(float(v.norm()) for v in g_s.values())
    rels = [(_rel(g_l[n], ref), n) for n, ref in g_s.items() if float(ref.norm()) >= 1e-4 * gmax]
    med = float(np.median([r for r, _ in rels]))
    bn = max((_rel(bufs[reps][k], v), k) for k, v in bufs[1].items())
    print(f"5s at batch {reps * B} vs batch {B}: loss {abs(loss_l - loss_s):.2e}, logits {el:.2e}, gradient rel-L2 median {med:.2e} "
          f"max {max(rels)[0]:.2e} ({max(rels)[1]}) over {len(rels)} tensors, running buffers {bn[0]:.2e} ({bn[1]})")
    for n, g in g_l.items():
        assert torch.isfinite(g).all(), n
    assert abs(loss_l - loss_s) < fwd_tol * max(1.0, abs(loss_s)), (loss_l, loss_s)
    assert el < 10 * fwd_tol * scale, (el, scale)
    bad = [(r, n) for r, n in rels if r >= grad_tol]
    assert not bad, max(bad)
    assert med < med_tol, med
    assert bn[0] < 10 * fwd_tol, bn
