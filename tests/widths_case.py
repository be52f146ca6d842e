"""Cases of tests/test_gpu_widths.py: inputs, calibrated states, the cached oracle steps and the tables of literals that
pin which kernels each released width runs.  Importable without a GPU (the oracle is torch CPU).

Geometry: B = 3 clips of 3 s (96 000 samples, 128 mels x 300 frames).  Planes P0 ... P4 (stem output, then after each stride-2
block): 64x150, 32x75, 16x38, 8x19, 4x10 - every one a multiple of 4 (the MFMA routes run, not the generic 4-byte kernel) and
the smallest at which every block still has a plane of more than one row.  The bf16 cases use 7 s (MN: 64x350, 32x175,
16x88, 8x44, 4x22 - at width 1.0 the geometry that stores every block) and 5 s (DyMN: 64x250, 32x125, 16x63, 8x32, 4x16).

Blocks (indices into features[1:-1] / layers): SE gate in 3, 4, 5, 10 ... 14; stride 2 in 1, 3, 6, 12; 5x5 taps in 3, 4, 5, 12, 13,
14; ReLU in 0 ... 5, Hardswish from 6.  Input planes P0: 0, 1; P1: 2, 3; P2: 4, 5, 6; P3: 7 ... 12; P4: 13, 14; depthwise output
planes P0: 0; P1: 1, 2; P2: 3, 4, 5; P3: 6 ... 11; P4: 12, 13, 14.  Channels per width: tests/test_widths_cpu.py."""
import functools

import torch
import torch.nn.functional as F

from oracle import eat_oracle as O
from oracle import synth

B = 3
N_BLOCKS = 15
GEOMETRIES = {"3s": 96000, "5s": 160000, "7s": 224000}
MN_WIDTHS = (0.1, 0.2, 0.4, 0.5, 2.0, 3.0)
MN_B16_WIDTHS = (0.1, 0.5, 2.0)
DYMN_WIDTH = 0.4
DYMN_VARIANTS = {"all": {}, "replace_se": {"use_dy_blocks": "replace_se"}}

# ------------------------------------------------------------------------------------------------ eval plan (mn.run_block)
# fused: blocks on eat_mbconv_fwd / eat_fused_expand_dw_fwd.  csrc/irb.hip:irb_dispatch has instantiations for ReLU blocks
# with C_in = 16 (3x3 / stride 2) or C_in = 24 (3x3 / stride 1, 5x5 / stride 2) only; the ReLU blocks with expand conv read
# 8 channels at 0.1 / 0.2, 8 / 16 at 0.4 (the 16-channel ones are 3x3 / stride 1 and 5x5), 8 / 16 / 24 at 0.5 (24: blocks 4, 5 -
# 5x5 / stride 1), 32 / 48 / 80 at 2.0 and 48 / 72 / 120 at 3.0: ops.block_fused_supported admits NO block at any of these widths.
# The stem has 8 / 32 / 48 channels, mn.fold_front wants 16: eat_front_fwd never runs.
# expand_dw: blocks on eat_expand_dw_bf16_fwd (ops.expand_dw_eligible: 3x3 / stride 1, F <= 8, T <= 64, 4 <= C_in <= 128, and
# the expand layer on bf16x3, i.e. _PW_MODE auto and C_in >= 40): of the 3x3 / stride-1 blocks on the 8x19 plane (7 ... 11, C_in
# 8 8 8 8 16 | 16 16 16 16 24 | 32 32 32 32 48 | 40 40 40 40 56 | 160 ... 224 | 240 ... 336) block 11 at 0.4 and blocks 7 ... 11 at 0.5
# (blocks 13, 14 on 4x10 have 5x5 taps).  Under _PW_MODE fp32 none.  Every other block: one eat_dw_conv_fwd.
EVAL_PLAN = {0.1: dict(fused=0, expand_dw=0), 0.2: dict(fused=0, expand_dw=0), 0.4: dict(fused=0, expand_dw=1),
             0.5: dict(fused=0, expand_dw=5), 2.0: dict(fused=0, expand_dw=0), 3.0: dict(fused=0, expand_dw=0)}

# ------------------------------------------------------------------------------------------ training plan (mn_train.py)
# The columns of test_gpu_mn_geometry.PLAN_F32 on fp32 storage (3 s and 7 s alike: every plane is a multiple of 4, every SE
# plane - at most 16 x 88 = 1408 positions - below 2000):
#   cat      two-source data-gradient GEMMs: the blocks with expand conv - 14, at width 0.1 (blocks 0 ... 3 without one) 11
#   on_load  depthwise BatchNorm + activation on load in the project conv and its weight gradient: the blocks without SE
#            gate (0, 1, 2, 6, 7, 8, 9), C_exp % 8 == 0 at every width
#   merged   merged depthwise backward (eat_dw_conv_bwd_bn_g): eat_dw_bwd_merged_ok takes all of these planes, so every block
#            with merged_res_ok - all 15, except block 2 of width 0.1: residual, no expand conv, not the fused stem's consumer
#   separate the blocks on the separate depthwise-backward passes instead (eat_dw_conv_wgrad + eat_dw_conv_dgrad, no expand
#            conv: block 2 of width 0.1)
PLAN_F32 = {w: dict(cat=14, on_load=7, merged=15, separate=0) for w in MN_WIDTHS}
PLAN_F32[0.1] = dict(cat=11, on_load=7, merged=14, separate=1)

# act_storage = 'bf16' at 7 s: ops.b16_block_ok depends on the planes, k and stride only (C_exp % 8 == 0 everywhere) and takes
# all 15 blocks, as at width 1.0; mn_train._block_fwd additionally wants merged_res_ok - block 2 of width 0.1 keeps fp32 storage
B16_BLOCKS = {0.1: tuple(i for i in range(N_BLOCKS) if i != 2), 0.5: tuple(range(N_BLOCKS)), 2.0: tuple(range(N_BLOCKS))}
# ... and the step's counts (columns of test_gpu_mn_geometry.PLAN_B16).  cat16: the stored blocks with expand conv and
# C_exp % 32 == 0 (the others take two single-source GEMMs):
#   0.1: C_exp 16 16 24 24 24 24 48 64 64 96 96 in 4 ... 14 -> 11, 12, 13, 14;  0.5: 32 40 40 64 64 120 104 96 96 240 336 336 480 480 in
#   1 ... 14 -> 1, 4, 5, 8, 9, 13, 14;  2.0: 128 144 144 240 240 480 400 368 368 960 1344 1344 1920 1920 -> 1, 6, 10, 11, 12, 13, 14
# on_load16: the stored blocks without SE gate; at 0.1 block 2 (not stored) stays on the fp32 forms: on_load 1, separate 1
PLAN_B16 = {
    0.1: dict(cat=0, cat16=4, on_load=1, on_load16=6, merged=0, merged16=14, stats16=14, separate=1),
    0.5: dict(cat=0, cat16=7, on_load=0, on_load16=7, merged=0, merged16=15, stats16=15, separate=0),
    2.0: dict(cat=0, cat16=7, on_load=0, on_load16=7, merged=0, merged16=15, stats16=15, separate=0),
}

# ------------------------------------------------------------------------------------------------ DyMN 0.4 (dymn_train.py)
# 3 s: To <= 512 and the merged depthwise backward takes every plane: all 15 blocks on the fused block step, none unfused.
# No K-concat GEMM (eat_pw_conv_kcat_fwd) in eval or training: ops.kcat_eligible wants an arithmetic other than fp32 (eval
# runs under the default, 'fp32'), C_in % 32 == 0 and C_out C_in > (C_in + C_out) S; under 'auto' the convs from C_in = 40 on
# take the bf16x3 per-sample pack first, and the C_in = 32 ones (forward: project of 2, 3, expand of 7 ... 10; data gradient:
# expand of 2, 3, project of 6 ... 9) have at most 32 x 192 weights against (32 + 192) x 152 activations.
# 5 s, act_storage = 'bf16': ops.dyn_b16_block_ok as the MN rule at 5 s (test_gpu_mn_geometry.B16_BLOCKS) - 64x250 tiles in 0
# (no expand conv: T > 128, 3x3 / stride 1) and 1, 4x16 plane kernels in 13, 14; C_in, C_out % 4 == 0 and C_exp % 8 == 0 everywhere.
DYMN_B16_BLOCKS_5S = (0, 1, 13, 14)


def rel(a, b):
    a, b = a.detach().double().cpu().reshape(-1), b.detach().double().cpu().reshape(-1)
    return float((a - b).norm() / max(1e-30, float(b.norm())))


def to_double(sd):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in sd.items()}


def grad_state(sd, double=False):
    return {k: ((v.double() if double else v.clone()).requires_grad_(True) if v.is_floating_point() and "running" not in k
                else (v.double() if double and v.is_floating_point() else v.clone())) for k, v in sd.items()}


def labels_and_mask(width):
    """Labels (seed 5) and the drop mask (seed 6) over the head's hidden layer: make_divisible(1280 x width) units."""
    y = (torch.rand(B, 527, generator=torch.Generator().manual_seed(5)) < 0.01).float()
    keep = (torch.rand(B, O.block_table(width)[1], generator=torch.Generator().manual_seed(6)) < 0.8).float()
    return y, keep


@functools.lru_cache(maxsize=None)
def clips(geo):
    n = GEOMETRIES[geo]
    x = O.mel_forward(synth.parity_clips(n, seed=7)[:B]).unsqueeze(1)
    assert x.shape == (B, 1, 128, n // 320)
    return x


def mn_fwd(width):
    return lambda s, xm, **k: O.mn_forward(s, xm, width_mult=width, **k)


def dymn_fwd(variant="all", temperature=1.0):
    return lambda s, xm, **k: O.dymn_forward(s, xm, width_mult=DYMN_WIDTH, temperature=temperature, **DYMN_VARIANTS[variant], **k)


@functools.lru_cache(maxsize=None)
def mn_case(width, geo):
    """(x (B, 1, 128, frames) fp32, state calibrated on that input: running statistics = its batch statistics)."""
    x = clips(geo)
    return x, synth.calibrate(synth.synth_state(synth.mn_shapes(width), seed=0), mn_fwd(width), x)


@functools.lru_cache(maxsize=None)
def mn_eval_ref(width, geo, batch):
    """fp64 oracle in eval mode on the first `batch` clips: (logits, 17 feature maps)."""
    x, sd = mn_case(width, geo)
    with torch.no_grad():
        return mn_fwd(width)(to_double(sd), x[:batch].double(), return_fmaps=True)


def _step(fwd, width, sd, x, double):
    y, keep = labels_and_mask(width)
    sdr = grad_state(sd, double=double)
    stats = {}
    cast = (lambda t: t.double()) if double else (lambda t: t)
    logits, _ = fwd(sdr, cast(x), train=True, stats=stats, drop_mask=cast(keep))
    loss = F.binary_cross_entropy_with_logits(logits, cast(y))
    loss.backward()
    return sdr, stats, logits.detach(), loss.detach()


@functools.lru_cache(maxsize=None)
def mn_fp64_step(width, geo):
    """fp64 autograd over the oracle: (state with .grad, running buffers, logits, loss)."""
    x, sd = mn_case(width, geo)
    return _step(mn_fwd(width), width, sd, x, True)


@functools.lru_cache(maxsize=None)
def mn_fp32_step(width, geo):
    """The oracle as it stands (fp32): the anchor of the bf16 criteria."""
    x, sd = mn_case(width, geo)
    return _step(mn_fwd(width), width, sd, x, False)


@functools.lru_cache(maxsize=None)
def dymn_case(geo, variant="all"):
    from efficientat_amd.dymn import get_model
    import contextlib
    import io
    x = clips(geo)
    kw = DYMN_VARIANTS[variant]
    if kw:
        with contextlib.redirect_stdout(io.StringIO()):
            shapes = synth.shapes_of(get_model(width_mult=DYMN_WIDTH, **kw))
    else:
        shapes = synth.dymn_shapes(DYMN_WIDTH)
    return x, synth.calibrate(synth.synth_state(shapes, seed=0), dymn_fwd(variant), x)


@functools.lru_cache(maxsize=None)
def dymn_eval_ref(geo, variant):
    x, sd = dymn_case(geo, variant)
    with torch.no_grad():
        return dymn_fwd(variant)(to_double(sd), x.double(), return_fmaps=True)


@functools.lru_cache(maxsize=None)
def dymn_fp64_step(geo):
    """One step at DynamicConv temperature 30, fp64 autograd over the oracle."""
    x, sd = dymn_case(geo)
    return _step(dymn_fwd(temperature=30.0), DYMN_WIDTH, sd, x, True)


@functools.lru_cache(maxsize=None)
def dymn_fp32_step(geo):
    x, sd = dymn_case(geo)
    return _step(dymn_fwd(temperature=30.0), DYMN_WIDTH, sd, x, False)
