"""Train-mode forward / backward of the MN trunk on the HIP kernels.

The reference trains through autograd over ~210 per-op launches (`ex_audioset.py:147-199`,
`models/mn/model.py:212-231`).  Here ONE `torch.autograd.Function` owns the whole network: its forward runs the
train-mode launch plan, its backward the hand-derived reverse plan and returns the gradient of
every parameter, so `loss.backward(); optimizer.step()` in the caller are unchanged.

The plan, stage by stage (a `_<stage>_fwd` / `_<stage>_bwd` pair each; csrc/train_fuse.hip has the algebra):
  * stem: no pre-activation tensor - BatchNorm statistics from the Gram matrix of the log-mel's 3x3 patches, BatchNorm +
    Hardswish in the conv's epilogue; backward in one pass over the block-0 gradient.
  * expand conv: statistics from the Gram matrix of the block input (no pass over z_e), BatchNorm + activation evaluated on
    load by the depthwise conv; backward WITHOUT dz_e: the depthwise backward's epilogue writes g = dy_e * act'(.) and
    sum g, the weight / data gradients follow from wgrad(g, x) and one two-source GEMM.
  * depthwise conv: statistics from the conv's epilogue; BatchNorm + activation (+ SE scale) evaluated on load by the project
    conv and its weight gradient; backward: weight gradient, data gradient, the BatchNorm's own backward and the expand
    activation's derivative as ONE kernel on the large planes.
  * project / last conv: statistics in the 1x1 conv's epilogue; the project data-gradient GEMM's epilogue takes the channel
    sums of the depthwise BatchNorm backward in blocks without SE gate.  SE gate, mlp head: two launches per backward.
Every stage keeps the separate-pass form for what its fused kernels do not cover: frozen BatchNorm, planes that are not a
multiple of 4, blocks without expand conv, SE blocks on small planes, a hipGraph capture before the pack plan exists.
`model.act_storage = "bf16"` stores a block's wide tensors (z_e, z_d, y_d; backward: dxs, g) in bf16.  Tiny (B, C)-shaped
glue of the SE gate and the head uses torch elementwise ops; every GEMM / conv / reduction over activations runs in
libeat_hip.so.
"""
from collections import namedtuple
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from . import _lib, ops
from .dp import GradReducer

NONE, RELU, HSWISH, SIGMOID = ops.ACT_NONE, ops.ACT_RELU, ops.ACT_HSWISH, ops.ACT_SIGMOID
_TRAIN_V = 2                         # (bench.py reports it; the round-2 plan behind EAT_TRAIN_V=1 was removed in round 4)
# bf16-storage plan: bf16 copy of the narrow operand of the expand / data-gradient conv from this expanded width (_cast_narrow)
_CAST_NARROW_MIN_CEXP = 200
# The depthwise BatchNorm's backward sums leave the project data-gradient GEMM's epilogue (blocks without SE gate; same-box
# A/B of the mn10 step: 24.29 / 24.17 ms without, 23.97 / 23.96 ms with; mn40 bf16 storage: 42.19 vs 42.17 ms - there the
# reduce pass reads 2-byte tensors and the epilogue saves little)
# ... from this size of the depthwise output on (same-box microbenchmarks at B = 256, conv + reduce pass -> conv with the
# epilogue + finish: 16 -> 16 at 64 x 500 387 -> 299 us, 24 -> 64 at 32 x 250 352 -> 280, 24 -> 72 378 -> 332; the 8 x 63 layers
# 80 -> 240 / 200 / 184: 89 -> 110, 76 -> 87, 67 -> 65 us - their reduce pass is cheaper than the epilogue's extra phase)
_GSTATS_MIN_ELEMS = 1 << 26


_zeros, _ones = ops.zeros_vec, ops.ones_vec           # cached constant vectors (the bias pointer of the train-mode convs)


def _prepack_plan(model):
    """All weight packs of the trunk's 1x1 convs (forward and data-gradient forms) from one launch per step
    (ops.PrepackPlan); None while a hipGraph is being captured before the plan exists, or for geometries it does not take."""
    plan = getattr(model, "_eat_prepack_plan", None)
    if plan is not None and not plan.stale():
        return plan
    if torch.cuda.is_current_stream_capturing():
        return None
    entries = []
    for bi, blk in enumerate(model.features[1:-1]):
        if blk.i_expand is not None:
            entries.append((("e", bi), blk.block[blk.i_expand][0].weight, False))
        pw = blk.block[blk.i_proj][0].weight
        entries += [(("p", bi), pw, False), (("pt", bi), pw, True)]
    lw = model.features[-1][0].weight
    entries += [(("l",), lw, False), (("lt",), lw, True)]
    try:
        plan = ops.PrepackPlan(entries)
    except _lib.EatHipError:                              # odd channel counts: per-matrix packs (which check for themselves)
        plan = None
    model._eat_prepack_plan = plan
    return plan


def _pk(plan, key, w, trans=False):
    return plan.get(key) if plan is not None else ops.pw_prepack(w.flatten(1), trans=trans)


class _GradSink:
    """`sink[name] = grad` forwards to GradReducer.push; `finish()` returns the (averaged) gradients."""

    def __init__(self, reducer):
        self.reducer = reducer

    def __setitem__(self, name, grad):
        self.reducer.push(name, grad)

    def alloc(self, name, like):
        """Memory for the gradient of parameter `like` inside the reducer's flat bucket buffer (zero-filled, shape of the 2-D
        weight matrix), or None when the pass is not bucketed - the producer then allocates for itself (dp.GradReducer)."""
        return self.reducer.alloc(name, (like.shape[0], like.numel() // like.shape[0]), like.device)

    def finish(self):
        return self.reducer.finish()


class _BnSums:
    """The fp64 channel sums (dbeta | dgamma) of every BatchNorm backward of a pass in ONE zeroed buffer: each layer reserves
    its (2C,) slice, and `flush` converts all of them to fp32 by one launch and hands dgamma / dbeta to the sink together."""

    def __init__(self, model, dev):
        total = 2 * sum(m.num_features for m in model.features.modules() if isinstance(m, torch.nn.BatchNorm2d))
        self.buf = ops.zero_arena.zeros((total,), torch.float64, dev)
        self.reg = []

    def reserve(self, C, pre):           # the slice of BatchNorm `pre` (`pre`.weight / `pre`.bias, C channels)
        off = sum(2 * r[1] for r in self.reg)
        self.reg.append((pre, C, off))
        return self.buf[off:off + 2 * C]

    def unreserve(self, pre):            # the kernel the slice reserved last was meant for declined: the next one takes it
        if self.reg and self.reg[-1][0] == pre:
            self.reg.pop()

    def flush(self, g):
        if self.reg:
            sf = self.buf.float()
            for pre, C, off in self.reg:
                g[pre + ".weight"], g[pre + ".bias"] = sf[off + C:off + 2 * C], sf[off:off + C]


def _act_storage_bf16(model):
    """True when the step stores its wide activations in bf16 (model.act_storage, mn.py); checks the combination."""
    st = getattr(model, "act_storage", "fp32")
    if st == "fp32":
        return False
    if st != "bf16":
        raise _lib.EatHipError(f"act_storage must be 'fp32' or 'bf16' (got {st!r})")
    if ops.precision.mode != "bf16":
        raise _lib.EatHipError("act_storage='bf16' needs train_precision='bf16' (plain bf16 GEMM operands): the split-operand "
                               f"kernels read fp32 activations (train_precision={ops.precision.mode!r})")
    return True


def _cast_narrow(cnf, x=None):
    """bf16-storage plan: hand the expand / data-gradient 1x1 conv of the widest blocks a bf16 COPY of its narrow fp32 operand
    (bit-identical results - the kernel rounds the operand the same way; measured on MI355X at B = 128: 320 -> 1920 at S = 504
    209 -> 144 us, 448 -> 2688 324 -> 238 us, 640 -> 3840 at S = 128 123 -> 91 us, 160 -> 960 at S = 2000 275 -> 220 us,
    64 -> 256 at S = 32000 667 -> 528 us; same-box A/B of the mn40 step with copies from expanded width 960 / 700 / 400 / 200:
    42.71 / 42.72 / 42.60 / 42.43 ms - every block with an expand conv).  The copy leaves the pass that produces the fp32 tensor
    (project BatchNorm forward / backward apply: `copy16`); `eat_cast_b16` (18 / 24 / 10 us on the shapes above) is the
    fallback when that pass ran on the fp32 kernels (frozen BatchNorm)."""
    return cnf.expanded_channels >= _CAST_NARROW_MIN_CEXP and (x is None or x.numel() % 8 == 0)


def _w_times_g(W, G):
    """T = W G (C_out, C_in) for a symmetric G (C_in, C_in), C_in % 4 == 0."""
    Co, Ci = W.shape
    if Ci % 4:
        return ops.linear(W, G, None, NONE)
    wp3 = ops.pw_prepack_bf16(W, None, split=True)
    return ops.pw_conv_bf16(G.view(1, Ci, Ci, 1), wp3, _zeros.get(Co, W.device), Co, NONE, split=True).view(Co, Ci)


def _pw_conv_bn(x, wp, Co, bn, tf=None, in_scale=None):
    """z = W x [of act(tf_a x + tf_b) * in_scale] and the state of the BatchNorm that follows: the batch statistics leave
    the conv's epilogue (ops.pw_conv_stats: no pass over z) where that exists and the layer is in training mode."""
    if bn.training:
        z, parts = ops.pw_conv_stats(x, wp, Co, tf=tf, in_scale=in_scale)
        if z is not None:
            return z, ops.bn_state_from_partials(parts, bn, z.numel() // Co)
    if tf is not None:
        z = ops.pw_conv_tf(x, tf, wp, _zeros.get(Co, x.device), Co, NONE, in_scale=in_scale)
    else:
        z = ops.pw_conv(x, wp, _zeros.get(Co, x.device), Co, NONE, in_scale=in_scale)
    return z, ops.bn_train_state(z, bn)


# ---- What the forward leaves for the backward, per stage.  Block records are dropped one by one as the backward passes them.
# stem: the log-mel input, BatchNorm state (a, b, mean, invstd), `fused` = the pre-activation tensor never existed
# (csrc/stem_train.hip); then z = that tensor (not fused), or Tm, sp = the Gram products of the 3x3 patches (fused, training)
_StemState = namedtuple("_StemState", "x st fused z Tm sp", defaults=(None, None, None))
# last 1x1 conv: input, output, BatchNorm state, plane size (the pool's divisor); head: what eat_mlp_head_bwd reads
_LastState = namedtuple("_LastState", "x z st S")
_HeadState = namedtuple("_HeadState", "feat u h2 drop_mask")


@dataclass
class _BlockState:
    inp: torch.Tensor                     # block input (fp32)
    b16: bool                             # this block's wide tensors (z_e, z_d, y_d; backward: dxs, g) are bf16 in HBM
    merged_res_ok: bool                   # the merged depthwise backward can serve the block's residual connection
    z_e: torch.Tensor = None              # expand conv (all five None in a block without one): its output,
    W_e: torch.Tensor = None              # the weights its statistics and backward coefficients describe (`_expand_weights`),
    st_e: tuple = None                    # its BatchNorm state (a, b, mean, invstd),
    Tm: torch.Tensor = None               # T = W Gc (None with a frozen BatchNorm)
    sx: torch.Tensor = None               # and the channel sums of the block input
    z_d: torch.Tensor = None              # depthwise conv output
    st_d: tuple = None                    # and its BatchNorm state
    on_load: bool = False                 # y_d = act(BN(z_d)) is evaluated on load by the project conv (y_d is None)
    y_d: torch.Tensor = None
    has_se: bool = False                  # squeeze-excitation gate:
    pool: torch.Tensor = None             # squeeze sums of y_d (B, C_exp),
    h: torch.Tensor = None                # hidden layer
    scale: torch.Tensor = None            # and the gate (None without SE)
    z_p: torch.Tensor = None              # project conv output
    st_p: tuple = None                    # and its BatchNorm state


# the pass: ops.PrepackPlan (or None), its run count at the forward, the records above (head: None in trunk mode, it ran outside)
_Saved = namedtuple("_Saved", "plan plan_run stem blocks last head")


# ---- stem (3x3 / stride 2 conv + BatchNorm + Hardswish)
def _stem_fwd(stem, x, need_sx):
    """-> (state, y, channel sums of y for the Gram statistics of a first block with expand conv - `need_sx` - or None)."""
    B, dev, C0 = x.shape[0], x.device, stem[0].out_channels
    W0 = stem[0].weight.reshape(C0, 9)
    if not need_sx:
        # the pre-activation stem tensor never exists: statistics from the Gram matrix of the log-mel's 3x3 patches,
        # BatchNorm + Hardswish in the conv's epilogue (csrc/stem_train.hip)
        Fo, To = (x.shape[2] - 1) // 2 + 1, (x.shape[3] - 1) // 2 + 1
        if stem[1].training:
            Tm0, sp0 = ops.stem_gram(x, W0)
            st0 = ops.gram_bn_state(Tm0, W0, sp0, stem[1], B * Fo * To)
        else:
            Tm0, sp0, st0 = None, None, ops.bn_frozen_state(stem[1])
        return _StemState(x, st0, True, None, Tm0, sp0), ops.stem_conv(x, W0 * st0[0].unsqueeze(1), st0[1], HSWISH), None
    z0 = ops.stem_conv(x, W0, _zeros.get(C0, dev), NONE)
    st0 = (ops.bn_state_from_partials(ops.bn_stats_partial(z0), stem[1], z0.numel() // C0) if stem[1].training
           else ops.bn_frozen_state(stem[1]))
    pool_c = torch.empty((B, C0), device=dev)
    y = ops.bn_act_fwd(z0, st0[0], st0[1], HSWISH, pool=pool_c)
    return _StemState(x, st0, False, z0), y, ops.col_sum(pool_c)


def _stem_bwd(stem, sv, dout, dout2, g):
    """dout2: second summand of the gradient (the residual branch of a first block without expand conv), added on load."""
    st0 = sv.st
    if sv.fused:
        # one pass over the block-0 gradient: g = dout * hswish'(.) from the log-mel window, Gx = sum g p^T, sum g
        W0 = stem[0].weight.reshape(-1, 9)
        Gx, gparts = ops.stem_bwd(dout, sv.x, W0, st0[0], st0[1], HSWISH, dy2=dout2)
        frozen = getattr(st0[2], "_eat_frozen", False)
        Tm0, sp0 = (Gx, _zeros.get(9, dout.device)) if frozen else (sv.Tm, sv.sp)      # frozen: not read (m1 = m2 = 0)
        dW, dgam, dbet = ops.expand_bwd_coef(W0, Gx, Tm0, sp0, gparts, st0[0], st0[2], st0[3], dout.numel() // W0.shape[0],
                                             frozen=frozen, need_dx=False)[:3]
        g["features.0.1.weight"], g["features.0.1.bias"] = dgam, dbet
        g["features.0.0.weight"] = dW.view_as(stem[0].weight)
    else:
        dz0, dgam, dbet = ops.bn_act_bwd(dout, sv.z, *st0, HSWISH)
        g["features.0.1.weight"], g["features.0.1.bias"] = dgam, dbet
        g["features.0.0.weight"] = ops.dw_conv_wgrad(dz0, sv.x, 3, 2).view_as(stem[0].weight)


# ---- inverted residual block (mn/block_types.py:177-181): expand / depthwise / SE / project
def _act(blk):
    return HSWISH if blk.cnf.use_hs else RELU


def _expand_weights(conv):
    """The (C_exp, C_in) matrix that the expand conv multiplies by: under precision 'bf16' its kernels round the weights to
    bf16, so the BatchNorm statistics taken from the Gram matrix and the backward's coefficients must describe W rounded -
    with the fp32 weights they describe a product the conv never forms (relative 2^-9 / sqrt(C_in) per channel, which the
    narrow models, C_in = 8 ... 40 at widths 0.1 ... 0.5, do not average away)."""
    W = conv.weight.flatten(1)
    return W.bfloat16().float() if ops.precision.mode == "bf16" else W


def _expand_fwd(blk, bi, rec, inp16, sx, plan, store16):
    """Expand conv; its BatchNorm + activation are left to the depthwise conv: -> tf = (a, b, act) to evaluate on load."""
    cnf, cna, inp = blk.cnf, blk.block[blk.i_expand], rec.inp
    W = rec.W_e = _expand_weights(cna[0]) if cna[1].training else cna[0].weight.flatten(1)
    n_e = inp.shape[0] * inp.shape[2] * inp.shape[3]
    if cna[1].training:
        # centred Gram matrix of the block input (reproducible; x - mean on load: the variance is not a
        # difference of two (mean / std)^2-times larger sums)
        exact = ops.precision.mode == "fp32"
        G = ops.gram(inp, exact=exact, sx=sx, plain_bf16=store16)
        if W.shape[1] <= 192:
            Tm, st_e = ops.gram_bn_state_g(G, W, sx, cna[1], n_e, centered=True)   # T = W Gc and the BatchNorm state, one launch
        else:
            # wide inputs (mn40: up to 640 channels): every block of the one-launch form would stream the whole
            # G from L2 (C_out x C_in^2 floats: 0.79 ms at 3840 x 640) - W G on the matrix cores instead: as the
            # 1x1 conv of the "image" G (1, C_in, C_in, 1) with W on the split-operand bf16x3 kernel (fp32-class
            # products whatever the step's precision: T feeds the BatchNorm variance; round 4 ran the K-split
            # `linear` kernel here, 15 TFLOP/s on 3840 x 640 x 640)
            Tm = ops.linear(W, G, None, NONE) if exact else _w_times_g(W, G)
            st_e = ops.gram_bn_state(Tm, W, sx, cna[1], n_e, centered=True)
    else:
        Tm, st_e = None, ops.bn_frozen_state(cna[1])
    wp, Ce = _pk(plan, ("e", bi), cna[0].weight), cnf.expanded_channels
    if rec.b16:
        x16 = inp16 if inp16 is not None else (ops.cast_b16(inp) if _cast_narrow(cnf, inp) else inp)
        rec.z_e = ops.pw_conv_b16(x16, wp, _zeros.get(Ce, inp.device), Ce, NONE, out_b16=True)
    else:
        rec.z_e = ops.pw_conv(inp, wp, _zeros.get(Ce, inp.device), Ce, NONE)
    rec.st_e, rec.Tm, rec.sx = st_e, Tm, sx
    return st_e[0], st_e[1], _act(blk)


def _expand_bwd(blk, i, rec, g_e, gparts, res_grad, wgrad, g):
    """Expand conv + BatchNorm + activation without dz_e (csrc/train_fuse.hip): g = dy_e * act'(.) and sum g left the
    depthwise backward; dW / dx follow from Gx = sum g x^T and the forward's Gram products.  -> gradient of the block input
    (incl. the residual branch's `res_grad`)."""
    cnf, cna, inp, st_e, b16 = blk.cnf, blk.block[blk.i_expand], rec.inp, rec.st_e, rec.b16
    pre = f"features.{i + 1}.block.{blk.i_expand}"
    Ci, Ce = cnf.input_channels, cnf.expanded_channels
    W = rec.W_e
    frozen = getattr(st_e[2], "_eat_frozen", False)
    n_e = inp.shape[0] * inp.shape[2] * inp.shape[3]
    Gx = wgrad(g_e, inp)
    Tm, sx = (Gx, st_e[2]) if frozen else (rec.Tm, rec.sx)      # frozen: not read (m1 = m2 = 0)
    o_e = g.alloc(pre + ".0.weight", cna[0].weight)
    # dx = [WaT | M] [g ; x] + c0 (+ residual-branch gradient) as ONE two-source GEMM where its kernel takes the geometry (g read
    # from its bf16 storage: its channels must fill whole k-chunks), its weight pack and bias from ONE launch after the coefficient
    # kernel - eat_expand_bwd_wcat (round 6: was transposes + pack + M GEMM + cat + pack; same-box A/B against that five-launch
    # form: mn10 24.23 -> 24.06 ms, mn40 bf16 42.59 -> 41.89 ms)
    cat = not frozen and (Ce % 32 == 0 if b16 else (inp.shape[2] * inp.shape[3]) % 4 == 0)
    if cat:
        dW, dgam, dbet, wcat, c0 = ops.expand_bwd_coef_cat(W, Gx, Tm, sx, gparts, st_e[0], st_e[2], st_e[3], n_e,
                                                           centered=True, dW_out=o_e)
    else:
        dW, dgam, dbet, WaT, M, c0 = ops.expand_bwd_coef(W, Gx, Tm, sx, gparts, st_e[0], st_e[2], st_e[3], n_e,
                                                         frozen=frozen, centered=not frozen, dW_out=o_e)
    g[pre + ".1.weight"], g[pre + ".1.bias"] = dgam, dbet
    g[pre + ".0.weight"] = dW.view_as(cna[0].weight)
    if cat:
        return (ops.pw_conv_b16(g_e, wcat, c0, Ci, NONE, x2=inp, res=res_grad) if b16
                else ops.pw_conv_cat(g_e, inp, wcat, c0, Ci, NONE, res=res_grad))
    t = res_grad
    if not frozen:                                                  # M x + c0 (+ residual-branch gradient)
        t = ops.pw_conv(inp, ops.pw_prepack(M), c0, Ci, NONE, res=res_grad)
    conv = ops.pw_conv_b16 if b16 else ops.pw_conv
    return conv(g_e, ops.pw_prepack(WaT), _zeros.get(Ci, inp.device), Ci, NONE, res=t)


def _dw_fwd(blk, rec, tf):
    """Depthwise conv of act(tf_a z_e + tf_b) - or of the block input without expand conv - with its batch statistics from
    the conv's epilogue, then y_d = act(BN(z_d)) and the SE squeeze where a pass over z_d is needed at all."""
    cnf, cna, act = blk.cnf, blk.block[blk.i_dw], _act(blk)
    k, Ce = cnf.kernel, cnf.expanded_channels
    src = rec.inp if tf is None else rec.z_e
    w_d = cna[0].weight.reshape(-1, k * k)
    if cna[1].training:
        z_d, parts = ops.dw_conv_stats(src, w_d, k, cnf.stride, tf=tf, out_b16=rec.b16)
        st_d = ops.bn_state_from_partials(parts, cna[1], z_d.numel() // Ce)
    else:
        if tf is not None:
            z_d = ops.dw_conv_tf(src, tf[0], tf[1], act, w_d, _zeros.get(Ce, src.device), k, cnf.stride)
        else:
            z_d = ops.dw_conv(src, w_d, _zeros.get(Ce, src.device), k, cnf.stride, NONE)
        st_d = ops.bn_frozen_state(cna[1])
    S_d = z_d.shape[2] * z_d.shape[3]
    pool = torch.empty((z_d.shape[0], Ce), device=src.device) if rec.has_se else None
    # on-load BatchNorm + activation in the project conv: saves the write AND the read of y_d in blocks without
    # SE, only the write in SE blocks (the squeeze needs a pass anyway) - there it pays on the large planes only
    # (measured: on the 8x63 / 4x32 SE blocks the transformed GEMM and weight gradient cost more than the write)
    on_load = ops.pw_tf_eligible(Ce, S_d) and (not rec.has_se or S_d >= 2000)
    if rec.has_se or not on_load:
        rec.y_d = ops.bn_act_fwd(z_d, st_d[0], st_d[1], act, pool=pool, write=not on_load)
    rec.z_d, rec.st_d, rec.on_load, rec.pool = z_d, st_d, on_load, pool


def _dw_bwd_merged(blk, i, rec, dxs, sums, gate, g, bn):
    """Large planes: dz_d is never written - ONE kernel evaluates the BatchNorm + activation backward of the depthwise output on
    load from (dxs, z_d) and the channel sums `sums` of the reduce pass (None: not taken yet) and writes the weight gradient and
    -> (g = dy_e * act'(.), partial sums of g) for the expand stage, or (gradient of the block input, None) without expand conv."""
    cnf, cna, act = blk.cnf, blk.block[blk.i_dw], _act(blk)
    pre = f"features.{i + 1}.block.{blk.i_dw}"
    k, Ce = cnf.kernel, cnf.expanded_channels
    gscale, gadd, se_P = gate
    if sums is None:                                   # (else they left the project data-gradient GEMM's epilogue)
        sums = ops.bn_act_bwd_sums(dxs, rec.z_d, *rec.st_d, act, gscale=gscale, gadd=gadd, se_P=se_P,
                                   sums=bn.reserve(Ce, pre + ".1"))[0]
    w_d = cna[0].weight.reshape(-1, k * k)
    # the conv's input: the block input as it is, or act(a z_e + b) of the expand conv evaluated on load
    x, a, b, in_act = ((rec.inp, _ones.get(Ce, dxs.device), _zeros.get(Ce, dxs.device), NONE) if blk.i_expand is None
                       else (rec.z_e, rec.st_e[0], rec.st_e[1], act))
    grad, gparts, dw_d = ops.dw_conv_bwd_bn_g(dxs, rec.z_d, rec.st_d, act, sums, w_d, x, a, b, in_act, k, cnf.stride,
                                              gscale=gscale, gadd=gadd, want_gsum=blk.i_expand is not None)
    g[pre + ".0.weight"] = dw_d.view_as(cna[0].weight)
    return grad, gparts


def _dw_bn_bwd(blk, i, rec, dxs, gate, bn):
    """Where the merged kernel does not run: the depthwise BatchNorm + activation backward as a pass of its own -> dz_d."""
    pre = f"features.{i + 1}.block.{blk.i_dw}"
    gscale, gadd, se_P = gate
    slot = bn.reserve(blk.cnf.expanded_channels, pre + ".1")
    if se_P is not None:
        return ops.bn_act_bwd_se(dxs, rec.z_d, *rec.st_d, _act(blk), se_P, gscale, gadd, sums=slot)[0]
    return ops.bn_act_bwd(dxs, rec.z_d, *rec.st_d, _act(blk), gscale=gscale, gadd=gadd, sums=slot)[0]


def _dw_conv_bwd(blk, i, rec, dz_d, res_grad, g):
    """... and the depthwise conv's backward from dz_d: -> what `_dw_bwd_merged` returns."""
    cnf, cna, act = blk.cnf, blk.block[blk.i_dw], _act(blk)
    pre, k = f"features.{i + 1}.block.{blk.i_dw}", cnf.kernel
    w_d = cna[0].weight.reshape(-1, k * k)
    if blk.i_expand is not None:
        # weight gradient, data gradient and the activation-derivative epilogue from ONE pass over dz_d and z_e
        g_e, gparts, dw_d = ops.dw_conv_bwd_g(dz_d, w_d, rec.z_e, rec.st_e[0], rec.st_e[1], act, k, cnf.stride)
        g[pre + ".0.weight"] = dw_d.view_as(cna[0].weight)
        return g_e, gparts
    g[pre + ".0.weight"] = ops.dw_conv_wgrad(dz_d, rec.inp, k, cnf.stride).view_as(cna[0].weight)
    return ops.dw_conv_dgrad(dz_d, w_d, tuple(rec.inp.shape), k, cnf.stride, res=res_grad), None


def _se_fwd(blk, rec):
    """Squeeze-excitation gate (mn/block_types.py:72-83) from the squeeze sums the depthwise stage took."""
    se = blk.block[blk.i_se].conc_se_layers[0]
    rec.h = ops.linear(rec.pool, se.fc1.weight, se.fc1.bias, RELU, 1.0 / (rec.z_d.shape[2] * rec.z_d.shape[3]))
    rec.scale = ops.linear(rec.h, se.fc2.weight, se.fc2.bias, SIGMOID)


def _se_bwd(blk, i, rec, dxs, g):
    """-> (gscale, gadd, se_P): the gradient arriving at y_d is dxs * gscale + gadd (per plane); se_P the plane sums."""
    se = blk.block[blk.i_se].conc_se_layers[0]
    sp = f"features.{i + 1}.block.{blk.i_se}.conc_se_layers.0"
    # one pass over (dxs, z_d) for the gate gradient AND the BatchNorm-backward plane sums
    st_d = rec.st_d
    se_P = ops.se_bn_bwd_partials(dxs, rec.z_d, st_d[0], st_d[1], st_d[2], _act(blk))
    # the gate MLP's backward as two launches (csrc/se_train.hip)
    o2, o1 = g.alloc(sp + ".fc2.weight", se.fc2.weight), g.alloc(sp + ".fc1.weight", se.fc1.weight)
    dW1, db1, dW2, db2, gadd = ops.se_mlp_bwd(se_P[0], rec.scale, rec.h, rec.pool, se.fc1.weight, se.fc2.weight,
                                              rec.z_d.shape[2] * rec.z_d.shape[3], dW1_out=o1, dW2_out=o2)
    g[sp + ".fc2.weight"], g[sp + ".fc2.bias"] = dW2, db2
    g[sp + ".fc1.weight"], g[sp + ".fc1.bias"] = dW1, db1
    return rec.scale, gadd, se_P


def _project_fwd(blk, bi, rec, nxt, plan):
    """Project conv of y_d (evaluated on load from z_d with rec.on_load) * SE gate, BatchNorm (no activation) + residual.
    -> (block output, its bf16 copy or None, its channel sums or None): the last two for a next block `nxt` with expand conv."""
    cnf, cna, inp = blk.cnf, blk.block[blk.i_proj], rec.inp
    Co, dev = cnf.out_channels, inp.device
    wp = _pk(plan, ("p", bi), cna[0].weight)
    src_p, tf_p = (rec.z_d, (rec.st_d[0], rec.st_d[1], _act(blk))) if rec.on_load else (rec.y_d, None)
    if not rec.b16:
        z_p, st_p = _pw_conv_bn(src_p, wp, Co, cna[1], tf=tf_p, in_scale=rec.scale)
    elif cna[1].training:
        # from the bf16-stored z_d / y_d, statistics in the epilogue; z_p too is stored in bf16 (statistics of the stored
        # values); the block output below is fp32
        z_p, parts = ops.pw_conv_b16(src_p, wp, _zeros.get(Co, dev), Co, NONE, tf=tf_p, in_scale=rec.scale, stats=True, out_b16=True)
        st_p = ops.bn_state_from_partials(parts, cna[1], z_p.numel() // Co)
    else:
        z_p = ops.pw_conv_b16(src_p, wp, _zeros.get(Co, dev), Co, NONE, tf=tf_p, in_scale=rec.scale)
        st_p = ops.bn_frozen_state(cna[1])
    need_sx = nxt is not None and nxt.i_expand is not None
    pool_c = torch.empty((inp.shape[0], Co), device=dev) if need_sx else None
    want16 = rec.b16 and z_p.dtype == torch.bfloat16 and need_sx and _cast_narrow(nxt.cnf)
    cur = ops.bn_act_fwd(z_p, st_p[0], st_p[1], NONE, res=inp if blk.use_res_connect else None, pool=pool_c, y_f32=True,
                         copy16=want16)
    cur, cur16 = cur if want16 else (cur, None)
    rec.z_p, rec.st_p = z_p, st_p
    return cur, cur16, ops.col_sum(pool_c) if need_sx else None


def _project_dgrad(blk, i, rec, dz_p, dz16, wpt, epi, bn):
    """dxs = W_p^T dz_p (stored in bf16 with rec.b16) -> (dxs, sums): with `epi`, the channel sums of the depthwise BatchNorm's
    backward from the GEMM's epilogue (ops.pw_conv_gstats) where its kernel takes the geometry, else None."""
    cnf, act, Ce, dev = blk.cnf, _act(blk), blk.cnf.expanded_channels, dz_p.device
    pre_d = f"features.{i + 1}.block.{blk.i_dw}.1"
    if rec.b16:
        if dz16 is None:
            dz16 = ops.cast_b16(dz_p) if _cast_narrow(cnf, dz_p) else dz_p
        gst = None
        if epi and dz16.dtype == torch.bfloat16 and rec.z_d.dtype == torch.bfloat16:
            gst = (rec.z_d, rec.st_d, act, bn.reserve(Ce, pre_d))
        dxs = ops.pw_conv_b16(dz16, wpt, _zeros.get(Ce, dev), Ce, NONE, out_b16=True, gstat=gst)
        return dxs if gst is not None else (dxs, None)
    if epi:
        dxs, sums = ops.pw_conv_gstats(dz_p, wpt, Ce, rec.z_d, rec.st_d, act, sums=bn.reserve(Ce, pre_d))
        if dxs is not None:
            return dxs, sums
        bn.unreserve(pre_d)
    return ops.pw_conv(dz_p, wpt, _zeros.get(Ce, dev), Ce, NONE), None


def _project_bwd(blk, i, rec, dout, merged, wgrad, g, bn, plan):
    """Project conv + BatchNorm (no activation; the residual branch passes dout through unchanged) -> (dxs, sums) of
    `_project_dgrad`: the gradient arriving at y_d * SE gate."""
    cnf, cna = blk.cnf, blk.block[blk.i_proj]
    pre = f"features.{i + 1}.block.{blk.i_proj}"
    want16 = rec.b16 and rec.z_p.dtype == torch.bfloat16 and _cast_narrow(cnf)
    dz_p = ops.bn_act_bwd(dout, rec.z_p, *rec.st_p, NONE, sums=bn.reserve(cnf.out_channels, pre + ".1"), copy16=want16)[0]
    dz_p, dz16 = dz_p if want16 else (dz_p, None)
    o_p = g.alloc(pre + ".0.weight", cna[0].weight)
    # (y_d = act(BN(z_d)) was evaluated on load in the forward: the same here)
    src, tf = (rec.z_d, (rec.st_d[0], rec.st_d[1], _act(blk))) if rec.on_load else (rec.y_d, None)
    g[pre + ".0.weight"] = wgrad(dz_p, src, x_scale=rec.scale, tf=tf, out=o_p).view_as(cna[0].weight)
    wpt = _pk(plan, ("pt", i), cna[0].weight, trans=True)
    # without an SE gate between the two, the channel sums of the depthwise BatchNorm's backward can leave the data-gradient
    # GEMM's epilogue (read by the merged depthwise backward only)
    epi = merged and not rec.has_se and rec.z_d.numel() >= _GSTATS_MIN_ELEMS
    return _project_dgrad(blk, i, rec, dz_p, dz16, wpt, epi, bn)


def _block_fwd(blk, bi, inp, inp16, sx, nxt, stem_fused, plan, store16):
    """-> (record, block output, its bf16 copy or None, its channel sums or None).  inp16: bf16 copy of `inp` (bf16-storage
    plan, _cast_narrow); sx: channel sums of `inp` (blocks with expand conv)."""
    cnf = blk.cnf
    # the backward's merged depthwise kernel has no residual input: of the residual blocks without expand conv it serves only the
    # fused stem's consumer (the stem's backward kernel adds the two gradients on load); any other - block 2 of the released
    # mn01 (width 0.1: 8 -> 8 -> 8, 3x3 / stride 1), or a custom inverted_residual_setting - takes the separate fp32 passes
    # there, which read fp32 tensors: no bf16 storage either (tests/test_gpu_widths.py pins both)
    merged_res_ok = blk.i_expand is not None or not blk.use_res_connect or (bi == 0 and stem_fused)
    # bf16 storage of this block's wide tensors (z_e, z_d, y_d; backward: dxs, g) where the kernels cover its geometry
    # (a block without expand conv: its depthwise conv reads the fp32 block input and its backward hands an fp32
    # gradient to the layer below - z_d, y_d and dxs are the bf16 tensors there)
    b16 = (store16 and blk.block[blk.i_dw][1].training
           and ops.b16_block_ok(inp.shape[0], cnf.expanded_channels, inp.shape[2], inp.shape[3], cnf.kernel, cnf.stride)
           and merged_res_ok)
    rec = _BlockState(inp, b16, merged_res_ok, has_se=blk.i_se is not None)
    tf = _expand_fwd(blk, bi, rec, inp16, sx, plan, store16) if blk.i_expand is not None else None
    _dw_fwd(blk, rec, tf)
    if rec.has_se:
        _se_fwd(blk, rec)
    return (rec,) + _project_fwd(blk, bi, rec, nxt, plan)


def _block_bwd(blk, i, rec, dout, g, bn, plan):
    """-> (dout, dout2): the gradient of the block input, as one tensor or - the fused stem's consumer - as two summands."""
    res_grad = dout if blk.use_res_connect else None
    wgrad = ops.pw_conv_wgrad_b16 if rec.b16 else ops.pw_conv_wgrad        # (one operand is the block's wide bf16 tensor)
    src = rec.inp if blk.i_expand is None else rec.z_e
    merged = rec.merged_res_ok and ops.dw_bwd_merged_ok(rec.z_d.shape, tuple(src.shape), blk.cnf.kernel, blk.cnf.stride)
    dxs, sums = _project_bwd(blk, i, rec, dout, merged, wgrad, g, bn, plan)
    gate = _se_bwd(blk, i, rec, dxs, g) if rec.has_se else (None, None, None)
    if merged:
        grad, gparts = _dw_bwd_merged(blk, i, rec, dxs, sums, gate, g, bn)
        del dxs
    else:
        dz_d = _dw_bn_bwd(blk, i, rec, dxs, gate, bn)
        del dxs
        grad, gparts = _dw_conv_bwd(blk, i, rec, dz_d, res_grad, g)
        del dz_d
    dout2 = None
    if blk.i_expand is not None:
        grad = _expand_bwd(blk, i, rec, grad, gparts, res_grad, wgrad, g)
    elif merged:
        dout2 = res_grad             # (the merged kernel has no residual input: the stem's backward adds the two on load)
    return grad, dout2


# ---- last 1x1 conv + BatchNorm + Hardswish, and the mlp head (mn/model.py:186-194)
def _last_fwd(last, x, plan):
    z_l, st_l = _pw_conv_bn(x, _pk(plan, ("l",), last[0].weight), last.out_channels, last[1])
    return _LastState(x, z_l, st_l, z_l.shape[2] * z_l.shape[3])


def _last_bwd(last, nm, sv, dy, dft, g, bn, plan):
    """dft None (trunk mode): dy is the gradient w.r.t. the last feature map; else dft is the gradient w.r.t. the pooled
    features (the pool's gradient is a per-plane constant).  -> gradient of the last block's output."""
    x_l, z_l, st_l, S_l = sv
    slot = bn.reserve(z_l.shape[1], nm + ".1")
    if dft is None:
        dz = ops.bn_act_bwd(dy.view_as(z_l), z_l, *st_l, HSWISH, sums=slot)[0]
    else:
        zeros_bc = torch.zeros((z_l.shape[0], z_l.shape[1]), device=z_l.device)
        dz = ops.bn_act_bwd(z_l, z_l, *st_l, HSWISH, gscale=zeros_bc, gadd=dft * (1.0 / S_l), sums=slot)[0]
    g[nm + ".0.weight"] = ops.pw_conv_wgrad(dz, x_l, out=g.alloc(nm + ".0.weight", last[0].weight)).view_as(last[0].weight)
    wpt = _pk(plan, ("lt",), last[0].weight, trans=True)
    return ops.pw_conv(dz, wpt, _zeros.get(x_l.shape[1], dz.device), x_l.shape[1], NONE)


def _head_fwd(model, last, drop_mask):
    """Pooled features -> (state, (logits, features)); the pool reads BatchNorm + Hardswish of z_l on load."""
    z_l, st_l = last.z, last.st
    pooled = torch.empty((z_l.shape[0], z_l.shape[1]), device=z_l.device)
    ops.bn_act_fwd(z_l, st_l[0], st_l[1], HSWISH, pool=pooled, write=False)
    feat = pooled * (1.0 / last.S)
    fc1, fc2 = model.classifier[2], model.classifier[5]
    u = ops.linear(feat, fc1.weight, fc1.bias, NONE)
    h2 = F.hardswish(u)
    if drop_mask is not None:
        h2 = h2 * drop_mask
    logits = ops.linear(h2, fc2.weight, fc2.bias, NONE)
    return _HeadState(feat, u, h2, drop_mask), (logits, feat)


def _head_bwd(model, sv, dlogits, dfeat, g):
    """Two launches of the library's stride-addressed tile GEMMs (csrc/se_train.hip: eat_mlp_head_bwd) -> gradient of the
    pooled features (incl. `dfeat`, the gradient arriving at the features output)."""
    feat, u, h2, drop_mask = sv
    fc1, fc2 = model.classifier[2], model.classifier[5]
    o2, o1 = g.alloc("classifier.5.weight", fc2.weight), g.alloc("classifier.2.weight", fc1.weight)   # (production order)
    dW1, db1, dW2, db2, dft = ops.mlp_head_bwd(dlogits, h2.contiguous(), u.contiguous(),
                                              None if drop_mask is None else drop_mask.contiguous(), feat.contiguous(),
                                              fc1.weight, fc2.weight, dW1_out=o1, dW2_out=o2)
    g["classifier.5.weight"], g["classifier.5.bias"] = dW2, db2
    g["classifier.2.weight"], g["classifier.2.bias"] = dW1, db1
    return dft if dfeat is None else dft + dfeat


class MNTrainFunction2(torch.autograd.Function):
    """mode 0: the whole network incl. the mlp head -> (logits, features).  mode 1 ("trunk"): up to the last feature map
    -> (y_last, fmap_0 ... fmap_15): the caller runs the head on y_last (non-default heads, `return_fmaps`); the block
    outputs are handed out as non-differentiable tensors."""

    @staticmethod
    def forward(ctx, model, x, drop_mask, mode, *params):
        keep = torch.is_grad_enabled() or any(p.requires_grad for p in params)
        x = x.contiguous().float()
        blocks = list(model.features[1:-1])
        store16 = _act_storage_bf16(model)
        plan = _prepack_plan(model)
        if plan is not None:
            plan.run()
        stem, cur, sx = _stem_fwd(model.features[0], x, need_sx=bool(blocks) and blocks[0].i_expand is not None)
        fmaps, recs, cur16 = [cur], [], None
        for bi, blk in enumerate(blocks):
            nxt = blocks[bi + 1] if bi + 1 < len(blocks) else None
            rec, cur, cur16, sx = _block_fwd(blk, bi, cur, cur16, sx, nxt, stem.fused, plan, store16)
            recs.append(rec)
            fmaps.append(cur)
        last = _last_fwd(model.features[-1], cur, plan)
        ctx.mode = mode
        if mode == 1:
            head, out = None, (ops.bn_act_fwd(last.z, last.st[0], last.st[1], HSWISH),) + tuple(fmaps)
            ctx.mark_non_differentiable(*fmaps)
        else:
            head, out = _head_fwd(model, last, drop_mask)
        if keep:
            ctx.saved, ctx.model = _Saved(plan, plan.runs if plan is not None else 0, stem, recs, last, head), model
            ctx.names = [n for n, _ in model.named_parameters()]
        return out

    @staticmethod
    def backward(ctx, dout0, *rest):
        model, sv = ctx.model, ctx.saved
        ctx.saved = None
        dfeat = rest[0] if ctx.mode == 0 else None
        with ops.precision(getattr(model, "train_precision", "fp32")), ops.zero_arena.scope("mn_bwd"):
            return _backward_impl(ctx, model, sv, dout0, dfeat, n_lead=4)


def _backward_impl(ctx, model, sv, dlogits, dfeat, n_lead):
    """Backward of MNTrainFunction2 (one pass, reverse layer order)."""
    # every `g[name] = grad` hands the gradient to the data-parallel reducer, which all-reduces full
    # buckets on RCCL's stream while the remaining layers' backward kernels run (dp.py)
    # a model that was never handed to dp.enable_data_parallel keeps its gradients local (no hidden collective)
    g = _GradSink(getattr(model, "_grad_reducer", None) or GradReducer(local=True))
    g.reducer.begin_pass()               # (an aborted earlier backward must not leak its slots into this one: ADVICE r5)
    dlogits = dlogits.contiguous().float()
    blocks = list(model.features[1:-1])
    bn = _BnSums(model, dlogits.device)
    # trunk mode: the head ran outside (torch autograd); dlogits is the gradient w.r.t. the last feature map
    dft = _head_bwd(model, sv.head, dlogits, dfeat, g) if sv.head is not None else None
    plan = sv.plan
    if plan is not None and plan.runs != sv.plan_run:
        # another forward of the model re-packed the plan's views since this pass's forward (two forwards before one
        # backward): the views hold the CURRENT weights - pack this backward's operands matrix by matrix instead
        plan = None
    dout = _last_bwd(model.features[-1], f"features.{len(blocks) + 1}", sv.last, dlogits, dft, g, bn, plan)
    dout2 = None                         # second summand of the gradient w.r.t. the stem output (_block_bwd)
    for i in range(len(blocks) - 1, -1, -1):
        dout, dout2 = _block_bwd(blocks[i], i, sv.blocks[i], dout, g, bn, plan)
        sv.blocks[i] = None
    _stem_bwd(model.features[0], sv.stem, dout, dout2, g)
    bn.flush(g)
    grads = g.finish()
    return (None,) * n_lead + tuple(grads.get(n) for n in ctx.names)


class AttentionPoolHead(torch.autograd.Function):
    """The multi-head attention-pooling head (models/mn/attention_pooling.py:37-56) on the library, in the layout of the
    1x1 kernels (csrc/attn_head.hip): y (B, C, F, T) -> logits (B, K).

    forward:  `ops.freq_mean` -> the projection as a 1x1 conv over the T positions (`ops.pw_conv`, pack by the active
              `ops.precision`) -> `ops.attn_pool` (adds the bias, saves o and s)
    backward: `ops.attn_pool_bwd` (dp, dbias, dhead_w) -> data gradient on the same conv kernel with the transposed pack
              -> `ops.pw_conv_wgrad(dp, xm)` -> `ops.freq_mean_bwd`
    Rows of xm / p / dp have the pitch `ops.pitch4(T)`, pad columns zero.  The data-gradient GEMM contracts over the 2 H K
    rows of dp and wants a multiple of 4 of them: an odd H K (one head, an odd class count) runs the backward on dp and a
    copy of the weight padded by two zero rows."""

    @staticmethod
    def forward(ctx, y, w, b, head_w, H, eps):
        y = y.contiguous()
        B, C, Fq, T = y.shape
        N = w.shape[0]
        Tp = ops.pitch4(T)
        xm = ops.freq_mean(y, Tp)
        wp = ops.pw_prepack(w.contiguous())
        p = ops.pw_conv(xm.view(B, C, 1, Tp), wp, ops.zeros_vec.get(N, y.device), N, NONE).view(B, N, Tp)
        hw = head_w.detach().contiguous()
        out, o, s = ops.attn_pool(p, b, hw, H, T, eps, save=True)
        ctx.save_for_backward(xm, p, o, s, w, b, hw)
        ctx.geo, ctx.prec, ctx.hw_shape = (Fq, T, H, eps), ops.precision.mode, head_w.shape
        return out

    @staticmethod
    def backward(ctx, g):
        xm, p, o, s, w, b, hw = ctx.saved_tensors
        Fq, T, H, eps = ctx.geo
        B, C, Tp = xm.shape
        N = w.shape[0]
        Np = (N + 3) // 4 * 4
        with ops.precision(ctx.prec), ops.zero_arena.scope("att_head_bwd"):
            # (the zero-filled memory of the weight gradient first: the pass's one fill precedes the head's own launches)
            dw = ops.zero_arena.zeros((Np, C), torch.float32, w.device)
            dp, db, dhw = ops.attn_pool_bwd(g.contiguous().float(), p, b, hw, o, s, H, T, eps, Np=Np)
            wt = w.contiguous()
            if Np != N:
                wt = ops.zero_arena.zeros((Np, C), torch.float32, w.device)
                wt[:N].copy_(w)
            dp4 = dp.view(B, Np, 1, Tp)
            dw = ops.pw_conv_wgrad(dp4, xm.view(B, C, 1, Tp), exact=None, out=dw)[:N].view_as(w)
            dy = None
            if ctx.needs_input_grad[0]:
                dxm = ops.pw_conv(dp4, ops.pw_prepack(wt, trans=True), ops.zeros_vec.get(C, w.device), C, NONE)
                dy = ops.freq_mean_bwd(dxm.view(B, C, Tp), Fq, T)
        return dy, dw, db, dhw.view(ctx.hw_shape), None, None


def attention_pool_head(head, y):
    """`MultiHeadAttentionPooling` on the last feature map y under autograd (both training plans)."""
    return AttentionPoolHead.apply(y, head.subspace_proj.weight, head.subspace_proj.bias, head.head_weight, head.num_heads,
                                   head.epsilon)


class FrameHead(torch.autograd.Function):
    """The mlp head applied to every time column of the last feature map (what `detection.frame_logits` runs in eval), in the
    layout of the 1x1 kernels: y (B, C, F, T) -> frame logits (B, K, Tp), Tp = `ops.pitch4(T)`.  keep (B, H) or None: the
    dropout factor of a (clip, hidden unit), shared by the clip's frames.

    forward:  `ops.freq_mean` -> fc1 as a 1x1 conv over the Tp positions, bias in its epilogue (`ops.pw_conv`, pack by the
              active `ops.precision`) -> `ops.frame_hidden_fwd` (Hardswish, keep) -> fc2 likewise
    backward: `ops.frame_grad_pad` (the arriving gradient with exactly-zero pad rows and columns, and db2) ->
              `ops.pw_conv_wgrad(dl, h)` -> dh on the conv kernel with the transposed pack -> `ops.frame_hidden_bwd` (dz1,
              db1) -> `ops.pw_conv_wgrad(dz1, xm)` -> dxm likewise -> `ops.freq_mean_bwd`
    Hidden rows are zero-padded to a multiple of 4 (hswish(0) = 0 against zero columns of fc2: nothing changes), as
    `detection._head_packs` pads them; the data-gradient GEMM of fc2 contracts over `pitch4(K)` rows of dl.  Pad columns
    [T, Tp) of the logits hold the head's answer to a zero column: callers must not read them."""

    @staticmethod
    def forward(ctx, y, w1, b1, w2, b2, keep):
        y = y.contiguous()
        B, C, Fq, T = y.shape
        H, K = w1.shape[0], w2.shape[0]
        Hp, Tp = ops.pitch4(H), ops.pitch4(T)
        w1p, b1p = w1.detach().contiguous(), b1.detach().contiguous()
        w2p = w2.detach().contiguous()
        if keep is not None:
            keep = keep.detach().contiguous().float()
        if Hp != H:
            w1p = torch.cat((w1p, w1p.new_zeros((Hp - H, C))))
            b1p = torch.cat((b1p, b1p.new_zeros(Hp - H)))
            w2p = torch.cat((w2p, w2p.new_zeros((K, Hp - H))), dim=1)
            if keep is not None:
                keep = torch.cat((keep, keep.new_ones((B, Hp - H))), dim=1)
        xm = ops.freq_mean(y, Tp)
        z1 = ops.pw_conv(xm.view(B, C, 1, Tp), ops.pw_prepack(w1p), b1p, Hp, NONE).view(B, Hp, Tp)
        h = ops.frame_hidden_fwd(z1, keep)
        z = ops.pw_conv(h.view(B, Hp, 1, Tp), ops.pw_prepack(w2p), b2.detach().contiguous(), K, NONE).view(B, K, Tp)
        ctx.save_for_backward(xm, z1, h, w1p, w2p, keep)
        ctx.geo, ctx.prec = (Fq, T, H, K), ops.precision.mode
        return z

    @staticmethod
    def backward(ctx, g):
        xm, z1, h, w1p, w2p, keep = ctx.saved_tensors
        Fq, T, H, K = ctx.geo
        B, C, Tp = xm.shape
        Hp, Kp = z1.shape[1], ops.pitch4(K)
        dev = xm.device
        with ops.precision(ctx.prec), ops.zero_arena.scope("frame_head_bwd"):
            # (the zero-filled memory first: the pass's one fill precedes the head's own launches)
            dw2 = ops.zero_arena.zeros((Kp, Hp), torch.float32, dev)
            dw1 = ops.zero_arena.zeros((Hp, C), torch.float32, dev)
            w2t = w2p
            if Kp != K:
                w2t = ops.zero_arena.zeros((Kp, Hp), torch.float32, dev)
                w2t[:K].copy_(w2p)
            # whatever autograd hands over (the fused loss's gradient times a scalar, or any other): pads re-established
            dl, db2 = ops.frame_grad_pad(g.contiguous().float(), T, Kp)
            dl4, h4, xm4 = dl.view(B, Kp, 1, Tp), h.view(B, Hp, 1, Tp), xm.view(B, C, 1, Tp)
            dw2 = ops.pw_conv_wgrad(dl4, h4, exact=None, out=dw2)[:K, :H]
            dh = ops.pw_conv(dl4, ops.pw_prepack(w2t, trans=True), ops.zeros_vec.get(Hp, dev), Hp, NONE)
            dz1, db1 = ops.frame_hidden_bwd(dh.view(B, Hp, Tp), z1, keep, H, T)
            dz4 = dz1.view(B, Hp, 1, Tp)
            dw1 = ops.pw_conv_wgrad(dz4, xm4, exact=None, out=dw1)[:H]
            dy = None
            if ctx.needs_input_grad[0]:
                dxm = ops.pw_conv(dz4, ops.pw_prepack(w1p, trans=True), ops.zeros_vec.get(C, dev), C, NONE)
                dy = ops.freq_mean_bwd(dxm.view(B, C, Tp), Fq, T)
        return dy, dw1, db1, (dw2 if Hp == H else dw2.contiguous()), db2, None


def _frame_scope(model):
    """What `forward_train_frames` covers: an MN with the mlp head on the monolithic plan.  Everything else: ValueError."""
    from .mn import MN as _MN
    if not isinstance(model, _MN):
        raise ValueError(f"forward_train_frames: {type(model).__name__} is not an MN: the frame-level training path covers the "
                         "static MobileNets only (a DyMN's trunk has no Function that hands back a differentiable last map)")
    head = model.head_type
    if head == "multihead_attention_pooling":
        raise ValueError("forward_train_frames: the multihead_attention_pooling head has no frame-level logits (its attention "
                         "is normalised over the whole clip)")
    if head == "fully_convolutional":
        raise ValueError("forward_train_frames: the fully_convolutional head carries a BatchNorm whose train-mode statistics "
                         "would have to span the frames of the batch; train the 'mlp' head")
    if head != "mlp":
        raise ValueError(f"forward_train_frames: head_type {head!r} has no frame-level plan")
    if model._modular_train:
        raise ValueError("forward_train_frames: this MN trains on the modular plan (dilated blocks or squeeze-excitation "
                         "beyond the channel axis), which has no trunk Function; only the monolithic plan is covered")


def forward_train_frames(model, x):
    """Train-mode frame logits (B, K, Tp) of an mlp-head MN under autograd: the trunk Function up to the last feature map
    (`MNTrainFunction2`, mode 1) and `FrameHead` on it.  Dropout (classifier[4]) is one keep value per (clip, hidden
    unit), shared by that clip's frames, drawn as `forward_train` draws its mask (`_drop_mask_override` replaces the draw)
    and scaled by 1 / (1 - p).  Frame t of the logits is column t < T = the last map's width; columns [T, Tp) are padding."""
    _frame_scope(model)
    if not model.training:
        raise ValueError("forward_train_frames needs the model in train mode (model.train()); `detection.frame_logits` is the "
                         "eval path")
    drop = model.classifier[4]
    keep = None
    if drop.p > 0 and drop.training:
        n_hidden = model.classifier[2].out_features
        keep = torch.empty((x.shape[0], n_hidden), device=x.device).bernoulli_(1.0 - drop.p) / (1.0 - drop.p)
    override = getattr(model, "_drop_mask_override", None)       # tests replay the reference's mask
    if override is not None and drop.training:
        keep = override.to(x.device).float() / (1.0 - drop.p)
    params = [p for _, p in model.named_parameters()]
    model._eat_trunk_active = True        # the head's gradients reach its parameters through autograd (forward_train)
    fc1, fc2 = model.classifier[2], model.classifier[5]
    with ops.precision(getattr(model, "train_precision", "fp32")), ops.bn_counters, ops.zero_arena.scope("mn_fwd"):
        y_l = MNTrainFunction2.apply(model, x, None, 1, *params)[0]
        return FrameHead.apply(y_l, fc1.weight, fc1.bias, fc2.weight, fc2.bias, keep)


def forward_train(model, x, return_fmaps=False):
    """Train-mode `(logits, features)` - or `(logits, fmaps)` - with autograd support (mn/model.py:212-231 in `.train()`).

    The default network (mlp head) is one Function incl. the head.  Non-default heads (`fully_convolutional`,
    `multihead_attention_pooling`; mn/model.py:170-185) and `return_fmaps=True` run the trunk Function up to the last
    feature map and the head on top of it: the attention-pooling head as the library's `AttentionPoolHead`, the
    fully-convolutional one as torch ops under torch autograd (both act on the 960 x 4 x 32 map only).  The 17 feature maps of
    `return_fmaps` are values only (no gradient flows back through them; the logits are differentiable as usual)."""
    drop = model.classifier[4] if model.head_type == "mlp" else None
    mask = None
    if drop is not None and drop.p > 0 and drop.training:
        n_hidden = model.classifier[2].out_features
        mask = torch.empty((x.shape[0], n_hidden), device=x.device).bernoulli_(1.0 - drop.p) / (1.0 - drop.p)
    override = getattr(model, "_drop_mask_override", None)       # tests replay the reference's mask
    if override is not None and drop is not None and drop.training:
        mask = override.to(x.device).float() / (1.0 - drop.p)
    params = [p for _, p in model.named_parameters()]
    trunk = return_fmaps or model.head_type != "mlp"
    model._eat_trunk_active = trunk       # dp.py: the head's gradients reach its parameters through autograd then (their own reducer hooks)
    with ops.precision(getattr(model, "train_precision", "fp32")), ops.bn_counters, ops.zero_arena.scope("mn_fwd"):
        if not trunk:
            return MNTrainFunction2.apply(model, x, mask, 0, *params)
        outs = MNTrainFunction2.apply(model, x, None, 1, *params)
        y_l, fmaps = outs[0], list(outs[1:])
        if model.head_type == "multihead_attention_pooling":
            # the library's head: frequency mean, GEMM, pooling - launched straight behind the trunk's last kernel
            logits = attention_pool_head(model.classifier, y_l)
            feat = y_l.mean(dim=(2, 3))
            return (logits, fmaps + [y_l]) if return_fmaps else (logits, feat)
        feat = y_l.mean(dim=(2, 3))
        if model.head_type == "mlp":
            fc1, fc2 = model.classifier[2], model.classifier[5]
            h = F.hardswish(F.linear(feat, fc1.weight, fc1.bias))
            if mask is not None:
                h = h * mask
            logits = F.linear(h, fc2.weight, fc2.bias)
        else:
            # fully-convolutional head (1x1 conv to the classes + BatchNorm + mean: the class count, 527, is not a
            # multiple of 4, which the library's data-gradient GEMM needs): a few MB of torch ops on the 4 x 32 map under
            # torch autograd
            logits = model.classifier(y_l).reshape(x.shape[0], -1)
    return (logits, fmaps + [y_l]) if return_fmaps else (logits, feat)


# ---------------------------------------------------------------------------------------------------------------------
# Modular train path for the variants the monolithic plan does not cover: dilated tails (`dilated=True`,
# models/mn/model.py:244-269) and squeeze-excitation over the time axis / several axes at once (`se_dims` beyond 'c',
# models/mn/block_types.py:10-83).  Neither has a released checkpoint or a measured configuration: every conv / BatchNorm is
# the library's kernel behind a per-layer autograd Function (the ones DyMN's static blocks use, dymn_train.py), the
# concurrent SE block - a mean over two axes, two Linears on a vector of <= 960 entries, a broadcast product and the
# max / avg / add / min of the gated copies - is torch ops under torch autograd.
def _concurrent_se_train(se_block, y):
    """ConcurrentSEBlock.forward (block_types.py:36-42) over SqueezeExcitation.forward (:72-83), differentiable."""
    outs = []
    for se in se_block.conc_se_layers:
        d = se.gate_dim                                            # the axis that keeps its extent (1 = c, 3 = t)
        m = y.mean(dim=[k for k in (1, 2, 3) if k != d])           # (B, extent)
        gate = torch.sigmoid(F.linear(F.relu(F.linear(m, se.fc1.weight, se.fc1.bias)), se.fc2.weight, se.fc2.bias))
        shape = [y.shape[0], 1, 1, 1]
        shape[d] = gate.shape[1]
        outs.append(gate.view(shape) * y)
    if len(outs) == 1:
        return outs[0]
    st = torch.stack(outs, dim=0)
    agg = se_block.se_agg
    return (st.max(dim=0)[0] if agg == "max" else st.mean(dim=0) if agg == "avg" else st.sum(dim=0) if agg == "add"
            else st.min(dim=0)[0])


def forward_train_modular(model, x, return_fmaps=False):
    """Train-mode `(logits, features)` / `(logits, fmaps)` of an MN with dilated blocks or SE beyond the channel axis."""
    from .dymn_train import BnAct, DwConv, Linear, PwConv, StemConv
    drop = model.classifier[4] if model.head_type == "mlp" else None
    with ops.precision(getattr(model, "train_precision", "fp32")), ops.bn_counters, ops.zero_arena.scope("mn_fwd"):
        x = x.contiguous().float()
        stem = model.features[0]
        cur = BnAct.apply(StemConv.apply(x, stem[0].weight), stem[1].weight, stem[1].bias, stem[1], HSWISH)
        fmaps = [cur]
        for blk in model.features[1:-1]:
            cnf = blk.cnf
            act = HSWISH if cnf.use_hs else RELU
            inp = cur
            if blk.i_expand is not None:
                conv, bn = blk.block[blk.i_expand][0], blk.block[blk.i_expand][1]
                cur = BnAct.apply(PwConv.apply(cur, conv.weight), bn.weight, bn.bias, bn, act)
            conv, bn = blk.block[blk.i_dw][0], blk.block[blk.i_dw][1]
            cur = BnAct.apply(DwConv.apply(cur, conv.weight, cnf.kernel, blk.dw_stride, cnf.dilation), bn.weight, bn.bias, bn, act)
            if blk.i_se is not None:
                cur = _concurrent_se_train(blk.block[blk.i_se], cur)
            conv, bn = blk.block[blk.i_proj][0], blk.block[blk.i_proj][1]
            cur = BnAct.apply(PwConv.apply(cur, conv.weight), bn.weight, bn.bias, bn, NONE)
            if blk.use_res_connect:
                cur = cur + inp
            fmaps.append(cur)
        last = model.features[-1]
        y_l = BnAct.apply(PwConv.apply(cur, last[0].weight), last[1].weight, last[1].bias, last[1], HSWISH)
        feat = y_l.mean(dim=(2, 3))
        if model.head_type == "mlp":
            fc1, fc2 = model.classifier[2], model.classifier[5]
            h = F.hardswish(Linear.apply(feat, fc1.weight, fc1.bias))
            override = getattr(model, "_drop_mask_override", None)
            if drop is not None and drop.training:
                if override is not None:
                    h = h * (override.to(h.device).float() / (1.0 - drop.p))
                elif drop.p > 0:
                    h = F.dropout(h, drop.p, True)
            logits = Linear.apply(h, fc2.weight, fc2.bias)
        elif model.head_type == "multihead_attention_pooling":
            logits = attention_pool_head(model.classifier, y_l)
        else:
            logits = model.classifier(y_l).reshape(x.shape[0], -1)
    return (logits, fmaps + [y_l]) if return_fmaps else (logits, feat)
