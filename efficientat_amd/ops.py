"""Python-side launchers for the C ABI (include/eat_hip.h): argument checks, output
allocation through PyTorch's caching allocator, launch on torch's current HIP stream.
PyTorch is plumbing here (device memory + streams); all arithmetic is in libeat_hip.so."""
import os

import torch

from . import _lib

ACT_NONE, ACT_RELU, ACT_HSWISH, ACT_SIGMOID = 0, 1, 2, 3


_PRIMARY = ("x", "dz", "wave", "z", "dy")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(t, name):
    if not t.is_cuda:
        raise _lib.EatHipError(f"{name} must live on the GPU: efficientat_amd has no CPU path "
                               f"(got device {t.device})")
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise _lib.EatHipError(f"{name} must be contiguous float32 (got {t.dtype}, contiguous={t.is_contiguous()})")
    if name in _PRIMARY and t.device.index != torch.cuda.current_device():   # checked on the main operand only
        # kernels are launched on the CURRENT device's stream: one process per GPU (torch.cuda.set_device), or
        # wrap the call in `with torch.cuda.device(t.device):`
        raise _lib.EatHipError(f"{name} lives on {t.device} but the current device is cuda:{torch.cuda.current_device()}")
    return t.data_ptr()


def _opt(t, name):
    return None if t is None else _dev(t, name)


def _dev16(t, name):
    """Device pointer of a contiguous bfloat16 activation tensor (the wide tensors of the bf16-storage plan)."""
    if not t.is_cuda:
        raise _lib.EatHipError(f"{name} must live on the GPU: efficientat_amd has no CPU path (got device {t.device})")
    if t.dtype != torch.bfloat16 or not t.is_contiguous():
        raise _lib.EatHipError(f"{name} must be contiguous bfloat16 (got {t.dtype}, contiguous={t.is_contiguous()})")
    if t.device.index != torch.cuda.current_device():
        raise _lib.EatHipError(f"{name} lives on {t.device} but the current device is cuda:{torch.cuda.current_device()}")
    return t.data_ptr()


def _is16(t):
    return t is not None and t.dtype == torch.bfloat16


class _ConstVec:
    """Cached constant fp32 vector, one buffer per device (zeros: the bias of the train-mode convs, whose entry points take a
    bias pointer; ones: the identity BatchNorm scale).  A buffer that has been handed out is never freed - a captured graph
    may hold its address - so one that has to grow keeps its predecessors alive."""

    def __init__(self, value):
        self.value, self.bufs, self.outgrown = value, {}, []

    def get(self, n, device):
        buf = self.bufs.get(device)
        if buf is None or buf.numel() < n:
            if buf is not None:
                self.outgrown.append(buf)
            buf = self.bufs[device] = torch.full((max(n, 4096),), self.value, device=device, dtype=torch.float32)
        return buf[:n]


zeros_vec, ones_vec = _ConstVec(0.0), _ConstVec(1.0)

_KCAT = True   # K-concat form of the late dynamic 1x1 convs (eval; `kcat_eligible`)


def conv_out(n, k, stride):
    """floor((n + 2p - (k-1) - 1)/s + 1), p=(k-1)//2   (models/mn/utils.py:24-26, dilation 1)."""
    p = (k - 1) // 2
    return (n + 2 * p - (k - 1) - 1) // stride + 1


def mel_fwd(wave, window, twiddle, band_w2, band_start, band_cnt, n_fft, hop, n_mels, fmask=(0, 0), tmask=(0, 0), out=None):
    B, L = wave.shape
    T = 1 + (L - 1) // hop
    if band_w2.shape[1:] != (n_mels, 2) or band_start.numel() != n_mels or band_cnt.numel() != n_mels:
        raise _lib.EatHipError("mel_fwd: band table must be (pairs, n_mels, 2) with n_mels starts / counts")
    if out is None:
        out = torch.empty((B, n_mels, T), device=wave.device, dtype=torch.float32)
    elif out.numel() != B * n_mels * T or out.dtype != torch.float32 or not out.is_contiguous():
        raise _lib.EatHipError(f"mel_fwd: out must be a contiguous fp32 buffer of {B} x {n_mels} x {T} elements")
    _lib.call("eat_mel_fwd", _dev(wave, "wave"), B, L, _dev(window, "window"), window.numel(), n_fft, hop,
              _dev(twiddle, "twiddle"), _dev(band_w2, "band_w2"), band_start.data_ptr(), band_cnt.data_ptr(), n_mels,
              band_w2.shape[0], out.data_ptr(), T, fmask[0], fmask[1], tmask[0], tmask[1], _stream())
    return out


def stem_conv(x, w, bias, act):
    B, _, F, T = x.shape
    C = w.shape[0]
    Fo, To = conv_out(F, 3, 2), conv_out(T, 3, 2)
    y = torch.empty((B, C, Fo, To), device=x.device, dtype=torch.float32)
    _lib.call("eat_stem_conv_fwd", _dev(x, "x"), _dev(w, "w"), _dev(bias, "bias"), y.data_ptr(), B, C, F, T,
              Fo, To, act, _stream())
    return y


def dw_conv(x, w, bias, k, stride, act, pool=None):
    B, C, F, T = x.shape
    Fo, To = conv_out(F, k, stride), conv_out(T, k, stride)
    y = torch.empty((B, C, Fo, To), device=x.device, dtype=torch.float32)
    _lib.call("eat_dw_conv_fwd", _dev(x, "x"), _dev(w, "w"), _dev(bias, "bias"), y.data_ptr(),
              _opt(pool, "pool"), B, C, F, T, Fo, To, k, stride, act, _stream())
    return y


def dw_conv_dilated(x, w, bias, k, stride, dilation, act, pool=None):
    """Dilated depthwise conv + bias + activation (+ per-plane sums of the output added into `pool` (B, C)); the batch goes
    through in ranges of <= 65535 planes (`_plane_chunks`: whole samples, so plane % C stays the channel)."""
    B, C, F, T = x.shape
    Fo, To = dilated_out(F, T, k, stride, dilation)
    y = torch.empty((B, C, Fo, To), device=x.device, dtype=torch.float32)
    if w.numel() != C * k * k or bias.numel() < C or (pool is not None and pool.numel() != B * C):
        raise _lib.EatHipError(f"dw_conv_dilated: w must hold {C} x {k * k} taps, bias {C} values, pool {B} x {C} sums")
    xp, wp, bp, pp = _dev(x, "x"), _dev(w, "w"), _dev(bias, "bias"), _opt(pool, "pool")
    for b0, b1 in _plane_chunks(B, C):
        _lib.call("eat_dw_conv_dilated_fwd", xp + 4 * b0 * C * F * T, wp, bp, y.data_ptr() + 4 * b0 * C * Fo * To,
                  None if pp is None else pp + 4 * b0 * C, b1 - b0, C, F, T, Fo, To, k, stride, dilation, act, _stream())
    return y


def dilated_out(F, T, k, stride, dilation):
    pad = (k - 1) // 2 * dilation
    return (F + 2 * pad - dilation * (k - 1) - 1) // stride + 1, (T + 2 * pad - dilation * (k - 1) - 1) // stride + 1


# Planes of one launch of the generic dilated kernels (their grids' y dimension).  65535 is the bound the project keeps for
# that dimension everywhere; the HIP runtime on an MI355X was seen to take 67200 in one launch, so this is portability, not a
# fault that was met.
_GRID_Y = 65535


def _plane_chunks(B, C):
    """Batch ranges whose (samples x channels) planes fit the y dimension of a launch grid (65535)."""
    if not 1 <= C <= _GRID_Y:
        raise _lib.EatHipError(f"dilated depthwise conv: {C} channels do not fit one launch (1..{_GRID_Y} planes per sample)")
    step = _GRID_Y // C
    return [(i, min(B, i + step)) for i in range(0, B, step)]


def dw_conv_dyn_dilated(x, taps, k, stride, dilation):
    """Dilated depthwise conv with PER-SAMPLE taps (B, C*k*k) - the depthwise DynamicConv of a dilated DY_Block
    (models/dymn/dy_block.py:103-131,322-348): a depthwise conv over B * C independent planes, i.e. the generic dilated
    kernels with the batch folded into the channel axis (in chunks of <= 65535 planes)."""
    B, C, F, T = x.shape
    Fo, To = dilated_out(F, T, k, stride, dilation)
    y = torch.empty((B, C, Fo, To), device=x.device, dtype=torch.float32)
    chunks = _plane_chunks(B, C)
    zb = zeros_vec.get(max(b1 - b0 for b0, b1 in chunks) * C, x.device)
    for b0, b1 in chunks:
        n = (b1 - b0) * C
        _lib.call("eat_dw_conv_dilated_fwd", _dev(x, "x") + 4 * b0 * C * F * T, _dev(taps, "taps") + 4 * b0 * C * k * k,
                  zb.data_ptr(), y.data_ptr() + 4 * b0 * C * Fo * To, None, 1, n, F, T, Fo, To, k, stride, dilation, ACT_NONE,
                  _stream())
    return y


def dw_conv_dyn_dilated_bwd(dz, x, taps, k, stride, dilation):
    """-> (dx, G (B, C*k*k) per-plane tap gradients) of `dw_conv_dyn_dilated`."""
    B, C, F, T = x.shape
    Fo, To = dz.shape[2], dz.shape[3]
    dx = torch.empty_like(x)
    G = torch.empty((B, C * k * k), device=x.device, dtype=torch.float32)
    for b0, b1 in _plane_chunks(B, C):
        n = (b1 - b0) * C
        _lib.call("eat_dw_conv_dilated_dgrad", _dev(dz, "dz") + 4 * b0 * C * Fo * To, _dev(taps, "taps") + 4 * b0 * C * k * k,
                  dx.data_ptr() + 4 * b0 * C * F * T, 1, n, F, T, Fo, To, k, stride, dilation, _stream())
        _lib.call("eat_dw_conv_dilated_wgrad", _dev(dz, "dz") + 4 * b0 * C * Fo * To, _dev(x, "x") + 4 * b0 * C * F * T,
                  G.data_ptr() + 4 * b0 * C * k * k, 1, n, F, T, Fo, To, k, stride, dilation, _stream())
    return dx, G


def dyrelu_ca(z, a, b, act, coef, gate_f, gate_t):
    """BatchNorm affine (a, b per channel) + DyReLU-B (coef (B, C, 4); None: the plain activation `act`) + CoordAtt (position-
    major PRE-sigmoid gates (B*Fo, C) / (B*To, C); None: no attention) of a (B, C, Fo, To) tensor - the stand-alone kernel
    of the dilated dynamic block (eat_dyrelu_ca_fwd; the ablations are expressed through constant operands: a1 = a2 = 1 is
    the identity, gates of +40 a sigmoid of exactly 1 in fp32)."""
    B, C, Fo, To = z.shape
    if coef is None:
        # plain activation in DyReLU's place: BatchNorm + act through the generic pass, attention (if any) on its output
        y = bn_act_fwd(z, a, b, act)
        if gate_f is None:
            return y
        z, a, b = y, None, None
        coef = torch.tensor([1.0, 1.0, 0.0, 0.0], device=z.device).expand(B, C, 4).contiguous()
    if gate_f is None:
        gate_f = torch.full((B * Fo, C), 40.0, device=z.device)
        gate_t = torch.full((B * To, C), 40.0, device=z.device)
    return dyrelu_ca_fwd(z, a, b, coef.contiguous(), gate_f.contiguous(), gate_t.contiguous())


def dw_conv_dilated_dgrad(dz, w, x_shape, k, stride, dilation):
    """Data gradient of the dilated depthwise conv (training of `dilated=True` networks; generic kernel), in the same batch
    ranges as the forward."""
    B, C, F, T = x_shape
    Fo, To = dz.shape[2], dz.shape[3]
    dx = torch.empty((B, C, F, T), device=dz.device, dtype=torch.float32)
    if tuple(dz.shape[:2]) != (B, C) or w.numel() != C * k * k:
        raise _lib.EatHipError(f"dw_conv_dilated_dgrad: dz must be ({B}, {C}, Fo, To) and w hold {C} x {k * k} taps")
    gp, wp = _dev(dz, "dz"), _dev(w, "w")
    for b0, b1 in _plane_chunks(B, C):
        _lib.call("eat_dw_conv_dilated_dgrad", gp + 4 * b0 * C * Fo * To, wp, dx.data_ptr() + 4 * b0 * C * F * T, b1 - b0, C,
                  F, T, Fo, To, k, stride, dilation, _stream())
    return dx


def dw_conv_dilated_wgrad(dz, x, k, stride, dilation):
    B, C, F, T = x.shape
    if C > _GRID_Y:   # one block per (tap, channel): the channels are the grid's y dimension
        raise _lib.EatHipError(f"dw_conv_dilated_wgrad: {C} channels do not fit one launch (at most {_GRID_Y})")
    dw = torch.empty((C, k * k), device=dz.device, dtype=torch.float32)
    _lib.call("eat_dw_conv_dilated_wgrad", _dev(dz, "dz"), _dev(x, "x"), dw.data_ptr(), B, C, F, T, dz.shape[2], dz.shape[3],
              k, stride, dilation, _stream())
    return dw


def dw_conv_tf(x, in_a, in_b, in_act, w, bias, k, stride):
    """Depthwise conv of act_in(in_a[c] * x + in_b[c]) (evaluated on load), no output activation (train mode)."""
    B, C, F, T = x.shape
    Fo, To = conv_out(F, k, stride), conv_out(T, k, stride)
    y = torch.empty((B, C, Fo, To), device=x.device, dtype=torch.float32)
    _lib.call("eat_dw_conv_fwd_tf", _dev(x, "x"), _dev(in_a, "in_a"), _dev(in_b, "in_b"), in_act, _dev(w, "w"),
              _dev(bias, "bias"), y.data_ptr(), B, C, F, T, Fo, To, k, stride, _stream())
    return y


def _pw_prepack_fp32(w2d, row_scale=None, trans=False):
    """trans: pack w2d^T (w2d is the stored (Ci, Co) matrix) - the data-gradient GEMM without a transposed copy."""
    Co, Ci = (w2d.shape[1], w2d.shape[0]) if trans else w2d.shape
    wp = torch.empty(((Ci // 4) * ((Co + 15) // 16) * 64,), device=w2d.device, dtype=torch.float32)
    _lib.call("eat_pw_prepack_t" if trans else "eat_pw_prepack", _dev(w2d, "w"), _opt(row_scale, "row_scale"),
              wp.data_ptr(), Co, Ci, _stream())
    return wp


def _pw_conv_fp32(x, wp, bias, Co, act, in_scale=None, res=None, pool=None, write=True):
    B, Ci, F, T = x.shape
    y = torch.empty((B, Co, F, T), device=x.device, dtype=torch.float32) if write else None
    _lib.call("eat_pw_conv_fwd", _dev(x, "x"), _dev(wp, "wp"), _dev(bias, "bias"), _opt(in_scale, "in_scale"),
              _opt(res, "res"), None if y is None else y.data_ptr(), _opt(pool, "pool"), B, Ci, Co, F * T, act,
              _stream())
    return y


def linear(x, w, bias, act, x_scale=1.0):
    B, K = x.shape
    N = w.shape[0]
    y = torch.empty((B, N), device=x.device, dtype=torch.float32)
    _lib.call("eat_linear_fwd", _dev(x, "x"), _dev(w, "w"), _opt(bias, "bias"), y.data_ptr(), B, K, N,
              float(x_scale), act, _stream())
    return y


# ------------------------------------------------------------------ training-step launchers
class _ZeroArena:
    """One zero-filled allocation per pass instead of ~90 `torch.zeros` launches: the kernels that accumulate with atomics
    (weight gradients, fp64 BatchNorm sums) carve their zeroed outputs out of it.  `with zero_arena.scope("bwd"):` opens
    a pass; its size is learnt from the first pass of that name (which falls back to individual `torch.zeros`)."""

    def __init__(self):
        self.need, self.buf, self.off, self.req, self.name = {}, None, 0, 0, None

    def scope(self, name):
        arena = self

        class _Scope:
            def __enter__(self):
                self.outer = (arena.name, arena.buf, arena.off, arena.req)
                arena.name, arena.buf, arena.off, arena.req = name, None, 0, 0

            def __exit__(self, *exc):
                arena.need[name] = max(arena.need.get(name, 0), arena.req)
                arena.name, arena.buf, arena.off, arena.req = self.outer

        return _Scope()

    def begin(self, name):
        """Open a pass that stays open until the next `begin` of the same name (DyMN: the backward runs inside autograd,
        after `forward_train` has returned, so no `with` block can span the step)."""
        if self.name == name:
            self.need[name] = max(self.need.get(name, 0), self.req)
        self.name, self.buf, self.off, self.req = name, None, 0, 0

    def end(self, name):
        """Close a pass opened with `begin` (DyMN: called when the backward reaches the stem, and by `graphs.capture` after
        every capture): later un-scoped callers get their own `torch.zeros` again instead of slices of the step's buffer -
        which a captured graph re-zeroes on every replay."""
        if self.name == name:
            self.need[name] = max(self.need.get(name, 0), self.req)
            self.name, self.buf, self.off, self.req = None, None, 0, 0

    def zeros(self, shape, dtype, device):
        if self.name is None:
            return torch.zeros(shape, device=device, dtype=dtype)
        numel = 1
        for d in shape:
            numel *= d
        nbytes = (numel * torch.empty((), dtype=dtype).element_size() + 255) // 256 * 256
        self.req += nbytes
        need = self.need.get(self.name, 0)
        if self.buf is None and need:
            self.buf = torch.zeros((need,), device=device, dtype=torch.uint8)
        if self.buf is None or self.off + nbytes > self.buf.numel() or self.buf.device != device:
            return torch.zeros(shape, device=device, dtype=dtype)
        v = self.buf[self.off:self.off + nbytes].view(dtype)[:numel].view(shape)
        self.off += nbytes
        return v


zero_arena = _ZeroArena()


class _DeferredCounters:
    """`bn.num_batches_tracked += 1` of every BatchNorm layer of a forward pass as ONE multi-tensor launch."""

    def __init__(self):
        self.depth, self.pending = 0, []

    def __enter__(self):
        self.depth += 1
        return self

    def __exit__(self, *exc):
        self.depth -= 1
        if self.depth == 0 and self.pending:
            torch._foreach_add_(self.pending, 1)
            self.pending = []

    def bump(self, bn):
        if self.depth:
            self.pending.append(bn.num_batches_tracked)
        else:
            bn.num_batches_tracked += 1


bn_counters = _DeferredCounters()


def bn_stats(z):
    B, C = z.shape[0], z.shape[1]
    S = z.numel() // (B * C)
    sums = zero_arena.zeros((2 * C,), torch.float64, z.device)
    _lib.call("eat_bn_stats", _dev(z, "z"), B, C, S, sums.data_ptr(), _stream())
    return sums


def bn_finalize(sums, bn, n, momentum=None):
    """-> (a, b, mean, invstd); updates bn.running_mean / running_var in place (momentum rule)."""
    C = bn.num_features
    out = torch.empty((4, C), device=sums.device, dtype=torch.float32)
    mom = momentum if momentum is not None else (bn.momentum if bn.momentum is not None else 0.0)
    _lib.call("eat_bn_finalize", sums.data_ptr(), _dev(bn.weight, "gamma"), _dev(bn.bias, "beta"),
              bn.running_mean.data_ptr(), bn.running_var.data_ptr(), float(mom), float(bn.eps), float(n), C,
              out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), _stream())
    return out[0], out[1], out[2], out[3]


def bn_frozen_state(bn):
    """(a, b, mean, invstd) of a BatchNorm layer in eval mode inside a train-mode pass (running statistics, no buffer
    update); flagged so that the backward treats the layer as a fixed affine map."""
    with torch.no_grad():
        invstd = torch.rsqrt(bn.running_var + bn.eps)
        a = (bn.weight * invstd).contiguous()
        st = (a, (bn.bias - bn.running_mean * a).contiguous(), bn.running_mean.clone(), invstd.contiguous())
    st[2]._eat_frozen = True
    return st


def bn_train_state(z, bn):
    """(a, b, mean, invstd) of one BatchNorm layer inside a train-mode pass, honouring the layer's OWN mode:
    * bn.training: batch statistics; running buffers updated with `momentum` (None = cumulative moving average
      with factor 1 / num_batches_tracked, torch semantics), num_batches_tracked += 1;
    * bn.eval() inside model.train() (the freeze-BN fine-tuning recipe): running statistics, no buffer update; the
      returned state is flagged so that `bn_act_bwd` treats the layer as a fixed affine map."""
    C = z.shape[1]
    if not bn.training:
        return bn_frozen_state(bn)
    mom = bn.momentum
    if mom is None:
        mom = 1.0 / (int(bn.num_batches_tracked) + 1)          # host read: this mode is not graph-capturable
    st = bn_finalize(bn_stats(z), bn, z.numel() // C, momentum=mom)
    bn_counters.bump(bn)
    return st


def bn_act_fwd(z, a, b, act, res=None, pool=None, write=True, y_f32=False, copy16=False):
    """y = act(a[c] z + b[c]) [+ res]; pool (B, C): plane sums of y.  A bf16 z (bf16-storage plan): y is bf16 too - or, with
    y_f32 (the project conv's BatchNorm: z_p stored in bf16, the block output fp32), fp32 with the optional fp32 residual;
    copy16 (with y_f32): -> (y, bf16 rounding of y), both written by the one pass."""
    B, C = z.shape[0], z.shape[1]
    S = z.numel() // (B * C)
    if _is16(z):                                   # bf16 storage (BASELINE configs[2]): pool = sums of the values as stored
        y16 = not y_f32
        if res is not None and y16:
            raise _lib.EatHipError("bn_act_fwd: a residual is added to an fp32 output only (y_f32=True)")
        y = torch.empty(z.shape, device=z.device, dtype=torch.bfloat16 if y16 else torch.float32) if write else None
        yc = torch.empty(z.shape, device=z.device, dtype=torch.bfloat16) if copy16 and y_f32 and write else None
        _lib.call("eat_bn_act_fwd_b16", _dev16(z, "z"), a.data_ptr(), b.data_ptr(), _opt(res, "res"),
                  None if y is None else y.data_ptr(), 1 if y16 else 0, None if yc is None else yc.data_ptr(),
                  _opt(pool, "pool"), B, C, S, act, _stream())
        return (y, yc) if copy16 else y
    y = torch.empty_like(z) if write else None
    _lib.call("eat_bn_act_fwd", _dev(z, "z"), a.data_ptr(), b.data_ptr(), _opt(res, "res"),
              None if y is None else y.data_ptr(), _opt(pool, "pool"), B, C, S, act, _stream())
    return y


def bn_act_bwd(dy, z, a, b, mean, invstd, act, gscale=None, gadd=None, frozen=None, sums=None, copy16=False):
    """-> (dz, dgamma, dbeta) for y = act(BN_batch(z)); incoming grad = dy*gscale[b,c] + gadd[b,c].
    frozen (default: the flag `bn_train_state` left on `mean`): the layer normalised with its running statistics,
    i.e. dz = a * g without the batch-mean terms (dgamma / dbeta are the same reductions)."""
    if frozen is None:
        frozen = getattr(mean, "_eat_frozen", False)
    B, C = z.shape[0], z.shape[1]
    S = z.numel() // (B * C)
    own = sums is None            # sums: a zeroed (2C,) float64 slice of the caller's arena (one fp32 conversion per pass)
    if own:
        sums = zero_arena.zeros((2 * C,), torch.float64, z.device)
    asums = torch.zeros_like(sums) if frozen else sums
    if _is16(z):                  # bf16-storage plan: the project conv's z_p is bf16, its gradient and dz are fp32 tensors
        tail = (a.data_ptr(), b.data_ptr(), mean.data_ptr(), invstd.data_ptr(), _opt(gscale, "gscale"), _opt(gadd, "gadd"))
        _lib.call("eat_bn_act_bwd_reduce_b16", _dev(dy, "dy"), 0, _dev16(z, "z"), *tail, B, C, S, act, sums.data_ptr(), _stream())
        dz = torch.empty(z.shape, device=z.device, dtype=torch.float32)
        dzc = torch.empty(z.shape, device=z.device, dtype=torch.bfloat16) if copy16 else None
        _lib.call("eat_bn_act_bwd_apply_b16", _dev(dy, "dy"), _dev16(z, "z"), *tail, asums.data_ptr(), dz.data_ptr(),
                  None if dzc is None else dzc.data_ptr(), B, C, S, act, _stream())
        if copy16:                 # (dz, its bf16 rounding): bf16-storage plan, z = the project conv's z_p
            dz = (dz, dzc)
        if not own:
            return dz, None, None
        sf = sums.float()
        return dz, sf[C:], sf[:C]
    args = (_dev(dy, "dy"), _dev(z, "z"), a.data_ptr(), b.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
            _opt(gscale, "gscale"), _opt(gadd, "gadd"))
    _lib.call("eat_bn_act_bwd_reduce", *args, B, C, S, act, sums.data_ptr(), _stream())
    dz = torch.empty_like(z)
    _lib.call("eat_bn_act_bwd_apply", *args, asums.data_ptr(), dz.data_ptr(), B, C, S, act, _stream())
    if not own:
        return dz, None, None
    sf = sums.float()
    return dz, sf[C:], sf[:C]


def se_bn_bwd_partials(d, z, a, b, mean, act):
    """One pass over (d, z) of a squeeze-excitation block -> P (5, B, C): P[0] = d s (the gate gradient, = plane_dot of d
    with act(a z + b)), P[1..4] the plane sums `bn_act_bwd_se` combines once gadd is known (csrc/train_fuse.hip)."""
    B, C = z.shape[0], z.shape[1]
    P = torch.empty((5, B, C), device=z.device, dtype=torch.float32)
    if _is16(z):
        _lib.call("eat_se_bn_bwd_partials_b16", _dev16(d, "dy"), _dev16(z, "z"), a.data_ptr(), b.data_ptr(), mean.data_ptr(),
                  P.data_ptr(), B, C, z.numel() // (B * C), act, _stream())
        return P
    _lib.call("eat_se_bn_bwd_partials", _dev(d, "dy"), _dev(z, "z"), a.data_ptr(), b.data_ptr(), mean.data_ptr(),
              P.data_ptr(), B, C, z.numel() // (B * C), act, _stream())
    return P


def bn_act_bwd_se(dy, z, a, b, mean, invstd, act, P, gscale, gadd, sums=None):
    """bn_act_bwd for a squeeze-excitation block whose plane sums P were taken by `se_bn_bwd_partials`: no reduce pass."""
    B, C = z.shape[0], z.shape[1]
    S = z.numel() // (B * C)
    own = sums is None
    if own:
        sums = torch.empty((2 * C,), device=z.device, dtype=torch.float64)
    _lib.call("eat_se_bn_bwd_combine", P.data_ptr(), _dev(gscale, "gscale"), _dev(gadd, "gadd"), invstd.data_ptr(), B, C,
              sums.data_ptr(), _stream())
    frozen = getattr(mean, "_eat_frozen", False)
    dz = torch.empty_like(z)
    asums = torch.zeros_like(sums) if frozen else sums
    _lib.call("eat_bn_act_bwd_apply", _dev(dy, "dy"), _dev(z, "z"), a.data_ptr(), b.data_ptr(), mean.data_ptr(),
              invstd.data_ptr(), gscale.data_ptr(), gadd.data_ptr(), asums.data_ptr(), dz.data_ptr(), B, C, S, act,
              _stream())
    if not own:
        return dz, None, None
    sf = sums.float()
    return dz, sf[C:], sf[:C]


def plane_dot(u, v, a=None, b=None, act=ACT_NONE):
    B, C = u.shape[0], u.shape[1]
    S = u.numel() // (B * C)
    out = torch.empty((B, C), device=u.device, dtype=torch.float32)
    _lib.call("eat_plane_dot", _dev(u, "u"), _dev(v, "v"), None if a is None else a.data_ptr(),
              None if b is None else b.data_ptr(), out.data_ptr(), B, C, S, act, _stream())
    return out


def dw_conv_dgrad(dz, w, x_shape, k, stride, res=None):
    B, C, F, T = x_shape
    Fo, To = dz.shape[2], dz.shape[3]
    dx = torch.empty(x_shape, device=dz.device, dtype=torch.float32)
    _lib.call("eat_dw_conv_dgrad", _dev(dz, "dz"), _dev(w, "w"), _opt(res, "res"), dx.data_ptr(), B, C, F, T, Fo, To,
              k, stride, _stream())
    return dx


def dw_conv_wgrad(dz, x, k, stride):
    B, C, Fo, To = dz.shape
    XC, F, T = x.shape[1], x.shape[2], x.shape[3]
    dw = zero_arena.zeros((C, k * k), torch.float32, dz.device)
    _lib.call("eat_dw_conv_wgrad", _dev(dz, "dz"), _dev(x, "x"), dw.data_ptr(), B, C, XC, F, T, Fo, To, k, stride,
              _stream())
    return dw


def dw_conv_wgrad_tf(dz, x, in_a, in_b, in_act, k, stride):
    """Depthwise weight gradient whose x operand is act_in(in_a[c] * x + in_b[c]), evaluated on load."""
    B, C, Fo, To = dz.shape
    F, T = x.shape[2], x.shape[3]
    dw = zero_arena.zeros((C, k * k), torch.float32, dz.device)
    _lib.call("eat_dw_conv_wgrad_tf", _dev(dz, "dz"), _dev(x, "x"), _dev(in_a, "in_a"), _dev(in_b, "in_b"), in_act,
              dw.data_ptr(), B, C, F, T, Fo, To, k, stride, _stream())
    return dw


def _pack_wmode(wp, per_sample=False):
    """`wmode` of the 1x1 entry points for a weight pack: 0 = fp32, 1 = plain bf16, 2 = bf16 hi / lo (per-sample bf16 packs
    are hi / lo)."""
    if wp.dtype == torch.float32:
        return 0
    return 2 if (per_sample or getattr(wp, "_eat_split", False)) else 1


def _stat_partials(B, S, Co, device, per_sample=False):
    """The [tile][2][Co] partial sums a 1x1 conv's statistics epilogue writes -> (part, tiles)."""
    tiles = int(_lib.lib().eat_pw_conv_stat_tiles(B, S, 1 if per_sample else 0))
    return torch.empty((tiles * 2 * Co,), device=device, dtype=torch.float32), tiles


def _gstat_finish(part, tiles, Co, st, sums):
    """BatchNorm-backward sums (2 Co,) float64 from the partials of a `gstats` epilogue; st = (a, b, mean, invstd)."""
    a, b, mean, invstd = st
    if sums is None:
        sums = torch.empty((2 * Co,), device=part.device, dtype=torch.float64)
    nws = int(_lib.lib().eat_bn_bwd_sums_ws_doubles(tiles, Co))
    ws = torch.empty((nws,), device=part.device, dtype=torch.float64) if nws else None
    _lib.call("eat_bn_bwd_sums_from_tiles", part.data_ptr(), tiles, Co, mean.data_ptr(), invstd.data_ptr(), a.data_ptr(),
              b.data_ptr(), None if ws is None else ws.data_ptr(), sums.data_ptr(), _stream())
    return sums


def pw_tf_eligible(Ci, S):
    """Geometry of the on-load BatchNorm + activation of the 1x1 kernels (eat_pw_conv_tf_fwd / eat_pw_conv_wgrad_tf)."""
    return Ci % 8 == 0 and S % 4 == 0


def pw_conv_tf(x, tf, wp, bias, Co, act, in_scale=None, res=None):
    """1x1 conv of act_in(tf_a[k] x + tf_b[k]) [* in_scale] evaluated on load; tf = (a, b, act_in); wp from `pw_prepack`."""
    B, Ci, F, T = x.shape
    wmode = _pack_wmode(wp)
    y = torch.empty((B, Co, F, T), device=x.device, dtype=torch.float32)
    _lib.call("eat_pw_conv_tf_fwd", _dev(x, "x"), tf[0].data_ptr(), tf[1].data_ptr(), tf[2], wp.data_ptr(), wmode,
              _dev(bias, "bias"), _opt(in_scale, "in_scale"), _opt(res, "res"), y.data_ptr(), B, Ci, Co, F * T, act,
              _stream())
    return y


def pw_conv_cat(x1, x2, wp, bias, Co, act, res=None):
    """1x1 conv over the concatenated channels of x1 (B,C1,F,T) and x2 (B,C2,F,T) without materialising the concatenation;
    wp = pw_prepack of the (Co, C1 + C2) matrix."""
    B, C1, F, T = x1.shape
    C2 = x2.shape[1]
    wmode = _pack_wmode(wp)
    y = torch.empty((B, Co, F, T), device=x1.device, dtype=torch.float32)
    _lib.call("eat_pw_conv_cat_fwd", _dev(x1, "x"), C1, _dev(x2, "x2"), C2, wp.data_ptr(), wmode, _dev(bias, "bias"),
              _opt(res, "res"), y.data_ptr(), B, Co, F * T, act, _stream())
    return y


def _wgrad_ws(B, Co, Ci, S, mode, same, x_scale, tf, reproducible):
    """Workspace of `eat_pw_conv_wgrad_ws` / `_tf` / `eat_gram_centered`: (copies of dW, zero-filled?), (0, False) = none.
    The stored-slice (wide-tile) kernel wants one copy per k-slice and writes every element of them: no zero fill.  The atomic
    kernels add into their copies: `reproducible` asks for one zeroed copy per block (`eat_pw_wgrad_slots`); otherwise the
    streaming kernel of the small matrices spreads its atomics over 8 zeroed copies (same-address atomics serialise in L2) and
    the other kernels take none."""
    h = _lib.lib()
    if not reproducible and Co <= 64 and Ci <= 64 and S % 4 == 0 and mode != 1:
        return 8, True
    stored = tf is None and h.eat_pw_wgrad_kernel_kind(B, Co, Ci, S, mode, 1 if same else 0, 1 if x_scale else 0, 0) == 3
    if reproducible or stored:
        return int(h.eat_pw_wgrad_slots(B, Co, Ci, S, mode, 1 if same else 0)), not stored
    return 0, False


def _ws_alloc(n_floats, zeroed, dev):
    return zero_arena.zeros((n_floats,), torch.float32, dev) if zeroed else torch.empty((n_floats,), dtype=torch.float32, device=dev)


def gram(x, exact=False, sx=None, plain_bf16=False):
    """G (C, C) = sum_{b,s} x x^T, bit-reproducible from run to run: every block of the weight-gradient kernel adds into
    its own zeroed copy and the copies are summed in a fixed order (the BatchNorm statistics of the expand conv follow
    from G - csrc/train_fuse.hip - so its round-off decides on which side of a ReLU / Hardswish kink activations fall).
    sx (C,) = sum_{b,s} x: the CENTRED matrix Gc = sum (x - m)(x - m)^T, m = sx / n, instead (`centered=True` in
    `gram_bn_state*` / `expand_bwd_coef`): the variance w^T Gc w / n is then not a difference of two large sums.
    plain_bf16: single bf16 products (the bf16-storage plan: the conv output these statistics describe is itself stored
    with 2^-9 relative rounding; the centring happens BEFORE the rounding, the accumulation stays fp32)."""
    B, C = x.shape[0], x.shape[1]
    S = x.numel() // (B * C)
    mode = 1 if exact else (2 if plain_bf16 else 0)
    # (64 < C <= 160: the wide-tile kernel STORES its per-slice copies - no zero fill needed for them)
    slots, zeroed = _wgrad_ws(B, C, C, S, mode, True, False, None, reproducible=True)
    G = zero_arena.zeros((C, C), torch.float32, x.device)
    if sx is not None:                                      # (the workspace holds the 2 C centring coefficients first)
        ws = _ws_alloc(2 * C + slots * C * C, zeroed, x.device)
        _lib.call("eat_gram_centered", _dev(x, "x"), _dev(sx, "sx"), 1.0 / (B * S), G.data_ptr(), ws.data_ptr(), slots, B, C,
                  S, mode, _stream())
    else:
        ws = _ws_alloc(slots * C * C, zeroed, x.device)
        _lib.call("eat_pw_conv_wgrad_ws", _dev(x, "x"), _dev(x, "x"), None, G.data_ptr(), ws.data_ptr(), slots, B, C, C, S,
                  mode, _stream())
    return G


def pw_conv_wgrad(dz, x, x_scale=None, exact=None, tf=None, out=None):
    """dW (Co, Ci) = sum_b dz[b] (Co,S) . (x[b] * x_scale[b])^T.  exact=True: fp32 MFMA kernel; False: split-operand
    bf16x3 kernel (fp32-class); None: follow the active `precision` context ('fp32' -> exact, 'bf16' -> plain bf16
    operands with fp32 accumulation, as autocast does to the conv weight gradient; otherwise bf16x3).
    tf = (a, b, act): the x operand is act(a[ci] x + b[ci]), evaluated on load (`eat_pw_conv_wgrad_tf`)."""
    mode = 1 if exact else 0
    if exact is None:
        mode = {"fp32": 1, "bf16": 2}.get(precision.mode, 0)
    B, Co = dz.shape[0], dz.shape[1]
    Ci = x.shape[1]
    S = dz.numel() // (B * Co)
    # out: ZERO-FILLED (Co, Ci) memory to accumulate into (dp.GradReducer.alloc: the gradient is produced inside its bucket)
    dW = out if out is not None else zero_arena.zeros((Co, Ci), torch.float32, dz.device)
    n, zeroed = _wgrad_ws(B, Co, Ci, S, mode, dz.data_ptr() == x.data_ptr(), x_scale is not None, tf, reproducible=False)
    ws = _ws_alloc(n * Co * Ci, zeroed, dz.device) if n else None
    if tf is not None:
        _lib.call("eat_pw_conv_wgrad_tf", _dev(dz, "dz"), _dev(x, "x"), tf[0].data_ptr(), tf[1].data_ptr(), tf[2],
                  _opt(x_scale, "x_scale"), dW.data_ptr(), None if ws is None else ws.data_ptr(), n, B, Co, Ci, S, mode,
                  _stream())
    elif ws is not None:
        _lib.call("eat_pw_conv_wgrad_ws", _dev(dz, "dz"), _dev(x, "x"), _opt(x_scale, "x_scale"), dW.data_ptr(),
                  ws.data_ptr(), n, B, Co, Ci, S, mode, _stream())
    else:
        _lib.call("eat_pw_conv_wgrad", _dev(dz, "dz"), _dev(x, "x"), _opt(x_scale, "x_scale"), dW.data_ptr(), B, Co, Ci,
                  S, mode, _stream())
    return dW


# ------------------------------------------------------------------ round-3 training launchers (csrc/train_fuse.hip)
import ctypes as _ct


def dw_partials_inner(F, T, Fo, To, k, stride, dgrad):
    """Upper bound of the partial slots per plane the fused training epilogues write (host helper)."""
    return int(_lib.lib().eat_dw_partials_inner(F, T, Fo, To, k, stride, 1 if dgrad else 0))


def dw_bwd_split(B, C, F, T, Fo, To, k, stride, bn):
    """How the merged depthwise backward cuts a shape (eat_dw_bwd_split: the launcher's own arithmetic; no device work):
    None where the geometry is not on that kernel, else {lane_group: 16 / 32 / 64, whole_rows: bool, tile_rows: 4 / 8,
    G: sample groups a wave walks, inner: tiles per plane}.  bn: the BatchNorm-on-load entry points."""
    out = [_ct.c_int(0) for _ in range(5)]
    if _lib.call_rc("eat_dw_bwd_split", B, C, F, T, Fo, To, k, stride, 1 if bn else 0, *[_ct.addressof(o) for o in out]):
        return None
    lane_group, whole_rows, tile_rows, G, inner = (o.value for o in out)
    return {"lane_group": lane_group, "whole_rows": bool(whole_rows), "tile_rows": tile_rows, "G": G, "inner": inner}


DW_WGRAD_KERNELS = ("plane", "tile", "column", "stem", "channel")


def dw_wgrad_split(B, C, XC, F, T, Fo, To, k, stride, per_sample=False):
    """Which kernel a depthwise weight-gradient call runs on and how it cuts the batch (eat_dw_wgrad_split; no device work):
    {kernel: one of DW_WGRAD_KERNELS, split: G (plane, tile) / samples per block (column, channel) / rows per block (stem),
    parts: sample groups / batch slices / row chunks, lane_samples: samples side by side in a wave}."""
    out = [_ct.c_int(0) for _ in range(3)]
    kind = int(_lib.lib().eat_dw_wgrad_split(B, C, XC, F, T, Fo, To, k, stride, 1 if per_sample else 0,
                                             *[_ct.addressof(o) for o in out]))
    if kind < 0:
        raise _lib.EatHipError(f"eat_dw_wgrad_split: no weight-gradient kernel takes C={C} XC={XC} k={k} stride={stride}")
    split, parts, lane_samples = (o.value for o in out)
    return {"kernel": DW_WGRAD_KERNELS[kind], "split": split, "parts": parts, "lane_samples": lane_samples}


def dw_conv_stats(x, w, k, stride, tf=None, out_b16=False):
    """Train-mode depthwise conv + the partial sums of its output for the BatchNorm that follows.
    tf = (in_a, in_b, in_act): the conv input is act(in_a[c] x + in_b[c]) evaluated on load.
    -> (y, (part, outer, inner)) for `bn_state_from_partials`.  A bf16 x - or out_b16 with an fp32 x - selects the
    bf16-storage kernels: y bf16, statistics of the stored values."""
    B, C, F, T = x.shape
    Fo, To = conv_out(F, k, stride), conv_out(T, k, stride)
    cap = dw_partials_inner(F, T, Fo, To, k, stride, False)
    x16 = _is16(x)
    y = torch.empty((B, C, Fo, To), device=x.device, dtype=torch.bfloat16 if (x16 or out_b16) else torch.float32)
    part = torch.empty((B * 2 * C * cap,), device=x.device, dtype=torch.float32)
    inner = _ct.c_int(0)
    a, b, act = tf if tf is not None else (None, None, 0)
    if x16 or out_b16:                             # bf16 storage: z_e (or the fp32 stem output) in, z_d out, statistics of the stored z_d
        _lib.call("eat_dw_conv_fwd_stats_b16", _dev16(x, "x") if x16 else _dev(x, "x"), 1 if x16 else 0, _opt(a, "in_a"),
                  _opt(b, "in_b"), act, _dev(w, "w"),
                  y.data_ptr(), part.data_ptr(), cap, _ct.addressof(inner), B, C, F, T, Fo, To, k, stride, _stream())
        return y, (part, B, inner.value)
    _lib.call("eat_dw_conv_fwd_stats", _dev(x, "x"), _opt(a, "in_a"), _opt(b, "in_b"), act, _dev(w, "w"), y.data_ptr(),
              part.data_ptr(), cap, _ct.addressof(inner), B, C, F, T, Fo, To, k, stride, _stream())
    return y, (part, B, inner.value)


def bn_stats_partial(z):
    B, C = z.shape[0], z.shape[1]
    part = torch.empty((B * 2 * C,), device=z.device, dtype=torch.float32)
    _lib.call("eat_bn_stats_partial", _dev(z, "z"), B, C, z.numel() // (B * C), part.data_ptr(), _stream())
    return part, B, 1


def _bn_momentum(bn):
    mom = bn.momentum
    if mom is None:
        mom = 1.0 / (int(bn.num_batches_tracked) + 1)          # host read: this mode is not graph-capturable
    return float(mom)


def bn_state_from_partials(parts, bn, n):
    """(a, b, mean, invstd) of a TRAINING BatchNorm layer from the producer's partial sums; updates the running buffers
    and num_batches_tracked as `bn_train_state` does."""
    part, outer, inner = parts
    C = bn.num_features
    out = torch.empty((4, C), device=part.device, dtype=torch.float32)
    nws = int(_lib.lib().eat_bn_finalize_ws_doubles(outer, C, inner))      # > 0: many partial rows, summed in groups first
    ws = torch.empty((nws,), device=part.device, dtype=torch.float64) if nws else None
    _lib.call("eat_bn_finalize_partials", part.data_ptr(), outer, C, inner, _dev(bn.weight, "gamma"), _dev(bn.bias, "beta"),
              bn.running_mean.data_ptr(), bn.running_var.data_ptr(), _bn_momentum(bn), float(bn.eps), float(n),
              out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
              None if ws is None else ws.data_ptr(), _stream())
    bn_counters.bump(bn)
    return out[0], out[1], out[2], out[3]


def gram_bn_state(Tm, W, sx, bn, n, centered=False):
    """(a, b, mean, invstd) of the TRAINING BatchNorm after the 1x1 conv z = W x from Tm = W G, sx (Gram matrix / sum of
    the conv input): see csrc/train_fuse.hip."""
    Co, Ci = W.shape
    out = torch.empty((4, Co), device=W.device, dtype=torch.float32)
    _lib.call("eat_gram_bn_finalize", _dev(Tm, "Tm"), _dev(W, "W"), _dev(sx, "sx"), Co, Ci, _dev(bn.weight, "gamma"),
              _dev(bn.bias, "beta"), bn.running_mean.data_ptr(), bn.running_var.data_ptr(), _bn_momentum(bn),
              float(bn.eps), float(n), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
              1 if centered else 0, _stream())
    bn_counters.bump(bn)
    return out[0], out[1], out[2], out[3]


def gram_bn_state_g(G, W, sx, bn, n, centered=False):
    """`gram_bn_state` straight from the Gram matrix G: -> (Tm = W G, (a, b, mean, invstd)); one launch, fp64 inside."""
    Co, Ci = W.shape
    out = torch.empty((4 * Co + Co * Ci,), device=W.device, dtype=torch.float32)
    st, Tm = out[:4 * Co].view(4, Co), out[4 * Co:].view(Co, Ci)
    _lib.call("eat_gram_bn_finalize_g", _dev(G, "G"), _dev(W, "W"), _dev(sx, "sx"), Co, Ci, _dev(bn.weight, "gamma"),
              _dev(bn.bias, "beta"), bn.running_mean.data_ptr(), bn.running_var.data_ptr(), _bn_momentum(bn),
              float(bn.eps), float(n), Tm.data_ptr(), st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(),
              st[3].data_ptr(), 1 if centered else 0, _stream())
    bn_counters.bump(bn)
    return Tm, (st[0], st[1], st[2], st[3])


def act_grad_sum(dy, z, a, b, act, inplace=False):
    """g = dy * act'(a[c] z + b[c]) and its per-plane sums -> (g, (gpart, B, 1))."""
    B, C = z.shape[0], z.shape[1]
    g = dy if inplace else torch.empty_like(dy)
    gpart = torch.empty((B * C,), device=z.device, dtype=torch.float32)
    _lib.call("eat_act_grad_sum", _dev(dy, "dy"), _dev(z, "z"), a.data_ptr(), b.data_ptr(), act, g.data_ptr(),
              gpart.data_ptr(), B, C, z.numel() // (B * C), _stream())
    return g, (gpart, B, 1)


def dw_conv_dgrad_g(dz, w, x_shape, k, stride, gz, ga, gb, gact):
    """Depthwise data gradient times act'(ga[c] gz + gb[c]) + its partial sums -> (g, (gpart, B, inner))."""
    B, C, F, T = x_shape
    Fo, To = dz.shape[2], dz.shape[3]
    cap = dw_partials_inner(F, T, Fo, To, k, stride, True)
    g = torch.empty(x_shape, device=dz.device, dtype=torch.float32)
    gpart = torch.empty((B * C * cap,), device=dz.device, dtype=torch.float32)
    inner = _ct.c_int(0)
    _lib.call("eat_dw_conv_dgrad_g", _dev(dz, "dz"), _dev(w, "w"), _dev(gz, "gz"), ga.data_ptr(), gb.data_ptr(), gact,
              g.data_ptr(), gpart.data_ptr(), cap, _ct.addressof(inner), B, C, F, T, Fo, To, k, stride, _stream())
    return g, (gpart, B, inner.value)


def dw_conv_bwd_g(dz, w, x, in_a, in_b, in_act, k, stride):
    """Merged depthwise backward: -> (g, (gpart, B, inner), dw) with g = dgrad(dz) * act'(in_a x + in_b) and dw the weight
    gradient w.r.t. the conv input act(in_a x + in_b); dz and x are read once (csrc/dw_plane.hip: dw_bwd_tile_kernel)."""
    B, C, F, T = x.shape
    Fo, To = dz.shape[2], dz.shape[3]
    h = _lib.lib()
    cap = max(int(h.eat_dw_bwd_partials_inner(F, T, Fo, To, k, stride)), dw_partials_inner(F, T, Fo, To, k, stride, True))
    g = torch.empty((B, C, F, T), device=dz.device, dtype=torch.float32)
    gpart = torch.empty((B * C * cap,), device=dz.device, dtype=torch.float32)
    dw = zero_arena.zeros((C, k * k), torch.float32, dz.device)
    inner = _ct.c_int(0)
    _lib.call("eat_dw_conv_bwd_g", _dev(dz, "dz"), _dev(x, "x"), in_a.data_ptr(), in_b.data_ptr(), in_act, _dev(w, "w"),
              g.data_ptr(), dw.data_ptr(), gpart.data_ptr(), cap, _ct.addressof(inner), B, C, F, T, Fo, To, k, stride,
              _stream())
    return g, (gpart, B, inner.value), dw


def dw_bwd_merged_ok(dy_shape, x_shape, k, stride):
    """True where the merged depthwise backward kernel runs (large planes): `dw_conv_bwd_bn_g` is available there."""
    B, C, F, T = x_shape
    return bool(_lib.lib().eat_dw_bwd_merged_ok(B, C, F, T, dy_shape[2], dy_shape[3], k, stride))


def bn_act_bwd_sums(dy, z, a, b, mean, invstd, act, gscale=None, gadd=None, se_P=None, sums=None):
    """The reduce half of `bn_act_bwd` / `bn_act_bwd_se`: -> (sums (2C,) float64, dgamma, dbeta); dz is left to the consumer
    (`dw_conv_bwd_bn_g` evaluates it on load)."""
    B, C = z.shape[0], z.shape[1]
    S = z.numel() // (B * C)
    own = sums is None
    if se_P is not None:
        if own:
            sums = torch.empty((2 * C,), device=z.device, dtype=torch.float64)
        _lib.call("eat_se_bn_bwd_combine", se_P.data_ptr(), _dev(gscale, "gscale"), _dev(gadd, "gadd"), invstd.data_ptr(), B,
                  C, sums.data_ptr(), _stream())
    else:
        if own:
            sums = zero_arena.zeros((2 * C,), torch.float64, z.device)
        b16 = _is16(z)
        tail = (a.data_ptr(), b.data_ptr(), mean.data_ptr(), invstd.data_ptr(), _opt(gscale, "gscale"), _opt(gadd, "gadd"), B, C, S,
                act, sums.data_ptr(), _stream())
        if b16:
            _lib.call("eat_bn_act_bwd_reduce_b16", _dev16(dy, "dy"), 1, _dev16(z, "z"), *tail)
        else:
            _lib.call("eat_bn_act_bwd_reduce", _dev(dy, "dy"), _dev(z, "z"), *tail)
    if not own:
        return sums, None, None
    sf = sums.float()
    return sums, sf[C:], sf[:C]


def dw_conv_bwd_bn_g(dy, z, st, act, sums, w, x, in_a, in_b, in_act, k, stride, gscale=None, gadd=None, want_gsum=True):
    """Merged depthwise backward with the BatchNorm + activation backward of the conv's own output evaluated on load from
    (dy, z): -> (g, (gpart, B, inner) or None, dw).  st = the forward's (a, b, mean, invstd); only where `dw_bwd_merged_ok`."""
    B, C, F, T = x.shape
    Fo, To = z.shape[2], z.shape[3]
    h = _lib.lib()
    cap = int(h.eat_dw_bwd_partials_inner(F, T, Fo, To, k, stride))
    b16 = _is16(z)                                 # bf16 storage: dy and z bf16; x and g bf16 (or both fp32: the first block)
    g = torch.empty((B, C, F, T), device=z.device, dtype=x.dtype if b16 else torch.float32)
    gpart = torch.empty((B * C * cap,), device=z.device, dtype=torch.float32) if want_gsum else None
    dw = zero_arena.zeros((C, k * k), torch.float32, z.device)
    inner = _ct.c_int(0)
    frozen = 1 if getattr(st[2], "_eat_frozen", False) else 0
    if b16:
        _lib.call("eat_dw_conv_bwd_bn_g_b16", _dev16(dy, "dy"), _dev16(z, "z"), st[0].data_ptr(), st[1].data_ptr(),
                  st[2].data_ptr(), st[3].data_ptr(), _opt(gscale, "gscale"), _opt(gadd, "gadd"), sums.data_ptr(), act, frozen,
                  _dev16(x, "x") if _is16(x) else _dev(x, "x"), 1 if _is16(x) else 0, in_a.data_ptr(), in_b.data_ptr(), in_act,
                  _dev(w, "w"), g.data_ptr(), dw.data_ptr(),
                  None if gpart is None else gpart.data_ptr(), cap, _ct.addressof(inner), B, C, F, T, Fo, To, k, stride,
                  _stream())
        return g, ((gpart, B, inner.value) if want_gsum else None), dw
    _lib.call("eat_dw_conv_bwd_bn_g", _dev(dy, "dy"), _dev(z, "z"), st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(),
              st[3].data_ptr(), _opt(gscale, "gscale"), _opt(gadd, "gadd"), sums.data_ptr(), act, frozen, _dev(x, "x"),
              in_a.data_ptr(), in_b.data_ptr(), in_act, _dev(w, "w"), g.data_ptr(), dw.data_ptr(),
              None if gpart is None else gpart.data_ptr(), cap, _ct.addressof(inner), B, C, F, T, Fo, To, k, stride,
              _stream())
    return g, ((gpart, B, inner.value) if want_gsum else None), dw


def se_mlp_bwd(ds, scale, h, pool, W1, W2, S, dW1_out=None, dW2_out=None):
    """Backward of the SE gate MLP in two launches -> (dW1, db1, dW2, db2, gadd); see csrc/se_train.hip."""
    B, C = ds.shape
    Cr = h.shape[1]
    dev = ds.device
    n_dh = int(_lib.lib().eat_se_mlp_dh_floats(B, C, Cr))            # dh + its k slices where the contraction is split
    buf = torch.empty((2 * C * Cr + C + Cr + n_dh + B * C,), device=dev, dtype=torch.float32)
    o = 0
    dW1 = buf[o:o + Cr * C].view(Cr, C); o += Cr * C
    dW2 = buf[o:o + C * Cr].view(C, Cr); o += C * Cr
    dW1 = dW1_out if dW1_out is not None else dW1            # (written, not accumulated: memory of the gradient buckets)
    dW2 = dW2_out if dW2_out is not None else dW2
    db1 = buf[o:o + Cr]; o += Cr
    db2 = buf[o:o + C]; o += C
    dh = buf[o:o + n_dh]; o += n_dh
    gadd = buf[o:o + B * C].view(B, C)
    _lib.call("eat_se_mlp_bwd", _dev(ds, "ds"), _dev(scale, "scale"), _dev(h, "h"), _dev(pool, "pool"), _dev(W1, "W1"),
              _dev(W2, "W2"), 1.0 / S, dW1.data_ptr(), db1.data_ptr(), dW2.data_ptr(), db2.data_ptr(), dh.data_ptr(),
              gadd.data_ptr(), B, C, Cr, _stream())
    return dW1, db1, dW2, db2, gadd


def mlp_head_bwd(dlogits, h2, u, drop_mask, feat, W1, W2, dW1_out=None, dW2_out=None):
    """Backward of the classifier head Linear -> Hardswish -> Dropout -> Linear in two launches (csrc/se_train.hip):
    -> (dW1, db1, dW2, db2, dfeat)."""
    B, N = dlogits.shape
    H, C = W1.shape
    dev = dlogits.device
    n_df = int(_lib.lib().eat_mlp_head_dfeat_floats(B, C, H))       # dfeat + its k slices where the contraction is split
    buf = torch.empty((H * C + H + N * H + N + B * H + n_df,), device=dev, dtype=torch.float32)
    o = 0
    dW1 = buf[o:o + H * C].view(H, C); o += H * C
    db1 = buf[o:o + H]; o += H
    dW2 = buf[o:o + N * H].view(N, H); o += N * H
    dW1 = dW1_out if dW1_out is not None else dW1            # (written, not accumulated: memory of the gradient buckets)
    dW2 = dW2_out if dW2_out is not None else dW2
    db2 = buf[o:o + N]; o += N
    du = buf[o:o + B * H]; o += B * H
    dfeat = buf[o:o + B * C].view(B, C)
    _lib.call("eat_mlp_head_bwd", _dev(dlogits, "dy"), _dev(h2, "h2"), _dev(u, "u"), _opt(drop_mask, "drop_mask"),
              _dev(feat, "feat"), _dev(W1, "W1"), _dev(W2, "W2"), dW1.data_ptr(), db1.data_ptr(), dW2.data_ptr(),
              db2.data_ptr(), du.data_ptr(), dfeat.data_ptr(), B, C, H, N, _stream())
    return dW1, db1, dW2, db2, dfeat


def stem_gram(x, W):
    """(Tm = W G9 (C, 9), sp (9)) of the stem conv's 3x3 / stride-2 patches of the log-mel x (B, 1, F, T): feeds
    `gram_bn_state` (csrc/stem_train.hip).  Bit-reproducible."""
    B, _, F, T = x.shape
    C = W.shape[0]
    Fo = (F - 1) // 2 + 1
    nblk = int(_lib.lib().eat_stem_gram_blocks(B, Fo))
    part = torch.empty((nblk, 54), device=x.device, dtype=torch.float32)
    out = torch.empty((C * 9 + 9,), device=x.device, dtype=torch.float32)
    Tm, sp = out[:C * 9].view(C, 9), out[C * 9:]
    _lib.call("eat_stem_gram", _dev(x, "x"), _dev(W, "W"), part.data_ptr(), Tm.data_ptr(), sp.data_ptr(), B, C, F, T,
              _stream())
    return Tm, sp


def stem_bwd(dy, x, W, a, b, act, dy2=None):
    """-> (Gx (C, 9) = sum g p^T, (s1, 1, 1)) with g = dy * act'(a (W p) + b): the stem's weight-gradient pass with the
    BatchNorm + activation backward folded in (`expand_bwd_coef` finishes)."""
    B, _, F, T = x.shape
    C = W.shape[0]
    buf = torch.empty((C * 10,), device=x.device, dtype=torch.float32)
    gx, s1 = buf[:C * 9].view(C, 9), buf[C * 9:]
    nblk = int(_lib.lib().eat_stem_bwd_blocks(B, (F - 1) // 2 + 1))
    part = torch.empty((nblk, C, 10), device=x.device, dtype=torch.float32)
    _lib.call("eat_stem_bwd", _dev(dy, "dy"), _opt(dy2, "dy2"), _dev(x, "x"), _dev(W, "W"), a.data_ptr(), b.data_ptr(), act,
              part.data_ptr(), gx.data_ptr(), s1.data_ptr(), B, C, F, T, _stream())
    return gx, (s1, 1, 1)


def expand_bwd_coef(W, Gx, Tm, sx, gparts, a, mean, invstd, n, frozen=False, need_dx=True, centered=False, dW_out=None):
    """-> (dW, dgamma, dbeta, WaT (Ci,Co), M (Ci,Ci), c0 (Ci)): backward of conv1x1 -> BN(train) -> act without dz."""
    gpart, outer, inner = gparts
    Co, Ci = W.shape
    dev = W.device
    dW = dW_out if dW_out is not None else torch.empty((Co, Ci), device=dev, dtype=torch.float32)   # (written, not accumulated)
    vec = torch.empty((2, Co), device=dev, dtype=torch.float32)           # dgamma, dbeta
    tr = torch.empty((3 * Ci + 1, Co), device=dev, dtype=torch.float32)   # WaT, WT, [W2T ; e1]: M and c0 from ONE GEMM
    w2e = tr[2 * Ci:]
    tr = (tr[:Ci], tr[Ci:2 * Ci], w2e[:Ci])
    _lib.call("eat_expand_bwd_coef", _dev(W, "W"), _dev(Gx, "Gx"), _dev(Tm, "Tm"), _dev(sx, "sx"), gpart.data_ptr(),
              outer, inner, Co, Ci, a.data_ptr(), mean.data_ptr(), invstd.data_ptr(), float(n), 1 if frozen else 0,
              dW.data_ptr(), vec[0].data_ptr(), vec[1].data_ptr(), tr[0].data_ptr(), tr[1].data_ptr(), tr[2].data_ptr(),
              w2e[Ci].data_ptr(), 1 if centered else 0, None, _stream())
    if frozen or not need_dx:
        return dW, vec[0], vec[1], tr[0], None, None
    if precision.mode != "fp32" and Ci % 4 == 0 and Co % 4 == 0 and W.is_contiguous():
        # [W2T ; e1] . W as the 1x1 conv of the "image" W (1, Co, Ci, 1) with the (Ci + 1, Co) matrix on the split-operand
        # bf16x3 kernel (fp32-class products; round 5: the K-split `linear` kernel ran these C_in x C_in x C_exp products at
        # 15 TFLOP/s - 14 launches of up to 213 us in the mn40 step)
        wp3 = pw_prepack_bf16(w2e, None, split=True)
        Mc = pw_conv_bf16(W.view(1, Co, Ci, 1), wp3, zeros_vec.get(Ci + 1, dev), Ci + 1, ACT_NONE, split=True).view(Ci + 1, Ci)
    else:
        Mc = linear(w2e, tr[1], None, ACT_NONE)                            # [W2T ; e1] . WT^T -> (Ci + 1, Ci)
    return dW, vec[0], vec[1], tr[0], Mc[:Ci], Mc[Ci]


def cat_pack_kind(K):
    """The pack `pw_prepack` would choose for a matrix with K reduction channels under the active precision
    (0 fp32 fragments, 1 bf16, 2 bf16 hi + lo)."""
    m = precision.mode
    if m == "bf16":
        return 1
    if m == "bf16x3" or (m == "auto" and K >= 40 and K % 4 == 0):
        return 2
    return 0


def expand_bwd_coef_cat(W, Gx, Tm, sx, gparts, a, mean, invstd, n, centered=False, dW_out=None):
    """`expand_bwd_coef` for the two-source data-gradient GEMM: -> (dW, dgamma, dbeta, wcat, c0) with wcat = the weight pack
    of [WaT | M] (Ci x (Co + Ci)) and c0 (Ci) written by ONE launch (csrc/train_fuse.hip: eat_expand_bwd_wcat) - no
    transposes, no separate M GEMM, no torch.cat, no prepack launches.  Training BatchNorm (not frozen) only."""
    gpart, outer, inner = gparts
    Co, Ci = W.shape
    dev = W.device
    dW = dW_out if dW_out is not None else torch.empty((Co, Ci), device=dev, dtype=torch.float32)
    vec = torch.empty((4, Co), device=dev, dtype=torch.float32)           # dgamma, dbeta, e1, e2
    _lib.call("eat_expand_bwd_coef", _dev(W, "W"), _dev(Gx, "Gx"), _dev(Tm, "Tm"), _dev(sx, "sx"), gpart.data_ptr(),
              outer, inner, Co, Ci, a.data_ptr(), mean.data_ptr(), invstd.data_ptr(), float(n), 0,
              dW.data_ptr(), vec[0].data_ptr(), vec[1].data_ptr(), None, None, None, vec[2].data_ptr(),
              1 if centered else 0, vec[3].data_ptr(), _stream())
    kind = cat_pack_kind(Co + Ci)
    nel = int(_lib.lib().eat_expand_bwd_wcat_elems(Co, Ci, kind))
    wcat = torch.empty((nel,), device=dev, dtype=torch.float32 if kind == 0 else torch.bfloat16)
    if kind == 2:
        wcat._eat_split = True
    c0 = torch.empty((Ci,), device=dev, dtype=torch.float32)
    _lib.call("eat_expand_bwd_wcat", _dev(W, "W"), a.data_ptr(), vec[3].data_ptr(), vec[2].data_ptr(), Co, Ci, kind,
              wcat.data_ptr(), c0.data_ptr(), _stream())
    return dW, vec[0], vec[1], wcat, c0


# ------------------------------------------------------------------------- DyMN launchers
def ctx_pool(x):
    B, C, F, T = x.shape
    seq = torch.empty((B, F + T, C), device=x.device, dtype=torch.float32)
    _lib.call("eat_ctx_pool", _dev(x, "x"), seq.data_ptr(), B, C, F, T, _stream())
    return seq


def ctx_pool_bwd(dseq, shape):
    """dseq (B, F+T, C) -> dx (B, C, F, T) of `ctx_pool`."""
    B, C, F, T = shape
    dx = torch.empty(shape, device=dseq.device, dtype=torch.float32)
    _lib.call("eat_ctx_pool_bwd", _dev(dseq, "dseq"), None, dx.data_ptr(), B, C, F, T, _stream())
    return dx


def dyn_aggregate(bank, att, gscale=None, group=1):
    K, N = bank.shape
    B = att.shape[0]
    out = torch.empty((B, N), device=bank.device, dtype=torch.float32)
    _lib.call("eat_dyn_aggregate", _dev(bank, "bank"), _dev(att, "att"), _opt(gscale, "gscale"), out.data_ptr(), B, K,
              N, group, _stream())
    return out


def dyn_bank_grad(G, att, bank, datt=None):
    """Gradients of the kernel aggregation W_b = sum_k att[b,k] bank[k] from the per-sample weight gradients G (B, N):
    -> (dbank (K, N) = att^T G, datt (B, K) = G bank^T).  datt: zeroed (B, K) memory to accumulate into (a slice of a
    block's (n_att, B, K) tensor), or None."""
    B, K, N = att.shape[0], bank.shape[0], bank.shape[1]
    dbank = torch.empty_like(bank)
    if datt is None:
        datt = zero_arena.zeros(tuple(att.shape), torch.float32, att.device)
    _lib.call("eat_dyn_bank_grad", _dev(G, "G"), _dev(att, "att"), _dev(bank, "bank"), dbank.data_ptr(), _dev(datt, "datt"),
              B, K, N, _stream())
    return dbank, datt


def dyn_heads_fwd(y, n_att, K, cexp, inv_t, lam, iv):
    """Pointwise tails of the Linear layers that read h_c, y (B, n_att*K + 4*cexp) being their row-concatenated output:
    -> (att (n_att, B, K) = softmax(logits * inv_t), sg (B, 4*cexp) = sigmoid(.), coef (B, cexp, 4) = (2 sg - 1) * lam + iv)."""
    B = y.shape[0]
    att = torch.empty((n_att, B, K), device=y.device, dtype=torch.float32)
    sg = torch.empty((B, 4 * cexp), device=y.device, dtype=torch.float32)
    coef = torch.empty((B, cexp, 4), device=y.device, dtype=torch.float32)
    _lib.call("eat_dyn_heads_fwd", _dev(y, "y"), B, n_att, K, cexp, inv_t[0], inv_t[1], inv_t[2], _dev(lam, "lambdas"),
              _dev(iv, "init_v"), att.data_ptr(), sg.data_ptr(), coef.data_ptr(), _stream())
    return att, sg, coef


def dyn_heads_bwd(datt, dcoef, att, sg, lam, cexp, inv_t):
    """-> dy (B, n_att*K + 4*cexp) of `dyn_heads_fwd`."""
    n_att, B, K = att.shape
    dy = torch.empty((B, n_att * K + 4 * cexp), device=att.device, dtype=torch.float32)
    _lib.call("eat_dyn_heads_bwd", _dev(datt, "datt"), _dev(dcoef, "dcoef"), _dev(att, "att"), _dev(sg, "sg"),
              _dev(lam, "lambdas"), B, n_att, K, cexp, inv_t[0], inv_t[1], inv_t[2], dy.data_ptr(), _stream())
    return dy


def dyn_pw_pack(bank, att, Co, Ci, row_scale=None, trans=False):
    """trans: `bank` (K, Ci*Co) stores the TRANSPOSED matrices (the data-gradient pack without a transposed bank copy)."""
    K, B = bank.shape[0], att.shape[0]
    wp = torch.empty((B, (Ci // 4) * ((Co + 15) // 16) * 64), device=bank.device, dtype=torch.float32)
    _lib.call("eat_dyn_pw_pack_t" if trans else "eat_dyn_pw_pack", _dev(bank, "bank"), _dev(att, "att"),
              _opt(row_scale, "row_scale"), wp.data_ptr(), B, K, Co, Ci, _stream())
    return wp


def pw_conv_dyn(x, wp_b, bias, Co, act, res=None):
    B, Ci, F, T = x.shape
    y = torch.empty((B, Co, F, T), device=x.device, dtype=torch.float32)
    _lib.call("eat_pw_conv_dyn_fwd", _dev(x, "x"), _dev(wp_b, "wp_b"), _dev(bias, "bias"), _opt(res, "res"),
              y.data_ptr(), B, Ci, Co, F * T, act, _stream())
    return y


def pw_conv_dyn_wgrad(dz, x):
    """Per-sample weight gradients G (B, Co*Ci) = dz[b] x[b]^T on the per-(tile, sample) kernels (fp32 operands)."""
    B, Co, Ci = dz.shape[0], dz.shape[1], x.shape[1]
    S = x.shape[2] * x.shape[3]
    if dyn_wgrad_needs_zero(Co, Ci, S):
        G = zero_arena.zeros((B, Co * Ci), torch.float32, x.device)
    else:                                       # bf16x3 kernel in per-sample mode: plain stores
        G = torch.empty((B, Co * Ci), device=x.device, dtype=torch.float32)
    _lib.call("eat_pw_conv_dyn_wgrad", _dev(dz, "dz"), _dev(x, "x"), G.data_ptr(), B, Co, Ci, S, _stream())
    return G


def dyn_bf16_eligible(Co, Ci, S):
    """Per-sample-weight dynamic 1x1 conv on split bf16 operands (bf16x3) - the rule `pw_prepack` applies to the static
    convs ('auto': from C_in = 40 on; 'bf16x3': everywhere; never under 'fp32' / plain 'bf16')."""
    m = precision.mode
    return S % 4 == 0 and Ci % 4 == 0 and (m == "bf16x3" or (m == "auto" and Ci >= 40))


def dyn_wgrad_needs_zero(Co, Ci, S):
    """True where `eat_pw_conv_dyn_wgrad` accumulates its per-sample output with atomics (the exact-fp32 tile kernel); the
    bf16x3 kernel covers a sample's whole reduction in one block and stores."""
    return bool(_lib.lib().eat_pw_dyn_wgrad_accumulates(Co, Ci, S))


def dyn_pw_pack_bf16(bank, att, Co, Ci, trans=False):
    """Aggregated per-sample weights sum_k att[b,k] bank[k] as bf16 hi / lo MFMA fragments (the per-sample form of
    `pw_prepack_bf16(split=True)`) -> (B, KK*MT*2*512) bfloat16.  trans: as in `dyn_pw_pack`."""
    K, B = bank.shape[0], att.shape[0]
    n = ((Ci + 31) // 32) * ((Co + 15) // 16) * 2 * 512
    wp = torch.empty((B, n), device=bank.device, dtype=torch.bfloat16)
    _lib.call("eat_dyn_pw_pack_bf16_t" if trans else "eat_dyn_pw_pack_bf16", _dev(bank, "bank"), _dev(att, "att"),
              wp.data_ptr(), B, K, Co, Ci, _stream())
    return wp


def pw_conv_dyn_bf16(x, wp_b, bias, Co, act, res=None):
    """Per-sample-weight 1x1 conv on the bf16x3 kernel (csrc/conv_pw_bf16.hip, tiles inside one sample)."""
    B, Ci, F, T = x.shape
    y = torch.empty((B, Co, F, T), device=x.device, dtype=torch.float32)
    _lib.call("eat_pw_conv_dyn_bf16_fwd", _dev(x, "x"), wp_b.data_ptr(), _dev(bias, "bias"), _opt(res, "res"),
              y.data_ptr(), B, Ci, Co, F * T, act, _stream())
    return y


def kcat_eligible(Co, Ci, S):
    """K-concat form of a dynamic 1x1 conv (no per-sample weights) pays where a sample's aggregated weight matrix is
    larger than its activations: the late, small-plane layers.  (Ci % 32: a k-chunk must not straddle two banks.)"""
    # (the K-concat kernel computes on split bf16x3 operands: under precision('fp32') the per-sample path with the exact
    #  fp32 MFMA is kept, so that `train_precision='fp32'` means what it says for every layer)
    return _KCAT and precision.mode != "fp32" and Ci % 32 == 0 and S % 4 == 0 and Co * Ci > (Ci + Co) * S


def kcat_pack(bank, Co, Ci, row_scale=None):
    """bank (K, Co*Ci) -> packed bf16 hi/lo fragments of [W_0 | ... | W_{K-1}]  (Co x K*Ci).
    (Not cached across training steps: fused optimizers and hipGraph replays update the bank without moving its version
    counter, so a version-keyed cache would serve stale weights; the eval plan caches its packs with the folded weights.)"""
    K = bank.shape[0]
    wcat = bank.view(K, Co, Ci).permute(1, 0, 2).reshape(Co, K * Ci).contiguous()
    return pw_prepack_bf16(wcat, row_scale, split=True)


def pw_conv_kcat(x, wp_cat, bias, att, Co, act, res=None):
    """Dynamic 1x1 conv as one GEMM over the concatenated banks; att (B, K) is the attention of the sample."""
    B, Ci, F, T = x.shape
    K = att.shape[1]
    scale = att.repeat_interleave(Ci, dim=1).contiguous()                  # (B, K*Ci)
    y = torch.empty((B, Co, F, T), device=x.device, dtype=torch.float32)
    _lib.call("eat_pw_conv_kcat_fwd", _dev(x, "x"), wp_cat.data_ptr(), _dev(bias, "bias"), _dev(scale, "att_scale"),
              _opt(res, "res"), y.data_ptr(), B, Ci, K, Co, F * T, act, _stream())
    return y


def dw_conv_dyn(x, w_bc, bias, coef, gate_f, gate_t, k, stride):
    """Depthwise conv with per-(b,c) taps w_bc (B, C*k*k); coef / gates None: the plain conv of the training step, whose
    DyReLU-B * CoordAtt runs after the BatchNorm (`dyrelu_ca_fwd`)."""
    B, C, F, T = x.shape
    Fo, To = conv_out(F, k, stride), conv_out(T, k, stride)
    y = torch.empty((B, C, Fo, To), device=x.device, dtype=torch.float32)
    _lib.call("eat_dw_conv_dyn_fwd", _dev(x, "x"), _dev(w_bc, "w_bc"), _dev(bias, "bias"), _opt(coef, "coef"),
              _opt(gate_f, "gate_f"), _opt(gate_t, "gate_t"), y.data_ptr(), B, C, F, T, Fo, To, k, stride, _stream())
    return y


def dw_conv_dyn_dgrad(dz, w_bc, x_shape, k, stride, res=None):
    """Data gradient of `dw_conv_dyn` (+ res, the skip connection's gradient)."""
    B, C, F, T = x_shape
    dx = torch.empty((B, C, F, T), device=dz.device, dtype=torch.float32)
    _lib.call("eat_dw_conv_dyn_dgrad", _dev(dz, "dz"), _dev(w_bc, "w_bc"), _opt(res, "res"), dx.data_ptr(), B, C, F, T,
              dz.shape[2], dz.shape[3], k, stride, _stream())
    return dx


def dw_conv_dyn_wgrad(dz, x, k, stride, out=None):
    """Per-plane tap gradients G (B, C*k*k) of `dw_conv_dyn`, accumulated with atomics.  out: ZERO-FILLED memory for G."""
    B, C, F, T = x.shape
    G = out if out is not None else torch.zeros((B, C * k * k), device=x.device, dtype=torch.float32)
    _lib.call("eat_dw_conv_dyn_wgrad", _dev(dz, "dz"), _dev(x, "x"), _dev(G, "G"), B, C, F, T, dz.shape[2], dz.shape[3], k,
              stride, _stream())
    return G


def dyrelu_ca_fwd(z, a, b, coef, gate_f, gate_t):
    """out = max(a1 v + b1, a2 v + b2) * sigmoid(gate_f) * sigmoid(gate_t), v = a[c] z + b[c] (a, b None: v = z); coef (B, C, 4),
    position-major pre-sigmoid gates (B*Fo, C) / (B*To, C)."""
    B, C, Fo, To = z.shape
    out = torch.empty_like(z)
    _lib.call("eat_dyrelu_ca_fwd", _dev(z, "z"), _opt(a, "a"), _opt(b, "b"), _dev(coef, "coef"), _dev(gate_f, "gate_f"),
              _dev(gate_t, "gate_t"), out.data_ptr(), B, C, Fo, To, _stream())
    return out


def dyrelu_ca_bwd(dout, z, a, b, coef, gate_f, gate_t):
    """-> (dv, dcoef, dgate_f, dgate_t) of `dyrelu_ca_fwd`, dv being the gradient of v = a[c] z + b[c]."""
    B, C, Fo, To = z.shape
    dv, dcoef = torch.empty_like(z), torch.empty_like(coef)
    dgf, dgt = torch.empty_like(gate_f), torch.empty_like(gate_t)
    _lib.call("eat_dyrelu_ca_bwd", _dev(dout, "dout"), _dev(z, "z"), _opt(a, "a"), _opt(b, "b"), _dev(coef, "coef"),
              _dev(gate_f, "gate_f"), _dev(gate_t, "gate_t"), dv.data_ptr(), dcoef.data_ptr(), dgf.data_ptr(), dgt.data_ptr(), B, C,
              Fo, To, _stream())
    return dv, dcoef, dgf, dgt


def dw_conv_dyn_act(x, w_bc, bias, act, coef, gate_f, gate_t, k, stride):
    """dw_conv_dyn for the block's ablations: plain activation `act` instead of / before DyReLU-B (coef None), no
    coordinate attention (gates None)."""
    B, C, F, T = x.shape
    Fo, To = conv_out(F, k, stride), conv_out(T, k, stride)
    y = torch.empty((B, C, Fo, To), device=x.device, dtype=torch.float32)
    _lib.call("eat_dw_conv_dyn_act_fwd", _dev(x, "x"), _dev(w_bc, "w_bc"), _dev(bias, "bias"), act, _opt(coef, "coef"),
              _opt(gate_f, "gate_f"), _opt(gate_t, "gate_t"), y.data_ptr(), B, C, F, T, Fo, To, k, stride, _stream())
    return y


def pw_conv_stats(x, wp, Co, per_sample=False, tf=None, in_scale=None):
    """Train-mode 1x1 conv z = W x with the batch statistics of z in the conv's epilogue: -> (z, (part, outer, inner)) for
    `bn_state_from_partials`, or (z, None) where the epilogue does not exist (the caller runs `bn_stats`).  wp: any pack of
    `pw_prepack` / `dyn_pw_pack*` (per_sample=True: one pack per sample); tf = (a, b, act): input transform on load."""
    B, Ci, F, T = x.shape
    S = F * T
    wmode = _pack_wmode(wp, per_sample)
    y = torch.empty((B, Co, F, T), device=x.device, dtype=torch.float32)
    part, tiles = _stat_partials(B, S, Co, x.device, per_sample)
    a, b, act = tf if tf is not None else (None, None, 0)
    rc = _lib.call_rc("eat_pw_conv_stats_fwd", _dev(x, "x"), wp.data_ptr(), wmode, 1 if per_sample else 0, _opt(a, "tf_a"),
                      _opt(b, "tf_b"), act, _opt(in_scale, "in_scale"), zeros_vec.get(Co, x.device).data_ptr(), y.data_ptr(),
                      part.data_ptr(), B, Ci, Co, S, _stream())
    if rc == 1:
        return None, None
    return y, (part, tiles, 1)


def pw_conv_gstats(x, wp, Co, z, st, act, sums=None):
    """Project conv's data-gradient GEMM y = W^T x (wp: transposed pack, fp32 or split bf16) with the BatchNorm + activation
    backward statistics of the depthwise output `z` (st = its (a, b, mean, invstd), act its activation) in the epilogue:
    -> (y, sums (2C,) float64) - what `bn_act_bwd_sums(y, z, *st, act)` returns, without the pass over (y, z) - or (None, None)
    where the epilogue does not exist (S % 4 != 0, plain-bf16 / fp32-free packs: the caller runs the separate pass)."""
    B, Ci, F, T = x.shape
    S = F * T
    wmode = _pack_wmode(wp)
    if wmode == 1 or S % 4 != 0 or z.dtype != torch.float32:
        return None, None
    y = torch.empty((B, Co, F, T), device=x.device, dtype=torch.float32)
    part, tiles = _stat_partials(B, S, Co, x.device)
    rc = _lib.call_rc("eat_pw_conv_gstats_fwd", _dev(x, "x"), wp.data_ptr(), wmode, zeros_vec.get(Co, x.device).data_ptr(),
                      y.data_ptr(), _dev(z, "z"), st[0].data_ptr(), st[1].data_ptr(), act, part.data_ptr(), B, Ci, Co, S,
                      _stream())
    if rc == 1:
        return None, None
    return y, _gstat_finish(part, tiles, Co, st, sums)


# ---- round 4: fused training passes of the dynamic block (csrc/dymn.hip, csrc/dw_plane.hip)
def dw_conv_dyn_stats(x, w_bc, k, stride, tf=None, out_b16=False):
    """`dw_conv_stats` with per-(b,c) taps w_bc (B, C*k*k): -> (y, (part, outer, inner)).  A bf16 x - or out_b16 with an fp32 x
    (the block without expand conv) - selects the bf16-storage kernels: y bf16, statistics of the stored values."""
    B, C, F, T = x.shape
    Fo, To = conv_out(F, k, stride), conv_out(T, k, stride)
    cap = dw_partials_inner(F, T, Fo, To, k, stride, False)
    x16 = _is16(x)
    y = torch.empty((B, C, Fo, To), device=x.device, dtype=torch.bfloat16 if (x16 or out_b16) else torch.float32)
    part = torch.empty((B * 2 * C * cap,), device=x.device, dtype=torch.float32)
    inner = _ct.c_int(0)
    a, b, act = tf if tf is not None else (None, None, 0)
    if x16 or out_b16:
        _lib.call("eat_dw_conv_dyn_fwd_stats_b16", _dev16(x, "x") if x16 else _dev(x, "x"), 1 if x16 else 0, _opt(a, "in_a"),
                  _opt(b, "in_b"), act, _dev(w_bc, "w_bc"), y.data_ptr(), part.data_ptr(), cap, _ct.addressof(inner), B, C, F, T,
                  Fo, To, k, stride, _stream())
        return y, (part, B, inner.value)
    _lib.call("eat_dw_conv_dyn_fwd_stats", _dev(x, "x"), _opt(a, "in_a"), _opt(b, "in_b"), act, _dev(w_bc, "w_bc"),
              y.data_ptr(), part.data_ptr(), cap, _ct.addressof(inner), B, C, F, T, Fo, To, k, stride, _stream())
    return y, (part, B, inner.value)


def ctx_pool_cm(x):
    """ContextGen's two average pools, channel-major: x (B, C, F, T) -> seq (1, C, B*(F+T), 1) = [c][b][l]."""
    B, C, F, T = x.shape
    seq = torch.empty((1, C, B * (F + T), 1), device=x.device, dtype=torch.float32)
    _lib.call("eat_ctx_pool_cm", _dev(x, "x"), seq.data_ptr(), B, C, F, T, _stream())
    return seq


def ctx_pool_cm_bwd(dseq, shape, add=None):
    B, C, F, T = shape
    dx = torch.empty(shape, device=dseq.device, dtype=torch.float32)
    _lib.call("eat_ctx_pool_cm_bwd", _dev(dseq, "dseq"), _opt(add, "add"), dx.data_ptr(), B, C, F, T, _stream())
    return dx


def ctx_split(g, B, F, T, stride):
    """g (1, H, B*(F+T), 1) -> (h_cf (1, H, B*Fo, 1), h_ct (1, H, B*To, 1), h_c (B, H))."""
    H = g.shape[1]
    Fo, To = (F - 1) // stride + 1, (T - 1) // stride + 1
    hcf = torch.empty((1, H, B * Fo, 1), device=g.device, dtype=torch.float32)
    hct = torch.empty((1, H, B * To, 1), device=g.device, dtype=torch.float32)
    hc = torch.empty((B, H), device=g.device, dtype=torch.float32)
    _lib.call("eat_ctx_split", _dev(g, "g"), hcf.data_ptr(), hct.data_ptr(), hc.data_ptr(), H, B, F, T, stride, _stream())
    return hcf, hct, hc


def ctx_split_bwd(dhcf, dhct, dhc, H, B, F, T, stride):
    dg = torch.empty((1, H, B * (F + T), 1), device=dhcf.device, dtype=torch.float32)
    _lib.call("eat_ctx_split_bwd", _dev(dhcf, "dhcf"), _dev(dhct, "dhct"), _opt(dhc, "dhc"), dg.data_ptr(), H, B, F, T, stride,
              _stream())
    return dg


def dyrelu_ca_fwd2(z, a, b, coef, gate_f, gate_t):
    """gate_f (C, B, Fo) / gate_t (C, B, To): channel-major pre-sigmoid gates (any shape with that memory layout)."""
    B, C, Fo, To = z.shape
    out = torch.empty_like(z)
    z16 = _is16(z)                                  # bf16 storage: z and out (rounded on store) are bf16
    _lib.call("eat_dyrelu_ca_fwd2_b16" if z16 else "eat_dyrelu_ca_fwd2", _dev16(z, "z") if z16 else _dev(z, "z"), _opt(a, "a"),
              _opt(b, "b"), _dev(coef, "coef"), _dev(gate_f, "gate_f"), _dev(gate_t, "gate_t"), out.data_ptr(), B, C, Fo, To,
              _stream())
    return out


def dyrelu_ca_bwd2(dout, z, a, b, coef, gate_f, gate_t, want_bn=True):
    """-> (dv, dcoef (B,C,4), dgate_f, dgate_t (layouts of the gates), bnpart (B,C,2) or None)."""
    B, C, Fo, To = z.shape
    dv = torch.empty_like(z)
    buf = torch.empty((B * C * (4 + (2 if want_bn else 0)),), device=z.device, dtype=torch.float32)
    dcoef = buf[:B * C * 4].view(B, C, 4)
    bnpart = buf[B * C * 4:].view(B, C, 2) if want_bn else None
    dgf, dgt = torch.empty_like(gate_f), torch.empty_like(gate_t)
    z16 = _is16(z)                                  # bf16 storage: dout, z and dv are bf16 (bnpart: sums of dv as stored)
    if z16 != _is16(dout):
        raise _lib.EatHipError("dyrelu_ca_bwd2: dout and z share one storage type")
    _lib.call("eat_dyrelu_ca_bwd2_b16" if z16 else "eat_dyrelu_ca_bwd2", _dev16(dout, "dout") if z16 else _dev(dout, "dout"),
              _dev16(z, "z") if z16 else _dev(z, "z"), _opt(a, "a"), _opt(b, "b"), _dev(coef, "coef"),
              _dev(gate_f, "gate_f"), _dev(gate_t, "gate_t"), dv.data_ptr(), dcoef.data_ptr(), dgf.data_ptr(), dgt.data_ptr(),
              None if bnpart is None else bnpart.data_ptr(), B, C, Fo, To, _stream())
    return dv, dcoef, dgf, dgt, bnpart


def bn_bwd_combine_partials(p0, p1, stride_e, B, C, inner, mean, invstd):
    """Channel sums of a BatchNorm backward from per-plane partials -> (sums (2C,) float64, dgamma, dbeta)."""
    sums = torch.empty((2 * C,), device=mean.device, dtype=torch.float64)
    vec = torch.empty((2, C), device=mean.device, dtype=torch.float32)
    _lib.call("eat_bn_bwd_combine_partials", p0.data_ptr(), p1.data_ptr(), stride_e, B, C, inner, mean.data_ptr(),
              invstd.data_ptr(), sums.data_ptr(), vec[0].data_ptr(), vec[1].data_ptr(), _stream())
    return sums, vec[0], vec[1]


def dw_conv_dyn_bwd_bn_g(dy, z, st, bn_act, sums, w_bc, x, in_a, in_b, in_act, k, stride, res=None, want_sums=True):
    """Merged backward of a dynamic depthwise conv with its own BatchNorm backward on load (`dw_conv_bwd_bn_g` with
    per-plane taps): -> (g, dw_bc (B, C*k*k), (gpart, gzpart, inner) or None)."""
    B, C, F, T = x.shape
    Fo, To = z.shape[2], z.shape[3]
    cap = int(_lib.lib().eat_dw_bwd_partials_inner(F, T, Fo, To, k, stride))
    g = torch.empty((B, C, F, T), device=z.device, dtype=x.dtype)
    parts = torch.empty((2, B * C * cap), device=z.device, dtype=torch.float32) if want_sums else None
    dw = zero_arena.zeros((B, C * k * k), torch.float32, z.device)
    inner = _ct.c_int(0)
    frozen = 1 if getattr(st[2], "_eat_frozen", False) else 0
    if _is16(z):                                    # bf16 storage: dy, z bf16; x and g bf16, or fp32 (block without expand conv)
        x16 = _is16(x)
        _lib.call("eat_dw_conv_dyn_bwd_bn_g_b16", _dev16(dy, "dy"), _dev16(z, "z"), st[0].data_ptr(), st[1].data_ptr(),
                  st[2].data_ptr(), st[3].data_ptr(), sums.data_ptr(), bn_act, frozen, _dev16(x, "x") if x16 else _dev(x, "x"),
                  1 if x16 else 0, in_a.data_ptr(), in_b.data_ptr(), in_act, _dev(w_bc, "w_bc"), _opt(res, "res"), g.data_ptr(),
                  dw.data_ptr(), None if parts is None else parts[0].data_ptr(), None if parts is None else parts[1].data_ptr(),
                  cap, _ct.addressof(inner), B, C, F, T, Fo, To, k, stride, _stream())
        return g, dw, ((parts[0], parts[1], inner.value) if want_sums else None)
    _lib.call("eat_dw_conv_dyn_bwd_bn_g", _dev(dy, "dy"), _dev(z, "z"), st[0].data_ptr(), st[1].data_ptr(), st[2].data_ptr(),
              st[3].data_ptr(), sums.data_ptr(), bn_act, frozen, _dev(x, "x"), in_a.data_ptr(), in_b.data_ptr(), in_act,
              _dev(w_bc, "w_bc"), _opt(res, "res"), g.data_ptr(), dw.data_ptr(),
              None if parts is None else parts[0].data_ptr(), None if parts is None else parts[1].data_ptr(), cap,
              _ct.addressof(inner), B, C, F, T, Fo, To, k, stride, _stream())
    return g, dw, ((parts[0], parts[1], inner.value) if want_sums else None)


def bn_bwd_apply(g, z, a, b, mean, invstd, sums, inplace=True):
    """dz = a (g - m1 - xhat m2) from the channel sums (g already carries the activation derivative); frozen statistics:
    dz = a g.  In place by default."""
    B, C = z.shape[0], z.shape[1]
    S = z.numel() // (B * C)
    dz = g if inplace else torch.empty_like(g)
    asums = torch.zeros_like(sums) if getattr(mean, "_eat_frozen", False) else sums
    if _is16(g):                                    # bf16 storage: g_e, z_e and dz_e are all wide tensors
        _lib.call("eat_bn_bwd_apply_b16", _dev16(g, "g"), _dev16(z, "z"), a.data_ptr(), b.data_ptr(), mean.data_ptr(),
                  invstd.data_ptr(), asums.data_ptr(), dz.data_ptr(), B, C, S, ACT_NONE, _stream())
        return dz
    _lib.call("eat_bn_act_bwd_apply", _dev(g, "g"), _dev(z, "z"), a.data_ptr(), b.data_ptr(), mean.data_ptr(),
              invstd.data_ptr(), None, None, asums.data_ptr(), dz.data_ptr(), B, C, S, ACT_NONE, _stream())
    return dz


def block_fused_supported(Cin, Cexp, Cout, k, stride, act, proj, F=64, T=500):
    """True where the register-resident block kernel (csrc/irb.hip) has an instantiation: `mbconv` (proj) / `fused_expand_dw`."""
    return bool(_lib.lib().eat_block_fused_supported(Cin, Cexp, Cout, F, T, k, stride, act, 1 if proj else 0))


def fused_expand_dw(x, wp_e, bias_e, w_d, bias_d, Cexp, k, stride, act, pool=None):
    """expand 1x1 + BN + act -> depthwise k x k + BN + act in one kernel (eval; early blocks)."""
    B, Cin, F, T = x.shape
    Fo, To = conv_out(F, k, stride), conv_out(T, k, stride)
    y = torch.empty((B, Cexp, Fo, To), device=x.device, dtype=torch.float32)
    _lib.call("eat_fused_expand_dw_fwd", _dev(x, "x"), _dev(wp_e, "wp_e"), _dev(bias_e, "bias_e"), _dev(w_d, "w_d"),
              _dev(bias_d, "bias_d"), y.data_ptr(), _opt(pool, "pool"), B, Cin, Cexp, F, T, Fo, To, k, stride, act,
              _stream())
    return y


def front(x, w_s, bias_s, w_d, bias_d, wp_p, bias_p, act):
    """Stem conv + BN + Hardswish and the first (expand-less, SE-less) block in one kernel (eval)."""
    B, _, F, T = x.shape
    C = w_s.shape[0]
    Fo, To = conv_out(F, 3, 2), conv_out(T, 3, 2)
    y = torch.empty((B, C, Fo, To), device=x.device, dtype=torch.float32)
    _lib.call("eat_front_fwd", _dev(x, "x"), _dev(w_s, "w_s"), _dev(bias_s, "bias_s"), _dev(w_d, "w_d"),
              _dev(bias_d, "bias_d"), _dev(wp_p, "wp_p"), _dev(bias_p, "bias_p"), y.data_ptr(), B, C, F, T, Fo, To, act,
              _stream())
    return y


def mbconv(x, wp_e, bias_e, w_d, bias_d, wp_p, bias_p, Cexp, Cout, k, stride, act, res=None):
    """Whole inverted-residual block without SE in one kernel (eval; early blocks): expand + depthwise +
    project (+ residual); wp_e / wp_p are fp32 `pw_prepack` buffers."""
    B, Cin, F, T = x.shape
    Fo, To = conv_out(F, k, stride), conv_out(T, k, stride)
    y = torch.empty((B, Cout, Fo, To), device=x.device, dtype=torch.float32)
    _lib.call("eat_mbconv_fwd", _dev(x, "x"), _dev(wp_e, "wp_e"), _dev(bias_e, "bias_e"), _dev(w_d, "w_d"),
              _dev(bias_d, "bias_d"), _dev(wp_p, "wp_p"), _dev(bias_p, "bias_p"), _opt(res, "res"), y.data_ptr(), B, Cin,
              Cexp, Cout, F, T, Fo, To, k, stride, act, _stream())
    return y


def pw_prepack_bf16(w2d, row_scale=None, split=True, trans=False):
    Co, Ci = (w2d.shape[1], w2d.shape[0]) if trans else w2d.shape
    n = ((Ci + 31) // 32) * ((Co + 15) // 16) * (2 if split else 1) * 512
    wp = torch.empty((n,), device=w2d.device, dtype=torch.bfloat16)
    _lib.call("eat_pw_prepack_bf16_t" if trans else "eat_pw_prepack_bf16", _dev(w2d, "w"), _opt(row_scale, "row_scale"),
              wp.data_ptr(), Co, Ci, 1 if split else 0, _stream())
    return wp


_FUSE_EXPAND_DW = True   # expand + depthwise of the 8 x 63-class blocks as one kernel (csrc/expand_dw.hip)


def expand_dw_eligible(Ci, F, T, k, stride):
    """Geometry of eat_expand_dw_bf16_fwd (csrc/expand_dw.hip): small planes, 3x3 / stride 1, C_in <= 128."""
    S = F * T
    return (_FUSE_EXPAND_DW and k == 3 and stride == 1 and 1 <= T <= 64 and 1 <= F <= 8 and S % 4 == 0 and S <= 512
            and Ci % 4 == 0 and 4 <= Ci <= 128)


def expand_dw_bf16(x, wp16_e, bias_e, w_d, bias_d, Ce, k, stride, act, pool=None):
    """expand 1x1 (bf16x3) + BN + act -> depthwise 3x3 + BN + act (+ SE squeeze sums) in one kernel; the expanded tensor
    never reaches HBM (eval; late blocks with small planes)."""
    B, Ci, F, T = x.shape
    y = torch.empty((B, Ce, F, T), device=x.device, dtype=torch.float32)
    _lib.call("eat_expand_dw_bf16_fwd", _dev(x, "x"), wp16_e.data_ptr(), _dev(bias_e, "bias_e"), _dev(w_d, "w_d"),
              _dev(bias_d, "bias_d"), y.data_ptr(), _opt(pool, "pool"), B, Ci, Ce, F, T, k, stride, act, _stream())
    return y


def pw_stream_mode(mode=-1):
    """Variant of the bf16 1x1 kernels (eat_pw_stream_mode): bit 0 expand-shaped layers on the x-resident kernel,
    bit 1 project-shaped layers on the K-streaming kernel; returns the previous mode, a negative argument only queries."""
    return _lib.lib().eat_pw_stream_mode(int(mode))


def pw_conv_bf16(x, wp16, bias, Co, act, split=True, in_scale=None, res=None, pool=None, write=True):
    """1x1 conv on the bf16 matrix cores (split=True: bf16x3, fp32-class accuracy; False: plain bf16)."""
    B, Ci, F, T = x.shape
    y = torch.empty((B, Co, F, T), device=x.device, dtype=torch.float32) if write else None
    _lib.call("eat_pw_conv_bf16_fwd", _dev(x, "x"), wp16.data_ptr(), _dev(bias, "bias"), _opt(in_scale, "in_scale"),
              _opt(res, "res"), None if y is None else y.data_ptr(), _opt(pool, "pool"), B, Ci, Co, F * T, act,
              1 if split else 0, _stream())
    return y


# ------------------------------------------------------------------ bf16 activation storage (BASELINE configs[2])
def b16_block_ok(B, C_exp, F, T, k, stride):
    """True where the bf16-storage kernels cover an inverted-residual block whose depthwise conv maps (F, T) planes of
    C_exp channels (csrc/dw_plane.hip geometries, even plane sizes, 16-byte row pieces for the 1x1 kernels)."""
    Fo, To = conv_out(F, k, stride), conv_out(T, k, stride)
    return (bool(_lib.lib().eat_dw_conv_b16_ok(B, C_exp, F, T, Fo, To, k, stride)) and (F * T) % 8 == 0
            and (Fo * To) % 8 == 0 and C_exp % 8 == 0)


def pw_conv_b16(x, wp, bias, Co, act, tf=None, in_scale=None, res=None, x2=None, stats=False, out_b16=False, gstat=None):
    """1x1 conv of the bf16-storage plan: exactly one of input / output is the wide bf16 tensor (`eat_pw_conv_b16_fwd`).
    x fp32 -> y bf16 (expand conv, project data gradient); x bf16 -> y fp32 (project conv with tf = (a, b, act) / in_scale /
    stats=True -> (y, parts); two-source data-gradient GEMM with x2 fp32 + res).  wp: plain bf16 pack (precision 'bf16')."""
    if wp.dtype != torch.bfloat16 or getattr(wp, "_eat_split", False):
        raise _lib.EatHipError("pw_conv_b16: needs a plain bf16 weight pack (precision('bf16'))")
    B, C1, F, T = x.shape
    S = F * T
    x16 = _is16(x)
    Ci = C1 + (x2.shape[1] if x2 is not None else 0)
    y16 = out_b16 or not x16                       # (fp32 in: always a bf16 output; bf16 in: fp32, or bf16 for z_p)
    y = torch.empty((B, Co, F, T), device=x.device, dtype=torch.bfloat16 if y16 else torch.float32)
    part, tiles = _stat_partials(B, S, Co, x.device) if stats or gstat is not None else (None, 0)
    a, b, tact = tf if tf is not None else (None, None, 0)
    # gstat = (z_d bf16, (a, b, mean, invstd), act, sums or None): bf16 -> bf16 project data gradient with the depthwise
    # BatchNorm's backward sums in the epilogue -> (y, sums (2 Co,) float64), see pw_conv_gstats
    gz, gst, gact, gsums = gstat if gstat is not None else (None, (None, None, None, None), 0, None)
    _lib.call("eat_pw_conv_b16_fwd", _dev16(x, "x") if x16 else _dev(x, "x"), 1 if x16 else 0, _opt(x2, "x2"), C1,
              wp.data_ptr(), _dev(bias, "bias"), _opt(a, "tf_a"), _opt(b, "tf_b"), tact, _opt(in_scale, "in_scale"),
              _opt(res, "res"), y.data_ptr(), 1 if y16 else 0, None if part is None else part.data_ptr(),
              None if gz is None else _dev16(gz, "gz"), _opt(gst[0], "g_a"), _opt(gst[1], "g_b"), gact, B, Ci, Co, S, act,
              _stream())
    if gstat is not None:
        return y, _gstat_finish(part, tiles, Co, gst, gsums)
    return (y, (part, tiles, 1)) if stats else y


def cast_b16(x):
    """bf16 copy of a contiguous fp32 tensor (numel % 8 == 0; `eat_cast_b16`)."""
    y = torch.empty(x.shape, device=x.device, dtype=torch.bfloat16)
    _lib.call("eat_cast_b16", _dev(x, "x"), y.data_ptr(), x.numel(), _stream())
    return y


def pw_conv_wgrad_b16(dz, x, x_scale=None, tf=None, out=None):
    """dW (Co, Ci) = sum_b dz[b] . (act(tf_a x + tf_b) * x_scale)[b]^T with exactly one bf16 (wide) operand; plain bf16
    products, fp32 accumulation (`eat_pw_conv_wgrad_b16`)."""
    B, Co = dz.shape[0], dz.shape[1]
    Ci = x.shape[1]
    S = dz.numel() // (B * Co)
    d16, x16 = _is16(dz), _is16(x)
    n = int(_lib.lib().eat_pw_wgrad_b16_slots(B, Co, Ci, S, 1 if x16 else 0))
    dW = out if out is not None else zero_arena.zeros((Co, Ci), torch.float32, dz.device)
    ws = torch.empty((n, Co, Ci), device=dz.device, dtype=torch.float32)
    a, b, tact = tf if tf is not None else (None, None, 0)
    _lib.call("eat_pw_conv_wgrad_b16", _dev16(dz, "dz") if d16 else _dev(dz, "dz"), 1 if d16 else 0,
              _dev16(x, "x") if x16 else _dev(x, "x"), 1 if x16 else 0, _opt(a, "tf_a"), _opt(b, "tf_b"), tact,
              _opt(x_scale, "x_scale"), dW.data_ptr(), ws.data_ptr(), n, B, Co, Ci, S, _stream())
    return dW


# ---- bf16 activation storage of the DyMN blocks (dymn_train.py; include/eat_hip.h "bf16 activation storage for the DyMN blocks")
def dyn_b16_block_ok(B, cin, cexp, cout, F, T, k, stride):
    """True where the bf16-storage kernels cover a fully dynamic DY_Block: depthwise geometry (`b16_block_ok`), 16-byte row
    pieces and whole 4-channel groups for the per-sample 1x1 kernels."""
    return b16_block_ok(B, cexp, F, T, k, stride) and cin % 4 == 0 and cout % 4 == 0 and cexp % 8 == 0


def dyn_pw_pack_b16(bank, att, Co, Ci, trans=False):
    """Aggregated per-sample weights sum_k att[b,k] bank[k] as PLAIN bf16 MFMA fragments (`eat_dyn_pw_pack_b16`) ->
    (B, KK*MT*512) bfloat16.  trans: `bank` (K, Ci*Co) holds the transposed matrices (the data-gradient pack)."""
    K, B = bank.shape[0], att.shape[0]
    n = ((Ci + 31) // 32) * ((Co + 15) // 16) * 512
    wp = torch.empty((B, n), device=bank.device, dtype=torch.bfloat16)
    _lib.call("eat_dyn_pw_pack_b16", _dev(bank, "bank"), _dev(att, "att"), wp.data_ptr(), B, K, Co, Ci, 1 if trans else 0,
              _stream())
    return wp


def pw_conv_dyn_b16(x, wp_b, Co, act, res=None, stats=False):
    """Per-sample-weight 1x1 conv of the bf16-storage plan (`eat_pw_conv_dyn_b16_fwd`): x fp32 -> y bf16, or x bf16 -> y fp32
    (+ res).  stats: -> (y, (part, tiles, 1)) with the batch statistics of y as stored."""
    B, Ci, F, T = x.shape
    S = F * T
    x16 = _is16(x)
    y = torch.empty((B, Co, F, T), device=x.device, dtype=torch.float32 if x16 else torch.bfloat16)
    part, tiles = _stat_partials(B, S, Co, x.device, per_sample=True) if stats else (None, 0)
    _lib.call("eat_pw_conv_dyn_b16_fwd", _dev16(x, "x") if x16 else _dev(x, "x"), 1 if x16 else 0, wp_b.data_ptr(),
              zeros_vec.get(Co, x.device).data_ptr(), _opt(res, "res"), y.data_ptr(), 0 if x16 else 1,
              None if part is None else part.data_ptr(), B, Ci, Co, S, act, _stream())
    return (y, (part, tiles, 1)) if stats else y


def pw_conv_dyn_wgrad_b16(dz, x):
    """Per-sample weight gradients G (B, Co*Ci) = dz[b] x[b]^T on the wide-tile kernel (`eat_pw_conv_dyn_wgrad_b16`): one bf16
    (wide) operand - plain bf16 products - or both fp32 - split-operand bf16x3 products; every element is stored.  None where
    the kernel does not take an all-fp32 shape."""
    B, Co = dz.shape[0], dz.shape[1]
    Ci = x.shape[1]
    S = dz.numel() // (B * Co)
    d16, x16 = _is16(dz), _is16(x)
    ns = int(_lib.lib().eat_pw_dyn_wgrad_b16_slices(B, Co, Ci, S, 1 if x16 else (0 if d16 else 2)))
    if ns < 1:
        return None                                 # (both fp32 and a shape the wide-tile kernel does not take: the caller's fallback)
    buf = torch.empty((ns, B, Co * Ci), device=dz.device, dtype=torch.float32)     # copy 0 = the result, the rest k-slice workspace
    _lib.call("eat_pw_conv_dyn_wgrad_b16", _dev16(dz, "dz") if d16 else _dev(dz, "dz"), 1 if d16 else 0,
              _dev16(x, "x") if x16 else _dev(x, "x"), 1 if x16 else 0, buf.data_ptr(), ns, B, Co, Ci, S, _stream())
    return buf[0]


# ------------------------------------------------------------------ precision switch (training plans)
class precision:
    """Context manager selecting the arithmetic of the 1x1 convs issued through pw_prepack/pw_conv:
    'fp32' (exact fp32 MFMA), 'auto' (fp32 below C_in = 40, split-operand bf16x3 - fp32-class accuracy at a
    multiple of the fp32 MFMA rate - from there on; see mn._pw_mode), 'bf16x3' (split everywhere) or 'bf16'
    (plain bf16 operands on v_mfma_f32_16x16x32_bf16, fp32 accumulation and fp32 activations in memory -
    BASELINE config 3)."""
    mode = "fp32"

    def __init__(self, mode):
        if mode not in ("fp32", "auto", "bf16x3", "bf16"):
            raise ValueError(f"unknown precision {mode!r}")
        self.new = mode

    def __enter__(self):
        self.old, precision.mode = precision.mode, self.new

    def __exit__(self, *exc):
        precision.mode = self.old


def _pack_kind(Ci):
    """Pack of a static 1x1 conv with Ci input channels under the active `precision`: 0 fp32 fragments, 1 plain bf16,
    2 split bf16 hi / lo ('bf16x3' everywhere, 'auto' from C_in = 40 on)."""
    m = precision.mode
    if m == "bf16":
        return 1
    return 2 if m == "bf16x3" or (m == "auto" and Ci >= 40 and Ci % 4 == 0) else 0


def pw_prepack(w2d, row_scale=None, trans=False):
    kind = _pack_kind(w2d.shape[0] if trans else w2d.shape[1])
    if kind == 1:
        return pw_prepack_bf16(w2d, row_scale, split=False, trans=trans)
    if kind == 2:
        wp = pw_prepack_bf16(w2d, row_scale, split=True, trans=trans)
        wp._eat_split = True                 # both bf16 packs share the dtype: mark the hi/lo one
        return wp
    return _pw_prepack_fp32(w2d, row_scale, trans=trans)


def pw_conv(x, wp, bias, Co, act, in_scale=None, res=None, pool=None, write=True):
    if wp.dtype == torch.bfloat16:
        return pw_conv_bf16(x, wp, bias, Co, act, getattr(wp, "_eat_split", False), in_scale=in_scale, res=res,
                            pool=pool, write=write)
    return _pw_conv_fp32(x, wp, bias, Co, act, in_scale=in_scale, res=res, pool=pool, write=write)


class PrepackPlan:
    """The weight packs of a model's 1x1 convs for one pass, produced by ONE launch (`eat_pw_prepack_multi`) instead of one
    per matrix.  entries: [(key, w2d, trans)] with w2d a contiguous (rows, cols) view of a parameter; the arithmetic
    (fp32 / bf16 / bf16x3 pack) follows `precision.mode` at construction exactly as `pw_prepack` decides it.  The packs live
    in a buffer owned by the plan and are refreshed by `run()`; `get(key)` hands out views (valid until the next run)."""

    def __init__(self, entries):
        import numpy as np
        self.mode = precision.mode
        dev = entries[0][1].device
        recs, views, off, max_threads = [], {}, 0, 1
        for key, w2d, trans in entries:      # w2d: the parameter itself (Co, Ci[, 1, 1]), contiguous
            if not w2d.is_contiguous():
                raise _lib.EatHipError("PrepackPlan: weights must be contiguous")
            rows, cols = w2d.shape[0], w2d.numel() // w2d.shape[0]
            Co, Ci = (cols, rows) if trans else (rows, cols)
            kind = _pack_kind(Ci)
            mt = (Co + 15) // 16
            if kind == 0:
                if Ci % 4:
                    raise _lib.EatHipError(f"PrepackPlan: Ci={Ci} must be a multiple of 4")
                nbytes, threads = (Ci // 4) * mt * 64 * 4, (Ci // 4) * mt * 64
            else:
                nbytes, threads = ((Ci + 31) // 32) * mt * kind * 512 * 2, ((Ci + 31) // 32) * mt * 64
            max_threads = max(max_threads, threads)
            recs.append((w2d, off, Co, Ci, kind, 1 if trans else 0, nbytes, key))
            off += (nbytes + 255) // 256 * 256
        self.buf = torch.empty((off,), device=dev, dtype=torch.uint8)
        table = np.zeros((len(recs),), dtype=[("w", "<u8"), ("wp", "<u8"), ("Co", "<i4"), ("Ci", "<i4"), ("kind", "<i4"), ("trans", "<i4")])
        self.ptrs = []
        for i, (w2d, o, Co, Ci, kind, trans, nbytes, key) in enumerate(recs):
            table[i] = (w2d.data_ptr(), self.buf.data_ptr() + o, Co, Ci, kind, trans)
            self.ptrs.append(w2d.data_ptr())
            v = self.buf[o:o + nbytes].view(torch.float32 if kind == 0 else torch.bfloat16)
            if kind == 2:
                v._eat_split = True
            views[key] = v
        self.keep = [r[0] for r in recs]
        self.views, self.n, self.max_threads = views, len(recs), max_threads
        self.table = torch.from_numpy(table.view(np.uint8).copy()).to(dev)

    @classmethod
    def of_weights(cls, weights):
        """The plan with the forward and the data-gradient pack of every distinct matrix of `weights` (`view(w, trans)` finds
        them); None for an empty list."""
        entries, seen = [], set()
        for w in weights:
            if w.data_ptr() not in seen:
                seen.add(w.data_ptr())
                entries += [((w.data_ptr(), False), w, False), ((w.data_ptr(), True), w, True)]
        return cls(entries) if entries else None

    def view(self, w, trans):
        """The pack of parameter `w` in a plan built by `of_weights`, or None if it holds none."""
        return self.views.get((w.data_ptr(), trans))

    def stale(self):
        """Parameters were re-allocated (model.to(), a new state dict with fresh storage) or the arithmetic changed."""
        return self.mode != precision.mode or any(t.data_ptr() != p for t, p in zip(self.keep, self.ptrs))

    runs = 0          # number of `run()` calls: a backward that finds it changed knows its views were re-packed since

    def run(self):
        self.runs += 1
        _lib.call("eat_pw_prepack_multi", self.table.data_ptr(), self.n, self.max_threads, _stream())

    def get(self, key):
        return self.views[key]


# ------------------------------------------------------------------ training-loop glue (ex_audioset.py:142-194)
def col_sum(m):
    """Column sums of a contiguous (R, C) matrix (bias gradients of the DyMN context path)."""
    R, C = m.shape
    out = torch.empty((C,), device=m.device, dtype=torch.float32)
    _lib.call("eat_col_sum", _dev(m, "m"), out.data_ptr(), R, C, _stream())
    return out


def _glue_operand(t, name, dtype, like, n=None, at_least=None):
    """Metadata check (no sync, no value read) of an operand whose pointer goes straight to a glue kernel: dtype, contiguity,
    element count and the device of the main operand `like`.  Runs before the residency check of `like`, so a refusal does
    not need a GPU."""
    want = f"a contiguous {str(dtype).replace('torch.', '')} tensor" + (f" of {n} elements" if n is not None else "") + \
        (f" of at least {at_least} elements" if at_least is not None else "")
    if not isinstance(t, torch.Tensor):
        raise _lib.EatHipError(f"{name} must be {want} (got {type(t).__name__})")
    if t.dtype != dtype or not t.is_contiguous() or (n is not None and t.numel() != n) or \
            (at_least is not None and t.numel() < at_least):
        raise _lib.EatHipError(f"{name} must be {want} (got {t.dtype}, {tuple(t.shape)}, contiguous={t.is_contiguous()})")
    if t.device != like.device:
        raise _lib.EatHipError(f"{name} must live on the device of its batch, {like.device} (got {t.device})")
    return t.data_ptr()


def _mix_operands(fn, perm, lam, B, like):
    """-> (perm pointer, lam pointer) of a mix-up draw, (None, None) without one: perm (B) int32, lam (B) fp32."""
    if (perm is None) != (lam is None):
        raise _lib.EatHipError(f"{fn}: perm and lam go together")
    if perm is None:
        return None, None
    return (_glue_operand(perm, f"{fn}: perm", torch.int32, like, n=B),
            _glue_operand(lam, f"{fn}: lam", torch.float32, like, n=B))


def mixup_fwd(x, perm, lam):
    """x[b] * lam[b] + x[perm[b]] * (1 - lam[b]) over the flattened per-sample axis; perm int32 (B), lam fp32 (B).  The
    VALUES of perm (in [0, B)) are the caller's responsibility: the kernel gathers rows by them."""
    if x.dim() < 1 or x.shape[0] < 1 or x.numel() < 1 or x.numel() % x.shape[0]:
        raise _lib.EatHipError(f"mixup_fwd: x must be a non-empty (B, ...) batch, got {tuple(x.shape)}")
    B = x.shape[0]
    if perm is None or lam is None:
        raise _lib.EatHipError("mixup_fwd: perm and lam are both required")
    p_perm, p_lam = _mix_operands("mixup_fwd", perm, lam, B, x)
    p_x = _dev(x, "x")
    out = torch.empty_like(x)
    _lib.call("eat_mixup_fwd", p_x, p_perm, p_lam, out.data_ptr(), B, x.numel() // B, _stream())
    return out


def wave_i16_to_f32(src, out=None, scale=1.0 / 32768.0):
    """int16 PCM (any shape, contiguous, on the GPU) -> fp32 waveform `src * scale` (f2: 16-bit transport over PCIe)."""
    if not src.is_cuda or src.dtype != torch.int16 or not src.is_contiguous():
        raise _lib.EatHipError(f"wave_i16_to_f32: src must be a contiguous int16 GPU tensor (got {src.dtype} on {src.device})")
    if out is None:
        out = torch.empty(src.shape, device=src.device, dtype=torch.float32)
    elif out.numel() != src.numel():
        raise _lib.EatHipError("wave_i16_to_f32: out has a different number of samples")
    _lib.call("eat_wave_i16_to_f32", src.data_ptr(), _dev(out, "out"), src.numel(), float(scale), _stream())
    return out


def kd_loss_fwd_bwd(logits, y, perm, lam, teacher, teacher_idx, kd_lambda, sums):
    """-> dlogits; accumulates (loss, label part, distillation part) into `sums` (>= 3 fp32) on the device.  perm (B) int32 and
    lam (B) fp32 come together or not at all; teacher (N, C) fp32 probabilities with teacher_idx (B) int64 (-1 = no entry).
    Operand types and shapes are checked here from metadata; the index VALUES (perm in [0, B), teacher_idx in [-1, N)) are
    the caller's responsibility - `KDTrainer` validates its table once on the host."""
    fn = "kd_loss_fwd_bwd"
    if logits.dim() != 2 or logits.numel() < 1:
        raise _lib.EatHipError(f"{fn}: logits must be a non-empty (B, C) matrix, got {tuple(logits.shape)}")
    B, C = logits.shape
    if tuple(y.shape) != (B, C):
        raise _lib.EatHipError(f"{fn}: y {tuple(y.shape)} does not match the logits {(B, C)}")
    kd_lambda = float(kd_lambda)
    if not 0.0 <= kd_lambda <= 1.0:
        raise _lib.EatHipError(f"{fn}: kd_lambda must lie in [0, 1] (got {kd_lambda})")
    p_perm, p_lam = _mix_operands(fn, perm, lam, B, logits)
    p_teacher = p_tidx = None
    n_teacher = 0
    if teacher is not None:
        if teacher.dim() != 2 or teacher.shape[0] < 1 or teacher.shape[1] != C:
            raise _lib.EatHipError(f"{fn}: teacher must be (N >= 1, {C}) probabilities, got {tuple(teacher.shape)}")
        _glue_operand(teacher, f"{fn}: teacher", torch.float32, logits)
        if teacher_idx is None and kd_lambda < 1.0:
            raise _lib.EatHipError(f"{fn}: teacher_idx is required with a teacher and kd_lambda < 1")
    if teacher_idx is not None:
        _glue_operand(teacher_idx, f"{fn}: teacher_idx", torch.int64, logits, n=B)
    if teacher is not None and teacher_idx is not None:       # (kd_lambda = 1 without an index: the pure label loss)
        p_teacher, p_tidx, n_teacher = teacher.data_ptr(), teacher_idx.data_ptr(), teacher.shape[0]
    p_sums = _glue_operand(sums, f"{fn}: sums", torch.float32, logits, at_least=3)
    p_logits, p_y = _dev(logits, "logits"), _dev(y, "y")
    dlogits = torch.empty_like(logits)
    _lib.call("eat_kd_loss_fwd_bwd", p_logits, p_y, p_perm, p_lam, p_teacher, p_tidx, n_teacher, kd_lambda, B, C, p_sums,
              dlogits.data_ptr(), _stream())
    return dlogits


# ------------------------------------------------------------------ single-label fine-tuning (ex_esc50.py:95-178)
def _dev_int32(t, name, n):
    if t is None:
        return None
    if not t.is_cuda or t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != n:
        raise _lib.EatHipError(f"{name} must be a contiguous int32 GPU tensor of {n} elements (got {t.dtype}, {tuple(t.shape)}, "
                               f"on {t.device})")
    return t.data_ptr()


def _row_loss_operands(fn, logits, perm, lam, sums, row_loss):
    """What `softmax_ce_fwd_bwd` and `masked_bce_fwd_bwd` check alike -> (B, C, perm, lam, sums, row_loss pointers)."""
    if logits.dim() != 2:
        raise _lib.EatHipError(f"{fn}: logits must be (B, C), got {tuple(logits.shape)}")
    B, C = logits.shape
    p_perm, p_lam = _mix_operands(fn, perm, lam, B, logits)
    p_sums = None if sums is None else _glue_operand(sums, f"{fn}: sums", torch.float32, logits, at_least=1)
    p_row = None if row_loss is None else _glue_operand(row_loss, f"{fn}: row_loss", torch.float32, logits, n=B)
    return B, C, p_perm, p_lam, p_sums, p_row


def softmax_ce_fwd_bwd(logits, y, perm=None, lam=None, sums=None, grad=True, row_loss=None, row_argmax=None):
    """Soft-target cross-entropy of (B, C) logits against y (B, C), with the mix-up t = lam y + (1 - lam) y[perm] folded in
    (include/eat_hip.h: eat_softmax_ce_fwd_bwd).  -> dlogits (B, C) (None with grad=False); `sums` (>= 1 fp32) += the batch
    mean; `row_loss` (B) fp32 and `row_argmax` (B) int32 are filled when given."""
    B, C, p_perm, p_lam, p_sums, p_row = _row_loss_operands("softmax_ce_fwd_bwd", logits, perm, lam, sums, row_loss)
    if tuple(y.shape) != (B, C):
        raise _lib.EatHipError(f"softmax_ce_fwd_bwd: y {tuple(y.shape)} does not match the logits {(B, C)}")
    dlogits = torch.empty_like(logits) if grad else None
    _lib.call("eat_softmax_ce_fwd_bwd", _dev(logits, "logits"), _dev(y, "y"), p_perm, p_lam, B, C, p_sums,
              _opt(dlogits, "dlogits"), p_row, _dev_int32(row_argmax, "row_argmax", B), _stream())
    return dlogits


def check_augment_draws(idx, shift, n_bank, L):
    """Host-side validation of the draw tables of `wave_augment` (CPU tensors of 2B values): primary rows in [0, n_bank),
    partners in [-1, n_bank), shifts in (-L, L)."""
    idx, shift = torch.as_tensor(idx), torch.as_tensor(shift)
    if idx.numel() % 2 or idx.numel() != shift.numel() or idx.numel() == 0:
        raise ValueError(f"wave_augment: idx / shift must hold 2B values each (got {idx.numel()}, {shift.numel()})")
    prim, part = idx[0::2], idx[1::2]
    if bool(((prim < 0) | (prim >= n_bank)).any()) or bool(((part < -1) | (part >= n_bank)).any()):
        raise ValueError(f"wave_augment: a bank index lies outside [0, {n_bank}) (partners may be -1)")
    if bool((shift.abs() >= L).any()):
        raise ValueError(f"wave_augment: a shift lies outside (-{L}, {L})")


def wave_augment(bank, bank_mean, bank_cls, idx, shift, amp, mix, n_classes, out=None, y=None):
    """Gain + roll + wave-mix of a batch gathered from the resident bank (include/eat_hip.h: eat_wave_augment) -> (out (B, L),
    y (B, n_classes)).  idx / shift (2B) int32, amp (2B) / mix (B) fp32: CPU tensors are validated here and uploaded; device
    tensors (the static buffers of a captured step) must have been validated before they were staged.  bank_cls = None:
    the waveforms only, -> (out, None) (the labels of a multi-label bank come from `openmic_targets`)."""
    n_bank, L = bank.shape
    B = torch.as_tensor(mix).numel()
    dev = bank.device
    if not idx.is_cuda:
        check_augment_draws(idx, shift, n_bank, L)
        idx, shift = (t.to(dev, torch.int32, non_blocking=True) for t in (idx, shift))
        amp, mix = (t.to(dev, torch.float32, non_blocking=True) for t in (amp, mix))
    if bank_mean.dtype != torch.float64 or not bank_mean.is_cuda or bank_mean.numel() != n_bank:
        raise _lib.EatHipError("wave_augment: bank_mean must be a float64 GPU tensor of one value per bank row")
    if out is None:
        out = torch.empty((B, L), device=dev, dtype=torch.float32)
    if bank_cls is None:
        if y is not None:
            raise _lib.EatHipError("wave_augment: y needs bank_cls")
        n_classes = 0
    elif y is None:
        y = torch.empty((B, n_classes), device=dev, dtype=torch.float32)
    if out.numel() != B * L or (y is not None and y.numel() != B * n_classes) or amp.numel() != 2 * B:
        raise _lib.EatHipError("wave_augment: out / y / amp do not match the batch")
    _lib.call("eat_wave_augment", _dev(bank, "bank"), bank_mean.data_ptr(), _dev_int32(bank_cls, "bank_cls", n_bank), n_bank, L,
              n_classes, _dev_int32(idx, "idx", 2 * B), _dev_int32(shift, "shift", 2 * B), _dev(amp, "amp"), _dev(mix, "mix"),
              _dev(out, "out"), _opt(y, "y"), B, _stream())
    return out, y


# ------------------------------------------------------------------ OpenMIC fine-tuning (ex_openmic.py:96-206)
def masked_bce_fwd_bwd(logits, yy, perm=None, lam=None, sums=None, grad=True, row_loss=None, probs=None, binarize=True):
    """Masked BCE-with-logits of (B, C) logits against packed rows yy (B, 2C) = [labels | mask], the mix-up of the (binarized)
    labels folded in (include/eat_hip.h: eat_masked_bce_fwd_bwd).  -> dlogits (B, C) (None with grad=False); `sums` (>= 1 fp32)
    += the batch mean; `row_loss` (B) fp32 is filled when given; `probs` (B, C) fp32 receives sigmoid(logits) - it may be a
    row slice of a wider matrix (unit column stride)."""
    B, C, p_perm, p_lam, p_sums, p_row = _row_loss_operands("masked_bce_fwd_bwd", logits, perm, lam, sums, row_loss)
    if tuple(yy.shape) != (B, 2 * C):
        raise _lib.EatHipError(f"masked_bce_fwd_bwd: yy {tuple(yy.shape)} does not match the logits: expected {(B, 2 * C)}")
    stride = 0
    if probs is not None:
        if (not probs.is_cuda or probs.dtype != torch.float32 or tuple(probs.shape) != (B, C) or probs.stride(1) != 1
                or (B > 1 and probs.stride(0) < C)):
            raise _lib.EatHipError(f"masked_bce_fwd_bwd: probs must be a float32 GPU view of shape {(B, C)} with unit column "
                                   f"stride (got {probs.dtype}, {tuple(probs.shape)}, strides {probs.stride()})")
        stride = probs.stride(0) if B > 1 else C
    dlogits = torch.empty_like(logits) if grad else None
    _lib.call("eat_masked_bce_fwd_bwd", _dev(logits, "logits"), _dev(yy, "yy"), p_perm, p_lam, B, C, int(bool(binarize)), p_sums,
              _opt(dlogits, "dlogits"), p_row, None if probs is None else probs.data_ptr(), stride, _stream())
    return dlogits


def openmic_targets(bank_y, idx, mix, out=None):
    """Label rows (B, 2C) of a wave-mixed batch from the resident labels bank_y (N, 2C) (include/eat_hip.h:
    eat_openmic_targets).  idx (2B) int32 / mix (B) fp32: the DEVICE tables handed to `wave_augment`, validated
    (`check_augment_draws`) before they were uploaded."""
    n_bank, W = bank_y.shape
    B = mix.numel()
    if W % 2 or W == 0:
        raise _lib.EatHipError(f"openmic_targets: bank_y must be (N, 2C), got {tuple(bank_y.shape)}")
    if out is None:
        out = torch.empty((B, W), device=bank_y.device, dtype=torch.float32)
    if out.numel() != B * W:
        raise _lib.EatHipError("openmic_targets: out does not match the batch")
    _lib.call("eat_openmic_targets", _dev(bank_y, "bank_y"), n_bank, W // 2, _dev_int32(idx, "idx", 2 * B), _dev(mix, "mix"),
              _dev(out, "out"), B, _stream())
    return out


# ------------------------------------------------------------------ FSD50K fine-tuning (ex_fsd50k.py:96-178)
def check_ragged_draws(idx, start, shift, lengths_cpu, L):
    """Host-side validation of the draw tables of `wave_augment_ragged` (CPU tensors of 2B values; lengths_cpu (N) the clip
    lengths): primary rows in [0, N), partners in [-1, N), shifts in (-L, L); start == 0 for a clip that fits (length <= L),
    0 <= start <= length - L for a longer one (the window is never padded: datasets/fsd50k.py:55-59)."""
    idx, start, shift = torch.as_tensor(idx), torch.as_tensor(start), torch.as_tensor(shift)
    lengths = torch.as_tensor(lengths_cpu).to(torch.int64)
    n_bank = lengths.numel()
    if idx.numel() % 2 or idx.numel() == 0 or idx.numel() != shift.numel() or idx.numel() != start.numel():
        raise ValueError(f"wave_augment_ragged: idx / start / shift must hold 2B values each (got {idx.numel()}, "
                         f"{start.numel()}, {shift.numel()})")
    prim, part = idx[0::2], idx[1::2]
    if bool(((prim < 0) | (prim >= n_bank)).any()) or bool(((part < -1) | (part >= n_bank)).any()):
        raise ValueError(f"wave_augment_ragged: a bank index lies outside [0, {n_bank}) (partners may be -1)")
    if bool((shift.abs() >= L).any()):
        raise ValueError(f"wave_augment_ragged: a shift lies outside (-{L}, {L})")
    used = idx >= 0
    room = (lengths[idx[used].long()] - L).clamp(min=0)                       # 0 for a clip that fits
    st = start[used].to(torch.int64)
    if bool(((st < 0) | (st > room)).any()):
        raise ValueError(f"wave_augment_ragged: a crop start lies outside [0, max(0, length - {L})]")


def _stage_draws(dev, check, ints, floats):
    """Draw tables -> on `dev`, int32 / fp32: CPU tables are validated with `check()` and uploaded, device tables pass as staged."""
    if ints[0].is_cuda:
        return (*ints, *floats)
    check()
    return (*(t.to(dev, torch.int32, non_blocking=True) for t in ints),
            *(t.to(dev, torch.float32, non_blocking=True) for t in floats))


def wave_augment_ragged(bank, idx, start, shift, amp, mix, L, out=None, yy=None, win_mean=None, labels=True):
    """Crop / pad + gain + roll + wave-mix of a batch gathered from a ragged resident bank, and its mixed label rows
    (include/eat_hip.h: eat_wave_augment_ragged) -> (out (B, L), yy (B, 2C) = [labels | ones]).  bank: the dict of
    `fsd50k.load_bank` (waves, offsets, lengths, clip_sum, bank_y on the device, lengths_cpu).  idx / start / shift (2B)
    int32, amp (2B) / mix (B) fp32: CPU tensors are validated here and uploaded; device tensors (the static buffers of a
    captured step) must have been validated before they were staged.  win_mean (2B) fp64: the kernel's workspace, allocated
    here unless given (a captured step passes a static one).  labels=False: the waveforms only, -> (out, None)."""
    waves, offsets, lengths, clip_sum, bank_y = (bank[k] for k in ("waves", "offsets", "lengths", "clip_sum", "bank_y"))
    n_bank, L = lengths.numel(), int(L)
    B = torch.as_tensor(mix).numel()
    dev = waves.device
    idx, start, shift, amp, mix = _stage_draws(dev, lambda: check_ragged_draws(idx, start, shift, bank["lengths_cpu"], L),
                                               (idx, start, shift), (amp, mix))
    if waves.dim() != 1 or offsets.dtype != torch.int64 or not offsets.is_cuda or offsets.numel() != n_bank:
        raise _lib.EatHipError("wave_augment_ragged: waves must be flat and offsets an int64 GPU tensor of one value per clip")
    if clip_sum.dtype != torch.float64 or not clip_sum.is_cuda or clip_sum.numel() != n_bank:
        raise _lib.EatHipError("wave_augment_ragged: clip_sum must be a float64 GPU tensor of one value per clip")
    if bank_y.dim() != 2 or bank_y.shape[0] != n_bank:
        raise _lib.EatHipError(f"wave_augment_ragged: bank_y must be (N, C) with N = {n_bank}, got {tuple(bank_y.shape)}")
    C = bank_y.shape[1]
    if out is None:
        out = torch.empty((B, L), device=dev, dtype=torch.float32)
    if not labels:
        if yy is not None:
            raise _lib.EatHipError("wave_augment_ragged: yy was given with labels=False")
    elif yy is None:
        yy = torch.empty((B, 2 * C), device=dev, dtype=torch.float32)
    if win_mean is None:
        win_mean = torch.empty(2 * B, device=dev, dtype=torch.float64)
    if (out.numel() != B * L or (yy is not None and yy.numel() != 2 * B * C) or amp.numel() != 2 * B
            or win_mean.dtype != torch.float64 or not win_mean.is_cuda or win_mean.numel() != 2 * B
            or not win_mean.is_contiguous()):
        raise _lib.EatHipError("wave_augment_ragged: out / yy / amp / win_mean do not match the batch")
    _lib.call("eat_wave_augment_ragged", _dev(waves, "waves"), waves.numel(), offsets.data_ptr(),
              _dev_int32(lengths, "lengths", n_bank), clip_sum.data_ptr(), _dev(bank_y, "bank_y"), n_bank, L, C,
              _dev_int32(idx, "idx", 2 * B), _dev_int32(start, "start", 2 * B), _dev_int32(shift, "shift", 2 * B),
              _dev(amp, "amp"), _dev(mix, "mix"), win_mean.data_ptr(), _dev(out, "out"), _opt(yy, "yy"), B, _stream())
    return out, yy


# ------------------------------------------------------------------ DCASE20 fine-tuning (ex_dcase20.py:99-123)
def check_mixstyle_perm(perm, B):
    """Host-side validation of the permutation of `freq_mixstyle` (a CPU tensor): B values in [0, B)."""
    perm = torch.as_tensor(perm)
    if perm.numel() != B:
        raise ValueError(f"freq_mixstyle: perm must hold B = {B} values (got {perm.numel()})")
    if bool(((perm < 0) | (perm >= B)).any()):
        raise ValueError(f"freq_mixstyle: a perm value lies outside [0, {B})")


def freq_mixstyle(x, perm, lam, apply=None, out=None, stats=None, eps=1e-6):
    """Frequency-wise MixStyle of a log-mel batch x (B, C, F, T) (include/eat_hip.h: eat_freq_mixstyle) -> out.  perm (B)
    integer, lam (B) fp32 (any shape of B values): CPU tensors are validated here and uploaded; device tensors (the static
    buffers of a captured step) must be int32 / fp32 and validated before they were staged.  apply: None, or a device int32
    scalar read by the kernel (0: out = x bit for bit, stats untouched).  stats (B, F, 2) fp32: the kernel's workspace ({mu,
    sig} per row), allocated here unless given."""
    if x.dim() != 4:
        raise _lib.EatHipError(f"freq_mixstyle: x must be (B, C, F, T), got {tuple(x.shape)}")
    B, C, F, T = x.shape
    dev = x.device
    if not perm.is_cuda:
        check_mixstyle_perm(perm, B)
        perm = perm.reshape(-1).to(dev, torch.int32, non_blocking=True)
    if lam.numel() != B:
        raise _lib.EatHipError(f"freq_mixstyle: lam must hold B = {B} values (got {lam.numel()})")
    if not lam.is_cuda:
        lam = lam.to(dev, torch.float32, non_blocking=True)
    lam = lam.reshape(-1)
    if apply is not None and (not torch.is_tensor(apply) or apply.numel() != 1):
        raise _lib.EatHipError("freq_mixstyle: apply must be None or a device int32 scalar")
    if out is None:
        out = torch.empty_like(x)
    if stats is None:
        stats = torch.empty((B, F, 2), device=dev, dtype=torch.float32)
    if out.numel() != x.numel() or stats.numel() != 2 * B * F:
        raise _lib.EatHipError("freq_mixstyle: out / stats do not match x")
    if out.data_ptr() == x.data_ptr():
        raise _lib.EatHipError("freq_mixstyle: out must not be x")
    _lib.call("eat_freq_mixstyle", _dev(x, "x"), _dev_int32(perm, "perm", B), _dev(lam, "lam"), _dev_int32(apply, "apply", 1),
              _dev(out, "out"), _dev(stats, "stats"), B, C, F, T, float(eps), _stream())
    return out


# ------------------------------------------------------------------ long-recording tagger (include/eat_tag.h)
def check_windows(win_start, win_valid, L, n_wave):
    """Host-side validation of a window table of `mel_windows` (CPU arrays): 0 <= valid <= L, start >= 0 and
    start + valid <= n_wave -> (start int64, valid int32) CPU tensors."""
    start = torch.as_tensor(win_start, dtype=torch.int64).reshape(-1)
    valid = torch.as_tensor(win_valid, dtype=torch.int64).reshape(-1)
    if start.numel() < 1 or start.numel() != valid.numel():
        raise _lib.EatHipError(f"mel_windows: need one (start, valid) pair per window (got {start.numel()} starts, {valid.numel()} valids)")
    if bool(((valid < 0) | (valid > L)).any()):
        raise _lib.EatHipError(f"mel_windows: a window's valid length lies outside [0, {L}]")
    if bool((start < 0).any()) or bool((start + valid > n_wave).any()):
        raise _lib.EatHipError(f"mel_windows: a window reads outside the waveform buffer of {n_wave} samples")
    return start.contiguous(), valid.to(torch.int32).contiguous()


def mel_windows(wave, win_start, win_valid, L, window, twiddle, band_w2, band_start, band_cnt, n_fft, hop, n_mels, out=None):
    """Log-mel of N windows of the flat waveform buffer `wave` (n_wave) -> out (N, n_mels, T): window w is wave[start[w] :
    start[w] + L] with positions >= valid[w] read as 0.0; the bits of `mel_fwd` on the materialised windows.  CPU
    descriptor arrays are validated here (`check_windows`) and uploaded; device tensors (slices of a table that was
    validated before it was uploaded) must be int64 / int32.  At most 65535 windows per call."""
    if wave.dim() != 1:
        raise _lib.EatHipError(f"mel_windows: wave must be a flat (n_wave) buffer, got {tuple(wave.shape)}")
    dev = wave.device
    if not (torch.is_tensor(win_start) and win_start.is_cuda and torch.is_tensor(win_valid) and win_valid.is_cuda):
        win_start, win_valid = (t.to(dev) for t in check_windows(win_start, win_valid, L, wave.numel()))
    N = win_start.numel()
    if (win_start.dtype != torch.int64 or not win_start.is_contiguous() or win_start.device != dev
            or win_valid.numel() != N):
        raise _lib.EatHipError("mel_windows: win_start must be a contiguous int64 tensor of N values on the wave's device")
    if band_w2.shape[1:] != (n_mels, 2) or band_start.numel() != n_mels or band_cnt.numel() != n_mels:
        raise _lib.EatHipError("mel_windows: band table must be (pairs, n_mels, 2) with n_mels starts / counts")
    T = 1 + (L - 1) // hop
    if out is None:
        out = torch.empty((N, n_mels, T), device=dev, dtype=torch.float32)
    elif out.numel() != N * n_mels * T or out.dtype != torch.float32 or not out.is_contiguous():
        raise _lib.EatHipError(f"mel_windows: out must be a contiguous fp32 buffer of {N} x {n_mels} x {T} elements")
    _lib.call("eat_mel_windows_fwd", _dev(wave, "wave"), wave.numel(), win_start.data_ptr(), _dev_int32(win_valid, "win_valid", N),
              N, L, _dev(window, "window"), window.numel(), n_fft, hop, _dev(twiddle, "twiddle"), _dev(band_w2, "band_w2"),
              band_start.data_ptr(), band_cnt.data_ptr(), n_mels, band_w2.shape[0], out.data_ptr(), T, _stream())
    return out


def tag_topk(logits, k, return_probs=False):
    """sigmoid + per-row top-k of (N, C) logits -> (prob (N, k) fp32, index (N, k) int32[, probs (N, C)]): descending
    probability, equal probabilities by ascending class index.  1 <= k <= min(C, 64)."""
    if logits.dim() != 2:
        raise _lib.EatHipError(f"tag_topk: logits must be (N, C), got {tuple(logits.shape)}")
    N, C = logits.shape
    prob = torch.empty((N, k), device=logits.device, dtype=torch.float32)
    index = torch.empty((N, k), device=logits.device, dtype=torch.int32)
    probs = torch.empty((N, C), device=logits.device, dtype=torch.float32) if return_probs else None
    _lib.call("eat_tag_topk", _dev(logits, "x"), N, C, k, prob.data_ptr(), index.data_ptr(), _opt(probs, "probs"), _stream())
    return (prob, index, probs) if return_probs else (prob, index)


def resampled_length(n_in, up, down):
    """ceil(n_in up / down): the output length of `resample_mono` (and of scipy.signal.resample_poly)."""
    return -(-int(n_in) * int(up) // int(down))


def resample_mono(frames, up, down, taps):
    """Interleaved (n_in, channels) or (n_in,) frames, int16 (scaled by 1 / 32768) or float32, on the GPU -> the mono
    waveform resampled by up / down with the FIR `taps` (tagger.resample_plan), (ceil(n_in up / down)) fp32."""
    if frames.dim() not in (1, 2) or frames.dtype not in (torch.int16, torch.float32) or not frames.is_cuda \
            or not frames.is_contiguous():
        raise _lib.EatHipError(f"resample_mono: frames must be a contiguous int16 / float32 GPU tensor (n_in,) or (n_in, channels) "
                               f"(got {frames.dtype}, {tuple(frames.shape)}, on {frames.device})")
    if frames.device.index != torch.cuda.current_device():
        raise _lib.EatHipError(f"resample_mono: frames live on {frames.device} but the current device is cuda:{torch.cuda.current_device()}")
    n_in = frames.shape[0]
    channels = frames.shape[1] if frames.dim() == 2 else 1
    n_out = resampled_length(n_in, up, down)
    out = torch.empty(max(n_out, 0), device=frames.device, dtype=torch.float32)
    _lib.call("eat_resample_mono", frames.data_ptr(), 1 if frames.dtype == torch.int16 else 0, n_in, channels, int(up), int(down),
              _dev(taps, "taps"), taps.numel(), out.data_ptr(), n_out, _stream())
    return out


# ------------------------------------------------------------------ embedding extractor (include/eat_embed.h)
_EMBED_GRID = 2 ** 31 - 1      # blocks of one eat_embed_pool launch: ceil(D / 4) * B
_EMBED_TABLES = {}             # (device, map shapes, lo, hi) -> (dims, seg) on the device
_EMBED_ADDRS = {}              # (device, map addresses, map shapes) -> address table per chunk over B, on the device


def check_segments(lo, hi, T_l):
    """Host-side validation of the segment tables of `embed_pool` (CPU arrays): lo, hi (n_maps, n_seg) with
    0 <= lo < hi <= T_l[map] everywhere -> (lo, hi) contiguous int32 CPU tensors."""
    try:
        lo_t, hi_t = (torch.as_tensor(v) for v in (lo, hi))
    except (ValueError, TypeError) as e:
        raise _lib.EatHipError(f"embed_pool: ragged segment table ({e})") from None
    T = torch.as_tensor(T_l, dtype=torch.int64).reshape(-1)
    if lo_t.dim() != 2 or lo_t.shape != hi_t.shape or lo_t.shape[0] != T.numel() or lo_t.shape[1] < 1:
        raise _lib.EatHipError(f"embed_pool: ragged segment table: need lo and hi of one (n_maps, n_seg >= 1) shape with a row "
                               f"per map (got lo {tuple(lo_t.shape)}, hi {tuple(hi_t.shape)}, {T.numel()} maps)")
    if lo_t.dtype.is_floating_point or hi_t.dtype.is_floating_point:
        raise _lib.EatHipError("embed_pool: segment bounds must be integers")
    lo_t, hi_t = lo_t.to(torch.int64), hi_t.to(torch.int64)
    bad = (lo_t < 0) | (lo_t >= hi_t) | (hi_t > T.view(-1, 1))
    if bool(bad.any()):
        l, s = (int(v) for v in bad.nonzero()[0])
        raise _lib.EatHipError(f"embed_pool: segment {s} of map {l} is [{int(lo_t[l, s])}, {int(hi_t[l, s])}): need "
                               f"0 <= lo < hi <= T_l = {int(T[l])}")
    return lo_t.to(torch.int32).contiguous(), hi_t.to(torch.int32).contiguous()


def embed_pool(fmaps, lo, hi, out=None):
    """Segment means of a list of feature maps (B, C_l, F_l, T_l), concatenated along the channel axis ->
    out (B, n_seg, D = sum C_l): out[b, s, off_l + c] = mean of fmaps[l][b, c, :, lo[l, s]:hi[l, s]].  lo, hi: CPU
    (n_maps, n_seg) tables, validated by `check_segments`; the scene embedding is lo = 0, hi = T_l with n_seg = 1.
    One launch for all maps and segments (chunks over B only beyond the grid limit).  The device copies of the shape and
    segment tables are cached per (map shapes, plan): a recording's chunks repeat them."""
    fmaps = list(fmaps)
    if not 1 <= len(fmaps) <= 64:
        raise _lib.EatHipError(f"embed_pool: need 1 to 64 feature maps (got {len(fmaps)})")
    if any(m.dim() != 4 or m.shape[0] != fmaps[0].shape[0] or m.device != fmaps[0].device for m in fmaps):
        raise _lib.EatHipError("embed_pool: every feature map must be (B, C, F, T) with one B, on one device")
    if any(m.numel() == 0 for m in fmaps):
        raise _lib.EatHipError("embed_pool: an empty feature map")
    ptrs = [_dev(m, "x") for m in fmaps]
    dev, B = fmaps[0].device, fmaps[0].shape[0]
    shapes = tuple(tuple(m.shape[1:]) for m in fmaps)
    lo_t, hi_t = check_segments(lo, hi, [s[2] for s in shapes])
    n_seg, D = lo_t.shape[1], sum(s[0] for s in shapes)
    key = (dev, shapes, lo_t.numpy().tobytes(), hi_t.numpy().tobytes())
    tables = _EMBED_TABLES.get(key)
    if tables is None:
        if len(_EMBED_TABLES) >= 64:
            _EMBED_TABLES.clear()
        offs, off = [], 0
        for s in shapes:
            offs.append(off)
            off += s[0]
        dims = torch.tensor([[c, f, t, o] for (c, f, t), o in zip(shapes, offs)], dtype=torch.int32)
        tables = _EMBED_TABLES[key] = (dims.to(dev), torch.stack((lo_t, hi_t), dim=2).contiguous().to(dev))
    dims, seg = tables
    if out is None:
        out = torch.empty((B, n_seg, D), device=dev, dtype=torch.float32)
    elif out.shape != (B, n_seg, D) or out.device != dev:
        raise _lib.EatHipError(f"embed_pool: out must be ({B}, {n_seg}, {D}) on {dev} (got {tuple(out.shape)} on {out.device})")
    o = _dev(out, "out")
    step = max(1, _EMBED_GRID // ((D + 3) // 4))
    # the caching allocator hands a recording's chunks the same addresses again and again: no upload in the steady state
    akey = (dev, tuple(ptrs), shapes, B)
    addrs = _EMBED_ADDRS.get(akey)
    if addrs is None:
        if len(_EMBED_ADDRS) >= 64:
            _EMBED_ADDRS.clear()
        addrs = _EMBED_ADDRS[akey] = [
            torch.tensor([p + 4 * b0 * c * f * t for p, (c, f, t) in zip(ptrs, shapes)], dtype=torch.int64).to(dev)
            for b0 in range(0, B, step)]
    for b0, addr in zip(range(0, B, step), addrs):
        nb = min(step, B - b0)
        _lib.call("eat_embed_pool", addr.data_ptr(), dims.data_ptr(), seg.data_ptr(), len(fmaps), nb, n_seg, D,
                  o + 4 * b0 * n_seg * D, _stream())
    return out


# ------------------------------------------------------------------ query-by-example search (include/eat_search.h)
SEARCH_MAX_K, SEARCH_MAX_Q = 128, 1024
# geometry of csrc/search.hip (kBlocks, kMaxGroup, kWaves x rows_per_wave), for callers that size a bank to it
SEARCH_BLOCKS, SEARCH_GROUP = 256, 16


def search_tile_rows(group):
    """Bank rows that one block of the scan takes per step when `group` queries (a power of two up to 16) are resident."""
    return 8 * 8                   # kWaves x rows_per_wave(group): the same for every group today


_SEARCH_WS = {}              # (device, Q, k) -> workspace of eat_embed_search_ws_bytes(Q, k) bytes


def rows_normalize(x, out=None):
    """x (N, D) -> x / sqrt(sum_d x^2) per row, fp32; a row whose sum of squares is 0 becomes zeros.  out: None, x itself (in
    place) or another (N, D) tensor that does not overlap x."""
    if x.dim() != 2 or x.shape[1] < 1:
        raise _lib.EatHipError(f"rows_normalize: x must be (N, D >= 1), got {tuple(x.shape)}")
    px = _dev(x, "x")
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.device != x.device:
        raise _lib.EatHipError(f"rows_normalize: out must be {tuple(x.shape)} on {x.device} (got {tuple(out.shape)} on {out.device})")
    _lib.call("eat_rows_normalize", px, x.shape[0], x.shape[1], _dev(out, "out"), _stream())
    return out


def check_skip(skip, Q):
    """Host-side validation of the exclusion table of `embed_search` (a CPU array): (Q, 2) integers lo, hi that fit int32
    -> contiguous int32 CPU tensor.  The kernel clamps both bounds into [0, N]; lo >= hi excludes nothing."""
    try:
        t = torch.as_tensor(skip)
    except (ValueError, TypeError) as e:
        raise _lib.EatHipError(f"embed_search: ragged skip table ({e})") from None
    if t.dim() != 2 or tuple(t.shape) != (Q, 2):
        raise _lib.EatHipError(f"embed_search: skip must be ({Q}, 2): lo, hi per query (got {tuple(t.shape)})")
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise _lib.EatHipError("embed_search: skip bounds must be integers")
    t = t.to(torch.int64).cpu()
    if bool(((t < -2 ** 31) | (t > 2 ** 31 - 1)).any()):
        raise _lib.EatHipError("embed_search: skip bounds must fit int32")
    return t.to(torch.int32).contiguous()


def embed_search(bank, queries, k, skip=None):
    """The k rows of `bank` (N, D) of largest dot product with each row of `queries` (Q, D), both L2-normalised already
    (`rows_normalize`) -> (score (Q, k) fp32, index (Q, k) int32): descending score, equal scores by ascending row; where
    fewer than k rows are eligible the remaining slots hold (-inf, -1).  skip: None or a CPU (Q, 2) table lo, hi - rows
    [lo, hi) are not eligible for that query (`check_skip`).  1 <= k <= 128, 1 <= Q <= 1024; no (Q, N) matrix exists at
    any time, the bank is read once per group of up to 16 queries."""
    if bank.dim() != 2 or queries.dim() != 2 or bank.shape[1] != queries.shape[1] or bank.shape[1] < 1:
        raise _lib.EatHipError(f"embed_search: bank (N, D) and queries (Q, D) must share D >= 1 (got {tuple(bank.shape)}, "
                               f"{tuple(queries.shape)})")
    pb, pq = _dev(bank, "x"), _dev(queries, "queries")
    if queries.device != bank.device:
        raise _lib.EatHipError(f"embed_search: bank lives on {bank.device}, queries on {queries.device}")
    (N, D), Q, k, dev = bank.shape, queries.shape[0], int(k), bank.device
    if not 1 <= k <= SEARCH_MAX_K or not 1 <= Q <= SEARCH_MAX_Q or N < 1:
        raise _lib.EatHipError(f"embed_search: need 1 <= k <= {SEARCH_MAX_K}, 1 <= Q <= {SEARCH_MAX_Q} and N >= 1 "
                               f"(got k={k}, Q={Q}, N={N})")
    skip_d = None if skip is None else check_skip(skip, Q).to(dev)
    ws = _SEARCH_WS.get((dev, Q, k))
    if ws is None:
        if len(_SEARCH_WS) >= 64:
            _SEARCH_WS.clear()
        ws = _SEARCH_WS[(dev, Q, k)] = torch.empty(_lib.lib().eat_embed_search_ws_bytes(Q, k), device=dev, dtype=torch.uint8)
    score = torch.empty((Q, k), device=dev, dtype=torch.float32)
    index = torch.empty((Q, k), device=dev, dtype=torch.int32)
    _lib.call("eat_embed_search", pb, N, D, pq, Q, k, None if skip_d is None else skip_d.data_ptr(), ws.data_ptr(), ws.numel(),
              score.data_ptr(), index.data_ptr(), _stream())
    return score, index


# ------------------------------------------------------------------ occurrence search (include/eat_match.h)
MATCH_MAX_L, MATCH_MAX_SEP = 1024, 4096
_MATCH_WS = {}               # (device, N, min(L, 16), k) -> workspace of eat_embed_match_ws_bytes(N, L, k) bytes


def embed_match(bank, seg, queries, k, sep, min_score=float("-inf"), skip=None):
    """Where in the files of `bank` (N, D) does the sequence `queries` (L, D) occur - both L2-normalised already
    (`rows_normalize`), the queries in time order at the bank's hop -> (score (k,) fp32, index (k,) int32).
    seg (F + 1,) int32 on the bank's device: file f is rows [seg[f], seg[f + 1]), strictly ascending from 0 to N (the
    caller's promise: the table is not read back).  The match score of a start row whose window fits its file is the mean
    over j of the `embed_search` score of query row j and bank row n + j; a start row is returned when no other start row
    of its file within `sep` rows is better (larger score, equal scores by lower row) and its score is at least
    `min_score`: local-maximum peak picking, not greedy suppression.  Descending score, equal scores by ascending row,
    (-inf, -1) in the slots that no peak fills.  skip: None or (lo, hi) - start rows [lo, hi) are neither returned nor
    suppress others.  1 <= L <= 1024, 1 <= k <= 128, 0 <= sep <= 4096."""
    if bank.dim() != 2 or queries.dim() != 2 or bank.shape[1] != queries.shape[1] or bank.shape[1] < 1:
        raise _lib.EatHipError(f"embed_match: bank (N, D) and queries (L, D) must share D >= 1 (got {tuple(bank.shape)}, "
                               f"{tuple(queries.shape)})")
    pb, pq = _dev(bank, "x"), _dev(queries, "queries")
    if queries.device != bank.device or seg.device != bank.device:
        raise _lib.EatHipError(f"embed_match: bank lives on {bank.device}, queries on {queries.device}, seg on {seg.device}")
    if seg.dim() != 1 or seg.dtype != torch.int32 or seg.shape[0] < 2 or not seg.is_contiguous():
        raise _lib.EatHipError(f"embed_match: seg must be a contiguous int32 vector of F + 1 >= 2 bounds (got {tuple(seg.shape)} "
                               f"{seg.dtype})")
    (N, D), L, k, sep, dev = bank.shape, queries.shape[0], int(k), int(sep), bank.device
    min_score = float(min_score)
    if not 1 <= k <= SEARCH_MAX_K or not 1 <= L <= MATCH_MAX_L or not 0 <= sep <= MATCH_MAX_SEP or N < 1:
        raise _lib.EatHipError(f"embed_match: need 1 <= k <= {SEARCH_MAX_K}, 1 <= L <= {MATCH_MAX_L}, 0 <= sep <= {MATCH_MAX_SEP} "
                               f"and N >= 1 (got k={k}, L={L}, sep={sep}, N={N})")
    if min_score != min_score:
        raise _lib.EatHipError("embed_match: min_score is NaN (-inf disables it)")
    lo, hi = (0, 0) if skip is None else (int(v) for v in check_skip([list(skip)], 1)[0])
    key = (dev, N, min(L, SEARCH_GROUP), k)
    ws = _MATCH_WS.get(key)
    if ws is None:
        _MATCH_WS.clear()                 # one bank at a time: a workspace holds (1 + min(L, 16)) x N floats
        ws = _MATCH_WS[key] = torch.empty(_lib.lib().eat_embed_match_ws_bytes(N, L, k), device=dev, dtype=torch.uint8)
    score = torch.empty((k,), device=dev, dtype=torch.float32)
    index = torch.empty((k,), device=dev, dtype=torch.int32)
    _lib.call("eat_embed_match", pb, N, D, seg.data_ptr(), seg.shape[0] - 1, pq, L, k, sep, min_score, lo, hi, ws.data_ptr(),
              ws.numel(), score.data_ptr(), index.data_ptr(), _stream())
    return score, index


# ------------------------------------------------------------------ the 8-bit search index (include/eat_search_q8.h)
SEARCH_Q8_MAX_D = 131072
# geometry of csrc/search_q8.hip (kBlocks, kMaxGroup, kTileRows = 16 rows per wavefront x 8 wavefronts)
SEARCH_Q8_BLOCKS, SEARCH_Q8_GROUP, SEARCH_Q8_TILE_ROWS = 256, 64, 128

_SEARCH_Q8_WS = {}           # (device, Q, k) -> workspace of eat_embed_search_q8_ws_bytes(Q, k) bytes


def q8_ld(D):
    """Row stride in bytes of q8 codes of D values: D rounded up to a multiple of 16."""
    return (int(D) + 15) // 16 * 16


def _dev_q8(fn, codes, scale, D, what):
    """Checks one q8 matrix - codes (N, ld) int8 with ld >= D a multiple of 16, scale (N,) fp32 -> (codes pointer, ld)."""
    if codes.dim() != 2 or not codes.is_cuda or codes.dtype != torch.int8 or not codes.is_contiguous():
        raise _lib.EatHipError(f"{fn}: {what} codes must be a contiguous (N, ld) int8 GPU tensor (got {codes.dtype}, "
                               f"{tuple(codes.shape)}, on {codes.device})")
    ld = codes.shape[1]
    if ld < D or ld % 16 != 0 or codes.data_ptr() % 16 != 0:
        raise _lib.EatHipError(f"{fn}: {what} codes need a 16-byte aligned base and a row stride that is a multiple of 16, "
                               f"at least D = {D} (got {ld})")
    if scale.shape != (codes.shape[0],) or scale.device != codes.device:
        raise _lib.EatHipError(f"{fn}: {what} scale must be ({codes.shape[0]},) on {codes.device} (got {tuple(scale.shape)} "
                               f"on {scale.device})")
    _dev(scale, f"{what} scale")
    return codes.data_ptr(), ld


def rows_quantize_q8(x, normalize=True, codes=None, scale=None):
    """x (N, D) fp32 -> (codes (N, ld) int8, scale (N,) fp32), ld = `q8_ld(D)`: row n stands for scale[n] * codes[n, :D].
    normalize: divide each row by its L2 norm first, with the bits of `rows_normalize`.  scale = max |row| / 127,
    code = rint(value / scale) in [-127, 127]; a zero row has scale 0 and zero codes; bytes [D, ld) are stored as zeros.
    codes, scale: None or where to store (rows of a resident bank)."""
    if x.dim() != 2 or not 1 <= x.shape[1] <= SEARCH_Q8_MAX_D:
        raise _lib.EatHipError(f"rows_quantize_q8: x must be (N, 1 <= D <= {SEARCH_Q8_MAX_D}), got {tuple(x.shape)}")
    px = _dev(x, "x")
    N, D = x.shape
    if codes is None:
        codes = torch.empty((N, q8_ld(D)), device=x.device, dtype=torch.int8)
    if scale is None:
        scale = torch.empty((N,), device=x.device, dtype=torch.float32)
    if codes.shape[0] != N or codes.device != x.device:
        raise _lib.EatHipError(f"rows_quantize_q8: codes must have {N} rows on {x.device} (got {tuple(codes.shape)} on {codes.device})")
    pc, ld = _dev_q8("rows_quantize_q8", codes, scale, D, "output")
    _lib.call("eat_rows_quantize_q8", px, N, D, 1 if normalize else 0, pc, ld, scale.data_ptr(), _stream())
    return codes, scale


def embed_search_q8(codes, scale, D, qcodes, qscale, k, skip=None):
    """`embed_search` over a q8 bank: codes (N, ld) int8 and scale (N,), queries qcodes (Q, qld) and qscale (Q,), both of D
    values (`rows_quantize_q8`) -> (score (Q, k) fp32, index (Q, k) int32).  score = float(integer dot product of the codes)
    * (qscale * scale): exact integer arithmetic on the matrix cores, so equal rows tie exactly.  The bank is read once per
    group of up to 64 queries."""
    D, k = int(D), int(k)
    if not 1 <= D <= SEARCH_Q8_MAX_D:
        raise _lib.EatHipError(f"embed_search_q8: need 1 <= D <= {SEARCH_Q8_MAX_D} (got {D})")
    pb, ld = _dev_q8("embed_search_q8", codes, scale, D, "bank")
    pq, qld = _dev_q8("embed_search_q8", qcodes, qscale, D, "query")
    if qcodes.device != codes.device:
        raise _lib.EatHipError(f"embed_search_q8: bank lives on {codes.device}, queries on {qcodes.device}")
    if codes.device.index != torch.cuda.current_device():
        raise _lib.EatHipError(f"embed_search_q8: the bank lives on {codes.device} but the current device is "
                               f"cuda:{torch.cuda.current_device()}")
    N, Q, dev = codes.shape[0], qcodes.shape[0], codes.device
    if not 1 <= k <= SEARCH_MAX_K or not 1 <= Q <= SEARCH_MAX_Q or N < 1:
        raise _lib.EatHipError(f"embed_search_q8: need 1 <= k <= {SEARCH_MAX_K}, 1 <= Q <= {SEARCH_MAX_Q} and N >= 1 "
                               f"(got k={k}, Q={Q}, N={N})")
    skip_d = None if skip is None else check_skip(skip, Q).to(dev)
    ws = _SEARCH_Q8_WS.get((dev, Q, k))
    if ws is None:
        if len(_SEARCH_Q8_WS) >= 64:
            _SEARCH_Q8_WS.clear()
        ws = _SEARCH_Q8_WS[(dev, Q, k)] = torch.empty(_lib.lib().eat_embed_search_q8_ws_bytes(Q, k), device=dev, dtype=torch.uint8)
    score = torch.empty((Q, k), device=dev, dtype=torch.float32)
    index = torch.empty((Q, k), device=dev, dtype=torch.int32)
    _lib.call("eat_embed_search_q8", pb, ld, scale.data_ptr(), N, D, pq, qld, qscale.data_ptr(), Q, k,
              None if skip_d is None else skip_d.data_ptr(), ws.data_ptr(), ws.numel(), score.data_ptr(), index.data_ptr(), _stream())
    return score, index


# ------------------------------------------------------------------ occurrence search over the 8-bit index (include/eat_match_q8.h)
MATCH_Q8_GROUP = 64          # kMaxGroup of csrc/match_q8.hip: query rows resident per pass over the bank
_MATCH_Q8_WS = {}            # (device, N, min(L, 64), k) -> workspace of eat_embed_match_q8_ws_bytes(N, L, k) bytes


def embed_match_q8(codes, scale, D, seg, qcodes, qscale, k, sep, min_score=float("-inf"), skip=None):
    """`embed_match` over a q8 bank: codes (N, ld) int8 and scale (N,), the clip's rows qcodes (L, qld) and qscale (L,) in
    time order, both of D values (`rows_quantize_q8`) -> (score (k,) fp32, index (k,) int32).  The score of a start row is
    the mean over j of the `embed_search_q8` score of query row j and bank row n + j - a mean of q8 scores, on the scale
    of `embed_search_q8` - and everything else (seg, the window inside one file, local-maximum peak picking within `sep`
    rows, `min_score`, skip = None or (lo, hi), the order, the (-inf, -1) padding) is `embed_match`.  The bank is read once
    per group of up to 64 query rows.  1 <= L <= 1024, 1 <= k <= 128, 0 <= sep <= 4096."""
    D, k, sep = int(D), int(k), int(sep)
    if not 1 <= D <= SEARCH_Q8_MAX_D:
        raise _lib.EatHipError(f"embed_match_q8: need 1 <= D <= {SEARCH_Q8_MAX_D} (got {D})")
    pb, ld = _dev_q8("embed_match_q8", codes, scale, D, "bank")
    pq, qld = _dev_q8("embed_match_q8", qcodes, qscale, D, "query")
    if qcodes.device != codes.device or seg.device != codes.device:
        raise _lib.EatHipError(f"embed_match_q8: bank lives on {codes.device}, queries on {qcodes.device}, seg on {seg.device}")
    if codes.device.index != torch.cuda.current_device():
        raise _lib.EatHipError(f"embed_match_q8: the bank lives on {codes.device} but the current device is "
                               f"cuda:{torch.cuda.current_device()}")
    if seg.dim() != 1 or seg.dtype != torch.int32 or seg.shape[0] < 2 or not seg.is_contiguous():
        raise _lib.EatHipError(f"embed_match_q8: seg must be a contiguous int32 vector of F + 1 >= 2 bounds (got {tuple(seg.shape)} "
                               f"{seg.dtype})")
    N, L, dev = codes.shape[0], qcodes.shape[0], codes.device
    min_score = float(min_score)
    if not 1 <= k <= SEARCH_MAX_K or not 1 <= L <= MATCH_MAX_L or not 0 <= sep <= MATCH_MAX_SEP or N < 1:
        raise _lib.EatHipError(f"embed_match_q8: need 1 <= k <= {SEARCH_MAX_K}, 1 <= L <= {MATCH_MAX_L}, 0 <= sep <= {MATCH_MAX_SEP} "
                               f"and N >= 1 (got k={k}, L={L}, sep={sep}, N={N})")
    if min_score != min_score:
        raise _lib.EatHipError("embed_match_q8: min_score is NaN (-inf disables it)")
    lo, hi = (0, 0) if skip is None else (int(v) for v in check_skip([list(skip)], 1)[0])
    key = (dev, N, min(L, MATCH_Q8_GROUP), k)
    ws = _MATCH_Q8_WS.get(key)
    if ws is None:
        _MATCH_Q8_WS.clear()              # one bank at a time: a workspace holds (1 + min(L, 64)) x N floats
        ws = _MATCH_Q8_WS[key] = torch.empty(_lib.lib().eat_embed_match_q8_ws_bytes(N, L, k), device=dev, dtype=torch.uint8)
    score = torch.empty((k,), device=dev, dtype=torch.float32)
    index = torch.empty((k,), device=dev, dtype=torch.int32)
    _lib.call("eat_embed_match_q8", pb, ld, scale.data_ptr(), N, D, seg.data_ptr(), seg.shape[0] - 1, pq, qld, qscale.data_ptr(), L, k,
              sep, min_score, lo, hi, ws.data_ptr(), ws.numel(), score.data_ptr(), index.data_ptr(), _stream())
    return score, index


# ------------------------------------------------------------------ attention-pooling head (models/mn/attention_pooling.py:9-56)
def pitch4(T):
    """Row pitch of the head's (B, rows, T) tensors: T rounded up to a multiple of 4 (16-byte row pieces of the 1x1 kernels)."""
    return (T + 3) // 4 * 4


def _head_out(out, name, shape, like):
    """A caller's output tensor (checked like an operand) or a fresh one."""
    if out is None:
        return torch.empty(shape, device=like.device, dtype=torch.float32)
    n = 1
    for d in shape:
        n *= d
    _glue_operand(out, name, torch.float32, like, n=n)
    return out


def _on_gpu(t, name):
    if not t.is_cuda:
        raise _lib.EatHipError(f"{name} must live on the GPU: efficientat_amd has no CPU path (got device {t.device})")
    if t.device.index != torch.cuda.current_device():
        raise _lib.EatHipError(f"{name} lives on {t.device} but the current device is cuda:{torch.cuda.current_device()}")
    return t.data_ptr()


def freq_mean(y, Tp=None, out=None):
    """xm (B, C, Tp) = mean over the frequency axis of y (B, C, F, T); pad columns [T, Tp) are written as zeros
    (Tp defaults to `pitch4(T)`)."""
    fn = "freq_mean"
    if not isinstance(y, torch.Tensor) or y.dim() != 4 or y.numel() < 1:
        raise _lib.EatHipError(f"{fn}: y must be a non-empty (B, C, F, T) tensor, got {tuple(getattr(y, 'shape', ()))}")
    B, C, F, T = y.shape
    Tp = pitch4(T) if Tp is None else int(Tp)
    if Tp < T:
        raise _lib.EatHipError(f"{fn}: Tp={Tp} is shorter than T={T}")
    _glue_operand(y, f"{fn}: y", torch.float32, y)
    xm = _head_out(out, f"{fn}: out", (B, C, Tp), y)
    _lib.call("eat_freq_mean_fwd", _on_gpu(y, f"{fn}: y"), xm.data_ptr(), B, C, F, T, Tp, _stream())
    return xm


def freq_mean_bwd(dxm, F, T, out=None):
    """dy (B, C, F, T) = dxm[b, c, t] / F from dxm (B, C, Tp), Tp >= T."""
    fn = "freq_mean_bwd"
    if not isinstance(dxm, torch.Tensor) or dxm.dim() != 3 or dxm.numel() < 1:
        raise _lib.EatHipError(f"{fn}: dxm must be a non-empty (B, C, Tp) tensor, got {tuple(getattr(dxm, 'shape', ()))}")
    B, C, Tp = dxm.shape
    F, T = int(F), int(T)
    if F < 1 or T < 1:
        raise _lib.EatHipError(f"{fn}: need F, T >= 1 (got {F}, {T})")
    if Tp < T:
        raise _lib.EatHipError(f"{fn}: Tp={Tp} is shorter than T={T}")
    _glue_operand(dxm, f"{fn}: dxm", torch.float32, dxm)
    dy = _head_out(out, f"{fn}: out", (B, C, F, T), dxm)
    _lib.call("eat_freq_mean_bwd", _on_gpu(dxm, f"{fn}: dxm"), dy.data_ptr(), B, C, F, T, Tp, _stream())
    return dy


def _pool_operands(fn, p, bias, head_w, H, T, eps):
    """Metadata checks shared by `attn_pool` / `attn_pool_bwd` -> (B, K, Tp, bias pointer or None, head_w pointer)."""
    if not isinstance(p, torch.Tensor) or p.dim() != 3 or p.numel() < 1:
        raise _lib.EatHipError(f"{fn}: p must be a non-empty (B, 2 H K, Tp) tensor, got {tuple(getattr(p, 'shape', ()))}")
    B, N, Tp = p.shape
    H, T = int(H), int(T)
    if H < 1 or N % (2 * H):
        raise _lib.EatHipError(f"{fn}: p has {N} rows per sample, not a multiple of 2 H = {2 * H}")
    if T < 1 or Tp < T:
        raise _lib.EatHipError(f"{fn}: Tp={Tp} is shorter than T={T} (or T < 1)")
    if not 0.0 <= float(eps) < 0.5:
        raise _lib.EatHipError(f"{fn}: eps must lie in [0, 0.5) (got {eps})")
    _glue_operand(p, f"{fn}: p", torch.float32, p)
    p_hw = _glue_operand(head_w, f"{fn}: head_w", torch.float32, p, n=H)
    p_bias = None if bias is None else _glue_operand(bias, f"{fn}: bias", torch.float32, p, n=N)
    return B, N // (2 * H), Tp, p_bias, p_hw


def attn_pool(p, bias, head_w, H, T, eps=1e-7, save=False, out=None, o=None, s=None):
    """Attention pooling of the projection p (B, 2 H K, Tp) -> out (B, K) (include/eat_attn.h: eat_attn_pool_fwd); bias (2 H K)
    or None is added to p on load, head_w holds H values.  save=True: -> (out, o, s) with o, s (B, H, K) for `attn_pool_bwd`."""
    fn = "attn_pool"
    B, K, Tp, p_bias, p_hw = _pool_operands(fn, p, bias, head_w, H, T, eps)
    out = _head_out(out, f"{fn}: out", (B, K), p)
    if save or o is not None or s is not None:
        o, s = _head_out(o, f"{fn}: o", (B, H, K), p), _head_out(s, f"{fn}: s", (B, H, K), p)
    _lib.call("eat_attn_pool_fwd", _on_gpu(p, f"{fn}: p"), p_bias, p_hw, float(eps), out.data_ptr(),
              None if o is None else o.data_ptr(), None if s is None else s.data_ptr(), B, int(H), K, int(T), Tp, _stream())
    return (out, o, s) if save else out


def attn_pool_bwd(g, p, bias, head_w, o, s, H, T, eps=1e-7, Np=None, dp=None, dbias=None, dhead_w=None):
    """Backward of `attn_pool` from g (B, K) -> (dp (B, Np, Tp), dbias (2 H K) or None without a bias, dhead_w (H)).
    Np >= 2 H K rows per sample of dp (default 2 H K); pad columns and pad rows of dp are written as zeros."""
    fn = "attn_pool_bwd"
    B, K, Tp, p_bias, p_hw = _pool_operands(fn, p, bias, head_w, H, T, eps)
    H, N = int(H), 2 * int(H) * K
    Np = N if Np is None else int(Np)
    if Np < N:
        raise _lib.EatHipError(f"{fn}: Np={Np} is smaller than 2 H K = {N}")
    p_g = _glue_operand(g, f"{fn}: g", torch.float32, p, n=B * K)
    p_o = _glue_operand(o, f"{fn}: o", torch.float32, p, n=B * H * K)
    p_s = _glue_operand(s, f"{fn}: s", torch.float32, p, n=B * H * K)
    dp = _head_out(dp, f"{fn}: dp", (B, Np, Tp), p)
    if bias is not None or dbias is not None:
        dbias = _head_out(dbias, f"{fn}: dbias", (N,), p)
    dhead_w = _head_out(dhead_w, f"{fn}: dhead_w", (H,), p)
    p_p = _on_gpu(p, f"{fn}: p")
    ws = torch.empty((B * (N + H),), device=p.device, dtype=torch.float32)
    _lib.call("eat_attn_pool_bwd", p_g, p_p, p_bias, p_hw, float(eps), p_o, p_s, dp.data_ptr(),
              None if dbias is None else dbias.data_ptr(), dhead_w.data_ptr(), ws.data_ptr(), B, H, K, int(T), Tp, Np, _stream())
    return dp, dbias, dhead_w


# ------------------------------------------------------------------ sound event detection (include/eat_detect.h)
_DETECT_MAX_M = 31             # widest median of eat_detect_median


class DetectTable:
    """The validated recording table of the detection kernels: per recording (first window, window count, goff, G) -
    its windows are rows [first, first + count) of the logits buffer, its G frames columns [goff, goff + G) of the
    (K, G_total) timelines.  Built by `detect_table` on the host; `dev(device)` uploads it once per device."""

    def __init__(self, rec):
        self.cpu, self.n_rec, self.G_total, self._dev = rec, int(rec.shape[0]), int(rec[-1, 2] + rec[-1, 3]), {}

    def dev(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = self.cpu.to(device)
        return self._dev[key]


def detect_table(rec):
    """Host-side validation of a recording table (CPU array (n_rec, 4) of integers: first window, window count, goff, G)
    -> DetectTable.  first >= 0, count >= 1, G >= 1, goff[0] = 0 and goff[i + 1] = goff[i] + G[i]: the recordings tile
    the timeline axis in order (the kernels bisect over goff), whose length stays below 2^31."""
    fn = "detect_table"
    try:
        t = torch.as_tensor(rec)
    except (ValueError, TypeError) as e:
        raise _lib.EatHipError(f"{fn}: rec is ragged ({e})") from None
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] != 4 or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise _lib.EatHipError(f"{fn}: rec must be an (n_rec >= 1, 4) table of integers (got {tuple(t.shape)}, {t.dtype})")
    t = t.to(device="cpu", dtype=torch.int64)
    first, count, goff, G = t.unbind(1)
    if bool((first < 0).any()) or bool((count < 1).any()):
        raise _lib.EatHipError(f"{fn}: rec needs first >= 0 and count >= 1 in every row")
    if bool((G < 1).any()):
        raise _lib.EatHipError(f"{fn}: rec needs G >= 1 in every row: a recording has at least one frame")
    want = torch.cumsum(G, 0) - G
    if not torch.equal(goff, want):
        i = int((goff != want).nonzero()[0])
        raise _lib.EatHipError(f"{fn}: rec row {i} has goff = {int(goff[i])}, but the recordings before it hold {int(want[i])} "
                               f"frames: goff must be the running sum of G")
    if int(G.sum()) >= 2 ** 31 or int((first + count).max()) >= 2 ** 31:
        raise _lib.EatHipError(f"{fn}: rec holds {int(G.sum())} frames / {int((first + count).max())} windows: 2^31 or more")
    return DetectTable(t.to(torch.int32).contiguous())


def _detect_table(fn, table):
    if not isinstance(table, DetectTable):
        raise _lib.EatHipError(f"{fn}: table must be a DetectTable from ops.detect_table (got {type(table).__name__})")
    return table


def _overlaps(a, b):
    if a.device != b.device:
        return False
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def detect_weights(T, taper="triangle"):
    """The window weights wt (T) float64 of `detect_stitch`: 'uniform' = ones, 'triangle' = min(j + 1, T - j)."""
    import numpy as np
    T = int(T)
    if T < 1:
        raise ValueError(f"detect_weights: need T >= 1 (got {T})")
    if taper == "uniform":
        return np.ones(T, dtype=np.float64)
    if taper == "triangle":
        j = np.arange(T, dtype=np.float64)
        return np.minimum(j + 1.0, T - j)
    raise ValueError(f"detect_weights: taper must be 'uniform' or 'triangle' (got {taper!r})")


def detect_stitch(p, table, Hf, T, wt, out=None):
    """Frame logits p (N_w, K, Tp) of overlapping windows -> prob (K, G_total) fp32: per recording of `table` the
    wt-weighted mean over its windows of sigmoid(p), column j of window q being frame q Hf + j (include/eat_detect.h).
    wt (T) fp32 > 0 on p's device (`detect_weights`); pad columns [T, Tp) of p are never read."""
    fn = "detect_stitch"
    if not isinstance(p, torch.Tensor) or p.dim() != 3 or p.numel() < 1:
        raise _lib.EatHipError(f"{fn}: p must be a non-empty (N_w, K, Tp) tensor, got {tuple(getattr(p, 'shape', ()))}")
    table = _detect_table(fn, table)
    n_w, K, Tp = p.shape
    Hf, T = int(Hf), int(T)
    if not 1 <= T <= Tp:
        raise _lib.EatHipError(f"{fn}: T={T} must lie in [1, Tp = {Tp}]")
    if not 1 <= Hf <= T:
        raise _lib.EatHipError(f"{fn}: Hf={Hf} must lie in [1, T = {T}]")
    _glue_operand(p, f"{fn}: p", torch.float32, p)
    p_wt = _glue_operand(wt, f"{fn}: wt", torch.float32, p, n=T)
    first, count, _, G = table.cpu.to(torch.int64).unbind(1)
    if int((first + count).max()) > n_w:
        raise _lib.EatHipError(f"{fn}: table names window {int((first + count).max()) - 1}, p holds {n_w}")
    short = ((count - 1) * Hf + T < G).nonzero()
    if short.numel():
        i = int(short[0])
        raise _lib.EatHipError(f"{fn}: table row {i}: {int(count[i])} windows of {T} frames every {Hf} do not cover its "
                               f"{int(G[i])} frames")
    prob = _head_out(out, f"{fn}: out", (K, table.G_total), p)
    if _overlaps(prob, p):
        raise _lib.EatHipError(f"{fn}: out must not overlap p")
    p_p = _on_gpu(p, f"{fn}: p")
    _lib.call("eat_detect_stitch", p_p, n_w, K, Tp, table.dev(p.device).data_ptr(), table.n_rec, Hf, T, p_wt,
              prob.data_ptr(), table.G_total, _stream())
    return prob.view(K, table.G_total)


def _timelines(fn, x, name, table):
    if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.numel() < 1:
        raise _lib.EatHipError(f"{fn}: {name} must be a non-empty (K, G_total) tensor, got {tuple(getattr(x, 'shape', ()))}")
    table = _detect_table(fn, table)
    if x.shape[1] != table.G_total:
        raise _lib.EatHipError(f"{fn}: {name} has {x.shape[1]} columns, the table {table.G_total} frames")
    _glue_operand(x, f"{fn}: {name}", torch.float32, x)
    return table, x.shape[0]


def detect_median(prob, table, m, out=None):
    """Running median of odd width m (1 <= m <= 31) along time of prob (K, G_total), per class and per recording of
    `table`, with periodic reflection at the recording's own ends -> filt (K, G_total).  out must not overlap prob."""
    fn = "detect_median"
    table, K = _timelines(fn, prob, "prob", table)
    if isinstance(m, bool) or int(m) != m or not 1 <= int(m) <= _DETECT_MAX_M or int(m) % 2 == 0:
        raise _lib.EatHipError(f"{fn}: m={m} must be an odd integer in [1, {_DETECT_MAX_M}]")
    filt = _head_out(out, f"{fn}: out", (K, table.G_total), prob)
    if _overlaps(filt, prob):
        raise _lib.EatHipError(f"{fn}: out must not overlap prob (the filter reads its neighbours)")
    p_x = _on_gpu(prob, f"{fn}: prob")
    _lib.call("eat_detect_median", p_x, K, table.G_total, table.dev(prob.device).data_ptr(), table.n_rec, int(m),
              filt.data_ptr(), _stream())
    return filt.view(K, table.G_total)


# ------------------------------------------------------------------ width-bank median (include/eat_median_bank.h)
class MedianWidthTable:
    """The validated widths of `detect_median_bank`: cpu (Mw, K) int32, width of slice j and class k, each odd and in
    [1, 31].  Built by `median_width_table` on the host; `dev(device)` uploads it once per device."""

    def __init__(self, widths):
        self.cpu, self.Mw, self.K, self._dev = widths, int(widths.shape[0]), int(widths.shape[1]), {}

    def dev(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = self.cpu.to(device)
        return self._dev[key]


def median_width_table(widths, K):
    """Host-side validation of median widths (CPU array or tensor of integers, (K,) = one slice or (Mw >= 1, K)) ->
    MedianWidthTable.  Every width odd and in [1, 31]; the first that is not is named with its slice, class and value."""
    fn = "median_width_table"
    K = int(K)
    if K < 1:
        raise _lib.EatHipError(f"{fn}: need K >= 1 (got {K})")
    try:
        t = torch.as_tensor(widths)
    except (ValueError, TypeError) as e:
        raise _lib.EatHipError(f"{fn}: widths is ragged ({e})") from None
    if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
        raise _lib.EatHipError(f"{fn}: widths must be integers (got {t.dtype})")
    if t.dim() == 1:
        t = t.unsqueeze(0)
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] != K:
        raise _lib.EatHipError(f"{fn}: widths must be (K,) or (Mw >= 1, K) with K = {K} (got {tuple(torch.as_tensor(widths).shape)})")
    t = t.to(device="cpu", dtype=torch.int64)
    bad = ((t < 1) | (t > _DETECT_MAX_M) | (t % 2 == 0)).nonzero()
    if bad.numel():
        j, k = (int(v) for v in bad[0])
        raise _lib.EatHipError(f"{fn}: slice {j}, class {k}: width {int(t[j, k])} must be an odd integer in [1, {_DETECT_MAX_M}]")
    return MedianWidthTable(t.to(torch.int32).contiguous())


def detect_median_bank(prob, table, widths, out=None):
    """Running medians of prob (K, G_total) for a bank of widths at once (include/eat_median_bank.h) -> filt (Mw, K, G_total):
    filt[j, k] is `detect_median` of prob[k] at width widths[j, k], per recording of `table`, bit for bit.  widths: a
    `MedianWidthTable`, or anything `median_width_table` takes.  prob is read from memory once; out must not overlap prob.
    One launch, no host wait."""
    fn = "detect_median_bank"
    table, K = _timelines(fn, prob, "prob", table)
    if not isinstance(widths, MedianWidthTable):
        widths = median_width_table(widths, K)
    if widths.K != K:
        raise _lib.EatHipError(f"{fn}: the width table holds {widths.K} classes, prob {K}")
    filt = _head_out(out, f"{fn}: out", (widths.Mw, K, table.G_total), prob)
    if _overlaps(filt, prob):
        raise _lib.EatHipError(f"{fn}: out must not overlap prob (the filter reads its neighbours)")
    p_x = _on_gpu(prob, f"{fn}: prob")
    _lib.call("eat_detect_median_bank", p_x, K, table.G_total, table.dev(prob.device).data_ptr(), table.n_rec,
              widths.dev(prob.device).data_ptr(), widths.Mw, filt.data_ptr(), _stream())
    return filt.view(widths.Mw, K, table.G_total)


def check_thresholds(hi, lo, K):
    """Host-side validation of per-class thresholds (CPU arrays of K values, or scalars): 0 < lo <= hi <= 1 ->
    (hi, lo) contiguous fp32 CPU tensors of K values, compared as the fp32 numbers the kernel sees."""
    fn = "detect_events"
    out = []
    for name, v in (("hi", hi), ("lo", lo)):
        t = torch.as_tensor(v, dtype=torch.float32).cpu()
        if t.dim() == 0:
            t = t.expand(K)
        if t.dim() != 1 or t.numel() != K:
            raise _lib.EatHipError(f"{fn}: {name} must be a scalar or hold K = {K} values (got {tuple(t.shape)})")
        out.append(t.contiguous())
    hi_t, lo_t = out
    if not bool(((lo_t > 0) & (lo_t <= hi_t) & (hi_t <= 1)).all()):           # (NaN fails every comparison)
        raise _lib.EatHipError(f"{fn}: thresholds need 0 < lo <= hi <= 1 in every class")
    return hi_t, lo_t


def detect_events(filt, table, hi, lo, max_gap=0, min_len=0):
    """Double-threshold events of every (recording, class) timeline of filt (K, G_total) (include/eat_detect.h) ->
    (ev_i (E, 4) int32: recording, class, onset, exclusive offset in frames of the recording; ev_f (E, 2) fp32: peak and
    mean of filt over the event), sorted by (recording, class, onset).  hi, lo: CPU arrays / scalars, validated by
    `check_thresholds` and uploaded, or fp32 device tensors of K values that were.  Two launches with torch's cumsum and
    one host read of the total between them; no event: empty tensors, no second launch."""
    fn = "detect_events"
    table, K = _timelines(fn, filt, "filt", table)
    max_gap, min_len = int(max_gap), int(min_len)
    if max_gap < 0 or min_len < 0:
        raise _lib.EatHipError(f"{fn}: max_gap and min_len must not be negative (got {max_gap}, {min_len})")
    if table.n_rec * K >= 2 ** 31:
        raise _lib.EatHipError(f"{fn}: {table.n_rec} recordings x {K} classes: 2^31 timelines or more")
    if not (isinstance(hi, torch.Tensor) and hi.is_cuda and isinstance(lo, torch.Tensor) and lo.is_cuda):
        hi, lo = (t.to(filt.device) for t in check_thresholds(hi, lo, K))
    p_hi = _glue_operand(hi, f"{fn}: hi", torch.float32, filt, n=K)
    p_lo = _glue_operand(lo, f"{fn}: lo", torch.float32, filt, n=K)
    p_x = _on_gpu(filt, f"{fn}: filt")
    dev = filt.device
    rec = table.dev(dev).data_ptr()
    count = torch.empty((table.n_rec * K,), device=dev, dtype=torch.int64)
    _lib.call("eat_detect_events_count", p_x, K, table.G_total, rec, table.n_rec, p_hi, p_lo, max_gap, min_len,
              count.data_ptr(), _stream())
    incl = torch.cumsum(count, 0)
    E = int(incl[-1].item())                                   # the one host read
    ev_i = torch.empty((E, 4), device=dev, dtype=torch.int32)
    ev_f = torch.empty((E, 2), device=dev, dtype=torch.float32)
    if E > 0:
        _lib.call("eat_detect_events_write", p_x, K, table.G_total, rec, table.n_rec, p_hi, p_lo, max_gap, min_len,
                  incl.data_ptr(), ev_i.data_ptr(), ev_f.data_ptr(), _stream())
    return ev_i, ev_f


# ------------------------------------------------------------------ event-based scoring (include/eat_event_score.h)
EVENT_SCORE_MAX_REF = 64       # reference events of one (recording, class): bits of the kernel's taken-mask


class EventRefs:
    """The validated reference events of the scoring kernel: ref (E, 3) int32 rows (class, onset, offset) in samples, tol (E)
    int32 offset tolerances, ro (N + 1) int64 - recording i owns the rows [ro[i], ro[i + 1]) - for K classes.  Built by
    `event_refs` on the host; `dev(device)` uploads the three tensors once per device."""

    def __init__(self, ref, tol, ro, K):
        self.ref, self.tol, self.ro, self.K, self._dev = ref, tol, ro, int(K), {}
        self.n_rec, self.E = int(ro.numel()) - 1, int(ref.shape[0])

    def dev(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(t.to(device) for t in (self.ref, self.tol, self.ro))
        return self._dev[key]


def event_refs(ref, ref_tol, ro, K):
    """Host-side validation of reference events (CPU tensors / arrays) -> EventRefs.  ref (E, 3) int32 rows (class, onset,
    offset) with 0 <= class < K and 0 <= onset <= offset; ref_tol (E) int32 >= 0; ro (N + 1) int64 rising from 0 to E; the
    rows of a recording sorted by (class, onset), at most EVENT_SCORE_MAX_REF of one class."""
    fn = "event_refs"
    ref, ref_tol, ro = (torch.as_tensor(t).cpu() for t in (ref, ref_tol, ro))
    K = int(K)
    if K < 1:
        raise _lib.EatHipError(f"{fn}: need K >= 1 (got {K})")
    if ref.dim() != 2 or ref.shape[1] != 3 or ref.dtype != torch.int32:
        raise _lib.EatHipError(f"{fn}: ref must be (E, 3) int32 rows (class, onset, offset), got {ref.dtype} {tuple(ref.shape)}")
    E = int(ref.shape[0])
    if ref_tol.dim() != 1 or ref_tol.numel() != E or ref_tol.dtype != torch.int32:
        raise _lib.EatHipError(f"{fn}: ref_tol must be (E,) = ({E},) int32, got {ref_tol.dtype} {tuple(ref_tol.shape)}")
    if ro.dim() != 1 or ro.numel() < 2 or ro.dtype != torch.int64:
        raise _lib.EatHipError(f"{fn}: ro must be (n_rec + 1 >= 2,) int64, got {ro.dtype} {tuple(ro.shape)}")
    d = ro[1:] - ro[:-1]
    if int(ro[0]) != 0 or int(ro[-1]) != E or bool((d < 0).any()):
        raise _lib.EatHipError(f"{fn}: ro must rise from 0 to E = {E} (got {int(ro[0])} .. {int(ro[-1])})")
    cls, on, off = (ref[:, j].to(torch.int64) for j in range(3))
    if E and (int(cls.min()) < 0 or int(cls.max()) >= K):
        raise _lib.EatHipError(f"{fn}: ref names a class outside [0, {K})")
    if bool(((on < 0) | (off < on)).any()):
        e = int(((on < 0) | (off < on)).nonzero()[0])
        raise _lib.EatHipError(f"{fn}: ref row {e} = {ref[e].tolist()} breaks 0 <= onset <= offset")
    if bool((ref_tol < 0).any()):
        raise _lib.EatHipError(f"{fn}: ref_tol row {int((ref_tol < 0).nonzero()[0])} is negative")
    rec = torch.repeat_interleave(torch.arange(ro.numel() - 1), d)            # the recording of every row
    if E > 1:
        same = rec[1:] == rec[:-1]
        ok = (cls[1:] > cls[:-1]) | ((cls[1:] == cls[:-1]) & (on[1:] >= on[:-1]))
        if bool((same & ~ok).any()):
            e = int((same & ~ok).nonzero()[0]) + 1
            raise _lib.EatHipError(f"{fn}: ref row {e} is out of order: a recording's rows are sorted by (class, onset)")
    if E:
        per = torch.bincount(rec * K + cls)
        if int(per.max()) > EVENT_SCORE_MAX_REF:
            j = int(per.argmax())
            raise _lib.EatHipError(f"{fn}: recording {j // K} holds {int(per[j])} reference events of class {j % K}: the "
                                   f"matching kernel takes at most {EVENT_SCORE_MAX_REF} per recording and class")
    return EventRefs(ref.contiguous(), ref_tol.contiguous(), ro.contiguous(), K)


def check_threshold_grid(hi, lo):
    """`check_thresholds` for a grid of V >= 1 threshold pairs (CPU arrays of one length): 0 < lo <= hi <= 1 ->
    (hi, lo) contiguous fp32 CPU tensors, compared as the fp32 numbers the kernel sees."""
    fn = "event_score"
    hi_t, lo_t = (torch.as_tensor(v, dtype=torch.float32).cpu().contiguous() for v in (hi, lo))
    if hi_t.dim() != 1 or hi_t.numel() < 1 or lo_t.shape != hi_t.shape:
        raise _lib.EatHipError(f"{fn}: hi and lo must hold V >= 1 values each (got {tuple(hi_t.shape)}, {tuple(lo_t.shape)})")
    if not bool(((lo_t > 0) & (lo_t <= hi_t) & (hi_t <= 1)).all()):           # (NaN fails every comparison)
        raise _lib.EatHipError(f"{fn}: thresholds need 0 < lo <= hi <= 1 in every pair")
    return hi_t, lo_t


def _score_operands(fn, filt, table, nsamp, R, refs, hi, lo, max_gap, min_len, first):
    """The operands `event_score` and `psds_count` share, checked in one place -> (table, K, R, max_gap, min_len, first,
    nsamp, hi, lo, V) with nsamp / hi / lo on filt's device."""
    table, K = _timelines(fn, filt, "filt", table)
    if not isinstance(refs, EventRefs):
        raise _lib.EatHipError(f"{fn}: refs must be an EventRefs from ops.event_refs (got {type(refs).__name__})")
    if refs.K != K:
        raise _lib.EatHipError(f"{fn}: refs hold {refs.K} classes, filt {K}")
    R, max_gap, min_len, first = int(R), int(max_gap), int(min_len), int(first)
    if R < 1:
        raise _lib.EatHipError(f"{fn}: need R >= 1 samples per frame (got {R})")
    if max_gap < 0 or min_len < 0:
        raise _lib.EatHipError(f"{fn}: max_gap and min_len must not be negative (got {max_gap}, {min_len})")
    if first < 0 or first + table.n_rec > refs.n_rec:
        raise _lib.EatHipError(f"{fn}: recordings [{first}, {first + table.n_rec}) lie outside the {refs.n_rec} of refs")
    if table.n_rec * K >= 2 ** 31:
        raise _lib.EatHipError(f"{fn}: {table.n_rec} recordings x {K} classes: 2^31 timelines or more")
    if not (isinstance(nsamp, torch.Tensor) and nsamp.is_cuda):
        nsamp = torch.as_tensor(nsamp).cpu()
        if nsamp.dim() != 1 or nsamp.numel() != table.n_rec or nsamp.dtype.is_floating_point or nsamp.dtype == torch.bool:
            raise _lib.EatHipError(f"{fn}: nsamp must hold n_rec = {table.n_rec} integers (got {nsamp.dtype} {tuple(nsamp.shape)})")
        if bool((nsamp < 1).any()):
            raise _lib.EatHipError(f"{fn}: nsamp needs >= 1 sample in every recording")
        nsamp = nsamp.to(device=filt.device, dtype=torch.int64)
    _glue_operand(nsamp, f"{fn}: nsamp", torch.int64, filt, n=table.n_rec)
    if not (isinstance(hi, torch.Tensor) and hi.is_cuda and isinstance(lo, torch.Tensor) and lo.is_cuda):
        try:
            hi, lo = (t.to(filt.device) for t in check_threshold_grid(hi, lo))
        except _lib.EatHipError as e:
            raise _lib.EatHipError(str(e).replace("event_score:", f"{fn}:", 1)) from None
    V = int(hi.numel())
    if V < 1 or V > 64 * 65535:
        raise _lib.EatHipError(f"{fn}: V = {V} threshold pairs must lie in [1, {64 * 65535}]")
    _glue_operand(hi, f"{fn}: hi", torch.float32, filt, n=V)
    _glue_operand(lo, f"{fn}: lo", torch.float32, filt, n=V)
    return table, K, R, max_gap, min_len, first, nsamp, hi, lo, V


def event_score(filt, table, nsamp, R, refs, c, hi, lo, max_gap=0, min_len=0, first=0, out=None):
    """Event-based scoring of every (recording, class) timeline of filt (K, G_total) at V threshold pairs at once
    (include/eat_event_score.h) -> counts (n_rec, K, V, 2) int32: (tp, n_est) - the events `detect_events` would list at
    (hi[v], lo[v], max_gap, min_len), in samples [on R, min(off R, nsamp)), matched against the reference events with
    |onset distance| <= c and |offset distance| <= tol.  The recordings of `table` are recordings [first, first + n_rec)
    of `refs` (an `EventRefs`).  nsamp: their lengths in samples, (n_rec) int64 on filt's device, or a CPU array that is
    checked (>= 1) and uploaded.  hi, lo: CPU arrays validated by `check_threshold_grid` and uploaded, or fp32 device
    tensors of V values that were.  One launch, no host wait."""
    fn = "event_score"
    c = int(c)
    if c < 0 or c >= 2 ** 31:
        raise _lib.EatHipError(f"{fn}: c must not be negative (got {c})")
    table, K, R, max_gap, min_len, first, nsamp, hi, lo, V = _score_operands(fn, filt, table, nsamp, R, refs, hi, lo, max_gap,
                                                                             min_len, first)
    n_out = table.n_rec * K * V * 2
    if out is None:
        out = torch.empty((table.n_rec, K, V, 2), device=filt.device, dtype=torch.int32)
    else:
        _glue_operand(out, f"{fn}: out", torch.int32, filt, n=n_out)
    p_x = _on_gpu(filt, f"{fn}: filt")
    ref, tol, ro = refs.dev(filt.device)
    _lib.call("eat_event_score", p_x, K, table.G_total, table.dev(filt.device).data_ptr(), table.n_rec, nsamp.data_ptr(), R,
              ref.data_ptr() if refs.E else None, tol.data_ptr() if refs.E else None, ro.data_ptr() + 8 * first, refs.E, c,
              hi.data_ptr(), lo.data_ptr(), V, max_gap, min_len, out.data_ptr(), _stream())
    return out.view(table.n_rec, K, V, 2)


# ------------------------------------------------------------------ PSDS counting (include/eat_psds.h)
def per_mille(name, x, lowest=1):
    """A criterion given as a ratio -> its whole number of per-mille in [lowest, 1000]; anything else (a ratio outside the
    range, or one that is no whole per-mille within 1e-9) is refused by name."""
    fn = "psds_count"
    try:
        f = float(x)
    except (TypeError, ValueError):
        raise _lib.EatHipError(f"{fn}: {name}={x!r} is not a number") from None
    pm = round(1000.0 * f) if f == f and abs(f) < 1e6 else None
    if pm is None or abs(1000.0 * f - pm) > 1e-9:
        raise _lib.EatHipError(f"{fn}: {name}={x!r} must be a whole number of per-mille (0.7, 0.105, ...)")
    if not lowest <= pm <= 1000:
        raise _lib.EatHipError(f"{fn}: {name}={x!r} must lie in {'(0, 1]' if lowest else '[0, 1]'}")
    return int(pm)


def psds_count(filt, table, nsamp, R, refs, dtc, gtc, cttc, hi, lo, max_gap=0, min_len=0, first=0, out=None, ct=None):
    """The integer counts behind PSDS of every (recording, class) timeline of filt (K, G_total) at V threshold pairs at once
    (include/eat_psds.h) -> (counts (n_rec, K, V, 4) int32: (tp, n_det, fp, n_ct), ct (V, K, K) int32 or None).  The
    detections are the events `detect_events` would list at (hi[v], lo[v], max_gap, min_len), in samples [on R, min(off R,
    nsamp)); dtc, gtc in (0, 1] and cttc in [0, 1] are the intersection criteria as ratios that are a whole number of
    per-mille.  ct[v, detection class, reference class] counts cross-triggers and is ADDED TO: allocated zeroed when None and
    cttc > 0, else the caller's (V, K, K) int32 device buffer; with cttc = 0 it is not touched.  The other operands are
    `event_score`'s (the tolerances of `refs` are not used).  One launch, no host wait."""
    fn = "psds_count"
    dtc_pm, gtc_pm, cttc_pm = per_mille("dtc", dtc), per_mille("gtc", gtc), per_mille("cttc", cttc, 0)
    table, K, R, max_gap, min_len, first, nsamp, hi, lo, V = _score_operands(fn, filt, table, nsamp, R, refs, hi, lo, max_gap,
                                                                             min_len, first)
    if out is None:
        out = torch.empty((table.n_rec, K, V, 4), device=filt.device, dtype=torch.int32)
    else:
        _glue_operand(out, f"{fn}: out", torch.int32, filt, n=table.n_rec * K * V * 4)
    if ct is not None:
        if not isinstance(ct, torch.Tensor) or tuple(ct.shape) != (V, K, K):
            raise _lib.EatHipError(f"{fn}: ct must be a (V, K, K) = ({V}, {K}, {K}) tensor (got {tuple(getattr(ct, 'shape', ()))})")
        _glue_operand(ct, f"{fn}: ct", torch.int32, filt, n=V * K * K)
    elif cttc_pm > 0:
        ct = torch.zeros((V, K, K), device=filt.device, dtype=torch.int32)
    p_x = _on_gpu(filt, f"{fn}: filt")
    ref, _, ro = refs.dev(filt.device)
    _lib.call("eat_psds_count", p_x, K, table.G_total, table.dev(filt.device).data_ptr(), table.n_rec, nsamp.data_ptr(), R,
              ref.data_ptr() if refs.E else None, ro.data_ptr() + 8 * first, refs.E, dtc_pm, gtc_pm, cttc_pm, hi.data_ptr(),
              lo.data_ptr(), V, max_gap, min_len, out.data_ptr(), ct.data_ptr() if ct is not None and cttc_pm > 0 else None,
              _stream())
    return out.view(table.n_rec, K, V, 4), ct


def pw_conv_into(x, pack, Co, act, out):
    """The 1x1 conv of `mn._pw` on a (packed weights, bias, mode) triple of `mn._pack_pw`, stored into the caller's
    contiguous fp32 buffer `out` of B x Co x S elements (a slice of a larger buffer) instead of a fresh tensor."""
    wp, bias, mode = pack
    B, Ci, F, T = x.shape
    p_out = _glue_operand(out, "pw_conv_into: out", torch.float32, x, n=B * Co * F * T)
    if mode == "fp32":
        _lib.call("eat_pw_conv_fwd", _dev(x, "x"), _dev(wp, "wp"), _dev(bias, "bias"), None, None, p_out, None, B, Ci, Co,
                  F * T, act, _stream())
    else:
        _lib.call("eat_pw_conv_bf16_fwd", _dev(x, "x"), wp.data_ptr(), _dev(bias, "bias"), None, None, p_out, None, B, Ci, Co,
                  F * T, act, 1 if mode == "bf16x3" else 0, _stream())
    return out


# ------------------------------------------------------------------ strong-label SED training (include/eat_sed.h)
def check_eval_draws(idx, start, lengths_cpu):
    """Host-side validation of evaluation tables of `sed_targets` (CPU tensors of 2B values): primary rows in [0, N),
    partners in [-1, N) and 0 <= start < length for every slot in use (an evaluation window may be padded)."""
    idx, start = torch.as_tensor(idx), torch.as_tensor(start)
    lengths = torch.as_tensor(lengths_cpu).to(torch.int64)
    n_bank = lengths.numel()
    if idx.numel() % 2 or idx.numel() == 0 or idx.numel() != start.numel():
        raise ValueError(f"sed_targets: idx / start must hold 2B values each (got {idx.numel()}, {start.numel()})")
    prim, part = idx[0::2], idx[1::2]
    if bool(((prim < 0) | (prim >= n_bank)).any()) or bool(((part < -1) | (part >= n_bank)).any()):
        raise ValueError(f"sed_targets: a bank index lies outside [0, {n_bank}) (partners may be -1)")
    used = idx >= 0
    st = start[used].to(torch.int64)
    if bool(((st < 0) | (st >= lengths[idx[used].long()])).any()):
        raise ValueError("sed_targets: a window start lies outside its clip")


def _event_bank_operands(fn, bank):
    """`sed.load_bank`'s event table, checked from metadata -> (events or None, E, event_offsets, lengths, n_bank, K, strong or None)."""
    events, eo, lengths, strong = bank["events"], bank["event_offsets"], bank["lengths"], bank.get("strong")
    n_bank, dev = lengths.numel(), lengths.device
    if (events.dtype != torch.int32 or events.dim() != 2 or events.shape[1] != 3 or not events.is_contiguous()
            or events.device != dev):
        raise _lib.EatHipError(f"{fn}: events must be a contiguous (E, 3) int32 tensor on {dev}")
    if eo.dtype != torch.int64 or eo.numel() != n_bank + 1 or not eo.is_contiguous() or eo.device != dev:
        raise _lib.EatHipError(f"{fn}: event_offsets must be a contiguous int64 tensor of N + 1 = {n_bank + 1} values on {dev}")
    p_strong = None if strong is None else _glue_operand(strong, f"{fn}: strong", torch.uint8, lengths, n=n_bank)
    E = events.shape[0]
    return events.data_ptr() if E else None, E, eo.data_ptr(), lengths, n_bank, len(bank["classes"]), p_strong


def sed_targets(bank, idx, start, shift, mix, L, R, T, Tp=None, out=None, train=True):
    """Frame targets y (B, K, Tp) of the batch that `wave_augment_ragged` builds from the same tables (include/eat_sed.h:
    eat_sed_targets).  bank: the dict of `sed.load_bank` (events (E, 3) int32, event_offsets (N + 1) int64, lengths on the
    device, lengths_cpu, classes).  idx / start / shift (2B) int32, mix (B) fp32: CPU tensors are validated here -
    `check_ragged_draws` with train=True, `check_eval_draws` (0 <= start < length) otherwise - and uploaded; device tensors
    (the static buffers of a captured step) must have been validated before they were staged.  L samples per window, R per
    frame, T frames, Tp >= T the row pitch (default `pitch4(T)`)."""
    fn = "sed_targets"
    lengths = bank["lengths"]
    L, R, T = int(L), int(R), int(T)
    Tp = pitch4(T) if Tp is None else int(Tp)
    B = torch.as_tensor(mix).numel()
    dev = lengths.device
    if L < 1 or R < 1 or T < 1 or Tp < T or B < 1:
        raise _lib.EatHipError(f"{fn}: need B, L, R, T >= 1 and Tp >= T (got B={B} L={L} R={R} T={T} Tp={Tp})")

    def check():
        if train:
            check_ragged_draws(idx, start, shift, bank["lengths_cpu"], L)
        else:
            check_eval_draws(idx, start, bank["lengths_cpu"])
            if torch.as_tensor(shift).numel() != 2 * B or bool((torch.as_tensor(shift).abs() >= L).any()):
                raise ValueError(f"{fn}: shift must hold 2B values inside (-{L}, {L})")

    idx, start, shift, mix = _stage_draws(dev, check, (idx, start, shift), (mix,))
    p_ev, E, p_eo, lengths, n_bank, K, _ = _event_bank_operands(fn, bank)
    p_mix = _glue_operand(mix, f"{fn}: mix", torch.float32, lengths, n=B)
    y = _head_out(out, f"{fn}: out", (B, K, Tp), lengths)
    _lib.call("eat_sed_targets", p_ev, E, p_eo, _dev_int32(lengths, "lengths", n_bank), n_bank,
              K, _dev_int32(idx, "idx", 2 * B), _dev_int32(start, "start", 2 * B), _dev_int32(shift, "shift", 2 * B), p_mix, B,
              L, R, T, Tp, _on_gpu(y, f"{fn}: out"), _stream())
    return y.view(B, K, Tp)


def _frame_geometry(fn, z, T, Kp):
    """The (B, K, Tp) logits of `frame_bce_fwd_bwd` / `weak_frame_bce_fwd_bwd` with T frames and Kp >= K rows -> (B, K, Tp, T, Kp)."""
    if not isinstance(z, torch.Tensor) or z.dim() != 3 or z.numel() < 1:
        raise _lib.EatHipError(f"{fn}: z must be a non-empty (B, K, Tp) tensor, got {tuple(getattr(z, 'shape', ()))}")
    B, K, Tp = z.shape
    T = int(T)
    Kp = K if Kp is None else int(Kp)
    if T < 1 or Tp < T or Kp < K:
        raise _lib.EatHipError(f"{fn}: need 1 <= T <= Tp and Kp >= K (got T={T} Tp={Tp} K={K} Kp={Kp})")
    return B, K, Tp, T, Kp


def _frame_loss_buffers(fn, z, K, Kp, sums, n_sums, n_ws, grad, dbias):
    """After every operand is checked: `sums` (>= n_sums fp32) with its fp64 workspace of n_ws values, dlogits (B, Kp, Tp) and
    dbias (K) -> (sums pointer, ws, dl, db); what is not asked for is None."""
    p_sums = ws = None
    if sums is not None:
        p_sums = _glue_operand(sums, f"{fn}: sums", torch.float32, z, at_least=n_sums)
        ws = torch.empty(n_ws, device=z.device, dtype=torch.float64)
    dl = torch.empty((z.shape[0], Kp, z.shape[2]), device=z.device, dtype=torch.float32) if grad else None
    db = torch.empty((K,), device=z.device, dtype=torch.float32) if dbias else None
    return p_sums, ws, dl, db


def frame_bce_fwd_bwd(z, y, T, perm=None, lam=None, nframes=None, sums=None, grad=True, Kp=None, dbias=False, counts=None,
                      thr=None, rows=None):
    """Frame-level BCE-with-logits of z (B, K, Tp) against y (B, K, Tp) over the frames t < T (t < nframes[b] with `nframes`
    (B) int32), the log-mel mix-up of the targets folded in (include/eat_sed.h: eat_frame_bce_fwd_bwd).
    -> (dlogits (B, Kp, Tp) or None with grad=False, dbias (K) or None): d mean-loss / d z with exactly-zero pad rows and
    columns.  `sums` (>= 1 fp32) += the mean; `counts` (K, 3) int64 += (tp, fp, fn) of sigmoid(z) >= thr (K) against
    y > 0.5 (not with perm); `rows` (B T, K) fp32 receives the logits as the row-major score matrix of `metrics.ap_auc`."""
    fn = "frame_bce_fwd_bwd"
    B, K, Tp, T, Kp = _frame_geometry(fn, z, T, Kp)
    _glue_operand(z, f"{fn}: z", torch.float32, z)
    p_y = _glue_operand(y, f"{fn}: y", torch.float32, z, n=B * K * Tp)
    p_perm, p_lam = _mix_operands(fn, perm, lam, B, z)
    p_nf = None if nframes is None else _glue_operand(nframes, f"{fn}: nframes", torch.int32, z, n=B)
    p_counts = p_thr = None
    if counts is not None:
        if perm is not None:
            raise _lib.EatHipError(f"{fn}: counts are taken against unmixed targets (perm given)")
        if thr is None:
            raise _lib.EatHipError(f"{fn}: counts need thr")
        p_counts = _glue_operand(counts, f"{fn}: counts", torch.int64, z, n=3 * K)
        p_thr = _glue_operand(thr, f"{fn}: thr", torch.float32, z, n=K)
    p_rows = None if rows is None else _glue_operand(rows, f"{fn}: rows", torch.float32, z, n=B * T * K)
    p_sums, ws, dl, db = _frame_loss_buffers(fn, z, K, Kp, sums, 1, K + 1, grad, dbias)
    _lib.call("eat_frame_bce_fwd_bwd", _on_gpu(z, f"{fn}: z"), p_y, p_perm, p_lam, p_nf, p_thr, B, K, T, Tp, Kp, p_sums,
              None if dl is None else dl.data_ptr(), None if db is None else db.data_ptr(), p_counts, p_rows,
              None if ws is None else ws.data_ptr(), _stream())
    return dl, db


def frame_grad_pad(g, T, Kp=None, out=None):
    """A gradient g (B, K, Tp) arriving at frame logits -> (dl (B, Kp, Tp): g with rows [K, Kp) and columns [T, Tp) exactly
    zero, db (K) = the sum of g over (b, t < T), fp64 inside, fixed order) (include/eat_sed.h: eat_frame_grad_pad).  out:
    the (B, Kp, Tp) buffer to store dl into."""
    fn = "frame_grad_pad"
    if not isinstance(g, torch.Tensor) or g.dim() != 3 or g.numel() < 1:
        raise _lib.EatHipError(f"{fn}: g must be a non-empty (B, K, Tp) tensor, got {tuple(getattr(g, 'shape', ()))}")
    B, K, Tp = g.shape
    T = int(T)
    Kp = K if Kp is None else int(Kp)
    if T < 1 or Tp < T or Kp < K:
        raise _lib.EatHipError(f"{fn}: need 1 <= T <= Tp and Kp >= K (got T={T} Tp={Tp} K={K} Kp={Kp})")
    _glue_operand(g, f"{fn}: g", torch.float32, g)
    dl = _head_out(out, f"{fn}: out", (B, Kp, Tp), g)
    db = torch.empty((K,), device=g.device, dtype=torch.float32)
    _lib.call("eat_frame_grad_pad", _on_gpu(g, f"{fn}: g"), dl.data_ptr(), db.data_ptr(), B, K, Kp, T, Tp, _stream())
    return dl.view(B, Kp, Tp), db


def _keep_operand(fn, keep, B, Hp, like):
    return None if keep is None else _glue_operand(keep, f"{fn}: keep", torch.float32, like, n=B * Hp)


def frame_hidden_fwd(z1, keep=None):
    """h = hswish(z1) keep[b, j] over z1 (B, Hp, Tp); keep (B, Hp) or None (include/eat_sed.h: eat_frame_hidden_fwd)."""
    fn = "frame_hidden_fwd"
    if not isinstance(z1, torch.Tensor) or z1.dim() != 3 or z1.numel() < 1:
        raise _lib.EatHipError(f"{fn}: z1 must be a non-empty (B, Hp, Tp) tensor, got {tuple(getattr(z1, 'shape', ()))}")
    B, Hp, Tp = z1.shape
    _glue_operand(z1, f"{fn}: z1", torch.float32, z1)
    p_keep = _keep_operand(fn, keep, B, Hp, z1)
    h = torch.empty_like(z1)
    _lib.call("eat_frame_hidden_fwd", _on_gpu(z1, f"{fn}: z1"), p_keep, h.data_ptr(), B, Hp, Tp, _stream())
    return h


def frame_hidden_bwd(dh, z1, keep, H, T):
    """-> (dz1 (B, Hp, Tp) = dh keep hswish'(z1), exactly zero in rows [H, Hp) and columns [T, Tp); db1 (H) = its sum over
    (b, t), fp64 inside, fixed order) (include/eat_sed.h: eat_frame_hidden_bwd)."""
    fn = "frame_hidden_bwd"
    if not isinstance(z1, torch.Tensor) or z1.dim() != 3 or z1.numel() < 1:
        raise _lib.EatHipError(f"{fn}: z1 must be a non-empty (B, Hp, Tp) tensor, got {tuple(getattr(z1, 'shape', ()))}")
    B, Hp, Tp = z1.shape
    H, T = int(H), int(T)
    if H < 1 or T < 1 or Hp < H or Tp < T:
        raise _lib.EatHipError(f"{fn}: need 1 <= H <= Hp and 1 <= T <= Tp (got H={H} Hp={Hp} T={T} Tp={Tp})")
    _glue_operand(z1, f"{fn}: z1", torch.float32, z1)
    p_dh = _glue_operand(dh, f"{fn}: dh", torch.float32, z1, n=B * Hp * Tp)
    p_keep = _keep_operand(fn, keep, B, Hp, z1)
    dz1 = torch.empty_like(z1)
    db1 = torch.empty((H,), device=z1.device, dtype=torch.float32)
    _lib.call("eat_frame_hidden_bwd", p_dh, _on_gpu(z1, f"{fn}: z1"), p_keep, dz1.data_ptr(), db1.data_ptr(), B, H, Hp, T, Tp,
              _stream())
    return dz1, db1


# ------------------------------------------------------------------ weak-label SED training (include/eat_weak_sed.h)
def sed_clip_targets(bank, idx, start, mix, L, out=None, framed_out=None):
    """Clip-level targets w (B, K) and the frame-truth flag framed (B) int32 of the batch that `wave_augment_ragged` builds
    from the same tables (include/eat_weak_sed.h: eat_sed_clip_targets).  bank: the dict of `sed.load_bank`; its "strong"
    (N) uint8 marks the clips with onset / offset annotation (absent: every clip).  idx / start (2B) int32, mix (B) fp32:
    CPU tensors are validated here with `check_ragged_draws` and uploaded; device tensors (the static buffers of a captured
    step) must have been validated before they were staged.  L samples per window.  -> (w, framed)."""
    fn = "sed_clip_targets"
    lengths = bank["lengths"]
    L = int(L)
    B = torch.as_tensor(mix).numel()
    dev = lengths.device
    if L < 1 or B < 1:
        raise _lib.EatHipError(f"{fn}: need B, L >= 1 (got B={B} L={L})")
    idx, start, mix = _stage_draws(
        dev, lambda: check_ragged_draws(idx, start, torch.zeros_like(torch.as_tensor(idx)), bank["lengths_cpu"], L), (idx, start),
        (mix,))
    p_ev, E, p_eo, lengths, n_bank, K, p_strong = _event_bank_operands(fn, bank)
    p_mix = _glue_operand(mix, f"{fn}: mix", torch.float32, lengths, n=B)
    w = _head_out(out, f"{fn}: out", (B, K), lengths)
    if framed_out is None:
        framed_out = torch.empty((B,), device=dev, dtype=torch.int32)
    p_framed = _glue_operand(framed_out, f"{fn}: framed_out", torch.int32, lengths, n=B)
    _lib.call("eat_sed_clip_targets", p_ev, E, p_eo, _dev_int32(lengths, "lengths", n_bank),
              n_bank, K, _dev_int32(idx, "idx", 2 * B), _dev_int32(start, "start", 2 * B), p_mix, p_strong, B, L,
              _on_gpu(w, f"{fn}: out"), p_framed, _stream())
    return w.view(B, K), framed_out


def weak_frame_bce_fwd_bwd(z, y, w, framed, T, perm=None, lam=None, weak_weight=1.0, eps=1e-7, sums=None, grad=True, Kp=None,
                           dbias=False, clip_prob=None):
    """Frame BCE of z (B, K, Tp) against y (B, K, Tp) over the samples with framed (B) int32 != 0, plus `weak_weight` times
    the clip-level BCE of the linear-softmax pooled frame probabilities against w (B, K), the log-mel mix-up of both targets
    folded in (include/eat_weak_sed.h: eat_weak_frame_bce_fwd_bwd).
    -> (dlogits (B, Kp, Tp) or None with grad=False, dbias (K) or None): d loss / d z with exactly-zero pad rows and columns.
    `sums` (>= 3 fp32) += (loss, frame term, clip term); `clip_prob` (B, K) fp32 receives the pooled probabilities."""
    fn = "weak_frame_bce_fwd_bwd"
    B, K, Tp, T, Kp = _frame_geometry(fn, z, T, Kp)
    weak_weight, eps = float(weak_weight), float(eps)
    if not 0.0 <= weak_weight < float("inf"):
        raise _lib.EatHipError(f"{fn}: weak_weight must be finite and not negative (got {weak_weight})")
    if not 0.0 < eps < 0.5:
        raise _lib.EatHipError(f"{fn}: eps must lie in (0, 0.5) (got {eps})")
    _glue_operand(z, f"{fn}: z", torch.float32, z)
    p_y = _glue_operand(y, f"{fn}: y", torch.float32, z, n=B * K * Tp)
    p_w = _glue_operand(w, f"{fn}: w", torch.float32, z, n=B * K)
    p_framed = _glue_operand(framed, f"{fn}: framed", torch.int32, z, n=B)
    p_perm, p_lam = _mix_operands(fn, perm, lam, B, z)
    p_cp = None if clip_prob is None else _glue_operand(clip_prob, f"{fn}: clip_prob", torch.float32, z, n=B * K)
    p_sums, ws, dl, db = _frame_loss_buffers(fn, z, K, Kp, sums, 3, 2 * K + 1, grad, dbias)
    _lib.call("eat_weak_frame_bce_fwd_bwd", _on_gpu(z, f"{fn}: z"), p_y, p_w, p_framed, p_perm, p_lam, weak_weight, eps, B, K, T,
              Tp, Kp, p_sums, None if dl is None else dl.data_ptr(), None if db is None else db.data_ptr(), p_cp,
              None if ws is None else ws.data_ptr(), _stream())
    return dl, db
