// Batch-statistics BatchNorm of the training step for gfx950, forward and backward, with the activation folded in:
// channel statistics, finalize, y = act(a z + b), the backward reduce and apply passes, the plane dot product of the
// squeeze-excitation backward, the stand-alone passes of the bf16-storage plan (act_io.h) and eat_cast_b16.
//   reference semantics: nn.BatchNorm2d(eps=1e-3, momentum=0.01) in train mode (models/mn/model.py:114-115), nn.Hardswish /
//   nn.ReLU (SURVEY.md Appendix C lists the formulas the reference leaves to autograd).
// Every pass is its own streaming kernel over (B, C, S) planes (one workgroup per plane, float4 along the time axis,
// wave-shuffle + LDS block reduction, per-channel totals accumulated in fp64 atomics so that sums over up to 8M elements
// do not lose precision).
#include "eat_common.h"
#include "act_io.h"

namespace {

using eat::Io;

template <int ACT>
__device__ __forceinline__ float act_grad(float u) {   // d act(u) / du  (PyTorch conventions)
  if constexpr (ACT == EAT_ACT_RELU) return u > 0.0f ? 1.0f : 0.0f;
  if constexpr (ACT == EAT_ACT_HSWISH) return u < -3.0f ? 0.0f : (u <= 3.0f ? u * (1.0f / 3.0f) + 0.5f : 1.0f);
  return 1.0f;
}

// block-wide sum of two values; result valid in thread 0
__device__ __forceinline__ void block_sum2(float& a, float& b, float* s_red) {
  a = eat::wave_sum(a);
  b = eat::wave_sum(b);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0) { s_red[wv] = a; s_red[8 + wv] = b; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = blockDim.x >> 6;
    float ta = 0.f, tb = 0.f;
    for (int i = 0; i < nw; ++i) { ta += s_red[i]; tb += s_red[8 + i]; }
    a = ta; b = tb;
  }
}

// ---- per-channel sum / sum of squares of z (B,C,S) -----------------------------------------
__global__ __launch_bounds__(256) void bn_stats_kernel(const float* __restrict__ z, int C, int S,
                                                       double* __restrict__ sums) {
  __shared__ float s_red[16];
  const int plane = blockIdx.x, c = plane % C;
  const float* p = z + (size_t)plane * S;
  float s1 = 0.f, s2 = 0.f;
  if ((S & 3) == 0) {
#pragma unroll 4
    for (int i = threadIdx.x * 4; i < S; i += blockDim.x * 4) {
      const float4 v = *reinterpret_cast<const float4*>(p + i);
      s1 += (v.x + v.y) + (v.z + v.w);
      s2 += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
    }
  } else {
    for (int i = threadIdx.x; i < S; i += blockDim.x) { const float v = p[i]; s1 += v; s2 += v * v; }
  }
  block_sum2(s1, s2, s_red);
  if (threadIdx.x == 0) {
    atomicAdd(sums + c, (double)s1);
    atomicAdd(sums + C + c, (double)s2);
  }
}

// Small planes (late stages: 8x63, 4x32 positions): with one block per plane the 2 x B x C fp64 atomics on C addresses
// are the whole cost (~50 us per launch for 20 MB tensors, 46 launches per step).  Here a block owns PPB samples of ONE
// channel: the same coalesced float4 reads, PPB times fewer atomics per channel.
__global__ __launch_bounds__(256) void bn_stats_multi_kernel(const float* __restrict__ z, int B, int C, int S4, int PPB,
                                                             double* __restrict__ sums) {
  __shared__ float s_red[16];
  const int c = blockIdx.x, b0 = blockIdx.y * PPB;
  const int nb = (B - b0) < PPB ? (B - b0) : PPB;
  float s1 = 0.f, s2 = 0.f;
  for (int e = threadIdx.x; e < nb * S4; e += 256) {
    const int bl = e / S4, i = e - bl * S4;
    const float4 v = *reinterpret_cast<const float4*>(z + ((size_t)(b0 + bl) * C + c) * (4 * S4) + 4 * i);
    s1 += (v.x + v.y) + (v.z + v.w);
    s2 += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
  }
  block_sum2(s1, s2, s_red);
  if (threadIdx.x == 0) {
    atomicAdd(sums + c, (double)s1);
    atomicAdd(sums + C + c, (double)s2);
  }
}

// ---- finalize: batch mean / biased var -> affine (a, b), saved (mean, invstd), running buffers --
__global__ void bn_finalize_kernel(const double* __restrict__ sums, const float* __restrict__ gamma,
                                   const float* __restrict__ beta, float* __restrict__ running_mean,
                                   float* __restrict__ running_var, float momentum, float eps, double n, int C,
                                   float* __restrict__ a, float* __restrict__ b, float* __restrict__ mean,
                                   float* __restrict__ invstd) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const double mu = sums[c] / n;
  double var = sums[C + c] / n - mu * mu;
  if (var < 0.0) var = 0.0;
  const float is = (float)(1.0 / sqrt(var + (double)eps));
  const float av = gamma[c] * is;
  a[c] = av;
  b[c] = beta[c] - (float)mu * av;
  mean[c] = (float)mu;
  invstd[c] = is;
  if (running_mean) {
    const double unbiased = n > 1.0 ? var * n / (n - 1.0) : var;
    running_mean[c] = (1.0f - momentum) * running_mean[c] + momentum * (float)mu;
    running_var[c] = (1.0f - momentum) * running_var[c] + momentum * (float)unbiased;
  }
}

// ---- y = act(a_c z + b_c) [+ res]; optional per-(b,c) sums of y (SE squeeze / head pool) ----------
// ZT / YT: storage types of z / y (act_io.h; bf16 in the bf16-storage plan: the pool sums the values as STORED; ZT = bf16 with
// YT = float: the project conv's BatchNorm - z_p is stored in bf16, the block output it produces is an fp32 tensor)
template <int ACT, typename ZT = float, typename YT = ZT>
__global__ __launch_bounds__(256) void bn_act_fwd_kernel(const ZT* __restrict__ z, const float* __restrict__ a,
                                                         const float* __restrict__ b, const float* __restrict__ res,
                                                         YT* __restrict__ y, float* __restrict__ pool, int C, int S,
                                                         eat::bf16_t* __restrict__ y16 = nullptr) {
  // y16: optional bf16 COPY of an fp32 y (the block output of the bf16-storage plan: the next block's expand conv reads the
  // copy - bit-identical to reading y, the conv rounds its operand the same way - at half the operand traffic)
  __shared__ float s_red[16];
  const int plane = blockIdx.x, c = plane % C;
  const float av = a[c], bv = b[c];
  const size_t base = (size_t)plane * S;
  float ps = 0.f, dummy = 0.f;
  if ((S & 3) == 0) {
#pragma unroll 4
    for (int i = threadIdx.x * 4; i < S; i += blockDim.x * 4) {
      const float4 v = Io<ZT>::load4(z + base + i);
      float4 o = make_float4(eat::activate<ACT>(fmaf(av, v.x, bv)), eat::activate<ACT>(fmaf(av, v.y, bv)),
                             eat::activate<ACT>(fmaf(av, v.z, bv)), eat::activate<ACT>(fmaf(av, v.w, bv)));
      if (res) {
        const float4 r = *reinterpret_cast<const float4*>(res + base + i);
        o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
      }
      if constexpr (Io<YT>::kBf) { o.x = eat::bf_round(o.x); o.y = eat::bf_round(o.y); o.z = eat::bf_round(o.z); o.w = eat::bf_round(o.w); }
      if (y) Io<YT>::store4(y + base + i, o);
      if (y16) Io<eat::bf16_t>::store4(y16 + base + i, o);
      ps += (o.x + o.y) + (o.z + o.w);
    }
  } else {
    for (int i = threadIdx.x; i < S; i += blockDim.x) {
      float o = Io<YT>::rnd(eat::activate<ACT>(fmaf(av, Io<ZT>::load1(z + base + i), bv)) + (res ? res[base + i] : 0.0f));
      if (y) Io<YT>::store1(y + base + i, o);
      if (y16) Io<eat::bf16_t>::store1(y16 + base + i, o);
      ps += o;
    }
  }
  if (pool) {
    block_sum2(ps, dummy, s_red);
    if (threadIdx.x == 0) pool[plane] = ps;       // one block per plane: plain store, no atomics
  }
}

// g = (dy * gscale[b,c] + gadd[b,c]) * act'(a z + b);  xhat = (z - mean) * invstd
template <int ACT>
__device__ __forceinline__ float grad_pre(float dy, float zv, float av, float bv, float gs, float ga) {
  return fmaf(dy, gs, ga) * act_grad<ACT>(fmaf(av, zv, bv));
}

// ---- backward pass 1: per-channel sum g and sum g*xhat -------------------------------------------------
template <int ACT, typename ZT = float, typename DT = ZT>
__global__ __launch_bounds__(256) void bn_act_bwd_reduce_kernel(
    const DT* __restrict__ dy, const ZT* __restrict__ z, const float* __restrict__ a,
    const float* __restrict__ b, const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ gscale, const float* __restrict__ gadd, int C, int S, double* __restrict__ sums) {
  __shared__ float s_red[16];
  const int plane = blockIdx.x, c = plane % C;
  const float av = a[c], bv = b[c], mu = mean[c], is = invstd[c];
  const float gs = gscale ? gscale[plane] : 1.0f, ga = gadd ? gadd[plane] : 0.0f;
  const size_t base = (size_t)plane * S;
  float s1 = 0.f, s2 = 0.f;
  if ((S & 3) == 0) {
#pragma unroll 4
    for (int i = threadIdx.x * 4; i < S; i += blockDim.x * 4) {
      const float4 d = Io<DT>::load4(dy + base + i);
      const float4 v = Io<ZT>::load4(z + base + i);
      const float g0 = grad_pre<ACT>(d.x, v.x, av, bv, gs, ga), g1 = grad_pre<ACT>(d.y, v.y, av, bv, gs, ga);
      const float g2 = grad_pre<ACT>(d.z, v.z, av, bv, gs, ga), g3 = grad_pre<ACT>(d.w, v.w, av, bv, gs, ga);
      s1 += (g0 + g1) + (g2 + g3);
      s2 += (g0 * (v.x - mu) + g1 * (v.y - mu)) + (g2 * (v.z - mu) + g3 * (v.w - mu));
    }
  } else {
    for (int i = threadIdx.x; i < S; i += blockDim.x) {
      const float zv = Io<ZT>::load1(z + base + i);
      const float g = grad_pre<ACT>(Io<DT>::load1(dy + base + i), zv, av, bv, gs, ga);
      s1 += g;
      s2 += g * (zv - mu);
    }
  }
  s2 *= is;
  block_sum2(s1, s2, s_red);
  if (threadIdx.x == 0) {
    atomicAdd(sums + c, (double)s1);
    atomicAdd(sums + C + c, (double)s2);
  }
}

// small planes: one block per (channel, PPB samples), see bn_stats_multi_kernel
template <int ACT, typename ZT = float, typename DT = ZT>
__global__ __launch_bounds__(256) void bn_act_bwd_reduce_multi_kernel(
    const DT* __restrict__ dy, const ZT* __restrict__ z, const float* __restrict__ a,
    const float* __restrict__ b, const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ gscale, const float* __restrict__ gadd, int B, int C, int S4, int PPB,
    double* __restrict__ sums) {
  __shared__ float s_red[16];
  const int c = blockIdx.x, b0 = blockIdx.y * PPB;
  const int nb = (B - b0) < PPB ? (B - b0) : PPB;
  const float av = a[c], bv = b[c], mu = mean[c], is = invstd[c];
  float s1 = 0.f, s2 = 0.f;
  for (int e = threadIdx.x; e < nb * S4; e += 256) {
    const int bl = e / S4, i = e - bl * S4;
    const size_t plane = (size_t)(b0 + bl) * C + c;
    const float gs = gscale ? gscale[plane] : 1.0f, ga = gadd ? gadd[plane] : 0.0f;
    const float4 d = Io<DT>::load4(dy + plane * (4 * S4) + 4 * i);
    const float4 v = Io<ZT>::load4(z + plane * (4 * S4) + 4 * i);
    const float g0 = grad_pre<ACT>(d.x, v.x, av, bv, gs, ga), g1 = grad_pre<ACT>(d.y, v.y, av, bv, gs, ga);
    const float g2 = grad_pre<ACT>(d.z, v.z, av, bv, gs, ga), g3 = grad_pre<ACT>(d.w, v.w, av, bv, gs, ga);
    s1 += (g0 + g1) + (g2 + g3);
    s2 += (g0 * (v.x - mu) + g1 * (v.y - mu)) + (g2 * (v.z - mu) + g3 * (v.w - mu));
  }
  s2 *= is;
  block_sum2(s1, s2, s_red);
  if (threadIdx.x == 0) {
    atomicAdd(sums + c, (double)s1);
    atomicAdd(sums + C + c, (double)s2);
  }
}

// ---- backward pass 2: dz = a * (g - sum_g/N - xhat * sum_gx/N) ----------------------------------------------
// DT: storage type of dy AND dz (fp32; bf16: the expand BatchNorm of a DyMN block under the bf16-storage plan, g_e -> dz_e in place)
template <int ACT, typename ZT = float, typename DT = float>
__global__ __launch_bounds__(256) void bn_act_bwd_apply_kernel(
    const DT* __restrict__ dy, const ZT* __restrict__ z, const float* __restrict__ a,
    const float* __restrict__ b, const float* __restrict__ mean, const float* __restrict__ invstd,
    const float* __restrict__ gscale, const float* __restrict__ gadd, const double* __restrict__ sums,
    DT* __restrict__ dz, int C, int S, double n, eat::bf16_t* __restrict__ dz16 = nullptr) {
  // dz16: optional bf16 COPY of dz (what the data-gradient 1x1 conv of the bf16-storage plan reads: see bn_act_fwd_kernel)
  const int plane = blockIdx.x, c = plane % C;
  const float av = a[c], bv = b[c], mu = mean[c], is = invstd[c];
  const float m1 = (float)(sums[c] / n), m2 = (float)(sums[C + c] / n);
  const float gs = gscale ? gscale[plane] : 1.0f, ga = gadd ? gadd[plane] : 0.0f;
  const size_t base = (size_t)plane * S;
  auto f = [&](float d, float v) {
    const float g = grad_pre<ACT>(d, v, av, bv, gs, ga);
    return av * (g - m1 - (v - mu) * is * m2);
  };
  if ((S & 3) == 0) {
#pragma unroll 4
    for (int i = threadIdx.x * 4; i < S; i += blockDim.x * 4) {
      const float4 d = Io<DT>::load4(dy + base + i);
      const float4 v = Io<ZT>::load4(z + base + i);
      const float4 o = make_float4(f(d.x, v.x), f(d.y, v.y), f(d.z, v.z), f(d.w, v.w));
      Io<DT>::store4(dz + base + i, o);
      if (dz16) Io<eat::bf16_t>::store4(dz16 + base + i, o);
    }
  } else {
    for (int i = threadIdx.x; i < S; i += blockDim.x) {
      const float o = f(Io<DT>::load1(dy + base + i), Io<ZT>::load1(z + base + i));
      Io<DT>::store1(dz + base + i, o);
      if (dz16) Io<eat::bf16_t>::store1(dz16 + base + i, o);
    }
  }
}

// ---- out[b,c] = sum_s u[b,c,s] * v'[b,c,s], v' = v or act(a_c v + b_c) (SE: d scale) ---------------------------------
template <int ACT>
__global__ __launch_bounds__(256) void plane_dot_kernel(const float* __restrict__ u, const float* __restrict__ v,
                                                        const float* __restrict__ a, const float* __restrict__ b,
                                                        float* __restrict__ out, int C, int S) {
  __shared__ float s_red[16];
  const int plane = blockIdx.x, c = plane % C;
  const float av = a ? a[c] : 1.0f, bv = b ? b[c] : 0.0f;
  const size_t base = (size_t)plane * S;
  float s1 = 0.f, dummy = 0.f;
  for (int i = threadIdx.x; i < S; i += blockDim.x) {
    float t = v[base + i];
    if (a) t = eat::activate<ACT>(fmaf(av, t, bv));
    s1 += u[base + i] * t;
  }
  block_sum2(s1, dummy, s_red);
  if (threadIdx.x == 0) out[plane] = s1;
}
}  // namespace

#define EAT_PLANES_GRID(B, C) dim3((unsigned)((B) * (C)))

// samples per block of the small-plane reducers: ~2048 blocks; 0 = use the one-block-per-plane kernels
static int bn_multi_ppb(int B, int C, int S) {
  if ((S & 3) != 0 || S > 2048 || (long long)B * C <= 4096) return 0;
  long long ppb = ((long long)B * C + 2047) / 2048;
  return (int)(ppb > B ? B : ppb);
}

extern "C" int eat_bn_stats(const float* z, int B, int C, int S, double* sums, eat_stream_t stream) {
  eat::clear_stale_error();
  if (const int ppb = bn_multi_ppb(B, C, S)) {
    hipLaunchKernelGGL(bn_stats_multi_kernel, dim3(C, (B + ppb - 1) / ppb), dim3(256), 0, (hipStream_t)stream, z, B, C, S >> 2,
                       ppb, sums);
    return eat::check_launch("eat_bn_stats");
  }
  hipLaunchKernelGGL(bn_stats_kernel, EAT_PLANES_GRID(B, C), dim3(S >= 1024 ? 256 : 64), 0, (hipStream_t)stream, z, C, S,
                     sums);
  return eat::check_launch("eat_bn_stats");
}

extern "C" int eat_bn_finalize(const double* sums, const float* gamma, const float* beta, float* running_mean,
                               float* running_var, float momentum, float eps, double n, int C, float* a, float* b,
                               float* mean, float* invstd, eat_stream_t stream) {
  eat::clear_stale_error();
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 127) / 128), dim3(128), 0, (hipStream_t)stream, sums, gamma, beta,
                     running_mean, running_var, momentum, eps, n, C, a, b, mean, invstd);
  return eat::check_launch("eat_bn_finalize");
}

extern "C" int eat_bn_act_fwd(const float* z, const float* a, const float* b, const float* res, float* y,
                              float* pool, int B, int C, int S, int act, eat_stream_t stream) {
  eat::clear_stale_error();
  if (act < 0 || act > 2) return eat::fail(EAT_EINVAL, "eat_bn_act_fwd: bad act %d", act);
  const dim3 blk(S >= 1024 ? 256 : 64);
  EAT_DISPATCH_ACT(act, hipLaunchKernelGGL((bn_act_fwd_kernel<ACT>), EAT_PLANES_GRID(B, C), blk, 0, (hipStream_t)stream, z,
                                           a, b, res, y, pool, C, S));
  return eat::check_launch("eat_bn_act_fwd");
}

extern "C" int eat_bn_act_bwd_reduce(const float* dy, const float* z, const float* a, const float* b,
                                     const float* mean, const float* invstd, const float* gscale, const float* gadd,
                                     int B, int C, int S, int act, double* sums, eat_stream_t stream) {
  eat::clear_stale_error();
  if (act < 0 || act > 2) return eat::fail(EAT_EINVAL, "eat_bn_act_bwd_reduce: bad act %d", act);
  if (const int ppb = bn_multi_ppb(B, C, S)) {
    EAT_DISPATCH_ACT(act, hipLaunchKernelGGL((bn_act_bwd_reduce_multi_kernel<ACT>), dim3(C, (B + ppb - 1) / ppb), dim3(256), 0,
                                             (hipStream_t)stream, dy, z, a, b, mean, invstd, gscale, gadd, B, C, S >> 2, ppb, sums));
    return eat::check_launch("eat_bn_act_bwd_reduce");
  }
  const dim3 blk(S >= 1024 ? 256 : 64);
  EAT_DISPATCH_ACT(act, hipLaunchKernelGGL((bn_act_bwd_reduce_kernel<ACT>), EAT_PLANES_GRID(B, C), blk, 0,
                                           (hipStream_t)stream, dy, z, a, b, mean, invstd, gscale, gadd, C, S, sums));
  return eat::check_launch("eat_bn_act_bwd_reduce");
}

// ---- bf16 copy of a NARROW fp32 tensor of the bf16-storage plan (block input / project-BatchNorm gradient of the widest
// blocks): the 1x1 conv kernel rounds its fp32 operand to bf16 in any case (same RNE rounding: the conv results are
// bit-identical), but it stages a bf16 operand at half the L2 -> LDS traffic and with two LDS stages - on the 448 -> 2688
// expand conv at S = 504, B = 128 that is 324 -> 238 us for a 24 us copy.
namespace {
__global__ __launch_bounds__(256) void cast_b16_kernel(const float* __restrict__ x, eat::bf16_t* __restrict__ y, long long n8) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long long)gridDim.x * 256) {
    const float4 p = reinterpret_cast<const float4*>(x)[2 * i], q = reinterpret_cast<const float4*>(x)[2 * i + 1];
    uint4 o;
    o.x = eat::pack_bf2(p.x, p.y); o.y = eat::pack_bf2(p.z, p.w); o.z = eat::pack_bf2(q.x, q.y); o.w = eat::pack_bf2(q.z, q.w);
    reinterpret_cast<uint4*>(y)[i] = o;
  }
}
}  // namespace
extern "C" int eat_cast_b16(const float* x, void* y, long long n, eat_stream_t stream) {
  eat::clear_stale_error();
  if (!x || !y || n < 8 || (n & 7)) return eat::fail(EAT_EINVAL, "eat_cast_b16: n=%lld must be a positive multiple of 8", n);
  const long long n8 = n >> 3;
  const long long blocks = (n8 + 255) / 256;
  hipLaunchKernelGGL(cast_b16_kernel, dim3((unsigned)(blocks < 256 * 16 ? blocks : 256 * 16)), dim3(256), 0, (hipStream_t)stream,
                     x, reinterpret_cast<eat::bf16_t*>(y), n8);
  return eat::check_launch("eat_cast_b16");
}

// ---- the two stand-alone BatchNorm passes of the bf16-storage plan (act_io.h; BASELINE configs[2]): the depthwise output
// z_d and the gradient arriving at it are bf16 in HBM.  Same arithmetic as the fp32 entry points; y (or NULL) is written in
// bf16 and `pool` sums the ROUNDED values - what the project conv will read.  (S % 4 != 0: element-wise path.)
extern "C" int eat_bn_act_fwd_b16(const void* z, const float* a, const float* b, const float* res, void* y, int y_b16,
                                  void* y_copy16, float* pool, int B, int C, int S, int act, eat_stream_t stream) {
  eat::clear_stale_error();
  if (act < 0 || act > 2) return eat::fail(EAT_EINVAL, "eat_bn_act_fwd_b16: bad act %d", act);
  if (!z || B < 1 || C < 1 || S < 1) return eat::fail(EAT_EINVAL, "eat_bn_act_fwd_b16: bad shape");
  if ((res || y_copy16) && y_b16)
    return eat::fail(EAT_EINVAL, "eat_bn_act_fwd_b16: a residual / a bf16 copy goes with an fp32 output only");
  const dim3 blk(S >= 1024 ? 256 : 64);
  const eat::bf16_t* z16 = reinterpret_cast<const eat::bf16_t*>(z);
  if (y_b16)
    EAT_DISPATCH_ACT(act, hipLaunchKernelGGL((bn_act_fwd_kernel<ACT, eat::bf16_t>), EAT_PLANES_GRID(B, C), blk, 0, (hipStream_t)stream,
                                             z16, a, b, (const float*)nullptr, reinterpret_cast<eat::bf16_t*>(y), pool, C, S));
  else
    EAT_DISPATCH_ACT(act, hipLaunchKernelGGL((bn_act_fwd_kernel<ACT, eat::bf16_t, float>), EAT_PLANES_GRID(B, C), blk, 0,
                                             (hipStream_t)stream, z16, a, b, res, reinterpret_cast<float*>(y), pool, C, S,
                                             reinterpret_cast<eat::bf16_t*>(y_copy16)));
  return eat::check_launch("eat_bn_act_fwd_b16");
}

extern "C" int eat_bn_act_bwd_reduce_b16(const void* dy, int dy_b16, const void* z, const float* a, const float* b,
                                         const float* mean, const float* invstd, const float* gscale, const float* gadd, int B,
                                         int C, int S, int act, double* sums, eat_stream_t stream) {
  eat::clear_stale_error();
  if (act < 0 || act > 2) return eat::fail(EAT_EINVAL, "eat_bn_act_bwd_reduce_b16: bad act %d", act);
  if (!dy || !z || B < 1 || C < 1 || S < 1) return eat::fail(EAT_EINVAL, "eat_bn_act_bwd_reduce_b16: bad shape");
  const eat::bf16_t* z16 = reinterpret_cast<const eat::bf16_t*>(z);
  const int ppb = bn_multi_ppb(B, C, S);
  const dim3 blk(S >= 1024 ? 256 : 64);
#define EAT_RED16(DT_, dyp)                                                                                                  \
  do {                                                                                                                      \
    if (ppb) {                                                                                                              \
      EAT_DISPATCH_ACT(act, hipLaunchKernelGGL((bn_act_bwd_reduce_multi_kernel<ACT, eat::bf16_t, DT_>), dim3(C, (B + ppb - 1) / ppb), \
                                               dim3(256), 0, (hipStream_t)stream, dyp, z16, a, b, mean, invstd, gscale, gadd, B, C, \
                                               S >> 2, ppb, sums));                                                         \
    } else {                                                                                                                \
      EAT_DISPATCH_ACT(act, hipLaunchKernelGGL((bn_act_bwd_reduce_kernel<ACT, eat::bf16_t, DT_>), EAT_PLANES_GRID(B, C), blk, 0,   \
                                               (hipStream_t)stream, dyp, z16, a, b, mean, invstd, gscale, gadd, C, S, sums)); \
    }                                                                                                                       \
  } while (0)
  if (dy_b16) EAT_RED16(eat::bf16_t, reinterpret_cast<const eat::bf16_t*>(dy));
  else EAT_RED16(float, reinterpret_cast<const float*>(dy));
#undef EAT_RED16
  return eat::check_launch("eat_bn_act_bwd_reduce_b16");
}

// apply pass over a bf16-stored z (the project conv's output z_p in the bf16-storage plan): dy and dz are fp32
extern "C" int eat_bn_act_bwd_apply_b16(const float* dy, const void* z, const float* a, const float* b, const float* mean,
                                        const float* invstd, const float* gscale, const float* gadd, const double* sums,
                                        float* dz, void* dz_copy16, int B, int C, int S, int act, eat_stream_t stream) {
  eat::clear_stale_error();
  if (act < 0 || act > 2) return eat::fail(EAT_EINVAL, "eat_bn_act_bwd_apply_b16: bad act %d", act);
  if (!dy || !z || !dz || B < 1 || C < 1 || S < 1) return eat::fail(EAT_EINVAL, "eat_bn_act_bwd_apply_b16: bad shape");
  const dim3 blk(S >= 1024 ? 256 : 64);
  const double n = (double)B * S;
  EAT_DISPATCH_ACT(act, hipLaunchKernelGGL((bn_act_bwd_apply_kernel<ACT, eat::bf16_t>), EAT_PLANES_GRID(B, C), blk, 0,
                                           (hipStream_t)stream, dy, reinterpret_cast<const eat::bf16_t*>(z), a, b, mean, invstd,
                                           gscale, gadd, sums, dz, C, S, n, reinterpret_cast<eat::bf16_t*>(dz_copy16)));
  return eat::check_launch("eat_bn_act_bwd_apply_b16");
}

// ... with dy AND dz in bf16 too (dz may alias dy): the expand BatchNorm of a DyMN block under the bf16-storage plan - g_e, z_e
// and dz_e are all wide tensors (models/dymn/dy_block.py:313-318 backward)
extern "C" int eat_bn_bwd_apply_b16(const void* dy, const void* z, const float* a, const float* b, const float* mean,
                                    const float* invstd, const double* sums, void* dz, int B, int C, int S, int act,
                                    eat_stream_t stream) {
  eat::clear_stale_error();
  if (act < 0 || act > 2) return eat::fail(EAT_EINVAL, "eat_bn_bwd_apply_b16: bad act %d", act);
  if (!dy || !z || !dz || !sums || B < 1 || C < 1 || S < 1) return eat::fail(EAT_EINVAL, "eat_bn_bwd_apply_b16: bad arguments");
  const dim3 blk(S >= 1024 ? 256 : 64);
  const double n = (double)B * S;
  EAT_DISPATCH_ACT(act, hipLaunchKernelGGL((bn_act_bwd_apply_kernel<ACT, eat::bf16_t, eat::bf16_t>), EAT_PLANES_GRID(B, C), blk, 0,
                                           (hipStream_t)stream, reinterpret_cast<const eat::bf16_t*>(dy),
                                           reinterpret_cast<const eat::bf16_t*>(z), a, b, mean, invstd, (const float*)nullptr,
                                           (const float*)nullptr, sums, reinterpret_cast<eat::bf16_t*>(dz), C, S, n,
                                           (eat::bf16_t*)nullptr));
  return eat::check_launch("eat_bn_bwd_apply_b16");
}

extern "C" int eat_bn_act_bwd_apply(const float* dy, const float* z, const float* a, const float* b,
                                    const float* mean, const float* invstd, const float* gscale, const float* gadd,
                                    const double* sums, float* dz, int B, int C, int S, int act, eat_stream_t stream) {
  eat::clear_stale_error();
  if (act < 0 || act > 2) return eat::fail(EAT_EINVAL, "eat_bn_act_bwd_apply: bad act %d", act);
  const dim3 blk(S >= 1024 ? 256 : 64);
  const double n = (double)B * S;
  EAT_DISPATCH_ACT(act, hipLaunchKernelGGL((bn_act_bwd_apply_kernel<ACT>), EAT_PLANES_GRID(B, C), blk, 0,
                                           (hipStream_t)stream, dy, z, a, b, mean, invstd, gscale, gadd, sums, dz, C, S, n));
  return eat::check_launch("eat_bn_act_bwd_apply");
}

extern "C" int eat_plane_dot(const float* u, const float* v, const float* a, const float* b, float* out, int B,
                             int C, int S, int act, eat_stream_t stream) {
  eat::clear_stale_error();
  if (act < 0 || act > 2) return eat::fail(EAT_EINVAL, "eat_plane_dot: bad act %d", act);
  const dim3 blk(S >= 1024 ? 256 : 64);
  EAT_DISPATCH_ACT(act, hipLaunchKernelGGL((plane_dot_kernel<ACT>), EAT_PLANES_GRID(B, C), blk, 0, (hipStream_t)stream, u,
                                           v, a, b, out, C, S));
  return eat::check_launch("eat_plane_dot");
}
