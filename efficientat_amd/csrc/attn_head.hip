// PSLA multi-head attention-pooling head (models/mn/attention_pooling.py:9-56), forward and backward, around the 1x1
// projection GEMM of conv_pw*.hip.  Nothing is transposed: the head stays in the (sample, channel, position) layout of the
// 1x1 kernels -
//   y (B, C, F, T) last feature map -> xm (B, C, Tp) mean over frequency -> p (B, N, Tp) = W xm, N = 2 H K,
//   row n = (j H + h) K + k of W (j = 0 attention logit, 1 value)   [the reference's reshape(b, t, 2, H, K)]
// with a row pitch Tp >= T: the MFMA kernels move 16 bytes per lane and want rows of a multiple of 4 floats.  Pad columns
// [T, Tp) are written as zeros by whoever produces a tensor (so the GEMMs that contract over positions stay exact) and are
// never read by the pooling kernels.
//
// Pooling geometry.  One (b, k) pair is owned by a group of L = min(64, pow2 >= Tp) consecutive lanes, 64 / L pairs per
// wavefront; the lanes run along t, the pair walks its H heads.  Neighbouring pairs are neighbouring rows of p, so a
// wavefront's loads are contiguous runs of rows (T = Tp = 32: two 128-byte rows per load instruction); every access is a
// 4-byte one, no row alignment is assumed.  Sums over t are xor-shuffle trees inside the group (all lanes end with the total),
// longer rows first add up t = j, j + L, ... in each lane.  Every output element is produced by one group in a fixed order:
// out, o, s, dp are bit-identical from run to run.  The two long reductions of the backward (dbias over b and t, dhead_w
// over b and k) go through per-sample partials (fp32, <= T resp. K terms) and a finish in fp64, in a fixed order: no atomics.
#include <cstdint>

#include "eat_common.h"
#include "loss_terms.h"
#include "../../include/eat_attn.h"

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ float group_sum(float v, int L) {      // L: power of two <= 64, group = L aligned lanes
  for (int o = L >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

int group_lanes(int Tp) {
  int L = 1;
  while (L < Tp && L < 64) L <<= 1;
  return L;
}

// ------------------------------------------------------------------------------------------------ frequency mean
// one thread per (b c, t) of xm, t in [0, Tp)
__global__ __launch_bounds__(kThreads) void freq_mean_fwd_kernel(const float* __restrict__ y, float* __restrict__ xm, long long BC,
                                                                 int F, int T, int Tp, float inv_f) {
  const long long n = BC * Tp;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const long long bc = i / Tp;
    const int t = (int)(i - bc * Tp);
    float v = 0.0f;
    if (t < T) {
      const float* p = y + bc * ((long long)F * T) + t;
      float acc = 0.0f;
#pragma unroll 4
      for (int f = 0; f < F; ++f) acc += p[(long long)f * T];
      v = acc * inv_f;
    }
    xm[i] = v;
  }
}

// one thread per (b c, t) of dxm, t in [0, T): its value goes to the F rows of the plane (a wavefront stores runs of rows)
__global__ __launch_bounds__(kThreads) void freq_mean_bwd_kernel(const float* __restrict__ dxm, float* __restrict__ dy, long long BC,
                                                                 int F, int T, int Tp, float inv_f) {
  const long long n = BC * T;
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
    const long long bc = i / T;
    const int t = (int)(i - bc * T);
    const float v = dxm[bc * Tp + t] * inv_f;
    float* p = dy + bc * ((long long)F * T) + t;
    for (int f = 0; f < F; ++f) p[(long long)f * T] = v;
  }
}

// ------------------------------------------------------------------------------------------------ pooling, forward
__global__ __launch_bounds__(kThreads) void attn_pool_fwd_kernel(const float* __restrict__ p, const float* __restrict__ bias,
                                                                 const float* __restrict__ head_w, float lo, float hi,
                                                                 float* __restrict__ out, float* __restrict__ o_out,
                                                                 float* __restrict__ s_out, int B, int H, int K, int T, int Tp,
                                                                 int L) {
  const int per_block = kThreads / L;
  const long long item = (long long)blockIdx.x * per_block + threadIdx.x / L;     // = b K + k
  const int j = threadIdx.x & (L - 1);
  const long long items = (long long)B * K;
  const bool live = item < items;                  // (dead groups run along with b = k = 0 loads masked: shuffles stay whole)
  const long long b = live ? item / K : 0;
  const int k = live ? (int)(item - b * K) : 0;
  const long long N = 2LL * H * K;
  const float* pb = p + b * N * Tp;
  float acc = 0.0f;
  for (int h = 0; h < H; ++h) {
    const long long na = (long long)h * K + k, nv = ((long long)H + h) * K + k;
    const float ba = bias ? bias[na] : 0.0f, bv = bias ? bias[nv] : 0.0f;
    const float* ra = pb + na * Tp;
    const float* rv = pb + nv * Tp;
    float s = 0.0f, m = 0.0f;
    for (int t = j; t < T; t += L) {
      if (live) {
        const float a = fminf(fmaxf(eat::sigmoid(ra[t] + ba), lo), hi);
        s += a;
        m += a * (rv[t] + bv);
      }
    }
    s = group_sum(s, L);
    m = group_sum(m, L);
    const float o = m / s;
    if (live && j == 0) {
      const long long q = (b * H + h) * K + k;
      if (o_out) o_out[q] = o;
      if (s_out) s_out[q] = s;
    }
    acc += head_w[h] * o;
  }
  if (live && j == 0) out[item] = acc;
}

// ------------------------------------------------------------------------------------------------ pooling, backward
// dp rows of one (b, k) pair for every head, and the per-sample row sums of dp (-> dbias) into part (B, N + H).
// Items past B K write the zero rows [N, Np) of a sample (Np > N: a projection padded to a multiple of 4 rows).
__global__ __launch_bounds__(kThreads) void attn_pool_bwd_kernel(const float* __restrict__ g, const float* __restrict__ p,
                                                                 const float* __restrict__ bias, const float* __restrict__ head_w,
                                                                 float lo, float hi, const float* __restrict__ o_in,
                                                                 const float* __restrict__ s_in, float* __restrict__ dp,
                                                                 float* __restrict__ part, int B, int H, int K, int T, int Tp,
                                                                 int Np, int L) {
  const int per_block = kThreads / L;
  const long long item = (long long)blockIdx.x * per_block + threadIdx.x / L;
  const int j = threadIdx.x & (L - 1);
  const long long N = 2LL * H * K, items = (long long)B * K;
  if (item >= items) {
    const long long z = item - items;              // zero row r of sample b
    if (z < (long long)B * (Np - N)) {
      const long long b = z / (Np - N), r = z - b * (Np - N);
      float* row = dp + (b * Np + N + r) * Tp;
      for (int t = j; t < Tp; t += L) row[t] = 0.0f;
    }
    return;                                        // whole groups leave together: L divides 64
  }
  const long long b = item / K;
  const int k = (int)(item - b * K);
  const float* pb = p + b * N * Tp;
  float* db = dp + b * (long long)Np * Tp;
  const float gk = g[item];
  for (int h = 0; h < H; ++h) {
    const long long na = (long long)h * K + k, nv = ((long long)H + h) * K + k;
    const float ba = bias ? bias[na] : 0.0f, bv = bias ? bias[nv] : 0.0f;
    const long long q = (b * H + h) * K + k;
    const float o = o_in[q], inv_s = 1.0f / s_in[q];
    const float d_o = gk * head_w[h];
    const float* ra = pb + na * Tp;
    const float* rv = pb + nv * Tp;
    float* da_row = db + na * Tp;
    float* dv_row = db + nv * Tp;
    float sa = 0.0f, sv = 0.0f;
    for (int t = j; t < Tp; t += L) {
      float dqa = 0.0f, dqv = 0.0f;
      if (t < T) {
        const float sg = eat::sigmoid(ra[t] + ba);
        const float a = fminf(fmaxf(sg, lo), hi);
        dqv = d_o * a * inv_s;
        const float da = d_o * ((rv[t] + bv) - o) * inv_s;
        dqa = (sg >= lo && sg <= hi) ? da * sg * (1.0f - sg) : 0.0f;
      }
      da_row[t] = dqa;
      dv_row[t] = dqv;
      sa += dqa;
      sv += dqv;
    }
    sa = group_sum(sa, L);
    sv = group_sum(sv, L);
    if (j == 0) {
      part[b * (N + H) + na] = sa;
      part[b * (N + H) + nv] = sv;
    }
  }
}

// part[b, N + h] = sum_k g[b, k] o[b, h, k]: one wavefront per (b, h)
__global__ __launch_bounds__(kThreads) void attn_pool_hw_part_kernel(const float* __restrict__ g, const float* __restrict__ o_in,
                                                                     float* __restrict__ part, int B, int H, int K) {
  const long long w = (long long)blockIdx.x * (kThreads / eat::kWave) + (threadIdx.x >> 6);   // = b H + h
  const int lane = threadIdx.x & 63;
  if (w >= (long long)B * H) return;               // wave-uniform
  const long long b = w / H;
  const int h = (int)(w - b * H);
  const float* gb = g + b * K;
  const float* ob = o_in + w * K;
  float acc = 0.0f;
  for (int k = lane; k < K; k += eat::kWave) acc += gb[k] * ob[k];
  acc = eat::wave_sum(acc);
  if (lane == 0) part[b * (2LL * H * K + H) + 2LL * H * K + h] = acc;
}

// column sums over b of part (B, M), M = N + H, in fp64: columns [0, N) -> dbias (if any), [N, M) -> dhead_w.
// 32 columns x 8 row groups per block; the 8 partial sums of a column are added in a fixed order.
__global__ __launch_bounds__(kThreads) void attn_pool_finish_kernel(const float* __restrict__ part, float* __restrict__ dbias,
                                                                    float* __restrict__ dhead_w, int B, long long N, int H) {
  __shared__ double red[8][32];
  const int c = threadIdx.x & 31, r = threadIdx.x >> 5;
  const long long M = N + H, col = (long long)blockIdx.x * 32 + c;
  double acc = 0.0;
  if (col < M) {
#pragma unroll 4
    for (int b = r; b < B; b += 8) acc += (double)part[b * M + col];
  }
  red[r][c] = acc;
  __syncthreads();
  if (r == 0 && col < M) {
    double v = red[0][c];
    for (int q = 1; q < 8; ++q) v += red[q][c];
    if (col < N) {
      if (dbias) dbias[col] = (float)v;
    } else {
      dhead_w[col - N] = (float)v;
    }
  }
}

int grid_for(long long n_threads, const char* who, unsigned* blocks) {
  const long long nb = (n_threads + kThreads - 1) / kThreads;
  if (nb > 0x7fffffffLL) return eat::fail(EAT_EINVAL, "%s: %lld blocks exceed the grid limit of 2147483647: chunk the call over B", who, nb);
  *blocks = (unsigned)nb;
  return EAT_OK;
}

int check_pool(const char* who, int B, int H, int K, int T, int Tp, double eps) {
  if (B < 1 || H < 1 || K < 1 || T < 1) return eat::fail(EAT_EINVAL, "%s: need B, H, K, T >= 1 (got %d, %d, %d, %d)", who, B, H, K, T);
  if (Tp < T) return eat::fail(EAT_EINVAL, "%s: row pitch Tp=%d is shorter than T=%d", who, Tp, T);
  if (2LL * H * K > 0x7fffffffLL) return eat::fail(EAT_EINVAL, "%s: 2 H K = %lld rows exceed the 32-bit row count", who, 2LL * H * K);
  if (!(eps >= 0.0 && eps < 0.5)) return eat::fail(EAT_EINVAL, "%s: eps=%g lies outside [0, 0.5)", who, eps);
  return EAT_OK;
}

}  // namespace

extern "C" int eat_freq_mean_fwd(const float* y, float* xm, int B, int C, int F, int T, int Tp, eat_stream_t stream) {
  eat::clear_stale_error();
  if (!y || !xm) return eat::fail(EAT_EINVAL, "eat_freq_mean_fwd: missing operand");
  if (B < 1 || C < 1 || F < 1 || T < 1) return eat::fail(EAT_EINVAL, "eat_freq_mean_fwd: need B, C, F, T >= 1 (got %d, %d, %d, %d)", B, C, F, T);
  if (Tp < T) return eat::fail(EAT_EINVAL, "eat_freq_mean_fwd: row pitch Tp=%d is shorter than T=%d", Tp, T);
  const long long BC = (long long)B * C;
  long long nb = (BC * Tp + kThreads - 1) / kThreads;
  if (nb > (1 << 20)) nb = 1 << 20;                 // grid-stride beyond
  hipLaunchKernelGGL(freq_mean_fwd_kernel, dim3((unsigned)nb), dim3(kThreads), 0, (hipStream_t)stream, y, xm, BC, F, T, Tp,
                     1.0f / (float)F);
  return eat::check_launch("eat_freq_mean_fwd");
}

extern "C" int eat_freq_mean_bwd(const float* dxm, float* dy, int B, int C, int F, int T, int Tp, eat_stream_t stream) {
  eat::clear_stale_error();
  if (!dxm || !dy) return eat::fail(EAT_EINVAL, "eat_freq_mean_bwd: missing operand");
  if (B < 1 || C < 1 || F < 1 || T < 1) return eat::fail(EAT_EINVAL, "eat_freq_mean_bwd: need B, C, F, T >= 1 (got %d, %d, %d, %d)", B, C, F, T);
  if (Tp < T) return eat::fail(EAT_EINVAL, "eat_freq_mean_bwd: row pitch Tp=%d is shorter than T=%d", Tp, T);
  const long long BC = (long long)B * C;
  long long nb = (BC * T + kThreads - 1) / kThreads;
  if (nb > (1 << 20)) nb = 1 << 20;
  hipLaunchKernelGGL(freq_mean_bwd_kernel, dim3((unsigned)nb), dim3(kThreads), 0, (hipStream_t)stream, dxm, dy, BC, F, T, Tp,
                     1.0f / (float)F);
  return eat::check_launch("eat_freq_mean_bwd");
}

extern "C" int eat_attn_pool_fwd(const float* p, const float* bias, const float* head_w, double eps, float* out, float* o,
                                 float* s, int B, int H, int K, int T, int Tp, eat_stream_t stream) {
  eat::clear_stale_error();
  if (!p || !head_w || !out) return eat::fail(EAT_EINVAL, "eat_attn_pool_fwd: missing operand (p, head_w and out are required)");
  if (int rc = check_pool("eat_attn_pool_fwd", B, H, K, T, Tp, eps)) return rc;
  const int L = group_lanes(Tp);
  unsigned blocks;
  if (int rc = grid_for((long long)B * K * L, "eat_attn_pool_fwd", &blocks)) return rc;
  hipLaunchKernelGGL(attn_pool_fwd_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, p, bias, head_w, (float)eps,
                     (float)(1.0 - eps), out, o, s, B, H, K, T, Tp, L);
  return eat::check_launch("eat_attn_pool_fwd");
}

extern "C" int eat_attn_pool_bwd(const float* g, const float* p, const float* bias, const float* head_w, double eps,
                                 const float* o, const float* s, float* dp, float* dbias, float* dhead_w, float* ws, int B, int H,
                                 int K, int T, int Tp, int Np, eat_stream_t stream) {
  eat::clear_stale_error();
  if (!g || !p || !head_w || !o || !s || !dp || !dhead_w || !ws)
    return eat::fail(EAT_EINVAL, "eat_attn_pool_bwd: missing operand (only bias and dbias are optional)");
  if (int rc = check_pool("eat_attn_pool_bwd", B, H, K, T, Tp, eps)) return rc;
  const long long N = 2LL * H * K;
  if (Np < N) return eat::fail(EAT_EINVAL, "eat_attn_pool_bwd: dp holds Np=%d rows per sample, fewer than 2 H K = %lld", Np, N);
  const int L = group_lanes(Tp);
  unsigned blocks, blocks_hw;
  if (int rc = grid_for(((long long)B * K + (long long)B * (Np - N)) * L, "eat_attn_pool_bwd", &blocks)) return rc;
  if (int rc = grid_for((long long)B * H * eat::kWave, "eat_attn_pool_bwd", &blocks_hw)) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(attn_pool_bwd_kernel, dim3(blocks), dim3(kThreads), 0, st, g, p, bias, head_w, (float)eps, (float)(1.0 - eps),
                     o, s, dp, ws, B, H, K, T, Tp, Np, L);
  hipLaunchKernelGGL(attn_pool_hw_part_kernel, dim3(blocks_hw), dim3(kThreads), 0, st, g, o, ws, B, H, K);
  hipLaunchKernelGGL(attn_pool_finish_kernel, dim3((unsigned)((N + H + 31) / 32)), dim3(kThreads), 0, st, ws, dbias, dhead_w, B, N, H);
  return eat::check_launch("eat_attn_pool_bwd");
}
