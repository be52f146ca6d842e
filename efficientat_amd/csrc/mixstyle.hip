// Frequency-wise MixStyle of ex_dcase20.py:104-107 (helpers/utils.py `mixstyle`) on the device: the augmentation that sits
// between the log-mel and the network of the DCASE20 fine-tuning step.
//   eat_freq_mixstyle   per (b, f) row of x (B, C, F, T): mean and unbiased variance over (c, t), then
//                       out = (x - mu) / sig * (lam sig + (1 - lam) sig[perm]) + (lam mu + (1 - lam) mu[perm])
// Two launches: the row statistics (one wave per (b, f) row, the row held in registers between the two passes), then the
// apply (one block per (b, c, f) row of T values, 16-byte stores).  A device flag switches the whole thing to a copy, so that
// a captured step can follow the reference's host coin flip without being captured again.
#include "eat_common.h"
#include "loss_terms.h"
#include "reduce.h"

namespace {

constexpr int kMsRowsPerBlock = 4;     // one wave per (b, f) row
constexpr int kMsReg = 16;             // C T <= 64 * kMsReg: the row stays in registers between the passes

// stats[(b F + f) 2] = {mu, sig} of row (b, f): n = C T values, C segments of T contiguous floats.  Lane l takes the values
// l, l + 64, ... of the row in order, sums them in fp64, then a fixed butterfly: mu = sum / n; the second pass sums
// (x - mu)^2 around that fp64 mean (never E[x^2] - E[x]^2), var = that / (n - 1), sig = sqrt(var + eps).
// KR > 0: the row is read once into registers (n <= 64 KR); KR == 0 re-reads it.
template <int KR>
__global__ __launch_bounds__(256) void mixstyle_stats_kernel(const float* __restrict__ x, const int* __restrict__ apply,
                                                             float* __restrict__ stats, int B, int C, int F, int T,
                                                             float eps) {
  if (apply != nullptr && *apply == 0) return;                     // not applied: the workspace keeps what it held
  const int row = blockIdx.x * kMsRowsPerBlock + (threadIdx.x >> 6);
  if (row >= B * F) return;
  const int lane = threadIdx.x & 63;
  const int b = row / F, f = row - b * F;
  const int n = C * T;
  const size_t seg = (size_t)F * T;                                // from channel c to c + 1 of the same (b, f)
  const float* xr = x + ((size_t)b * C * F + f) * T;
  auto at = [&](int j) -> float {
    if (C == 1) return xr[j];
    const int c = j / T;
    return xr[c * seg + (size_t)(j - c * T)];
  };
  float v[KR > 0 ? KR : 1];
  double s = 0.0;
  if constexpr (KR > 0) {
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int j = lane + 64 * k;
      v[k] = j < n ? at(j) : 0.0f;
    }
#pragma unroll
    for (int k = 0; k < KR; ++k)
      if (lane + 64 * k < n) s += (double)v[k];
  } else {
    for (int j = lane; j < n; j += 64) s += (double)at(j);
  }
  const double mu = eat::wave_sum_d(s) / (double)n;
  double q = 0.0;
  if constexpr (KR > 0) {
#pragma unroll
    for (int k = 0; k < KR; ++k)
      if (lane + 64 * k < n) {
        const double d = (double)v[k] - mu;
        q += d * d;
      }
  } else {
    for (int j = lane; j < n; j += 64) {
      const double d = (double)at(j) - mu;
      q += d * d;
    }
  }
  const double var = eat::wave_sum_d(q) / (double)(n - 1);
  if (lane == 0) {
    stats[2 * (size_t)row] = (float)mu;
    stats[2 * (size_t)row + 1] = (float)sqrt(var + (double)eps);
  }
}

// Block r writes out row r = (b, c, f) (T values).  The row's three coefficients come from the fp32 statistics of rows
// (b, f) and (perm[b], f), combined in fp64; every element is then one fp64 multiply-add rounded once to fp32.  4 outputs per
// thread and trip, one 16-byte store where the row position is 16-byte aligned (the first `head` and the last `tail` < 4
// values of a row are scalar stores); x is read 16 bytes at a time when it is aligned like out, else value by value.
__global__ __launch_bounds__(256) void mixstyle_apply_kernel(const float* __restrict__ x, const int* __restrict__ perm,
                                                             const float* __restrict__ lam, const int* __restrict__ apply,
                                                             const float* __restrict__ stats, float* __restrict__ out, int B,
                                                             int C, int F, int T, int xvec) {
  const size_t row = blockIdx.x;
  const int bc = (int)(row / (size_t)F);
  const int f = (int)(row - (size_t)bc * F);
  const int b = bc / C;
  const float* xr = x + row * T;
  float* o = out + row * T;
  const bool on = apply == nullptr || *apply != 0;
  double a = 1.0, m0 = 0.0, m1 = 0.0;
  if (on) {
    const eat::MixRow mr = eat::mix_row(perm, lam, b, B);         // (the wrapper validates; never read outside stats)
    const int pb = mr.pb;
    const double l = mr.lam;
    const float* sa = stats + 2 * ((size_t)b * F + f);
    const float* sp = stats + 2 * ((size_t)pb * F + f);
    const double mu = (double)sa[0], sig = (double)sa[1];
    a = (l * sig + (1.0 - l) * (double)sp[1]) / sig;
    m0 = mu;
    m1 = l * mu + (1.0 - l) * (double)sp[0];
  }
  auto val = [&](float v) -> float { return on ? (float)(((double)v - m0) * a + m1) : v; };

  const int head = min((int)((4 - (((uintptr_t)o >> 2) & 3)) & 3), T);
  const int nv = (T - head) >> 2;
  const int tail0 = head + 4 * nv;
  for (int i = threadIdx.x; i < nv; i += blockDim.x) {
    const int t = head + 4 * i;
    float4 u;
    if (xvec)
      u = *reinterpret_cast<const float4*>(xr + t);
    else
      u = make_float4(xr[t], xr[t + 1], xr[t + 2], xr[t + 3]);
    *reinterpret_cast<float4*>(o + t) = make_float4(val(u.x), val(u.y), val(u.z), val(u.w));
  }
  if (threadIdx.x < 8) {
    const int t = threadIdx.x < 4 ? threadIdx.x : tail0 + threadIdx.x - 4;
    if ((threadIdx.x < 4 && t < head) || (threadIdx.x >= 4 && t < T)) o[t] = val(xr[t]);
  }
}

}  // namespace

extern "C" int eat_freq_mixstyle(const float* x, const int* perm, const float* lam, const int* apply, float* out, float* stats,
                                 int B, int C, int F, int T, float eps, eat_stream_t stream) {
  eat::clear_stale_error();
  if (B < 1 || C < 1 || F < 1 || T < 1 || (long long)C * T < 2 || (long long)B * C * F * T > 0x7fffffffLL)
    return eat::fail(EAT_EINVAL, "eat_freq_mixstyle: bad shape (B = %d, C = %d, F = %d, T = %d)", B, C, F, T);
  if (!x || !perm || !lam || !out || !stats) return eat::fail(EAT_EINVAL, "eat_freq_mixstyle: a required pointer is NULL");
  if (out == x) return eat::fail(EAT_EINVAL, "eat_freq_mixstyle: out must not be x");
  hipStream_t s = (hipStream_t)stream;
  const unsigned sblocks = (unsigned)(((long long)B * F + kMsRowsPerBlock - 1) / kMsRowsPerBlock);
  if ((long long)C * T <= 64 * kMsReg)
    hipLaunchKernelGGL(mixstyle_stats_kernel<kMsReg>, dim3(sblocks), dim3(256), 0, s, x, apply, stats, B, C, F, T, eps);
  else
    hipLaunchKernelGGL(mixstyle_stats_kernel<0>, dim3(sblocks), dim3(256), 0, s, x, apply, stats, B, C, F, T, eps);
  // x and out are float arrays: congruent modulo 16 bytes means every 16-byte position of an out row is one of x too
  const int xvec = (((uintptr_t)x ^ (uintptr_t)out) & 15) == 0;
  const int nv = T / 4;
  const int threads = nv <= 64 ? 64 : nv <= 128 ? 128 : 256;
  hipLaunchKernelGGL(mixstyle_apply_kernel, dim3((unsigned)((long long)B * C * F)), dim3(threads), 0, s, x, perm, lam, apply,
                     stats, out, B, C, F, T, xvec);
  return eat::check_launch("eat_freq_mixstyle");
}
