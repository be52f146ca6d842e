// Fine-tuning glue of ex_esc50.py on the device: the single-label loss and the waveform augmentation of the training batch.
//   eat_softmax_ce_fwd_bwd  soft-target softmax cross-entropy with the mix-up of the targets folded in, its gradient w.r.t.
//                           the logits, the per-row loss and the per-row argmax in one pass over the (B, C) logits
//                           (ex_esc50.py:102-118 training, :154-178 evaluation)
//   eat_wave_augment        gain + roll + wave-mix of clips gathered from a device-resident bank (datasets/esc50.py gain and
//                           pad, datasets/helpers/audiodatasets.py roll, MixupDataset), and the matching target rows
// and the multi-label, partially observed variant of ex_openmic.py:
//   eat_masked_bce_fwd_bwd  BCE-with-logits times the "this label was annotated" mask, the mix-up of the binarized labels
//                           folded in, its gradient, the per-row loss and sigmoid(z) in one pass (ex_openmic.py:102-121, :160-187)
//   eat_openmic_targets     the label rule of OpenMIC's MixupDataset (datasets/openmic.py:74-95) for the rows of a wave-mixed batch
#include "eat_common.h"
#include "loss_terms.h"
#include "reduce.h"

namespace {

constexpr int kCeRowsPerBlock = 4;     // one wave per row
constexpr int kCeReg = 4;              // C <= 64 * kCeReg: the row stays in registers between the passes

using eat::wave_sum_d;

// numpy argmax order: a NaN beats every number (first NaN wins), otherwise the larger value, ties to the lower index.  A total
// order, so the xor butterfly leaves the same (value, index) in every lane.
__device__ __forceinline__ bool argmax_before(float va, int ia, float vb, int ib) {
  const bool na = va != va, nb = vb != vb;
  if (na || nb) return na && (!nb || ia < ib);
  return va > vb || (va == vb && ia < ib);
}

struct CeRow {
  double ce;      // sum_c t_c (lse - z_c)
  double lse;
  double s;       // sum_c t_c
  int amax;
};

// target element of row b: t = lam y_b + (1 - lam) y_perm[b], or y_b without mix-up
__device__ __forceinline__ double ce_target(const float* __restrict__ y, int C, int b, int pb, double l, int c) {
  const double ya = (double)y[(size_t)b * C + c];
  return pb < 0 ? ya : l * ya + (1.0 - l) * (double)y[(size_t)pb * C + c];
}

// One row by one wave.  KR > 0: the row's logits and targets are read once into registers (C <= 64 KR); KR == 0 re-reads them
// per pass.  dz (if not NULL) receives (S softmax(z) - t) / B.
template <int KR>
__device__ CeRow ce_row(const float* __restrict__ z, const float* __restrict__ y, const int* __restrict__ perm,
                        const float* __restrict__ lam, int B, int C, int b, float* __restrict__ dz) {
  const int lane = threadIdx.x & 63;
  const eat::MixRow m = eat::mix_row(perm, lam, b, B);
  const int pb = m.mixed ? m.pb : -1;              // (-1: no mix-up)
  const double l = m.lam;
  const float* zr = z + (size_t)b * C;
  float zv[KR > 0 ? KR : 1];
  double tv[KR > 0 ? KR : 1];
  float bv = -__builtin_inff();
  int bi = 0x7fffffff;
  double s = 0.0, tz = 0.0;
  if constexpr (KR > 0) {
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int c = lane + 64 * k;
      zv[k] = c < C ? zr[c] : 0.0f;
      tv[k] = c < C ? ce_target(y, C, b, pb, l, c) : 0.0;
    }
#pragma unroll
    for (int k = 0; k < KR; ++k) {
      const int c = lane + 64 * k;
      if (c < C) {
        if (argmax_before(zv[k], c, bv, bi)) bv = zv[k], bi = c;
        s += tv[k];
        tz += tv[k] * (double)zv[k];
      }
    }
  } else {
    for (int c = lane; c < C; c += 64) {
      const float v = zr[c];
      const double t = ce_target(y, C, b, pb, l, c);
      if (argmax_before(v, c, bv, bi)) bv = v, bi = c;
      s += t;
      tz += t * (double)v;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (argmax_before(ov, oi, bv, bi)) bv = ov, bi = oi;
  }
  s = wave_sum_d(s);
  tz = wave_sum_d(tz);
  const double mx = (double)bv;                    // NaN row: NaN loss and gradient, as torch
  double se = 0.0;
  if constexpr (KR > 0) {
#pragma unroll
    for (int k = 0; k < KR; ++k)
      if (lane + 64 * k < C) se += exp((double)zv[k] - mx);
  } else {
    for (int c = lane; c < C; c += 64) se += exp((double)zr[c] - mx);
  }
  const double lse = mx + log(wave_sum_d(se));
  if (dz != nullptr) {
    float* dr = dz + (size_t)b * C;
    const double inv_b = 1.0 / (double)B;
    if constexpr (KR > 0) {
#pragma unroll
      for (int k = 0; k < KR; ++k) {
        const int c = lane + 64 * k;
        if (c < C) dr[c] = (float)((s * exp((double)zv[k] - lse) - tv[k]) * inv_b);
      }
    } else {
      for (int c = lane; c < C; c += 64)
        dr[c] = (float)((s * exp((double)zr[c] - lse) - ce_target(y, C, b, pb, l, c)) * inv_b);
    }
  }
  return CeRow{s * lse - tz, lse, s, bi};
}

template <int KR>
__global__ __launch_bounds__(256) void ce_rows_kernel(const float* __restrict__ z, const float* __restrict__ y,
                                                      const int* __restrict__ perm, const float* __restrict__ lam, int B, int C,
                                                      float* __restrict__ dz, float* __restrict__ row_loss,
                                                      int* __restrict__ row_argmax) {
  const int b = blockIdx.x * kCeRowsPerBlock + (threadIdx.x >> 6);
  if (b >= B) return;
  const CeRow r = ce_row<KR>(z, y, perm, lam, B, C, b, dz);
  if ((threadIdx.x & 63) == 0) {
    if (row_loss) row_loss[b] = (float)r.ce;
    if (row_argmax) row_argmax[b] = r.amax;
  }
}

// sums[0] += mean_b CE_b, one block, fixed order: thread t adds rows t, t + 256, ... (each CE_b rounded to fp32 as row_loss
// holds it), then a fixed butterfly and a fixed combination of the four waves.  With row_loss == NULL the rows are recomputed
// here 256 at a time through LDS, so that the same values are added in the same order.
template <int KR>
__global__ __launch_bounds__(256) void ce_sum_kernel(const float* __restrict__ z, const float* __restrict__ y,
                                                     const int* __restrict__ perm, const float* __restrict__ lam, int B, int C,
                                                     const float* __restrict__ row_loss, float* __restrict__ sums) {
  __shared__ float s_row[256];
  __shared__ double s_red[4];
  const int t = threadIdx.x, w = t >> 6;
  double acc = 0.0;
  for (int r0 = 0; r0 < B; r0 += 256) {
    if (row_loss != nullptr) {
      if (r0 + t < B) acc += (double)row_loss[r0 + t];
    } else {
      for (int r = w; r < 256 && r0 + r < B; r += 4) {
        const CeRow cr = ce_row<KR>(z, y, perm, lam, B, C, r0 + r, nullptr);
        if ((t & 63) == 0) s_row[r] = (float)cr.ce;
      }
      __syncthreads();
      if (r0 + t < B) acc += (double)s_row[t];
      __syncthreads();
    }
  }
  acc = wave_sum_d(acc);
  if ((t & 63) == 0) s_red[w] = acc;
  __syncthreads();
  if (t == 0) sums[0] += (float)((((s_red[0] + s_red[1]) + s_red[2]) + s_red[3]) / (double)B);
}

template <int KR>
void ce_launch(const float* logits, const float* y, const int* perm, const float* lam, int B, int C, float* sums,
               float* dlogits, float* row_loss, int* row_argmax, hipStream_t s) {
  if (dlogits || row_loss || row_argmax)
    hipLaunchKernelGGL(ce_rows_kernel<KR>, dim3((unsigned)((B + kCeRowsPerBlock - 1) / kCeRowsPerBlock)), dim3(256), 0, s,
                       logits, y, perm, lam, B, C, dlogits, row_loss, row_argmax);
  if (sums) hipLaunchKernelGGL(ce_sum_kernel<KR>, dim3(1), dim3(256), 0, s, logits, y, perm, lam, B, C, row_loss, sums);
}

// ---- wave augmentation.  Block (x, b) writes a slice of out row b; 4 outputs per thread and trip, one 16-byte store where
// the row position is 16-byte aligned (the first `head` and the last `tail` < 4 samples of a row are scalar stores).
__global__ __launch_bounds__(256) void wave_augment_kernel(const float* __restrict__ bank, const double* __restrict__ bank_mean,
                                                           const int* __restrict__ bank_cls, long long n_bank, int L, int C,
                                                           const int* __restrict__ idx, const int* __restrict__ shift,
                                                           const float* __restrict__ amp, const float* __restrict__ mix,
                                                           float* __restrict__ out, float* __restrict__ y, int vec) {
  const int b = blockIdx.y;
  const int i0 = idx[2 * b], i1 = idx[2 * b + 1];
  const bool ok = i0 >= 0 && i0 < n_bank && i1 >= -1 && i1 < n_bank;   // (the wrapper validates; never read outside bank)
  const bool wm = ok && i1 >= 0;
  // roll by s: source position (n - s) mod L; s reduced to [0, L) once per block
  const int s0 = (int)(((long long)shift[2 * b] % L + L) % L);
  const int s1 = wm ? (int)(((long long)shift[2 * b + 1] % L + L) % L) : 0;
  const float a0 = amp[2 * b], a1 = wm ? amp[2 * b + 1] : 0.0f;
  const float l = wm ? mix[b] : 1.0f, lm = 1.0f - l;
  const float am0 = wm ? (float)((double)a0 * bank_mean[i0]) : 0.0f;
  const float am1 = wm ? (float)((double)a1 * bank_mean[i1]) : 0.0f;
  const float* r0 = bank + (ok ? (long long)i0 * L : 0);
  const float* r1 = bank + (wm ? (long long)i1 * L : 0);
  float* o = out + (long long)b * L;

  auto sample = [&](int n) -> float {
    if (!ok) return __builtin_nanf("");
    int p = n - s0;
    p += p < 0 ? L : 0;
    const float x0 = a0 * r0[p];
    if (!wm) return x0;
    int q = n - s1;
    q += q < 0 ? L : 0;
    return l * (x0 - am0) + lm * (a1 * r1[q] - am1);
  };

  const int head = vec ? min((int)((4 - ((long long)b * L & 3)) & 3), L) : L;
  const int nv = (L - head) >> 2;
  const int tail0 = head + 4 * nv;
  const int stride = gridDim.x * blockDim.x;
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += stride) {
    const int n = head + 4 * v;
    *reinterpret_cast<float4*>(o + n) = make_float4(sample(n), sample(n + 1), sample(n + 2), sample(n + 3));
  }
  if (blockIdx.x == 0) {
    if (!vec) {
      for (int n = threadIdx.x; n < L; n += blockDim.x) o[n] = sample(n);
    } else if (threadIdx.x < 8) {
      const int n = threadIdx.x < 4 ? threadIdx.x : tail0 + threadIdx.x - 4;
      if ((threadIdx.x < 4 && n < head) || (threadIdx.x >= 4 && n < L)) o[n] = sample(n);
    }
    if (y != nullptr) {
      const int c0 = ok ? bank_cls[i0] : -1, c1 = wm ? bank_cls[i1] : -1;
      for (int c = threadIdx.x; c < C; c += blockDim.x)
        y[(long long)b * C + c] = (c == c0 ? l : 0.0f) + (c == c1 ? lm : 0.0f);
    }
  }
}

// ---- masked BCE.  One row by one wave, one pass: lane l takes columns l, l + 64, ... in order, then a fixed butterfly.
// yy row = [labels (C) | mask (C)].  -> sum_c m_c bce(z_c, t_c) / C; dz / probs (if not NULL) are written on the way.
__device__ double bce_row(const float* __restrict__ z, const float* __restrict__ yy, const int* __restrict__ perm,
                          const float* __restrict__ lam, int B, int C, int binarize, int b, float* __restrict__ dz,
                          float* __restrict__ probs, long long probs_stride) {
  const int lane = threadIdx.x & 63;
  const eat::MixRow mr = eat::mix_row(perm, lam, b, B);
  const float* zr = z + (size_t)b * C;
  const float* ya = yy + (size_t)b * 2 * C;
  const float* yp = yy + (size_t)mr.pb * 2 * C;
  const double inv_bc = 1.0 / ((double)B * (double)C);
  double acc = 0.0;
  for (int c = lane; c < C; c += 64) {
    const double v = (double)zr[c];
    const double m = (double)ya[C + c];                     // the mask of row b only: the log-mel mix-up does not mix masks
    double t = binarize ? (ya[c] > 0.5f ? 1.0 : 0.0) : (double)ya[c];
    if (mr.mixed) t = mr.lam * t + (1.0 - mr.lam) * (binarize ? (yp[c] > 0.5f ? 1.0 : 0.0) : (double)yp[c]);
    const eat::BceTerm r = eat::bce_term(v);                               // NaN logit: NaN
    acc += m * r.loss(v, t);                                               // 0 * NaN = NaN: a NaN logit shows under mask 0 too
    if (dz != nullptr) dz[(size_t)b * C + c] = (float)(m * (r.p - t) * inv_bc);
    if (probs != nullptr) probs[(long long)b * probs_stride + c] = (float)r.p;
  }
  return wave_sum_d(acc) / (double)C;
}

__global__ __launch_bounds__(256) void bce_rows_kernel(const float* __restrict__ z, const float* __restrict__ yy,
                                                       const int* __restrict__ perm, const float* __restrict__ lam, int B, int C,
                                                       int binarize, float* __restrict__ dz, float* __restrict__ row_loss,
                                                       float* __restrict__ probs, long long probs_stride) {
  const int b = blockIdx.x * kCeRowsPerBlock + (threadIdx.x >> 6);
  if (b >= B) return;
  const double r = bce_row(z, yy, perm, lam, B, C, binarize, b, dz, probs, probs_stride);
  if ((threadIdx.x & 63) == 0 && row_loss) row_loss[b] = (float)r;
}

// sums[0] += mean_b row_b in the fixed order of ce_sum_kernel (rows as fp32, thread t adds rows t, t + 256, ...); with
// row_loss == NULL the rows are recomputed here so that the same values are added in the same order.
__global__ __launch_bounds__(256) void bce_sum_kernel(const float* __restrict__ z, const float* __restrict__ yy,
                                                      const int* __restrict__ perm, const float* __restrict__ lam, int B, int C,
                                                      int binarize, const float* __restrict__ row_loss, float* __restrict__ sums) {
  __shared__ float s_row[256];
  __shared__ double s_red[4];
  const int t = threadIdx.x, w = t >> 6;
  double acc = 0.0;
  for (int r0 = 0; r0 < B; r0 += 256) {
    if (row_loss != nullptr) {
      if (r0 + t < B) acc += (double)row_loss[r0 + t];
    } else {
      for (int r = w; r < 256 && r0 + r < B; r += 4) {
        const double v = bce_row(z, yy, perm, lam, B, C, binarize, r0 + r, nullptr, nullptr, 0);
        if ((t & 63) == 0) s_row[r] = (float)v;
      }
      __syncthreads();
      if (r0 + t < B) acc += (double)s_row[t];
      __syncthreads();
    }
  }
  acc = wave_sum_d(acc);
  if ((t & 63) == 0) s_red[w] = acc;
  __syncthreads();
  if (t == 0) sums[0] += (float)((((s_red[0] + s_red[1]) + s_red[2]) + s_red[3]) / (double)B);
}

// ---- OpenMIC wave-mix labels: block b writes yy row b (2C values) from bank_y rows idx[2b], idx[2b + 1].
__global__ __launch_bounds__(64) void openmic_targets_kernel(const float* __restrict__ bank_y, long long n_bank, int C,
                                                             const int* __restrict__ idx, const float* __restrict__ mix,
                                                             float* __restrict__ yy) {
  const int b = blockIdx.x;
  const int i0 = idx[2 * b], i1 = idx[2 * b + 1];
  const bool ok = i0 >= 0 && i0 < n_bank && i1 >= -1 && i1 < n_bank;   // (as wave_augment_kernel: never read outside bank_y)
  const bool wm = ok && i1 >= 0;
  const float* y1 = bank_y + (ok ? (long long)i0 * 2 * C : 0);
  const float* y2 = bank_y + (wm ? (long long)i1 * 2 * C : 0);
  const double l = wm ? (double)mix[b] : 1.0;
  float* o = yy + (long long)b * 2 * C;
  for (int c = threadIdx.x; c < C; c += blockDim.x) {
    if (!ok) {
      o[c] = o[C + c] = __builtin_nanf("");
    } else if (!wm) {
      o[c] = y1[c];                                          // an unmixed row is a copy: its labels are not masked
      o[C + c] = y1[C + c];
    } else {
      const double m1 = y1[C + c] > 0.5f ? 1.0 : 0.0, m2 = y2[C + c] > 0.5f ? 1.0 : 0.0;
      // (both products are exact in fp64, so the sum is rounded once there and once to fp32, fused or not)
      o[c] = (float)(l * ((double)y1[c] * m1) + (1.0 - l) * ((double)y2[c] * m2));
      o[C + c] = (float)(m1 > m2 ? m1 : m2);
    }
  }
}

}  // namespace

extern "C" int eat_softmax_ce_fwd_bwd(const float* logits, const float* y, const int* perm, const float* lam, int B, int C,
                                      float* sums, float* dlogits, float* row_loss, int* row_argmax, eat_stream_t stream) {
  eat::clear_stale_error();
  if (B < 1 || C < 1 || (long long)B * C > 0x7fffffffLL)
    return eat::fail(EAT_EINVAL, "eat_softmax_ce_fwd_bwd: bad shape (B = %d, C = %d)", B, C);
  if ((perm == nullptr) != (lam == nullptr)) return eat::fail(EAT_EINVAL, "eat_softmax_ce_fwd_bwd: perm and lam go together");
  if (!logits || !y) return eat::fail(EAT_EINVAL, "eat_softmax_ce_fwd_bwd: logits and y are required");
  hipStream_t s = (hipStream_t)stream;
  if (C <= 64 * kCeReg)
    ce_launch<kCeReg>(logits, y, perm, lam, B, C, sums, dlogits, row_loss, row_argmax, s);
  else
    ce_launch<0>(logits, y, perm, lam, B, C, sums, dlogits, row_loss, row_argmax, s);
  return eat::check_launch("eat_softmax_ce_fwd_bwd");
}

extern "C" int eat_wave_augment(const float* bank, const double* bank_mean, const int* bank_cls, long long n_bank, int L, int C,
                                const int* idx, const int* shift, const float* amp, const float* mix, float* out, float* y, int B,
                                eat_stream_t stream) {
  eat::clear_stale_error();
  if (B < 1 || L < 1 || n_bank < 1 || (y != nullptr && C < 1))
    return eat::fail(EAT_EINVAL, "eat_wave_augment: bad shape (B = %d, L = %d, n_bank = %lld, C = %d)", B, L, n_bank, C);
  if (!bank || !bank_mean || !idx || !shift || !amp || !mix || !out || (y && !bank_cls))
    return eat::fail(EAT_EINVAL, "eat_wave_augment: a required pointer is NULL");
  if (B > 65535) return eat::fail(EAT_EINVAL, "eat_wave_augment: B = %d > 65535", B);
  const int vec = ((uintptr_t)out & 15) == 0;
  const long long nv = (long long)L / 4;
  long long bx = (nv + 255) / 256;
  if (bx < 1) bx = 1;
  if (bx > 1024) bx = 1024;
  hipLaunchKernelGGL(wave_augment_kernel, dim3((unsigned)bx, (unsigned)B), dim3(256), 0, (hipStream_t)stream, bank, bank_mean,
                     bank_cls, n_bank, L, C, idx, shift, amp, mix, out, y, vec);
  return eat::check_launch("eat_wave_augment");
}

extern "C" int eat_masked_bce_fwd_bwd(const float* logits, const float* yy, const int* perm, const float* lam, int B, int C,
                                      int binarize, float* sums, float* dlogits, float* row_loss, float* probs,
                                      long long probs_stride, eat_stream_t stream) {
  eat::clear_stale_error();
  if (B < 1 || C < 1 || 2LL * B * C > 0x7fffffffLL)
    return eat::fail(EAT_EINVAL, "eat_masked_bce_fwd_bwd: bad shape (B = %d, C = %d)", B, C);
  if ((perm == nullptr) != (lam == nullptr)) return eat::fail(EAT_EINVAL, "eat_masked_bce_fwd_bwd: perm and lam go together");
  if (!logits || !yy) return eat::fail(EAT_EINVAL, "eat_masked_bce_fwd_bwd: logits and yy are required");
  if (probs != nullptr && probs_stride < C)
    return eat::fail(EAT_EINVAL, "eat_masked_bce_fwd_bwd: probs_stride = %lld < C = %d", probs_stride, C);
  hipStream_t s = (hipStream_t)stream;
  if (dlogits || row_loss || probs)
    hipLaunchKernelGGL(bce_rows_kernel, dim3((unsigned)((B + kCeRowsPerBlock - 1) / kCeRowsPerBlock)), dim3(256), 0, s, logits,
                       yy, perm, lam, B, C, binarize ? 1 : 0, dlogits, row_loss, probs, probs_stride);
  if (sums)
    hipLaunchKernelGGL(bce_sum_kernel, dim3(1), dim3(256), 0, s, logits, yy, perm, lam, B, C, binarize ? 1 : 0, row_loss, sums);
  return eat::check_launch("eat_masked_bce_fwd_bwd");
}

extern "C" int eat_openmic_targets(const float* bank_y, long long n_bank, int C, const int* idx, const float* mix, float* yy,
                                   int B, eat_stream_t stream) {
  eat::clear_stale_error();
  if (B < 1 || C < 1 || n_bank < 1 || 2LL * B * C > 0x7fffffffLL)
    return eat::fail(EAT_EINVAL, "eat_openmic_targets: bad shape (B = %d, C = %d, n_bank = %lld)", B, C, n_bank);
  if (!bank_y || !idx || !mix || !yy) return eat::fail(EAT_EINVAL, "eat_openmic_targets: a required pointer is NULL");
  hipLaunchKernelGGL(openmic_targets_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, bank_y, n_bank, C, idx, mix, yy);
  return eat::check_launch("eat_openmic_targets");
}
