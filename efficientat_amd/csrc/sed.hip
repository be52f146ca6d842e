// Device side of strong-label sound-event-detection training (include/eat_sed.h): frame targets that follow a clip through
// the crop / pad / roll / wave-mix of eat_wave_augment_ragged (ragged.hip), the frame-level BCE with its gradient and the
// evaluation counts, the padded copy + bias gradient of a gradient arriving at the frame logits, and the elementwise halves of
// the frame head's hidden layer.
//
// Layout.  Frame tensors are (B, rows, Tp) with the time axis innermost.  sed_targets runs one lane per (class, frame) of a
// sample, flat over the K Tp elements of its rows: every store is contiguous, and each lane bisects its clip's class-sorted
// event run and walks its own class only.  The reducing kernels (bce, grad_pad, hidden_bwd) give one block a class / unit row
// over all (b, t): a thread takes the elements tid, tid + 256, ... in order and adds in fp64, then a fixed butterfly and the four
// waves in order - no atomics, the same bits on every call.  Reads are runs of Tp contiguous floats per sample.
#include "eat_common.h"
#include "event_bank.h"
#include "loss_terms.h"
#include "reduce.h"
#include "../../include/eat_sed.h"

namespace {

constexpr int kThreads = 256;
constexpr int kGridY = 65535;

using eat::block_sum_d, eat::block_sum_ll;

// ---------------------------------------------------------------------------------------------------------- targets
struct SedSlot {
  long long e0, e1;      // the clip's event rows, clipped to the table
  int st, w, s;          // crop start, window length, roll reduced to [0, L)
  bool ok;
};

__device__ __forceinline__ SedSlot sed_slot(const long long* __restrict__ eo, const int* __restrict__ lengths, long long n_bank,
                                            long long n_events, int L, int i, int st, int sh) {
  const eat::ClipWindow cw = eat::clip_window(lengths, n_bank, L, i, st);
  if (!cw.ok) return SedSlot{0, 0, 0, 0, 0, false};
  const eat::EventRows r = eat::event_rows(eo, n_events, i);
  return SedSlot{r.e0, r.e1, st, cw.w, (int)(((long long)sh % L + L) % L), true};
}

// 1 iff an event of class c of the slot's clip shows in one of the output samples [n0, n1) of the rolled window
__device__ __forceinline__ int sed_active(const int* __restrict__ ev, const SedSlot& q, int c, long long n0, long long n1, int L) {
  // window positions p = (n - s) mod L of the frame: [a_lo, a_hi) from its samples n >= s, [b_lo, b_hi) from those below s;
  // only p < w is signal
  const long long s = q.s, w = q.w;
  const long long a_lo = (n0 > s ? n0 : s) - s, a_hi = min(n1 - s, w);
  const long long b_lo = n0 - s + L, b_hi = min((n1 < s ? n1 : s) - s + L, w);
  return eat::any_row_of_class(ev, q.e0, q.e1, c, [&](long long ev_on, long long ev_off) {
    const long long on = ev_on - q.st, off = ev_off - q.st;
    return (a_lo < a_hi && on < a_hi && off > a_lo) || (b_lo < b_hi && on < b_hi && off > b_lo);
  });
}

__global__ __launch_bounds__(kThreads) void sed_targets_kernel(
    const int* __restrict__ ev, long long n_events, const long long* __restrict__ eo, const int* __restrict__ lengths,
    long long n_bank, int K, const int* __restrict__ idx, const int* __restrict__ start, const int* __restrict__ shift,
    const float* __restrict__ mix, int B, int L, int R, int T, int Tp, float* __restrict__ y) {
  const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (j >= (long long)K * Tp) return;
  const int c = (int)(j / Tp), t = (int)(j - (long long)c * Tp);
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    float v = 0.0f;
    if (t < T) {
      const int i1 = idx[2 * b + 1];
      const SedSlot q0 = sed_slot(eo, lengths, n_bank, n_events, L, idx[2 * b], start[2 * b], shift[2 * b]);
      const SedSlot q1 = i1 == -1 ? SedSlot{0, 0, 0, 0, 0, false}
                                  : sed_slot(eo, lengths, n_bank, n_events, L, i1, start[2 * b + 1], shift[2 * b + 1]);
      const bool ok = q0.ok && (i1 == -1 || q1.ok);
      const long long n0 = (long long)t * R;
      const long long n1 = min(n0 + R, (long long)L);
      if (!ok) {
        v = __builtin_nanf("");
      } else if (n0 < L) {                                   // (a frame past the window owns no sample: 0)
        const int a0 = sed_active(ev, q0, c, n0, n1, L);
        if (i1 == -1) {
          v = (float)a0;
        } else {
          const int a1 = sed_active(ev, q1, c, n0, n1, L);
          const double l = (double)mix[b];
          // (both products are exact in fp64, so the sum is rounded once there and once to fp32, fused or not)
          v = (float)(l * (double)a0 + (1.0 - l) * (double)a1);
        }
      }
    }
    y[(long long)b * K * Tp + j] = v;
  }
}

// ---------------------------------------------------------------------------------------------------------- frame BCE
__device__ __forceinline__ int row_frames(const int* __restrict__ nframes, int b, int T) {
  if (nframes == nullptr) return T;
  const int n = nframes[b];
  return n < 0 ? 0 : (n > T ? T : n);
}

// Block c: class row c of every sample.  ws[c] = the class's loss sum (fp64), ws[K] = M (block 0).
__global__ __launch_bounds__(kThreads) void frame_bce_kernel(
    const float* __restrict__ z, const float* __restrict__ y, const int* __restrict__ perm, const float* __restrict__ lam,
    const int* __restrict__ nframes, const float* __restrict__ thr, int B, int K, int T, int Tp, int Kp,
    float* __restrict__ dl, float* __restrict__ dbias, long long* __restrict__ counts, float* __restrict__ rows,
    double* __restrict__ ws) {
  __shared__ double s_d[4];
  __shared__ long long s_l[4];
  const int c = blockIdx.x, tid = threadIdx.x;
  const long long items = (long long)B * Tp;
  if (c >= K) {                                              // block-uniform: a pad row of dlogits
    if (dl != nullptr)
      for (long long j = tid; j < items; j += kThreads) {
        const long long b = j / Tp;
        dl[(b * Kp + c) * Tp + (j - b * Tp)] = 0.0f;
      }
    return;
  }
  long long nsum = 0;
  for (int b = tid; b < B; b += kThreads) nsum += row_frames(nframes, b, T);
  const long long M = (long long)K * block_sum_ll(nsum, s_l);
  const double dM = (double)M;
  const float th = counts != nullptr ? thr[c] : 0.0f;
  double loss = 0.0, db = 0.0;
  long long tp = 0, fp = 0, fn = 0;
  for (long long j = tid; j < items; j += kThreads) {
    const int b = (int)(j / Tp), t = (int)(j - (long long)b * Tp);
    const int nb = row_frames(nframes, b, T);
    const long long at = ((long long)b * K + c) * Tp + t;
    float zf = 0.0f;
    if (t < T) zf = z[at];
    if (rows != nullptr && t < T) rows[((long long)b * T + t) * K + c] = zf;
    double d = 0.0;
    if (t < nb) {
      const float yf = y[at];
      double tt = (double)yf;
      const eat::MixRow mr = eat::mix_row(perm, lam, b, B);
      if (mr.mixed) tt = mr.lam * tt + (1.0 - mr.lam) * (double)y[((long long)mr.pb * K + c) * Tp + t];
      const double v = (double)zf;
      const eat::BceTerm r = eat::bce_term(v);
      loss += r.loss(v, tt);
      d = (r.p - tt) / dM;                                           // (nb >= 1 here, so M >= 1)
      db += d;
      if (counts != nullptr) {
        const bool p = eat::sigmoid(zf) >= th, g = yf > 0.5f;
        tp += (p && g) ? 1 : 0;
        fp += (p && !g) ? 1 : 0;
        fn += (!p && g) ? 1 : 0;
      }
    }
    if (dl != nullptr) dl[((long long)b * Kp + c) * Tp + t] = (float)d;
  }
  if (ws != nullptr) {
    loss = block_sum_d(loss, s_d);
    if (tid == 0) {
      ws[c] = loss;
      if (c == 0) ws[K] = dM;
    }
  }
  if (dbias != nullptr) {
    db = block_sum_d(db, s_d);
    if (tid == 0) dbias[c] = (float)db;
  }
  if (counts != nullptr) {
    tp = block_sum_ll(tp, s_l);
    fp = block_sum_ll(fp, s_l);
    fn = block_sum_ll(fn, s_l);
    if (tid == 0) {
      counts[3 * (long long)c] += tp;
      counts[3 * (long long)c + 1] += fp;
      counts[3 * (long long)c + 2] += fn;
    }
  }
}

// sums[0] += (sum_c ws[c]) / M: thread t adds the classes t, t + 256, ... in order
__global__ __launch_bounds__(kThreads) void frame_bce_sum_kernel(const double* __restrict__ ws, int K, float* __restrict__ sums) {
  __shared__ double s_d[4];
  double acc = 0.0;
  for (int c = threadIdx.x; c < K; c += kThreads) acc += ws[c];
  acc = block_sum_d(acc, s_d);
  const double M = ws[K];
  if (threadIdx.x == 0) sums[0] += M > 0.0 ? (float)(acc / M) : 0.0f;
}

// Block c: row c of dl for every sample, and db[c]
__global__ __launch_bounds__(kThreads) void frame_grad_pad_kernel(const float* __restrict__ g, float* __restrict__ dl,
                                                                  float* __restrict__ db, int B, int K, int Kp, int T, int Tp) {
  __shared__ double s_d[4];
  const int c = blockIdx.x, tid = threadIdx.x;
  const long long items = (long long)B * Tp;
  double acc = 0.0;
  for (long long j = tid; j < items; j += kThreads) {
    const long long b = j / Tp;
    const int t = (int)(j - b * Tp);
    float v = 0.0f;
    if (c < K && t < T) v = g[(b * K + c) * Tp + t];
    acc += (double)v;
    dl[(b * Kp + c) * Tp + t] = v;
  }
  if (c >= K || db == nullptr) return;                       // block-uniform
  acc = block_sum_d(acc, s_d);
  if (tid == 0) db[c] = (float)acc;
}

// ---------------------------------------------------------------------------------------------------------- hidden layer
__device__ __forceinline__ float hswish(float v) { return eat::activate<EAT_ACT_HSWISH>(v); }
// the derivative of mlp_head_bwd (se_train.hip), kinks included
__device__ __forceinline__ float hswish_grad(float u) { return u < -3.0f ? 0.0f : (u <= 3.0f ? u * (1.0f / 3.0f) + 0.5f : 1.0f); }

// VEC: Tp % 4 == 0 and 16-byte aligned operands - a float4 never straddles a row
template <bool VEC>
__global__ __launch_bounds__(kThreads) void frame_hidden_fwd_kernel(const float* __restrict__ z1, const float* __restrict__ keep,
                                                                    float* __restrict__ h, long long n, int Tp) {
  const long long stride = (long long)gridDim.x * kThreads;
  if constexpr (VEC) {
    const float4* zv = reinterpret_cast<const float4*>(z1);
    float4* hv = reinterpret_cast<float4*>(h);
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; 4 * i < n; i += stride) {
      const float k = keep != nullptr ? keep[4 * i / Tp] : 1.0f;
      const float4 v = zv[i];
      hv[i] = make_float4(hswish(v.x) * k, hswish(v.y) * k, hswish(v.z) * k, hswish(v.w) * k);
    }
  } else {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += stride)
      h[i] = hswish(z1[i]) * (keep != nullptr ? keep[i / Tp] : 1.0f);
  }
}

// Block j: hidden row j of every sample, and db1[j]
__global__ __launch_bounds__(kThreads) void frame_hidden_bwd_kernel(const float* __restrict__ dh, const float* __restrict__ z1,
                                                                    const float* __restrict__ keep, float* __restrict__ dz1,
                                                                    float* __restrict__ db1, int B, int H, int Hp, int T, int Tp) {
  __shared__ double s_d[4];
  const int jr = blockIdx.x, tid = threadIdx.x;
  const long long items = (long long)B * Tp;
  double acc = 0.0;
  for (long long j = tid; j < items; j += kThreads) {
    const long long b = j / Tp;
    const int t = (int)(j - b * Tp);
    const long long at = (b * Hp + jr) * Tp + t;
    float v = 0.0f;
    if (jr < H && t < T) v = dh[at] * (keep != nullptr ? keep[b * Hp + jr] : 1.0f) * hswish_grad(z1[at]);
    acc += (double)v;
    dz1[at] = v;
  }
  if (jr >= H || db1 == nullptr) return;                     // block-uniform
  acc = block_sum_d(acc, s_d);
  if (tid == 0) db1[jr] = (float)acc;
}

}  // namespace

extern "C" int eat_sed_targets(const int* events, long long n_events, const long long* event_offsets, const int* lengths,
                               long long n_bank, int K, const int* idx, const int* start, const int* shift, const float* mix,
                               int B, int L, int R, int T, int Tp, float* y, eat_stream_t stream) {
  eat::clear_stale_error();
  if (!event_offsets || !lengths || !idx || !start || !shift || !mix || !y || (!events && n_events != 0))
    return eat::fail(EAT_EINVAL, "eat_sed_targets: missing operand");
  if (B < 1 || K < 1 || L < 1 || R < 1 || T < 1 || n_bank < 1 || n_events < 0 || Tp < T)
    return eat::fail(EAT_EINVAL, "eat_sed_targets: need B, K, L, R, T, n_bank >= 1, n_events >= 0 and Tp >= T (got B=%d K=%d L=%d "
                     "R=%d T=%d n_bank=%lld n_events=%lld Tp=%d)", B, K, L, R, T, n_bank, n_events, Tp);
  const long long bx = ((long long)K * Tp + kThreads - 1) / kThreads;
  if (bx > 0x7fffffffLL) return eat::fail(EAT_EINVAL, "eat_sed_targets: K=%d x Tp=%d exceeds the grid", K, Tp);
  hipLaunchKernelGGL(sed_targets_kernel, dim3((unsigned)bx, (unsigned)(B < kGridY ? B : kGridY)), dim3(kThreads), 0,
                     (hipStream_t)stream, events, n_events, event_offsets, lengths, n_bank, K, idx, start, shift, mix, B, L, R, T,
                     Tp, y);
  return eat::check_launch("eat_sed_targets");
}

extern "C" int eat_frame_bce_fwd_bwd(const float* z, const float* y, const int* perm, const float* lam, const int* nframes,
                                     const float* thr, int B, int K, int T, int Tp, int Kp, float* sums, float* dlogits,
                                     float* dbias, long long* counts, float* rows, double* ws, eat_stream_t stream) {
  eat::clear_stale_error();
  if (!z || !y) return eat::fail(EAT_EINVAL, "eat_frame_bce_fwd_bwd: missing operand (z and y are required)");
  if ((perm == nullptr) != (lam == nullptr)) return eat::fail(EAT_EINVAL, "eat_frame_bce_fwd_bwd: perm and lam go together");
  if (counts && !thr) return eat::fail(EAT_EINVAL, "eat_frame_bce_fwd_bwd: missing operand (counts need thr)");
  if (counts && perm) return eat::fail(EAT_EINVAL, "eat_frame_bce_fwd_bwd: counts are taken against unmixed targets (perm given)");
  if (sums && !ws) return eat::fail(EAT_EINVAL, "eat_frame_bce_fwd_bwd: missing operand (sums need the workspace ws)");
  if (B < 1 || K < 1 || T < 1 || Tp < T || Kp < K)
    return eat::fail(EAT_EINVAL, "eat_frame_bce_fwd_bwd: need B, K, T >= 1, Tp >= T and Kp >= K (got B=%d K=%d T=%d Tp=%d Kp=%d)", B,
                     K, T, Tp, Kp);
  hipStream_t s = (hipStream_t)stream;
  if (sums || dlogits || dbias || counts || rows)
    hipLaunchKernelGGL(frame_bce_kernel, dim3((unsigned)(dlogits ? Kp : K)), dim3(kThreads), 0, s, z, y, perm, lam, nframes, thr, B,
                       K, T, Tp, Kp, dlogits, dbias, counts, rows, sums ? ws : (double*)nullptr);
  if (sums) hipLaunchKernelGGL(frame_bce_sum_kernel, dim3(1), dim3(kThreads), 0, s, ws, K, sums);
  return eat::check_launch("eat_frame_bce_fwd_bwd");
}

extern "C" int eat_frame_grad_pad(const float* g, float* dl, float* db, int B, int K, int Kp, int T, int Tp, eat_stream_t stream) {
  eat::clear_stale_error();
  if (!g || !dl) return eat::fail(EAT_EINVAL, "eat_frame_grad_pad: missing operand");
  if (g == dl) return eat::fail(EAT_EINVAL, "eat_frame_grad_pad: dl must not be g");
  if (B < 1 || K < 1 || T < 1 || Tp < T || Kp < K)
    return eat::fail(EAT_EINVAL, "eat_frame_grad_pad: need B, K, T >= 1, Tp >= T and Kp >= K (got B=%d K=%d T=%d Tp=%d Kp=%d)", B, K,
                     T, Tp, Kp);
  hipLaunchKernelGGL(frame_grad_pad_kernel, dim3((unsigned)Kp), dim3(kThreads), 0, (hipStream_t)stream, g, dl, db, B, K, Kp, T, Tp);
  return eat::check_launch("eat_frame_grad_pad");
}

extern "C" int eat_frame_hidden_fwd(const float* z1, const float* keep, float* h, int B, int Hp, int Tp, eat_stream_t stream) {
  eat::clear_stale_error();
  if (!z1 || !h) return eat::fail(EAT_EINVAL, "eat_frame_hidden_fwd: missing operand");
  if (B < 1 || Hp < 1 || Tp < 1)
    return eat::fail(EAT_EINVAL, "eat_frame_hidden_fwd: need B, Hp, Tp >= 1 (got %d, %d, %d)", B, Hp, Tp);
  const long long n = (long long)B * Hp * Tp;
  const bool vec = Tp % 4 == 0 && (((uintptr_t)z1 | (uintptr_t)h) & 15) == 0;
  long long blocks = ((vec ? n / 4 : n) + kThreads - 1) / kThreads;
  if (blocks > 4096) blocks = 4096;
  if (vec)
    hipLaunchKernelGGL(frame_hidden_fwd_kernel<true>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, z1, keep, h, n,
                       Tp);
  else
    hipLaunchKernelGGL(frame_hidden_fwd_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, z1, keep, h,
                       n, Tp);
  return eat::check_launch("eat_frame_hidden_fwd");
}

extern "C" int eat_frame_hidden_bwd(const float* dh, const float* z1, const float* keep, float* dz1, float* db1, int B, int H,
                                    int Hp, int T, int Tp, eat_stream_t stream) {
  eat::clear_stale_error();
  if (!dh || !z1 || !dz1) return eat::fail(EAT_EINVAL, "eat_frame_hidden_bwd: missing operand");
  if (B < 1 || H < 1 || T < 1 || Hp < H || Tp < T)
    return eat::fail(EAT_EINVAL, "eat_frame_hidden_bwd: need B, H, T >= 1, Hp >= H and Tp >= T (got B=%d H=%d Hp=%d T=%d Tp=%d)", B,
                     H, Hp, T, Tp);
  hipLaunchKernelGGL(frame_hidden_bwd_kernel, dim3((unsigned)Hp), dim3(kThreads), 0, (hipStream_t)stream, dh, z1, keep, dz1, db1, B,
                     H, Hp, T, Tp);
  return eat::check_launch("eat_frame_hidden_bwd");
}
