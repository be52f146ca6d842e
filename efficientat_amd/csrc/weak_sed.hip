// Device side of weak-label sound-event-detection training (include/eat_weak_sed.h): the clip-level targets and the
// frame-truth flag of a batch drawn by eat_wave_augment_ragged, and the frame BCE over the samples that have frame truth fused
// with the clip-level BCE behind linear-softmax pooling, P = sum_t p_t^2 / sum_t p_t, of the frame probabilities.
//
// Layout.  sed_clip_targets runs one lane per (sample, class): it bisects its clip's class-sorted event run and walks its own
// class only (the walk of sed_active in sed.hip without the roll).  weak_frame_bce gives block c class row c of every sample,
// as frame_bce_kernel (sed.hip) does, but a ROW (b, c) of T contiguous floats belongs to one group of G lanes - G = 32 for
// T <= 32 (two rows per wave at the default geometry), else 64 - because the pooled term needs the row's S1 and S2 before any
// of its gradients: lane l takes t = l, l + G, ..., an xor butterfly over the group leaves S1, S2 in every lane, and the
// gradient is formed from the probability kept in registers (t < G) or recomputed from a cached re-read (t >= G).  The groups
// walk b = group, group + 256 / G, ... in order; loss and bias sums are added in fp64 per lane, then a fixed butterfly and the
// four waves in order - no atomics, the same bits on every call.  The number of framed samples is counted by every block from
// `framed` itself, so a captured step serves any mixture of strong and weak clips.
#include "eat_common.h"
#include "event_bank.h"
#include "loss_terms.h"
#include "reduce.h"
#include "../../include/eat_weak_sed.h"

namespace {

constexpr int kThreads = 256;

using eat::block_sum_d, eat::block_sum_ll;

// ---------------------------------------------------------------------------------------------------------- clip targets
struct ClipSlot {
  long long e0, e1;      // the clip's event rows, clipped to the table
  long long lo, hi;      // the clip's samples the slot shows: [lo, hi)
  bool ok;
};

__device__ __forceinline__ ClipSlot clip_slot(const long long* __restrict__ eo, const int* __restrict__ lengths, long long n_bank,
                                              long long n_events, int L, int i, int st) {
  const eat::ClipWindow cw = eat::clip_window(lengths, n_bank, L, i, st);
  if (!cw.ok) return ClipSlot{0, 0, 0, 0, false};
  const eat::EventRows r = eat::event_rows(eo, n_events, i);
  return ClipSlot{r.e0, r.e1, st, (long long)st + cw.w, true};
}

// 1 iff an event of class c of the slot's clip meets the samples the slot shows
__device__ __forceinline__ int clip_active(const int* __restrict__ ev, const ClipSlot& q, int c) {
  return eat::class_run_overlaps(ev, q.e0, q.e1, c, q.lo, q.hi);
}

__global__ __launch_bounds__(kThreads) void sed_clip_targets_kernel(
    const int* __restrict__ ev, long long n_events, const long long* __restrict__ eo, const int* __restrict__ lengths,
    long long n_bank, int K, const int* __restrict__ idx, const int* __restrict__ start, const float* __restrict__ mix,
    const unsigned char* __restrict__ strong, int B, int L, float* __restrict__ w, int* __restrict__ framed) {
  const long long j = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (j >= (long long)B * K) return;
  const long long b = j / K;
  const int c = (int)(j - b * K);
  const int i0 = idx[2 * b], i1 = idx[2 * b + 1];
  const ClipSlot q0 = clip_slot(eo, lengths, n_bank, n_events, L, i0, start[2 * b]);
  const ClipSlot q1 = i1 == -1 ? ClipSlot{0, 0, 0, 0, false} : clip_slot(eo, lengths, n_bank, n_events, L, i1, start[2 * b + 1]);
  float v = __builtin_nanf("");
  int fr = 0;
  if (q0.ok && (i1 == -1 || q1.ok)) {
    const int a0 = clip_active(ev, q0, c);
    fr = strong == nullptr || strong[i0] != 0;
    if (i1 == -1) {
      v = (float)a0;
    } else {
      const int a1 = clip_active(ev, q1, c);
      const double l = (double)mix[b];
      // (both products are exact in fp64, so the sum is rounded once there and once to fp32, fused or not)
      v = (float)(l * (double)a0 + (1.0 - l) * (double)a1);
      fr = fr && (strong == nullptr || strong[i1] != 0);
    }
  }
  w[j] = v;
  if (c == 0) framed[b] = fr;
}

// ---------------------------------------------------------------------------------------------------------- the fused loss
// f_b: the sample and its mix-up partner both carry frame truth (a bad permutation falls back to the sample itself)
__device__ __forceinline__ int row_framed(const int* __restrict__ framed, const int* __restrict__ perm, int b, int B) {
  int f = framed[b] != 0;
  if (perm != nullptr) {
    const int pb = perm[b];
    if (pb >= 0 && pb < B) f = f && framed[pb] != 0;
  }
  return f;
}

// Block c: class row c of every sample, a group of G lanes per row (b, c).  ws[c] = the class's frame-loss sum, ws[K + c] its
// clip-loss sum (fp64, not yet normalised), ws[2 K] = N_f (block 0).
template <int G>
__global__ __launch_bounds__(kThreads) void weak_frame_bce_kernel(
    const float* __restrict__ z, const float* __restrict__ y, const float* __restrict__ w, const int* __restrict__ framed,
    const int* __restrict__ perm, const float* __restrict__ lam, float weak_weight, float eps_f, int B, int K, int T, int Tp,
    int Kp, float* __restrict__ dl, float* __restrict__ dbias, float* __restrict__ clip_prob, double* __restrict__ ws) {
  __shared__ double s_d[4];
  __shared__ long long s_l[4];
  constexpr int kGroups = kThreads / G;
  const int c = blockIdx.x, tid = threadIdx.x;
  if (c >= K) {                                              // block-uniform: a pad row of dlogits
    if (dl != nullptr) {
      const long long items = (long long)B * Tp;
      for (long long j = tid; j < items; j += kThreads) {
        const long long b = j / Tp;
        dl[(b * Kp + c) * Tp + (j - b * Tp)] = 0.0f;
      }
    }
    return;
  }
  long long nsum = 0;
  for (int b = tid; b < B; b += kThreads) nsum += row_framed(framed, perm, b, B);
  const double Nf = (double)K * (double)T * (double)block_sum_ll(nsum, s_l);
  const double ww = (double)weak_weight, eps = (double)eps_f, BK = (double)B * (double)K;
  const int g = tid / G, l = tid % G;
  double loss_f = 0.0, loss_c = 0.0, db = 0.0;
  for (int b0 = 0; b0 < B; b0 += kGroups) {                  // (the trip count is block-uniform: every lane meets every shuffle)
    const int b = b0 + g;
    const bool live = b < B;                                 // group-uniform
    int pb = live ? b : 0, fb = 0;
    bool bad = false;
    double lm = 1.0, tw = 0.0;
    if (live) {
      fb = framed[b] != 0;
      tw = (double)w[(long long)b * K + c];
      if (perm != nullptr) {
        const eat::MixRow mr = eat::mix_row(perm, lam, b, B);
        pb = mr.pb, lm = mr.lam, bad = mr.bad;
        tw = lm * tw + (1.0 - lm) * (double)w[(long long)pb * K + c];
        fb = fb && framed[pb] != 0;
      }
    }
    const long long row = ((long long)(live ? b : 0) * K + c) * Tp, prow = ((long long)pb * K + c) * Tp;
    // pass 1: S1, S2 and the frame loss; the lane's first frame stays in registers
    double s1 = 0.0, s2 = 0.0, p0 = 0.0, q0 = 0.0, ty0 = 0.0;
    if (live)
      for (int t = l; t < T; t += G) {
        const double v = (double)z[row + t];
        const eat::BceTerm r = eat::bce_term(v);
        s1 += r.p;
        s2 += r.p * r.p;
        double ty = 0.0;
        if (fb) {
          ty = (double)y[row + t];
          if (perm != nullptr) ty = lm * ty + (1.0 - lm) * (double)y[prow + t];
          loss_f += r.loss(v, ty);
        }
        if (t == l) p0 = r.p, q0 = r.q, ty0 = ty;
      }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {                    // within the group: every lane of it holds the row's sums
      s1 += __shfl_xor(s1, o, 64);
      s2 += __shfl_xor(s2, o, 64);
    }
    const double P = s1 > 0.0 ? s2 / s1 : 0.0;
    const double Pc = fmin(fmax(P, eps), 1.0 - eps);
    // weak_weight (Pc - tw) / (Pc (1 - Pc)) / S1 / (B K): what multiplies (2 p_t - P) p_t (1 - p_t)
    const double coef = s1 > 0.0 ? ww * ((Pc - tw) / (Pc * (1.0 - Pc))) / s1 / BK : 0.0;
    if (live && l == 0) {
      loss_c += -(tw * log(Pc) + (1.0 - tw) * log1p(-Pc));
      if (clip_prob != nullptr) clip_prob[(long long)b * K + c] = (float)P;
    }
    // pass 2: the gradient, pads included
    if (live && (dl != nullptr || dbias != nullptr))
      for (int t = l; t < Tp; t += G) {
        double d = 0.0;
        if (t < T) {
          double p = p0, q = q0, ty = ty0;
          if (t != l) {
            const eat::BceTerm r = eat::bce_term((double)z[row + t]);
            p = r.p, q = r.q;
            if (fb) {
              ty = (double)y[row + t];
              if (perm != nullptr) ty = lm * ty + (1.0 - lm) * (double)y[prow + t];
            }
          }
          if (fb) d = (p - ty) / Nf;                         // (fb: N_f >= K T >= 1)
          d += coef * ((2.0 * p - P) * p * q);
          if (bad) d = __builtin_nan("");
          db += d;
        }
        if (dl != nullptr) dl[((long long)b * Kp + c) * Tp + t] = (float)d;
      }
  }
  if (ws != nullptr) {
    loss_f = block_sum_d(loss_f, s_d);
    loss_c = block_sum_d(loss_c, s_d);
    if (tid == 0) {
      ws[c] = loss_f;
      ws[K + c] = loss_c;
      if (c == 0) ws[2 * (long long)K] = Nf;
    }
  }
  if (dbias != nullptr) {
    db = block_sum_d(db, s_d);
    if (tid == 0) dbias[c] = (float)db;
  }
}

// sums += (L_f + weak_weight L_c, L_f, L_c): thread t adds the classes t, t + 256, ... in order
__global__ __launch_bounds__(kThreads) void weak_frame_bce_sum_kernel(const double* __restrict__ ws, int B, int K,
                                                                      float weak_weight, float* __restrict__ sums) {
  __shared__ double s_d[4];
  double af = 0.0, ac = 0.0;
  for (int c = threadIdx.x; c < K; c += kThreads) af += ws[c], ac += ws[K + c];
  af = block_sum_d(af, s_d);
  ac = block_sum_d(ac, s_d);
  if (threadIdx.x != 0) return;
  const double Nf = ws[2 * (long long)K];
  const double Lf = Nf > 0.0 ? af / Nf : 0.0, Lc = ac / ((double)B * (double)K);
  sums[0] += (float)(Lf + (double)weak_weight * Lc);
  sums[1] += (float)Lf;
  sums[2] += (float)Lc;
}

}  // namespace

extern "C" int eat_sed_clip_targets(const int* events, long long n_events, const long long* event_offsets, const int* lengths,
                                    long long n_bank, int K, const int* idx, const int* start, const float* mix,
                                    const unsigned char* strong, int B, int L, float* w, int* framed, eat_stream_t stream) {
  eat::clear_stale_error();
  if (!event_offsets || !lengths || !idx || !start || !mix || !w || !framed || (!events && n_events != 0))
    return eat::fail(EAT_EINVAL, "eat_sed_clip_targets: missing operand");
  if (B < 1 || K < 1 || L < 1 || n_bank < 1 || n_events < 0)
    return eat::fail(EAT_EINVAL, "eat_sed_clip_targets: need B, K, L, n_bank >= 1 and n_events >= 0 (got B=%d K=%d L=%d "
                     "n_bank=%lld n_events=%lld)", B, K, L, n_bank, n_events);
  const long long bx = ((long long)B * K + kThreads - 1) / kThreads;
  if (bx > 0x7fffffffLL) return eat::fail(EAT_EINVAL, "eat_sed_clip_targets: B=%d x K=%d exceeds the grid", B, K);
  hipLaunchKernelGGL(sed_clip_targets_kernel, dim3((unsigned)bx), dim3(kThreads), 0, (hipStream_t)stream, events, n_events,
                     event_offsets, lengths, n_bank, K, idx, start, mix, strong, B, L, w, framed);
  return eat::check_launch("eat_sed_clip_targets");
}

extern "C" int eat_weak_frame_bce_fwd_bwd(const float* z, const float* y, const float* w, const int* framed, const int* perm,
                                          const float* lam, float weak_weight, float eps, int B, int K, int T, int Tp, int Kp,
                                          float* sums, float* dlogits, float* dbias, float* clip_prob, double* ws,
                                          eat_stream_t stream) {
  eat::clear_stale_error();
  if (!z || !y || !w || !framed)
    return eat::fail(EAT_EINVAL, "eat_weak_frame_bce_fwd_bwd: missing operand (z, y, w and framed are required)");
  if ((perm == nullptr) != (lam == nullptr)) return eat::fail(EAT_EINVAL, "eat_weak_frame_bce_fwd_bwd: perm and lam go together");
  if (sums && !ws) return eat::fail(EAT_EINVAL, "eat_weak_frame_bce_fwd_bwd: missing operand (sums need the workspace ws)");
  if (B < 1 || K < 1 || T < 1 || Tp < T || Kp < K)
    return eat::fail(EAT_EINVAL, "eat_weak_frame_bce_fwd_bwd: need B, K, T >= 1, Tp >= T and Kp >= K (got B=%d K=%d T=%d Tp=%d "
                     "Kp=%d)", B, K, T, Tp, Kp);
  if (!(weak_weight >= 0.0f) || !(weak_weight <= 3.402823466e38f))
    return eat::fail(EAT_EINVAL, "eat_weak_frame_bce_fwd_bwd: weak_weight must be finite and not negative (got %g)",
                     (double)weak_weight);
  if (!(eps > 0.0f) || !(eps < 0.5f))
    return eat::fail(EAT_EINVAL, "eat_weak_frame_bce_fwd_bwd: eps must lie in (0, 0.5) (got %g)", (double)eps);
  hipStream_t s = (hipStream_t)stream;
  if (sums || dlogits || dbias || clip_prob) {
    const dim3 grid((unsigned)(dlogits ? Kp : K));
    double* wsp = sums ? ws : (double*)nullptr;
    if (T <= 32)
      hipLaunchKernelGGL(weak_frame_bce_kernel<32>, grid, dim3(kThreads), 0, s, z, y, w, framed, perm, lam, weak_weight, eps, B, K,
                         T, Tp, Kp, dlogits, dbias, clip_prob, wsp);
    else
      hipLaunchKernelGGL(weak_frame_bce_kernel<64>, grid, dim3(kThreads), 0, s, z, y, w, framed, perm, lam, weak_weight, eps, B, K,
                         T, Tp, Kp, dlogits, dbias, clip_prob, wsp);
  }
  if (sums) hipLaunchKernelGGL(weak_frame_bce_sum_kernel, dim3(1), dim3(kThreads), 0, s, ws, B, K, weak_weight, sums);
  return eat::check_launch("eat_weak_frame_bce_fwd_bwd");
}
