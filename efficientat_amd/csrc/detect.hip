// Device side of sound event detection (include/eat_detect.h): the frame-level logits of overlapping windows become one
// probability timeline per recording and class (stitch), the timeline is median-filtered per recording (median) and
// binarised with two thresholds into a sorted event list (events: count, then write).  What DCASE-style post-processing
// does on the host with scipy.ndimage.median_filter and a Python loop over the classes.
//
// Geometry.  The timelines are (K, G_total) with all recordings of a call side by side along the time axis; a column's
// recording is found by bisection over the recording table's goff column (wave-uniform wherever a tile lies inside one
// recording).  stitch and median run lanes along time, 256 columns per block, classes on grid.y: loads of p and of prob
// and every store are contiguous.  median keeps the tile plus its reflected halo in LDS, one tile piece per recording
// that the block's columns touch, and ranks by counting.  events gives one wavefront (= one block) a whole timeline and
// walks it 64 frames per step on ballot masks; everything it carries from step to step is wave-uniform.
#include "eat_common.h"
#include "loss_terms.h"
#include "timeline.h"
#include "../../include/eat_detect.h"

namespace {

constexpr int kTile = 256;            // columns per block of stitch / median
constexpr int kMaxM = 31;             // widest median
constexpr int kGridY = 65535;

using eat::find_rec, eat::load_rec, eat::Rec, eat::reflect;

__global__ __launch_bounds__(kTile) void detect_stitch_kernel(const float* __restrict__ p, int n_w, int K, int Tp,
                                                              const int* __restrict__ rec, int n_rec, int Hf, int T,
                                                              const float* __restrict__ wt, float* __restrict__ prob,
                                                              int G_total) {
  const long long c = (long long)blockIdx.x * kTile + threadIdx.x;
  if (c >= G_total) return;
  const Rec r = load_rec(rec, find_rec(rec, n_rec, (int)c));
  const int g = (int)c - r.goff;
  // windows q with 0 <= g - q Hf < T
  int q_lo = g - T + 1 <= 0 ? 0 : (g - T + Hf) / Hf;
  int q_hi = min(g / Hf, r.count - 1);
  if (g < 0 || g >= r.G) q_hi = -1;                        // (a table that does not tile the axis: store zeros)
  q_hi = min(q_hi, n_w - 1 - r.first);                     // never a row outside p
  if (r.first < 0) q_hi = -1;
  for (int k = blockIdx.y; k < K; k += gridDim.y) {
    float num = 0.0f, den = 0.0f;
    for (int q = q_lo; q <= q_hi; ++q) {
      const int j = g - q * Hf;
      const float w = wt[j];
      num += w * eat::sigmoid(p[((long long)(r.first + q) * K + k) * Tp + j]);
      den += w;
    }
    prob[(long long)k * G_total + c] = q_hi >= q_lo ? num / den : 0.0f;
  }
}

__global__ __launch_bounds__(kTile) void detect_median_kernel(const float* __restrict__ x, int K, int G_total,
                                                              const int* __restrict__ rec, int n_rec, int m,
                                                              float* __restrict__ y) {
  __shared__ float s[kTile + kMaxM - 1];
  const int tid = threadIdx.x, h = m >> 1;
  const long long c0 = (long long)blockIdx.x * kTile;
  const int c1 = (int)min(c0 + kTile, (long long)G_total);
  const int r0 = find_rec(rec, n_rec, (int)c0);
  for (int k = blockIdx.y; k < K; k += gridDim.y) {
    const float* xr = x + (long long)k * G_total;
    float* yr = y + (long long)k * G_total;
    // every trip count below is the same in all threads of the block: the barriers are not divergent
    for (int ri = r0; ri < n_rec; ++ri) {
      const Rec r = load_rec(rec, ri);
      if (r.goff >= c1) break;
      const int G = min(r.G, G_total - r.goff);
      const int a = max((int)c0, r.goff), b = min(c1, r.goff + G);
      const int n = b - a;                                 // outputs of this piece
      if (n < 1) continue;
      for (int e = tid; e < n + 2 * h; e += kTile) s[e] = xr[r.goff + reflect((long long)(a - r.goff) - h + e, G)];
      __syncthreads();
      if (tid < n) {
        // the element of rank h in the order (value, position): for each candidate count the samples before it
        float res = s[tid + h];
        for (int i = 0; i < m; ++i) {
          const float v = s[tid + i];
          int before = 0;
          for (int j = 0; j < m; ++j) {
            const float u = s[tid + j];
            before += (u < v || (u == v && j < i)) ? 1 : 0;
          }
          if (before == h) res = v;
        }
        yr[a + tid] = res;
      }
      __syncthreads();
    }
  }
}

// One timeline per wavefront.  WRITE = false: count[tl] = number of events; WRITE = true: the events themselves.
template <bool WRITE>
__global__ __launch_bounds__(64) void detect_events_kernel(const float* __restrict__ filt, int K, int G_total,
                                                           const int* __restrict__ rec, int n_rec,
                                                           const float* __restrict__ hi_k, const float* __restrict__ lo_k,
                                                           int max_gap, int min_len, long long* __restrict__ count,
                                                           const long long* __restrict__ incl, int* __restrict__ ev_i,
                                                           float* __restrict__ ev_f) {
  const int lane = threadIdx.x;
  const long long tl = blockIdx.x;
  const int i = (int)(tl / K), k = (int)(tl - (long long)i * K);
  const Rec r = load_rec(rec, i);
  const int G = max(0, min(r.G, G_total - r.goff));
  const float* x = filt + (long long)k * G_total + r.goff;
  const float hi = hi_k[k], lo = lo_k[k];
  long long e = 0;                                         // row of the next event
  if constexpr (WRITE) e = tl == 0 ? 0 : incl[tl - 1];
  long long n_ev = 0;

  bool open = false, hit = false, cur = false;             // a run in progress; it has reached hi; a pending event
  int rs = 0, cur_on = 0, cur_off = 0;

  auto emit = [&](int on, int off) {
    if (off - on < min_len) return;
    if constexpr (WRITE) {
      float mx = x[on];
      for (int t = on + lane; t < off; t += 64) mx = fmaxf(mx, x[t]);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
      double sum = 0.0;                                    // in time order: lane after lane, chunk after chunk
      for (int t0 = on; t0 < off; t0 += 64) {
        const float v = t0 + lane < off ? x[t0 + lane] : 0.0f;
        const int n = min(64, off - t0);
        for (int l = 0; l < n; ++l) sum += (double)__shfl(v, l, 64);
      }
      if (lane == 0) {
        const long long row = e + n_ev;
        ev_i[4 * row] = i;
        ev_i[4 * row + 1] = k;
        ev_i[4 * row + 2] = on;
        ev_i[4 * row + 3] = off;
        ev_f[2 * row] = mx;
        ev_f[2 * row + 1] = (float)(sum / (double)(off - on));
      }
    }
    ++n_ev;
  };
  auto close_run = [&](int re) {                           // the run [rs, re) ends
    if (hit) {
      if (cur && rs - cur_off <= max_gap) {
        cur_off = re;
      } else {
        if (cur) emit(cur_on, cur_off);
        cur = true;
        cur_on = rs;
        cur_off = re;
      }
    }
    open = false;
  };

  for (int t0 = 0; t0 < G; t0 += 64) {
    const int t = t0 + lane;
    const float v = t < G ? x[t] : 0.0f;
    const unsigned long long A = __ballot(t < G && v >= lo);
    const unsigned long long H = __ballot(t < G && v >= hi);
    int pos = 0;                                           // bits below pos are dealt with; pos <= 63
    while (true) {
      if (!open) {
        const unsigned long long nxt = A & (~0ULL << pos);
        if (nxt == 0) break;
        pos = __ffsll((long long)nxt) - 1;
        open = true;
        hit = false;
        rs = t0 + pos;
      }
      const unsigned long long clr = ~A & (~0ULL << pos);
      const int end = clr != 0 ? __ffsll((long long)clr) - 1 : 64;        // the run covers bits [pos, end)
      const unsigned long long body = (end == 64 ? ~0ULL : ((1ULL << end) - 1)) & (~0ULL << pos);
      if ((H & body) != 0) hit = true;
      if (end == 64) break;                                // it goes on in the next step
      close_run(t0 + end);
      pos = end;
    }
  }
  if (open) close_run(G);
  if (cur) emit(cur_on, cur_off);
  if constexpr (!WRITE)
    if (lane == 0) count[tl] = n_ev;
}

}  // namespace

extern "C" int eat_detect_stitch(const float* p, int n_w, int K, int Tp, const int* rec, int n_rec, int Hf, int T,
                                 const float* wt, float* prob, int G_total, eat_stream_t stream) {
  eat::clear_stale_error();
  if (!p || !rec || !wt || !prob) return eat::fail(EAT_EINVAL, "eat_detect_stitch: missing operand");
  if (n_w < 1 || K < 1 || n_rec < 1 || T < 1 || Hf < 1 || G_total < 1 || Tp < T || Hf > T)
    return eat::fail(EAT_EINVAL, "eat_detect_stitch: need n_w, K, n_rec, G_total >= 1 and 1 <= Hf <= T <= Tp (got n_w=%d K=%d "
                     "n_rec=%d G_total=%d Hf=%d T=%d Tp=%d)", n_w, K, n_rec, G_total, Hf, T, Tp);
  const dim3 grid((unsigned)(((long long)G_total + kTile - 1) / kTile), (unsigned)(K < kGridY ? K : kGridY));
  hipLaunchKernelGGL(detect_stitch_kernel, grid, dim3(kTile), 0, (hipStream_t)stream, p, n_w, K, Tp, rec, n_rec, Hf, T, wt, prob,
                     G_total);
  return eat::check_launch("eat_detect_stitch");
}

extern "C" int eat_detect_median(const float* prob, int K, int G_total, const int* rec, int n_rec, int m, float* filt,
                                 eat_stream_t stream) {
  eat::clear_stale_error();
  if (!prob || !rec || !filt) return eat::fail(EAT_EINVAL, "eat_detect_median: missing operand");
  if (prob == filt) return eat::fail(EAT_EINVAL, "eat_detect_median: filt must not be prob");
  if (K < 1 || n_rec < 1 || G_total < 1)
    return eat::fail(EAT_EINVAL, "eat_detect_median: need K, n_rec, G_total >= 1 (got %d, %d, %d)", K, n_rec, G_total);
  if (m < 1 || m > kMaxM || m % 2 == 0)
    return eat::fail(EAT_EINVAL, "eat_detect_median: m=%d must be odd and lie in [1, %d]", m, kMaxM);
  const dim3 grid((unsigned)(((long long)G_total + kTile - 1) / kTile), (unsigned)(K < kGridY ? K : kGridY));
  hipLaunchKernelGGL(detect_median_kernel, grid, dim3(kTile), 0, (hipStream_t)stream, prob, K, G_total, rec, n_rec, m, filt);
  return eat::check_launch("eat_detect_median");
}

static int events_args(const char* fn, const void* filt, int K, int G_total, const void* rec, int n_rec, const void* hi,
                       const void* lo, int max_gap, int min_len, const void* a, const void* b, const void* c) {
  if (!filt || !rec || !hi || !lo || !a || !b || !c) return eat::fail(EAT_EINVAL, "%s: missing operand", fn);
  if (K < 1 || n_rec < 1 || G_total < 1)
    return eat::fail(EAT_EINVAL, "%s: need K, n_rec, G_total >= 1 (got %d, %d, %d)", fn, K, n_rec, G_total);
  if (max_gap < 0 || min_len < 0)
    return eat::fail(EAT_EINVAL, "%s: need max_gap, min_len >= 0 (got %d, %d)", fn, max_gap, min_len);
  if ((long long)n_rec * K > 0x7fffffffLL)
    return eat::fail(EAT_EINVAL, "%s: n_rec=%d x K=%d timelines exceed the grid limit of 2147483647", fn, n_rec, K);
  return EAT_OK;
}

extern "C" int eat_detect_events_count(const float* filt, int K, int G_total, const int* rec, int n_rec, const float* hi,
                                       const float* lo, int max_gap, int min_len, long long* count, eat_stream_t stream) {
  eat::clear_stale_error();
  const int rc = events_args("eat_detect_events_count", filt, K, G_total, rec, n_rec, hi, lo, max_gap, min_len, count, count,
                             count);
  if (rc != EAT_OK) return rc;
  hipLaunchKernelGGL(detect_events_kernel<false>, dim3((unsigned)n_rec * (unsigned)K), dim3(64), 0, (hipStream_t)stream, filt, K,
                     G_total, rec, n_rec, hi, lo, max_gap, min_len, count, (const long long*)nullptr, (int*)nullptr,
                     (float*)nullptr);
  return eat::check_launch("eat_detect_events_count");
}

extern "C" int eat_detect_events_write(const float* filt, int K, int G_total, const int* rec, int n_rec, const float* hi,
                                       const float* lo, int max_gap, int min_len, const long long* incl, int* ev_i, float* ev_f,
                                       eat_stream_t stream) {
  eat::clear_stale_error();
  const int rc = events_args("eat_detect_events_write", filt, K, G_total, rec, n_rec, hi, lo, max_gap, min_len, incl, ev_i, ev_f);
  if (rc != EAT_OK) return rc;
  hipLaunchKernelGGL(detect_events_kernel<true>, dim3((unsigned)n_rec * (unsigned)K), dim3(64), 0, (hipStream_t)stream, filt, K,
                     G_total, rec, n_rec, hi, lo, max_gap, min_len, (long long*)nullptr, incl, ev_i, ev_f);
  return eat::check_launch("eat_detect_events_write");
}
