// Device side of event-based (collar) scoring (include/eat_event_score.h): the detector's events of every (recording,
// class) timeline at a whole grid of threshold pairs, matched on the fly against the reference events, as integer counts.
// What a DCASE-style evaluation does on the host with one pass of sed_eval per threshold.
//
// Geometry.  One wavefront (= one block) takes one timeline and 64 threshold pairs, one pair per lane.  The timeline is
// loaded 64 frames at a time with one coalesced load and handed round by lane broadcast; each lane runs the run / merge /
// drop state machine of detect.hip's events kernel frame by frame on its own pair and matches an event the moment it is
// final (the walk of event_walk.h, shared with psds.hip).  The timeline's reference rows (at most 64) sit in LDS; a lane keeps a
// taken-mask over them.
#include "eat_common.h"
#include "event_walk.h"
#include "../../include/eat_event_score.h"

namespace {

constexpr int kMaxRef = EAT_EVENT_SCORE_MAX_REF;          // = bits of the taken-mask
constexpr int kGridY = 65535;

__global__ __launch_bounds__(64) void event_score_kernel(const float* __restrict__ filt, int K, int G_total,
                                                         const int* __restrict__ rec, const long long* __restrict__ nsamp,
                                                         int R, const int* __restrict__ ref, const int* __restrict__ ref_tol,
                                                         const long long* __restrict__ ro, int n_ref, int c,
                                                         const float* __restrict__ hi_v, const float* __restrict__ lo_v, int V,
                                                         int max_gap, int min_len, int* __restrict__ counts) {
  __shared__ int s_on[kMaxRef], s_off[kMaxRef], s_tol[kMaxRef];
  const int lane = threadIdx.x;
  const long long tl = blockIdx.x;
  const int i = (int)(tl / K), k = (int)(tl - (long long)i * K);
  const int v = (int)blockIdx.y * 64 + lane;
  const bool live = v < V;
  const int goff = rec[4 * (long long)i + 2];
  const int G = goff < 0 ? 0 : max(0, min(rec[4 * (long long)i + 3], G_total - goff));
  const float* x = filt + (long long)k * G_total + goff;
  const long long n_i = nsamp[i];

  // the rows of class k among the recording's rows [a, b), sorted by (class, onset): two bisections, wave-uniform
  const long long a = min(max(ro[i], 0LL), (long long)n_ref), b = min(max(ro[i + 1], a), (long long)n_ref);
  const long long b0 = eat::first_row_of_class(ref, a, b, k);
  const int nref = (int)min(eat::first_row_of_class(ref, a, b, k + 1) - b0, (long long)kMaxRef);
  if (lane < nref) {
    s_on[lane] = ref[3 * (b0 + lane) + 1];
    s_off[lane] = ref[3 * (b0 + lane) + 2];
    s_tol[lane] = ref_tol[b0 + lane];
  }
  __syncthreads();

  const float inf = __builtin_huge_valf();
  const float hi = live ? hi_v[v] : inf, lo = live ? lo_v[v] : inf;       // a lane without a pair never sees an active frame
  int n_est = 0, tp = 0, first = 0;                        // references before `first` start too early for what follows
  unsigned long long taken = 0;

  eat::event_walk(x, G, hi, lo, max_gap, min_len, [&](int on, int off) {
    ++n_est;
    const long long on_s = (long long)on * R;
    const long long off_s = min((long long)off * R, n_i);
    while (first < nref && (long long)s_on[first] < on_s - c) ++first;
    for (int j = first; j < nref; ++j) {
      if ((long long)s_on[j] > on_s + c) break;            // (sorted by onset: nor does any later row match)
      if ((taken >> j) & 1ULL) continue;
      const long long d = (long long)s_off[j] - off_s;
      if ((d < 0 ? -d : d) <= (long long)s_tol[j]) {
        taken |= 1ULL << j;
        ++tp;
        break;
      }
    }
  });
  if (live) {
    int2* out = reinterpret_cast<int2*>(counts) + (tl * V + v);
    *out = make_int2(tp, n_est);
  }
}

}  // namespace

extern "C" int eat_event_score(const float* filt, int K, int G_total, const int* rec, int n_rec, const long long* nsamp, int R,
                               const int* ref, const int* ref_tol, const long long* ro, int n_ref, int c, const float* hi,
                               const float* lo, int V, int max_gap, int min_len, int* counts, eat_stream_t stream) {
  eat::clear_stale_error();
  const char* fn = "eat_event_score";
  if (!filt || !rec || !nsamp || !ro || !hi || !lo || !counts || (n_ref > 0 && (!ref || !ref_tol)))
    return eat::fail(EAT_EINVAL, "%s: missing operand", fn);
  if (K < 1 || n_rec < 1 || G_total < 1 || R < 1 || V < 1)
    return eat::fail(EAT_EINVAL, "%s: need K, n_rec, G_total, R, V >= 1 (got %d, %d, %d, %d, %d)", fn, K, n_rec, G_total, R, V);
  if (n_ref < 0 || c < 0 || max_gap < 0 || min_len < 0)
    return eat::fail(EAT_EINVAL, "%s: need n_ref, c, max_gap, min_len >= 0 (got %d, %d, %d, %d)", fn, n_ref, c, max_gap, min_len);
  if ((long long)n_rec * K > 0x7fffffffLL)
    return eat::fail(EAT_EINVAL, "%s: n_rec=%d x K=%d timelines exceed the grid limit of 2147483647", fn, n_rec, K);
  if (V > 64 * kGridY) return eat::fail(EAT_EINVAL, "%s: V=%d threshold pairs exceed %d", fn, V, 64 * kGridY);
  const dim3 grid((unsigned)n_rec * (unsigned)K, (unsigned)((V + 63) / 64));
  hipLaunchKernelGGL(event_score_kernel, grid, dim3(64), 0, (hipStream_t)stream, filt, K, G_total, rec, nsamp, R, ref, ref_tol, ro,
                     n_ref, c, hi, lo, V, max_gap, min_len, counts);
  return eat::check_launch(fn);
}
