// Device side of PSDS counting (include/eat_psds.h): the detector's events of every (recording, class) timeline at a whole
// grid of threshold pairs, judged on the fly against the reference events by the three intersection criteria of the
// polyphonic sound detection score, as integer counts.  What psds_eval does on the host with one pass per threshold.
//
// Geometry.  That of event_score.hip: one wavefront (= one block) takes one timeline and 64 threshold pairs, one pair per
// lane, and walks the timeline with event_walk.h.  The class's reference rows (at most 64) sit in LDS, and next to them one
// int32 coverage counter per (row, lane), laid out [row][lane] so that the lanes of a wave hit distinct banks: the relevant
// detections of one lane are disjoint, so a row's coverage never exceeds its length.  A lane whose detection fails the
// detection criterion walks the recording's rows of the other classes straight from global memory: they are sorted by class,
// so one running sum per class run is all the state it needs.
#include "eat_common.h"
#include "event_walk.h"
#include "../../include/eat_psds.h"

namespace {

constexpr int kMaxRef = EAT_PSDS_MAX_REF;
constexpr int kGridY = 65535;
// Reference rows are int32, so a sum of intersections over one class's 64 rows stays below 2^37 and 1000 times it below
// 2^47: a detection longer than 2^50 samples meets no ratio of at least 1 per mille, and pm L is not formed for it.
constexpr long long kMaxLen = 1LL << 50;

// 1000 S >= pm L for a length L > 0, without overflow
__device__ __forceinline__ bool meets(long long S, int pm, long long L) {
  return L > 0 && L <= kMaxLen && 1000LL * S >= (long long)pm * L;
}

__device__ __forceinline__ long long overlap(long long on, long long off, int r_on, int r_off) {
  return min(off, (long long)r_off) - max(on, (long long)r_on);   // (not clamped: the callers keep what is > 0)
}

__global__ __launch_bounds__(64) void psds_count_kernel(const float* __restrict__ filt, int K, int G_total,
                                                        const int* __restrict__ rec, const long long* __restrict__ nsamp, int R,
                                                        const int* __restrict__ ref, const long long* __restrict__ ro, int n_ref,
                                                        int dtc_pm, int gtc_pm, int cttc_pm, const float* __restrict__ hi_v,
                                                        const float* __restrict__ lo_v, int V, int max_gap, int min_len,
                                                        int* __restrict__ counts, int* __restrict__ ct) {
  __shared__ int s_on[kMaxRef], s_off[kMaxRef];
  __shared__ int s_cov[kMaxRef][64];
  const int lane = threadIdx.x;
  const long long tl = blockIdx.x;
  const int i = (int)(tl / K), k = (int)(tl - (long long)i * K);
  const int v = (int)blockIdx.y * 64 + lane;
  const bool live = v < V;
  const int goff = rec[4 * (long long)i + 2];
  const int G = goff < 0 ? 0 : max(0, min(rec[4 * (long long)i + 3], G_total - goff));
  const float* x = filt + (long long)k * G_total + goff;
  const long long n_i = nsamp[i];

  // the recording's rows [a, b) and among them those of class k: two bisections, wave-uniform
  const long long a = min(max(ro[i], 0LL), (long long)n_ref), b = min(max(ro[i + 1], a), (long long)n_ref);
  const long long b0 = eat::first_row_of_class(ref, a, b, k);
  const int nref = (int)min(eat::first_row_of_class(ref, a, b, k + 1) - b0, (long long)kMaxRef);
  if (lane < nref) {
    s_on[lane] = ref[3 * (b0 + lane) + 1];
    s_off[lane] = ref[3 * (b0 + lane) + 2];
  }
  for (int j = 0; j < nref; ++j) s_cov[j][lane] = 0;       // only the rows in use; a lane reads its own column alone
  __syncthreads();

  const float inf = __builtin_huge_valf();
  const float hi = live ? hi_v[v] : inf, lo = live ? lo_v[v] : inf;       // a lane without a pair never sees an active frame
  int n_det = 0, fp = 0, n_ct = 0;

  eat::event_walk(x, G, hi, lo, max_gap, min_len, [&](int on, int off) {
    ++n_det;
    const long long on_s = (long long)on * R;
    const long long off_s = min((long long)off * R, n_i);
    const long long L = off_s - on_s;
    long long S = 0;
    for (int j = 0; j < nref; ++j) {
      if ((long long)s_on[j] >= off_s) break;              // (sorted by onset: nor does any later row overlap)
      S += max(0LL, overlap(on_s, off_s, s_on[j], s_off[j]));
    }
    if (meets(S, dtc_pm, L)) {
      for (int j = 0; j < nref; ++j) {
        if ((long long)s_on[j] >= off_s) break;
        const long long I = overlap(on_s, off_s, s_on[j], s_off[j]);
        if (I > 0) s_cov[j][lane] += (int)I;               // I <= the row's length < 2^31
      }
      return;
    }
    ++fp;
    if (cttc_pm == 0 || L <= 0) return;
    // the other classes' rows: one running sum per class run, judged where the run ends
    int cls = -1;
    long long Sc = 0;
    auto judge = [&]() {
      if (cls >= 0 && cls < K && cls != k && meets(Sc, cttc_pm, L)) {
        atomicAdd(ct + ((long long)v * K + k) * K + cls, 1);
        ++n_ct;
      }
    };
    for (long long e = a; e < b; ++e) {
      if (e == b0 && nref > 0) {                           // skip class k's own rows
        e = b0 + nref - 1;
        continue;
      }
      const int c = ref[3 * e];
      if (c != cls) {
        judge();
        cls = c;
        Sc = 0;
      }
      Sc += max(0LL, overlap(on_s, off_s, ref[3 * e + 1], ref[3 * e + 2]));
    }
    judge();
  });

  if (live) {
    int tp = 0;
    for (int j = 0; j < nref; ++j) {
      const long long Lr = (long long)s_off[j] - s_on[j];
      if (meets(s_cov[j][lane], gtc_pm, Lr)) ++tp;
    }
    int4* out = reinterpret_cast<int4*>(counts) + (tl * V + v);
    *out = make_int4(tp, n_det, fp, n_ct);
  }
}

}  // namespace

extern "C" int eat_psds_count(const float* filt, int K, int G_total, const int* rec, int n_rec, const long long* nsamp, int R,
                              const int* ref, const long long* ro, int n_ref, int dtc_pm, int gtc_pm, int cttc_pm,
                              const float* hi, const float* lo, int V, int max_gap, int min_len, int* counts, int* ct,
                              eat_stream_t stream) {
  eat::clear_stale_error();
  const char* fn = "eat_psds_count";
  if (!filt || !rec || !nsamp || !ro || !hi || !lo || !counts || (n_ref > 0 && !ref))
    return eat::fail(EAT_EINVAL, "%s: missing operand", fn);
  if (K < 1 || n_rec < 1 || G_total < 1 || R < 1 || V < 1)
    return eat::fail(EAT_EINVAL, "%s: need K, n_rec, G_total, R, V >= 1 (got %d, %d, %d, %d, %d)", fn, K, n_rec, G_total, R, V);
  if (n_ref < 0 || max_gap < 0 || min_len < 0)
    return eat::fail(EAT_EINVAL, "%s: need n_ref, max_gap, min_len >= 0 (got %d, %d, %d)", fn, n_ref, max_gap, min_len);
  if (dtc_pm < 1 || dtc_pm > 1000 || gtc_pm < 1 || gtc_pm > 1000)
    return eat::fail(EAT_EINVAL, "%s: dtc_pm=%d and gtc_pm=%d must lie in [1, 1000] per mille", fn, dtc_pm, gtc_pm);
  if (cttc_pm < 0 || cttc_pm > 1000) return eat::fail(EAT_EINVAL, "%s: cttc_pm=%d must lie in [0, 1000] per mille", fn, cttc_pm);
  if (cttc_pm > 0 && !ct) return eat::fail(EAT_EINVAL, "%s: cttc_pm=%d needs the cross-trigger buffer ct", fn, cttc_pm);
  if ((long long)n_rec * K > 0x7fffffffLL)
    return eat::fail(EAT_EINVAL, "%s: n_rec=%d x K=%d timelines exceed the grid limit of 2147483647", fn, n_rec, K);
  if (V > 64 * kGridY) return eat::fail(EAT_EINVAL, "%s: V=%d threshold pairs exceed %d", fn, V, 64 * kGridY);
  const dim3 grid((unsigned)n_rec * (unsigned)K, (unsigned)((V + 63) / 64));
  hipLaunchKernelGGL(psds_count_kernel, grid, dim3(64), 0, (hipStream_t)stream, filt, K, G_total, rec, nsamp, R, ref, ro, n_ref,
                     dtc_pm, gtc_pm, cttc_pm, hi, lo, V, max_gap, min_len, counts, ct);
  return eat::check_launch(fn);
}
