// The width-bank median of sound event detection (include/eat_median_bank.h): the running median of detect.hip's
// detect_median_kernel for Mw widths per class in one launch.  Tuning the detector's median per class (sed.py:
// tune_postprocessing) tries a grid of widths on the same timelines; per-class widths in `detect` are the Mw = 1 case.
//
// Geometry: detect_median_kernel's.  Lanes along time, 256 columns per block, classes on grid.y, one tile piece per
// recording that the block's columns touch.  The piece and the reflected halo of the WIDEST width the class has in the bank
// are staged in LDS once; every slice then ranks by counting inside that one staging, its own window centred in it.  The
// width of a (slice, class) is the same in every thread of the block, so every trip count and barrier is block-uniform.
#include "eat_common.h"
#include "timeline.h"
#include "../../include/eat_median_bank.h"

namespace {

constexpr int kTile = 256;            // columns per block
constexpr int kMaxM = 31;             // widest median
constexpr int kGridY = 65535;

using eat::find_rec, eat::load_rec, eat::Rec, eat::reflect;

// the width the kernel uses for a table entry: odd and in [1, kMaxM] whatever the entry holds (the host refuses others)
__device__ __forceinline__ int safe_width(int w) { return min(max(w, 1), kMaxM) | 1; }

__global__ __launch_bounds__(kTile) void detect_median_bank_kernel(const float* __restrict__ x, int K, int G_total,
                                                                   const int* __restrict__ rec, int n_rec,
                                                                   const int* __restrict__ widths, int Mw,
                                                                   float* __restrict__ y) {
  __shared__ float s[kTile + kMaxM - 1];
  const int tid = threadIdx.x;
  const long long c0 = (long long)blockIdx.x * kTile;
  const int c1 = (int)min(c0 + kTile, (long long)G_total);
  const int r0 = find_rec(rec, n_rec, (int)c0);
  for (int k = blockIdx.y; k < K; k += gridDim.y) {
    const float* xr = x + (long long)k * G_total;
    int hw = 0;                                            // half of the class's widest width: hw <= kMaxM / 2
    for (int j = 0; j < Mw; ++j) hw = max(hw, safe_width(widths[(long long)j * K + k]) >> 1);
    // every trip count below is the same in all threads of the block: the barriers are not divergent
    for (int ri = r0; ri < n_rec; ++ri) {
      const Rec r = load_rec(rec, ri);
      if (r.goff >= c1) break;
      const int G = min(r.G, G_total - r.goff);
      const int a = max((int)c0, r.goff), b = min(c1, r.goff + G);
      const int n = b - a;                                 // outputs of this piece: n <= kTile, n + 2 hw <= the array
      if (n < 1) continue;
      for (int e = tid; e < n + 2 * hw; e += kTile) s[e] = xr[r.goff + reflect((long long)(a - r.goff) - hw + e, G)];
      __syncthreads();
      if (tid < n) {
        for (int j = 0; j < Mw; ++j) {
          const int m = safe_width(widths[(long long)j * K + k]), h = m >> 1;
          const float* w = s + tid + (hw - h);             // the m samples of this output: w[0 .. m), all inside s
          // the element of rank h in the order (value, position): for each candidate count the samples before it
          float res = w[h];
          for (int i = 0; i < m; ++i) {
            const float v = w[i];
            int before = 0;
            for (int q = 0; q < m; ++q) {
              const float u = w[q];
              before += (u < v || (u == v && q < i)) ? 1 : 0;
            }
            if (before == h) res = v;
          }
          y[((long long)j * K + k) * G_total + a + tid] = res;
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace

extern "C" int eat_detect_median_bank(const float* prob, int K, int G_total, const int* rec, int n_rec, const int* widths,
                                      int Mw, float* filt, eat_stream_t stream) {
  eat::clear_stale_error();
  if (!prob || !rec || !widths || !filt) return eat::fail(EAT_EINVAL, "eat_detect_median_bank: missing operand");
  if (prob == filt) return eat::fail(EAT_EINVAL, "eat_detect_median_bank: filt must not be prob");
  if (K < 1 || n_rec < 1 || G_total < 1 || Mw < 1)
    return eat::fail(EAT_EINVAL, "eat_detect_median_bank: need K, n_rec, G_total, Mw >= 1 (got %d, %d, %d, %d)", K, n_rec,
                     G_total, Mw);
  const dim3 grid((unsigned)(((long long)G_total + kTile - 1) / kTile), (unsigned)(K < kGridY ? K : kGridY));
  hipLaunchKernelGGL(detect_median_bank_kernel, grid, dim3(kTile), 0, (hipStream_t)stream, prob, K, G_total, rec, n_rec, widths,
                     Mw, filt);
  return eat::check_launch("eat_detect_median_bank");
}
