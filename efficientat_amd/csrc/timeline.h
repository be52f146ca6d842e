// The recording table of the detector's timelines, (n_rec, 4) int32 rows (first, count, goff, G), for detect.hip / median_bank.hip
#pragma once
#include <hip/hip_runtime.h>

namespace eat {

struct Rec { int first, count, goff, G; };

__device__ __forceinline__ Rec load_rec(const int* __restrict__ rec, int r) {
  const int4 v = *reinterpret_cast<const int4*>(rec + 4 * (long long)r);
  return Rec{v.x, v.y, v.z, v.w};
}

// the last recording whose goff is <= c (goff ascending, goff[0] = 0)
__device__ __forceinline__ int find_rec(const int* __restrict__ rec, int n_rec, int c) {
  int lo = 0, hi = n_rec - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (rec[4 * (long long)mid + 2] <= c) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// periodic reflection of index j about the ends of [0, G)
__device__ __forceinline__ int reflect(long long j, int G) {
  const long long P = 2LL * G;
  long long u = j % P;
  if (u < 0) u += P;
  return (int)(u < G ? u : P - 1 - u);
}

}  // namespace eat
