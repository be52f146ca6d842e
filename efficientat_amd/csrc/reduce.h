// The fixed-order sums behind "the same bits on every call": an xor butterfly over a wave; the block sums assume EXACTLY 256
// threads (four waves, added as ((s[0] + s[1]) + s[2]) + s[3]) and must be reached by every thread of the block.
#pragma once
#include <hip/hip_runtime.h>

namespace eat {

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ long long wave_sum_ll(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over the block in a fixed order (every thread receives it); s: 4 values of LDS, free to reuse after the call
__device__ __forceinline__ double block_sum_d(double v, double* s) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  const double r = ((s[0] + s[1]) + s[2]) + s[3];
  __syncthreads();
  return r;
}
__device__ __forceinline__ long long block_sum_ll(long long v, long long* s) {
  v = wave_sum_ll(v);
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  const long long r = s[0] + s[1] + s[2] + s[3];
  __syncthreads();
  return r;
}

}  // namespace eat
