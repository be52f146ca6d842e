// What the fp32 scan (search.hip) and the int8 scan (search_q8.hip) share: the order of results, the running top-k list
// of a query in LDS, the stage-2 merge of the blocks' lists, and the sum of squares behind eat_rows_normalize.  All of it
// works on fp32 scores and int32 row indices, whatever produced the scores.
//
// Everything sits in an unnamed namespace on purpose: each file that includes this header gets kernels of its own, in its
// own code object.
#pragma once
#include <cstdint>

#include "eat_common.h"

namespace eat {
namespace {

// LDS written by one lane of the wavefront is read by another: order the two (no barrier instruction is needed inside a wave)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the order of results: larger score first, equal scores by ascending index; the pad (-inf, -1) is last of all
__device__ __forceinline__ bool better(float s, int i, float ts, int ti) {
  return s > ts || (s == ts && (unsigned)i < (unsigned)ti);
}

// (s, i) into the sorted list (ls, li) of k entries, whose last entry it beats; the whole wavefront calls it
__device__ __forceinline__ void list_insert(float* ls, int* li, int k, float s, int i, int lane) {
  const int i0 = lane, i1 = lane + 64;
  const bool a0 = i0 < k && better(ls[i0], li[i0], s, i);
  const bool a1 = i1 < k && better(ls[i1], li[i1], s, i);
  const int pos = __popcll(__ballot(a0)) + __popcll(__ballot(a1));        // entries ahead of (s, i); pos <= k - 1
  float s0 = 0.0f, s1 = 0.0f;
  int j0 = 0, j1 = 0;
  if (i0 < k && i0 > pos) { s0 = ls[i0 - 1]; j0 = li[i0 - 1]; }
  if (i1 < k && i1 > pos) { s1 = ls[i1 - 1]; j1 = li[i1 - 1]; }
  wave_sync();
  if (i0 < k && i0 > pos) { ls[i0] = s0; li[i0] = j0; }
  if (i1 < k && i1 > pos) { ls[i1] = s1; li[i1] = j1; }
  if (i0 == pos) { ls[i0] = s; li[i0] = i; }
  if (i1 == pos) { ls[i1] = s; li[i1] = i; }
  wave_sync();
}

// Up to 64 consecutive rows from row0 on, lane j holding the score s of row row0 + j and whether it is eligible, offered to
// the list (ls, li) that this wavefront owns: a score enters only if it beats the list's last entry, in ascending row.
__device__ __forceinline__ void list_offer(float* ls, int* li, int k, float s, long long row0, bool eligible, int lane) {
  unsigned long long pass = __ballot(eligible && better(s, (int)(row0 + lane), ls[k - 1], li[k - 1]));
  while (pass != 0) {                                               // wave-uniform; ascending row
    const int j = __ffsll((long long)pass) - 1;
    pass &= pass - 1;
    const float cs = __shfl(s, j, 64);
    const int ci = (int)(row0 + j);
    if (better(cs, ci, ls[k - 1], li[k - 1])) list_insert(ls, li, k, cs, ci, lane);
  }
}

// one block of NB threads per query of the group: score / index (Qg, k) from ws [Qg][NB][k], each list sorted.  Thread t
// holds the head of block t's list; k rounds of a block-wide arg-max pop the final order.
template <int NB>
__global__ __launch_bounds__(NB) void search_merge_kernel(const float* __restrict__ ws_s, const int* __restrict__ ws_i, int k,
                                                          float* __restrict__ score, int* __restrict__ index) {
  __shared__ float w_s[2][NB / 64];
  __shared__ int w_i[2][NB / 64], w_t[2][NB / 64];
  const int g = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const size_t base = ((size_t)g * NB + tid) * k;
  int head = 0;
  float s = ws_s[base];
  int i = ws_i[base];
  for (int r = 0; r < k; ++r) {
    float bs = s;
    int bi = i, bt = tid;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float os = __shfl_xor(bs, o, 64);
      const int oi = __shfl_xor(bi, o, 64), ot = __shfl_xor(bt, o, 64);
      if (better(os, oi, bs, bi) || (os == bs && oi == bi && ot < bt)) { bs = os; bi = oi; bt = ot; }
    }
    const int p = r & 1;                                              // slots of round r are rewritten in round r + 2,
    if (lane == 0) { w_s[p][wave] = bs; w_i[p][wave] = bi; w_t[p][wave] = bt; }      // past the barrier of round r + 1
    __syncthreads();
    bs = w_s[p][0]; bi = w_i[p][0]; bt = w_t[p][0];
#pragma unroll
    for (int w = 1; w < NB / 64; ++w)
      if (better(w_s[p][w], w_i[p][w], bs, bi)) { bs = w_s[p][w]; bi = w_i[p][w]; bt = w_t[p][w]; }      // ties: the lower wave
    if (tid == 0) {
      score[(size_t)g * k + r] = bs;
      index[(size_t)g * k + r] = bi;
    }
    if (tid == bt) {                                                  // pop the winner's list
      ++head;
      s = head < k ? ws_s[base + head] : -INFINITY;
      i = head < k ? ws_i[base + head] : -1;
    }
  }
}

// sum_d r[d]^2 of one row by one wavefront, every lane receiving it: lane l takes elements 4 l + 256 i .. + 3 in ascending
// d with one fmaf each, then the 64 lanes are summed by one fixed butterfly.  VEC: 16-byte loads (D % 4 == 0, an aligned
// row); the 4-byte path adds the same elements per lane in the same order: the same bits.
template <bool VEC>
__device__ __forceinline__ float row_sumsq(const float* r, unsigned D, int lane) {
  float ss = 0.0f;
  if constexpr (VEC) {
    for (unsigned d = 4u * lane; d < D; d += 256) {
      const float4 v = *reinterpret_cast<const float4*>(r + d);
      ss = __builtin_fmaf(v.x, v.x, ss);
      ss = __builtin_fmaf(v.y, v.y, ss);
      ss = __builtin_fmaf(v.z, v.z, ss);
      ss = __builtin_fmaf(v.w, v.w, ss);
    }
  } else {
    for (unsigned d = 4u * lane; d < D; d += 256)
      for (unsigned j = d; j < min(d + 4u, D); ++j) ss = __builtin_fmaf(r[j], r[j], ss);
  }
  return eat::wave_sum(ss);
}

}  // namespace
}  // namespace eat
