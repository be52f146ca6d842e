// The fp32 cosine score of search.hip and match.hip: the loads of a row, the multiply-adds of a 256-float chunk, the
// transposing butterfly, and `scan_rows`, which puts them together for the R rows of a wavefront.  Both scans call the same code, so s[q, n] has the same bits in both: element d of a row always goes to lane
// (d / 4) % 64, the lane adds its elements in ascending d with one fmaf each, and the butterfly adds lanes in one fixed
// tree whatever the slot (row r, query g) of the sum.
//
// Everything sits in an unnamed namespace on purpose, as in search_topk.h.
#pragma once
#include <cstdint>

#include "eat_common.h"

namespace eat {
namespace {

constexpr int kChunk = 256;             // floats of a row that a wavefront takes per step: 64 lanes x 16 bytes
constexpr long long kLdsBytes = 160 * 1024;

// elements d .. d + 3 of a row (zeros from D on).  VEC: one 16-byte load (D % 4 == 0, 16-byte aligned rows).
// TAIL = false: the caller knows d + 3 < D.
template <bool VEC, bool TAIL>
__device__ __forceinline__ float4 load4(const float* __restrict__ row, unsigned d, unsigned D) {
  float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if constexpr (VEC) {
    if (!TAIL || d < D) v = *reinterpret_cast<const float4*>(row + d);
  } else {
    if (!TAIL || d < D) v.x = row[d];
    if (!TAIL || d + 1 < D) v.y = row[d + 1];
    if (!TAIL || d + 2 < D) v.z = row[d + 2];
    if (!TAIL || d + 3 < D) v.w = row[d + 3];
  }
  return v;
}

// sum (r, g) lives at acc[(r * G + g) / VH][(r * G + g) % VH]: halves of at most 64 sums, one transposing butterfly each
// sum (r, g) += b[r] . q_g[d .. d + 3], one fmaf per element in ascending d
template <int G, int R, int H, int VH, bool QLDS, bool TAIL>
__device__ __forceinline__ void fma_chunk(float (&acc)[H][VH], const float4 (&b)[R], const float* q_lds, unsigned Dp,
                                          const float* __restrict__ q_glb, unsigned d, unsigned D) {
#pragma unroll
  for (int g = 0; g < G; ++g) {
    float4 qv;
    if constexpr (QLDS) qv = *reinterpret_cast<const float4*>(q_lds + (size_t)g * Dp + d);
    else qv = load4<false, TAIL>(q_glb + (size_t)g * D, d, D);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      float a = acc[(r * G + g) / VH][(r * G + g) % VH];
      a = __builtin_fmaf(b[r].x, qv.x, a);
      a = __builtin_fmaf(b[r].y, qv.y, a);
      a = __builtin_fmaf(b[r].z, qv.z, a);
      a = __builtin_fmaf(b[r].w, qv.w, a);
      acc[(r * G + g) / VH][(r * G + g) % VH] = a;
    }
  }
}

// Sums over the 64 lanes of V values per lane (V a power of two <= 64): log2 V transposing steps, in each of which a lane
// keeps one half of its values and receives its partner's copies of that half, then plain butterfly steps.  Every lane ends
// with the complete sum of value v = lane / (64 / V); the tree of additions is the same for every v.
template <int V, int O = 32>
__device__ __forceinline__ float transpose_sum(const float (&a)[V], int lane) {
  static_assert(V >= 1 && (V == 1 || V <= 2 * O) && (V & (V - 1)) == 0, "V must be a power of two up to 64");
  if constexpr (V > 1) {
    constexpr int H = V / 2;
    const bool upper = (lane & O) != 0;
    float half[H];                            // a fresh array per step: every index is a constant, all of it stays in registers
#pragma unroll
    for (int i = 0; i < H; ++i) {
      const float lo = a[i], hi = a[i + H];
      half[i] = (upper ? hi : lo) + __shfl_xor(upper ? lo : hi, O, 64);
    }
    return transpose_sum<H, O / 2>(half, lane);
  } else {
    float v = a[0];
#pragma unroll
    for (int o = O; o >= 1; o /= 2) v += __shfl_xor(v, o, 64);
    return v;
  }
}

// floats of LDS that G queries of D elements take, zero-padded to whole chunks
__host__ __device__ constexpr long long padded_dim(long long D) { return (D + kChunk - 1) / kChunk * kChunk; }

// queries (Qg <= G rows of D) into q_lds (G rows of Dp), zeros elsewhere; the whole block of THREADS calls it, the caller
// synchronises
template <int G, int THREADS>
__device__ __forceinline__ void stage_queries(float* q_lds, unsigned Dp, const float* __restrict__ queries, int Qg, unsigned D,
                                              int tid) {
  for (int g = 0; g < G; ++g)
    for (unsigned d = tid; d < Dp; d += THREADS) q_lds[(size_t)g * Dp + d] = (g < Qg && d < D) ? queries[(size_t)g * D + d] : 0.0f;
}

// The scores of bank rows n0 .. n0 + R - 1 against the G resident queries, by one wavefront: store(r, g, s) is called
// once per (row r, query g), by the lane that holds the sum.  A row past N is clamped to row N - 1: scored, for the
// caller to drop.  Neither G nor R (rows a wavefront multiplies at once) changes a score's bits.
template <int G, int R, bool VEC, bool QLDS, class Store>
__device__ __forceinline__ void scan_rows(const float* __restrict__ bank, long long N, unsigned D, long long n0,
                                          const float* q_lds, unsigned Dp, const float* __restrict__ queries, int lane,
                                          Store store) {
  constexpr int V = R * G;
  constexpr int VH = V < 64 ? V : 64, H = V / VH;                     // the V sums of a lane, in H halves of VH
  const unsigned n_full = D / kChunk;
  const bool tail = (D % kChunk) != 0;
  const float* rows[R];
#pragma unroll
  for (int r = 0; r < R; ++r) rows[r] = bank + min(n0 + r, N - 1) * (long long)D;
  float acc[H][VH];
#pragma unroll
  for (int v = 0; v < V; ++v) acc[v / VH][v % VH] = 0.0f;
  float4 b[R];
  for (unsigned c = 0; c < n_full; ++c) {
    const unsigned d = c * kChunk + 4u * lane;
#pragma unroll
    for (int r = 0; r < R; ++r) b[r] = load4<VEC, false>(rows[r], d, D);
    fma_chunk<G, R, H, VH, QLDS, false>(acc, b, q_lds, Dp, queries, d, D);
  }
  if (tail) {
    const unsigned d = n_full * kChunk + 4u * lane;
#pragma unroll
    for (int r = 0; r < R; ++r) b[r] = load4<VEC, true>(rows[r], d, D);
    fma_chunk<G, R, H, VH, QLDS, true>(acc, b, q_lds, Dp, queries, d, D);
  }
#pragma unroll
  for (int h = 0; h < H; ++h) {
    const float total = transpose_sum<VH>(acc[h], lane);
    if (lane % (64 / VH) == 0) {
      const int v = h * VH + lane / (64 / VH);
      store(v / G, v % G, total);
    }
  }
}

}  // namespace
}  // namespace eat
