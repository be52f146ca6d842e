// The exact integer dot products of search_q8.hip and match_q8.hip: how a group of query codes lies in LDS, and
// `q8_dot_rows`, the k loop of v_mfma_i32_16x16x64_i8 over one wavefront's 16 bank rows with its order of issue.  Both
// scans call the same code; the sums are integers, so their bits would not depend on it, but the order of issue was
// measured once and should exist once.
//
// Everything sits in an unnamed namespace on purpose, as in search_topk.h.
#pragma once
#include <cstdint>

#include "eat_common.h"

namespace eat {
namespace {

constexpr int kQ8Ahead = 8;             // k-steps whose bank loads are issued before the first MFMA

typedef int v4i __attribute__((ext_vector_type(4)));

// bytes between two queries in LDS: D rounded up to 16, and an odd number of 16-byte pieces, so that the 16 queries of
// an A operand start in different banks
__host__ __device__ constexpr long long q_pitch(long long D) {
  const long long p = (D + 15) / 16;
  return 16 * (p % 2 ? p : p + 1);
}

// the codes of Qg <= G queries to LDS at q_pitch(D); the bytes from D on, and the slots from Qg on, become zeros
template <int G, int THREADS>
__device__ __forceinline__ void q8_stage_queries(unsigned char* q_lds, unsigned pitch, const int8_t* __restrict__ qcodes,
                                                 long long qld, int Qg, unsigned D, int tid) {
  const unsigned wpr = pitch / 4;                                    // 32-bit words per query
  for (unsigned i = tid; i < (unsigned)G * wpr; i += THREADS) {
    const unsigned g = i / wpr, d = 4u * (i - g * wpr);
    unsigned v = 0;
    if ((int)g < Qg && d < D) {                                      // d + 3 < qld: qld >= D is a multiple of 16
      v = *reinterpret_cast<const unsigned*>(qcodes + (long long)g * qld + d);
      if (d + 4u > D) v &= (1u << (8u * (D - d))) - 1u;              // the bytes from D on: zero, whatever the caller left there
    }
    reinterpret_cast<unsigned*>(q_lds)[i] = v;
  }
}

// acc[qt] = the 16 x 16 sums of queries 16 qt .. 16 qt + 15 (a_row[qt]: this lane's query in LDS, + 16 quad) and the
// wavefront's 16 bank rows (b_row: this lane's row, + 16 quad) over Dr = D rounded up to 16 bytes
template <int QT>
__device__ __forceinline__ void q8_dot_rows(v4i (&acc)[QT], const unsigned char* (&a_row)[QT], const int8_t* __restrict__ b_row,
                                            unsigned Dr, int quad) {
  constexpr int kAhead = kQ8Ahead;
  const unsigned n_steps = (Dr + 63u) / 64u, n_full = Dr / 64u;
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) acc[qt] = v4i{0, 0, 0, 0};
  unsigned step = 0;
  for (; step + kAhead <= n_full; step += kAhead) {
    v4i b[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) b[u] = *reinterpret_cast<const v4i*>(b_row + 64u * (step + u));
#pragma unroll
    for (int u = 0; u < kAhead; ++u)
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) {
        const v4i a = *reinterpret_cast<const v4i*>(a_row[qt] + 64u * (step + u));
        acc[qt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b[u], acc[qt], 0, 0, 0);
      }
    // the order of issue, which the compiler otherwise picks for the fewest registers (two bank loads in flight, every
    // MFMA waiting for its own LDS read): all bank loads of the batch, then the A operands of step u + 1 ahead of the
    // MFMAs of step u
    __builtin_amdgcn_sched_group_barrier(0x020, kAhead, 0);          // VMEM reads
    __builtin_amdgcn_sched_group_barrier(0x100, QT, 0);              // DS reads
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      if (u + 1 < kAhead) __builtin_amdgcn_sched_group_barrier(0x100, QT, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, QT, 0);            // MFMAs
    }
  }
  if (step < n_steps) {                                              // the rest of the row: fewer steps, the last one ragged
    v4i b[kAhead];
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      const unsigned off = 64u * (step + u) + 16u * quad;            // off < Dr <= ld: inside the row
      b[u] = v4i{0, 0, 0, 0};
      if (off < Dr) b[u] = *reinterpret_cast<const v4i*>(b_row + 64u * (step + u));
    }
#pragma unroll
    for (int u = 0; u < kAhead; ++u) {
      if (step + u < n_steps) {                                      // wave-uniform
        const unsigned off = 64u * (step + u) + 16u * quad;
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) {
          v4i a = v4i{0, 0, 0, 0};
          if (off < Dr) a = *reinterpret_cast<const v4i*>(a_row[qt] + 64u * (step + u));
          acc[qt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b[u], acc[qt], 0, 0, 0);
        }
      }
    }
  }
}

// the checks that the quantiser, the search and the match share on one q8 matrix
inline int check_q8(const char* who, const char* name, const void* p, long long ld, int D) {
  if (ld < D) return eat::fail(EAT_EINVAL, "%s: %s=%lld is below D=%d", who, name, ld, D);
  if (ld % 16 != 0) return eat::fail(EAT_EINVAL, "%s: %s=%lld is no multiple of 16", who, name, ld);
  if ((reinterpret_cast<uintptr_t>(p) & 15) != 0) return eat::fail(EAT_EINVAL, "%s: the codes behind %s are not 16-byte aligned", who, name);
  return EAT_OK;
}

}  // namespace
}  // namespace eat
