// What follows the group scan of a sequence match, whatever the bank's storage: the diagonal accumulate, the peak
// picking, the merge, their launches and the layout of the workspace.  match.hip (fp32 rows) and match_q8.hip (int8 codes)
// both include it, so acc, m and the peaks have the same bits for the same row scores S.
//
// Diagonal accumulate, match_accumulate_kernel.  acc[n] = acc[n] + S[g, n + j0 + g] for g ascending, group after group
// (the first group starts from S[0, n], not from 0 + S[0, n]): the additions of a start row happen in ascending j one at
// a time whatever the tile and group boundaries.  A start row whose window leaves the bank skips the rows past N: it is
// no candidate, its acc is never looked at.
//
// Peaks, match_peaks_kernel.  A fixed grid walks tiles of 256 start rows, a row per thread.  m = acc / L for the tile
// and a halo of sep rows on either side goes to LDS ((256 + 2 x 4096) x 4 B = 33 KB at most: several blocks per CU); a
// thread finds its row's file by a binary search in seg, tests candidacy and min_score, then walks the candidates of its
// file within sep and stops at the first that is better.  Each wavefront owns a sorted list of k (score, row) in LDS and
// offers its 64 rows' peaks with list_offer; the block stores its four lists, and search_merge_kernel (one block, a thread
// per list) pops the final order.  No atomics anywhere.
//
// Everything sits in an unnamed namespace on purpose, as in search_topk.h.
#pragma once
#include <cmath>
#include <cstdint>

#include "eat_common.h"
#include "search_topk.h"

namespace eat {
namespace {

constexpr int kPeakBlocks = 256, kPeakThreads = 256;       // a tile of the peak kernel is kPeakThreads start rows
constexpr int kPeakWaves = kPeakThreads / eat::kWave;
constexpr int kLists = kPeakBlocks * kPeakWaves;            // one sorted list per wavefront; the threads of the merge block
static_assert(kLists <= 1024, "the merge is one block with a thread per list");

// acc[n] (+)= S[g, n + j0 + g], g ascending; j0: the group's first query row
__global__ __launch_bounds__(256) void match_accumulate_kernel(const float* __restrict__ S, long long N, int Qg, int j0,
                                                               float* __restrict__ acc) {
  for (long long n = (long long)blockIdx.x * 256 + threadIdx.x; n < N; n += (long long)gridDim.x * 256) {
    float a = j0 == 0 ? S[n] : acc[n];
    for (int g = j0 == 0 ? 1 : 0; g < Qg; ++g) {
      const long long row = n + j0 + g;
      if (row < N) a = a + S[(long long)g * N + row];
    }
    acc[n] = a;
  }
}

// ws_s / ws_i: [kLists][k]
__global__ __launch_bounds__(kPeakThreads) void match_peaks_kernel(const float* __restrict__ acc, long long N,
                                                                   const int* __restrict__ seg, int F, int L, int k, int sep,
                                                                   float min_score, int skip_lo, int skip_hi,
                                                                   float* __restrict__ ws_s, int* __restrict__ ws_i) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int span = kPeakThreads + 2 * sep;
  float* const m = smem;                                               // m of rows base .. base + span - 1
  float* const list_s = smem + span;                                   // [kPeakWaves][k]
  int* const list_i = reinterpret_cast<int*>(list_s + kPeakWaves * k);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float* const ls = list_s + wave * k;
  int* const li = list_i + wave * k;
  for (int i = lane; i < k; i += 64) {                                 // this wavefront's own list
    ls[i] = -INFINITY;
    li[i] = -1;
  }
  const long long s_lo = min(max((long long)skip_lo, 0LL), N), s_hi = min(max((long long)skip_hi, 0LL), N);
  const float Lf = (float)L;

  const long long n_tiles = (N + kPeakThreads - 1) / kPeakThreads;
  for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const long long t0 = t * kPeakThreads, base = t0 - sep;
    __syncthreads();                                                   // every wavefront is done with the tile before
    for (int i = tid; i < span; i += kPeakThreads) {
      const long long x = base + i;
      if (x >= 0 && x < N) m[i] = __fdiv_rn(acc[x], Lf);
    }
    __syncthreads();

    const long long n = t0 + tid;
    float mine = 0.0f;
    bool peak = false;
    if (n < N) {
      int f = 0, top = F - 1;                                          // the file of row n: the last f with seg[f] <= n
      while (f < top) {
        const int mid = (f + top + 1) >> 1;
        if (seg[mid] <= n) f = mid; else top = mid - 1;
      }
      const long long first = seg[f], last = (long long)seg[f + 1] - L;      // the file's valid start rows: first .. last
      mine = m[tid + sep];
      peak = n >= first && n <= last && !(n >= s_lo && n < s_hi) && mine >= min_score;
      if (peak) {
        const long long lo = max(first, n - sep), hi = min(last, n + sep);   // within [base, base + span): inside m
        for (long long x = lo; x <= hi; ++x) {
          if (x == n || (x >= s_lo && x < s_hi)) continue;
          const float mx = m[x - base];
          if (!(mine > mx || (mine == mx && n < x))) {                 // n is not better than candidate x
            peak = false;
            break;
          }
        }
      }
    }
    list_offer(ls, li, k, mine, t0 + wave * 64, peak, lane);
  }
  for (int i = lane; i < k; i += 64) {
    const size_t o = ((size_t)blockIdx.x * kPeakWaves + wave) * k + i;
    ws_s[o] = ls[i];
    ws_i[o] = li[i];
  }
}

constexpr long long padded_rows(long long N) { return (N + 3) / 4 * 4; }      // every part of ws starts 16-byte aligned

// a match workspace: [kLists][k] scores, then indices; acc (N); S [group][N]
constexpr long long match_ws_bytes(long long N, int group, int k) { return 8LL * kLists * k + 4 * padded_rows(N) * (1 + group); }

struct MatchWs {
  float* ws_s; int* ws_i; float* acc; float* S;
  MatchWs(void* ws, long long N, int k)
      : ws_s(static_cast<float*>(ws)), ws_i(reinterpret_cast<int*>(ws_s + (size_t)kLists * k)),
        acc(reinterpret_cast<float*>(ws_i + (size_t)kLists * k)), S(acc + padded_rows(N)) {}
};

// after the scan of the group of Qg query rows that starts at j0 has stored S
inline void launch_accumulate(const MatchWs& w, long long N, int Qg, int j0, hipStream_t s) {
  const unsigned acc_blocks = (unsigned)((N + 255) / 256 < 4096 ? (N + 255) / 256 : 4096);
  hipLaunchKernelGGL(match_accumulate_kernel, dim3(acc_blocks), dim3(256), 0, s, w.S, N, Qg, j0, w.acc);
}

// after the last group: the peaks of acc / L and the k best of them
inline void launch_peaks(const MatchWs& w, long long N, const int* seg, int F, int L, int k, int sep, float min_score, int skip_lo,
                         int skip_hi, float* score, int* index, hipStream_t s) {
  const size_t peaks_lds = 4 * ((size_t)kPeakThreads + 2 * (size_t)sep + 2 * (size_t)kPeakWaves * k);
  hipLaunchKernelGGL(match_peaks_kernel, dim3(kPeakBlocks), dim3(kPeakThreads), peaks_lds, s, w.acc, N, seg, F, L, k, sep,
                     min_score, skip_lo, skip_hi, w.ws_s, w.ws_i);
  hipLaunchKernelGGL(search_merge_kernel<kLists>, dim3(1), dim3(kLists), 0, s, w.ws_s, w.ws_i, k, score, index);
}

}  // namespace
}  // namespace eat
