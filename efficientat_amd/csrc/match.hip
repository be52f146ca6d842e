// Device side of occurrence search (include/eat_match.h): the mean cosine of a sequence of L query rows laid over every
// start row of a bank, local-maximum peak picking within each file, and the k best peaks.
//
// Group scan, match_scan_kernel.  The stage-1 scan of search.hip - the same fixed grid, the same tiles of 64 bank rows, a
// group of G <= 16 consecutive query rows in LDS, the same `scan_rows` of search_scan.h and so the same bits per score -
// which stores the tile's scores to a workspace S (G, N) instead of offering them to lists: 64 bytes per bank row
// against 4 D read.  The scores pass through LDS (double-buffered, one barrier per tile) so that each query's 64
// scores leave as one 256-byte line.
//
// Diagonal accumulate, peaks and merge: match_peaks.h, shared with match_q8.hip.
#include <cmath>
#include <cstdint>

#include "eat_common.h"
#include "match_peaks.h"
#include "search_scan.h"
#include "search_topk.h"
#include "../../include/eat_match.h"

namespace {

using namespace eat;

constexpr int kMaxK = 128, kMaxL = 1024, kMaxSep = 4096;
// the group scan has the geometry that search.hip measured for its stage 1
constexpr int kScanBlocks = 256;        // a fixed grid, whatever N
constexpr int kScanThreads = 512;
constexpr int kScanWaves = kScanThreads / eat::kWave;
constexpr int kMaxGroup = 16;           // query rows resident per pass over the bank
constexpr int kRows = 8;                // bank rows a wavefront multiplies at once
// LDS of one scan block: G x Dp floats of queries (QLDS), 2 x G x tile-rows scores
__host__ __device__ constexpr long long scan_lds_bytes(int G, long long Dp) {
  return 4 * ((long long)G * Dp + 2LL * G * kScanWaves * kRows);
}

// queries: those of this group (Qg <= G of them); S [G][N]
template <int G, bool VEC, bool QLDS>
__global__ __launch_bounds__(kScanThreads) void match_scan_kernel(const float* __restrict__ bank, long long N, int D_,
                                                                  const float* __restrict__ queries, int Qg,
                                                                  float* __restrict__ S) {
  constexpr int R = kRows, TR = kScanWaves * R;                        // TR = 64 rows per tile
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const unsigned D = (unsigned)D_;
  const unsigned Dp = QLDS ? (unsigned)padded_dim(D) : 0u;
  float* const q_lds = smem;
  float* const sc = smem + (size_t)G * Dp;                             // [2][G][TR]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

  if constexpr (QLDS) {
    stage_queries<G, kScanThreads>(q_lds, Dp, queries, Qg, D, tid);
    __syncthreads();
  }
  const long long n_tiles = (N + TR - 1) / TR;
  int buf = 0;
  for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x, buf ^= 1) {
    float* const sc_t = sc + buf * G * TR;
    scan_rows<G, R, VEC, QLDS>(bank, N, D, t * TR + wave * R, q_lds, Dp, queries, lane,
                            [&](int r, int g, float s) { sc_t[g * TR + wave * R + r] = s; });       // a row past N: dropped below
    __syncthreads();
    // the next tile writes the other half of sc, and a wavefront reaches the tile after that only past the next barrier,
    // which every wavefront passes after its stores here: one barrier per tile
    for (int i = tid; i < Qg * TR; i += kScanThreads) {
      const int g = i / TR, r = i - g * TR;
      const long long row = t * TR + r;
      if (row < N) S[(long long)g * N + row] = sc_t[i];
    }
  }
}

struct ScanArgs {
  const float* bank; long long N; int D; const float* queries; int Qg; float* S; hipStream_t stream;
};

template <int G, bool VEC, bool QLDS>
int launch_scan(const ScanArgs& a) {
  auto kern = match_scan_kernel<G, VEC, QLDS>;
  const long long lds = scan_lds_bytes(G, QLDS ? padded_dim(a.D) : 0);
  if (lds > 64 * 1024) {          // per device, and cheap: asked for on every call
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return eat::fail(EAT_ELAUNCH, "eat_embed_match: hipFuncSetAttribute(%lld bytes of LDS) failed", lds);
  }
  hipLaunchKernelGGL(kern, dim3(kScanBlocks), dim3(kScanThreads), (size_t)lds, a.stream, a.bank, a.N, a.D, a.queries, a.Qg, a.S);
  return EAT_OK;
}

template <bool VEC>
int launch_scan_g(const ScanArgs& a, int G, bool qlds) {
  if (!qlds) return launch_scan<1, VEC, false>(a);
  switch (G) {
    case 16: return launch_scan<16, VEC, true>(a);
    case 8: return launch_scan<8, VEC, true>(a);
    case 4: return launch_scan<4, VEC, true>(a);
    case 2: return launch_scan<2, VEC, true>(a);
    default: return launch_scan<1, VEC, true>(a);
  }
}

}  // namespace

extern "C" long long eat_embed_match_ws_bytes(long long N, int L, int k) {
  if (N < 1 || N > 0x7fffffffLL || L < 1 || L > kMaxL || k < 1 || k > kMaxK) return -1;
  return match_ws_bytes(N, L < kMaxGroup ? L : kMaxGroup, k);
}

extern "C" int eat_embed_match(const float* bank, long long N, int D, const int* seg, int F, const float* queries, int L, int k,
                               int sep, float min_score, int skip_lo, int skip_hi, void* ws, long long ws_bytes, float* score,
                               int* index, eat_stream_t stream) {
  eat::clear_stale_error();
  if (L < 1 || L > kMaxL) return eat::fail(EAT_EINVAL, "eat_embed_match: L=%d lies outside [1, %d]", L, kMaxL);
  if (k < 1 || k > kMaxK) return eat::fail(EAT_EINVAL, "eat_embed_match: k=%d lies outside [1, %d]", k, kMaxK);
  if (sep < 0 || sep > kMaxSep) return eat::fail(EAT_EINVAL, "eat_embed_match: sep=%d lies outside [0, %d]", sep, kMaxSep);
  if (N < 1 || N > 0x7fffffffLL) return eat::fail(EAT_EINVAL, "eat_embed_match: N=%lld lies outside [1, 2147483647]", N);
  if (F < 1) return eat::fail(EAT_EINVAL, "eat_embed_match: need F >= 1 (got %d)", F);
  if (D < 1) return eat::fail(EAT_EINVAL, "eat_embed_match: need D >= 1 (got %d)", D);
  if (std::isnan(min_score)) return eat::fail(EAT_EINVAL, "eat_embed_match: min_score is NaN (-inf disables it)");
  const long long need = eat_embed_match_ws_bytes(N, L, k);
  if (ws_bytes < need)
    return eat::fail(EAT_EINVAL, "eat_embed_match: ws_bytes=%lld is below eat_embed_match_ws_bytes(N=%lld, L=%d, k=%d) = %lld",
                     ws_bytes, N, L, k, need);

  // the largest group whose query rows fit the LDS of a CU; not even one row: it is read from global memory
  const long long Dp = padded_dim(D);
  int g_max = kMaxGroup;
  while (g_max > 1 && scan_lds_bytes(g_max, Dp) > kLdsBytes) g_max /= 2;
  const bool qlds = scan_lds_bytes(g_max, Dp) <= kLdsBytes;
  const bool vec = D % 4 == 0 && (reinterpret_cast<uintptr_t>(bank) & 15) == 0;
  hipStream_t s = (hipStream_t)stream;
  const MatchWs w(ws, N, k);
  for (int j0 = 0; j0 < L;) {
    int G = g_max;
    while (G / 2 >= L - j0) G /= 2;                                     // the smallest instance that holds what is left
    const int Qg = L - j0 < G ? L - j0 : G;
    const ScanArgs a{bank, N, D, queries + (size_t)j0 * D, Qg, w.S, s};
    const int rc = vec ? launch_scan_g<true>(a, G, qlds) : launch_scan_g<false>(a, G, qlds);
    if (rc != EAT_OK) return rc;
    launch_accumulate(w, N, Qg, j0, s);
    j0 += Qg;
  }
  launch_peaks(w, N, seg, F, L, k, sep, min_score, skip_lo, skip_hi, score, index, s);
  return eat::check_launch("eat_embed_match");
}
