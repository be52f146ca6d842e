// Device side of occurrence search over an 8-bit index (include/eat_match_q8.h): the sequence match of match.hip with the
// row scores of search_q8.hip.
//
// Group scan, match_q8_scan_kernel.  The stage-1 scan of search_q8.hip - the same fixed grid of kBlocks blocks of 8
// wavefronts, the same tiles of 128 bank rows with one 16-row MFMA tile per wavefront, a group of G <= 64 consecutive
// query rows as int8 codes in LDS, the same `q8_dot_rows` of search_q8_scan.h, the same scaling and so the same bits per
// score - which stores the tile's scores to a workspace S (G, N) instead of offering them to lists.  There are no lists,
// no skip table and no selection: the LDS holds the codes, the staged scores and the query scales, so 64 rows fit at
// D = 2184 whatever k.  The scores pass through LDS 16 query rows at a time (2 x 16 x 128 floats double-buffered, one
// block barrier per round) so that a query row's 128 scores leave as one 512-byte run: a thread stores 4 consecutive
// scores, as one 16-byte store where the tile is whole and the address allows it.
//
// Diagonal accumulate, peaks and merge: match_peaks.h, shared with match.hip.  No atomics anywhere.
#include <cmath>
#include <cstdint>

#include "eat_common.h"
#include "match_peaks.h"
#include "search_q8_scan.h"
#include "../../include/eat_match_q8.h"

namespace {

using namespace eat;

constexpr int kMaxK = 128, kMaxL = 1024, kMaxSep = 4096, kMaxD = 131072;
// the geometry that search_q8.hip measured for its stage 1
constexpr int kBlocks = 256;            // a fixed grid, whatever N
constexpr int kThreads = 512;
constexpr int kWaves = kThreads / eat::kWave;
constexpr int kTileRows = 16 * kWaves;  // bank rows of a block per step: one 16-row MFMA tile per wavefront
constexpr int kMaxGroup = 64;           // query rows resident per pass over the bank
constexpr long long kLdsBytes = 160 * 1024;
static_assert(16 * kTileRows == 4 * kThreads, "a round's 16 x kTileRows scores are 4 per thread");

// LDS of one scan block: G queries, 2 x 16 x kTileRows staged scores, a scale per query slot
__host__ __device__ constexpr long long scan_lds_bytes(int G, long long D) {
  return (long long)G * q_pitch(D) + 4LL * 2 * 16 * kTileRows + 4LL * ((G + 15) / 16 * 16);
}

// qcodes / scale_q: those of this group (Qg <= G of them); S [G][N]
// waves_per_eu: as for q8_scan_kernel - one block of 8 wavefronts per CU, two per SIMD
template <int G>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void match_q8_scan_kernel(
    const int8_t* __restrict__ codes, long long ld, const float* __restrict__ scale_n, long long N, int D_,
    const int8_t* __restrict__ qcodes, long long qld, const float* __restrict__ scale_q, int Qg, float* __restrict__ S) {
  constexpr int QT = (G + 15) / 16, GP = 16 * QT;                    // accumulator tiles of 16 queries; query slots
  extern __shared__ __attribute__((aligned(16))) unsigned char smem8[];
  const unsigned D = (unsigned)D_, Dr = (D + 15u) & ~15u;
  const unsigned pitch = (unsigned)q_pitch(D);
  unsigned char* const q_lds = smem8;
  float* const sc = reinterpret_cast<float*>(smem8 + (size_t)G * pitch);       // [2][16][kTileRows]; pitch % 16 == 0
  float* const s_sq = sc + 2 * 16 * kTileRows;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

  q8_stage_queries<G, kThreads>(q_lds, pitch, qcodes, qld, Qg, D, tid);
  if (tid < GP) s_sq[tid] = tid < Qg ? scale_q[tid] : 0.0f;
  __syncthreads();

  const int col = lane & 15, quad = lane >> 4;
  const long long n_tiles = (N + kTileRows - 1) / kTileRows;
  const unsigned char* a_row[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) a_row[qt] = q_lds + (size_t)min(16 * qt + col, G - 1) * pitch + 16 * quad;
  const int st_q = tid / (kTileRows / 4), st_c = 4 * (tid % (kTileRows / 4));   // the 4 staged scores this thread stores
  int buf = 0;
  for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const long long n = min(t * kTileRows + wave * 16 + col, N - 1);   // a row past N: scored and dropped
    const int8_t* const b_row = codes + n * ld + 16 * quad;
    v4i acc[QT];
    q8_dot_rows<QT>(acc, a_row, b_row, Dr, quad);

    const float sn = scale_n[n];
    const long long row0 = t * kTileRows + st_c;
    const bool whole = (t + 1) * kTileRows <= N;
#pragma unroll
    for (int qt = 0; qt < QT; ++qt, buf ^= 1) {
      // a round: the scores of queries 16 qt .. 16 qt + 15 against the block's 128 rows
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int ql = 4 * quad + r;
        sc[(buf * 16 + ql) * kTileRows + wave * 16 + col] = (float)acc[qt][r] * (s_sq[16 * qt + ql] * sn);
      }
      __syncthreads();
      // the next round writes the other half of sc, and a wavefront reaches the round after that only past the next
      // barrier, which every wavefront passes after its stores here: one barrier per round
      const int g = 16 * qt + st_q;
      if (g < Qg) {
        const float4 v = *reinterpret_cast<const float4*>(sc + (buf * 16 + st_q) * kTileRows + st_c);
        float* const out = S + ((long long)g * N + row0);
        if (whole && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
          *reinterpret_cast<float4*>(out) = v;
        } else {
          if (row0 < N) out[0] = v.x;
          if (row0 + 1 < N) out[1] = v.y;
          if (row0 + 2 < N) out[2] = v.z;
          if (row0 + 3 < N) out[3] = v.w;
        }
      }
    }
  }
}

struct ScanArgs {
  const int8_t* codes; long long ld; const float* scale_n; long long N; int D; const int8_t* qcodes; long long qld;
  const float* scale_q; int Qg; float* S; hipStream_t stream;
};

template <int G>
int launch_scan(const ScanArgs& a) {
  auto kern = match_q8_scan_kernel<G>;
  const long long lds = scan_lds_bytes(G, a.D);
  if (lds > 64 * 1024) {          // per device, and cheap: asked for on every call
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return eat::fail(EAT_ELAUNCH, "eat_embed_match_q8: hipFuncSetAttribute(%lld bytes of LDS) failed", lds);
  }
  hipLaunchKernelGGL(kern, dim3(kBlocks), dim3(kThreads), (size_t)lds, a.stream, a.codes, a.ld, a.scale_n, a.N, a.D, a.qcodes,
                     a.qld, a.scale_q, a.Qg, a.S);
  return EAT_OK;
}

int launch_scan_g(const ScanArgs& a, int G) {
  switch (G) {
    case 64: return launch_scan<64>(a);
    case 32: return launch_scan<32>(a);
    case 16: return launch_scan<16>(a);
    case 8: return launch_scan<8>(a);
    case 4: return launch_scan<4>(a);
    case 2: return launch_scan<2>(a);
    default: return launch_scan<1>(a);
  }
}

}  // namespace

extern "C" long long eat_embed_match_q8_ws_bytes(long long N, int L, int k) {
  if (N < 1 || N > 0x7fffffffLL || L < 1 || L > kMaxL || k < 1 || k > kMaxK) return -1;
  return match_ws_bytes(N, L < kMaxGroup ? L : kMaxGroup, k);
}

extern "C" int eat_embed_match_q8(const signed char* codes, long long ld, const float* scale_n, long long N, int D, const int* seg,
                                  int F, const signed char* qcodes, long long qld, const float* scale_q, int L, int k, int sep,
                                  float min_score, int skip_lo, int skip_hi, void* ws, long long ws_bytes, float* score, int* index,
                                  eat_stream_t stream) {
  eat::clear_stale_error();
  const char* const who = "eat_embed_match_q8";
  if (L < 1 || L > kMaxL) return eat::fail(EAT_EINVAL, "%s: L=%d lies outside [1, %d]", who, L, kMaxL);
  if (k < 1 || k > kMaxK) return eat::fail(EAT_EINVAL, "%s: k=%d lies outside [1, %d]", who, k, kMaxK);
  if (sep < 0 || sep > kMaxSep) return eat::fail(EAT_EINVAL, "%s: sep=%d lies outside [0, %d]", who, sep, kMaxSep);
  if (N < 1 || N > 0x7fffffffLL) return eat::fail(EAT_EINVAL, "%s: N=%lld lies outside [1, 2147483647]", who, N);
  if (F < 1) return eat::fail(EAT_EINVAL, "%s: need F >= 1 (got %d)", who, F);
  if (D < 1 || D > kMaxD) return eat::fail(EAT_EINVAL, "%s: D=%d lies outside [1, %d]", who, D, kMaxD);
  if (std::isnan(min_score)) return eat::fail(EAT_EINVAL, "%s: min_score is NaN (-inf disables it)", who);
  int rc = check_q8(who, "ld", codes, ld, D);
  if (rc == EAT_OK) rc = check_q8(who, "qld", qcodes, qld, D);
  if (rc != EAT_OK) return rc;
  const long long need = eat_embed_match_q8_ws_bytes(N, L, k);
  if (ws_bytes < need)
    return eat::fail(EAT_EINVAL, "%s: ws_bytes=%lld is below eat_embed_match_q8_ws_bytes(N=%lld, L=%d, k=%d) = %lld", who, ws_bytes, N,
                     L, k, need);

  // the largest group whose codes fit the LDS of a CU; one row of kMaxD values always does
  static_assert(scan_lds_bytes(1, kMaxD) <= kLdsBytes, "a single query row must fit");
  int g_max = kMaxGroup;
  while (g_max > 1 && scan_lds_bytes(g_max, D) > kLdsBytes) g_max /= 2;
  hipStream_t s = (hipStream_t)stream;
  const MatchWs w(ws, N, k);
  for (int j0 = 0; j0 < L;) {
    int G = g_max;
    while (G / 2 >= L - j0) G /= 2;                                     // the smallest instance that holds what is left
    const int Qg = L - j0 < G ? L - j0 : G;
    const ScanArgs a{reinterpret_cast<const int8_t*>(codes), ld, scale_n, N, D, reinterpret_cast<const int8_t*>(qcodes) + (long long)j0 * qld,
                     qld, scale_q + j0, Qg, w.S, s};
    rc = launch_scan_g(a, G);
    if (rc != EAT_OK) return rc;
    launch_accumulate(w, N, Qg, j0, s);
    j0 += Qg;
  }
  launch_peaks(w, N, seg, F, L, k, sep, min_score, skip_lo, skip_hi, score, index, s);
  return eat::check_launch(who);
}
