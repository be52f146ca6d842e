// Device side of the 8-bit search index (include/eat_search_q8.h): rows quantised to int8 codes with one fp32 scale each,
// and the fused top-k of search.hip over such a bank with exact integer dot products on the matrix cores.
//
// Stage 1, q8_scan_kernel.  A FIXED grid of kBlocks blocks of 8 wavefronts walks tiles of 128 bank rows at a grid stride.
// A group of G <= 64 queries sits in LDS as int8 codes (64 x 2192 B = 140 KB at D = 2184; bytes from D on are zeroed
// there, which is what masks d >= D), so the bank is read once per group.  A wavefront takes 16 bank rows: per k-step of
// 64, lane l loads 16 bytes of row l & 15 at byte 64 step + 16 (l >> 4) - the B operand of v_mfma_i32_16x16x64_i8 - and
// per 16 queries reads 16 bytes of query l & 15 at the same k from LDS - the A operand.  Both operands take their bytes
// from the same k, so the order of k inside the instruction does not matter; D[i][j] = sum_k A[i][k] B[k][j] has the
// query on its row, 4 (lane >> 4) + reg, and the bank row on its column, lane & 15.  The loads of kQ8Ahead = 8 k-steps are
// issued before the first MFMA of the batch (8 KB in flight per wavefront, 64 KB per CU); the tail of a row is one more
// batch with lanes and steps past D predicated off.  The arithmetic is far from the limit: 4 MFMAs and 4 KB of LDS
// reads per KB of bank at G = 64, against the ~10 bytes per clock that a CU's share of HBM delivers.
//
// The score (float)acc * (scale_q * scale_n) is a function of the two rows' contents alone: integer sums have no order.
//
// Running top-k: as in search.hip (search_topk.h), but the scores of a tile are staged 16 queries at a time - a round per
// accumulator tile, 2 x 16 x 128 floats double-buffered, one block barrier per round - because 64 x 128 staged scores
// would not fit beside 140 KB of queries.  Wavefront w owns the lists of queries 16 qt + w and 16 qt + w + 8.
//
// Stage 2: search_merge_kernel of search_topk.h.  No atomics anywhere.
//
// Quantiser, rows_quantize_kernel: a wavefront per row like eat_rows_normalize, whose sum of squares it shares
// (row_sumsq); lane l owns elements 4 l + 256 i .. + 3 in every pass and stores their four codes as one 32-bit word.
#include <cstdint>

#include "eat_common.h"
#include "search_q8_scan.h"
#include "search_topk.h"
#include "../../include/eat_search_q8.h"

namespace {

using namespace eat;

constexpr int kBlocks = 256;            // stage-1 grid, whatever N; also the threads of a stage-2 block (one per list)
constexpr int kThreads = 512;           // stage 1
constexpr int kWaves = kThreads / eat::kWave;
constexpr int kTileRows = 16 * kWaves;  // bank rows of a block per step: one 16-row MFMA tile per wavefront
constexpr int kMaxGroup = 64;           // queries resident per pass over the bank
constexpr int kMaxK = 128, kMaxQ = 1024, kMaxD = 131072;
constexpr long long kLdsBytes = 160 * 1024;

// LDS of one stage-1 block: G queries, G x k (score, index), 2 x 16 x kTileRows staged scores, (lo, hi, scale) per query slot
__host__ __device__ constexpr long long scan_lds_bytes(int G, long long D, int k) {
  return (long long)G * q_pitch(D) + 8LL * G * k + 4LL * 2 * 16 * kTileRows + 12LL * ((G + 15) / 16 * 16);
}

// qcodes / scale_q / skip: those of this group (Qg <= G of them); ws_s / ws_i: [Qg][kBlocks][k]
// waves_per_eu: the grid is one block of 8 wavefronts per CU, two per SIMD; told so, the compiler spends the registers that
// the issue order below needs (110 at G = 64) - without it the order is ignored in favour of 86 registers
template <int G>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void q8_scan_kernel(const int8_t* __restrict__ codes, long long ld,
                                                           const float* __restrict__ scale_n, long long N, int D_,
                                                           const int8_t* __restrict__ qcodes, long long qld,
                                                           const float* __restrict__ scale_q, int Qg, int k,
                                                           const int* __restrict__ skip, float* __restrict__ ws_s,
                                                           int* __restrict__ ws_i) {
  constexpr int QT = (G + 15) / 16, GP = 16 * QT;                    // accumulator tiles of 16 queries; query slots
  extern __shared__ __attribute__((aligned(16))) unsigned char smem8[];
  const unsigned D = (unsigned)D_, Dr = (D + 15u) & ~15u;
  const unsigned pitch = (unsigned)q_pitch(D);
  unsigned char* const q_lds = smem8;
  float* const list_s = reinterpret_cast<float*>(smem8 + (size_t)G * pitch);
  int* const list_i = reinterpret_cast<int*>(list_s + G * k);
  float* const sc = reinterpret_cast<float*>(list_i + G * k);        // [2][16][kTileRows]
  int* const s_lo = reinterpret_cast<int*>(sc + 2 * 16 * kTileRows);
  int* const s_hi = s_lo + GP;
  float* const s_sq = reinterpret_cast<float*>(s_hi + GP);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

  q8_stage_queries<G, kThreads>(q_lds, pitch, qcodes, qld, Qg, D, tid);
  for (int i = tid; i < G * k; i += kThreads) {
    list_s[i] = -INFINITY;
    list_i[i] = -1;
  }
  if (tid < GP) {
    int lo = 0, hi = 0;
    if (skip != nullptr && tid < Qg) {
      lo = skip[2 * tid];
      hi = skip[2 * tid + 1];
    }
    const int n_max = (int)N;                                        // N <= 2^31 - 1
    s_lo[tid] = min(max(lo, 0), n_max);
    s_hi[tid] = min(max(hi, 0), n_max);
    s_sq[tid] = tid < Qg ? scale_q[tid] : 0.0f;
  }
  __syncthreads();

  const int col = lane & 15, quad = lane >> 4;
  const long long n_tiles = (N + kTileRows - 1) / kTileRows;
  const unsigned char* a_row[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) a_row[qt] = q_lds + (size_t)min(16 * qt + col, G - 1) * pitch + 16 * quad;
  int buf = 0;
  for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const long long n = min(t * kTileRows + wave * 16 + col, N - 1);   // a row past N: scored and dropped
    const int8_t* const b_row = codes + n * ld + 16 * quad;
    v4i acc[QT];
    q8_dot_rows<QT>(acc, a_row, b_row, Dr, quad);

    const float sn = scale_n[n];
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
      // barrier, which every wavefront passes after its selection here: one barrier per round
      for (int ql = wave; ql < 16; ql += kWaves) {                     // wave-uniform: this wavefront owns list 16 qt + ql
        const int g = 16 * qt + ql;
        if (g >= Qg) break;
        float* const ls = list_s + g * k;
        int* const li = list_i + g * k;
#pragma unroll
        for (int half = 0; half < kTileRows / 64; ++half) {
          const long long row0 = t * kTileRows + 64 * half, row = row0 + lane;
          const float s = sc[(buf * 16 + ql) * kTileRows + 64 * half + lane];
          const bool eligible = row < N && !(row >= s_lo[g] && row < s_hi[g]);
          list_offer(ls, li, k, s, row0, eligible, lane);
        }
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < Qg * k; i += kThreads) {
    const int g = i / k, j = i - g * k;
    const size_t o = ((size_t)g * kBlocks + blockIdx.x) * k + j;
    ws_s[o] = list_s[i];
    ws_i[o] = list_i[i];
  }
}

// elements d .. d + 3 of a row (zeros from D on); VEC: one 16-byte load where the four lie inside the row
template <bool VEC>
__device__ __forceinline__ float4 load_x4(const float* __restrict__ r, unsigned d, unsigned D) {
  float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  if constexpr (VEC) {
    if (d < D) v = *reinterpret_cast<const float4*>(r + d);          // D % 4 == 0
  } else {
    if (d < D) v.x = r[d];
    if (d + 1 < D) v.y = r[d + 1];
    if (d + 2 < D) v.z = r[d + 2];
    if (d + 3 < D) v.w = r[d + 3];
  }
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(256) void rows_quantize_kernel(const float* __restrict__ x, long long N, int D_, int normalize,
                                                            int8_t* __restrict__ codes, long long ld, float* __restrict__ scale) {
  const unsigned D = (unsigned)D_;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (long long n = (long long)blockIdx.x * 4 + wave; n < N; n += (long long)gridDim.x * 4) {       // a wavefront per row
    const float* r = x + n * (long long)D;
    float norm = 1.0f;
    bool zero = false;
    if (normalize) {
      const float ss = row_sumsq<VEC>(r, D, lane);
      norm = sqrtf(ss);
      zero = !(ss > 0.0f);
    }
    // xh = x / norm as eat_rows_normalize divides, or x itself
    auto hat = [&](float v) { return normalize ? (zero ? 0.0f : v / norm) : v; };
    float amax = 0.0f;
    for (unsigned d = 4u * lane; d < D; d += 256) {
      const float4 v = load_x4<VEC>(r, d, D);
      amax = fmaxf(fmaxf(amax, fabsf(hat(v.x))), fmaxf(fabsf(hat(v.y)), fmaxf(fabsf(hat(v.z)), fabsf(hat(v.w)))));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o, 64));
    const float sc = __fdiv_rn(amax, 127.0f);
    const bool flat = !(amax > 0.0f);
    auto code = [&](float v) { return flat ? 0u : (unsigned)(int)rintf(__fdiv_rn(hat(v), sc)) & 0xffu; };
    int8_t* const o = codes + n * ld;
    for (long long d = 4 * lane; d < ld; d += 256) {                 // up to ld: the pad bytes are stored as zeros
      const float4 v = load_x4<VEC>(r, d < D ? (unsigned)d : D, D);  // zeros from D on, whose code is 0
      *reinterpret_cast<unsigned*>(o + d) = code(v.x) | code(v.y) << 8 | code(v.z) << 16 | code(v.w) << 24;
    }
    if (lane == 0) scale[n] = sc;
  }
}

struct ScanArgs {
  const int8_t* codes; long long ld; const float* scale_n; long long N; int D; const int8_t* qcodes; long long qld;
  const float* scale_q; int Qg, k; const int* skip; float* ws_s; int* ws_i; hipStream_t stream;
};

template <int G>
int launch_scan(const ScanArgs& a) {
  auto kern = q8_scan_kernel<G>;
  const long long lds = scan_lds_bytes(G, a.D, a.k);
  if (lds > 64 * 1024) {          // per device, and cheap: asked for on every call
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return eat::fail(EAT_ELAUNCH, "eat_embed_search_q8: hipFuncSetAttribute(%lld bytes of LDS) failed", lds);
  }
  hipLaunchKernelGGL(kern, dim3(kBlocks), dim3(kThreads), (size_t)lds, a.stream, a.codes, a.ld, a.scale_n, a.N, a.D, a.qcodes,
                     a.qld, a.scale_q, a.Qg, a.k, a.skip, a.ws_s, a.ws_i);
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

extern "C" int eat_rows_quantize_q8(const float* x, long long N, int D, int normalize, signed char* codes, long long ld,
                                    float* scale, eat_stream_t stream) {
  eat::clear_stale_error();
  if (N < 0) return eat::fail(EAT_EINVAL, "eat_rows_quantize_q8: need N >= 0 (got %lld)", N);
  if (D < 1 || D > kMaxD) return eat::fail(EAT_EINVAL, "eat_rows_quantize_q8: D=%d lies outside [1, %d]", D, kMaxD);
  const int rc = check_q8("eat_rows_quantize_q8", "ld", codes, ld, D);
  if (rc != EAT_OK) return rc;
  if (N == 0) return EAT_OK;
  const unsigned blocks = (unsigned)((N + 3) / 4 < (1LL << 20) ? (N + 3) / 4 : (1LL << 20));
  const bool vec = D % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  int8_t* const c = reinterpret_cast<int8_t*>(codes);
  if (vec) hipLaunchKernelGGL(rows_quantize_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, N, D, normalize, c, ld, scale);
  else hipLaunchKernelGGL(rows_quantize_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, N, D, normalize, c, ld, scale);
  return eat::check_launch("eat_rows_quantize_q8");
}

extern "C" long long eat_embed_search_q8_ws_bytes(int Q, int k) {
  if (Q < 1 || Q > kMaxQ || k < 1 || k > kMaxK) return -1;
  return 8LL * (Q < kMaxGroup ? Q : kMaxGroup) * kBlocks * k;            // [group][kBlocks][k] scores, then indices
}

extern "C" int eat_embed_search_q8(const signed char* codes, long long ld, const float* scale_n, long long N, int D,
                                   const signed char* qcodes, long long qld, const float* scale_q, int Q, int k, const int* skip,
                                   void* ws, long long ws_bytes, float* score, int* index, eat_stream_t stream) {
  eat::clear_stale_error();
  const char* const who = "eat_embed_search_q8";
  if (k < 1 || k > kMaxK) return eat::fail(EAT_EINVAL, "%s: k=%d lies outside [1, %d]", who, k, kMaxK);
  if (Q < 1 || Q > kMaxQ) return eat::fail(EAT_EINVAL, "%s: Q=%d lies outside [1, %d]", who, Q, kMaxQ);
  if (N < 1 || N > 0x7fffffffLL) return eat::fail(EAT_EINVAL, "%s: N=%lld lies outside [1, 2147483647]", who, N);
  if (D < 1 || D > kMaxD) return eat::fail(EAT_EINVAL, "%s: D=%d lies outside [1, %d]", who, D, kMaxD);
  int rc = check_q8(who, "ld", codes, ld, D);
  if (rc == EAT_OK) rc = check_q8(who, "qld", qcodes, qld, D);
  if (rc != EAT_OK) return rc;
  const long long need = eat_embed_search_q8_ws_bytes(Q, k);
  if (ws_bytes < need)
    return eat::fail(EAT_EINVAL, "%s: ws_bytes=%lld is below eat_embed_search_q8_ws_bytes(Q=%d, k=%d) = %lld", who, ws_bytes, Q, k, need);

  // the largest group whose codes and lists fit the LDS of a CU; one query of kMaxD values with lists of kMaxK always does
  static_assert(scan_lds_bytes(1, kMaxD, kMaxK) <= kLdsBytes, "a single query must fit");
  int g_max = kMaxGroup;
  while (g_max > 1 && scan_lds_bytes(g_max, D, k) > kLdsBytes) g_max /= 2;
  const int group_cap = Q < kMaxGroup ? Q : kMaxGroup;
  float* const ws_s = static_cast<float*>(ws);
  int* const ws_i = reinterpret_cast<int*>(ws_s + (size_t)group_cap * kBlocks * k);
  for (int q0 = 0; q0 < Q;) {
    int G = g_max;
    while (G / 2 >= Q - q0) G /= 2;                                     // the smallest instance that holds what is left
    const int Qg = Q - q0 < G ? Q - q0 : G;
    const ScanArgs a{reinterpret_cast<const int8_t*>(codes), ld, scale_n, N, D, reinterpret_cast<const int8_t*>(qcodes) + (long long)q0 * qld,
                     qld, scale_q + q0, Qg, k, skip ? skip + 2 * q0 : nullptr, ws_s, ws_i, (hipStream_t)stream};
    rc = launch_scan_g(a, G);
    if (rc != EAT_OK) return rc;
    hipLaunchKernelGGL(search_merge_kernel<kBlocks>, dim3(Qg), dim3(kBlocks), 0, (hipStream_t)stream, ws_s, ws_i, k,
                       score + (size_t)q0 * k, index + (size_t)q0 * k);
    const int rc2 = eat::check_launch(who);
    if (rc2 != EAT_OK) return rc2;
    q0 += Qg;
  }
  return EAT_OK;
}
