// Device side of query-by-example search (include/eat_search.h): L2 normalisation of rows, and a fused cosine top-k of
// a group of queries over a resident bank of embeddings, without a (Q, N) score matrix.
//
// Stage 1, search_scan_kernel.  A FIXED grid of kBlocks blocks of 8 wavefronts walks tiles of 64 bank rows at a grid stride.
// A group of G <= 16 normalised queries sits in LDS, zero-padded to whole 256-float chunks (16 x 2304 x 4 B = 144 KB at
// D = 2184), so the bank is read once per group.  A wavefront takes R = 8 rows at a time (R x G = 128 accumulators at G = 16),
// lanes along d: per 256-float chunk it loads R x 16 bytes per lane from the bank (R loads in flight per wavefront, 8 R
// per CU) and G x 16 bytes from LDS, each LDS value feeding R v_fma.  The R x G partial sums of the 64 lanes
// are summed by a transposing butterfly (63 shuffles for 64 sums instead of 384) that leaves sum v in lane v.
// (R = 4 at G = 8, 16 was measured first: 8 rows halve the LDS reads per bank byte and double the loads in flight)
//
// The score of a wavefront's rows (loads, multiply-adds, butterfly) is `scan_rows` of search_scan.h, which match.hip calls too.
// Position independence: element d of a row always goes to lane (d / 4) % 64, the lane adds its elements in ascending d
// with one fmaf each, and the butterfly adds lanes in one fixed tree whatever the slot (row r, query g) of the sum - fp32
// addition commutes, so which partner keeps a pair's sum does not matter.  The 4-byte path (D % 4 != 0 or an unaligned
// bank) loads the same four elements per lane with scalar loads, and rows past N are clamped to row N - 1 and dropped
// afterwards: the bits of a score depend on the two rows' contents and on D alone.
//
// Running top-k: the tile's scores go to LDS (double-buffered: one block barrier per tile), then wavefront g % 8 owns the
// sorted list of query g, k <= 128 (score, index) pairs in LDS: a score enters only if it beats the list's last entry
// under (score desc, index asc), by a wave-wide count of the entries ahead of it and a shift.  After warm-up almost
// nothing does.  At its end the block stores its lists, padded with (-inf, -1), to ws[g][block][k].
//
// Stage 2, search_merge_kernel: one block per query, thread t holds the head of block t's sorted list; k rounds of a
// block-wide arg-max pop the final order.  No atomics anywhere.
#include <cstdint>

#include "eat_common.h"
#include "search_scan.h"
#include "search_topk.h"
#include "../../include/eat_search.h"

namespace {

using namespace eat;             // search_scan.h: the score of a row; search_topk.h: better, list_offer, search_merge_kernel, row_sumsq

constexpr int kBlocks = 256;            // stage-1 grid, whatever N; also the threads of a stage-2 block (one per list)
constexpr int kThreads = 512;           // stage 1
constexpr int kWaves = kThreads / eat::kWave;
constexpr int kMaxGroup = 16;           // queries resident per pass over the bank
constexpr int kMaxK = 128, kMaxQ = 1024;

constexpr int rows_per_wave(int G) { return 8; }                       // R: rows a wavefront multiplies at once

// LDS of one stage-1 block: G x Dp floats of queries (QLDS), G x k (score, index), 2 x G x tile-rows scores, G x (lo, hi)
__host__ __device__ constexpr long long scan_lds_bytes(int G, long long Dp, int k) {
  return 4 * ((long long)G * Dp + 2LL * G * k + 2LL * G * kWaves * rows_per_wave(G) + 2LL * G);
}

// queries / skip: those of this group (Qg <= G of them); ws_s / ws_i: [Qg][kBlocks][k]
template <int G, bool VEC, bool QLDS>
__global__ __launch_bounds__(kThreads) void search_scan_kernel(const float* __restrict__ bank, long long N, int D_,
                                                               const float* __restrict__ queries, int Qg, int k,
                                                               const int* __restrict__ skip, float* __restrict__ ws_s,
                                                               int* __restrict__ ws_i) {
  constexpr int R = rows_per_wave(G), TR = kWaves * R;                 // TR = 64 rows per tile
  static_assert(TR <= 64, "one lane per row of the tile in the selection");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const unsigned D = (unsigned)D_;
  const unsigned Dp = QLDS ? (unsigned)padded_dim(D) : 0u;
  float* const q_lds = smem;
  float* const list_s = smem + (size_t)G * Dp;
  int* const list_i = reinterpret_cast<int*>(list_s + G * k);
  float* const sc = reinterpret_cast<float*>(list_i + G * k);        // [2][G][TR]
  int* const s_lo = reinterpret_cast<int*>(sc + 2 * G * TR);
  int* const s_hi = s_lo + G;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;

  if constexpr (QLDS) stage_queries<G, kThreads>(q_lds, Dp, queries, Qg, D, tid);
  for (int i = tid; i < G * k; i += kThreads) {
    list_s[i] = -INFINITY;
    list_i[i] = -1;
  }
  if (tid < G) {
    int lo = 0, hi = 0;
    if (skip != nullptr && tid < Qg) {
      lo = skip[2 * tid];
      hi = skip[2 * tid + 1];
    }
    const int n_max = (int)N;                                        // N <= 2^31 - 1
    s_lo[tid] = min(max(lo, 0), n_max);
    s_hi[tid] = min(max(hi, 0), n_max);
  }
  __syncthreads();

  const long long n_tiles = (N + TR - 1) / TR;
  int buf = 0;
  for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x, buf ^= 1) {
    float* const sc_t = sc + buf * G * TR;
    scan_rows<G, R, VEC, QLDS>(bank, N, D, t * TR + wave * R, q_lds, Dp, queries, lane,
                            [&](int r, int g, float s) { sc_t[g * TR + wave * R + r] = s; });       // a row past N: dropped below
    __syncthreads();
    // the next tile writes the other half of sc, and a wavefront reaches the tile after that only past the next barrier,
    // which every wavefront passes after its selection here: one barrier per tile

    for (int g = wave; g < Qg; g += kWaves) {                         // wave-uniform: this wavefront owns list g
      float* const ls = list_s + g * k;
      int* const li = list_i + g * k;
      const long long row = t * TR + lane;
      const float s = lane < TR ? sc[(buf * G + g) * TR + lane] : 0.0f;
      const bool eligible = lane < TR && row < N && !(row >= s_lo[g] && row < s_hi[g]);
      list_offer(ls, li, k, s, t * TR, eligible, lane);
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

template <bool VEC>
__global__ __launch_bounds__(256) void rows_normalize_kernel(const float* x, long long N, int D_, float* out) {
  const unsigned D = (unsigned)D_;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (long long n = (long long)blockIdx.x * 4 + wave; n < N; n += (long long)gridDim.x * 4) {       // a wavefront per row
    const float* r = x + n * (long long)D;
    float* o = out + n * (long long)D;
    const float ss = row_sumsq<VEC>(r, D, lane);      // every load of the row has landed here: out may be x
    const float norm = sqrtf(ss);
    const bool zero = !(ss > 0.0f);
    if constexpr (VEC) {
      for (unsigned d = 4u * lane; d < D; d += 256) {
        float4 v = *reinterpret_cast<const float4*>(r + d);
        v = zero ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : make_float4(v.x / norm, v.y / norm, v.z / norm, v.w / norm);
        *reinterpret_cast<float4*>(o + d) = v;
      }
    } else {
      for (unsigned d = lane; d < D; d += 64) o[d] = zero ? 0.0f : r[d] / norm;
    }
  }
}

struct ScanArgs {
  const float* bank; long long N; int D; const float* queries; int Qg, k; const int* skip; float* ws_s; int* ws_i;
  hipStream_t stream;
};

template <int G, bool VEC, bool QLDS>
int launch_scan(const ScanArgs& a) {
  auto kern = search_scan_kernel<G, VEC, QLDS>;
  const long long Dp = QLDS ? padded_dim(a.D) : 0;
  const long long lds = scan_lds_bytes(G, Dp, a.k);
  if (lds > 64 * 1024) {          // per device, and cheap: asked for on every call
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
      return eat::fail(EAT_ELAUNCH, "eat_embed_search: hipFuncSetAttribute(%lld bytes of LDS) failed", lds);
  }
  hipLaunchKernelGGL(kern, dim3(kBlocks), dim3(kThreads), (size_t)lds, a.stream, a.bank, a.N, a.D, a.queries, a.Qg, a.k, a.skip,
                     a.ws_s, a.ws_i);
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

extern "C" int eat_rows_normalize(const float* x, long long N, int D, float* out, eat_stream_t stream) {
  eat::clear_stale_error();
  if (N < 0) return eat::fail(EAT_EINVAL, "eat_rows_normalize: need N >= 0 (got %lld)", N);
  if (D < 1) return eat::fail(EAT_EINVAL, "eat_rows_normalize: need D >= 1 (got %d)", D);
  if (N == 0) return EAT_OK;
  const unsigned blocks = (unsigned)((N + 3) / 4 < (1LL << 20) ? (N + 3) / 4 : (1LL << 20));
  const bool vec = D % 4 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  if (vec) hipLaunchKernelGGL(rows_normalize_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, N, D, out);
  else hipLaunchKernelGGL(rows_normalize_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, N, D, out);
  return eat::check_launch("eat_rows_normalize");
}

extern "C" long long eat_embed_search_ws_bytes(int Q, int k) {
  if (Q < 1 || Q > kMaxQ || k < 1 || k > kMaxK) return -1;
  return 8LL * (Q < kMaxGroup ? Q : kMaxGroup) * kBlocks * k;            // [group][kBlocks][k] scores, then indices
}

extern "C" int eat_embed_search(const float* bank, long long N, int D, const float* queries, int Q, int k, const int* skip,
                                void* ws, long long ws_bytes, float* score, int* index, eat_stream_t stream) {
  eat::clear_stale_error();
  if (k < 1 || k > kMaxK) return eat::fail(EAT_EINVAL, "eat_embed_search: k=%d lies outside [1, %d]", k, kMaxK);
  if (Q < 1 || Q > kMaxQ) return eat::fail(EAT_EINVAL, "eat_embed_search: Q=%d lies outside [1, %d]", Q, kMaxQ);
  if (N < 1 || N > 0x7fffffffLL) return eat::fail(EAT_EINVAL, "eat_embed_search: N=%lld lies outside [1, 2147483647]", N);
  if (D < 1) return eat::fail(EAT_EINVAL, "eat_embed_search: need D >= 1 (got %d)", D);
  const long long need = eat_embed_search_ws_bytes(Q, k);
  if (ws_bytes < need)
    return eat::fail(EAT_EINVAL, "eat_embed_search: ws_bytes=%lld is below eat_embed_search_ws_bytes(Q=%d, k=%d) = %lld", ws_bytes,
                     Q, k, need);

  // the largest group whose queries and lists fit the LDS of a CU; not even one query: it is read from global memory
  const long long Dp = padded_dim(D);
  int g_max = kMaxGroup;
  while (g_max > 1 && scan_lds_bytes(g_max, Dp, k) > kLdsBytes) g_max /= 2;
  const bool qlds = scan_lds_bytes(g_max, Dp, k) <= kLdsBytes;
  const bool vec = D % 4 == 0 && (reinterpret_cast<uintptr_t>(bank) & 15) == 0;
  const int group_cap = Q < kMaxGroup ? Q : kMaxGroup;
  float* const ws_s = static_cast<float*>(ws);
  int* const ws_i = reinterpret_cast<int*>(ws_s + (size_t)group_cap * kBlocks * k);
  for (int q0 = 0; q0 < Q;) {
    int G = g_max;
    while (G / 2 >= Q - q0) G /= 2;                                     // the smallest instance that holds what is left
    const int Qg = Q - q0 < G ? Q - q0 : G;
    const ScanArgs a{bank, N, D, queries + (size_t)q0 * D, Qg, k, skip ? skip + 2 * q0 : nullptr, ws_s, ws_i, (hipStream_t)stream};
    const int rc = vec ? launch_scan_g<true>(a, G, qlds) : launch_scan_g<false>(a, G, qlds);
    if (rc != EAT_OK) return rc;
    hipLaunchKernelGGL(search_merge_kernel<kBlocks>, dim3(Qg), dim3(kBlocks), 0, (hipStream_t)stream, ws_s, ws_i, k, score + (size_t)q0 * k,
                       index + (size_t)q0 * k);
    const int rc2 = eat::check_launch("eat_embed_search");
    if (rc2 != EAT_OK) return rc2;
    q0 += Qg;
  }
  return EAT_OK;
}
