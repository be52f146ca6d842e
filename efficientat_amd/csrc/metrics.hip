// Per-class average precision and ROC AUC over an (N, C) score matrix (eat_rank_metrics): the metric of the reference's
// `_test` (ex_audioset.py:231-256, sklearn's average_precision_score / roc_auc_score with average=None), on the device.
//
//   1. rank_keys_kernel   one coalesced pass over the row-major (N, C) scores / targets, transposed through LDS: every
//                         column becomes N 64-bit items (descending-order key << 32 | label) in the workspace, column-major.
//                         Validates every score (finite) and target (exactly 0 or 1) into the status word.
//   2. rank_sort_kernel   one workgroup per class: LSD radix sort of the 32-bit keys, 4 passes of 8 bits between the two
//                         halves of the workspace.  One read builds all four digit histograms; a pass whose digit is the
//                         same for every item is skipped.  Stable ranking inside a 512-item tile: per-wave match masks
//                         from 8 ballots, per-wave digit counts in LDS.
//   3. rank_scan_kernel   one workgroup per class over the sorted column: TP = running sum of labels; an item is the end
//                         of a tie group when the next key differs.  At a group end with TP / count (TPp / cntp at the
//                         previous group end: exclusive max-scans, both are non-decreasing):
//                           AP  += (TP - TPp) * TP / count            (recall step x precision; / n_pos at the end)
//                           AUC += (FP - FPp) * (TP + TPp)            (twice the trapezoid; integer, exact)
//                         The AP terms are fp64, summed per thread in tile order and then over the workgroup in a fixed
//                         tree: two calls give bit-identical results.
//
// eat_rank_metrics_masked (sklearn's sample_weight with 0 / 1 weights, ex_openmic.py:194-204) runs the same three kernels:
// the item's low word carries the weight in bit 1 next to the label in bit 0, `count` becomes the running sum of weights and
// TP the running sum of label & weight.  An item of weight 0 still belongs to its tie group but adds nothing to it.
#include "eat_common.h"

#include <stdint.h>

namespace eat {
namespace {

constexpr int kSortThreads = 512;                       // 8 waves; one item per thread per tile
constexpr int kSortWaves = kSortThreads / kWave;
constexpr int kTile = 64;                               // rank_keys_kernel: 64 x 64 transpose tile, 256 threads

// fp32 -> uint32 whose ASCENDING order is the DESCENDING order of the floats; -0.0 is folded onto +0.0 first (they tie)
__device__ __forceinline__ uint32_t desc_key(float v) {
  uint32_t u = __float_as_uint(v == 0.0f ? 0.0f : v);
  uint32_t asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}

__device__ __forceinline__ float load_score(const void* s, int b16, size_t i) {
  if (b16) return __uint_as_float(uint32_t(static_cast<const uint16_t*>(s)[i]) << 16);
  return static_cast<const float*>(s)[i];
}

template <bool W>
__global__ void __launch_bounds__(256) rank_keys_kernel(const void* __restrict__ scores, int b16,
                                                        const float* __restrict__ targets, const float* __restrict__ weights,
                                                        int N, int C, unsigned long long* __restrict__ items,
                                                        int* __restrict__ status) {
  __shared__ unsigned long long tile[kTile][kTile + 1];
  const int n0 = blockIdx.x * kTile, c0 = blockIdx.y * kTile;
  const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;     // 64 x 4
  int bad = 0;
  for (int r = ty; r < kTile; r += 4) {
    const int n = n0 + r, c = c0 + tx;
    unsigned long long it = 0;
    if (n < N && c < C) {
      const size_t i = size_t(n) * C + c;
      const float v = load_score(scores, b16, i);
      const float y = targets[i];
      if (!isfinite(v)) bad |= 1;
      if (!(y == 0.0f || y == 1.0f)) bad |= 2;
      uint32_t low = y == 1.0f ? 1u : 0u;
      if constexpr (W) {
        const float wt = weights[i];
        if (!(wt == 0.0f || wt == 1.0f)) bad |= 4;
        low |= wt == 1.0f ? 2u : 0u;
      }
      it = (static_cast<unsigned long long>(desc_key(v)) << 32) | low;
    }
    tile[r][tx] = it;
  }
  if (bad) atomicOr(status, bad);
  __syncthreads();
  for (int r = ty; r < kTile; r += 4) {                  // r: column within the tile, tx: row
    const int c = c0 + r, n = n0 + tx;
    if (n < N && c < C) items[size_t(c) * N + n] = tile[tx][r];
  }
}

__global__ void __launch_bounds__(kSortThreads) rank_sort_kernel(unsigned long long* __restrict__ buf0,
                                                                 unsigned long long* __restrict__ buf1, int N) {
  __shared__ int hist[4][256];
  __shared__ int base[256];
  __shared__ int wcnt[kSortWaves][256];
  const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
  const size_t col = size_t(blockIdx.x) * N;
  unsigned long long* src = buf0 + col;
  unsigned long long* dst = buf1 + col;

  for (int i = t; i < 4 * 256; i += kSortThreads) (&hist[0][0])[i] = 0;
  __syncthreads();
  for (int i = t; i < N; i += kSortThreads) {
    const uint32_t k = uint32_t(src[i] >> 32);
#pragma unroll
    for (int p = 0; p < 4; ++p) atomicAdd(&hist[p][(k >> (8 * p)) & 255], 1);
  }
  __syncthreads();
  const uint32_t k0 = uint32_t(src[0] >> 32);
  const unsigned long long lt = (1ull << lane) - 1ull;

  for (int p = 0; p < 4; ++p) {
    if (hist[p][(k0 >> (8 * p)) & 255] == N) continue;  // one digit value for every item: the pass is the identity
    if (w == 0) {                                        // exclusive scan of the 256 bins: 4 per lane + a wave scan
      int v[4], s = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) { v[j] = hist[p][4 * lane + j]; s += v[j]; }
      int inc = s;
#pragma unroll
      for (int o = 1; o < kWave; o <<= 1) {
        const int u = __shfl_up(inc, o, kWave);
        if (lane >= o) inc += u;
      }
      int run = inc - s;
#pragma unroll
      for (int j = 0; j < 4; ++j) { base[4 * lane + j] = run; run += v[j]; }
    }
    for (int i0 = 0; i0 < N; i0 += kSortThreads) {
      for (int i = t; i < kSortWaves * 256; i += kSortThreads) (&wcnt[0][0])[i] = 0;
      __syncthreads();
      const int i = i0 + t;
      const bool valid = i < N;
      const unsigned long long it = valid ? src[i] : 0ull;
      const int d = int((it >> (32 + 8 * p)) & 255);
      unsigned long long m = __ballot(valid);
#pragma unroll
      for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1;
        const unsigned long long bal = __ballot(bit);
        m &= bit ? bal : ~bal;
      }
      const int rank = __popcll(m & lt);
      if (valid && rank == 0) wcnt[w][d] = __popcll(m);
      __syncthreads();
      if (valid) {
        int off = base[d] + rank;
        for (int v = 0; v < w; ++v) off += wcnt[v][d];
        dst[off] = it;
      }
      __syncthreads();
      if (t < 256) {
        int s = 0;
#pragma unroll
        for (int v = 0; v < kSortWaves; ++v) s += wcnt[v][t];
        base[t] += s;
      }
      __syncthreads();
    }
    __threadfence();                                     // the scattered items are the next pass's input
    __syncthreads();
    unsigned long long* tmp = src;
    src = dst;
    dst = tmp;
  }
  if (src != buf0 + col) {                               // an odd number of passes ran: the result goes back to buf0
    for (int i = t; i < N; i += kSortThreads) dst[i] = src[i];
  }
}

// inclusive scan over the workgroup (sum for a, max for c, sum (BSUM) or max for b), carries from the previous tiles not
// included
template <bool BSUM = false>
__device__ __forceinline__ void block_scan3(int& a, int& b, int& c, int (*sh)[kSortWaves], int lane, int w) {
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int ua = __shfl_up(a, o, kWave), ub = __shfl_up(b, o, kWave), uc = __shfl_up(c, o, kWave);
    if (lane >= o) { a += ua; b = BSUM ? b + ub : max(b, ub); c = max(c, uc); }
  }
  if (lane == kWave - 1) { sh[0][w] = a; sh[1][w] = b; sh[2][w] = c; }
  __syncthreads();
  for (int v = 0; v < w; ++v) { a += sh[0][v]; b = BSUM ? b + sh[1][v] : max(b, sh[1][v]); c = max(c, sh[2][v]); }
}

// W: weighted items (bit 1 of the low word); count = the running sum of weights instead of the position
template <bool W>
__global__ void __launch_bounds__(kSortThreads) rank_scan_kernel(const unsigned long long* __restrict__ items, int N,
                                                                 double* __restrict__ ap, double* __restrict__ auc,
                                                                 int* __restrict__ n_pos) {
  __shared__ int sh[3][kSortWaves];
  __shared__ int tail[4];                                // last inclusive values of the tile: TP, TP and count at a group end,
                                                         // and (W) the count
  __shared__ double dsum[kSortWaves];
  __shared__ unsigned long long usum[kSortWaves];
  const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
  const unsigned long long* col = items + size_t(blockIdx.x) * N;
  int carry_tp = 0, carry_etp = 0, carry_ecnt = 0, carry_cnt = 0;
  double acc_ap = 0.0;
  unsigned long long acc_auc = 0ull;
  for (int i0 = 0; i0 < N; i0 += kSortThreads) {
    const int i = i0 + t;
    int lab = 0, wgt = 0, end = 0;
    if (i < N) {
      const unsigned long long it = col[i];
      wgt = W ? int((it >> 1) & 1ull) : 1;
      lab = int(it & 1ull) & wgt;
      end = (i == N - 1) || (uint32_t(col[i + 1] >> 32) != uint32_t(it >> 32));
    }
    int tp = lab, etp = W ? wgt : 0, ecnt = 0;
    block_scan3<W>(tp, etp, ecnt, sh, lane, w);          // pass 1: the running TP (W: and the running count, in etp)
    tp += carry_tp;
    const int cnt = W ? etp + carry_cnt : i + 1;
    // pass 2 (after the barrier that ends block_scan3's use of sh): the previous group end's TP and count
    int etp_in = end ? tp : 0, ecnt_in = end ? cnt : 0, dummy = 0;
    __syncthreads();
    int etp_inc = etp_in, ecnt_inc = ecnt_in;
    block_scan3(dummy, etp_inc, ecnt_inc, sh, lane, w);
    // exclusive = inclusive of the lane before (the previous wave's aggregate for lane 0), then the carry
    int etp_ex = __shfl_up(etp_inc, 1, kWave), ecnt_ex = __shfl_up(ecnt_inc, 1, kWave);
    if (lane == 0) {
      etp_ex = 0; ecnt_ex = 0;
      for (int v = 0; v < w; ++v) { etp_ex = max(etp_ex, sh[1][v]); ecnt_ex = max(ecnt_ex, sh[2][v]); }
    }
    etp_ex = max(etp_ex, carry_etp);
    ecnt_ex = max(ecnt_ex, carry_ecnt);
    if (i < N && end && cnt > 0) {                        // (cnt == 0: every item so far has weight 0 - no 0 / 0 term)
      const int dtp = tp - etp_ex, dfp = (cnt - tp) - (ecnt_ex - etp_ex);
      acc_ap += double(dtp) * double(tp) / double(cnt);
      acc_auc += static_cast<unsigned long long>(dfp) * static_cast<unsigned long long>(tp + etp_ex);
    }
    if (t == kSortThreads - 1) {
      tail[0] = tp; tail[1] = max(etp_inc, carry_etp); tail[2] = max(ecnt_inc, carry_ecnt); tail[3] = cnt;
    }
    __syncthreads();
    carry_tp = tail[0];
    carry_etp = tail[1];
    carry_ecnt = tail[2];
    carry_cnt = tail[3];
    __syncthreads();
  }
  // fixed-order reductions: a butterfly inside each wave, then the waves in index order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc_ap += __shfl_xor(acc_ap, o, kWave);
    acc_auc += __shfl_xor(acc_auc, o, kWave);
  }
  if (lane == 0) { dsum[w] = acc_ap; usum[w] = acc_auc; }
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    unsigned long long u = 0ull;
    for (int v = 0; v < kSortWaves; ++v) { s += dsum[v]; u += usum[v]; }
    const int np = carry_tp, nn = (W ? carry_cnt : N) - carry_tp;
    ap[blockIdx.x] = np == 0 ? 0.0 : (nn == 0 ? 1.0 : s / double(np));
    auc[blockIdx.x] = (np == 0 || nn == 0) ? __builtin_nan("") : double(u) / (2.0 * double(np) * double(nn));
    n_pos[blockIdx.x] = np;
  }
}

bool rank_metrics_shape_ok(int N, int C) {
  return N >= 1 && C >= 1 && N <= (1 << 22) && C <= (1 << 16) && static_cast<long long>(N) * C <= 0x7fffffffLL;
}

template <bool W>
int rank_metrics_run(const char* what, const void* scores, int scores_b16, const float* targets, const float* weights, int N,
                     int C, void* ws, double* ap, double* auc, int* n_pos, int* status, eat_stream_t stream) {
  if (!rank_metrics_shape_ok(N, C))
    return fail(EAT_EINVAL, "%s: N = %d, C = %d (1 <= N <= 2^22, 1 <= C <= 2^16, N*C < 2^31)", what, N, C);
  if (!scores || !targets || (W && !weights) || !ws || !ap || !auc || !n_pos || !status)
    return fail(EAT_EINVAL, "%s: null pointer", what);
  clear_stale_error();
  hipStream_t s = static_cast<hipStream_t>(stream);
  auto* buf0 = static_cast<unsigned long long*>(ws);
  auto* buf1 = buf0 + static_cast<size_t>(N) * C;
  if (hipMemsetAsync(status, 0, sizeof(int), s) != hipSuccess)
    return fail(EAT_ELAUNCH, "%s: status memset: %s", what, hipGetErrorString(hipGetLastError()));
  hipLaunchKernelGGL(rank_keys_kernel<W>, dim3((N + kTile - 1) / kTile, (C + kTile - 1) / kTile), dim3(256), 0, s, scores,
                     scores_b16 ? 1 : 0, targets, weights, N, C, buf0, status);
  if (int rc = check_launch("eat_rank_metrics: keys")) return rc;
  hipLaunchKernelGGL(rank_sort_kernel, dim3(C), dim3(kSortThreads), 0, s, buf0, buf1, N);
  if (int rc = check_launch("eat_rank_metrics: sort")) return rc;
  hipLaunchKernelGGL(rank_scan_kernel<W>, dim3(C), dim3(kSortThreads), 0, s, buf0, N, ap, auc, n_pos);
  return check_launch("eat_rank_metrics: scan");
}

}  // namespace
}  // namespace eat

extern "C" long long eat_rank_metrics_ws_bytes(int N, int C) {
  if (!eat::rank_metrics_shape_ok(N, C))
    return eat::fail(EAT_EINVAL, "eat_rank_metrics_ws_bytes: N = %d, C = %d (1 <= N <= 2^22, 1 <= C <= 2^16, N*C < 2^31)", N, C);
  return 2LL * 8LL * N * C;
}

extern "C" int eat_rank_metrics(const void* scores, int scores_b16, const float* targets, int N, int C, void* ws,
                                double* ap, double* auc, int* n_pos, int* status, eat_stream_t stream) {
  return eat::rank_metrics_run<false>("eat_rank_metrics", scores, scores_b16, targets, nullptr, N, C, ws, ap, auc, n_pos,
                                      status, stream);
}

extern "C" int eat_rank_metrics_masked(const void* scores, int scores_b16, const float* targets, const float* weights, int N,
                                       int C, void* ws, double* ap, double* auc, int* n_pos, int* status, eat_stream_t stream) {
  return eat::rank_metrics_run<true>("eat_rank_metrics_masked", scores, scores_b16, targets, weights, N, C, ws, ap, auc, n_pos,
                                     status, stream);
}
