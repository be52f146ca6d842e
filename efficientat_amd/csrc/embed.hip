// Device side of the embedding extractor (include/eat_embed.h): per-channel means of every feature map of a forward,
// over the whole plane or over time segments, in ONE launch for all maps, all samples and all segments.
//
// Geometry.  Output channel d of sample b is one (F, T) plane of the map whose [off, off + C) covers d, and one wavefront
// owns it from the first load to the last store: four planes per block, side by side, no block-wide barrier anywhere.
// That packs the 4 x 32 ... 8 x 63 planes of the late maps four to a block and still gives a 64 x 500 plane of the
// early maps 64 lanes x 8 loads of 16 bytes in flight.  Blocks are numbered channel-group major, sample minor, so the
// blocks of the early, large maps are dispatched first and the small ones fill in behind them.  The map of a channel is
// found by one lane per map (hence n_maps <= 64) and a ballot, and the first 64 segments are fetched together with the
// plane: two dependent memory round trips from the start of a wavefront to its stores.
//
// Per plane: (1) column sums over f into LDS - lanes run along t (coalesced rows, 16-byte loads where every row start
// is 16-byte aligned, 8-byte or 4-byte loads otherwise); a plane narrower than the wavefront has R = 64 / ceil(T / V)
// rows in flight at once, whose R partial rows are folded in a fixed order; (2) every segment is summed from those
// column sums: one lane per segment for short segments, the whole wavefront (strided partial sums + shuffle tree) for
// long ones.  Each input element is read once however the segments overlap.  No atomics: the order of every addition is
// fixed.
#include <cstdint>

#include "eat_common.h"
#include "../../include/eat_embed.h"

namespace {

constexpr int kThreads = 256;
constexpr int kPlanesPerBlock = 4;      // = wavefronts per block
constexpr int kColCap = 1024;           // column sums of one plane held in LDS, per wavefront; wider planes: pool_direct
constexpr int kShortSeg = 16;           // segments up to this many columns are summed by one lane

// LDS written by one lane of the wavefront is read by another: order the two (no barrier instruction is needed inside a wave)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int V> struct Vec;
template <> struct Vec<1> { using type = float; };
template <> struct Vec<2> { using type = float2; };
template <> struct Vec<4> { using type = float4; };

template <int V>
__device__ __forceinline__ void add_row(float (&acc)[V], const float* p) {
  const typename Vec<V>::type v = *reinterpret_cast<const typename Vec<V>::type*>(p);
  if constexpr (V == 1) acc[0] += v;
  if constexpr (V == 2) { acc[0] += v.x; acc[1] += v.y; }
  if constexpr (V == 4) { acc[0] += v.x; acc[1] += v.y; acc[2] += v.z; acc[3] += v.w; }
}

// col[t] = sum_f x[f, t], t in [0, T).  V > 1 needs T % V == 0 and x aligned to 4 V bytes.  col holds max(T, NT * V)
// floats.  Ends with a wave_sync: col is readable by the whole wavefront afterwards.
template <int V>
__device__ void column_sums(const float* __restrict__ x, int F, int T, float* col, int tid) {
  constexpr int NT = eat::kWave;
  constexpr int kLoads = V == 4 ? 6 : 8;    // loads in flight per lane; 6 x 16 bytes keep the kernel at 8 waves per SIMD
  const int G = (T + V - 1) / V;            // column groups per row
  if (G <= NT) {
    const int R = NT / G;                   // rows in flight; R * G * V <= NT * V floats of partial rows
    const int r = tid / G, g = tid - r * G;
    if (r < R) {
      float acc[V] = {};
      const float* p = x + (long long)r * T + g * V;
      const long long step = (long long)R * T;
#pragma unroll kLoads
      for (int f = r; f < F; f += R, p += step) add_row<V>(acc, p);
#pragma unroll
      for (int k = 0; k < V; ++k) col[(r * G + g) * V + k] = acc[k];
    }
    wave_sync();
    if (R > 1) {
      // G * V == T here (V == 1: G = T; V > 1: T % V == 0); column t is folded by one lane, into partial row 0
      for (int t = tid; t < T; t += NT) {
        float s = col[t];
        for (int q = 1; q < R; ++q) s += col[q * T + t];
        col[t] = s;
      }
      wave_sync();
    }
  } else {
    for (int g = tid; g < G; g += NT) {
      float acc[V] = {};
      const float* p = x + g * V;
#pragma unroll kLoads
      for (int f = 0; f < F; ++f, p += T) add_row<V>(acc, p);
#pragma unroll
      for (int k = 0; k < V; ++k) col[g * V + k] = acc[k];
    }
    wave_sync();
  }
}

// out[s * D] = sum of col[lo_s, hi_s) / (F (hi_s - lo_s)) for every segment, lo / hi clamped into [0, T].
// (lo0, hi0): segment `lane` as the table holds it, loaded by the caller ahead of the plane's own loads.
__device__ void segment_means(const float* col, int F, int T, const int* __restrict__ seg, int n_seg, int lo0, int hi0,
                              float* __restrict__ out, long long D, int lane) {
  constexpr int NT = eat::kWave;
  for (int s0 = 0; s0 < n_seg; s0 += NT) {          // the same trip count in every lane of the wavefront
    const int s = s0 + lane;
    int lo = 0, hi = 0;
    if (s < n_seg) {
      lo = min(max(s0 == 0 ? lo0 : seg[2 * s], 0), T);
      hi = min(max(s0 == 0 ? hi0 : seg[2 * s + 1], 0), T);
    }
    const int len = hi - lo;
    float sum = 0.0f;
    if (len <= kShortSeg)
      for (int t = lo; t < hi; ++t) sum += col[t];
    unsigned long long longs = __ballot(len > kShortSeg);
    while (longs != 0) {                            // wave-uniform
      const int j = __ffsll((long long)longs) - 1;
      longs &= longs - 1;
      const int jlo = __shfl(lo, j, 64), jhi = __shfl(hi, j, 64);
      float a = 0.0f;
      for (int t = jlo + lane; t < jhi; t += 64) a += col[t];
      a = eat::wave_sum(a);
      if (lane == j) sum = a;
    }
    if (s < n_seg) out[s * D] = len > 0 ? sum / ((float)F * (float)len) : 0.0f;
  }
}

// T > kColCap: every segment summed straight from the map (an element is read once per covering segment)
__device__ void pool_direct(const float* __restrict__ x, int F, int T, const int* __restrict__ seg, int n_seg,
                            float* __restrict__ out, long long D, int lane) {
  for (int s = 0; s < n_seg; ++s) {
    const int lo = min(max(seg[2 * s], 0), T), hi = min(max(seg[2 * s + 1], 0), T);
    float a = 0.0f;
    for (int f = 0; f < F; ++f) {
      const float* row = x + (long long)f * T;
      for (int t = lo + lane; t < hi; t += eat::kWave) a += row[t];
    }
    a = eat::wave_sum(a);
    if (lane == 0) out[s * D] = hi > lo ? a / ((float)F * (float)(hi - lo)) : 0.0f;
  }
}

__global__ __launch_bounds__(kThreads, 8) void embed_pool_kernel(const long long* __restrict__ maps, const int* __restrict__ dims,
                                                             const int* __restrict__ seg, int n_maps, int B, int n_seg, int D,
                                                             float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) float lds[kPlanesPerBlock][kColCap];
  constexpr int NT = eat::kWave;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int b = blockIdx.x % (unsigned)B;
  const int d = (blockIdx.x / (unsigned)B) * kPlanesPerBlock + wave;
  if (d >= D) return;                                          // wave-uniform, and nothing below synchronises the block
  float* const o = out + (long long)b * n_seg * D + d;

  // lane l looks at map l: does [off, off + C) cover d?
  int C = 0, F = 0, T = 0, off = 0;
  long long addr = 0;
  if (lane < n_maps) {
    addr = maps[lane];
    C = dims[4 * lane];
    F = dims[4 * lane + 1];
    T = dims[4 * lane + 2];
    off = dims[4 * lane + 3];
  }
  const long long c = (long long)d - off;
  const unsigned long long hits = __ballot(lane < n_maps && C >= 1 && F >= 1 && T >= 1 && c >= 0 && c < C);
  if (hits == 0) {                                             // no map covers the channel: zeros
    for (int s = lane; s < n_seg; s += NT) o[(long long)s * D] = 0.0f;
    return;
  }
  const int l = __ffsll((long long)hits) - 1;                  // the first map listed wins
  C = __shfl(C, l, 64);
  F = __shfl(F, l, 64);
  T = __shfl(T, l, 64);
  off = __shfl(off, l, 64);
  addr = ((long long)__shfl((int)(addr >> 32), l, 64) << 32) | (unsigned)__shfl((int)addr, l, 64);
  const float* x = reinterpret_cast<const float*>(addr) + ((long long)b * C + (d - off)) * ((long long)F * T);
  const int* sg = seg + (long long)l * n_seg * 2;
  int lo0 = 0, hi0 = 0;                                        // in flight together with the plane's loads
  if (lane < n_seg) {
    lo0 = sg[2 * lane];
    hi0 = sg[2 * lane + 1];
  }
  if (T > kColCap) {
    pool_direct(x, F, T, sg, n_seg, o, D, lane);
    return;
  }
  float* col = lds[wave];
  const uintptr_t a = reinterpret_cast<uintptr_t>(x);
  if ((T & 3) == 0 && (a & 15) == 0) column_sums<4>(x, F, T, col, lane);
  else if ((T & 1) == 0 && (a & 7) == 0) column_sums<2>(x, F, T, col, lane);
  else column_sums<1>(x, F, T, col, lane);
  segment_means(col, F, T, sg, n_seg, lo0, hi0, o, D, lane);
}

}  // namespace

extern "C" int eat_embed_pool(const long long* maps, const int* dims, const int* seg, int n_maps, int B, int n_seg, int D,
                              float* out, eat_stream_t stream) {
  eat::clear_stale_error();
  if (n_maps < 1 || n_maps > 64) return eat::fail(EAT_EINVAL, "eat_embed_pool: n_maps=%d lies outside [1, 64]", n_maps);
  if (B < 1) return eat::fail(EAT_EINVAL, "eat_embed_pool: need B >= 1 (got %d)", B);
  if (n_seg < 1) return eat::fail(EAT_EINVAL, "eat_embed_pool: need n_seg >= 1 (got %d)", n_seg);
  if (D < 1) return eat::fail(EAT_EINVAL, "eat_embed_pool: need D >= 1 (got %d)", D);
  const long long blocks = ((long long)D + kPlanesPerBlock - 1) / kPlanesPerBlock * B;
  if (blocks > 0x7fffffffLL)
    return eat::fail(EAT_EINVAL, "eat_embed_pool: B=%d x ceil(D=%d / %d) = %lld blocks exceed the grid limit of 2147483647: "
                     "chunk the call over B", B, D, kPlanesPerBlock, blocks);
  hipLaunchKernelGGL(embed_pool_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, maps, dims, seg, n_maps,
                     B, n_seg, D, out);
  return eat::check_launch("eat_embed_pool");
}
