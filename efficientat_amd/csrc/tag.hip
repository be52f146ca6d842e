// Device side of the long-recording tagger (include/eat_tag.h): what the reference's windowed_inference.py does per window
// on the host - sigmoid, device->host copy, numpy argsort - and what librosa.load does per file - dequantise, down-mix,
// resample - as two kernels over all windows / all samples at once.  (The windowed mel front-end is in mel.hip.)
#include "eat_common.h"
#include "loss_terms.h"
#include "../../include/eat_tag.h"

namespace {

constexpr int kRowsPerBlock = 4;      // one wavefront per row

// eat::sigmoid is ONE expression for p, used by the store of probs_all and by every selection round: the rounds recompute
// p from the logits (C / 64 exps per lane and round, L1 hits) instead of caching a row whose length has no bound.

// (p, i) ranks before (q, j): larger probability first, equal probabilities by ascending class index
__device__ __forceinline__ bool before(float p, int i, float q, int j) { return p > q || (p == q && i < j); }

// Round r takes the first element, in that order, that ranks strictly after the winner of round r - 1: a selection sort
// without marks, k * ceil(C / 64) steps per lane.  No element is taken twice because (p, i) pairs are distinct.
__global__ __launch_bounds__(64 * kRowsPerBlock) void tag_topk_kernel(const float* __restrict__ logits, int N, int C, int k,
                                                                      float* __restrict__ prob, int* __restrict__ index,
                                                                      float* __restrict__ probs_all) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * kRowsPerBlock + (threadIdx.x >> 6);
  if (row >= N) return;                                    // wave-uniform
  const float* z = logits + row * C;
  if (probs_all != nullptr)
    for (int i = lane; i < C; i += 64) probs_all[row * C + i] = eat::sigmoid(z[i]);
  float lp = 2.0f;                                         // the winner of the previous round; p <= 1 ranks after (2, -1)
  int li = -1;
  for (int r = 0; r < k; ++r) {
    float bp = -1.0f;                                      // p >= 0 ranks before (-1, C)
    int bi = C;
    for (int i = lane; i < C; i += 64) {
      const float p = eat::sigmoid(z[i]);
      if (before(lp, li, p, i) && before(p, i, bp, bi)) { bp = p; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float qp = __shfl_xor(bp, o, 64);
      const int qi = __shfl_xor(bi, o, 64);
      if (before(qp, qi, bp, bi)) { bp = qp; bi = qi; }
    }
    lp = bp;
    li = bi;
    if (lane == 0) {
      prob[row * k + r] = bp;
      index[row * k + r] = bi;
    }
  }
}

// One output sample per thread.  Tap index t = j * down - i * up + half lies in [0, n_taps) for
// ceil((j * down - half) / up) <= i <= floor((j * down + half) / up): 2 * half / up + 1 input frames at the most
// (21 when up >= down, 28 for 44.1 -> 32 kHz), neighbours in a wave reading the same frames.  The sum runs in fp64:
// the taps and the frames are fp32 values, so the result is the correctly rounded one up to the final conversion.
template <bool kI16>
__global__ __launch_bounds__(256) void resample_mono_kernel(const void* __restrict__ in, long long n_in, int channels, int up,
                                                            int down, const float* __restrict__ taps, int half,
                                                            float* __restrict__ out, long long n_out) {
  const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_out) return;
  const long long c = j * down;                            // > 2^31 after 150 s of 32 kHz output at down = 441
  long long lo = c - half;
  lo = lo <= 0 ? 0 : (lo + up - 1) / up;
  const long long hi = min((c + half) / up, n_in - 1);
  const float scale = (kI16 ? 1.0f / 32768.0f : 1.0f) / (float)channels;
  double acc = 0.0;
  for (long long i = lo; i <= hi; ++i) {
    float s = 0.0f;
    for (int ch = 0; ch < channels; ++ch) {
      if constexpr (kI16) s += (float)static_cast<const short*>(in)[i * channels + ch];
      else s += static_cast<const float*>(in)[i * channels + ch];
    }
    acc = fma((double)(s * scale), (double)taps[c - i * up + half], acc);
  }
  out[j] = (float)acc;
}

}  // namespace

extern "C" int eat_tag_topk(const float* logits, int N, int C, int k, float* prob, int* index, float* probs_all,
                            eat_stream_t stream) {
  eat::clear_stale_error();
  if (N < 1 || C < 1 || k < 1 || k > C || k > 64)
    return eat::fail(EAT_EINVAL, "eat_tag_topk: need N >= 1, C >= 1 and 1 <= k <= min(C, 64) (got N=%d C=%d k=%d)", N, C, k);
  hipLaunchKernelGGL(tag_topk_kernel, dim3((N + kRowsPerBlock - 1) / kRowsPerBlock), dim3(64 * kRowsPerBlock), 0,
                     (hipStream_t)stream, logits, N, C, k, prob, index, probs_all);
  return eat::check_launch("eat_tag_topk");
}

extern "C" int eat_resample_mono(const void* in, int in_i16, long long n_in, int channels, int up, int down,
                                 const float* taps, int n_taps, float* out, long long n_out, eat_stream_t stream) {
  eat::clear_stale_error();
  if (up < 1 || down < 1 || channels < 1 || n_in < 1)
    return eat::fail(EAT_EINVAL, "eat_resample_mono: need up, down, channels, n_in >= 1 (got %d, %d, %d, %lld)", up, down,
                     channels, n_in);
  if (n_taps < 1 || n_taps % 2 == 0) return eat::fail(EAT_EINVAL, "eat_resample_mono: n_taps=%d must be odd", n_taps);
  if (n_in > (1LL << 61) / (up > down ? up : down))         // n_in * up and n_out * down stay inside 64 bits
    return eat::fail(EAT_EINVAL, "eat_resample_mono: n_in=%lld is too long for up=%d down=%d", n_in, up, down);
  const long long want = (n_in * up + down - 1) / down;
  if (n_out != want)
    return eat::fail(EAT_EINVAL, "eat_resample_mono: n_out=%lld, but ceil(n_in * up / down) = %lld", n_out, want);
  const long long blocks = (n_out + 255) / 256;
  if (blocks > 0x7fffffffLL) return eat::fail(EAT_EINVAL, "eat_resample_mono: n_out=%lld needs too many blocks", n_out);
  const int half = (n_taps - 1) / 2;
  if (in_i16)
    hipLaunchKernelGGL(resample_mono_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, n_in,
                       channels, up, down, taps, half, out, n_out);
  else
    hipLaunchKernelGGL(resample_mono_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, in, n_in,
                       channels, up, down, taps, half, out, n_out);
  return eat::check_launch("eat_resample_mono");
}
