// Training batch of ex_fsd50k.py built on the device from a RAGGED resident clip bank (datasets/fsd50k.py: gain, pad or random
// crop, roll, MixupDataset): one flat sample buffer plus per-clip offsets and lengths, because FSD50K clips run from 0.3 s to
// 30 s and a long clip's window is redrawn on every fetch.
//   eat_wave_augment_ragged  launch 1: the mean of each wave-mixed slot's window (fp64, fixed order) into a workspace;
//                            launch 2: crop / pad + gain + roll + wave-mix of the rows, and the mixed multi-hot label rows
#include "eat_common.h"
#include "event_bank.h"
#include "reduce.h"

namespace {

constexpr int kMeanThreads = 1024;     // one block per slot: 16 waves of 16-byte loads keep ~64 KB in flight per window

// One slot (clip i cropped at st): where its window starts in `waves` and how many samples of it exist.  ok = false: a table
// entry or a bank entry that would read outside `waves` or outside the clip - nothing is read for such a slot.
struct Slot {
  long long src;     // offsets[i] + st
  int w;             // min(lengths[i] - st, L)
  int whole;         // the window is the whole clip: its sum is clip_sum[i]
  bool ok;
};

__device__ __forceinline__ Slot ragged_slot(const long long* __restrict__ offsets, const int* __restrict__ lengths,
                                            long long n_bank, long long n_samples, int L, int i, int st) {
  if (i < 0 || i >= n_bank) return Slot{0, 0, 0, false};
  const long long off = offsets[i];                             // (issued with clip_window's load of lengths[i])
  const eat::ClipWindow cw = eat::clip_window(lengths, n_bank, L, i, st);
  if (!cw.ok || off < 0 || off > n_samples - cw.len) return Slot{0, 0, 0, false};
  return Slot{off + st, cw.w, st == 0 && cw.len <= L, true};
}

struct Row {
  Slot s0, s1;
  bool ok, wm;
};

__device__ __forceinline__ Row ragged_row(const long long* __restrict__ offsets, const int* __restrict__ lengths, long long n_bank,
                                          long long n_samples, int L, const int* __restrict__ idx, const int* __restrict__ start,
                                          int b) {
  Row r;
  const int i1 = idx[2 * b + 1];
  r.s0 = ragged_slot(offsets, lengths, n_bank, n_samples, L, idx[2 * b], start[2 * b]);
  r.s1 = i1 == -1 ? Slot{0, 0, 0, false} : ragged_slot(offsets, lengths, n_bank, n_samples, L, i1, start[2 * b + 1]);
  r.ok = r.s0.ok && (i1 == -1 || r.s1.ok);
  r.wm = r.ok && i1 != -1;
  return r;
}

// ---- launch 1.  Block k = slot k of row k / 2.  win_mean[k] = amp_k / L * sum of the slot's window for the slots of wave-mixed
// rows (0 for every other slot).  A whole clip takes clip_sum; a cropped one is summed here in fp64 in a fixed order: up to 3
// scalar samples in front of the first 16-byte boundary and the < 4 behind the last one go to thread 0, thread t adds the
// float4s t, t + 1024, ... in order (x, y, z, w), then a fixed butterfly and the 16 waves in order.  The order depends on the
// window's address and length only, so repeated calls are bit-identical.
__global__ __launch_bounds__(kMeanThreads) void ragged_mean_kernel(
    const float* __restrict__ waves, long long n_samples, const long long* __restrict__ offsets, const int* __restrict__ lengths,
    const double* __restrict__ clip_sum, long long n_bank, int L, const int* __restrict__ idx, const int* __restrict__ start,
    const float* __restrict__ amp, double* __restrict__ win_mean) {
  __shared__ double s_red[kMeanThreads / 64];
  const int k = blockIdx.x, t = threadIdx.x;
  const Row r = ragged_row(offsets, lengths, n_bank, n_samples, L, idx, start, k >> 1);
  const Slot s = (k & 1) ? r.s1 : r.s0;
  if (!r.wm || s.whole) {                                       // block-uniform
    if (t == 0) win_mean[k] = r.wm ? (double)amp[k] * clip_sum[idx[k]] / (double)L : 0.0;
    return;
  }
  const float* x = waves + s.src;
  const int head = min(s.w, (int)((4 - ((reinterpret_cast<uintptr_t>(x) >> 2) & 3)) & 3));
  const int nv = (s.w - head) >> 2;
  const float4* xv = reinterpret_cast<const float4*>(x + head);
  double acc = 0.0;
  if (t == 0)
    for (int n = 0; n < head; ++n) acc += (double)x[n];
  int v = t;
  for (; v + 3 * kMeanThreads < nv; v += 4 * kMeanThreads) {   // four loads in flight per thread
    const float4 q0 = xv[v], q1 = xv[v + kMeanThreads], q2 = xv[v + 2 * kMeanThreads], q3 = xv[v + 3 * kMeanThreads];
    acc += (double)q0.x; acc += (double)q0.y; acc += (double)q0.z; acc += (double)q0.w;
    acc += (double)q1.x; acc += (double)q1.y; acc += (double)q1.z; acc += (double)q1.w;
    acc += (double)q2.x; acc += (double)q2.y; acc += (double)q2.z; acc += (double)q2.w;
    acc += (double)q3.x; acc += (double)q3.y; acc += (double)q3.z; acc += (double)q3.w;
  }
  for (; v < nv; v += kMeanThreads) {
    const float4 q = xv[v];
    acc += (double)q.x; acc += (double)q.y; acc += (double)q.z; acc += (double)q.w;
  }
  if (t == 0)
    for (int n = head + 4 * nv; n < s.w; ++n) acc += (double)x[n];
  acc = eat::wave_sum_d(acc);
  if ((t & 63) == 0) s_red[t >> 6] = acc;
  __syncthreads();
  if (t == 0) {
    double tot = 0.0;
#pragma unroll
    for (int j = 0; j < kMeanThreads / 64; ++j) tot += s_red[j];
    win_mean[k] = (double)amp[k] * tot / (double)L;
  }
}

// ---- launch 2.  Block (x, b) writes a slice of out row b as wave_augment_kernel does: 4 outputs per thread and trip, one
// 16-byte store from the first 16-byte boundary of the row on, scalar stores for the < 4 samples in front of it and behind the
// last whole group.  A source sample outside the slot's window is the padding: exactly 0, whatever the gain.
__global__ __launch_bounds__(256) void ragged_gather_kernel(
    const float* __restrict__ waves, long long n_samples, const long long* __restrict__ offsets, const int* __restrict__ lengths,
    const float* __restrict__ bank_y, long long n_bank, int L, int C, const int* __restrict__ idx, const int* __restrict__ start,
    const int* __restrict__ shift, const float* __restrict__ amp, const float* __restrict__ mix,
    const double* __restrict__ win_mean, float* __restrict__ out, float* __restrict__ yy) {
  const int b = blockIdx.y;
  const Row r = ragged_row(offsets, lengths, n_bank, n_samples, L, idx, start, b);
  const bool ok = r.ok, wm = r.wm;
  // roll by s: source position (n - s) mod L; s reduced to [0, L) once per block
  const int s0 = (int)(((long long)shift[2 * b] % L + L) % L);
  const int s1 = wm ? (int)(((long long)shift[2 * b + 1] % L + L) % L) : 0;
  const float a0 = amp[2 * b], a1 = wm ? amp[2 * b + 1] : 0.0f;
  const float l = wm ? mix[b] : 1.0f, lm = 1.0f - l;
  const float m0 = wm ? (float)win_mean[2 * b] : 0.0f;
  const float m1 = wm ? (float)win_mean[2 * b + 1] : 0.0f;
  const float* r0 = waves + (ok ? r.s0.src : 0);
  const float* r1 = waves + (wm ? r.s1.src : 0);
  const int w0 = ok ? r.s0.w : 0, w1 = wm ? r.s1.w : 0;
  float* o = out + (long long)b * L;

  auto sample = [&](int n) -> float {
    if (!ok) return __builtin_nanf("");
    int p = n - s0;
    p += p < 0 ? L : 0;
    const float x0 = p < w0 ? a0 * r0[p] : 0.0f;
    if (!wm) return x0;
    int q = n - s1;
    q += q < 0 ? L : 0;
    const float x1 = q < w1 ? a1 * r1[q] : 0.0f;
    return l * (x0 - m0) + lm * (x1 - m1);
  };

  const int head = min(L, (int)((4 - ((reinterpret_cast<uintptr_t>(o) >> 2) & 3)) & 3));
  const int nv = (L - head) >> 2;
  const int tail0 = head + 4 * nv;
  const int stride = gridDim.x * blockDim.x;
  for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < nv; v += stride) {
    const int n = head + 4 * v;
    *reinterpret_cast<float4*>(o + n) = make_float4(sample(n), sample(n + 1), sample(n + 2), sample(n + 3));
  }
  if (blockIdx.x == 0) {
    if (threadIdx.x < 8) {
      const int n = threadIdx.x < 4 ? threadIdx.x : tail0 + threadIdx.x - 4;
      if ((threadIdx.x < 4 && n < head) || (threadIdx.x >= 4 && n < L)) o[n] = sample(n);
    }
    if (yy != nullptr) {
      const float* y0 = bank_y + (ok ? (long long)idx[2 * b] * C : 0);
      const float* y1 = bank_y + (wm ? (long long)idx[2 * b + 1] * C : 0);
      const double ld = wm ? (double)mix[b] : 1.0;
      float* yo = yy + (long long)b * 2 * C;
      for (int c = threadIdx.x; c < C; c += blockDim.x) {
        // (both products are exact in fp64, so the sum is rounded once there and once to fp32, fused or not)
        yo[c] = !ok ? __builtin_nanf("") : (wm ? (float)(ld * (double)y0[c] + (1.0 - ld) * (double)y1[c]) : y0[c]);
        yo[C + c] = ok ? 1.0f : __builtin_nanf("");
      }
    }
  }
}

}  // namespace

extern "C" int eat_wave_augment_ragged(const float* waves, long long n_samples, const long long* offsets, const int* lengths,
                                       const double* clip_sum, const float* bank_y, long long n_bank, int L, int C,
                                       const int* idx, const int* start, const int* shift, const float* amp, const float* mix,
                                       double* win_mean, float* out, float* yy, int B, eat_stream_t stream) {
  eat::clear_stale_error();
  if (B < 1 || L < 1 || n_bank < 1 || n_samples < 1 || (yy != nullptr && (C < 1 || 2LL * B * C > 0x7fffffffLL)))
    return eat::fail(EAT_EINVAL, "eat_wave_augment_ragged: bad shape (B = %d, L = %d, n_bank = %lld, n_samples = %lld, C = %d)", B,
                     L, n_bank, n_samples, C);
  if (!waves || !offsets || !lengths || !clip_sum || !idx || !start || !shift || !amp || !mix || !win_mean || !out ||
      (yy && !bank_y))
    return eat::fail(EAT_EINVAL, "eat_wave_augment_ragged: a required pointer is NULL");
  if (B > 65535) return eat::fail(EAT_EINVAL, "eat_wave_augment_ragged: B = %d > 65535", B);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ragged_mean_kernel, dim3((unsigned)(2 * B)), dim3(kMeanThreads), 0, s, waves, n_samples, offsets, lengths,
                     clip_sum, n_bank, L, idx, start, amp, win_mean);
  const long long nv = (long long)L / 4;
  long long bx = (nv + 255) / 256;
  if (bx < 1) bx = 1;
  if (bx > 1024) bx = 1024;
  hipLaunchKernelGGL(ragged_gather_kernel, dim3((unsigned)bx, (unsigned)B), dim3(256), 0, s, waves, n_samples, offsets, lengths,
                     bank_y, n_bank, L, C, idx, start, shift, amp, mix, win_mean, out, yy);
  return eat::check_launch("eat_wave_augment_ragged");
}
