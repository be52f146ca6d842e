// Generic (any geometry) gradients of the depthwise and stem convolutions for gfx950 (autograd of F.conv2d, SURVEY.md Appendix
// C) and every eat_dw_conv_*grad* / *bwd* entry point: each tries dw_plane.hip first (eat::dw_*_try), then the kernels below.
#include "eat_common.h"

namespace {

// ---- depthwise data gradient: dx[c,i,j] = sum_{u,v} w[c,u,v] dz[c,(i+p-u)/s,(j+p-v)/s] (+ res) ----------
template <int K, int STRIDE>
__global__ __launch_bounds__(256) void dw_dgrad_kernel(const float* __restrict__ dz, const float* __restrict__ w,
                                                       const float* __restrict__ res, float* __restrict__ dx,
                                                       int C, int F, int T, int Fo, int To, int per_plane_w) {
  constexpr int P = (K - 1) / 2;
  const int plane = blockIdx.y, c = plane % C;
  float wr[K * K];
#pragma unroll
  for (int i = 0; i < K * K; ++i) wr[i] = w[(size_t)(per_plane_w ? plane : c) * K * K + i];
  const float* g = dz + (size_t)plane * Fo * To;
  const size_t base = (size_t)plane * F * T;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < F * T; e += gridDim.x * blockDim.x) {
    const int i = e / T, j = e - i * T;
    float acc = res ? res[base + e] : 0.0f;
#pragma unroll
    for (int u = 0; u < K; ++u) {
      const int ii = i + P - u;
      if (ii < 0 || (ii % STRIDE) != 0) continue;
      const int io = ii / STRIDE;
      if (io >= Fo) continue;
#pragma unroll
      for (int v = 0; v < K; ++v) {
        const int jj = j + P - v;
        if (jj < 0 || (jj % STRIDE) != 0) continue;
        const int jo = jj / STRIDE;
        if (jo < To) acc = fmaf(wr[u * K + v], g[(size_t)io * To + jo], acc);
      }
    }
    dx[base + e] = acc;
  }
}

// ---- depthwise data gradient, stride 2, sliding form: one thread per dx column j walking down the
// rows; only the taps whose parity matches contribute (<= ceil(K/2)^2 loads per element instead of
// K*K predicated iterations), lanes on consecutive j read dz at half stride (coalesced).
template <int K>
__global__ __launch_bounds__(256) void dw_dgrad_s2_kernel(const float* __restrict__ dz, const float* __restrict__ w,
                                                          const float* __restrict__ res, float* __restrict__ dx,
                                                          int n_planes, int C, int F, int T, int Fo, int To,
                                                          int per_plane_w) {
  // Polyphase form: dx[i][j] = sum over the taps (u, v) with (i + P - u), (j + P - v) even of w[u][v] dz[(i+P-u)/2][(j+P-v)/2].
  // The column parity of a thread is fixed, so its tap columns v = v0 + 2q are selected ONCE into registers (the round-1
  // kernel indexed the tap array with run-time (u, v) inside the row loop); the rows are walked in pairs (2m, 2m+1), whose
  // tap rows are compile-time constants, over a sliding window of dz rows m-1, m, m+1 - every dz row is loaded once per
  // thread, one row ahead of its use.  Writes are coalesced 256-byte row segments per wave.
  constexpr int P = (K - 1) / 2;
  constexpr int NV = (K + 1) / 2;
  const int j = blockIdx.x * 64 + (threadIdx.x & 63);
  const int plane = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (plane >= n_planes || j >= T) return;
  const int c = plane % C;
  const float* wp = w + (size_t)(per_plane_w ? plane : c) * K * K;
  const int v0 = (j + P) & 1;
  float ws[K][NV];
  int jo[NV];
  bool jok[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const int v = v0 + 2 * q;
    jo[q] = (j + P - v) >> 1;
    jok[q] = v < K && (j + P - v) >= 0 && jo[q] < To;
    if (!jok[q]) jo[q] = 0;
#pragma unroll
    for (int u = 0; u < K; ++u) ws[u][q] = v < K ? wp[u * K + v] : 0.0f;
  }
  const float* g = dz + (size_t)plane * Fo * To;
  auto load_row = [&](int io, float (&r)[NV]) {
    const bool rok = io >= 0 && io < Fo;
    const float* row = g + (size_t)(rok ? io : 0) * To;
#pragma unroll
    for (int q = 0; q < NV; ++q) r[q] = (rok && jok[q]) ? row[jo[q]] : 0.0f;
  };
  const size_t base = (size_t)plane * F * T + j;
  float rm[NV], r0[NV], r1[NV], r2[NV];        // dz rows m-1, m, m+1 and the prefetched m+2
#pragma unroll
  for (int q = 0; q < NV; ++q) rm[q] = 0.0f;
  load_row(0, r0);
  load_row(1, r1);
  for (int m = 0; 2 * m < F; ++m) {
    load_row(m + 2, r2);
    const int ie = 2 * m, io_ = 2 * m + 1;
    float ae = res ? res[base + (size_t)ie * T] : 0.0f;
    float ao = (res && io_ < F) ? res[base + (size_t)io_ * T] : 0.0f;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
      if constexpr (K == 3) {
        ae = fmaf(ws[1][q], r0[q], ae);                                 // row 2m:   u = 1 -> dz row m
        ao = fmaf(ws[0][q], r1[q], fmaf(ws[2][q], r0[q], ao));          // row 2m+1: u = 0 -> m+1, u = 2 -> m
      } else {
        ae = fmaf(ws[0][q], r1[q], fmaf(ws[2][q], r0[q], fmaf(ws[4][q], rm[q], ae)));   // u = 0, 2, 4 -> m+1, m, m-1
        ao = fmaf(ws[1][q], r1[q], fmaf(ws[3][q], r0[q], ao));                          // u = 1, 3    -> m+1, m
      }
    }
    dx[base + (size_t)ie * T] = ae;
    if (io_ < F) dx[base + (size_t)io_ * T] = ao;
#pragma unroll
    for (int q = 0; q < NV; ++q) { rm[q] = r0[q]; r0[q] = r1[q]; r1[q] = r2[q]; }
  }
}

// ---- depthwise / stem weight gradient: dw[c,u,v] = sum_{b,i,j} dz[b,c,i,j] x[b,cx,i*s+u-p,j*s+v-p] -------
// One block per (channel, batch slice); x has XC channels (XC == C depthwise, XC == 1 stem).
template <int K, int STRIDE>
__global__ __launch_bounds__(256) void dw_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ x,
                                                       float* __restrict__ dw, int B, int C, int XC, int F, int T,
                                                       int Fo, int To, int b_per_block, int per_sample) {
  constexpr int P = (K - 1) / 2;
  __shared__ float s_red[4][K * K];
  const int c = blockIdx.x, b0 = blockIdx.y * b_per_block;
  const int b1 = (b0 + b_per_block) < B ? (b0 + b_per_block) : B;
  float acc[K * K];
#pragma unroll
  for (int i = 0; i < K * K; ++i) acc[i] = 0.f;
  const int plane_o = Fo * To;
  for (int bb = b0; bb < b1; ++bb) {
    const float* g = dz + ((size_t)bb * C + c) * plane_o;
    const float* xp = x + ((size_t)bb * XC + (XC == 1 ? 0 : c)) * F * T;
    for (int e = threadIdx.x; e < plane_o; e += blockDim.x) {
      const int i = e / To, j = e - i * To;
      const float gv = g[e];
#pragma unroll
      for (int u = 0; u < K; ++u) {
        const int fi = i * STRIDE + u - P;
        const bool rok = fi >= 0 && fi < F;
#pragma unroll
        for (int v = 0; v < K; ++v) {
          const int ti = j * STRIDE + v - P;
          const float xv = (rok && ti >= 0 && ti < T) ? xp[(size_t)fi * T + ti] : 0.0f;
          acc[u * K + v] = fmaf(gv, xv, acc[u * K + v]);
        }
      }
    }
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < K * K; ++i) {
    const float t = eat::wave_sum(acc[i]);
    if (lane == 0) s_red[wv][i] = t;
  }
  __syncthreads();
  if (threadIdx.x < K * K)
    atomicAdd(dw + ((size_t)(per_sample ? b0 * C : 0) + c) * K * K + threadIdx.x,
              s_red[0][threadIdx.x] + s_red[1][threadIdx.x] + s_red[2][threadIdx.x] + s_red[3][threadIdx.x]);
}


// Stem weight gradient (models/mn/model.py:124-133: 3x3 / stride 2, ONE input channel, C = 16 w output channels):
// dW[c][u][v] = sum_{b,i,j} dz[b,c,i,j] x[b,0,2i+u-1,2j+v-1].  The generic kernel above walks one channel per block and
// gathers 9 predicated x values per dz element (710 us at B = 256 for 655 MB: 0.9 TB/s).  Here a thread owns output
// columns, keeps the 3x3 x window of a position in registers and applies it to 16 channels at once (16 coalesced dz
// loads per position, the window is loaded once per position and channel group), 144 accumulators per thread; one
// wave reduction + 144 atomics per block.
template <int CG>
__global__ __launch_bounds__(256) void stem_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ x,
                                                         float* __restrict__ dw, int C, int F, int T, int Fo, int To,
                                                         int rows_per_block) {
  __shared__ float s_red[4][CG * 9];
  const int b = blockIdx.y;
  const int i0 = blockIdx.x * rows_per_block;
  const int i1 = (i0 + rows_per_block) < Fo ? (i0 + rows_per_block) : Fo;
  const float* xb = x + (size_t)b * F * T;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int c0 = 0; c0 < C; c0 += CG) {
    float acc[CG][9];
#pragma unroll
    for (int c = 0; c < CG; ++c)
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[c][t] = 0.0f;
    const float* gz = dz + ((size_t)b * C + c0) * Fo * To;
    for (int i = i0; i < i1; ++i) {
      for (int j = threadIdx.x; j < To; j += 256) {
        float xw[9];
#pragma unroll
        for (int u = 0; u < 3; ++u) {
          const int fi = 2 * i + u - 1;
          const bool rok = fi >= 0 && fi < F;
#pragma unroll
          for (int v = 0; v < 3; ++v) {
            const int ti = 2 * j + v - 1;
            xw[u * 3 + v] = (rok && ti >= 0 && ti < T) ? xb[(size_t)fi * T + ti] : 0.0f;
          }
        }
        const size_t pos = (size_t)i * To + j;
#pragma unroll
        for (int c = 0; c < CG; ++c) {
          const float g = (c0 + c < C) ? gz[(size_t)c * Fo * To + pos] : 0.0f;
#pragma unroll
          for (int t = 0; t < 9; ++t) acc[c][t] = fmaf(g, xw[t], acc[c][t]);
        }
      }
    }
#pragma unroll
    for (int c = 0; c < CG; ++c)
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const float v = eat::wave_sum(acc[c][t]);
        if (lane == 0) s_red[wv][c * 9 + t] = v;
      }
    __syncthreads();
    for (int e = threadIdx.x; e < CG * 9; e += 256) {
      const int c = e / 9;
      if (c0 + c < C) atomicAdd(dw + (size_t)(c0 + c) * 9 + (e - c * 9), s_red[0][e] + s_red[1][e] + s_red[2][e] + s_red[3][e]);
    }
    __syncthreads();
  }
}

// Column-walking variant (depthwise, XC == C): the kernel above loads K*K predicated 4-byte x values per output
// element (25 narrow loads for a 5x5) and is bound by the texture unit at ~1.4 TB/s.  Here a thread owns one output
// column of one (b, c) plane and walks down the rows with the K x K input window in a register ring, as the forward
// kernel does: K*STRIDE new x values + one dz value per output.  A block = one channel, TY samples x TX columns, and
// loops over its slice of the batch; the K*K partial sums are reduced once per block (shuffles, LDS, K*K atomics).
template <int K, int STRIDE>
__global__ __launch_bounds__(256) void dw_wgrad_col_kernel(const float* __restrict__ dz, const float* __restrict__ x,
                                                           float* __restrict__ dw, int B, int C, int F, int T, int Fo,
                                                           int To, int TX, int b_per_block, int per_sample,
                                                           const float* __restrict__ in_a,
                                                           const float* __restrict__ in_b, int in_act) {
  constexpr int P = (K - 1) / 2;
  constexpr int NSLOT = K;                              // ring of K rows: step R uses slots (u + R*STRIDE) % K
  __shared__ float s_red[4][K * K];
  const int tid = threadIdx.x;
  const int tx = tid % TX, ty = tid / TX, TY = 256 / TX;
  const int to = blockIdx.x * TX + tx;
  const int c = blockIdx.y;
  const int b0 = blockIdx.z * b_per_block;
  const int b1 = (b0 + b_per_block) < B ? (b0 + b_per_block) : B;
  float acc[K * K];
#pragma unroll
  for (int i = 0; i < K * K; ++i) acc[i] = 0.f;
  // in_a != NULL: the conv input was act_in(in_a[c] * x + in_b[c]) evaluated on load (eat_dw_conv_fwd_tf)
  const bool has_tf = in_a != nullptr;
  const float ia = has_tf ? in_a[c] : 1.0f, ib = has_tf ? in_b[c] : 0.0f;
  if (to < To) {
    const int t0 = to * STRIDE - P;
    bool cok[K];
#pragma unroll
    for (int v = 0; v < K; ++v) cok[v] = (t0 + v >= 0) && (t0 + v < T);
    for (int bb = b0 + ty; bb < b1; bb += TY) {
      const float* g = dz + ((size_t)bb * C + c) * Fo * To + to;
      const float* xp = x + ((size_t)bb * C + c) * F * T;
      float win[NSLOT][K];
      auto load_row = [&](int fi, float (&dst)[K]) {
        const bool rok = fi >= 0 && fi < F;
        const float* src = xp + (size_t)(rok ? fi : 0) * T + t0;
        if (has_tf) {
#pragma unroll
          for (int v = 0; v < K; ++v) dst[v] = (rok && cok[v]) ? eat::activate_rt(fmaf(ia, src[v], ib), in_act) : 0.0f;
        } else {
#pragma unroll
          for (int v = 0; v < K; ++v) dst[v] = (rok && cok[v]) ? src[v] : 0.0f;
        }
      };
#pragma unroll
      for (int u = 0; u < K - STRIDE; ++u) load_row(u - P, win[u]);      // rows kept from "step -1"
      for (int fo0 = 0; fo0 < Fo; fo0 += K) {
#pragma unroll
        for (int R = 0; R < K; ++R) {                   // K steps = one full rotation of the ring
          const int fo = fo0 + R;
          if (fo < Fo) {
#pragma unroll
            for (int u = K - STRIDE; u < K; ++u) load_row(fo * STRIDE - P + u, win[(u + R * STRIDE) % NSLOT]);
            const float gv = g[(size_t)fo * To];
#pragma unroll
            for (int u = 0; u < K; ++u)
#pragma unroll
              for (int v = 0; v < K; ++v) acc[u * K + v] = fmaf(gv, win[(u + R * STRIDE) % NSLOT][v], acc[u * K + v]);
          }
        }
      }
    }
  }
  const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int i = 0; i < K * K; ++i) {
    const float t = eat::wave_sum(acc[i]);
    if (lane == 0) s_red[wv][i] = t;
  }
  __syncthreads();
  if (tid < K * K)
    atomicAdd(dw + ((size_t)(per_sample ? b0 * C : 0) + c) * K * K + tid,
              s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid]);
}
}  // namespace

static int dw_dgrad2_try(const float* dz, const float* w, const float* res, float* dx, int B, int C, int F, int T, int Fo,
                         int To, int k, int per_plane_w, hipStream_t s, const eat::DwEpi* epi = nullptr) {
  eat::DwDgrad2Req r{}; r.dim = {B, C, F, T, Fo, To, k, 2};
  r.dz = dz; r.w = w; r.res = res; r.dx = dx; r.per_plane_w = per_plane_w; r.epi = epi; r.stream = s;
  return eat::dw_tile_dgrad2_try(r);
}

static int dw_dgrad_impl(const float* dz, const float* w, const float* res, float* dx, int B, int C, int F, int T,
                         int Fo, int To, int k, int stride, int per_plane_w, eat_stream_t stream) {
  hipStream_t s = (hipStream_t)stream;
  if (stride == 1 && (k == 3 || k == 5)) {
    return eat::dw_conv_dgrad_s1(dz, w, nullptr, res, dx, B, C, F, T, k, per_plane_w, s);
  }
  if (stride == 2 && (k == 3 || k == 5)) {
    // tile kernel (dw_plane.hip): one dz column per lane, dx row segments as 8-byte stores; 1 = not applicable
    const int rc = dw_dgrad2_try(dz, w, res, dx, B, C, F, T, Fo, To, k, per_plane_w, s);
    if (rc != 1) return rc;
    dim3 g2((T + 63) / 64, (B * C + 3) / 4);
    if (k == 3) hipLaunchKernelGGL((dw_dgrad_s2_kernel<3>), g2, dim3(256), 0, s, dz, w, res, dx, B * C, C, F, T, Fo, To, per_plane_w);
    else hipLaunchKernelGGL((dw_dgrad_s2_kernel<5>), g2, dim3(256), 0, s, dz, w, res, dx, B * C, C, F, T, Fo, To, per_plane_w);
    return eat::check_launch("eat_dw_conv_dgrad");
  }
  int gx = (F * T + 255) / 256;
  if (gx > 64) gx = 64;
  dim3 grid(gx, B * C);
#define EAT_DG(KK, SS) hipLaunchKernelGGL((dw_dgrad_kernel<KK, SS>), grid, dim3(256), 0, s, dz, w, res, dx, C, F, T, Fo, To, per_plane_w)
  if (k == 3 && stride == 1) EAT_DG(3, 1);
  else if (k == 3 && stride == 2) EAT_DG(3, 2);
  else if (k == 5 && stride == 1) EAT_DG(5, 1);
  else if (k == 5 && stride == 2) EAT_DG(5, 2);
  else return eat::fail(EAT_EINVAL, "eat_dw_conv_dgrad: unsupported k=%d stride=%d", k, stride);
#undef EAT_DG
  return eat::check_launch("eat_dw_conv_dgrad");
}

extern "C" int eat_dw_conv_dgrad(const float* dz, const float* w, const float* res, float* dx, int B, int C, int F,
                                 int T, int Fo, int To, int k, int stride, eat_stream_t stream) {
  eat::clear_stale_error();
  return dw_dgrad_impl(dz, w, res, dx, B, C, F, T, Fo, To, k, stride, 0, stream);
}

// Depthwise data gradient with the backward of the PRECEDING (forward order) BatchNorm + activation started in its
// epilogue: g = dgrad(dz) * act'(ga[c] * gz + gb[c]) and the per-wave partial sums of g (gpart [b][C][inner]); gz is the
// pre-BN output of the expand conv (same shape as g).  See train_fuse.hip for what consumes g / gpart.
extern "C" int eat_dw_conv_dgrad_g(const float* dz, const float* w, const float* gz, const float* ga, const float* gb,
                                   int gact, float* g, float* gpart, int inner_cap, int* h_inner, int B, int C, int F,
                                   int T, int Fo, int To, int k, int stride, eat_stream_t stream) {
  eat::clear_stale_error();
  if (!gz || !ga || !gb || !gpart || !h_inner) return eat::fail(EAT_EINVAL, "eat_dw_conv_dgrad_g: gz, ga, gb, gpart, h_inner are required");
  if (gact < 0 || gact > 2) return eat::fail(EAT_EINVAL, "eat_dw_conv_dgrad_g: bad act %d", gact);
  if (inner_cap < eat_dw_partials_inner(F, T, Fo, To, k, stride, 1))
    return eat::fail(EAT_EINVAL, "eat_dw_conv_dgrad_g: partial buffer too small (inner_cap %d)", inner_cap);
  hipStream_t s = (hipStream_t)stream;
  if ((k == 3 || k == 5) && (stride == 1 || stride == 2)) {
    int inner = 1;
    const eat::DwEpi epi{nullptr, gz, ga, gb, gact, gpart, &inner};
    const int rc = stride == 1 ? eat::dw_conv_dgrad_s1(dz, w, nullptr, nullptr, g, B, C, F, T, k, 0, s, &epi)
                               : dw_dgrad2_try(dz, w, nullptr, g, B, C, F, T, Fo, To, k, 0, s, &epi);
    if (rc != 1) { *h_inner = inner; return rc; }
  }
  const int rc = dw_dgrad_impl(dz, w, nullptr, g, B, C, F, T, Fo, To, k, stride, 0, stream);
  if (rc != 0) return rc;
  *h_inner = 1;
  return eat::act_grad_sum(g, gz, ga, gb, gact, g, gpart, B, C, F * T, s);
}

extern "C" int eat_dw_conv_dyn_dgrad(const float* dz, const float* w_bc, const float* res, float* dx, int B, int C,
                                     int F, int T, int Fo, int To, int k, int stride, eat_stream_t stream) {
  eat::clear_stale_error();
  return dw_dgrad_impl(dz, w_bc, res, dx, B, C, F, T, Fo, To, k, stride, 1, stream);
}

// Which kernel a weight-gradient call runs on and how it cuts the batch: dw_wgrad_impl launches what this answers and
// eat_dw_wgrad_split reports it.  (k / stride outside {3, 5} x {1, 2} end on the per-channel kernel's EAT_EINVAL.)
static void dw_wgrad_plan(int B, int C, int XC, int F, int T, int Fo, int To, int k, int stride, int per_sample,
                          eat::DwWgradPlan* p) {
  // register-resident kernels (dw_plane.hip); 1 = geometry not instantiated
  if (XC == C && eat::dw_plane_wgrad_plan(eat::DwGeom{B, C, F, T, Fo, To, k, stride}, per_sample != 0, p) == 0) return;
  *p = eat::DwWgradPlan{};
  p->npw = 1;
  if (XC == C && !per_sample && (k == 3 || k == 5) && (stride == 1 || stride == 2)) {
    p->kernel = eat::kDwWgColumn;
    p->TX = To > 32 ? 64 : 32;
    const int TY = 256 / p->TX;
    p->ct = (To + p->TX - 1) / p->TX;
    // ~2048 blocks, but every thread should walk several planes before the block-wide reduction
    long long want = (2048 + (long long)C * p->ct - 1) / ((long long)C * p->ct);
    if (want < 1) want = 1;
    p->bpb = (int)((B + want - 1) / want);
    if (p->bpb < 4 * TY) p->bpb = 4 * TY < B ? 4 * TY : B;
    p->slices = (B + p->bpb - 1) / p->bpb;
    return;
  }
  if (XC == 1 && k == 3 && stride == 2 && !per_sample) {
    p->kernel = eat::kDwWgStem;
    // ~2048 blocks: (row chunks) x (samples)
    p->rpb = (int)(((long long)Fo * B + 2047) / 2048);
    if (p->rpb < 1) p->rpb = 1;
    p->chunks = (Fo + p->rpb - 1) / p->rpb;
    return;
  }
  p->kernel = eat::kDwWgChannel;
  // enough blocks to fill the chip: split the batch when there are few channels
  int splits = (2048 + C - 1) / C;
  if (splits > B || per_sample) splits = B;
  p->bpb = (B + splits - 1) / splits;
  p->slices = (B + p->bpb - 1) / p->bpb;
}

// Host helper: the kernel of eat_dw_conv_wgrad / eat_dw_conv_wgrad_tf (per_sample = 0) or eat_dw_conv_dyn_wgrad (1) for a
// shape - 0 whole-plane, 1 tile, 2 column-walking, 3 stem, 4 per-channel - and its split; -1: the call would be refused
extern "C" int eat_dw_wgrad_split(int B, int C, int XC, int F, int T, int Fo, int To, int k, int stride, int per_sample,
                                  int* split, int* parts, int* lane_samples) {
  if (B < 1 || C < 1 || (XC != C && XC != 1) || (k != 3 && k != 5) || (stride != 1 && stride != 2)) return -1;
  eat::DwWgradPlan pl;
  dw_wgrad_plan(B, C, XC, F, T, Fo, To, k, stride, per_sample, &pl);
  int sp = 0, pa = 0;
  switch (pl.kernel) {
    case eat::kDwWgPlane: sp = pl.G; pa = (int)(pl.waves / C); break;
    case eat::kDwWgTile: sp = pl.G; pa = (int)(pl.waves / ((long long)C * pl.n_rc * pl.n_cs)); break;
    case eat::kDwWgStem: sp = pl.rpb; pa = pl.chunks; break;
    default: sp = pl.bpb; pa = pl.slices; break;
  }
  if (split) *split = sp;
  if (parts) *parts = pa;
  if (lane_samples) *lane_samples = pl.npw;
  return pl.kernel;
}

static int dw_wgrad_impl(const float* dz, const float* x, float* dw, int B, int C, int XC, int F, int T, int Fo, int To,
                         int k, int stride, int per_sample, eat_stream_t stream, const float* in_a = nullptr,
                         const float* in_b = nullptr, int in_act = 0) {
  if (XC != C && XC != 1) return eat::fail(EAT_EINVAL, "eat_dw_conv_wgrad: x must have C or 1 channels");
  if (in_a && XC != C) return eat::fail(EAT_EINVAL, "eat_dw_conv_wgrad_tf: needs the column-walking kernel");
  eat::DwWgradPlan pl;
  dw_wgrad_plan(B, C, XC, F, T, Fo, To, k, stride, per_sample, &pl);
  if (pl.kernel == eat::kDwWgPlane || pl.kernel == eat::kDwWgTile) {
    // register-resident kernels (dw_plane.hip): every element loaded once
    eat::DwWgradReq r{}; r.dim = {B, C, F, T, Fo, To, k, stride};
    r.dz = dz; r.x = x; r.dw = dw; r.per_plane = per_sample; r.tf = {in_a, in_b, in_act}; r.stream = (hipStream_t)stream;
    return eat::dw_plane_wgrad_run(r, pl);
  }
  if (pl.kernel == eat::kDwWgColumn) {
    // column-walking kernel: block = (column tile, channel, batch slice)
    const int TX = pl.TX, bpb = pl.bpb;
    dim3 grid(pl.ct, C, pl.slices);
    hipStream_t s = (hipStream_t)stream;
#define EAT_WGC(KK, SS) hipLaunchKernelGGL((dw_wgrad_col_kernel<KK, SS>), grid, dim3(256), 0, s, dz, x, dw, B, C, F, T, Fo, To, TX, bpb, per_sample, in_a, in_b, in_act)
    if (k == 3 && stride == 1) EAT_WGC(3, 1);
    else if (k == 3 && stride == 2) EAT_WGC(3, 2);
    else if (k == 5 && stride == 1) EAT_WGC(5, 1);
    else EAT_WGC(5, 2);
#undef EAT_WGC
    return eat::check_launch("eat_dw_conv_wgrad");
  }
  if (pl.kernel == eat::kDwWgStem) {
    hipLaunchKernelGGL(stem_wgrad_kernel<16>, dim3(pl.chunks, B), dim3(256), 0, (hipStream_t)stream, dz, x, dw, C, F, T,
                       Fo, To, pl.rpb);
    return eat::check_launch("eat_dw_conv_wgrad(stem)");
  }
  const int bpb = pl.bpb;
  dim3 grid(C, pl.slices);
  hipStream_t s = (hipStream_t)stream;
#define EAT_WG(KK, SS) hipLaunchKernelGGL((dw_wgrad_kernel<KK, SS>), grid, dim3(256), 0, s, dz, x, dw, B, C, XC, F, T, Fo, To, bpb, per_sample)
  if (k == 3 && stride == 1) EAT_WG(3, 1);
  else if (k == 3 && stride == 2) EAT_WG(3, 2);
  else if (k == 5 && stride == 1) EAT_WG(5, 1);
  else if (k == 5 && stride == 2) EAT_WG(5, 2);
  else return eat::fail(EAT_EINVAL, "eat_dw_conv_wgrad: unsupported k=%d stride=%d", k, stride);
#undef EAT_WG
  return eat::check_launch("eat_dw_conv_wgrad");
}

extern "C" int eat_dw_conv_wgrad(const float* dz, const float* x, float* dw, int B, int C, int XC, int F, int T,
                                 int Fo, int To, int k, int stride, eat_stream_t stream) {
  eat::clear_stale_error();
  return dw_wgrad_impl(dz, x, dw, B, C, XC, F, T, Fo, To, k, stride, 0, stream);
}

extern "C" int eat_dw_conv_wgrad_tf(const float* dz, const float* x, const float* in_a, const float* in_b, int in_act,
                                    float* dw, int B, int C, int F, int T, int Fo, int To, int k, int stride,
                                    eat_stream_t stream) {
  eat::clear_stale_error();
  if (!in_a || !in_b) return eat::fail(EAT_EINVAL, "eat_dw_conv_wgrad_tf: in_a and in_b are required");
  if (in_act < 0 || in_act > 2) return eat::fail(EAT_EINVAL, "eat_dw_conv_wgrad_tf: bad in_act %d", in_act);
  return dw_wgrad_impl(dz, x, dw, B, C, C, F, T, Fo, To, k, stride, 0, stream, in_a, in_b, in_act);
}

// Backward of the depthwise conv of an inverted-residual block in ONE pass (autograd of models/mn/block_types.py:150-162
// + the first half of the backward of the expand conv's BatchNorm + activation): from dz (B,C,Fo,To) and the pre-BN expand
// output x (B,C,F,T) with its BN affine (in_a, in_b) and activation in_act
//   dw (C,k,k) += weight gradient w.r.t. the conv input act(in_a x + in_b)            [dw zeroed by the caller]
//   g (B,C,F,T) = dgrad(dz) * act'(in_a x + in_b),   gpart [B][C][inner] = per-tile sums of g
// = eat_dw_conv_wgrad_tf + eat_dw_conv_dgrad_g with dz and x read once.  inner_cap >= eat_dw_bwd_partials_inner(...)
// AND >= eat_dw_partials_inner(..., 1) (the two-kernel fallback writes its own layout); *h_inner receives inner.
extern "C" int eat_dw_conv_bwd_g(const float* dz, const float* x, const float* in_a, const float* in_b, int in_act,
                                 const float* w, float* g, float* dw, float* gpart, int inner_cap, int* h_inner, int B,
                                 int C, int F, int T, int Fo, int To, int k, int stride, eat_stream_t stream) {
  eat::clear_stale_error();
  if (!in_a || !in_b || !gpart || !h_inner) return eat::fail(EAT_EINVAL, "eat_dw_conv_bwd_g: in_a, in_b, gpart, h_inner are required");
  if (in_act < 0 || in_act > 2) return eat::fail(EAT_EINVAL, "eat_dw_conv_bwd_g: bad act %d", in_act);
  if (inner_cap < eat_dw_bwd_partials_inner(F, T, Fo, To, k, stride) || inner_cap < eat_dw_partials_inner(F, T, Fo, To, k, stride, 1))
    return eat::fail(EAT_EINVAL, "eat_dw_conv_bwd_g: partial buffer too small (inner_cap %d)", inner_cap);
  if ((k == 3 || k == 5) && (stride == 1 || stride == 2)) {
    eat::DwBwdReq r{}; r.dim = {B, C, F, T, Fo, To, k, stride};
    r.dz = dz; r.x = x; r.tf = {in_a, in_b, in_act}; r.w = w; r.g = g; r.dw = dw; r.gpart = gpart; r.h_inner = h_inner;
    r.stream = (hipStream_t)stream;
    const int rc = eat::dw_bwd_try(r);
    if (rc != 1) return rc;
  }
  int rc = dw_wgrad_impl(dz, x, dw, B, C, C, F, T, Fo, To, k, stride, 0, stream, in_a, in_b, in_act);
  if (rc != 0) return rc;
  return eat_dw_conv_dgrad_g(dz, w, x, in_a, in_b, in_act, g, gpart, inner_cap, h_inner, B, C, F, T, Fo, To, k, stride, stream);
}

// Host helper: 1 where the geometry is one of the merged kernel's, i.e. where the eat_dw_conv_*bwd_bn_g* entry points run
extern "C" int eat_dw_bwd_merged_ok(int B, int C, int F, int T, int Fo, int To, int k, int stride) {
  if ((long long)B * C > 0x3fffffffLL || (long long)F * T >= (1 << 28)) return 0;
  if (!((k == 3 || k == 5) && (stride == 1 || stride == 2))) return 0;
  if (stride == 1 && (Fo != F || To != T)) return 0;
  if ((long long)4 * C * F * T * 4 >= 0x7fffffffLL) return 0;         // lane-group offsets inside a wave's samples are 32-bit
  return 1;
}

// The same with the BatchNorm + activation backward of THIS conv's output evaluated on load (dw_plane.hip, DzBn): dy is the
// gradient w.r.t. act(BN(z)) (times gscale[b,c] plus gadd[b,c] for a squeeze-excitation block), sums the fp64 channel sums
// of eat_bn_act_bwd_reduce / eat_se_bn_bwd_combine.  Blocks without an expand conv: in_a = 1, in_b = 0, in_act = none,
// gpart may be NULL.  Only where eat_dw_bwd_merged_ok(...) != 0, else EAT_EINVAL.  The four entry points fill a request
// and its BatchNorm constants (r.bn); this is their one validation and launch, `who` the entry point called.
static int dw_bwd_bn_run(const char* who, const eat::DwBwdReq& r, int inner_cap) {
  eat::clear_stale_error();
  const eat::DwGeom& d = r.dim;
  const eat::DwBnBwd& bn = *r.bn;
  if (!r.dz || !bn.z || !bn.a || !bn.b || !bn.mean || !bn.invstd || !bn.sums || !r.x || !r.tf.a || !r.tf.b || !r.w || !r.g || !r.dw)
    return eat::fail(EAT_EINVAL, "%s: missing operand", who);
  if (r.tf.act < 0 || r.tf.act > 2 || bn.act < 0 || bn.act > 2) return eat::fail(EAT_EINVAL, "%s: bad act", who);
  if (r.res && r.store == eat::kDwB16) return eat::fail(EAT_EINVAL, "%s: the skip gradient goes with an fp32 g (x_b16 = 0)", who);
  if (!eat_dw_bwd_merged_ok(d.B, d.C, d.F, d.T, d.Fo, d.To, d.k, d.stride) ||
      (r.store != eat::kDwF32 && ((d.F * d.T) % 2 != 0 || (d.Fo * d.To) % 2 != 0)))
    return eat::fail(EAT_EINVAL, "%s: geometry not covered by the merged kernel (F=%d T=%d k=%d stride=%d)", who, d.F, d.T, d.k, d.stride);
  if ((r.gpart || r.gzpart) && inner_cap < eat_dw_bwd_partials_inner(d.F, d.T, d.Fo, d.To, d.k, d.stride))
    return eat::fail(EAT_EINVAL, "%s: partial buffer too small (inner_cap %d)", who, inner_cap);
  const int rc = eat::dw_bwd_try(r);
  if (rc == 1) return eat::fail(EAT_EINVAL, "%s: no merged-kernel instance for F=%d T=%d k=%d stride=%d", who, d.F, d.T, d.k, d.stride);
  return rc;
}

extern "C" int eat_dw_conv_bwd_bn_g(const float* dy, const float* z, const float* bn_a, const float* bn_b,
                                    const float* bn_mean, const float* bn_invstd, const float* gscale, const float* gadd,
                                    const double* sums, int bn_act, int frozen, const float* x, const float* in_a,
                                    const float* in_b, int in_act, const float* w, float* g, float* dw,
                                    float* gpart, int inner_cap, int* h_inner, int B, int C, int F, int T, int Fo, int To,
                                    int k, int stride, eat_stream_t stream) {
  eat::DwBwdReq r{}; r.dim = {B, C, F, T, Fo, To, k, stride}; r.stream = (hipStream_t)stream;
  r.dz = dy; r.x = x; r.tf = {in_a, in_b, in_act}; r.w = w; r.g = g; r.dw = dw; r.gpart = gpart; r.h_inner = h_inner;
  eat::DwBnBwd bn{}; bn.z = z; bn.a = bn_a; bn.b = bn_b; bn.mean = bn_mean; bn.invstd = bn_invstd; bn.sums = sums; bn.act = bn_act;
  bn.frozen = frozen; bn.gscale = gscale; bn.gadd = gadd; r.bn = &bn;
  return dw_bwd_bn_run("eat_dw_conv_bwd_bn_g", r, inner_cap);
}

// The same over bf16-stored dy, z, x and g (act_io.h; the bf16-storage plan of BASELINE configs[2]): every wide tensor the
// backward of a block touches is 16-bit in HBM (x_b16 = 0: x and g are fp32 - the first block, whose conv input is the stem
// output); coefficients, channel sums, taps, dw and the partial sums (taken of the g values as stored) are fp32 / fp64.
extern "C" int eat_dw_conv_bwd_bn_g_b16(const void* dy, const void* z, const float* bn_a, const float* bn_b,
                                        const float* bn_mean, const float* bn_invstd, const float* gscale, const float* gadd,
                                        const double* sums, int bn_act, int frozen, const void* x, int x_b16, const float* in_a,
                                        const float* in_b, int in_act, const float* w, void* g, float* dw, float* gpart,
                                        int inner_cap, int* h_inner, int B, int C, int F, int T, int Fo, int To, int k,
                                        int stride, eat_stream_t stream) {
  eat::DwBwdReq r{}; r.dim = {B, C, F, T, Fo, To, k, stride};
  r.dz = dy; r.x = x; r.tf = {in_a, in_b, in_act}; r.w = w; r.g = g; r.dw = dw; r.gpart = gpart; r.h_inner = h_inner;
  r.store = x_b16 ? eat::kDwB16 : eat::kDwB16XF32; r.stream = (hipStream_t)stream;
  eat::DwBnBwd bn{}; bn.z = z; bn.a = bn_a; bn.b = bn_b; bn.mean = bn_mean; bn.invstd = bn_invstd; bn.sums = sums; bn.act = bn_act;
  bn.frozen = frozen; bn.gscale = gscale; bn.gadd = gadd; r.bn = &bn;
  return dw_bwd_bn_run("eat_dw_conv_bwd_bn_g_b16", r, inner_cap);
}

// The same for DyMN's dynamic depthwise conv (per-(b,c) taps w_bc (B, C, k*k), models/dymn/dy_block.py:103-131 backward):
// dw_bc (B, C, k*k) receives the per-plane tap gradients (zero-filled by the caller: planes of several tiles are added),
// res (shape of g) or NULL is added to g after the partial sums are taken (the skip connection of a block without expand
// conv), gzpart (layout of gpart) or NULL receives the per-tile sums of g * x (x raw): with gpart the two sums the
// BatchNorm backward of the expand conv needs - no reduce pass over (g, x).
extern "C" int eat_dw_conv_dyn_bwd_bn_g(const float* dy, const float* z, const float* bn_a, const float* bn_b,
                                        const float* bn_mean, const float* bn_invstd, const double* sums, int bn_act,
                                        int frozen, const float* x, const float* in_a, const float* in_b, int in_act,
                                        const float* w_bc, const float* res, float* g, float* dw_bc, float* gpart,
                                        float* gzpart, int inner_cap, int* h_inner, int B, int C, int F, int T, int Fo,
                                        int To, int k, int stride, eat_stream_t stream) {
  eat::DwBwdReq r{}; r.dim = {B, C, F, T, Fo, To, k, stride}; r.stream = (hipStream_t)stream;
  r.dz = dy; r.x = x; r.tf = {in_a, in_b, in_act}; r.w = w_bc; r.g = g; r.dw = dw_bc; r.gpart = gpart; r.h_inner = h_inner;
  r.per_plane_w = 1; r.res = res; r.gzpart = gzpart;
  eat::DwBnBwd bn{}; bn.z = z; bn.a = bn_a; bn.b = bn_b; bn.mean = bn_mean; bn.invstd = bn_invstd; bn.sums = sums; bn.act = bn_act;
  bn.frozen = frozen; r.bn = &bn;
  return dw_bwd_bn_run("eat_dw_conv_dyn_bwd_bn_g", r, inner_cap);
}

// ... over bf16-stored dy, z (and x, g when x_b16 != 0; x_b16 = 0: the block without expand conv - x is the fp32 block input, g
// the fp32 input gradient, res its skip gradient): the DyMN blocks of the bf16-storage plan.  res needs x_b16 = 0.
extern "C" int eat_dw_conv_dyn_bwd_bn_g_b16(const void* dy, const void* z, const float* bn_a, const float* bn_b,
                                            const float* bn_mean, const float* bn_invstd, const double* sums, int bn_act,
                                            int frozen, const void* x, int x_b16, const float* in_a, const float* in_b, int in_act,
                                            const float* w_bc, const float* res, void* g, float* dw_bc, float* gpart,
                                            float* gzpart, int inner_cap, int* h_inner, int B, int C, int F, int T, int Fo,
                                            int To, int k, int stride, eat_stream_t stream) {
  eat::DwBwdReq r{}; r.dim = {B, C, F, T, Fo, To, k, stride};
  r.dz = dy; r.x = x; r.tf = {in_a, in_b, in_act}; r.w = w_bc; r.g = g; r.dw = dw_bc; r.gpart = gpart; r.h_inner = h_inner;
  r.per_plane_w = 1; r.res = res; r.gzpart = gzpart;
  r.store = x_b16 ? eat::kDwB16 : eat::kDwB16XF32; r.stream = (hipStream_t)stream;
  eat::DwBnBwd bn{}; bn.z = z; bn.a = bn_a; bn.b = bn_b; bn.mean = bn_mean; bn.invstd = bn_invstd; bn.sums = sums; bn.act = bn_act;
  bn.frozen = frozen; r.bn = &bn;
  return dw_bwd_bn_run("eat_dw_conv_dyn_bwd_bn_g_b16", r, inner_cap);
}

extern "C" int eat_dw_conv_dyn_wgrad(const float* dz, const float* x, float* dw_bc, int B, int C, int F, int T, int Fo,
                                     int To, int k, int stride, eat_stream_t stream) {
  eat::clear_stale_error();
  return dw_wgrad_impl(dz, x, dw_bc, B, C, C, F, T, Fo, To, k, stride, 1, stream);
}
