// 1x1 (pointwise) weight-gradient and Gram-matrix kernels of the training step for gfx950 and their entry points: autograd
// of F.conv2d w.r.t. the weight (SURVEY.md Appendix C lists the formulas the reference leaves to autograd).  Which kernel a
// shape runs on and how its k range is cut is decided in wgrad_plan.h (host-only, one request -> one plan); the host layer at
// the end of this file turns a plan into launches.  The BatchNorm passes are in bn_train.hip, the depthwise / stem gradients
// in dw_grad.hip.
#include "eat_common.h"
#include "act_io.h"
#include "wgrad_plan.h"

namespace wg = eat::wg;

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// Optional transform of the x operand of the 1x1 weight gradient: x' = act(a[ci] * x + b[ci]) evaluated on load (training:
// the project conv read BN + act of the depthwise output on load, so the activated tensor does not exist; mn_train.py)
// actr (Co) or NULL: additive constant of the dz operand, per row, applied to loaded elements only - with a = 1, b = actr =
// -mean and dz == x the kernels form the CENTRED Gram matrix sum (x - m)(x - m)^T (eat_gram_centered)
struct WgTf { const float* a; const float* b; int act; const float* actr = nullptr; };
// atomic add on a pointer KNOWN to be global memory (hipcc cannot always infer the address space of a pointer offset by a
// run-time slot index, and its expansion of a flat fp32 atomic fails on gfx950: "Operand has incorrect register class")
__device__ __forceinline__ void global_atomic_add(float* p, float v) {
  typedef __attribute__((address_space(1))) float gfloat;
  __hip_atomic_fetch_add((gfloat*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// branch-free: act(u) = max(u, lo) * clamp(u * ca + cb, 0, 1) with (lo, ca, cb) = none (-inf, 0, 1), ReLU (0, 0, 1),
// Hardswish (-inf, 1/6, 1/2) - the weight-gradient kernels are VALU-bound on the bf16 hi/lo split already
__device__ __forceinline__ float wg_tf(float v, float a, float b, int act) {
  const float u = fmaf(a, v, b);
  if (act == EAT_ACT_NONE) return u;                       // (wave-uniform) the centring transform of the Gram / Gx launches
  const float lo = act == EAT_ACT_RELU ? 0.0f : -__builtin_huge_valf();
  const float ca = act == EAT_ACT_HSWISH ? (1.0f / 6.0f) : 0.0f, cb = act == EAT_ACT_HSWISH ? 0.5f : 1.0f;
  return fmaxf(u, lo) * __builtin_amdgcn_fmed3f(fmaf(u, ca, cb), 0.0f, 1.0f);
}

// ---- pointwise weight gradient: dW[co,ci] = sum_{b,s} dz[b,co,s] x[b,ci,s] --------------------------------------
// Both operands are contiguous along the reduction axis s: each lane loads 4 consecutive s as one
// float4 and feeds them to 4 MFMAs (consistent k permutation).  Block = 4 waves on one 32 x 32
// tile of dW, each wave reducing its own slice of the (b, s) range; partials combined in LDS and
// added to dW with one atomic per element per block.
__global__ __launch_bounds__(256) void pw_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ x,
                                                       const float* __restrict__ xscale, float* __restrict__ dW,
                                                       int B, int Co, int Ci, int S, int b_per_block, int per_sample,
                                                       WgTf tf, int n_slots) {
  __shared__ float s_red[3][4][4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int m0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
  const int b0 = blockIdx.z * b_per_block;
  const int b1 = (b0 + b_per_block) < B ? (b0 + b_per_block) : B;
  const int row = lane & 15, kq = lane >> 4;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool vec = (S & 3) == 0;
  auto load4 = [&](const float* base, int r, int rmax, size_t rs, int s, float (&o)[4]) {
    o[0] = o[1] = o[2] = o[3] = 0.f;
    if (r >= rmax || s >= S) return;
    const float* p = base + (size_t)r * rs + s;
    if (vec) {
      const float4 t = *reinterpret_cast<const float4*>(p);
      o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) if (s + e < S) o[e] = p[e];
    }
  };
  // x operand transform (zero padding applies to the transformed values: only loaded elements are transformed)
  const float ta0 = (tf.a && n0 + row < Ci) ? tf.a[n0 + row] : 1.0f, tb0 = (tf.a && n0 + row < Ci) ? tf.b[n0 + row] : 0.0f;
  const float ta1 = (tf.a && n0 + 16 + row < Ci) ? tf.a[n0 + 16 + row] : 1.0f, tb1 = (tf.a && n0 + 16 + row < Ci) ? tf.b[n0 + 16 + row] : 0.0f;
  auto tf4 = [&](float (&o)[4], int r, int s, float ta, float tb) {
    if (!tf.a || r >= Ci) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) if (s + e < S) o[e] = wg_tf(o[e], ta, tb, tf.act);
  };
  const float ac0 = (tf.actr && m0 + row < Co) ? tf.actr[m0 + row] : 0.0f;
  const float ac1 = (tf.actr && m0 + 16 + row < Co) ? tf.actr[m0 + 16 + row] : 0.0f;
  auto ctr4 = [&](float (&o)[4], int r, int s, float c) {
    if (!tf.actr || r >= Co) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) if (s + e < S) o[e] += c;
  };
  for (int bb = b0; bb < b1; ++bb) {
    const float* gz = dz + (size_t)bb * Co * S;
    const float* gx = x + (size_t)bb * Ci * S;
    // the conv input may be x * xscale[b, ci] (squeeze-excitation): fold the scale into the B operand
    const float sc0 = (xscale && n0 + row < Ci) ? xscale[(size_t)bb * Ci + n0 + row] : 1.0f;
    const float sc1 = (xscale && n0 + 16 + row < Ci) ? xscale[(size_t)bb * Ci + n0 + 16 + row] : 1.0f;
    for (int s0 = wv * 64; s0 < S; s0 += 256) {              // wave w takes s-blocks w, w+4, ...
      float ga[4][2][4], xb[4][2][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int s = s0 + 16 * u + 4 * kq;
        load4(gz, m0 + row, Co, S, s, ga[u][0]);
        load4(gz, m0 + 16 + row, Co, S, s, ga[u][1]);
        load4(gx, n0 + row, Ci, S, s, xb[u][0]);
        load4(gx, n0 + 16 + row, Ci, S, s, xb[u][1]);
        tf4(xb[u][0], n0 + row, s, ta0, tb0);
        tf4(xb[u][1], n0 + 16 + row, s, ta1, tb1);
        ctr4(ga[u][0], m0 + row, s, ac0);
        ctr4(ga[u][1], m0 + 16 + row, s, ac1);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ga[u][i][e], xb[u][j][e] * (j ? sc1 : sc0), acc[i][j], 0, 0, 0);
    }
  }
  if (wv > 0) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) s_red[wv - 1][i * 2 + j][r][lane] = acc[i][j][r];
  }
  __syncthreads();
  if (wv != 0) return;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + 16 * i + kq * 4 + r, n = n0 + 16 * j + row;   // C/D: col = lane&15, row = kq*4+r
        if (m < Co && n < Ci) {
          const int q = i * 2 + j;
          global_atomic_add(dW + (size_t)(per_sample ? (unsigned)b0 : blockIdx.z % (unsigned)(n_slots > 0 ? n_slots : 1)) * Co * Ci + (size_t)m * Ci + n,
                    acc[i][j][r] + s_red[0][q][r][lane] + s_red[1][q][r][lane] + s_red[2][q][r][lane]);
        }
      }
}


// ---- pointwise weight gradient on the bf16 matrix cores ("bf16x3", see conv_pw_bf16.hip) ---------------------------
// dW (Co x Ci) = sum over k = (b, s) of dz[co, k] x[ci, k]: both operands are contiguous along k, which is exactly the
// operand layout of v_mfma_f32_16x16x32_bf16 (lane = (row, 8 consecutive k)), so every lane loads its 8 k-values
// straight from HBM/L2 as two float4, splits them into bf16 hi + lo in registers and issues hi*hi + hi*lo + lo*hi.
// Block = 4 waves as 2 x 2 on a 128 x 128 tile of dW (each wave 64 x 64 = 4 x 4 MFMA tiles, 64 accumulator VGPRs):
// dz is read ceil(Ci/128) times and x ceil(Co/128) times (the 32 x 32-tile fp32 kernel above reads them Ci/32 and
// Co/32 times: 1.3 GB of L2 traffic for the 112 -> 672 layer instead of 0.35 GB).  The k range is cut into units of 32
// positions of one sample and split over blockIdx.z; partial tiles are added to dW with atomics.
using bf16x8_t = __attribute__((ext_vector_type(8))) __bf16;
using f32x2_t = __attribute__((ext_vector_type(2))) float;
using bf16x2_t = __attribute__((ext_vector_type(2))) __bf16;

__device__ __forceinline__ void split8(const float (&v)[8], bf16x8_t& hi, bf16x8_t& lo) {
#pragma unroll
  for (int i = 0; i < 8; i += 2) {
    const bf16x2_t h = __builtin_convertvector(f32x2_t{v[i], v[i + 1]}, bf16x2_t);
    const bf16x2_t l = __builtin_convertvector(f32x2_t{v[i] - (float)h[0], v[i + 1] - (float)h[1]}, bf16x2_t);
    hi[i] = h[0]; hi[i + 1] = h[1];
    lo[i] = l[0]; lo[i + 1] = l[1];
  }
}

// LDS staging (v3): a lane-per-row direct load makes every lane of a load instruction touch a different cache line
// (measured: ~18 k cycles per 32-k step, the texture-address unit is the bottleneck).  Instead the operand tiles go
// through LDS by LDS-DMA with a coalesced mapping - lane l of one instruction fetches the 16-byte chunk
// (l & 7) ^ ((row >> 1) & 7) of row l >> 3, i.e. 8 rows x one full 128-byte line - and the XOR swizzle of the chunk
// index makes the later MFMA-fragment reads (16 lanes = 16 rows, same chunk) hit 16 different bank groups.
typedef __attribute__((address_space(3))) void wg_lds_void;
__device__ __forceinline__ void wg_glds16(const void* g, void* lds_wave_base) {
  const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(wg_lds_void*)lds_wave_base);
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(dst), "v"(g) : "memory", "m0");
}

// NPROD = 3: split operands (hi*hi + hi*lo + lo*hi, fp32-class); NPROD = 1: plain bf16 operands, fp32 accumulation
// (train_precision "bf16", BASELINE configs[2] - what autocast does to the conv weight gradient in the reference)
template <int NPROD>
__global__ __launch_bounds__(256, 2) void pw_wgrad_x3_kernel(const float* __restrict__ dz, const float* __restrict__ x,
                                                             const float* __restrict__ xscale, float* __restrict__ dW,
                                                             int B, int Co, int Ci, int S, int sps, int units_per_block,
                                                             int per_sample, WgTf tf, int n_slots) {
  // stage = [A: 128 rows x 128 B][B: 128 rows x 128 B] = 32 KB; 2 stages
  __shared__ __attribute__((aligned(16))) float s_op[2][2][128 * 32];
  // wv through readfirstlane: the compiler then knows it (and the tile counts derived from it) to be wave-uniform - scalar
  // branches instead of exec-masked blocks around the loads and MFMAs of rows beyond the matrix
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int r = lane & 15, kg = lane >> 4;
  // (an XCD-aware workgroup order - all tiles of a k-slice on one XCD, so that their shared operand rows meet in one L2 -
  //  was measured slower in round 3 and removed in round 4; the wide-tile kernel below reads each operand once instead)
  const int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  const int mb = bx * 128, nb = by * 128;                          // block tile origin
  const int mw = (wv & 1) * 64, nw = (wv >> 1) * 64;              // wave sub-tile inside the block tile
  const int total = B * sps;
  const int u0 = bz * units_per_block;
  const int u1 = (u0 + units_per_block) < total ? (u0 + units_per_block) : total;
  if (u0 >= u1) return;
  int mt_n = (Co - mb - mw + 15) / 16, nt_n = (Ci - nb - nw + 15) / 16;   // valid 16-row tiles of this wave (uniform)
  mt_n = mt_n < 0 ? 0 : (mt_n > 4 ? 4 : mt_n);
  nt_n = nt_n < 0 ? 0 : (nt_n > 4 ? 4 : nt_n);
  const bool active = mt_n > 0 && nt_n > 0;                        // idle waves still help with the loads
  // Gram matrix (dz == x, train_fuse.hip): a diagonal block's two operand tiles are the same rows - one DMA, one LDS tile
  const bool same_tile = dz == x && mb == nb && !xscale;
  // n_slots > 0: dW is a zero-filled workspace of n_slots copies, block z adds into copy z % n_slots (one block per copy
  // when n_slots == gridDim.z: bit-reproducible, reduced in a fixed order by wgrad_slot_reduce_kernel)
  const unsigned out_slot = per_sample ? (unsigned)(bz * units_per_block / sps) : (unsigned)bz % (unsigned)(n_slots > 0 ? n_slots : 1);
  const size_t out_off = (size_t)__builtin_amdgcn_readfirstlane((int)out_slot) * Co * Ci;
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // loader role: this wave moves rows [32 wv, 32 wv + 32) of both operand tiles: 4 DMA instructions per operand
  const int lrow = lane >> 3;                                      // row within the 8-row group
  auto issue = [&](int bb, int stt, int stage) {
    const int s_base = stt * 32;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = 32 * wv + 8 * q + lrow;                      // row of the 128-row tile
      const int chunk = (lane & 7) ^ ((row >> 1) & 7);             // swizzled 16-byte chunk this lane fetches
      int sidx = s_base + 4 * chunk;
      if (sidx > S - 4) sidx = S - 4;                              // tail unit: valid dummy, zeroed by the reader
      if (mb + 32 * wv + 8 * q < Co) {                             // skip row groups beyond the matrix (uniform)
        int ra = mb + row;
        if (ra >= Co) ra = Co - 1;
        wg_glds16(dz + ((size_t)bb * Co + ra) * S + sidx, &s_op[stage][0][(32 * wv + 8 * q) * 32]);
      }
      if (!same_tile && nb + 32 * wv + 8 * q < Ci) {
        int rb = nb + row;
        if (rb >= Ci) rb = Ci - 1;
        wg_glds16(x + ((size_t)bb * Ci + rb) * S + sidx, &s_op[stage][1][(32 * wv + 8 * q) * 32]);
      }
    }
  };

  int b = u0 / sps, st = u0 - b * sps;
  float sc[4] = {1.f, 1.f, 1.f, 1.f};
  float tfa[4] = {1.f, 1.f, 1.f, 1.f}, tfb[4] = {0.f, 0.f, 0.f, 0.f}, actr[4] = {0.f, 0.f, 0.f, 0.f};
  if (tf.a) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = nb + nw + 16 * j + r;
      tfa[j] = row < Ci ? tf.a[row] : 0.0f;
      tfb[j] = row < Ci ? tf.b[row] : 0.0f;
    }
  }
  if (tf.actr) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = mb + mw + 16 * i + r;
      actr[i] = row < Co ? tf.actr[row] : 0.0f;
    }
  }
  int b_sc = -1;
  issue(b, st, 0);
  int stage = 0;
  for (int u = u0; u < u1; ++u) {
    int bn = b, stn = st + 1;
    if (stn == sps) { stn = 0; ++bn; }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // unit u landed; the other stage is free
    if (u + 1 < u1) issue(bn, stn, stage ^ 1);
    if (active) {
      if (xscale && b != b_sc) {      // squeeze-excitation scale of the conv input, per (sample, input channel)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int row = nb + nw + 16 * j + r;
          sc[j] = row < Ci ? xscale[(size_t)b * Ci + row] : 0.0f;
        }
        b_sc = b;
      }
      // fragment of (row, kg): global chunks 2kg and 2kg+1 of that row, stored at the swizzled slots
      const int s_lo = st * 32 + 8 * kg;
      const bool k0 = s_lo < S, k1 = s_lo + 4 < S;
      auto frag = [&](int which, int row_in_tile, bool row_ok, float scale, bf16x8_t& hi, bf16x8_t& lo,
                      bool xf = false, float fa = 1.0f, float fb = 0.0f) {
        // (indexed, not passed as a pointer: a generic pointer to LDS makes hipcc emit a flat-address check that its gfx950
        //  back end rejects - "Operand has incorrect register class")
        const int sw = (row_in_tile >> 1) & 7;
        float4 t0 = *reinterpret_cast<const float4*>(&s_op[stage][which][row_in_tile * 32 + 4 * ((2 * kg) ^ sw)]);
        float4 t1 = *reinterpret_cast<const float4*>(&s_op[stage][which][row_in_tile * 32 + 4 * ((2 * kg + 1) ^ sw)]);
        if (xf) {                                                  // block-uniform
          t0.x = wg_tf(t0.x, fa, fb, tf.act); t0.y = wg_tf(t0.y, fa, fb, tf.act); t0.z = wg_tf(t0.z, fa, fb, tf.act); t0.w = wg_tf(t0.w, fa, fb, tf.act);
          t1.x = wg_tf(t1.x, fa, fb, tf.act); t1.y = wg_tf(t1.y, fa, fb, tf.act); t1.z = wg_tf(t1.z, fa, fb, tf.act); t1.w = wg_tf(t1.w, fa, fb, tf.act);
        }
        // row_ok also guards LDS rows that were never loaded (select, not multiply: they may hold anything)
        const bool q0 = row_ok && k0, q1 = row_ok && k1;
        const float v[8] = {q0 ? t0.x * scale : 0.0f, q0 ? t0.y * scale : 0.0f, q0 ? t0.z * scale : 0.0f,
                            q0 ? t0.w * scale : 0.0f, q1 ? t1.x * scale : 0.0f, q1 ? t1.y * scale : 0.0f,
                            q1 ? t1.z * scale : 0.0f, q1 ? t1.w * scale : 0.0f};
        if constexpr (NPROD == 3) {
          split8(v, hi, lo);
        } else {
#pragma unroll
          for (int i = 0; i < 8; i += 2) {
            const bf16x2_t h = __builtin_convertvector(f32x2_t{v[i], v[i + 1]}, bf16x2_t);
            hi[i] = h[0]; hi[i + 1] = h[1];
          }
        }
      };
      bf16x8_t bh[4], bl[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = nw + 16 * j + r;
        frag(same_tile ? 0 : 1, row, j < nt_n && nb + row < Ci, sc[j], bh[j], bl[j], tf.a != nullptr, tfa[j], tfb[j]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (i < mt_n) {
          const int row = mw + 16 * i + r;
          bf16x8_t ah, al;
          frag(0, row, mb + row < Co, 1.0f, ah, al, tf.actr != nullptr, 1.0f, actr[i]);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (j < nt_n) {
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh[j], acc[i][j], 0, 0, 0);
              if constexpr (NPROD == 3) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl[j], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh[j], acc[i][j], 0, 0, 0);
              }
            }
          }
        }
      }
    }
    b = bn; st = stn; stage ^= 1;
  }
  if (!active) return;
  float* out = dW + out_off;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (!(i < mt_n && j < nt_n)) continue;                        // wave-uniform
      // a 16 x 16 tile that lies inside the matrix (wave-uniform test) adds without per-lane tests: the 64 guarded
      // atomics of a wave were 64 exec-masked blocks
      const bool full = mb + mw + 16 * i + 16 <= Co && nb + nw + 16 * j + 16 <= Ci;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int m = mb + mw + 16 * i + kg * 4 + q, n = nb + nw + 16 * j + r;   // C/D: row = kg*4+q, col = lane&15
        float* o = out + (size_t)m * Ci + n;
        if (full) {
          if (per_sample) *o = acc[i][j][q];
          else global_atomic_add(o, acc[i][j][q]);
        } else if (m < Co && n < Ci) {
          // per-sample gradients: the block covered the sample's whole k range - a plain store, no read-modify-write
          if (per_sample) *o = acc[i][j][q];
          else global_atomic_add(o, acc[i][j][q]);
        }
      }
    }
}

// ---- "wide-tile" weight gradient with producer / consumer waves (round 4) -------------------------------------------
// Measured on pw_wgrad_x3_kernel with its phases switched off one at a time (672 x 112 at 504 positions x 256 clips):
// loads alone 68 us (6 TB/s), fragment preparation + MFMAs alone > 100 us, the atomics 25 us - and the phases add up:
// every wave of a block goes through load wait, bf16 hi / lo split, MFMAs in lock step, so the matrix pipe idles while the
// VALUs convert and the memory pipe idles while both work.  The split itself is repeated by every wave for every fragment
// it multiplies (a row tile of the 128 x 128 block is converted by 2 waves).  And the 128-row tiles re-read the narrow
// operand once per row tile, missing L2 (PMC: FETCH_SIZE = the loads; the row tiles of a k-slice run on different XCDs):
// 694 MB loaded for 404 MB of operands.  This kernel:
//  * one block of 8 waves per CU owns a tile of up to 256 rows of the WIDE operand P (whichever of dz / x has more rows;
//    SWAP = x) times up to 160 rows of the narrow operand Q - for every mn10 layer all of Q, so both operands are read
//    once; the row tiles are balanced (672 rows = 3 tiles of 224, not 256 + 256 + 160);
//  * PRODUCER / CONSUMER waves: a workgroup's waves are dealt to the SIMDs round robin, so waves 0-3 (consumers) and 4-7
//    (producers) are one of each per SIMD.  A producer loads 1 KB pieces (8 rows x 32 positions, 16 bytes per lane: 8 full
//    128-byte lines per instruction) into REGISTERS, three 32-position units ahead (3 x 13 pieces x 4 VGPRs: the bytes in
//    flight live in the producers' otherwise idle register file, ~126 KB per CU, not in LDS), CONVERTS ONCE - 4 floats ->
//    4 bf16 hi + 4 bf16 lo with the x side's transform, SE scale and the k-tail mask applied there: 12 VALU per 4 elements
//    once instead of ~45 per fragment in each of the waves using it - and stores the fragments to one of two LDS slots.  A
//    consumer owns 64 rows of P x all of Q (up to 4 x 10 accumulator tiles) and does nothing but ds_read_b128 + MFMA.
//    One s_barrier per unit hands unit u + 1 to the consumers and the slot of unit u - 1 back to the producers: loads of
//    units u + 2 ... u + 4 and the conversion of u + 1 overlap the MFMAs of u on the same SIMD.
//  * LDS layout of a slot: row-major, 128 bytes per (row, 32 positions); the two 4-position chunks 2 kg, 2 kg + 1 of an
//    MFMA fragment share a 32-byte block [8 hi | 8 lo] (or [8 lo | 8 hi]: rows with bit 1 set swap the halves, and the block
//    index is XORed with bits 2-3 of the row, so that the 16 rows of a fragment read hit 16 different 16-byte bank groups).
using u32x2_t = __attribute__((ext_vector_type(2))) unsigned;
constexpr int WIDE_PT = 4, WIDE_QT = 10;                           // 16-row tiles per consumer wave: 64 rows of P x 160 rows of Q
constexpr int WIDE_NP = 13, WIDE_TP = 8;                            // register slots per producer wave and unit: 8 pieces of P (4 waves
                                                                   // x 8 x 8 rows = 256) and 5 of Q (160 rows)
constexpr int WIDE_RD = 3;                                         // units a producer holds in registers
template <int V> struct WideInt { static constexpr int value = V; };
// (an instantiation with the x operand read through act(a v + b) - the project conv's on-load input - made the producers the
//  pole: 40 x 120 at 2000 positions 152 us against 128 for the 128 x 128-tile kernel; those launches keep that kernel)
// RADD: an additive constant per x row (radd), applied to loaded elements only - the centred Gram matrix (same = 1)
// P16: the P operand is bf16 in HBM (act_io.h; the bf16-storage plan: P = the wide tensor - the project conv's input y_d / z_d
// when SWAP, the expand conv's gradient g otherwise - and Q the narrow fp32 one).  A producer then moves 8 bytes per lane and
// piece and its fragments need NO conversion; PTF (with SWAP, P16): the x rows are act(tf_a[ci] v + tf_b[ci]) evaluated on
// load (the on-load BatchNorm of the project conv's input), times the SE scale - unpack, 4 VALU, one v_cvt_pk per pair, which
// the fp32 instantiation could not afford next to its hi / lo split.  Host: P16 only with NPROD = 1.
template <int NPROD, bool SWAP, bool SCALE, bool RADD, bool P16 = false, bool PTF = false>
__global__ __launch_bounds__(512) void pw_wgrad_wide_kernel(const float* __restrict__ dz, const float* __restrict__ x,
                                                            const float* __restrict__ xscale, float* __restrict__ dW, int B,
                                                            int Co, int Ci, int S, int sps, int units_per_block,
                                                            int p_tile_rows, int q_tile_rows,
                                                            const float* __restrict__ radd, int same,
                                                            const float* __restrict__ tf_a = nullptr,
                                                            const float* __restrict__ tf_b = nullptr, int tf_act = 0,
                                                            int ps_ns = 0) {
  // ps_ns > 0 (per-sample gradients, eat_pw_conv_dyn_wgrad_b16): gridDim.z = B * ps_ns, block z multiplies slice z % ps_ns
  // (units_per_block units, clipped to the sample) of sample z / ps_ns and stores it as copy (slice * B + sample) of dW: copy
  // 0 of every sample forms the (B, Co, Ci) result, to which the caller adds the other slices
  static_assert(!P16 || NPROD == 1, "bf16-stored operand: plain bf16 products");
  static_assert(!PTF || (P16 && SWAP), "on-load transform: the bf16-stored x operand");
  constexpr unsigned PB = P16 ? 2u : 4u;                              // bytes per element of P
  extern __shared__ __attribute__((aligned(16))) float w_smem[];
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const float* __restrict__ P = SWAP ? x : dz;
  const float* __restrict__ Q = SWAP ? dz : x;
  const int PR = SWAP ? Ci : Co, QR = SWAP ? Co : Ci;
  // same (Gram matrix, dz == x, one tile): the Q operand IS the P operand - no Q pieces, Q fragments read from P's rows;
  // radd (or NULL): additive constant per x row, applied to loaded elements only (the centred Gram matrix)
  const int p0 = blockIdx.x * p_tile_rows, q0 = blockIdx.y * q_tile_rows;
  const int pv = (PR - p0) < p_tile_rows ? (PR - p0) : p_tile_rows;   // valid rows of this block's tile
  const int qv = (QR - q0) < q_tile_rows ? (QR - q0) : q_tile_rows;
  const int total = B * sps;
  int u0 = blockIdx.z * units_per_block;
  int u1 = (u0 + units_per_block) < total ? (u0 + units_per_block) : total;
  unsigned out_slot = blockIdx.z;
  if (ps_ns > 0) {
    const int sb = (int)blockIdx.z / ps_ns, sj = (int)blockIdx.z - sb * ps_ns;
    u0 = sb * sps + sj * units_per_block;
    u1 = (u0 + units_per_block) < (sb + 1) * sps ? (u0 + units_per_block) : (sb + 1) * sps;
    out_slot = (unsigned)(sj * B + sb);
  }
  if (pv <= 0 || qv <= 0 || u0 >= u1) return;                         // block-uniform, before any barrier
  const int pt = (pv + 15) >> 4, qt = (qv + 15) >> 4;                 // 16-row tiles
  const int GP = pt * 2, GQ = same ? 0 : (qv + 7) >> 3;               // 8-row pieces (P: whole 16-row tiles, so that the Q rows start
                                                                      // on a multiple of 16: one swizzle term for all tiles)
  const int GD = GP + GQ;
  const int slot_f = GD * 256;                                        // floats per LDS slot
  const int wq = wv & 3;

  // (measured without effect: s_setprio 1 / 3 for the producers - the later-dispatched half -, for the consumers, and
  //  the roles swapped: 141 - 146 us against 143 - 151 for 672 x 112)
  if (wv >= 4) {
    // ------------------------------------------------------------------ producer: loads, conversion, LDS stores
    // The loads of a unit are STRAIGHT-LINE code - every producer issues WIDE_NP of them per unit whatever the tile size
    // (slots past the last piece fetch one broadcast line), units past the block's range re-fetch the last unit, the SE scale
    // is fetched every step for the unit converted in the next one: with loads inside conditional blocks the compiler's
    // wait-count pass falls back to vmcnt(0) at every use, which drains the three units in flight.
    const int lrow = lane >> 3, chunk = lane & 7;                     // this lane's 16 bytes of a piece: row lrow, positions 4 chunk ...
    // register slot t of a producer: t < WIDE_TP -> piece wq + 4 t of P, else piece wq + 4 (t - WIDE_TP) of Q (fixed slot classes:
    // the slots that hold x rows - transform coefficients, SE scale - are known at compile time)
    constexpr int XS0 = SWAP ? 0 : WIDE_TP, XN = SWAP ? WIDE_TP : WIDE_NP - WIDE_TP;
    // per slot: byte offset of this lane's 16 bytes relative to (operand + sample offset + 32 * unit)
    unsigned roff[WIDE_NP];
    int xrow[SCALE ? XN : 1];
    float ra[RADD ? XN : 1];
    float tfa[PTF ? XN : 1], tfb[PTF ? XN : 1];
#pragma unroll
    for (int t = 0; t < WIDE_NP; ++t) {
      const bool isp = t < WIDE_TP;
      const int g = wq + 4 * (isp ? t : t - WIDE_TP);                 // piece of P / of Q (wave-uniform)
      const int mr = g * 8 + lrow, nv = isp ? pv : qv;
      const int row = (isp ? p0 : q0) + (mr > nv - 1 ? nv - 1 : mr);
      const bool valid = g < (isp ? GP : GQ);
      const unsigned eb = isp ? PB : 4u;
      roff[t] = valid ? eb * ((unsigned)row * (unsigned)S + 4u * (unsigned)chunk) : eb * (unsigned)(isp ? p0 : q0) * (unsigned)S;
      if (t >= XS0 && t < XS0 + XN) {
        const int xr = row < Ci ? row : Ci - 1;
        if constexpr (SCALE) xrow[t - XS0] = xr;
        if constexpr (RADD) ra[t - XS0] = radd[xr];
        if constexpr (PTF) { tfa[t - XS0] = tf_a[xr]; tfb[t - XS0] = tf_b[xr]; }
      }
    }
    if constexpr (PTF) {
#pragma unroll
      for (int t = 0; t < XN; ++t) asm volatile("" ::"v"(tfa[t]), "v"(tfb[t]));
    }
    // (the loads above must be back - and known to the compiler to be back - before the loop: a wait it placed at their first
    //  use inside the loop would be a vmcnt(0) per step; the empty asm statements read the registers)
    if constexpr (RADD) {
#pragma unroll
      for (int t = 0; t < XN; ++t) asm volatile("" ::"v"(ra[t]));
    }
    const bool tail = (S & 31) != 0;
    float4 buf[WIDE_RD][WIDE_NP];
    u32x2_t pbuf[WIDE_RD][P16 ? WIDE_TP : 1];                        // P16: the P slots hold 4 bf16 (not members of a float4:
                                                                      // hipcc folded `.y` of a partly written float4 into `.x`)
    float xs[SCALE ? XN : 1], xs_next[SCALE ? XN : 1];
    auto load_unit = [&](auto ktag, int bb, int stt) {
      constexpr int K = decltype(ktag)::value;
      const char* pb = reinterpret_cast<const char*>(P) + ((size_t)bb * PR * S + (size_t)stt * 32) * PB;
      const char* qb = reinterpret_cast<const char*>(Q + ((size_t)bb * QR * S + (size_t)stt * 32));
      // the sample's last unit: chunks past S fetch a valid dummy (zeroed by the converter)
      const int lim = S - 4 - stt * 32;                               // largest valid k offset inside this unit
      const unsigned back_e = (tail && stt == sps - 1 && 4 * chunk > lim) ? (unsigned)(4 * chunk - lim) : 0u;   // elements
#pragma unroll
      for (int t = 0; t < WIDE_NP; ++t) {
        const bool isp = t < WIDE_TP;
        const bool valid = wq + 4 * (isp ? t : t - WIDE_TP) < (isp ? GP : GQ);
        if (isp && P16) {                                             // (compile-time per slot) 4 bf16 = 8 bytes
          pbuf[K][t < WIDE_TP ? t : 0] = *reinterpret_cast<const u32x2_t*>(pb + (valid ? roff[t] - PB * back_e : roff[t]));
        } else {
          buf[K][t] = *reinterpret_cast<const float4*>((isp ? pb : qb) + (valid ? roff[t] - (isp ? PB : 4u) * back_e : roff[t]));
        }
      }
    };
    auto load_scale = [&](int bb) {                                   // SE scale of the conv input, per (sample, input channel)
      if constexpr (SCALE) {
#pragma unroll
        for (int t = 0; t < XN; ++t) xs_next[t] = xscale[(size_t)bb * Ci + xrow[t]];
      }
    };
    const int hb = (lrow >> 1) & 1;
    auto convert_unit = [&](auto ktag, int slot, int stt) {
      constexpr int K = decltype(ktag)::value;
      const int sb = slot * slot_f;
      const bool kz = tail && stt * 32 + 4 * chunk >= S;              // k tail (S % 4 == 0: whole chunks)
#pragma unroll
      for (int t = 0; t < WIDE_NP; ++t) {
        const bool isp = t < WIDE_TP;
        const int g = wq + 4 * (isp ? t : t - WIDE_TP);
        if (g < (isp ? GP : GQ)) {
          const int gi = isp ? g : GP + g;                            // piece of the LDS slot
          float4 w = (isp && P16) ? float4{0.f, 0.f, 0.f, 0.f} : buf[K][t];
          const int blk = (chunk >> 1) ^ (((gi & 1) << 1) | (lrow >> 2));   // 32-byte block of the row: (c >> 1) ^ ((row >> 2) & 3)
          const int rowf = sb + gi * 256 + lrow * 32 + 8 * blk + 2 * (chunk & 1);
          if (isp && P16) {                                            // (compile-time per slot) finished bf16 pairs
            unsigned w01 = pbuf[K][t < WIDE_TP ? t : 0][0], w23 = pbuf[K][t < WIDE_TP ? t : 0][1];
            if constexpr (SWAP && (SCALE || PTF)) {                    // P = the x rows: transform / SE scale on load
              float v0 = eat::bf_lo(w01), v1 = eat::bf_hi(w01), v2 = eat::bf_lo(w23), v3 = eat::bf_hi(w23);
              if constexpr (PTF) {
                const float fa = tfa[t < XN ? t : 0], fb = tfb[t < XN ? t : 0];
                v0 = wg_tf(v0, fa, fb, tf_act); v1 = wg_tf(v1, fa, fb, tf_act);
                v2 = wg_tf(v2, fa, fb, tf_act); v3 = wg_tf(v3, fa, fb, tf_act);
              }
              if constexpr (SCALE) {
                const float sc = xs[t < XN ? t : 0];
                v0 *= sc; v1 *= sc; v2 *= sc; v3 *= sc;
              }
              w01 = eat::pack_bf2(v0, v1); w23 = eat::pack_bf2(v2, v3);
            }
            if (kz) { w01 = 0u; w23 = 0u; }
            *reinterpret_cast<u32x2_t*>(&w_smem[rowf + 4 * hb]) = u32x2_t{w01, w23};
            continue;
          }
          if constexpr (SCALE) {
            if (t >= XS0 && t < XS0 + XN) {
              const float sc = xs[t - XS0 < 0 ? 0 : t - XS0];
              w.x *= sc; w.y *= sc; w.z *= sc; w.w *= sc;
            }
          }
          if constexpr (RADD) {
            if (t >= XS0 && t < XS0 + XN) {                           // centring constant of the row
              const float c = ra[t - XS0 < 0 ? 0 : t - XS0];
              w.x += c; w.y += c; w.z += c; w.w += c;
            }
          }
          if (kz) w = float4{0.f, 0.f, 0.f, 0.f};
          const bf16x2_t h01 = __builtin_convertvector(f32x2_t{w.x, w.y}, bf16x2_t);
          const bf16x2_t h23 = __builtin_convertvector(f32x2_t{w.z, w.w}, bf16x2_t);
          *reinterpret_cast<u32x2_t*>(&w_smem[rowf + 4 * hb]) = u32x2_t{__builtin_bit_cast(unsigned, h01), __builtin_bit_cast(unsigned, h23)};
          if constexpr (NPROD == 3) {
            const bf16x2_t l01 = __builtin_convertvector(f32x2_t{w.x - (float)h01[0], w.y - (float)h01[1]}, bf16x2_t);
            const bf16x2_t l23 = __builtin_convertvector(f32x2_t{w.z - (float)h23[0], w.w - (float)h23[1]}, bf16x2_t);
            *reinterpret_cast<u32x2_t*>(&w_smem[rowf + 4 * (1 - hb)]) = u32x2_t{__builtin_bit_cast(unsigned, l01), __builtin_bit_cast(unsigned, l23)};
          }
        }
      }
    };
    // (the lambdas take the unit's coordinates by value and the code below advances them: counters captured by reference
    //  and modified inside a generic lambda ended up in scratch memory)
    int bi = u0 / sps, sti = u0 - bi * sps, ui = u0;                  // next unit to load (stops at the last unit of the range)
    int bc = bi, stc = sti, uc = u0;                                  // next unit to convert
#define WIDE_LOAD(K_)                                                          \
    do {                                                                       \
      load_unit(WideInt<K_>{}, bi, sti);                                       \
      if (ui + 1 < u1) { ++ui; if (++sti == sps) { sti = 0; ++bi; } }          \
    } while (0)
    // conversion of unit uc; before it, the SE scale of the unit converted NEXT is requested (used one step later, when
    // only the loads issued after it are still in flight)
#define WIDE_CONVERT(K_, SLOT_)                                                \
    do {                                                                       \
      if constexpr (SCALE) {                                                   \
        _Pragma("unroll") for (int t = 0; t < XN; ++t) xs[t] = xs_next[t];      \
        const int bn = stc + 1 == sps ? bc + 1 : bc;                           \
        load_scale(bn < B ? bn : B - 1);                                       \
      }                                                                        \
      if (uc < u1) convert_unit(WideInt<K_>{}, SLOT_, stc);                    \
      ++uc;                                                                    \
      if (++stc == sps) { stc = 0; ++bc; }                                     \
    } while (0)
    // unit u0 + m lives in buf[m % 3] and goes to LDS slot m % 2
    load_scale(bc);
    WIDE_LOAD(0); WIDE_LOAD(1); WIDE_LOAD(2);
    WIDE_CONVERT(0, 0);
    WIDE_LOAD(0);
    // step n (after barrier n the consumers multiply unit n): convert unit n + 1, reload its registers with unit n + 4
    const int nsteps = u1 - u0;
    for (int n = 0; n < nsteps; n += 3) {
      __syncthreads();                                                // barrier n: unit n is in LDS; the slot of unit n - 1 is free
      WIDE_CONVERT(1, (n + 1) & 1);
      WIDE_LOAD(1);
      if (n + 1 >= nsteps) break;
      __syncthreads();
      WIDE_CONVERT(2, (n + 2) & 1);
      WIDE_LOAD(2);
      if (n + 2 >= nsteps) break;
      __syncthreads();
      WIDE_CONVERT(0, (n + 3) & 1);
      WIDE_LOAD(0);
    }
#undef WIDE_LOAD
#undef WIDE_CONVERT
    return;
  }

  // -------------------------------------------------------------------- consumer: fragments + MFMA
  const int r = lane & 15, kg = lane >> 4;
  const int pbase = pt >> 2, pext = pt & 3;                           // P tiles of this wave: [pm0, pm0 + pm_n)
  const int pm_n = pbase + (wq < pext ? 1 : 0), pm0 = wq * pbase + (wq < pext ? wq : pext);
  f32x4 acc[WIDE_PT][WIDE_QT];
#pragma unroll
  for (int i = 0; i < WIDE_PT; ++i)
#pragma unroll
    for (int j = 0; j < WIDE_QT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // per-lane LDS offsets (floats) of the fragment of row r (of any 16-row tile), k group kg: 16 bytes of hi, 16 bytes of lo
  // inside the row's 32-byte block kg ^ ((r >> 2) & 3), halves swapped for rows with bit 1 set (see the converter)
  const int fblk = r * 32 + 8 * (kg ^ ((r >> 2) & 3));
  const int f_hi = fblk + 4 * ((r >> 1) & 1), f_lo = fblk + 4 * (1 - ((r >> 1) & 1));
  const int p_off = pm0 * 512, q_off = same ? 0 : GP * 256;
  for (int u = u0; u < u1; ++u) {
    __syncthreads();                                                  // unit u is in LDS slot (u - u0) & 1
    if (pm_n > 0) {
      const int sb = ((u - u0) & 1) * slot_f;
      // all WIDE_PT fragments of P, whatever pm_n is: a wave with 3 tiles multiplies a 4th (the next wave's rows, or Q rows,
      // or zeros past the end of LDS) into accumulators that are never written - it would wait at the barrier for the waves
      // with 4 tiles anyway, and the loop has no data-dependent control flow around its fragment registers
      bf16x8_t ph[WIDE_PT], pl[WIDE_PT];
#pragma unroll
      for (int i = 0; i < WIDE_PT; ++i) {
        ph[i] = *reinterpret_cast<const bf16x8_t*>(&w_smem[sb + p_off + 512 * i + f_hi]);
        if constexpr (NPROD == 3) pl[i] = *reinterpret_cast<const bf16x8_t*>(&w_smem[sb + p_off + 512 * i + f_lo]);
      }
      // the Q fragment of tile j + 1 is read before the MFMAs of tile j (past the last tile it reads the other slot or zeros
      // beyond the LDS allocation - never used)
      bf16x8_t qh, ql;
      qh = *reinterpret_cast<const bf16x8_t*>(&w_smem[sb + q_off + f_hi]);
      if constexpr (NPROD == 3) ql = *reinterpret_cast<const bf16x8_t*>(&w_smem[sb + q_off + f_lo]);
#pragma unroll
      for (int j = 0; j < WIDE_QT; ++j) {
        if (j < qt) {
          bf16x8_t nh, nl;
          if (j + 1 < WIDE_QT) {
            nh = *reinterpret_cast<const bf16x8_t*>(&w_smem[sb + q_off + 512 * (j + 1) + f_hi]);
            if constexpr (NPROD == 3) nl = *reinterpret_cast<const bf16x8_t*>(&w_smem[sb + q_off + 512 * (j + 1) + f_lo]);
          }
#pragma unroll
          for (int i = 0; i < WIDE_PT; ++i) {
            // D rows (kg * 4 + e) follow the first operand, D columns (lane & 15) the second: the x / Ci index goes FIRST, so
            // that a lane's four accumulator values are four consecutive columns of dW (one 16-byte store)
            if constexpr (SWAP) {
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph[i], qh, acc[i][j], 0, 0, 0);
              if constexpr (NPROD == 3) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ph[i], ql, acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pl[i], qh, acc[i][j], 0, 0, 0);
              }
            } else {
              acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qh, ph[i], acc[i][j], 0, 0, 0);
              if constexpr (NPROD == 3) {
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qh, pl[i], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ql, ph[i], acc[i][j], 0, 0, 0);
              }
            }
          }
          if (j + 1 < WIDE_QT) { qh = nh; if constexpr (NPROD == 3) ql = nl; }
        }
      }
    }
  }
  if (pm_n <= 0) return;
  // Epilogue: PLAIN 16-byte stores into this k-slice's own copy of dW (ws holds gridDim.z copies; wgrad_slot_reduce4_kernel
  // adds them in a fixed order: bit-reproducible).  The atomic form - 160 wave-instructions of 64 fp32 atomics per consumer -
  // cost 25 - 35 us of the 85 - 145 us launches (the same-address adds of all k-slices arrive together).
  float* out = dW + (size_t)out_slot * Co * Ci;
#pragma unroll
  for (int i = 0; i < WIDE_PT; ++i)
#pragma unroll
    for (int j = 0; j < WIDE_QT; ++j) {
      if (!(i < pm_n && j < qt)) continue;                            // wave-uniform
      const int pr0 = 16 * (pm0 + i), qr0 = 16 * j;                   // tile origins inside the block tile
      // C/D layout: row = kg * 4 + e (first MFMA operand = the x rows = columns n of dW), column = lane & 15 (the dz rows m);
      // rows / columns past the matrix hold products of the clamped duplicate rows and are not written (Ci % 4 == 0)
      const int m = SWAP ? q0 + qr0 + r : p0 + pr0 + r;
      const int n = (SWAP ? p0 + pr0 : q0 + qr0) + kg * 4;
      if (m < Co && n < Ci) *reinterpret_cast<f32x4*>(out + (size_t)m * Ci + n) = acc[i][j];
    }
}

// units of one wave in registers (one being multiplied, the others in flight) for a block tile of `tiles` operand row
// tiles (8 VGPRs of raw data each), as measured at B = 256 (profiles/thin_wgrad_before_after.md): a third unit pays on
// the five-tile blocks (64 x 16 @ 32000: 446 vs 460 us), deeper rings cost the small blocks their occupancy (1024 blocks
// want four resident per CU) and gained nothing; seven tiles hold two units in 256 VGPRs (two blocks per CU, no scratch)
constexpr int narrow_ring(int tiles) { return tiles <= 1 ? 4 : tiles == 5 ? 3 : 2; }

// Narrow layers (one side <= 16 channels, the other <= 64: mn10 block 1 and the expand of block 2, planes of 32000
// positions): dW is a single 64 x 64 wave tile and the gradient is a pure streaming reduction over k.  Here the direct,
// LDS-free form wins: the 4 waves of a block split the k range, every lane loads the 8 consecutive k of its row straight
// from HBM (one full 128-byte line per row and unit).  The tile counts are compile-time (a 16 x 16 product keeps 8, not
// 128, operand registers), the raw rows of the next 1 - 3 units are in flight behind the MFMAs of the current one, and
// SAME (dz == x: the Gram matrix of train_fuse.hip) loads once.
template <int MTN, int NTN, bool SAME>
__global__ __launch_bounds__(256, 2) void pw_wgrad_x3_narrow_kernel(const float* __restrict__ dz, const float* __restrict__ x,
                                                                    const float* __restrict__ xscale, float* __restrict__ dW,
                                                                    int B, int Co, int Ci, int S, int sps,
                                                                    int units_per_block, int n_slots, WgTf tf, int ps_spl) {
  // the four waves' tiles are combined in LDS (ds_add_f32) before ONE set of global atomics per block, and the blocks
  // are spread over n_slots copies of dW (reduced by wgrad_slot_reduce_kernel): atomics on the same address serialise
  // in L2 at ~40 ns each, which made the 8192 (= 2048 blocks x 4 waves) adds per element the whole cost of this kernel
  // on the 16 x 16 layers (311 us for 105 us of HBM time)
  __shared__ float s_tile[MTN * NTN * 256];
  // wv through readfirstlane: the compiler then knows it (and the tile counts derived from it) to be wave-uniform - scalar
  // branches instead of exec-masked blocks around the loads and MFMAs of rows beyond the matrix
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int r = lane & 15, kg = lane >> 4;
  // round 3: blockIdx.x / blockIdx.y select a group of MTN / NTN row tiles ("thin" matrices: up to ~8 x 8 tiles over a
  // long k axis stream faster through this LDS-free kernel than through the barrier-per-32-positions LDS pipeline)
  const int m0 = blockIdx.x * (16 * MTN), n0 = SAME ? m0 : blockIdx.y * (16 * NTN);
  // ps_spl > 0: per-sample gradients (DyMN, models/dymn/dy_block.py:120-127 backward): ps_spl blocks share a sample's k
  // range and add into that sample's own Co x Ci matrix
  const int ps_b = ps_spl > 0 ? (int)blockIdx.z / ps_spl : 0;
  const int total = ps_spl > 0 ? (ps_b + 1) * sps : B * sps;
  const int u0 = ps_spl > 0 ? ps_b * sps + ((int)blockIdx.z - ps_b * ps_spl) * units_per_block : (int)blockIdx.z * units_per_block;
  const int u1 = (u0 + units_per_block) < total ? (u0 + units_per_block) : total;
  for (int i = threadIdx.x; i < MTN * NTN * 256; i += 256) s_tile[i] = 0.0f;
  __syncthreads();
  f32x4 acc[MTN][NTN];
#pragma unroll
  for (int i = 0; i < MTN; ++i)
#pragma unroll
    for (int j = 0; j < NTN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // No load of this kernel depends on a per-lane condition: rows and positions are clamped to valid addresses and what
  // lies outside the matrix / plane is zeroed by a select at conversion time.  A load inside a conditional block
  // (`ok ? load : 0`) makes the compiler's wait-count pass fall back to vmcnt(0) at its use, which drains every unit in flight.
  const float* tfa_p = tf.a ? tf.a : x;                         // (x holds >= Ci, dz >= Co floats: stand-ins, selected away)
  const float* tfb_p = tf.a ? tf.b : x;
  const float* actr_p = tf.actr ? tf.actr : dz;
  const float* sc_p = xscale ? xscale : x;
  float tfa[NTN], tfb[NTN], actr[MTN];
  size_t xoff[SAME ? 1 : NTN], zoff[MTN];                       // clamped row * S
  int xrow[SAME ? 1 : NTN];
  bool xok[NTN], zok[MTN];
#pragma unroll
  for (int j = 0; j < NTN; ++j) {
    const int row = n0 + 16 * j + r, rc = row < Ci ? row : Ci - 1;
    xok[j] = row < Ci;
    if constexpr (!SAME) { xrow[j] = rc; xoff[j] = (size_t)rc * S; }
    const float ta = tfa_p[rc], tb = tfb_p[rc];
    tfa[j] = (tf.a && row < Ci) ? ta : 1.0f;
    tfb[j] = (tf.a && row < Ci) ? tb : 0.0f;
  }
#pragma unroll
  for (int i = 0; i < MTN; ++i) {
    const int row = m0 + 16 * i + r, rc = row < Co ? row : Co - 1;
    zok[i] = row < Co;
    zoff[i] = (size_t)rc * S;
    const float tc = actr_p[rc];
    actr[i] = (tf.actr && row < Co) ? tc : 0.0f;
  }
  // (the coefficient loads must be back - and known to the compiler to be back - before the loop: a wait placed at their
  //  first use inside it would be a full drain per step; the empty asm statements read the registers)
#pragma unroll
  for (int j = 0; j < NTN; ++j) asm volatile("" ::"v"(tfa[j]), "v"(tfb[j]));
#pragma unroll
  for (int i = 0; i < MTN; ++i) asm volatile("" ::"v"(actr[i]));

  // one unit of one wave: the raw 2 x 16 bytes per row tile, the SE scale of the unit's sample (requested with the unit,
  // RING - 1 steps before its use) and the lane's first position
  struct Unit { float4 a[MTN][2]; float4 b[SAME ? 1 : NTN][2]; float sc[SAME ? 1 : NTN]; int s; };
  auto load = [&](int u, Unit& q) {
    const int b = u / sps, st = u - b * sps;                    // (u < u1, wave-uniform)
    const int s = st * 32 + 8 * kg;
    const int s0 = s < S - 4 ? s : S - 4, s1 = s + 4 < S - 4 ? s + 4 : S - 4;   // (S % 4 == 0, S >= 4)
    q.s = s;
    const float* zb = dz + (size_t)b * Co * S;
#pragma unroll
    for (int i = 0; i < MTN; ++i) {
      q.a[i][0] = *reinterpret_cast<const float4*>(zb + zoff[i] + s0);
      q.a[i][1] = *reinterpret_cast<const float4*>(zb + zoff[i] + s1);
    }
    if constexpr (!SAME) {
      const float* xb = x + (size_t)b * Ci * S;
      const float* sb = sc_p + (xscale ? (size_t)b * Ci : (size_t)0);
#pragma unroll
      for (int j = 0; j < NTN; ++j) {
        q.b[j][0] = *reinterpret_cast<const float4*>(xb + xoff[j] + s0);
        q.b[j][1] = *reinterpret_cast<const float4*>(xb + xoff[j] + s1);
        q.sc[j] = sb[xrow[j]];
      }
    }
  };
  auto compute = [&](const Unit& q) {
    const bool k0 = q.s < S, k1 = q.s + 4 < S;
    bf16x8_t ah[MTN], al[MTN];
#pragma unroll
    for (int i = 0; i < MTN; ++i) {
      const bool ok0 = zok[i] && k0, ok1 = zok[i] && k1;
      const float c0 = ok0 ? actr[i] : 0.0f, c1 = ok1 ? actr[i] : 0.0f;      // (0 without centring: elements unchanged)
      const float4 t0 = q.a[i][0], t1 = q.a[i][1];
      const float av[8] = {(ok0 ? t0.x : 0.0f) + c0, (ok0 ? t0.y : 0.0f) + c0, (ok0 ? t0.z : 0.0f) + c0, (ok0 ? t0.w : 0.0f) + c0,
                           (ok1 ? t1.x : 0.0f) + c1, (ok1 ? t1.y : 0.0f) + c1, (ok1 ? t1.z : 0.0f) + c1, (ok1 ? t1.w : 0.0f) + c1};
      split8(av, ah[i], al[i]);
    }
#pragma unroll
    for (int j = 0; j < NTN; ++j) {
      bf16x8_t bh, bl;
      if constexpr (SAME) {
        bh = ah[j]; bl = al[j];                                 // host: MTN == NTN
      } else {
        const bool ok0 = xok[j] && k0, ok1 = xok[j] && k1;
        const float4 t0 = q.b[j][0], t1 = q.b[j][1];
        float t[8] = {ok0 ? t0.x : 0.0f, ok0 ? t0.y : 0.0f, ok0 ? t0.z : 0.0f, ok0 ? t0.w : 0.0f,
                      ok1 ? t1.x : 0.0f, ok1 ? t1.y : 0.0f, ok1 ? t1.z : 0.0f, ok1 ? t1.w : 0.0f};
        if (tf.a) {                                             // block-uniform; invalid elements stay 0
#pragma unroll
          for (int e = 0; e < 8; ++e) t[e] = (e < 4 ? ok0 : ok1) ? wg_tf(t[e], tfa[j], tfb[j], tf.act) : 0.0f;
        }
        const float scj = xscale ? (xok[j] ? q.sc[j] : 0.0f) : 1.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) t[e] *= scj;
        split8(t, bh, bl);
      }
#pragma unroll
      for (int i = 0; i < MTN; ++i) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl, acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh, acc[i][j], 0, 0, 0);
      }
    }
  };

  // a ring of RING units per wave, RING - 1 of them in flight behind the one being multiplied; a wave still takes its
  // units in the order u0 + wv, + 4, + 8, ... (the sum order of a block's tile does not depend on RING).  The main loop
  // runs while all of its loads are inside the range: no condition around a load or a unit's MFMAs, counted waits.  The
  // first RING - 1 requests and the last <= 2 RING - 2 units sit behind wave-uniform range checks instead of re-fetching
  // a clamped unit: the 16-unit blocks of the 40-channel Gram launches are all head and tail, and fetching the last unit
  // again for every slot past the range cost them 3 - 7 us of 37.
  constexpr int RING = narrow_ring(MTN + (SAME ? 0 : NTN));
  Unit ring[RING];
  int u = u0 + wv;
#pragma unroll
  for (int k = 0; k + 1 < RING; ++k)
    if (u + 4 * k < u1) load(u + 4 * k, ring[k]);
  for (; u + 4 * (2 * RING - 2) < u1; u += 4 * RING) {
#pragma unroll
    for (int k = 0; k < RING; ++k) {
      load(u + 4 * (k + RING - 1), ring[(k + RING - 1) % RING]);
      compute(ring[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < 2 * RING - 2; ++k) {
    if (u + 4 * (k + RING - 1) < u1) load(u + 4 * (k + RING - 1), ring[(k + RING - 1) % RING]);
    if (u + 4 * k < u1) compute(ring[k % RING]);
  }
  // the four waves add their tiles in a FIXED order (wave 0, 1, 2, 3): with one slot per block the result is then
  // bit-reproducible from run to run - needed for the Gram matrix, whose round-off reaches the BatchNorm statistics
  for (int w = 0; w < 4; ++w) {
    if (wv == w) {
#pragma unroll
      for (int i = 0; i < MTN; ++i)
#pragma unroll
        for (int j = 0; j < NTN; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q) s_tile[((i * NTN + j) * 4 + q) * 64 + lane] += acc[i][j][q];
    }
    __syncthreads();
  }
  float* out = dW + (size_t)(ps_spl > 0 ? ps_b : (int)(blockIdx.z % n_slots)) * Co * Ci;
  for (int e = threadIdx.x; e < MTN * NTN * 256; e += 256) {
    const int ln = e & 63, q = (e >> 6) & 3, ij = e >> 8;
    const int i = ij / NTN, j = ij - i * NTN;
    const int m = m0 + 16 * i + (ln >> 4) * 4 + q, n = n0 + 16 * j + (ln & 15);
    if (m < Co && n < Ci) atomicAdd(out + (size_t)m * Ci + n, s_tile[e]);
  }
}

// dW[e] += sum over the slots of ws, in a fixed order (bit-reproducible): a block owns 64 consecutive elements, its four
// waves split the slots (wave w: slots w, w+4, ...; the loads of 16 slots are in flight together), the four partial
// sums are added in wave order.  (One thread per element walking up to 1024 slots took ~250 us: a serial latency chain.)
__global__ __launch_bounds__(256) void wgrad_slot_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dW, int n,
                                                                int n_slots) {
  __shared__ float s_part[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int e = blockIdx.x * 64 + lane;
  float t = 0.0f;
  if (e < n) {
    int sidx = wv;
    for (; sidx + 60 < n_slots; sidx += 64) {
      float v[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) v[q] = ws[(size_t)(sidx + 4 * q) * n + e];
#pragma unroll
      for (int q = 0; q < 16; ++q) t += v[q];
    }
    for (; sidx < n_slots; sidx += 4) t += ws[(size_t)sidx * n + e];
  }
  s_part[wv][lane] = t;
  __syncthreads();
  if (wv == 0 && e < n) dW[e] += ((s_part[0][lane] + s_part[1][lane]) + s_part[2][lane]) + s_part[3][lane];
}

// the same for n % 4 == 0 with 16-byte loads: a block adds 256 elements of up to n_slots copies (the wide-tile kernel's
// per-k-slice copies: 25 - 39 MB per launch on the late mn10 layers)
__global__ __launch_bounds__(256) void wgrad_slot_reduce4_kernel(const float* __restrict__ ws, float* __restrict__ dW, int n,
                                                                 int n_slots) {
  __shared__ f32x4 s_part[4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int e = blockIdx.x * 256 + 4 * lane;
  f32x4 t{0.f, 0.f, 0.f, 0.f};
  if (e < n) {
    int sidx = wv;
    for (; sidx + 28 < n_slots; sidx += 32) {
      f32x4 v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = *reinterpret_cast<const f32x4*>(ws + (size_t)(sidx + 4 * q) * n + e);
#pragma unroll
      for (int q = 0; q < 8; ++q) t += v[q];
    }
    for (; sidx < n_slots; sidx += 4) t += *reinterpret_cast<const f32x4*>(ws + (size_t)sidx * n + e);
  }
  s_part[wv][lane] = t;
  __syncthreads();
  if (wv == 0 && e < n) {
    f32x4* o = reinterpret_cast<f32x4*>(dW + e);
    *o = *o + (((s_part[0][lane] + s_part[1][lane]) + s_part[2][lane]) + s_part[3][lane]);
  }
}

// One instance of the streaming kernel; false where the pair has no instance of the asked form (4 x 4 exists in the Gram form only)
template <int MTN, int NTN>
static bool launch_narrow(const float* dz, const float* x, const float* x_scale, float* dW, int B, int Co, int Ci, int S,
                          const wg::WgPlan& p, int n_slots, hipStream_t s, WgTf tf) {
  if constexpr (MTN == NTN) {                                  // Gram matrix (dz == x, Co == Ci): the operand is loaded once
    if (p.gram) {
      hipLaunchKernelGGL((pw_wgrad_x3_narrow_kernel<MTN, NTN, true>), dim3(1, 1, p.nz), dim3(256), 0, s, dz, x, x_scale, dW, B,
                         Co, Ci, S, p.sps, p.upb, n_slots, tf, 0);
      return true;
    }
  }
  if constexpr (MTN * NTN < 16) {
    hipLaunchKernelGGL((pw_wgrad_x3_narrow_kernel<MTN, NTN, false>), dim3(p.mg, p.ng, p.nz), dim3(256), 0, s, dz, x, x_scale,
                       dW, B, Co, Ci, S, p.sps, p.upb, n_slots, tf, p.ps_spl);
    return true;
  }
  return false;
}

// One launch of pw_wgrad_wide_kernel: the kernel's arguments by name (what a launch does not use stays at its default)
struct WideArgs {
  const char* who;                       // entry point, for the error message
  hipStream_t stream;
  const float* dz; const float* x; const float* x_scale;
  float* out;                            // nz copies of dW (per-sample: see ps_ns)
  int B, Co, Ci, S, sps, upb; unsigned nz;
  wg::WideShape w;
  const float* radd = nullptr;           // RADD: additive constant per x row (centred Gram matrix)
  int same = 0;
  const float* tf_a = nullptr; const float* tf_b = nullptr; int tf_act = 0;   // PTF
  int ps_ns = 0;                         // per-sample launch: k-slices per sample
};
template <int NPROD, bool SWAP, bool SCALE, bool RADD, bool P16 = false, bool PTF = false>
static int launch_wide(const WideArgs& a) {
  auto kern = pw_wgrad_wide_kernel<NPROD, SWAP, SCALE, RADD, P16, PTF>;
  static bool attr_set = false;
  if (!attr_set) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, wg::wide_lds_limit) != hipSuccess)
      return eat::fail(EAT_ELAUNCH, "%s: hipFuncSetAttribute(160 KB of LDS) failed", a.who);
    attr_set = true;
  }
  hipLaunchKernelGGL(kern, dim3(a.w.ptn, a.w.qtn, a.nz), dim3(512), (size_t)wg::wide_lds_bytes(a.w), a.stream, a.dz, a.x,
                     a.x_scale, a.out, a.B, a.Co, a.Ci, a.S, a.sps, a.upb, a.w.ptr, a.w.qtr, a.radd, a.same, a.tf_a, a.tf_b,
                     a.tf_act, a.ps_ns);
  return EAT_OK;
}
// <SWAP, SCALE> from the run-time operand order and SE scale.  A bf16-stored dz as P (P16, not SWAP) has neither SE scale nor
// transform (the entry points refuse them): those instances do not exist
template <int NPROD, bool P16 = false, bool PTF = false>
static int launch_wide_sw_sc(const WideArgs& a) {
  if (a.w.swap) return a.x_scale ? launch_wide<NPROD, true, true, false, P16, PTF>(a) : launch_wide<NPROD, true, false, false, P16, PTF>(a);
  if constexpr (PTF) return eat::fail(EAT_EINVAL, "%s: internal: the on-load transform belongs to the x operand as P", a.who);
  else if constexpr (P16) return launch_wide<NPROD, false, false, false, true>(a);
  else return a.x_scale ? launch_wide<NPROD, false, true, false>(a) : launch_wide<NPROD, false, false, false>(a);
}

}  // namespace

static wg::WgReq wg_req(int B, int Co, int Ci, int S, bool per_sample, int exact_fp32, bool same, bool x_scale, wg::Xf xf,
                        int ws_slots) {
  wg::WgReq r{};
  r.B = B; r.Co = Co; r.Ci = Ci; r.S = S;
  r.per_sample = per_sample; r.arith = wg::arith_of(exact_fp32); r.same = same; r.x_scale = x_scale; r.xf = xf;
  r.ws_slots = ws_slots;
  return r;
}

static int pw_wgrad_impl(const float* dz, const float* x, const float* x_scale, float* dW, int B, int Co, int Ci, int S,
                         int per_sample, int exact_fp32, eat_stream_t stream, float* ws = nullptr, int n_slots = 0,
                         WgTf tf = WgTf{nullptr, nullptr, 0}) {
  // default: split-operand bf16 MFMA kernel (fp32-class accuracy); exact_fp32 (the caller's precision choice),
  // EAT_WGRAD_FP32=1 (process-wide debug override) or S % 4 != 0: exact fp32 MFMA kernel.
  // per-sample gradients (DyMN: K = one plane, B x Co x Ci outputs): the bf16x3 kernel with one block per (tile, sample)
  // and plain stores from Co, Ci >= 64 on.
  // ws / n_slots (zero-filled, n_slots * Co * Ci floats): the blocks' atomics go to copy blockIdx.z % n_slots and a
  // second kernel adds the copies into dW in a fixed order; n_slots >= eat_pw_wgrad_slots(...) gives every block its own
  // copy (bit-reproducible result).  The LDS-staged and exact kernels use the workspace only in that one-per-block form.
  // centring form of the Gram launches (eat_gram_centered): a = 1, b = actr = -mean, no activation - an additive row constant
  const wg::Xf xf = tf.a == nullptr ? wg::Xf::none : tf.actr != nullptr && tf.act == EAT_ACT_NONE ? wg::Xf::centre : wg::Xf::bn_act;
  // (a workspace pointer with no copy behind it is refused where the stored-slice kernel wants one: < 0, not "no workspace")
  const wg::Planned pl = wg::plan(wg_req(B, Co, Ci, S, per_sample != 0, exact_fp32, dz == x, x_scale != nullptr, xf,
                                         ws == nullptr ? 0 : n_slots != 0 ? n_slots : -1));
  if (pl.ws_short)
    return eat::fail(EAT_EINVAL, "eat_pw_conv_wgrad_ws: workspace of %d copies, the stored-slice kernel needs %u "
                     "(eat_pw_wgrad_slots)", n_slots, pl.wide_nz);
  const wg::WgPlan& p = pl.p;
  hipStream_t hs = (hipStream_t)stream;
  if (p.kind == 0) {
    const bool use_ws = ws != nullptr && n_slots > 1;
    float* target = use_ws ? ws : dW;
    const int slots = use_ws ? (n_slots < (int)p.nz ? n_slots : (int)p.nz) : 1;
    bool launched = false;
#define EAT_NARROW(M_, N_) if (p.mtb == M_ && p.ntb == N_) launched = launch_narrow<M_, N_>(dz, x, x_scale, target, B, Co, Ci, S, p, slots, hs, tf);
    EAT_WG_THIN_PAIRS(EAT_NARROW)
#undef EAT_NARROW
    if (!launched) return eat::fail(EAT_EINVAL, "eat_pw_conv_wgrad: internal: no streaming instance for %d x %d", p.mtb, p.ntb);
    if (use_ws)
      hipLaunchKernelGGL(wgrad_slot_reduce_kernel, dim3((Co * Ci + 63) / 64), dim3(256), 0, hs, ws, dW, Co * Ci, slots);
    return eat::check_launch("eat_pw_conv_wgrad");
  }
  const bool priv = ws != nullptr && !per_sample && n_slots >= (int)p.nz;     // one copy per block
  float* target = priv ? ws : dW;
  const int slots = priv ? (int)p.nz : 0;
  if (p.kind == 3) {
    WideArgs a{"eat_pw_conv_wgrad", hs, dz, x, x_scale, target, B, Co, Ci, S, p.sps, p.upb, p.nz, p.w};
    a.same = dz == x ? 1 : 0;
    int rc;
    if (xf == wg::Xf::centre) {                                // Gram matrices: P = x, no SE scale
      a.radd = tf.b;
      rc = exact_fp32 == 2 ? launch_wide<1, true, false, true>(a) : launch_wide<3, true, false, true>(a);
    } else {
      rc = exact_fp32 == 2 ? launch_wide_sw_sc<1>(a) : launch_wide_sw_sc<3>(a);
    }
    if (rc != EAT_OK) return rc;
  } else if (p.kind == 1) {
    dim3 grid((Co + 127) / 128, (Ci + 127) / 128, p.nz);
    if (exact_fp32 == 2)
      hipLaunchKernelGGL(pw_wgrad_x3_kernel<1>, grid, dim3(256), 0, hs, dz, x, x_scale, target, B, Co, Ci, S, p.sps, p.upb,
                         per_sample, tf, slots);
    else
      hipLaunchKernelGGL(pw_wgrad_x3_kernel<3>, grid, dim3(256), 0, hs, dz, x, x_scale, target, B, Co, Ci, S, p.sps, p.upb,
                         per_sample, tf, slots);
  } else {
    dim3 grid((Co + 31) / 32, (Ci + 31) / 32, p.nz);
    hipLaunchKernelGGL(pw_wgrad_kernel, grid, dim3(256), 0, hs, dz, x, x_scale, target, B, Co, Ci, S, p.bpb, per_sample, tf,
                       slots);
  }
  if (priv && p.kind == 3)
    hipLaunchKernelGGL(wgrad_slot_reduce4_kernel, dim3((Co * Ci + 255) / 256), dim3(256), 0, hs, ws, dW, Co * Ci, slots);
  else if (priv)
    hipLaunchKernelGGL(wgrad_slot_reduce_kernel, dim3((Co * Ci + 63) / 64), dim3(256), 0, hs, ws, dW, Co * Ci, slots);
  return eat::check_launch("eat_pw_conv_wgrad");
}

// Which kernel family eat_pw_conv_wgrad[_ws|_tf] launches for a shape when the caller brings the workspace the plan asks for
// (host helper for bench.py's byte models and the profiles): 0 = pw_wgrad_x3_narrow_kernel<mtb, ntb> (returned as
// 1000 * mtb + 10 * ntb + gram), 1 = pw_wgrad_x3_kernel, 2 = pw_wgrad_kernel (exact fp32), 3 = pw_wgrad_wide_kernel; encoded as
// kind + 10 * detail.
extern "C" int eat_pw_wgrad_kernel_kind(int B, int Co, int Ci, int S, int exact_fp32, int same, int has_scale, int has_tf) {
  const wg::WgPlan p = wg::plan(wg_req(B, Co, Ci, S, false, exact_fp32, same != 0, has_scale != 0,
                                       has_tf != 0 ? wg::Xf::bn_act : wg::Xf::none, wg::ws_enough)).p;
  return p.kind == 0 ? 10 * (1000 * p.mtb + 10 * p.ntb + (p.gram ? 1 : 0)) : p.kind;
}

// Number of workspace copies that gives every block of eat_pw_conv_wgrad_ws its own (bit-reproducible result); `same`: the
// two operands are the same tensor (Gram matrix).  Host helper.  It has no argument for an SE scale or an operand transform
// and assumes neither, and where the plan prefers the stored-slice kernel it answers for that kernel whether or not the rows
// of dW are 16-byte aligned: callers ask eat_pw_wgrad_kernel_kind first.
extern "C" int eat_pw_wgrad_slots(int B, int Co, int Ci, int S, int exact_fp32, int same) {
  const wg::Planned pl = wg::plan(wg_req(B, Co, Ci, S, false, exact_fp32, same != 0, false, wg::Xf::none, wg::ws_enough));
  return (int)(pl.wide_nz ? pl.wide_nz : pl.p.nz);
}

extern "C" int eat_pw_conv_wgrad(const float* dz, const float* x, const float* x_scale, float* dW, int B, int Co,
                                 int Ci, int S, int exact_fp32, eat_stream_t stream) {
  eat::clear_stale_error();
  return pw_wgrad_impl(dz, x, x_scale, dW, B, Co, Ci, S, 0, exact_fp32, stream);
}

// The same with a zero-filled workspace ws of n_slots * Co * Ci floats: the streaming kernel of the small matrices spreads
// its atomics over the slots (same-address atomics serialise in L2) and a second kernel adds the slots into dW.
// Matrices that do not run on that kernel ignore ws.
extern "C" int eat_pw_conv_wgrad_ws(const float* dz, const float* x, const float* x_scale, float* dW, float* ws,
                                    int n_slots, int B, int Co, int Ci, int S, int exact_fp32, eat_stream_t stream) {
  eat::clear_stale_error();
  return pw_wgrad_impl(dz, x, x_scale, dW, B, Co, Ci, S, 0, exact_fp32, stream, ws, n_slots);
}

// ... and with the x operand act(tf_a[ci] * x + tf_b[ci]) evaluated on load (x_scale multiplies the transformed value):
// the weight gradient of a project conv that was run by eat_pw_conv_tf_fwd.  ws / n_slots as above (may be NULL / 0).
extern "C" int eat_pw_conv_wgrad_tf(const float* dz, const float* x, const float* tf_a, const float* tf_b, int tf_act,
                                    const float* x_scale, float* dW, float* ws, int n_slots, int B, int Co, int Ci, int S,
                                    int exact_fp32, eat_stream_t stream) {
  eat::clear_stale_error();
  if (!tf_a || !tf_b) return eat::fail(EAT_EINVAL, "eat_pw_conv_wgrad_tf: tf_a and tf_b are required");
  if (tf_act < 0 || tf_act > 2) return eat::fail(EAT_EINVAL, "eat_pw_conv_wgrad_tf: bad act %d", tf_act);
  return pw_wgrad_impl(dz, x, x_scale, dW, B, Co, Ci, S, 0, exact_fp32, stream, ws, n_slots, WgTf{tf_a, tf_b, tf_act});
}

// ---- 1x1 weight gradient of the bf16-storage plan (act_io.h; BASELINE configs[2]): ONE of the operands - the wide tensor -
// is bf16 in HBM: x (the project conv's input y_d, or z_d with act(tf_a x + tf_b) evaluated on load, times x_scale) or dz (the
// expand conv's incoming gradient g).  Plain bf16 products, fp32 accumulation (what autocast does to the conv weight
// gradient, ex_pl_audioset.py:287-293).  Always the wide-tile producer / consumer kernel with the bf16 operand as P (its
// fragments need no conversion); ws: >= eat_pw_wgrad_b16_slots(...) * Co * Ci floats (no zero fill), dW is added to (zeroed by
// the caller).  S % 4 == 0, Ci % 4 == 0.
extern "C" int eat_pw_wgrad_b16_slots(int B, int Co, int Ci, int S, int x_b16) {
  return (int)wg::plan_b16(B, Co, Ci, S, x_b16).nz;
}

extern "C" int eat_pw_conv_wgrad_b16(const void* dz, int dz_b16, const void* x, int x_b16, const float* tf_a,
                                     const float* tf_b, int tf_act, const float* x_scale, float* dW, float* ws, int n_slots,
                                     int B, int Co, int Ci, int S, eat_stream_t stream) {
  eat::clear_stale_error();
  if (!dz || !x || !dW || !ws) return eat::fail(EAT_EINVAL, "eat_pw_conv_wgrad_b16: missing operand");
  if ((dz_b16 != 0) == (x_b16 != 0)) return eat::fail(EAT_EINVAL, "eat_pw_conv_wgrad_b16: exactly one of dz / x is the bf16 (wide) tensor");
  if (B < 1 || Co < 1 || Ci < 4 || (Ci & 3) != 0 || S < 4 || (S & 3) != 0)
    return eat::fail(EAT_EINVAL, "eat_pw_conv_wgrad_b16: Ci=%d and S=%d must be multiples of 4", Ci, S);
  if ((tf_a == nullptr) != (tf_b == nullptr) || tf_act < 0 || tf_act > 2) return eat::fail(EAT_EINVAL, "eat_pw_conv_wgrad_b16: bad transform");
  if (dz_b16 && (tf_a || x_scale)) return eat::fail(EAT_EINVAL, "eat_pw_conv_wgrad_b16: transform / scale belong to a bf16 x operand");
  const wg::WgB16Plan p = wg::plan_b16(B, Co, Ci, S, x_b16);
  if (!p.w.ok) return eat::fail(EAT_EINVAL, "eat_pw_conv_wgrad_b16: internal tiling error (%d x %d)", Co, Ci);
  if (n_slots < (int)p.nz) return eat::fail(EAT_EINVAL, "eat_pw_conv_wgrad_b16: workspace of %d copies, %u needed", n_slots, p.nz);
  if ((long long)(x_b16 ? Ci : Co) * S * 2 > 0x7fffffffLL || (long long)(x_b16 ? Co : Ci) * S * 4 > 0x7fffffffLL)
    return eat::fail(EAT_EINVAL, "eat_pw_conv_wgrad_b16: a sample exceeds the 32-bit row offsets");
  hipStream_t hs = (hipStream_t)stream;
  WideArgs a{"eat_pw_conv_wgrad_b16", hs, reinterpret_cast<const float*>(dz), reinterpret_cast<const float*>(x), x_scale, ws,
             B, Co, Ci, S, p.sps, p.upb, p.nz, p.w};
  a.tf_a = tf_a; a.tf_b = tf_b; a.tf_act = tf_act;
  const int rc = tf_a ? launch_wide_sw_sc<1, true, true>(a) : launch_wide_sw_sc<1, true>(a);
  if (rc != EAT_OK) return rc;
  hipLaunchKernelGGL(wgrad_slot_reduce4_kernel, dim3((Co * Ci + 255) / 256), dim3(256), 0, hs, ws, dW, Co * Ci, (int)p.nz);
  return eat::check_launch("eat_pw_conv_wgrad_b16");
}

// Per-sample weight gradients of a dynamic 1x1 conv under the bf16-storage plan (autograd of the grouped F.conv2d of
// models/dymn/dy_block.py:120-127): dW_b (B, Co, Ci) = dz[b] x[b]^T with exactly one bf16 operand (the wide tensor), plain bf16
// products, fp32 accumulation.  The wide-tile kernel of eat_pw_conv_wgrad_b16 with one k-slice per SAMPLE: slice b is stored as
// dW_b[b] - every element of dW_b is written, no zero fill, no reduction - or wg::dyn_b16_slices(...) k-slices per sample.
// S % 4 == 0, Ci % 4 == 0.
extern "C" int eat_pw_dyn_wgrad_b16_slices(int B, int Co, int Ci, int S, int x_b16) {
  const wg::WgB16Plan p = wg::plan_b16(B, Co, Ci, S, x_b16);
  return p.w.ok && (S & 3) == 0 && (Ci & 3) == 0 ? wg::dyn_b16_slices(p, B) : 0;   // (0: not on the wide-tile kernel)
}

extern "C" int eat_pw_conv_dyn_wgrad_b16(const void* dz, int dz_b16, const void* x, int x_b16, float* dW_b, int n_slices, int B,
                                         int Co, int Ci, int S, eat_stream_t stream) {
  eat::clear_stale_error();
  if (!dz || !x || !dW_b) return eat::fail(EAT_EINVAL, "eat_pw_conv_dyn_wgrad_b16: missing operand");
  if (dz_b16 && x_b16) return eat::fail(EAT_EINVAL, "eat_pw_conv_dyn_wgrad_b16: at most one of dz / x is a bf16 tensor");
  if (B < 1 || Co < 1 || Ci < 4 || (Ci & 3) != 0 || S < 4 || (S & 3) != 0)
    return eat::fail(EAT_EINVAL, "eat_pw_conv_dyn_wgrad_b16: Ci=%d and S=%d must be multiples of 4", Ci, S);
  const bool f32 = !dz_b16 && !x_b16;                                  // both fp32: split-operand (bf16x3) products
  const wg::WgB16Plan p = wg::plan_b16(B, Co, Ci, S, f32 ? 2 : x_b16);
  if (!p.w.ok) return eat::fail(EAT_EINVAL, "eat_pw_conv_dyn_wgrad_b16: internal tiling error (%d x %d)", Co, Ci);
  if ((long long)(Ci > Co ? Ci : Co) * S * 4 > 0x7fffffffLL)
    return eat::fail(EAT_EINVAL, "eat_pw_conv_dyn_wgrad_b16: a sample exceeds the 32-bit row offsets");
  const int ns = wg::dyn_b16_slices(p, B);
  if (n_slices < ns) return eat::fail(EAT_EINVAL, "eat_pw_conv_dyn_wgrad_b16: dW_b holds %d copies, %d needed (eat_pw_dyn_wgrad_b16_slices)", n_slices, ns);
  hipStream_t hs = (hipStream_t)stream;
  WideArgs a{"eat_pw_conv_dyn_wgrad_b16", hs, reinterpret_cast<const float*>(dz), reinterpret_cast<const float*>(x), nullptr,
             dW_b, B, Co, Ci, S, p.sps, (p.sps + ns - 1) / ns, (unsigned)(B * ns), p.w};   // ns k-slices per sample
  a.ps_ns = ns;
  const int rc = f32 ? launch_wide_sw_sc<3>(a) : launch_wide_sw_sc<1, true>(a);
  if (rc != EAT_OK) return rc;
  if (ns > 1) {                                                        // copy 0 (B, Co, Ci) += copies 1 .. ns - 1, fixed order
    const long long n = (long long)B * Co * Ci;
    if (n > 0x7fffffffLL) return eat::fail(EAT_EINVAL, "eat_pw_conv_dyn_wgrad_b16: B*Co*Ci exceeds the 32-bit index of the slice reduction");
    hipLaunchKernelGGL(wgrad_slot_reduce4_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, hs, dW_b + n, dW_b, (int)n, ns - 1);
  }
  return eat::check_launch("eat_pw_conv_dyn_wgrad_b16");
}

// 1 where eat_pw_conv_dyn_wgrad adds into dW_b (the caller zero-fills it), 0 where it stores.  Host helper.  (The plan of ONE
// sample: the batch size moves only the streaming kernel's blocks per sample, never the choice of kernel.)
extern "C" int eat_pw_dyn_wgrad_accumulates(int Co, int Ci, int S) {
  return wg::plan(wg_req(1, Co, Ci, S, true, 0, false, false, wg::Xf::none, 0)).p.kind == 1 ? 0 : 1;
}

// Centred Gram matrix Gc = sum (x - m)(x - m)^T, m = sx * inv_n (see include/eat_hip.h): both operands are centred on
// load (operand transform a = 1, b = -m on the x side, additive row constant -m on the dz side; elements beyond the k
// range stay zero).
namespace {
__global__ void gram_center_coef_kernel(const float* __restrict__ sx, float inv_n, float* __restrict__ ab, int C) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < C) { ab[c] = 1.0f; ab[C + c] = -sx[c] * inv_n; }
}
}  // namespace
extern "C" int eat_gram_centered(const float* x, const float* sx, float inv_n, float* G, float* ws, int n_slots, int B, int C,
                                 int S, int exact_fp32, eat_stream_t stream) {
  eat::clear_stale_error();
  if (!x || !sx || !G || !ws || n_slots < 1) return eat::fail(EAT_EINVAL, "eat_gram_centered: missing operand (ws holds the (1, -m) coefficients first)");
  // ws: [2 C floats of transform coefficients][n_slots copies of G]
  float* ab = ws;
  hipLaunchKernelGGL(gram_center_coef_kernel, dim3((C + 255) / 256), dim3(256), 0, (hipStream_t)stream, sx, inv_n, ab, C);
  return pw_wgrad_impl(x, x, nullptr, G, B, C, C, S, 0, exact_fp32, stream, ws + 2 * (size_t)C, n_slots,
                       WgTf{ab, ab + C, EAT_ACT_NONE, ab + C});
}

extern "C" int eat_pw_conv_dyn_wgrad(const float* dz, const float* x, float* dW_b, int B, int Co, int Ci, int S,
                                     eat_stream_t stream) {
  eat::clear_stale_error();
  return pw_wgrad_impl(dz, x, nullptr, dW_b, B, Co, Ci, S, 1, 0, stream);
}
