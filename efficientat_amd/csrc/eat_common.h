// Shared helpers for the gfx950 kernels of libeat_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>

#include "../../include/eat_hip.h"
#include "pw_fwd_plan.h"

namespace eat {

// thread-local last-error text behind eat_last_error_string()
char* err_buf();
int fail(int code, const char* fmt, ...);

// hipGetLastError is sticky per thread: drop whatever an earlier, unrelated runtime call left behind
inline void clear_stale_error() { (void)hipGetLastError(); }

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(EAT_ELAUNCH, "%s: %s", what, hipGetErrorString(e));
  return EAT_OK;
}

template <int ACT>
__device__ __forceinline__ float activate(float v) {
  if constexpr (ACT == EAT_ACT_RELU) return fmaxf(v, 0.0f);
  if constexpr (ACT == EAT_ACT_HSWISH) return v * fminf(fmaxf(v + 3.0f, 0.0f), 6.0f) * (1.0f / 6.0f);
  return v;
}

__device__ __forceinline__ float activate_rt(float v, int act) {
  if (act == EAT_ACT_RELU) return fmaxf(v, 0.0f);
  if (act == EAT_ACT_HSWISH) return v * fminf(fmaxf(v + 3.0f, 0.0f), 6.0f) * (1.0f / 6.0f);
  return v;
}

// 64-lane wavefront sum (all lanes receive the total)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

constexpr int kWave = 64;

// A value the optimiser cannot see through (no instruction is emitted).  Used for 0 / 1 validity factors: LLVM rewrites
// `x * (cond ? 1 : 0)` into `cond ? x : 0` and then sinks the loads x depends on into an exec-masked block with its own
// s_waitcnt - one exposed memory latency per element instead of one per batch of loads.
// (not `volatile`: a volatile asm is a scheduling boundary and would itself keep loads from being batched)
__device__ __forceinline__ float opaque(float v) {
  asm("" : "+v"(v));
  return v;
}
__device__ __forceinline__ float opaque_uniform(float v) {       // wave-uniform value, stays in a scalar register
  asm("" : "+s"(v));
  return v;
}

// Training epilogues of the register-resident depthwise kernels (dw_plane.hip), all optional:
//   stats   forward: per-wave partial sums of the conv output, floats [b][2][C][inner] (sum, sum of squares) - the
//           BatchNorm batch statistics without a separate pass over the tensor (eat_bn_finalize_partials reduces them);
//   gz/ga/gb/gact/gpart   data gradient: the output dx is multiplied by act'(ga[c] * gz + gb[c]) (gz: the pre-BN tensor
//           of the layer below, same shape as dx) and summed per wave into gpart [b][C][inner];
//   inner   (host pointer) receives the number of partial slots per plane of the kernel that ran.
struct DwEpi {
  float* stats;
  const float* gz; const float* ga; const float* gb; int gact; float* gpart;
  int* inner;
};

// conv_spatial.hip: stride-1 depthwise data gradient on the forward sliding-window kernel
// (epi with gz: the training epilogue; returns 1 when no register-resident kernel covers the geometry)
int dw_conv_dgrad_s1(const float* dz, const float* w, const float* zero_bias, const float* res, float* dx, int B, int C,
                     int F, int T, int k, int per_plane_w, hipStream_t s, const DwEpi* epi = nullptr);

// train_fuse.hip: generic (any geometry) forms of the two training epilogues, one block per plane, inner = 1
int bn_stats_partial(const float* z, int B, int C, int S, float* part, hipStream_t s);
int act_grad_sum(const float* dy, const float* z, const float* a, const float* b, int act, float* g, float* gpart, int B,
                 int C, int S, hipStream_t s);

// BatchNorm-backward statistics in a 1x1 conv's epilogue (pw_epilogue.h: pw_epilogue_gstats): z = the tensor whose
// BatchNorm + activation backward is being reduced (layout of the conv output), a / b = that BatchNorm's folded affine
struct PwGStat { const void* z; const float* a; const float* b; int act; };
// centring constant of the BatchNorm-backward partials of pw_epilogue_gstats (pw_epilogue.h) and of bn_bwd_sums_finish_kernel
// (train_fuse.hip), from the BatchNorm's (a, b): the zero of the pre-activation.  ONE expression, so that the epilogue subtracts
// and the finish adds back the same fp32 number.
__host__ __device__ __forceinline__ float gstat_center(float a, float b) { return a != 0.0f ? -b / a : 0.0f; }

// ---- dw_plane.hip: the register-resident depthwise kernels.  Each dispatcher takes one request, filled by field name
// (value-initialise it: every optional field is then NULL / 0), and returns 1 when no kernel covers it: the caller falls back.
struct DwGeom { int B, C, F, T, Fo, To, k, stride; };      // conv input planes (F, T), output planes (Fo, To)
// optional transform of the conv INPUT, evaluated once per loaded element: act(a[c] * x + b[c]); a == NULL: none
struct InTf { const float* a; const float* b; int act; };
// storage of the WIDE tensors in HBM (act_io.h) - x, y of the forward; dz, bn->z, x, g of the backward, void* in the requests:
// all fp32 / all bf16 (the statistics forward and the BatchNorm-on-load backward instances only) / bf16 with the conv INPUT
// side (x; g of the backward) fp32: a block without expand conv.  Narrow operands are always fp32.
enum DwStore { kDwF32 = 0, kDwB16 = 1, kDwB16XF32 = 2 };

struct DwFwdReq {
  DwGeom dim; const void* x; const float* w; const float* bias; const float* res; void* y; float* pool;
  int act, flip, per_plane_w; InTf tf; const DwEpi* epi; DwStore store; hipStream_t stream;
};
int dw_plane_try(const DwFwdReq& r);
struct DwWgradReq { DwGeom dim; const float* dz; const float* x; float* dw; int per_plane; InTf tf; hipStream_t stream; };
// Where the batch picks the decomposition of the weight-gradient kernels: which kernel runs and its split.  The launchers
// take their split from these plans and eat_dw_wgrad_split (eat_hip.h) answers from them - one copy of the arithmetic.
enum DwWgradKernel { kDwWgPlane = 0, kDwWgTile = 1, kDwWgColumn = 2, kDwWgStem = 3, kDwWgChannel = 4 };
struct DwWgradPlan {
  int kernel;                    // DwWgradKernel
  int inst, npw;                 // whole-plane: which of the five instances, samples side by side in a wave (else npw = 1)
  int n_rc, n_cs, WO;            // tile: row chunks, column strips and strip width of a plane
  int G; long long waves;        // whole-plane, tile: samples a lane group walks, waves launched
  int TX, ct;                    // column-walking: columns per block, column tiles
  int bpb, slices;               // column-walking, per-channel: samples per block, batch slices
  int rpb, chunks;               // stem: output rows per block, row chunks
};
int dw_plane_wgrad_plan(const DwGeom& d, bool per_plane, DwWgradPlan* p);     // 1: no register-resident instance
int dw_plane_wgrad_run(const DwWgradReq& r, const DwWgradPlan& p);            // p: dw_plane_wgrad_plan's answer for r
// merged depthwise backward: weight gradient + data gradient + activation-derivative epilogue in one pass
// bn != NULL: dz is the gradient w.r.t. the activated BatchNorm output of this conv; the BatchNorm + activation backward is
// evaluated on load from (dz, bn->z) with the channel sums of the reduce pass (sums[0..C) = sum g, [C..2C) = sum g xhat)
struct DwBnBwd {
  const void* z; const float* a; const float* b; const float* mean; const float* invstd;
  const float* gscale; const float* gadd; const double* sums; int act; int frozen;
};
struct DwBwdReq {
  DwGeom dim; const void* dz; const void* x; InTf tf; const float* w; void* g; float* dw; float* gpart; int* h_inner;
  const DwBnBwd* bn; int per_plane_w;
  const float* res;      // per_plane_w: added to g after the partial sums are taken, or NULL
  float* gzpart;         // per_plane_w: per-tile sums of g * x, layout of gpart, or NULL
  DwStore store; hipStream_t stream;
};
int dw_bwd_try(const DwBwdReq& r);
// the merged kernel's split of a geometry (bn: the BatchNorm-on-load instances): lane-group width, whole rows or column
// strips, rows per tile, tiles of a plane and G = the groups of 64 / lpp samples a wave walks.  dw_bwd_try launches what this
// answers and eat_dw_bwd_split (eat_hip.h) reports it.  1: not on the merged kernel.
struct DwBwdPlan { int lpp, wr, ro, n_rc, n_cs, WO, G; long long waves; };
int dw_bwd_plan(const DwGeom& d, bool bn, DwBwdPlan* p);
// stride-2 data gradient on tiles (dim.stride is 2; epi with gz: the training epilogue)
struct DwDgrad2Req {
  DwGeom dim; const float* dz; const float* w; const float* res; float* dx; int per_plane_w; const DwEpi* epi; hipStream_t stream;
};
int dw_tile_dgrad2_try(const DwDgrad2Req& r);

// ---- the forward 1x1 (pointwise) convolutions: every entry point fills one request by field name (value-initialise it: every
// optional field is then NULL / 0) and hands it to pw_conv_run, which checks it, asks pw_fwd_plan.h for the route and launches.
struct PwFwdReq {
  int B, Ci, Co, S;                          // Ci: the whole reduction axis (both sources / every bank)
  const void* x; pw::Store x_store;
  const float* x2; int c1;                   // two-source form: x has c1 channels, x2 (fp32) the other Ci - c1; NULL: one source
  int ci_x;                                  // K-concat form: channels of x, the reduction axis is Ci / ci_x copies; 0: plain
  const void* wp; pw::Pack pack; bool per_sample;
  const float* bias;
  InTf tf;                                   // act(a[k] * x + b[k]) evaluated on load; a == NULL: none
  const float* in_scale; const float* res;
  void* y; pw::Store y_store;
  float* pool; int act;
  float* stats; PwGStat gs;                  // [tile][2][Co] partials of the statistics epilogue; gs.z: its BatchNorm-backward form
  hipStream_t stream;
  const char* who;                           // the entry point, for messages
};
// conv_pw.hip: check -> plan -> launch; 1 = no kernel with the statistics epilogue for this geometry, nothing launched
int pw_conv_run(const PwFwdReq& r);
// one launcher per file: the template switch over the plan (conv_pw.hip, conv_pw_bf16.hip, conv_pw_stream.hip: expand and
// K-streaming kernels, conv_pw_generic.hip)
int pw_lds_f32_launch(const PwFwdReq& r, const pw::PwPlan& p);
int pw_lds_b16_launch(const PwFwdReq& r, const pw::PwPlan& p);
int pw_stream_launch(const PwFwdReq& r, const pw::PwPlan& p);
int pw_generic_launch(const PwFwdReq& r, const pw::PwPlan& p);

}  // namespace eat

#define EAT_DISPATCH_ACT(act, ...)                                    \
  do {                                                                \
    if ((act) == EAT_ACT_NONE) { constexpr int ACT = EAT_ACT_NONE; __VA_ARGS__; }        \
    else if ((act) == EAT_ACT_RELU) { constexpr int ACT = EAT_ACT_RELU; __VA_ARGS__; }   \
    else { constexpr int ACT = EAT_ACT_HSWISH; __VA_ARGS__; }                            \
  } while (0)
