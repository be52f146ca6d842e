// Launch plan of the 1x1 (pointwise) weight-gradient and Gram kernels of train.hip: which kernel, how the output is tiled and
// how the k range (b, s) is cut.  Pure integer arithmetic on the host: no HIP, no eat_common.h - tests/wgrad_plan_check.cpp
// builds it with a host compiler alone.  train.hip asks plan() once per launch and once per sizing helper.
#pragma once
#include <climits>
#include <cstdlib>

namespace eat {
namespace wg {

// ---- the request ------------------------------------------------------------------------------------------------------
enum class Arith { bf16x3 = 0, fp32 = 1, bf16 = 2 };   // split-operand bf16 (fp32-class), exact fp32 MFMA, plain bf16 products
// transform of the x operand on load: none, act(a[ci] x + b[ci]) (the project conv's BatchNorm + activation), or the centring
// of both operands of a Gram matrix (eat_gram_centered; on distinct operands it plans like bn_act - no entry point asks that)
enum class Xf { none, bn_act, centre };
inline Arith arith_of(int exact_fp32) { return exact_fp32 == 1 ? Arith::fp32 : exact_fp32 == 2 ? Arith::bf16 : Arith::bf16x3; }

constexpr int ws_enough = INT_MAX;   // ws_slots of a caller that will bring as many copies as the plan asks for
struct WgReq {
  int B, Co, Ci, S;
  bool per_sample;     // B matrices dW_b (DyMN) instead of their sum
  Arith arith;
  bool same;           // dz == x (Gram matrix)
  bool x_scale;        // the SE scale multiplies x
  Xf xf;
  int ws_slots;        // copies of dW in the caller's workspace; 0 = no workspace (< 0: a workspace without a copy)
};

// EAT_WGRAD_FP32=1: process-wide debug override, every request plans as Arith::fp32
inline bool env_fp32() {
  static const bool on = getenv("EAT_WGRAD_FP32") && atoi(getenv("EAT_WGRAD_FP32")) != 0;
  return on;
}

// ---- the streaming kernel's instances -----------------------------------------------------------------------------------
// (row tiles of dz, row tiles of x) per block that pw_wgrad_x3_narrow_kernel is instantiated for: the x side carries the SE
// scale / BatchNorm transform and costs more registers per tile (<= 3 tiles there, <= 4 on the dz side); 1 x 4 for a single-
// tile dz against <= 64 channels; 4 x 4 in the Gram form only (the operand is loaded once);
// plus 5 x 2 / 2 x 5: 72 x 24 and 24 x 72 as ONE row group (both operands read once, no zero tiles)
#define EAT_WG_THIN_PAIRS(X)                                                                                              \
  X(1, 1) X(1, 2) X(1, 3) X(1, 4) X(2, 1) X(3, 1) X(4, 1) X(2, 2) X(3, 3) X(4, 4) X(2, 3) X(3, 2) X(4, 2) X(4, 3) X(5, 2) X(2, 5)
constexpr bool thin_pair(int m, int n) {
#define EAT_WG_IS(M_, N_) (m == M_ && n == N_) ||
  return EAT_WG_THIN_PAIRS(EAT_WG_IS) false;
#undef EAT_WG_IS
}

// ---- shared arithmetic --------------------------------------------------------------------------------------------------
// Tiles of the wide-tile kernel over a (PR rows of P) x (QR rows of Q) matrix: a block owns <= 256 rows of P and <= 160 rows of
// Q (4 producers x 5 pieces of 8 rows), both cut evenly and rounded up to MFMA tiles of 16.
// (tile limits measured: P <= 192 / 128 rows per block instead of 256: 672 x 112 147 -> 157 / 198 us, mn10 step +0.3 ms)
struct WideShape { bool ok; bool swap; int ptr, qtr, ptn, qtn; };     // swap: P = x (else dz); tile rows, tile counts
inline WideShape wide_tiles(int PR, int QR) {
  WideShape w{false, false, 0, 0, 0, 0};
  w.ptn = (PR + 255) / 256;
  w.ptr = ((PR + w.ptn - 1) / w.ptn + 15) / 16 * 16;
  w.qtn = (QR + 159) / 160;
  w.qtr = ((QR + w.qtn - 1) / w.qtn + 15) / 16 * 16;
  w.ok = (w.ptn - 1) * w.ptr < PR && (w.qtn - 1) * w.qtr < QR;
  return w;
}
constexpr int wide_lds_limit = 160 * 1024;                           // what the launcher asks hipFuncSetAttribute for
inline int wide_lds_bytes(const WideShape& w) { return (w.ptr / 8 + w.qtr / 8) * 2 * 1024; }   // two slots of converted fragments

// Cut `total` k units (32 positions each) so that `tiles` output tiles give about `target` blocks - never more - with at
// least 16 units (512 k) of MFMA work in front of a block's stores or atomics
struct KSplit { int upb; unsigned nz; };                              // units per block, blocks along k
inline KSplit k_split(long long total, int tiles, int target) {
  long long splits = tiles >= target ? 1 : target / tiles;
  if (splits > total / 16) splits = total / 16;
  if (splits < 1) splits = 1;
  KSplit k;
  k.upb = (int)((total + splits - 1) / splits);
  k.nz = (unsigned)((total + k.upb - 1) / k.upb);
  return k;
}

// ---- the fp32-storage plan ----------------------------------------------------------------------------------------------
// kind: 0 LDS-free streaming kernel (thin matrices), 1 LDS-staged x3, 2 exact fp32, 3 wide-tile LDS ring (pw_wgrad_wide_kernel);
// upb / nz: k units per block, blocks along k (sps units per sample); bpb: samples per block of kind 2;
// mtb / ntb: row tiles per block, mg / ng groups of kind 0; ps_spl: its blocks per sample (per-sample mode); w: tiles of kind 3
struct WgPlan { int kind; int upb; unsigned nz; int sps; int bpb; int mtb, ntb, mg, ng; bool gram; int ps_spl; WideShape w; };

// Tile shape of the wide-tile kernel for a (Co, Ci) matrix, and whether the plan uses it.
// Measured (tools/bench_kernels.py wgrad): the producers' fixed cost per unit (13 load instructions, one barrier) loses on
// tiles of fewer than ~20 pieces (160 rows of P + Q), and the on-load transform makes the producers the pole.
inline WideShape wide_shape(const WgReq& r) {
  constexpr int wide_min = 20;
  const bool has_tf = r.xf == Xf::bn_act || (r.xf == Xf::centre && !r.same);
  WideShape none{false, r.Ci > r.Co, 0, 0, 0, 0};
  if (r.per_sample || has_tf || (r.x_scale && (r.Ci & 3) != 0)) return none;
  if (r.same) {
    // Gram matrix (dz == x, train_fuse.hip): ONE operand, loaded once - P = x, the Q fragments are read from P's rows.  Above
    // the streaming kernel's range (C > 64) up to what one consumer quartet holds (10 column tiles: ONE tile of P and Q);
    // 80 x 80 at 504 positions x 256 clips: 62 us on the 128 x 128-tile kernel for 41 MB of input
    if (r.Co != r.Ci || r.Co <= 64 || r.Co > 160 || r.x_scale) return none;
    WideShape w = wide_tiles(r.Co, r.Co);
    w.swap = true;
    return w;
  }
  // (384 blocks instead of one per CU: +0.3 ms; minimum of 14 / 30 pieces instead of 20: +0.1 ms per mn10 step)
  WideShape w = none.swap ? wide_tiles(r.Ci, r.Co) : wide_tiles(r.Co, r.Ci);
  w.swap = none.swap;
  w.ok = w.ok && w.ptr / 8 + w.qtr / 8 >= wide_min;
  return w;
}

inline WgPlan plan_with(const WgReq& r, bool allow_wide) {
  const int B = r.B, Co = r.Co, Ci = r.Ci, S = r.S;
  const bool per_sample = r.per_sample;
  const bool force_fp32 = env_fp32() || r.arith == Arith::fp32;
  const bool ps_x3 = per_sample && Co >= 64 && Ci >= 64;
  const WideShape wide = allow_wide ? wide_shape(r) : WideShape{false, Ci > Co, 0, 0, 0, 0};
  WgPlan p{2, 0, 0, (S + 31) / 32, 0, 0, 0, 1, 1, false, 0, WideShape{false, false, 0, 0, 0, 0}};
  const int sps = p.sps;
  const int mtn = (Co + 15) / 16, ntn = (Ci + 15) / 16;
  if (!force_fp32 && (S & 3) == 0 && per_sample && !ps_x3 && sps >= 32) {
    // per-sample gradients of the thin early-layer matrices (one side < 64 channels, planes of >= 1024 positions):
    // the same streaming kernel, a few blocks per sample adding into the sample's own matrix
    const int mg = (mtn + 3) / 4, ng = (ntn + 2) / 3;
    const int mtb = (mtn + mg - 1) / mg, ntb = (ntn + ng - 1) / ng;
    if (mg * ng <= 4 && thin_pair(mtb, ntb)) {
      int spl = 1024 / (mg * ng * B);
      if (spl > sps / 16) spl = sps / 16;
      if (spl < 1) spl = 1;
      p.kind = 0; p.mtb = mtb; p.ntb = ntb; p.mg = mg; p.ng = ng;
      p.upb = (sps + spl - 1) / spl;
      p.ps_spl = (sps + p.upb - 1) / p.upb;
      p.nz = (unsigned)(B * p.ps_spl);
      return p;
    }
  }
  if (!force_fp32 && (!per_sample || ps_x3) && (S & 3) == 0) {
    const long long total = (long long)B * sps;
    // (a centring transform keeps the Gram plan: both operands are the same centred rows)
    const bool gram = r.same && Co == Ci && !r.x_scale && r.xf != Xf::bn_act;
    bool thin = false;
    if (!per_sample) {
      if (gram && Co <= 64) {                                  // Gram matrix: the operand is loaded once
        thin = true; p.mtb = p.ntb = mtn; p.mg = p.ng = 1; p.gram = true;
      } else if (Co <= 64 && Ci <= 64 && (Co <= 16 || Ci <= 16)) {
        thin = true; p.mtb = mtn; p.ntb = ntn; p.mg = p.ng = 1;
      } else {
        // few rows over a long k axis: groups of <= 4 x 3 row tiles per block, at most 4 groups (the other operand is re-read
        // once per group, from L2); 72 x 24 / 24 x 72 as one 5 x 2 / 2 x 5 group (both operands read once, no zero tiles:
        // measured faster at B = 256, profiles/thin_wgrad_before_after.md).  "Long": each of a row group's 1024 / groups
        // blocks gets >= 512 k positions (16 units, 4 per wave) to stream in front of its tile's atomics.
        const bool one52 = (mtn == 5 && ntn == 2) || (mtn == 2 && ntn == 5);
        const int mg = one52 ? 1 : (mtn + 3) / 4, ng = one52 ? 1 : (ntn + 2) / 3;
        const int mtb = (mtn + mg - 1) / mg, ntb = (ntn + ng - 1) / ng;
        if (mg * ng <= 4 && thin_pair(mtb, ntb) && total * 32 * (mg * ng) >= (1 << 19)) {
          thin = true; p.mtb = mtb; p.ntb = ntb; p.mg = mg; p.ng = ng;
        }
        // more than one row group = the other operand is read once per group: the wide-tile kernel reads it once
        if (thin && mg * ng > 1 && wide.ok) thin = false;
      }
    }
    if (thin) {
      const long long splits = (1024 / (p.mg * p.ng)) < total ? (1024 / (p.mg * p.ng)) : total;
      p.kind = 0;
      p.upb = (int)((total + splits - 1) / splits);
      p.nz = (unsigned)((total + p.upb - 1) / p.upb);
      return p;
    }
    if (wide.ok) {
      const KSplit k = k_split(total, wide.ptn * wide.qtn, 256);     // one block per CU
      p.kind = 3; p.w = wide; p.upb = k.upb; p.nz = k.nz;
      return p;
    }
    p.kind = 1;
    p.upb = sps;                                             // per-sample gradients: one sample per block
    if (!per_sample) {
      // ~512 blocks (512 = one round of two resident blocks per CU; 1024 measured 0.26 ms slower per mn10 step: the second
      // round pays prologue, tail and the Co x Ci atomics again), never MORE: 516 blocks (6 tiles x 86 slices, the 672 x 112
      // layers) ran as a full round of 512 resident blocks plus a second round of 4 (183 -> 158 us with 510)
      p.upb = k_split(total, ((Co + 127) / 128) * ((Ci + 127) / 128), 512).upb;
    }
    p.nz = (unsigned)((total + p.upb - 1) / p.upb);
    return p;
  }
  const int tiles = ((Co + 31) / 32) * ((Ci + 31) / 32);
  int splits = (1024 + tiles - 1) / tiles;
  if (splits > B || per_sample) splits = B;
  p.bpb = (B + splits - 1) / splits;
  p.nz = (unsigned)((B + p.bpb - 1) / p.bpb);
  return p;
}

// The plan the launch uses.  The wide-tile kernel stores one copy of dW per k-slice: it needs a workspace of >= nz copies and
// 16-byte aligned rows of dW (Ci % 4 == 0); without them the plan is the one without that kernel.  A caller that DID bring a
// workspace sized it with the helpers and - for this kernel - left it uninitialised: too few copies there would let the
// atomic kernels of the fallback plan add into garbage, so that is an error (ws_short), not a fallback.
// wide_nz: k-slices of the wide-tile kernel where the plan prefers it, taken or not (0: it does not).
struct Planned { WgPlan p; unsigned wide_nz; bool ws_short; };
inline Planned plan(const WgReq& r) {
  Planned o{plan_with(r, true), 0, false};
  if (o.p.kind != 3) return o;
  o.wide_nz = o.p.nz;
  const bool rows16 = (r.Ci & 3) == 0;
  if (rows16 && r.ws_slots >= (int)o.wide_nz) return o;
  o.ws_short = rows16 && r.ws_slots != 0;
  o.p = plan_with(r, false);
  return o;
}

// ---- the bf16-storage plan (eat_pw_conv_wgrad_b16, eat_pw_conv_dyn_wgrad_b16): always the wide-tile kernel ----------------
// x_b16: 1 = x is the bf16 (wide) operand, 0 = dz is; 2 = BOTH operands fp32 (the per-sample gradients of the fp32-storage
// DyMN plan on the same kernel, split-operand products): P = the operand with more rows
struct WgB16Plan { WideShape w; int upb; unsigned nz; int sps; };
inline WgB16Plan plan_b16(int B, int Co, int Ci, int S, int x_b16) {
  WgB16Plan p{};
  p.sps = (S + 31) / 32;
  const bool swap = x_b16 == 2 ? Ci > Co : x_b16 != 0;
  p.w = swap ? wide_tiles(Ci, Co) : wide_tiles(Co, Ci);
  p.w.swap = swap;
  const KSplit k = k_split((long long)B * p.sps, p.w.ptn * p.w.qtn, 256);   // one block per CU
  p.upb = k.upb; p.nz = k.nz;
  return p;
}

// k-slices per sample of the per-sample launch: a sample's reduction is cut into several blocks where B x (tiles of dW) alone
// would leave CUs idle - the early layers (thin matrices, planes of thousands of positions: 128 one-tile blocks walking 1000
// units each ran at 1.9 TB/s)
inline int dyn_b16_slices(const WgB16Plan& p, int B) {
  const long long blocks = (long long)p.w.ptn * p.w.qtn * B;
  int ns = 1;
  while (ns < 8 && blocks * ns < 1024 && p.sps / (2 * ns) >= 8) ns *= 2;
  while (ns > 1 && (ns - 1) * ((p.sps + ns - 1) / ns) >= p.sps) --ns;    // every slice must own at least one unit
  return ns;
}

}  // namespace wg
}  // namespace eat
