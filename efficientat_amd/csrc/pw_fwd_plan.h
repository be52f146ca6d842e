// Route and launch plan of the forward 1x1 (pointwise) convolutions: which of the kernels of conv_pw.hip, conv_pw_bf16.hip,
// conv_pw_stream.hip and conv_pw_generic.hip a request runs on, how the output is tiled and how much LDS the launch takes.
// Pure integer arithmetic on the host: no HIP, no eat_common.h - tests/pw_fwd_plan_check.cpp builds it with a host compiler
// alone.  eat::pw_conv_run (conv_pw.hip) asks check() and plan() once per call; every entry point goes through it.
#pragma once

namespace eat {
namespace pw {

// ---- the request, as far as the route depends on it (eat::PwFwdReq in eat_common.h carries the pointers) ---------------------
enum class Store { f32 = 0, b16 = 1 };                 // storage of x / y in HBM (act_io.h)
enum class Pack { f32 = 0, b16 = 1, b16x2 = 2 };       // eat_pw_prepack / eat_pw_prepack_bf16 plain / hi + lo: the entry points' wmode
inline Pack pack_of(int wmode) { return wmode == 0 ? Pack::f32 : wmode == 2 ? Pack::b16x2 : Pack::b16; }

struct PwKey {
  int B, Ci, Co, S;
  int ci_x;                    // channels of x; < Ci: the reduction axis is Ci / ci_x copies of them ("K-concat", DyMN)
  int c1;                      // two-source form: channels of x, x2 carries the other Ci - c1; 0 = one source
  Store x_store, y_store;
  Pack pack;
  bool per_sample;             // one weight pack per sample: column tiles lie inside samples
  bool operands;               // x, wp and bias are there
  bool y, scale, res, pool;    // which optional operands are there
  bool tf, tf_half;            // on-load transform: both of (a, b) / exactly one of them
  bool stats, gstat;           // statistics epilogue; its BatchNorm-backward form
  int act, tf_act, gs_act;
};

// EAT_PW_STREAM / eat_pw_stream_mode bits: which launches leave the LDS-staged bf16 kernel for conv_pw_stream.hip
enum StreamMode { kStreamExpand = 1, kStreamProject = 2, kStreamRest = 4, kStreamKcat = 8 };

enum class Route {
  none,        // no kernel with the statistics epilogue for this geometry: nothing is launched, the entry point answers 1
  generic,     // pw_conv_generic_kernel: plane sizes that are no multiple of 4
  lds_f32,     // pw_conv_kernel: fp32 MFMA, operands staged in LDS
  lds_b16,     // pw_conv_bf16_kernel: bf16 MFMA, operands staged in LDS
  expand,      // pw_expand_kernel: x resident in registers, output rows streamed
  kstream      // pw_kstream_kernel: output tile resident, K streamed
};

constexpr int kTileN = 256;      // columns per block
constexpr int kKC = 32;          // max k rows per LDS stage (fp32 kernel); k rows per chunk (bf16 kernels)
constexpr int kPipeKC = 16;      // k rows per chunk of the pipelined fp32 kernel
constexpr int kLdsLimit = 160 * 1024;
constexpr long long kMaxColumns = 0x7fff0000LL;      // B * S the 32-bit column index of the bf16 kernels reaches

// LDS stage of the fp32 kernel = [A: (kc/4)*MTW fragment rows of 64 floats, padded to 256][X: kc rows x 256][scale: kc x NS]
// (the kernel walks the stage with its own copy of these two expressions, conv_pw.hip)
constexpr int a_stage_floats(int mtw, int kc) { return (((kc >> 2) * mtw * 64) + 255) & ~255; }
constexpr int stage_floats(int mtw, int kc, int ns) { return a_stage_floats(mtw, kc) + kc * kTileN + ((kc * ns + 3) & ~3); }

// column tiles = [tile][2][Co] partials of the statistics epilogue (eat_pw_conv_stat_tiles)
inline int stat_tiles(int B, int S, bool per_sample) {
  return per_sample ? B * ((S + kTileN - 1) / kTileN) : (int)(((long long)B * S + kTileN - 1) / kTileN);
}

// ---- the argument rules, once ----------------------------------------------------------------------------------------------
// NULL = the request is valid; otherwise what is wrong with it (the caller adds the entry point's name and the values)
inline const char* check(const PwKey& k) {
  if (!k.operands) return "x, wp and bias are required";
  if (!k.y && !k.pool) return "y or pool is required";
  if (k.B < 1 || k.Ci < 4 || k.Co < 1 || k.S < 1) return "bad shape";
  if (k.Ci % 4 != 0) return "Ci must be a multiple of 4";
  if (k.act < 0 || k.act > 2 || k.tf_act < 0 || k.tf_act > 2 || k.gs_act < 0 || k.gs_act > 2) return "bad activation code";
  if (k.tf_half) return "tf_a and tf_b go together";
  if (k.tf && k.Ci % 8 != 0) return "the on-load transform needs Ci % 8 == 0";
  if (k.gstat && !k.stats) return "the BatchNorm-backward epilogue needs the partials";
  const bool wide16 = k.x_store == Store::b16 || k.y_store == Store::b16;
  if (wide16 && k.pack != Pack::b16) return "bf16 storage needs the plain bf16 pack";
  // (the on-load transform exists for fp32 -> fp32 and bf16 -> fp32 / bf16: the project conv of the training plans)
  if (k.tf && k.x_store == Store::f32 && k.y_store == Store::b16) return "the on-load transform needs an fp32 output or a bf16 input";
  if (k.c1 != 0) {
    if (k.c1 < 4 || k.c1 % 4 != 0 || k.Ci - k.c1 < 4) return "two sources need c1 and Ci - c1 multiples of 4";
    if (k.x_store == Store::b16 && k.c1 % 32 != 0) return "a bf16 first source needs c1 % 32 == 0";   // a chunk is one source or the other
    if (k.ci_x != k.Ci) return "two sources and K-concat do not combine";
  }
  if (k.ci_x != k.Ci) {
    // (ci_x % 32 == 0: a 32-row chunk never straddles two banks; the attention rides in the input scale)
    if (k.ci_x < 32 || k.ci_x % 32 != 0 || k.Ci % k.ci_x != 0) return "K-concat needs ci_x % 32 == 0 and whole banks";
    if (!k.scale || k.pack == Pack::f32) return "K-concat needs the input scale and a bf16 pack";
  }
  if (k.S % 4 != 0) {
    // the plain 4-byte kernel: fp32 tensors, one source, no transform; the statistics entry points answer 1 there
    if (k.stats) return nullptr;
    if (k.tf || k.c1 != 0 || k.ci_x != k.Ci || wide16) return "S must be a multiple of 4";
    return nullptr;
  }
  if (k.pack != Pack::f32 && (long long)k.B * k.S > kMaxColumns) return "B*S exceeds the 32-bit column index";
  return nullptr;
}

// ---- the plan ---------------------------------------------------------------------------------------------------------------
struct PwPlan {
  Route route;
  int MT;                 // m-tiles of 16 output rows
  int MC, mtw;            // row chunks, m-tiles per block (the kernels' MTW; MTB of the expand kernel)
  int n_tiles, tps;       // column tiles; tiles per sample (per-sample weights), else 0: tiles may straddle samples
  int NS;                 // samples whose input scale a column tile stages, 0 without scale
  long long wp_bstride;   // elements of the pack between two samples' weights
  int nprod;              // bf16 kernels: 3 = split operands (bf16x3), 1 = plain bf16; 0 = fp32 MFMA
  bool tf;                // the instance with the on-load transform
  bool pipe;              // fp32 kernel: counted-wait ring of 16-row chunks (else the 2-stage fallback)
  int kc, n_stages;       // k rows per LDS stage, stages
  int n_chunks;           // k chunks (expand kernel: its NCH)
  int sc_bytes;           // bf16 LDS kernel: bytes of scale per stage
  int lds_bytes;          // dynamic LDS of the launch
  unsigned grid[3];
};

inline PwPlan plan(const PwKey& k, int mode) {
  const int B = k.B, Ci = k.Ci, Co = k.Co, S = k.S;
  PwPlan p{};
  p.route = Route::none;
  p.MT = (Co + 15) / 16;
  const int MT = p.MT;
  p.tf = k.tf;
  p.nprod = k.pack == Pack::f32 ? 0 : k.pack == Pack::b16x2 ? 3 : 1;
  const int np2 = p.nprod == 3 ? 2 : 1;
  p.wp_bstride = k.pack == Pack::f32 ? (long long)(Ci / 4) * MT * 64 : (long long)((Ci + kKC - 1) / kKC) * MT * np2 * 512;
  if (S % 4 != 0) {    // planes that do not start on 16-byte boundaries (e.g. 40-mel models): plain 4-byte kernel
    if (k.stats) return p;                           // no epilogue statistics there: the caller runs the separate pass
    p.route = Route::generic;
    if (!k.per_sample) p.wp_bstride = 0;
    p.grid[0] = (unsigned)((S + 63) / 64); p.grid[1] = (unsigned)MT; p.grid[2] = (unsigned)B;
    return p;
  }
  p.tps = k.per_sample ? (S + kTileN - 1) / kTileN : 0;
  p.n_tiles = stat_tiles(B, S, k.per_sample);
  const int tiles8 = (p.n_tiles + 7) / 8 * 8;
  p.NS = kTileN / S + 2;
  if (p.NS > B) p.NS = B;
  if (!k.scale) p.NS = 0;
  p.grid[1] = p.grid[2] = 1;

  if (k.pack != Pack::f32 && mode != 0 && k.x_store == Store::f32 && k.y_store == Store::f32 && !k.per_sample && !k.tf &&
      k.c1 == 0 && !k.stats) {
    // conv_pw_stream.hip: barrier-free kernels for plain fp32 -> fp32 convs
    p.n_chunks = (Ci + kKC - 1) / kKC;
    if ((mode & kStreamExpand) && k.ci_x == Ci && !k.scale && !k.res && !k.pool && k.y && p.n_chunks <= 4 && Co >= 2 * Ci &&
        (long long)B * Co * S * 4 < 0x7fffffffLL) {
      // all rows in one block when the column tiles alone fill the chip twice; otherwise split the rows (x is re-read
      // from the XCD's L2 by the other m-chunks)
      int MC = 1;
      while (p.n_tiles * MC < 448 && (MT + 2 * MC - 1) / (2 * MC) >= 4) MC *= 2;
      while ((MT + MC - 1) / MC > 64) ++MC;                      // s_bias holds 64 m-tiles
      p.mtw = (MT + MC - 1) / MC;
      p.MC = (MT + p.mtw - 1) / p.mtw;
      p.route = Route::expand;
      p.grid[0] = (unsigned)(tiles8 * p.MC);
      return p;
    }
    // bit 1 (the default): project-shaped layers where the K-streaming kernel measured faster in the mn10 forward at
    // B = 256 - long reductions (C_in >= 160) that need no more row chunks than the LDS-staged kernel (<= 6 m-tiles, or as
    // many chunks of <= 6 as of <= 8): 240->80 36->28 us, 672->160 41->28, 960->160 59->38; NOT 120->40 @ 16x125 (4
    // chunks of K: 82 vs 86 us) and NOT 7 m-tiles (4 + 3 against one block of 7: 480->112 76 vs 87 us).
    // bit 2: every other layer as row chunks of the K-streaming kernel (A/B and tests).
    // bit 3: DyMN's K-concat launches.
    const bool measured_win = Co <= 2 * Ci && Ci >= 160 && (MT + 5) / 6 == (MT + 7) / 8;
    if (k.ci_x != Ci ? (mode & kStreamKcat) != 0 : (((mode & kStreamProject) && measured_win) || (mode & kStreamRest))) {
      p.MC = (MT + 5) / 6;                           // at most 6 m-tiles of accumulators + fragments per wave
      p.mtw = (MT + p.MC - 1) / p.MC;
      p.MC = (MT + p.mtw - 1) / p.mtw;
      p.route = Route::kstream;
      p.grid[0] = (unsigned)(tiles8 * p.MC);
      return p;
    }
  }

  // Row chunking of the LDS-staged kernels.  Every block re-reads its 256-column x tile, and a CU takes in only ~10 B/clk, so
  // the tile must be tall: up to 8 m-tiles (128 rows) per block, balanced over the row chunks.
  // (K-concat launches with few output rows - 128 x 1920 -> 320 @ 4x32: 192 blocks of 240 chunks - do NOT gain from more,
  // smaller row chunks: every block re-streams its x tile once per bank through L2, 425 -> 480 us with 448 blocks)
  p.MC = (MT + 7) / 8;
  p.mtw = (MT + p.MC - 1) / p.MC;
  p.MC = (MT + p.mtw - 1) / p.mtw;
  p.grid[0] = (unsigned)(tiles8 * p.MC);
  if (k.pack == Pack::f32) {
    p.route = Route::lds_f32;
    p.pipe = kPipeKC * p.NS <= 64;
    int floats;
    if (p.pipe) {
      p.kc = kPipeKC;
      p.n_chunks = (Ci + p.kc - 1) / p.kc;
      p.n_stages = p.n_chunks < 3 ? p.n_chunks : 3;
      // the scale slot is a fixed 64-float piece in this mode
      floats = p.n_stages * (a_stage_floats(p.mtw, p.kc) + p.kc * kTileN + (k.scale ? 64 : 0));
    } else {
      // generic: <= 32 rows per stage, chunks balanced, multiple of 4
      const int n32 = (Ci + kKC - 1) / kKC;
      p.kc = (((Ci + n32 - 1) / n32) + 3) & ~3;
      p.n_chunks = (Ci + p.kc - 1) / p.kc;
      p.n_stages = p.n_chunks > 1 ? 2 : 1;
      floats = p.n_stages * stage_floats(p.mtw, p.kc, p.NS);
    }
    if (k.stats && floats < 10 * p.mtw * 16) floats = 10 * p.mtw * 16;   // wave partials + (a, b)
    p.lds_bytes = floats * 4;
    return p;
  }
  p.route = Route::lds_b16;
  p.kc = kKC;
  p.n_chunks = (Ci + kKC - 1) / kKC;
  p.sc_bytes = k.scale ? ((kKC * p.NS + 63) / 64) * 256 : 0;
  // Two LDS stages (chunk c+1 in flight under the MFMAs of chunk c) when two such blocks fit a CU or when
  // there are not enough blocks for two per CU anyway; otherwise ONE stage, so that a second resident
  // block hides the load latency and the store phase instead (measured on MI355X, B=256: 80->480 95 vs
  // 135 us, 160->960 48 vs 83 us; the K-heavy 960->160 with 256 blocks keeps two stages: 45 vs 56 us).
  const int stage = p.mtw * np2 * 1024 + kKC * kTileN * ((k.x_store == Store::b16 && k.c1 == 0) ? 2 : 4) + p.sc_bytes;
  p.n_stages = (2 * stage <= 78 * 1024 || (int)p.grid[0] < 2 * 256) ? 2 : 1;
  p.lds_bytes = p.n_stages * stage;
  return p;
}

}  // namespace pw
}  // namespace eat
