// Stand-alone structure check of efficientat_amd/csrc/wgrad_plan.h (built and run by tests/test_wgrad_plan_cpu.py with a host
// compiler and -fsanitize=address,undefined): walks a grid of requests and checks that every plan is a launchable cover of
// its problem.  It knows nothing of WHICH kernel a shape should get - the table in the test does.  Exit status 0 = no violation.
#include <cstdio>
#include <initializer_list>
#include "wgrad_plan.h"

using namespace eat::wg;

static long long n_plans = 0, n_bad = 0, n_kind[4] = {0, 0, 0, 0}, n_refused = 0, n_b16_untiled = 0;
static const WgReq* cur = nullptr;
static void need(bool ok, const char* what) {
  if (ok) return;
  if (++n_bad <= 20)
    printf("VIOLATION %s: B=%d Co=%d Ci=%d S=%d per_sample=%d arith=%d same=%d x_scale=%d xf=%d ws_slots=%d\n", what, cur->B, cur->Co,
           cur->Ci, cur->S, cur->per_sample, (int)cur->arith, cur->same, cur->x_scale, (int)cur->xf, cur->ws_slots);
}
// nz blocks of upb units cover `total` units and the last block is not empty
static bool cut(long long total, long long upb, long long nz) { return upb >= 1 && nz >= 1 && (nz - 1) * upb < total && total <= nz * upb; }
static void check_wide(const WideShape& w, int Co, int Ci) {
  const int PR = w.swap ? Ci : Co, QR = w.swap ? Co : Ci;
  need(cut(PR, w.ptr, w.ptn) && cut(QR, w.qtr, w.qtn), "wide tiles cover P and Q exactly");
  need(w.ptr % 16 == 0 && w.qtr % 16 == 0 && w.ptr <= 256 && w.qtr <= 160, "wide tile rows");
  need(wide_lds_bytes(w) <= wide_lds_limit, "wide tile LDS");
}

static void check_plan(const WgReq& r) {
  cur = &r;
  const Planned o = plan(r);
  ++n_plans;
  if (o.ws_short) {                                           // refused: only a too small workspace in front of 16-byte rows
    ++n_refused;
    need(r.ws_slots != 0 && r.ws_slots < (int)o.wide_nz && (r.Ci & 3) == 0, "refusal");
    return;
  }
  const WgPlan& p = o.p;
  need(p.kind >= 0 && p.kind <= 3, "kind");
  ++n_kind[p.kind & 3];
  need(p.sps == (r.S + 31) / 32, "units per sample");
  const long long total = (long long)r.B * p.sps;
  if (p.kind == 2) {
    need(cut(r.B, p.bpb, p.nz), "samples per block");
    need(!r.per_sample || p.bpb == 1, "per-sample: one sample per block");
    return;
  }
  need((r.S & 3) == 0 && r.arith != Arith::fp32, "16-byte loads along k");
  if (r.per_sample) {                                         // blocks never straddle samples
    const int per = p.kind == 0 ? p.ps_spl : 1;
    need(p.kind != 3 && cut(p.sps, p.upb, per) && p.nz == (unsigned)(r.B * per), "per-sample k cut");
  } else {
    need(cut(total, p.upb, p.nz), "k cut");
  }
  if (p.kind == 0) {
    need(thin_pair(p.mtb, p.ntb), "streaming instance");
    need(p.mtb * p.ntb < 16 || p.gram, "4 x 4 is a Gram instance");
    need(!p.gram || (r.same && r.Co == r.Ci && p.mtb == p.ntb && p.mg == 1 && p.ng == 1), "Gram form");
    need(p.mg >= 1 && p.ng >= 1 && p.mg * p.ng <= 4, "row groups");
    need(p.mg * p.mtb * 16 >= r.Co && p.ng * p.ntb * 16 >= r.Ci, "row groups cover Co x Ci");
    need((p.mg - 1) * p.mtb * 16 < r.Co && (p.ng - 1) * p.ntb * 16 < r.Ci, "no empty row group");
  }
  if (p.kind == 3) {
    need(p.w.ok && (r.Ci & 3) == 0 && r.ws_slots >= (int)p.nz && o.wide_nz == p.nz, "wide plan has its workspace and 16-byte rows");
    need(!r.same || p.w.ptn * p.w.qtn == 1, "Gram: one tile");
    check_wide(p.w, r.Co, r.Ci);
  }
}

static void check_b16(int B, int Co, int Ci, int S, int x_b16) {
  WgReq r{};
  r.B = B; r.Co = Co; r.Ci = Ci; r.S = S; r.ws_slots = -(100 + x_b16);      // (for the message only)
  cur = &r;
  const WgB16Plan p = plan_b16(B, Co, Ci, S, x_b16);
  ++n_plans;
  need(cut((long long)B * p.sps, p.upb, p.nz), "b16 k cut");
  if (!p.w.ok) { ++n_b16_untiled; return; }                   // (the entry points refuse: "internal tiling error")
  check_wide(p.w, Co, Ci);
  const int ns = dyn_b16_slices(p, B);
  need(ns >= 1 && ns <= 8 && cut(p.sps, (p.sps + ns - 1) / ns, ns), "per-sample slices own a unit each");
}

int main() {
  const int Bs[] = {1, 2, 3, 5, 48, 128, 256};
  // the channel counts of the 1x1 convs of mn10, mn40 and dymn20 (in / expanded / out / SE / head), and counts that are no
  // multiple of 4 or of 16
  const int Cs[] = {16,  24,  32,  40,  48,  64,  72,  80,  96,  104, 112, 120, 128, 144, 160,  168,  184,  200,  224,  240,  256, 288,
                    320, 368, 400, 448, 480, 512, 576, 640, 672, 736, 800, 960, 1280, 1344, 1472, 1600, 1920, 2560, 2688, 3840, 5120,
                    3,   7,   17,  18,  30,  50,  66,  70,  90,  100, 130, 161, 250, 322};
  const int Ss[] = {4, 6, 20, 36, 72, 128, 500, 504, 2000, 8000, 32000};
  for (int B : Bs) for (int Co : Cs) for (int Ci : Cs) for (int S : Ss) {
    for (int x_b16 = 0; x_b16 < 3; ++x_b16) check_b16(B, Co, Ci, S, x_b16);
    for (int ar = 0; ar < 3; ++ar) for (int ps = 0; ps < 2; ++ps) for (int same = 0; same < 2; ++same)
      for (int xs = 0; xs < 2; ++xs) for (int xf = 0; xf < 3; ++xf) {
        WgReq r{};
        r.B = B; r.Co = Co; r.Ci = Ci; r.S = S; r.per_sample = ps != 0; r.arith = arith_of(ar); r.same = same != 0;
        r.x_scale = xs != 0; r.xf = (Xf)xf;
        r.ws_slots = ws_enough;
        check_plan(r);
        const int enough = (int)plan(r).wide_nz;                // (0: the plan does not look at the workspace)
        if (enough == 0) continue;
        for (int ws : {0, 8, enough, enough - 1}) {             // workspace absent, 8 copies, exactly enough, one too few
          r.ws_slots = ws;
          check_plan(r);
        }
      }
  }
  printf("%lld plans, %lld violations (kinds 0/1/2/3: %lld %lld %lld %lld; refused %lld; bf16 shapes without a tiling %lld)\n", n_plans,
         n_bad, n_kind[0], n_kind[1], n_kind[2], n_kind[3], n_refused, n_b16_untiled);
  return n_bad != 0;
}
