// Stand-alone check of efficientat_amd/csrc/pw_fwd_plan.h (built and run by tests/test_pw_fwd_plan_cpu.py with a host compiler
// and -fsanitize=address,undefined): the route table of the forward 1x1 convs, the argument rules of check(), and the plan's
// structure over a grid of requests.  Exit status 0 = the table holds and no violation.
//
// The table was recorded from the library as it stood BEFORE the route moved into pw_fwd_plan.h: the forward 1x1 calls of one
// eager training step of mn10 (fp32 storage, batch 256), mn40 with bf16 storage (batch 128) and dymn20 (batch 128), of the mn10
// and dymn20 eval forwards, and of the cases of tests/test_gpu_pw_fwd_routes.py (the row's first column says which).  Kernel
// instance and grid come from a kernel trace of those runs, the dynamic LDS size from the launch arguments of the same calls.
// A changed row is a changed launch, to be measured like one.
//   entry: the eat_pw_conv_<entry>_fwd entry point (fwd = eat_pw_conv_fwd); pack 0 fp32, 1 bf16, 2 bf16 hi + lo; c1: channels
//   of the first of two sources; ci_x: channels of x of a K-concat launch; mode: eat_pw_stream_mode at the call
//   flags: p per-sample weights, x / w bf16 storage of x / y, y output written, s input scale, r residual, o pooled sums,
//   t on-load transform, a statistics partials, g their BatchNorm-backward form
//   -> route, MTW (0: not a template parameter), NPROD, var (NSTG of the bf16 LDS kernel, PIPE of the fp32 LDS kernel, NCH
//   of the expand kernel), TF, grid blocks, dynamic LDS bytes
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include "pw_fwd_plan.h"

using namespace eat::pw;

struct Row {
  const char* src; const char* entry; int B, Ci, Co, S, pack, c1, ci_x, mode; const char* flags;
  Route route; int mtw, nprod, var, tf, blocks, lds;
};
static const Row kTable[] = {
  {"generic-stats", "stats", 2, 8, 24, 15, 0, 0, 0, 2, "ya", Route::none, 0, 0, 0, 0, 0, 0},
  {"generic-gstats", "gstats", 2, 8, 24, 15, 0, 0, 0, 2, "yag", Route::none, 0, 0, 0, 0, 0, 0},
  {"f32-pipe", "fwd", 2, 8, 24, 60, 0, 0, 0, 2, "yro", Route::lds_f32, 2, 0, 1, 0, 8, 18432},
  {"f32-nopipe", "fwd", 6, 72, 24, 16, 0, 0, 0, 2, "ys", Route::lds_f32, 2, 0, 0, 0, 8, 56448},
  {"f32-two-row-chunks", "fwd", 2, 8, 136, 64, 0, 0, 0, 2, "y", Route::lds_f32, 5, 0, 1, 0, 16, 21504},
  {"f32-lds-above-64k", "fwd", 2, 48, 128, 64, 0, 0, 0, 2, "y", Route::lds_f32, 8, 0, 1, 0, 8, 73728},
  {"generic-f32", "fwd", 2, 8, 24, 15, 0, 0, 0, 2, "ysro", Route::generic, 0, 0, 0, 0, 4, 0},
  {"generic-b16", "bf16", 2, 8, 24, 15, 1, 0, 0, 2, "ysro", Route::generic, 0, 0, 0, 0, 4, 0},
  {"generic-x3", "bf16", 2, 8, 24, 15, 2, 0, 0, 2, "ysro", Route::generic, 0, 0, 0, 0, 4, 0},
  {"generic-dyn", "dyn", 2, 8, 24, 15, 0, 0, 0, 2, "pyr", Route::generic, 0, 0, 0, 0, 4, 0},
  {"b16lds-two-stages-x3", "bf16", 2, 40, 48, 64, 2, 0, 0, 2, "yr", Route::lds_b16, 3, 3, 2, 0, 8, 77824},
  {"b16lds-two-stages-b16", "bf16", 2, 40, 48, 64, 1, 0, 0, 2, "yr", Route::lds_b16, 3, 1, 2, 0, 8, 71680},
  {"b16lds-one-stage", "bf16", 8, 32, 128, 16384, 2, 0, 0, 2, "yr", Route::lds_b16, 8, 3, 1, 0, 512, 49152},
  {"expand-32-64", "bf16", 2, 32, 64, 64, 2, 0, 0, 3, "y", Route::expand, 0, 3, 1, 0, 8, 0},
  {"expand-32-256", "bf16", 2, 32, 256, 64, 2, 0, 0, 3, "y", Route::expand, 0, 3, 1, 0, 32, 0},
  {"expand-128-256", "bf16", 2, 128, 256, 64, 1, 0, 0, 3, "y", Route::expand, 0, 1, 4, 0, 32, 0},
  {"expand-128-1024", "bf16", 2, 128, 1024, 64, 2, 0, 0, 3, "y", Route::expand, 0, 3, 4, 0, 128, 0},
  {"kstream-160-40-x3", "bf16", 2, 160, 40, 64, 2, 0, 0, 2, "ysro", Route::kstream, 3, 3, 0, 0, 8, 0},
  {"kstream-160-40-b16", "bf16", 2, 160, 40, 64, 1, 0, 0, 2, "ysr", Route::kstream, 3, 1, 0, 0, 8, 0},
  {"kstream-not-7-tiles", "bf16", 2, 160, 112, 64, 2, 0, 0, 2, "ysr", Route::lds_b16, 7, 3, 2, 0, 8, 94720},
  {"kcat-lds", "kcat", 3, 128, 48, 8, 2, 0, 32, 2, "ysr", Route::lds_b16, 3, 3, 2, 0, 8, 78848},
  {"kcat-kstream", "kcat", 3, 128, 48, 8, 2, 0, 32, 10, "ysr", Route::kstream, 3, 3, 0, 0, 8, 0},
  {"tf-f32", "tf", 2, 16, 24, 64, 0, 0, 0, 2, "yrt", Route::lds_f32, 2, 0, 1, 1, 8, 18432},
  {"tf-f32-scale", "tf", 2, 16, 24, 64, 0, 0, 0, 2, "yst", Route::lds_f32, 2, 0, 1, 1, 8, 18688},
  {"tf-x3", "tf", 2, 16, 24, 64, 2, 0, 0, 2, "yrt", Route::lds_b16, 2, 3, 2, 1, 8, 73728},
  {"tf-x3-scale", "tf", 2, 16, 24, 64, 2, 0, 0, 2, "yst", Route::lds_b16, 2, 3, 2, 1, 8, 74240},
  {"cat-f32", "cat", 2, 20, 24, 64, 0, 8, 0, 2, "yr", Route::lds_f32, 2, 0, 1, 0, 8, 36864},
  {"cat-x3", "cat", 2, 40, 24, 64, 2, 32, 0, 2, "yr", Route::lds_b16, 2, 3, 2, 0, 8, 73728},
  {"cat-b16", "cat", 2, 40, 24, 64, 1, 32, 0, 2, "y", Route::lds_b16, 2, 1, 2, 0, 8, 69632},
  {"dyn-f32", "dyn", 3, 16, 24, 260, 0, 0, 0, 2, "pyr", Route::lds_f32, 2, 0, 1, 0, 8, 18432},
  {"dyn-x3", "dyn_bf16", 3, 16, 24, 260, 2, 0, 0, 2, "pyr", Route::lds_b16, 2, 3, 2, 0, 8, 73728},
  {"stats-f32", "stats", 3, 16, 24, 260, 0, 0, 0, 2, "ya", Route::lds_f32, 2, 0, 1, 0, 8, 18432},
  {"stats-x3-tf-scale", "stats", 3, 16, 24, 260, 2, 0, 0, 2, "ysta", Route::lds_b16, 2, 3, 2, 1, 8, 74240},
  {"stats-b16", "stats", 3, 16, 24, 260, 1, 0, 0, 2, "ya", Route::lds_b16, 2, 1, 2, 0, 8, 69632},
  {"stats-f32-per-sample", "stats", 3, 16, 24, 260, 0, 0, 0, 2, "pya", Route::lds_f32, 2, 0, 1, 0, 8, 18432},
  {"stats-x3-per-sample", "stats", 3, 16, 24, 260, 2, 0, 0, 2, "pya", Route::lds_b16, 2, 3, 2, 0, 8, 73728},
  {"gstats-f32", "gstats", 3, 16, 24, 260, 0, 0, 0, 2, "yag", Route::lds_f32, 2, 0, 1, 0, 8, 18432},
  {"gstats-x3", "gstats", 3, 16, 24, 260, 2, 0, 0, 2, "yag", Route::lds_b16, 2, 3, 2, 0, 8, 73728},
  {"b16-f32-to-b16", "b16", 2, 32, 64, 64, 1, 0, 0, 2, "wy", Route::lds_b16, 4, 1, 2, 0, 8, 73728},
  {"b16-b16-to-f32", "b16", 2, 32, 64, 64, 1, 0, 0, 2, "xyra", Route::lds_b16, 4, 1, 2, 0, 8, 40960},
  {"b16-b16-to-b16", "b16", 2, 32, 64, 64, 1, 0, 0, 2, "xwya", Route::lds_b16, 4, 1, 2, 0, 8, 40960},
  {"b16-two-sources", "b16", 2, 40, 24, 64, 1, 32, 0, 2, "xyr", Route::lds_b16, 2, 1, 2, 0, 8, 69632},
  {"b16-gz", "b16", 2, 32, 64, 64, 1, 0, 0, 2, "xwyag", Route::lds_b16, 4, 1, 2, 0, 8, 40960},
  {"dyn-b16-out-s8-stats", "dyn_b16", 3, 16, 24, 8, 1, 0, 0, 2, "pwya", Route::lds_b16, 2, 1, 2, 0, 8, 69632},
  {"dyn-b16-out-s264", "dyn_b16", 3, 16, 24, 264, 1, 0, 0, 2, "pwy", Route::lds_b16, 2, 1, 2, 0, 8, 69632},
  {"dyn-b16-in-s264-stats", "dyn_b16", 3, 16, 24, 264, 1, 0, 0, 2, "pxyra", Route::lds_b16, 2, 1, 2, 0, 8, 36864},
  {"dyn-b16-in-s8", "dyn_b16", 3, 16, 24, 8, 1, 0, 0, 2, "pxy", Route::lds_b16, 2, 1, 2, 0, 8, 36864},
  {"mn10-train", "stats", 256, 16, 16, 32000, 0, 0, 0, 2, "yta", Route::lds_f32, 1, 0, 1, 1, 32000, 17408},
  {"mn10-train", "fwd", 256, 16, 64, 32000, 0, 0, 0, 2, "y", Route::lds_f32, 4, 0, 1, 0, 32000, 20480},
  {"mn10-train", "stats", 256, 64, 24, 8000, 2, 0, 0, 2, "yta", Route::lds_b16, 2, 3, 2, 1, 8000, 73728},
  {"mn10-train", "fwd", 256, 24, 72, 8000, 0, 0, 0, 2, "y", Route::lds_f32, 5, 0, 1, 0, 8000, 43008},
  {"mn10-train", "stats", 256, 72, 24, 8000, 2, 0, 0, 2, "yta", Route::lds_b16, 2, 3, 2, 1, 8000, 73728},
  {"mn10-train", "stats", 256, 72, 40, 2000, 2, 0, 0, 2, "ysta", Route::lds_b16, 3, 3, 2, 1, 2000, 78336},
  {"mn10-eval+mn10-train", "bf16", 256, 40, 120, 2000, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 1, 0, 2000, 49152},
  {"mn10-train", "stats", 256, 120, 40, 2000, 2, 0, 0, 2, "ysta", Route::lds_b16, 3, 3, 2, 1, 2000, 78336},
  {"mn10-eval+mn10-train", "bf16", 256, 40, 240, 2000, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 1, 0, 4000, 49152},
  {"mn10-train", "stats", 256, 240, 80, 504, 2, 0, 0, 2, "yta", Route::lds_b16, 5, 3, 2, 1, 504, 86016},
  {"mn10-train", "bf16", 256, 80, 200, 504, 2, 0, 0, 2, "y", Route::lds_b16, 7, 3, 1, 0, 1008, 47104},
  {"mn10-train", "stats", 256, 200, 80, 504, 2, 0, 0, 2, "yta", Route::lds_b16, 5, 3, 2, 1, 504, 86016},
  {"mn10-train", "bf16", 256, 80, 184, 504, 2, 0, 0, 2, "y", Route::lds_b16, 6, 3, 1, 0, 1008, 45056},
  {"mn10-train", "stats", 256, 184, 80, 504, 2, 0, 0, 2, "yta", Route::lds_b16, 5, 3, 2, 1, 504, 86016},
  {"mn10-train", "bf16", 256, 80, 480, 504, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 1, 0, 2016, 49152},
  {"mn10-train", "stats", 256, 480, 112, 504, 2, 0, 0, 2, "ysa", Route::lds_b16, 7, 3, 2, 0, 504, 94720},
  {"mn10-eval+mn10-train", "bf16", 256, 112, 672, 504, 2, 0, 0, 2, "y", Route::lds_b16, 7, 3, 1, 0, 3024, 47104},
  {"mn10-train", "stats", 256, 672, 112, 504, 2, 0, 0, 2, "ysa", Route::lds_b16, 7, 3, 2, 0, 504, 94720},
  {"mn10-train", "stats", 256, 672, 160, 128, 2, 0, 0, 2, "ysa", Route::lds_b16, 5, 3, 2, 0, 256, 87040},
  {"mn10-eval+mn10-train", "bf16", 256, 160, 960, 128, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 1, 0, 1024, 49152},
  {"mn10-train", "stats", 256, 960, 160, 128, 2, 0, 0, 2, "ysa", Route::lds_b16, 5, 3, 2, 0, 256, 87040},
  {"mn10-train", "stats", 256, 160, 960, 128, 2, 0, 0, 2, "ya", Route::lds_b16, 8, 3, 1, 0, 1024, 49152},
  {"mn10-train", "bf16", 256, 960, 160, 128, 2, 0, 0, 2, "y", Route::kstream, 5, 3, 0, 0, 256, 0},
  {"mn10-train", "cat", 256, 1120, 160, 128, 2, 960, 0, 2, "yr", Route::lds_b16, 5, 3, 2, 0, 256, 86016},
  {"mn10-train", "bf16", 256, 160, 672, 128, 2, 0, 0, 2, "y", Route::lds_b16, 7, 3, 1, 0, 768, 47104},
  {"mn10-train", "cat", 256, 784, 112, 504, 2, 672, 0, 2, "y", Route::lds_b16, 7, 3, 2, 0, 504, 94208},
  {"mn10-train", "cat", 256, 784, 112, 504, 2, 672, 0, 2, "yr", Route::lds_b16, 7, 3, 2, 0, 504, 94208},
  {"mn10-train", "bf16", 256, 112, 480, 504, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 1, 0, 2016, 49152},
  {"mn10-train", "cat", 256, 560, 80, 504, 2, 480, 0, 2, "y", Route::lds_b16, 5, 3, 2, 0, 504, 86016},
  {"mn10-train", "cat", 256, 264, 80, 504, 2, 184, 0, 2, "yr", Route::lds_b16, 5, 3, 2, 0, 504, 86016},
  {"mn10-train", "cat", 256, 280, 80, 504, 2, 200, 0, 2, "yr", Route::lds_b16, 5, 3, 2, 0, 504, 86016},
  {"mn10-train", "bf16", 256, 80, 240, 504, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 1, 0, 1008, 49152},
  {"mn10-train", "cat", 256, 280, 40, 2000, 2, 240, 0, 2, "y", Route::lds_b16, 3, 3, 2, 0, 2000, 77824},
  {"mn10-train", "cat", 256, 160, 40, 2000, 2, 120, 0, 2, "yr", Route::lds_b16, 3, 3, 2, 0, 2000, 77824},
  {"mn10-train", "bf16", 256, 40, 72, 2000, 2, 0, 0, 2, "y", Route::lds_b16, 5, 3, 1, 0, 2000, 43008},
  {"mn10-train", "cat", 256, 96, 24, 8000, 2, 72, 0, 2, "y", Route::lds_b16, 2, 3, 2, 0, 8000, 73728},
  {"mn10-train", "gstats", 256, 24, 72, 8000, 0, 0, 0, 2, "yag", Route::lds_f32, 5, 0, 1, 0, 8000, 43008},
  {"mn10-train", "cat", 256, 96, 24, 8000, 2, 72, 0, 2, "yr", Route::lds_b16, 2, 3, 2, 0, 8000, 73728},
  {"mn10-train", "gstats", 256, 24, 64, 8000, 0, 0, 0, 2, "yag", Route::lds_f32, 4, 0, 1, 0, 8000, 40960},
  {"mn10-train", "cat", 256, 80, 16, 32000, 2, 64, 0, 2, "y", Route::lds_b16, 1, 3, 2, 0, 32000, 69632},
  {"mn10-train", "gstats", 256, 16, 16, 32000, 0, 0, 0, 2, "yag", Route::lds_f32, 1, 0, 1, 0, 32000, 17408},
  {"mn40b-train", "b16", 128, 64, 64, 32000, 1, 0, 0, 2, "xwyta", Route::lds_b16, 4, 1, 2, 1, 16000, 40960},
  {"mn40b-train", "b16", 128, 64, 256, 32000, 1, 0, 0, 2, "xwy", Route::lds_b16, 8, 1, 2, 0, 32000, 49152},
  {"mn40b-train", "b16", 128, 256, 96, 8000, 1, 0, 0, 2, "xwyta", Route::lds_b16, 6, 1, 2, 1, 4000, 45056},
  {"mn40b-train", "b16", 128, 96, 288, 8000, 1, 0, 0, 2, "xwy", Route::lds_b16, 6, 1, 2, 0, 12000, 45056},
  {"mn40b-train", "b16", 128, 288, 96, 8000, 1, 0, 0, 2, "xwyta", Route::lds_b16, 6, 1, 2, 1, 4000, 45056},
  {"mn40b-train", "b16", 128, 288, 160, 2000, 1, 0, 0, 2, "xwysta", Route::lds_b16, 5, 1, 2, 1, 2000, 43520},
  {"mn40b-train", "b16", 128, 160, 480, 2000, 1, 0, 0, 2, "xwy", Route::lds_b16, 8, 1, 2, 0, 4000, 49152},
  {"mn40b-train", "b16", 128, 480, 160, 2000, 1, 0, 0, 2, "xwysta", Route::lds_b16, 5, 1, 2, 1, 2000, 43520},
  {"mn40b-train", "b16", 128, 160, 960, 2000, 1, 0, 0, 2, "xwy", Route::lds_b16, 8, 1, 2, 0, 8000, 49152},
  {"mn40b-train", "b16", 128, 960, 320, 504, 1, 0, 0, 2, "xwyta", Route::lds_b16, 7, 1, 2, 1, 768, 47104},
  {"mn40b-train", "bf16", 1, 320, 800, 320, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 56, 98304},
  {"mn40b-train", "b16", 128, 320, 800, 504, 1, 0, 0, 2, "xwy", Route::lds_b16, 8, 1, 2, 0, 1792, 49152},
  {"mn40b-train", "b16", 128, 800, 320, 504, 1, 0, 0, 2, "xwyta", Route::lds_b16, 7, 1, 2, 1, 768, 47104},
  {"mn40b-train", "bf16", 1, 320, 736, 320, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 48, 98304},
  {"mn40b-train", "b16", 128, 320, 736, 504, 1, 0, 0, 2, "xwy", Route::lds_b16, 8, 1, 2, 0, 1536, 49152},
  {"mn40b-train", "b16", 128, 736, 320, 504, 1, 0, 0, 2, "xwyta", Route::lds_b16, 7, 1, 2, 1, 768, 47104},
  {"mn40b-train", "bf16", 1, 320, 1920, 320, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 120, 98304},
  {"mn40b-train", "b16", 128, 320, 1920, 504, 1, 0, 0, 2, "xwy", Route::lds_b16, 8, 1, 2, 0, 3840, 49152},
  {"mn40b-train", "b16", 128, 1920, 448, 504, 1, 0, 0, 2, "xwysa", Route::lds_b16, 7, 1, 2, 0, 1024, 47616},
  {"mn40b-train", "bf16", 1, 448, 2688, 448, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 168, 98304},
  {"mn40b-train", "b16", 128, 448, 2688, 504, 1, 0, 0, 2, "xwy", Route::lds_b16, 8, 1, 2, 0, 5376, 49152},
  {"mn40b-train", "b16", 128, 2688, 448, 504, 1, 0, 0, 2, "xwysa", Route::lds_b16, 7, 1, 2, 0, 1024, 47616},
  {"mn40b-train", "b16", 128, 2688, 640, 128, 1, 0, 0, 2, "xwysa", Route::lds_b16, 8, 1, 2, 0, 320, 50176},
  {"mn40b-train", "bf16", 1, 640, 3840, 640, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 240, 98304},
  {"mn40b-train", "b16", 128, 640, 3840, 128, 1, 0, 0, 2, "xwy", Route::lds_b16, 8, 1, 2, 0, 1920, 49152},
  {"mn40b-train", "b16", 128, 3840, 640, 128, 1, 0, 0, 2, "xwysa", Route::lds_b16, 8, 1, 2, 0, 320, 50176},
  {"mn40b-train", "stats", 128, 640, 3840, 128, 1, 0, 0, 2, "ya", Route::lds_b16, 8, 1, 1, 0, 1920, 40960},
  {"mn40b-train", "bf16", 128, 3840, 640, 128, 1, 0, 0, 2, "y", Route::lds_b16, 8, 1, 2, 0, 320, 81920},
  {"mn40b-train", "b16", 128, 4480, 640, 128, 1, 3840, 0, 2, "xyr", Route::lds_b16, 8, 1, 2, 0, 320, 81920},
  {"mn40b-train", "b16", 128, 640, 2688, 128, 1, 0, 0, 2, "xwy", Route::lds_b16, 8, 1, 2, 0, 1344, 49152},
  {"mn40b-train", "b16", 128, 3136, 448, 504, 1, 2688, 0, 2, "xy", Route::lds_b16, 7, 1, 2, 0, 1024, 79872},
  {"mn40b-train", "b16", 128, 3136, 448, 504, 1, 2688, 0, 2, "xyr", Route::lds_b16, 7, 1, 2, 0, 1024, 79872},
  {"mn40b-train", "b16", 128, 448, 1920, 504, 1, 0, 0, 2, "xwy", Route::lds_b16, 8, 1, 2, 0, 3840, 49152},
  {"mn40b-train", "b16", 128, 2240, 320, 504, 1, 1920, 0, 2, "xy", Route::lds_b16, 7, 1, 2, 0, 768, 79872},
  {"mn40b-train", "b16", 128, 1056, 320, 504, 1, 736, 0, 2, "xyr", Route::lds_b16, 7, 1, 2, 0, 768, 79872},
  {"mn40b-train", "b16", 128, 1120, 320, 504, 1, 800, 0, 2, "xyr", Route::lds_b16, 7, 1, 2, 0, 768, 79872},
  {"mn40b-train", "b16", 128, 320, 960, 504, 1, 0, 0, 2, "xwy", Route::lds_b16, 8, 1, 2, 0, 2048, 49152},
  {"mn40b-train", "b16", 128, 1120, 160, 2000, 1, 960, 0, 2, "xy", Route::lds_b16, 5, 1, 2, 0, 2000, 75776},
  {"mn40b-train", "b16", 128, 640, 160, 2000, 1, 480, 0, 2, "xyr", Route::lds_b16, 5, 1, 2, 0, 2000, 75776},
  {"mn40b-train", "b16", 128, 160, 288, 2000, 1, 0, 0, 2, "xwy", Route::lds_b16, 6, 1, 2, 0, 3000, 45056},
  {"mn40b-train", "b16", 128, 384, 96, 8000, 1, 288, 0, 2, "xy", Route::lds_b16, 6, 1, 2, 0, 4000, 77824},
  {"mn40b-train", "b16", 128, 96, 288, 8000, 1, 0, 0, 2, "xwyag", Route::lds_b16, 6, 1, 2, 0, 12000, 45056},
  {"mn40b-train", "b16", 128, 384, 96, 8000, 1, 288, 0, 2, "xyr", Route::lds_b16, 6, 1, 2, 0, 4000, 77824},
  {"mn40b-train", "b16", 128, 96, 256, 8000, 1, 0, 0, 2, "xwyag", Route::lds_b16, 8, 1, 2, 0, 8000, 49152},
  {"mn40b-train", "b16", 128, 320, 64, 32000, 1, 256, 0, 2, "xy", Route::lds_b16, 4, 1, 2, 0, 16000, 73728},
  {"mn40b-train", "b16", 128, 64, 64, 32000, 1, 0, 0, 2, "wy", Route::lds_b16, 4, 1, 2, 0, 16000, 73728},
  {"dymn20-train", "fwd", 1, 32, 64, 72192, 0, 0, 0, 2, "y", Route::lds_f32, 4, 0, 1, 0, 288, 40960},
  {"dymn20-train", "bf16", 1, 64, 32, 8192, 2, 0, 0, 2, "y", Route::lds_b16, 2, 3, 2, 0, 32, 73728},
  {"dymn20-train", "bf16", 1, 64, 32, 64000, 2, 0, 0, 2, "y", Route::lds_b16, 2, 3, 2, 0, 256, 73728},
  {"dymn20-train", "stats", 128, 32, 32, 32000, 0, 0, 0, 2, "pya", Route::lds_f32, 2, 0, 1, 0, 16000, 36864},
  {"dymn20-train", "bf16", 1, 64, 128, 4096, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 16, 98304},
  {"dymn20-train", "bf16", 1, 64, 128, 32000, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 128, 98304},
  {"dymn20-train", "stats", 128, 32, 128, 32000, 0, 0, 0, 2, "pya", Route::lds_f32, 8, 0, 1, 0, 16000, 49152},
  {"dymn20-train", "stats", 128, 128, 48, 8000, 2, 0, 0, 2, "pya", Route::lds_b16, 3, 3, 2, 0, 4096, 77824},
  {"dymn20-train", "bf16", 1, 48, 64, 36096, 2, 0, 0, 2, "y", Route::lds_b16, 4, 3, 2, 0, 144, 81920},
  {"dymn20-train", "bf16", 1, 64, 144, 4096, 2, 0, 0, 2, "y", Route::lds_b16, 5, 3, 2, 0, 32, 86016},
  {"dymn20-train", "bf16", 1, 64, 144, 32000, 2, 0, 0, 2, "y", Route::lds_b16, 5, 3, 2, 0, 256, 86016},
  {"dymn20-train", "stats", 128, 48, 144, 8000, 2, 0, 0, 2, "pya", Route::lds_b16, 5, 3, 1, 0, 8192, 43008},
  {"dymn20-train", "stats", 128, 144, 48, 8000, 2, 0, 0, 2, "pya", Route::lds_b16, 3, 3, 2, 0, 4096, 77824},
  {"dymn20-train", "bf16", 1, 64, 144, 2048, 2, 0, 0, 2, "y", Route::lds_b16, 5, 3, 2, 0, 16, 86016},
  {"dymn20-train", "bf16", 1, 64, 144, 16000, 2, 0, 0, 2, "y", Route::lds_b16, 5, 3, 2, 0, 128, 86016},
  {"dymn20-train", "stats", 128, 144, 80, 2000, 2, 0, 0, 2, "pya", Route::lds_b16, 5, 3, 1, 0, 1024, 43008},
  {"dymn20-train", "bf16", 1, 80, 64, 18048, 2, 0, 0, 2, "y", Route::lds_b16, 4, 3, 2, 0, 72, 81920},
  {"dymn20-train", "bf16", 1, 64, 240, 2048, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 16, 98304},
  {"dymn20-train", "bf16", 1, 64, 240, 16000, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 128, 98304},
  {"dymn20-train", "stats", 128, 80, 240, 2000, 2, 0, 0, 2, "pya", Route::lds_b16, 8, 3, 1, 0, 2048, 49152},
  {"dymn20-train", "stats", 128, 240, 80, 2000, 2, 0, 0, 2, "pya", Route::lds_b16, 5, 3, 1, 0, 1024, 43008},
  {"dymn20-train", "bf16", 1, 80, 120, 18048, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 72, 98304},
  {"dymn20-train", "bf16", 1, 120, 480, 1024, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 32, 98304},
  {"dymn20-train", "bf16", 1, 120, 480, 8064, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 128, 98304},
  {"dymn20-train", "stats", 128, 80, 480, 2000, 2, 0, 0, 2, "pya", Route::lds_b16, 8, 3, 1, 0, 4096, 49152},
  {"dymn20-train", "stats", 128, 480, 160, 504, 2, 0, 0, 2, "pya", Route::lds_b16, 5, 3, 1, 0, 512, 43008},
  {"dymn20-train", "bf16", 1, 160, 104, 9088, 2, 0, 0, 2, "y", Route::lds_b16, 7, 3, 2, 0, 40, 94208},
  {"dymn20-train", "bf16", 1, 104, 400, 1024, 2, 0, 0, 2, "y", Route::lds_b16, 7, 3, 2, 0, 32, 94208},
  {"dymn20-train", "bf16", 1, 104, 400, 8064, 2, 0, 0, 2, "y", Route::lds_b16, 7, 3, 2, 0, 128, 94208},
  {"dymn20-train", "stats", 128, 160, 400, 504, 2, 0, 0, 2, "pya", Route::lds_b16, 7, 3, 1, 0, 1024, 47104},
  {"dymn20-train", "stats", 128, 400, 160, 504, 2, 0, 0, 2, "pya", Route::lds_b16, 5, 3, 1, 0, 512, 43008},
  {"dymn20-train", "bf16", 1, 160, 96, 9088, 2, 0, 0, 2, "y", Route::kstream, 6, 3, 0, 0, 40, 0},
  {"dymn20-train", "bf16", 1, 96, 368, 1024, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 24, 98304},
  {"dymn20-train", "bf16", 1, 96, 368, 8064, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 96, 98304},
  {"dymn20-train", "stats", 128, 160, 368, 504, 2, 0, 0, 2, "pya", Route::lds_b16, 8, 3, 1, 0, 768, 49152},
  {"dymn20-train", "stats", 128, 368, 160, 504, 2, 0, 0, 2, "pya", Route::lds_b16, 5, 3, 1, 0, 512, 43008},
  {"dymn20-train", "bf16", 1, 160, 240, 9088, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 80, 98304},
  {"dymn20-train", "bf16", 1, 240, 960, 1024, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 64, 98304},
  {"dymn20-train", "bf16", 1, 240, 960, 8064, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 256, 98304},
  {"dymn20-train", "stats", 128, 160, 960, 504, 2, 0, 0, 2, "pya", Route::lds_b16, 8, 3, 1, 0, 2048, 49152},
  {"dymn20-train", "stats", 128, 960, 224, 504, 2, 0, 0, 2, "pya", Route::lds_b16, 7, 3, 1, 0, 512, 47104},
  {"dymn20-train", "bf16", 1, 224, 256, 9088, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 80, 98304},
  {"dymn20-train", "bf16", 1, 256, 1344, 1024, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 88, 98304},
  {"dymn20-train", "bf16", 1, 256, 1344, 8064, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 352, 98304},
  {"dymn20-train", "stats", 128, 224, 1344, 504, 2, 0, 0, 2, "pya", Route::lds_b16, 8, 3, 1, 0, 2816, 49152},
  {"dymn20-train", "stats", 128, 1344, 224, 504, 2, 0, 0, 2, "pya", Route::lds_b16, 7, 3, 1, 0, 512, 47104},
  {"dymn20-train", "bf16", 1, 256, 1344, 512, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 88, 98304},
  {"dymn20-train", "bf16", 1, 256, 1344, 4096, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 176, 98304},
  {"dymn20-train", "stats", 128, 1344, 320, 128, 2, 0, 0, 2, "pya", Route::lds_b16, 7, 3, 2, 0, 384, 94208},
  {"dymn20-train", "bf16", 1, 320, 256, 4608, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 48, 98304},
  {"dymn20-train", "bf16", 1, 256, 1920, 512, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 120, 98304},
  {"dymn20-train", "bf16", 1, 256, 1920, 4096, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 240, 98304},
  {"dymn20-train", "stats", 128, 320, 1920, 128, 2, 0, 0, 2, "pya", Route::lds_b16, 8, 3, 1, 0, 1920, 49152},
  {"dymn20-train", "stats", 128, 1920, 320, 128, 2, 0, 0, 2, "pya", Route::lds_b16, 7, 3, 2, 0, 384, 94208},
  {"dymn20-train", "bf16", 128, 320, 1920, 128, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 1, 0, 960, 49152},
  {"dymn20-train", "bf16", 128, 1920, 320, 128, 2, 0, 0, 2, "y", Route::lds_b16, 7, 3, 2, 0, 192, 94208},
  {"dymn20-train", "dyn_bf16", 128, 320, 1920, 128, 2, 0, 0, 2, "py", Route::lds_b16, 8, 3, 1, 0, 1920, 49152},
  {"dymn20-train", "dyn_bf16", 128, 1920, 320, 128, 2, 0, 0, 2, "pyr", Route::lds_b16, 7, 3, 2, 0, 384, 94208},
  {"dymn20-train", "bf16", 1, 1920, 256, 4096, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 32, 98304},
  {"dymn20-train", "bf16", 1, 1920, 256, 512, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 16, 98304},
  {"dymn20-train", "bf16", 1, 256, 320, 4608, 2, 0, 0, 2, "y", Route::lds_b16, 7, 3, 2, 0, 72, 94208},
  {"dymn20-train", "dyn_bf16", 128, 320, 1344, 128, 2, 0, 0, 2, "py", Route::lds_b16, 8, 3, 1, 0, 1408, 49152},
  {"dymn20-train", "dyn_bf16", 128, 1344, 224, 504, 2, 0, 0, 2, "py", Route::lds_b16, 7, 3, 1, 0, 512, 47104},
  {"dymn20-train", "bf16", 1, 1344, 256, 4096, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 32, 98304},
  {"dymn20-train", "bf16", 1, 1344, 256, 512, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 16, 98304},
  {"dymn20-train", "bf16", 1, 256, 224, 9088, 2, 0, 0, 2, "y", Route::lds_b16, 7, 3, 2, 0, 80, 94208},
  {"dymn20-train", "dyn_bf16", 128, 224, 1344, 504, 2, 0, 0, 2, "py", Route::lds_b16, 8, 3, 1, 0, 2816, 49152},
  {"dymn20-train", "dyn_bf16", 128, 1344, 224, 504, 2, 0, 0, 2, "pyr", Route::lds_b16, 7, 3, 1, 0, 512, 47104},
  {"dymn20-train", "bf16", 1, 1344, 256, 8064, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 64, 98304},
  {"dymn20-train", "bf16", 1, 1344, 256, 1024, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 16, 98304},
  {"dymn20-train", "dyn_bf16", 128, 224, 960, 504, 2, 0, 0, 2, "py", Route::lds_b16, 8, 3, 1, 0, 2048, 49152},
  {"dymn20-train", "dyn_bf16", 128, 960, 160, 504, 2, 0, 0, 2, "py", Route::lds_b16, 5, 3, 1, 0, 512, 43008},
  {"dymn20-train", "bf16", 1, 960, 240, 8064, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 64, 98304},
  {"dymn20-train", "bf16", 1, 960, 240, 1024, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 16, 98304},
  {"dymn20-train", "bf16", 1, 240, 160, 9088, 2, 0, 0, 2, "y", Route::kstream, 5, 3, 0, 0, 80, 0},
  {"dymn20-train", "dyn_bf16", 128, 160, 368, 504, 2, 0, 0, 2, "py", Route::lds_b16, 8, 3, 1, 0, 768, 49152},
  {"dymn20-train", "dyn_bf16", 128, 368, 160, 504, 2, 0, 0, 2, "pyr", Route::lds_b16, 5, 3, 1, 0, 512, 43008},
  {"dymn20-train", "bf16", 1, 368, 96, 8064, 2, 0, 0, 2, "y", Route::kstream, 6, 3, 0, 0, 32, 0},
  {"dymn20-train", "bf16", 1, 368, 96, 1024, 2, 0, 0, 2, "y", Route::kstream, 6, 3, 0, 0, 8, 0},
  {"dymn20-train", "bf16", 1, 96, 160, 9088, 2, 0, 0, 2, "y", Route::lds_b16, 5, 3, 2, 0, 80, 86016},
  {"dymn20-train", "dyn_bf16", 128, 160, 400, 504, 2, 0, 0, 2, "py", Route::lds_b16, 7, 3, 1, 0, 1024, 47104},
  {"dymn20-train", "dyn_bf16", 128, 400, 160, 504, 2, 0, 0, 2, "pyr", Route::lds_b16, 5, 3, 1, 0, 512, 43008},
  {"dymn20-train", "bf16", 1, 400, 104, 8064, 2, 0, 0, 2, "y", Route::lds_b16, 7, 3, 2, 0, 32, 94208},
  {"dymn20-train", "bf16", 1, 400, 104, 1024, 2, 0, 0, 2, "y", Route::lds_b16, 7, 3, 2, 0, 8, 94208},
  {"dymn20-train", "bf16", 1, 104, 160, 9088, 2, 0, 0, 2, "y", Route::lds_b16, 5, 3, 2, 0, 80, 86016},
  {"dymn20-train", "dyn_bf16", 128, 160, 480, 504, 2, 0, 0, 2, "py", Route::lds_b16, 8, 3, 1, 0, 1024, 49152},
  {"dymn20-train", "dyn_bf16", 128, 480, 80, 2000, 2, 0, 0, 2, "py", Route::lds_b16, 5, 3, 1, 0, 1024, 43008},
  {"dymn20-train", "bf16", 1, 480, 120, 8064, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 32, 98304},
  {"dymn20-train", "bf16", 1, 480, 120, 1024, 2, 0, 0, 2, "y", Route::lds_b16, 8, 3, 2, 0, 8, 98304},
  {"dymn20-train", "bf16", 1, 120, 80, 18048, 2, 0, 0, 2, "y", Route::lds_b16, 5, 3, 2, 0, 72, 86016},
  {"dymn20-train", "dyn_bf16", 128, 80, 240, 2000, 2, 0, 0, 2, "py", Route::lds_b16, 8, 3, 1, 0, 2048, 49152},
  {"dymn20-train", "dyn_bf16", 128, 240, 80, 2000, 2, 0, 0, 2, "pyr", Route::lds_b16, 5, 3, 1, 0, 1024, 43008},
  {"dymn20-train", "bf16", 1, 240, 64, 16000, 2, 0, 0, 2, "y", Route::kstream, 4, 3, 0, 0, 64, 0},
  {"dymn20-train", "bf16", 1, 240, 64, 2048, 2, 0, 0, 2, "y", Route::kstream, 4, 3, 0, 0, 8, 0},
  {"dymn20-train", "bf16", 1, 64, 80, 18048, 2, 0, 0, 2, "y", Route::lds_b16, 5, 3, 2, 0, 72, 86016},
  {"dymn20-train", "dyn_bf16", 128, 80, 144, 2000, 2, 0, 0, 2, "py", Route::lds_b16, 5, 3, 1, 0, 2048, 43008},
  {"dymn20-train", "dyn_bf16", 128, 144, 48, 8000, 2, 0, 0, 2, "py", Route::lds_b16, 3, 3, 2, 0, 4096, 77824},
  {"dymn20-train", "bf16", 1, 144, 64, 16000, 2, 0, 0, 2, "y", Route::lds_b16, 4, 3, 2, 0, 64, 81920},
  {"dymn20-train", "bf16", 1, 144, 64, 2048, 2, 0, 0, 2, "y", Route::lds_b16, 4, 3, 2, 0, 8, 81920},
  {"dymn20-train", "bf16", 1, 64, 48, 36096, 2, 0, 0, 2, "y", Route::lds_b16, 3, 3, 2, 0, 144, 77824},
  {"dymn20-train", "dyn_bf16", 128, 48, 144, 8000, 2, 0, 0, 2, "py", Route::lds_b16, 5, 3, 1, 0, 8192, 43008},
  {"dymn20-train", "dyn_bf16", 128, 144, 48, 8000, 2, 0, 0, 2, "pyr", Route::lds_b16, 3, 3, 2, 0, 4096, 77824},
  {"dymn20-train", "bf16", 1, 144, 64, 32000, 2, 0, 0, 2, "y", Route::lds_b16, 4, 3, 2, 0, 128, 81920},
  {"dymn20-train", "bf16", 1, 144, 64, 4096, 2, 0, 0, 2, "y", Route::lds_b16, 4, 3, 2, 0, 16, 81920},
  {"dymn20-train", "dyn_bf16", 128, 48, 128, 8000, 2, 0, 0, 2, "py", Route::lds_b16, 8, 3, 1, 0, 4096, 49152},
  {"dymn20-train", "dyn_bf16", 128, 128, 32, 32000, 2, 0, 0, 2, "py", Route::lds_b16, 2, 3, 2, 0, 16000, 73728},
  {"dymn20-train", "bf16", 1, 128, 64, 32000, 2, 0, 0, 2, "y", Route::lds_b16, 4, 3, 2, 0, 128, 81920},
  {"dymn20-train", "bf16", 1, 128, 64, 4096, 2, 0, 0, 2, "y", Route::lds_b16, 4, 3, 2, 0, 16, 81920},
  {"dymn20-train", "bf16", 1, 64, 32, 72192, 2, 0, 0, 2, "y", Route::lds_b16, 2, 3, 2, 0, 288, 73728},
  {"dymn20-train", "dyn", 128, 32, 32, 32000, 0, 0, 0, 2, "py", Route::lds_f32, 2, 0, 1, 0, 16000, 36864},
  {"dymn20-train", "fwd", 1, 32, 64, 64000, 0, 0, 0, 2, "y", Route::lds_f32, 4, 0, 1, 0, 256, 40960},
  {"dymn20-train", "fwd", 1, 32, 64, 8192, 0, 0, 0, 2, "y", Route::lds_f32, 4, 0, 1, 0, 32, 40960},
  {"mn10-eval", "bf16", 256, 72, 40, 2000, 2, 0, 0, 2, "ys", Route::lds_b16, 3, 3, 2, 0, 2000, 78336},
  {"mn10-eval", "bf16", 256, 120, 40, 2000, 2, 0, 0, 2, "ysr", Route::lds_b16, 3, 3, 2, 0, 2000, 78336},
  {"mn10-eval", "bf16", 256, 240, 80, 504, 2, 0, 0, 2, "y", Route::kstream, 5, 3, 0, 0, 504, 0},
  {"mn10-eval", "bf16", 256, 200, 80, 504, 2, 0, 0, 2, "yr", Route::kstream, 5, 3, 0, 0, 504, 0},
  {"mn10-eval", "bf16", 256, 184, 80, 504, 2, 0, 0, 2, "yr", Route::kstream, 5, 3, 0, 0, 504, 0},
  {"mn10-eval", "bf16", 256, 480, 112, 504, 2, 0, 0, 2, "ys", Route::lds_b16, 7, 3, 2, 0, 504, 94720},
  {"mn10-eval", "bf16", 256, 672, 112, 504, 2, 0, 0, 2, "ysr", Route::lds_b16, 7, 3, 2, 0, 504, 94720},
  {"mn10-eval", "bf16", 256, 672, 160, 128, 2, 0, 0, 2, "ys", Route::kstream, 5, 3, 0, 0, 256, 0},
  {"mn10-eval", "bf16", 256, 960, 160, 128, 2, 0, 0, 2, "ysr", Route::kstream, 5, 3, 0, 0, 256, 0},
  {"mn10-eval", "bf16", 256, 160, 960, 128, 2, 0, 0, 2, "o", Route::lds_b16, 8, 3, 1, 0, 1024, 49152},
  {"dymn20-eval", "dyn", 128, 32, 32, 32000, 0, 0, 0, 2, "pyr", Route::lds_f32, 2, 0, 1, 0, 16000, 36864},
  {"dymn20-eval", "dyn", 128, 32, 128, 32000, 0, 0, 0, 2, "py", Route::lds_f32, 8, 0, 1, 0, 16000, 49152},
  {"dymn20-eval", "dyn", 128, 128, 48, 8000, 0, 0, 0, 2, "py", Route::lds_f32, 3, 0, 1, 0, 4096, 58368},
  {"dymn20-eval", "dyn", 128, 48, 144, 8000, 0, 0, 0, 2, "py", Route::lds_f32, 5, 0, 1, 0, 8192, 64512},
  {"dymn20-eval", "dyn", 128, 144, 48, 8000, 0, 0, 0, 2, "pyr", Route::lds_f32, 3, 0, 1, 0, 4096, 58368},
  {"dymn20-eval", "dyn", 128, 144, 80, 2000, 0, 0, 0, 2, "py", Route::lds_f32, 5, 0, 1, 0, 1024, 64512},
  {"dymn20-eval", "dyn", 128, 80, 240, 2000, 0, 0, 0, 2, "py", Route::lds_f32, 8, 0, 1, 0, 2048, 73728},
  {"dymn20-eval", "dyn", 128, 240, 80, 2000, 0, 0, 0, 2, "pyr", Route::lds_f32, 5, 0, 1, 0, 1024, 64512},
  {"dymn20-eval", "dyn", 128, 80, 480, 2000, 0, 0, 0, 2, "py", Route::lds_f32, 8, 0, 1, 0, 4096, 73728},
  {"dymn20-eval", "dyn", 128, 480, 160, 504, 0, 0, 0, 2, "py", Route::lds_f32, 5, 0, 1, 0, 512, 64512},
  {"dymn20-eval", "dyn", 128, 160, 400, 504, 0, 0, 0, 2, "py", Route::lds_f32, 7, 0, 1, 0, 1024, 70656},
  {"dymn20-eval", "dyn", 128, 400, 160, 504, 0, 0, 0, 2, "pyr", Route::lds_f32, 5, 0, 1, 0, 512, 64512},
  {"dymn20-eval", "dyn", 128, 160, 368, 504, 0, 0, 0, 2, "py", Route::lds_f32, 8, 0, 1, 0, 768, 73728},
  {"dymn20-eval", "dyn", 128, 368, 160, 504, 0, 0, 0, 2, "pyr", Route::lds_f32, 5, 0, 1, 0, 512, 64512},
  {"dymn20-eval", "dyn", 128, 160, 960, 504, 0, 0, 0, 2, "py", Route::lds_f32, 8, 0, 1, 0, 2048, 73728},
  {"dymn20-eval", "dyn", 128, 960, 224, 504, 0, 0, 0, 2, "py", Route::lds_f32, 7, 0, 1, 0, 512, 70656},
  {"dymn20-eval", "dyn", 128, 224, 1344, 504, 0, 0, 0, 2, "py", Route::lds_f32, 8, 0, 1, 0, 2816, 73728},
  {"dymn20-eval", "dyn", 128, 1344, 224, 504, 0, 0, 0, 2, "pyr", Route::lds_f32, 7, 0, 1, 0, 512, 70656},
  {"dymn20-eval", "dyn", 128, 1344, 320, 128, 0, 0, 0, 2, "py", Route::lds_f32, 7, 0, 1, 0, 384, 70656},
  {"dymn20-eval", "dyn", 128, 320, 1920, 128, 0, 0, 0, 2, "py", Route::lds_f32, 8, 0, 1, 0, 1920, 73728},
  {"dymn20-eval", "dyn", 128, 1920, 320, 128, 0, 0, 0, 2, "pyr", Route::lds_f32, 7, 0, 1, 0, 384, 70656},
  {"dymn20-eval", "fwd", 128, 320, 1920, 128, 0, 0, 0, 2, "o", Route::lds_f32, 8, 0, 1, 0, 960, 73728},
};

static PwKey make_key(int B, int Ci, int Co, int S, int pack, int c1, int ci_x, const char* flags) {
  PwKey k{};
  auto has = [&](char c) { return strchr(flags, c) != nullptr; };
  k.B = B; k.Ci = Ci; k.Co = Co; k.S = S; k.ci_x = ci_x ? ci_x : Ci; k.c1 = c1;
  k.x_store = has('x') ? Store::b16 : Store::f32; k.y_store = has('w') ? Store::b16 : Store::f32;
  k.pack = (Pack)pack; k.per_sample = has('p'); k.operands = true;
  k.y = has('y'); k.scale = has('s'); k.res = has('r'); k.pool = has('o'); k.tf = has('t'); k.stats = has('a'); k.gstat = has('g');
  return k;
}

static long long n_bad = 0;
static void bad_row(const Row& r, const char* what, long long got, long long want) {
  if (++n_bad <= 20) printf("TABLE %s (%s %s B=%d Ci=%d Co=%d S=%d flags=%s): got %lld, recorded %lld\n", what, r.src, r.entry, r.B, r.Ci, r.Co, r.S, r.flags, got, want);
}
static void check_table() {
  for (const Row& r : kTable) {
    const PwKey k = make_key(r.B, r.Ci, r.Co, r.S, r.pack, r.c1, r.ci_x, r.flags);
    if (const char* why = check(k)) { ++n_bad; printf("TABLE row refused (%s %s): %s\n", r.src, r.entry, why); continue; }
    const PwPlan p = plan(k, r.mode);
    if (p.route != r.route) { bad_row(r, "route", (int)p.route, (int)r.route); continue; }
    if (r.route == Route::none) continue;
    const long long blocks = (long long)p.grid[0] * p.grid[1] * p.grid[2];
    if (blocks != r.blocks) bad_row(r, "grid blocks", blocks, r.blocks);
    if (p.lds_bytes != r.lds) bad_row(r, "dynamic LDS", p.lds_bytes, r.lds);
    if (r.route == Route::generic) continue;
    if (r.mtw && p.mtw != r.mtw) bad_row(r, "MTW", p.mtw, r.mtw);
    if (p.nprod != r.nprod) bad_row(r, "NPROD", p.nprod, r.nprod);
    const int var = r.route == Route::lds_b16 ? p.n_stages : r.route == Route::lds_f32 ? (int)p.pipe : r.route == Route::expand ? p.n_chunks : 0;
    if (var != r.var) bad_row(r, "NSTG / PIPE / NCH", var, r.var);
    if ((r.route == Route::lds_b16 || r.route == Route::lds_f32) && (int)p.tf != r.tf) bad_row(r, "TF", p.tf, r.tf);
  }
}

// ---- check(): one request per shared rule that must be refused (the per-entry-point rules and the entry points' own rows are in
// tests/test_pw_fwd_plan_cpu.py, against the library); the acceptances are the rows of the table above
static void check_rules() {
  struct Rule { const char* what; PwKey k; };
  const PwKey ok = make_key(2, 32, 24, 64, 2, 0, 0, "y");
  auto with = [&](auto f) { PwKey k = ok; f(k); return k; };
  const Rule rules[] = {
    {"operands", with([](PwKey& k) { k.operands = false; })},
    {"no output", with([](PwKey& k) { k.y = false; })},
    {"B", with([](PwKey& k) { k.B = 0; })}, {"Co", with([](PwKey& k) { k.Co = 0; })}, {"S", with([](PwKey& k) { k.S = 0; })},
    {"Ci < 4", with([](PwKey& k) { k.Ci = k.ci_x = 0; })}, {"Ci % 4", with([](PwKey& k) { k.Ci = k.ci_x = 30; })},
    {"act", with([](PwKey& k) { k.act = 3; })}, {"tf_act", with([](PwKey& k) { k.tf_act = -1; })}, {"gs_act", with([](PwKey& k) { k.gs_act = 3; })},
    {"tf half", with([](PwKey& k) { k.tf_half = true; })}, {"tf Ci % 8", with([](PwKey& k) { k.tf = true; k.Ci = k.ci_x = 36; })},
    {"tf S % 4", with([](PwKey& k) { k.tf = true; k.S = 15; })},
    {"gstat without partials", with([](PwKey& k) { k.gstat = true; })},
    {"bf16 storage, split pack", with([](PwKey& k) { k.x_store = Store::b16; })},
    {"bf16 storage, fp32 pack", with([](PwKey& k) { k.y_store = Store::b16; k.pack = Pack::f32; })},
    {"tf into a bf16 output of an fp32 input", with([](PwKey& k) { k.pack = Pack::b16; k.y_store = Store::b16; k.tf = true; })},
    {"c1 % 4", with([](PwKey& k) { k.c1 = 6; })}, {"c1 leaves nothing", with([](PwKey& k) { k.c1 = 32; })},
    {"c1 % 32 of a bf16 source", with([](PwKey& k) { k.pack = Pack::b16; k.x_store = Store::b16; k.Ci = k.ci_x = 40; k.c1 = 16; })},
    {"two sources S % 4", with([](PwKey& k) { k.c1 = 8; k.S = 15; })},
    {"K-concat ci_x % 32", with([](PwKey& k) { k.Ci = 64; k.ci_x = 16; k.scale = true; })},
    {"K-concat whole banks", with([](PwKey& k) { k.Ci = 80; k.ci_x = 32; k.scale = true; })},
    {"K-concat without scale", with([](PwKey& k) { k.Ci = 64; k.ci_x = 32; })},
    {"K-concat fp32 pack", with([](PwKey& k) { k.Ci = 64; k.ci_x = 32; k.scale = true; k.pack = Pack::f32; })},
    {"K-concat S % 4", with([](PwKey& k) { k.Ci = 64; k.ci_x = 32; k.scale = true; k.S = 15; })},
    {"bf16 storage S % 4", with([](PwKey& k) { k.pack = Pack::b16; k.y_store = Store::b16; k.S = 15; })},
    {"32-bit column index", with([](PwKey& k) { k.B = 70000; k.S = 32768; })},
  };
  if (check(ok)) { ++n_bad; printf("RULE the base request is refused: %s\n", check(ok)); }
  for (const Rule& r : rules)
    if (!check(r.k)) { ++n_bad; printf("RULE %s: accepted\n", r.what); }
  // the same 2^31 columns are fine for the fp32 kernel (64-bit column index), and S % 4 != 0 with statistics answers 1
  if (check(with([](PwKey& k) { k.B = 70000; k.S = 32768; k.pack = Pack::f32; }))) { ++n_bad; printf("RULE fp32 pack, 2^31 columns: refused\n"); }
  const PwKey st = with([](PwKey& k) { k.S = 15; k.stats = true; k.tf = true; });
  if (check(st) || plan(st, 2).route != Route::none) { ++n_bad; printf("RULE statistics at S %% 4 != 0 answer 1\n"); }
}

// ---- structure over a grid ----------------------------------------------------------------------------------------------------
static long long n_plans = 0, n_refused = 0, n_route[6] = {0, 0, 0, 0, 0, 0};
static void need(bool ok, const char* what, const PwKey& k, int mode) {
  if (ok) return;
  if (++n_bad <= 20)
    printf("VIOLATION %s: B=%d Ci=%d Co=%d S=%d ci_x=%d c1=%d pack=%d x16=%d y16=%d per_sample=%d y=%d scale=%d res=%d pool=%d tf=%d stats=%d gstat=%d mode=%d\n",
           what, k.B, k.Ci, k.Co, k.S, k.ci_x, k.c1, (int)k.pack, (int)k.x_store, (int)k.y_store, k.per_sample, k.y, k.scale, k.res, k.pool,
           k.tf, k.stats, k.gstat, mode);
}
static void check_plan(const PwKey& k, int mode) {
  if (check(k)) { ++n_refused; return; }
  const PwPlan p = plan(k, mode);
  ++n_plans; ++n_route[(int)p.route];
  need(p.MT == (k.Co + 15) / 16, "m-tiles", k, mode);
  if (k.S % 4 != 0) {
    need(p.route == (k.stats ? Route::none : Route::generic), "plane sizes off the 16-byte grid", k, mode);
    need(p.route == Route::none || (p.grid[0] * 64 >= (unsigned)k.S && p.grid[1] == (unsigned)p.MT && p.grid[2] == (unsigned)k.B), "generic grid", k, mode);
    need(k.per_sample == (p.wp_bstride != 0) || p.route == Route::none, "generic per-sample stride", k, mode);
    return;
  }
  need(p.route != Route::none && p.route != Route::generic, "a 16-byte plane gets an MFMA kernel", k, mode);
  need(p.route != Route::lds_f32 || k.pack == Pack::f32, "fp32 kernel, fp32 pack", k, mode);
  need(p.route == Route::lds_f32 || k.pack != Pack::f32, "bf16 kernels, bf16 packs", k, mode);
  need(p.n_tiles == stat_tiles(k.B, k.S, k.per_sample) && p.n_tiles >= 1, "column tiles", k, mode);
  need((long long)p.n_tiles * kTileN >= (long long)k.B * k.S, "column tiles cover B x S", k, mode);
  need(p.grid[0] == (unsigned)((p.n_tiles + 7) / 8 * 8 * p.MC) && p.grid[1] == 1 && p.grid[2] == 1, "grid", k, mode);
  const int max_mtw = p.route == Route::kstream ? 6 : p.route == Route::expand ? 64 : 8;
  need(p.mtw >= 1 && p.mtw <= max_mtw, "the instance exists", k, mode);
  need(p.MC >= 1 && p.MC * p.mtw >= p.MT, "row chunks cover the m-tiles", k, mode);
  need((p.MC - 1) * p.mtw < p.MT, "no empty row chunk", k, mode);
  need(p.lds_bytes >= 0 && p.lds_bytes <= kLdsLimit, "LDS", k, mode);
  need(k.scale ? (p.NS >= 1 && p.NS <= k.B) : p.NS == 0, "scale samples per tile", k, mode);
  need(k.ci_x == k.Ci || k.ci_x % 32 == 0, "K-concat chunks stay inside a bank", k, mode);
  const bool streamed = p.route == Route::expand || p.route == Route::kstream;
  need(!streamed || (mode != 0 && k.x_store == Store::f32 && k.y_store == Store::f32 && !k.per_sample && !k.tf && k.c1 == 0 && !k.stats),
       "streaming kernels take plain fp32 -> fp32 convs", k, mode);
  if (p.route == Route::expand) {
    need(p.n_chunks >= 1 && p.n_chunks <= 4 && p.n_chunks * kKC >= k.Ci, "expand chunks", k, mode);
    need(!k.scale && !k.res && !k.pool && k.y && k.ci_x == k.Ci && (mode & kStreamExpand), "expand: no scale / res / pool, a y", k, mode);
  }
  if (p.route == Route::kstream) need(k.ci_x != k.Ci ? (mode & kStreamKcat) != 0 : (mode & (kStreamProject | kStreamRest)) != 0, "kstream mode bits", k, mode);
  if (p.route == Route::lds_f32) {
    need(!p.pipe || (kPipeKC * p.NS <= 64 && p.NS <= 4 && p.kc == kPipeKC && p.n_stages >= 1 && p.n_stages <= 3), "pipelined ring", k, mode);
    need(p.pipe || (p.kc % 4 == 0 && p.kc >= 4 && p.kc <= kKC && p.n_stages >= 1 && p.n_stages <= 2), "two-stage fallback", k, mode);
    need(p.n_chunks * p.kc >= k.Ci && (p.n_chunks - 1) * p.kc < k.Ci, "k chunks", k, mode);
    need(!k.stats || p.lds_bytes >= 10 * p.mtw * 16 * 4, "room for the wave partials", k, mode);
  }
  if (p.route == Route::lds_b16) {
    need(p.n_stages == 1 || p.n_stages == 2, "stages", k, mode);
    need(k.scale ? (p.sc_bytes % 256 == 0 && p.sc_bytes >= kKC * p.NS * 4) : p.sc_bytes == 0, "scale bytes", k, mode);
    need(p.nprod == (k.pack == Pack::b16x2 ? 3 : 1), "NPROD", k, mode);
  }
}

int main() {
  check_table();
  check_rules();
  const int Bs[] = {1, 2, 6, 256};
  const int Cs[] = {4, 8, 12, 16, 20, 24, 32, 40, 48, 64, 72, 100, 112, 128, 136, 160, 184, 240, 320, 480, 672, 960, 1030, 1920, 6, 18, 30};
  const int Ss[] = {8, 15, 16, 60, 128, 504, 2000};
  const int modes[] = {0, 1, 2, 3, 4, 8, 10, 15};
  for (int B : Bs) for (int Co : Cs) for (int Ci : Cs) for (int S : Ss) {
    // eat_pw_conv_fwd / _bf16_fwd: every pack, scale / res / pool / y
    for (int pack = 0; pack < 3; ++pack) for (int f = 0; f < 16; ++f) {
      char fl[8]; int n = 0;
      for (int b = 0; b < 4; ++b)
        if (f & (1 << b)) fl[n++] = "sroy"[b];
      fl[n] = 0;
      for (int mode : modes) { check_plan(make_key(B, Ci, Co, S, pack, 0, 0, fl), mode); if (pack == 0) break; }
    }
    for (int pack = 0; pack < 3; ++pack) {
      // _tf_fwd, _cat_fwd, _dyn_fwd / _dyn_bf16_fwd, _stats_fwd, _gstats_fwd
      for (const char* fl : {"yt", "yts", "ytr", "ytsr"}) check_plan(make_key(B, Ci, Co, S, pack, 0, 0, fl), 2);
      for (int c1 : {4, 8, 32, Ci / 2}) for (const char* fl : {"y", "yr"}) check_plan(make_key(B, Ci, Co, S, pack, c1, 0, fl), 2);
      if (pack != 1) for (const char* fl : {"yp", "ypr"}) check_plan(make_key(B, Ci, Co, S, pack, 0, 0, fl), 2);
      for (const char* fl : {"ya", "yas", "yat", "yats", "yap"}) check_plan(make_key(B, Ci, Co, S, pack, 0, 0, fl), 2);
      if (pack != 1) check_plan(make_key(B, Ci, Co, S, pack, 0, 0, "yag"), 2);
    }
    // _kcat_fwd: nbank banks of Ci channels
    for (int nbank : {1, 2, 4}) for (const char* fl : {"ys", "ysr"}) for (int mode : {2, 10})
      check_plan(make_key(B, nbank * Ci, Co, S, 2, 0, Ci, fl), mode);
    // _b16_fwd and _dyn_b16_fwd: plain bf16 pack, the storage combinations
    for (const char* fl : {"yw", "yx", "yxr", "yxa", "yxta", "yxsa", "yxtsa", "yxw", "yxwa", "yxwag", "yxwtsa", "ypw", "ypwa", "ypx", "ypxr", "ypxa"})
      check_plan(make_key(B, Ci, Co, S, 1, 0, 0, fl), 2);
    for (int c1 : {32, 64}) check_plan(make_key(B, Ci, Co, S, 1, c1, 0, "yxr"), 2);
  }
  printf("%zu table rows; %lld plans, %lld refused requests, %lld violations (routes none/generic/lds_f32/lds_b16/expand/kstream: %lld %lld %lld %lld %lld %lld)\n",
         sizeof(kTable) / sizeof(kTable[0]), n_plans, n_refused, n_bad, n_route[0], n_route[1], n_route[2], n_route[3], n_route[4], n_route[5]);
  return n_bad != 0;
}
