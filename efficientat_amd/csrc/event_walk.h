// The detector's events of one timeline at 64 threshold pairs, one pair per lane of a single wavefront: the walk that
// event_score.hip and psds.hip share.  Steps 1-3 of eat_detect_events (include/eat_detect.h) - runs of x >= lo that reach
// hi, runs at most max_gap frames apart merged, merged events shorter than min_len dropped - with every final event
// handed to `emit(on, off)` (frames, exclusive offset) in onset order, the moment no later frame can change it.
//
// The timeline is loaded 64 frames at a time with one coalesced load and handed round by lane broadcast.  A frame below
// every lane's lo that follows such a frame changes no lane's state: the ballot finds the others and only they are
// walked (wave-uniform).  The block must be ONE wavefront of 64 lanes; a lane without a pair passes hi = lo = +inf,
// never sees an active frame and never emits.
#pragma once
#include <hip/hip_runtime.h>
#include "event_bank.h"

namespace eat {

template <class Emit>
__device__ __forceinline__ void event_walk(const float* __restrict__ x, int G, float hi, float lo, int max_gap, int min_len,
                                           Emit&& emit) {
  const int lane = threadIdx.x;
  float lo_min = lo;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lo_min = fminf(lo_min, __shfl_xor(lo_min, o, 64));

  bool open = false, hit = false, cur = false;             // a run in progress; it has reached hi; a pending event
  int rs = 0, cur_on = 0, cur_off = 0;

  auto final_event = [&](int on, int off) {
    if (off - on >= min_len) emit(on, off);
  };
  auto close_run = [&](int re) {                           // the run [rs, re) ends
    if (hit) {
      if (cur && rs - cur_off <= max_gap) {
        cur_off = re;
      } else {
        if (cur) final_event(cur_on, cur_off);
        cur = true;
        cur_on = rs;
        cur_off = re;
      }
    }
    open = false;
  };

  unsigned long long carry = 0;                            // the last frame of the step before was active in some lane
  for (int t0 = 0; t0 < G; t0 += 64) {
    const int t = t0 + lane;
    const float val = t < G ? x[t] : 0.0f;
    const unsigned long long inside = G - t0 >= 64 ? ~0ULL : (1ULL << (G - t0)) - 1;
    const unsigned long long M = __ballot(t < G && val >= lo_min);
    unsigned long long todo = (M | (M << 1) | carry) & inside;
    carry = M >> 63;
    while (todo != 0) {
      const int j = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const float f = __shfl(val, j, 64);
      if (f >= lo) {
        if (!open) {
          open = true;
          hit = false;
          rs = t0 + j;
        }
        if (f >= hi) hit = true;
      } else if (open) {
        close_run(t0 + j);
      }
    }
  }
  if (open) close_run(G);
  if (cur) final_event(cur_on, cur_off);
}

}  // namespace eat
