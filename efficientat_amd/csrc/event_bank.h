// The slot refusals and event-row walks of a ragged clip bank, written once: what "nothing outside the bank is read" rests
// on.  Compiles for the host alone too (tests/event_bank_check.cpp, under AddressSanitizer): no device-only overloads.
// lengths holds n_bank entries, eo n_bank + 1, ev n_events rows (class, onset, offset); ev may be NULL when n_events is 0.
#pragma once

#ifdef __HIPCC__
#define EAT_BANK_FN __host__ __device__ __forceinline__
#else
#define EAT_BANK_FN inline
#endif

namespace eat {

struct ClipWindow { int len, w; bool ok; };     // the clip's length; samples of it in the window: min(len - st, L)

// Clip i cropped at st into L samples.  Refused (ok = false): i outside [0, n_bank), len < 1, st outside [0, len).
EAT_BANK_FN ClipWindow clip_window(const int* __restrict__ lengths, long long n_bank, int L, int i, int st) {
  ClipWindow q{0, 0, false};
  if (i < 0 || i >= n_bank) return q;
  const int len = lengths[i];
  if (len < 1 || st < 0 || st >= len) return q;
  q.len = len;
  q.w = len - st < L ? len - st : L;
  q.ok = true;
  return q;
}

struct EventRows { long long e0, e1; };         // [e0, e1), inside [0, n_events] and not descending

// the event rows of clip i (0 <= i < n_bank), clipped to the table
EAT_BANK_FN EventRows event_rows(const long long* __restrict__ eo, long long n_events, int i) {
  const long long a = eo[i], b = eo[i + 1];
  EventRows r;
  r.e0 = a < 0 ? 0 : (a > n_events ? n_events : a);
  r.e1 = b < r.e0 ? r.e0 : (b > n_events ? n_events : b);
  return r;
}

// the first row of [a, b), sorted by (class, onset), whose class is not below cls: a bisection that reads rows of [a, b) only
EAT_BANK_FN long long first_row_of_class(const int* __restrict__ ref, long long a, long long b, int cls) {
  long long l = a, h = b;
  while (l < h) {
    const long long m = (l + h) >> 1;
    if (ref[3 * m] < cls) l = m + 1; else h = m;
  }
  return l;
}

// 1 iff pred(onset, offset) holds for a row of class c among the sorted rows [e0, e1); the walk stops at the first hit
template <class Pred>
EAT_BANK_FN int any_row_of_class(const int* __restrict__ ev, long long e0, long long e1, int c, Pred&& pred) {
  for (long long e = first_row_of_class(ev, e0, e1, c); e < e1; ++e) {
    if (ev[3 * e] != c) break;
    if (pred((long long)ev[3 * e + 1], (long long)ev[3 * e + 2])) return 1;
  }
  return 0;
}

// 1 iff an event of class c among the sorted rows [e0, e1) meets the samples [lo, hi); touching an edge is no overlap
EAT_BANK_FN int class_run_overlaps(const int* __restrict__ ev, long long e0, long long e1, int c, long long lo, long long hi) {
  return any_row_of_class(ev, e0, e1, c, [=](long long on, long long off) { return on < hi && off > lo; });
}

}  // namespace eat
