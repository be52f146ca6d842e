// Stand-alone check of efficientat_amd/csrc/event_bank.h (built and run by tests/test_event_bank_cpu.py with a host compiler
// and -fsanitize=address,undefined): the slot refusals, the clamp of a clip's event rows and the class walk against brute
// force on small banks.  Every table is a heap array of exactly the size its contract promises, so a read outside one is an
// AddressSanitizer error, not a wrong value.  Exit status 0 = no violation.
#include <cstdio>
#include <cstring>
#include <vector>
#include "event_bank.h"

static long long n_checks = 0, n_bad = 0;
static void need(bool ok, const char* what, long long a = 0, long long b = 0, long long c = 0, long long d = 0) {
  ++n_checks;
  if (ok) return;
  if (++n_bad <= 20) printf("VIOLATION %s (%lld, %lld, %lld, %lld)\n", what, a, b, c, d);
}

// an exact-size heap copy (NULL for no element: what the wrappers pass for an empty event table)
template <class T>
static T* heap(const std::vector<T>& v) {
  if (v.empty()) return nullptr;
  T* p = new T[v.size()];
  memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}

// ---- clip_window: i in {-2, -1, 0, n_bank - 1, n_bank}, st in {-1, 0, len - 1, len}, len in {0, 1, L - 1, L, L + 1}
static void check_windows(int L) {
  const std::vector<int> lens = {0, 1, L - 1, L, L + 1};
  const long long n_bank = (long long)lens.size();
  int* lengths = heap(lens);
  for (int i = -2; i <= n_bank; ++i) {
    const bool in = i >= 0 && i < n_bank;
    const int len = in ? lens[i] : 0;
    for (int st : {-1, 0, len - 1, len, len + 1}) {
      const eat::ClipWindow q = eat::clip_window(lengths, n_bank, L, i, st);
      const bool ok = in && len >= 1 && st >= 0 && st < len;
      need(q.ok == ok, "clip_window refusal", L, i, st, len);
      if (ok) {
        int w = 0;                                            // the samples of [st, st + L) that the clip has
        for (int p = st; p < st + L; ++p) w += p < len ? 1 : 0;
        need(q.len == len && q.w == w && q.w >= 1 && q.w <= L, "clip_window length and width", L, i, st, q.w);
      }
    }
  }
  delete[] lengths;
}

// ---- event tables.  Rows (class, onset, offset), each clip's run sorted by (class, onset); K = 4 classes.
static const int K = 4;
static const std::vector<int> kRows = {
    2, 0, 4,  2, 4, 8,  2, 10, 12,                           // clip 0: one class holds all rows
    0, 2, 5,  3, 5, 9,                                       // clip 1: the first and the last class, one row each
                                                             // clip 2: no row
    0, 0, 3,  0, 3, 6,  1, 6, 7,  3, 1, 2,  3, 8, 20,        // clip 3
    1, 5, 6,                                                 // clip 4: one row
};

static bool sorted_run(const int* ev, long long e0, long long e1) {
  for (long long e = e0 + 1; e < e1; ++e)
    if (ev[3 * e] < ev[3 * (e - 1)] || (ev[3 * e] == ev[3 * (e - 1)] && ev[3 * e + 1] < ev[3 * (e - 1) + 1])) return false;
  return true;
}

static void check_rows(const std::vector<int>& rows, const std::vector<long long>& offs, bool expect_sorted) {
  const long long n_events = (long long)rows.size() / 3, n_bank = (long long)offs.size() - 1;
  int* ev = heap(rows);
  long long* eo = heap(offs);
  for (int i = 0; i < n_bank; ++i) {
    const eat::EventRows r = eat::event_rows(eo, n_events, i);
    need(r.e0 >= 0 && r.e0 <= r.e1 && r.e1 <= n_events, "event_rows inside the table", i, r.e0, r.e1, n_events);
    const bool plain = offs[i] >= 0 && offs[i] <= offs[i + 1] && offs[i + 1] <= n_events;
    if (plain) need(r.e0 == offs[i] && r.e1 == offs[i + 1], "event_rows of a sound table", i, r.e0, r.e1);
    const bool sorted = sorted_run(ev, r.e0, r.e1);
    if (expect_sorted) need(sorted, "the fixture's runs are sorted", i);
    for (int c = -1; c <= K; ++c) {
      const long long f = eat::first_row_of_class(ev, r.e0, r.e1, c);
      need(f >= r.e0 && f <= r.e1, "first_row_of_class inside the run", i, c, f);
      if (sorted) {
        long long want = r.e0;
        while (want < r.e1 && ev[3 * want] < c) ++want;
        need(f == want, "first_row_of_class", i, c, f, want);
      }
      for (long long lo = -1; lo <= 21; ++lo)
        for (long long hi = lo; hi <= 22; ++hi) {             // (hi == lo: an empty window meets nothing)
          const int got = eat::class_run_overlaps(ev, r.e0, r.e1, c, lo, hi);
          if (!sorted) continue;
          int want = 0;
          for (long long e = r.e0; e < r.e1; ++e) want |= ev[3 * e] == c && ev[3 * e + 1] < hi && ev[3 * e + 2] > lo;
          need(got == want, "class_run_overlaps", i, c, lo, hi);
        }
    }
  }
  delete[] ev;
  delete[] eo;
}

// rows that touch the window's edge without overlapping it, spelled out (clip 4 holds the one row (1, 5, 6))
static void check_edges() {
  int* ev = heap(kRows);
  const long long e0 = 10, e1 = 11;
  need(eat::class_run_overlaps(ev, e0, e1, 1, 5, 6) == 1, "the row itself");
  need(eat::class_run_overlaps(ev, e0, e1, 1, 6, 9) == 0, "offset == window start");
  need(eat::class_run_overlaps(ev, e0, e1, 1, 3, 5) == 0, "onset == window end");
  need(eat::class_run_overlaps(ev, e0, e1, 1, 5, 5) == 0, "empty window");
  need(eat::class_run_overlaps(ev, e0, e1, 0, 5, 6) == 0 && eat::class_run_overlaps(ev, e0, e1, 2, 5, 6) == 0, "other classes");
  delete[] ev;
}

int main() {
  for (int L : {2, 3, 8}) check_windows(L);
  check_rows(kRows, {0, 3, 5, 5, 10, 11}, true);
  check_rows(kRows, {-3, 3, 5, 5, 10, 11}, false);           // a negative row
  check_rows(kRows, {0, 5, 3, 3, 11, 10}, false);            // descending
  check_rows(kRows, {0, 3, 5, 5, 10, 99}, false);            // beyond n_events
  check_rows(kRows, {-7, 99, -1, 50, 12, 11}, false);
  check_rows({}, {0, 0, 0}, true);                           // n_events = 0, events NULL
  check_rows({}, {-1, 4, 2}, false);
  check_edges();
  printf("%lld checks, %lld violations\n", n_checks, n_bad);
  return n_bad == 0 ? 0 : 1;
}
