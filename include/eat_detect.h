/* eat_detect.h -- C ABI of sound event detection in libeat_hip.so (efficientat_amd/detection.py, csrc/detect.hip):
 * what DCASE-style post-processing does on the host with scipy.ndimage.median_filter and a Python loop over classes --
 * stitch overlapping windows of frame-level logits into one probability timeline per recording, median-filter it,
 * binarise it with two thresholds and list the events -- as four launches over all recordings and classes at once.
 *
 * A further header of the same library with the conventions of eat_hip.h: every pointer is a DEVICE pointer, fp32
 * unless noted, the caller owns every buffer, work is enqueued on `stream` with no hidden synchronisation, the
 * return value is EAT_OK or a negative EAT_E* code, and eat_last_error_string() holds the message.  No atomics:
 * every kernel stores every element of its outputs and gives the same bits from call to call.
 *
 * The recording table `rec` (n_rec, 4) int32 holds per recording (first window, window count, goff, G): its windows
 * are rows [first, first + count) of p, its G >= 1 frames are columns [goff, goff + G) of the (K, G_total) timelines.
 * The caller guarantees goff[0] = 0, goff[i + 1] = goff[i] + G[i] and goff[n_rec - 1] + G[n_rec - 1] = G_total
 * (the kernels find a column's recording by bisection over goff), and that every window row lies inside p.
 */
#ifndef EAT_DETECT_H
#define EAT_DETECT_H
#include "eat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- stitch: overlapping windows of frame logits -> one probability timeline per recording ------------------
 * p (n_w, K, Tp) logits, columns [T, Tp) of a row are padding and never read.  Column j of the recording's window
 * q is its frame q Hf + j.  prob (K, G_total):
 *   prob[k, goff + g] = sum_q wt[j] s(p[first + q, k, j]) / sum_q wt[j],  j = g - q Hf,
 * over the recording's windows q (ascending) with 0 <= j < T; s(v) = 1 / (1 + exp(-v)) in fp32, the sigmoid of
 * eat_tag_topk.  wt (T) > 0.  A frame that no window covers is stored as 0 (the caller's plan covers every frame).
 * No column with q Hf + j >= G is read.  Lanes run along g.  All index arithmetic is 64-bit.
 * EAT_EINVAL: n_w, K, n_rec, T, Hf or G_total < 1, Tp < T, Hf > T, a missing operand. */
int eat_detect_stitch(const float* p, int n_w, int K, int Tp, const int* rec, int n_rec, int Hf, int T, const float* wt,
                      float* prob, int G_total, eat_stream_t stream);

/* ---- running median along time, per class and per recording ------------------------------------------------
 * filt[k, goff + i] = the median of the m samples prob[k, goff + r(i + d)], d = -(m / 2) .. m / 2, with periodic
 * reflection at the recording's own ends: u = j mod 2 G (non-negative), r(j) = u if u < G, else 2 G - 1 - u.
 * That is scipy.ndimage.median_filter(mode="reflect") wherever m / 2 <= G; nothing is read across a recording
 * boundary.  m odd, 1 <= m <= 31; m = 1 is a copy.  The median is a selection (rank by counting, ties by position):
 * the result carries the bits of one input sample.  Inputs must not be NaN.  filt must not overlap prob.
 * EAT_EINVAL: K, n_rec or G_total < 1, an even m or one outside [1, 31], a missing operand, filt == prob. */
int eat_detect_median(const float* prob, int K, int G_total, const int* rec, int n_rec, int m, float* filt,
                      eat_stream_t stream);

/* ---- events: double-threshold binarisation of every (recording, class) timeline ----------------------------
 * Timeline (i, k) is filt[k, goff_i .. goff_i + G_i), thresholds 0 < lo[k] <= hi[k].
 *   1. a run is a maximal set of consecutive frames with v >= lo[k]; it counts if one of its frames has v >= hi[k];
 *   2. counting runs with at most max_gap frames between the end of one and the start of the next are merged, the
 *      frames between them (below lo, or a run that does not count) become part of the event;
 *   3. merged events shorter than min_len frames are dropped.
 * eat_detect_events_count stores the number of events of timeline i K + k in count[i K + k] (int64).  The caller
 * turns count into its INCLUSIVE prefix sum `incl` (int64, same layout), reads the total E = incl[n_rec K - 1] and,
 * if E > 0, calls eat_detect_events_write, which stores event e of the order (recording, class, onset):
 *   ev_i[e] = (recording, class, onset, offset) int32, frames [onset, offset) of the recording;
 *   ev_f[e] = (peak, mean) fp32 of filt over [onset, offset): the maximum, and the fp64 sum taken in time order,
 *             divided by the length in fp64 and rounded once.
 * One wavefront per timeline, 64 frames per step.  max_gap >= 0, min_len >= 0.
 * EAT_EINVAL: K, n_rec or G_total < 1, max_gap or min_len < 0, n_rec K > 2^31 - 1, a missing operand. */
int eat_detect_events_count(const float* filt, int K, int G_total, const int* rec, int n_rec, const float* hi,
                            const float* lo, int max_gap, int min_len, long long* count, eat_stream_t stream);
int eat_detect_events_write(const float* filt, int K, int G_total, const int* rec, int n_rec, const float* hi,
                            const float* lo, int max_gap, int min_len, const long long* incl, int* ev_i, float* ev_f,
                            eat_stream_t stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* EAT_DETECT_H */
