/* eat_event_score.h -- C ABI of event-based (collar) scoring of a sound event detector in libeat_hip.so
 * (efficientat_amd/sed.py: evaluate_events, csrc/event_score.hip): for a whole grid of threshold pairs at once, form the
 * detector's events of every (recording, class) timeline by the rule of eat_detect_events (eat_detect.h), match them to
 * reference events with onset / offset collars and store integer counts.  The estimated events never exist in memory.
 *
 * A further header of the same library with the conventions of eat_hip.h: every pointer is a DEVICE pointer, the caller
 * owns every buffer, work is enqueued on `stream` with no hidden synchronisation (capture-safe), the return value is
 * EAT_OK or a negative EAT_E* code, and eat_last_error_string() holds the message.  No atomics: every element of the
 * output is stored and the same inputs give the same bits from call to call.  Everything but the comparison of a
 * timeline value with a threshold is integer arithmetic; sample positions are 64-bit.
 */
#ifndef EAT_EVENT_SCORE_H
#define EAT_EVENT_SCORE_H
#include "eat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- collar matching of estimated against reference events, V threshold pairs at once ----------------------
 * filt (K, G_total) fp32 and rec (n_rec, 4) int32 are the timelines and the recording table of eat_detect.h: timeline
 * (i, k) is filt[k, goff_i .. goff_i + G_i).  Threshold pair v is 0 < lo[v] <= hi[v] (fp32, V values each, compared
 * with >=).
 *
 * Estimated events of (i, k, v): steps 1-3 of eat_detect_events with hi[v], lo[v], max_gap, min_len.  An event of
 * frames [on, off) spans the samples [on R, min(off R, nsamp[i])), nsamp (n_rec) int64 the recordings' lengths.
 *
 * Reference events: ref (n_ref, 3) int32 rows (class, onset sample, offset sample), ref_tol (n_ref) int32 the offset
 * tolerance of every row in samples; recording i owns the rows [ro[i], ro[i + 1]), ro (n_rec + 1) int64 rising from 0
 * to n_ref, sorted by (class, onset).  n_ref = 0 (then ref and ref_tol may be NULL) scores against nothing.  Of one
 * recording and class only the FIRST EAT_EVENT_SCORE_MAX_REF rows take part: the caller refuses more.
 *
 * Match: reference r and estimate e of the same recording and class are compatible iff |r.onset - e.onset| <= c and
 * |r.offset - e.offset| <= ref_tol[r].  For each estimate in onset order, the first compatible reference (row order)
 * not yet taken is taken: the same pairs as sed_eval's loop "for each reference in row order, the first compatible
 * estimate in onset order not yet taken", because both sides rank the other by one master order.
 *
 * counts (n_rec, K, V, 2) int32: counts[i, k, v] = (tp = matched pairs, n_est = estimated events); fp = n_est - tp,
 * fn = (reference rows of (i, k)) - tp.
 *
 * One wavefront per (recording, class) and 64 threshold pairs, one lane per pair; the timeline is read once per
 * wavefront, 64 frames per coalesced load.
 * EAT_EINVAL (before the device is touched): a missing operand; K, n_rec, G_total, R or V < 1; n_ref, c, max_gap or
 * min_len < 0; n_rec K > 2^31 - 1; V > 64 * 65535. */
#define EAT_EVENT_SCORE_MAX_REF 64
int eat_event_score(const float* filt, int K, int G_total, const int* rec, int n_rec, const long long* nsamp, int R,
                    const int* ref, const int* ref_tol, const long long* ro, int n_ref, int c, const float* hi,
                    const float* lo, int V, int max_gap, int min_len, int* counts, eat_stream_t stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* EAT_EVENT_SCORE_H */
