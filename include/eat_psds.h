/* eat_psds.h -- C ABI of the counting half of PSDS, the polyphonic sound detection score (Bilen et al., ICASSP 2020), in
 * libeat_hip.so (efficientat_amd/sed.py: evaluate_psds, csrc/psds.hip): for a whole grid of threshold pairs at once, form
 * the detector's events of every (recording, class) timeline by the rule of eat_detect_events (eat_detect.h), judge them
 * against the reference events by intersection ratios and store integer counts.  The detections never exist in memory;
 * the curve and its integral are host work on the counts (sed.psds_from_counts).
 *
 * A further header of the same library with the conventions of eat_hip.h: every pointer is a DEVICE pointer, the caller
 * owns every buffer, work is enqueued on `stream` with no hidden synchronisation (capture-safe), the return value is
 * EAT_OK or a negative EAT_E* code, and eat_last_error_string() holds the message.  Everything but the comparison of a
 * timeline value with a threshold is integer arithmetic, sample positions and all products 64-bit; the only atomics are
 * integer additions, so the same inputs give the same bits from call to call.
 */
#ifndef EAT_PSDS_H
#define EAT_PSDS_H
#include "eat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- intersection criteria of detections against reference events, V threshold pairs at once -----------------
 * filt, rec, nsamp, R, hi, lo, max_gap, min_len, ref, ro and n_ref are those of eat_event_score (eat_event_score.h):
 * timeline (i, k) is filt[k, goff_i .. goff_i + G_i); ref (n_ref, 3) int32 rows (class, onset sample, offset sample),
 * recording i owning the rows [ro[i], ro[i + 1]) sorted by (class, onset); of one recording and class only the first
 * EAT_PSDS_MAX_REF rows take part as references of that class (the caller refuses more).
 *
 * Detections of (i, k, v): steps 1-3 of eat_detect_events with hi[v], lo[v], max_gap, min_len.  A detection d of frames
 * [on, off) spans the samples [on R, min(off R, nsamp[i])), L_d its length; I(d, r) = max(0, min(d.off, r.off) -
 * max(d.on, r.on)).  The criteria are per-mille integers:
 *   DTC   S(d) = sum of I(d, r) over the rows of (i, k) (overlapping rows add).  d is RELEVANT iff L_d > 0 and
 *         1000 S(d) >= dtc_pm L_d, else a false positive.
 *   GTC   C(r) = sum of I(d, r) over the relevant detections of (i, k, v).  Row r is a true positive iff
 *         L_r = offset - onset > 0 and 1000 C(r) >= gtc_pm L_r.
 *   CTTC  (cttc_pm > 0) a false positive d of class k and a class c != k with rows in recording i: S_c(d) = sum of
 *         I(d, r) over the rows of class c; L_d > 0 and 1000 S_c(d) >= cttc_pm L_d is one cross-trigger (k -> c).
 *
 * counts (n_rec, K, V, 4) int32: counts[i, k, v] = (tp, n_det = detections, fp, n_ct = cross-triggers raised by the
 * timeline); every element is stored.  ct (V, K, K) int32, [v, detection class, reference class], is ADDED TO: the caller
 * zero-fills it once and the chunks of a split accumulate into it.  ct may be NULL iff cttc_pm == 0 and is then not
 * touched (n_ct = 0).
 *
 * One wavefront per (recording, class) and 64 threshold pairs, one lane per pair; the timeline is read once per
 * wavefront; the class's rows and a coverage counter per (row, lane) sit in LDS.
 * EAT_EINVAL (before the device is touched): a missing operand; K, n_rec, G_total, R or V < 1; n_ref, max_gap or
 * min_len < 0; n_rec K > 2^31 - 1; V > 64 * 65535; dtc_pm or gtc_pm outside [1, 1000]; cttc_pm outside [0, 1000];
 * ct == NULL with cttc_pm > 0. */
#define EAT_PSDS_MAX_REF 64
int eat_psds_count(const float* filt, int K, int G_total, const int* rec, int n_rec, const long long* nsamp, int R,
                   const int* ref, const long long* ro, int n_ref, int dtc_pm, int gtc_pm, int cttc_pm,
                   const float* hi, const float* lo, int V, int max_gap, int min_len,
                   int* counts, int* ct, eat_stream_t stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* EAT_PSDS_H */
