/* eat_median_bank.h -- C ABI of the width-bank median of sound event detection in libeat_hip.so (efficientat_amd/sed.py:
 * tune_postprocessing, detection.EADetector with per-class widths; csrc/median_bank.hip): the running median of
 * eat_detect_median (eat_detect.h) for a whole bank of widths at once, one width per (slice, class), so that the
 * timelines are read from memory once however many widths are tried.
 *
 * A further header of the same library with the conventions of eat_hip.h: every pointer is a DEVICE pointer, the caller
 * owns every buffer, work is enqueued on `stream` with no hidden synchronisation (capture-safe), the return value is
 * EAT_OK or a negative EAT_E* code, and eat_last_error_string() holds the message.  No atomics: every element of the
 * output is stored and the same inputs give the same bits from call to call.
 */
#ifndef EAT_MEDIAN_BANK_H
#define EAT_MEDIAN_BANK_H
#include "eat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- running median along time for Mw widths per class ------------------------------------------------------
 * prob (K, G_total) fp32 and rec (n_rec, 4) int32 are those of eat_detect.h.  widths (Mw, K) int32: widths[j, k] is odd
 * and lies in [1, 31] (the caller validates; a kernel cannot refuse, so it reads min(max(w, 1), 31) | 1 and can index
 * neither outside its LDS array nor outside a recording whatever the table holds).  filt (Mw, K, G_total) fp32:
 *   filt[j, k, goff + i] = the median of the m = widths[j, k] samples prob[k, goff + r(i + d)], d = -(m / 2) .. m / 2,
 * r the periodic reflection of eat_detect_median at the recording's own ends, the median the element of rank m / 2 in the
 * order (value, position): a selection, every output carries the bits of one input sample; m = 1 is a copy.  Slice j is
 * bit for bit what eat_detect_median stores for a width that is the same in every class.  Inputs must not be NaN.
 * filt must not overlap prob.
 *
 * 256 columns per block, classes on grid.y; per (class, recording piece of the tile) the piece and the reflected halo of
 * the class's widest width are staged in LDS once and all Mw slices are ranked from it.  All index arithmetic is 64-bit:
 * (j K + k) G_total + c passes 2^31 long before K G_total does.
 * EAT_EINVAL (before the device is touched): a missing operand, filt == prob, K, n_rec, G_total or Mw < 1. */
int eat_detect_median_bank(const float* prob, int K, int G_total, const int* rec, int n_rec, const int* widths, int Mw,
                           float* filt, eat_stream_t stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* EAT_MEDIAN_BANK_H */
