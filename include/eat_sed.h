/* eat_sed.h -- C ABI of strong-label sound-event-detection training in libeat_hip.so (efficientat_amd/sed.py,
 * mn_train.FrameHead, csrc/sed.hip): frame-level targets that follow a clip through the crop / pad / roll / wave-mix of
 * eat_wave_augment_ragged, the frame-level BCE-with-logits with its gradient and evaluation counts, and the elementwise
 * halves of the frame head's hidden layer.
 *
 * A further header of the same library with the conventions of eat_hip.h: every pointer is a DEVICE pointer, fp32
 * unless noted, the caller owns every buffer, work is enqueued on `stream` with no hidden synchronisation, the
 * return value is EAT_OK or a negative EAT_E* code, and eat_last_error_string() holds the message.  No atomics:
 * every kernel stores every element of its outputs, pads included, and gives the same bits from call to call.  Nothing
 * allocates or synchronises, so every entry point may be captured into a graph.  Index arithmetic is 64-bit.  Argument
 * checks return before anything touches the device.
 *
 * Frame tensors are (B, rows, Tp): Tp >= T columns per row, columns [T, Tp) are padding.
 */
#ifndef EAT_SED_H
#define EAT_SED_H
#include "eat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- frame targets of a batch drawn by eat_wave_augment_ragged ---------------------------------------------
 * The strong-label bank: events (n_events, 3) int32 rows (class, onset sample, offset sample), event_offsets
 * (n_bank + 1) int64 -- clip i owns rows [event_offsets[i], event_offsets[i + 1]), sorted by (class, onset), with
 * 0 <= onset < offset <= lengths[i] -- and lengths (n_bank) int32.  idx / start / shift (2B) int32 and mix (B) are the
 * tables handed to eat_wave_augment_ragged: slot k of sample b holds clip i = idx[2b + k] cropped at start[2b + k]
 * (window length w = min(lengths[i] - start, L)) and rolled by shift; idx[2b + 1] = -1: no wave-mix.
 * Frame t owns the output samples n in [t R, min((t + 1) R, L)); output sample n shows window position
 * p = (n - shift) mod L (the padding p >= w rolls with the clip).  a_k[c, t] = 1 iff an event (c, on, off) of the slot's
 * clip and a sample n of frame t have p < w and on <= start + p < off, else 0.  y (B, K, Tp):
 *   y[b, c, t] = a_0                                          without wave-mix
 *              = (float)(l a_0 + (1 - l) a_1), l = mix[b]     with it (the sum in fp64, rounded once: the rule of the
 *                                                             label rows of eat_wave_augment_ragged)
 * for t < T; columns [T, Tp) are 0.  A row whose slot does not name a clip of the bank or whose start lies outside
 * its clip is NaN in [0, T) (as the waveform row of eat_wave_augment_ragged is); nothing outside the tables is read:
 * event ranges are clipped to [0, n_events).
 * EAT_EINVAL: B, K, L, R, T or n_bank < 1, n_events < 0, Tp < T, a missing operand (events may be NULL only with
 * n_events = 0). */
int eat_sed_targets(const int* events, long long n_events, const long long* event_offsets, const int* lengths,
                    long long n_bank, int K, const int* idx, const int* start, const int* shift, const float* mix, int B,
                    int L, int R, int T, int Tp, float* y, eat_stream_t stream);

/* ---- frame-level BCE-with-logits, its gradient, and evaluation counts, in one pass over the logits -----------
 * z, y (B, K, Tp).  perm (B) int32 / lam (B): the log-mel mix-up, both NULL or both given;
 * t[b,c,t] = lam[b] y[b,c,t] + (1 - lam[b]) y[perm[b],c,t].  nframes (B) int32 or NULL: row b counts its frames
 * t < n_b = clamp(nframes[b], 0, T) (NULL: T).  M = K sum_b n_b.
 *   l = max(z, 0) - z t + log1p(exp(-|z|)) in fp64;  sums[0] += (float)(sum l / M)   (fixed order; 0 when M = 0)
 *   dlogits (B, Kp, Tp), Kp >= K: (sigmoid(z) - t) / M for c < K and t < n_b; exactly 0 in rows [K, Kp), in columns
 *                        [n_b, Tp), and everywhere when M = 0
 *   dbias (K) = sum_{b,t} dlogits[b,c,t], fp64 accumulation in a fixed order
 *   counts (K, 3) int64 += (tp, fp, fn) over the frames t < n_b: prediction s(z) >= thr[c] with s the fp32 sigmoid of
 *                        eat_detect_stitch, truth y > 0.5.  Needs thr (K); refused with perm.
 *   rows (B T, K): rows[(b T + t) K + c] = z[b,c,t]   (the score matrix of the mAP / ROC metric)
 * Any of sums, dlogits, dbias, counts, rows may be NULL.  ws: K + 1 doubles of workspace, needed with sums.  A perm
 * entry outside [0, B) makes the loss and the gradient of its row NaN; nothing outside y is read.  Two launches with
 * sums, else one: block c takes class c over all (b, t).
 * EAT_EINVAL: B, K or T < 1, Tp < T, Kp < K, a missing z / y, perm without lam or lam without perm, counts without
 * thr or with perm, sums without ws. */
int eat_frame_bce_fwd_bwd(const float* z, const float* y, const int* perm, const float* lam, const int* nframes,
                          const float* thr, int B, int K, int T, int Tp, int Kp, float* sums, float* dlogits, float* dbias,
                          long long* counts, float* rows, double* ws, eat_stream_t stream);

/* ---- a gradient arriving at the frame logits -> the padded operand of the head's backward, and the bias gradient
 * g (B, K, Tp) -> dl (B, Kp, Tp): dl = g for c < K and t < T, exactly 0 in rows [K, Kp) and columns [T, Tp) whatever g
 * holds there; db (K) = sum_{b, t < T} g[b,c,t], fp64 accumulation in a fixed order.  db may be NULL; dl must not be g.
 * EAT_EINVAL: B, K or T < 1, Tp < T, Kp < K, a missing g / dl, dl == g. */
int eat_frame_grad_pad(const float* g, float* dl, float* db, int B, int K, int Kp, int T, int Tp, eat_stream_t stream);

/* ---- hidden layer of the frame head: Hardswish and the per-(clip, unit) dropout factor -----------------------
 * z1, h, dh, dz1 (B, Hp, Tp); keep (B, Hp) or NULL (ones).
 *   fwd: h = hswish(z1) keep[b, j]                                    every element
 *   bwd: dz1 = dh keep[b, j] hswish'(z1) for j < H and t < T, exactly 0 in rows [H, Hp) and columns [T, Tp);
 *        db1 (H) = sum_{b, t < T} dz1[b,j,t], fp64 accumulation in a fixed order.  db1 may be NULL.
 * hswish'(u) = 0 for u < -3, u / 3 + 1 / 2 for -3 <= u <= 3, 1 above: the derivative of eat_mlp_head_bwd, kinks included.
 * EAT_EINVAL: B, Hp, Tp (fwd) or B, H, T (bwd) < 1, Hp < H, Tp < T, a missing operand. */
int eat_frame_hidden_fwd(const float* z1, const float* keep, float* h, int B, int Hp, int Tp, eat_stream_t stream);
int eat_frame_hidden_bwd(const float* dh, const float* z1, const float* keep, float* dz1, float* db1, int B, int H, int Hp,
                         int T, int Tp, eat_stream_t stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* EAT_SED_H */
