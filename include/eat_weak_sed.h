/* eat_weak_sed.h -- C ABI of weak-label sound-event-detection training in libeat_hip.so (efficientat_amd/sed.py:
 * WeakFrameTrainer, csrc/weak_sed.hip): the clip-level targets and the frame-truth flag of a batch drawn by
 * eat_wave_augment_ragged, and the frame BCE over the samples that have frame truth fused with a clip-level BCE behind
 * linear-softmax pooling of the frame probabilities (Wang et al., ICASSP 2019).
 *
 * A further header of the same library with the conventions of eat_sed.h: every pointer is a DEVICE pointer, fp32
 * unless noted, the caller owns every buffer, work is enqueued on `stream` with no hidden synchronisation, the
 * return value is EAT_OK or a negative EAT_E* code, and eat_last_error_string() holds the message.  No atomics:
 * every kernel stores every element of its outputs, pads included, and gives the same bits from call to call.  Nothing
 * allocates or synchronises, so every entry point may be captured into a graph.  Index arithmetic is 64-bit.  Argument
 * checks return before anything touches the device.
 *
 * Frame tensors are (B, rows, Tp): Tp >= T columns per row, columns [T, Tp) are padding.
 */
#ifndef EAT_WEAK_SED_H
#define EAT_WEAK_SED_H
#include "eat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- clip-level targets and the frame-truth flag of a batch drawn by eat_wave_augment_ragged ------------------
 * events, n_events, event_offsets, lengths, n_bank, K, idx, start, mix, B, L: the tables of eat_sed_targets (eat_sed.h).
 * strong (n_bank) uint8 or NULL: strong[i] != 0 iff clip i carries onset / offset annotation (NULL: every clip does); a
 * weakly labelled clip holds its tags as events (class, 0, lengths[i]).
 * Slot k of sample b names clip i = idx[2b + k] cropped at st = start[2b + k]; it shows the clip's samples
 * [st, st + min(lengths[i] - st, L)) (the roll does not matter at clip level).  a_k[c] = 1 iff an event (c, on, off) of
 * that clip has on < st + min(lengths[i] - st, L) and off > st, else 0.  w (B, K):
 *   w[b, c] = a_0                                          without wave-mix (idx[2b + 1] = -1)
 *           = (float)(l a_0 + (1 - l) a_1), l = mix[b]     with it (the sum in fp64, rounded once: the rule of eat_sed_targets)
 * framed (B) int32: 1 iff every slot in use names a clip with strong != 0, else 0.
 * A sample with a slot that eat_sed_targets refuses (an index outside the bank, a start outside the clip) has a NaN row
 * w[b, :] and framed[b] = 0; nothing outside the tables is read: event ranges are clipped to [0, n_events).
 * EAT_EINVAL: B, K, L or n_bank < 1, n_events < 0, a missing operand (events may be NULL only with n_events = 0;
 * strong may always be NULL). */
int eat_sed_clip_targets(const int* events, long long n_events, const long long* event_offsets, const int* lengths,
                         long long n_bank, int K, const int* idx, const int* start, const float* mix,
                         const unsigned char* strong, int B, int L, float* w, int* framed, eat_stream_t stream);

/* ---- frame BCE over the samples with frame truth + pooled clip BCE over all samples, one pass over the logits --
 * z, y (B, K, Tp); w (B, K) clip targets; framed (B) int32.  perm (B) int32 / lam (B): the log-mel mix-up, both NULL
 * or both given:
 *   ty[b,c,t] = lam[b] y[b,c,t] + (1 - lam[b]) y[perm[b],c,t],  tw[b,c] likewise of w,  f_b = framed[b] && framed[perm[b]]
 *   (without perm: ty = y, tw = w, f_b = framed[b]).
 * All arithmetic in fp64, rounded to fp32 at the store.  p_t = s(z[b,c,t]) with s the branch form
 * z >= 0 ? 1 / (1 + e) : e / (1 + e), e = exp(-|z|); 1 - p_t is taken as s(-z) in the same form, so it does not cancel.
 *   frame term  N_f = K T sum_b f_b;  L_f = sum_{b: f_b} sum_{c, t < T} [max(z, 0) - z ty + log1p(e)] / N_f   (0 when N_f = 0)
 *   pooling     S1 = sum_{t < T} p_t, S2 = sum_{t < T} p_t^2;  P = S2 / S1 if S1 > 0 else 0   (linear-softmax pooling)
 *   clip term   Pc = min(max(P, eps), 1 - eps);  l = -(tw log Pc + (1 - tw) log1p(-Pc));  L_c = sum_{b,c} l / (B K)
 *   sums[0] += (float)(L_f + weak_weight L_c), sums[1] += (float)L_f, sums[2] += (float)L_c        (fixed order)
 *   dlogits (B, Kp, Tp), Kp >= K: for c < K and t < T
 *               f_b (p_t - ty) / N_f + weak_weight g,
 *               g = (Pc - tw) / (Pc (1 - Pc)) (2 p_t - P) p_t (1 - p_t) / S1 / (B K), g = 0 when S1 = 0
 *               (the clamp passes the gradient straight through: a saturated row keeps a finite gradient bounded by
 *               1 / eps); exactly 0 in rows [K, Kp) and columns [T, Tp)
 *   dbias (K) = sum_{b,t} dlogits[b,c,t], fp64 accumulation in a fixed order
 *   clip_prob (B, K) = (float)P, unclamped
 * Any of sums, dlogits, dbias, clip_prob may be NULL.  ws: 2 K + 1 doubles of workspace, needed with sums.  A perm
 * entry outside [0, B) makes the loss and the gradient of its row NaN; nothing outside y, w and framed is read.  Two
 * launches with sums, else one: block c takes class c, a group of 32 (T <= 32) or 64 lanes one row (b, c) at a time.
 * EAT_EINVAL: B, K or T < 1, Tp < T, Kp < K, a missing z / y / w / framed, perm without lam or lam without perm, sums
 * without ws, weak_weight negative or not finite, eps outside (0, 0.5). */
int eat_weak_frame_bce_fwd_bwd(const float* z, const float* y, const float* w, const int* framed, const int* perm,
                               const float* lam, float weak_weight, float eps, int B, int K, int T, int Tp, int Kp,
                               float* sums, float* dlogits, float* dbias, float* clip_prob, double* ws,
                               eat_stream_t stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* EAT_WEAK_SED_H */
