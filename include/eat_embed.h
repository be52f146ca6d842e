/* eat_embed.h -- C ABI of the audio-embedding extractor in libeat_hip.so (efficientat_amd/embeddings.py): the
 * channel means of a model's feature maps, over the whole map (scene embedding) or over time segments (timestamp
 * embeddings), for every map and every segment in one launch.
 *
 * A third header of the same library with the conventions of eat_hip.h and eat_tag.h: every pointer is a DEVICE
 * pointer, fp32 unless noted, the caller owns every buffer, work is enqueued on `stream` with no hidden
 * synchronisation, the return value is EAT_OK or a negative EAT_E* code, and eat_last_error_string() holds the message.
 */
#ifndef EAT_EMBED_H
#define EAT_EMBED_H
#include "eat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- segment means of n_maps feature maps, concatenated along the channel axis ------------------------------
 * maps (n_maps) int64: device addresses of contiguous fp32 maps x_l (B, C_l, F_l, T_l), each 4-byte aligned.
 * dims (n_maps, 4) int32: C_l, F_l, T_l, off_l.   seg (n_maps, n_seg, 2) int32: lo, hi of segment s on map l.
 * out (B, n_seg, D):  out[b, s, off_l + c] = sum_f sum_{t in [lo, hi)} x_l[b, c, f, t] / (F_l (hi - lo)).
 * The scene embedding is n_seg = 1 with (0, T_l).  Segments may overlap, repeat and leave columns out.
 * The kernel clamps lo and hi into [0, T_l] and stores 0.0 for a segment that is empty after clamping: it never reads
 * outside a map and never divides by zero, whatever seg holds.  EVERY element of out is written, with a plain store
 * (0.0 at a channel index that no map's [off_l, off_l + C_l) covers; where two maps cover one, the first one listed
 * wins): out needs no initialisation.  fp32 accumulation in a fixed order and no atomics: two calls on the same
 * input give identical bits.  One launch; an input element is read once (plane sums over f are formed once and
 * every segment is built from them) unless T_l > 1024, where it is read once per covering segment.
 * EAT_EINVAL, before anything is launched: n_maps outside [1, 64]; B, n_seg or D < 1; ceil(D / 4) * B blocks
 * beyond 2^31 - 1 (chunk the call over B). */
int eat_embed_pool(const long long* maps, const int* dims, const int* seg, int n_maps, int B, int n_seg, int D,
                   float* out, eat_stream_t stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* EAT_EMBED_H */
