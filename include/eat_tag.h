/* eat_tag.h -- C ABI of the long-recording tagger in libeat_hip.so: the device side of the reference's
 * windowed_inference.py (EATagger.tag_audio_window), which loops on the host over one window at a time.
 *
 * A second header of the same library with the conventions of eat_hip.h: every pointer is a DEVICE pointer,
 * fp32 unless noted, the caller owns every buffer, work is enqueued on `stream` with no hidden synchronisation,
 * the return value is EAT_OK or a negative EAT_E* code, and eat_last_error_string() holds the message.
 */
#ifndef EAT_TAG_H
#define EAT_TAG_H
#include "eat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- log-mel of N windows of one flat waveform buffer: windowed_inference.py:96-104 -------------------------
 * wave (n_wave) holds any number of recordings back to back.  Window w is the L samples from wave[win_start[w]];
 * positions >= win_valid[w] inside the window read as 0.0 (0 <= win_valid[w] <= L): the zero tail that the
 * reference appends with F.pad before it slices.  Pre-emphasis and reflect padding are per window, about the
 * window of length L, exactly as for one row of eat_mel_fwd, and out (N, n_mels, T) holds the bits that eat_mel_fwd
 * gives on the materialised (padded, sliced, contiguous) windows.  No masks: evaluation only.
 * Windows may overlap and may start on odd or even elements.  The caller guarantees win_start[w] >= 0 and
 * win_start[w] + win_valid[w] <= n_wave; the kernel also clamps both, so it never reads outside the buffer.
 *   win_start (N) int64, win_valid (N) int32; window .. band_pairs and T = 1 + (L - 1) / hop as for eat_mel_fwd.
 * EAT_EINVAL: the geometry errors of eat_mel_fwd, N < 1, N > 65535 (chunk the call), n_wave < 0. */
int eat_mel_windows_fwd(const float* wave, long long n_wave, const long long* win_start, const int* win_valid,
                        int N, int L, const float* window, int win_length, int n_fft, int hop,
                        const float* twiddle, const float* band_w2, const int* band_start, const int* band_cnt,
                        int n_mels, int band_pairs, float* out, int T, eat_stream_t stream);

/* ---- sigmoid + per-row top-k: windowed_inference.py:106-107 (sigmoid, np.argsort(p)[::-1]) ------------------
 * logits (N, C) finite -> p = 1 / (1 + exp(-logit)) in fp32; prob (N, k) and index (N, k) int32 receive the k
 * largest p of each row in descending order, EQUAL p ordered by ascending class index (the reference leaves ties
 * unspecified).  probs_all (N, C) receives every p, or NULL.  1 <= k <= min(C, 64), any C >= 1.
 * One wavefront per row and no atomics: results are identical from run to run. */
int eat_tag_topk(const float* logits, int N, int C, int k, float* prob, int* index, float* probs_all,
                 eat_stream_t stream);

/* ---- dequantise + down-mix + polyphase resampling: librosa.core.load(path, sr, mono=True) -------------------
 * in: interleaved (n_in, channels) frames, int16 (in_i16 != 0, scaled by 1/32768) or float32;  m[i] = channel
 * mean of frame i.  out[j] = sum_i m[i] * taps[j * down - i * up + half], half = (n_taps - 1) / 2, over the i
 * with a tap index inside [0, n_taps) and 0 <= i < n_in: scipy.signal.resample_poly(m, up, down) with
 * padtype='constant' when taps = firwin(2 * half + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up and
 * half = 10 * max(up, down) (the host designs them in fp64 and rounds once).  n_out = ceil(n_in * up / down).
 * All index arithmetic is 64-bit.
 * EAT_EINVAL: up, down, channels or n_in < 1, an even or non-positive n_taps, another n_out. */
int eat_resample_mono(const void* in, int in_i16, long long n_in, int channels, int up, int down,
                      const float* taps, int n_taps, float* out, long long n_out, eat_stream_t stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* EAT_TAG_H */
