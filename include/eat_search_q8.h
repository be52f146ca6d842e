/* eat_search_q8.h -- C ABI of the 8-bit ("q8") storage of a search index in libeat_hip.so (efficientat_amd/retrieval.py,
 * EmbeddingIndex(storage="q8")): rows quantised to int8 codes with one fp32 scale each, and the top-k of eat_search.h over
 * such a bank with exact integer dot products (v_mfma_i32_16x16x64_i8).  A quarter of the bytes per row of the fp32 index.
 *
 * One more header of the same library with the conventions of eat_hip.h and eat_search.h: every pointer is a DEVICE
 * pointer, the caller owns every buffer, work is enqueued on `stream` with no hidden synchronisation, the return value is
 * EAT_OK or a negative EAT_E* code, and eat_last_error_string() holds the message.
 *
 * A q8 matrix of N rows of D values: codes, int8, row n at byte n * ld (ld >= D, ld % 16 == 0, base 16-byte aligned), and
 * scale (N,) fp32.  Row n stands for scale[n] * codes[n, 0 : D].
 */
#ifndef EAT_SEARCH_Q8_H
#define EAT_SEARCH_Q8_H
#include "eat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- quantise the rows of x (N, D) fp32, contiguous ------------------------------------------------------------------
 * xh = x / sqrt(sum_d x^2) with the very bits of eat_rows_normalize (a row whose sum is 0 becomes zeros) where
 * normalize != 0, else xh = x.  amax = max_d |xh[d]|, scale = amax / 127.0f (one IEEE fp32 division),
 * code[d] = (int8) rintf(xh[d] / scale): an IEEE fp32 division, rounded half to even, in [-127, 127]; -128 never occurs.
 * A row with amax == 0 gets scale 0 and all-zero codes.  Bytes [D, ld) of every row are stored as ZEROS: every byte of
 * codes[0 : N * ld] and every element of scale is stored.  Any D; 16-byte loads of x only where D % 4 == 0 and x is
 * 16-byte aligned, with the same bits either way.  The caller guarantees finite input.
 * EAT_EINVAL, before anything is launched: N < 0 (N == 0 launches nothing), D outside [1, 131072], ld < D, ld % 16 != 0,
 * codes not 16-byte aligned. */
int eat_rows_quantize_q8(const float* x, long long N, int D, int normalize, signed char* codes, long long ld, float* scale,
                         eat_stream_t stream);

/* ---- bytes of workspace that eat_embed_search_q8 needs for Q queries and k results: a function of (Q, k) alone, positive
 * and non-decreasing in both; -1 where Q or k lies outside the limits below. */
long long eat_embed_search_q8_ws_bytes(int Q, int k);

/* ---- top-k over a q8 bank ---------------------------------------------------------------------------------------------
 * codes / ld / scale_n: the bank, N rows; qcodes / qld / scale_q: the queries, Q rows; both of D values.
 * acc[q, n] = sum_d qcodes[q, d] codes[n, d] in int32: exact, 127^2 D < 2^31 for D <= 131072.
 * s[q, n] = (float)acc[q, n] * (scale_q[q] * scale_n[n]): one int -> fp32 conversion (round to nearest even) and two fp32
 * multiplies in that association.  No term depends on n, N, the block, the tile slot or the alignment: identical rows tie
 * exactly, and the same bits come back from call to call.
 * The kernel masks d >= D (it zeroes those bytes of its copy of the queries, so the products vanish): bytes [D, ld) of a
 * bank row and [D, qld) of a query row may hold anything.  -128 is a legal code as far as the arithmetic goes only while
 * the sum stays inside int32; eat_rows_quantize_q8 never produces it.
 * skip, score, index: exactly as in eat_embed_search - the k eligible rows by (s descending, n ascending), skip (Q, 2)
 * int32 or NULL clamped into [0, N], (-inf, -1) in the slots beyond the eligible rows, EVERY element of both stored, no
 * atomics.  The bank is read once per group of up to 64 queries (fewer where D or k is large: a group's codes and
 * running top-k lists stay in LDS).  Every offset into the bank is 64-bit.
 * ws: scratch of at least eat_embed_search_q8_ws_bytes(Q, k) bytes, 16-byte aligned.
 * EAT_EINVAL, before anything touches the device: k outside [1, 128], Q outside [1, 1024], N outside [1, 2^31 - 1],
 * D outside [1, 131072], ld or qld below D or no multiple of 16, codes or qcodes not 16-byte aligned, ws_bytes below
 * eat_embed_search_q8_ws_bytes(Q, k). */
int eat_embed_search_q8(const signed char* codes, long long ld, const float* scale_n, long long N, int D,
                        const signed char* qcodes, long long qld, const float* scale_q, int Q, int k, const int* skip, void* ws,
                        long long ws_bytes, float* score, int* index, eat_stream_t stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* EAT_SEARCH_Q8_H */
