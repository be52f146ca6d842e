/* eat_match_q8.h -- C ABI of occurrence search over an 8-bit ("q8") timestamp index in libeat_hip.so
 * (efficientat_amd/retrieval.py: EmbeddingIndex.find(allow_q8=True) on an index of storage="q8"): eat_match.h with the
 * row scores of eat_search_q8.h, and nothing else new.
 *
 * One more header of the same library with the conventions of eat_hip.h and eat_search.h: every pointer is a DEVICE
 * pointer, the caller owns every buffer, work is enqueued on `stream` with no hidden synchronisation, the return value is
 * EAT_OK or a negative EAT_E* code, and eat_last_error_string() holds the message.
 */
#ifndef EAT_MATCH_Q8_H
#define EAT_MATCH_Q8_H
#include "eat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- bytes of workspace that eat_embed_match_q8 needs: positive and non-decreasing in each argument, the same for every
 * L >= 64; -1 where N, L or k lies outside the limits below.  It holds the lists of the peak kernel, acc (N) and
 * S (min(L, 64), N) fp32, each part 16-byte aligned. */
long long eat_embed_match_q8_ws_bytes(long long N, int L, int k);

/* ---- sequence match with peak picking over a q8 bank -------------------------------------------------------------------
 * codes / ld / scale_n: the bank of eat_search_q8.h, N rows of D values (row n at byte n * ld, ld >= D, ld % 16 == 0, base
 * 16-byte aligned, scale_n (N,) fp32).  qcodes / qld / scale_q: one clip's L rows in time order at the bank's hop,
 * quantised by eat_rows_quantize_q8 like the bank.  Bytes [D, ld) of a bank row and [D, qld) of a query row may hold
 * anything: the kernel masks d >= D as eat_embed_search_q8 does.
 * s[j, n] = (float)acc * (scale_q[j] * scale_n[n]) with acc the exact int32 dot product of the two rows' codes: the score
 * of eat_embed_search_q8 for that pair, bit for bit.
 * Everything else is eat_embed_match, word for word.  seg (F + 1) int32: file f is the bank rows [seg[f], seg[f + 1]);
 * the caller guarantees seg[0] = 0, seg[F] = N and a strictly ascending table (it lives on the device and is not checked;
 * whatever it holds, no access leaves a buffer).  Start row n of file f is VALID when n + L <= seg[f + 1].  Then
 *   acc = s[0, n];  acc = acc + s[j, n + j] for j = 1 .. L - 1 in ascending j, one fp32 addition at a time;
 *   m[n] = acc / (float)L, correctly rounded
 * a mean of q8 scores, on the scale of eat_embed_search_q8's scores (L = 1: s[0, n] itself).  The bits of m[n] depend on the
 * L query rows and on bank rows n .. n + L - 1 alone, so a file stored twice ties exactly.
 * A CANDIDATE is a valid start row outside the exclusion range [skip_lo, skip_hi) (both bounds clamped into [0, N];
 * lo >= hi excludes nothing).  a is BETTER than b when m[a] > m[b], or m[a] == m[b] and a < b.  n is a PEAK when it is a
 * candidate and better than every other candidate x of the same file with 0 < |x - n| <= sep: local-maximum picking, NOT
 * greedy suppression.  sep = 0 makes every candidate a peak.
 * score (k), index (k) int32: the k peaks with m >= min_score, in descending m, equal m by ascending row; the remaining
 * slots hold index -1 and score -inf.  EVERY element of both is stored.  min_score = -inf disables the threshold.
 * No atomics anywhere: the same bits from call to call.  The bank is read once per group of up to 64 query rows (fewer
 * where D is large: a group's codes stay in LDS).  Every offset into the bank and into S is 64-bit.
 * ws: scratch of at least eat_embed_match_q8_ws_bytes(N, L, k) bytes, 16-byte aligned, free for reuse once the stream has
 * passed the call.  One call is one query clip.
 * EAT_EINVAL, before anything touches the device: L outside [1, 1024], k outside [1, 128], sep outside [0, 4096],
 * N outside [1, 2^31 - 1], F < 1, D outside [1, 131072], min_score NaN, ld or qld below D or no multiple of 16, codes or
 * qcodes not 16-byte aligned, ws_bytes below eat_embed_match_q8_ws_bytes(N, L, k). */
int eat_embed_match_q8(const signed char* codes, long long ld, const float* scale_n, long long N, int D, const int* seg, int F,
                       const signed char* qcodes, long long qld, const float* scale_q, int L, int k, int sep, float min_score,
                       int skip_lo, int skip_hi, void* ws, long long ws_bytes, float* score, int* index, eat_stream_t stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* EAT_MATCH_Q8_H */
