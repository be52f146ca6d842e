/* eat_match.h -- C ABI of occurrence search over a timestamp index in libeat_hip.so (efficientat_amd/retrieval.py:
 * EmbeddingIndex.find): where in the files of a bank does a SEQUENCE of query rows occur.  The mean cosine of the
 * sequence laid over every start row of every file, local-maximum peak picking within a file, and the k best peaks.
 *
 * One more header of the same library with the conventions of eat_hip.h and eat_search.h: every pointer is a DEVICE
 * pointer, fp32 unless noted, the caller owns every buffer, work is enqueued on `stream` with no hidden
 * synchronisation, the return value is EAT_OK or a negative EAT_E* code, and eat_last_error_string() holds the message.
 */
#ifndef EAT_MATCH_H
#define EAT_MATCH_H
#include "eat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- bytes of workspace that eat_embed_match needs: positive and non-decreasing in each argument; -1 where N, L or k
 * lies outside the limits below. */
long long eat_embed_match_ws_bytes(long long N, int L, int k);

/* ---- sequence match with peak picking ---------------------------------------------------------------------------------
 * bank (N, D) and queries (L, D): contiguous, rows ALREADY L2-normalised (eat_rows_normalize); the queries are one clip's
 * rows in time order, at the bank's hop.
 * seg (F + 1) int32: file f is the bank rows [seg[f], seg[f + 1]); the caller guarantees seg[0] = 0, seg[F] = N and a
 * strictly ascending table (it lives on the device and is not checked; whatever it holds, no access leaves a buffer).
 * s[j, n]: the score of eat_embed_search for query row j and bank row n, bit for bit (the same code computes it).
 * Start row n of file f is VALID when the whole window fits the file, n + L <= seg[f + 1].  Then
 *   acc = s[0, n];  acc = acc + s[j, n + j] for j = 1 .. L - 1 in ascending j, one fp32 addition at a time;
 *   m[n] = acc / (float)L, correctly rounded
 * a mean cosine, on the scale of eat_embed_search's scores (L = 1: s[0, n] itself).  The bits of m[n] depend on the L
 * query rows, on bank rows n .. n + L - 1 and on (D, L) alone - not on n, N, the block or the alignment - so a file stored
 * twice ties exactly.
 * A CANDIDATE is a valid start row outside the exclusion range [skip_lo, skip_hi) (both bounds clamped into [0, N];
 * lo >= hi excludes nothing).  a is BETTER than b when m[a] > m[b], or m[a] == m[b] and a < b.
 * n is a PEAK when it is a candidate and better than every other candidate x of the same file with 0 < |x - n| <= sep.
 * Rows of other files and excluded rows never suppress; sep = 0 makes every candidate a peak.  This is local-maximum
 * picking, NOT greedy suppression: a place weaker than a neighbour within sep is dropped even when that neighbour is
 * itself dropped by a still better one.
 * score (k), index (k) int32: the k peaks with m >= min_score, in descending m, equal m by ascending row; the remaining
 * slots hold index -1 and score -inf.  EVERY element of both is stored.  min_score = -inf disables the threshold.
 * No atomics anywhere: the same bits from call to call.  The bank is read once per group of up to 16 query rows.
 * ws: scratch of at least eat_embed_match_ws_bytes(N, L, k) bytes, 16-byte aligned, free for reuse once the stream has
 * passed the call.  One call is one query clip; several clips are a loop on the host.
 * EAT_EINVAL, before anything touches the device: L outside [1, 1024], k outside [1, 128], sep outside [0, 4096],
 * N outside [1, 2^31 - 1], F < 1, D < 1, min_score NaN, ws_bytes below eat_embed_match_ws_bytes(N, L, k). */
int eat_embed_match(const float* bank, long long N, int D, const int* seg, int F, const float* queries, int L, int k,
                    int sep, float min_score, int skip_lo, int skip_hi, void* ws, long long ws_bytes, float* score,
                    int* index, eat_stream_t stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* EAT_MATCH_H */
