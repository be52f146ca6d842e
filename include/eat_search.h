/* eat_search.h -- C ABI of query-by-example search over an index of embeddings in libeat_hip.so
 * (efficientat_amd/retrieval.py): L2 normalisation of rows, and the k rows of a resident bank of largest cosine score
 * for each query, in order, without a (Q, N) score matrix.
 *
 * One more header of the same library with the conventions of eat_hip.h and eat_embed.h: every pointer is a DEVICE
 * pointer, fp32 unless noted, the caller owns every buffer, work is enqueued on `stream` with no hidden
 * synchronisation, the return value is EAT_OK or a negative EAT_E* code, and eat_last_error_string() holds the message.
 */
#ifndef EAT_SEARCH_H
#define EAT_SEARCH_H
#include "eat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- out[n, :] = x[n, :] / sqrt(sum_d x[n, d]^2), x and out (N, D) contiguous ---------------------------------------
 * The sum of squares is an fp32 sum in a fixed order; a row whose sum is 0 becomes all zeros.  out may be x itself
 * (any other overlap is undefined).  Any D >= 1; 16-byte accesses only where D % 4 == 0 and both bases are 16-byte
 * aligned.  EVERY element of out is stored.  The caller guarantees finite input.
 * EAT_EINVAL, before anything is launched: N < 0 (N == 0 launches nothing), D < 1. */
int eat_rows_normalize(const float* x, long long N, int D, float* out, eat_stream_t stream);

/* ---- bytes of workspace that eat_embed_search needs for Q queries and k results: a function of (Q, k) alone, positive
 * and non-decreasing in both; -1 where Q or k lies outside the limits below. */
long long eat_embed_search_ws_bytes(int Q, int k);

/* ---- cosine top-k ----------------------------------------------------------------------------------------------------
 * bank (N, D) and queries (Q, D): contiguous, rows ALREADY L2-normalised (eat_rows_normalize).
 * s[q, n] = sum_d queries[q, d] bank[n, d]: fp32 products and fp32 accumulation (v_fma) in an order that depends on D
 * alone, so the bits of s[q, n] are a function of the two rows' contents - not of n, N, the block or the alignment - and
 * identical rows tie exactly.
 * skip (Q, 2) int32 or NULL: row n is not eligible for query q when skip[q, 0] <= n < skip[q, 1]; both bounds are
 * clamped into [0, N], lo >= hi excludes nothing.
 * score (Q, k), index (Q, k) int32: the k eligible rows of largest s in descending s, equal s by ascending n; where fewer
 * than k rows are eligible the remaining slots hold index -1 and score -inf.  EVERY element of both is stored.
 * No atomics anywhere: the same bits from call to call.  The bank is read once per group of up to 16 queries (fewer
 * where D or k is large: a group's queries and running top-k lists stay in LDS).
 * ws: scratch of at least eat_embed_search_ws_bytes(Q, k) bytes, 16-byte aligned, free for reuse once the stream has
 * passed the call.
 * EAT_EINVAL, before anything touches the device: k outside [1, 128], Q outside [1, 1024], N outside [1, 2^31 - 1],
 * D < 1, ws_bytes below eat_embed_search_ws_bytes(Q, k). */
int eat_embed_search(const float* bank, long long N, int D, const float* queries, int Q, int k, const int* skip, void* ws,
                     long long ws_bytes, float* score, int* index, eat_stream_t stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* EAT_SEARCH_H */
