/* eat_attn.h -- C ABI of the multi-head attention-pooling head in libeat_hip.so (efficientat_amd/mn.py:
 * MultiHeadAttentionPooling, efficientat_amd/mn_train.py: AttentionPoolHead; csrc/attn_head.hip).
 *
 * A fourth header of the same library with the conventions of eat_hip.h: every pointer is a DEVICE pointer, fp32 unless
 * noted, the caller owns every buffer, work is enqueued on `stream` with no hidden synchronisation, the return value is
 * EAT_OK or a negative EAT_E* code, and eat_last_error_string() holds the message.
 */
#ifndef EAT_ATTN_H
#define EAT_ATTN_H
#include "eat_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

/* ---- multi-head attention-pooling head: models/mn/attention_pooling.py:9-56 (head_type="multihead_attention_pooling") ---
 * The head stays in the layout of the 1x1 kernels, nothing is transposed:
 *   y (B, C, F, T) last feature map -> xm (B, C, Tp) mean over frequency -> p (B, N, Tp) = W xm on eat_pw_conv_fwd /
 *   eat_pw_conv_bf16_fwd with S = Tp, N = 2 H K -> out (B, K).
 * Row n = (j H + h) K + k of subspace_proj.weight (N, C): j = 0 the attention logit, j = 1 the value of head h, class k (the
 * reference's reshape(b, t, 2, H, K) of the Linear output).  Tp >= T is the row pitch of xm / p / dp: a multiple of 4 for
 * the MFMA kernels (S % 4 == 0).  Pad columns [T, Tp) are WRITTEN as zeros by eat_freq_mean_fwd and eat_attn_pool_bwd, so
 * that the GEMMs contracting over positions stay exact, and are never read by the pooling kernels.
 *
 * eat_freq_mean_fwd: xm[b, c, t] = (1 / F) sum_f y[b, c, f, t] (t < T), 0 (T <= t < Tp)   [x.mean(dim=2), :38]
 * eat_freq_mean_bwd: dy[b, c, f, t] = dxm[b, c, t] / F
 * eat_attn_pool_fwd (:41-56), one pass over t, no intermediate tensor:
 *   q = p + bias (bias (N) or NULL);  a_t = clamp(sigmoid(q_att), lo, hi), lo / hi = eps and 1 - eps (evaluated in double)
 *   rounded to fp32, as torch clamps an fp32 tensor with Python floats;  s = sum_t a_t;  o = sum_t a_t q_val / s;
 *   out[b, k] = sum_h head_w[h] o[b, h, k].   o, s (B, H, K): saved for the backward, or both NULL.
 * eat_attn_pool_bwd, g (B, K) = d loss / d out:
 *   do = g head_w[h];  dq_val = do a_t / s;  da_t = do (q_val - o) / s;
 *   dq_att = da_t sig (1 - sig) where lo <= sig <= hi, else 0 (torch's clamp gradient, bounds inclusive);
 *   dp (B, Np, Tp) = (dq_att, dq_val), pad columns and the rows [N, Np) of every sample 0 (Np >= N: a projection padded
 *   to a multiple of 4 rows for the data-gradient GEMM);  dbias[n] = sum_{b,t} dp (or NULL);  dhead_w[h] = sum_{b,k} g o.
 *   ws: B (N + H) floats of workspace (per-sample partial sums; every element is written before it is read).
 * out, xm, dy, dp come from one thread group each in a fixed order: bit-identical from run to run.  dbias / dhead_w are
 * per-sample fp32 partials summed over b in fp64 in a fixed order (three launches in all); no atomics anywhere.
 * Any T >= 1, any 4-byte aligned base (4-byte accesses, contiguous along t).  B, C, F, H, K, T >= 1, Tp >= T, 0 <= eps < 0.5
 * and the required pointers not NULL, else EAT_EINVAL and nothing is launched. */
int eat_freq_mean_fwd(const float* y, float* xm, int B, int C, int F, int T, int Tp, eat_stream_t stream);
int eat_freq_mean_bwd(const float* dxm, float* dy, int B, int C, int F, int T, int Tp, eat_stream_t stream);
int eat_attn_pool_fwd(const float* p, const float* bias, const float* head_w, double eps, float* out, float* o, float* s,
                      int B, int H, int K, int T, int Tp, eat_stream_t stream);
int eat_attn_pool_bwd(const float* g, const float* p, const float* bias, const float* head_w, double eps, const float* o,
                      const float* s, float* dp, float* dbias, float* dhead_w, float* ws, int B, int H, int K, int T, int Tp,
                      int Np, eat_stream_t stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* EAT_ATTN_H */
