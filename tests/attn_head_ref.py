"""Float64 restatement of the attention-pooling head's formulas (include/eat_attn.h, csrc/attn_head.hip) in the layout of the
kernels: plain loops-as-tensor-algebra on CPU tensors, no autograd, nothing shared with the code under test.

Layout: xm (B, C, T) mean over frequency; p (B, N, T) with N = 2 H K and row n = (j H + h) K + k (j = 0 attention logit,
1 value); out (B, K).  The functions take tensors WITHOUT pad columns; `pad` / `unpad` convert to and from a row pitch."""
import numpy as np
import torch

F64 = torch.float64


def freq_mean(y):
    """y (B, C, F, T) -> xm (B, C, T)."""
    y = y.to(F64)
    return y.sum(dim=2) / y.shape[2]


def freq_mean_bwd(dxm, F):
    """dxm (B, C, T) -> dy (B, C, F, T)."""
    dxm = dxm.to(F64)
    return (dxm / F).unsqueeze(2).expand(-1, -1, F, -1).contiguous()


def _split(p, bias, H):
    B, N, T = p.shape
    K = N // (2 * H)
    q = p.to(F64)
    if bias is not None:
        q = q + bias.to(F64).view(1, N, 1)
    q = q.view(B, 2, H, K, T)
    return q[:, 0], q[:, 1], K                                   # (B, H, K, T) each


def attn_pool(p, bias, head_w, H, eps=1e-7):
    """-> out (B, K), o (B, H, K), s (B, H, K)."""
    qa, qv, _ = _split(p, bias, H)
    sig = 1.0 / (1.0 + torch.exp(-qa))
    a = torch.clamp(sig, eps, 1.0 - eps)
    s = a.sum(dim=3)
    o = (a * qv).sum(dim=3) / s
    out = (head_w.to(F64).view(1, H, 1) * o).sum(dim=1)
    return out, o, s


def attn_pool_bwd(g, p, bias, head_w, H, eps=1e-7):
    """-> dp (B, N, T), dbias (N), dhead_w (H)."""
    B, N, T = p.shape
    qa, qv, K = _split(p, bias, H)
    _, o, s = attn_pool(p, bias, head_w, H, eps)
    sig = 1.0 / (1.0 + torch.exp(-qa))
    a = torch.clamp(sig, eps, 1.0 - eps)
    g = g.to(F64)
    d_o = g.view(B, 1, K) * head_w.to(F64).view(1, H, 1)        # (B, H, K)
    dqv = d_o.unsqueeze(3) * a / s.unsqueeze(3)
    da = d_o.unsqueeze(3) * (qv - o.unsqueeze(3)) / s.unsqueeze(3)
    inside = (sig >= eps) & (sig <= 1.0 - eps)
    dqa = torch.where(inside, da * sig * (1.0 - sig), torch.zeros_like(da))
    dp = torch.stack((dqa, dqv), dim=1).reshape(B, N, T)
    dbias = dp.sum(dim=(0, 2))
    dhead_w = (g.view(B, 1, K) * o).sum(dim=(0, 2))
    return dp, dbias, dhead_w


def head(y, w, b, head_w, H, eps=1e-7):
    """The whole head: y (B, C, F, T), w (N, C), b (N), head_w (H values) -> out (B, K)."""
    xm = freq_mean(y)
    p = torch.einsum("nc,bct->bnt", w.to(F64), xm)
    return attn_pool(p, b, head_w.reshape(-1), H, eps)[0]


def head_bwd(g, y, w, b, head_w, H, eps=1e-7):
    """-> dy, dw, db, dhead_w of `head`."""
    xm = freq_mean(y)
    p = torch.einsum("nc,bct->bnt", w.to(F64), xm)
    dp, db, dhw = attn_pool_bwd(g, p, b, head_w.reshape(-1), H, eps)
    dw = torch.einsum("bnt,bct->nc", dp, xm)
    dxm = torch.einsum("nc,bnt->bct", w.to(F64), dp)
    return freq_mean_bwd(dxm, y.shape[2]), dw, db, dhw


def pad(x, Tp, fill=0.0):
    """(..., T) -> (..., Tp) with `fill` in the pad columns."""
    out = torch.full(x.shape[:-1] + (Tp,), fill, dtype=x.dtype)
    out[..., :x.shape[-1]] = x
    return out


def pool_inputs(B, H, K, T, seed, with_bias=True):
    """The pooling kernels' test inputs as fp32 CPU tensors (p already holds logits - bias, so that q = p + bias has the
    stated distribution): logits 1.5 N(0, 1) clamped to |q| <= 12, 5 % of them replaced by +-(20 + 10 U) - both clamp bounds
    are hit, none lies where fp32 and fp64 would put the sigmoid on different sides of a bound - bias 0.3 N, head_w 0.1 + U,
    g N(0, 1)."""
    rng = np.random.default_rng(seed)
    N = 2 * H * K
    q = np.clip(1.5 * rng.standard_normal((B, N, T)), -12.0, 12.0)
    hit = rng.random((B, N, T)) < 0.05
    hit[:, H * K:] = False                                       # the value half keeps its distribution
    q = np.where(hit, np.where(rng.random((B, N, T)) < 0.5, -1.0, 1.0) * (20.0 + 10.0 * rng.random((B, N, T))), q)
    bias = (0.3 * rng.standard_normal(N)).astype(np.float32) if with_bias else None
    p = (q - (bias.astype(np.float64)[None, :, None] if with_bias else 0.0)).astype(np.float32)
    head_w = (0.1 + rng.random(H)).astype(np.float32)
    g = rng.standard_normal((B, K)).astype(np.float32)
    t = torch.from_numpy
    return t(p), (t(bias) if with_bias else None), t(head_w), t(g)
