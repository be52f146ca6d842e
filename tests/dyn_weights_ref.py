"""fp64 oracle of DyMN's per-sample weight kernels (csrc/dymn.hip: dyn_aggregate, the three dyn_pw_pack forms, dyn_bank_grad)
and of the fp32 per-sample 1x1 conv that reads the fp32 pack - a helper, not a test module.  numpy / torch on the CPU only;
every input is widened to fp64 first, so an fp32 operand enters with exactly the value the kernel reads.

The pack layouts are taken from their documentation and from what the CONSUMER kernels read, not from the pack kernels:
  fp32  (csrc/conv_pw.hip, v_mfma_f32_16x16x4f32: lane l holds A[l & 15][l >> 4] of a 16 x 4 fragment)
        wp[b][(ks*MT + mt)*64 + lane]                  = W_b[mt*16 + (lane & 15)][ks*4 + (lane >> 4)]
  bf16  (csrc/conv_pw_bf16.hip, v_mfma_f32_16x16x32_bf16: lane l holds 8 consecutive k of row l & 15)
        wp[b][((kk*MT + mt)*NP2 + h)*512 + lane*8 + i] = part h of W_b[mt*16 + (lane & 15)][kk*32 + 8*(lane >> 4) + i]
        NP2 = 2: h = 0 the bf16 rounding of the value, h = 1 the bf16 rounding of what is left; NP2 = 1: the rounding alone
with MT = ceil(Co / 16), KK = ceil(Ci / 32); rows >= Co and columns >= Ci of the fragments are zero.
The DECODERS gather through the index formula above; the ENCODERS go the other way by reshaping / permuting the padded
matrix, so that "decode(encode(W)) == W" compares two independent statements of the layout.
"""
import numpy as np
import torch

U32 = 2.0 ** -24                                              # unit round-off of fp32
U16 = 2.0 ** -8                                               # ... of bf16 (8 significant bits, round to nearest even)
SLACK = 2.0                                                   # fma versus separately rounded multiply + add; nothing else


def _f64(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().double().numpy()
    return np.asarray(a).astype(np.float64)


# ---------------------------------------------------------------------------------------------------- the operation in fp64
def aggregate(bank, att, gscale=None, group=1):
    """bank (K, N), att (B, K) [, gscale (ceil(N / group),)] -> (W (B, N) = gscale[n // group] * sum_k att[b,k] bank[k,n],
    A (B, N) = sum_k |att[b,k]| |bank[k,n]|, the magnitude sum of the bounds - WITHOUT gscale)."""
    bank, att = _f64(bank), _f64(att)
    W, A = att @ bank, np.abs(att) @ np.abs(bank)
    if gscale is not None:
        W = W * _f64(gscale)[np.arange(bank.shape[1]) // group][None, :]
    return W, A


def transposed_bank(bank, Co, Ci):
    """bank (K, Co*Ci) of row-major (Co, Ci) matrices -> the bank of their transposes (K, Ci*Co) (the `trans` packs' input)."""
    K = bank.shape[0]
    return bank.reshape(K, Co, Ci).transpose(1, 2).contiguous().reshape(K, Ci * Co)


# ------------------------------------------------------------------------------------------------------------------ layouts
def _mt(Co):
    return (Co + 15) // 16


def _kk(Ci):
    return (Ci + 31) // 32


def fp32_pack_len(Co, Ci):
    return (Ci // 4) * _mt(Co) * 64


def bf16_pack_len(Co, Ci, np2):
    return _kk(Ci) * _mt(Co) * np2 * 512


def _fp32_index(Co, Ci):
    """(MT*16, Ci) int64: position of padded-matrix element [row][col] inside one sample's fp32 pack."""
    MT = _mt(Co)
    row, col = np.arange(MT * 16)[:, None], np.arange(Ci)[None, :]
    lane = (row % 16) + 16 * (col % 4)
    return ((col // 4) * MT + row // 16) * 64 + lane


def _bf16_index(Co, Ci, np2, h):
    """(MT*16, KK*32) int64: position of part h of padded-matrix element [row][col] inside one sample's bf16 pack."""
    MT = _mt(Co)
    row, col = np.arange(MT * 16)[:, None], np.arange(_kk(Ci) * 32)[None, :]
    lane = (row % 16) + 16 * ((col % 32) // 8)
    return (((col // 32) * MT + row // 16) * np2 + h) * 512 + lane * 8 + col % 8


def _gather(wp, idx):
    B = wp.shape[0]
    flat = torch.from_numpy(idx.reshape(-1))
    return wp.index_select(1, flat).reshape(B, *idx.shape)


def decode_fp32(wp, Co, Ci):
    """wp (B, fp32_pack_len) float32 -> (B, MT*16, Ci) float32, the padding rows included."""
    assert wp.dtype == torch.float32 and wp.shape[1] == fp32_pack_len(Co, Ci) and Ci % 4 == 0
    return _gather(wp, _fp32_index(Co, Ci))


def decode_b16(wp, Co, Ci):
    """Plain bf16 pack (B, bf16_pack_len(.., 1)) -> (B, MT*16, KK*32) bfloat16, the padding rows and columns included."""
    assert wp.dtype == torch.bfloat16 and wp.shape[1] == bf16_pack_len(Co, Ci, 1)
    return _gather(wp, _bf16_index(Co, Ci, 1, 0))


def decode_bf16_hilo(wp, Co, Ci):
    """hi / lo pack (B, bf16_pack_len(.., 2)) -> (hi, lo), each (B, MT*16, KK*32) bfloat16 with the padding included."""
    assert wp.dtype == torch.bfloat16 and wp.shape[1] == bf16_pack_len(Co, Ci, 2)
    return _gather(wp, _bf16_index(Co, Ci, 2, 0)), _gather(wp, _bf16_index(Co, Ci, 2, 1))


def _padded(W, rows, cols):
    B, Co, Ci = W.shape
    P = torch.zeros((B, rows, cols), dtype=W.dtype)
    P[:, :Co, :Ci] = W
    return P


def encode_fp32(W):
    """W (B, Co, Ci) float32 -> the fp32 pack (B, fp32_pack_len): [ks][mt][lane >> 4][lane & 15] <- [mt][m][ks][kq]."""
    assert W.dtype == torch.float32 and W.shape[2] % 4 == 0
    B, Co, Ci = W.shape
    MT = _mt(Co)
    P = _padded(W, MT * 16, Ci).reshape(B, MT, 16, Ci // 4, 4)
    return P.permute(0, 3, 1, 4, 2).contiguous().reshape(B, -1)


def split_bf16(v):
    """fp32 tensor -> (hi = bf16(v), lo = bf16(v - hi)), the arithmetic of the hi / lo packs."""
    hi = v.to(torch.bfloat16)
    return hi, (v - hi.float()).to(torch.bfloat16)


def _frag_order(P, B, MT, KK):
    # [mt][m][kk][kq][i] -> [kk][mt][kq][m][i]: the 512 values of a fragment are lane-major, lane = kq * 16 + m
    return P.reshape(B, MT, 16, KK, 4, 8).permute(0, 3, 1, 4, 2, 5).contiguous().reshape(B, KK, MT, 512)


def encode_b16(W):
    """W (B, Co, Ci) float32 -> the plain bf16 pack (B, bf16_pack_len(.., 1))."""
    assert W.dtype == torch.float32
    B, Co, Ci = W.shape
    MT, KK = _mt(Co), _kk(Ci)
    return _frag_order(_padded(W, MT * 16, KK * 32).to(torch.bfloat16), B, MT, KK).reshape(B, -1)


def encode_bf16_hilo(W):
    """W (B, Co, Ci) float32 -> the hi / lo pack (B, bf16_pack_len(.., 2)): the two fragments of a (kk, mt) are neighbours."""
    assert W.dtype == torch.float32
    B, Co, Ci = W.shape
    MT, KK = _mt(Co), _kk(Ci)
    hi, lo = split_bf16(_padded(W, MT * 16, KK * 32))
    return torch.stack([_frag_order(hi, B, MT, KK), _frag_order(lo, B, MT, KK)], dim=3).reshape(B, -1)


def padding_mask(Co, Ci, rows, cols):
    """(rows, cols) bool: True on the padding of a decoded matrix."""
    m = np.ones((rows, cols), dtype=bool)
    m[:Co, :Ci] = False
    return m


def is_plus_zero(t):
    """Element-wise: the bit pattern is +0 (a -0 or a denormal is not)."""
    bits = t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)
    return (bits == 0).numpy()


# ------------------------------------------------------------------------------------------------------------------- bounds
# The kernels form v = fl32(sum_k att_k bank_k) as a chain of K fmas from 0: |v - W| <= K u32 A to first order (every partial
# sum is bounded by A and each of the K fmas rounds once).  SLACK covers a compiler that splits an fma.
def aggregate_bound(A, K, W=None, scale=None):
    """|out - W| for out = fl(v) (scale None) or fl(v * scale): K u32 A |scale| + u32 |scale W| (W: the SCALED fp64 value)."""
    if scale is None:
        return SLACK * K * U32 * A
    return SLACK * (K * U32 * A * np.abs(scale) + U32 * np.abs(W))


def b16_pack_bound(W, A, K):
    """plain bf16: |bf16(v) - W| <= u16 |v| + |v - W| <= u16 |W| + (1 + u16) K u32 A."""
    return SLACK * (U16 * np.abs(W) + (1.0 + U16) * K * U32 * A)


def hilo_pack_bound(W, A, K):
    """hi = bf16(v), lo = bf16(v - hi): v - hi is exact in fp32 and at most u16 |v|, so |hi + lo - v| <= u16^2 |v| and
    |hi + lo - W| <= u16^2 |W| + (1 + u16^2) K u32 A."""
    return SLACK * (U16 * U16 * np.abs(W) + (1.0 + U16 * U16) * K * U32 * A)


def emulate_aggregate_fp32(bank, att):
    """The kernel's arithmetic on the CPU: an fp32 fma chain over k from 0 (each step computed in fp64 and rounded once to
    fp32 - a 24 x 24 bit product plus a 24 bit addend is exact in fp64, so this IS the fma)."""
    bank, att = np.asarray(bank, dtype=np.float32), np.asarray(att, dtype=np.float32)
    acc = np.zeros((att.shape[0], bank.shape[1]), dtype=np.float32)
    for k in range(bank.shape[0]):
        acc = (att[:, k:k + 1].astype(np.float64) * bank[k][None, :].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


# ------------------------------------------------------------------------------------------- per-sample 1x1 conv (fp32 pack)
def _act(v, act):
    if act == 1:
        return np.maximum(v, 0.0)
    if act == 2:
        return v * np.clip(v + 3.0, 0.0, 6.0) / 6.0
    return v


def pw_conv_dyn(x, W, bias, act, res=None):
    """x (B, Ci, S), W (B, Co, Ci), bias (Co,) -> (y (B, Co, S) = act(W_b x_b + bias) [+ res], bound (B, Co, S)).
    bound = (Ci + 2) u32 M on the pre-activation, M = sum_i |w||x| + |bias| (the bias is one more term of the same sum); the
    activations are 1-Lipschitz except Hardswish (slope <= 1.5); the residual add rounds once more: + u32 |res|."""
    x, W, bias = _f64(x), _f64(W), _f64(bias)
    Ci = W.shape[2]
    pre = np.einsum("boi,bis->bos", W, x) + bias[None, :, None]
    M = np.einsum("boi,bis->bos", np.abs(W), np.abs(x)) + np.abs(bias)[None, :, None]
    y = _act(pre, act)
    bound = (Ci + 2) * U32 * M * (1.5 if act == 2 else 1.0)
    if res is not None:
        y = y + _f64(res)
        bound = bound + U32 * np.abs(_f64(res))
    return y, bound


# ------------------------------------------------------------------------------------------------- gradients of the aggregate
def bank_grad(G, att, bank):
    """G (B, N), att (B, K), bank (K, N) -> (dbank (K, N) = att^T G, datt (B, K) = G bank^T, bound of dbank = B u32 sum_b
    |att||G|, bound of datt = N u32 sum_n |G||bank|): worst-case bounds of a B- (N-) term fp32 sum in any order."""
    G, att, bank = _f64(G), _f64(att), _f64(bank)
    B, N = G.shape
    return (att.T @ G, G @ bank.T, B * U32 * (np.abs(att).T @ np.abs(G)), N * U32 * (np.abs(G) @ np.abs(bank).T))


# ---------------------------------------------------------------------------------------- shared cases of the CPU / GPU tests
# (Co, Ci, K, B, samples per block the bf16 pack kernels launch with, samples of the tail block): the smallest batches that
# reach each SB for the two geometries - MT * pieces * ceil(B / SB) >= 2048 with MT = 13, pieces = 1 and MT = 5, pieces = 2
#   200 x 36 : last m-tile 8 rows, KK = 2 with 4 real columns in the last chunk
#   72 x 260 : two 256-column pieces (the second 4 columns wide), KK = 9
BF16_PACK_CASES = (
    (200, 36, 4, 5, 1, 1), (200, 36, 4, 317, 2, 1), (200, 36, 4, 633, 4, 1), (200, 36, 4, 1259, 8, 3),
    (72, 260, 4, 411, 2, 1), (72, 260, 4, 819, 4, 3),
    (200, 36, 3, 317, 2, 1), (200, 36, 5, 317, 2, 1),             # K != 4: the kernel without register-resident bank tiles
)


def pack_operands(B, K, Co, Ci, seed=0):
    """bank (K, Co*Ci) of scale Ci^-1/2 and att (B, K) = softmax(3 randn): a different, peaked attention row per sample."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * B + 101 * K + 13 * Co + Ci)
    bank = torch.randn(K, Co * Ci, generator=g) * Ci ** -0.5
    att = torch.softmax(3.0 * torch.randn(B, K, generator=g), dim=-1)
    return bank, att
