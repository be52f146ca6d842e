"""fp64 numpy oracle of the training-loop glue kernels (csrc/train_glue.hip) and of the DyMN head tails (csrc/dymn.hip:
eat_dyn_heads_fwd / _bwd) - a helper, not a test module.  Every input is widened to fp64 first, so an fp32 operand enters with
exactly the value the kernel reads.

`kd_loss` has the semantics of the reference loop (ex_audioset.py:149-189) as include/eat_hip.h states them:
  * index -1 selects the LAST teacher row (`teacher_preds[-1]`);
  * only the sample's OWN unknown flag zeroes its distillation term; the mix-up partner's row is used whatever its status;
  * loss = kd_lambda * label + (1 - kd_lambda) * kd with a teacher, loss = label without one.
"""
import numpy as np

EPS = 2.0 ** -24                                               # unit round-off of fp32


def _f64(a):
    return np.asarray(a).astype(np.float64)


def sigmoid(z):
    z = _f64(z)
    e = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def bce_with_logits(z, t):
    """max(z, 0) - z t + log(1 + exp(-|z|)) element-wise."""
    z, t = _f64(z), _f64(t)
    return np.maximum(z, 0.0) - z * t + np.log1p(np.exp(-np.abs(z)))


def kd_loss(z, y, perm, lam, teacher, idx, kd_lambda):
    """-> (loss, weighted label part, weighted distillation part, dz (B, C)).  perm / lam None: no mix-up; teacher None: the
    pure label loss (kd_lambda is not applied)."""
    z, y = _f64(z), _f64(y)
    B, C = z.shape
    if perm is None:
        perm, lam = np.arange(B), np.ones(B)
    perm, lam = np.asarray(perm).astype(np.int64), _f64(lam).reshape(B, 1)
    ym = y * lam + y[perm] * (1.0 - lam)
    sg = sigmoid(z)
    label = bce_with_logits(z, ym).mean()
    dz = (sg - ym) / (B * C)
    if teacher is None:
        return label, label, 0.0, dz
    teacher, idx = _f64(teacher), np.asarray(idx).astype(np.int64)
    known = (idx != -1).astype(np.float64).reshape(B, 1)
    rows = np.where(idx < 0, teacher.shape[0] + idx, idx)         # python's teacher[-1]: the last row
    ta, tb = teacher[rows], teacher[rows[perm]]
    kd_rows = bce_with_logits(z, ta).mean(axis=1, keepdims=True) * lam + \
        bce_with_logits(z, tb).mean(axis=1, keepdims=True) * (1.0 - lam)
    kd = (kd_rows * known).mean()
    w = float(kd_lambda)
    dz = w * dz + (1.0 - w) * known * (sg - (ta * lam + tb * (1.0 - lam))) / (B * C)
    return w * label + (1.0 - w) * kd, w * label, (1.0 - w) * kd, dz


def mixup(x, perm, lam):
    x = _f64(x)
    lam = _f64(lam).reshape((-1,) + (1,) * (x.ndim - 1))
    return x * lam + x[np.asarray(perm).astype(np.int64)] * (1.0 - lam)


def col_sum(m):
    return _f64(m).sum(axis=0)


def dyn_heads_fwd(y, n_att, K, cexp, inv_t, lam4, iv4):
    """y (B, n_att*K + 4*cexp) -> (att (n_att, B, K) = softmax(y_head * inv_t[head]), sg (B, 4*cexp), coef (B, cexp, 4) =
    (2 sg - 1) * lam4[m] + iv4[m])."""
    y, lam4, iv4 = _f64(y), _f64(lam4), _f64(iv4)
    B = y.shape[0]
    att = np.empty((n_att, B, K))
    for i in range(n_att):
        s = y[:, i * K:(i + 1) * K] * float(inv_t[i])
        e = np.exp(s - s.max(axis=1, keepdims=True))
        att[i] = e / e.sum(axis=1, keepdims=True)
    sg = sigmoid(y[:, n_att * K:])
    coef = (2.0 * sg.reshape(B, cexp, 4) - 1.0) * lam4 + iv4
    return att, sg, coef


def dyn_heads_bwd(datt, dcoef, att, sg, lam4, inv_t):
    """The backward formula in fp64 from the GIVEN att / sg: -> dy (B, n_att*K + 4*cexp)."""
    datt, dcoef, att, sg, lam4 = _f64(datt), _f64(dcoef), _f64(att), _f64(sg), _f64(lam4)
    n_att, B, K = att.shape
    dy = np.empty((B, n_att * K + sg.shape[1]))
    for i in range(n_att):
        dot = (datt[i] * att[i]).sum(axis=1, keepdims=True)
        dy[:, i * K:(i + 1) * K] = att[i] * (datt[i] - dot) * float(inv_t[i])
    dy[:, n_att * K:] = (dcoef.reshape(B, -1, 4) * lam4).reshape(B, -1) * (2.0 * sg * (1.0 - sg))
    return dy


# ---------------------------------------------------------------- shared cases and bounds of the CPU and the GPU test files
KD_C = (1, 63, 64, 65, 255, 256, 257, 527, 1000)               # the 256-thread column loop: < one wave, 256 +- 1, several trips
KD_N_TEACHER = 7
# B = 9: sample 0 is a fixed point of the permutation; sample 1 is KNOWN with an UNKNOWN partner (2), sample 2 UNKNOWN with a
# KNOWN partner (1), sample 3 UNKNOWN with an UNKNOWN partner (4); rows 0 (all 0.0), 1 (all 1.0) and the last one are all used
# B = 2: the known sample 0 has lam = 0.5, so that under the swap its unknown partner's row (the last one) carries weight
_KD_PERM = {1: [[0]], 2: [[0, 1], [1, 0]], 9: [[0, 2, 1, 4, 5, 3, 7, 8, 6]]}
_KD_IDX = {1: [3], 2: [3, -1], 9: [0, 1, -1, -1, -1, 6, 2, 5, 4]}
_KD_LAM = {1: [0.5], 2: [0.5, 1.0], 9: [0.8125, 0.5, 0.6, 0.9, 0.55, 0.7, 1.0, 0.97, 0.51]}


def kd_perms(B):
    """The permutations a KD case of batch B is run with: each has a fixed point; B = 2 adds the swap, without which no
    sample there would have a partner other than itself."""
    return [np.array(p, dtype=np.int32) for p in _KD_PERM[B]]


def kd_case(B, C, scale, seed=0):
    """-> dict of fp32 / integer numpy operands: logits of the given scale with elements forced to +-100, 5 % labels, a
    7-row teacher table (row 0 all 0.0, row 1 all 1.0, a last row unlike the others), lam with an exact 1.0 and 0.5."""
    rng = np.random.default_rng(1000 * B + C + seed)
    z = (rng.standard_normal((B, C)) * scale).astype(np.float32)
    hit = rng.random((B, C)) < 0.02
    z[hit] = np.where(rng.random(int(hit.sum())) < 0.5, 100.0, -100.0).astype(np.float32)
    y = (rng.random((B, C)) < 0.05).astype(np.float32)
    z.flat[0], y.flat[0] = 100.0, 1.0                             # saturated on the side of its label: a term of ~0
    if z.size > 1:
        z.flat[-1], y.flat[-1] = -100.0, 1.0                      # saturated against its label: a term of 100, gradient -1
    else:
        y.flat[0] = 0.0                                           # (one element: the costly side, so that dropping it shows)
    teacher = (1.0 / (1.0 + np.exp(-(rng.standard_normal((KD_N_TEACHER, C)) * 2 - 2)))).astype(np.float32)
    teacher[0], teacher[1] = 0.0, 1.0
    teacher[-1] = (0.25 + 0.5 * rng.random(C)).astype(np.float32)
    return dict(z=z, y=y, perm=kd_perms(B)[0], lam=np.array(_KD_LAM[B], dtype=np.float32), teacher=teacher,
                idx=np.array(_KD_IDX[B], dtype=np.int64))


def kd_bounds(z):
    """(bound of each of the three loss terms, bound of every gradient element) - from the kernel's arithmetic: every BCE term
    carries a rounding error proportional to 1 + |z|, all terms are non-negative, about C/256 + 10 + B additions."""
    z = _f64(z)
    return 16.0 * EPS * float(np.mean(1.0 + np.abs(z))), 16.0 * EPS / z.size


def mixup_bound(x, perm, lam):
    x = _f64(x)
    lam = _f64(lam).reshape((-1,) + (1,) * (x.ndim - 1))
    return 2.0 * EPS * (np.abs(x) * lam + np.abs(x[np.asarray(perm).astype(np.int64)]) * (1.0 - lam))


COL_R = (1, 7, 8, 9, 15, 16, 17, 511, 512, 513, 575, 577, 1100)   # row groups of 8 / 16, the 512 | 513 kernel switch, 64-row blocks
COL_C = (1, 31, 32, 33, 63, 64, 65, 300)                           # the 32- and 64-column block edges


def col_row_blocks(R, C):
    """Number of row blocks whose partial sums meet in one output element: 1 for the fixed-order kernel (R <= 512), the grid
    height of the atomic kernel (~1024 blocks of at least 64 rows) above."""
    if R <= 512:
        return 1
    cb = (C + 63) // 64
    rows = max(64, (R * cb + 1023) // 1024)
    return (R + rows - 1) // rows


def col_sum_bound(m):
    """Per column: (R/16 + 8 + row blocks) eps sum_r |m[r, c]| - the worst-case summation bound of either kernel (a thread's
    longest chain has ~R/16 additions, the trees and the block combination the rest)."""
    m = _f64(m)
    R, C = m.shape
    return (R / 16.0 + 8.0 + col_row_blocks(R, C)) * EPS * np.abs(m).sum(axis=0)


def col_case(R, C, kind):
    rng = np.random.default_rng(R * 10007 + C)
    if kind == "int":                                             # |partial sums| <= 8 * 1100 < 2^24: exact in fp32
        return rng.integers(-8, 9, (R, C)).astype(np.float32)
    return rng.standard_normal((R, C)).astype(np.float32)


# three DISTINCT inverse temperatures, as the fp32 values the entry point receives
HEAD_INV_T = tuple(float(np.float32(v)) for v in (1.0 / 30.0, 1.0 / 7.0, 1.0))
KD_LAMBDA = float(np.float32(0.1))                                 # the flagship weight, as the fp32 value the kernel receives
HEAD_LAM4 = np.array([1.0, 0.5, -0.75, 0.3], dtype=np.float32)     # distinct per j & 3
HEAD_IV4 = np.array([1.0, -0.25, 0.125, 0.6], dtype=np.float32)
HEAD_N_ATT, HEAD_K, HEAD_CEXP, HEAD_B = (1, 2, 3), (1, 3, 4, 32), (1, 63, 64, 65, 960), (1, 5)


def heads_case(B, n_att, K, cexp, scale):
    rng = np.random.default_rng(B * 100003 + n_att * 10007 + K * 1009 + cexp + int(scale))
    W = n_att * K + 4 * cexp
    return dict(y=(rng.standard_normal((B, W)) * scale).astype(np.float32),
                datt=rng.standard_normal((n_att, B, K)).astype(np.float32),
                dcoef=rng.standard_normal((B, cexp, 4)).astype(np.float32))


def heads_fwd_bounds(y, n_att, K, cexp, inv_t, lam4, iv4):
    """-> (att bound (n_att, 1, 1), sg bound, coef bound (4,))."""
    y = _f64(y)
    att = np.array([(4.0 + 2.0 * np.abs(y[:, i * K:(i + 1) * K] * float(inv_t[i])).max()) * EPS for i in range(n_att)])
    return att.reshape(n_att, 1, 1), 4.0 * EPS, 8.0 * EPS * (np.abs(_f64(lam4)) + np.abs(_f64(iv4)))


def heads_bwd_bound(datt, dcoef, lam4, inv_t):
    """-> bound (B, n_att*K + 4*cexp): attention columns (K + 6) eps |inv_t| max_k |datt_k|, coefficient columns
    4 eps |dcoef lam_m|."""
    datt, dcoef = _f64(datt), _f64(dcoef)
    n_att, B, K = datt.shape
    a = [np.repeat((K + 6.0) * EPS * abs(float(inv_t[i])) * np.abs(datt[i]).max(axis=1, keepdims=True), K, axis=1)
         for i in range(n_att)]
    return np.concatenate(a + [(4.0 * EPS * np.abs(dcoef * _f64(lam4))).reshape(B, -1)], axis=1)
