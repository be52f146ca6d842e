"""tests/glue_ref.py (the fp64 oracle of the training-loop glue kernels and the DyMN head tails) on the CPU:
  * `kd_loss` against the torch-op formulation of the reference loop (ex_audioset.py:142-189) in torch.float64, gradient by
    autograd, to 1e-12 relative, for the four (mix, kd) combinations;
  * `dyn_heads_fwd` / `_bwd` against fp64 autograd of softmax / sigmoid;
  * fp32 numpy emulations of the kernels' formulas and summation orders over the sweeps of tests/test_gpu_glue_kernels.py:
    each must stay within HALF of the bound the GPU test asserts, which is what sizes those bounds (the mix-up, whose
    bound is the worst case of its three roundings, within the bound itself).
"""
import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import glue_ref as G

f32 = np.float32


def _reference_loss(y_hat, y, rn, lam, teacher_probs, indices, kd_lambda):
    """ex_audioset.py:142-189 in torch ops (the formulation of tests/test_gpu_trainloop.py), dtype of its operands."""
    bs = y_hat.shape[0]
    distillation_loss = nn.BCEWithLogitsLoss(reduction="none")
    if rn is not None:
        y_mix = y * lam.reshape(bs, 1) + y[rn] * (1. - lam.reshape(bs, 1))
    else:
        y_mix = y
    label_loss = F.binary_cross_entropy_with_logits(y_hat, y_mix, reduction="none").mean()
    if kd_lambda > 0 and teacher_probs is not None:
        unknown = indices == -1
        soft = teacher_probs[indices]
        if rn is not None:
            st = distillation_loss(y_hat, soft).mean(dim=1) * lam.reshape(bs) + \
                distillation_loss(y_hat, soft[rn]).mean(dim=1) * (1. - lam.reshape(bs))
        else:
            st = distillation_loss(y_hat, soft).mean(dim=1)
        st = torch.where(unknown, torch.zeros_like(st), st).mean()
        label_loss = kd_lambda * label_loss
        st = (1 - kd_lambda) * st
    else:
        st = torch.zeros((), dtype=y_hat.dtype)
    return label_loss + st, label_loss, st


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("mix,kd", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("B,C", [(1, 1), (2, 65), (9, 527)])
def test_kd_loss_oracle_equals_the_fp64_torch_formulation(mix, kd, B, C):
    for perm in G.kd_perms(B):
        c = G.kd_case(B, C, 3.0)
        t64 = {k: torch.from_numpy(v).double() for k, v in c.items() if k in ("z", "y", "lam", "teacher")}
        z = t64["z"].clone().requires_grad_(True)
        rn = torch.from_numpy(perm).long() if mix else None
        loss, lab, st = _reference_loss(z, t64["y"], rn, t64["lam"] if mix else None, t64["teacher"] if kd else None,
                                        torch.from_numpy(c["idx"]), G.KD_LAMBDA if kd else 0.0)
        loss.backward()
        got = G.kd_loss(c["z"], c["y"], perm if mix else None, c["lam"] if mix else None, c["teacher"] if kd else None,
                        c["idx"] if kd else None, G.KD_LAMBDA if kd else 1.0)
        assert _rel(got[0], loss.item()) <= 1e-12 and _rel(got[1], lab.item()) <= 1e-12
        assert abs(got[2] - st.item()) <= 1e-12 * abs(loss.item())
        assert _rel(got[3], z.grad.numpy()) <= 1e-12


def test_kd_loss_oracle_index_semantics_by_hand():
    """-1 reads the LAST teacher row; the sample's own flag alone zeroes its term; the partner's row counts whatever its flag."""
    z = np.zeros((2, 1))
    y = np.zeros((2, 1))
    teacher = np.array([[0.0], [1.0], [0.25]])
    ln2 = np.log(2.0)                                            # BCE(0, t) = log 2 for every t: the loss cannot tell rows apart,
    lam = np.array([0.5, 0.5])                                   # the gradient sigmoid(0) - t can
    _, _, kd, dz = G.kd_loss(z, y, [1, 0], lam, teacher, [1, -1], 0.0)
    assert kd == pytest.approx(0.5 * ln2)                        # sample 1 is unknown: only sample 0 contributes
    assert dz[1, 0] == 0.0
    assert dz[0, 0] == pytest.approx((0.5 - (0.5 * 1.0 + 0.5 * 0.25)) / 2)   # partner -1 -> the last row (0.25), used
    _, lab, kd, dz = G.kd_loss(z, y, None, None, teacher, [-1, -1], 0.25)
    assert kd == 0.0 and lab == pytest.approx(0.25 * ln2) and np.allclose(dz, 0.25 * 0.5 / 2)
    loss, lab, kd, _ = G.kd_loss(z, y, None, None, None, None, 0.25)
    assert loss == lab == pytest.approx(ln2) and kd == 0.0       # no teacher: kd_lambda is not applied


def test_mixup_and_col_sum_oracles_by_hand():
    x = np.array([[1.0, 2.0], [10.0, 20.0], [100.0, 200.0]], dtype=f32)
    out = G.mixup(x, [2, 1, 0], np.array([1.0, 0.25, 0.0], dtype=f32))
    assert np.array_equal(out, [[1.0, 2.0], [10.0, 20.0], [1.0, 2.0]])
    assert np.array_equal(G.col_sum(x), [111.0, 222.0])
    assert G.col_row_blocks(512, 300) == 1 and G.col_row_blocks(513, 300) == 9 and G.col_row_blocks(1100, 1) == 18


@pytest.mark.parametrize("n_att,K,cexp", [(1, 1, 1), (2, 3, 5), (3, 32, 7)])
def test_dyn_heads_oracle_equals_fp64_autograd(n_att, K, cexp):
    B = 4
    c = G.heads_case(B, n_att, K, cexp, 3.0)
    y = torch.from_numpy(c["y"]).double().requires_grad_(True)
    lam4, iv4 = torch.from_numpy(G.HEAD_LAM4).double(), torch.from_numpy(G.HEAD_IV4).double()
    att_t = torch.stack([torch.softmax(y[:, i * K:(i + 1) * K] * G.HEAD_INV_T[i], dim=1) for i in range(n_att)])
    sg_t = torch.sigmoid(y[:, n_att * K:])
    coef_t = (2 * sg_t.reshape(B, cexp, 4) - 1) * lam4 + iv4
    att, sg, coef = G.dyn_heads_fwd(c["y"], n_att, K, cexp, G.HEAD_INV_T, G.HEAD_LAM4, G.HEAD_IV4)
    assert _rel(att, att_t.detach().numpy()) <= 1e-12 and _rel(sg, sg_t.detach().numpy()) <= 1e-12
    assert _rel(coef, coef_t.detach().numpy()) <= 1e-12
    datt, dcoef = torch.from_numpy(c["datt"]).double(), torch.from_numpy(c["dcoef"]).double()
    ((att_t * datt).sum() + (coef_t * dcoef).sum()).backward()
    dy = G.dyn_heads_bwd(c["datt"], c["dcoef"], att, sg, G.HEAD_LAM4, G.HEAD_INV_T)
    assert _rel(dy, y.grad.numpy()) <= 1e-12


# ------------------------------------------------------------------ fp32 emulations of the kernels: they size the GPU bounds
def _sig32(z):
    with np.errstate(over="ignore"):                             # exp(100) = inf in fp32, 1 / (1 + inf) = 0: as in the kernel
        return f32(1.0) / (f32(1.0) + np.exp(-z))


def _bce32(z, t):
    return np.maximum(z, f32(0.0)) - z * t + np.log1p(np.exp(-np.abs(z)))


def _block_sum32(v):
    """A 256-thread block's sum of per-column terms v (C,) in the kernel's order: thread t adds columns t, t + 256, ... in
    turn, a 64-lane xor butterfly per wave, the four wave sums left to right."""
    C = v.shape[0]
    pad = np.zeros(((C + 255) // 256) * 256, dtype=f32)
    pad[:C] = v
    acc = np.zeros(256, dtype=f32)
    for trip in pad.reshape(-1, 256):
        acc = acc + trip
    lanes = np.arange(256)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[lanes ^ o]
    return ((acc[0] + acc[64]) + acc[128]) + acc[192]


def emulate_kd_loss(z, y, perm, lam, teacher, idx, kd_lambda):
    """kd_loss_kernel in numpy fp32 -> (sums (3,), dz)."""
    B, C = z.shape
    kd_lambda = f32(kd_lambda)
    kd = teacher is not None and kd_lambda < 1
    inv = f32(1.0) / (f32(B) * f32(C))
    sums, dz = np.zeros(3, dtype=f32), np.empty((B, C), dtype=f32)
    for b in range(B):
        pb = b if perm is None else int(perm[b])
        l = f32(1.0) if perm is None else f32(lam[b])
        m = f32(1.0) - l
        ym = y[b] * l + (y[pb] * m if perm is not None else f32(0.0))
        sg = _sig32(z[b])
        wl, wk = (kd_lambda, (f32(1.0) - kd_lambda) * f32(idx[b] >= 0)) if kd else (f32(1.0), f32(0.0))
        g = wl * (sg - ym)
        s_kd = f32(0.0)
        if kd:
            ta, tb = teacher[idx[b]], teacher[idx[pb]]           # numpy's [-1] is the last row, like the kernel's
            s_kd = _block_sum32(_bce32(z[b], ta) * l + _bce32(z[b], tb) * m)
            g = g + wk * (sg - (ta * l + tb * m))
        dz[b] = g * inv
        a = _block_sum32(_bce32(z[b], ym)) * inv * wl
        k = s_kd * inv * wk
        sums += np.array([a + k, a, k], dtype=f32)
    return sums, dz


@pytest.mark.parametrize("C", G.KD_C)
def test_fp32_emulation_of_the_kd_loss_stays_within_half_the_bounds(C):
    worst = [0.0, 0.0]
    for B in (1, 2, 9):
        for scale in (3.0, 30.0):
            c = G.kd_case(B, C, scale)
            for perm in G.kd_perms(B):
                for mix, kd, w in [(True, True, G.KD_LAMBDA), (True, False, 1.0), (False, True, G.KD_LAMBDA),
                                   (False, False, 1.0), (True, True, 0.0)]:
                    args = (c["z"], c["y"], perm if mix else None, c["lam"] if mix else None, c["teacher"] if kd else None,
                            c["idx"] if kd else None, w)
                    sums, dz = emulate_kd_loss(*args)
                    ref = G.kd_loss(*args)
                    b_loss, b_grad = G.kd_bounds(c["z"])
                    worst[0] = max(worst[0], max(abs(float(sums[i]) - ref[i]) for i in range(3)) / b_loss)
                    worst[1] = max(worst[1], float(np.abs(dz - ref[3]).max()) / b_grad)
    print(f"kd emulation C={C}: loss terms {worst[0] * 16:.2f}, gradient {worst[1] * 16:.2f} (units of eps x scale; bound 16)")
    assert worst[0] <= 0.5 and worst[1] <= 0.5


def test_fp32_emulation_of_the_mixup_stays_within_the_bound():
    """Two products and one sum, each rounded once, with 1 - lam exact (lam >= 0.5, or 0): 2 eps (|x| lam + |x_perm| (1 - lam))
    is the worst case of this unfused form itself, not a margin over it - so it is the bound, not half of it, that holds here
    (the kernel may contract one product into an fma, which only removes a rounding)."""
    rng = np.random.default_rng(5)
    x = rng.standard_normal((3, 65541)).astype(f32)
    perm, lam = np.array([2, 1, 0]), np.array([1.0, 0.0, 0.7], dtype=f32)
    l = lam.reshape(3, 1)
    got = x * l + x[perm] * (f32(1.0) - l)
    err = np.abs(got - G.mixup(x, perm, lam))
    bound = G.mixup_bound(x, perm, lam)
    assert np.all(err <= bound)
    assert np.array_equal(got[0], x[0])


def emulate_col_sum(m):
    """Either col_sum kernel in numpy fp32, every column at once."""
    R, C = m.shape
    zero = np.zeros(C, dtype=f32)
    if R <= 512:                                                 # col_sum_det_kernel: 8 row groups, two accumulators each
        part = []
        for g in range(8):
            a0, a1, r = zero.copy(), zero.copy(), g
            while r + 8 < R:
                a0, a1, r = a0 + m[r], a1 + m[r + 8], r + 16
            if r < R:
                a0 = a0 + m[r]
            part.append(a0 + a1)
        return ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]))
    cb = (C + 63) // 64
    rows = max(64, (R * cb + 1023) // 1024)
    out = zero.copy()
    for r0 in range(0, R, rows):                                 # col_sum_kernel: 4 row groups, four accumulators each
        r1 = min(r0 + rows, R)
        part = []
        for ty in range(4):
            a, r = [zero.copy() for _ in range(4)], r0 + ty
            while r + 12 < r1:
                a = [a[i] + m[r + 4 * i] for i in range(4)]
                r += 16
            while r < r1:
                a[0], r = a[0] + m[r], r + 4
            part.append((a[0] + a[1]) + (a[2] + a[3]))
        out = out + ((part[0] + part[1]) + (part[2] + part[3]))
    return out


@pytest.mark.parametrize("R", G.COL_R)
def test_fp32_emulation_of_the_column_sums(R):
    for C in G.COL_C:
        mi = G.col_case(R, C, "int")
        assert np.array_equal(emulate_col_sum(mi).astype(np.float64), G.col_sum(mi))      # the emulation drops no row
        mg = G.col_case(R, C, "gauss")
        assert np.all(np.abs(emulate_col_sum(mg) - G.col_sum(mg)) <= 0.5 * G.col_sum_bound(mg))


def emulate_heads_fwd(y, n_att, K, cexp, inv_t, lam4, iv4):
    B = y.shape[0]
    att = np.empty((n_att, B, K), dtype=f32)
    for i in range(n_att):
        s = y[:, i * K:(i + 1) * K] * f32(inv_t[i])
        e = np.exp(s - s.max(axis=1, keepdims=True))
        tot = np.zeros((B, 1), dtype=f32)
        for k in range(K):
            tot = tot + e[:, k:k + 1]
        att[i] = e * (f32(1.0) / tot)
    sg = _sig32(y[:, n_att * K:])
    coef = (f32(2.0) * sg.reshape(B, cexp, 4) - f32(1.0)) * lam4 + iv4
    return att, sg, coef


def emulate_heads_bwd(datt, dcoef, att, sg, lam4, inv_t):
    n_att, B, K = att.shape
    dy = np.empty((B, n_att * K + sg.shape[1]), dtype=f32)
    for i in range(n_att):
        dot = np.zeros((B, 1), dtype=f32)
        for k in range(K):
            dot = dot + datt[i][:, k:k + 1] * att[i][:, k:k + 1]
        dy[:, i * K:(i + 1) * K] = att[i] * (datt[i] - dot) * f32(inv_t[i])
    dy[:, n_att * K:] = (dcoef * lam4).reshape(B, -1) * (f32(2.0) * sg * (f32(1.0) - sg))
    return dy


@pytest.mark.parametrize("n_att", G.HEAD_N_ATT)
@pytest.mark.parametrize("K", G.HEAD_K)
def test_fp32_emulation_of_the_dynamic_heads_stays_within_half_the_bounds(n_att, K):
    for cexp in (1, 65, 960):
        for scale in (1.0, 40.0):
            c = G.heads_case(5, n_att, K, cexp, scale)
            cfg = (n_att, K, cexp, G.HEAD_INV_T, G.HEAD_LAM4, G.HEAD_IV4)
            att, sg, coef = emulate_heads_fwd(c["y"], *cfg)
            r_att, r_sg, r_coef = G.dyn_heads_fwd(c["y"], *cfg)
            b_att, b_sg, b_coef = G.heads_fwd_bounds(c["y"], *cfg)
            assert np.all(np.abs(att - r_att) <= 0.5 * b_att) and np.all(np.abs(sg - r_sg) <= 0.5 * b_sg)
            assert np.all(np.abs(coef - r_coef) <= 0.5 * b_coef)
            dy = emulate_heads_bwd(c["datt"], c["dcoef"], att, sg, G.HEAD_LAM4, G.HEAD_INV_T)
            ref = G.dyn_heads_bwd(c["datt"], c["dcoef"], att, sg, G.HEAD_LAM4, G.HEAD_INV_T)
            assert np.all(np.abs(dy - ref) <= 0.5 * G.heads_bwd_bound(c["datt"], c["dcoef"], G.HEAD_LAM4, G.HEAD_INV_T))
