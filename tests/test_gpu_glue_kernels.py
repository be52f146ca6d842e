"""The glue kernels of the AudioSet knowledge-distillation step (csrc/train_glue.hip: eat_kd_loss_fwd_bwd, eat_mixup_fwd,
eat_wave_i16_to_f32, eat_col_sum) and the DyMN head tails (csrc/dymn.hip: eat_dyn_heads_fwd / _bwd) against the fp64 numpy
oracle tests/glue_ref.py, at the shapes where their launches change: the 256-thread column loop of the loss (C < 64, 256 +- 1),
the 64-block grid cap of the mix-up, the grid-stride loop of the int16 transport, the row groups, the 512 | 513 kernel switch
and the 32- / 64-column blocks of the column sums, every (n_att, K) of the heads with three distinct temperatures.

Every bound is a formula of tests/glue_ref.py (eps = 2^-24), sized by the fp32 emulations of tests/test_glue_ref_cpu.py, which
stay within half of each.  Integer-valued column sums, the int16 transport, lam = 1 rows of the mix-up, the zeroed loss terms
and the scaled backward are compared for equality.

Largest errors observed on an MI355X, in units of the bound (`pytest -s` prints them):
  KD loss      each loss term 0.07 (1.1 of the 16 units), gradient 0.18 (2.9 of 16; the CPU emulation: 1.0 and 3.0 units)
  mix-up       0.88 (the bound is the worst case of its roundings, not a margin over it)
  column sums  Gaussian 0.17; integer-valued matrices equal the fp64 sums
  heads        att 0.21, sg 0.37, coef 0.39, backward: attention columns 0.12, coefficient columns 0.39
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from tests import glue_ref as G  # noqa: E402

from efficientat_amd import _lib, ops  # noqa: E402
from efficientat_amd._lib import EatHipError  # noqa: E402
from efficientat_amd.train_loop import KDTrainer, kd_loss  # noqa: E402

DEV = torch.device("cuda:0")
MODES = [(True, True), (True, False), (False, True), (False, False)]


def _d(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _kd_args(c, perm, mix, kd, w):
    """The operand tuple of one case, as the oracle takes it."""
    return (c["z"], c["y"], perm if mix else None, c["lam"] if mix else None, c["teacher"] if kd else None,
            c["idx"] if kd else None, w)


def _kd_gpu(args):
    """ops.kd_loss_fwd_bwd on a zeroed fp32 `sums` -> (sums (3,) as float64 numpy, dz fp32 numpy)."""
    z, y, perm, lam, teacher, idx, w = args
    sums = torch.zeros(3, device=DEV)
    dz = ops.kd_loss_fwd_bwd(_d(z), _d(y), _d(perm), _d(lam), _d(teacher), _d(idx), w, sums)
    return sums.cpu().numpy().astype(np.float64), dz.cpu().numpy()


def _kd_check(args, worst):
    """One launch against the oracle within the two bounds; -> (sums, dz) for the exact checks of the caller."""
    sums, dz = _kd_gpu(args)
    ref = G.kd_loss(*args)
    b_loss, b_grad = G.kd_bounds(args[0])
    e_loss = max(abs(sums[i] - ref[i]) for i in range(3)) / b_loss
    e_grad = float(np.abs(dz - ref[3]).max()) / b_grad
    worst[0], worst[1] = max(worst[0], e_loss), max(worst[1], e_grad)
    assert e_loss <= 1.0, (sums, ref[:3], b_loss)
    assert e_grad <= 1.0, (float(np.abs(dz - ref[3]).max()), b_grad)
    return sums, dz


def _report(what, worst):
    print(f"\n{what}: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()) + " of the bound")


# ------------------------------------------------------------------ KD loss
@pytest.mark.parametrize("mix,kd", MODES)
@pytest.mark.parametrize("B", [1, 2, 9])
@pytest.mark.parametrize("C", G.KD_C)
def test_kd_loss_and_gradient_against_fp64(C, B, mix, kd):
    worst = [0.0, 0.0]
    for scale in (3.0, 30.0):
        c = G.kd_case(B, C, scale)
        for perm in G.kd_perms(B):
            _kd_check(_kd_args(c, perm, mix, kd, G.KD_LAMBDA if kd else 1.0), worst)
    _report(f"kd loss C={C} B={B} mix={mix} kd={kd}", dict(loss=worst[0], gradient=worst[1]))


@pytest.mark.parametrize("B", [2, 9])
@pytest.mark.parametrize("C", G.KD_C)
def test_kd_all_unknown_batch_has_no_distillation_term(C, B):
    worst = [0.0, 0.0]
    for scale in (3.0, 30.0):
        c = G.kd_case(B, C, scale)
        c["idx"] = np.full(B, -1, dtype=np.int64)
        for perm in G.kd_perms(B):
            for mix in (True, False):
                args = _kd_args(c, perm, mix, True, G.KD_LAMBDA)
                sums, dz = _kd_check(args, worst)
                assert sums[2] == 0.0                                                   # exactly: every weight is 0
                label_grad = G.kd_loss(*_kd_args(c, perm, mix, False, 1.0))[3]          # fp64, no teacher
                assert float(np.abs(dz - G.KD_LAMBDA * label_grad).max()) <= G.kd_bounds(c["z"])[1]
    _report(f"kd all-unknown C={C} B={B}", dict(loss=worst[0], gradient=worst[1]))


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("C", G.KD_C)
def test_kd_lambda_zero_and_one_with_a_teacher(C, B):
    worst = [0.0, 0.0]
    for scale in (3.0, 30.0):
        c = G.kd_case(B, C, scale)
        perm = G.kd_perms(B)[0]
        for w in (0.0, G.KD_LAMBDA, 1.0):
            sums, dz = _kd_check(_kd_args(c, perm, True, True, w), worst)
            if w == 0.0:
                assert sums[1] == 0.0                                                   # the label part is exactly 0.0
            if w == 1.0:                                                                # the pure label loss, teacher unread
                assert sums[2] == 0.0
                ref = G.kd_loss(*_kd_args(c, perm, True, False, 1.0))
                assert abs(sums[0] - ref[0]) <= G.kd_bounds(c["z"])[0]
                assert np.array_equal(dz, _kd_gpu(_kd_args(c, perm, True, False, 1.0))[1])
    _report(f"kd lambda 0 / 0.1 / 1 C={C} B={B}", dict(loss=worst[0], gradient=worst[1]))


@pytest.mark.parametrize("B,C", [(9, 527), (2, 65)])
def test_kd_loss_function_scalar_accumulator_and_scaled_backward(B, C):
    c = G.kd_case(B, C, 3.0)
    perm = G.kd_perms(B)[-1]
    args = _kd_args(c, perm, True, True, G.KD_LAMBDA)
    ref = G.kd_loss(*args)
    b_loss = G.kd_bounds(c["z"])[0]
    t = [_d(a) for a in args[:6]]
    sums = torch.zeros(3, device=DEV, dtype=torch.float64)
    z1 = t[0].clone().requires_grad_(True)
    loss1 = kd_loss(z1, *t[1:], kd_lambda=G.KD_LAMBDA, sums=sums)
    s1 = sums.clone()
    assert loss1.dtype == torch.float32 and loss1.item() == s1[0].item()                # the scalar IS the step's term 0
    assert all(abs(s1[i].item() - ref[i]) <= b_loss for i in range(3))
    z2 = t[0].clone().requires_grad_(True)
    loss2 = kd_loss(z2, *t[1:], kd_lambda=G.KD_LAMBDA, sums=sums)
    # two fp32 terms of one magnitude add exactly in fp64: the accumulator holds the sum of both steps, term by term
    step2 = sums - s1
    assert step2[0].item() == loss2.item()
    assert all(abs(step2[i].item() - ref[i]) <= b_loss for i in range(3))
    # an upstream gradient other than 1: one multiplication, one rounding
    dz = _kd_gpu(args)[1]
    (3.0 * loss1).backward()
    assert np.array_equal(z1.grad.cpu().numpy(), np.float32(3.0) * dz)
    loss2.backward()
    assert np.array_equal(z2.grad.cpu().numpy(), dz)


def test_kd_trainer_with_lambda_zero_trains_on_the_unweighted_label_loss():
    """The reference's `kd_lambda == 0` branch (ex_audioset.py:158, 185-186): teacher logits given, distillation off."""
    B, C = 9, 527
    c = G.kd_case(B, C, 3.0)
    tr = KDTrainer(nn.Linear(2, 2).to(DEV), None, None, teacher_preds=torch.zeros(G.KD_N_TEACHER, C), fname_to_index={"a": 1},
                   kd_lambda=0.0)
    loss = tr._loss(_d(c["z"]), _d(c["y"]), _d(c["perm"]), _d(c["lam"]), _d(c["idx"]))
    ref = G.kd_loss(c["z"], c["y"], c["perm"], c["lam"], None, None, 1.0)
    b_loss = G.kd_bounds(c["z"])[0]
    s = tr.sums.cpu().numpy()
    assert abs(loss.item() - ref[0]) <= b_loss and abs(s[1] - ref[0]) <= b_loss and s[2] == 0.0


def test_kd_and_mixup_refuse_misread_index_tables_and_null_pointers():
    """(tests/test_glue_operands_cpu.py holds the full list on CPU tensors.)  An int64 perm - what torch.randperm returns - or
    an int32 teacher_idx would be read at the wrong width and gather rows out of bounds: refused before any launch."""
    c = G.kd_case(9, 65, 3.0)
    z, y, perm, lam, teacher, idx = (_d(c[k]) for k in ("z", "y", "perm", "lam", "teacher", "idx"))
    sums = torch.zeros(3, device=DEV)
    with pytest.raises(EatHipError, match="kd_loss_fwd_bwd: perm"):
        ops.kd_loss_fwd_bwd(z, y, perm.long(), lam, teacher, idx, 0.1, sums)
    with pytest.raises(EatHipError, match="kd_loss_fwd_bwd: teacher_idx"):
        ops.kd_loss_fwd_bwd(z, y, perm, lam, teacher, idx.int(), 0.1, sums)
    with pytest.raises(EatHipError, match="mixup_fwd: perm"):
        ops.mixup_fwd(z, perm.long(), lam)
    assert float(sums.abs().sum()) == 0.0
    dz = torch.empty_like(z)
    good = [z.data_ptr(), y.data_ptr(), perm.data_ptr(), lam.data_ptr(), teacher.data_ptr(), idx.data_ptr(), G.KD_N_TEACHER, 0.1,
            9, 65, sums.data_ptr(), dz.data_ptr(), None]
    for slot in (0, 1, 10, 11):                                  # logits, y, sums, dlogits
        with pytest.raises(EatHipError, match="must not be NULL"):
            _lib.call("eat_kd_loss_fwd_bwd", *[None if i == slot else a for i, a in enumerate(good)])
    good = [z.data_ptr(), perm.data_ptr(), lam.data_ptr(), dz.data_ptr(), 9, 65, None]
    for slot in range(4):                                        # x, perm, lam, out
        with pytest.raises(EatHipError, match="must not be NULL"):
            _lib.call("eat_mixup_fwd", *[None if i == slot else a for i, a in enumerate(good)])


# ------------------------------------------------------------------ mix-up
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 1024, 65540, 65541])    # float4 and scalar kernels; the last two pass 64 blocks
def test_mixup_against_fp64(n, B):
    x = np.random.default_rng(n * 7 + B).standard_normal((B, n)).astype(np.float32)
    worst = 0.0
    draws = [([1, 2, 0], [1.0, 0.0, 0.7])] if B == 3 else [([0], [lam]) for lam in (1.0, 0.0, 0.7)]
    for perm, lam in draws:
        perm, lam = np.array(perm, dtype=np.int32), np.array(lam, dtype=np.float32)
        got = ops.mixup_fwd(_d(x), _d(perm), _d(lam)).cpu().numpy()
        err, bound = np.abs(got - G.mixup(x, perm, lam)), G.mixup_bound(x, perm, lam)
        assert np.all(err <= bound)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        for b in range(B):
            if lam[b] == 1.0:                                     # lam = 1: the row itself, bit for bit
                assert np.array_equal(got[b], x[b])
            if lam[b] == 0.0:                                     # lam = 0: the partner's row, bit for bit
                assert np.array_equal(got[b], x[perm[b]])
    _report(f"mixup n={n} B={B}", dict(out=worst))


# ------------------------------------------------------------------ int16 -> fp32
def _pcm(n, seed):
    """Full-scale values and packed 32-bit words whose halves differ in sign, both ways round, then random samples."""
    q = np.random.default_rng(seed).integers(-32768, 32768, n).astype(np.int16)
    head = np.array([-32768, 32767, -5, 7, 9, -3, 32767, -32768, -1, 0, 0, -1], dtype=np.int16)
    q[:min(n, head.size)] = head[:n]
    if n > 24:
        q[-12:] = head[::-1]                                      # the same in the tail kernel's reach
    return torch.from_numpy(q)


@pytest.mark.parametrize("n", [1, 7, 9, 15, 16, 17])
def test_int16_transport_is_exact_at_the_vector_edges(n):
    q = _pcm(n, n)
    for scale in (1.0 / 32768.0, 1.0 / 32767.0):
        assert torch.equal(ops.wave_i16_to_f32(q.to(DEV), scale=scale).cpu(), q.float() * scale)


def test_int16_transport_grid_stride_loop():
    """4096 blocks x 256 lanes x 8 samples = 8 388 608 samples per grid pass: 300 more vector trips and a 5-sample tail (17 MB
    in, 34 MB out - the one large tensor of this file; the loop's trip count exceeds 1 nowhere below this size)."""
    n = 8388608 + 8 * 300 + 5
    q = _pcm(n, 1)
    qd = q.to(DEV)
    out = torch.full((n,), float("nan"), device=DEV)
    assert ops.wave_i16_to_f32(qd, out=out) is out
    assert torch.equal(out.cpu(), q.float() * (1.0 / 32768.0))


def test_int16_transport_out_argument_and_alignment():
    q = _pcm(24, 3).to(DEV)
    out = torch.empty((2, 3, 4), device=DEV)                      # another shape, the same number of samples
    assert ops.wave_i16_to_f32(q, out=out) is out
    assert torch.equal(out.reshape(-1).cpu(), q.cpu().float() * (1.0 / 32768.0))
    with pytest.raises(EatHipError, match="out"):
        ops.wave_i16_to_f32(q, out=torch.empty(23, device=DEV))
    src = q[1:]                                                   # contiguous, but 2-byte aligned: refused by the entry point
    assert src.is_contiguous() and src.data_ptr() % 16 == 2
    with pytest.raises(EatHipError, match="16-byte aligned"):
        ops.wave_i16_to_f32(src)


# ------------------------------------------------------------------ column sums
def _col_sum_into_nan(m):
    """eat_col_sum into a NaN-filled buffer of C + 64 elements -> (the C sums, the 64 elements behind them)."""
    R, C = m.shape
    buf = torch.full((C + 64,), float("nan"), device=DEV)
    _lib.call("eat_col_sum", m.data_ptr(), buf.data_ptr(), R, C, torch.cuda.current_stream().cuda_stream)
    buf = buf.cpu().numpy()
    return buf[:C], buf[C:]


@pytest.mark.parametrize("R", G.COL_R)
def test_col_sum_against_fp64(R):
    worst = 0.0
    for C in G.COL_C:
        mi = G.col_case(R, C, "int")                              # every partial sum is exact: no tolerance to hide in
        got = ops.col_sum(_d(mi)).cpu().numpy()
        assert np.array_equal(got.astype(np.float64), G.col_sum(mi)), (R, C)
        mg = G.col_case(R, C, "gauss")
        md = _d(mg)
        got = ops.col_sum(md).cpu().numpy()
        err, bound = np.abs(got - G.col_sum(mg)), G.col_sum_bound(mg)
        assert np.all(err <= bound), (R, C)
        worst = max(worst, float((err / bound).max()))
        if R <= 512:                                              # the fixed-order kernel: bit-reproducible
            assert np.array_equal(got, ops.col_sum(md).cpu().numpy()), (R, C)
        direct, behind = _col_sum_into_nan(_d(mi))                # every column written, nothing behind them
        assert np.array_equal(direct.astype(np.float64), G.col_sum(mi)) and np.all(np.isnan(behind)), (R, C)
    _report(f"col_sum R={R}", dict(gauss=worst))


def test_col_sum_refuses_more_than_8192_columns():
    with pytest.raises(EatHipError, match="eat_col_sum"):
        ops.col_sum(torch.zeros(2, 8193, device=DEV))
    assert ops.col_sum(torch.ones(2, 8192, device=DEV)).cpu().eq(2.0).all()


# ------------------------------------------------------------------ dynamic heads
@pytest.mark.parametrize("K", G.HEAD_K)
@pytest.mark.parametrize("n_att", G.HEAD_N_ATT)
def test_dyn_heads_forward_and_backward_against_fp64(n_att, K):
    worst = dict(att=0.0, sg=0.0, coef=0.0, dy_att=0.0, dy_coef=0.0)
    lam4, iv4 = _d(G.HEAD_LAM4), _d(G.HEAD_IV4)
    for cexp in G.HEAD_CEXP:
        for B in G.HEAD_B:
            for scale in (1.0, 40.0):
                c = G.heads_case(B, n_att, K, cexp, scale)
                cfg = (n_att, K, cexp, G.HEAD_INV_T, G.HEAD_LAM4, G.HEAD_IV4)
                att_d, sg_d, coef_d = ops.dyn_heads_fwd(_d(c["y"]), n_att, K, cexp, G.HEAD_INV_T, lam4, iv4)
                assert att_d.shape == (n_att, B, K) and sg_d.shape == (B, 4 * cexp) and coef_d.shape == (B, cexp, 4)
                got = [t.cpu().numpy() for t in (att_d, sg_d, coef_d)]
                ref, bound = G.dyn_heads_fwd(c["y"], *cfg), G.heads_fwd_bounds(c["y"], *cfg)
                for name, g, r, b in zip(("att", "sg", "coef"), got, ref, bound):
                    e = np.abs(g - r) / b
                    assert np.all(e <= 1.0), (name, cexp, B, scale, float(e.max()))
                    worst[name] = max(worst[name], float(e.max()))
                # backward: the oracle gets the kernel's own fp32 att / sg
                dy = ops.dyn_heads_bwd(_d(c["datt"]), _d(c["dcoef"]), att_d, sg_d, lam4, cexp, G.HEAD_INV_T).cpu().numpy()
                assert dy.shape == (B, n_att * K + 4 * cexp)
                ref = G.dyn_heads_bwd(c["datt"], c["dcoef"], got[0], got[1], G.HEAD_LAM4, G.HEAD_INV_T)
                b = G.heads_bwd_bound(c["datt"], c["dcoef"], G.HEAD_LAM4, G.HEAD_INV_T)
                e = np.abs(dy - ref) / np.maximum(b, 1e-300)
                assert np.all(np.abs(dy - ref) <= b), (cexp, B, scale, float(e.max()))
                worst["dy_att"] = max(worst["dy_att"], float(e[:, :n_att * K].max()))
                worst["dy_coef"] = max(worst["dy_coef"], float(e[:, n_att * K:].max()))
    _report(f"dyn heads n_att={n_att} K={K}", worst)


@pytest.mark.parametrize("n_att,K", [(4, 4), (3, 33)])
def test_dyn_heads_refuse_what_one_lane_per_head_cannot_take(n_att, K):
    B, cexp = 2, 8
    lam4, iv4 = _d(G.HEAD_LAM4), _d(G.HEAD_IV4)
    inv_t = G.HEAD_INV_T + (1.0,)
    with pytest.raises(EatHipError, match="eat_dyn_heads_fwd"):
        ops.dyn_heads_fwd(torch.zeros(B, n_att * K + 4 * cexp, device=DEV), n_att, K, cexp, inv_t, lam4, iv4)
    with pytest.raises(EatHipError, match="eat_dyn_heads_bwd"):
        ops.dyn_heads_bwd(torch.zeros(n_att, B, K, device=DEV), torch.zeros(B, cexp, 4, device=DEV),
                          torch.zeros(n_att, B, K, device=DEV), torch.zeros(B, 4 * cexp, device=DEV), lam4, cexp, inv_t)
