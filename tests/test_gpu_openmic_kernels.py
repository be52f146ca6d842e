"""eat_masked_bce_fwd_bwd, eat_openmic_targets (csrc/finetune.hip) and eat_rank_metrics_masked (csrc/metrics.hip) against the
float64 references of tests/openmic_ref.py."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, metrics, ops  # noqa: E402
from tests.openmic_ref import masked_ap_auc, masked_bce_ref, openmic_targets_ref  # noqa: E402
from tests.test_gpu_metrics import _data  # noqa: E402

DEV = torch.device("cuda:0")


def _case(B, C, seed, nan_row=True):
    """Logits and packed rows with every row kind of the contract: row 0 reaches |z| = 100, row 2 holds NaNs (also under mask
    0); masks cycle through all-ones / all-zero / random 0-1 rows; labels are soft, on both sides of 0.5 and exactly 0.5."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C, generator=g) * 3
    z[0] = torch.rand(C, generator=g) * 200 - 100
    lab = torch.rand(B, C, generator=g)
    lab[torch.rand(B, C, generator=g) < 0.3] = 0.5
    lab[torch.rand(B, C, generator=g) < 0.3] = 1.0
    mask = (torch.rand(B, C, generator=g) < 0.5).float()
    mask[0::3] = 1.0
    mask[1::3] = 0.0
    if nan_row and B > 2:
        z[2, C // 2] = float("nan")
        z[2, -1] = float("nan")
        mask[2, -1] = 0.0
    return z, torch.cat([lab, mask], 1)


def _run(z, yy, perm=None, lam=None, binarize=True):
    B, C = z.shape
    sums = torch.zeros(1, device=DEV)
    rl = torch.full((B,), -7.0, device=DEV)
    pr = torch.full((B, C), -7.0, device=DEV)
    pd = None if perm is None else perm.to(DEV, torch.int32)
    ld = None if lam is None else lam.to(DEV)
    d = ops.masked_bce_fwd_bwd(z.to(DEV), yy.to(DEV), pd, ld, sums=sums, row_loss=rl, probs=pr, binarize=binarize)
    torch.cuda.synchronize()
    return dict(sums=sums.cpu(), dlogits=d.cpu(), row_loss=rl.cpu(), probs=pr.cpu())


def _check(got, ref, z):
    """The bounds of the CE kernel's test for the same arithmetic (fp32 rounding of fp64 values): 1e-6 (1 + max |z|) on the row
    and total loss, 2e-7 on B C dlogits; sigmoid: 2^-24 (one fp32 rounding of a value <= 1).  -> the measured worst cases."""
    B, C = z.shape
    zmax = np.nan_to_num(np.abs(z.numpy()), nan=0.0).max(axis=1)
    nan_rows = np.isnan(ref["row_loss"])
    rl = got["row_loss"].double().numpy()
    assert np.array_equal(np.isnan(rl), nan_rows)
    ok = ~nan_rows
    err_l = np.abs(rl[ok] - ref["row_loss"][ok]) / (1 + zmax[ok])
    d = got["dlogits"].double().numpy()
    assert np.array_equal(np.isnan(d), np.isnan(ref["dlogits"]))
    fin = ~np.isnan(d)
    err_d = np.abs(B * C * (d[fin] - ref["dlogits"][fin]))
    p = got["probs"].double().numpy()
    assert np.array_equal(np.isnan(p), np.isnan(ref["probs"]))
    err_p = np.abs(p[fin] - ref["probs"][fin])
    worst = [float(e.max(initial=0)) for e in (err_l, err_d, err_p)]
    if nan_rows.any():
        assert np.isnan(float(got["sums"][0]))
        worst.append(0.0)
    else:
        worst.append(abs(float(got["sums"][0]) - ref["loss"]) / (1 + zmax.max()))
    return worst


@pytest.mark.parametrize("B", [1, 3, 64, 130])
@pytest.mark.parametrize("C", [1, 20, 63, 64, 65, 527])
def test_masked_bce_against_fp64(B, C):
    g = torch.Generator().manual_seed(C)
    cases = [(None, None), (torch.arange(B), torch.rand(B, generator=g)), (torch.randperm(B, generator=g), torch.rand(B, generator=g)),
             (torch.randperm(B, generator=g), torch.ones(B))]
    worst = [0.0] * 4
    for nan_row in (True, False):                                # (without the NaN row the total loss is a number)
        z, yy = _case(B, C, seed=B * 10007 + C, nan_row=nan_row)
        for perm, lam in cases:
            ref = masked_bce_ref(z.numpy(), yy.numpy(), None if perm is None else perm.numpy(),
                                 None if lam is None else lam.numpy())
            worst = [max(a, b) for a, b in zip(worst, _check(_run(z, yy, perm, lam), ref, z))]
    print(f"B={B} C={C}: max |d row_loss| / (1 + max|z|) {worst[0]:.2e}, |d B C dlogits| {worst[1]:.2e}, |d sigmoid| {worst[2]:.2e}, "
          f"|d loss| / (1 + max|z|) {worst[3]:.2e}")
    assert worst[0] <= 1e-6 and worst[1] <= 2e-7 and worst[2] <= 2.0 ** -24 and worst[3] <= 1e-6, worst
    # soft labels (binarize = 0) through the same bounds
    z, yy = _case(B, C, seed=C, nan_row=False)
    w = _check(_run(z, yy, *cases[2], binarize=False), masked_bce_ref(z.numpy(), yy.numpy(), cases[2][0].numpy(),
                                                                        cases[2][1].numpy(), binarize=False), z)
    assert w[0] <= 1e-6 and w[1] <= 2e-7 and w[3] <= 1e-6, w


def test_masked_bce_null_outputs_and_repeatability():
    """Each NULL-output combination computes what the full call does (bit-equal), and repeated calls are bit-identical -
    `sums` included, with and without row_loss (the second launch then recomputes the rows)."""
    for B, C in [(64, 20), (300, 65)]:
        z, yy = _case(B, C, seed=5, nan_row=False)
        zd, yd = z.to(DEV), yy.to(DEV)
        perm = torch.randperm(B).to(DEV, torch.int32)
        lam = torch.rand(B).to(DEV)
        full = _run(z, yy, perm.cpu(), lam.cpu())
        assert np.isfinite(float(full["sums"]))
        for mask in range(16):
            want_s, want_d, want_l, want_p = (mask >> 0) & 1, (mask >> 1) & 1, (mask >> 2) & 1, (mask >> 3) & 1
            for rep in range(2):
                sums = torch.zeros(1, device=DEV) if want_s else None
                rl = torch.empty(B, device=DEV) if want_l else None
                pr = torch.empty(B, C, device=DEV) if want_p else None
                d = ops.masked_bce_fwd_bwd(zd, yd, perm, lam, sums=sums, grad=bool(want_d), row_loss=rl, probs=pr)
                torch.cuda.synchronize()
                assert (d is None) == (not want_d)
                if want_s:
                    assert torch.equal(sums.cpu(), full["sums"]), (mask, float(sums), float(full["sums"]))
                if want_d:
                    assert torch.equal(d.cpu(), full["dlogits"])
                if want_l:
                    assert torch.equal(rl.cpu(), full["row_loss"])
                if want_p:
                    assert torch.equal(pr.cpu(), full["probs"])
        acc = torch.full((1,), 1.5, device=DEV)                       # accumulation: sums += loss, call after call
        for _ in range(3):
            ops.masked_bce_fwd_bwd(zd, yd, perm, lam, sums=acc, grad=False)
        torch.cuda.synchronize()
        want = np.float32(1.5)
        for _ in range(3):
            want = np.float32(want + full["sums"].numpy()[0])
        assert float(acc) == float(want)


def test_masked_bce_strided_probs_land_in_a_slice():
    """probs through a row stride: a row range of the (N, C) evaluation matrix, and a column range of a wider matrix; nothing
    else is written."""
    B, C = 37, 20
    z, yy = _case(B, C, seed=9, nan_row=False)
    want = _run(z, yy)["probs"]
    big = torch.full((100, C), float("nan"), device=DEV)
    ops.masked_bce_fwd_bwd(z.to(DEV), yy.to(DEV), grad=False, probs=big[50:50 + B])
    wide = torch.full((B, C + 7), float("nan"), device=DEV)
    ops.masked_bce_fwd_bwd(z.to(DEV), yy.to(DEV), grad=False, probs=wide[:, 3:3 + C])
    torch.cuda.synchronize()
    assert torch.equal(big[50:50 + B].cpu(), want) and torch.isnan(big[:50]).all() and torch.isnan(big[50 + B:]).all()
    assert torch.equal(wide[:, 3:3 + C].cpu(), want) and torch.isnan(wide[:, :3]).all() and torch.isnan(wide[:, 3 + C:]).all()
    with pytest.raises(_lib.EatHipError):
        ops.masked_bce_fwd_bwd(z.to(DEV), yy.to(DEV), grad=False, probs=torch.empty(B, 2 * C, device=DEV)[:, ::2])


def test_masked_bce_bad_perm_poisons_its_row_only():
    B, C = 6, 20
    z, yy = _case(B, C, seed=1, nan_row=False)
    perm = torch.tensor([1, B, 0, -1, 5, 2 ** 31 - 1])
    lam = torch.full((B,), 0.7)
    got = _run(z, yy, perm, lam)
    ref = masked_bce_ref(z.numpy(), yy.numpy(), perm.numpy(), lam.numpy())
    assert list(np.isnan(got["row_loss"].numpy())) == [False, True, False, True, False, True]
    assert np.isnan(got["dlogits"].numpy()[[1, 3, 5]]).all() and np.isnan(float(got["sums"]))
    w = _check(got, ref, z)
    assert w[0] <= 1e-6 and w[1] <= 2e-7, w


def test_masked_bce_rejects_bad_arguments():
    h = _lib.lib()
    z = torch.zeros(4, 8, device=DEV)
    p = z.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    for B, C, perm, lam in [(0, 4, None, None), (4, 0, None, None), (-1, 4, None, None), (4, 4, p, None), (4, 4, None, p),
                            (65536, 16384, None, None)]:
        assert h.eat_masked_bce_fwd_bwd(p, p, perm, lam, B, C, 1, p, p, None, None, 0, st) == -1, (B, C)
    assert h.eat_masked_bce_fwd_bwd(p, p, None, None, 4, 4, 1, None, None, None, p, 3, st) == -1       # probs_stride < C
    assert ctypes.c_int(h.eat_masked_bce_fwd_bwd(None, p, None, None, 4, 4, 1, p, None, None, None, 0, st)).value == -1
    assert b"eat_masked_bce_fwd_bwd" in h.eat_last_error_string()
    torch.cuda.synchronize()
    with pytest.raises(_lib.EatHipError):
        ops.masked_bce_fwd_bwd(z, torch.zeros(4, 8, device=DEV))                                      # yy must be (B, 2C)
    with pytest.raises(_lib.EatHipError):
        ops.masked_bce_fwd_bwd(z, torch.zeros(4, 16, device=DEV), perm=torch.zeros(4, device=DEV, dtype=torch.int32))


# one table per mask combination for C = 1: bank masks are 1, 0, 1, 0, 1, 0, 1 there
TABLES = [([5, -1, 0, 2, 0, 1, 1, 3, 4, 4], "unmixed, (1, 1), (1, 0), (0, 0), itself"),
          ([1, 0, 6, -1, 2, 2, 3, 5, 5, 3], "(0, 1), unmixed, itself, (0, 0), (0, 0)")]


@pytest.mark.parametrize("C", [1, 20])
@pytest.mark.parametrize("table", [0, 1])
def test_openmic_targets_equal_the_reference(C, table):
    rng = np.random.default_rng(10 * C + table)
    n, B = 7, 5
    lab = rng.random((n, C)).astype(np.float32)
    mask = (rng.random((n, C)) < 0.5).astype(np.float32)
    mask[:, 0] = np.arange(n) % 2 == 0
    bank_y = np.concatenate([lab, mask], 1)
    idx = torch.tensor(TABLES[table][0], dtype=torch.int32)
    b = rng.beta(2, 2, B)
    mix = torch.tensor(np.maximum(b, 1 - b), dtype=torch.float32)
    mix[idx[1::2] < 0] = 1.0
    out = torch.full((B, 2 * C), -3.0, device=DEV)
    ops.openmic_targets(torch.from_numpy(bank_y).to(DEV), idx.to(DEV), mix.to(DEV), out=out)
    torch.cuda.synchronize()
    want = openmic_targets_ref(bank_y, idx.numpy(), mix.numpy()).astype(np.float32)
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    unmixed = int(np.flatnonzero(idx.numpy()[1::2] < 0)[0])
    np.testing.assert_array_equal(out.cpu().numpy()[unmixed], bank_y[int(idx[2 * unmixed])])     # a copy, labels not masked


def test_openmic_targets_invalid_indices_give_nan_rows():
    n, C = 7, 20
    bank_y = torch.rand(n, 2 * C, device=DEV)
    idx = torch.tensor([7, -1, 0, 7, -1, -1, 0, -2, 3, 4, 2, -1], dtype=torch.int32, device=DEV)
    mix = torch.full((6,), 0.75, device=DEV)
    guard = torch.full((6 * 2 * C + 8,), 5.0, device=DEV)
    out = guard[4:4 + 6 * 2 * C].view(6, 2 * C)
    ops.openmic_targets(bank_y, idx, mix, out=out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isnan(got[:4]).all() and np.isfinite(got[4:]).all()
    np.testing.assert_array_equal(got, openmic_targets_ref(bank_y.cpu().numpy(), idx.cpu().numpy(), mix.cpu().numpy()).astype(np.float32))
    assert (guard[:4] == 5.0).all() and (guard[-4:] == 5.0).all()
    h = _lib.lib()
    p, st = bank_y.data_ptr(), torch.cuda.current_stream().cuda_stream
    for nb, c, B in [(0, 20, 6), (7, 0, 6), (7, 20, 0)]:
        assert h.eat_openmic_targets(p, nb, c, p, p, p, B, st) == -1
    assert ctypes.c_int(h.eat_openmic_targets(None, 7, 20, p, p, p, 6, st)).value == -1
    torch.cuda.synchronize()
    with pytest.raises(_lib.EatHipError):
        ops.openmic_targets(torch.rand(n, 2 * C + 1, device=DEV), idx, mix)


ATOL = 1e-9                                                           # the bound of tests/test_gpu_metrics.py


def _check_metrics(s, y, w, scores_dev=None):
    ap, auc = metrics.ap_auc(scores_dev if scores_dev is not None else s.to(DEV), y.to(DEV), sample_weight=w.to(DEV))
    ap_r, auc_r = masked_ap_auc(s.float().numpy(), y.numpy(), w.numpy())
    ap, auc = ap.cpu().numpy(), auc.cpu().numpy()
    err = max(np.abs(ap - ap_r).max(), np.nan_to_num(np.abs(auc - auc_r)).max())
    np.testing.assert_allclose(ap, ap_r, rtol=0, atol=ATOL)
    np.testing.assert_allclose(auc, auc_r, rtol=0, atol=ATOL, equal_nan=True)
    assert np.array_equal(np.isnan(auc), np.isnan(auc_r))
    return float(err)


@pytest.mark.parametrize("n", [1, 2, 64, 65, 1025, 20481])
@pytest.mark.parametrize("c", [1, 20])
def test_masked_ap_auc_matches_fp64_oracle(n, c):
    s, y = _data(n, c, seed=n * 1000 + c, p=0.3 if n < 100 else 0.05)
    g = torch.Generator().manual_seed(n + c)
    w = (torch.rand(n, c, generator=g) < 0.6).float()
    err = _check_metrics(s, y, w)
    w[s.argmax(0), torch.arange(c)] = 0.0                             # the top-ranked item of every column masked out
    err = max(err, _check_metrics(s, y, w))
    print(f"N={n} C={c}: max |metric - oracle| {err:.2e}")
    # all-ones weights: the unweighted call, bit for bit
    ap_w, auc_w = metrics.ap_auc(s.to(DEV), y.to(DEV), sample_weight=torch.ones(n, c, device=DEV))
    ap_u, auc_u = metrics.ap_auc(s.to(DEV), y.to(DEV))
    assert torch.equal(ap_w, ap_u) and torch.equal(torch.nan_to_num(auc_w, nan=-1.0), torch.nan_to_num(auc_u, nan=-1.0))


def test_masked_ap_auc_degenerate_columns_and_invalid_weights():
    n = 3000
    s, y = _data(n, 6, seed=4, p=0.2)
    g = torch.Generator().manual_seed(8)
    w = (torch.rand(n, 6, generator=g) < 0.5).float()
    w[:, 0] = 0.0                                                     # no weighted item at all: AP 0, AUC NaN
    w[:, 1] = y[:, 1]                                                 # only positives among the weighted items: AP 1, AUC NaN
    w[:, 2] = 1.0 - y[:, 2]                                           # only negatives: AP 0, AUC NaN
    order = s[:, 3].argsort(descending=True)
    w[order[:700], 3] = 0.0                                           # a long masked run at the top: count stays 0 over tiles
    _check_metrics(s, y, w)
    ap, auc = metrics.ap_auc(s.to(DEV), y.to(DEV), sample_weight=w.to(DEV))
    assert ap[:3].tolist() == [0.0, 1.0, 0.0] and torch.isnan(auc[:3]).all() and torch.isfinite(auc[3:]).all()
    assert torch.equal(metrics.average_precision(s.to(DEV), y.to(DEV), sample_weight=w.to(DEV)), ap)
    assert torch.isnan(metrics.roc_auc(s.to(DEV), y.to(DEV), average="macro", sample_weight=w.to(DEV)))
    a2, u2 = metrics.ap_auc(s.to(DEV), y.to(DEV), sample_weight=w.to(DEV))                     # bit-identical repeats
    assert torch.equal(ap, a2) and torch.equal(torch.nan_to_num(auc), torch.nan_to_num(u2))
    for bad in (0.5, 2.0, float("nan")):
        wb = w.clone()
        wb[17, 4] = bad
        with pytest.raises(ValueError, match="sample_weight"):
            metrics.ap_auc(s.to(DEV), y.to(DEV), sample_weight=wb.to(DEV))
    with pytest.raises(ValueError):
        metrics.ap_auc(s.to(DEV), y.to(DEV), sample_weight=w[:, :5].to(DEV))
    _check_metrics(s, y, w)                                           # the next call is clean again


@pytest.mark.parametrize("n,c", [(65, 20), (1025, 20)])
def test_masked_ap_auc_bf16_scores(n, c):
    s, y = _data(n, c, seed=7 + n)
    w = (torch.rand(n, c, generator=torch.Generator().manual_seed(n)) < 0.6).float()
    sb = s.to(torch.bfloat16)
    _check_metrics(sb.float(), y, w, scores_dev=sb.to(DEV))          # the oracle gets the bf16 values widened to fp32
