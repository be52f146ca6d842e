"""eat_softmax_ce_fwd_bwd and eat_wave_augment (csrc/finetune.hip) against the float64 references of tests/finetune_ref.py."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, ops  # noqa: E402
from tests.finetune_ref import softmax_ce_ref, wave_augment_ref  # noqa: E402

DEV = torch.device("cuda:0")
KINDS = ("onehot", "soft", "zero", "nonnorm")


def _case(B, C, seed):
    """Logits with every row kind of the contract: rows cycle through one-hot / soft / zero / non-normalised targets; row 0
    reaches |z| = 100, row 1 is all-equal (argmax 0), row 2 holds NaNs (argmax = the first NaN)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C, generator=g) * 3
    if B > 0:
        z[0] = torch.rand(C, generator=g) * 200 - 100
    if B > 1:
        z[1] = 0.25
    if B > 2 and C > 1:
        z[2, C // 2] = float("nan")
        z[2, -1] = float("nan")
    y = torch.zeros(B, C)
    for b in range(B):
        kind = KINDS[b % 4]
        if kind == "onehot":
            y[b, int(torch.randint(C, (1,), generator=g))] = 1
        elif kind == "soft":
            r = torch.rand(C, generator=g)
            y[b] = r / r.sum()
        elif kind == "nonnorm":
            y[b] = torch.rand(C, generator=g) * 2.5
    return z, y


def _run(z, y, perm=None, lam=None):
    B, C = z.shape
    zd, yd = z.to(DEV), y.to(DEV)
    sums = torch.zeros(1, device=DEV)
    rl = torch.full((B,), -7.0, device=DEV)
    am = torch.full((B,), -7, device=DEV, dtype=torch.int32)
    pd = None if perm is None else perm.to(DEV, torch.int32)
    ld = None if lam is None else lam.to(DEV)
    d = ops.softmax_ce_fwd_bwd(zd, yd, pd, ld, sums=sums, row_loss=rl, row_argmax=am)
    torch.cuda.synchronize()
    return dict(sums=sums.cpu(), dlogits=d.cpu(), row_loss=rl.cpu(), argmax=am.cpu())


def _check(got, ref, z, B):
    zmax = np.nan_to_num(np.abs(z.numpy()), nan=0.0).max(axis=1)
    s1 = np.maximum(1.0, np.abs(ref["S"]))
    nan_rows = np.isnan(ref["row_loss"])
    rl = got["row_loss"].double().numpy()
    assert np.array_equal(np.isnan(rl), nan_rows)
    ok = ~nan_rows
    err_l = np.abs(rl[ok] - ref["row_loss"][ok]) / ((1 + zmax[ok]) * s1[ok])
    assert (err_l <= 1e-6).all(), float(err_l.max())
    d = got["dlogits"].double().numpy()
    assert np.array_equal(np.isnan(d), np.isnan(ref["dlogits"]))
    err_d = np.abs(B * (d[ok] - ref["dlogits"][ok])) / s1[ok, None]
    assert (err_d <= 2e-7).all(), float(err_d.max())         # (measured <= 6e-8: fp32 rounding of fp64 values)
    np.testing.assert_array_equal(got["argmax"].numpy(), ref["argmax"])
    if nan_rows.any():
        assert np.isnan(float(got["sums"][0]))
    else:
        assert abs(float(got["sums"][0]) - ref["loss"]) <= 1e-6 * (1 + zmax.max()) * s1.max()
    return float(err_l.max(initial=0)), float(err_d.max(initial=0))


@pytest.mark.parametrize("B", [1, 3, 128, 1000])
@pytest.mark.parametrize("C", [1, 2, 10, 50, 63, 64, 65, 527, 4097])
def test_softmax_ce_against_fp64(B, C):
    z, y = _case(B, C, seed=B * 10007 + C)
    g = torch.Generator().manual_seed(C)
    worst = [0.0, 0.0]
    cases = [(None, None), (torch.arange(B), torch.rand(B, generator=g)), (torch.randperm(B, generator=g), torch.rand(B, generator=g)),
             (torch.randperm(B, generator=g), torch.ones(B))]
    for perm, lam in cases:
        got = _run(z, y, perm, lam)
        ref = softmax_ce_ref(z.numpy(), y.numpy(), None if perm is None else perm.numpy(), None if lam is None else lam.numpy())
        el, ed = _check(got, ref, z, B)
        worst = [max(worst[0], el), max(worst[1], ed)]
    print(f"B={B} C={C}: max scaled |d row_loss| {worst[0]:.2e}, |d B dlogits| {worst[1]:.2e}")


def test_softmax_ce_null_outputs_and_repeatability():
    """Each NULL-output combination computes what the full call does (bit-equal), and repeated calls are bit-identical -
    `sums` included, with and without row_loss (the second launch then recomputes the rows)."""
    for B, C in [(128, 50), (37, 527)]:
        z, y = _case(B, C, seed=5)
        z[2] = 0.5                                                     # (no NaN row: the sums must be finite)
        zd, yd = z.to(DEV), y.to(DEV)
        perm = torch.randperm(B).to(DEV, torch.int32)
        lam = torch.rand(B).to(DEV)
        full = _run(z, y, perm.cpu(), lam.cpu())
        for mask in range(16):
            want_s, want_d, want_l, want_a = (mask >> 0) & 1, (mask >> 1) & 1, (mask >> 2) & 1, (mask >> 3) & 1
            for rep in range(2):
                sums = torch.zeros(1, device=DEV) if want_s else None
                rl = torch.empty(B, device=DEV) if want_l else None
                am = torch.empty(B, device=DEV, dtype=torch.int32) if want_a else None
                d = ops.softmax_ce_fwd_bwd(zd, yd, perm, lam, sums=sums, grad=bool(want_d), row_loss=rl, row_argmax=am)
                torch.cuda.synchronize()
                assert (d is None) == (not want_d)
                if want_s:
                    assert torch.equal(sums.cpu(), full["sums"]), (mask, float(sums), float(full["sums"]))
                if want_d:
                    assert torch.equal(d.cpu(), full["dlogits"])
                if want_l:
                    assert torch.equal(rl.cpu(), full["row_loss"])
                if want_a:
                    assert torch.equal(am.cpu(), full["argmax"])
        # accumulation: sums += loss, call after call
        acc = torch.full((1,), 1.5, device=DEV)
        for _ in range(3):
            ops.softmax_ce_fwd_bwd(zd, yd, perm, lam, sums=acc, grad=False)
        torch.cuda.synchronize()
        want = np.float32(1.5)
        for _ in range(3):
            want = np.float32(want + full["sums"].numpy()[0])
        assert float(acc) == float(want)


def test_softmax_ce_rejects_bad_arguments():
    h = _lib.lib()
    z = torch.zeros(4, 4, device=DEV)
    p = z.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    for B, C, perm, lam in [(0, 4, None, None), (4, 0, None, None), (-1, 4, None, None), (4, 4, p, None), (4, 4, None, p),
                            (65536, 32768, None, None)]:
        assert h.eat_softmax_ce_fwd_bwd(p, p, perm, lam, B, C, p, p, None, None, st) == -1, (B, C)
    torch.cuda.synchronize()
    with pytest.raises(_lib.EatHipError):
        ops.softmax_ce_fwd_bwd(z, torch.zeros(4, 5, device=DEV))
    with pytest.raises(_lib.EatHipError):
        ops.softmax_ce_fwd_bwd(z, z, perm=torch.zeros(4, device=DEV, dtype=torch.int32))


def _augment_draws(L, n_bank, g):
    shifts = [-4000, -1, 0, 1, 4000, L - 1, -(L - 1)]
    gains = [12, -12, 0, 7, -3]
    idx, shift, amp, mix = [], [], [], []
    for b in range(12):
        i0 = int(torch.randint(n_bank, (1,), generator=g))
        mode = b % 3                                                   # 0: no wave-mix, 1: random partner, 2: itself
        i1 = -1 if mode == 0 else (i0 if mode == 2 else int(torch.randint(n_bank, (1,), generator=g)))
        idx += [i0, i1]
        shift += [shifts[b % len(shifts)], shifts[(b + 3) % len(shifts)]]
        amp += [10 ** (gains[b % len(gains)] / 20), 10 ** (gains[(b + 2) % len(gains)] / 20)]
        lm = float(torch.rand(1, generator=g))
        mix.append(max(lm, 1 - lm) if mode else 1.0)
    return (torch.tensor(idx, dtype=torch.int32), torch.tensor(shift, dtype=torch.int32), torch.tensor(amp, dtype=torch.float32),
            torch.tensor(mix, dtype=torch.float32))


@pytest.mark.parametrize("L", [160000, 16001])
@pytest.mark.parametrize("aligned", [True, False])
def test_wave_augment_against_reference(L, aligned):
    g = torch.Generator().manual_seed(L)
    n_bank, C = 9, 50
    bank = (torch.randn(n_bank, L, generator=g) * 0.2 + torch.linspace(-0.1, 0.3, n_bank).unsqueeze(1)).float()
    cls = torch.tensor([3, 49, 0, 3, 17, 8, 8, 22, 1], dtype=torch.int32)
    mean = bank.double().mean(1)
    idx, shift, amp, mix = _augment_draws(L, n_bank, g)
    B = mix.numel()
    bd = bank.to(DEV)
    buf = torch.full((B * L + 1,), float("nan"), device=DEV)
    out = buf[0 if aligned else 1:][:B * L].view(B, L)                 # (unaligned: every row start off by 4 bytes)
    y = torch.full((B, C), -3.0, device=DEV)
    ops.wave_augment(bd, mean.to(DEV), cls.to(DEV), idx, shift, amp, mix, C, out=out, y=y)
    torch.cuda.synchronize()
    want, want_y = wave_augment_ref(bank.numpy(), cls.numpy(), idx.numpy(), shift.numpy(), amp.numpy(), mix.numpy(), C)
    got = out.cpu().double().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"L={L} aligned={aligned}: max |out - ref| / max |ref| = {err:.2e}")
    assert err <= 1e-6
    np.testing.assert_allclose(y.cpu().double().numpy(), want_y, rtol=0, atol=1e-7)
    if not aligned:
        assert torch.isnan(buf[0]).item()                               # nothing written before the view
    # the same draws through device tables (the captured step's path) give the same bits
    out2, y2 = ops.wave_augment(bd, mean.to(DEV), cls.to(DEV), idx.to(DEV), shift.to(DEV), amp.to(DEV), mix.to(DEV), C)
    torch.cuda.synchronize()
    assert torch.equal(out2.cpu(), out.cpu()) and torch.equal(y2.cpu(), y.cpu())


def test_wave_augment_rejects_bad_draws():
    bank = torch.zeros(3, 100, device=DEV)
    mean = torch.zeros(3, device=DEV, dtype=torch.float64)
    cls = torch.zeros(3, device=DEV, dtype=torch.int32)
    one = torch.ones(2)
    with pytest.raises(ValueError):
        ops.wave_augment(bank, mean, cls, torch.tensor([3, -1], dtype=torch.int32), torch.zeros(2, dtype=torch.int32), one,
                         torch.ones(1), 5)
    with pytest.raises(ValueError):
        ops.wave_augment(bank, mean, cls, torch.tensor([0, -1], dtype=torch.int32), torch.tensor([100, 0], dtype=torch.int32),
                         one, torch.ones(1), 5)
    h = _lib.lib()
    p = bank.data_ptr()
    st = torch.cuda.current_stream().cuda_stream
    assert h.eat_wave_augment(p, p, p, 3, 100, 5, p, p, p, p, p, p, 0, st) == -1
    assert h.eat_wave_augment(p, p, p, 0, 100, 5, p, p, p, p, p, p, 1, st) == -1
    assert h.eat_wave_augment(p, p, p, 3, 0, 5, p, p, p, p, p, p, 1, st) == -1
    assert ctypes.c_int(h.eat_wave_augment(None, p, p, 3, 100, 5, p, p, p, p, p, p, 1, st)).value == -1
    torch.cuda.synchronize()
