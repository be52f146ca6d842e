"""eat_wave_augment_ragged (csrc/ragged.hip) against the float64 reference of tests/fsd50k_ref.py."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, ops  # noqa: E402
from tests.fsd50k_ref import ragged_augment_ref  # noqa: E402

DEV = torch.device("cuda:0")
C = 13


def _clips(L, seed):
    """Clips of length 1, L - 1, L, L + 1, 2L + 3 and 3L, each with its own offset level, laid out back to back with a NaN
    sample in front wherever that makes the clip's start odd: a read outside a clip's window shows as NaN."""
    rng = np.random.default_rng(seed)
    lens = [1, L - 1, L, L + 1, 2 * L + 3, 3 * L]
    parts, offsets, pos = [], [], 0
    for k, n in enumerate(lens):
        if pos % 2 == 0:
            parts.append(np.full(1, np.nan, dtype=np.float32))
            pos += 1
        offsets.append(pos)
        parts.append((rng.standard_normal(n) * 0.2 + (-0.1 + 0.08 * k)).astype(np.float32))
        pos += n
    parts.append(np.full(3, np.nan, dtype=np.float32))
    bank_y = (rng.random((len(lens), C)) < 0.4).astype(np.float32)
    return np.concatenate(parts), np.array(offsets, dtype=np.int64), np.array(lens, dtype=np.int64), bank_y


def _rows(L, rng):
    """(idx, start, shift, amp, mix) covering every row kind: unmixed short (L - 1, and 1 sample), exactly L, long at start 0
    / in the middle / at len - L, L + 1 at start 1; mixed short + long, long + long, a clip with itself at two starts, long +
    one sample, L with L + 1.  Shifts from {0, +-1, +-4000, +-(L - 1)}, gains within +-12 dB."""
    S, ONE, EQ, P1, L2, L3 = 1, 0, 2, 3, 4, 5
    rows = [(S, 0, -1, 0), (ONE, 0, -1, 0), (EQ, 0, -1, 0), (L3, 0, -1, 0), (L3, L + 7, -1, 0), (L2, L + 3, -1, 0), (P1, 1, -1, 0),
            (S, 0, L3, 5), (L2, 3, L3, 2 * L), (L3, 11, L3, L + 5), (L3, 2 * L - 1, ONE, 0), (EQ, 0, P1, 0)]
    shifts = [0, 1, -1, 4000, -4000, L - 1, -(L - 1)]
    gains = [12, -12, 0, 7, -3]
    idx, start, shift, amp, mix = [], [], [], [], []
    for b, (i0, t0, i1, t1) in enumerate(rows):
        idx += [i0, i1]
        start += [t0, t1]
        shift += [shifts[b % 7], shifts[(b + 3) % 7] if i1 >= 0 else 0]
        amp += [10 ** (gains[b % 5] / 20), 10 ** (gains[(b + 2) % 5] / 20)]
        lm = float(rng.random())
        mix.append(max(lm, 1 - lm) if i1 >= 0 else 1.0)
    return (torch.tensor(idx, dtype=torch.int32), torch.tensor(start, dtype=torch.int32), torch.tensor(shift, dtype=torch.int32),
            torch.tensor(amp, dtype=torch.float32), torch.tensor(mix, dtype=torch.float32))


def _bank(waves, offsets, lens, bank_y, waves_dev=None):
    w = torch.from_numpy(waves)
    off = torch.from_numpy(offsets)
    csum = torch.tensor([float(w[o:o + n].double().sum()) for o, n in zip(offsets.tolist(), lens.tolist())], dtype=torch.float64)
    return dict(waves=w.to(DEV) if waves_dev is None else waves_dev, offsets=off.to(DEV),
                lengths=torch.from_numpy(lens.astype(np.int32)).to(DEV), clip_sum=csum.to(DEV),
                bank_y=torch.from_numpy(bank_y).to(DEV), lengths_cpu=torch.from_numpy(lens))


def _check(got, yy, wm, ref, tables, waves, offsets, lens, L):
    """The issue's bounds: out 1e-6 max|ref| (test_wave_augment_against_reference's, the same fp32 arithmetic on fp64-exact
    inputs), labels 1e-7, mask half exactly 1, window means 2e-11 amp mean|x| (any fp64 summation order of n <= 160000 terms
    errs by at most (n - 1) 2^-53 sum|x| = 1.8e-11 sum|x|), padding of unmixed short rows exactly 0."""
    want, want_yy, want_wm = ref
    idx, start, shift, amp, mix = (t.numpy() for t in tables)
    got = got.double().numpy()
    assert np.isfinite(got).all()
    err = np.abs(got - want).max() / np.abs(want).max()
    assert err <= 1e-6, err
    yy = yy.double().numpy()
    assert np.abs(yy[:, :C] - want_yy[:, :C]).max() <= 1e-7 and (yy[:, C:] == 1.0).all()
    worst = 0.0
    for k in range(len(idx)):
        if idx[k | 1] < 0:
            assert wm[k] == 0.0
            continue
        o = int(offsets[idx[k]]) + int(start[k])
        x = waves[o:o + min(int(lens[idx[k]]) - int(start[k]), L)].astype(np.float64)
        bound = 2e-11 * float(amp[k]) * np.abs(x).sum() / L
        worst = max(worst, abs(float(wm[k]) - want_wm[k]) / bound)
        assert abs(float(wm[k]) - want_wm[k]) <= bound, (k, float(wm[k]), want_wm[k], bound)
    for b in range(len(mix)):
        n = int(lens[idx[2 * b]])
        if idx[2 * b + 1] < 0 and n < L:
            pad = np.roll(np.arange(L) >= n, int(shift[2 * b]))
            assert (got[b][pad] == 0.0).all() and pad.sum() == L - n
    return err, worst


@pytest.mark.parametrize("L", [16001, 160000])
@pytest.mark.parametrize("aligned", [True, False])
def test_ragged_augment_against_reference(L, aligned):
    waves, offsets, lens, bank_y = _clips(L, seed=L)
    assert all(o % 2 == 1 for o in offsets)
    tables = _rows(L, np.random.default_rng(L + 1))
    ops.check_ragged_draws(tables[0], tables[1], tables[2], lens, L)
    bank = _bank(waves, offsets, lens, bank_y)
    B = tables[4].numel()
    buf = torch.full((B * L + 8,), float("nan"), device=DEV)
    lo = 4 if aligned else 5                                           # (unaligned: every row start off by 4 bytes)
    out = buf[lo:lo + B * L].view(B, L)
    yy = torch.full((B, 2 * C), -3.0, device=DEV)
    wm = torch.full((2 * B,), -3.0, device=DEV, dtype=torch.float64)
    ops.wave_augment_ragged(bank, *tables, L, out=out, yy=yy, win_mean=wm)
    torch.cuda.synchronize()
    ref = ragged_augment_ref(waves, offsets, lens, bank_y, *(t.numpy() for t in tables), L)
    err, worst = _check(out.cpu(), yy.cpu(), wm.cpu(), ref, tables, waves, offsets, lens, L)
    print(f"L={L} aligned={aligned}: max |out - ref| / max |ref| = {err:.2e}; worst |window mean - ref| / bound = {worst:.2e}")
    assert torch.isnan(buf[:lo]).all() and torch.isnan(buf[lo + B * L:]).all()       # the sentinels around out


def test_ragged_device_tables_repeats_and_null_labels():
    """Device tables (the captured step's path) give the bits of host tables; a repeated call is bit-identical, workspace
    included; yy = NULL (no label row is written: there is no buffer to write) gives the same out bits."""
    L = 16001
    waves, offsets, lens, bank_y = _clips(L, seed=5)
    tables = _rows(L, np.random.default_rng(6))
    bank = _bank(waves, offsets, lens, bank_y)
    B = tables[4].numel()
    wm = [torch.empty(2 * B, device=DEV, dtype=torch.float64) for _ in range(3)]
    out, yy = ops.wave_augment_ragged(bank, *tables, L, win_mean=wm[0])
    dt = tuple(t.to(DEV) for t in tables)
    out2, yy2 = ops.wave_augment_ragged(bank, *dt, L, win_mean=wm[1])
    out3, yy3 = ops.wave_augment_ragged(bank, *dt, L, win_mean=wm[2])
    h = _lib.lib()
    out4 = torch.empty_like(out)
    rc = h.eat_wave_augment_ragged(bank["waves"].data_ptr(), bank["waves"].numel(), bank["offsets"].data_ptr(),
                                   bank["lengths"].data_ptr(), bank["clip_sum"].data_ptr(), None, len(lens), L, 0,
                                   dt[0].data_ptr(), dt[1].data_ptr(), dt[2].data_ptr(), dt[3].data_ptr(), dt[4].data_ptr(),
                                   wm[0].data_ptr(), out4.data_ptr(), None, B, torch.cuda.current_stream().cuda_stream)
    out5, none = ops.wave_augment_ragged(bank, *dt, L, labels=False)
    torch.cuda.synchronize()
    assert rc == 0 and none is None
    for o, y, w in ((out2, yy2, wm[1]), (out3, yy3, wm[2])):
        assert torch.equal(o, out) and torch.equal(y, yy) and torch.equal(w, wm[0])
    assert torch.equal(out4, out) and torch.equal(out5, out)
    assert torch.isfinite(out).all()


def test_ragged_offsets_past_2_31():
    """A flat buffer of 2^31 + 3L samples (torch.empty: only the test's clips are written), two clips past sample 2^31 and one
    across it: the same checks.  The reference runs on a compact copy of the same clips (the result does not depend on the offsets)."""
    L = 16001
    S = 2 ** 31 + 3 * L
    free, _ = torch.cuda.mem_get_info(DEV)
    if free < 10 * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GB of device memory free: the 8.6 GB buffer needs 10")
    waves, offsets, lens, bank_y = _clips(L, seed=9)
    # the clips of _clips, moved: 2L + 3 straddles sample 2^31, L + 1 and L - 1 lie wholly behind it (the last one ends with
    # the buffer), all at odd starts; the others stay at the front
    far = offsets.copy()
    far[4] = 2 ** 31 - L - 4
    far[3] = far[4] + lens[4] + 1
    far[1] = far[3] + lens[3]
    assert all(o % 2 == 1 for o in far) and far[3] > 2 ** 31 and far[1] > 2 ** 31 and far[1] + lens[1] == S
    assert offsets[5] + lens[5] < far[4]
    big = torch.empty(S, device=DEV)
    for i in range(6):
        big[int(far[i]):int(far[i]) + int(lens[i])] = torch.from_numpy(waves[offsets[i]:offsets[i] + lens[i]]).to(DEV)
    tables = _rows(L, np.random.default_rng(10))
    bank = _bank(waves, offsets, lens, bank_y, waves_dev=big)
    bank["offsets"] = torch.from_numpy(far).to(DEV)
    B = tables[4].numel()
    wm = torch.empty(2 * B, device=DEV, dtype=torch.float64)
    out, yy = ops.wave_augment_ragged(bank, *tables, L, win_mean=wm)
    torch.cuda.synchronize()
    ref = ragged_augment_ref(waves, offsets, lens, bank_y, *(t.numpy() for t in tables), L)
    err, worst = _check(out.cpu(), yy.cpu(), wm.cpu(), ref, tables, waves, offsets, lens, L)
    print(f"offsets up to {int(far[1])}: max |out - ref| / max |ref| = {err:.2e}; worst window mean / bound = {worst:.2e}")
    del big, bank
    torch.cuda.empty_cache()


def test_ragged_rejects_bad_draws_and_arguments():
    L = 100
    lens = np.array([99, 100, 101, 300], dtype=np.int64)
    offsets = np.concatenate(([0], np.cumsum(lens)[:-1]))
    bank = _bank(np.zeros(int(lens.sum()), dtype=np.float32), offsets, lens, np.zeros((4, C), dtype=np.float32))

    def t(*v):
        return torch.tensor(v, dtype=torch.int32)

    z, one, m = t(0, 0), torch.ones(2), torch.ones(1)
    ops.wave_augment_ragged(bank, t(3, 2), t(200, 1), t(99, -99), one, m, L)                     # the boundary cases pass
    ops.wave_augment_ragged(bank, t(1, -1), z, z, one, m, L)
    for idx, start, shift in [(t(4, -1), z, z), (t(-1, -1), z, z), (t(0, 4), z, z), (t(0, -2), z, z), (t(0, -1), z, t(100, 0)),
                              (t(0, -1), z, t(-100, 0)), (t(0, -1), t(1, 0), z), (t(1, -1), t(1, 0), z), (t(3, -1), t(201, 0), z),
                              (t(3, -1), t(-1, 0), z), (t(0, 2), t(0, 2), z)]:
        with pytest.raises(ValueError):
            ops.wave_augment_ragged(bank, idx, start, shift, one, m, L)
    with pytest.raises(_lib.EatHipError):
        ops.wave_augment_ragged(bank, t(0, -1), z, z, one, m, L, win_mean=torch.zeros(2, device=DEV))       # fp32 workspace
    h = _lib.lib()
    p, st = bank["waves"].data_ptr(), torch.cuda.current_stream().cuda_stream

    def entry(B=1, L_=L, n_bank=4, n_samples=600, waves=p, out=p, ws=p, yy=p, bank_y=p):
        return ctypes.c_int(h.eat_wave_augment_ragged(waves, n_samples, p, p, p, bank_y, n_bank, L_, C, p, p, p, p, p, ws, out, yy,
                                                      B, st)).value

    assert entry(B=0) == -1 and entry(L_=0) == -1 and entry(n_bank=0) == -1 and entry(n_samples=0) == -1
    assert entry(waves=None) == -1 and entry(out=None) == -1 and entry(ws=None) == -1 and entry(bank_y=None) == -1
    assert entry(B=65536) == -1
    assert b"eat_wave_augment_ragged" in h.eat_last_error_string()
    torch.cuda.synchronize()
