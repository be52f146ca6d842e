"""CPU checks of OpenMIC fine-tuning: the float64 references of tests/openmic_ref.py against the reference's own torch
expressions and sklearn, the host draws, the bank reader, the program's defaults and the new library symbols."""
import importlib.util
import inspect
import io
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from efficientat_amd import _lib, esc50, openmic, ops
from tests import rank_metrics_ref as R
from tests.openmic_ref import masked_ap_auc, masked_bce_ref, openmic_targets_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _packed(B, C, g):
    """Post-wave-mix rows: soft labels on both sides of 0.5 and exactly 0.5, hard labels, masks 0 / 1 with an all-zero and
    an all-one row."""
    lab = torch.rand(B, C, generator=g)
    lab[torch.rand(B, C, generator=g) < 0.2] = 0.5
    lab[torch.rand(B, C, generator=g) < 0.2] = 1.0
    lab[torch.rand(B, C, generator=g) < 0.2] = 0.0
    lab[0, 0] = 0.5
    lab[-1, -1] = float(np.nextafter(np.float32(0.5), np.float32(1)))
    mask = (torch.rand(B, C, generator=g) < 0.6).float()
    mask[0] = 0.0
    mask[-1] = 1.0
    return torch.cat([lab, mask], 1).float()


@pytest.mark.parametrize("mix", [False, True])
def test_bce_reference_matches_the_reference_loss_expression(mix):
    """fp64 reference == the literal lines of ex_openmic.py:102-121 (evaluated in float64) on the loss and on the autograd
    gradient, with and without mix-up."""
    g = torch.Generator().manual_seed(3)
    for bs, C in [(1, 1), (3, 2), (9, 20), (16, 65)]:
        y_hat = (torch.randn(bs, C, generator=g) * 4).float()
        packed = _packed(bs, C, g)
        zz = y_hat.double().requires_grad_(True)
        y = packed.double()
        y_mask = y[:, C:]
        y = y[:, :C] > 0.5
        y = y.double()
        if mix:
            rn_indices = torch.randperm(bs, generator=g)
            lam32 = torch.rand(bs, generator=g).float()
            lam = lam32.double()
            y_mix = y * lam.reshape(bs, 1) + y[rn_indices] * (1. - lam.reshape(bs, 1))
            samples_loss = F.binary_cross_entropy_with_logits(zz, y_mix, reduction="none")
            samples_loss = y_mask * samples_loss
            ref = masked_bce_ref(y_hat.numpy(), packed.numpy(), rn_indices.numpy(), lam32.numpy())
        else:
            samples_loss = F.binary_cross_entropy_with_logits(zz, y, reduction="none")
            samples_loss = y_mask * samples_loss
            ref = masked_bce_ref(y_hat.numpy(), packed.numpy())
        loss = samples_loss.mean()
        loss.backward()
        assert abs(ref["loss"] - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
        np.testing.assert_allclose(ref["row_loss"], samples_loss.detach().mean(1).numpy(), rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(ref["dlogits"], zz.grad.numpy(), rtol=1e-10, atol=1e-15)
        np.testing.assert_allclose(ref["probs"], torch.sigmoid(y_hat.double()).numpy(), rtol=1e-13, atol=0)


def test_bce_reference_binarizes_masks_rows_and_propagates_nan():
    z = np.array([[2.0, -3.0], [np.nan, 1.0], [0.5, 0.5]], dtype=np.float32)
    half_up = np.nextafter(np.float32(0.5), np.float32(1))
    yy = np.array([[0.5, half_up, 1, 1], [1, 0, 0, 0], [0.3, 0.9, 0, 1]], dtype=np.float32)
    ref = masked_bce_ref(z, yy)
    sp = lambda v: np.log1p(np.exp(v))                                    # noqa: E731  softplus
    assert ref["row_loss"][0] == pytest.approx((sp(2.0) + sp(3.0)) / 2, rel=1e-14)      # 0.5 -> 0, just above -> 1
    assert np.isnan(ref["row_loss"][1]) and np.isnan(ref["loss"])         # a NaN logit under mask 0: 0 * nan
    assert np.isnan(ref["dlogits"][1, 0]) and ref["dlogits"][1, 1] == 0.0
    assert ref["row_loss"][2] == pytest.approx(sp(-0.5) / 2, rel=1e-14) and ref["dlogits"][2, 0] == 0.0
    soft = masked_bce_ref(z[2:], yy[2:], binarize=False)
    assert soft["row_loss"][0] == pytest.approx((sp(0.5) - 0.5 * 0.9) / 2, rel=1e-6)
    bad = masked_bce_ref(z, yy, perm=np.array([1, 3, 0]), lam=np.float32([0.7, 0.7, 0.7]))
    assert np.isnan(bad["row_loss"][1]) and np.isnan(bad["dlogits"][1]).all() and np.isfinite(bad["row_loss"][2])


def _mixup_dataset_item(item1, item2, mixing, l):
    """MixupDataset.__getitem__ (datasets/openmic.py:74-95) on the label rows, with its draws handed in."""
    y1 = torch.as_tensor(item1.copy())
    if mixing:
        y2 = torch.as_tensor(item2.copy())
        assert len(y1) == 40, "only for openmic this works"
        y_mask1 = (torch.as_tensor(y1[20:]) > 0.5).float()
        y_mask2 = (torch.as_tensor(y2[20:]) > 0.5).float()
        y1[:20] *= y_mask1
        y2[:20] *= y_mask2
        yres = (y1 * l + y2 * (1. - l))
        yres[20:] = torch.stack([y_mask1, y_mask2]).max(dim=0).values
        return yres
    return y1


def test_label_reference_restates_mixup_dataset():
    """Labels in eighths and weights exact in fp32: the reference's fp32 arithmetic is exact, so is the equality.  With
    arbitrary labels and weights the reference rounds its two products and the sum to fp32 (and its 1 - l from a double l):
    at most 4 roundings of 2^-24 on values <= 1, i.e. 2.4e-7."""
    rng = np.random.default_rng(0)
    n = 7
    lab = rng.integers(0, 9, (n, 20)).astype(np.float32) / 8
    mask = (rng.random((n, 20)) < 0.5).astype(np.float32)
    mask[0], mask[1] = 1.0, 0.0
    bank_y = np.concatenate([lab, mask], 1)
    idx = np.array([0, -1, 1, -1, 2, 3, 3, 2, 4, 4, 0, 1, 1, 0, 5, 6], dtype=np.int32)
    mix = np.float32([1.0, 1.0, 0.75, 0.625, 0.5, 0.8125, 0.5, 0.9375])
    ref = openmic_targets_ref(bank_y, idx, mix)
    for b in range(len(mix)):
        i0, i1 = idx[2 * b], idx[2 * b + 1]
        want = _mixup_dataset_item(bank_y[i0], bank_y[max(i1, 0)], i1 >= 0, float(mix[b]))
        np.testing.assert_array_equal(ref[b], want.double().numpy())
    assert np.array_equal(ref[1], bank_y[1])                              # unmixed: the labels are NOT multiplied by the mask
    assert (ref[1, :20] != 0).any() and not ref[1, 20:].any()
    bank_y[:, :20] = rng.random((n, 20)).astype(np.float32)
    ls = rng.beta(2, 2, len(mix))
    ls = np.maximum(ls, 1 - ls)
    ref = openmic_targets_ref(bank_y, idx, np.float32(ls))
    for b in range(len(mix)):
        i0, i1 = idx[2 * b], idx[2 * b + 1]
        want = _mixup_dataset_item(bank_y[i0], bank_y[max(i1, 0)], i1 >= 0, float(ls[b]))
        np.testing.assert_allclose(ref[b], want.double().numpy(), rtol=0, atol=2.4e-7)
    assert np.isnan(openmic_targets_ref(bank_y, [7, -1, 0, 7, -1, -1, 0, -2], np.ones(4, np.float32))).all()


def test_draw_augment_consumes_the_rng_streams_in_openmics_order():
    """MixupDataset.__getitem__ order of datasets/openmic.py:74-81 restated with the reference's own calls: the clip's gain
    (torch.randint) and roll (np.random.random_integers) FIRST, then torch.rand(1) < 0.5, the partner, its gain and roll, and
    beta(2, 2).  ESC-50's order (torch.rand first) turns the same streams into other tables."""
    N, g = 37, 12
    batch = [5, 0, 36, 17, 17, 2, 9, 30, 11, 4]
    differs = False
    for wavmix, roll, gain in [(True, True, g), (False, True, g), (True, False, 0), (True, True, 0)]:
        torch.manual_seed(4); np.random.seed(4)
        idx, shift, amp, mix = openmic.draw_augment(batch, N, gain_augment=gain, roll=roll, wavmix=wavmix)
        after = (torch.rand(1).item(), np.random.rand())
        torch.manual_seed(4); np.random.seed(4)
        want = []

        def item(i):
            a = 1.0
            if gain:
                a = 10 ** ((torch.randint(gain * 2, (1,)).item() - gain) / 20)
            s = 0
            if roll:
                with pytest.warns(DeprecationWarning):
                    s = int(np.random.random_integers(-4000, 4000))
            return i, s, a

        for i in batch:
            p = item(i)                                                   # x1, f1, y1 = self.dataset[index]
            if wavmix and torch.rand(1) < 0.5:
                j = torch.randint(N, (1,)).item()
                q = item(j)
                lm = np.random.beta(2, 2)
                want.append((p, q, max(lm, 1 - lm)))
            else:
                want.append((p, (-1, 0, 1.0), 1.0))
        assert (torch.rand(1).item(), np.random.rand()) == after
        for b, (p, q, lm) in enumerate(want):
            assert int(idx[2 * b]) == p[0] and int(shift[2 * b]) == p[1] and float(amp[2 * b]) == np.float32(p[2])
            assert int(idx[2 * b + 1]) == q[0] and int(shift[2 * b + 1]) == q[1]
            if q[0] >= 0:
                assert float(amp[2 * b + 1]) == np.float32(q[2])
            assert float(mix[b]) == np.float32(lm)
        ops.check_augment_draws(idx, shift, N, 320000)
        torch.manual_seed(4); np.random.seed(4)
        other = esc50.draw_augment(batch, N, gain_augment=gain, roll=roll, wavmix=wavmix)
        same = all(torch.equal(a, b) for a, b in zip((idx, shift, amp, mix), other))
        # torch.rand and the gain share the torch stream: the two orders differ exactly when both are drawn (the roll and
        # the beta are numpy's, in the same order either way)
        assert same == (not (wavmix and gain))
        differs |= not same
    assert differs


def _metric_columns(rng, n):
    """(scores, targets, weights) columns, tied and untied, whose top-ranked item is masked out."""
    cols = []
    for k in range(300):
        s = rng.standard_normal(n) if k % 2 else rng.integers(0, 1 + k % 7, n).astype(np.float64)
        y = (rng.random(n) < 0.3).astype(np.float64)
        w = (rng.random(n) < 0.6).astype(np.float64)
        w[np.argmax(s)] = 0.0
        cols.append((s.astype(np.float32), y, w))
    return cols


def test_masked_oracle_is_sklearns_sample_weight():
    """The oracle on the rows of weight 1 == sklearn's average_precision_score / roc_auc_score with sample_weight (what
    ex_openmic.py:194-204 calls) - columns where sklearn raises (one class among the weighted rows) are left out."""
    sk = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(1)
    worst, used = 0.0, 0
    for s, y, w in _metric_columns(rng, 40):
        ap, auc = masked_ap_auc(s, y, w)
        try:
            auc_sk = sk.roc_auc_score(y, s, sample_weight=w)
        except ValueError:
            continue
        ap_sk = sk.average_precision_score(y, s, sample_weight=w)
        worst = max(worst, abs(ap[0] - ap_sk), abs(auc[0] - auc_sk))
        used += 1
    print(f"{used} columns, worst |oracle - sklearn| {worst:.2e}")
    assert used > 200 and worst <= 1e-12


def test_masked_oracle_degenerate_columns():
    s = np.float32([0.9, 0.8, 0.7, 0.6])
    y = np.float64([1, 0, 1, 0])
    assert masked_ap_auc(s, y, np.float64([1, 1, 1, 1])) == tuple(np.array([v]) for v in R.ap_auc_column(s, y))
    ap, auc = masked_ap_auc(s, y, np.zeros(4))
    assert ap[0] == 0.0 and np.isnan(auc[0])                              # no weighted item at all
    ap, auc = masked_ap_auc(s, y, np.float64([1, 0, 1, 0]))
    assert ap[0] == 1.0 and np.isnan(auc[0])                              # only positives among the weighted items
    ap, auc = masked_ap_auc(s, y, np.float64([0, 1, 0, 1]))
    assert ap[0] == 0.0 and np.isnan(auc[0])                              # only negatives
    ap, auc = masked_ap_auc(s, y, np.float64([0, 1, 1, 1]))               # top item masked: 0.8 (neg), 0.7 (pos), 0.6 (neg)
    assert ap[0] == pytest.approx(0.5) and auc[0] == pytest.approx(0.5)


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_load_bank_round_trip(tmp_path, dtype):
    rng = np.random.default_rng(2)
    n, L = 5, 1000
    wave = rng.uniform(-0.9, 0.9, (n, L)).astype(np.float32)
    stored = np.rint(wave * 32767.0).astype(np.int16) if dtype == np.int16 else wave
    targets = np.concatenate([rng.random((n, 20)), rng.random((n, 20)) < 0.5], 1).astype(np.float32)
    names = [f"{i:06d}_{i * 10}" for i in range(n)]
    np.save(tmp_path / "waves.npy", stored)
    np.save(tmp_path / "targets.npy", targets)
    (tmp_path / "names.txt").write_text("\n".join(names) + "\n")
    bank = openmic.load_bank(str(tmp_path))
    want = stored.astype(np.float32) / np.float32(32767.0) if dtype == np.int16 else wave
    assert bank["bank"].dtype == torch.float32 and bank["bank_mean"].dtype == torch.float64
    np.testing.assert_array_equal(bank["bank"].numpy(), want)
    assert np.abs(bank["bank"].numpy() - wave).max() <= 0.5 / 32767 + 1e-7
    np.testing.assert_allclose(bank["bank_mean"].numpy(), want.astype(np.float64).mean(1), rtol=0, atol=1e-15)
    np.testing.assert_array_equal(bank["bank_y"].numpy(), targets)
    assert bank["names"] == names and openmic.N_CLASSES == 20 and openmic.CLIP_SECONDS == 10
    np.save(tmp_path / "targets.npy", targets[:, :39])
    with pytest.raises(ValueError):
        openmic.load_bank(str(tmp_path))
    np.save(tmp_path / "targets.npy", targets[:4])
    with pytest.raises(ValueError):
        openmic.load_bank(str(tmp_path))
    np.save(tmp_path / "targets.npy", targets)
    (tmp_path / "names.txt").write_text("\n".join(names[:3]) + "\n")
    with pytest.raises(ValueError):
        openmic.load_bank(str(tmp_path))


def test_program_defaults_are_ex_openmics():
    from efficientat_amd.finetune_openmic import parse_args
    a = parse_args(["--train_bank", "x", "--test_bank", "y"])
    want = dict(experiment_name="OpenMic", batch_size=64, model_name="mn10_as", pretrain_final_temp=1.0, model_width=1.0,
                head_type="mlp", se_dims="c", n_epochs=80, mixup_alpha=0.3, no_roll=False, no_wavmix=False, gain_augment=12,
                weight_decay=0.0, lr=1e-5, warm_up_len=10, ramp_down_start=10, ramp_down_len=65, last_lr_value=0.01,
                resample_rate=32000, window_size=800, hop_size=320, n_fft=1024, n_mels=128, freqm=0, timem=0, fmin=0,
                fmax=None, fmin_aug_range=10, fmax_aug_range=2000)
    assert {k: getattr(a, k) for k in want} == want
    assert (a.train_bank, a.test_bank, a.init_checkpoint, a.seed, a.no_graph, a.max_steps, a.precision, a.out, a.eval_dump,
            a.json) == ("x", "y", None, 0, False, 0, None, None, None, False)
    for gone in ("cuda", "num_workers", "pretrained", "train"):
        assert not hasattr(a, gone)


def test_library_exports_the_openmic_symbols():
    """(that the library exports what the header declares: tests/test_host_cpu.py, which names these three)"""
    from efficientat_amd import metrics
    assert {"eat_masked_bce_fwd_bwd", "eat_openmic_targets", "eat_rank_metrics_masked"} <= set(_lib.exported_symbols())
    for fn in (metrics.ap_auc, metrics.average_precision, metrics.roc_auc):
        assert inspect.signature(fn).parameters["sample_weight"].default is None


def test_hdf5_converter_round_trip(tmp_path):
    """tools/openmic_to_bank.py (QUARANTINED, never run where this package was built): a 3-clip HDF5 + mp3 file in the layout
    of openmic_*.csv_mp3.hdf, converted and read back by openmic.load_bank.  Needs h5py and PyAV - skipped where they are
    missing, so a pass anywhere is the first execution of that tool."""
    h5py = pytest.importorskip("h5py")
    av = pytest.importorskip("av")
    sr, n = 32000, 3
    rng = np.random.default_rng(0)
    names, blobs = [], []
    for i in range(n):
        wave = (0.3 * np.sin(2 * np.pi * (300.0 + 200 * i) * np.arange(2 * sr) / sr)).astype(np.float32)
        buf = io.BytesIO()
        with av.open(buf, mode="w", format="mp3") as c:
            st = c.add_stream("mp3", rate=sr)
            frame = av.AudioFrame.from_ndarray(wave.reshape(1, -1), format="fltp", layout="mono")
            frame.sample_rate = sr
            for pkt in st.encode(frame):
                c.mux(pkt)
            for pkt in st.encode(None):
                c.mux(pkt)
        blobs.append(np.frombuffer(buf.getvalue(), dtype=np.uint8))
        names.append(("%06d_%d" % (i, 10 * i)).encode())
    targets = rng.random((n, 40)).astype(np.float32)
    with h5py.File(tmp_path / "openmic_test.csv_mp3.hdf", "w") as f:
        f.create_dataset("audio_name", data=np.array(names))
        d = f.create_dataset("mp3", (n,), dtype=h5py.vlen_dtype(np.dtype("uint8")))
        for i, b in enumerate(blobs):
            d[i] = b
        f.create_dataset("target", data=targets)
    spec = importlib.util.spec_from_file_location("eat_openmic_to_bank", os.path.join(ROOT, "tools", "openmic_to_bank.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.convert(str(tmp_path / "openmic_test.csv_mp3.hdf"), str(tmp_path / "bank")) == n
    bank = openmic.load_bank(str(tmp_path / "bank"))
    assert bank["bank"].shape == (n, 10 * sr) and bank["names"] == [b.decode() for b in names]
    np.testing.assert_array_equal(bank["bank_y"].numpy(), targets)
    x = bank["bank"].numpy()
    assert 0.1 < np.abs(x[1, :2 * sr]).max() < 0.5 and np.abs(x[1, 3 * sr:]).max() == 0.0     # decoded tone, zero padding
