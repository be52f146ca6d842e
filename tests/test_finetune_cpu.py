"""CPU checks of ESC-50 fine-tuning: the float64 references of the two kernels against torch / the reference's transforms,
the host draws, the ESC-50 reader, the program's defaults and the checkpoint surgery."""
import contextlib
import csv
import io
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from efficientat_amd import esc50, ops
from tests.finetune_ref import softmax_ce_ref, wave_augment_ref


def _targets(kind, B, C, g):
    if kind == "onehot":
        y = torch.zeros(B, C, dtype=torch.float64)
        y[torch.arange(B), torch.randint(C, (B,), generator=g)] = 1
    elif kind == "soft":
        y = torch.rand(B, C, generator=g, dtype=torch.float64)
        y /= y.sum(1, keepdim=True)
    elif kind == "zero":
        y = torch.zeros(B, C, dtype=torch.float64)
    else:                                                          # non-normalised rows
        y = torch.rand(B, C, generator=g, dtype=torch.float64) * 3
    return y.float()


@pytest.mark.parametrize("kind", ["onehot", "soft", "zero", "nonnorm"])
@pytest.mark.parametrize("mix", [False, True])
def test_ce_reference_matches_torch_cross_entropy(kind, mix):
    """fp64 CE reference == F.cross_entropy (float64, probability targets) on the loss and the autograd gradient, including the
    reference's two-term mix-up form lam CE(z, y) + (1 - lam) CE(z, y[perm]) (ex_esc50.py:109-112)."""
    g = torch.Generator().manual_seed(7)
    for B, C in [(1, 1), (3, 2), (9, 50), (16, 65)]:
        z = (torch.randn(B, C, generator=g) * 4).float()
        y = _targets(kind, B, C, g)
        zz = z.double().requires_grad_(True)
        if mix:
            perm = torch.randperm(B, generator=g)
            lam = torch.rand(B, generator=g).float()
            l64 = lam.double()
            loss = (F.cross_entropy(zz, y.double(), reduction="none") * l64
                    + F.cross_entropy(zz, y.double()[perm], reduction="none") * (1 - l64)).mean()
            ref = softmax_ce_ref(z.numpy(), y.numpy(), perm.numpy(), lam.numpy())
        else:
            loss = F.cross_entropy(zz, y.double())
            ref = softmax_ce_ref(z.numpy(), y.numpy())
        loss.backward()
        assert abs(ref["loss"] - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
        np.testing.assert_allclose(ref["dlogits"], zz.grad.numpy(), rtol=1e-10, atol=1e-14)
        np.testing.assert_array_equal(ref["argmax"], z.numpy().argmax(1))


def test_ce_reference_argmax_and_nan_semantics():
    z = np.array([[0.0, 0.0, 0.0], [1.0, np.nan, np.nan], [-1.0, 3.0, 3.0]], dtype=np.float32)
    ref = softmax_ce_ref(z, np.eye(3, dtype=np.float32))
    assert list(ref["argmax"]) == [0, 1, 1]
    assert np.isnan(ref["row_loss"][1]) and np.isfinite(ref["row_loss"][[0, 2]]).all()


def _reference_item(raw, L, gain, shift):
    """datasets/esc50.py:43-48 gain (fp32 waveform * python float) + :35-40 pad / truncate, then audiodatasets.py roll."""
    w = raw * 10 ** (gain / 20) if gain else raw
    w = esc50.pad_or_truncate(w.astype(np.float32), L)
    return torch.as_tensor(w.reshape(1, -1)).roll(shift, 1)


def test_augment_reference_restates_the_reference_transforms():
    """Fixed draws: gain, pad / truncate, torch.roll and MixupDataset's arithmetic (x - mean, mix, x - mean) equal the
    reference of eat_wave_augment on the bank of padded rows."""
    rng = np.random.default_rng(3)
    L = 1000
    raws = [rng.standard_normal(n).astype(np.float32) * 0.3 + 0.05 for n in (700, 1000, 1300, 999)]
    bank = np.stack([esc50.pad_or_truncate(r, L) for r in raws])
    cls = np.array([4, 0, 9, 4], dtype=np.int32)
    draws = [(0, 12, -400, -1, 0, 0, 1.0), (1, -12, 999, 2, 5, -999, 0.7), (3, 3, 0, 3, -7, 1, 0.5), (2, 0, 1, 2, 0, -1, 0.9)]
    idx, shift, amp, mix = [], [], [], []
    want, want_y = [], []
    for i0, g0, s0, i1, g1, s1, lm in draws:
        x0 = _reference_item(raws[i0], L, g0, s0)
        idx += [i0, i1]
        shift += [s0, s1]
        amp += [10 ** (g0 / 20), 10 ** (g1 / 20)]
        mix.append(lm)
        y = np.zeros(10)
        if i1 < 0:
            want.append(x0.numpy()[0])
            y[cls[i0]] = 1
        else:
            x1 = _reference_item(raws[i1], L, g1, s1)
            x0, x1 = x0 - x0.mean(), x1 - x1.mean()
            x = x0 * lm + x1 * (1.0 - lm)
            want.append((x - x.mean()).numpy()[0])
            y[cls[i0]] += lm
            y[cls[i1]] += 1 - lm
        want_y.append(y)
    out, y = wave_augment_ref(bank, cls, idx, shift, np.float32(amp), np.float32(mix), 10)
    want = np.stack(want)
    assert np.abs(out - want).max() <= 1e-6 * np.abs(want).max()
    np.testing.assert_allclose(y, np.stack(want_y), atol=1e-7)


def test_draw_augment_consumes_the_rng_streams_in_the_reference_order():
    """MixupDataset.__getitem__ order (datasets/esc50.py:58-71) restated with the reference's own calls: torch.rand(1) < 0.5,
    the clip's gain (torch.randint), its roll (np.random.random_integers), then partner, its gain and roll, and beta(2, 2)."""
    N, g = 37, 12
    batch = [5, 0, 36, 17, 17, 2, 9, 30, 11, 4]
    for wavmix, roll, gain in [(True, True, g), (False, True, g), (True, False, 0), (True, True, 0)]:
        torch.manual_seed(4); np.random.seed(4)
        idx, shift, amp, mix = esc50.draw_augment(batch, N, gain_augment=gain, roll=roll, wavmix=wavmix)
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
            if wavmix and torch.rand(1) < 0.5:
                p = item(i)
                j = torch.randint(N, (1,)).item()
                q = item(j)
                lm = np.random.beta(2, 2)
                want.append((p, q, max(lm, 1 - lm)))
            else:
                want.append((item(i), (-1, 0, 1.0), 1.0))
        assert (torch.rand(1).item(), np.random.rand()) == after
        for b, (p, q, lm) in enumerate(want):
            assert int(idx[2 * b]) == p[0] and int(shift[2 * b]) == p[1] and float(amp[2 * b]) == np.float32(p[2])
            assert int(idx[2 * b + 1]) == q[0] and int(shift[2 * b + 1]) == q[1]
            if q[0] >= 0:
                assert float(amp[2 * b + 1]) == np.float32(q[2])
            assert float(mix[b]) == np.float32(lm)
        ops.check_augment_draws(idx, shift, N, 160000)


def test_augment_draw_validation():
    ops.check_augment_draws(torch.tensor([0, -1, 4, 4]), torch.tensor([0, 0, 99, -99]), 5, 100)
    for idx, shift in [([5, -1], [0, 0]), ([-1, -1], [0, 0]), ([0, -2], [0, 0]), ([0, 5], [0, 0]), ([0, -1], [100, 0]),
                       ([0, -1], [0, -100]), ([0], [0])]:
        with pytest.raises(ValueError):
            ops.check_augment_draws(torch.tensor(idx), torch.tensor(shift), 5, 100)


def _write_wav(path, sr, x):
    from scipy.io import wavfile
    wavfile.write(path, sr, (np.clip(x, -1, 1) * 32767).astype(np.int16))


def test_esc50_reader_on_a_synthetic_folder(tmp_path):
    """Fold split, pad / truncate to 5 s, 44.1 kHz -> 32 kHz resampling (audio_io.load_audio) and the class ids."""
    from efficientat_amd.audio_io import load_audio
    d = tmp_path / "ESC-50"
    (d / "meta").mkdir(parents=True)
    (d / "audio").mkdir()
    rng = np.random.default_rng(1)
    rows = []
    for k in range(10):
        fold, target = 1 + k % 5, (7 * k) % 50
        name = f"{fold}-{k}-A-{target}.wav"
        n = [44100 * 5, 44100 * 2, 44100 * 6, 1000][k % 4]
        _write_wav(str(d / "audio" / name), 44100, 0.3 * rng.standard_normal(n))
        rows.append((name, fold, target))
    with open(d / "meta" / "esc50.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["filename", "fold", "target", "category", "esc10", "src_file", "take"])
        for name, fold, target in rows:
            w.writerow([name, fold, target, "c", "False", "x", "A"])
    for fold in (1, 3):
        tr = esc50.load_split(str(d), fold, True)
        te = esc50.load_split(str(d), fold, False)
        assert tr["names"] == [r[0] for r in rows if r[1] != fold]
        assert te["names"] == [r[0] for r in rows if r[1] == fold]
        for split in (tr, te):
            assert split["bank"].shape == (len(split["names"]), 160000) and split["bank"].dtype == torch.float32
            assert split["bank_cls"].dtype == torch.int32
            for i, name in enumerate(split["names"]):
                assert int(split["bank_cls"][i]) == next(r[2] for r in rows if r[0] == name)
                x, sr = load_audio(str(d / "audio" / name), sr=32000)
                assert sr == 32000
                n = min(len(x), 160000)
                assert torch.equal(split["bank"][i, :n], torch.from_numpy(x[:n]))
                assert not split["bank"][i, n:].any()
            np.testing.assert_allclose(split["bank_mean"].numpy(), split["bank"].double().mean(1).numpy(), rtol=0, atol=1e-15)
    # a 6 s clip at 44.1 kHz resamples to 192000 samples and is truncated, a 2 s one is padded
    assert len(load_audio(str(d / "audio" / rows[2][0]), sr=32000)[0]) == 192000
    # audio_32k/ is preferred when present
    (d / "audio_32k").mkdir()
    for name, _, _ in rows:
        _write_wav(str(d / "audio_32k" / name), 32000, np.full(100, 0.5))
    te = esc50.load_split(str(d), 2, False)
    assert float(te["bank"][0, 50]) == pytest.approx(16383 / 32768, abs=1e-6) and not te["bank"][0, 100:].any()


def test_program_defaults_are_ex_esc50s():
    from efficientat_amd.finetune_esc50 import parse_args
    a = parse_args(["--data", "x"])
    want = dict(experiment_name="ESC50", batch_size=128, fold=1, model_name="mn10_as", pretrain_final_temp=1.0,
                model_width=1.0, head_type="mlp", se_dims="c", n_epochs=80, mixup_alpha=0.3, no_roll=False, no_wavmix=False,
                gain_augment=12, weight_decay=0.0, lr=6e-5, warm_up_len=10, ramp_down_start=10, ramp_down_len=65,
                last_lr_value=0.01, resample_rate=32000, window_size=800, hop_size=320, n_fft=1024, n_mels=128, freqm=0,
                timem=0, fmin=0, fmax=None, fmin_aug_range=10, fmax_aug_range=2000)
    got = {k: getattr(a, k) for k in want}
    assert got == want
    assert (a.init_checkpoint, a.no_graph, a.max_steps, a.out, a.eval_dump, a.json) == (None, False, 0, None, None, False)


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


@pytest.mark.parametrize("head", ["mlp", "fully_convolutional"])
def test_load_init_checkpoint_drops_exactly_the_output_layer(tmp_path, head):
    from efficientat_amd.finetune import load_init_checkpoint
    from efficientat_amd.mn import get_model
    torch.manual_seed(0)
    src = _quiet(get_model, num_classes=527, width_mult=1.0, head_type=head)
    path = str(tmp_path / "as.pt")
    torch.save(src.state_dict(), path)
    torch.manual_seed(1)
    dst = _quiet(get_model, num_classes=50, width_mult=1.0, head_type=head)
    before = {k: v.clone() for k, v in dst.state_dict().items()}
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        dropped = load_init_checkpoint(dst, path)
    assert "Number of classes defined: 50, but try to load pre-trained layer with logits: 527\nDropping last layer." in out.getvalue()
    want = ["classifier.5.weight", "classifier.5.bias"] if head == "mlp" else \
        ["classifier.0.weight"] + [k for k in src.state_dict() if k.startswith("classifier.1.")]
    assert sorted(dropped) == sorted(want)
    ssd = src.state_dict()
    for k, v in dst.state_dict().items():
        if k in want:
            assert torch.equal(v, before[k]), k                                # the new output layer keeps its init
        else:
            assert torch.equal(v, ssd[k]), k
    # same class count: a plain strict load
    same = _quiet(get_model, num_classes=527, width_mult=1.0, head_type=head)
    assert load_init_checkpoint(same, path) == []
    assert all(torch.equal(v, ssd[k]) for k, v in same.state_dict().items())


def test_load_init_checkpoint_refuses_other_mismatches(tmp_path):
    from efficientat_amd.finetune import load_init_checkpoint
    from efficientat_amd.mn import get_model
    path = str(tmp_path / "as.pt")
    torch.save(_quiet(get_model, num_classes=527, head_type="multihead_attention_pooling").state_dict(), path)
    with pytest.raises(ValueError):
        load_init_checkpoint(_quiet(get_model, num_classes=50, head_type="multihead_attention_pooling"), path)
    torch.save(_quiet(get_model, num_classes=527, width_mult=0.5).state_dict(), path)
    with pytest.raises(ValueError):
        load_init_checkpoint(_quiet(get_model, num_classes=50, width_mult=1.0), path)
