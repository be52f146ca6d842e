"""CPU checks of FSD50K fine-tuning: the host draws against a transcription of the reference's call sequence, the float64
reference of tests/fsd50k_ref.py against the reference's own float32 transforms, the draw validation, the ragged bank reader,
the program's defaults and the new library symbol."""
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

from efficientat_amd import _lib, esc50, fsd50k, openmic, ops
from tests.fsd50k_ref import ragged_augment_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_draws(batch, lengths, L, gain, roll, wavmix):
    """datasets/fsd50k.py restated with the reference's own calls: MixupDataset.__getitem__ (:80-92) around
    PreprocessDataset(roll_func) around AudioSetDataset.__getitem__ (:147-149: pydub_augment, then pad_or_truncate).
    -> per sample ((index, start, shift, amp), partner tuple or None, l) and the number of crop draws made."""
    N = len(lengths)
    crops = [0]

    def fetch(i):
        a = 1.0
        if gain:                                                              # pydub_augment
            g = torch.randint(gain * 2, (1,)).item() - gain
            a = 10 ** (g / 20)
        st = 0
        if not lengths[i] <= L:                                               # pad_or_truncate: the else branch draws
            st = torch.randint(0, lengths[i] - L + 1, (1,)).item()
            crops[0] += 1
        sf = 0
        if roll:                                                              # roll_func
            with pytest.warns(DeprecationWarning):
                sf = int(np.random.random_integers(-4000, 4000))
        return i, st, sf, a

    want = []
    for index in batch:
        if wavmix and torch.rand(1) < 0.5:
            p = fetch(index)
            idx2 = torch.randint(N, (1,)).item()
            q = fetch(idx2)
            l = np.random.beta(2, 2)
            l = max(l, 1. - l)
            want.append((p, q, l))
        else:
            want.append((fetch(index), None, 1.0))
    return want, crops[0]


def test_draw_augment_consumes_the_rng_streams_in_fsd50ks_order():
    L = 5000                                                                  # (above the roll's range of 4000)
    lengths = [L - 1, L, L + 1, 3 * L, 300, 2 * L + 3, L + 1, 7]
    N = len(lengths)
    batch = [3, 0, 2, 1, 5, 5, 4, 6, 7, 3, 2, 0]
    crop_draws = 0
    for wavmix, roll, gain in [(True, True, 12), (False, True, 12), (True, False, 0), (True, True, 0), (False, False, 0)]:
        torch.manual_seed(4); np.random.seed(4)
        idx, start, shift, amp, mix = fsd50k.draw_augment(batch, torch.tensor(lengths), L, gain_augment=gain, roll=roll,
                                                          wavmix=wavmix)
        after = (torch.random.get_rng_state(), np.random.get_state())
        torch.manual_seed(4); np.random.seed(4)
        want, n_crops = _reference_draws(batch, lengths, L, gain, roll, wavmix)
        crop_draws += n_crops
        # nothing extra was consumed from either stream
        assert torch.equal(torch.random.get_rng_state(), after[0])
        st = np.random.get_state()
        assert st[0] == after[1][0] and np.array_equal(st[1], after[1][1]) and st[2:] == after[1][2:]
        n_long = 0
        for b, (p, q, lm) in enumerate(want):
            q = q or (-1, 0, 0, 1.0)
            for k, s in ((2 * b, p), (2 * b + 1, q)):
                assert (int(idx[k]), int(start[k]), int(shift[k])) == s[:3], (b, k)
                assert float(amp[k]) == np.float32(s[3])
                if s[0] >= 0:
                    # the crop is drawn only for len > L, and stays inside the clip
                    assert (int(start[k]) == 0) if lengths[s[0]] <= L else (0 <= int(start[k]) <= lengths[s[0]] - L)
                    n_long += lengths[s[0]] > L
            assert float(mix[b]) == np.float32(lm)
        assert n_crops == n_long                                              # one crop draw per long-clip fetch, no other
        ops.check_ragged_draws(idx, start, shift, torch.tensor(lengths), L)
        # ESC-50's and OpenMIC's orders turn the same streams into other tables: the crop draws sit in the torch stream
        for other in (esc50.draw_augment, openmic.draw_augment):
            torch.manual_seed(4); np.random.seed(4)
            o = other(batch, N, gain_augment=gain, roll=roll, wavmix=wavmix)
            same = all(torch.equal(a, b) for a, b in zip((idx, shift, amp, mix), o))
            assert same == (not (wavmix or gain)), (other.__module__, wavmix, gain)   # (no later torch draw: nothing to shift)
    assert crop_draws > 10
    # a bank without long clips draws nothing for the crop: ESC-50's order exactly, OpenMIC's is still another
    short = torch.tensor([L - 1, L, 300, 7, L, 20, 4999, 1])
    torch.manual_seed(4); np.random.seed(4)
    idx, start, shift, amp, mix = fsd50k.draw_augment(batch, short, L)
    assert not start.any()
    torch.manual_seed(4); np.random.seed(4)
    assert all(torch.equal(a, b) for a, b in zip((idx, shift, amp, mix), esc50.draw_augment(batch, N)))
    torch.manual_seed(4); np.random.seed(4)
    assert not all(torch.equal(a, b) for a, b in zip((idx, shift, amp, mix), openmic.draw_augment(batch, N)))


def test_draw_eval_crops_draws_per_long_clip_in_bank_order():
    L = 1000
    lengths = [L - 1, L, L + 1, 3 * L, 300, 2 * L + 3]
    torch.manual_seed(9)
    got = fsd50k.draw_eval_crops(torch.tensor(lengths), L)
    after = torch.random.get_rng_state()
    torch.manual_seed(9)
    want = [torch.randint(0, n - L + 1, (1,)).item() if n > L else 0 for n in lengths]
    assert got.tolist() == want and got.dtype == torch.int32 and torch.equal(torch.random.get_rng_state(), after)
    assert all(0 <= s <= max(0, n - L) for s, n in zip(want, lengths)) and want[3] > 0


def _pad_or_truncate_at(x, audio_length, offset):
    """datasets/fsd50k.py:50-59 with its torch.randint draw handed in."""
    if len(x) <= audio_length:
        return np.concatenate((x, np.zeros(audio_length - len(x), dtype=np.float32)), axis=0)
    else:
        return x[offset:offset + audio_length]


def _reference_item(raw, L, gain, offset, sf):
    """AudioSetDataset.__getitem__ (pydub_augment: fp32 waveform * python float; pad_or_truncate; reshape(1, -1)), then
    roll_func."""
    waveform = raw * 10 ** (gain / 20) if gain else raw
    waveform = _pad_or_truncate_at(waveform.astype(np.float32), L, offset)
    return torch.as_tensor(waveform.reshape(1, -1)).roll(sf, 1)


def test_ragged_reference_restates_the_reference_transforms():
    """Fixed draws through the reference's float32 transforms - gain, pad or crop, torch.roll, MixupDataset.__getitem__
    including its final `x - x.mean()` - against the float64 reference of eat_wave_augment_ragged, at the bound
    tests/test_finetune_cpu.py takes for ESC-50: 1e-6 max|x|.  The final mean the kernel drops is zero in real arithmetic;
    in the reference's float32 it is the rounding left over from the two earlier mean subtractions - measured here below
    1e-7 max|x| (a few units of 2^-24), and asserted below 1e-6 max|x|."""
    rng = np.random.default_rng(3)
    L = 1000
    lens = [700, 1000, 1001, 2003, 3000, 1]
    raws = [rng.standard_normal(n).astype(np.float32) * 0.3 + 0.05 for n in lens]
    offsets = np.concatenate(([0], np.cumsum(lens)[:-1]))
    waves = np.concatenate(raws)
    bank_y = (rng.random((len(lens), 7)) < 0.4).astype(np.float32)
    # (i0, gain0, start0, shift0, i1, gain1, start1, shift1, l)
    draws = [(0, 12, 0, -400, -1, 0, 0, 0, 1.0), (3, -12, 1003, 999, -1, 0, 0, 0, 1.0), (2, 5, 1, 0, -1, 0, 0, 0, 1.0),
             (0, -3, 0, 17, 4, 12, 2000, -999, 0.7), (4, 0, 0, 1, 3, -7, 500, -1, 0.5), (4, 3, 100, 4, 4, -3, 1900, -4, 0.9),
             (5, 12, 0, 0, 1, -12, 0, 3, 0.625), (1, 0, 0, 0, -1, 0, 0, 0, 1.0)]
    idx, start, shift, amp, mix, want, want_y, dropped = [], [], [], [], [], [], [], 0.0
    for i0, g0, t0, s0, i1, g1, t1, s1, l in draws:
        idx += [i0, i1]; start += [t0, t1]; shift += [s0, s1]; amp += [10 ** (g0 / 20), 10 ** (g1 / 20)]; mix.append(l)
        x1, y1 = _reference_item(raws[i0], L, g0, t0, s0), bank_y[i0]
        if i1 < 0:
            want.append(x1.numpy()[0]); want_y.append(y1)
            continue
        x2, y2 = _reference_item(raws[i1], L, g1, t1, s1), bank_y[i1]
        x1 = x1 - x1.mean()
        x2 = x2 - x2.mean()
        x = (x1 * l + x2 * (1. - l))
        dropped = max(dropped, abs(float(x.mean())) / float(x.abs().max()))
        x = x - x.mean()
        want.append(x.numpy()[0]); want_y.append((y1 * l + y2 * (1. - l)))
    ops.check_ragged_draws(torch.tensor(idx), torch.tensor(start), torch.tensor(shift), torch.tensor(lens), L)
    out, yy, wm = ragged_augment_ref(waves, offsets, lens, bank_y, idx, start, shift, np.float32(amp), np.float32(mix), L)
    want = np.stack(want).astype(np.float64)
    err = np.abs(out - want).max() / np.abs(want).max()
    print(f"max |ref - reference transforms| / max|x| {err:.2e}; dropped final mean / max|x| {dropped:.2e}")
    assert err <= 1e-6 and dropped <= 1e-6
    np.testing.assert_allclose(yy[:, :7], np.stack(want_y), rtol=0, atol=1e-7)
    assert (yy[:, 7:] == 1.0).all()
    # the padding of an unmixed short row is exactly zero and rolls with the clip: 700 samples rolled by -400
    assert not out[0, 300:600].any() and out[0, :300].all() and out[0, 600:].all()
    assert not wm[[0, 1, 2, 3, 4, 5, 14, 15]].any() and wm[6:14].all()


def test_check_ragged_draws_boundaries_and_violations():
    L = 1000
    lengths = torch.tensor([999, 1000, 1001, 3000])
    z = torch.zeros(2, dtype=torch.int32)

    def t(*v):
        return torch.tensor(v, dtype=torch.int32)

    ops.check_ragged_draws(t(3, 2), t(2000, 1), t(999, -999), lengths, L)     # start = len - L, shifts at the ends
    ops.check_ragged_draws(t(1, -1), z, z, lengths, L)                        # len == L: start 0
    ops.check_ragged_draws(t(0, 3), t(0, 0), z, lengths, L)
    for idx, start, shift in [(t(4, -1), z, z), (t(-1, -1), z, z), (t(0, 4), z, z), (t(0, -2), z, z),          # rows
                              (t(0, -1), z, t(1000, 0)), (t(0, -1), z, t(-1000, 0)),                           # |shift| < L
                              (t(0, -1), t(1, 0), z), (t(1, -1), t(1, 0), z),                                  # fits: start 0
                              (t(3, -1), t(2001, 0), z), (t(3, -1), t(-1, 0), z), (t(0, 2), t(0, 2), z),       # long: the range
                              (t(0), t(0), t(0)), (t(0, -1), t(0), z), (torch.zeros(0), torch.zeros(0), torch.zeros(0))]:
        with pytest.raises(ValueError):
            ops.check_ragged_draws(idx, start, shift, lengths, L)


@pytest.mark.parametrize("dtype", [np.int16, np.float32])
def test_load_bank_round_trip(tmp_path, dtype):
    rng = np.random.default_rng(2)
    lens = np.array([300, 1, 2500, 1000, 77], dtype=np.int64)
    wave = rng.uniform(-0.9, 0.9, int(lens.sum())).astype(np.float32) + 0.05
    stored = np.rint(wave * 32767.0).astype(np.int16) if dtype == np.int16 else wave
    targets = (rng.random((5, 200)) < 0.05)
    targets = targets.astype(np.uint8) if dtype == np.int16 else targets.astype(np.float32)
    names = [f"{i * 1000}" for i in range(5)]

    def write(w=stored, le=lens, t=targets, nm=names):
        np.save(tmp_path / "waves.npy", w)
        np.save(tmp_path / "lengths.npy", le)
        np.save(tmp_path / "targets.npy", t)
        (tmp_path / "names.txt").write_text("\n".join(nm) + "\n")

    write()
    bank = fsd50k.load_bank(str(tmp_path))
    want = stored.astype(np.float32) / np.float32(32767.0) if dtype == np.int16 else wave
    assert bank["waves"].dtype == torch.float32 and bank["clip_sum"].dtype == torch.float64
    assert bank["offsets"].dtype == torch.int64 and bank["lengths"].dtype == torch.int32 and bank["bank_y"].dtype == torch.float32
    np.testing.assert_array_equal(bank["waves"].numpy(), want)
    assert np.abs(bank["waves"].numpy() - wave).max() <= 0.5 / 32767 + 1e-7
    offs = np.concatenate(([0], np.cumsum(lens)[:-1]))
    np.testing.assert_array_equal(bank["offsets"].numpy(), offs)
    np.testing.assert_array_equal(bank["lengths"].numpy(), lens)
    np.testing.assert_array_equal(bank["lengths_cpu"].numpy(), lens)
    for i in range(5):
        x = want[offs[i]:offs[i] + lens[i]].astype(np.float64)
        # the fp64 sum, whatever the order: (n - 1) 2^-53 sum|x|
        assert abs(float(bank["clip_sum"][i]) - x.sum()) <= lens[i] * 2.0 ** -53 * np.abs(x).sum()
    np.testing.assert_array_equal(bank["bank_y"].numpy(), targets.astype(np.float32))
    assert bank["names"] == names and fsd50k.N_CLASSES == 200 and fsd50k.CLIP_SECONDS == 10
    bad = [dict(w=stored[:-1]), dict(w=stored.reshape(1, -1)), dict(w=stored.astype(np.float64)),
           dict(le=lens[:4]), dict(le=np.array([300, 0, 2501, 1000, 77])), dict(le=lens.astype(np.float32)),
           dict(le=lens.reshape(1, -1)), dict(t=targets[:, :199]), dict(t=targets[:4]), dict(t=targets.astype(np.int32)),
           dict(nm=names[:3])]
    for kw in bad:
        write(**kw)
        with pytest.raises(ValueError):
            fsd50k.load_bank(str(tmp_path))
    write()
    fsd50k.load_bank(str(tmp_path))


def test_program_defaults_are_ex_fsd50ks():
    from efficientat_amd.finetune_fsd50k import parse_args
    a = parse_args(["--eval_bank", "z"])
    want = dict(experiment_name="FSD50K", train=False, batch_size=64, variable_eval_length=False, model_name="mn10_as",
                pretrain_final_temp=1.0, model_width=1.0, head_type="mlp", se_dims="c", n_epochs=80, mixup_alpha=0.3,
                no_roll=False, no_wavmix=False, gain_augment=12, weight_decay=0.0, lr=7e-5, warm_up_len=10, ramp_down_start=10,
                ramp_down_len=65, last_lr_value=0.01, resample_rate=32000, window_size=800, hop_size=320, n_fft=1024,
                n_mels=128, freqm=0, timem=0, fmin=0, fmax=None, fmin_aug_range=10, fmax_aug_range=2000)
    assert {k: getattr(a, k) for k in want} == want
    assert (a.train_bank, a.valid_bank, a.eval_bank, a.init_checkpoint, a.seed, a.no_graph, a.max_steps, a.precision, a.out,
            a.eval_dump, a.json, a.clip_seconds) == (None, None, "z", None, 0, False, 0, None, None, None, False, 10.0)
    for gone in ("cuda", "num_workers", "pretrained"):
        assert not hasattr(a, gone)
    a = parse_args(["--train", "--train_bank", "x", "--valid_bank", "y", "--variable_eval_length"])
    assert a.train and a.variable_eval_length and (a.train_bank, a.valid_bank) == ("x", "y")
    for argv in (["--eval_bank", "z", "--resample_rate", "16000"], ["--train", "--train_bank", "x"], []):
        with pytest.raises(SystemExit):
            parse_args(argv)


def test_library_exports_the_ragged_symbol():
    """(that the library exports what the header declares: tests/test_host_cpu.py, which names this symbol)"""
    from efficientat_amd import build
    assert "eat_wave_augment_ragged" in _lib.exported_symbols()
    assert "ragged.hip" in build.SOURCES


def test_hdf5_converter_round_trip(tmp_path):
    """tools/fsd50k_to_bank.py (QUARANTINED, never run where this package was built): a 3-clip HDF5 + mp3 file in the layout
    of FSD50K.*_mp3.hdf (bit-packed targets), converted and read back by fsd50k.load_bank.  Needs h5py and PyAV - skipped
    where they are missing, so a pass anywhere is the first execution of that tool."""
    h5py = pytest.importorskip("h5py")
    av = pytest.importorskip("av")
    sr, n = 32000, 3
    rng = np.random.default_rng(0)
    names, blobs = [], []
    for i in range(n):
        wave = (0.3 * np.sin(2 * np.pi * (300.0 + 200 * i) * np.arange((i + 1) * sr) / sr)).astype(np.float32)
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
        names.append(("%d" % (1000 * i)).encode())
    targets = (rng.random((n, 200)) < 0.1).astype(np.uint8)
    with h5py.File(tmp_path / "FSD50K.eval_mp3.hdf", "w") as f:
        f.create_dataset("audio_name", data=np.array(names))
        d = f.create_dataset("mp3", (n,), dtype=h5py.vlen_dtype(np.dtype("uint8")))
        for i, b in enumerate(blobs):
            d[i] = b
        f.create_dataset("target", data=np.packbits(targets, axis=-1))
    spec = importlib.util.spec_from_file_location("eat_fsd50k_to_bank", os.path.join(ROOT, "tools", "fsd50k_to_bank.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert tool.convert(str(tmp_path / "FSD50K.eval_mp3.hdf"), str(tmp_path / "bank")) == n
    bank = fsd50k.load_bank(str(tmp_path / "bank"))
    assert bank["names"] == [b.decode() for b in names]
    le = bank["lengths_cpu"].tolist()
    assert all(abs(le[i] - (i + 1) * sr) < 4000 for i in range(n))            # (mp3 framing pads a clip by a few frames)
    np.testing.assert_array_equal(bank["bank_y"].numpy(), targets.astype(np.float32))
    x = bank["waves"].numpy()
    assert 0.1 < np.abs(x[le[0]:le[0] + sr]).max() < 0.5
