"""Strong-label SED without a GPU: the two reference rasterisers against each other, the bank loader's refusals, the
WAV + TSV converter, the draw tables, the C header and its bindings with the argument checks that return before anything
touches the device, and the scope of `forward_train_frames`."""
import contextlib
import ctypes
import importlib.util
import io
import os

import numpy as np
import pytest
import torch

from efficientat_amd import _lib, build, fsd50k, ops, sed
from efficientat_amd._lib import EatHipError
from efficientat_amd.mn_train import forward_train_frames
from tests import sed_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = R.target_cases()


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_reference_closed_form_equals_brute_force(case):
    brute, closed = R.targets_brute(*R.case_args(case)), R.targets_closed(*R.case_args(case))
    assert brute.dtype == np.float32 and brute.shape == (len(case["mix"]), case["K"], case["Tp"])
    assert np.array_equal(brute, closed, equal_nan=True)
    assert not brute[:, :, case["T"]:].any()                                  # pad columns are 0, NaN rows included


def test_reference_cases_hold_what_they_promise():
    """The properties the case list is chosen for, read off the brute-force result."""
    by = {c["name"]: R.targets_brute(*R.case_args(c)) for c in CASES}
    y = by["R8-L100-rows0"]
    assert y[0, 0, :4].tolist() == [0, 1, 0, 0]                               # (0, 8, 16): frame 1 only, frame 2 stays 0
    assert y[0, 1].sum() == 1 and y[0, 1, 4] == 1                             # the event of one sample (37 -> frame 4)
    assert y[0, 2, 1:7].all() and y[0, 2].sum() == 6                          # two overlapping events do not add up
    assert y[0, 3, 11:13].all() and y[0, :, 13].sum() == 0                    # partial frame 12, empty frame 13
    assert y[1, 0, :4].tolist() == [0, 1, 1, 0]                               # shift + 1: sample 16 is now active
    y = by["R8-L100-rows3"]
    assert y[2, 3, 0] == 1 and y[2, 3, 1] == 1 and y[2, 3, 12] == 0           # shift 10: (3, 95, 100) wraps to the front
    y = by["R8-L100-rows6"]
    assert y[0, :, 5:].sum() == 0                                             # clip 1 (40 samples): the padding stays 0 ...
    assert y[1, 0, 8] == 1 and y[1, 0, :8].sum() == 0 and y[1, 4, :2].all()          # ... and rolls with the clip (shift 70)
    assert y[2].max() == 0.5                                                  # mix 0.5
    y = by["R8-L100-rows9"]
    assert y[0, 1].sum() == 0 and y[0, 2].sum() > 0                           # (1, 0, 20) lies wholly outside the crop at 100
    assert np.float32(0.3) in y[1] or np.float32(1.0 - np.float64(np.float32(0.3))) in y[1]
    y = by["R8-L100-rows12"]
    assert y[0].sum() == 0                                                    # the clip without events
    y = by["R8-L100-rows15"]
    assert np.isnan(y[0, :, :14]).all() and np.isnan(y[1, :, :14]).all() and not np.isnan(y[2]).any()


# ---------------------------------------------------------------------------------------------------- bank loader
def _write_bank(path, **over):
    n = np.asarray([50, 30, 20], dtype=np.int64)
    d = dict(waves=(np.arange(100) % 7).astype(np.float32) / 7, lengths=n,
             events=np.asarray([[0, 0, 10], [0, 5, 50], [2, 49, 50], [1, 0, 30]], dtype=np.int32),
             event_offsets=np.asarray([0, 3, 4, 4], dtype=np.int64), names=["a", "b", "c"], classes=["x", "y", "z"])
    d.update(over)
    os.makedirs(path, exist_ok=True)
    for k in ("waves", "lengths", "events", "event_offsets"):
        np.save(os.path.join(path, k + ".npy"), d[k])
    for k in ("names", "classes"):
        with open(os.path.join(path, k + ".txt"), "w") as f:
            f.write("\n".join(d[k]) + ("\n" if d[k] else ""))
    return d


def test_bank_loader_returns_the_ragged_bank_with_weak_labels_and_events(tmp_path):
    d = _write_bank(str(tmp_path))
    bank = sed.load_bank(str(tmp_path))
    for key in ("waves", "offsets", "lengths", "clip_sum", "bank_y", "lengths_cpu", "names"):   # what wave_augment_ragged reads
        assert key in bank
    assert bank["offsets"].tolist() == [0, 50, 80] and bank["lengths"].dtype == torch.int32
    assert bank["bank_y"].tolist() == [[1, 0, 1], [0, 1, 0], [0, 0, 0]]       # weak: at least one event of the class
    assert bank["events"].dtype == torch.int32 and bank["events"].tolist() == d["events"].tolist()
    assert bank["event_offsets"].dtype == torch.int64 and bank["event_offsets"].tolist() == [0, 3, 4, 4]
    assert bank["classes"] == ["x", "y", "z"] and bank["names"] == ["a", "b", "c"]
    np.testing.assert_allclose(bank["clip_sum"].numpy(), [d["waves"][:50].astype(np.float64).sum(),
                                                          d["waves"][50:80].astype(np.float64).sum(),
                                                          d["waves"][80:].astype(np.float64).sum()], rtol=1e-12)
    i16 = _write_bank(str(tmp_path / "i16"), waves=np.arange(100, dtype=np.int16))
    assert sed.load_bank(str(tmp_path / "i16"))["waves"][5].item() == pytest.approx(i16["waves"][5] / 32767.0)


E3 = np.int32
BAD_BANKS = [
    ("waves.npy", dict(waves=np.zeros((10, 10), dtype=np.float32))),
    ("waves.npy", dict(waves=np.zeros(100, dtype=np.float64))),
    ("lengths.npy", dict(lengths=np.asarray([50.0, 30.0, 20.0]))),
    ("lengths.npy", dict(lengths=np.asarray([50, 30, 21], dtype=np.int64))),
    ("lengths.npy", dict(lengths=np.asarray([50, 50, 0], dtype=np.int64))),
    ("names.txt", dict(names=["a", "b"])),
    ("classes.txt", dict(classes=[])),
    ("classes.txt", dict(classes=["x", "x", "z"])),
    ("events.npy", dict(events=np.zeros((4, 3), dtype=np.int64))),
    ("events.npy", dict(events=np.zeros((4, 2), dtype=E3))),
    ("event_offsets.npy", dict(event_offsets=np.asarray([0, 3, 4], dtype=np.int64))),
    ("event_offsets.npy", dict(event_offsets=np.asarray([0, 3, 4, 4], dtype=np.int32))),
    ("event_offsets.npy", dict(event_offsets=np.asarray([1, 3, 4, 4], dtype=np.int64))),
    ("event_offsets.npy", dict(event_offsets=np.asarray([0, 3, 4, 3], dtype=np.int64))),
    ("event_offsets.npy", dict(event_offsets=np.asarray([0, 4, 3, 4], dtype=np.int64))),
    ("events.npy", dict(events=np.asarray([[0, 0, 10], [0, 5, 50], [3, 49, 50], [1, 0, 30]], dtype=E3))),      # class >= K
    ("events.npy", dict(events=np.asarray([[-1, 0, 10], [0, 5, 50], [2, 49, 50], [1, 0, 30]], dtype=E3))),
    ("events.npy", dict(events=np.asarray([[0, 0, 10], [0, 5, 51], [2, 49, 50], [1, 0, 30]], dtype=E3))),      # offset > length
    ("events.npy", dict(events=np.asarray([[0, 0, 10], [0, 5, 5], [2, 49, 50], [1, 0, 30]], dtype=E3))),       # empty
    ("events.npy", dict(events=np.asarray([[0, -1, 10], [0, 5, 50], [2, 49, 50], [1, 0, 30]], dtype=E3))),
    ("events.npy", dict(events=np.asarray([[0, 5, 50], [0, 0, 10], [2, 49, 50], [1, 0, 30]], dtype=E3))),      # onset order
    ("events.npy", dict(events=np.asarray([[2, 49, 50], [0, 0, 10], [0, 5, 50], [1, 0, 30]], dtype=E3))),      # class order
    ("events.npy", dict(events=np.asarray([[0, 0, 10], [0, 5, 50], [2, 49, 50], [1, 0, 31]], dtype=E3))),      # clip 1 is 30 long
]


@pytest.mark.parametrize("file,over", BAD_BANKS, ids=[f"{i}-{f}" for i, (f, _) in enumerate(BAD_BANKS)])
def test_bank_loader_refuses_every_format_violation_naming_the_file(tmp_path, file, over):
    _write_bank(str(tmp_path), **over)
    with pytest.raises(ValueError, match=file.replace(".", r"\.")):
        sed.load_bank(str(tmp_path))


# ---------------------------------------------------------------------------------------------------- converter
def _tool():
    spec = importlib.util.spec_from_file_location("strong_to_bank", os.path.join(ROOT, "tools", "strong_to_bank.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("header", [True, False])
def test_converter_round_trip(tmp_path, header):
    from scipy.io import wavfile
    audio = tmp_path / "audio"
    audio.mkdir()
    t441 = np.arange(44100 * 2) / 44100.0
    stereo = np.stack([np.sin(2 * np.pi * 440 * t441), 0.5 * np.sin(2 * np.pi * 220 * t441)], axis=1)
    wavfile.write(str(audio / "b_stereo.wav"), 44100, np.rint(stereo * 20000).astype(np.int16))       # 2 s, 44.1 kHz, int16
    mono = (0.25 * np.sin(2 * np.pi * 330 * np.arange(48000) / 32000.0)).astype(np.float32)
    wavfile.write(str(audio / "a_mono.wav"), 32000, mono)                                             # 1.5 s, 32 kHz, float
    wavfile.write(str(audio / "c_silent.wav"), 32000, np.zeros(16000, dtype=np.float32))              # no rows: no events
    rows = [("b_stereo.wav", 0.5, 1.25, "speech"), ("a_mono.wav", 0.10001, 0.2, "dog"), ("a_mono.wav", 1.0, 9.0, "speech"),
            ("a_mono.wav", 0.0, 0.05, "dog"), ("b_stereo.wav", 2.5, 3.0, "dog")]                       # the last: past the end
    with open(tmp_path / "ann.tsv", "w") as f:
        if header:
            f.write("filename\tonset\toffset\tevent_label\n")
        for r in rows:
            f.write("\t".join(str(v) for v in r) + "\n")
    out = str(tmp_path / "bank")
    n, kept, dropped = _tool().convert(str(audio), str(tmp_path / "ann.tsv"), out, float32=True)
    assert (n, kept, dropped) == (3, 4, 1)                                    # the event past the end is dropped and reported
    bank = sed.load_bank(out)
    assert bank["names"] == ["a_mono.wav", "b_stereo.wav", "c_silent.wav"] and bank["classes"] == ["dog", "speech"]
    assert bank["lengths_cpu"].tolist() == [48000, 64000, 16000]              # 2 s of 44.1 kHz -> 64000 samples at 32 kHz
    assert bank["event_offsets"].tolist() == [0, 3, 4, 4]
    # sorted by (class, onset); onset floored, offset ceiled and clipped to the clip
    assert bank["events"].tolist() == [[0, 0, 1600], [0, 3200, 6400], [1, 32000, 48000], [1, 16000, 40000]]
    np.testing.assert_array_equal(bank["waves"][:48000].numpy(), mono)
    from efficientat_amd.audio_io import load_audio
    ref, _ = load_audio(str(audio / "b_stereo.wav"), sr=32000, mono=True)
    np.testing.assert_array_equal(bank["waves"][48000:112000].numpy(), ref)
    # --classes fixes the order; int16 storage is the default
    with open(tmp_path / "classes.txt", "w") as f:
        f.write("speech\ncat\ndog\n")
    out2 = str(tmp_path / "bank2")
    _tool().convert(str(audio), str(tmp_path / "ann.tsv"), out2, classes_file=str(tmp_path / "classes.txt"))
    bank2 = sed.load_bank(out2)
    assert bank2["classes"] == ["speech", "cat", "dog"] and bank2["events"][:, 0].tolist() == [0, 2, 2, 0]
    assert np.load(os.path.join(out2, "waves.npy")).dtype == np.int16
    with open(tmp_path / "bad.tsv", "w") as f:
        f.write("nofile.wav\t0\t1\tdog\n")
    with pytest.raises(ValueError, match="not in"):
        _tool().convert(str(audio), str(tmp_path / "bad.tsv"), str(tmp_path / "bank3"))


# ---------------------------------------------------------------------------------------------------- draws
def test_draw_augment_is_the_fsd50k_draw():
    assert sed.draw_augment is fsd50k.draw_augment
    lengths = torch.tensor([5000, 400000, 32000, 700000])
    out = []
    for fn in (sed.draw_augment, fsd50k.draw_augment):
        torch.manual_seed(11)
        np.random.seed(12)
        out.append(fn([1, 3, 0, 2, 1], lengths, 327680))
    for a, b in zip(*out):
        assert torch.equal(a, b)
    ops.check_ragged_draws(*out[0][:3], lengths, 327680)


def test_host_side_table_checks():
    lengths = torch.tensor([100, 40])
    ok = (torch.tensor([0, -1, 1, 0], dtype=torch.int32), torch.tensor([99, 0, 39, 50], dtype=torch.int32))
    ops.check_eval_draws(*ok, lengths)                                        # 0 <= start < length is all evaluation needs
    with pytest.raises(ValueError, match="window start"):
        ops.check_eval_draws(ok[0], torch.tensor([100, 0, 0, 0], dtype=torch.int32), lengths)
    with pytest.raises(ValueError, match="bank index"):
        ops.check_eval_draws(torch.tensor([2, -1, 1, 0], dtype=torch.int32), ok[1], lengths)
    with pytest.raises(ValueError, match="2B values"):
        ops.check_eval_draws(ok[0][:3], ok[1][:3], lengths)
    # a training table with a crop start that pads the window is refused before anything is uploaded
    bank = dict(events=torch.zeros((0, 3), dtype=torch.int32), event_offsets=torch.zeros(3, dtype=torch.int64),
                lengths=lengths.int(), lengths_cpu=lengths, classes=["a"])
    with pytest.raises(ValueError, match="crop start"):
        ops.sed_targets(bank, torch.tensor([0, -1], dtype=torch.int32), torch.tensor([37, 0], dtype=torch.int32),
                        torch.zeros(2, dtype=torch.int32), torch.ones(1), 64, 8, 8)
    with pytest.raises(ValueError, match="window start"):
        ops.sed_targets(bank, torch.tensor([1, -1], dtype=torch.int32), torch.tensor([40, 0], dtype=torch.int32),
                        torch.zeros(2, dtype=torch.int32), torch.ones(1), 64, 8, 8, train=False)


# ---------------------------------------------------------------------------------------------------- header
def test_the_sed_header_parses_is_disjoint_from_the_other_headers_and_is_bound():
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    with open(os.path.join(ROOT, "include", "eat_sed.h")) as f:
        protos = _lib.parse_prototypes(f.read())
    assert protos == _lib.SED_PROTOTYPES
    assert set(protos) == {"eat_sed_targets", "eat_frame_bce_fwd_bwd", "eat_frame_grad_pad", "eat_frame_hidden_fwd",
                           "eat_frame_hidden_bwd"}
    assert protos["eat_sed_targets"] == (I, [P, L, P, P, L, I, P, P, P, P, I, I, I, I, I, P, P])
    assert protos["eat_frame_bce_fwd_bwd"] == (I, [P, P, P, P, P, P, I, I, I, I, I, P, P, P, P, P, P, P])
    assert protos["eat_frame_grad_pad"] == (I, [P, P, P, I, I, I, I, I, P])
    assert protos["eat_frame_hidden_fwd"] == (I, [P, P, P, I, I, I, P])
    assert protos["eat_frame_hidden_bwd"] == (I, [P, P, P, P, P, I, I, I, I, I, P])
    for other in (_lib.PROTOTYPES, _lib.TAG_PROTOTYPES, _lib.EMBED_PROTOTYPES, _lib.ATTN_PROTOTYPES, _lib.DETECT_PROTOTYPES):
        assert not set(protos) & set(other)
    assert "sed.hip" in build.SOURCES
    build.build()
    for name, (restype, args) in protos.items():
        fn = getattr(_lib.lib(), name)
        assert list(fn.argtypes) == args and fn.restype is restype, name
    # argument checks that return before anything touches the device: `one` is never dereferenced
    one, two = ctypes.c_void_p(16), ctypes.c_void_p(32)

    def targets(**kw):
        a = dict(events=one, n_events=1, eo=one, lengths=one, n_bank=1, K=1, idx=one, start=one, shift=one, mix=one, B=1, L=8,
                 R=8, T=1, Tp=1, y=one)
        a.update(kw)
        _lib.call("eat_sed_targets", *a.values(), None)

    for missing in ("events", "eo", "lengths", "idx", "start", "shift", "mix", "y"):
        with pytest.raises(EatHipError, match="eat_sed_targets: missing operand"):
            targets(**{missing: None})
    for bad in (dict(B=0), dict(K=0), dict(L=0), dict(R=0), dict(T=0), dict(n_bank=0), dict(T=5, Tp=4), dict(n_events=-1)):
        with pytest.raises(EatHipError, match="eat_sed_targets: need B, K, L, R, T, n_bank >= 1"):
            targets(**bad)

    def bce(**kw):
        a = dict(z=one, y=one, perm=None, lam=None, nframes=None, thr=None, B=1, K=1, T=1, Tp=1, Kp=1, sums=None, dl=one,
                 dbias=None, counts=None, rows=None, ws=None)
        a.update(kw)
        _lib.call("eat_frame_bce_fwd_bwd", *a.values(), None)

    for kw, msg in ((dict(z=None), "missing operand"), (dict(y=None), "missing operand"),
                    (dict(perm=one), "perm and lam go together"), (dict(lam=one), "perm and lam go together"),
                    (dict(counts=one), "counts need thr"), (dict(counts=one, thr=one, perm=one, lam=one), "perm given"),
                    (dict(sums=one), "sums need the workspace"), (dict(B=0), "need B, K, T >= 1"), (dict(K=0), "need B, K, T >= 1"),
                    (dict(T=0), "need B, K, T >= 1"), (dict(T=2), "Tp >= T"), (dict(K=2), "Kp >= K")):
        with pytest.raises(EatHipError, match="eat_frame_bce_fwd_bwd: .*" + msg):
            bce(**kw)
    for args, msg in (((None, two, None, 1, 1, 1, 1, 1), "missing operand"), ((one, None, None, 1, 1, 1, 1, 1), "missing operand"),
                      ((one, one, None, 1, 1, 1, 1, 1), "dl must not be g"), ((one, two, None, 0, 1, 1, 1, 1), "need B, K, T >= 1"),
                      ((one, two, None, 1, 2, 1, 1, 1), "Kp >= K"), ((one, two, None, 1, 1, 1, 2, 1), "Tp >= T")):
        with pytest.raises(EatHipError, match="eat_frame_grad_pad: .*" + msg):
            _lib.call("eat_frame_grad_pad", *args, None)
    for args, msg in (((None, None, one, 1, 1, 1), "missing operand"), ((one, None, None, 1, 1, 1), "missing operand"),
                      ((one, None, one, 0, 1, 1), "need B, Hp, Tp >= 1"), ((one, None, one, 1, 0, 1), "need B, Hp, Tp >= 1"),
                      ((one, None, one, 1, 1, 0), "need B, Hp, Tp >= 1")):
        with pytest.raises(EatHipError, match="eat_frame_hidden_fwd: " + msg):
            _lib.call("eat_frame_hidden_fwd", *args, None)
    for args, msg in (((None, one, None, one, None, 1, 1, 1, 1, 1), "missing operand"),
                      ((one, None, None, one, None, 1, 1, 1, 1, 1), "missing operand"),
                      ((one, one, None, None, None, 1, 1, 1, 1, 1), "missing operand"),
                      ((one, one, None, one, None, 0, 1, 1, 1, 1), "need B, H, T >= 1"),
                      ((one, one, None, one, None, 1, 2, 1, 1, 1), "Hp >= H"),
                      ((one, one, None, one, None, 1, 1, 1, 2, 1), "Tp >= T")):
        with pytest.raises(EatHipError, match="eat_frame_hidden_bwd: .*" + msg):
            _lib.call("eat_frame_hidden_bwd", *args, None)


# ---------------------------------------------------------------------------------------------------- scope
def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def test_forward_train_frames_refuses_what_it_does_not_cover():
    from efficientat_amd.dymn import get_model as get_dymn
    from efficientat_amd.mn import get_model
    x = torch.zeros(1, 1, 128, 96)
    with pytest.raises(ValueError, match="not an MN"):
        forward_train_frames(_quiet(get_dymn, width_mult=0.4), x)
    with pytest.raises(ValueError, match="modular plan"):
        forward_train_frames(_quiet(get_model, width_mult=0.4, se_dims="ct", input_dim_t=96), x)
    with pytest.raises(ValueError, match="BatchNorm whose train-mode statistics"):
        forward_train_frames(_quiet(get_model, width_mult=0.4, head_type="fully_convolutional"), x)
    with pytest.raises(ValueError, match="normalised over the whole clip"):
        forward_train_frames(_quiet(get_model, width_mult=0.4, head_type="multihead_attention_pooling"), x)
    with pytest.raises(ValueError, match="train mode"):
        forward_train_frames(_quiet(get_model, width_mult=0.4).eval(), x)
    with pytest.raises(ValueError, match="multiple of R"):
        sed.frame_geometry(_quiet(get_model, width_mult=0.4), type("M", (), {"hopsize": 320})(), 327680 + 320)
    assert sed.frame_geometry(_quiet(get_model, width_mult=0.4, num_classes=7), type("M", (), {"hopsize": 320})(),
                              327680) == (10240, 32, 7)
