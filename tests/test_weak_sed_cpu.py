"""Weak-label SED without a GPU: the closed-form gradient of the fused loss against fp64 autograd, the bank loader with and
without strong.npy and its refusals, the converter with a weak table, the C header and its bindings with the argument checks
that return before anything touches the device, the evaluators' refusal of a weak bank, and the rules of `finetune_sed`."""
import ctypes
import filecmp
import importlib.util
import os

import numpy as np
import pytest
import torch

from efficientat_amd import _lib, build, finetune_sed, ops, sed
from efficientat_amd._lib import EatHipError
from tests import sed_ref as R
from tests import weak_sed_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("mix", [False, True], ids=["plain", "mixup"])
@pytest.mark.parametrize("shape", [(5, 3, 7), (1, 1, 1), (2, 3, 33)], ids=lambda s: "x".join(map(str, s)))
def test_closed_form_gradient_equals_autograd(shape, mix):
    """z in [-8, 8]: P stays inside (eps, 1 - eps), where autograd through the clamp and the straight-through rule coincide.
    Both are fp64 evaluations of one formula: 1e-12 relative leaves four digits of room above their round-off."""
    B, K, T = shape
    g = torch.Generator().manual_seed(B * 100 + T)
    z = (16.0 * torch.rand(B, K, T + 1, generator=g) - 8.0).numpy()
    y = (torch.rand(B, K, T + 1, generator=g) < 0.3).float().numpy()
    w = (torch.rand(B, K, generator=g) < 0.5).float().numpy()
    framed = (np.arange(B) % 2 == 0).astype(np.int32)
    perm = torch.randperm(B, generator=g).numpy() if mix else None
    lam = (0.5 + 0.5 * torch.rand(B, generator=g)).numpy() if mix else None
    for ww in (0.0, 0.5, 1.0):
        loss, lf, lc, dz, P = W.loss_autograd(z, y, w, framed, T, perm, lam, ww)
        c = W.loss_closed(z, y, w, framed, T, perm=perm, lam=lam, weak_weight=ww)
        assert float(P.min()) > 1e-7 and float(P.max()) < 1.0 - 1e-7
        assert c["loss"] == pytest.approx(loss, rel=1e-12) and c["frame"] == pytest.approx(lf, rel=1e-12)
        assert c["clip"] == pytest.approx(lc, rel=1e-12) and c["loss"] == pytest.approx(lf + ww * lc, rel=1e-12)
        err = np.linalg.norm(c["dl"] - dz) / max(np.linalg.norm(dz), 1e-300)
        assert err <= 1e-12, err
        np.testing.assert_allclose(c["P"], P, rtol=1e-13)


def test_closed_form_on_saturated_rows_is_finite_and_what_the_header_says():
    eps = float(np.float32(1e-7))
    for wv in (0.0, 1.0):
        hot = W.loss_closed(np.full((1, 1, 4), 40.0), np.zeros((1, 1, 4)), np.full((1, 1), wv), np.zeros(1, np.int32), 4)
        assert np.isfinite(hot["dl"]).all() and hot["P"][0, 0] == 1.0 and np.abs(hot["dl"]).max() <= 1.0 / eps
        assert hot["clip"] == pytest.approx(-(wv * np.log(1 - eps) + (1 - wv) * np.log(eps)), rel=1e-12)
        cold = W.loss_closed(np.full((1, 1, 4), -800.0), np.zeros((1, 1, 4)), np.full((1, 1), wv), np.zeros(1, np.int32), 4)
        assert not cold["dl"].any() and cold["P"][0, 0] == 0.0
        assert cold["clip"] == pytest.approx(-(wv * np.log(eps) + (1 - wv) * np.log1p(-eps)), rel=1e-12)


@pytest.mark.parametrize("case", R.target_cases()[:7], ids=lambda c: c["name"])
def test_brute_force_clip_targets_are_the_maximum_of_the_frame_targets(case):
    """Where the frames cover the window (T R >= L), an unmixed sample's clip target is the maximum of its frame targets."""
    ev, eo, lengths, K = case["events"], case["eo"], case["lengths"], case["K"]
    for name, strong in W.strong_vectors(len(lengths)).items():
        w, framed = W.clip_targets_brute(ev, eo, lengths, K, case["idx"], case["start"], case["mix"], case["L"], strong)
        y = R.targets_brute(*R.case_args(case))
        assert case["T"] * case["R"] >= case["L"]
        for b in range(len(case["mix"])):
            i0, i1 = int(case["idx"][2 * b]), int(case["idx"][2 * b + 1])
            if np.isnan(y[b, :, :case["T"]]).any():
                assert np.isnan(w[b]).all() and framed[b] == 0
                continue
            if i1 == -1:
                assert np.array_equal(w[b], y[b, :, :case["T"]].max(axis=1))
            want = all(strong is None or strong[i] != 0 for i in (i0, i1) if i != -1)
            assert framed[b] == int(want), (name, b)


# ---------------------------------------------------------------------------------------------------- bank loader
def _write_bank(path, strong=None, **over):
    n = np.asarray([50, 30, 20], dtype=np.int64)
    d = dict(waves=(np.arange(100) % 7).astype(np.float32) / 7, lengths=n,
             events=np.asarray([[0, 0, 10], [0, 5, 50], [2, 49, 50], [0, 0, 30], [1, 0, 30]], dtype=np.int32),
             event_offsets=np.asarray([0, 3, 5, 5], dtype=np.int64), names=["a", "b", "c"], classes=["x", "y", "z"])
    d.update(over)
    os.makedirs(path, exist_ok=True)
    for k in ("waves", "lengths", "events", "event_offsets"):
        np.save(os.path.join(path, k + ".npy"), d[k])
    for k in ("names", "classes"):
        with open(os.path.join(path, k + ".txt"), "w") as f:
            f.write("\n".join(d[k]) + "\n")
    if strong is not None:
        np.save(os.path.join(path, "strong.npy"), strong)
    return d


def test_bank_loader_with_and_without_the_strong_file(tmp_path):
    _write_bank(str(tmp_path / "plain"))
    bank = sed.load_bank(str(tmp_path / "plain"))
    assert bank["strong"].dtype == torch.uint8 and bank["strong"].tolist() == [1, 1, 1] and sed.n_weak(bank) == 0
    _write_bank(str(tmp_path / "weak"), strong=np.asarray([1, 0, 0], dtype=np.uint8))      # clip 2: weak, without tags
    bank = sed.load_bank(str(tmp_path / "weak"))
    assert bank["strong"].tolist() == [1, 0, 0] and sed.n_weak(bank) == 2
    assert bank["bank_y"].tolist() == [[1, 0, 1], [1, 1, 0], [0, 0, 0]]       # the whole-clip events keep bank_y right
    assert bank["events"].tolist()[3:] == [[0, 0, 30], [1, 0, 30]]


BAD_STRONG = [np.asarray([1, 0], dtype=np.uint8), np.asarray([[1, 0, 0]], dtype=np.uint8), np.asarray([1, 0, 0], dtype=np.int64),
              np.asarray([1.0, 0.0, 0.0], dtype=np.float32), np.asarray([1, 2, 0], dtype=np.uint8),
              np.asarray([0, 0, 1], dtype=np.uint8)]                          # the last: clip 0's events do not span it


@pytest.mark.parametrize("strong", BAD_STRONG, ids=range(len(BAD_STRONG)))
def test_bank_loader_refuses_a_bad_strong_file_naming_it(tmp_path, strong):
    _write_bank(str(tmp_path), strong=strong)
    with pytest.raises(ValueError, match=r"strong\.npy"):
        sed.load_bank(str(tmp_path))


def test_bank_loader_refuses_a_weak_clip_with_a_partial_event(tmp_path):
    ev = np.asarray([[0, 0, 10], [0, 5, 50], [2, 49, 50], [0, 0, 30], [1, 1, 30]], dtype=np.int32)
    _write_bank(str(tmp_path), strong=np.asarray([1, 0, 1], dtype=np.uint8), events=ev)
    with pytest.raises(ValueError, match=r"strong\.npy.*clip 1"):
        sed.load_bank(str(tmp_path))


# ---------------------------------------------------------------------------------------------------- converter
def _tool():
    spec = importlib.util.spec_from_file_location("strong_to_bank", os.path.join(ROOT, "tools", "strong_to_bank.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("header", [True, False])
def test_converter_round_trip_with_a_weak_table(tmp_path, header):
    from scipy.io import wavfile
    audio = tmp_path / "audio"
    audio.mkdir()
    rng = np.random.RandomState(0)
    for name, n in (("a.wav", 16000), ("b.wav", 24000), ("c.wav", 8000), ("d.wav", 12000)):
        wavfile.write(str(audio / name), 32000, (0.1 * rng.randn(n)).astype(np.float32))
    with open(tmp_path / "strong.tsv", "w") as f:
        if header:
            f.write("filename\tonset\toffset\tevent_label\n")
        f.write("a.wav\t0.1\t0.3\tdog\na.wav\t0.0\t0.2\tspeech\n")
    with open(tmp_path / "weak.tsv", "w") as f:
        if header:
            f.write("filename\tevent_labels\n")
        f.write("c.wav\tspeech,cat\nb.wav\tdog\n")
    tool = _tool()
    out = str(tmp_path / "bank")
    n, kept, dropped = tool.convert(str(audio), str(tmp_path / "strong.tsv"), out, float32=True,
                                    weak_table=str(tmp_path / "weak.tsv"))
    assert (n, kept, dropped) == (4, 5, 0)
    assert np.load(os.path.join(out, "strong.npy")).dtype == np.uint8
    assert np.load(os.path.join(out, "strong.npy")).tolist() == [1, 0, 0, 1]  # d.wav: in neither table, strong without events
    bank = sed.load_bank(out)
    assert bank["classes"] == ["cat", "dog", "speech"] and sed.n_weak(bank) == 2
    assert bank["event_offsets"].tolist() == [0, 2, 3, 5, 5]
    assert bank["events"].tolist() == [[1, 3200, 9600], [2, 0, 6400], [1, 0, 24000], [0, 0, 8000], [2, 0, 8000]]
    # a file in both tables, a weak file that is not there
    with open(tmp_path / "both.tsv", "w") as f:
        f.write("a.wav\tdog\n")
    with pytest.raises(ValueError, match="both tables"):
        tool.convert(str(audio), str(tmp_path / "strong.tsv"), str(tmp_path / "b2"), weak_table=str(tmp_path / "both.tsv"))
    with open(tmp_path / "stray.tsv", "w") as f:
        f.write("nofile.wav\tdog\n")
    with pytest.raises(ValueError, match="not in"):
        tool.convert(str(audio), str(tmp_path / "strong.tsv"), str(tmp_path / "b3"), weak_table=str(tmp_path / "stray.tsv"))
    # without a weak table: no strong.npy, and the files the strong-only converter writes, byte for byte
    plain, again = str(tmp_path / "plain"), str(tmp_path / "again")
    tool.convert(str(audio), str(tmp_path / "strong.tsv"), plain, float32=True)
    tool.convert(str(audio), str(tmp_path / "strong.tsv"), again, float32=True, weak_table=None)
    files = ["waves.npy", "lengths.npy", "events.npy", "event_offsets.npy", "names.txt", "classes.txt"]
    assert sorted(os.listdir(plain)) == sorted(files)
    assert filecmp.cmpfiles(plain, again, files, shallow=False)[0] == files
    assert np.load(os.path.join(plain, "events.npy")).tolist() == [[0, 3200, 9600], [1, 0, 6400]]
    assert np.load(os.path.join(plain, "event_offsets.npy")).tolist() == [0, 2, 2, 2, 2]
    # the strong clips of the mixed bank hold the waveforms and (up to the class index) the events of the strong-only one
    assert np.array_equal(np.load(os.path.join(plain, "waves.npy")), np.load(os.path.join(out, "waves.npy")))


# ---------------------------------------------------------------------------------------------------- header
def test_the_weak_sed_header_parses_is_disjoint_from_the_other_headers_and_is_bound():
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
    with open(os.path.join(ROOT, "include", "eat_weak_sed.h")) as f:
        protos = _lib.parse_prototypes(f.read())
    assert protos == _lib.WEAK_SED_PROTOTYPES
    assert set(protos) == {"eat_sed_clip_targets", "eat_weak_frame_bce_fwd_bwd"}
    assert protos["eat_sed_clip_targets"] == (I, [P, L, P, P, L, I, P, P, P, P, I, I, P, P, P])
    assert protos["eat_weak_frame_bce_fwd_bwd"] == (I, [P, P, P, P, P, P, F, F, I, I, I, I, I, P, P, P, P, P, P])
    others = [v for k, v in vars(_lib).items() if k.endswith("PROTOTYPES") and k != "WEAK_SED_PROTOTYPES"]
    assert len(others) >= 8
    for other in others:
        assert not set(protos) & set(other)
    assert "weak_sed.hip" in build.SOURCES and "sed.hip" in build.SOURCES
    build.build()
    for name, (restype, args) in protos.items():
        fn = getattr(_lib.lib(), name)
        assert list(fn.argtypes) == args and fn.restype is restype, name
    # argument checks that return before anything touches the device: `one` is never dereferenced
    one = ctypes.c_void_p(16)

    def targets(**kw):
        a = dict(events=one, n_events=1, eo=one, lengths=one, n_bank=1, K=1, idx=one, start=one, mix=one, strong=None, B=1, L=8,
                 w=one, framed=one)
        a.update(kw)
        _lib.call("eat_sed_clip_targets", *a.values(), None)

    for missing in ("events", "eo", "lengths", "idx", "start", "mix", "w", "framed"):
        with pytest.raises(EatHipError, match="eat_sed_clip_targets: missing operand"):
            targets(**{missing: None})
    for bad in (dict(B=0), dict(K=0), dict(L=0), dict(n_bank=0), dict(n_events=-1)):
        with pytest.raises(EatHipError, match="eat_sed_clip_targets: need B, K, L, n_bank >= 1"):
            targets(**bad)

    def loss(**kw):
        a = dict(z=one, y=one, w=one, framed=one, perm=None, lam=None, weak_weight=1.0, eps=1e-7, B=1, K=1, T=1, Tp=1, Kp=1,
                 sums=None, dl=one, dbias=None, clip_prob=None, ws=None)
        a.update(kw)
        _lib.call("eat_weak_frame_bce_fwd_bwd", *a.values(), None)

    for kw, msg in ((dict(z=None), "missing operand"), (dict(y=None), "missing operand"), (dict(w=None), "missing operand"),
                    (dict(framed=None), "missing operand"), (dict(perm=one), "perm and lam go together"),
                    (dict(lam=one), "perm and lam go together"), (dict(sums=one), "sums need the workspace"),
                    (dict(B=0), "need B, K, T >= 1"), (dict(K=0), "need B, K, T >= 1"), (dict(T=0), "need B, K, T >= 1"),
                    (dict(T=2), "Tp >= T"), (dict(K=2), "Kp >= K"), (dict(weak_weight=-0.5), "weak_weight must be finite"),
                    (dict(weak_weight=float("inf")), "weak_weight must be finite"),
                    (dict(weak_weight=float("nan")), "weak_weight must be finite"), (dict(eps=0.0), r"eps must lie in \(0, 0.5\)"),
                    (dict(eps=0.5), r"eps must lie in \(0, 0.5\)"), (dict(eps=-1e-7), r"eps must lie in \(0, 0.5\)"),
                    (dict(eps=float("nan")), r"eps must lie in \(0, 0.5\)")):
        with pytest.raises(EatHipError, match="eat_weak_frame_bce_fwd_bwd: .*" + msg):
            loss(**kw)


def test_ops_wrappers_refuse_bad_operands_from_metadata():
    z, w, fr = torch.zeros(2, 3, 4), torch.zeros(2, 3), torch.zeros(2, dtype=torch.int32)
    for kw, msg in ((dict(weak_weight=-1.0), "weak_weight"), (dict(eps=0.5), "eps"), (dict(T=5), "T <= Tp"),
                    (dict(w=torch.zeros(2, 4)), "w must be"), (dict(framed=fr.long()), "framed must be"),
                    (dict(perm=torch.zeros(2, dtype=torch.int32)), "perm and lam"),
                    (dict(clip_prob=torch.zeros(5)), "clip_prob must be"), (dict(sums=torch.zeros(2)), "sums must be")):
        a = dict(z=z, y=z, w=w, framed=fr, T=4)
        a.update(kw)
        with pytest.raises(EatHipError, match=msg):
            ops.weak_frame_bce_fwd_bwd(**a)
    with pytest.raises(EatHipError, match="GPU"):                             # well-formed CPU operands: no CPU path
        ops.weak_frame_bce_fwd_bwd(z, z, w, fr, 4)
    lengths = torch.tensor([100, 40])
    bank = dict(events=torch.zeros((0, 3), dtype=torch.int32), event_offsets=torch.zeros(3, dtype=torch.int64),
                lengths=lengths.int(), lengths_cpu=lengths, classes=["a"], strong=torch.ones(2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="crop start"):                      # CPU tables are validated before the upload
        ops.sed_clip_targets(bank, torch.tensor([0, -1], dtype=torch.int32), torch.tensor([37, 0], dtype=torch.int32),
                             torch.ones(1), 64)
    with pytest.raises(ValueError, match="bank index"):
        ops.sed_clip_targets(bank, torch.tensor([2, -1], dtype=torch.int32), torch.tensor([0, 0], dtype=torch.int32),
                             torch.ones(1), 64)


# ---------------------------------------------------------------------------------------------------- evaluators, program
def test_evaluators_refuse_a_weak_bank_before_using_the_model(tmp_path):
    _write_bank(str(tmp_path), strong=np.asarray([1, 0, 1], dtype=np.uint8))
    bank = sed.load_bank(str(tmp_path))
    for fn in (sed.evaluate_frames, sed.evaluate_events, sed.evaluate_psds):
        with pytest.raises(ValueError, match=r"strong\.npy"):
            fn(None, None, bank)


def test_finetune_sed_argument_rules(capsys):
    base = ["--train_bank", "a", "--valid_bank", "b"]
    args = finetune_sed.parse_args(base)
    assert args.weak_weight == 0.0
    assert finetune_sed.parse_args(base + ["--weak_weight", "0.5"]).weak_weight == 0.5
    for bad in ("-1", "inf", "nan"):
        with pytest.raises(SystemExit):
            finetune_sed.parse_args(base + ["--weak_weight", bad])
    finetune_sed.check_weak_banks(args, 0, 0)                                 # all strong, W = 0: today's path
    finetune_sed.check_weak_banks(finetune_sed.parse_args(base + ["--weak_weight", "1"]), 0, 0)
    finetune_sed.check_weak_banks(finetune_sed.parse_args(base + ["--weak_weight", "1"]), 4, 0)
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        finetune_sed.check_weak_banks(args, 4, 0)
    assert e.value.code == 2 and "--weak_weight" in capsys.readouterr().err   # the error says to set the flag
    with pytest.raises(SystemExit) as e:
        finetune_sed.check_weak_banks(finetune_sed.parse_args(base + ["--weak_weight", "1"]), 0, 2)
    assert e.value.code == 2 and "--valid_bank" in capsys.readouterr().err
