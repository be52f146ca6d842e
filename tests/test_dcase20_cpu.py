"""Host logic of the DCASE20 path (efficientat_amd/dcase20.py, tools/dcase20_to_bank.py, finetune_dcase20.parse_args): the
draw orders against their restatements, the meta reader, the bank round trip and the argument table.  No GPU."""
import importlib.util
import json
import os
import wave

import numpy as np
import pytest
import torch

from efficientat_amd import dcase20, esc50
from efficientat_amd.audio_io import load_audio
from efficientat_amd.finetune_dcase20 import parse_args
from tests.dcase20_ref import nested_dataset_draws

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, *path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def dropin_utils(tmp_path_factory):
    """dropin/helpers/utils.py reads ./metadata/class_labels_indices.csv at import, like the reference's."""
    d = tmp_path_factory.mktemp("cwd")
    os.makedirs(d / "metadata")
    (d / "metadata" / "class_labels_indices.csv").write_text("index,mid,display_name\n0,/m/0,Speech\n")
    cwd = os.getcwd()
    os.chdir(d)
    try:
        return _load("eat_dropin_helpers_utils", "dropin", "helpers", "utils.py")
    finally:
        os.chdir(cwd)


def _states():
    return torch.get_rng_state(), np.random.get_state()


def _same_states(a, b):
    return (torch.equal(a[0], b[0]) and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:])


def test_draw_mixstyle_makes_the_draws_of_the_dropin_mixstyle(dropin_utils):
    B, p, alpha = 6, 0.5, 0.4
    x = torch.arange(B * 2 * 3 * 5, dtype=torch.float32).reshape(B, 2, 3, 5).sin()
    seen = set()
    for seed in range(12):
        torch.manual_seed(seed); np.random.seed(seed)
        start = _states()
        res = dropin_utils.mixstyle(x, p, alpha, mix_labels=True)
        after_ref = _states()
        torch.manual_seed(seed); np.random.seed(seed)
        on, perm, lam = dcase20.draw_mixstyle(B, p, alpha)
        assert _same_states(_states(), after_ref), seed
        seen.add(on)
        if on:
            _, rperm, rlam = res
            assert torch.equal(perm, rperm) and perm.dtype == torch.int64
            assert lam.shape == (B,) and lam.dtype == torch.float32 and torch.equal(lam, rlam.reshape(B))
        else:
            assert res is x and perm is None and lam is None
            assert torch.equal(after_ref[0], start[0])                         # an unapplied step draws from numpy only
            assert not np.array_equal(after_ref[1][1], start[1][1]) or after_ref[1][2] != start[1][2]
    assert seen == {True, False}


@pytest.mark.parametrize("kw", [dict(), dict(gain_augment=0), dict(roll=False), dict(wavmix=False),
                                dict(gain_augment=0, roll=False), dict(gain_augment=6, shift_range=50, beta=1.0, rate=0.8)])
def test_draw_augment_follows_the_nested_datasets(kw):
    n_bank, batch = 7, [3, 0, 6, 6, 1, 2, 5, 4, 0, 3]
    mixed = set()
    for seed in (0, 1, 2):
        torch.manual_seed(seed); np.random.seed(seed)
        want = nested_dataset_draws(batch, n_bank, **kw)
        after = _states()
        torch.manual_seed(seed); np.random.seed(seed)
        idx, shift, amp, mix = dcase20.draw_augment(batch, n_bank, **kw)
        assert _same_states(_states(), after)
        assert idx.dtype == torch.int32 and shift.dtype == torch.int32 and amp.dtype == torch.float32
        assert idx.tolist() == want[0] and shift.tolist() == want[1]
        assert torch.equal(amp, torch.tensor(want[2], dtype=torch.float32))
        assert torch.equal(mix, torch.tensor(want[3], dtype=torch.float32))
        mixed |= set((idx[1::2] >= 0).tolist())
        assert (idx[0::2].tolist() == batch) and bool(((mix >= 0.5) & (mix <= 1.0)).all())
        if kw.get("gain_augment", 12) == 0:
            assert bool((amp == 1).all())
        if not kw.get("roll", True):
            assert not shift.any()
    assert mixed == ({False} if not kw.get("wavmix", True) else {True, False})


def test_draw_augment_is_not_esc50s_order():
    batch = list(range(8))
    torch.manual_seed(4); np.random.seed(4)
    ours = dcase20.draw_augment(batch, 7)
    torch.manual_seed(4); np.random.seed(4)
    theirs = esc50.draw_augment(batch, 7)
    assert any(not torch.equal(a, b) for a, b in zip(ours, theirs))            # (the coin after the clip, roll before gain)


# meta.csv rows: (filename, scene, identifier, device); label order is not sorted, the train split is not a prefix, and the
# city "vienna" appears in the test split only
META = [("audio/tram-lyon-1-a.wav", "tram", "lyon-1-10", "s2"),
        ("audio/airport-barcelona-0-a.wav", "airport", "barcelona-0-3", "a"),
        ("audio/park-vienna-7-b.wav", "park", "vienna-7-1", "b"),
        ("audio/bus-lyon-2-a.wav", "bus", "lyon-2-4", "a"),
        ("audio/airport-lyon-3-s1.wav", "airport", "lyon-3-9", "s1"),
        ("audio/park-barcelona-4-c.wav", "park", "barcelona-4-2", "c"),
        ("audio/tram-vienna-5-a.wav", "tram", "vienna-5-5", "a"),
        ("audio/bus-barcelona-6-b.wav", "bus", "barcelona-6-6", "b")]
TRAIN = [7, 1, 3, 4, 5]                                                        # (listed out of meta order on purpose)
TEST = [6, 2, 0]


def _write_meta(root):
    os.makedirs(os.path.join(root, "evaluation_setup"))
    os.makedirs(os.path.join(root, "audio"))
    with open(os.path.join(root, "meta.csv"), "w") as f:
        f.write("filename\tscene_label\tidentifier\tsource_label\n")
        for r in META:
            f.write("\t".join(r) + "\n")
    for name, rows in (("fold1_train.csv", TRAIN), ("fold1_evaluate.csv", TEST)):
        with open(os.path.join(root, "evaluation_setup", name), "w") as f:
            f.write("filename\tscene_label\n")
            for i in rows:
                f.write(f"{META[i][0]}\t{META[i][1]}\n")


def test_read_meta_and_split_rows(tmp_path):
    root = str(tmp_path / "tau")
    _write_meta(root)
    rows, enc = dcase20.read_meta(root)
    assert enc == {"scene": ["airport", "bus", "park", "tram"], "device": ["a", "b", "c", "s1", "s2"],
                   "city": ["barcelona", "lyon", "vienna"]}
    assert [r[0] for r in rows] == [m[0] for m in META]
    assert rows[0][1:] == (3, 4, 1) and rows[2][1:] == (2, 1, 2) and rows[4][1:] == (0, 3, 1)
    tr, enc_tr = dcase20.split_rows(root, True)
    te, enc_te = dcase20.split_rows(root, False)
    assert [r[0] for r in tr] == [META[i][0] for i in sorted(TRAIN)]            # meta order, not the split file's
    assert [r[0] for r in te] == [META[i][0] for i in sorted(TEST)]
    assert enc_tr == enc and enc_te == enc                                      # "vienna" keeps code 2 in the training split
    assert all(r[3] != 2 for r in tr) and [r[3] for r in te] == [1, 2, 2]
    assert dcase20.N_CLASSES == 10 and dcase20.CLIP_SECONDS == 10


def _write_wav(path, x, rate):
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.rint(np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def _write_audio(root):
    rng = np.random.default_rng(3)
    for i, m in enumerate(META):
        rate, n = 32000, 32000
        if i == 1:
            rate, n = 44100, 44100                                             # resampled on load
        if i == 3:
            n = 20000                                                          # a short file: padded with zeros
        t = np.arange(n) / rate
        _write_wav(os.path.join(root, m[0]), 0.4 * np.sin(2 * np.pi * (200 + 90 * i) * t) + 0.05 * rng.standard_normal(n), rate)


@pytest.mark.parametrize("float32", [False, True])
def test_converter_and_load_bank_round_trip(tmp_path, float32):
    root = str(tmp_path / "tau")
    _write_meta(root)
    _write_audio(root)
    tool = _load("eat_dcase20_to_bank", "tools", "dcase20_to_bank.py")
    L = 32000
    for split, want in (("train", sorted(TRAIN)), ("test", sorted(TEST))):
        out = str(tmp_path / f"bank_{split}")
        assert tool.convert(root, out, split=split, float32=float32, clip_seconds=1) == len(want)
        assert np.load(os.path.join(out, "waves.npy"), mmap_mode="r").dtype == (np.float32 if float32 else np.int16)
        bank = dcase20.load_bank(out)
        assert bank["bank"].shape == (len(want), L) and bank["bank"].dtype == torch.float32
        assert bank["names"] == [META[i][0] for i in want]
        assert bank["classes"] == {"scene": ["airport", "bus", "park", "tram"], "device": ["a", "b", "c", "s1", "s2"],
                                   "city": ["barcelona", "lyon", "vienna"]}
        rows, _ = dcase20.split_rows(root, split == "train")
        for k, col in (("bank_cls", 1), ("bank_dev", 2), ("bank_city", 3)):
            assert bank[k].dtype == torch.int32 and bank[k].tolist() == [r[col] for r in rows]
        for j, i in enumerate(want):
            x, _ = load_audio(os.path.join(root, META[i][0]), sr=32000, mono=True)
            ref = np.zeros(L, dtype=np.float32)
            ref[:min(L, len(x))] = x[:L]
            got = bank["bank"][j].numpy()
            if float32:
                assert np.array_equal(got, ref)
            else:                                                              # int16 on disk: half a step of 1 / 32767
                assert np.abs(got - np.clip(ref, -1, 1)).max() <= 0.5 / 32767 + 1e-7
            if i == 3:
                assert not got[20000:].any() and got[:20000].any()
            assert abs(float(bank["bank_mean"][j]) - got.astype(np.float64).mean()) < 1e-12
        assert bank["bank_mean"].dtype == torch.float64


def test_load_bank_rejects_malformed_banks(tmp_path):
    def bank(name, n=3, L=16, dtype=np.int16, labels=None, names=None, classes=None):
        d = str(tmp_path / name)
        os.makedirs(d)
        np.save(os.path.join(d, "waves.npy"), np.zeros((n, L), dtype=dtype))
        np.save(os.path.join(d, "labels.npy"), np.zeros((n, 3), dtype=np.int32) if labels is None else labels)
        with open(os.path.join(d, "names.txt"), "w") as f:
            f.write("".join(f"{k}\n" for k in (range(n) if names is None else names)))
        with open(os.path.join(d, "classes.json"), "w") as f:
            json.dump(dict(scene=["a", "b"], device=["a"], city=["x", "y"]) if classes is None else classes, f)
        return d

    assert dcase20.load_bank(bank("good"))["bank"].shape == (3, 16)
    lab = np.zeros((3, 3), dtype=np.int32)
    for name, kw in [("fewer_labels", dict(labels=np.zeros((2, 3), dtype=np.int32))),
                     ("fewer_names", dict(names=["a", "b"])),
                     ("empty", dict(n=0)),
                     ("two_columns", dict(labels=np.zeros((3, 2), dtype=np.int32))),
                     ("float_labels", dict(labels=np.zeros((3, 3), dtype=np.float32))),
                     ("scene_outside", dict(labels=lab + np.array([2, 0, 0], dtype=np.int32))),
                     ("device_outside", dict(labels=lab + np.array([0, 1, 0], dtype=np.int32))),
                     ("city_negative", dict(labels=lab - np.array([0, 0, 1], dtype=np.int32))),
                     ("no_city_list", dict(classes=dict(scene=["a"], device=["a"]))),
                     ("eleven_scenes", dict(classes=dict(scene=[str(k) for k in range(11)], device=["a"], city=["x"]))),
                     ("float64_waves", dict(dtype=np.float64))]:
        with pytest.raises(ValueError):
            dcase20.load_bank(bank(name, **kw))


def test_argument_defaults_are_ex_dcase20s():
    a = parse_args(["--train_bank", "tr", "--test_bank", "te"])
    table = dict(experiment_name="DCASE20", batch_size=64, model_name="mn10_as", pretrain_final_temp=1.0, model_width=1.0,
                 head_type="mlp", se_dims="c", n_epochs=80, mixup_alpha=0.3, mixstyle_p=0.0, mixstyle_alpha=0.4, no_roll=False,
                 no_wavmix=False, gain_augment=12, weight_decay=0.0, lr=8e-4, warm_up_len=10, ramp_down_start=10,
                 ramp_down_len=65, last_lr_value=0.01, resample_rate=32000, window_size=800, hop_size=320, n_fft=1024,
                 n_mels=128, freqm=0, timem=0, fmin=0, fmax=None, fmin_aug_range=10, fmax_aug_range=2000)
    for k, v in table.items():
        assert getattr(a, k) == v and type(getattr(a, k)) is type(v), k
    assert (a.train_bank, a.test_bank) == ("tr", "te")
    assert (a.init_checkpoint, a.seed, a.no_graph, a.max_steps, a.precision, a.out, a.eval_dump, a.json) == \
           (None, 0, False, 0, None, None, None, False)
    for dropped in ("cuda", "num_workers", "pretrained", "cache_path"):
        assert not hasattr(a, dropped)
    with pytest.raises(SystemExit):
        parse_args([])
