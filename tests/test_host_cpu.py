"""CPU-side checks: the C-ABI library builds/loads and exports every declared symbol, and the host
logic of the drop-in mirrors (mel basis table, config math, state-dict layout, error behaviour)."""
import contextlib
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch

from efficientat_amd import _lib, build, utils
from efficientat_amd.mn import get_model, _mobilenet_v3_conf
from efficientat_amd.preprocess import AugmentMelSTFT, band_table, kaldi_mel_basis
from oracle import eat_oracle as O
from oracle import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


@pytest.fixture(scope="session")
def libpath():
    return build.build()


def test_library_exports_every_declared_symbol(libpath):
    header = open(os.path.join(ROOT, "include", "eat_hip.h")).read()
    declared = set(re.findall(r"\b(eat_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    import torch  # noqa: F401  (load order: see efficientat_amd/_lib.py)
    h = ctypes.CDLL(libpath)
    for name in sorted(declared):
        assert hasattr(h, name), f"{name} declared in include/eat_hip.h but not exported"
    assert declared == set(_lib.exported_symbols())
    assert h.eat_version() >= 100
    # the fine-tuning entry points (tests/test_openmic_cpu.py, tests/test_fsd50k_cpu.py) by name
    assert {"eat_masked_bce_fwd_bwd", "eat_openmic_targets", "eat_rank_metrics_masked", "eat_wave_augment_ragged"} <= declared


_VOCABULARY = {ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_longlong}


def test_ctypes_signatures_are_parsed_from_the_header(libpath):
    """_lib has no signature table of its own: argtypes / restype of every symbol come from include/eat_hip.h."""
    P, I, F, D, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_longlong
    with open(os.path.join(ROOT, "include", "eat_hip.h")) as f:
        protos = _lib.parse_prototypes(f.read())
    assert len(protos) == 139 and protos == _lib.PROTOTYPES
    assert _lib.SIGNATURES == {name: args for name, (_, args) in protos.items()}
    for name, (restype, args) in protos.items():
        assert set(args) <= _VOCABULARY and restype in (I, LL, ctypes.c_char_p), name
    assert os.path.realpath(_lib.LIB_PATH) == os.path.realpath(libpath)
    h = _lib.lib()
    for name, (restype, args) in protos.items():
        fn = getattr(h, name)
        assert list(fn.argtypes) == args and fn.restype is restype, name
    # order-sensitive literals, written from the header by hand: a parser that drops or swaps a parameter cannot agree
    assert protos["eat_adam_multi"] == (I, [P, I, P, D, P, F, D, D, D, D, I, D, P])
    assert protos["eat_wave_augment"] == (I, [P, P, P, LL, I, I, P, P, P, P, P, P, I, P])
    assert protos["eat_rank_metrics_ws_bytes"] == (LL, [I, I])
    assert protos["eat_last_error_string"] == (ctypes.c_char_p, [])
    assert protos["eat_version"] == (I, []) and protos["eat_pw_stream_mode"] == (I, [I])


@pytest.mark.parametrize("proto", [
    "int eat_x(const float* a, unsigned n, eat_stream_t stream);",      # parameter type outside the vocabulary
    "int eat_x(long n);",
    "int eat_x(size_t n);",
    "float eat_x(int n);",                                              # return type outside the vocabulary
    "char* eat_x(void);",
])
def test_header_parser_refuses_a_type_outside_its_vocabulary(proto):
    with pytest.raises(_lib.EatHipError, match="eat_x"):
        _lib.parse_prototypes("/* a header */\n#define EAT_OK 0\nint eat_fine(int a, long long b, const char* c);\n" + proto)
    assert _lib.parse_prototypes("int eat_fine(int a, long long, double* c);  // " + proto) == \
        {"eat_fine": (ctypes.c_int, [ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p])}


def test_mel_basis_is_bit_identical_to_oracle_and_banded():
    for fmin, fmax in [(0.0, 15000), (3, 14500), (9, 16000), (0.0, 14001)]:
        b = kaldi_mel_basis(128, 1024, 32000, fmin, fmax)
        ref = O.kaldi_mel_banks(128, 1024, 32000, fmin, float(fmax))
        assert torch.equal(b, ref[:, :512])                       # same fp32 values => same bin indices
        bw2, bs, cnt = band_table(b)
        pairs = bw2.shape[0]
        dense = torch.zeros_like(b)
        for m in range(128):
            dense[m, bs[m]:bs[m] + 2 * pairs] = bw2[:, m, :].reshape(-1)
            assert not bw2[int(cnt[m]):, m, :].any()             # the kernel stops after max(cnt) pairs per 64 rows
        assert torch.equal(dense, b)
        assert int(bs.max()) + 2 * pairs <= 512 and not (bs % 2).any() and int(cnt.max()) == pairs
    b = kaldi_mel_basis(128, 1024, 32000, 0.0, 15000)
    assert int((b != 0).sum()) == 948 and float(b[127, 480]) > 0


def test_mel_module_mirrors_reference_surface():
    m = _quiet(AugmentMelSTFT)
    assert m.fmax == 15000 and len(m.state_dict()) == 0
    assert m.window.shape == (800,) and m.preemphasis_coefficient.shape == (1, 1, 2)
    with pytest.raises(AssertionError):
        AugmentMelSTFT(fmin_aug_range=0, fmax=1)
    with pytest.raises(_lib.EatHipError):
        m.eval()(torch.zeros(1, 32000))          # CPU tensor: no fallback


def test_config_math():
    assert [utils.NAME_TO_WIDTH(n) for n in ("mn10_as", "mn40_as_ext(2)", "dymn20_as", "foo")] == [1.0, 4.0, 2.0, 1.0]
    for v in (8, 12, 17.6, 64 * 0.4, 960 * 4.0, 23):
        assert utils.make_divisible(v, 8) == O.make_divisible(v, 8)
    setting, last = _mobilenet_v3_conf(width_mult=1.0)
    assert last == 1280 and [c.out_channels for c in setting][-1] == 160
    ref, _ = O.block_table(2.0)
    got, _ = _mobilenet_v3_conf(width_mult=2.0)
    assert [(c.input_channels, c.expanded_channels, c.out_channels, c.kernel, c.stride) for c in got] == \
           [(r["cin"], r["cexp"], r["cout"], r["k"], r["stride"]) for r in ref]


@pytest.mark.parametrize("width,n_params", [(1.0, 4876831), (0.4, None), (4.0, 68427303)])
def test_state_dict_layout_matches_reference(width, n_params):
    model = _quiet(get_model, width_mult=width)
    shapes = synth.mn_shapes(width)
    sd = model.state_dict()
    assert list(sd.keys()) == list(shapes.keys())
    assert all(tuple(sd[k].shape) == tuple(v) for k, v in shapes.items())
    if n_params:
        assert sum(p.numel() for p in model.parameters()) == n_params


def test_error_behaviour_matches_reference():
    with pytest.raises(NotImplementedError):
        _quiet(get_model, pretrained_name="no_such_model")
    with pytest.raises(NotImplementedError):
        _quiet(get_model, head_type="bogus")
    with pytest.raises(AssertionError):
        _quiet(get_model, se_dims="x")
    with pytest.raises(ValueError):
        from efficientat_amd.mn import MN
        MN([], 1280)


@pytest.mark.parametrize("width,n_params", [(1.0, 10548479), (2.0, 39966143)])
def test_dymn_state_dict_layout_matches_reference(width, n_params):
    from efficientat_amd.dymn import get_model as get_dymn
    model = _quiet(get_dymn, width_mult=width)
    shapes = synth.dymn_shapes(width)
    sd = model.state_dict()
    assert list(sd.keys()) == list(shapes.keys())
    assert all(tuple(sd[k].shape) == tuple(v) for k, v in shapes.items())
    assert sum(p.numel() for p in model.parameters()) == n_params
    assert [b.context_dim for b in model.layers] == [O.context_dim(c["cexp"], width) for c in O.block_table(width)[0]]


def test_dymn_temperature_schedule_and_api():
    from efficientat_amd.dymn import DynamicConv, get_model as get_dymn
    m = _quiet(get_dymn, width_mult=0.4, T_max=30.0, T0_slope=1.0, T1_slope=0.02, T_min=1)
    convs = [c for c in m.modules() if isinstance(c, DynamicConv)]
    assert len(convs) == 44 and all(c.temperature == 30.0 for c in convs)
    for epoch in (0, 10, 29, 40, 200):
        _quiet(m.update_params, epoch)
        assert abs(convs[0].temperature - O.dyconv_temperature(epoch)) < 1e-9
    with pytest.raises(NotImplementedError):
        _quiet(get_dymn, use_dy_blocks="bogus")
    with pytest.raises(Exception):
        m.eval()(torch.zeros(1, 1, 128, 100))          # CPU tensor: no fallback


def test_synthetic_audioset_standin_matches_reference_tuple_layout(tmp_path, monkeypatch):
    """dropin/datasets/audioset.py: same public functions and item layout as the reference's datasets/audioset.py
    (:94-103 AddIndexDataset, :138-161 item = (waveform (1, 320000) f32, name, target (527,) f32))."""
    import importlib.util
    monkeypatch.setenv("EAT_SYNTH_AUDIOSET", "1")
    monkeypatch.setenv("EAT_SYNTH_AUDIOSET_TRAIN", "16")
    monkeypatch.setenv("EAT_SYNTH_AUDIOSET_TEST", "527")
    spec = importlib.util.spec_from_file_location("eat_synth_audioset", os.path.join(ROOT, "dropin", "datasets", "audioset.py"))
    ds = importlib.util.module_from_spec(spec)
    with contextlib.redirect_stdout(io.StringIO()):
        spec.loader.exec_module(ds)
        full, test = ds.get_full_training_set(), ds.get_test_set()
        sampler = ds.get_ft_weighted_sampler(epoch_len=24)
    assert len(full) == 64 and len(test) == 527 and len(list(sampler)) == 24
    x, name, y, idx = full[5]
    assert x.shape == (1, 320000) and x.dtype == np.float32 and y.shape == (527,) and y.dtype == np.float32 and idx == 5
    assert name == "syn0000005" and y.sum() >= 1 and np.abs(x).max() <= 1.0
    x2, _, y2, _ = full[5]
    assert np.array_equal(x, x2) and np.array_equal(y, y2)                 # deterministic per index
    xt, nt, yt = test[3]
    assert xt.shape == (1, 320000) and isinstance(nt, str) and len(test[3]) == 3
    ys = test.targets()
    assert ys.sum(0).min() >= 1 and (1 - ys).sum(0).min() >= 1             # per-class AP / ROC of `_test` are defined
    with contextlib.redirect_stdout(io.StringIO()):
        mixed = ds.get_training_set(roll=True, wavmix=True, gain_augment=3)
    xm, _, ym, _ = mixed[1]
    assert xm.shape == (1, 320000) and ym.shape == (527,)


def test_audioset_dropin_never_falls_back_to_synthetic_silently(tmp_path, monkeypatch):
    """Without EAT_SYNTH_AUDIOSET=1 the module behaves like the reference's (datasets/audioset.py:19-22): an assertion
    unless the AudioSet HDF5 files are really there - nobody trains or evaluates on synthetic noise by accident."""
    import importlib.util

    def load():
        spec = importlib.util.spec_from_file_location("eat_audioset_mode", os.path.join(ROOT, "dropin", "datasets", "audioset.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    monkeypatch.delenv("EAT_SYNTH_AUDIOSET", raising=False)
    monkeypatch.delenv("EAT_AUDIOSET_DIR", raising=False)
    with pytest.raises(AssertionError, match="EAT_SYNTH_AUDIOSET=1"):
        load()
    monkeypatch.setenv("EAT_AUDIOSET_DIR", str(tmp_path))
    with pytest.raises(AssertionError, match="not found"):
        load()
    for f in ("balanced_train_segments_mp3.hdf", "unbalanced_train_segments_mp3.hdf", "eval_segments_mp3.hdf"):
        (tmp_path / f).write_bytes(b"")
    mod = load()                                                        # real back-end selected (h5py is needed to open it)
    assert mod.SYNTHETIC is False and mod.AudioSetDataset.__name__ == "Hdf5AudioSet"        # (dropin/datasets/_hdf5_reader.py)
    assert mod.dataset_config["eval_hdf5"].endswith("eval_segments_mp3.hdf")


def test_audio_loader_resamples_like_librosa_load(tmp_path):
    """efficientat_amd.audio_io.load_audio = the `librosa.core.load(path, sr=32000, mono=True)` contract of
    inference.py:45: PCM decode, channel mean, 44.1 -> 32 kHz polyphase resampling."""
    from scipy.io import wavfile
    from efficientat_amd.audio_io import load_audio
    t = np.arange(44100) / 44100.0
    sig = 0.5 * np.sin(2 * np.pi * 1000.0 * t)
    wavfile.write(tmp_path / "a.wav", 44100, (np.stack([sig, sig], 1) * 32767).astype(np.int16))
    y, sr = load_audio(str(tmp_path / "a.wav"), sr=32000, mono=True)
    assert sr == 32000 and y.dtype == np.float32 and y.shape == (32000,)
    ref = 0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(32000) / 32000.0)
    assert np.abs(y[200:-200] - ref[200:-200]).max() < 2e-3                # away from the filter's edge transients
    y2, sr2 = load_audio(str(tmp_path / "a.wav"), sr=None, mono=False)
    assert sr2 == 44100 and y2.shape == (2, 44100)


def test_fused_expand_dw_eligibility_rule():
    """ops.expand_dw_eligible mirrors the geometry check of eat_expand_dw_bf16_fwd (csrc/expand_dw.hip): mn10's blocks
    8-12 at 10 s clips qualify, the 16x125 / 4x32-with-C_in-160 / strided / 5x5 blocks do not."""
    from efficientat_amd import ops
    assert ops._FUSE_EXPAND_DW                                 # (a constant since round 5)
    assert ops.expand_dw_eligible(80, 8, 63, 3, 1) and ops.expand_dw_eligible(112, 8, 63, 3, 1)
    assert ops.expand_dw_eligible(40, 4, 32, 3, 1)
    assert not ops.expand_dw_eligible(40, 16, 125, 5, 1)      # plane too large, 5x5
    assert not ops.expand_dw_eligible(112, 8, 63, 5, 2)       # stride 2
    assert not ops.expand_dw_eligible(160, 4, 32, 3, 1)       # five chunks of x fragments do not fit the registers
    assert not ops.expand_dw_eligible(80, 8, 63 + 2, 3, 1)    # wider than a wave
    assert not ops.expand_dw_eligible(80, 7, 9, 3, 1)         # 63 positions: not a multiple of 4


def test_mel_basis_matches_real_torchaudio_when_installed():
    """The kaldi mel basis is restated from torchaudio 0.13 (not importable in the build image).  Wherever the real
    library IS installed, the restatement must agree with it bit for bit (models/preprocess.py:52-53 call site)."""
    kaldi = pytest.importorskip("torchaudio.compliance.kaldi", reason="torchaudio not installed")
    if "ref_shims" in (getattr(kaldi, "__file__", "") or ""):
        pytest.skip("oracle/ref_shims stand-in on the path, not the real torchaudio")
    for fmin, fmax in [(0.0, 15000.0), (3.0, 14001.0), (9.0, 16000.0), (5.0, 15500.0)]:
        ref, _ = kaldi.get_mel_banks(128, 1024, 32000, fmin, fmax, 100.0, -500.0, 1.0)
        assert torch.equal(kaldi_mel_basis(128, 1024, 32000, fmin, fmax), ref)


def test_prepack_plan_builds_the_32_byte_records_the_kernel_reads():
    """ops.PrepackPlan (host side of eat_pw_prepack_multi): one 32-byte record {w, wp, Co, Ci, kind, trans} per matrix,
    pack kinds chosen as pw_prepack chooses them, destinations 256-byte aligned inside one buffer (no launch: CPU tensors)."""
    import numpy as np
    import torch
    from efficientat_amd import ops
    ws = [torch.randn(64, 16, 1, 1), torch.randn(24, 72, 1, 1), torch.randn(960, 160, 1, 1)]
    entries = []
    for i, w in enumerate(ws):
        entries += [((i, "n"), w, False), ((i, "t"), w, True)]
    with ops.precision("auto"):
        plan = ops.PrepackPlan(entries)
        assert not plan.stale()
    rec = plan.table.numpy().view([("w", "<u8"), ("wp", "<u8"), ("Co", "<i4"), ("Ci", "<i4"), ("kind", "<i4"), ("trans", "<i4")])
    assert plan.table.numel() == 32 * 6 and len(rec) == 6
    # (Co, Ci) as the GEMM sees them; 'auto': fp32 pack below 40 input channels, split bf16 pack from there on
    want = [(64, 16, 0, 0), (16, 64, 2, 1), (24, 72, 2, 0), (72, 24, 0, 1), (960, 160, 2, 0), (160, 960, 2, 1)]
    assert [(int(r["Co"]), int(r["Ci"]), int(r["kind"]), int(r["trans"])) for r in rec] == want
    base = plan.buf.data_ptr()
    for r, (key, w, _) in zip(rec, entries):
        assert int(r["w"]) == w.data_ptr() and (int(r["wp"]) - base) % 256 == 0
        v = plan.get(key)
        assert v.data_ptr() == int(r["wp"]) and v.dtype == (torch.float32 if int(r["kind"]) == 0 else torch.bfloat16)
        assert getattr(v, "_eat_split", False) == (int(r["kind"]) == 2)
    with ops.precision("fp32"):
        assert plan.stale()                                    # another arithmetic: the plan must be rebuilt


def test_rank_shard_sampler_partitions_the_epoch():
    """train_dp.RankShardSampler: every rank generates the same epoch list from the base sampler (seed + epoch) and takes
    its stride - disjoint shards of equal length whose union is the list (what Lightning's DistributedSamplerWrapper does
    with the reference's WeightedRandomSampler, ex_pl_audioset.py:265-293)."""
    from torch.utils.data import WeightedRandomSampler
    from efficientat_amd.train_dp import RankShardSampler
    w = torch.rand(101, generator=torch.Generator().manual_seed(0)) + 0.01
    world = 4
    shards = []
    for r in range(world):
        s = RankShardSampler(WeightedRandomSampler(w, num_samples=50, replacement=False), r, world, seed=3)
        s.set_epoch(2)
        shards.append(list(s))
        assert len(shards[-1]) == len(s) == 12
    one = RankShardSampler(WeightedRandomSampler(w, num_samples=50, replacement=False), 0, 1, seed=3)
    one.set_epoch(2)
    full = list(one)
    inter = [full[i] for i in range(48)]
    assert [shards[i % world][i // world] for i in range(48)] == inter
    other = RankShardSampler(WeightedRandomSampler(w, num_samples=50, replacement=False), 0, world, seed=3)
    other.set_epoch(3)
    assert list(other) != shards[0]


def test_lr_schedule_matches_the_reference_formula():
    """helpers/utils.py:35-66 (exp warm-up x linear ramp-down), the LambdaLR factor of ex_audioset.py:93-96."""
    from efficientat_amd.utils import exp_warmup_linear_down
    f = exp_warmup_linear_down(8, 95, 80, 0.01)
    def ref(e):
        up = 1.0 if e >= 8 else float(np.exp(-5.0 * (1.0 - np.clip(e, 0.5, 8) / 8) ** 2))
        down = 1.0 if e <= 80 else (0.01 if e - 80 >= 95 else 0.01 + 0.99 * (95 - e + 80) / 95)
        return up * down
    for e in (0, 1, 7, 8, 50, 80, 81, 120, 174, 175, 199):
        assert abs(f(e) - ref(e)) < 1e-12


def test_keep_state_puts_back_model_optimizer_and_extra_tensors():
    """graphs.keep_state (the captured trainers' warm-up steps run inside it): after two Adam steps in the block, parameters,
    BatchNorm running statistics and counters are bit-identical to before; optimizer state that existed before is back, state
    created inside is zero; FusedAdam-style `_counters` and the extra tensor are back; the fold cache is dropped."""
    from efficientat_amd.graphs import keep_state
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(8, 4), torch.nn.BatchNorm1d(4)).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-2)
    x = torch.randn(16, 8)
    model[0](x).square().sum().backward()               # Adam state for the Linear only (the BatchNorm has no gradient yet)
    opt.step()
    opt.zero_grad()
    opt._counters = {0: torch.tensor(3.0)}

    class _Cache:
        n = 0

        def invalidate(self):
            self.n += 1
    model._cache = _Cache()
    sums = torch.tensor([1.5, -2.25], dtype=torch.float64)
    lin, bn = list(model[0].parameters()), list(model[1].parameters())
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    st0 = {p: {n: t.clone() for n, t in opt.state[p].items()} for p in lin}
    assert all(p not in opt.state for p in bn)
    with keep_state(model, opt, sums):
        for _ in range(2):
            opt.zero_grad()
            model(x).square().sum().backward()
            opt.step()
            opt._counters[0] += 1
            opt._counters[1] = torch.tensor(7.0)
            sums += 1.0
        assert not torch.equal(model[0].weight, sd0["0.weight"]) and int(model[1].num_batches_tracked) == 2
    for k, v in model.state_dict().items():
        assert torch.equal(v, sd0[k]), k
    for p in lin:
        for n, t in opt.state[p].items():
            assert torch.equal(t, st0[p][n]), n
    for p in bn:
        assert opt.state[p] and all(not bool(t.any()) for t in opt.state[p].values())
    assert float(opt._counters[0]) == 3.0 and float(opt._counters[1]) == 0.0
    assert sums.tolist() == [1.5, -2.25]
    assert model._cache.n == 1


def test_band_table_with_fixed_pairs_is_the_same_basis():
    """preprocess.band_table(pairs=P): the fixed-shape table a captured step takes as an input buffer holds the same
    non-zeros as the tight one, for the corners and the widest point of the train-mode (fmin, fmax) draw space."""
    from efficientat_amd.preprocess import AugmentMelSTFT, band_table, kaldi_mel_basis
    with contextlib.redirect_stdout(io.StringIO()):
        mel = AugmentMelSTFT(freqm=0, timem=0)
    P = mel.max_band_pairs()
    def dense(t):
        w2, st, cnt = t
        d = torch.zeros(128, 512)
        for m in range(128):
            for j in range(int(cnt[m])):
                d[m, int(st[m]) + 2 * j: int(st[m]) + 2 * j + 2] = w2[j, m]
        return d
    for fmin, fmax in ((0, 15000), (0, 16000), (9, 14001), (0, 15688), (5, 15123)):
        basis = kaldi_mel_basis(128, 1024, 32000, fmin, fmax)
        tight, fixed = band_table(basis), band_table(basis, pairs=P)
        assert fixed[0].shape == (P, 128, 2) and tight[0].shape[0] <= P - 1
        assert torch.equal(dense(fixed), basis) and torch.equal(dense(tight), basis)
        assert bool((fixed[1] + 2 * P <= 512).all()) and bool((fixed[1] % 2 == 0).all())
    with pytest.raises(ValueError):
        band_table(basis, pairs=3)


def test_hdf5_reader_round_trip(tmp_path, monkeypatch):
    """dropin/datasets/_hdf5_reader.py (QUARANTINED: datasets/audioset.py:32-47,106-177 restated, never run where this
    package was built): a 3-clip HDF5 + mp3 file written here and read back through the public `datasets.audioset` API.
    Needs h5py and PyAV - skipped where they are missing, so a pass anywhere is the first execution of that file."""
    h5py = pytest.importorskip("h5py")
    av = pytest.importorskip("av")
    import importlib.util
    sr, n = 32000, 3
    rng = np.random.default_rng(0)
    names, blobs, targets = [], [], []
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
        names.append(("Yclip%d.mp3" % i).encode())
        y = (rng.random(527) < 0.01)
        y[i] = True
        targets.append(np.packbits(y))
    for fn in ("balanced_train_segments_mp3.hdf", "unbalanced_train_segments_mp3.hdf", "eval_segments_mp3.hdf"):
        with h5py.File(tmp_path / fn, "w") as f:
            f.create_dataset("audio_name", data=np.array(names))
            dt = h5py.vlen_dtype(np.dtype("uint8"))
            d = f.create_dataset("mp3", (n,), dtype=dt)
            for i, b in enumerate(blobs):
                d[i] = b
            f.create_dataset("target", data=np.stack(targets))
    monkeypatch.delenv("EAT_SYNTH_AUDIOSET", raising=False)
    monkeypatch.setenv("EAT_AUDIOSET_DIR", str(tmp_path))
    spec = importlib.util.spec_from_file_location("eat_audioset_real", os.path.join(ROOT, "dropin", "datasets", "audioset.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with contextlib.redirect_stdout(io.StringIO()):
        ds = mod.get_test_set()
    assert len(ds) == n
    x, name, y = ds[1]
    assert x.shape == (1, 10 * sr) and x.dtype == np.float32 and name == "clip1" and y.shape == (527,) and y[1] == 1.0
    assert 0.1 < np.abs(x[0, :2 * sr]).max() < 0.5 and np.abs(x[0, 3 * sr:]).max() == 0.0        # decoded tone, zero padding
    assert ds.targets().shape == (n, 527)


# ------------------------------------------------------------------ mel tables beyond the default geometry
def _default_fmax(sr):
    return sr // 2 - 1000


def _dense_from_table(table, nb=512):
    """The dense basis a band table stands for, from ALL its pairs (not only the cnt[m] the kernel must walk)."""
    w2, st, cnt = table
    P, n_mels, _ = w2.shape
    d = torch.zeros(n_mels, nb)
    for m in range(n_mels):
        d[m, int(st[m]):int(st[m]) + 2 * P] = w2[:, m, :].reshape(-1)
    return d


@pytest.mark.parametrize("sr", [16000, 32000, 44100])
@pytest.mark.parametrize("n_mels", [1, 8, 40, 63, 64, 65, 129, 256])
def test_band_table_round_trips_at_other_mel_counts_and_rates(n_mels, sr):
    """band_table -> dense is the identity (bit-equal) for tight and fixed-width tables, incl. all-zero mel rows."""
    basis = kaldi_mel_basis(n_mels, 1024, sr, 0.0, _default_fmax(sr))
    assert torch.equal(basis, O.kaldi_mel_banks(n_mels, 1024, sr, 0.0, float(_default_fmax(sr)))[:, :512])
    empty = ~(basis != 0).any(dim=1)
    if (n_mels, sr) == (256, 32000):
        assert int(empty.sum()) >= 1                              # 13 where this was written
    tight = band_table(basis)
    widest = tight[0].shape[0]
    assert int(tight[2].max()) == widest or not (basis != 0).any()
    for pairs in (None, min(256, widest + 3), 256):
        w2, st, cnt = table = band_table(basis, pairs=pairs)
        P = w2.shape[0]
        assert P == (widest if pairs is None else pairs) and w2.shape == (P, n_mels, 2)
        assert st.dtype == torch.int32 and cnt.dtype == torch.int32
        assert not (st % 2).any() and int(st.min()) >= 0 and int(st.max()) + 2 * P <= 512
        assert int(cnt.min()) >= 0 and int(cnt.max()) <= P
        assert torch.equal(cnt == 0, empty)
        for m in range(n_mels):
            assert not w2[int(cnt[m]):, m, :].any()               # the kernel stops after max(cnt) pairs per 64 rows
        assert torch.equal(_dense_from_table(table), basis)
    if widest > 1:
        with pytest.raises(ValueError):
            band_table(basis, pairs=widest - 1)


def test_band_table_round_trips_at_128_mels_44100():
    basis = kaldi_mel_basis(128, 1024, 44100, 0.0, 21050)
    assert int((~(basis != 0).any(dim=1)).sum()) >= 1             # 1 where this was written
    for pairs in (None, 16, 64):
        table = band_table(basis, pairs=pairs)
        assert torch.equal(_dense_from_table(table), basis) and int((table[2] == 0).sum()) >= 1


def _widest_pairs(basis):
    return band_table(basis)[0].shape[0]


# (n_mels, sr, module kwargs, widest band of the whole jitter space by brute force, one draw that has it, static P)
JITTER_SPACES = [
    (128, 32000, {}, 14, (0, 15952), 15),
    (40, 32000, {}, 39, (0, 15750), 40),
    (64, 32000, {}, 26, (0, 15876), 27),
    (128, 44100, {}, 15, (0, 21620), 16),
    (64, 16000, dict(fmax_aug_range=1000), 22, (0, 7938), 23),
]


@pytest.mark.parametrize("n_mels,sr,kw,worst,worst_at,P", JITTER_SPACES,
                         ids=[f"mels{c[0]}_sr{c[1]}" for c in JITTER_SPACES])
def test_max_band_pairs_bounds_the_jitter_space(n_mels, sr, kw, worst, worst_at, P):
    """A captured trainer stages band_table(..., pairs=max_band_pairs()) every step and raises mid-run if one draw needs
    more.  Sweep of the (fmin, fmax) draw space: every fmin, fmax with a stride of 8 (the full 20000-draw sweep, which
    gave the `worst` recorded above, takes ~10 s per space), plus the corners and the recorded widest draw.  `worst` is
    a record, not a bar: the last non-zero of a filter is an fp32 value next to zero whose sign the host's log decides,
    so the width at one draw can differ by a pair between hosts.  The bar is P."""
    mel = _quiet(AugmentMelSTFT, n_mels=n_mels, sr=sr, **kw)
    assert mel.max_band_pairs() == P and worst <= P
    hi = mel.fmax + mel.fmax_aug_range // 2
    lo = hi - mel.fmax_aug_range + 1
    fmins = range(int(mel.fmin), int(mel.fmin) + mel.fmin_aug_range)
    draws = {(a, b) for a in fmins for b in list(range(lo, hi + 1, 8)) + [lo, hi, mel.fmax]} | {worst_at}
    seen = max(_widest_pairs(kaldi_mel_basis(n_mels, 1024, sr, a, b)) for a, b in sorted(draws))
    assert P - 2 <= seen <= P, (seen, worst, P)          # P is the widest corner + 2
    # and the fixed-width table of the widest draw is the same basis
    basis = kaldi_mel_basis(n_mels, 1024, sr, *worst_at)
    assert torch.equal(_dense_from_table(band_table(basis, pairs=P)), basis)


def test_draw_computes_the_frame_count_the_kernel_demands():
    """For every geometry of tests/test_gpu_mel_geometry.py: the T that draw() hands to the time-mask draw is the T the
    entry point demands (1 + (L-1) // hop) and the number of frames the oracle's STFT yields, and both mask draws stay
    inside their axes.  Mask parameters are capped at the axis length, which is torchaudio's precondition for
    mask_along_axis (a larger one draws a negative start; the kernel then masks nothing, like torchaudio's compare)."""
    from tests import mel_cases as MC
    for _, cid, L, _, geom in MC.ALL:
        g = MC.full_geom(geom)
        T = MC.frames(L, g["hopsize"])
        ref = O.mel_forward(torch.zeros(1, L), **g)
        assert ref.shape == (1, g["n_mels"], T), cid
        mel = _quiet(AugmentMelSTFT, n_mels=g["n_mels"], sr=g["sr"], win_length=g["win_length"], hopsize=g["hopsize"],
                     fmin=g["fmin"], fmax=g["fmax"], freqm=min(48, g["n_mels"]), timem=min(192, T)).train()
        sizes = []
        real = mel._draw_mask
        mel._draw_mask = lambda param, size: (sizes.append((param, size)), real(param, size))[1]
        torch.manual_seed(len(cid))
        for _ in range(50):
            fmin, fmax, fmask, tmask = mel.draw(L)
            assert g["fmin"] <= fmin < g["fmin"] + 10 and g["fmax"] - 1000 < fmax <= g["fmax"] + 1000
            assert 0 <= fmask[0] <= fmask[1] <= g["n_mels"], (cid, fmask)
            assert 0 <= tmask[0] <= tmask[1] <= T, (cid, tmask)
        assert set(sizes) == {(mel.freqm, g["n_mels"]), (mel.timem, T)}, cid
        assert mel.eval().draw(L) == (g["fmin"], g["fmax"], (0, 0), (0, 0))


@pytest.mark.parametrize("C", [1, 7, 960, 65535])
@pytest.mark.parametrize("B", [1, 68, 69, 70, 300])
def test_plane_chunks_partition_the_batch_within_one_launch(B, C):
    """ops._plane_chunks: the batch ranges of the dilated depthwise launchers are disjoint, in order, cover [0, B) and hold at
    most 65535 (sample, channel) planes each - the y dimension of one launch grid."""
    from efficientat_amd import ops
    chunks = ops._plane_chunks(B, C)
    assert chunks[0][0] == 0 and chunks[-1][1] == B
    for (a0, a1), (b0, _) in zip(chunks, chunks[1:]):
        assert a1 == b0                                           # in order, no gap, no overlap
    for b0, b1 in chunks:
        assert b0 < b1 and (b1 - b0) * C <= 65535
    assert len(chunks) == -(-B // (65535 // C))                   # and no more launches than that takes


@pytest.mark.parametrize("C", [65536, 100000, 0])
def test_plane_chunks_refuse_a_sample_wider_than_one_launch(C):
    from efficientat_amd import ops
    with pytest.raises(_lib.EatHipError, match="channels"):
        ops._plane_chunks(4, C)
