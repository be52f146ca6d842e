"""The embedding extractor (efficientat_amd/embeddings.py) end to end, on seeded random weights.

The yardstick is the model's own feature maps (`_forward_impl(mel, return_fmaps=True)`, pre-existing code): a scene
embedding must be their fp64 channel means, timestamp embeddings their fp64 segment means under the brute-force plan
(tests/embed_ref.py), both within the project's per-op bar 2e-5 mean|x| over the plane / the segment.  Two forwards of one
input agree to a few fp32 ulps at worst (the squeeze-excitation sums are atomic), three orders of magnitude below the bar.
Everything about windows, weights, timestamps, layer choice and the command line runs at clip_seconds = 1.0."""
import contextlib
import io

import numpy as np
import pytest
import torch
from scipy.io import wavfile

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import embed, embeddings  # noqa: E402
from efficientat_amd.dymn import get_model as get_dymn  # noqa: E402
from efficientat_amd.mn import get_model  # noqa: E402
from tests import embed_ref as R  # noqa: E402

DEV = torch.device("cuda:0")
SR, W1 = 32000, 32000
BAR = 2e-5
_CACHE = {}


def _model(name):
    if name not in _CACHE:
        torch.manual_seed(11)
        with contextlib.redirect_stdout(io.StringIO()):
            if name == "mn04":
                m, mels = get_model(width_mult=0.4), 128
            elif name == "mn04_64mel":
                m, mels = get_model(width_mult=0.4, input_dim_f=64), 64
            else:
                m, mels = get_dymn(width_mult=0.4), 128
        _CACHE[name] = (m.to(DEV).eval(), mels)
    return _CACHE[name]


def _waves(n, length, seed=3):
    g = torch.Generator().manual_seed(seed)
    return 0.1 * torch.randn((n, length), generator=g)


def _brute_plan(T_l):
    key = ("plan", tuple(T_l))
    if key not in _CACHE:
        _CACHE[key] = R.segment_plan_brute(1000, T_l, R.MN_STRIDES, 10.0, 50.0, 160.0)
    return _CACHE[key]


@pytest.mark.parametrize("name", ["mn04", "mn04_64mel", "dymn04"])
def test_embeddings_are_the_means_of_the_models_own_feature_maps(name):
    model, mels = _model(name)
    ex = embeddings.EmbeddingExtractor(model=model, n_mels=mels)
    waves = _waves(2, SR)
    padded = torch.zeros((2, ex.W))
    padded[:, :SR] = waves
    with torch.no_grad():
        spec = ex.mel(padded.to(DEV))
        maps = [m.double().cpu().numpy() for m in model._forward_impl(spec.unsqueeze(1), return_fmaps=True)[1]]
    assert len(maps) == 17 and spec.shape == (2, mels, 1000)
    D = sum(m.shape[1] for m in maps)
    assert ex.scene_embedding_size == D and ex.timestamp_embedding_size == D and ex.sample_rate == SR
    T_l = [m.shape[3] for m in maps]
    assert T_l == R.mn_widths(1000)
    assert all(float(np.abs(m).mean()) > 0 for m in maps)

    scene = ex.scene_embeddings(waves.to(DEV))
    assert scene.shape == (2, D) and scene.dtype == torch.float32 and scene.is_cuda
    ref = np.concatenate([m.mean(axis=(2, 3)) for m in maps], axis=1)
    scale = np.concatenate([np.abs(m).mean(axis=(2, 3)) for m in maps], axis=1)
    err = np.abs(scene.double().cpu().numpy() - ref)
    print(f"EMB {name} scene: max err / mean|x| = {float((err[scale > 0] / scale[scale > 0]).max()):.3e}")
    assert bool((err <= BAR * scale).all())

    lo, hi, t = _brute_plan(T_l)
    res = ex.timestamp_embeddings([w for w in waves])
    want, wscale = R.embed_pool_ref(maps, lo, hi), R.segment_abs_mean_ref(maps, lo, hi)
    assert len(res) == 2
    for b, (emb, t_ms) in enumerate(res):
        # one second of a ten-second window: frames 0..99, timestamps centred on frames 0, 5, .., 95
        assert emb.shape == (20, D) and emb.is_cuda and t_ms.dtype == np.float64 and np.array_equal(t_ms, t[:20])
        err = np.abs(emb.double().cpu().numpy() - want[b, :20])
        s = wscale[b, :20]
        print(f"EMB {name} timestamps[{b}]: max err / mean|x| = {float((err[s > 0] / s[s > 0]).max()):.3e}")
        assert bool((err <= BAR * s).all())


def _same(got, want):
    """Two runs of one computation (another batch composition, another process of the command line): each forward may differ
    by fp32 ulps of the activations' magnitude, and a channel mean can be small against that magnitude by cancellation
    (the linear project convs), so the bar is taken against |want| plus the mean |want| of the whole vector."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool((np.abs(got - want) <= BAR * (np.abs(want) + np.abs(want).mean())).all())


def _one_second_extractor(**kw):
    model, mels = _model("mn04")
    return embeddings.EmbeddingExtractor(model=model, n_mels=mels, clip_seconds=1.0, **kw)


LENGTHS = [5000, 32000, 32001, 70007]


def _recordings():
    return [_waves(1, n, seed=n)[0] for n in LENGTHS]


@pytest.mark.parametrize("batch_windows", [64, 2])
def test_scene_embedding_of_recordings_is_the_weighted_mean_of_their_windows(batch_windows):
    ex = _one_second_extractor(batch_windows=batch_windows)
    recs = _recordings()
    got = ex.scene_embeddings(recs).double().cpu().numpy()
    assert got.shape == (4, ex.scene_embedding_size)
    counts, weights = embeddings.window_weights(LENGTHS, W1)
    assert counts == [1, 1, 2, 3]
    row = 0
    for i, (rec, c) in enumerate(zip(recs, counts)):
        per_window = [ex.scene_embeddings([rec[q * W1:(q + 1) * W1]]).double().cpu().numpy()[0] for q in range(c)]
        hand = sum(w * e for w, e in zip(weights[row:row + c], per_window))
        err = np.abs(got[i] - hand)
        print(f"EMB weighted mean, {LENGTHS[i]} samples: max err {float(err.max()):.3e}, mean |e| {float(np.abs(hand).mean()):.3e}")
        assert _same(got[i], hand)
        row += c
    assert float(np.abs(got[2] - got[1]).max()) > 0                   # the one-sample window counts for something


def test_timestamp_counts_offsets_and_window_boundaries():
    ex = _one_second_extractor()
    recs = _recordings()
    res = ex.timestamp_embeddings(recs, hop_ms=50.0, width_ms=160.0)
    full = np.arange(20) * 50.0
    want_t = [full[:4],                                               # 5000 samples: 16 frames, centres 0, 5, 10, 15
              full,
              np.concatenate((full, [1000.0])),                       # a second window of one sample: its frame 0 alone
              np.concatenate((full, 1000.0 + full, 2000.0 + full[:4]))]          # 6007 samples left: 19 frames
    for (emb, t_ms), want in zip(res, want_t):
        assert np.array_equal(t_ms, want) and emb.shape == (len(want), ex.timestamp_embedding_size)
    # pooling does not cross window boundaries: the second window of the long recording, on its own
    alone, t_alone = ex.timestamp_embeddings([recs[3][W1:2 * W1]])[0]
    assert np.array_equal(t_alone, full)
    assert _same(res[3][0][20:40].cpu().numpy(), alone.cpu().numpy())
    with pytest.raises(ValueError, match="must be a multiple of hop_ms"):
        ex.timestamp_embeddings(recs[:1], hop_ms=30.0)


def test_layer_choice():
    ex_all, ex_two = _one_second_extractor(), _one_second_extractor(layers=[0, 16])
    model, _ = _model("mn04")
    c0, c16 = model.features[0][0].out_channels, model.features[-1].out_channels
    D = ex_all.scene_embedding_size
    assert ex_two.scene_embedding_size == c0 + c16 == ex_two.timestamp_embedding_size
    recs = _recordings()[2:]
    a, b = ex_all.scene_embeddings(recs).cpu().numpy(), ex_two.scene_embeddings(recs).cpu().numpy()
    assert b.shape == (2, c0 + c16)
    assert _same(b, np.concatenate((a[:, :c0], a[:, D - c16:]), axis=1))
    ta, tb = ex_all.timestamp_embeddings(recs[:1])[0], ex_two.timestamp_embeddings(recs[:1])[0]
    assert np.array_equal(ta[1], tb[1])
    ta, tb = ta[0].cpu().numpy(), tb[0].cpu().numpy()
    assert _same(tb, np.concatenate((ta[:, :c0], ta[:, D - c16:]), axis=1))
    for bad in ([17], [-1], []):
        with pytest.raises(ValueError, match="layers must name feature maps"):
            _one_second_extractor(layers=bad)


def test_what_the_extractor_refuses():
    with contextlib.redirect_stdout(io.StringIO()):
        training = get_model(width_mult=0.4).to(DEV).train()
    with pytest.raises(ValueError, match="eval mode"):
        embeddings.EmbeddingExtractor(model=training)
    model, _ = _model("mn04")
    ex = embeddings.EmbeddingExtractor(model=model, clip_seconds=1.0)
    model.train()
    try:
        with pytest.raises(ValueError, match="eval mode"):
            ex.scene_embeddings(_waves(1, 1000))
    finally:
        model.eval()
    with pytest.raises(TypeError, match=r"_forward_impl\(x, return_fmaps=True\)"):
        embeddings.EmbeddingExtractor(model=torch.nn.Linear(4, 4))
    with pytest.raises(ValueError, match="provide a model name"):
        embeddings.EmbeddingExtractor()
    with pytest.raises(ValueError, match="empty recording"):
        ex.scene_embeddings([torch.zeros(0)])


def test_command_line_writes_what_the_api_returns(tmp_path, capsys):
    model, _ = _model("mn04")
    ckpt = str(tmp_path / "mn04.pt")
    torch.save(model.state_dict(), ckpt)
    paths = []
    for i, n in enumerate((48000, 20000)):
        pcm = (_waves(1, n, seed=40 + i)[0].clamp(-1, 1) * 32767).to(torch.int16).numpy()
        paths.append(str(tmp_path / f"clip{i}.wav"))
        wavfile.write(paths[-1], SR, pcm)
    ex = _one_second_extractor()
    waves = [ex.load_waveform(p) for p in paths]
    assert [int(w.numel()) for w in waves] == [48000, 20000]
    common = ["--audio_path", *paths, "--checkpoint", ckpt, "--width", "0.4", "--clip_seconds", "1.0"]

    out = str(tmp_path / "scene.npz")
    assert embed.main(common + ["--out", out]) == 0
    z = np.load(out)
    assert list(z["audio_path"]) == paths
    assert _same(z["scene"], ex.scene_embeddings(waves).cpu().numpy())

    out = str(tmp_path / "stamps.npz")
    assert embed.main(common + ["--out", out, "--timestamps", "--hop_ms", "100", "--width_ms", "200", "--json"]) == 0
    z = np.load(out)
    api = ex.timestamp_embeddings(waves, hop_ms=100.0, width_ms=200.0)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 2
    for i, (emb, t_ms) in enumerate(api):
        assert np.array_equal(z[f"timestamps_ms_{i}"], t_ms) and len(t_ms) == (15, 7)[i]
        assert _same(z[f"emb_{i}"], emb.cpu().numpy())
