"""The long-recording tagger (efficientat_amd/tagger.py) end to end.

1. Against the CPU oracle (O.mel_forward + O.mn_forward per materialised window, calibrated synthetic mn10 weights): 137600
   samples, window 1.0 s, hop 0.75 s -> 6 windows of 128 x 100 frames, the last with 17600 valid samples.  The oracle's logits
   of any two windows differ by at least 0.5 in some class, so a tagger that mixes up windows cannot pass; the gap between
   ranked probabilities goes down to 4e-5, so indices are NOT compared with the oracle's.  Bars: probs within 1e-3 of the
   oracle's sigmoid (the project's logit bar; sigmoid only contracts it), prob[:, r] within 1e-3 of the oracle's r-th
   largest, the oracle's probability at index[:, r] within 1e-3 of prob[:, r].
2. Chunking and ordering, exact: a stub model whose logits are a fixed slice of its input, two recordings of different
   length (9 windows) with batch_windows=4, bit for bit against the materialised path.
3. tag_audio_window on a 44.1 kHz stereo int16 WAV: the reference's output format, the device-resampled waveform against
   `audio_io.load_audio` within the resampler's bar (tests/test_gpu_tagger_kernels.py), and the --json command line.
"""
import contextlib
import io
import json

import numpy as np
import pytest
import torch
from scipy.io import wavfile
from scipy.signal import resample_poly

from oracle import eat_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import audio_io, ops, tag, tagger  # noqa: E402
from efficientat_amd.mn import get_model  # noqa: E402

DEV = torch.device("cuda:0")
SR = 32000
N_SAMPLES, WIN_S, HOP_S = 137600, 1.0, 0.75

_ORACLE = {}


def _materialise(rec, starts, valids, W):
    x = torch.zeros((len(starts), W))
    for r, (s, v) in enumerate(zip(starts, valids)):
        x[r, :int(v)] = rec[int(s):int(s) + int(v)]
    return x


def _oracle():
    """The recording, the calibrated weights and the oracle's probabilities (6, 527), computed once."""
    if not _ORACLE:
        rec = synth.parity_clips(SR, seed=7).reshape(-1)[:N_SAMPLES].contiguous()
        starts, valids, W = tagger.window_plan(N_SAMPLES, WIN_S, HOP_S, SR)
        assert len(starts) == 6 and int(valids[-1]) == 17600 and W == SR
        x = O.mel_forward(_materialise(rec, starts, valids, W)).unsqueeze(1)
        assert x.shape == (6, 1, 128, 100)
        sd = synth.calibrate(synth.synth_state(synth.mn_shapes(1.0), seed=0), O.mn_forward, x)
        with torch.no_grad():
            logits, _ = O.mn_forward(sd, x)
        d = (logits[:, None, :] - logits[None, :, :]).abs().amax(dim=2) + 10.0 * torch.eye(6)
        assert float(d.min()) >= 0.5, float(d.min())                 # no two windows look alike
        with contextlib.redirect_stdout(io.StringIO()):
            model = get_model(width_mult=1.0)
        model.load_state_dict(sd)
        _ORACLE.update(rec=rec, sd=sd, p=torch.sigmoid(logits.double()).numpy(), starts=starts, W=W, model=model)
    return _ORACLE


@pytest.mark.parametrize("batch_windows", [4, 64])
def test_tagger_matches_the_cpu_oracle(batch_windows):
    o = _oracle()
    t = tagger.EATagger(model=o["model"], batch_windows=batch_windows)
    (r,) = t.tag_waveforms([o["rec"]], window_size=WIN_S, hop_length=HOP_S, return_probs=True)
    p = o["p"]
    assert r["probs"].shape == (6, 527) and r["index"].shape == (6, 10) and r["prob"].shape == (6, 10)
    assert np.array_equal(r["start"], o["starts"] / SR) and np.array_equal(r["end"], (o["starts"] + o["W"]) / SR)
    e_all = float(np.abs(r["probs"] - p).max())
    ranked = -np.sort(-p, axis=1)[:, :10]
    e_rank = float(np.abs(r["prob"] - ranked).max())
    e_at = float(np.abs(np.take_along_axis(p, r["index"].astype(np.int64), axis=1) - r["prob"]).max())
    print(f"TAGGER oracle batch_windows={batch_windows}: probs {e_all:.3e} ranked {e_rank:.3e} at-index {e_at:.3e}")
    assert e_all <= 1e-3 and e_rank <= 1e-3 and e_at <= 1e-3
    assert bool((np.diff(r["prob"], axis=1) <= 0).all())
    assert np.array_equal(np.take_along_axis(r["probs"], r["index"].astype(np.int64), axis=1), r["prob"])


class _SliceModel(torch.nn.Module):
    """logits = 50 fixed cells of the input spectrogram: independent of the batch a window runs in."""

    def forward(self, x):
        return x[:, 0, 5:55, 7].contiguous() * 4.0 - 2.0, None


def test_chunking_and_ordering_are_exact():
    win_s, hop_s = 0.3, 0.25                                        # W = 9600, H = 8000
    clips = synth.parity_clips(40000, seed=21)
    recs = [clips[0, :37001].contiguous(), clips[4, :30000].contiguous()]     # 5 + 4 windows; the second starts on an odd word
    t = tagger.EATagger(model=_SliceModel(), batch_windows=4, top_k=7)
    got = t.tag_waveforms(recs, window_size=win_s, hop_length=hop_s, return_probs=True)
    assert [len(r["start"]) for r in got] == [5, 4]
    one = tagger.EATagger(model=_SliceModel(), batch_windows=64, top_k=7)
    for rec, r, single in zip(recs, got, one.tag_waveforms(recs, window_size=win_s, hop_length=hop_s, return_probs=True)):
        starts, valids, W = tagger.window_plan(rec.numel(), win_s, hop_s, SR)
        assert W == 9600 and int(valids[-1]) < W
        with torch.no_grad():
            logits = _SliceModel()(t.mel(_materialise(rec, starts, valids, W).to(DEV)).unsqueeze(1))[0]
        prob, index, probs = (x.cpu().numpy() for x in ops.tag_topk(logits, 7, return_probs=True))
        assert np.array_equal(r["probs"], probs) and np.array_equal(r["index"], index) and np.array_equal(r["prob"], prob)
        assert np.array_equal(r["start"], starts / SR) and np.array_equal(r["end"], (starts + W) / SR)
        for key in ("probs", "index", "prob", "start", "end"):
            assert np.array_equal(single[key], r[key]), key
    assert not np.array_equal(got[0]["probs"][:4], got[1]["probs"])


def _write_wav(path, rate, n, channels, dtype, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / rate
    x = np.stack([0.3 * np.sin(2 * np.pi * (220.0 * (c + 1)) * t) + 0.05 * rng.standard_normal(n) for c in range(channels)], axis=1)
    data = np.clip(x * 32768.0, -32768, 32767).astype(np.int16) if dtype == np.int16 else x.astype(np.float32)
    wavfile.write(str(path), rate, data if channels > 1 else data[:, 0])
    return data


def test_tag_audio_window_on_a_44k_stereo_int16_file(tmp_path, capsys):
    o = _oracle()
    path = tmp_path / "stereo44.wav"
    data = _write_wav(path, 44100, 3 * 44100, 2, np.int16, seed=3)
    labels = [f"class{i}" for i in range(527)]
    t = tagger.EATagger(model=o["model"], labels=labels)

    # the device-resampled waveform against load_audio (scipy in float32) and against fp64
    wave = t.load_waveform(str(path))
    ref32, sr = audio_io.load_audio(str(path), sr=SR)
    exact = resample_poly((data.astype(np.float64) / 32768.0).mean(axis=1), 320, 441)
    assert sr == SR and wave.shape == (96000,) and ref32.shape == (96000,)
    e_hip = float(np.abs(wave.cpu().numpy().astype(np.float64) - exact).max())
    e_ref = float(np.abs(ref32.astype(np.float64) - exact).max())
    print(f"TAGGER load_waveform: e_hip={e_hip:.3e} e_ref32={e_ref:.3e}")
    assert e_hip <= 3.0 * e_ref + 1e-6

    # the reference's output format
    tags = t.tag_audio_window(str(path), window_size=WIN_S, hop_length=HOP_S)
    assert [w["start"] for w in tags] == [0.0, 0.75, 1.5, 2.25] and [w["end"] for w in tags] == [1.0, 1.75, 2.5, 3.25]
    for w in tags:
        assert sorted(w) == ["end", "start", "tags"] and len(w["tags"]) == 10
        assert all(sorted(x) == ["probability", "tag"] and x["tag"] in labels for x in w["tags"])
        ps = [float(x["probability"]) for x in w["tags"]]
        assert ps == sorted(ps, reverse=True) and 0.0 <= ps[-1] and ps[0] <= 1.0
    (r,) = t.tag_waveforms([wave], window_size=WIN_S, hop_length=HOP_S)
    assert [[labels.index(x["tag"]) for x in w["tags"]] for w in tags] == r["index"].tolist()
    unnamed = tagger.EATagger(model=o["model"]).tag_audio_window(str(path), WIN_S, HOP_S)
    assert unnamed[0]["tags"][0]["tag"] == int(r["index"][0, 0])   # labels=None: the class index is the name

    # the command line, --json with --checkpoint
    ckpt = tmp_path / "mn10.pt"
    torch.save(o["sd"], str(ckpt))
    capsys.readouterr()
    argv = ["--audio_path", str(path), "--checkpoint", str(ckpt), "--window_size", str(WIN_S), "--hop_length", str(HOP_S)]
    assert tag.main(argv + ["--json"]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    doc = json.loads(lines[0])
    assert doc["audio_path"] == str(path) and len(doc["windows"]) == 4
    assert [[x["tag"] for x in w["tags"]] for w in doc["windows"]] == r["index"].tolist()
    assert np.array_equal(np.array([[x["probability"] for x in w["tags"]] for w in doc["windows"]], dtype=np.float32), r["prob"])
    # and the reference's text output: "Window: a - b" and five tab-indented tags per window
    assert tag.main(argv) == 0
    text = capsys.readouterr().out
    assert text.count("Window: ") == 4 and "Window: 0.75 - 1.75" in text and text.count("\n\t") == 20


def test_load_waveform_at_the_target_rate(tmp_path):
    """Same-rate files: mono float32 goes through untouched (no launch); stereo int16 is dequantised and down-mixed,
    which is exact in fp32, so it equals load_audio to the bit."""
    t = tagger.EATagger(model=_SliceModel())
    mono = _write_wav(tmp_path / "mono32.wav", SR, 5000, 1, np.float32, seed=8)
    assert np.array_equal(t.load_waveform(str(tmp_path / "mono32.wav")).cpu().numpy(), mono[:, 0])
    _write_wav(tmp_path / "stereo32.wav", SR, 5001, 2, np.int16, seed=9)
    got = t.load_waveform(str(tmp_path / "stereo32.wav")).cpu().numpy()
    assert np.array_equal(got, audio_io.load_audio(str(tmp_path / "stereo32.wav"), sr=SR)[0])
