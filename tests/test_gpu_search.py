"""Query-by-example search (efficientat_amd/retrieval.py, efficientat_amd/search.py) end to end, on the seeded
random-weight model of tests/test_gpu_embed.py and synthetic waveforms (noise and a tone, both by seed), at clip_seconds = 1.0.

The yardstick is the fp64 reference of tests/search_ref.py applied to the extractor's own embeddings, downloaded: scores
within the project's per-op bar 2e-5 and the ranking check that needs no index equality.  Two forwards of one input agree
to a few fp32 ulps only (the squeeze-excitation sums are atomic), so wherever two separate forwards are compared - an index
built by `from_recordings` or by the command line against the API - the bar is 2e-5 as well, never bit equality; one index
saved and loaded again must give the same bits."""
import contextlib
import io
import json

import numpy as np
import pytest
import torch
from scipy.io import wavfile

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, embeddings, retrieval, search  # noqa: E402
from efficientat_amd.mn import get_model  # noqa: E402
from tests import search_ref as R  # noqa: E402

DEV = torch.device("cuda:0")
SR = 32000
BAR = 2e-5
_CACHE = {}


def _model():
    if "model" not in _CACHE:
        torch.manual_seed(11)
        with contextlib.redirect_stdout(io.StringIO()):
            _CACHE["model"] = get_model(width_mult=0.4).to(DEV).eval()
    return _CACHE["model"]


def _extractor(**kw):
    return embeddings.EmbeddingExtractor(model=_model(), clip_seconds=1.0, **kw)


def _wave(n, seed):
    """Noise at a level, and a tone at a pitch, that depend on the seed: recordings that do not all sound alike."""
    noise = torch.randn(n, generator=torch.Generator().manual_seed(seed))
    tone = torch.sin(2.0 * np.pi * (150.0 * (1 + seed % 7)) * torch.arange(n, dtype=torch.float64) / SR).float()
    return 0.02 * (1 + seed % 5) * noise + 0.05 * (1 + seed % 3) * tone


LENGTHS = [20000, 32000, 40000, 32000, 12000, 50000]
NAMES = [f"rec{i}.wav" for i in range(6)]


def _recordings():
    recs = [_wave(n, seed=100 + i) for i, n in enumerate(LENGTHS)]
    recs[3] = recs[1].clone()                               # rec3 is rec1 again
    return recs


def _scene():
    """(extractor, embeddings (6, D) on the device, index built from exactly those embeddings), shared and left unchanged."""
    if "scene" not in _CACHE:
        ex = _extractor()
        emb = ex.scene_embeddings(_recordings())
        index = retrieval.EmbeddingIndex(ex.scene_embedding_size, device=DEV, meta={"layers": ex.layers, "clip_seconds": 1.0})
        for i, name in enumerate(NAMES):
            assert index.add(emb[i], name) == (i, i + 1)
        _CACHE["scene"] = (ex, emb, index)
    return _CACHE["scene"]


def _close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool((np.abs(got - want) <= BAR * (np.abs(want) + np.abs(want).mean())).all())


def test_scene_index_ranks_like_the_reference_and_finds_the_twin():
    ex, emb, index = _scene()
    host = emb.cpu().numpy()
    assert len(index) == 6 and index.meta["kind"] == "scene" and index.bank.shape == host.shape and index.bank.is_cuda
    assert bool((np.abs(index.bank.double().cpu().numpy() - R.normalize_ref(host)) <= 2e-6).all())
    ref = R.scores_ref(host, host)
    score, rows = index.search(emb, 4, extractor=ex)
    assert score.is_cuda and rows.is_cuda and rows.dtype == torch.int32
    s, i = score.cpu().numpy(), rows.cpu().numpy()
    R.check_ranking(s, i, ref, 4, bar=BAR, slack=2 * BAR, tag="scene index")
    for q, twin in ((1, 3), (3, 1)):                        # a recording and its copy: both at cosine 1, then the others
        assert sorted(i[q, :2].tolist()) == [1, 3] and bool((np.abs(s[q, :2].astype(np.float64) - 1.0) <= BAR).all())
    for q in range(6):
        assert abs(float(s[q, 0]) - 1.0) <= BAR             # every recording finds itself (or its twin) first

    skip = [list(index.row_range(name)) for name in NAMES]
    score, rows = index.search(emb, 6, exclude=NAMES)
    s, i = score.cpu().numpy(), rows.cpu().numpy()
    R.check_ranking(s, i, ref, 6, skip, bar=BAR, slack=2 * BAR, tag="scene index, exclude self")
    assert i[1, 0] == 3 and i[3, 0] == 1 and bool((i[:, 5] == -1).all()) and not bool((i == np.arange(6)[:, None]).any())
    found = index.hits(score, rows)
    assert [len(f) for f in found] == [5] * 6 and found[1][0]["name"] == "rec3.wav" and found[1][0]["time_ms"] is None
    assert found[1][0]["row"] == 3 and abs(found[1][0]["score"] - 1.0) <= BAR
    # one name for every query, none for some
    one = index.search(emb[:2], 3, exclude="rec1.wav")[1].cpu().numpy()
    assert not bool((one == 1).any())
    some = index.search(emb[:2], 3, exclude=[None, "rec1.wav"])[1].cpu().numpy()
    assert some[0].tolist() == i_free(index, emb[:1], 3) and some[1, 0] == 3


def i_free(index, queries, k):
    return index.search(queries, k)[1].cpu().numpy()[0].tolist()


def test_what_the_index_refuses():
    ex, emb, index = _scene()
    with pytest.raises(ValueError, match="do not compare"):
        index.search(emb, 3, extractor=_extractor(layers=[0, 16]))
    with pytest.raises(ValueError, match=r"queries must be \(Q >= 1"):
        index.search(emb[:, :-1], 3)
    with pytest.raises(ValueError, match="no file named 'nobody.wav'"):
        index.search(emb[:1], 3, exclude=["nobody.wav"])
    with pytest.raises(ValueError, match="one name or None per query"):
        index.search(emb, 3, exclude=["rec0.wav"])
    with pytest.raises(_lib.EatHipError, match="need 1 <= k <= 128"):
        index.search(emb, 129)
    with pytest.raises(ValueError, match="the index is empty"):
        retrieval.EmbeddingIndex(4, device=DEV).search(torch.zeros(1, 4), 1)
    with pytest.raises(ValueError, match="is in the index already"):
        index.add(emb[0], "rec0.wav")
    assert len(index) == 6


def test_the_bank_grows_by_doubling_and_keeps_its_rows():
    D = 24
    rng = np.random.default_rng(0)
    index = retrieval.EmbeddingIndex(D, device=DEV)
    chunks = [rng.standard_normal((n, D)).astype(np.float32) for n in (50, 20, 130, 1)]
    for j, c in enumerate(chunks):
        index.add(c, f"f{j}", np.arange(len(c)) * 10.0)
    rows = np.concatenate(chunks)
    assert len(index) == 201 and index._bank.shape[0] == 256
    assert bool((np.abs(index.bank.double().cpu().numpy() - R.normalize_ref(rows)) <= 2e-6).all())
    score, idx = index.search(rows[[0, 69, 200]], 1)
    assert idx.cpu().numpy()[:, 0].tolist() == [0, 69, 200]
    assert [h[0]["name"] for h in index.hits(score, idx)] == ["f0", "f1", "f3"] and index.hits(score, idx)[1][0]["time_ms"] == 190.0


def test_timestamp_index_save_and_load(tmp_path):
    ex = _extractor()
    recs = [_wave(40000, seed=7), _wave(20000, seed=8), _wave(33000, seed=9)]
    names = ["long.wav", "short.wav", "mid.wav"]
    api = ex.timestamp_embeddings(recs, hop_ms=50.0, width_ms=160.0)
    index = retrieval.EmbeddingIndex.from_recordings(ex, recs, names, timestamps=True, hop_ms=50.0, width_ms=160.0)
    assert index.meta == {"version": 1, "D": ex.timestamp_embedding_size, "kind": "timestamps", "model_name": None,
                          "layers": list(range(17)), "clip_seconds": 1.0, "hop_ms": 50.0, "width_ms": 160.0}
    assert len(index) == sum(len(t) for _, t in api) and index.names == names
    row = 0
    for j, (emb, t_ms) in enumerate(api):                   # rows and times: those of each file, in order
        lo, hi = index.row_range(names[j])
        assert (lo, hi) == (row, row + len(t_ms)) and np.array_equal(index.time_ms[lo:hi], t_ms)
        assert bool((index.file_ids[lo:hi] == j).all())
        assert _close(index.bank[lo:hi].cpu().numpy(), R.normalize_ref(emb.cpu().numpy()))
        row = hi
    # rows of the index as queries find themselves: the right file at the right time
    picks = [3, index.row_range("short.wav")[0] + 5, len(index) - 1]
    queries = index.bank[picks].clone()
    score, rows = index.search(queries, 5)
    found = index.hits(score, rows)
    for q, p in enumerate(picks):
        assert found[q][0]["row"] == p and abs(found[q][0]["score"] - 1.0) <= BAR
    assert (found[0][0]["name"], found[0][0]["time_ms"]) == ("long.wav", 150.0)
    assert (found[1][0]["name"], found[1][0]["time_ms"]) == ("short.wav", 250.0)
    assert (found[2][0]["name"], found[2][0]["time_ms"]) == ("mid.wav", float(api[2][1][-1]))
    ref = R.scores_ref(index.bank.cpu().numpy(), queries.cpu().numpy())
    R.check_ranking(score.cpu().numpy(), rows.cpu().numpy(), ref, 5, bar=BAR, slack=2 * BAR, tag="timestamp index")
    # leaving a file out leaves every one of its rows out
    _, rows_x = index.search(queries, 5, exclude=["long.wav", None, "mid.wav"])
    lo, hi = index.row_range("long.wav")
    assert not bool(((rows_x[0] >= lo) & (rows_x[0] < hi)).any()) and torch.equal(rows_x[1], rows[1])

    path = str(tmp_path / "idx")
    index.save(path)
    back = retrieval.EmbeddingIndex.load(path, device="cuda")
    assert back.device == DEV and back.bank.is_cuda and torch.equal(back.bank, index.bank) and back.meta == index.meta
    score_b, rows_b = back.search(queries, 5, extractor=ex)
    assert torch.equal(score_b, score) and torch.equal(rows_b, rows)          # the same bits
    assert back.hits(score_b, rows_b) == found
    cpu = retrieval.EmbeddingIndex.load(path)
    assert cpu.device is None and np.array_equal(cpu.bank.numpy(), index.bank.cpu().numpy())
    with pytest.raises(_lib.EatHipError, match="needs the index on a GPU"):
        cpu.search(queries, 5)


def _write_wavs(tmp_path, lengths, twin=None):
    paths = []
    for i, n in enumerate(lengths):
        wave = _wave(n, seed=40 + (twin[i] if twin else i))
        paths.append(str(tmp_path / f"clip{i}.wav"))
        wavfile.write(paths[-1], SR, (wave.clamp(-1, 1) * 32767).to(torch.int16).numpy())
    return paths


def _json_lines(capsys):
    return [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]


def test_command_line_scene_index(tmp_path, capsys):
    ckpt = str(tmp_path / "mn04.pt")
    torch.save(_model().state_dict(), ckpt)
    paths = _write_wavs(tmp_path, (48000, 20000, 48000, 30000), twin=(0, 1, 0, 3))       # clip2 is clip0 again
    model = ["--checkpoint", ckpt, "--width", "0.4", "--clip_seconds", "1.0"]
    idx = str(tmp_path / "idx")
    assert search.main(["index", "--audio_path", *paths, "--out", idx] + model) == 0
    index = retrieval.EmbeddingIndex.load(idx)
    assert index.names == paths and len(index) == 4 and index.meta["kind"] == "scene" and index.meta["layers"] == list(range(17))
    ex = _extractor()
    api = ex.scene_embeddings([ex.load_waveform(p) for p in paths]).cpu().numpy()
    assert _close(index.bank.numpy(), R.normalize_ref(api))
    ref = R.scores_ref(api, api)
    capsys.readouterr()

    assert search.main(["query", "--index", idx, "--audio_path", paths[0], paths[1], "--k", "3", "--json"] + model) == 0
    lines = _json_lines(capsys)
    assert [ln["audio_path"] for ln in lines] == paths[:2] and all(len(ln["hits"]) == 3 for ln in lines)
    assert sorted(h["name"] for h in lines[0]["hits"][:2]) == [paths[0], paths[2]] and lines[1]["hits"][0]["name"] == paths[1]
    for q, ln in enumerate(lines):
        for h in ln["hits"]:
            assert set(h) == {"name", "time_ms", "score"} and h["time_ms"] is None
            assert abs(h["score"] - ref[q, paths.index(h["name"])]) <= BAR

    assert search.main(["query", "--index", idx, "--audio_path", paths[0], "--k", "4", "--exclude_self", "--json"] + model) == 0
    (line,) = _json_lines(capsys)
    assert [h["name"] for h in line["hits"]][0] == paths[2] and len(line["hits"]) == 3 and paths[0] not in [h["name"] for h in line["hits"]]

    assert search.main(["query", "--index", idx, "--audio_path", paths[3], "--k", "2"] + model) == 0      # the table
    out = capsys.readouterr().out.splitlines()
    head = out.index(paths[3])
    assert len(out) == head + 3 and out[head + 1].split()[0] == "1" and out[head + 1].endswith(paths[3]) and out[head + 2].split()[0] == "2"

    with pytest.raises(ValueError, match=r"the index was built with .* do not compare"):
        search.main(["query", "--index", idx, "--audio_path", paths[0], "--layers", "0", "16"] + model)


def test_command_line_timestamp_index(tmp_path, capsys):
    ckpt = str(tmp_path / "mn04.pt")
    torch.save(_model().state_dict(), ckpt)
    paths = _write_wavs(tmp_path, (48000, 20000))
    model = ["--checkpoint", ckpt, "--width", "0.4", "--clip_seconds", "1.0", "--layers", "0", "5", "16"]
    idx = str(tmp_path / "idx")
    assert search.main(["index", "--audio_path", *paths, "--out", idx, "--timestamps", "--hop_ms", "100", "--width_ms", "200"] + model) == 0
    index = retrieval.EmbeddingIndex.load(idx)
    assert len(index) == 15 + 7 and index.meta["layers"] == [0, 5, 16] and (index.meta["hop_ms"], index.meta["width_ms"]) == (100.0, 200.0)
    assert np.array_equal(index.time_ms[:15], np.arange(15) * 100.0) and index.file_ids.tolist() == [0] * 15 + [1] * 7
    capsys.readouterr()
    assert search.main(["query", "--index", idx, "--audio_path", paths[1], "--k", "5", "--json", "--exclude_self"] + model) == 0
    (line,) = _json_lines(capsys)
    assert len(line["hits"]) == 5 and all(h["name"] == paths[0] and h["time_ms"] in (np.arange(15) * 100.0) for h in line["hits"])
    scores = [h["score"] for h in line["hits"]]
    assert scores == sorted(scores, reverse=True) and 0.0 < scores[0] <= 1.0 + BAR
    with pytest.raises(ValueError, match=r"the index was built with .* do not compare"):
        search.main(["query", "--index", idx, "--audio_path", paths[1], "--checkpoint", ckpt, "--width", "0.4", "--clip_seconds", "1.0"])
