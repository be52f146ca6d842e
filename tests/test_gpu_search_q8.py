"""`EmbeddingIndex(storage="q8")` (efficientat_amd/retrieval.py) and the command line's --storage / `convert` end to end, on the
seeded random-weight model and the synthetic waveforms of tests/test_gpu_search.py at clip_seconds = 1.0.

What a q8 index stores and returns is defined exactly (tests/search_q8_ref.py), so an index fed given rows is compared bit
for bit: its codes and scales with the emulation, its results with the emulation's top-k, and a saved and loaded index with
the one it was saved from.  Where two separate forwards of the model are involved only the ranking is compared: the
embeddings of two forwards agree to a few fp32 ulps, which can move a code by one."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, embeddings, ops, retrieval, search  # noqa: E402
from efficientat_amd.mn import get_model  # noqa: E402
from tests import search_q8_ref as R8  # noqa: E402

DEV = torch.device("cuda:0")
SR = 32000
_CACHE = {}


def _model():
    if "model" not in _CACHE:
        torch.manual_seed(11)
        with contextlib.redirect_stdout(io.StringIO()):
            _CACHE["model"] = get_model(width_mult=0.4).to(DEV).eval()
    return _CACHE["model"]


def _wave(n, seed):
    """Noise at a level, and a tone at a pitch, that depend on the seed: recordings that do not all sound alike."""
    noise = torch.randn(n, generator=torch.Generator().manual_seed(seed))
    tone = torch.sin(2.0 * np.pi * (150.0 * (1 + seed % 7)) * torch.arange(n, dtype=torch.float64) / SR).float()
    return 0.02 * (1 + seed % 5) * noise + 0.05 * (1 + seed % 3) * tone


def _bits(t):
    return torch.as_tensor(t).cpu().numpy().view(np.int32)


CHUNKS = (50, 20, 130, 1)
D = 24


def _rows():
    rng = np.random.default_rng(0)
    return [rng.standard_normal((n, D)).astype(np.float32) for n in CHUNKS]


def _filled(storage="q8"):
    index = retrieval.EmbeddingIndex(D, device=DEV, storage=storage)
    for j, c in enumerate(_rows()):
        lo, hi = index.add(c, f"f{j}", np.arange(len(c)) * 10.0)
        assert hi - lo == len(c)
    return index


def test_a_q8_index_adds_searches_excludes_saves_and_loads_with_the_same_bits(tmp_path):
    index = _filled()
    rows = np.concatenate(_rows())
    assert index.storage == "q8" and len(index) == 201 and index.meta["version"] == 2 and index.meta["kind"] == "timestamps"
    assert index.codes.shape == (201, 32) and index.codes.is_cuda and index.codes.dtype == torch.int8 and index.scales.shape == (201,)
    with pytest.raises(ValueError, match="storage 'q8' has no fp32 bank"):
        index.bank
    ref_c, ref_s = R8.quantize_ref(rows, normalize=True)
    codes, scales = index.codes.cpu().numpy(), index.scales.cpu().numpy()
    assert np.array_equal(codes[:, :D], ref_c) and not codes[:, D:].any() and np.array_equal(_bits(scales), _bits(ref_s))

    picks = [0, 69, 200, 100]
    queries = rows[picks] * np.float32(3.0)                 # a row at another length: the same direction
    qc, qs = R8.quantize_ref(queries, normalize=True)
    score, found = index.search(queries, 5)
    assert score.is_cuda and found.dtype == torch.int32
    want_s, want_i = R8.search_q8_ref(ref_c, ref_s, qc, qs, 5)
    assert np.array_equal(found.cpu().numpy(), want_i) and np.array_equal(_bits(score), _bits(want_s))
    assert found[:, 0].tolist() == picks and bool((score[:, 0] > 0.99).all())
    hits = index.hits(score, found)
    assert [h[0]["name"] for h in hits] == ["f0", "f1", "f3", "f2"] and hits[1][0]["time_ms"] == 190.0 and hits[3][0]["row"] == 100

    exclude = ["f0", None, "f3", "f2"]
    score_x, found_x = index.search(queries, 5, exclude=exclude)
    skip = [(0, 0) if name is None else index.row_range(name) for name in exclude]
    want_s, want_i = R8.search_q8_ref(ref_c, ref_s, qc, qs, 5, skip)
    assert np.array_equal(found_x.cpu().numpy(), want_i) and np.array_equal(_bits(score_x), _bits(want_s))
    assert int(found_x[0].min()) >= 50 and torch.equal(found_x[1], found[1]) and 200 not in found_x[2].tolist()
    assert not bool(((found_x[3] >= 70) & (found_x[3] < 200)).any())
    with pytest.raises(ValueError, match="no file named 'nobody.wav'"):
        index.search(queries[:1], 3, exclude=["nobody.wav"])
    with pytest.raises(ValueError, match=r"queries must be \(Q >= 1"):
        index.search(queries[:, :-1], 3)

    path = str(tmp_path / "idx")
    index.save(path)
    assert sorted(os.listdir(path)) == ["codes.npy", "file.npy", "meta.json", "names.txt", "scale.npy", "time_ms.npy"]
    assert np.array_equal(np.load(os.path.join(path, "codes.npy")), ref_c)
    back = retrieval.EmbeddingIndex.load(path, device="cuda")
    assert back.storage == "q8" and back.device == DEV and back.meta == index.meta and back.names == index.names
    assert torch.equal(back.codes, index.codes) and torch.equal(back.scales, index.scales) and back.codes.is_cuda
    score_b, found_b = back.search(queries, 5)
    assert torch.equal(found_b, found) and np.array_equal(_bits(score_b), _bits(score))          # the same bits
    assert back.hits(score_b, found_b) == hits
    assert back.add(rows[:3], "later", [0.0, 1.0, 2.0]) == (201, 204)                       # a loaded index grows like any other
    assert torch.equal(back.codes[:201], index.codes) and torch.equal(back.codes[201:], index.codes[:3])
    cpu = retrieval.EmbeddingIndex.load(path)
    assert cpu.device is None and torch.equal(cpu.codes, index.codes.cpu())
    with pytest.raises(_lib.EatHipError, match="needs the index on a GPU"):
        cpu.search(queries, 5)


def test_quantized_of_an_fp32_index_equals_adding_the_rows_to_a_q8_index():
    fp32, q8 = _filled("fp32"), _filled("q8")
    conv = fp32.quantized()
    assert conv.storage == "q8" and conv.device == DEV and len(conv) == 201 and conv.names == q8.names
    assert conv.meta == q8.meta and np.array_equal(conv.file_ids, q8.file_ids) and np.array_equal(conv.time_ms, q8.time_ms)
    assert [conv.row_range(n) for n in conv.names] == [q8.row_range(n) for n in q8.names]
    assert torch.equal(conv.codes, q8.codes) and torch.equal(conv.scales, q8.scales)
    assert conv.add(_rows()[0][:2], "more", [0.0, 1.0]) == (201, 203) and len(fp32) == 201 and "more" not in fp32.names
    with pytest.raises(ValueError, match="needs an fp32 index on a GPU"):
        q8.quantized()
    empty = retrieval.EmbeddingIndex(D, device=DEV).quantized()
    assert len(empty) == 0 and empty.storage == "q8"
    with pytest.raises(ValueError, match="the index is empty"):
        empty.search(torch.zeros(1, D), 1)


def test_the_bank_grows_by_doubling_and_keeps_earlier_codes():
    index = retrieval.EmbeddingIndex(D, device=DEV, storage="q8")
    seen = []
    for j, c in enumerate(_rows()):
        index.add(c, f"f{j}", np.arange(len(c)) * 10.0)
        seen.append((index.codes.clone(), index.scales.clone()))
    assert [index._codes.shape[0], index._scale.shape[0]] == [256, 256] and index._codes.shape[1] == ops.q8_ld(D)
    n = 0
    for (codes, scales), c in zip(seen, _rows()):           # what each add left is still there after the later ones
        n += len(c)
        assert torch.equal(index.codes[:n], codes) and torch.equal(index.scales[:n], scales)


def _extractor():
    return embeddings.EmbeddingExtractor(model=_model(), clip_seconds=1.0)


def test_from_recordings_finds_each_recording_and_exclude_hides_it():
    ex = _extractor()
    recs, names = [_wave(40000, seed=7), _wave(20000, seed=8)], ["long.wav", "short.wav"]
    index = retrieval.EmbeddingIndex.from_recordings(ex, recs, names, storage="q8")
    assert index.storage == "q8" and len(index) == 2 and index.meta["kind"] == "scene" and index.meta["version"] == 2
    assert index.meta["layers"] == list(range(17)) and index.codes.shape == (2, ops.q8_ld(ex.scene_embedding_size))
    queries = ex.scene_embeddings(recs)
    score, rows = index.search(queries, 2, extractor=ex)
    assert rows[:, 0].tolist() == [0, 1] and bool((score[:, 0] > 0.99).all()) and bool((score[:, 0] > score[:, 1]).all())
    assert [h[0]["name"] for h in index.hits(score, rows)] == names
    score, rows = index.search(queries, 2, exclude=names)
    assert rows.tolist() == [[1, -1], [0, -1]] and bool(torch.isneginf(score[:, 1]).all())
    stamps = retrieval.EmbeddingIndex.from_recordings(ex, recs, names, timestamps=True, hop_ms=100.0, width_ms=200.0, storage="q8")
    assert stamps.storage == "q8" and stamps.meta["kind"] == "timestamps" and len(stamps) == len(stamps.time_ms) > 2
    _, rows = stamps.search(queries, 3, exclude=["long.wav", None])
    lo, hi = stamps.row_range("long.wav")
    assert not bool(((rows[0] >= lo) & (rows[0] < hi)).any())


def _json_lines(capsys):
    return [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]


def test_command_line_index_query_and_convert(tmp_path, capsys):
    ckpt = str(tmp_path / "mn04.pt")
    torch.save(_model().state_dict(), ckpt)
    paths = []
    for i, (n, seed) in enumerate(((48000, 40), (20000, 41), (48000, 40), (30000, 43))):      # clip2 is clip0 again
        paths.append(str(tmp_path / f"clip{i}.wav"))
        wavfile.write(paths[-1], SR, (_wave(n, seed).clamp(-1, 1) * 32767).to(torch.int16).numpy())
    model = ["--checkpoint", ckpt, "--width", "0.4", "--clip_seconds", "1.0"]
    q8_dir, fp32_dir, conv_dir = (str(tmp_path / name) for name in ("q8", "fp32", "conv"))
    assert search.main(["index", "--audio_path", *paths, "--out", q8_dir, "--storage", "q8"] + model) == 0
    index = retrieval.EmbeddingIndex.load(q8_dir)
    assert index.storage == "q8" and index.names == paths and len(index) == 4
    assert sorted(os.listdir(q8_dir)) == ["codes.npy", "file.npy", "meta.json", "names.txt", "scale.npy", "time_ms.npy"]
    capsys.readouterr()

    assert search.main(["query", "--index", q8_dir, "--audio_path", paths[0], paths[1], "--k", "3", "--json"] + model) == 0
    lines = _json_lines(capsys)
    assert [ln["audio_path"] for ln in lines] == paths[:2] and all(ln["storage"] == "q8" and len(ln["hits"]) == 3 for ln in lines)
    assert sorted(h["name"] for h in lines[0]["hits"][:2]) == [paths[0], paths[2]] and lines[1]["hits"][0]["name"] == paths[1]
    assert all(set(h) == {"name", "time_ms", "score"} and h["time_ms"] is None for ln in lines for h in ln["hits"])
    assert search.main(["query", "--index", q8_dir, "--audio_path", paths[0], "--k", "4", "--exclude_self", "--json"] + model) == 0
    (line,) = _json_lines(capsys)
    assert line["hits"][0]["name"] == paths[2] and len(line["hits"]) == 3 and paths[0] not in [h["name"] for h in line["hits"]]

    assert search.main(["index", "--audio_path", *paths, "--out", fp32_dir] + model) == 0
    assert search.main(["convert", "--index", fp32_dir, "--out", conv_dir, "--storage", "q8"]) == 0
    fp32, conv = retrieval.EmbeddingIndex.load(fp32_dir, device="cuda"), retrieval.EmbeddingIndex.load(conv_dir, device="cuda")
    assert fp32.storage == "fp32" and conv.storage == "q8" and conv.names == paths and conv.meta["layers"] == list(range(17))
    again = fp32.quantized()
    assert torch.equal(conv.codes, again.codes) and torch.equal(conv.scales, again.scales)     # the rows as stored, quantised
    capsys.readouterr()
    assert search.main(["query", "--index", fp32_dir, "--audio_path", paths[3], "--k", "1", "--json"] + model) == 0
    (line,) = _json_lines(capsys)
    assert line["storage"] == "fp32" and line["hits"][0]["name"] == paths[3]
    assert search.main(["query", "--index", conv_dir, "--audio_path", paths[3], "--k", "1", "--json"] + model) == 0
    (line,) = _json_lines(capsys)
    assert line["storage"] == "q8" and line["hits"][0]["name"] == paths[3]
    assert search.main(["convert", "--index", conv_dir, "--out", str(tmp_path / "twice"), "--storage", "q8"]) == 2
    assert "has storage q8 already" in capsys.readouterr().err
