"""Occurrence search on a q8 index end to end: `EmbeddingIndex.find(allow_q8=True)` / `find_recordings` and the `find`
command on an index of storage "q8".

The planted scene is that of tests/test_gpu_match.py.  The yardstick is tests/match_ref.py in fp64 on the fp32 index's stored
rows; the bound of a q8 score is the mean over its window of the per-pair quantisation bound
    sq sn (0.5 sum |cq| + 0.5 sum |cn| + 0.25 D) + 2e-5
of tests/test_gpu_search_q8_kernels.py (tests/test_match_q8_cpu.py: `pair_bounds`): at D = 48 a planted place scores 0.99950
where fp64 says 1.00000, so 2e-5 alone is not the bar here.  The end-to-end part runs on the seeded random-weight model and
synthetic WAVs of tests/test_gpu_search.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import ops, retrieval, search  # noqa: E402
from tests import match_ref as M  # noqa: E402
from tests.test_gpu_match import AT, D, HOP, L, ROWS, _planted, _reference  # noqa: E402
from tests.test_gpu_search import _extractor, _json_lines, _model, _write_wavs  # noqa: E402
from tests.test_match_q8_cpu import PLANTED_ROWS, pair_bounds  # noqa: E402

DEV = torch.device("cuda:0")
_CACHE = {}


def _q8():
    """(fp32 index, its q8 twin, clip): shared and left unchanged."""
    if "q8" not in _CACHE:
        index, clip = _planted()
        _CACHE["q8"] = (index, index.quantized(), clip)
    return _CACHE["q8"]


def _bounds(q8, queries):
    """(N,) fp64: per start row, the mean over its window of the per-pair bound for these query rows."""
    with torch.cuda.device(q8.device):
        qcodes, qscale = ops.rows_quantize_q8(torch.as_tensor(queries).to(device=q8.device, dtype=torch.float32).contiguous())
    dim = q8.D
    return M.window_means(pair_bounds(q8.codes[:, :dim].cpu().numpy(), q8.scales.cpu().numpy(), qcodes[:, :dim].cpu().numpy(),
                                      qscale.cpu().numpy(), dim))


def test_the_planted_places_come_first_with_the_rows_of_the_fp32_index():
    index, q8, clip = _q8()
    assert q8.storage == "q8" and len(q8) == 2 * ROWS
    k, sep = 10, L
    score, row = q8.find(clip, k, allow_q8=True)
    assert score.is_cuda and row.is_cuda and score.shape == (k,) and score.dtype == torch.float32 and row.dtype == torch.int32
    s, r = score.cpu().numpy(), row.cpu().numpy()
    assert r[:2].tolist() == [AT, ROWS + AT]
    assert r.tolist() == index.find(clip, k)[1].cpu().tolist() == PLANTED_ROWS
    _, want_r, m64 = _reference(index, clip, k, sep)
    assert r.tolist() == want_r.tolist()
    err, bound = np.abs(s - m64[r]), _bounds(q8, clip)[r]
    print(f"MATCH_Q8 planted: scores {s[:2].tolist()}, largest |m - m64| = {float(err.max()):.3e}, "
          f"largest share of the bound {float((err / bound).max()):.4f}")
    assert bool((err <= bound).all())
    found = q8.hits(score, row, query_rows=L)
    assert [(h["name"], h["time_ms"], h["end_ms"], h["row"]) for h in found[:2]] == [("a.wav", AT * HOP, (AT + L) * HOP, AT),
                                                                                   ("b.wav", AT * HOP, (AT + L) * HOP, ROWS + AT)]
    assert all(h["score"] == float(v) for h, v in zip(found, s)) and len(found) == k
    # the same separation spelt out, and the same bits from call to call
    again = q8.find(torch.from_numpy(clip), k, min_separation_rows=sep, allow_q8=True)
    assert torch.equal(again[0], score) and torch.equal(again[1], row)
    # the scores are those of the codes: on the scale of `search` on the same index (L = 1: the very bits)
    one = q8.find(clip[:1], 3, min_separation_rows=0, exclude="b.wav", allow_q8=True)
    plain = q8.search(clip[:1], 3, exclude="b.wav")
    assert torch.equal(one[0], plain[0][0]) and torch.equal(one[1], plain[1][0])
    # on an fp32 index the keyword changes nothing
    a, b = index.find(clip, k), index.find(clip, k, allow_q8=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_threshold_exclusion_and_a_file_added_later():
    index, q8, clip = _q8()
    score, row = q8.find(clip, 5, min_score=0.9, allow_q8=True)
    assert row.cpu().tolist() == [AT, ROWS + AT, -1, -1, -1] and bool(torch.isneginf(score[2:]).all())
    score, row = q8.find(clip, 5, exclude="a.wav", allow_q8=True)
    r = row.cpu().numpy()
    lo, hi = q8.row_range("a.wav")
    assert r[0] == ROWS + AT and not bool(((r >= lo) & (r < hi)).any()) and bool((r >= 0).all())
    # the fifth place is a near-tie of neighbouring rows 564 / 565, closer than the quantisation error: rows are not compared
    # with the fp32 index's here, scores are, at the rows returned
    m64 = _reference(index, clip, 5, L, skip=(lo, hi))[2]
    assert bool((np.abs(score.cpu().numpy() - m64[r]) <= _bounds(q8, clip)[r]).all())
    assert r[:4].tolist() == index.find(clip, 5, exclude="a.wav")[1].cpu().tolist()[:4]
    with pytest.raises(ValueError, match="no file named 'nobody.wav'"):
        q8.find(clip, 5, exclude="nobody.wav", allow_q8=True)
    # the default-argument refusal still stands
    with pytest.raises(ValueError, match="needs the fp32 index"):
        q8.find(clip, 3)
    # a file added after a match: the file bounds on the device are rebuilt
    meta = {"kind": "timestamps", "hop_ms": HOP, "width_ms": 160.0}
    grown = retrieval.EmbeddingIndex(D, device=DEV, meta=meta, storage="q8")
    rng = np.random.default_rng(6)
    first = rng.standard_normal((40, D)).astype(np.float32)
    grown.add(first, "first.wav", np.arange(40) * HOP)
    assert grown.find(clip, 2, allow_q8=True)[1].cpu().numpy()[0] >= 0
    later = rng.standard_normal((30, D)).astype(np.float32)
    later[5:5 + L] = clip
    grown.add(later, "later.wav", 1000.0 + np.arange(30) * HOP)                # a progression need not start at 0
    score, row = grown.find(clip, 2, allow_q8=True)
    (best, *_) = grown.hits(score, row, query_rows=L)
    assert (best["name"], best["row"], best["time_ms"], best["end_ms"]) == ("later.wav", 45, 1250.0, 1250.0 + L * HOP)
    assert abs(best["score"] - 1.0) <= float(_bounds(grown, clip)[45])      # the clip's own codes: the bound of a self-match
    # a clip longer than every file: nothing
    assert grown.find(rng.standard_normal((41, D)).astype(np.float32), 3, allow_q8=True)[1].cpu().tolist() == [-1, -1, -1]


def test_save_and_load_give_the_same_bits(tmp_path):
    _, q8, clip = _q8()
    q8.save(str(tmp_path / "idx"))
    loaded = retrieval.EmbeddingIndex.load(str(tmp_path / "idx"), device="cuda")
    assert loaded.storage == "q8" and torch.equal(loaded.codes[:, :D], q8.codes[:, :D]) and torch.equal(loaded.scales, q8.scales)
    for kwargs in (dict(), dict(min_separation_rows=7), dict(exclude="a.wav", min_score=0.3)):
        a, b = q8.find(clip, 10, allow_q8=True, **kwargs), loaded.find(clip, 10, allow_q8=True, **kwargs)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), kwargs


def test_find_recordings_and_the_command_line(tmp_path, capsys):
    ckpt = str(tmp_path / "mn04.pt")
    torch.save(_model().state_dict(), ckpt)
    paths = _write_wavs(tmp_path, (48000, 20000, 40000))
    model = ["--checkpoint", ckpt, "--width", "0.4", "--clip_seconds", "1.0", "--layers", "0", "5", "16"]
    idx, idx32 = str(tmp_path / "idx_q8"), str(tmp_path / "idx_fp32")
    common = ["--audio_path", *paths, "--timestamps", "--hop_ms", "100", "--width_ms", "200"] + model
    assert search.main(["index", "--out", idx, "--storage", "q8"] + common) == 0
    assert search.main(["index", "--out", idx32] + common) == 0
    index = retrieval.EmbeddingIndex.load(idx, device="cuda")
    fp32 = retrieval.EmbeddingIndex.load(idx32, device="cuda")
    assert index.storage == "q8" and index.meta["kind"] == "timestamps" and index.names == paths and len(index) == len(fp32)
    ex = _extractor(layers=[0, 5, 16])
    waves = [ex.load_waveform(p) for p in paths[1:]]
    clips = [emb for emb, _ in ex.timestamp_embeddings(waves, hop_ms=100.0, width_ms=200.0)]
    k = 4
    with pytest.raises(ValueError, match="needs the fp32 index"):
        index.find_recordings(ex, waves, k)
    results = index.find_recordings(ex, waves, k, exclude=[paths[1], None], allow_q8=True)
    assert len(results) == 2 and [n for _, _, n in results] == [c.shape[0] for c in clips]
    lo1, hi1 = index.row_range(paths[1])
    for (score, row, n), clip, skip in zip(results, clips, ((lo1, hi1), None)):
        s, r = score.cpu().numpy(), row.cpu().numpy()
        m64 = _reference(fp32, clip.cpu().numpy(), k, n, skip)[2]
        bound = _bounds(index, clip)
        kept = r >= 0
        assert kept.any() and bool((np.abs(s[kept] - m64[r[kept]]) <= bound[r[kept]]).all())
    r0 = results[0][1].cpu().numpy()
    assert not bool(((r0 >= lo1) & (r0 < hi1)).any())
    lo2 = index.row_range(paths[2])[0]
    assert results[1][1].cpu().numpy()[0] == lo2                                       # a recording finds itself
    assert abs(float(results[1][0][0]) - 1.0) <= float(_bounds(index, clips[1])[lo2])
    capsys.readouterr()

    assert search.main(["find", "--index", idx, "--audio_path", paths[1], paths[2], "--k", str(k), "--json"] + model) == 0
    lines = _json_lines(capsys)
    assert [ln["audio_path"] for ln in lines] == paths[1:] and [ln["rows"] for ln in lines] == [c.shape[0] for c in clips]
    for ln, clip in zip(lines, clips):
        n = clip.shape[0]
        m64 = _reference(fp32, clip.cpu().numpy(), k, n)[2]
        bound = _bounds(index, clip)
        assert ln["storage"] == "q8" and ln["query"] == "sequence" and 1 <= len(ln["hits"]) <= k
        assert (ln["hits"][0]["name"], ln["hits"][0]["time_ms"]) == (ln["audio_path"], float(index.time_ms[index.row_range(ln["audio_path"])[0]]))
        for h in ln["hits"]:
            assert set(h) == {"name", "time_ms", "end_ms", "score"} and h["end_ms"] == h["time_ms"] + n * 100.0
            lo, hi = index.row_range(h["name"])
            at = lo + int(np.flatnonzero(index.time_ms[lo:hi] == h["time_ms"])[0])
            assert abs(h["score"] - m64[at]) <= bound[at]
    # the fp32 index answers as before, and says what it is
    assert search.main(["find", "--index", idx32, "--audio_path", paths[2], "--k", "2", "--json"] + model) == 0
    (line,) = _json_lines(capsys)
    assert line["storage"] == "fp32" and line["hits"][0]["name"] == paths[2]
    assert search.main(["find", "--index", idx, "--audio_path", paths[2], "--k", "2", "--min_score", "0.5"] + model) == 0      # the table
    out = capsys.readouterr().out.splitlines()
    head = out.index(paths[2])
    assert len(out) in (head + 2, head + 3) and out[head + 1].split()[0] == "1" and out[head + 1].endswith(paths[2])
