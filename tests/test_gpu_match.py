"""Occurrence search end to end: `EmbeddingIndex.find` / `find_recordings` (efficientat_amd/retrieval.py) and the `find`
command (efficientat_amd/search.py).

The planted scene: two files of 300 rows, smoothed along time so that neighbouring rows are nearly equal - which is what
rows 50 ms apart that pool overlapping feature-map columns look like - and one clip of 20 rows planted in each.  A plain
`search` for the clip returns the same place over and over; `find` must return the two planted places first and then
distinct places at least a separation apart.  The yardstick is tests/match_ref.py in fp64 on the index's stored rows: scores
within the project's per-op bar 2e-5.  The end-to-end part runs on the seeded random-weight model and synthetic WAVs of
tests/test_gpu_search.py; two forwards of one input agree to a few fp32 ulps only, so there too the bar is 2e-5."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, retrieval, search  # noqa: E402
from tests import match_ref as M  # noqa: E402
from tests import search_ref as R  # noqa: E402
from tests.test_gpu_search import _extractor, _json_lines, _model, _write_wavs  # noqa: E402

DEV = torch.device("cuda:0")
BAR = 2e-5
D, ROWS, L, AT, HOP = 48, 300, 20, 100, 50.0
_CACHE = {}


def _smooth(rows, width=9):
    """A moving average along time: neighbouring rows share most of what they average."""
    kernel = np.ones(width) / width
    return np.stack([np.convolve(rows[:, d], kernel, mode="same") for d in range(rows.shape[1])], axis=1)


def _planted():
    """(index, clip (L, D) numpy): files a.wav and b.wav, the clip at row AT of each (b's copy slightly disturbed)."""
    if "planted" not in _CACHE:
        rng = np.random.default_rng(5)
        clip = _smooth(rng.standard_normal((L + 8, D)))[4:4 + L]
        index = retrieval.EmbeddingIndex(D, device=DEV, meta={"kind": "timestamps", "hop_ms": HOP, "width_ms": 160.0})
        for name, noise in (("a.wav", 0.0), ("b.wav", 0.03)):
            rows = _smooth(rng.standard_normal((ROWS, D)))
            rows[AT:AT + L] = clip + noise * rng.standard_normal((L, D))
            index.add(rows.astype(np.float32), name, np.arange(ROWS) * HOP)
        _CACHE["planted"] = (index, clip.astype(np.float32))
    return _CACHE["planted"]


def _reference(index, queries, k, sep, skip=None):
    """match_ref in fp64 on the rows as stored -> (score, row, m64 of every start row)."""
    S = R.scores_ref(index.bank.cpu().numpy(), np.asarray(queries))
    seg = [0] + [index.row_range(name)[1] for name in index.names]
    score, row = M.match_ref(S, seg, k, sep, skip=skip)
    return score, row, M.window_means(S)


def test_the_planted_places_come_first_with_their_files_and_times():
    index, clip = _planted()
    k, sep = 10, L                                            # the default separation: max(L, ceil(160 / 50))
    score, row = index.find(clip, k)
    assert score.is_cuda and row.is_cuda and score.shape == (k,) and row.dtype == torch.int32
    s, r = score.cpu().numpy(), row.cpu().numpy()
    want_s, want_r, m64 = _reference(index, clip, k, sep)
    assert r[:2].tolist() == [AT, ROWS + AT] == want_r[:2].tolist()
    assert bool((r >= 0).all()) and bool((np.abs(s - m64[r]) <= BAR).all()) and bool((np.abs(s - want_s) <= 2 * BAR).all())
    assert abs(float(s[0]) - 1.0) <= BAR and 0.9 < float(s[1]) < float(s[0]) and float(s[2]) < float(s[1]) - 0.02
    found = index.hits(score, row, query_rows=L)
    assert [(h["name"], h["time_ms"], h["end_ms"], h["row"]) for h in found[:2]] == [("a.wav", AT * HOP, (AT + L) * HOP, AT),
                                                                                   ("b.wav", AT * HOP, (AT + L) * HOP, ROWS + AT)]
    assert all(abs(h["score"] - float(v)) == 0 for h, v in zip(found, s)) and len(found) == k
    # the same separation spelt out, and the same bits from call to call
    again = index.find(torch.from_numpy(clip), k, min_separation_rows=sep)
    assert torch.equal(again[0], score) and torch.equal(again[1], row)


def test_find_returns_distinct_places_where_search_returns_one_place_over_and_over():
    index, clip = _planted()
    k = 10
    _, rows = index.search(clip.mean(axis=0), k)
    rows = np.sort(rows.cpu().numpy()[0])
    places = 1 + int((np.diff(rows) > L).sum())
    print(f"search: {k} rows in {places} places; rows {rows.tolist()}")
    assert places <= 2
    for sep in (L, 7, 45):
        r = index.find(clip, k, min_separation_rows=sep)[1].cpu().numpy()
        r = r[:k if sep < 45 else 7]                                            # 45 rows apart, the two files hold 7 places
        assert bool((r >= 0).all()) and len(set(r.tolist())) == len(r)
        for a in r:
            lo, hi = index.row_range(index.names[index.file_ids[a]])
            assert lo <= a and a + L <= hi                                     # the whole window lies in one file
            near = [b for b in r if b != a and index.file_ids[b] == index.file_ids[a] and abs(int(b) - int(a)) <= sep]
            assert not near, (sep, a, near)


def test_threshold_exclusion_and_a_file_added_later():
    index, clip = _planted()
    score, row = index.find(clip, 5, min_score=0.9)
    assert row.cpu().tolist() == [AT, ROWS + AT, -1, -1, -1] and bool(torch.isneginf(score[2:]).all())
    score, row = index.find(clip, 5, exclude="a.wav")
    r = row.cpu().numpy()
    lo, hi = index.row_range("a.wav")
    assert r[0] == ROWS + AT and not bool(((r >= lo) & (r < hi)).any()) and bool((r >= 0).all())
    want_s, want_r, _ = _reference(index, clip, 5, L, skip=(lo, hi))
    assert r[:1].tolist() == want_r[:1].tolist() and bool((np.abs(score.cpu().numpy() - want_s) <= 2 * BAR).all())
    with pytest.raises(ValueError, match="no file named 'nobody.wav'"):
        index.find(clip, 5, exclude="nobody.wav")
    # a file added after a match: the file bounds on the device are rebuilt
    grown = retrieval.EmbeddingIndex(D, device=DEV, meta={"kind": "timestamps", "hop_ms": HOP, "width_ms": 160.0})
    rng = np.random.default_rng(6)
    first = rng.standard_normal((40, D)).astype(np.float32)
    grown.add(first, "first.wav", np.arange(40) * HOP)
    assert grown.find(clip, 2)[1].cpu().numpy()[0] >= 0
    later = rng.standard_normal((30, D)).astype(np.float32)
    later[5:5 + L] = clip
    grown.add(later, "later.wav", 1000.0 + np.arange(30) * HOP)                # a progression need not start at 0
    score, row = grown.find(clip, 2)
    (best, *_) = grown.hits(score, row, query_rows=L)
    assert (best["name"], best["row"], best["time_ms"], best["end_ms"]) == ("later.wav", 45, 1250.0, 1250.0 + L * HOP)
    assert abs(best["score"] - 1.0) <= BAR
    # a clip longer than every file: nothing
    assert grown.find(rng.standard_normal((41, D)).astype(np.float32), 3)[1].cpu().tolist() == [-1, -1, -1]


def test_what_find_refuses():
    index, clip = _planted()
    with pytest.raises(ValueError, match=rf"query_rows must be \(L >= 1, {D}\)"):
        index.find(clip[:, :-1], 3)
    with pytest.raises(_lib.EatHipError, match="need 1 <= k <= 128"):
        index.find(clip, 129)
    with pytest.raises(ValueError, match="min_separation_rows must be an integer >= 0"):
        index.find(clip, 3, min_separation_rows=-1)
    uneven = retrieval.EmbeddingIndex(D, device=DEV, meta={"kind": "timestamps", "hop_ms": HOP, "width_ms": 160.0})
    uneven.add(clip, "a.wav", np.arange(L) * HOP)
    uneven.add(clip[:3], "b.wav", [0.0, 50.0, 150.0])
    with pytest.raises(ValueError, match="do not step by hop_ms = 50.0"):
        uneven.find(clip[:2], 3)
    scene = retrieval.EmbeddingIndex(D, device=DEV)
    scene.add(clip[0], "x")
    with pytest.raises(ValueError, match="an index of kind 'timestamps'"):
        scene.find(clip[:2], 3)
    with pytest.raises(ValueError, match="needs the fp32 index"):
        index.quantized().find(clip, 3)
    with pytest.raises(ValueError, match="the index is empty"):
        retrieval.EmbeddingIndex(D, device=DEV, meta={"kind": "timestamps", "hop_ms": HOP}).find(clip, 3)


def test_find_recordings_and_the_command_line(tmp_path, capsys):
    ckpt = str(tmp_path / "mn04.pt")
    torch.save(_model().state_dict(), ckpt)
    paths = _write_wavs(tmp_path, (48000, 20000, 40000))
    model = ["--checkpoint", ckpt, "--width", "0.4", "--clip_seconds", "1.0", "--layers", "0", "5", "16"]
    idx = str(tmp_path / "idx")
    assert search.main(["index", "--audio_path", *paths, "--out", idx, "--timestamps", "--hop_ms", "100", "--width_ms", "200"] + model) == 0
    index = retrieval.EmbeddingIndex.load(idx, device="cuda")
    ex = _extractor(layers=[0, 5, 16])
    waves = [ex.load_waveform(p) for p in paths[1:]]
    clips = [emb for emb, _ in ex.timestamp_embeddings(waves, hop_ms=100.0, width_ms=200.0)]
    k = 4
    results = index.find_recordings(ex, waves, k, exclude=[paths[1], None])
    assert len(results) == 2 and [n for _, _, n in results] == [c.shape[0] for c in clips]
    lo1, hi1 = index.row_range(paths[1])
    for (score, row, n), clip, skip in zip(results, clips, ((lo1, hi1), None)):
        s, r = score.cpu().numpy(), row.cpu().numpy()
        own = index.find(clip, k, exclude=paths[1] if skip else None)
        m64 = _reference(index, clip.cpu().numpy(), k, n, skip)[2]
        kept = r >= 0
        assert kept.any() and np.array_equal(own[1].cpu().numpy()[kept] >= 0, kept[kept])
        assert bool((np.abs(s[kept] - m64[r[kept]]) <= BAR).all())
        assert bool((np.abs(own[0].cpu().numpy()[kept] - m64[own[1].cpu().numpy()[kept]]) <= BAR).all())
    r0 = results[0][1].cpu().numpy()
    assert not bool(((r0 >= lo1) & (r0 < hi1)).any())
    lo2 = index.row_range(paths[2])[0]
    assert results[1][1].cpu().numpy()[0] == lo2 and abs(float(results[1][0][0]) - 1.0) <= BAR      # a recording finds itself
    capsys.readouterr()

    assert search.main(["find", "--index", idx, "--audio_path", paths[1], paths[2], "--k", str(k), "--json"] + model) == 0
    lines = _json_lines(capsys)
    assert [ln["audio_path"] for ln in lines] == paths[1:] and [ln["rows"] for ln in lines] == [c.shape[0] for c in clips]
    for ln, clip in zip(lines, clips):
        n = clip.shape[0]
        m64 = _reference(index, clip.cpu().numpy(), k, n)[2]
        assert ln["query"] == "sequence" and 1 <= len(ln["hits"]) <= k
        assert (ln["hits"][0]["name"], ln["hits"][0]["time_ms"]) == (ln["audio_path"], float(index.time_ms[index.row_range(ln["audio_path"])[0]]))
        for h in ln["hits"]:
            assert set(h) == {"name", "time_ms", "end_ms", "score"} and h["end_ms"] == h["time_ms"] + n * 100.0
            lo, hi = index.row_range(h["name"])
            at = lo + int(np.flatnonzero(index.time_ms[lo:hi] == h["time_ms"])[0])
            assert abs(h["score"] - m64[at]) <= BAR
    assert search.main(["find", "--index", idx, "--audio_path", paths[1], "--k", "3", "--exclude_self", "--json",
                        "--min_separation_ms", "250", "--query", "scene"] + model) == 0
    (line,) = _json_lines(capsys)
    assert line["query"] == "scene" and line["rows"] == 1 and 1 <= len(line["hits"]) <= 3
    assert all(h["name"] != paths[1] and h["end_ms"] == h["time_ms"] + 100.0 for h in line["hits"])
    times = {}
    for h in line["hits"]:
        assert all(abs(h["time_ms"] - t) > 250.0 - 1e-9 for t in times.get(h["name"], [])), line["hits"]      # 3 rows apart: > 200 ms
        times.setdefault(h["name"], []).append(h["time_ms"])
    assert search.main(["find", "--index", idx, "--audio_path", paths[2], "--k", "2", "--min_score", "0.5"] + model) == 0      # the table
    out = capsys.readouterr().out.splitlines()
    head = out.index(paths[2])
    assert len(out) in (head + 2, head + 3) and out[head + 1].split()[0] == "1" and out[head + 1].endswith(paths[2])
