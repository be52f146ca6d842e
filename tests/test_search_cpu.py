"""Host side of query-by-example search: the header include/eat_search.h with its argument checks, the fp64 reference
(tests/search_ref.py) against a brute-force sort, `EmbeddingIndex` (efficientat_amd/retrieval.py) on the CPU - bookkeeping,
save and load - and the command line's argument errors."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from efficientat_amd import _lib, build, ops, retrieval, search
from tests import search_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"eat_rows_normalize", "eat_embed_search_ws_bytes", "eat_embed_search"}


def test_the_search_header_parses_and_is_disjoint_from_the_other_headers():
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    with open(os.path.join(ROOT, "include", "eat_search.h")) as f:
        protos = _lib.parse_prototypes(f.read())
    assert protos == _lib.SEARCH_PROTOTYPES
    assert set(protos) == NAMES
    assert protos["eat_rows_normalize"] == (I, [P, L, I, P, P])
    assert protos["eat_embed_search_ws_bytes"] == (L, [I, I])
    assert protos["eat_embed_search"] == (I, [P, L, I, P, I, I, P, P, L, P, P, P])
    others = [v for k, v in vars(_lib).items() if k.endswith("PROTOTYPES") and k != "SEARCH_PROTOTYPES"]
    assert len(others) >= 10 and not any(set(protos) & set(o) for o in others)
    assert os.path.samefile(_lib.SEARCH_HEADER_PATH, os.path.join(ROOT, "include", "eat_search.h"))


def test_the_library_exports_and_binds_the_search_entry_points():
    build.build()
    assert "search.hip" in build.SOURCES
    for name in NAMES:
        fn = getattr(_lib.lib(), name)
        restype, args = _lib.SEARCH_PROTOTYPES[name]
        assert list(fn.argtypes) == args and fn.restype is restype


def test_every_argument_error_is_raised_before_anything_touches_the_device():
    build.build()
    big = 2 ** 40
    # (N, D, Q, k, ws_bytes)
    for (N, D, Q, k, ws), match in (((10, 8, 1, 0, big), r"k=0 lies outside \[1, 128\]"),
                                    ((10, 8, 1, 129, big), r"k=129 lies outside \[1, 128\]"),
                                    ((10, 8, 1, -1, big), r"k=-1 lies outside \[1, 128\]"),
                                    ((10, 8, 0, 5, big), r"Q=0 lies outside \[1, 1024\]"),
                                    ((10, 8, 1025, 5, big), r"Q=1025 lies outside \[1, 1024\]"),
                                    ((0, 8, 1, 5, big), r"N=0 lies outside \[1, 2147483647\]"),
                                    ((-4, 8, 1, 5, big), r"N=-4 lies outside \[1, 2147483647\]"),
                                    ((2 ** 31, 8, 1, 5, big), r"N=2147483648 lies outside \[1, 2147483647\]"),
                                    ((10, 0, 1, 5, big), r"need D >= 1 \(got 0\)"),
                                    ((10, -2, 1, 5, big), r"need D >= 1 \(got -2\)"),
                                    ((10, 8, 3, 5, 0), r"ws_bytes=0 is below eat_embed_search_ws_bytes\(Q=3, k=5\) = \d+"),
                                    ((10, 8, 3, 5, -1), r"ws_bytes=-1 is below")):
        with pytest.raises(_lib.EatHipError, match=match):
            _lib.call("eat_embed_search", None, N, D, None, Q, k, None, None, ws, None, None, None)
    need = _lib.lib().eat_embed_search_ws_bytes(3, 5)
    with pytest.raises(_lib.EatHipError, match=rf"ws_bytes={need - 1} is below eat_embed_search_ws_bytes\(Q=3, k=5\) = {need}"):
        _lib.call("eat_embed_search", None, 10, 8, None, 3, 5, None, None, need - 1, None, None, None)
    for (N, D), match in (((-1, 8), r"need N >= 0 \(got -1\)"), ((4, 0), r"need D >= 1 \(got 0\)"), ((4, -7), r"need D >= 1 \(got -7\)")):
        with pytest.raises(_lib.EatHipError, match=match):
            _lib.call("eat_rows_normalize", None, N, D, None, None)


def test_workspace_bytes_are_positive_and_grow_with_q_and_k():
    build.build()
    ws = _lib.lib().eat_embed_search_ws_bytes
    Qs, ks = [1, 2, 15, 16, 17, 64, 1024], [1, 2, 10, 64, 127, 128]
    table = np.array([[ws(Q, k) for k in ks] for Q in Qs])
    assert bool((table > 0).all())
    assert bool((np.diff(table, axis=0) >= 0).all()) and bool((np.diff(table, axis=1) >= 0).all())
    # room for (score, index) lists of k entries from every block, for a whole group of queries
    assert ws(16, 128) >= 8 * ops.SEARCH_GROUP * ops.SEARCH_BLOCKS * 128
    for Q, k in ((0, 5), (1025, 5), (5, 0), (5, 129)):
        assert ws(Q, k) == -1


def test_the_geometry_that_ops_quotes_is_the_kernels():
    with open(os.path.join(ROOT, "efficientat_amd", "csrc", "search.hip")) as f:
        src = f.read()
    assert int(re.search(r"constexpr int kBlocks = (\d+);", src).group(1)) == ops.SEARCH_BLOCKS
    assert int(re.search(r"constexpr int kMaxGroup = (\d+);", src).group(1)) == ops.SEARCH_GROUP
    assert int(re.search(r"constexpr int kThreads = (\d+);", src).group(1)) == 8 * 64
    assert re.search(r"constexpr int rows_per_wave\(int G\) \{ return 8; \}", src)
    assert all(ops.search_tile_rows(g) == 8 * 8 for g in (1, 2, 4, 8, 16))
    k_max, q_max = re.search(r"constexpr int kMaxK = (\d+), kMaxQ = (\d+);", src).groups()
    assert (int(k_max), int(q_max)) == (ops.SEARCH_MAX_K, ops.SEARCH_MAX_Q)


def _brute(bank, queries, k, skip):
    """Python sort of (-score, index) pairs, scores by a plain loop."""
    out = []
    N = len(bank)
    for q, vec in enumerate(queries):
        qn = R.normalize_ref([vec])[0]
        lo, hi = (0, 0) if skip is None else (min(max(skip[q][0], 0), N), min(max(skip[q][1], 0), N))
        pairs = []
        for n, row in enumerate(R.normalize_ref(bank)):
            if not lo <= n < hi:
                pairs.append((-float(sum(a * b for a, b in zip(qn, row))), n))
        pairs.sort()
        pairs = pairs[:k] + [(np.inf, -1)] * (k - len(pairs))
        out.append(pairs)
    return np.array([[-s for s, _ in p] for p in out]), np.array([[n for _, n in p] for p in out])


@pytest.mark.parametrize("k", [1, 3, 9])
def test_the_reference_is_a_brute_force_sort(k):
    rng = np.random.default_rng(5)
    bank = np.clip(0.75 + rng.standard_normal((7, 3)), 0, None)
    bank[4] = bank[1]                       # an exact tie
    bank[6] = bank[1]                       # and a third copy: identical rows score identically, whatever the summation
    bank[2] = 0.0                           # a zero row: score 0, not NaN
    queries = np.clip(0.75 + rng.standard_normal((4, 3)), 0, None)
    queries[3] = 0.0
    for skip in (None, [[0, 0], [1, 5], [-3, 100], [5, 2]]):
        s, i = R.search_ref(bank, queries, k, skip)
        bs, bi = _brute(bank, queries, k, skip)
        assert np.array_equal(i, bi) and np.allclose(s, bs, rtol=0, atol=1e-15) and not bool(np.isnan(s).any())
    s, i = R.search_ref(bank, queries, k)
    assert list(i[3]) == list(range(min(k, 7))) + [-1] * max(0, k - 7) and bool((s[3][:min(k, 7)] == 0.0).all())
    where1, where4 = np.flatnonzero(i[0] == 1), np.flatnonzero(i[0] == 4)
    if len(where1) and len(where4):
        assert where4[0] == where1[0] + 1 and s[0][where1[0]] == s[0][where4[0]]
    s, i = R.search_ref(bank, queries, k, [[-3, 100]] * 4)
    assert bool((i == -1).all()) and bool(np.isneginf(s).all())


def _cpu_index():
    rng = np.random.default_rng(2)
    index = retrieval.EmbeddingIndex(5, meta={"kind": "timestamps", "layers": [0, 3], "clip_seconds": 1.0, "hop_ms": 50.0,
                                              "width_ms": 160.0})
    rows = [rng.standard_normal((n, 5)).astype(np.float32) for n in (3, 1, 70)]
    assert index.add(rows[0], "a.wav", [0.0, 50.0, 100.0]) == (0, 3)
    assert index.add(torch.from_numpy(rows[1]), "b.wav", [0.0]) == (3, 4)
    assert index.add(rows[2], "dir/c d.wav", np.arange(70) * 50.0) == (4, 74)
    return index, np.concatenate(rows)


def test_index_on_the_cpu_keeps_books_saves_and_loads_bit_for_bit(tmp_path):
    index, rows = _cpu_index()
    assert len(index) == 74 and index.device is None and index.names == ["a.wav", "b.wav", "dir/c d.wav"]
    assert index.row_range("b.wav") == (3, 4) and index.bank.shape == (74, 5)
    assert np.array_equal(index.bank.numpy(), rows)                       # without a device the rows are stored as given
    assert index.file_ids.tolist() == [0] * 3 + [1] + [2] * 70 and index.time_ms[5] == 50.0
    with pytest.raises(ValueError, match="'a.wav' is in the index already"):
        index.add(rows[:2], "a.wav", [0.0, 1.0])
    with pytest.raises(ValueError, match=r"must be \(n >= 1, 5\)"):
        index.add(rows[:2, :4], "e.wav", [0.0, 1.0])
    with pytest.raises(ValueError, match="must be 2 finite values >= 0"):
        index.add(rows[:2], "e.wav", [0.0, -1.0])
    with pytest.raises(ValueError, match="scene rows into an index of timestamps rows"):
        index.add(rows[:2], "e.wav")
    with pytest.raises(ValueError, match="one non-empty line"):
        index.add(rows[:2], "e\n.wav", [0.0, 1.0])
    with pytest.raises(ValueError, match="no file named 'zzz'"):
        index.row_range("zzz")
    with pytest.raises(_lib.EatHipError, match="needs the index on a GPU"):
        index.search(rows[:1], 3)
    assert len(index) == 74

    path = str(tmp_path / "idx")
    index.save(path)
    assert sorted(os.listdir(path)) == ["emb.npy", "file.npy", "meta.json", "names.txt", "time_ms.npy"]
    with open(os.path.join(path, "meta.json")) as f:
        meta = json.load(f)
    assert meta == {"version": 1, "D": 5, "kind": "timestamps", "model_name": None, "layers": [0, 3], "clip_seconds": 1.0,
                    "hop_ms": 50.0, "width_ms": 160.0}
    back = retrieval.EmbeddingIndex.load(path)
    assert back.device is None and back.D == 5 and back.meta == index.meta and back.names == index.names and len(back) == 74
    assert back.bank.numpy().tobytes() == rows.tobytes()
    assert np.array_equal(back.file_ids, index.file_ids) and back.file_ids.dtype == np.int32
    assert np.array_equal(back.time_ms, index.time_ms) and back.time_ms.dtype == np.float64
    assert [back.row_range(n) for n in back.names] == [(0, 3), (3, 4), (4, 74)]
    assert back.add(rows[:1], "later.wav", [0.0]) == (74, 75)               # a loaded index grows like any other


def test_hits_name_the_file_and_time_and_drop_the_empty_slots():
    index, _ = _cpu_index()
    score = torch.tensor([[0.9, 0.5, -np.inf], [1.0, -np.inf, -np.inf]])
    rows = torch.tensor([[5, 3, -1], [0, -1, -1]], dtype=torch.int32)
    assert index.hits(score, rows) == [[{"name": "dir/c d.wav", "time_ms": 50.0, "row": 5, "score": pytest.approx(0.9)},
                                        {"name": "b.wav", "time_ms": 0.0, "row": 3, "score": 0.5}],
                                       [{"name": "a.wav", "time_ms": 0.0, "row": 0, "score": 1.0}]]
    with pytest.raises(ValueError, match=r"outside \[-1, 74\)"):
        index.hits(score, torch.tensor([[5, 3, 74], [0, -1, -1]], dtype=torch.int32))
    scene = retrieval.EmbeddingIndex(2)
    scene.add([[1.0, 0.0]], "x")
    assert scene.meta["kind"] == "scene" and scene.hits([[0.25]], [[0]]) == [[{"name": "x", "time_ms": None, "row": 0, "score": 0.25}]]


def test_an_extractor_of_another_shape_is_refused():
    index, _ = _cpu_index()

    class Extractor:
        scene_embedding_size, layers, clip_seconds = 5, [0, 3], 1.0

    index.check_extractor(Extractor())
    for field, value in (("scene_embedding_size", 6), ("layers", [0, 4]), ("clip_seconds", 10.0)):
        other = Extractor()
        setattr(other, field, value)
        with pytest.raises(ValueError, match="do not compare"):
            index.check_extractor(other)


def test_load_names_the_path_for_each_malformed_directory(tmp_path):
    index, rows = _cpu_index()
    good = str(tmp_path / "good")
    index.save(good)

    def broken(name, **files):
        """A copy of the good directory with some files replaced (None: removed)."""
        path = str(tmp_path / name)
        os.makedirs(path)
        for f in os.listdir(good):
            with open(os.path.join(good, f), "rb") as src:
                data = src.read()
            if f in files and files[f] is None:
                continue
            if f in files and isinstance(files[f], (bytes, str)):
                data = files[f] if isinstance(files[f], bytes) else files[f].encode()
            with open(os.path.join(path, f), "wb") as dst:
                dst.write(data)
            if f in files and isinstance(files[f], np.ndarray):
                np.save(os.path.join(path, f), files[f])
        return path

    with open(os.path.join(good, "meta.json")) as f:
        meta = json.load(f)
    file_ids, times = index.file_ids.copy(), index.time_ms.copy()
    swapped = file_ids.copy()
    swapped[1], swapped[3] = 1, 0                           # a row of b.wav inside a.wav
    nan_rows = rows.copy()
    nan_rows[7, 2] = np.nan
    cases = [("no_emb", {"emb.npy": None}, "emb.npy is missing"),
             ("no_meta", {"meta.json": None}, "meta.json is missing"),
             ("no_names", {"names.txt": None}, "names.txt is missing"),
             ("meta_text", {"meta.json": "{"}, "meta.json is not JSON"),
             ("meta_keys", {"meta.json": json.dumps({k: v for k, v in meta.items() if k != "layers"})}, "exactly the entries"),
             ("meta_version", {"meta.json": json.dumps(dict(meta, version=2))}, "version 2"),
             ("meta_kind", {"meta.json": json.dumps(dict(meta, kind="frames"))}, "kind in"),
             ("meta_d", {"meta.json": json.dumps(dict(meta, D=6))}, r"emb.npy must be \(N, 6\) float32"),
             ("emb_f64", {"emb.npy": rows.astype(np.float64)}, r"emb.npy must be \(N, 5\) float32"),
             ("emb_nan", {"emb.npy": nan_rows}, "not finite"),
             ("emb_garbage", {"emb.npy": b"not an array"}, "emb.npy is unreadable"),
             ("file_short", {"file.npy": file_ids[:-1]}, r"file.npy must be \(74,\) int32"),
             ("file_i64", {"file.npy": file_ids.astype(np.int64)}, r"file.npy must be \(74,\) int32"),
             ("file_range", {"file.npy": np.where(file_ids == 2, 3, file_ids).astype(np.int32)}, r"outside \[0, 3\)"),
             ("file_split", {"file.npy": swapped}, "must be contiguous"),
             ("file_unused", {"names.txt": "a.wav\nb.wav\ndir/c d.wav\nnever.wav\n"}, "every file must have rows"),
             ("time_f32", {"time_ms.npy": times.astype(np.float32)}, r"time_ms.npy must be \(74,\) float64"),
             ("time_scene", {"time_ms.npy": np.where(np.arange(74) == 9, -1.0, times)}, "times >= 0 otherwise"),
             ("names_twice", {"names.txt": "a.wav\nb.wav\na.wav\n"}, "repeated name"),
             ("names_cut", {"names.txt": "a.wav\nb.wav\ndir/c d.wav"}, "does not end with a newline")]
    for name, files, match in cases:
        path = broken(name, **files)
        with pytest.raises(ValueError, match=match) as e:
            retrieval.EmbeddingIndex.load(path)
        assert path in str(e.value), name
    assert len(retrieval.EmbeddingIndex.load(good)) == 74


def test_skip_tables_are_validated_on_the_host():
    t = ops.check_skip([[0, 5], [7, 2]], 2)
    assert t.dtype == torch.int32 and t.tolist() == [[0, 5], [7, 2]] and t.is_contiguous()
    assert ops.check_skip(np.array([[-5, 2 ** 31 - 1]]), 1).tolist() == [[-5, 2 ** 31 - 1]]
    for skip, Q, match in (([[0, 5]], 2, r"skip must be \(2, 2\)"), ([0, 5], 1, r"skip must be \(1, 2\)"),
                           ([[0.0, 5.0]], 1, "must be integers"), ([[0, 2 ** 31]], 1, "must fit int32"),
                           ([[0, 1], [2]], 2, "ragged")):
        with pytest.raises(_lib.EatHipError, match=match):
            ops.check_skip(skip, Q)


def test_command_line_argument_errors(capsys):
    for argv, match in ((["query", "--audio_path", "q.wav"], "--index"),
                        (["index", "--audio_path", "a.wav"], "--out"),
                        (["index", "--out", "idx"], "--audio_path"),
                        (["index", "--audio_path", "a.wav", "a.wav", "--out", "idx"], "names a file twice"),
                        (["query", "--index", "idx", "--audio_path", "q.wav", "--k", "0"], r"--k must lie in \[1, 128\]"),
                        (["query", "--index", "idx", "--audio_path", "q.wav", "--k", "129"], r"--k must lie in \[1, 128\]"),
                        (["index", "--audio_path", "a.wav", "--out", "idx", "--hop_ms", "0"], "must be positive"),
                        (["query", "--index", "idx", "--audio_path", "q.wav", "--layers", "x"], "invalid int value"),
                        (["frobnicate"], "invalid choice"), ([], "required")):
        with pytest.raises(SystemExit) as e:
            search.parse(argv)
        assert e.value.code == 2
        assert re.search(match, capsys.readouterr().err), argv
    args = search.parse(["query", "--index", "idx", "--audio_path", "q.wav", "r.wav", "--layers", "0", "16", "--exclude_self", "--json"])
    assert args.k == 10 and args.layers == [0, 16] and args.exclude_self and args.json and args.audio_path == ["q.wav", "r.wav"]
    args = search.parse(["index", "--audio_path", "a.wav", "--out", "idx", "--timestamps"])
    assert args.timestamps and (args.hop_ms, args.width_ms, args.layers) == (50.0, 160.0, None)
