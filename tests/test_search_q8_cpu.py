"""Host side of the 8-bit search index: the header include/eat_search_q8.h with its argument checks, the emulation
(tests/search_q8_ref.py) against a brute-force loop, `EmbeddingIndex(storage="q8")` on the CPU - bookkeeping, save and load -
and the command line's --storage and `convert`."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

from efficientat_amd import _lib, build, ops, retrieval, search
from tests import search_q8_ref as R8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"eat_rows_quantize_q8", "eat_embed_search_q8_ws_bytes", "eat_embed_search_q8"}


def test_the_q8_header_parses_and_is_disjoint_from_the_other_headers():
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    with open(os.path.join(ROOT, "include", "eat_search_q8.h")) as f:
        protos = _lib.parse_prototypes(f.read())
    assert protos == _lib.SEARCH_Q8_PROTOTYPES
    assert set(protos) == NAMES
    assert protos["eat_rows_quantize_q8"] == (I, [P, L, I, I, P, L, P, P])
    assert protos["eat_embed_search_q8_ws_bytes"] == (L, [I, I])
    assert protos["eat_embed_search_q8"] == (I, [P, L, P, L, I, P, L, P, I, I, P, P, L, P, P, P])
    others = [v for k, v in vars(_lib).items() if k.endswith("PROTOTYPES") and k != "SEARCH_Q8_PROTOTYPES"]
    assert len(others) >= 11 and not any(set(protos) & set(o) for o in others)
    assert os.path.samefile(_lib.SEARCH_Q8_HEADER_PATH, os.path.join(ROOT, "include", "eat_search_q8.h"))


def test_the_library_exports_and_binds_the_q8_entry_points():
    build.build()
    assert "search_q8.hip" in build.SOURCES
    for name in NAMES:
        fn = getattr(_lib.lib(), name)
        restype, args = _lib.SEARCH_Q8_PROTOTYPES[name]
        assert list(fn.argtypes) == args and fn.restype is restype


def test_every_argument_error_is_raised_before_anything_touches_the_device():
    build.build()
    big = 2 ** 40
    # (N, D, Q, k, ld, qld, ws_bytes)
    for (N, D, Q, k, ld, qld, ws), match in (((10, 8, 1, 0, 16, 16, big), r"k=0 lies outside \[1, 128\]"),
                                             ((10, 8, 1, 129, 16, 16, big), r"k=129 lies outside \[1, 128\]"),
                                             ((10, 8, 0, 5, 16, 16, big), r"Q=0 lies outside \[1, 1024\]"),
                                             ((10, 8, 1025, 5, 16, 16, big), r"Q=1025 lies outside \[1, 1024\]"),
                                             ((0, 8, 1, 5, 16, 16, big), r"N=0 lies outside \[1, 2147483647\]"),
                                             ((2 ** 31, 8, 1, 5, 16, 16, big), r"N=2147483648 lies outside \[1, 2147483647\]"),
                                             ((10, 0, 1, 5, 16, 16, big), r"D=0 lies outside \[1, 131072\]"),
                                             ((10, 131073, 1, 5, 131088, 131088, big), r"D=131073 lies outside \[1, 131072\]"),
                                             ((10, 17, 1, 5, 16, 32, big), r"ld=16 is below D=17"),
                                             ((10, 17, 1, 5, 32, 16, big), r"qld=16 is below D=17"),
                                             ((10, 8, 1, 5, 24, 16, big), r"ld=24 is no multiple of 16"),
                                             ((10, 8, 1, 5, 16, 40, big), r"qld=40 is no multiple of 16"),
                                             ((10, 8, 3, 5, 16, 16, 0), r"ws_bytes=0 is below eat_embed_search_q8_ws_bytes\(Q=3, k=5\) = \d+"),
                                             ((10, 8, 3, 5, 16, 16, -1), r"ws_bytes=-1 is below")):
        with pytest.raises(_lib.EatHipError, match=match):
            _lib.call("eat_embed_search_q8", None, ld, None, N, D, None, qld, None, Q, k, None, None, ws, None, None, None)
    need = _lib.lib().eat_embed_search_q8_ws_bytes(3, 5)
    with pytest.raises(_lib.EatHipError, match=rf"ws_bytes={need - 1} is below eat_embed_search_q8_ws_bytes\(Q=3, k=5\) = {need}"):
        _lib.call("eat_embed_search_q8", None, 16, None, 10, 8, None, 16, None, 3, 5, None, None, need - 1, None, None, None)
    for (N, D, ld), match in (((-1, 8, 16), r"need N >= 0 \(got -1\)"), ((4, 0, 16), r"D=0 lies outside \[1, 131072\]"),
                              ((4, 131073, 131088), r"D=131073 lies outside"), ((4, 20, 16), r"ld=16 is below D=20"),
                              ((4, 20, 36), r"ld=36 is no multiple of 16")):
        with pytest.raises(_lib.EatHipError, match=match):
            _lib.call("eat_rows_quantize_q8", None, N, D, 1, None, ld, None, None)
    _lib.call("eat_rows_quantize_q8", None, 0, 8, 1, None, 16, None, None)          # N == 0: nothing is launched


def test_workspace_bytes_are_positive_and_grow_with_q_and_k():
    build.build()
    ws = _lib.lib().eat_embed_search_q8_ws_bytes
    Qs, ks = [1, 2, 15, 16, 17, 63, 64, 65, 1024], [1, 2, 10, 64, 127, 128]
    table = np.array([[ws(Q, k) for k in ks] for Q in Qs])
    assert bool((table > 0).all())
    assert bool((np.diff(table, axis=0) >= 0).all()) and bool((np.diff(table, axis=1) >= 0).all())
    assert ws(64, 128) >= 8 * ops.SEARCH_Q8_GROUP * ops.SEARCH_Q8_BLOCKS * 128
    for Q, k in ((0, 5), (1025, 5), (5, 0), (5, 129)):
        assert ws(Q, k) == -1


def test_the_geometry_that_ops_quotes_is_the_kernels():
    with open(os.path.join(ROOT, "efficientat_amd", "csrc", "search_q8.hip")) as f:
        src = f.read()
    assert int(re.search(r"constexpr int kBlocks = (\d+);", src).group(1)) == ops.SEARCH_Q8_BLOCKS
    assert int(re.search(r"constexpr int kMaxGroup = (\d+);", src).group(1)) == ops.SEARCH_Q8_GROUP
    assert int(re.search(r"constexpr int kThreads = (\d+);", src).group(1)) * 16 // 64 == ops.SEARCH_Q8_TILE_ROWS
    assert re.search(r"constexpr int kTileRows = 16 \* kWaves;", src)
    k_max, q_max, d_max = re.search(r"constexpr int kMaxK = (\d+), kMaxQ = (\d+), kMaxD = (\d+);", src).groups()
    assert (int(k_max), int(q_max), int(d_max)) == (ops.SEARCH_MAX_K, ops.SEARCH_MAX_Q, ops.SEARCH_Q8_MAX_D)
    assert [ops.q8_ld(D) for D in (1, 15, 16, 17, 2184)] == [16, 16, 16, 32, 2192]


def _brute(x, xq, k, skip):
    """The definition by plain Python loops over float32 scalars."""
    f = np.float32

    def quant(row):
        amax = max((abs(f(v)) for v in row), default=f(0))
        scale = f(amax) / f(127.0)
        return [0 if amax == 0 else int(np.rint(f(v) / scale)) for v in row], f(scale)

    bank, queries = [quant(r) for r in x], [quant(r) for r in xq]
    N = len(bank)
    out_s, out_i = [], []
    for q, (cq, sq) in enumerate(queries):
        lo, hi = (0, 0) if skip is None else (min(max(skip[q][0], 0), N), min(max(skip[q][1], 0), N))
        pairs = []
        for n, (cn, sn) in enumerate(bank):
            if not lo <= n < hi:
                acc = sum(a * b for a, b in zip(cq, cn))
                pairs.append((-float(f(acc) * f(sq * sn)), n))
        pairs.sort()
        pairs = pairs[:k] + [(np.inf, -1)] * (k - len(pairs))
        out_s.append([-s for s, _ in pairs])
        out_i.append([n for _, n in pairs])
    return np.array(out_s, dtype=np.float32), np.array(out_i, dtype=np.int32)


@pytest.mark.parametrize("k", [1, 3, 9])
def test_the_emulation_is_a_brute_force_loop(k):
    rng = np.random.default_rng(5)
    x = np.clip(0.75 + rng.standard_normal((7, 3)), 0, None).astype(np.float32)
    x[4] = x[1]                             # an exact tie
    x[6] = 2.0 * x[1]                       # the same codes at another scale
    x[2] = 0.0                              # a zero row: scale 0, score 0, not NaN
    xq = np.clip(0.75 + rng.standard_normal((4, 3)), 0, None).astype(np.float32)
    xq[3] = 0.0
    codes, scale = R8.quantize_ref(x)
    qcodes, qscale = R8.quantize_ref(xq)
    assert scale[2] == 0 and not codes[2].any() and qscale[3] == 0 and np.array_equal(codes[4], codes[1]) and scale[4] == scale[1]
    assert np.array_equal(codes[6], codes[1]) and int(np.abs(codes).max()) == 127 and codes.dtype == np.int8
    for skip in (None, [[0, 0], [1, 5], [-3, 100], [5, 2]]):
        s, i = R8.search_q8_ref(codes, scale, qcodes, qscale, k, skip)
        bs, bi = _brute(x, xq, k, skip)
        assert np.array_equal(i, bi) and np.array_equal(s.view(np.int32), bs.view(np.int32)) and not bool(np.isnan(s).any())
    s, i = R8.search_q8_ref(codes, scale, qcodes, qscale, k)
    assert list(i[3]) == list(range(min(k, 7))) + [-1] * max(0, k - 7) and bool((s[3][:min(k, 7)] == 0.0).all())
    where1, where4 = np.flatnonzero(i[0] == 1), np.flatnonzero(i[0] == 4)
    if len(where1) and len(where4):
        assert where4[0] == where1[0] + 1 and s[0][where1[0]] == s[0][where4[0]]
    s, i = R8.search_q8_ref(codes, scale, qcodes, qscale, k, [[-3, 100]] * 4)
    assert bool((i == -1).all()) and bool(np.isneginf(s).all())


def test_the_emulated_normalisation_is_fp32_with_fused_multiply_adds():
    # one rounding per multiply-add: 1 + 2^-12 squared is 1 + 2^-11 + 2^-24, and the last bit survives only in a fused sum
    a = np.array([1 + 2.0 ** -12], dtype=np.float32)
    assert R8.fma_f32(a, a, np.array([-1.0], dtype=np.float32))[0] == np.float32(2.0 ** -11 + 2.0 ** -24)
    # what rounding twice (to float64, then to float32) gets wrong: (1 + 2^-23)(1 - 2^-23) 2^-24 + (1 + 2^-23) lies 2^-70 below
    # the midpoint of two float32 values; in float64 it becomes the midpoint, and the tie then goes up to the even neighbour
    f = np.float32
    a, b, c = np.array([f(1) + f(2.0 ** -23)]), np.array([(f(1) - f(2.0 ** -23)) * f(2.0 ** -24)]), np.array([f(1) + f(2.0 ** -23)])
    assert a.dtype == b.dtype == c.dtype == np.float32
    assert (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f)[0] == f(1 + 2.0 ** -22)
    assert R8.fma_f32(a, b, c)[0] == f(1 + 2.0 ** -23)
    x = np.random.default_rng(3).standard_normal((9, 300)).astype(np.float32)
    x[4] = 0.0
    out = R8.normalize_f32(x)
    assert out.dtype == np.float32 and not out[4].any() and not bool(np.isnan(out).any())
    norms = np.sqrt((out.astype(np.float64) ** 2).sum(axis=1))
    assert bool((np.abs(np.delete(norms, 4) - 1.0) <= 2e-6).all())
    codes, scale = R8.quantize_ref(x, normalize=True)
    again, scale2 = R8.quantize_ref(out)
    assert np.array_equal(codes, again) and np.array_equal(scale, scale2)


META = {"kind": "timestamps", "layers": [0, 3], "clip_seconds": 1.0, "hop_ms": 50.0, "width_ms": 160.0}


def _q8_directory(path):
    """A q8 index directory as `save` writes it, from the emulation: 74 rows of 5 values of three files."""
    rng = np.random.default_rng(2)
    rows = rng.standard_normal((74, 5)).astype(np.float32)
    rows[9] = 0.0
    codes, scale = R8.quantize_ref(rows, normalize=True)
    os.makedirs(path)
    np.save(os.path.join(path, "codes.npy"), codes)
    np.save(os.path.join(path, "scale.npy"), scale)
    np.save(os.path.join(path, "file.npy"), np.array([0] * 3 + [1] + [2] * 70, dtype=np.int32))
    np.save(os.path.join(path, "time_ms.npy"), np.concatenate((np.arange(3), [0], np.arange(70))) * 50.0)
    with open(os.path.join(path, "names.txt"), "w") as f:
        f.write("a.wav\nb.wav\ndir/c d.wav\n")
    meta = dict({"version": 2, "D": 5, "model_name": None}, **META, storage="q8")
    with open(os.path.join(path, "meta.json"), "w") as f:
        json.dump(meta, f)
    return codes, scale, meta


def test_a_q8_index_on_the_cpu_keeps_books_saves_and_loads_bit_for_bit(tmp_path):
    first = str(tmp_path / "first")
    codes, scale, meta = _q8_directory(first)
    index = retrieval.EmbeddingIndex.load(first)
    assert index.storage == "q8" and index.device is None and len(index) == 74 and index.D == 5
    assert index.names == ["a.wav", "b.wav", "dir/c d.wav"] and index.row_range("dir/c d.wav") == (4, 74)
    assert index.codes.shape == (74, 16) and index.codes.dtype == torch.int8 and index.scales.shape == (74,)
    assert np.array_equal(index.codes.numpy()[:, :5], codes) and not index.codes.numpy()[:, 5:].any()
    assert index.scales.numpy().tobytes() == scale.tobytes()
    with pytest.raises(ValueError, match="storage 'q8' has no fp32 bank"):
        index.bank
    with pytest.raises(_lib.EatHipError, match="needs a q8 index on a GPU"):
        index.add(np.ones((2, 5), dtype=np.float32), "e.wav", [0.0, 1.0])
    with pytest.raises(ValueError, match="'a.wav' is in the index already"):
        index.add(np.ones((2, 5), dtype=np.float32), "a.wav", [0.0, 1.0])
    with pytest.raises(_lib.EatHipError, match="needs the index on a GPU"):
        index.search(np.ones((1, 5), dtype=np.float32), 3)
    assert len(index) == 74 and index.names == ["a.wav", "b.wav", "dir/c d.wav"]
    hits = index.hits(torch.tensor([[0.5, -np.inf]]), torch.tensor([[5, -1]], dtype=torch.int32))
    assert hits == [[{"name": "dir/c d.wav", "time_ms": 50.0, "row": 5, "score": 0.5}]]

    second = str(tmp_path / "second")
    index.save(second)
    assert sorted(os.listdir(second)) == ["codes.npy", "file.npy", "meta.json", "names.txt", "scale.npy", "time_ms.npy"]
    with open(os.path.join(second, "meta.json")) as f:
        assert json.load(f) == meta == {"version": 2, "D": 5, "kind": "timestamps", "model_name": None, "layers": [0, 3],
                                        "clip_seconds": 1.0, "hop_ms": 50.0, "width_ms": 160.0, "storage": "q8"}
    for name in ("codes.npy", "scale.npy", "file.npy", "time_ms.npy"):
        a, b = np.load(os.path.join(first, name)), np.load(os.path.join(second, name))
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    assert np.load(os.path.join(second, "codes.npy")).shape == (74, 5)                       # unpadded on disk
    back = retrieval.EmbeddingIndex.load(second)
    assert back.storage == "q8" and back.meta == index.meta and back.meta["version"] == 2
    assert torch.equal(back.codes, index.codes) and torch.equal(back.scales, index.scales)
    assert [back.row_range(n) for n in back.names] == [(0, 3), (3, 4), (4, 74)]

    with pytest.raises(ValueError, match="storage must be one of"):
        retrieval.EmbeddingIndex(5, storage="int4")
    with pytest.raises(ValueError, match="q8 storage needs D <= 131072"):
        retrieval.EmbeddingIndex(131073, storage="q8")
    empty = retrieval.EmbeddingIndex(5, storage="q8")
    assert len(empty) == 0 and empty.codes.shape == (0, 16) and empty.meta["version"] == 2
    with pytest.raises(ValueError, match="needs an fp32 index on a GPU"):
        empty.quantized()


def test_an_fp32_index_still_writes_version_1_and_the_same_five_files(tmp_path):
    index = retrieval.EmbeddingIndex(5, meta=META)
    rows = np.random.default_rng(1).standard_normal((4, 5)).astype(np.float32)
    index.add(rows, "a.wav", np.arange(4) * 50.0)
    assert index.storage == "fp32"
    with pytest.raises(ValueError, match="storage 'fp32' has no codes"):
        index.codes
    with pytest.raises(ValueError, match="storage 'fp32' has no scales"):
        index.scales
    path = str(tmp_path / "idx")
    index.save(path)
    assert sorted(os.listdir(path)) == ["emb.npy", "file.npy", "meta.json", "names.txt", "time_ms.npy"]
    with open(os.path.join(path, "meta.json")) as f:
        text = f.read()
    assert json.loads(text) == {"version": 1, "D": 5, "kind": "timestamps", "model_name": None, "layers": [0, 3],
                                "clip_seconds": 1.0, "hop_ms": 50.0, "width_ms": 160.0}
    assert list(json.loads(text)) == list(retrieval.META_KEYS) and text.endswith("}\n")
    assert np.load(os.path.join(path, "emb.npy")).tobytes() == rows.tobytes()
    back = retrieval.EmbeddingIndex.load(path)
    assert back.storage == "fp32" and back.meta["version"] == 1


def test_load_names_the_path_for_each_malformed_q8_directory(tmp_path):
    good = str(tmp_path / "good")
    codes, scale, meta = _q8_directory(good)

    def broken(name, **files):
        """A copy of the good directory with some files replaced (None: removed)."""
        path = str(tmp_path / name)
        os.makedirs(path)
        for f in os.listdir(good):
            if f in files and files[f] is None:
                continue
            if f in files and isinstance(files[f], np.ndarray):
                np.save(os.path.join(path, f), files[f])
                continue
            with open(os.path.join(good, f), "rb") as src:
                data = src.read()
            if f in files:
                data = files[f].encode()
            with open(os.path.join(path, f), "wb") as dst:
                dst.write(data)
        return path

    def changed(arr, at, value):
        out = arr.copy()
        out[at] = value
        return out

    v1_keys = {k: v for k, v in meta.items() if k != "storage"}
    cases = [("no_scale", {"scale.npy": None}, "scale.npy is missing"),
             ("no_codes", {"codes.npy": None}, "codes.npy is missing"),
             ("code_128", {"codes.npy": changed(codes, (7, 2), -128)}, r"codes.npy holds a code outside \[-127, 127\]"),
             ("scale_neg", {"scale.npy": changed(scale, 3, -scale[3])}, "scale.npy holds a scale that is negative or not finite"),
             ("scale_nan", {"scale.npy": changed(scale, 3, np.nan)}, "scale.npy holds a scale that is negative or not finite"),
             ("scale_inf", {"scale.npy": changed(scale, 3, np.inf)}, "negative or not finite"),
             ("scale_zero", {"scale.npy": changed(scale, 3, 0.0)}, "non-zero codes in a row whose scale is 0"),
             ("codes_i16", {"codes.npy": codes.astype(np.int16)}, r"codes.npy must be \(N, 5\) int8"),
             ("codes_u8", {"codes.npy": codes.astype(np.uint8)}, r"codes.npy must be \(N, 5\) int8"),
             ("codes_padded", {"codes.npy": R8.padded(codes)}, r"codes.npy must be \(N, 5\) int8"),
             ("codes_flat", {"codes.npy": codes.reshape(-1)}, r"codes.npy must be \(N, 5\) int8"),
             ("scale_f64", {"scale.npy": scale.astype(np.float64)}, r"scale.npy must be \(74,\) float32"),
             ("scale_short", {"scale.npy": scale[:-1]}, r"scale.npy must be \(74,\) float32"),
             ("scale_2d", {"scale.npy": scale[:, None]}, r"scale.npy must be \(74,\) float32"),
             ("codes_short", {"codes.npy": codes[:-1]}, r"scale.npy must be \(73,\) float32"),
             ("file_short", {"file.npy": np.load(os.path.join(good, "file.npy"))[:-1]}, r"file.npy must be \(74,\) int32"),
             ("storage_other", {"meta.json": json.dumps(dict(meta, storage="fp32"))}, "version 2 needs storage = 'q8'"),
             ("storage_int4", {"meta.json": json.dumps(dict(meta, storage="int4"))}, "version 2 needs storage = 'q8'"),
             ("v2_without_storage", {"meta.json": json.dumps(v1_keys)}, "version 2 must hold exactly the entries"),
             ("v1_with_storage", {"meta.json": json.dumps(dict(meta, version=1))}, "exactly the entries"),
             ("v3", {"meta.json": json.dumps(dict(v1_keys, version=3))}, "has version 3, this code reads version 1"),
             ("meta_d", {"meta.json": json.dumps(dict(meta, D=6))}, r"codes.npy must be \(N, 6\) int8")]
    for name, files, match in cases:
        path = broken(name, **files)
        with pytest.raises(ValueError, match=match) as e:
            retrieval.EmbeddingIndex.load(path)
        assert path in str(e.value), name
    # a q8 directory has no emb.npy, an fp32 directory no codes.npy: neither loads as the other
    path = broken("as_v1", **{"meta.json": json.dumps(dict(v1_keys, version=1))})
    with pytest.raises(ValueError, match="emb.npy is missing"):
        retrieval.EmbeddingIndex.load(path)
    assert len(retrieval.EmbeddingIndex.load(good)) == 74


def test_command_line_storage_and_convert(capsys):
    for argv, match in ((["index", "--audio_path", "a.wav", "--out", "idx", "--storage", "int4"], "invalid choice"),
                        (["query", "--index", "idx", "--audio_path", "q.wav", "--storage", "q8"], "unrecognized arguments"),
                        (["convert", "--index", "idx", "--out", "out"], "--storage"),
                        (["convert", "--index", "idx", "--out", "out", "--storage", "fp32"], "invalid choice"),
                        (["convert", "--out", "out", "--storage", "q8"], "--index"),
                        (["convert", "--index", "idx", "--storage", "q8"], "--out")):
        with pytest.raises(SystemExit) as e:
            search.parse(argv)
        assert e.value.code == 2
        assert re.search(match, capsys.readouterr().err), argv
    assert search.parse(["index", "--audio_path", "a.wav", "--out", "idx"]).storage == "fp32"
    assert search.parse(["index", "--audio_path", "a.wav", "--out", "idx", "--storage", "q8", "--timestamps"]).storage == "q8"
    args = search.parse(["convert", "--index", "idx", "--out", "out", "--storage", "q8"])
    assert (args.command, args.index, args.out, args.storage) == ("convert", "idx", "out", "q8")
