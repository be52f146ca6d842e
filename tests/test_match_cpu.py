"""Host side of occurrence search: the reference tests/match_ref.py against a brute-force reading of the definition
(include/eat_match.h), the header with its argument checks, the `find` command's arguments, and what
`EmbeddingIndex.find` refuses without a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from efficientat_amd import _lib, build, ops, retrieval, search
from tests import match_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"eat_embed_match_ws_bytes", "eat_embed_match"}


def match_brute(S, seg, k, sep, min_score=-np.inf, skip=None):
    """The definition, read literally with Python loops, in the dtype of S."""
    S = np.asarray(S)
    L, N = S.shape
    lo, hi = (0, 0) if skip is None else (min(max(int(skip[0]), 0), N), min(max(int(skip[1]), 0), N))
    file_of, m, cand = {}, {}, set()
    for f in range(len(seg) - 1):
        for n in range(seg[f], seg[f + 1]):
            file_of[n] = f
            if n + L <= seg[f + 1]:                                    # valid
                acc = S[0, n]
                for j in range(1, L):
                    acc = acc + S[j, n + j]
                m[n] = acc / S.dtype.type(L)
                if not lo <= n < hi:
                    cand.add(n)

    def better(a, b):
        return m[a] > m[b] or (m[a] == m[b] and a < b)

    peaks = [n for n in sorted(cand)
             if all(better(n, x) for x in cand if x != n and file_of[x] == file_of[n] and abs(x - n) <= sep)]
    peaks = [n for n in peaks if m[n] >= S.dtype.type(min_score)]
    peaks.sort(key=lambda n: (-float(m[n]), n))
    peaks = peaks[:k]
    score = np.array([m[n] for n in peaks] + [-np.inf] * (k - len(peaks)), dtype=S.dtype)
    return score, np.array(peaks + [-1] * (k - len(peaks)), dtype=np.int64)


def _same(a, b):
    return a[0].dtype == b[0].dtype and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_reference_is_the_definition_on_random_tiny_cases(dtype):
    """Scores on a grid of eighths: exact ties between neighbours, between files and with the threshold are common."""
    rng = np.random.default_rng(3)
    for case in range(300):
        L = int(rng.integers(1, 5))
        lens = rng.integers(1, 9, size=int(rng.integers(1, 5)))
        seg = [0] + np.cumsum(lens).tolist()
        N = seg[-1]
        S = (rng.integers(0, 8, size=(L, N)) / 8.0).astype(dtype)
        k, sep = int(rng.integers(1, 7)), int(rng.integers(0, 12))
        skip = None if case % 3 == 0 else sorted(rng.integers(-3, N + 4, size=2).tolist())
        min_score = -np.inf if case % 2 else float(rng.integers(0, 8)) / 8.0
        assert _same(M.match_ref(S, seg, k, sep, min_score, skip), match_brute(S, seg, k, sep, min_score, skip)), (case, seg, L, sep, skip)


def test_the_reference_on_the_named_edge_cases():
    f32 = np.float32
    # ties: equal means, the lower row wins within sep; with sep = 0 both stay, lower row first
    S = np.array([[0.5, 0.5, 0.25, 0.5]], dtype=f32)
    assert M.match_ref(S, [0, 4], 4, 1)[1].tolist() == [0, 3, -1, -1]
    assert M.match_ref(S, [0, 4], 4, 0)[1].tolist() == [0, 1, 3, 2]
    # local maxima, not greedy suppression: 1 is dropped by 2, and 0, weaker than 1 within sep, is dropped although 1 is;
    # 4 ties with 3, which is the lower row and itself dropped by 2
    S = np.array([[0.1, 0.2, 0.3, 0.0, 0.0]], dtype=f32)
    assert M.match_ref(S, [0, 5], 5, 1)[1].tolist() == [2, -1, -1, -1, -1]
    # a file shorter than L has no start row; a file of exactly L rows has one
    S = np.ones((3, 9), dtype=f32)
    S[:, 2:5] = 0.5
    score, index = M.match_ref(S, [0, 2, 5, 9], 5, 0)
    assert index.tolist() == [5, 6, 2, -1, -1] and score[:3].tolist() == [1.0, 1.0, 0.5]
    # sep larger than a file: one peak per file with a start row
    assert M.match_ref(S, [0, 2, 5, 9], 5, 4096)[1].tolist() == [5, 2, -1, -1, -1]
    # a neighbour across a file boundary does not suppress
    S = np.array([[0.1, 0.9, 0.8, 0.1]], dtype=f32)
    assert M.match_ref(S, [0, 2, 4], 4, 3)[1].tolist() == [1, 2, -1, -1]
    assert M.match_ref(S, [0, 4], 4, 3)[1].tolist() == [1, -1, -1, -1]
    # an excluded row is neither returned nor does it suppress; the range is clamped
    assert M.match_ref(S, [0, 4], 4, 3, skip=(1, 2))[1].tolist() == [2, -1, -1, -1]
    assert M.match_ref(S, [0, 4], 4, 0, skip=(-7, 2))[1].tolist() == [2, 3, -1, -1]
    assert M.match_ref(S, [0, 4], 4, 0, skip=(3, 1))[1].tolist() == [1, 2, 0, 3]
    # min_score keeps m >= it; a peak below it is dropped, what it suppressed stays dropped
    assert M.match_ref(S, [0, 4], 4, 1, min_score=0.85)[1].tolist() == [1, -1, -1, -1]
    assert M.match_ref(S, [0, 4], 4, 0, min_score=0.8)[0].tolist()[:2] == [f32(0.9), f32(0.8)]
    # float32 means are sequential fp32 sums and one IEEE division; float64 ones differ
    S = np.array([[0.1] * 3, [0.7] * 3, [0.3] * 3], dtype=f32)
    want = (f32(0.1) + f32(0.7) + f32(0.3)) / f32(3)
    got = M.match_ref(S, [0, 3], 1, 0)[0]
    assert got.dtype == f32 and got[0] == want and M.match_ref(S.astype(np.float64), [0, 3], 1, 0)[0].dtype == np.float64


def test_the_match_header_parses_and_is_disjoint_from_the_other_headers():
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
    with open(os.path.join(ROOT, "include", "eat_match.h")) as f:
        protos = _lib.parse_prototypes(f.read())
    assert protos == _lib.MATCH_PROTOTYPES
    assert set(protos) == NAMES
    assert protos["eat_embed_match_ws_bytes"] == (L, [L, I, I])
    assert protos["eat_embed_match"] == (I, [P, L, I, P, I, P, I, I, I, F, I, I, P, L, P, P, P])
    others = [v for k, v in vars(_lib).items() if k.endswith("PROTOTYPES") and k != "MATCH_PROTOTYPES"]
    assert len(others) >= 12 and not any(set(protos) & set(o) for o in others)
    assert os.path.samefile(_lib.MATCH_HEADER_PATH, os.path.join(ROOT, "include", "eat_match.h"))
    assert "match.hip" in build.SOURCES


def test_the_library_binds_the_entry_points_and_refuses_every_limit_before_the_device():
    build.build()
    for name in NAMES:
        fn = getattr(_lib.lib(), name)
        restype, args = _lib.MATCH_PROTOTYPES[name]
        assert list(fn.argtypes) == args and fn.restype is restype
    big = 2 ** 50
    ok = dict(N=10, D=8, F=2, L=3, k=5, sep=4, min_score=0.0, ws=big)
    for change, match in ((dict(L=0), r"L=0 lies outside \[1, 1024\]"), (dict(L=1025), r"L=1025 lies outside \[1, 1024\]"),
                          (dict(k=0), r"k=0 lies outside \[1, 128\]"), (dict(k=129), r"k=129 lies outside \[1, 128\]"),
                          (dict(sep=-1), r"sep=-1 lies outside \[0, 4096\]"), (dict(sep=4097), r"sep=4097 lies outside \[0, 4096\]"),
                          (dict(N=0), r"N=0 lies outside \[1, 2147483647\]"), (dict(N=2 ** 31), r"N=2147483648 lies outside"),
                          (dict(F=0), r"need F >= 1 \(got 0\)"), (dict(D=0), r"need D >= 1 \(got 0\)"),
                          (dict(min_score=float("nan")), "min_score is NaN"),
                          (dict(ws=0), r"ws_bytes=0 is below eat_embed_match_ws_bytes\(N=10, L=3, k=5\) = \d+"),
                          (dict(ws=_lib.lib().eat_embed_match_ws_bytes(10, 3, 5) - 1), "is below eat_embed_match_ws_bytes")):
        a = dict(ok, **change)
        with pytest.raises(_lib.EatHipError, match=match):
            _lib.call("eat_embed_match", None, a["N"], a["D"], None, a["F"], None, a["L"], a["k"], a["sep"], a["min_score"], 0, 0,
                      None, a["ws"], None, None, None)
    ws = _lib.lib().eat_embed_match_ws_bytes
    for N, L, k in ((0, 3, 5), (2 ** 31, 3, 5), (10, 0, 5), (10, 1025, 5), (10, 3, 0), (10, 3, 129)):
        assert ws(N, L, k) == -1
    Ns, Ls, ks = [1, 2, 63, 1000, 2 ** 31 - 1], [1, 2, 15, 16, 17, 1024], [1, 10, 128]
    table = np.array([[[ws(N, L, k) for k in ks] for L in Ls] for N in Ns], dtype=np.int64)
    assert bool((table > 0).all()) and all(bool((np.diff(table, axis=a) >= 0).all()) for a in range(3))
    # room for the group's scores and the running sums of every start row
    assert ws(1000, 16, 1) >= 4 * 1000 * 17 and ws(1000, 1024, 1) == ws(1000, 16, 1)
    assert (ops.MATCH_MAX_L, ops.MATCH_MAX_SEP) == (1024, 4096)
    with open(os.path.join(ROOT, "efficientat_amd", "csrc", "match.hip")) as f:
        k_max, l_max, s_max = re.search(r"constexpr int kMaxK = (\d+), kMaxL = (\d+), kMaxSep = (\d+);", f.read()).groups()
    assert (int(k_max), int(l_max), int(s_max)) == (ops.SEARCH_MAX_K, ops.MATCH_MAX_L, ops.MATCH_MAX_SEP)


def test_find_command_arguments(capsys):
    base = ["find", "--index", "idx", "--audio_path", "q.wav"]
    for argv, match in ((["find", "--audio_path", "q.wav"], "--index"), (["find", "--index", "idx"], "--audio_path"),
                        (base + ["--k", "0"], r"--k must lie in \[1, 128\]"), (base + ["--k", "129"], r"--k must lie in \[1, 128\]"),
                        (base + ["--min_separation_ms", "-1"], "--min_separation_ms must be >= 0"),
                        (base + ["--min_score", "nan"], "--min_score must be a number"),
                        (base + ["--query", "both"], "invalid choice")):
        with pytest.raises(SystemExit) as e:
            search.parse(argv)
        assert e.value.code == 2
        assert re.search(match, capsys.readouterr().err), argv
    args = search.parse(base + ["r.wav"])
    assert (args.command, args.k, args.min_separation_ms, args.min_score, args.query) == ("find", 10, None, None, "sequence")
    assert not args.exclude_self and not args.json and args.audio_path == ["q.wav", "r.wav"] and args.model_name == "mn10_as"
    args = search.parse(base + ["--k", "3", "--min_separation_ms", "250", "--min_score", "0.5", "--exclude_self", "--query", "scene", "--json"])
    assert (args.k, args.min_separation_ms, args.min_score, args.query) == (3, 250.0, 0.5, "scene") and args.exclude_self and args.json
    # `query` is what it was
    assert not hasattr(search.parse(["query", "--index", "idx", "--audio_path", "q.wav"]), "min_score")


def test_what_find_refuses_without_a_device():
    meta = {"kind": "timestamps", "hop_ms": 50.0, "width_ms": 160.0}
    rows = np.random.default_rng(0).standard_normal((6, 5)).astype(np.float32)
    index = retrieval.EmbeddingIndex(5, meta=meta)
    index.add(rows, "a.wav", np.arange(6) * 50.0)
    with pytest.raises(_lib.EatHipError, match="find needs the index on a GPU"):
        index.find(rows[:2], 3)
    scene = retrieval.EmbeddingIndex(5)
    scene.add(rows[0], "x")
    with pytest.raises(ValueError, match="an index of kind 'timestamps'"):
        scene.find(rows[:2], 3)
    with pytest.raises(ValueError, match="needs the fp32 index"):
        retrieval.EmbeddingIndex(5, meta=meta, storage="q8").find(rows[:2], 3)
    # hits of a find: one list, each place with its end
    found = index.hits(torch.tensor([0.75, -np.inf]), torch.tensor([2, -1], dtype=torch.int32), query_rows=3)
    assert found == [{"name": "a.wav", "time_ms": 100.0, "row": 2, "score": 0.75, "end_ms": 250.0}]
    with pytest.raises(ValueError, match=r"the \(k,\) outputs of `find`"):
        index.hits(torch.zeros((1, 2)), torch.zeros((1, 2), dtype=torch.int32), query_rows=3)
    # the times of every file must step by hop_ms
    index._check_times()
    index.add(rows[:3], "b.wav", [0.0, 50.0, 150.0])
    with pytest.raises(ValueError, match="do not step by hop_ms = 50.0"):
        index._check_times()
    with pytest.raises(ValueError, match="records no hop_ms"):
        other = retrieval.EmbeddingIndex(5, meta={"kind": "timestamps"})
        other.add(rows, "a.wav", np.arange(6) * 50.0)
        other._check_times()
