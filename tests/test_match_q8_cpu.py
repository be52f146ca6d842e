"""Host side of occurrence search over the 8-bit index (include/eat_match_q8.h): the header with its argument checks and
workspace query, the reference on its own, and what `EmbeddingIndex.find(allow_q8=...)` does without a device.

The reference composes two existing ones and adds nothing: tests/search_q8_ref.py (`quantize_ref` -> `scores_q8_ref`: the
score bits of eat_embed_search_q8) -> tests/match_ref.py in float32 (the bits of eat_embed_match given the row scores).
Here it is held against `match_ref` in fp64 on the normalised rows.  The bound of a window mean is the mean over the window
of the per-pair bound derived in tests/test_gpu_search_q8_kernels.py,
    sq sn (0.5 sum |cq| + 0.5 sum |cn| + 0.25 D) + 2e-5:
the error of a mean is at most the mean of its terms' errors, and the 2e-5 also covers the L fp32 additions and the
division (3.4e-7 at L = 200 in tests/test_gpu_match_kernels.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from efficientat_amd import _lib, build, ops, retrieval, search
from tests import match_ref as M
from tests import search_q8_ref as R8
from tests import search_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"eat_embed_match_q8_ws_bytes", "eat_embed_match_q8"}


def _values(n, D, seed):
    return np.clip(0.75 + np.random.default_rng(seed).standard_normal((n, D)), 0, None).astype(np.float32)


def pair_bounds(codes, scale, qcodes, qscale, D):
    """(L, N) fp64: the per-pair bound of |q8 score - cosine|."""
    c, sn, cq, sq = (np.asarray(t).astype(np.float64) for t in (codes, scale, qcodes, qscale))
    return sq[:, None] * sn[None, :] * (0.5 * np.abs(cq).sum(axis=1)[:, None] + 0.5 * np.abs(c).sum(axis=1)[None, :] + 0.25 * D) + 2e-5


def q8_reference(bank, queries):
    """Normalised fp32 rows -> (S (L, N) float32 of the codes, S64 (L, N) fp64 of the rows, window means of the pair bound)."""
    D = bank.shape[1]
    codes, scale = R8.quantize_ref(bank, normalize=False)
    qcodes, qscale = R8.quantize_ref(queries, normalize=False)
    S = R8.scores_q8_ref(codes, scale, qcodes, qscale)
    S64 = R.scores_ref(bank, queries, normalize=False)
    return S, S64, M.window_means(pair_bounds(codes, scale, qcodes, qscale, D))


def test_the_header_parses_and_is_disjoint_from_the_other_headers():
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_float
    with open(os.path.join(ROOT, "include", "eat_match_q8.h")) as f:
        protos = _lib.parse_prototypes(f.read())
    assert protos == _lib.MATCH_Q8_PROTOTYPES
    assert set(protos) == NAMES
    assert protos["eat_embed_match_q8_ws_bytes"] == (L, [L, I, I])
    assert protos["eat_embed_match_q8"] == (I, [P, L, P, L, I, P, I, P, L, P, I, I, I, F, I, I, P, L, P, P, P])
    others = [v for k, v in vars(_lib).items() if k.endswith("PROTOTYPES") and k != "MATCH_Q8_PROTOTYPES"]
    assert len(others) >= 13 and not any(set(protos) & set(o) for o in others)
    assert len(_lib.PROTOTYPES) == 139
    assert os.path.samefile(_lib.MATCH_Q8_HEADER_PATH, os.path.join(ROOT, "include", "eat_match_q8.h"))
    assert "match_q8.hip" in build.SOURCES
    with open(os.path.join(ROOT, "efficientat_amd", "csrc", "match_q8.hip")) as f:
        src = f.read()
    assert int(re.search(r"constexpr int kMaxGroup = (\d+);", src).group(1)) == ops.MATCH_Q8_GROUP == 64
    # the scan has the geometry of the q8 search: nothing else ties the two files' constants together
    with open(os.path.join(ROOT, "efficientat_amd", "csrc", "search_q8.hip")) as f:
        search_src = f.read()
    for line in (r"constexpr int kBlocks = (\d+);", r"constexpr int kThreads = (\d+);", r"constexpr int kTileRows = (16 \* kWaves);",
                 r"constexpr int kMaxGroup = (\d+);", r"constexpr long long kLdsBytes = (160 \* 1024);"):
        assert re.search(line, src).group(1) == re.search(line, search_src).group(1), line
    assert int(re.search(r"constexpr int kBlocks = (\d+);", src).group(1)) == ops.SEARCH_Q8_BLOCKS
    assert int(re.search(r"constexpr int kThreads = (\d+);", src).group(1)) * 16 // 64 == ops.SEARCH_Q8_TILE_ROWS
    k_max, l_max, s_max, d_max = re.search(r"constexpr int kMaxK = (\d+), kMaxL = (\d+), kMaxSep = (\d+), kMaxD = (\d+);", src).groups()
    assert (int(k_max), int(l_max), int(s_max), int(d_max)) == (ops.SEARCH_MAX_K, ops.MATCH_MAX_L, ops.MATCH_MAX_SEP, ops.SEARCH_Q8_MAX_D)


def test_the_library_binds_the_entry_points_and_refuses_every_limit_before_the_device():
    build.build()
    for name in NAMES:
        fn = getattr(_lib.lib(), name)
        restype, args = _lib.MATCH_Q8_PROTOTYPES[name]
        assert list(fn.argtypes) == args and fn.restype is restype
    ws = _lib.lib().eat_embed_match_q8_ws_bytes
    big = 2 ** 50
    ok = dict(N=10, D=20, F=2, L=3, k=5, sep=4, min_score=0.0, ws=big, ld=32, qld=32)
    for change, match in ((dict(L=0), r"L=0 lies outside \[1, 1024\]"), (dict(L=1025), r"L=1025 lies outside \[1, 1024\]"),
                          (dict(k=0), r"k=0 lies outside \[1, 128\]"), (dict(k=129), r"k=129 lies outside \[1, 128\]"),
                          (dict(sep=-1), r"sep=-1 lies outside \[0, 4096\]"), (dict(sep=4097), r"sep=4097 lies outside \[0, 4096\]"),
                          (dict(N=0), r"N=0 lies outside \[1, 2147483647\]"), (dict(N=2 ** 31), r"N=2147483648 lies outside"),
                          (dict(F=0), r"need F >= 1 \(got 0\)"),
                          (dict(D=0), r"D=0 lies outside \[1, 131072\]"),
                          (dict(D=131073, ld=131088, qld=131088), r"D=131073 lies outside \[1, 131072\]"),
                          (dict(min_score=float("nan")), "min_score is NaN"),
                          (dict(ld=16), r"ld=16 is below D=20"), (dict(qld=16), r"qld=16 is below D=20"),
                          (dict(ld=40), r"ld=40 is no multiple of 16"), (dict(qld=24), r"qld=24 is no multiple of 16"),
                          (dict(ws=0), r"ws_bytes=0 is below eat_embed_match_q8_ws_bytes\(N=10, L=3, k=5\) = \d+"),
                          (dict(ws=ws(10, 3, 5) - 1), "is below eat_embed_match_q8_ws_bytes")):
        a = dict(ok, **change)
        with pytest.raises(_lib.EatHipError, match=r"eat_embed_match_q8 failed \(-\d+\): eat_embed_match_q8: .*" + match):
            _lib.call("eat_embed_match_q8", None, a["ld"], None, a["N"], a["D"], None, a["F"], None, a["qld"], None, a["L"], a["k"],
                      a["sep"], a["min_score"], 0, 0, None, a["ws"], None, None, None)


def test_the_workspace_query():
    ws = _lib.lib().eat_embed_match_q8_ws_bytes
    for N, L, k in ((0, 3, 5), (2 ** 31, 3, 5), (10, 0, 5), (10, 1025, 5), (10, 3, 0), (10, 3, 129)):
        assert ws(N, L, k) == -1
    Ns, Ls, ks = [1, 2, 63, 1000, 2 ** 31 - 1], [1, 2, 15, 16, 17, 63, 64, 65, 1024], [1, 10, 128]
    table = np.array([[[ws(N, L, k) for k in ks] for L in Ls] for N in Ns], dtype=np.int64)
    assert bool((table > 0).all()) and all(bool((np.diff(table, axis=a) >= 0).all()) for a in range(3))
    assert bool((table % 16 == 0).all())
    # room for the group's scores and the running sums of every start row; one size from a full group on
    assert ws(1000, 64, 1) >= 4 * 1000 * 65 and ws(1000, 1024, 1) == ws(1000, 64, 1)
    assert ws(1000, 63, 1) < ws(1000, 64, 1) == ws(1000, 65, 1)


@pytest.mark.parametrize("shape", [(130, 200, 1000), (2184, 64, 600)], ids=lambda s: "x".join(map(str, s)))
def test_the_reference_lies_within_the_quantisation_bound_of_fp64(shape):
    D, L, N = shape
    bank = R.normalize_ref(_values(N, D, seed=D)).astype(np.float32)
    queries = R.normalize_ref(_values(L, D, seed=D + 1)).astype(np.float32)
    S, S64, bound = q8_reference(bank, queries)
    assert S.dtype == np.float32 and S64.dtype == np.float64
    m, m64 = M.window_means(S), M.window_means(S64)
    valid = ~np.isnan(m64)
    assert int(valid.sum()) == N - L + 1 and np.array_equal(valid, ~np.isnan(m)) and m.dtype == np.float32
    err = np.abs(m[valid].astype(np.float64) - m64[valid])
    print(f"MATCH_Q8 reference {shape}: largest |m - m64| = {float(err.max()):.3e}, "
          f"largest share of the bound {float((err / bound[valid]).max()):.4f}")
    assert bool((err <= bound[valid]).all())
    # and the peaks it names are fp64's wherever fp64 leaves no doubt: the best place is the same
    seg = [0, N // 3, N]
    want = M.match_ref(S64, seg, 5, L)
    got = M.match_ref(S, seg, 5, L)
    assert got[0].dtype == np.float32 and got[1][0] == want[1][0]


def _smooth(rows, width=9):
    kernel = np.ones(width) / width
    return np.stack([np.convolve(rows[:, d], kernel, mode="same") for d in range(rows.shape[1])], axis=1)


def planted_scene():
    """The scene of tests/test_gpu_match.py: (bank (600, 48) normalised fp32, clip (20, 48) normalised fp32, seg)."""
    D, ROWS, L, AT = 48, 300, 20, 100
    rng = np.random.default_rng(5)
    clip = _smooth(rng.standard_normal((L + 8, D)))[4:4 + L]
    files = []
    for noise in (0.0, 0.03):
        rows = _smooth(rng.standard_normal((ROWS, D)))
        rows[AT:AT + L] = clip + noise * rng.standard_normal((L, D))
        files.append(rows.astype(np.float32))
    bank = R8.normalize_f32(np.concatenate(files))
    return bank, R8.normalize_f32(clip.astype(np.float32)), [0, ROWS, 2 * ROWS]


PLANTED_ROWS = [100, 400, 54, 32, 499, 259, 312, 171, 337, 144]


def test_the_planted_scene():
    bank, clip, seg = planted_scene()
    S, S64, bound = q8_reference(bank, clip)
    k, sep = 10, 20
    score, row = M.match_ref(S, seg, k, sep)
    score64, row64 = M.match_ref(S64, seg, k, sep)
    assert row.tolist() == row64.tolist() == PLANTED_ROWS
    err = np.abs(score.astype(np.float64) - score64)
    print(f"MATCH_Q8 planted: q8 {score[:2].tolist()} fp64 {score64[:2].tolist()}; largest |m - m64| = {float(err.max()):.3e}")
    assert bool((err <= bound[row]).all())
    assert abs(float(score[0]) - 0.99950) < 5e-6 and abs(float(score[1]) - 0.99488) < 5e-6
    assert abs(float(score64[0]) - 1.0) < 5e-6 and abs(float(score64[1]) - 0.99522) < 5e-6


def test_find_on_a_q8_index_without_a_device():
    meta = {"kind": "timestamps", "hop_ms": 50.0, "width_ms": 160.0}
    rows = np.random.default_rng(0).standard_normal((6, 5)).astype(np.float32)
    q8 = retrieval.EmbeddingIndex(5, meta=meta, storage="q8")
    with pytest.raises(ValueError, match="needs the fp32 index"):
        q8.find(rows[:2], 3)
    with pytest.raises(ValueError, match="allow_q8=True"):
        q8.find(rows[:2], 3, allow_q8=False)
    with pytest.raises(_lib.EatHipError, match="find needs the index on a GPU"):
        q8.find(rows[:2], 3, allow_q8=True)
    # on an fp32 index the keyword changes nothing
    fp32 = retrieval.EmbeddingIndex(5, meta=meta)
    fp32.add(rows, "a.wav", np.arange(6) * 50.0)
    for allow in (False, True):
        with pytest.raises(_lib.EatHipError, match="find needs the index on a GPU"):
            fp32.find(rows[:2], 3, allow_q8=allow)
    scene = retrieval.EmbeddingIndex(5, storage="q8")
    with pytest.raises(ValueError, match="an index of kind 'timestamps'"):
        scene.find(rows[:2], 3, allow_q8=True)
    # operands on the host are refused by the wrapper as well
    import torch
    with pytest.raises(_lib.EatHipError, match="bank codes must be a contiguous"):
        ops.embed_match_q8(torch.zeros((4, 16), dtype=torch.int8), torch.zeros(4), 5, torch.tensor([0, 4], dtype=torch.int32),
                           torch.zeros((2, 16), dtype=torch.int8), torch.zeros(2), 3, 2)


def test_the_find_command_parses_as_before():
    base = ["find", "--index", "idx", "--audio_path", "q.wav"]
    args = search.parse(base + ["r.wav"])
    assert (args.command, args.k, args.min_separation_ms, args.min_score, args.query) == ("find", 10, None, None, "sequence")
    assert not args.exclude_self and not args.json and args.audio_path == ["q.wav", "r.wav"] and args.model_name == "mn10_as"
    assert sorted(vars(args)) == sorted(vars(search.parse(base)))
    assert not hasattr(args, "allow_q8") and not hasattr(args, "storage")
