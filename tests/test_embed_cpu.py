"""Host side of the embedding extractor (efficientat_amd/embeddings.py): the segment plan against a brute-force
enumeration of column centres, the segment-table check, the third header include/eat_embed.h with its argument checks, and
the window weights of the scene embedding."""
import ctypes
import os

import numpy as np
import pytest

from efficientat_amd import _lib, build, embeddings, ops
from tests import embed_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_MS = 10.0          # 1000 * 320 / 32000

T_MELS = [1, 17, 101, 501, 1000]
PLANS = [(50, 160), (10, 10), (500, 1000), (33, 70)]


@pytest.mark.parametrize("hop_ms,width_ms", PLANS)
@pytest.mark.parametrize("T_mel", T_MELS)
def test_segment_plan_is_the_enumeration_of_column_centres(T_mel, hop_ms, width_ms):
    T_l = R.mn_widths(T_mel)
    lo, hi, t = embeddings.segment_plan(T_mel, T_l, R.MN_STRIDES, FRAME_MS, hop_ms, width_ms)
    blo, bhi, bt = R.segment_plan_brute(T_mel, T_l, R.MN_STRIDES, FRAME_MS, hop_ms, width_ms)
    n = (T_mel - 1) * 10 // hop_ms + 1                       # exact integer form of floor((T_mel - 1) frame_ms / hop_ms) + 1
    assert lo.shape == hi.shape == (17, n) and t.shape == (n,)
    assert lo.dtype == np.int32 and hi.dtype == np.int32 and t.dtype == np.float64
    assert np.array_equal(t, np.arange(n) * float(hop_ms)) and np.array_equal(t, bt)
    assert np.array_equal(lo, blo) and np.array_equal(hi, bhi)
    assert bool((hi > lo).all()) and bool((lo >= 0).all()) and bool((hi <= np.asarray(T_l)[:, None]).all())
    ops.check_segments(lo, hi, T_l)


def test_segment_plan_named_cases():
    T_l = R.mn_widths(1000)
    assert T_l == [500, 500, 250, 250, 125, 125, 125, 63, 63, 63, 63, 63, 63, 32, 32, 32, 32]
    lo, hi, t = embeddings.segment_plan(1000, T_l, R.MN_STRIDES, FRAME_MS)          # the defaults: (50, 160)
    assert len(t) == 200 and t[-1] == 9950.0
    # timestamp 4 (200 ms, frame 20) owns frames [12, 28): columns 6..13 at stride 2, 3..6 at 4, 2..3 at 8, 1 at 16, none at 32
    assert (lo[0, 4], hi[0, 4]) == (6, 14) and (lo[2, 4], hi[2, 4]) == (3, 7) and (lo[4, 4], hi[4, 4]) == (2, 4)
    assert (lo[7, 4], hi[7, 4]) == (1, 2)
    assert (lo[13, 4], hi[13, 4]) == (1, 2)                   # nearest: 20 / 32 + 0.5 = 1.125
    assert (lo[0, 0], hi[0, 0]) == (0, 4)                     # clamped at the left edge: frames [-8, 8)
    assert bool((hi[0, 2:199] - lo[0, 2:199] == 8).all()) and bool((lo[0, 1:] < hi[0, :-1]).all())      # neighbours overlap
    with pytest.raises(ValueError, match="one T_l"):
        embeddings.segment_plan(100, [50, 25], [2], FRAME_MS)
    with pytest.raises(ValueError, match="must be positive"):
        embeddings.segment_plan(100, [50], [2], FRAME_MS, hop_ms=0)


def test_segment_tables_are_validated_on_the_host():
    lo, hi = ops.check_segments([[0, 1], [2, 0]], [[1, 5], [3, 3]], [5, 3])
    assert lo.tolist() == [[0, 1], [2, 0]] and hi.tolist() == [[1, 5], [3, 3]]
    assert not lo.dtype.is_floating_point and lo.is_contiguous() and hi.is_contiguous()
    for lo, hi, T_l, match in (([[0, 2]], [[1, 2]], [5], "need 0 <= lo < hi"),            # lo == hi
                               ([[0, 3]], [[1, 2]], [5], "need 0 <= lo < hi"),            # lo > hi
                               ([[0, 1]], [[1, 6]], [5], "need 0 <= lo < hi"),            # hi > T_l
                               ([[0, 1], [0, 1]], [[1, 5], [1, 4]], [5, 3], "segment 1 of map 1"),
                               ([[-1, 1]], [[1, 2]], [5], "need 0 <= lo < hi"),           # negative lo
                               ([[0, 1], [0]], [[1, 2], [1]], [5, 5], "ragged"),
                               ([[0, 1]], [[1, 2, 3]], [5], "ragged"),
                               ([[0, 1]], [[1, 2]], [5, 5], "ragged"),                    # one row, two maps
                               ([0, 1], [1, 2], [5], "ragged"),
                               ([[]], [[]], [5], "ragged")):
        with pytest.raises(_lib.EatHipError, match=match):
            ops.check_segments(lo, hi, T_l)


def test_the_embed_header_parses_and_is_disjoint_from_the_other_headers():
    P, I = ctypes.c_void_p, ctypes.c_int
    with open(os.path.join(ROOT, "include", "eat_embed.h")) as f:
        protos = _lib.parse_prototypes(f.read())
    assert protos == _lib.EMBED_PROTOTYPES
    assert set(protos) == {"eat_embed_pool"}
    assert protos["eat_embed_pool"] == (I, [P, P, P, I, I, I, I, P, P])
    assert not set(protos) & set(_lib.PROTOTYPES) and not set(protos) & set(_lib.TAG_PROTOTYPES)
    assert os.path.samefile(_lib.EMBED_HEADER_PATH, os.path.join(ROOT, "include", "eat_embed.h"))


def test_the_library_exports_and_binds_the_embed_entry_point():
    build.build()
    fn = getattr(_lib.lib(), "eat_embed_pool")
    restype, args = _lib.EMBED_PROTOTYPES["eat_embed_pool"]
    assert list(fn.argtypes) == args and fn.restype is restype
    assert "embed.hip" in build.SOURCES
    # argument checks that return before anything touches the device: (n_maps, B, n_seg, D)
    for shape, match in (((0, 1, 1, 8), r"n_maps=0 lies outside \[1, 64\]"), ((65, 1, 1, 8), r"n_maps=65 lies outside \[1, 64\]"),
                         ((1, 0, 1, 8), r"need B >= 1 \(got 0\)"), ((1, 1, 0, 8), r"need n_seg >= 1 \(got 0\)"),
                         ((1, 1, 1, 0), r"need D >= 1 \(got 0\)"), ((1, -3, 1, 8), r"need B >= 1 \(got -3\)"),
                         ((1, 2 ** 31 - 1, 1, 8), r"exceed the grid limit of 2147483647: chunk the call over B")):
        with pytest.raises(_lib.EatHipError, match=match):
            _lib.call("eat_embed_pool", None, None, None, *shape, None, None)


@pytest.mark.parametrize("W", [32000, 7])
def test_window_weights_of_the_scene_embedding(W):
    lengths = [1, W - 1, W, W + 1, 2 * W + 7]
    counts, w = embeddings.window_weights(lengths, W)
    assert counts == [1, 1, 1, 2, 3] and w.dtype == np.float64 and len(w) == sum(counts)
    want = [[1.0], [1.0], [1.0], [W / (W + 1), 1 / (W + 1)], [W / (2 * W + 7), W / (2 * W + 7), 7 / (2 * W + 7)]]
    row = 0
    for c, ws, n in zip(counts, want, lengths):
        got = w[row:row + c]
        assert np.allclose(got, ws, rtol=1e-15, atol=0) and abs(got.sum() - 1.0) < 1e-15
        # the weight of a window is the share of the recording's samples it holds
        valid = np.clip(n - np.arange(c) * W, 0, W)
        assert np.allclose(got, valid / n, rtol=1e-15, atol=0)
        row += c
