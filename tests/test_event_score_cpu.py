"""Event-based scoring without a GPU: the numpy restatement on hand-built cases, the two serial matching orders against
each other, the tolerance rule, the threshold grid and choice, the operating-point file, the C header and its binding with
the argument checks that return before anything touches the device, and the host-side refusals of `ops.event_score`."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from efficientat_amd import _lib, build, ops, sed
from efficientat_amd._lib import EatHipError
from tests import event_score_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _n(refs, tols, ests, c):
    return len(R.match_ref_outer(refs, tols, ests, c))


# ---------------------------------------------------------------------------------------------------- the restatement
def test_matching_on_hand_built_cases():
    c = 10
    assert R.match_ref_outer([(100, 200)], [10], [(100, 200)], c) == [(0, 0)]                 # equal
    assert _n([(100, 200)], [10], [(110, 200)], c) == 1 and _n([(100, 200)], [10], [(111, 200)], c) == 0    # onset: c, c + 1
    assert _n([(100, 200)], [10], [(90, 200)], c) == 1 and _n([(100, 200)], [10], [(89, 200)], c) == 0
    assert _n([(100, 200)], [10], [(100, 210)], c) == 1 and _n([(100, 200)], [10], [(100, 211)], c) == 0    # offset: c, c + 1
    assert _n([(100, 200)], [10], [(100, 190)], c) == 1 and _n([(100, 200)], [10], [(100, 189)], c) == 0
    # tol from pct * length where that exceeds c: length 1000, pct 0.2 -> 200
    ev = np.asarray([[0, 0, 1000], [0, 0, 40]])
    assert R.tolerances(ev, c, 0.2) == [200, 10]
    assert _n([(0, 1000)], [200], [(0, 800)], c) == 1 and _n([(0, 1000)], [200], [(0, 799)], c) == 0
    assert _n([(0, 1000)], [200], [(0, 1200)], c) == 1 and _n([(0, 1000)], [200], [(0, 1201)], c) == 0
    # two overlapping references of one class compete for one estimate: the first row takes it
    assert R.match_ref_outer([(100, 200), (105, 205)], [10, 10], [(102, 203)], c) == [(0, 0)]
    # an estimate that two references could take: the first row takes it, the second takes the next estimate
    assert R.match_ref_outer([(100, 200), (108, 200)], [10, 10], [(95, 200), (104, 200)], c) == [(0, 0), (1, 1)]
    # ... and where the second reference fits that estimate alone it stays unmatched: the greedy answer, not the maximal one
    assert R.match_ref_outer([(100, 200), (100, 290)], [100, 10], [(98, 285), (110, 150)], c) == [(0, 0)]
    assert R.match_ref_outer([], [], [(0, 5)], c) == [] and R.match_ref_outer([(0, 5)], [10], [], c) == []


def test_score_ref_counts_events_in_samples_clipped_to_the_recording():
    # one recording of 5 frames, R = 10, 47 samples: the event [3, 5) frames spans samples [30, 47)
    filt = np.asarray([[0, 0, 0, 1, 1]], dtype=np.float32)
    rec = [(0, 1, 0, 5)]
    for off, want in ((47, 1), (50, 0)):
        out = R.score_ref(filt, rec, [47], 10, [[0, 30, off]], [0], [0, 1], 0, [0.5], [0.5])
        assert out.tolist() == [[[[want, 1]]]]
    assert R.to_samples([(419431, 419432)], 10240, 2 ** 40) == [(2 ** 32 + 6144, 2 ** 32 + 6144 + 10240)]


def test_reference_outer_and_estimate_outer_matching_agree():
    rng = np.random.default_rng(5)
    some = 0
    for _ in range(4000):
        c = int(rng.integers(0, 6))
        nr, ne = int(rng.integers(0, 7)), int(rng.integers(0, 7))
        refs = sorted((int(a), int(a) + int(d)) for a, d in zip(rng.integers(0, 30, nr), rng.integers(1, 12, nr)))
        refs.sort(key=lambda r: r[0])
        tols = [max(c, int(0.3 * (b - a))) for a, b in refs]
        on = np.sort(rng.integers(0, 30, ne))
        ests = [(int(a), int(a) + int(d)) for a, d in zip(on, rng.integers(1, 12, ne))]       # in onset order, overlaps allowed
        a, b = R.match_ref_outer(refs, tols, ests, c), R.match_est_outer(refs, tols, ests, c)
        assert sorted(a) == sorted(b)
        some += len(a)
    assert some > 2000


def test_event_tolerances_against_fp64_by_hand():
    ev = np.asarray([[0, 0, 10], [1, 5, 1005], [2, 7, 8], [0, 100, 100 + 33333], [0, 0, 2 ** 31 - 1]], dtype=np.int32)
    got = sed.event_tolerances(ev, 6400, 0.2)
    assert got.dtype == np.int32
    assert got.tolist() == [6400, 6400, 6400, 6666, int(np.floor(np.float64(0.2) * np.float64(2 ** 31 - 1)))]
    assert got.tolist() == R.tolerances(ev, 6400, 0.2)
    assert sed.event_tolerances(torch.from_numpy(ev), 0, 0.5).tolist() == [5, 500, 0, 16666, (2 ** 31 - 1) // 2]
    assert sed.event_tolerances(np.zeros((0, 3), dtype=np.int32), 5, 0.2).shape == (0,)
    assert sed.collar_samples(200, 32000) == 6400 and sed.collar_samples(0, 32000) == 0
    with pytest.raises(ValueError, match="negative"):
        sed.event_tolerances(ev, -1, 0.2)
    with pytest.raises(ValueError, match=r"\(E, 3\)"):
        sed.event_tolerances(np.zeros((3, 2), dtype=np.int32), 1, 0.2)


def test_threshold_grid_and_choice():
    hi, lo = sed.threshold_grid()
    assert hi.dtype == np.float32 and hi.shape == (49,) and np.array_equal(hi, lo)
    assert hi[0] == np.float32(0.02) and hi[24] == np.float32(0.5) and hi[48] == np.float32(0.98)
    hi, lo = sed.threshold_grid([0.5, 2e-38], 0.5)
    assert lo[0] == np.float32(0.25) and lo[1] == np.finfo(np.float32).tiny and bool((lo <= hi).all()) and bool((lo > 0).all())
    assert sed.threshold_grid(None, 0.0)[1].tolist() == [float(np.finfo(np.float32).tiny)] * 49
    for bad in ([], [0.0], [1.5], [float("nan")]):
        with pytest.raises(ValueError, match="thresholds"):
            sed.threshold_grid(bad)
    with pytest.raises(ValueError, match="low_ratio"):
        sed.threshold_grid(None, 1.5)
    # counts (V = 3, K = 4, 3): class 0 peaks at v = 1 and ties at v = 2 (the first wins); class 1 has nothing to score
    # anywhere and keeps the argument; class 2 has no reference and false positives only at v = 0; class 3 is best at v = 0
    counts = np.asarray([[[1, 1, 3], [0, 0, 0], [0, 2, 0], [5, 0, 0]],
                         [[3, 1, 1], [0, 0, 0], [0, 0, 0], [4, 0, 1]],
                         [[3, 1, 1], [0, 0, 0], [0, 0, 0], [0, 0, 5]]])
    hi, lo = sed.threshold_grid([0.2, 0.5, 0.8], 0.5)
    at, best, b_hi, b_lo = sed.pick_thresholds(counts, hi, lo, 0.6, 0.5)
    assert at == 1 and best.tolist() == [1, -1, 0, 0]
    assert b_hi.tolist() == [0.5, float(np.float32(0.6)), float(np.float32(0.2)), float(np.float32(0.2))]
    assert b_lo.tolist() == [0.25, float(np.float32(0.5) * np.float32(0.6)), float(lo[0]), float(lo[0])]
    f = sed.class_f1(counts)
    assert f[0, 0] == 2 / 6 and f[1, 0] == 6 / 8 and np.isnan(f[:, 1]).all() and f[0, 2] == 0 and np.isnan(f[1, 2])


# ---------------------------------------------------------------------------------------------------- operating points
def _result(K=3):
    return {"best_threshold": np.asarray([0.3, 0.5, 0.72], dtype=np.float32)[:K],
            "best_low_threshold": np.asarray([0.15, 0.25, 0.36], dtype=np.float32)[:K], "threshold": 0.5, "n_clips": 7, "n_ref": 19,
            "thresholds": sed.threshold_grid()[0], "macro_f1_best": 0.5, "micro_f1": 0.4, "micro_precision": 0.3,
            "micro_recall": 0.6, "macro_f1": 0.35, "macro_precision": 0.25, "macro_recall": 0.5,
            "settings": {"median_ms": 960.0, "min_duration_ms": 320.0, "max_gap_ms": 0.0, "taper": "uniform", "window_size": 10.24,
                         "hop_length": 5.12, "collar_ms": 200.0, "offset_pct": 0.2, "low_ratio": 0.5}}


def test_operating_points_round_trip(tmp_path):
    path = str(tmp_path / "sub" / "ops.json")
    classes = ["dog", "cat", "speech"]
    sed.save_operating_points(path, _result(), classes)
    got = sed.load_operating_points(path, classes=classes, n_classes=3)
    assert got["classes"] == classes
    assert got["threshold"].dtype == np.float32 and np.array_equal(got["threshold"], _result()["best_threshold"])
    assert np.array_equal(got["low_threshold"], _result()["best_low_threshold"])           # fp32 survives the decimal text
    assert (got["median_ms"], got["min_duration_ms"], got["max_gap_ms"], got["taper"]) == (960.0, 320.0, 0.0, "uniform")
    assert (got["window_size"], got["hop_length"]) == (10.24, 5.12)
    assert got["scoring"]["collar_ms"] == 200.0 and got["scoring"]["offset_pct"] == 0.2 and got["scores"]["macro_f1_best"] == 0.5
    with pytest.raises(ValueError, match="classes"):
        sed.save_operating_points(path, _result(), classes[:2])


def test_operating_points_errors_name_the_file(tmp_path):
    path = str(tmp_path / "ops.json")
    classes = ["dog", "cat", "speech"]
    good = sed.save_operating_points(path, _result(), classes)

    def refuse(match, classes_arg=None, n=None, **over):
        doc = dict(good)
        doc.update(over)
        for k, v in over.items():
            if v is None:
                del doc[k]
        with open(path, "w") as f:
            json.dump(doc, f)
        with pytest.raises(ValueError, match=match) as e:
            sed.load_operating_points(path, classes=classes_arg, n_classes=n)
        assert "ops.json" in str(e.value)

    refuse("K = 3 values", threshold=[0.5, 0.5])                              # wrong length
    refuse("K = 3 values", low_threshold=[0.1] * 4)
    refuse("4 are expected", n=4)
    refuse("not the expected names", classes_arg=["cat", "dog", "speech"])    # another class order
    refuse("0 < low_threshold <= threshold <= 1", threshold=[0.3, 0.5, 1.5])
    refuse("0 < low_threshold <= threshold <= 1", low_threshold=[0.15, 0.6, 0.36])
    refuse("0 < low_threshold <= threshold <= 1", low_threshold=[0.0, 0.25, 0.36])
    refuse("missing median_ms", median_ms=None)
    refuse("taper", taper="cosine")
    refuse("numbers", max_gap_ms="soon")
    refuse("not negative", min_duration_ms=-1.0)
    refuse("list of K", classes=[])
    with open(path, "w") as f:
        f.write("{ not json")
    with pytest.raises(ValueError, match="ops.json.*JSON"):
        sed.load_operating_points(path)
    with pytest.raises(ValueError, match="nothere.json"):
        sed.load_operating_points(str(tmp_path / "nothere.json"))


# ---------------------------------------------------------------------------------------------------- header
def test_the_event_score_header_parses_is_disjoint_from_the_other_headers_and_is_bound():
    P, I = ctypes.c_void_p, ctypes.c_int
    with open(os.path.join(ROOT, "include", "eat_event_score.h")) as f:
        protos = _lib.parse_prototypes(f.read())
    assert protos == _lib.EVENT_SCORE_PROTOTYPES
    assert set(protos) == {"eat_event_score"}
    assert protos["eat_event_score"] == (I, [P, I, I, P, I, P, I, P, P, P, I, I, P, P, I, I, I, P, P])
    others = [v for k, v in vars(_lib).items() if k.endswith("PROTOTYPES") and k != "EVENT_SCORE_PROTOTYPES"]
    assert len(others) >= 6
    for other in others:
        assert not set(protos) & set(other)
    assert "eat_event_score" not in _lib.exported_symbols()
    assert "event_score.hip" in build.SOURCES
    build.build()
    for name, (restype, args) in protos.items():
        fn = getattr(_lib.lib(), name)
        assert list(fn.argtypes) == args and fn.restype is restype, name
    # argument checks that return before anything touches the device: `one` is never dereferenced
    one = ctypes.c_void_p(16)

    def score(**kw):
        a = dict(filt=one, K=1, G_total=1, rec=one, n_rec=1, nsamp=one, R=1, ref=one, ref_tol=one, ro=one, n_ref=1, c=0, hi=one,
                 lo=one, V=1, max_gap=0, min_len=0, counts=one)
        a.update(kw)
        _lib.call("eat_event_score", *a.values(), None)

    for missing in ("filt", "rec", "nsamp", "ref", "ref_tol", "ro", "hi", "lo", "counts"):
        with pytest.raises(EatHipError, match="eat_event_score: missing operand"):
            score(**{missing: None})
    for bad in (dict(K=0), dict(G_total=0), dict(n_rec=0), dict(R=0), dict(V=0), dict(K=-1)):
        with pytest.raises(EatHipError, match="eat_event_score: need K, n_rec, G_total, R, V >= 1"):
            score(**bad)
    for bad in (dict(c=-1), dict(max_gap=-1), dict(min_len=-1), dict(n_ref=-1)):
        with pytest.raises(EatHipError, match="eat_event_score: need n_ref, c, max_gap, min_len >= 0"):
            score(**bad)
    with pytest.raises(EatHipError, match="exceed the grid limit"):
        score(n_rec=2 ** 16, K=2 ** 15)
    with pytest.raises(EatHipError, match="threshold pairs exceed"):
        score(V=64 * 65535 + 1)


# ---------------------------------------------------------------------------------------------------- ops refusals
REF = torch.tensor([[0, 0, 10], [0, 5, 50], [2, 49, 50], [1, 0, 30]], dtype=torch.int32)
TOL = torch.tensor([3, 9, 3, 6], dtype=torch.int32)
RO = torch.tensor([0, 3, 4, 4], dtype=torch.int64)


def test_event_refs_accepts_a_bank_table_and_refuses_every_violation():
    refs = ops.event_refs(REF, TOL, RO, 3)
    assert (refs.n_rec, refs.E, refs.K) == (3, 4, 3)
    assert ops.event_refs(REF.numpy(), TOL.numpy(), RO.numpy(), 3).E == 4
    empty = ops.event_refs(torch.zeros((0, 3), dtype=torch.int32), torch.zeros(0, dtype=torch.int32),
                           torch.zeros(3, dtype=torch.int64), 2)
    assert (empty.n_rec, empty.E) == (2, 0)
    for args, msg in (((REF.long(), TOL, RO, 3), r"\(E, 3\) int32"), ((REF[:, :2].contiguous(), TOL, RO, 3), r"\(E, 3\) int32"),
                      ((REF, TOL[:3], RO, 3), "ref_tol must be"), ((REF, TOL.long(), RO, 3), "ref_tol must be"),
                      ((REF, TOL, RO.int(), 3), "ro must be"), ((REF, TOL, RO[:1], 3), "ro must be"),
                      ((REF, TOL, torch.tensor([1, 3, 4, 4]), 3), "rise from 0 to E = 4"),
                      ((REF, TOL, torch.tensor([0, 3, 4, 3]), 3), "rise from 0 to E = 4"),
                      ((REF, TOL, torch.tensor([0, 4, 3, 4]), 3), "rise from 0 to E = 4"),
                      ((REF, TOL, RO, 2), "class outside"), ((REF, TOL, RO, 0), "K >= 1"),
                      ((REF, -TOL, RO, 3), "negative"),
                      ((torch.tensor([[0, 5, 50], [0, 0, 10]], dtype=torch.int32), TOL[:2], torch.tensor([0, 2]), 1), "out of order"),
                      ((torch.tensor([[1, 0, 10], [0, 0, 10]], dtype=torch.int32), TOL[:2], torch.tensor([0, 2]), 2), "out of order"),
                      ((torch.tensor([[0, 12, 10]], dtype=torch.int32), TOL[:1], torch.tensor([0, 1]), 1), "onset <= offset")):
        with pytest.raises(EatHipError, match="event_refs: .*" + msg):
            ops.event_refs(*args)
    # at most 64 reference events of one recording and class: the refusal names both
    n = ops.EVENT_SCORE_MAX_REF
    assert n >= 64
    many = torch.zeros((n + 3, 3), dtype=torch.int32)
    many[:, 0] = torch.tensor([0, 0] + [1] * (n + 1))
    many[:, 1] = torch.arange(n + 3)
    many[:, 2] = many[:, 1] + 1
    with pytest.raises(EatHipError, match=f"recording 1 holds {n + 1} reference events of class 1"):
        ops.event_refs(many, torch.zeros(n + 3, dtype=torch.int32), torch.tensor([0, 1, n + 3]), 2)
    assert ops.event_refs(many[:-1].contiguous(), torch.zeros(n + 2, dtype=torch.int32), torch.tensor([0, 1, n + 2]), 2).E == n + 2


def test_event_score_host_side_refusals():
    table = ops.detect_table([[0, 1, 0, 5], [1, 1, 5, 3], [2, 1, 8, 2]])
    refs = ops.event_refs(REF, TOL, RO, 3)
    filt = torch.zeros((3, 10))
    ok = dict(filt=filt, table=table, nsamp=[50, 30, 20], R=10, refs=refs, c=2, hi=[0.5, 0.7], lo=[0.5, 0.3])

    def refuse(match, **over):
        a = dict(ok)
        a.update(over)
        with pytest.raises(EatHipError, match="event_score: .*" + match):
            ops.event_score(**a)

    refuse("no CPU path")                                                     # everything else is in order: only the device is missing
    refuse(r"\(K, G_total\)", filt=torch.zeros(10))
    refuse("10 frames", filt=torch.zeros((3, 11)))
    refuse("float32", filt=torch.zeros((3, 10), dtype=torch.float64))
    refuse("float32", filt=torch.zeros((10, 3)).t())
    refuse("DetectTable", table=[[0, 1, 0, 10]])
    refuse("EventRefs", refs=(REF, TOL, RO))
    refuse("refs hold 3 classes, filt 2", filt=torch.zeros((2, 10)))
    refuse("R >= 1", R=0)
    refuse("must not be negative", c=-1)
    refuse("must not be negative", max_gap=-1)
    refuse("must not be negative", min_len=-2)
    refuse(r"recordings \[1, 4\) lie outside the 3", first=1)
    refuse("outside", first=-1)
    refuse("nsamp must hold n_rec = 3 integers", nsamp=[50, 30])
    refuse("nsamp must hold n_rec = 3 integers", nsamp=[50.0, 30.0, 20.0])
    refuse(">= 1 sample", nsamp=[50, 0, 20])
    refuse("V >= 1 values each", hi=[], lo=[])
    refuse("V >= 1 values each", hi=[0.5, 0.7], lo=[0.5])
    refuse("0 < lo <= hi <= 1", lo=[0.5, 0.8])
    refuse("0 < lo <= hi <= 1", lo=[0.0, 0.3])
    refuse("0 < lo <= hi <= 1", hi=[0.5, 1.5])
    refuse("0 < lo <= hi <= 1", hi=[0.5, float("nan")])
    refuse("out must be", out=torch.zeros((3, 3, 2, 2), dtype=torch.int64))
    refuse("out must be", out=torch.zeros((3, 3, 2), dtype=torch.int32))
