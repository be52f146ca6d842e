"""Host side of per-class median tuning: the restatement of the width-bank median against scipy, `sed.pick_operating_points`
against brute force and its tie rules, the width validators, operating-point files with `class_median_ms`, and the programs'
new arguments.  No GPU."""
import contextlib
import io
import json

import numpy as np
import pytest
import torch
from scipy.ndimage import median_filter

from efficientat_amd import detection, finetune_sed, ops, score_sed, sed
from efficientat_amd._lib import EatHipError
from tests import event_score_ref as score_ref_mod
from tests import tune_case as C
from tests.detect_ref import median_ref
from tests.median_bank_ref import median_bank_ref

FRAME_S = 0.32


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
        return fn(*a, **k)


# ------------------------------------------------------------------------------------------------ the restatement
def test_median_bank_ref_is_scipy_median_filter_per_recording():
    """Tenths, so that ties are frequent; two recordings side by side; every width with m // 2 <= G."""
    rng = np.random.default_rng(0)
    rec = [(0, 1, 0, 40), (1, 1, 40, 17)]
    x = (rng.integers(0, 11, size=(3, 57)) / 10.0).astype(np.float32)
    widths = np.asarray([[1, 3, 5], [31, 7, 1], [9, 9, 9]])
    got = median_bank_ref(x, rec, widths)
    assert got.shape == (3, 3, 57) and got.dtype == np.float32
    for j in range(3):
        for k in range(3):
            for _, _, goff, G in rec:
                m = int(widths[j, k])
                assert m // 2 <= G
                want = median_filter(x[k, goff:goff + G], size=m, mode="reflect")
                assert np.array_equal(got[j, k, goff:goff + G], want), (j, k, goff)
    assert np.array_equal(got[0, 0], x[0]) and np.array_equal(median_bank_ref(x, rec, [1, 1, 1])[0], x)


# ------------------------------------------------------------------------------------------------ pick_operating_points
def _brute(counts_grid, ref_index):
    """Per class the first (width, threshold) of maximal F1 in width-major order, NaN below everything -> (j, v) or (ref, -1)."""
    Mw, V, K, _ = counts_grid.shape
    out = []
    for k in range(K):
        best, arg = None, (ref_index, -1)
        for j in range(Mw):
            for v in range(V):
                tp, fp, fn = (int(t) for t in counts_grid[j, v, k])
                if 2 * tp + fp + fn == 0:
                    continue
                f = 2 * tp / (2 * tp + fp + fn)
                if best is None or f > best:
                    best, arg = f, (j, v)
        out.append(arg)
    return out


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_pick_operating_points_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    Mw, V, K = 5, 7, 9
    counts = rng.integers(0, 4, size=(Mw, V, K, 3)).astype(np.int64)
    counts[:, :, 2] = 0                                          # a class with nothing to score anywhere
    counts[1:, 2:, 4] = 0                                        # ... and one with nothing at most points
    hi, lo = sed.threshold_grid(np.linspace(0.2, 0.8, V), 0.5)
    at, bj, bv, b_hi, b_lo = sed.pick_operating_points(counts, hi, lo, 0.5, 3, 0.5)
    want = _brute(counts, 3)
    assert at == 3 and list(zip(bj.tolist(), bv.tolist())) == want
    assert want[2] == (3, -1) and b_hi[2] == np.float32(0.5) and b_lo[2] == np.float32(0.25)
    for k, (j, v) in enumerate(want):
        if v >= 0:
            assert b_hi[k] == hi[v] and b_lo[k] == lo[v]
    assert b_hi.dtype == np.float32 and b_lo.dtype == np.float32
    # one width: exactly pick_thresholds
    at1, best1, hi1, lo1 = sed.pick_thresholds(counts[2], hi, lo, 0.5, 0.5)
    at2, j2, v2, hi2, lo2 = sed.pick_operating_points(counts[2:3], hi, lo, 0.5, 0, 0.5)
    assert at1 == at2 and np.array_equal(best1, v2) and not j2.any() and np.array_equal(hi1, hi2) and np.array_equal(lo1, lo2)


def test_pick_operating_points_tie_rules():
    hi, lo = sed.threshold_grid([0.3, 0.5, 0.7])
    c = np.zeros((3, 3, 2, 3), dtype=np.int64)
    c[..., 2] = 4                                                # four references, nothing found: F1 = 0 everywhere
    c[1, 2, 0] = c[2, 0, 0] = c[1, 1, 0] = (2, 0, 2)             # class 0: equal F1 at (1, 1), (1, 2), (2, 0)
    c[2, 1, 1] = (1, 0, 3)
    c[0, 1, 1] = (1, 0, 3)                                       # class 1: equal F1 at widths 0 and 2
    _, bj, bv, b_hi, _ = sed.pick_operating_points(c, hi, lo, 0.5, 2)
    assert (bj.tolist(), bv.tolist()) == ([1, 0], [1, 1])        # the narrower width, then the lower threshold
    assert b_hi.tolist() == [0.5, 0.5]
    c[:] = 0                                                     # nothing to score anywhere: the reference is kept
    at, bj, bv, b_hi, b_lo = sed.pick_operating_points(c, hi, lo, 0.45, 2)
    assert at == 1 and bj.tolist() == [2, 2] and bv.tolist() == [-1, -1]
    assert b_hi.tolist() == [float(np.float32(0.45))] * 2 and b_lo.tolist() == b_hi.tolist()
    with pytest.raises(ValueError, match="ref_index"):
        sed.pick_operating_points(c, hi, lo, 0.5, 3)
    with pytest.raises(ValueError, match="counts_grid"):
        sed.pick_operating_points(c[:, :2], hi, lo, 0.5, 0)


def test_tuned_scores_on_the_two_class_case():
    """The counts of the discriminating case of tests/test_gpu_tune_postprocessing.py (6 and 12 references): no single width
    serves both classes, width 5 for the long events and width 3 for the short ones serves each."""
    frames = list(C.WIDTHS)
    prob, rec, nsamp, ref, ro = C.build()
    tol = score_ref_mod.tolerances(ref, C.COLLAR, C.PCT)
    res = np.stack([score_ref_mod.score_ref(median_ref(prob, rec, m), rec, nsamp, C.R, ref, tol, ro, C.COLLAR, [0.5], [0.5]).sum(0)
                    for m in frames])                            # (Mw, K, 1, 2) through the numpy restatements
    assert {m: tuple(tuple(int(v) for v in res[j, k, 0]) for k in range(2)) for j, m in enumerate(frames)} == C.EXPECTED
    counts = C.counts_grid(res)
    assert counts.shape == (7, 1, 2, 3)
    hi, lo = sed.threshold_grid([0.5])
    t = sed.tuned_scores(counts, hi, lo, 0.5, 1)
    assert [frames[j] for j in t["best_median_index"]] == [5, 3] and t["best_index"].tolist() == [0, 0]
    assert t["macro_f1_tuned"] == 1.0 and t["macro_f1_best_single"] == 0.5 and frames[t["best_single_index"]] == 3
    single = [sed.segment_scores(counts[j, 0])["macro_f1"] for j in range(7)]
    assert single == pytest.approx([1 / 3, 0.5, 0.5, 0.5, 0.5, 0.5, 0.0], abs=1e-15)


# ------------------------------------------------------------------------------------------------ widths
def test_median_frames_per_class():
    assert detection.median_frames_per_class(960, FRAME_S, 4).tolist() == [3, 3, 3, 3]
    got = detection.median_frames_per_class([0, 320, 960, 1280, 9920], FRAME_S, 5)
    assert got.dtype == np.int32 and got.tolist() == [1, 1, 3, 5, 31]
    assert got.tolist() == [detection.median_frames(v, FRAME_S) for v in (0, 320, 960, 1280, 9920)]
    with pytest.raises(ValueError, match="class 2.*33 frames"):
        detection.median_frames_per_class([0, 320, 10240], FRAME_S, 3)
    with pytest.raises(ValueError, match="class 1"):
        detection.median_frames_per_class([0, float("nan"), 320], FRAME_S, 3)
    with pytest.raises(ValueError, match="class 0"):
        detection.median_frames_per_class([-1, 0, 320], FRAME_S, 3)
    with pytest.raises(ValueError, match="one value per class, K = 3"):
        detection.median_frames_per_class([0, 320], FRAME_S, 3)
    with pytest.raises(ValueError, match="33 frames"):           # a scalar: the message of median_frames itself
        detection.median_frames_per_class(10240, FRAME_S, 3)


def test_median_width_table():
    t = ops.median_width_table([1, 3, 31], 3)
    assert (t.Mw, t.K) == (1, 3) and t.cpu.dtype == torch.int32 and t.cpu.tolist() == [[1, 3, 31]]
    t = ops.median_width_table(np.asarray([[1, 3], [5, 7], [31, 1]], dtype=np.int64), 2)
    assert (t.Mw, t.K) == (3, 2) and t.cpu.is_contiguous() and t.cpu.tolist() == [[1, 3], [5, 7], [31, 1]]
    assert ops.median_width_table(torch.tensor([[9, 9]], dtype=torch.int16), 2).cpu.tolist() == [[9, 9]]
    for bad in (2, 0, 33, -3):
        with pytest.raises(EatHipError, match=f"slice 1, class 2: width {bad} "):
            ops.median_width_table([[1, 1, 1], [3, 5, bad]], 3)
    with pytest.raises(EatHipError, match="integers"):
        ops.median_width_table([1.0, 3.0], 2)
    with pytest.raises(EatHipError, match="integers"):
        ops.median_width_table([True, True], 2)
    for shape in ((3,), (2, 3), (0, 2), (1, 1, 2)):
        with pytest.raises(EatHipError, match=r"\(K,\) or \(Mw >= 1, K\) with K = 2"):
            ops.median_width_table(np.ones(shape, dtype=np.int64), 2)


# ------------------------------------------------------------------------------------------------ operating-point files
CLASSES = ["alarm", "dog", "speech"]
# what save_operating_points wrote before class_median_ms existed, field for field
OLD_DOC = {"classes": CLASSES, "threshold": [0.42, 0.5, 0.58], "low_threshold": [0.3, 0.5, 0.4], "median_ms": 960.0,
           "min_duration_ms": 640.0, "max_gap_ms": 320.0, "taper": "triangle", "window_size": 10.24, "hop_length": 5.12,
           "scoring": {"collar_ms": 200.0, "offset_pct": 0.2, "low_ratio": 0.8, "reference_threshold": 0.5, "n_clips": 6,
                       "n_ref": 20, "grid": [0.25, 0.5, 0.75]},
           "scores": {"macro_f1_best": 0.5, "micro_f1": 0.4, "micro_precision": 0.4, "micro_recall": 0.4, "macro_f1": 0.3,
                      "macro_precision": 0.3, "macro_recall": 0.3}}


def _result(tuned):
    """A result dict with the fields save_operating_points reads."""
    r = {"best_threshold": np.asarray(OLD_DOC["threshold"], dtype=np.float32),
         "best_low_threshold": np.asarray(OLD_DOC["low_threshold"], dtype=np.float32), "threshold": 0.5, "n_clips": 6, "n_ref": 20,
         "thresholds": np.asarray([0.25, 0.5, 0.75], dtype=np.float32), "macro_f1_best": 0.5,
         "settings": {"median_ms": 960.0, "min_duration_ms": 640.0, "max_gap_ms": 320.0, "taper": "triangle", "window_size": 10.24,
                      "hop_length": 5.12, "collar_ms": 200.0, "offset_pct": 0.2, "low_ratio": 0.8}}
    r.update({"micro_f1": 0.4, "micro_precision": 0.4, "micro_recall": 0.4, "macro_f1": 0.3, "macro_precision": 0.3,
              "macro_recall": 0.3})
    if tuned:
        r["settings"]["frame_ms"] = 320.0
        r.update({"best_median_ms": np.asarray([1600.0, 960.0, 320.0]), "macro_f1_tuned": 0.75, "macro_f1_best_single": 0.5,
                  "best_single_median_ms": 960.0})
    return r


def test_operating_points_round_trip_with_class_median_ms(tmp_path):
    path = str(tmp_path / "ops.json")
    doc = sed.save_operating_points(path, _result(True), CLASSES)
    assert doc["class_median_ms"] == [1600.0, 960.0, 320.0] and doc["median_ms"] == 960.0 and doc["frame_ms"] == 320.0
    assert doc["scores"]["macro_f1_tuned"] == 0.75 and doc["scores"]["best_single_median_ms"] == 960.0
    pts = sed.load_operating_points(path, classes=CLASSES, n_classes=3)
    assert pts["class_median_ms"].dtype == np.float64 and pts["class_median_ms"].tolist() == [1600.0, 960.0, 320.0]
    assert pts["median_ms"] == 960.0 and pts["threshold"].tolist() == doc["threshold"] == [float(np.float32(v)) for v in (0.42, 0.5, 0.58)]
    assert detection.median_frames_per_class(pts["class_median_ms"], FRAME_S, 3).tolist() == [5, 3, 1]


def test_a_file_of_the_earlier_format_loads_as_before_and_is_still_what_an_untuned_result_writes(tmp_path):
    path = str(tmp_path / "old.json")
    with open(path, "w") as f:
        json.dump(OLD_DOC, f, indent=1)
        f.write("\n")
    pts = sed.load_operating_points(path, classes=CLASSES)
    assert set(pts) == set(OLD_DOC) and "class_median_ms" not in pts and "frame_ms" not in pts
    assert pts["threshold"].dtype == np.float32 and pts["threshold"].tolist() == [float(np.float32(v)) for v in OLD_DOC["threshold"]]
    assert pts["low_threshold"].tolist() == [float(np.float32(v)) for v in OLD_DOC["low_threshold"]]
    for k in ("classes", "median_ms", "min_duration_ms", "max_gap_ms", "taper", "window_size", "hop_length", "scoring", "scores"):
        assert pts[k] == OLD_DOC[k], k
    # an evaluate_events result still writes exactly those fields, in that order
    again = str(tmp_path / "again.json")
    doc = sed.save_operating_points(again, _result(False), CLASSES)
    assert list(doc) == list(OLD_DOC) and list(doc["scoring"]) == list(OLD_DOC["scoring"]) and list(doc["scores"]) == list(OLD_DOC["scores"])
    assert doc["scoring"] == OLD_DOC["scoring"] and doc["scores"] == OLD_DOC["scores"]


@pytest.mark.parametrize("bad,what", [([960.0, 960.0], "K = 3 values"), ([960.0, float("nan"), 320.0], "class 1"),
                                      ([960.0, 320.0, 10240.0], "class 2.*33 frames"), ("wide", "numbers"),
                                      ([[960.0, 320.0, 0.0]], "K = 3 values")])
def test_bad_class_median_ms_is_refused_naming_the_file(tmp_path, bad, what):
    path = str(tmp_path / "bad.json")
    doc = dict(OLD_DOC, class_median_ms=bad)
    with open(path, "w") as f:
        json.dump(doc, f)
    with pytest.raises(ValueError, match=what) as e:
        sed.load_operating_points(path)
    assert path in str(e.value) and "class_median_ms" in str(e.value)
    doc = dict(OLD_DOC, class_median_ms=[960.0, 320.0, 0.0], frame_ms=0.0)
    with open(path, "w") as f:
        json.dump(doc, f)
    with pytest.raises(ValueError, match="frame_ms") as e:
        sed.load_operating_points(path)
    assert path in str(e.value)
    doc["frame_ms"] = 20.0                                       # another geometry: 960 ms is 48 frames there
    with open(path, "w") as f:
        json.dump(doc, f)
    with pytest.raises(ValueError, match="class 0.*49 frames"):
        sed.load_operating_points(path)


# ------------------------------------------------------------------------------------------------ arguments
def test_score_sed_arguments():
    base = ["--checkpoint", "c.pt", "--bank", "d"]
    a = score_sed.parse_args(base)
    assert a.tune_median is False and a.median_grid_ms is None and a.operating_points is None
    a = score_sed.parse_args(base + ["--tune_median", "--median_grid_ms", "0,960, 2240", "--operating_points", "ops.json"])
    assert a.tune_median is True and a.median_grid_ms == [0.0, 960.0, 2240.0] and a.operating_points == "ops.json"
    for bad in (["--median_grid_ms", "0,960"], ["--tune_median", "--median_grid_ms", "a,b"], ["--tune_median", "--median_grid_ms", ","]):
        with pytest.raises(SystemExit):
            _quiet(score_sed.parse_args, base + bad)


def test_finetune_sed_arguments():
    base = ["--train_bank", "a", "--valid_bank", "b"]
    a = finetune_sed.parse_args(base)
    assert a.tune_median is False and a.median_grid_ms is None
    a = finetune_sed.parse_args(base + ["--event_eval", "--tune_median", "--median_grid_ms", "320,1600"])
    assert a.tune_median is True and a.median_grid_ms == [320.0, 1600.0]
    for bad in (["--tune_median"], ["--event_eval", "--median_grid_ms", "320"]):
        with pytest.raises(SystemExit):
            _quiet(finetune_sed.parse_args, base + bad)
