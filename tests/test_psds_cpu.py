"""PSDS without a GPU: the numpy restatement (tests/psds_ref.py) against a per-sample boolean-mask computation, the curve on
a hand-worked case and on perfect / empty detectors, its invariances, the scenario table, the C header and its binding with
the argument checks that return before anything touches the device, and the host-side refusals of `ops.psds_count`."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from efficientat_amd import _lib, build, ops, sed
from efficientat_amd._lib import EatHipError
from tests import psds_ref as P
from tests.detect_ref import timeline_events

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- the restatement
def _mask(n, on, off):
    m = np.zeros(n, dtype=bool)
    m[max(on, 0):max(min(off, n), 0)] = True
    return m


def _brute(filt, rec, nsamp, R, ref, ro, dtc_pm, gtc_pm, cttc_pm, hi, lo, max_gap, min_len):
    """Every intersection as the population count of two per-sample masks; detections by frame, then painted."""
    K, V = filt.shape[0], len(hi)
    counts = np.zeros((len(rec), K, V, 4), dtype=np.int64)
    ct = np.zeros((V, K, K), dtype=np.int64)
    for i, (_, _, goff, G) in enumerate(rec):
        n = int(nsamp[i])
        span = G * R                                                          # masks as long as the frames reach, cut to n below
        rows = [(int(c), _mask(span, on, off), off - on) for c, on, off in ref[ro[i]:ro[i + 1]]]
        for k in range(K):
            for v in range(V):
                cover = [0] * len(rows)
                tp = fp = n_ct = n_det = 0
                for on, off in timeline_events(filt[k, goff:goff + G], hi[v], lo[v], max_gap, min_len):
                    d = _mask(span, on * R, off * R)
                    d[n:] = False
                    L = int(d.sum())
                    n_det += 1
                    S = sum(int((d & m).sum()) for c, m, _ in rows if c == k)
                    if L > 0 and 1000 * S >= dtc_pm * L:
                        for j, (c, m, _) in enumerate(rows):
                            if c == k:
                                cover[j] += int((d & m).sum())
                        continue
                    fp += 1
                    if cttc_pm > 0 and L > 0:
                        for c in sorted({c for c, _, _ in rows if c != k}):
                            if 1000 * sum(int((d & m).sum()) for cc, m, _ in rows if cc == c) >= cttc_pm * L:
                                ct[v, k, c] += 1
                                n_ct += 1
                for j, (c, _, length) in enumerate(rows):
                    if c == k and length > 0 and 1000 * cover[j] >= gtc_pm * length:
                        tp += 1
                counts[i, k, v] = (tp, n_det, fp, n_ct)
    return counts, ct


def test_the_restatement_equals_a_per_sample_mask_computation():
    rng = np.random.default_rng(11)
    levels = np.asarray([0.0, 0.2, 0.5, 0.9], dtype=np.float32)
    seen = np.zeros(4, dtype=np.int64)
    crossed = 0
    for case in range(60):
        K, R = int(rng.integers(1, 4)), int(rng.integers(1, 5))
        Gs = [int(rng.integers(1, 200 // R + 1)) for _ in range(int(rng.integers(1, 4)))]
        goff = np.cumsum(Gs) - np.asarray(Gs)
        rec = [(i, 1, int(o), g) for i, (o, g) in enumerate(zip(goff, Gs))]
        nsamp = [max(1, g * R - int(rng.integers(0, R))) for g in Gs]
        filt = levels[rng.integers(0, 4, size=(K, sum(Gs)))]
        filt = np.where(rng.random(filt.shape) < 0.5, np.roll(filt, 1, axis=1), filt).astype(np.float32)
        rows, ro = [], [0]
        for n in nsamp:
            mine = []
            for _ in range(int(rng.integers(0, 7))):
                on = int(rng.integers(0, n))
                mine.append((int(rng.integers(0, K)), on, min(n, on + int(rng.integers(0, 40)))))
            rows.extend(sorted(mine))
            ro.append(len(rows))
        ref = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
        crit = (int(rng.choice([100, 500, 700, 1000])), int(rng.choice([100, 500, 700, 1000])), int(rng.choice([0, 300, 1000])))
        hi = np.asarray([0.5, 0.9, 0.2], dtype=np.float32)
        lo = np.asarray([0.5, 0.2, 0.2], dtype=np.float32)
        gap, mlen = int(rng.integers(0, 3)), int(rng.integers(0, 3))
        got = P.count_ref(filt, rec, nsamp, R, ref, ro, *crit, hi, lo, gap, mlen)
        want = _brute(filt, rec, nsamp, R, ref.tolist(), ro, *crit, hi, lo, gap, mlen)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), case
        assert np.array_equal(got[1].sum(2).T, got[0][..., 3].sum(0))
        assert np.array_equal(got[0][..., 1] >= got[0][..., 2], np.ones_like(got[0][..., 1], dtype=bool))
        seen += got[0].sum((0, 1, 2))
        crossed += int(got[1].sum())
    assert seen.min() > 0 and crossed > 0                                     # every count occurs


def test_the_criteria_on_hand_built_cases():
    # DTC exactly on the ratio and one sample short: L = 1000, intersection 700 / 699 at 700 per mille
    assert P.judge_timeline([(0, 1000)], [(300, 2000)], {}, 700, 100, 0)[::2] == (1, 0)
    assert P.judge_timeline([(0, 1000)], [(301, 2000)], {}, 700, 100, 0)[::2] == (0, 1)
    # GTC: a reference of 1000 covered by 700 / 699
    assert P.judge_timeline([(0, 700)], [(0, 1000)], {}, 700, 700, 0)[0] == 1
    assert P.judge_timeline([(0, 699)], [(0, 1000)], {}, 700, 700, 0)[0] == 0
    # two references of the class, and references that overlap each other, add in S
    assert P.judge_timeline([(0, 100)], [(0, 35), (65, 100)], {}, 700, 1000, 0) == (2, 1, 0, [])
    assert P.judge_timeline([(0, 100)], [(0, 35), (0, 35)], {}, 700, 1000, 0) == (2, 1, 0, [])
    # a reference covered by two detections of which one fails DTC: that one does not count towards GTC
    assert P.judge_timeline([(0, 50), (50, 300)], [(0, 100)], {}, 700, 1000, 0) == (0, 2, 1, [])
    assert P.judge_timeline([(0, 50), (50, 300)], [(0, 100)], {}, 200, 1000, 0) == (1, 2, 0, [])
    # a relevant detection raises no cross-trigger; a false positive raises one per class at or above CTTC
    assert P.judge_timeline([(0, 100)], [(0, 100)], {1: [(0, 100)]}, 700, 700, 300) == (1, 1, 0, [])
    assert P.judge_timeline([(0, 100)], [], {1: [(0, 30)], 2: [(0, 29)]}, 700, 700, 300) == (0, 1, 1, [1])
    assert P.judge_timeline([(0, 100)], [], {1: [(0, 30)]}, 700, 700, 0) == (0, 1, 1, [])
    # a zero-length reference is never detected; a zero-length detection is a false positive without cross-triggers
    assert P.judge_timeline([(0, 100)], [(50, 50), (0, 100)], {}, 700, 1, 0)[0] == 1
    assert P.judge_timeline([(40, 40)], [(0, 100)], {1: [(0, 100)]}, 1, 1, 1) == (0, 1, 1, [])


# ---------------------------------------------------------------------------------------------------- the curve
HAND = dict(n_ref=[2, 4], ref_seconds=[1800.0, 900.0], total_seconds=3600.0)
TP, FP = np.asarray([[1, 2], [2, 2]]), np.asarray([[0, 10], [50, 10]])


def _both(tp, fp, ct, alpha_ct, alpha_st, e_max=100.0, **kw):
    kw = kw or HAND
    ours = sed.psds_from_counts(tp, fp, ct, kw["n_ref"], kw["ref_seconds"], kw["total_seconds"], alpha_ct, alpha_st, e_max)
    ref = P.curve_ref(tp, fp, np.zeros((len(tp), len(tp[0]), len(tp[0]))) if ct is None else ct, kw["n_ref"], kw["ref_seconds"],
                      kw["total_seconds"], alpha_ct, alpha_st, e_max)
    if math.isnan(ref[0]):
        assert math.isnan(ours["psds"]) and ours["etpr_x"].size == 0
    else:
        # (two fp64 evaluations of the same few dozen terms in different orders: 1e-12 leaves three decades)
        assert ours["psds"] == pytest.approx(ref[0], rel=1e-12, abs=1e-15)
    return ours


def test_the_hand_worked_curve():
    ct = np.zeros((2, 2, 2), dtype=np.int64)
    assert _both(TP, FP, ct, 0.0, 0.0)["psds"] == pytest.approx(0.60, abs=1e-12)
    assert _both(TP, FP, ct, 0.0, 1.0)["psds"] == pytest.approx(0.45, abs=1e-12)
    assert _both(TP, FP, None, 0.0, 1.0)["psds"] == pytest.approx(0.45, abs=1e-12)
    ct[1, 0, 1] = 5
    out = _both(TP, FP, ct, 1.0, 0.0)
    assert out["psds"] == pytest.approx(0.55, abs=1e-12)
    assert out["efpr"].tolist() == [[0.0, 10.0], [70.0, 10.0]] and out["tpr"].tolist() == [[0.5, 0.5], [1.0, 0.5]]
    assert out["etpr_x"].tolist() == [0.0, 10.0, 70.0, 100.0] and out["etpr_y"][:3].tolist() == [0.25, 0.5, 0.75]
    # a cross-trigger onto a class without reference time counts for nothing; K = 1 has no cross-trigger term at all
    z = dict(n_ref=[2, 0], ref_seconds=[1800.0, 0.0], total_seconds=3600.0)
    assert _both(TP, FP, ct, 1.0, 0.0, **z)["efpr"][1, 0] == 50.0
    one = dict(n_ref=[2], ref_seconds=[10.0], total_seconds=3600.0)
    assert _both(TP[:, :1], FP[:, :1], np.full((2, 1, 1), 9), 1.0, 1.0, **one)["psds"] == pytest.approx(0.75, abs=1e-12)


def test_perfect_empty_and_unscored():
    n_ref = [3, 5, 2]
    kw = dict(n_ref=n_ref, ref_seconds=[30.0, 50.0, 20.0], total_seconds=600.0)
    V = 4
    perfect = np.tile(np.asarray(n_ref), (V, 1))
    zero = np.zeros((V, 3), dtype=np.int64)
    for a_ct, a_st in ((0.0, 1.0), (0.5, 1.0)):
        assert _both(perfect, zero, None, a_ct, a_st, **kw)["psds"] == pytest.approx(1.0, abs=1e-12)
        assert _both(zero, zero, None, a_ct, a_st, **kw)["psds"] == 0.0
    # false positives only: still 0; all of them beyond e_max: the curve is empty inside [0, e_max]
    assert _both(zero, zero + 7, None, 0.0, 1.0, **kw)["psds"] == 0.0
    assert _both(perfect, zero + 10 ** 6, None, 0.0, 1.0, **kw)["psds"] == 0.0
    # a class without references is left out of the statistics; none at all is NaN
    part = dict(n_ref=[3, 0, 2], ref_seconds=[30.0, 0.0, 20.0], total_seconds=600.0)
    assert _both(perfect, zero, None, 0.0, 1.0, **part)["psds"] == pytest.approx(1.0, abs=1e-12)
    assert np.isnan(_both(perfect, zero, None, 0.0, 1.0, **part)["tpr"][:, 1]).all()
    none = dict(n_ref=[0, 0, 0], ref_seconds=[0.0, 0.0, 0.0], total_seconds=600.0)
    assert math.isnan(_both(zero, zero + 1, None, 0.0, 1.0, **none)["psds"])
    with pytest.raises(ValueError, match="total_seconds"):
        sed.psds_from_counts(zero, zero, None, n_ref, kw["ref_seconds"], 0.0, 0.0, 1.0)
    with pytest.raises(ValueError, match=r"\(V, K\)"):
        sed.psds_from_counts(zero, zero[:2], None, n_ref, kw["ref_seconds"], 600.0, 0.0, 1.0)


def test_a_duplicated_or_dominated_threshold_leaves_psds_unchanged():
    rng = np.random.default_rng(3)
    for _ in range(50):
        V, K = int(rng.integers(1, 6)), int(rng.integers(1, 4))
        n_ref = rng.integers(1, 9, size=K)
        tp = np.minimum(rng.integers(0, 9, size=(V, K)), n_ref)
        fp = rng.integers(0, 12, size=(V, K))
        ct = rng.integers(0, 4, size=(V, K, K))
        kw = dict(n_ref=n_ref.tolist(), ref_seconds=(n_ref * 7.5).tolist(), total_seconds=1800.0)
        base = _both(tp, fp, ct, 0.5, 1.0, e_max=30.0, **kw)["psds"]
        v = int(rng.integers(0, V))
        dup = [np.concatenate([a, a[v:v + 1]]) for a in (tp, fp, ct)]
        assert _both(*dup, 0.5, 1.0, e_max=30.0, **kw)["psds"] == pytest.approx(base, abs=1e-12)
        # dominated: no more true positives, at least as many false positives and cross-triggers, in every class
        dom = [np.concatenate([tp, np.maximum(tp[v:v + 1] - 1, 0)]), np.concatenate([fp, fp[v:v + 1] + 2]),
               np.concatenate([ct, ct[v:v + 1] + 1])]
        assert _both(*dom, 0.5, 1.0, e_max=30.0, **kw)["psds"] == pytest.approx(base, abs=1e-12)


def test_the_scenario_table():
    assert sed.PSDS_SCENARIOS == {1: dict(dtc=0.7, gtc=0.7, cttc=0.0, alpha_ct=0.0, alpha_st=1.0, e_max=100.0),
                                  2: dict(dtc=0.1, gtc=0.1, cttc=0.3, alpha_ct=0.5, alpha_st=1.0, e_max=100.0)}
    assert [ops.per_mille(k, sed.PSDS_SCENARIOS[1][k], 0) for k in ("dtc", "gtc", "cttc")] == [700, 700, 0]
    assert [ops.per_mille(k, sed.PSDS_SCENARIOS[2][k], 0) for k in ("dtc", "gtc", "cttc")] == [100, 100, 300]
    with pytest.raises(ValueError, match="scenario"):
        sed.evaluate_psds(None, None, None, scenario=3)


# ---------------------------------------------------------------------------------------------------- header
def test_the_psds_header_parses_is_disjoint_from_the_other_headers_and_is_bound():
    P_, I = ctypes.c_void_p, ctypes.c_int
    with open(os.path.join(ROOT, "include", "eat_psds.h")) as f:
        protos = _lib.parse_prototypes(f.read())
    assert protos == _lib.PSDS_PROTOTYPES
    assert set(protos) == {"eat_psds_count"}
    assert protos["eat_psds_count"] == (I, [P_, I, I, P_, I, P_, I, P_, P_, I, I, I, I, P_, P_, I, I, I, P_, P_, P_])
    others = [v for k, v in vars(_lib).items() if k.endswith("PROTOTYPES") and k != "PSDS_PROTOTYPES"]
    assert len(others) >= 7
    for other in others:
        assert not set(protos) & set(other)
    assert "eat_psds_count" not in _lib.exported_symbols()
    assert "psds.hip" in build.SOURCES and os.path.exists(os.path.join(ROOT, "efficientat_amd", "csrc", "event_walk.h"))
    build.build()
    for name, (restype, args) in protos.items():
        fn = getattr(_lib.lib(), name)
        assert list(fn.argtypes) == args and fn.restype is restype, name
    # argument checks that return before anything touches the device: `one` is never dereferenced
    one = ctypes.c_void_p(16)

    def count(**kw):
        a = dict(filt=one, K=1, G_total=1, rec=one, n_rec=1, nsamp=one, R=1, ref=one, ro=one, n_ref=1, dtc_pm=700, gtc_pm=700,
                 cttc_pm=300, hi=one, lo=one, V=1, max_gap=0, min_len=0, counts=one, ct=one)
        a.update(kw)
        _lib.call("eat_psds_count", *a.values(), None)

    for missing in ("filt", "rec", "nsamp", "ref", "ro", "hi", "lo", "counts"):
        with pytest.raises(EatHipError, match="eat_psds_count: missing operand"):
            count(**{missing: None})
    for bad in (dict(K=0), dict(G_total=0), dict(n_rec=0), dict(R=0), dict(V=0), dict(K=-1)):
        with pytest.raises(EatHipError, match="eat_psds_count: need K, n_rec, G_total, R, V >= 1"):
            count(**bad)
    for bad in (dict(max_gap=-1), dict(min_len=-1), dict(n_ref=-1)):
        with pytest.raises(EatHipError, match="eat_psds_count: need n_ref, max_gap, min_len >= 0"):
            count(**bad)
    for bad in (dict(dtc_pm=0), dict(dtc_pm=1001), dict(gtc_pm=0), dict(gtc_pm=1001), dict(dtc_pm=-5)):
        with pytest.raises(EatHipError, match=r"must lie in \[1, 1000\]"):
            count(**bad)
    for bad in (dict(cttc_pm=-1), dict(cttc_pm=1001)):
        with pytest.raises(EatHipError, match=r"cttc_pm=-?\d+ must lie in \[0, 1000\]"):
            count(**bad)
    with pytest.raises(EatHipError, match="cttc_pm=300 needs the cross-trigger buffer ct"):
        count(ct=None)
    with pytest.raises(EatHipError, match="exceed the grid limit"):
        count(n_rec=2 ** 16, K=2 ** 15)
    with pytest.raises(EatHipError, match="threshold pairs exceed"):
        count(V=64 * 65535 + 1)


# ---------------------------------------------------------------------------------------------------- ops refusals
REF = torch.tensor([[0, 0, 10], [0, 5, 50], [2, 49, 50], [1, 0, 30]], dtype=torch.int32)
RO = torch.tensor([0, 3, 4, 4], dtype=torch.int64)


def test_psds_count_host_side_refusals():
    table = ops.detect_table([[0, 1, 0, 5], [1, 1, 5, 3], [2, 1, 8, 2]])
    refs = ops.event_refs(REF, torch.zeros(4, dtype=torch.int32), RO, 3)
    filt = torch.zeros((3, 10))
    ok = dict(filt=filt, table=table, nsamp=[50, 30, 20], R=10, refs=refs, dtc=0.7, gtc=0.7, cttc=0.3, hi=[0.5, 0.7], lo=[0.5, 0.3])

    def refuse(match, **over):
        a = dict(ok)
        a.update(over)
        with pytest.raises(EatHipError, match="psds_count: .*" + match):
            ops.psds_count(**a)

    refuse("no CPU path")                                                     # everything else is in order: only the device is missing
    refuse("no CPU path", cttc=0.0)
    for name in ("dtc", "gtc", "cttc"):
        refuse(f"{name}=0.7004 must be a whole number of per-mille", **{name: 0.7004})
        refuse(f"{name}=1.001 must lie in", **{name: 1.001})
        refuse(f"{name}=-0.1 must lie in", **{name: -0.1})
        refuse(f"{name}=nan must be a whole number", **{name: float("nan")})
        refuse(f"{name}='x' is not a number", **{name: "x"})
    refuse(r"dtc=0 must lie in \(0, 1\]", dtc=0)
    refuse(r"gtc=0.0 must lie in \(0, 1\]", gtc=0.0)
    assert [ops.per_mille("x", v) for v in (0.001, 0.105, 0.7, 1, 0.3)] == [1, 105, 700, 1000, 300]
    refuse(r"\(K, G_total\)", filt=torch.zeros(10))
    refuse("10 frames", filt=torch.zeros((3, 11)))
    refuse("float32", filt=torch.zeros((3, 10), dtype=torch.float64))
    refuse("DetectTable", table=[[0, 1, 0, 10]])
    refuse("EventRefs", refs=(REF, RO))
    refuse("refs hold 3 classes, filt 2", filt=torch.zeros((2, 10)))
    refuse("R >= 1", R=0)
    refuse("must not be negative", max_gap=-1)
    refuse("must not be negative", min_len=-2)
    refuse(r"recordings \[1, 4\) lie outside the 3", first=1)
    refuse("nsamp must hold n_rec = 3 integers", nsamp=[50, 30])
    refuse(">= 1 sample", nsamp=[50, 0, 20])
    refuse("V >= 1 values each", hi=[], lo=[])
    refuse("0 < lo <= hi <= 1", lo=[0.5, 0.8])
    refuse(r"out must be a contiguous int32 tensor of 72 elements", out=torch.zeros((3, 3, 2, 2), dtype=torch.int32))
    refuse(r"ct must be a \(V, K, K\) = \(2, 3, 3\) tensor", ct=torch.zeros((3, 3, 2), dtype=torch.int32))
    refuse("ct must be a contiguous int32", ct=torch.zeros((2, 3, 3), dtype=torch.int64))
