"""Host side of sound event detection, no GPU: the window / frame plan against brute-force enumeration, the references of
tests/detect_ref.py against scipy and hand-worked timelines, the ms -> frame conversions, every refusal of
`detection` and of the `ops` wrappers (which fire from tensor metadata before the library is touched), and the header."""
import contextlib
import io
import types

import numpy as np
import pytest
import torch

from efficientat_amd import detection, ops
from efficientat_amd._lib import EatHipError
from tests import detect_ref as R

GEO = detection.frame_geometry(32, 320, 32000, 10.24, 5.12)


# ------------------------------------------------------------------------------------------------ geometry
def test_default_geometry():
    assert GEO == (32, 10240, 0.32, 327680, 163840, 32, 16)
    g = detection.frame_geometry(32, 320, 32000, 0.64, 0.32)
    assert (g.W, g.Hs, g.T, g.Hf) == (20480, 10240, 2, 1)
    assert detection.frame_geometry(32, 320, 32000, 0.32, 0.32).T == 1
    for clip, hop in ((10.0, 5.12), (10.24, 5.0), (0.0, 0.32), (10.24, 0.0), (-0.32, 0.32), (float("nan"), 0.32), (0.1, 0.1)):
        with pytest.raises(ValueError, match="R = 10240"):
            detection.frame_geometry(32, 320, 32000, clip, hop)
    with pytest.raises(ValueError, match="exceeds clip_seconds.*R = 10240"):
        detection.frame_geometry(32, 320, 32000, 5.12, 10.24)


@pytest.mark.parametrize("clip,hop", [(10.24, 5.12), (10.24, 10.24), (0.96, 0.32), (0.32, 0.32)])
def test_plan_against_brute_force(clip, hop):
    geo = detection.frame_geometry(32, 320, 32000, clip, hop)
    Rs, W, Hs, T, Hf = geo.R, geo.W, geo.Hs, geo.T, geo.Hf
    lengths = [1, Rs - 1, Rs, Rs + 1, W - 1, W, W + 1, W + Hs, W + Hs + 1, 7 * W + 3]
    for n in lengths:
        n_w, valid, G = detection.frame_plan(n, geo)
        want_G = len([g for g in range(n // Rs + 2) if g * Rs < n])             # frames that begin inside the recording
        want_w = 1
        while (want_w - 1) * Hs + W < n:
            want_w += 1
        assert (n_w, G) == (want_w, want_G), n
        assert [int(v) for v in valid] == [len(range(q * Hs, min(q * Hs + W, n))) for q in range(n_w)]
        assert (n_w - 1) * Hs + int(valid[-1]) == n and int(valid.min()) >= 1    # the last window reaches n, none is empty
        frames = {q * Hf + j for q in range(n_w) for j in range(T) if q * Hf + j < G}
        assert frames == set(range(G))                                           # every frame < G, none >= G
        assert all(q * Hf * Rs < n for q in range(n_w))                          # every window's first column exists
        print(f"plan clip={clip} hop={hop} n={n}: n_w={n_w} G={G} last valid={int(valid[-1])}")
    starts, valids, table = detection.EADetector.plan(types.SimpleNamespace(geometry=geo), lengths)
    rec, base, first, goff = table.cpu.tolist(), 0, 0, 0
    for n, row in zip(lengths, rec):
        n_w, valid, G = detection.frame_plan(n, geo)
        assert row == [first, n_w, goff, G]
        assert list(starts[first:first + n_w]) == [base + q * Hs for q in range(n_w)]
        assert list(valids[first:first + n_w]) == list(valid)
        base, first, goff = base + n, first + n_w, goff + G
    assert table.G_total == goff and table.n_rec == len(lengths) and len(starts) == first
    with pytest.raises(ValueError, match="empty recording"):
        detection.frame_plan(0, geo)


def test_ms_to_frames_and_thresholds():
    f = GEO.frame_s
    assert [detection.ms_to_frames(ms, f) for ms in (0, 100, 159.9, 160, 320, 479, 480, 960, 1000)] == [0, 0, 0, 1, 1, 1, 2, 3, 3]
    assert [detection.median_frames(ms, f) for ms in (0, 160, 320, 640, 960, 1280, 9920)] == [1, 1, 1, 3, 3, 5, 31]
    for ms in (10400, 1e9):
        with pytest.raises(ValueError, match="the filter takes 1 to 31"):
            detection.median_frames(ms, f)
    for ms in (-1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite and not negative"):
            detection.ms_to_frames(ms, f)
    hi, lo = detection.thresholds(0.5, None, 3)
    assert hi.dtype == np.float32 and hi.tolist() == [0.5] * 3 and lo.tolist() == [0.5] * 3
    hi, lo = detection.thresholds([0.5, 0.6, 1.0], 0.25, 3)
    assert lo.tolist() == [0.25] * 3 and hi[1] == np.float32(0.6)
    for t, low in ((0.0, None), (1.5, None), (0.5, 0.6), (0.5, 0.0), (float("nan"), None), ([0.5, 0.5, 0.0], None)):
        with pytest.raises(ValueError, match="0 < low_threshold <= threshold <= 1"):
            detection.thresholds(t, low, 3)
    for t, low in (([0.5, 0.5], None), (0.5, [0.1] * 4), ([[0.5] * 3], None)):
        with pytest.raises(ValueError, match="one value per class, K = 3"):
            detection.thresholds(t, low, 3)
    assert ops.detect_weights(1).tolist() == [1.0] and ops.detect_weights(5).tolist() == [1, 2, 3, 2, 1]
    assert ops.detect_weights(4).tolist() == [1, 2, 2, 1] and ops.detect_weights(3, "uniform").tolist() == [1, 1, 1]
    with pytest.raises(ValueError, match="taper"):
        ops.detect_weights(3, "hann")


# ------------------------------------------------------------------------------------------------ references
def test_median_ref_is_scipy_reflect_wherever_the_window_fits():
    from scipy.ndimage import median_filter
    rng = np.random.default_rng(5)
    agree = 0
    for G in (1, 2, 3, 4, 5, 7, 30, 31, 64, 65, 300):
        for m in (1, 3, 5, 9, 31):
            if m // 2 > G:
                continue
            for x in (rng.random(G), np.round(rng.random(G), 1)):
                got = R.median_ref(x[None, :], [(0, 1, 0, G)], m)[0]
                assert np.array_equal(got, median_filter(x, size=m, mode="reflect")), (G, m)
                agree += 1
    print(f"median_ref == scipy reflect on {agree} inputs")
    assert agree == 2 * 45
    # the short recordings, by hand: the contract is the periodic reflection, not scipy
    assert [R.reflect_index(j, 3) for j in range(-7, 8)] == [0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1]
    assert [R.reflect_index(j, 1) for j in range(-3, 4)] == [0] * 7
    one = np.array([[0.3]], dtype=np.float32)
    assert R.median_ref(one, [(0, 1, 0, 1)], 31).tolist() == one.tolist()          # every sample is the one there is
    # G = 2, m = 9 at i = 0 reads indices 0 1 1 0 0 1 1 0 0: five times x[0] -> x[0]; at i = 1 five times x[1]
    assert R.median_ref(np.array([[0.9, 0.1]]), [(0, 1, 0, 2)], 9).tolist() == [[0.9, 0.1]]
    assert R.median_ref(np.array([[0.9, 0.1]]), [(0, 1, 0, 2)], 31).tolist() == [[0.1, 0.9]]   # 16 x the other one
    # G = 3, m = 9, x = 1 2 3 at i = 0 reads 3 3 2 1 1 2 3 3 2 -> sorted 1 1 2 2 [2] 3 3 3 3
    assert R.median_ref(np.array([[1.0, 2.0, 3.0]]), [(0, 1, 0, 3)], 9).tolist() == [[2.0, 2.0, 2.0]]
    # two recordings side by side do not see each other
    x = np.array([[0.1, 0.1, 0.1, 0.9, 0.9]])
    assert R.median_ref(x, [(0, 1, 0, 3), (1, 1, 3, 2)], 5).tolist() == x.tolist()
    assert R.median_ref(x, [(0, 1, 0, 5)], 5).tolist() == [[0.1, 0.1, 0.1, 0.9, 0.9]]
    assert R.median_ref(x, [(0, 1, 0, 5)], 3).tolist() == [[0.1, 0.1, 0.1, 0.9, 0.9]]
    y = np.array([[0.1, 0.9, 0.1, 0.9, 0.9]])
    assert R.median_ref(y, [(0, 1, 0, 5)], 3).tolist() == [[0.1, 0.1, 0.9, 0.9, 0.9]]


def test_events_ref_on_hand_worked_timelines():
    E = R.timeline_events
    a, b, z = 0.6, 0.4, 0.1                                    # reaches hi = 0.5; between lo = 0.3 and hi; below lo
    assert E([a, z, z, a], 0.5, 0.3, 0, 0) == [(0, 1), (3, 4)]                   # events at frame 0 and at the last frame
    assert E([z, b, b, z], 0.5, 0.3, 0, 0) == []                                 # a run that never reaches hi
    assert E([z, b, a, b, z], 0.5, 0.3, 0, 0) == [(1, 4)]                        # the run is the event, not the peak alone
    assert E([z, b, a, b, z], 0.5, 0.5, 0, 0) == [(2, 3)]                        # lo == hi
    assert E([a, z, z, a], 0.5, 0.3, 2, 0) == [(0, 4)]                           # a gap of exactly max_gap: merged
    assert E([a, z, z, z, a], 0.5, 0.3, 2, 0) == [(0, 1), (4, 5)]                # max_gap + 1: not merged
    assert E([a, a, z, a], 0.5, 0.3, 0, 2) == [(0, 2)]                           # exactly min_len stays, one less goes
    assert E([a, z, a, z, z, z, a], 0.5, 0.3, 1, 3) == [(0, 3)]                  # merge first, then drop
    assert E([a, z, a], 0.5, 0.3, 0, 2) == []                                    # (without the merge both are too short)
    assert E([a, z, b, z, a], 0.5, 0.3, 3, 0) == [(0, 5)]                        # a run that does not count is part of the gap
    assert E([a, z, b, z, a], 0.5, 0.3, 2, 0) == [(0, 1), (4, 5)]
    assert E([a, a, a], 0.5, 0.3, 0, 0) == [(0, 3)] and E([z, z], 0.5, 0.3, 5, 0) == [] and E([], 0.5, 0.3, 0, 0) == []
    assert E([0.5], 0.5, 0.5, 0, 0) == [(0, 1)]                                  # >= on both thresholds
    filt = np.array([[a, a, z, a, b], [z, a, a, z, z]], dtype=np.float32)
    ev, peak, mean = R.events_ref(filt, [(0, 1, 0, 2), (1, 1, 2, 3)], [0.5, 0.5], [0.3, 0.3])
    # recording A ends active and B starts inactive / active: per-recording timelines, sorted by (recording, class, onset)
    assert ev.tolist() == [[0, 0, 0, 2], [0, 1, 1, 2], [1, 0, 1, 3], [1, 1, 0, 1]] and ev.dtype == np.int32
    assert peak.tolist() == [np.float32(a)] * 4 and peak.dtype == np.float32
    assert mean.tolist() == [float(np.float32(a)), float(np.float32(a)), (float(np.float32(a)) + float(np.float32(b))) / 2,
                             float(np.float32(a))]
    ev, peak, mean = R.events_ref(filt, [(0, 1, 0, 5)], [0.5, 0.7], [0.3, 0.3])     # per-class thresholds
    assert ev.tolist() == [[0, 0, 0, 2], [0, 0, 3, 5]]
    ev, peak, mean = R.events_ref(filt[:, :2] * 0, [(0, 1, 0, 2)], 0.5, 0.5)
    assert ev.shape == (0, 4) and peak.shape == (0,) and mean.shape == (0,)


def test_stitch_ref_by_hand():
    p = np.zeros((2, 1, 4))
    p[0, 0, :3] = [0.0, 100.0, -100.0]
    p[1, 0, :3] = [100.0, 0.0, 0.0]
    p[:, :, 3] = np.nan                                        # the pad column
    got = R.stitch_ref(p, [(0, 2, 0, 4)], 1, 3, [1.0, 2.0, 1.0])
    # frame 0: window 0 col 0; frame 1: w0 c1 (2) + w1 c0 (1); frame 2: w0 c2 (1) + w1 c1 (2); frame 3: w1 c2
    assert np.allclose(got, [[0.5, 1.0, (0.0 + 2 * 0.5) / 3, 0.5]], atol=1e-15)
    got = R.stitch_ref(p, [(0, 1, 0, 2), (1, 1, 2, 1)], 3, 3, [1.0, 1.0, 1.0])      # columns past G are not read
    assert np.allclose(got, [[0.5, 1.0, 1.0]], atol=1e-15)


# ------------------------------------------------------------------------------------------------ refusals
def _tiny(head="mlp", **kw):
    from efficientat_amd.mn import get_model
    with contextlib.redirect_stdout(io.StringIO()):
        return get_model(width_mult=0.1, num_classes=7, head_type=head, **kw)


def test_what_detection_refuses_without_a_gpu():
    model = _tiny().eval()
    assert detection.check_model(model) == (model.features[-1].out_channels, 32, 7)
    assert detection.check_model(_tiny("fully_convolutional").eval())[2] == 7
    with pytest.raises(ValueError, match="multihead_attention_pooling head has no frame-level logits"):
        detection.check_model(_tiny("multihead_attention_pooling"))
    with pytest.raises(ValueError, match="multihead_attention_pooling"):
        detection.EADetector(model=_tiny("multihead_attention_pooling").eval())
    with pytest.raises(TypeError, match=r"_forward_impl\(x, return_fmaps=True\)"):
        detection.EADetector(model=torch.nn.Linear(4, 4))
    with pytest.raises(TypeError, match=r"_forward_impl\(x, return_fmaps=True\)"):
        detection.frame_logits(torch.nn.Linear(4, 4), torch.zeros(1, 4, 1, 1))
    with pytest.raises(ValueError, match="eval mode"):
        detection.EADetector(model=_tiny().train())
    with pytest.raises(ValueError, match="eval mode"):
        detection.frame_logits(_tiny().train(), torch.zeros(1, model.features[-1].out_channels, 4, 2))
    with pytest.raises(ValueError, match="last feature map"):
        detection.frame_logits(model, torch.zeros(1, 5, 4, 2))
    with pytest.raises(ValueError, match="provide a model name"):
        detection.EADetector()
    with pytest.raises(ValueError, match="R = 10240"):
        detection.EADetector(model=model, clip_seconds=10.0)
    with pytest.raises(ValueError, match="R = 10240"):
        detection.EADetector(model=model, hop_seconds=5.0)
    with pytest.raises(ValueError, match="taper"):
        detection.EADetector(model=model, taper="hann")
    with pytest.raises(ValueError, match="batch_windows"):
        detection.EADetector(model=model, batch_windows=0)
    with pytest.raises(ValueError, match="labels holds 3 names"):
        detection.EADetector(model=model, labels=["a", "b", "c"])


def _table():
    return ops.detect_table([[0, 2, 0, 5], [2, 1, 5, 3]])            # 3 windows, 8 frames


TABLE_REFUSALS = [
    ("integers", [[0.0, 1.0, 0.0, 1.0]]),
    ("integers", [0, 1, 0, 1]),
    ("integers", np.zeros((0, 4), dtype=np.int64)),
    ("integers", [[0, 1, 0]]),
    ("ragged", [[0, 1, 0, 1], [1, 1]]),
    ("first >= 0", [[-1, 1, 0, 1]]),
    ("count >= 1", [[0, 0, 0, 1]]),
    ("G >= 1", [[0, 1, 0, 0]]),
    ("goff", [[0, 1, 1, 4]]),
    ("goff", [[0, 1, 0, 4], [1, 1, 5, 2]]),
    ("goff", [[0, 1, 0, 4], [1, 1, 3, 2]]),
    ("2\\^31", [[0, 1, 0, 2 ** 30], [1, 1, 2 ** 30, 2 ** 30]]),
]


@pytest.mark.parametrize("what,rec", TABLE_REFUSALS, ids=[f"{w}-{i}" for i, (w, _) in enumerate(TABLE_REFUSALS)])
def test_table_refusals(what, rec):
    with pytest.raises(EatHipError, match=f"detect_table: .*{what}"):
        ops.detect_table(rec)


def test_table_holds_what_it_was_given():
    t = _table()
    assert (t.n_rec, t.G_total) == (2, 8) and t.cpu.dtype == torch.int32 and t.cpu.is_contiguous()
    assert t.cpu.tolist() == [[0, 2, 0, 5], [2, 1, 5, 3]]


def _stitch(**over):
    a = dict(p=torch.zeros(3, 2, 4), table=_table(), Hf=2, T=4, wt=torch.ones(4))
    a.update(over)
    return a


_BUF = torch.zeros(64)

STITCH_REFUSALS = [
    ("p", dict(p=torch.zeros(3, 8))),
    ("p", dict(p=torch.zeros(0, 2, 4))),
    ("p", dict(p=None)),
    ("p", dict(p=torch.zeros(3, 2, 4, dtype=torch.float64))),
    ("p", dict(p=torch.zeros(3, 2, 8)[:, :, ::2])),
    ("table", dict(table=[[0, 3, 0, 8]])),
    ("table names window 2", dict(p=torch.zeros(2, 2, 4))),
    ("table row 0", dict(Hf=1, T=3, wt=torch.ones(3))),            # 2 windows of 3 frames every 1 cover 4 frames, not 5
    ("T=5", dict(T=5, wt=torch.ones(5))),
    ("T=0", dict(T=0, wt=torch.ones(0))),
    ("Hf=5", dict(Hf=5)),
    ("Hf=0", dict(Hf=0)),
    ("wt", dict(wt=torch.ones(3))),
    ("wt", dict(wt=torch.ones(4, dtype=torch.float64))),
    ("wt", dict(wt=torch.ones(8)[::2])),
    ("wt", dict(wt=[1.0] * 4)),
    ("out", dict(out=torch.zeros(2, 7))),
    ("out", dict(out=torch.zeros(2, 8, dtype=torch.float64))),
    ("out must not overlap p", dict(p=_BUF[:24].view(3, 2, 4), out=_BUF[16:32].view(2, 8))),
]


@pytest.mark.parametrize("what,over", STITCH_REFUSALS, ids=[f"{w}-{i}" for i, (w, _) in enumerate(STITCH_REFUSALS)])
def test_stitch_refusals(what, over):
    with pytest.raises(EatHipError, match=f"detect_stitch: .*{what}"):
        ops.detect_stitch(**_stitch(**over))


def _median(**over):
    a = dict(prob=torch.zeros(2, 8), table=_table(), m=3)
    a.update(over)
    return a


MEDIAN_REFUSALS = [
    ("prob", dict(prob=torch.zeros(16))),
    ("prob", dict(prob=torch.zeros(2, 8, dtype=torch.float16))),
    ("prob", dict(prob=torch.zeros(8, 2).t())),
    ("prob has 7 columns", dict(prob=torch.zeros(2, 7))),
    ("table", dict(table=None)),
    ("m=2", dict(m=2)),
    ("m=0", dict(m=0)),
    ("m=33", dict(m=33)),
    ("m=-1", dict(m=-1)),
    ("m=2.5", dict(m=2.5)),
    ("out", dict(out=torch.zeros(2, 9))),
    ("out must not overlap prob", dict(prob=_BUF[:16].view(2, 8), out=_BUF[:16].view(2, 8))),
    ("out must not overlap prob", dict(prob=_BUF[:16].view(2, 8), out=_BUF[15:31].view(2, 8))),
]


@pytest.mark.parametrize("what,over", MEDIAN_REFUSALS, ids=[f"{w}-{i}" for i, (w, _) in enumerate(MEDIAN_REFUSALS)])
def test_median_refusals(what, over):
    with pytest.raises(EatHipError, match=f"detect_median: .*{what}"):
        ops.detect_median(**_median(**over))


def _events(**over):
    a = dict(filt=torch.zeros(2, 8), table=_table(), hi=0.5, lo=0.3)
    a.update(over)
    return a


EVENTS_REFUSALS = [
    ("filt", dict(filt=torch.zeros(2, 2, 4))),
    ("filt", dict(filt=torch.zeros(2, 8, dtype=torch.float64))),
    ("filt has 9 columns", dict(filt=torch.zeros(2, 9))),
    ("table", dict(table="t")),
    ("max_gap", dict(max_gap=-1)),
    ("min_len", dict(min_len=-2)),
    ("hi must be a scalar or hold K = 2", dict(hi=[0.5, 0.5, 0.5])),
    ("lo must be a scalar or hold K = 2", dict(lo=[[0.3, 0.3]])),
    ("0 < lo <= hi <= 1", dict(hi=0.2)),
    ("0 < lo <= hi <= 1", dict(lo=0.0)),
    ("0 < lo <= hi <= 1", dict(hi=1.01)),
    ("0 < lo <= hi <= 1", dict(hi=[0.5, float("nan")])),
    ("0 < lo <= hi <= 1", dict(lo=[0.3, 0.6])),
]


@pytest.mark.parametrize("what,over", EVENTS_REFUSALS, ids=[f"{w}-{i}" for i, (w, _) in enumerate(EVENTS_REFUSALS)])
def test_events_refusals(what, over):
    with pytest.raises(EatHipError, match=f"detect_events: .*{what}"):
        ops.detect_events(**_events(**over))


def test_well_formed_cpu_calls_stop_at_the_residency_check():
    with pytest.raises(EatHipError, match="detect_stitch: p must live on the GPU"):
        ops.detect_stitch(**_stitch())
    with pytest.raises(EatHipError, match="detect_median: prob must live on the GPU"):
        ops.detect_median(**_median())
    with pytest.raises(EatHipError, match="detect_events: filt must live on the GPU"):
        ops.detect_events(**_events())
    with pytest.raises(EatHipError, match="pw_conv_into: out"):
        ops.pw_conv_into(torch.zeros(1, 4, 1, 4), (torch.zeros(64), torch.zeros(2), "fp32"), 2, ops.ACT_NONE, torch.zeros(7))


# ------------------------------------------------------------------------------------------------ header and build
def test_the_detect_header_parses_is_disjoint_from_the_other_headers_and_is_bound():
    import ctypes
    import os
    from efficientat_amd import _lib, build
    P, I = ctypes.c_void_p, ctypes.c_int
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "eat_detect.h")) as f:
        protos = _lib.parse_prototypes(f.read())
    assert protos == _lib.DETECT_PROTOTYPES
    assert set(protos) == {"eat_detect_stitch", "eat_detect_median", "eat_detect_events_count", "eat_detect_events_write"}
    assert protos["eat_detect_stitch"] == (I, [P, I, I, I, P, I, I, I, P, P, I, P])
    assert protos["eat_detect_median"] == (I, [P, I, I, P, I, I, P, P])
    assert protos["eat_detect_events_count"] == (I, [P, I, I, P, I, P, P, I, I, P, P])
    assert protos["eat_detect_events_write"] == (I, [P, I, I, P, I, P, P, I, I, P, P, P, P])
    for other in (_lib.PROTOTYPES, _lib.TAG_PROTOTYPES, _lib.EMBED_PROTOTYPES, _lib.ATTN_PROTOTYPES):
        assert not set(protos) & set(other)
    assert "detect.hip" in build.SOURCES
    build.build()
    for name, (restype, args) in protos.items():
        fn = getattr(_lib.lib(), name)
        assert list(fn.argtypes) == args and fn.restype is restype, name
    # argument checks that return before anything touches the device
    with pytest.raises(EatHipError, match="eat_detect_stitch: missing operand"):
        _lib.call("eat_detect_stitch", None, 1, 1, 1, None, 1, 1, 1, None, None, 1, None)
    with pytest.raises(EatHipError, match="eat_detect_median: missing operand"):
        _lib.call("eat_detect_median", None, 1, 1, None, 1, 1, None, None)
    with pytest.raises(EatHipError, match="eat_detect_events_count: missing operand"):
        _lib.call("eat_detect_events_count", None, 1, 1, None, 1, None, None, 0, 0, None, None)
    with pytest.raises(EatHipError, match="eat_detect_events_write: missing operand"):
        _lib.call("eat_detect_events_write", None, 1, 1, None, 1, None, None, 0, 0, None, None, None, None)
    one = ctypes.c_void_p(16)                                    # a non-null pointer that is never dereferenced
    with pytest.raises(EatHipError, match="eat_detect_median: m=4 must be odd"):
        _lib.call("eat_detect_median", one, 1, 1, one, 1, 4, ctypes.c_void_p(32), None)
    with pytest.raises(EatHipError, match="eat_detect_median: filt must not be prob"):
        _lib.call("eat_detect_median", one, 1, 1, one, 1, 3, one, None)
    with pytest.raises(EatHipError, match="eat_detect_stitch: need .* 1 <= Hf <= T <= Tp"):
        _lib.call("eat_detect_stitch", one, 1, 1, 4, one, 1, 5, 4, one, one, 1, None)
    with pytest.raises(EatHipError, match="eat_detect_events_count: need max_gap, min_len >= 0"):
        _lib.call("eat_detect_events_count", one, 1, 1, one, 1, one, one, -1, 0, one, None)
