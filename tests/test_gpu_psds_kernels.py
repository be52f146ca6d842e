"""The PSDS counting kernel (include/eat_psds.h) against the numpy restatement (tests/psds_ref.py): exact integer equality of
(tp, n_det, fp, n_ct) for every recording, class and threshold pair and of the cross-trigger table, on hand-built cases that
sit on and one sample beside each criterion and on seeded random timelines whose values come from a small set that holds the
thresholds themselves, so that `>=` ties occur.  Every case also checks that the cross-trigger table sums to the per-timeline
counts and that a second call gives the same bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import ops  # noqa: E402
from tests import psds_ref as P  # noqa: E402

DEV = torch.device("cuda:0")
LEVELS = np.asarray([0.0, 0.2, 0.3, 0.5, 0.6, 0.9], dtype=np.float32)
SENTINEL = -77
MID = (np.asarray([0.5], dtype=np.float32),) * 2                              # one threshold pair, hi = lo = 0.5


def _rec(Gs):
    goff = np.cumsum(Gs) - np.asarray(Gs)
    return [(i, 1, int(o), int(g)) for i, (o, g) in enumerate(zip(goff, Gs))]


def _paint(K, Gs, runs):
    """(K, sum(Gs)) float32 of zeros with 0.9 on the frames [on, off) of every (recording, class, on, off) in `runs`."""
    rec = _rec(Gs)
    x = np.zeros((K, sum(Gs)), dtype=np.float32)
    for i, k, on, off in runs:
        assert 0 <= on < off <= Gs[i]
        x[k, rec[i][2] + on:rec[i][2] + off] = 0.9
    return x


def _refs(rows_per_rec):
    """[[(class, on, off), ...] per recording] -> (ref (E, 3) int32, ro (n + 1) int64), each recording's rows sorted."""
    rows, ro = [], [0]
    for mine in rows_per_rec:
        rows.extend(sorted(mine))
        ro.append(len(rows))
    return np.asarray(rows, dtype=np.int32).reshape(-1, 3), np.asarray(ro, dtype=np.int64)


def _grid(V, lower):
    pool = np.asarray([0.5, 0.2, 0.9, 0.3, 0.6, 0.45, 0.25, 0.75, 1.0, 0.05], dtype=np.float32)
    hi = pool[np.arange(V) % len(pool)].copy()
    hi[len(pool):] -= (np.arange(V)[len(pool):] // len(pool)).astype(np.float32) * np.float32(0.01)
    hi = np.clip(hi, np.float32(0.01), np.float32(1.0)).astype(np.float32)
    if not lower:
        return hi, hi.copy()
    lo = hi.copy()
    for v in range(V):
        below = LEVELS[(LEVELS > 0) & (LEVELS < hi[v])]
        lo[v] = below[-1] if v % 2 == 0 and below.size else hi[v] * np.float32(0.5)
    return hi, lo.astype(np.float32)


def _run(x, Gs, nsamp, R, ref, ro, crit, hi, lo, max_gap=0, min_len=0):
    """Kernel against restatement for criteria `crit` = (dtc, gtc, cttc) in per-mille -> (counts (n_rec, K, V, 4), ct (V, K, K))
    int64 of the restatement, after asserting that the kernel gives exactly them, twice, into a pre-filled ct as well."""
    K, V = x.shape[0], len(hi)
    rec = _rec(Gs)
    want, want_ct = P.count_ref(x, rec, nsamp, R, ref, ro, *crit, hi, lo, max_gap, min_len)
    assert np.array_equal(want_ct.sum(2).T, want[..., 3].sum(0))
    d_x, table = torch.from_numpy(x).to(DEV), ops.detect_table(np.asarray(rec, dtype=np.int64))
    refs = ops.event_refs(ref, np.zeros(len(ref), dtype=np.int32), ro, K)
    ratio = [c / 1000.0 for c in crit]
    out = torch.full((len(rec), K, V, 4), SENTINEL, device=DEV, dtype=torch.int32)
    got, ct = ops.psds_count(d_x, table, nsamp, R, refs, *ratio, hi, lo, max_gap, min_len, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert torch.equal(got.cpu(), torch.from_numpy(want).to(torch.int32))     # (no sentinel is left: every element is stored)
    if crit[2] == 0:
        assert ct is None and not want[..., 3].any()
    else:
        assert ct.dtype == torch.int32 and torch.equal(ct.cpu(), torch.from_numpy(want_ct).to(torch.int32))
        assert torch.equal(ct.sum(2).T.cpu(), got[..., 3].sum(0).cpu())
        seven = torch.full((V, K, K), 7, device=DEV, dtype=torch.int32)
        again, ct7 = ops.psds_count(d_x, table, torch.tensor(nsamp, device=DEV), R, refs, *ratio, torch.from_numpy(hi).to(DEV),
                                    torch.from_numpy(lo).to(DEV), max_gap, min_len, ct=seven)
        assert ct7.data_ptr() == seven.data_ptr() and torch.equal(ct7.cpu(), torch.from_numpy(want_ct + 7).to(torch.int32))
        assert torch.equal(again, got)
    again, ct2 = ops.psds_count(d_x, table, nsamp, R, refs, *ratio, hi, lo, max_gap, min_len)
    assert torch.equal(again, got) and (ct is None or torch.equal(ct2, ct))   # the same bits from call to call
    return want, want_ct


# ---------------------------------------------------------------------------------------------------- sizes
_SIZES = {}


def _size_data(K):
    if K not in _SIZES:
        Gs = (1, 63, 64, 65, 129)
        rng = np.random.default_rng(200 + K)
        x = np.zeros((K, sum(Gs)), dtype=np.float32)
        for k in range(K):
            level = 0
            for g in range(x.shape[1]):
                if rng.random() > 0.6:
                    level = int(rng.integers(len(LEVELS)))
                x[k, g] = LEVELS[level]
        R = 16
        nsamp = [g * R - s for g, s in zip(Gs, (0, 5, 0, 3, 15))]
        rows = []
        for n in nsamp:
            mine = []
            for _ in range(int(rng.integers(2, 9))):
                on = int(rng.integers(0, n))
                mine.append((int(rng.integers(0, K)), on, min(n, on + int(rng.integers(1, 20 * R)))))
            rows.append(mine)
        _SIZES[K] = (x, Gs, nsamp, R) + _refs(rows)
    return _SIZES[K]


@pytest.mark.parametrize("lower", [False, True], ids=["lo=hi", "lo<hi"])
@pytest.mark.parametrize("V", [1, 64, 65])
@pytest.mark.parametrize("K", [1, 3])
def test_kernel_equals_the_restatement_at_every_size(K, V, lower):
    x, Gs, nsamp, R, ref, ro = _size_data(K)
    hi, lo = _grid(V, lower)
    want, want_ct = _run(x, Gs, nsamp, R, ref, ro, (300, 300, 300), hi, lo, max_gap=2 if lower else 0, min_len=2 if V == 64 else 0)
    tot = want.sum((0, 1, 2))
    print(f"K={K} V={V} lower={lower}: tp {tot[0]}, n_det {tot[1]}, fp {tot[2]}, n_ct {tot[3]}")
    assert tot[0] > 0 and tot[2] > 0 and (K == 1 or V == 1 or tot[3] > 0)
    _run(x, Gs, nsamp, R, ref, ro, (700, 700, 0), hi, lo)                     # scenario 1: no cross-trigger buffer at all


def test_no_reference_at_all():
    x, Gs, nsamp, R, _, _ = _size_data(3)
    hi, lo = _grid(5, True)
    want, want_ct = _run(x, Gs, nsamp, R, np.zeros((0, 3), dtype=np.int32), np.zeros(len(Gs) + 1, dtype=np.int64), (100, 100, 300), hi, lo)
    assert not want[..., 0].any() and want[..., 1].any() and np.array_equal(want[..., 1], want[..., 2]) and not want_ct.any()


def test_a_chunk_of_a_larger_table():
    """The same recordings as recordings [2, 7) of a table of 8: `first` moves the row ranges, not the rows."""
    x, Gs, nsamp, R, ref, ro = _size_data(3)
    hi, lo = _grid(5, True)
    want, want_ct = _run(x, Gs, nsamp, R, ref, ro, (300, 300, 300), hi, lo)
    pad = np.asarray([[0, 1, 9], [2, 3, 30]], dtype=np.int32)
    ref8 = np.concatenate([pad, ref, pad[:1]])
    ro8 = np.concatenate([[0, 1, 2], ro[1:] + 2, [len(ref) + 3]]).astype(np.int64)
    refs8 = ops.event_refs(ref8, np.zeros(len(ref8), dtype=np.int32), ro8, 3)
    table = ops.detect_table(np.asarray(_rec(Gs), dtype=np.int64))
    got, ct = ops.psds_count(torch.from_numpy(x).to(DEV), table, nsamp, R, refs8, 0.3, 0.3, 0.3, hi, lo, first=2)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(ct.cpu().numpy(), want_ct) and want[..., 0].any()


# ---------------------------------------------------------------------------------------------------- the criteria
def test_dtc_gtc_and_cttc_exactly_on_the_ratio_and_one_sample_short():
    R, Gs = 10, (100, 100)
    # DTC: L = 1000, intersection 700 against 699 at 700 per mille
    x = _paint(1, Gs, [(0, 0, 0, 100), (1, 0, 0, 100)])
    want, _ = _run(x, Gs, [1000, 1000], R, *_refs([[(0, 300, 1000)], [(0, 301, 1000)]]), (700, 100, 0), *MID)
    assert want[:, 0, 0, :3].tolist() == [[1, 1, 0], [0, 1, 1]]
    # GTC: a reference of 1000 covered by 700 against 699 (the second recording ends at sample 699)
    x = _paint(1, Gs, [(0, 0, 0, 70), (1, 0, 0, 70)])
    want, _ = _run(x, Gs, [1000, 699], R, *_refs([[(0, 0, 1000)], [(0, 0, 1000)]]), (700, 700, 0), *MID)
    assert want[:, 0, 0, :3].tolist() == [[1, 1, 0], [0, 1, 0]]
    # CTTC: a false positive of class 0 over class 1 (300 of 1000: on the ratio) and class 2 (299: short)
    x = _paint(3, Gs[:1], [(0, 0, 0, 100)])
    want, ct = _run(x, Gs[:1], [1000], R, *_refs([[(1, 0, 300), (2, 0, 299)]]), (700, 700, 300), *MID)
    assert want[0, :, 0].tolist() == [[0, 1, 1, 1], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert ct[0].tolist() == [[0, 1, 0], [0, 0, 0], [0, 0, 0]]
    # ... split over two rows of class 2 that add up to the ratio, with class 0's own rows in between the two classes' runs
    want, ct = _run(x, Gs[:1], [1000], R, *_refs([[(0, 0, 100), (1, 0, 299), (2, 0, 150), (2, 100, 250)]]), (700, 700, 300), *MID)
    assert want[0, 0, 0].tolist() == [0, 1, 1, 1] and ct[0, 0].tolist() == [0, 0, 1]


def test_intersections_add_and_only_relevant_detections_cover():
    R = 10
    # a detection over two references of its class; references that overlap each other: both add up to 700 per mille
    x = _paint(1, (10, 10), [(0, 0, 0, 10), (1, 0, 0, 10)])
    want, _ = _run(x, (10, 10), [100, 100], R, *_refs([[(0, 0, 35), (0, 65, 100)], [(0, 0, 35), (0, 0, 35)]]), (700, 1000, 0), *MID)
    assert want[:, 0, 0, :3].tolist() == [[2, 1, 0], [2, 1, 0]]
    # a reference [0, 100) under the detections [0, 50) (relevant) and [60, 300) (40 of 240: fails DTC): its coverage is 50, not 90
    x = _paint(1, (30,), [(0, 0, 0, 5), (0, 0, 6, 30)])
    for gtc, tp in ((500, 1), (510, 0), (900, 0)):
        want, _ = _run(x, (30,), [300], R, *_refs([[(0, 0, 100)]]), (700, gtc, 0), *MID)
        assert want[0, 0, 0, :3].tolist() == [tp, 2, 1]
    # a relevant detection that overlaps another class raises no cross-trigger
    x = _paint(2, (10,), [(0, 0, 0, 10)])
    want, ct = _run(x, (10,), [100], R, *_refs([[(0, 0, 100), (1, 0, 100)]]), (700, 700, 300), *MID)
    assert want[0, :, 0].tolist() == [[1, 1, 0, 0], [0, 0, 0, 0]] and not ct.any()
    # a zero-length reference counts for nothing, wherever it lies
    want, _ = _run(x[:1], (10,), [100], R, *_refs([[(0, 0, 100), (0, 50, 50)]]), (700, 1, 0), *MID)
    assert want[0, 0, 0, :3].tolist() == [1, 1, 0]


def test_event_formation_merge_drop_and_clip():
    R, Gs = 10, (129,)
    x = _paint(1, Gs, [(0, 0, 60, 63), (0, 0, 65, 70), (0, 0, 100, 102), (0, 0, 126, 129)])
    ref = _refs([[(0, 600, 700), (0, 1000, 1020), (0, 1260, 1285)]])
    # every detection lies inside a reference; [600, 630) and [650, 700) cover 80 of the first reference's 100 samples
    want, _ = _run(x, Gs, [1285], R, *ref, (700, 900, 0), *MID)
    assert want[0, 0, 0, :3].tolist() == [2, 4, 0]
    want, _ = _run(x, Gs, [1285], R, *ref, (700, 900, 0), *MID, max_gap=2)    # merged across frame 64: [600, 700) covers it all
    assert want[0, 0, 0, :3].tolist() == [3, 3, 0]
    want, _ = _run(x, Gs, [1285], R, *ref, (700, 900, 0), *MID, max_gap=2, min_len=3)   # [1000, 1020) is dropped
    assert want[0, 0, 0, :3].tolist() == [2, 2, 0]
    # the last detection is clipped to the recording: [1260, 1285) is 25 samples, all inside the reference; unclipped it
    # would be 30 samples of which 25 / 30 < 900 per mille
    want, _ = _run(x, Gs, [1285], R, *ref, (900, 700, 0), *MID, max_gap=2, min_len=3)
    assert want[0, 0, 0, :3].tolist() == [2, 2, 0]
    want, _ = _run(x, Gs, [1290], R, *ref, (900, 700, 0), *MID, max_gap=2, min_len=3)
    assert want[0, 0, 0, :3].tolist() == [1, 2, 1]


def test_64_references_of_one_class_among_200_rows_of_other_classes():
    rng = np.random.default_rng(17)
    K, R, G = 5, 16, 200
    n = G * R
    mine = []
    for k, count in ((0, 50), (1, 50), (2, ops.EVENT_SCORE_MAX_REF), (3, 50), (4, 50)):
        for _ in range(count):
            on = int(rng.integers(0, n - 1))
            mine.append((k, on, min(n, on + int(rng.integers(1, 12 * R)))))
    x = LEVELS[rng.integers(0, len(LEVELS), size=(K, G // 4))].repeat(4, axis=1).astype(np.float32)
    hi, lo = _grid(7, True)
    want, want_ct = _run(x, (G,), [n], R, *_refs([mine]), (300, 300, 100), hi, lo)
    assert want[0, 2, :, 0].max() > 10 and want_ct[:, 2].any() and want_ct[:, :, 2].any()


def test_sample_positions_and_products_are_64_bit():
    """R = 2^22 and 1100 frames: the detection of frames [0, 300) is L = 1 258 291 200 samples long, so 700 L and 1000 S pass
    2^32 by far, and it is judged against a reference of exactly 0.7 L and one a sample shorter; the detection of frames
    [1030, 1040) starts at sample 2^32 + 25 165 824, past every int32 reference row, and is a false positive without a
    cross-trigger - a 32-bit product would wrap it onto the rows that start at 0."""
    R, Gs = 2 ** 22, (1100, 1100)
    L = 300 * R
    assert 7 * L % 10 == 0 and 0 < 1030 * R - 2 ** 32 < L and 1000 * (7 * L // 10) > 2 ** 32
    x = _paint(2, Gs, [(0, 0, 0, 300), (0, 0, 1030, 1040), (1, 0, 0, 300), (1, 0, 1030, 1040)])
    top = 2 ** 31 - 1
    rows = [[(0, 0, 7 * L // 10), (1, 0, top)], [(0, 0, 7 * L // 10 - 1), (1, 0, top)]]
    want, ct = _run(x, Gs, [1100 * R, 1100 * R], R, *_refs(rows), (700, 700, 300), *MID)
    # recording 0: [0, 300) is relevant and covers its reference; [1030, 1040) is a false positive, no cross-trigger.
    # recording 1: [0, 300) misses DTC by one sample and cross-triggers class 1, whose row covers all of it.
    assert want[:, 0, 0].tolist() == [[1, 2, 1, 0], [0, 2, 2, 1]] and ct[0].tolist() == [[0, 1], [0, 0]]


def test_seeded_random_timelines():
    rng = np.random.default_rng(23)
    n_rec, K, V, R = 24, 5, 70, 16
    Gs = tuple(int(g) for g in rng.integers(1, 41, size=n_rec))
    x = np.zeros((K, sum(Gs)), dtype=np.float32)
    for k in range(K):
        level = 0
        for g in range(x.shape[1]):
            if rng.random() > 0.6:
                level = int(rng.integers(len(LEVELS)))
            x[k, g] = LEVELS[level]
    nsamp = [max(1, g * R - int(rng.integers(0, R))) for g in Gs]
    rows = []
    for n in nsamp:
        mine = []
        for _ in range(int(rng.integers(0, 10))):
            on = int(rng.integers(0, n))
            mine.append((int(rng.integers(0, K)), on, min(n, on + int(rng.integers(0, 12 * R)))))
        rows.append(mine)
    ref, ro = _refs(rows)
    hi, lo = _grid(V, True)
    for crit, gap_len in (((100, 100, 300), (1, 0)), ((700, 700, 0), (0, 2)), ((500, 900, 1000), (2, 2))):
        want, want_ct = _run(x, Gs, nsamp, R, ref, ro, crit, hi, lo, *gap_len)
        tot = want.sum((0, 1, 2))
        print(f"random {crit}: tp {tot[0]}, n_det {tot[1]}, fp {tot[2]}, n_ct {tot[3]}")
        assert tot[0] > 0 and tot[2] > 0 and (crit[2] == 0 or tot[3] > 0 or crit[2] == 1000)
