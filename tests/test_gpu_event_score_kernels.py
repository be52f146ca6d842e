"""The event-scoring kernel (include/eat_event_score.h) against the numpy restatement (tests/event_score_ref.py): exact
integer equality of (tp, n_est) for every recording, class and threshold pair, on seeded random timelines whose values come
from a small set that holds the thresholds themselves, so that `>=` ties occur."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import ops, sed  # noqa: E402
from tests import event_score_ref as R  # noqa: E402
from tests.detect_ref import timeline_events  # noqa: E402

DEV = torch.device("cuda:0")
RS = 16                                                                       # samples per frame
GS = (1, 63, 64, 65, 129, 200)
SHORT = (0, 5, 0, 3, 15, 0)                                                   # samples the last frame of a recording lacks
LEVELS = np.asarray([0.0, 0.2, 0.3, 0.5, 0.6, 0.9], dtype=np.float32)
GAP_LEN = ((0, 0), (2, 0), (0, 3), (2, 3))
MAX_REF = ops.EVENT_SCORE_MAX_REF
SENTINEL = -77


def _rec():
    goff = np.cumsum(GS) - np.asarray(GS)
    return [(i, 1, int(o), int(g)) for i, (o, g) in enumerate(zip(goff, GS))]


def _nsamp():
    return [g * RS - s for g, s in zip(GS, SHORT)]


def _timelines(K):
    """(K, G_total) float32: a random walk over LEVELS that keeps its level with probability 0.6, with the special cases
    written in: recording 1 / class 0 never reaches the lowest threshold; in recording 4 an event straddles the 64-frame
    step and one is open at the last frame; in recording 5 two runs two frames apart lie on either side of frame 128."""
    rng = np.random.default_rng(100 + K)
    rec = _rec()
    G_total = rec[-1][2] + rec[-1][3]
    x = np.zeros((K, G_total), dtype=np.float32)
    for k in range(K):
        level = 0
        for g in range(G_total):
            if rng.random() > 0.6:
                level = int(rng.integers(len(LEVELS)))
            x[k, g] = LEVELS[level]
    g1, g4, g5 = rec[1][2], rec[4][2], rec[5][2]
    x[0, g1:g1 + 63] = 0.0
    x[0, g4 + 58:g4 + 60] = 0.0
    x[0, g4 + 60:g4 + 70] = 0.9
    x[0, g4 + 70:g4 + 72] = 0.0
    x[0, g4 + 123:g4 + 126] = 0.0
    x[0, g4 + 126:g4 + 129] = 0.9
    x[0, g5 + 120:g5 + 124] = 0.0
    x[0, g5 + 124:g5 + 127] = 0.9
    x[0, g5 + 127:g5 + 129] = 0.0
    x[0, g5 + 129:g5 + 133] = 0.9
    x[0, g5 + 133:g5 + 136] = 0.0
    return x


def _grid(V, lower):
    """V threshold pairs: hi cycles through the timeline's own levels and values between them; lo = hi, or (lower) a level
    below hi on even v and hi / 2 on odd v."""
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


def _references(x, K):
    """Reference rows near the events of the middle threshold (0.5 / 0.5, no merging): every such event gives one row, an exact
    copy in a third of the cases, else moved by up to RS / 2 + 2 samples at either end.  Recording 3's last class gets
    none; recording 5 / class 0 is filled up to MAX_REF rows with overlapping events.  -> (ref (E, 3) int32, ro)."""
    rng = np.random.default_rng(7 + K)
    rows, ro = [], [0]
    for i, ((_, _, goff, G), n) in enumerate(zip(_rec(), _nsamp())):
        mine = []
        for k in range(K):
            if i == 3 and k == K - 1 and K > 1:
                continue
            ests = R.to_samples(timeline_events(x[k, goff:goff + G], np.float32(0.5), np.float32(0.5), 0, 0), RS, n)
            for on, off in ests:
                if rng.random() > 1 / 3:
                    j = RS // 2 + 2
                    on, off = on + int(rng.integers(-j, j + 1)), off + int(rng.integers(-j, j + 1))
                on = min(max(on, 0), n - 1)
                mine.append((k, on, min(max(off, on + 1), n)))
            if i == 5 and k == 0:
                have = sum(1 for r in mine if r[0] == 0)
                for _ in range(MAX_REF - have):
                    on = int(rng.integers(0, n - 1))
                    mine.append((0, on, min(n, on + int(rng.integers(1, 6 * RS)))))
        rows.extend(sorted(mine))
        ro.append(len(rows))
    return np.asarray(rows, dtype=np.int32).reshape(-1, 3), np.asarray(ro, dtype=np.int64)


_DATA = {}


def _data(K):
    if K not in _DATA:
        x = _timelines(K)
        ref, ro = _references(x, K)
        _DATA[K] = (x, ref, ro, torch.from_numpy(x).to(DEV), ops.detect_table(np.asarray(_rec(), dtype=np.int64)))
    return _DATA[K]


def test_the_data_holds_the_cases_it_is_chosen_for():
    x, ref, ro, _, _ = _data(3)
    rec = _rec()
    per = {(i, int(c)): 0 for i in range(len(rec)) for c in range(3)}
    for i in range(len(rec)):
        for e in range(ro[i], ro[i + 1]):
            per[(i, int(ref[e, 0]))] += 1
    assert per[(5, 0)] == MAX_REF and per[(3, 2)] == 0 and max(per.values()) == MAX_REF
    assert not timeline_events(x[0, rec[1][2]:rec[1][2] + 63], 0.05, 0.05, 0, 0)              # never reaches lo
    ev4 = timeline_events(x[0, rec[4][2]:rec[4][2] + 129], 0.9, 0.9, 0, 0)
    assert (60, 70) in ev4 and ev4[-1] == (126, 129)                          # straddles frame 64; open at the last frame
    g5 = rec[5][2]
    assert (124, 127) in timeline_events(x[0, g5:g5 + 200], 0.9, 0.9, 0, 0)
    assert (124, 133) in timeline_events(x[0, g5:g5 + 200], 0.9, 0.9, 2, 0)   # a merge across frame 128
    rows = ref[ro[5]:ro[6]]
    rows = rows[rows[:, 0] == 0]
    assert bool((rows[1:, 1] < rows[:-1, 2]).any())                           # overlapping references
    assert any(n % RS for n in _nsamp())


@pytest.mark.parametrize("gap_len", GAP_LEN, ids=[f"gap{g}-len{m}" for g, m in GAP_LEN])
@pytest.mark.parametrize("lower", [False, True], ids=["lo=hi", "lo<hi"])
@pytest.mark.parametrize("V", [1, 64, 65])
@pytest.mark.parametrize("K", [1, 3])
def test_kernel_equals_the_restatement(K, V, lower, gap_len):
    x, ref, ro, d_x, table = _data(K)
    max_gap, min_len = gap_len
    hi, lo = _grid(V, lower)
    assert bool(((lo > 0) & (lo <= hi) & (hi <= 1)).all()) and (not lower or bool((lo < hi).all()))
    rec, nsamp = _rec(), _nsamp()
    mid = 0                                                                   # _grid's first pair is the middle threshold 0.5
    assert hi[mid] == np.float32(0.5)
    n_est_seen = None
    for c in (0, RS // 2):
        tol = sed.event_tolerances(ref, c, 0.2)
        want = R.score_ref(x, rec, nsamp, RS, ref, tol, ro, c, hi, lo, max_gap, min_len)
        refs = ops.event_refs(ref, tol, ro, K)
        out = torch.full((len(rec), K, V, 2), SENTINEL, device=DEV, dtype=torch.int32)
        got = ops.event_score(d_x, table, nsamp, RS, refs, c, hi, lo, max_gap, min_len, out=out)
        again = ops.event_score(d_x, table, torch.tensor(nsamp, device=DEV), RS, refs, c, torch.from_numpy(hi).to(DEV),
                                torch.from_numpy(lo).to(DEV), max_gap, min_len)
        got_h, again_h = got.cpu().numpy(), again.cpu().numpy()
        assert got.data_ptr() == out.data_ptr() and not (got_h == SENTINEL).any()
        assert np.array_equal(got_h, again_h)
        assert np.array_equal(got_h.astype(np.int64), want)
        tp_mid = int(want[:, :, mid, 0].sum())
        print(f"K={K} V={V} c={c}: tp at the middle threshold {tp_mid}, tp {int(want[..., 0].sum())}, n_est {int(want[..., 1].sum())}")
        assert tp_mid > 0 and int(want[..., 1].sum()) > int(want[..., 0].sum())
        n_est_seen = got_h[..., 1]
    # n_est is the per-timeline event count of the detection kernels at each threshold pair
    for v in range(V):
        ev_i, _ = ops.detect_events(d_x, table, np.full(K, hi[v], dtype=np.float32), np.full(K, lo[v], dtype=np.float32),
                                    max_gap, min_len)
        ev_i = ev_i.cpu().numpy()
        count = np.bincount(ev_i[:, 0].astype(np.int64) * K + ev_i[:, 1], minlength=len(rec) * K).reshape(len(rec), K)
        assert np.array_equal(count, n_est_seen[:, :, v]), v


def test_no_reference_at_all_and_a_chunk_of_a_larger_table():
    x, ref, ro, d_x, table = _data(3)
    hi, lo = _grid(5, True)
    empty = ops.event_refs(np.zeros((0, 3), dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(len(GS) + 1, dtype=np.int64), 3)
    got = ops.event_score(d_x, table, _nsamp(), RS, empty, 4, hi, lo).cpu().numpy()
    want = R.score_ref(x, _rec(), _nsamp(), RS, ref[:0], [], np.zeros(len(GS) + 1, dtype=np.int64), 4, hi, lo)
    assert np.array_equal(got, want) and not got[..., 0].any() and got[..., 1].any()
    # the same recordings as recordings [2, 8) of a table of 9: `first` moves the row ranges, not the rows
    tol = sed.event_tolerances(ref, 4, 0.2)
    pad = np.asarray([[0, 1, 9], [2, 3, 30]], dtype=np.int32)
    ref9 = np.concatenate([pad, ref, pad])
    ro9 = np.concatenate([[0, 1, 2], ro[1:] + 2, [len(ref) + 4]]).astype(np.int64)
    refs9 = ops.event_refs(ref9, np.concatenate([[4, 4], tol, [4, 4]]).astype(np.int32), ro9, 3)
    one = ops.event_score(d_x, table, _nsamp(), RS, ops.event_refs(ref, tol, ro, 3), 4, hi, lo).cpu().numpy()
    assert np.array_equal(ops.event_score(d_x, table, _nsamp(), RS, refs9, 4, hi, lo, first=2).cpu().numpy(), one)
    assert one[..., 0].any()


def test_sample_positions_are_64_bit():
    """One recording of 420 000 frames at R = 10240: a run at frame 419 431, where on R = 2^32 + 6144, and one at frame 3.
    References at onset 6144 and at 3 R, c = 0: exactly one tp and one fp - a 32-bit product would claim two tp."""
    G, Rl = 420000, 10240
    x = np.zeros((1, G), dtype=np.float32)
    x[0, 419431] = x[0, 3] = 0.9
    assert 419431 * Rl == 2 ** 32 + 6144
    ref = np.asarray([[0, 6144, 6144 + Rl], [0, 3 * Rl, 4 * Rl]], dtype=np.int32)
    ro = np.asarray([0, 2], dtype=np.int64)
    tol = sed.event_tolerances(ref, 0, 0.2)
    hi = np.asarray([0.5, 0.7], dtype=np.float32)
    rec = [(0, 1, 0, G)]
    want = R.score_ref(x, rec, [G * Rl], Rl, ref, tol, ro, 0, hi, hi)
    assert want.tolist() == [[[[1, 2], [1, 2]]]]
    table = ops.detect_table(np.asarray(rec, dtype=np.int64))
    got = ops.event_score(torch.from_numpy(x).to(DEV), table, [G * Rl], Rl, ops.event_refs(ref, tol, ro, 1), 0, hi, hi)
    assert got.cpu().numpy().tolist() == want.tolist()
