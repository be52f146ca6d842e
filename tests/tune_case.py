"""The two-class case in which no single median width serves both classes, shared by tests/test_tune_postprocessing_cpu.py
(through the numpy restatements) and tests/test_gpu_tune_postprocessing.py (through the kernels).

Six recordings of 64 frames of R = 10240 samples, base level 0.1, clip i shifted by s = i:
class 0  0.9 on [10 + s, 50) with dropouts (0.1) at [20 + s, 22 + s) and at frame 35; reference (10 + s, 50) in frames
class 1  0.9 on [8, 10), on [30 + s, 32 + s) and spikes at frames 20 and 45 + s; references the two 2-frame events
A median of 1 or 3 frames leaves class 0 in pieces, one of 5 or more removes class 1's events."""
import numpy as np

R, G, N, K = 10240, 64, 6, 2
COLLAR, PCT = 6400, 0.2
WIDTHS = (1, 3, 5, 7, 9, 15, 31)
# (tp, n_est) per class, summed over the clips
EXPECTED = {1: ((0, 18), (12, 24)), 3: ((0, 12), (12, 12)), 5: ((6, 6), (0, 0)), 7: ((6, 6), (0, 0)), 9: ((6, 6), (0, 0)),
            15: ((6, 6), (0, 0)), 31: ((0, 6), (0, 0))}
N_REF = (6, 12)


def build():
    """-> (prob (K, N G) float32, rec rows, nsamp (N,), ref (E, 3) int32 rows (class, onset, offset) in samples, ro (N + 1,))."""
    prob = np.full((K, N * G), 0.1, dtype=np.float32)
    rec, ref, ro = [], [], [0]
    for i in range(N):
        s, x = i, prob[:, i * G:(i + 1) * G]
        x[0, 10 + s:50] = 0.9
        x[0, 20 + s:22 + s] = 0.1
        x[0, 35] = 0.1
        x[1, 8:10] = 0.9
        x[1, 30 + s:32 + s] = 0.9
        x[1, 20] = 0.9
        x[1, 45 + s] = 0.9
        rec.append((i, 1, i * G, G))
        ref += [(0, (10 + s) * R, 50 * R), (1, 8 * R, 10 * R), (1, (30 + s) * R, (32 + s) * R)]
        ro.append(len(ref))
    return prob, rec, np.full(N, G * R, dtype=np.int64), np.asarray(ref, dtype=np.int32), np.asarray(ro, dtype=np.int64)


def counts_grid(res):
    """(Mw, K, V = 1, 2) sums of (tp, n_est) over the clips -> (Mw, 1, K, 3) (tp, fp, fn)."""
    res = np.asarray(res, dtype=np.int64)
    tp, n_est = res[:, :, 0, 0], res[:, :, 0, 1]
    return np.stack([tp, n_est - tp, np.asarray(N_REF)[None, :] - tp], axis=2)[:, None]
