"""float64 reference of eat_wave_augment_ragged (efficientat_amd/csrc/ragged.hip), in numpy, written from the contract in
include/eat_hip.h (a helper, not a test module)."""
import numpy as np


def ragged_augment_ref(waves, offsets, lengths, bank_y, idx, start, shift, amp, mix, L):
    """-> (out (B, L), yy (B, 2C), win_mean (2B)) float64.  Slot k, clip i, w = min(len_i - start_k, L):
    u_k = amp_k * window, zero-padded to L; r_k = roll(u_k, shift_k); m_k = amp_k / L * sum(window);
    out = r_0 (unmixed) or l (r_0 - m_0) + (1 - l) (r_1 - m_1); yy = [y_0 or l y_0 + (1 - l) y_1 | ones];
    win_mean = m_k for the slots of mixed rows, 0 elsewhere."""
    offsets, lengths = np.asarray(offsets, dtype=np.int64), np.asarray(lengths, dtype=np.int64)
    bank_y = np.asarray(bank_y, dtype=np.float32).astype(np.float64)
    idx, start, shift = np.asarray(idx), np.asarray(start), np.asarray(shift)
    amp = np.asarray(amp, dtype=np.float32).astype(np.float64)
    mix = np.asarray(mix, dtype=np.float32).astype(np.float64)
    B, C = len(mix), bank_y.shape[1]
    out = np.zeros((B, L))
    yy = np.ones((B, 2 * C))
    win_mean = np.zeros(2 * B)

    def slot(k):
        i, st = int(idx[k]), int(start[k])
        w = min(int(lengths[i]) - st, L)
        x = np.asarray(waves[int(offsets[i]) + st:int(offsets[i]) + st + w], dtype=np.float32).astype(np.float64)
        u = np.zeros(L)
        u[:w] = amp[k] * x
        return np.roll(u, int(shift[k])), amp[k] / L * x.sum()

    for b in range(B):
        r0, m0 = slot(2 * b)
        if idx[2 * b + 1] < 0:
            out[b] = r0
            yy[b, :C] = bank_y[int(idx[2 * b])]
            continue
        r1, m1 = slot(2 * b + 1)
        lm = mix[b]
        out[b] = lm * (r0 - m0) + (1.0 - lm) * (r1 - m1)
        yy[b, :C] = lm * bank_y[int(idx[2 * b])] + (1.0 - lm) * bank_y[int(idx[2 * b + 1])]
        win_mean[2 * b], win_mean[2 * b + 1] = m0, m1
    return out, yy, win_mean
