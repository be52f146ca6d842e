"""fp64 references of the embedding extractor (efficientat_amd/embeddings.py, include/eat_embed.h).  Helpers, not tests."""
import math

import numpy as np

# cumulative time strides of the 17 maps of the MobileNetV3 table with strides (2, 2, 2, 2): stem, 15 blocks, last conv
MN_STRIDES = [2, 2, 4, 4, 8, 8, 8, 16, 16, 16, 16, 16, 16, 32, 32, 32, 32]


def mn_widths(T_mel):
    """T_l of the 17 maps for T_mel input frames: every stride-2 conv is 3x3 / 5x5 'same' padded, T -> (T - 1) // 2 + 1."""
    out, T, r = [], T_mel, 1
    for s in MN_STRIDES:
        while r < s:
            T, r = (T - 1) // 2 + 1, r * 2
        out.append(T)
    return out


def embed_pool_ref(maps, lo, hi):
    """maps: list of (B, C_l, F_l, T_l) arrays; lo, hi (n_maps, n_seg) -> (B, n_seg, sum C_l) float64, the segment means
    out[b, s, off_l + c] = mean of maps[l][b, c, :, lo[l, s]:hi[l, s]]; bounds are clamped into [0, T_l] and an empty
    segment gives 0.0 (what the kernel promises for unvalidated tables)."""
    B, n_seg = maps[0].shape[0], np.asarray(lo).shape[1]
    out = np.zeros((B, n_seg, sum(m.shape[1] for m in maps)))
    off = 0
    for l, m in enumerate(maps):
        m = np.asarray(m, dtype=np.float64)
        C, T = m.shape[1], m.shape[3]
        for s in range(n_seg):
            a, b = min(max(int(lo[l][s]), 0), T), min(max(int(hi[l][s]), 0), T)
            if b > a:
                out[:, s, off:off + C] = m[:, :, :, a:b].mean(axis=(2, 3))
        off += C
    return out


def segment_abs_mean_ref(maps, lo, hi):
    """mean |x| over each segment, laid out like `embed_pool_ref`: the scale of the project's per-op bar."""
    return embed_pool_ref([np.abs(np.asarray(m, dtype=np.float64)) for m in maps], lo, hi)


def segment_plan_brute(T_mel, T_l, r_l, frame_ms, hop_ms, width_ms):
    """The definition by enumeration: timestamp k (centre m = k hop_ms / frame_ms mel frames) owns the columns j of a map
    whose centre j r lies in [m - w / 2, m + w / 2); where there is none, the nearest column, ties to the larger j."""
    n = int(math.floor((T_mel - 1) * float(frame_ms) / float(hop_ms))) + 1
    stamps = np.array([k * float(hop_ms) for k in range(n)], dtype=np.float64)
    w = float(width_ms) / float(frame_ms)
    lo = np.zeros((len(T_l), n), dtype=np.int32)
    hi = np.zeros((len(T_l), n), dtype=np.int32)
    for l, (T, r) in enumerate(zip(T_l, r_l)):
        for k in range(n):
            m = stamps[k] / float(frame_ms)
            a, b = m - w / 2, m + w / 2
            inside = [j for j in range(T) if a <= j * r < b]
            if inside:
                assert inside == list(range(inside[0], inside[-1] + 1))
                lo[l, k], hi[l, k] = inside[0], inside[-1] + 1
            else:
                best = min(range(T), key=lambda j: (abs(j * r - m), -j))
                lo[l, k], hi[l, k] = best, best + 1
    return lo, hi, stamps
