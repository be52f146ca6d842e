"""Cases of tests/test_gpu_dw_batch_splits.py: the shapes at which the BATCH picks the work decomposition of the depthwise
training launchers (csrc/dw_plane.hip: launch_dw_bwd, launch_tile_wgrad, launch_plane_wgrad; csrc/dw_grad.hip:
dw_wgrad_impl), each with the branch it claims.  tests/test_dw_split_cpu.py asks the library for every claim without a GPU,
the GPU file asserts it again before it runs the case.  Importable without a GPU.

Planes are tiny and channels many: the launchers keep G = 8 sample groups per wave only while the launch still has 8192
waves, so a case reaches G > 1 with a few million elements.  Every row is ragged: its batch is no multiple of the samples a
wave walks, so the last wave of a channel runs out of samples inside its loop (and, where 2 or 4 samples sit side by side
in a wave, its last lane groups have none)."""
from efficientat_amd import ops


def out(n, k, s):
    return (n + 2 * ((k - 1) // 2) - k) // s + 1


def geom(row):
    """(B, C, F, T, k, stride) -> (B, C, F, T, Fo, To, k, stride), the argument order of the library's helpers."""
    B, C, F, T, k, s = row
    return B, C, F, T, out(F, k, s), out(T, k, s), k, s


def case_id(row):
    return "x".join(str(v) for v in row[:4]) + f"-k{row[4]}s{row[5]}"


# ---- merged backward with BatchNorm on load (eat_dw_conv_bwd_bn_g and its _dyn / _b16 forms)
# (B, C, F, T, k, stride), act, {lane_group, whole_rows, tile_rows, G, inner}
# nb = ceil(B / (64 / lane_group)) sample groups, of which a wave walks G
BN_ROWS = [
    ((49, 1368, 4, 8, 3, 1), 1, dict(lane_group=16, whole_rows=True, tile_rows=8, G=2, inner=1)),      # nb = 13, last quad: 1 sample
    ((277, 960, 4, 8, 5, 1), 2, dict(lane_group=16, whole_rows=True, tile_rows=4, G=8, inner=1)),      # nb = 70, last wave 6 of 8
    ((139, 960, 8, 16, 5, 2), 2, dict(lane_group=16, whole_rows=True, tile_rows=4, G=4, inner=1)),     # nb = 35, last wave 3 of 4
    ((75, 1024, 2, 40, 3, 1), 1, dict(lane_group=32, whole_rows=True, tile_rows=8, G=4, inner=1)),     # nb = 38, last pair: 1 sample
    ((21, 1640, 4, 63, 5, 2), 2, dict(lane_group=32, whole_rows=True, tile_rows=4, G=2, inner=1)),     # nb = 11
    ((133, 1000, 2, 34, 3, 2), 1, dict(lane_group=32, whole_rows=True, tile_rows=8, G=8, inner=1)),    # nb = 67, last wave 3 of 8
    ((5, 2740, 2, 66, 5, 1), 2, dict(lane_group=64, whole_rows=True, tile_rows=8, G=2, inner=1)),      # one plane per wave
    ((13, 2731, 2, 128, 3, 2), 1, dict(lane_group=64, whole_rows=True, tile_rows=8, G=4, inner=1)),
    ((5, 1366, 2, 130, 3, 1), 1, dict(lane_group=64, whole_rows=False, tile_rows=8, G=2, inner=2)),    # two strips
    ((9, 1366, 4, 129, 5, 1), 2, dict(lane_group=64, whole_rows=False, tile_rows=8, G=4, inner=2)),
    ((13, 1366, 2, 250, 5, 2), 2, dict(lane_group=64, whole_rows=False, tile_rows=8, G=8, inner=3)),   # three strips
]
# `frozen` and `no_expand`: one row of each lane-group width, and one in strip mode
BN_ROWS_ALL_VARIANTS = [BN_ROWS[0], BN_ROWS[3], BN_ROWS[6], BN_ROWS[8]]
# per-sample taps (eat_dw_conv_dyn_bwd_bn_g[_b16]): 16-lane groups and strips.  The third row is the 16-lane geometry the bf16
# entry points cover (eat_dw_conv_b16_ok: 5x5 / stride 1 on 4-row planes; 3x3 on a 4 x 8 plane is refused): nb = 5, last quad
# 1 sample, last wave 1 of 2
DYN_ROWS = [
    BN_ROWS[0],
    BN_ROWS[8],
    ((17, 2731, 4, 8, 5, 1), 2, dict(lane_group=16, whole_rows=True, tile_rows=4, G=2, inner=1)),
]

# ---- merged backward without BatchNorm (eat_dw_conv_bwd_g; T > 128 only: strips)
PLAIN_ROWS = [
    ((5, 1366, 2, 130, 3, 1), 1, dict(lane_group=64, whole_rows=False, tile_rows=8, G=2, inner=2)),
    ((59, 280, 2, 130, 5, 1), 2, dict(lane_group=64, whole_rows=False, tile_rows=8, G=4, inner=2)),
    ((29, 280, 2, 260, 3, 2), 1, dict(lane_group=64, whole_rows=False, tile_rows=8, G=2, inner=3)),
    ((27, 1366, 2, 130, 5, 2), 2, dict(lane_group=64, whole_rows=False, tile_rows=8, G=8, inner=2)),
]

# ---- stand-alone weight gradients (eat_dw_conv_wgrad, eat_dw_conv_wgrad_tf)
# (B, C, F, T, k, stride), on-load transform, {kernel, split, parts, lane_samples}
#   plane / tile: split = G, parts = waves per channel and tile; column: split = samples per block, parts = batch slices
WGRAD_ROWS = [
    # tile kernel (T > 128)
    ((5, 1366, 2, 130, 3, 1), False, dict(kernel="tile", split=2, parts=3, lane_samples=1)),
    ((29, 560, 2, 130, 3, 2), True, dict(kernel="tile", split=4, parts=8, lane_samples=1)),
    ((59, 560, 2, 130, 5, 2), False, dict(kernel="tile", split=8, parts=8, lane_samples=1)),           # last wave 3 of 8
    # whole-plane kernel: its five instances, then G = 8 (two planes per wave: 117 = 7 x 16 + 5)
    ((5, 2740, 8, 37, 3, 1), False, dict(kernel="plane", split=2, parts=3, lane_samples=1)),
    ((5, 2740, 16, 65, 5, 1), False, dict(kernel="plane", split=2, parts=3, lane_samples=1)),
    ((11, 2740, 8, 33, 5, 2), False, dict(kernel="plane", split=2, parts=3, lane_samples=2)),
    ((5, 2740, 16, 65, 3, 2), True, dict(kernel="plane", split=2, parts=3, lane_samples=1)),
    ((11, 2740, 4, 32, 5, 1), False, dict(kernel="plane", split=2, parts=3, lane_samples=2)),
    ((117, 1100, 4, 9, 5, 1), False, dict(kernel="plane", split=8, parts=8, lane_samples=2)),
    # column-walking kernel (no whole-plane instance, T <= 128): slices of 32 + 5, of 32 + 32 + 6, of 16 + 16 + 13 (64 columns
    # per block), and the control - C * column tiles >= 2048: one slice
    ((37, 9, 5, 20, 3, 1), False, dict(kernel="column", split=32, parts=2, lane_samples=1)),
    ((70, 7, 9, 40, 5, 2), False, dict(kernel="column", split=32, parts=3, lane_samples=1)),
    ((45, 6, 7, 70, 5, 1), True, dict(kernel="column", split=16, parts=3, lane_samples=1)),
    ((5, 2048, 3, 9, 3, 1), False, dict(kernel="column", split=5, parts=1, lane_samples=1)),
]
CONTROLS = {(5, 2048, 3, 9, 3, 1)}                # the rows that claim ONE part

# ---- stem weight gradient (XC = 1, 3x3 / stride 2): x (B, 1, F, T), 16 output channels
# (B, F, T), {split = output rows per block, parts = row chunks}: 64 rows in 22 chunks of 3 (the last holds one row), 63 rows in
# 32 chunks of 2 (the last holds one row)
STEM_C = 16
STEM_ROWS = [
    ((70, 128, 20), dict(kernel="stem", split=3, parts=22, lane_samples=1)),
    ((37, 126, 20), dict(kernel="stem", split=2, parts=32, lane_samples=1)),
]


def bwd_split(row, bn):
    return ops.dw_bwd_split(*geom(row), bn)


def wgrad_split(row):
    B, C = row[0], row[1]
    return ops.dw_wgrad_split(B, C, C, *geom(row)[2:])


def stem_split(row):
    B, F, T = row
    return ops.dw_wgrad_split(B, STEM_C, 1, F, T, out(F, 3, 2), out(T, 3, 2), 3, 2)


def ragged_bwd(row, split):
    """The batch is no multiple of the samples a wave of the merged backward walks."""
    return row[0] % ((64 // split["lane_group"]) * split["G"]) != 0


def ragged_wgrad(row, split):
    return row[0] % (split["lane_samples"] * split["split"]) != 0
