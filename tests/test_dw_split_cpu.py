"""How the depthwise training launchers cut the batch (eat_dw_bwd_split, eat_dw_wgrad_split: the host functions the launchers of
csrc/dw_plane.hip and csrc/dw_grad.hip call for their split) without a GPU: every case of tests/test_gpu_dw_batch_splits.py
takes the branch its table row claims, the splits of the depthwise layers of two training steps against a recorded table, and
the partial slots a launch reports against the bounds the hosts size their buffers with."""
import pytest

from efficientat_amd import _lib, build, ops
from tests import dw_split_cases as K


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.lib()


_ID = dict(ids=lambda r: K.case_id(r[0]))


# ------------------------------------------------------------------ the GPU file's cases take the branches they claim
@pytest.mark.parametrize("row", K.BN_ROWS + K.DYN_ROWS[2:], **_ID)
def test_merged_backward_with_batchnorm_rows(lib, row):
    shape, act, claim = row
    got = K.bwd_split(shape, True)
    assert got == claim
    assert got["G"] > 1 and K.ragged_bwd(shape, got)


@pytest.mark.parametrize("row", K.PLAIN_ROWS, **_ID)
def test_merged_backward_without_batchnorm_rows(lib, row):
    shape, act, claim = row
    got = K.bwd_split(shape, False)
    assert got == claim and shape[3] > 128
    assert got["G"] > 1 and K.ragged_bwd(shape, got)


@pytest.mark.parametrize("row", K.WGRAD_ROWS, **_ID)
def test_weight_gradient_rows(lib, row):
    shape, tf, claim = row
    got = K.wgrad_split(shape)
    assert got == claim
    if shape in K.CONTROLS:
        assert got["parts"] == 1
    else:
        assert got["split"] > 1 and got["parts"] > 1 and K.ragged_wgrad(shape, got)
    if got["kernel"] == "column":                  # no whole-plane instance, T <= 128
        assert shape[3] <= 128


@pytest.mark.parametrize("row", K.STEM_ROWS, ids=lambda r: "x".join(str(v) for v in r[0]))
def test_stem_weight_gradient_rows(lib, row):
    shape, claim = row
    got = K.stem_split(shape)
    assert got == claim
    Fo = K.out(shape[1], 3, 2)
    assert got["split"] > 1 and got["parts"] > 1 and Fo % got["split"] != 0          # the last chunk is short


def test_every_group_count_and_lane_group_mode_has_a_ragged_case(lib):
    """G in {2, 4, 8} and 16-lane, 32-lane, whole-row 64-lane and strip mode each occur (the rows are all ragged: the tests
    above); the whole-plane weight gradient runs each of its five instances, one and two planes per wave, and G = 8."""
    rows = [(s, K.bwd_split(s, True)) for s, _, _ in K.BN_ROWS]
    assert {g["G"] for _, g in rows} == {2, 4, 8}
    assert {(g["lane_group"], g["whole_rows"]) for _, g in rows} == {(16, True), (32, True), (64, True), (64, False)}
    assert {g["tile_rows"] for _, g in rows} == {4, 8}
    assert {K.bwd_split(s, False)["G"] for s, _, _ in K.PLAIN_ROWS} == {2, 4, 8}
    planes = [(s, c) for s, _, c in K.WGRAD_ROWS if c["kernel"] == "plane"]
    assert {(s[2], s[4], s[5]) for s, _ in planes} == {(8, 3, 1), (16, 5, 1), (8, 5, 2), (16, 3, 2), (4, 5, 1)}
    assert {c["lane_samples"] for _, c in planes} == {1, 2} and 8 in {c["split"] for _, c in planes}
    assert {c["split"] for s, _, c in K.WGRAD_ROWS if c["kernel"] == "tile"} == {2, 4, 8}


# ------------------------------------------------------------------ one training step's depthwise layers
# The split of every depthwise layer of an mn10 step at 256 clips and an mn40 step at 128 clips (128 mels x 1000 frames: the
# stem leaves 64 x 500 planes), recorded from the library at the commit that added the helpers; a changed row is a changed
# launch plan, to be measured like one.
#   merged backward with BatchNorm on load: lane group, whole rows, rows per tile, G, tiles per plane
#   stand-alone weight gradient of the same layer: kernel, G, waves per channel (and tile)
# (model, B, C, F, T, k, stride) -> (lane_group, whole_rows, tile_rows, G, inner), (kernel, split, parts)
STEP_LAYERS = [
    ('mn10', 256,   16, 64, 500, 3, 1, 64, 0, 8, 8, 32, 'tile', 8, 32),
    ('mn10', 256,   64, 64, 500, 3, 2, 64, 0, 8, 8, 20, 'tile', 8, 32),
    ('mn10', 256,   72, 32, 250, 3, 1, 64, 0, 8, 8,  8, 'tile', 8, 32),
    ('mn10', 256,   72, 32, 250, 5, 2, 64, 0, 8, 8,  6, 'tile', 8, 32),
    ('mn10', 256,  120, 16, 125, 5, 1, 64, 1, 8, 4,  2, 'plane', 2, 128),
    ('mn10', 256,  240, 16, 125, 3, 2, 64, 1, 8, 4,  1, 'plane', 4, 64),
    ('mn10', 256,  200,  8,  63, 3, 1, 32, 1, 8, 2,  1, 'plane', 4, 64),
    ('mn10', 256,  184,  8,  63, 3, 1, 32, 1, 8, 2,  1, 'plane', 4, 64),
    ('mn10', 256,  480,  8,  63, 3, 1, 32, 1, 8, 4,  1, 'plane', 8, 32),
    ('mn10', 256,  672,  8,  63, 3, 1, 32, 1, 8, 8,  1, 'plane', 8, 32),
    ('mn10', 256,  672,  8,  63, 5, 2, 32, 1, 4, 8,  1, 'plane', 8, 16),
    ('mn10', 256,  960,  4,  32, 5, 1, 16, 1, 4, 4,  1, 'plane', 8, 16),
    ('mn40', 128,   64, 64, 500, 3, 1, 64, 0, 8, 8, 32, 'tile', 8, 16),
    ('mn40', 128,  256, 64, 500, 3, 2, 64, 0, 8, 8, 20, 'tile', 8, 16),
    ('mn40', 128,  288, 32, 250, 3, 1, 64, 0, 8, 8,  8, 'tile', 8, 16),
    ('mn40', 128,  288, 32, 250, 5, 2, 64, 0, 8, 8,  6, 'tile', 8, 16),
    ('mn40', 128,  480, 16, 125, 5, 1, 64, 1, 8, 8,  2, 'plane', 4, 32),
    ('mn40', 128,  960, 16, 125, 3, 2, 64, 1, 8, 8,  1, 'plane', 8, 16),
    ('mn40', 128,  800,  8,  63, 3, 1, 32, 1, 8, 4,  1, 'plane', 8, 16),
    ('mn40', 128,  736,  8,  63, 3, 1, 32, 1, 8, 4,  1, 'plane', 8, 16),
    ('mn40', 128, 1920,  8,  63, 3, 1, 32, 1, 8, 8,  1, 'plane', 8, 16),
    ('mn40', 128, 2688,  8,  63, 3, 1, 32, 1, 8, 8,  1, 'plane', 8, 16),
    ('mn40', 128, 2688,  8,  63, 5, 2, 32, 1, 4, 8,  1, 'plane', 8,  8),
    ('mn40', 128, 3840,  4,  32, 5, 1, 16, 1, 4, 8,  1, 'plane', 8,  8),
]
# the stem's weight gradient (x (B, 1, 128, 1000)): (model, B, C) -> (rows per block, row chunks)
STEP_STEMS = [('mn10', 256, 16, 8, 8), ('mn40', 128, 64, 4, 16)]


@pytest.mark.parametrize("row", STEP_LAYERS, ids=lambda r: f"{r[0]}-{r[2]}x{r[3]}x{r[4]}-k{r[5]}s{r[6]}")
def test_split_of_the_training_steps_depthwise_layers(lib, row):
    model, B, C, F, T, k, s, lane_group, whole_rows, tile_rows, G, inner, kernel, split, parts = row
    Fo, To = K.out(F, k, s), K.out(T, k, s)
    assert ops.dw_bwd_split(B, C, F, T, Fo, To, k, s, True) == dict(lane_group=lane_group, whole_rows=bool(whole_rows),
                                                                     tile_rows=tile_rows, G=G, inner=inner)
    lane_samples = 2 if kernel == "plane" and (F, k) in ((8, 5), (4, 5)) else 1
    assert ops.dw_wgrad_split(B, C, C, F, T, Fo, To, k, s) == dict(kernel=kernel, split=split, parts=parts, lane_samples=lane_samples)


@pytest.mark.parametrize("row", STEP_STEMS, ids=lambda r: r[0])
def test_split_of_the_training_steps_stem(lib, row):
    model, B, C, rpb, chunks = row
    assert ops.dw_wgrad_split(B, C, 1, 128, 1000, 64, 500, 3, 2) == dict(kernel="stem", split=rpb, parts=chunks, lane_samples=1)


# ------------------------------------------------------------------ what a launch reports fits what the hosts allocate
def test_reported_partials_fit_the_hosts_buffers(lib):
    """*h_inner of a merged-backward launch (`inner` of the query: tiles per plane) never exceeds eat_dw_bwd_partials_inner,
    with which ops.dw_conv_bwd_bn_g / dw_conv_dyn_bwd_bn_g size gpart and gzpart; ops.dw_conv_bwd_g takes the larger of that
    and eat_dw_partials_inner(..., dgrad) (its two-kernel fallback writes that layout)."""
    shapes = [(s, True) for s, _, _ in K.BN_ROWS + K.DYN_ROWS] + [(s, False) for s, _, _ in K.PLAIN_ROWS]
    shapes += [((r[1], r[2], r[3], r[4], r[5], r[6]), True) for r in STEP_LAYERS]
    shapes += [((r[1], r[2], r[3], r[4], r[5], r[6]), False) for r in STEP_LAYERS if r[4] > 128]
    for shape, bn in shapes:
        B, C, F, T, Fo, To, k, s = K.geom(shape)
        got = ops.dw_bwd_split(B, C, F, T, Fo, To, k, s, bn)
        cap = lib.eat_dw_bwd_partials_inner(F, T, Fo, To, k, s)
        assert 1 <= got["inner"] <= cap, (shape, bn, got, cap)
        if not bn:
            assert got["inner"] <= max(cap, lib.eat_dw_partials_inner(F, T, Fo, To, k, s, 1))


def test_geometries_outside_the_merged_kernel_and_refused_weight_gradients(lib):
    """"Not on this kernel" where dw_bwd_try answers 1: without BatchNorm the planes of up to 128 columns, a stride-1 output
    of another size, taps other than 3x3 / 5x5; the weight-gradient helper answers -1 where the entry point fails."""
    assert ops.dw_bwd_split(4, 16, 8, 128, 8, 128, 3, 1, False) is None
    assert ops.dw_bwd_split(4, 16, 8, 129, 8, 129, 3, 1, False) is not None
    assert ops.dw_bwd_split(4, 16, 8, 128, 8, 128, 3, 1, True) is not None
    assert ops.dw_bwd_split(4, 16, 8, 130, 8, 128, 3, 1, True) is None
    assert ops.dw_bwd_split(4, 16, 8, 130, 8, 130, 7, 1, True) is None
    assert ops.dw_bwd_split(4, 16, 8, 130, 4, 65, 3, 3, True) is None
    with pytest.raises(_lib.EatHipError):
        ops.dw_wgrad_split(4, 16, 8, 8, 130, 8, 130, 3, 1)                     # x with neither C nor 1 channels
    with pytest.raises(_lib.EatHipError):
        ops.dw_wgrad_split(4, 16, 16, 8, 130, 8, 130, 7, 1)
    # per-sample gradients (eat_dw_conv_dyn_wgrad): one sample per wave on the register-resident kernels, else per channel
    assert ops.dw_wgrad_split(59, 560, 560, 2, 130, 1, 65, 5, 2, per_sample=True) == dict(kernel="tile", split=1, parts=59, lane_samples=1)
    assert ops.dw_wgrad_split(37, 9, 9, 5, 20, 5, 20, 3, 1, per_sample=True) == dict(kernel="channel", split=1, parts=37, lane_samples=1)
    # one input channel with taps other than the stem's: the per-channel kernel
    assert ops.dw_wgrad_split(3, 16, 1, 16, 20, 16, 20, 3, 1)["kernel"] == "channel"
