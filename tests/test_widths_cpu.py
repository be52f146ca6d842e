"""What each released width IS, as literals: mn01 ... mn40 and dymn04 / dymn10 / dymn20 (the reference's README model table).

Width changes what the launch plans decide, not only tensor sizes: the stem width decides the fused front, a block without
expand conv takes other kernels (and a residual one beyond block 0 the separate depthwise-backward passes of
mn_train._block_fwd), the squeeze widths reach the tile edges of the SE kernels, the DyMN context dimension the K-concat rule.
tests/test_gpu_widths.py rests on the tables below: if `make_divisible` or the block table changes, this file fails first.
CPU only (model construction and state loading need no GPU)."""
import contextlib
import io

import pytest

from oracle import eat_oracle as O
from oracle import synth

# width: (parameters, stem channels, blocks without expand conv, the residual ones of those, SE squeeze widths)
MN = {
    0.1: (123783, 8, [0, 1, 2, 3], [0, 2], {8, 16, 24}),
    0.2: (324695, 8, [0], [0], {8, 24, 32, 48}),
    0.4: (983599, 8, [0], [0], {8, 16, 48, 72, 96}),
    0.5: (1431239, 8, [0], [0], {16, 64, 88, 120}),
    1.0: (4876831, 16, [0], [0], {24, 32, 120, 168, 240}),
    2.0: (17909287, 32, [0], [0], {40, 64, 240, 336, 480}),
    3.0: (39086367, 48, [0], [0], {56, 88, 360, 504, 720}),
    4.0: (68427303, 64, [0], [0], {72, 120, 480, 672, 960}),
}
# (c_in, c_exp, c_out) of the 15 blocks at the two widths whose tables differ in kind from width 1.0
MN_CHANNELS = {
    0.1: [(8, 8, 8), (8, 8, 8), (8, 8, 8), (8, 8, 8), (8, 16, 8), (8, 16, 8), (8, 24, 8), (8, 24, 8), (8, 24, 8), (8, 24, 8),
          (8, 48, 16), (16, 64, 16), (16, 64, 16), (16, 96, 16), (16, 96, 16)],
    0.5: [(8, 8, 8), (8, 32, 16), (16, 40, 16), (16, 40, 24), (24, 64, 24), (24, 64, 24), (24, 120, 40), (40, 104, 40),
          (40, 96, 40), (40, 96, 40), (40, 240, 56), (56, 336, 56), (56, 336, 80), (80, 480, 80), (80, 480, 80)],
}
# width: (parameters, context dimensions of the 15 blocks)
DYMN = {
    0.4: (1961239, [16] * 6 + [24] * 4 + [48] * 5),
    1.0: (10548479, [32] * 6 + [64, 48, 48, 48, 120] + [128] * 4),
    2.0: (39966143, [64] * 6 + [120, 104, 96, 96, 240] + [256] * 4),
}
SE_BLOCKS = [3, 4, 5, 10, 11, 12, 13, 14]


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


@pytest.mark.parametrize("width", list(MN))
def test_mn_width_is_what_the_gpu_cases_assume(width):
    from efficientat_amd.mn import get_model
    n_params, stem, no_expand, no_expand_res, squeeze = MN[width]
    shapes = synth.mn_shapes(width)
    assert synth.n_params(shapes) == n_params
    model = _quiet(get_model, width_mult=width)
    model.load_state_dict(synth.synth_state(shapes, seed=0), strict=True)
    assert sum(p.numel() for p in model.parameters()) == n_params
    blocks = list(model.features[1:-1])
    assert len(blocks) == 15
    assert model.features[0][0].out_channels == stem and shapes["features.0.0.weight"] == (stem, 1, 3, 3)
    assert [i for i, b in enumerate(blocks) if b.i_expand is None] == no_expand
    assert [i for i, b in enumerate(blocks) if b.i_expand is None and b.use_res_connect] == no_expand_res
    assert [i for i, b in enumerate(blocks) if b.i_se is not None] == SE_BLOCKS
    assert {b.block[b.i_se].conc_se_layers[0].fc1.weight.shape[0] for b in blocks if b.i_se is not None} == squeeze
    # the oracle's table (what the fp64 reference of the GPU cases runs) says the same
    table, last = O.block_table(width)
    assert [(b.cnf.input_channels, b.cnf.expanded_channels, b.cnf.out_channels) for b in blocks] == \
        [(c["cin"], c["cexp"], c["cout"]) for c in table]
    assert model.classifier[2].out_features == last
    if width in MN_CHANNELS:
        assert [(c["cin"], c["cexp"], c["cout"]) for c in table] == MN_CHANNELS[width]


@pytest.mark.parametrize("width", list(DYMN))
def test_dymn_width_is_what_the_gpu_cases_assume(width):
    from efficientat_amd.dymn import get_model
    n_params, ctx = DYMN[width]
    shapes = synth.dymn_shapes(width)
    assert synth.n_params(shapes) == n_params and len(shapes) == 578
    model = _quiet(get_model, width_mult=width)
    model.load_state_dict(synth.synth_state(shapes, seed=0), strict=True)
    assert sum(p.numel() for p in model.parameters()) == n_params
    assert [shapes[f"layers.{i}.context_gen.joint_conv.weight"][0] for i in range(15)] == ctx
    assert [model.state_dict()[f"layers.{i}.context_gen.joint_conv.weight"].shape[0] for i in range(15)] == ctx
    table, _ = O.block_table(width)
    assert [O.context_dim(c["cexp"], width) for c in table] == ctx


def test_dymn04_channels_against_the_dynamic_1x1_rules():
    """dymn04's dynamic 1x1 convs against the two channel rules of dymn_train: the K-concat GEMM needs C_in % 32 == 0 (and a
    weight matrix larger than the sample's activations, and an arithmetic other than fp32), the per-sample weight-gradient
    plan C_out >= 64 and C_in >= 64.  (block, conv) lists as literals: test_gpu_widths.py states from them that a 3 s step
    launches no K-concat GEMM."""
    table, _ = O.block_table(0.4)
    assert [(c["cin"], c["cexp"], c["cout"]) for c in table] == [
        (8, 8, 8), (8, 24, 16), (16, 32, 16), (16, 32, 16), (16, 48, 16), (16, 48, 16), (16, 96, 32), (32, 80, 32), (32, 72, 32),
        (32, 72, 32), (32, 192, 48), (48, 272, 48), (48, 272, 64), (64, 384, 64), (64, 384, 64)]
    convs = [(i, n, ci, co) for i, c in enumerate(table)
             for n, ci, co in (("exp", c["cin"], c["cexp"]), ("proj", c["cexp"], c["cout"])) if n == "proj" or c["cexp"] != c["cin"]]
    assert [(i, n) for i, n, ci, co in convs if ci % 32 == 0] == [
        (2, "proj"), (3, "proj"), (6, "proj"), (7, "exp"), (8, "exp"), (9, "exp"), (10, "exp"), (10, "proj"), (13, "exp"),
        (13, "proj"), (14, "exp"), (14, "proj")]
    assert [(i, n) for i, n, ci, co in convs if ci >= 64 and co >= 64] == [
        (12, "proj"), (13, "exp"), (13, "proj"), (14, "exp"), (14, "proj")]


# ---------------------------------------------------------------- the plan literals of tests/widths_case.py against the predicates
def _mn_train_plan(width, geo, store16):
    """The per-block decisions of mn_train._block_fwd / _block_bwd / _expand_bwd / _dw_fwd, restated over the host predicates
    of the library (no kernel runs): the columns of widths_case.PLAN_F32 / PLAN_B16 and the bf16-stored blocks."""
    from efficientat_amd import ops
    from efficientat_amd.mn import get_model
    from tests import widths_case as W
    blocks = list(_quiet(get_model, width_mult=width).features[1:-1])
    f, t = 64, (W.GEOMETRIES[geo] // 320 - 1) // 2 + 1
    stem_fused = blocks[0].i_expand is None
    plan = dict(cat=0, cat16=0, on_load=0, on_load16=0, merged=0, merged16=0, stats16=0, separate=0)
    stored = []
    for bi, blk in enumerate(blocks):
        c = blk.cnf
        ce, k, s = c.expanded_channels, c.kernel, c.stride
        fo, to = ops.conv_out(f, k, s), ops.conv_out(t, k, s)
        merged_res_ok = blk.i_expand is not None or not blk.use_res_connect or (bi == 0 and stem_fused)
        b16 = bool(store16 and ops.b16_block_ok(W.B, ce, f, t, k, s) and merged_res_ok)
        sfx = "16" if b16 else ""
        if b16:
            stored.append(bi)
        if blk.i_expand is not None:
            plan["cat" + sfx] += (ce % 32 == 0) if b16 else (f * t) % 4 == 0
        plan["on_load" + sfx] += ops.pw_tf_eligible(ce, fo * to) and (blk.i_se is None or fo * to >= 2000)
        if merged_res_ok and ops.dw_bwd_merged_ok((W.B, ce, fo, to), (W.B, ce, f, t), k, s):
            plan["merged" + sfx] += 1
        else:
            plan["separate"] += 1
        plan["stats16"] += b16
        f, t = fo, to
    return plan, tuple(stored)


def test_plan_literals_of_the_gpu_cases_are_what_the_predicates_say(monkeypatch):
    from efficientat_amd import mn as mn_mod
    from efficientat_amd import ops
    from efficientat_amd.mn import get_model
    from tests import widths_case as W
    none16 = dict(cat16=0, on_load16=0, merged16=0, stats16=0)
    for width in W.MN_WIDTHS:
        for geo in ("3s", "7s"):
            assert _mn_train_plan(width, geo, False) == (dict(none16, **W.PLAN_F32[width]), ()), (width, geo)
        # the eval plan of mn.run_block at 3 s
        for pw_mode in ("auto", "fp32"):
            monkeypatch.setattr(mn_mod, "_PW_MODE", pw_mode)
            model = _quiet(get_model, width_mult=width)
            assert mn_mod.fold_front(model.features[0], model.features[1]) is None          # no fused front: stem != 16
            f, t, fused, expand_dw = 64, 150, 0, 0
            for blk in model.features[1:-1]:
                c = blk.cnf
                if mn_mod._fusable(blk, True) or mn_mod._fusable(blk, False):
                    fused += 1
                elif (blk.i_expand is not None and mn_mod._pw_mode(c.expanded_channels, c.input_channels) == "bf16x3"
                      and ops.expand_dw_eligible(c.input_channels, f, t, c.kernel, c.stride)):
                    expand_dw += 1
                f, t = ops.conv_out(f, c.kernel, c.stride), ops.conv_out(t, c.kernel, c.stride)
            want = W.EVAL_PLAN[width] if pw_mode == "auto" else dict(fused=0, expand_dw=0)
            assert dict(fused=fused, expand_dw=expand_dw) == want, (width, pw_mode)
    for width in W.MN_B16_WIDTHS:
        assert _mn_train_plan(width, "7s", True) == (W.PLAN_B16[width], W.B16_BLOCKS[width]), width
    assert 2 not in W.B16_BLOCKS[0.1]
