"""GPU tests of the LDS-free streaming 1x1 weight-gradient kernel (csrc/train.hip: pw_wgrad_x3_narrow_kernel) on every
path of its load ring: planes that end inside a unit, row counts that are no multiple of 16, k ranges shorter than the
ring and one off a multiple of it, the Gram form with centring, the SE scale and the on-load transform, the per-sample
form, and the grouped / 5 x 2 / 2 x 5 tile shapes that only the long-k rule (>= 512 k positions per block) selects.
Every case first asserts its route through eat_pw_wgrad_kernel_kind and compares against an fp64 einsum of the same
operands with the bars of tests/test_gpu_train.py (relative L2 2e-5 for 'auto', 3e-5 for 'bf16' with a transform; the
streaming kernel multiplies split bf16 operands in every mode, so its 'bf16' result is held against the unrounded fp64)."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, ops  # noqa: E402

DEV = torch.device("cuda:0")


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _rel(got, ref):
    got = got.detach().cpu().double().reshape(-1)
    ref = ref.detach().cpu().double().reshape(-1)
    return float((got - ref).norm() / max(1e-30, float(ref.norm())))


def _streaming(m, n, gram=0):
    """eat_pw_wgrad_kernel_kind of pw_wgrad_x3_narrow_kernel<m, n> (kind 0, detail 1000 m + 10 n + gram)."""
    return 10 * (1000 * m + 10 * n + gram)


def _case(B, Co, Ci, S, opt):
    """Operands, the library-side options and the fp64 reference of one weight gradient."""
    dz, x = _rand(B, Co, S, 1, seed=1), _rand(B, Ci, S, 1, seed=2)
    sc = torch.rand(B, Ci, generator=torch.Generator().manual_seed(5)) + 0.25 if "scale" in opt else None
    a = torch.rand(Ci, generator=torch.Generator().manual_seed(6)) + 0.5
    b = 0.3 * torch.randn(Ci, generator=torch.Generator().manual_seed(7))
    xe, tf = x[..., 0].double(), None
    if "tf" in opt:
        act = ops.ACT_RELU if "relu" in opt else ops.ACT_HSWISH
        u = a.double()[None, :, None] * xe + b.double()[None, :, None]
        xe = torch.relu(u) if act == ops.ACT_RELU else F.hardswish(u)
        tf = (a.to(DEV), b.to(DEV), act)
    if sc is not None:
        xe = xe * sc.double()[:, :, None]
    ref = torch.einsum("bos,bis->oi", dz[..., 0].double(), xe)
    # (what a single-bf16-product kernel is held against, as tests/test_gpu_train.py does: the rounded operands in fp64)
    refb = (lambda: torch.einsum("bos,bis->oi", dz[..., 0].bfloat16().double(), xe.float().bfloat16().double()))
    return dz.to(DEV), x.to(DEV), None if sc is None else sc.to(DEV), tf, ref, refb


def _check(B, Co, Ci, S, opt, kind):
    got_kind = _lib.lib().eat_pw_wgrad_kernel_kind(B, Co, Ci, S, 0, 0, 1 if "scale" in opt else 0, 1 if "tf" in opt else 0)
    assert got_kind == kind, (got_kind, kind)
    dz, x, sc, tf, ref, refb = _case(B, Co, Ci, S, opt)
    for mode in (("auto", "bf16") if tf is not None else ("auto",)):
        with ops.precision(mode):
            got = ops.pw_conv_wgrad(dz, x, x_scale=sc, exact=None, tf=tf)
        err = _rel(got, refb() if (mode == "bf16" and kind % 10 != 0) else ref)
        print(f"{B} x {Co} x {Ci} @ {S} {opt} {mode}: rel L2 {err:.3e}")
        assert err < (3e-5 if mode == "bf16" else 2e-5), (mode, err)


# Always thin (Co, Ci <= 64, one side <= 16): a few clips, tiny planes.  S = 36 / 100 / 8004: a multiple of 4, not of 32
# (the last unit of a plane is 4 / 4 / 4 positions; lanes of k groups 1..3 load from clamped positions).  Rows 24 / 40 /
# 56 against 8 / 12 / 16: the last row tile is half empty, the narrow side has 8 / 12 rows of one tile.  Both operand
# orders, every option (the x side carries scale and transform).
@pytest.mark.parametrize("B,Co,Ci,S,opt,tile", [
    (2, 16, 16, 100, "plain", (1, 1)), (3, 24, 8, 36, "plain", (2, 1)), (2, 40, 12, 100, "scale", (3, 1)),
    (2, 56, 16, 8004, "tf_relu", (4, 1)), (2, 8, 24, 100, "tf_hswish", (1, 2)), (3, 12, 40, 36, "tf_hswish+scale", (1, 3)),
    (2, 16, 56, 8004, "tf_relu+scale", (1, 4)), (2, 64, 16, 8004, "plain", (4, 1)), (2, 16, 40, 100, "scale", (1, 3))])
def test_thin_shapes_ragged_planes_and_rows(B, Co, Ci, S, opt, tile):
    _check(B, Co, Ci, S, opt, _streaming(*tile))


# k ranges against the ring (a block's four waves take units u0 + w, + 4, ...; a wave holds RING units, RING - 1 of them
# requested ahead).  Fewer than 4 units in all: some waves have none and every prefetch runs past the range from the
# first step (S = 4: the whole plane is half of one lane group's 32 bytes).  One below / one above RING x 4 units per
# block (1024 blocks: total = 1024 x units): <1, 1> RING 6 -> 23 / 25 units, <4, 1> RING 3 -> 11 / 13 units.
@pytest.mark.parametrize("B,Co,Ci,S,opt,tile", [
    (1, 16, 16, 36, "tf_hswish+scale", (1, 1)), (3, 64, 16, 4, "plain", (4, 1)), (1, 8, 56, 68, "scale", (1, 4)),
    (1, 16, 16, 4, "tf_relu", (1, 1)),
    (64, 16, 16, 11776, "tf_hswish+scale", (1, 1)), (64, 16, 16, 12800, "plain", (1, 1)),
    (32, 64, 16, 11264, "plain", (4, 1)), (32, 64, 16, 13312, "plain", (4, 1))])
def test_k_ranges_shorter_than_and_one_off_the_ring(B, Co, Ci, S, opt, tile):
    _check(B, Co, Ci, S, opt, _streaming(*tile))


# Gram form with centring (dz == x, additive row constant -mean; one slot per block and a fixed wave order: two runs are
# bit-identical).  C = 16 / 24 / 40 / 56: one to four row tiles, the last one ragged; S as above; one unit in all; RING 8
# of <1, 1, gram>: 31 / 33 units per block.
@pytest.mark.parametrize("B,C,S", [(3, 16, 36), (2, 24, 100), (2, 40, 8004), (2, 56, 100), (1, 16, 4), (1, 24, 36),
                                   (64, 16, 15872), (64, 16, 16896)])
def test_gram_centred_against_fp64_and_bit_reproducible(B, C, S):
    t = (C + 15) // 16
    assert _lib.lib().eat_pw_wgrad_kernel_kind(B, C, C, S, 0, 1, 0, 0) == _streaming(t, t, 1)
    x = _rand(B, C, S, 1, seed=3) + _rand(1, C, 1, 1, seed=4) + 1.0
    xd = x.to(DEV)
    n = B * S
    sx = x.double().sum((0, 2, 3)).float().contiguous().to(DEV)
    G = ops.gram(xd, sx=sx)
    assert torch.equal(G, ops.gram(xd, sx=sx))
    xc = x[..., 0].double() - (sx.cpu().double() / n).view(1, C, 1)
    err = _rel(G, torch.einsum("bis,bjs->ij", xc, xc))
    print(f"gram {B} x {C} @ {S}: rel L2 {err:.3e}")
    assert err < 2e-5


# Per-sample form (DyMN: one Co x Ci matrix per clip, a few blocks per sample sharing its k range): thin shapes with planes
# of >= 1024 positions; the output is poisoned where the library stores and zeroed where it says it accumulates.
@pytest.mark.parametrize("B,Co,Ci,S", [(3, 16, 64, 1028), (3, 64, 16, 1028), (2, 24, 40, 2052)])
def test_per_sample_gradients_on_the_streaming_kernel(B, Co, Ci, S):
    assert ops.dyn_wgrad_needs_zero(Co, Ci, S)                         # not the 128 x 128-tile kernel, which stores
    dz, x = _rand(B, Co, S, 1, seed=1), _rand(B, Ci, S, 1, seed=2)
    G = torch.full((B, Co * Ci), float("nan"), device=DEV)             # poison wherever the library stores
    if ops.dyn_wgrad_needs_zero(Co, Ci, S):
        G.zero_()
    dzd, xd = dz.to(DEV), x.to(DEV)
    _lib.call("eat_pw_conv_dyn_wgrad", dzd.data_ptr(), xd.data_ptr(), G.data_ptr(), B, Co, Ci, S,
              torch.cuda.current_stream().cuda_stream)
    ref = torch.einsum("bos,bis->boi", dz[..., 0].double(), x[..., 0].double()).reshape(B, -1)
    err = _rel(G, ref)
    print(f"per-sample {B} x {Co} x {Ci} @ {S}: rel L2 {err:.3e}")
    assert err < 2e-5


# Grouped and 5 x 2 / 2 x 5 tiles: only the long-k rule selects them (>= 512 k positions for each of a row group's
# 1024 / groups blocks), so every case has >= 2^19 / groups positions.  72 x 24 and 24 x 72 run as ONE row group; 24 x 64
# as two groups of <2, 2>; 40 x 72 / 40 x 120 at S = 2000 as two / three groups of <3, 3>.  The last two sit just above
# and just below the rule for two groups (2 x 32 x 63 x B >= 2^19 from B = 131 on): B = 130 runs the 128 x 128-tile kernel.
@pytest.mark.parametrize("B,Co,Ci,S,opt,kind", [
    (66, 72, 24, 8000, "plain", _streaming(5, 2)), (66, 24, 72, 8000, "plain", _streaming(2, 5)),
    (66, 24, 72, 8000, "tf_relu+scale", _streaming(2, 5)), (66, 24, 64, 8000, "tf_relu+scale", _streaming(2, 2)),
    (263, 40, 72, 2000, "tf_relu+scale", _streaming(3, 3)), (263, 40, 120, 2000, "tf_hswish+scale", _streaming(3, 3)),
    (131, 40, 72, 2000, "tf_hswish+scale", _streaming(3, 3)), (130, 40, 72, 2000, "tf_hswish+scale", 1)])
def test_grouped_and_new_tile_shapes_under_the_long_k_rule(B, Co, Ci, S, opt, kind):
    _check(B, Co, Ci, S, opt, kind)
