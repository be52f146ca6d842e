"""tests/dyn_weights_ref.py (the fp64 oracle, pack decoders and bounds of DyMN's per-sample weight kernels) on the CPU: the
decoders against the encoders, the bounds against an fp32 emulation of the kernels' arithmetic - and against emulated packs
that are wrong in the ways a pack kernel can be wrong, so that the GPU tests built on these bounds are known to be able to
fail.  The samples-per-block query of the bf16 packs is a host function and is pinned here too."""
import numpy as np
import pytest
import torch

from tests import dyn_weights_ref as R

# ragged m-tile (200 = 12 * 16 + 8, 72 = 4 * 16 + 8, 7 < 16), ragged 32-column chunk (36, 260, 4), more than one sample
SHAPES = [(3, 200, 36), (2, 72, 260), (3, 7, 4), (2, 16, 256)]


def _matrix(B, Co, Ci, seed=0):
    return torch.randn(B, Co, Ci, generator=torch.Generator().manual_seed(seed + 31 * Co + Ci))


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


@pytest.mark.parametrize("B,Co,Ci", SHAPES)
def test_decoders_invert_the_encoders_bit_for_bit_and_padding_is_zero(B, Co, Ci):
    W = _matrix(B, Co, Ci)
    MT, KK = (Co + 15) // 16, (Ci + 31) // 32
    # fp32
    wp = R.encode_fp32(W)
    assert wp.shape == (B, R.fp32_pack_len(Co, Ci))
    D = R.decode_fp32(wp, Co, Ci)
    assert D.shape == (B, MT * 16, Ci) and torch.equal(_bits(D[:, :Co]), _bits(W))
    assert R.is_plus_zero(D)[:, R.padding_mask(Co, Ci, MT * 16, Ci)].all()
    # plain bf16
    wp = R.encode_b16(W)
    assert wp.shape == (B, R.bf16_pack_len(Co, Ci, 1))
    D = R.decode_b16(wp, Co, Ci)
    assert D.shape == (B, MT * 16, KK * 32) and torch.equal(_bits(D[:, :Co, :Ci]), _bits(W.to(torch.bfloat16)))
    pad = R.padding_mask(Co, Ci, MT * 16, KK * 32)
    assert R.is_plus_zero(D)[:, pad].all()
    # hi / lo
    wp = R.encode_bf16_hilo(W)
    assert wp.shape == (B, R.bf16_pack_len(Co, Ci, 2))
    hi, lo = R.decode_bf16_hilo(wp, Co, Ci)
    h_ref, l_ref = R.split_bf16(W)
    assert torch.equal(_bits(hi[:, :Co, :Ci]), _bits(h_ref)) and torch.equal(_bits(lo[:, :Co, :Ci]), _bits(l_ref))
    assert R.is_plus_zero(hi)[:, pad].all() and R.is_plus_zero(lo)[:, pad].all()
    assert float((hi.double() + lo.double())[:, :Co, :Ci].sub(W.double()).abs().max()) <= 2.0 ** -16 * float(W.abs().max())


@pytest.mark.parametrize("Co,Ci", [(200, 36), (72, 260), (7, 4)])
def test_every_pack_position_is_decoded_exactly_once(Co, Ci):
    """The index maps are bijections onto a sample's pack: no element of a kernel's output escapes the decoded matrix."""
    for idx, n in ((R._fp32_index(Co, Ci), R.fp32_pack_len(Co, Ci)), (R._bf16_index(Co, Ci, 1, 0), R.bf16_pack_len(Co, Ci, 1)),
                   (np.stack([R._bf16_index(Co, Ci, 2, 0), R._bf16_index(Co, Ci, 2, 1)]), R.bf16_pack_len(Co, Ci, 2))):
        assert np.array_equal(np.sort(idx.reshape(-1)), np.arange(n))


def test_layout_literals_written_from_the_documented_formulas():
    """A few positions worked out by hand from `wp[(ks*MT + mt)*64 + lane]` and `wp[((kk*MT + mt)*NP2 + h)*512 + lane*8 + i]`."""
    Co, Ci = 40, 72                                                  # MT = 3, KK = 3
    W = torch.arange(Co * Ci, dtype=torch.float32).reshape(1, Co, Ci)
    f = R.encode_fp32(W)[0]
    # W[17][9]: mt = 1, m = 1, ks = 2, kq = 1 -> lane 17 -> (2 * 3 + 1) * 64 + 17
    assert float(f[(2 * 3 + 1) * 64 + 17]) == 17 * Ci + 9
    assert float(f[(0 * 3 + 2) * 64 + 8]) == 0.0                     # row 2 * 16 + 8 = 40 = Co: padding
    W = (torch.arange(Co * Ci, dtype=torch.float32) % 251).reshape(1, Co, Ci)      # integers < 256: exact in bf16
    p = R.encode_b16(W)[0]
    # W[35][70]: mt = 2, m = 3, kk = 2, kq = (70 - 64) // 8 = 0, i = 6 -> lane 3 -> ((2 * 3 + 2) * 1 + 0) * 512 + 3 * 8 + 6
    assert float(p[(2 * 3 + 2) * 512 + 3 * 8 + 6]) == float((35 * Ci + 70) % 251)
    assert float(p[(2 * 3 + 0) * 512 + (16 * 1 + 0) * 8 + 0]) == 0.0               # column 64 + 8 = 72 = Ci: padding
    q = R.encode_bf16_hilo(W)[0]
    assert float(q[((2 * 3 + 2) * 2 + 0) * 512 + 3 * 8 + 6]) == float((35 * Ci + 70) % 251)
    assert float(q[((2 * 3 + 2) * 2 + 1) * 512 + 3 * 8 + 6]) == 0.0                # lo of an exactly representable value


def _emulated(B, K, Co, Ci):
    bank, att = R.pack_operands(B, K, Co, Ci)
    v = torch.from_numpy(R.emulate_aggregate_fp32(bank.numpy(), att.numpy())).reshape(B, Co, Ci)
    W, A = R.aggregate(bank, att)
    return v, W.reshape(B, Co, Ci), A.reshape(B, Co, Ci)


@pytest.mark.parametrize("B,K,Co,Ci", [(5, 4, 200, 36), (3, 4, 72, 260), (4, 3, 200, 36), (4, 8, 7, 4), (6, 1, 16, 256)])
def test_bounds_hold_for_the_fp32_emulation_of_the_kernels(B, K, Co, Ci):
    v, W, A = _emulated(B, K, Co, Ci)
    vd = v.double().numpy()
    assert (np.abs(vd - W) <= R.aggregate_bound(A, K)).all()
    rs = torch.rand(Co, generator=torch.Generator().manual_seed(3)) + 0.5
    scaled = (v * rs[None, :, None]).double().numpy()                # one more fp32 rounding, as the kernel's `* rs`
    rs64 = rs.double().numpy()[None, :, None]
    assert (np.abs(scaled - W * rs64) <= R.aggregate_bound(A, K, W * rs64, rs64)).all()
    hi, lo = R.split_bf16(v)
    assert (np.abs(hi.double().numpy() - W) <= R.b16_pack_bound(W, A, K)).all()
    assert (np.abs(hi.double().numpy() + lo.double().numpy() - W) <= R.hilo_pack_bound(W, A, K)).all()
    # the rounding terms WITHOUT the slack factor hold for the emulation (it forms true fmas): the factor is not a fit
    assert (np.abs(hi.double().numpy() - W) <= R.b16_pack_bound(W, A, K) / R.SLACK).all()
    assert (np.abs(hi.double().numpy() + lo.double().numpy() - W) <= R.hilo_pack_bound(W, A, K) / R.SLACK).all()


def _violations(got, W, bound):
    return int((np.abs(got - W) > bound).sum())


def test_bounds_fail_for_packs_that_are_wrong():
    """What the GPU tests must be able to see: an element in a neighbouring slot, a dropped lo part, two samples swapped (the
    output offset of a multi-sample block), the previous sample's values (a missing barrier), a skipped ragged chunk."""
    B, K, Co, Ci = 5, 4, 200, 36
    v, W, A = _emulated(B, K, Co, Ci)
    hb, b1 = R.hilo_pack_bound(W, A, K), R.b16_pack_bound(W, A, K)

    def hilo_of(wp):
        hi, lo = R.decode_bf16_hilo(wp, Co, Ci)
        return (hi.double() + lo.double()).numpy()[:, :Co, :Ci]

    good = R.encode_bf16_hilo(v)
    assert _violations(hilo_of(good), W, hb) == 0
    # one element moved to the neighbouring slot (the two exchange places)
    moved = good.clone()
    j = R._bf16_index(Co, Ci, 2, 0)[17, 9]
    moved[2, j], moved[2, j + 1] = good[2, j + 1], good[2, j]
    assert _violations(hilo_of(moved), W, hb) == 2
    # lo dropped
    hi, lo = R.decode_bf16_hilo(good, Co, Ci)
    assert _violations(hi.double().numpy()[:, :Co, :Ci], W, hb) > 0.9 * W.size
    # hi and lo fragments exchanged: the decoded sum is unchanged, so the parts are checked on their own as well
    swapped = good.reshape(B, -1, 2, 512).flip(2).reshape(B, -1)
    hs, ls = R.decode_bf16_hilo(swapped, Co, Ci)
    assert _violations(hs.double().numpy()[:, :Co, :Ci], W, b1) > 0.9 * W.size
    # samples 1 and 2 swapped; every sample of a block written to the block's first sample
    perm = good[[0, 2, 1, 3, 4]]
    assert _violations(hilo_of(perm)[1:3], W[1:3], hb[1:3]) > 0.9 * 2 * Co * Ci
    stale = good[[0, 0, 2, 2, 4]]
    assert _violations(hilo_of(stale), W, hb) > 0.9 * 2 * Co * Ci
    # plain pack: the last, ragged 32-column chunk never written (nkk = cols >> 5) - zeros where values belong
    plain = R.encode_b16(v)
    assert _violations(R.decode_b16(plain, Co, Ci).double().numpy()[:, :Co, :Ci], W, b1) == 0
    short = plain.reshape(B, 2, -1).clone()
    short[:, 1] = 0
    assert _violations(R.decode_b16(short.reshape(B, -1), Co, Ci).double().numpy()[:, :Co, :Ci], W, b1) > 0.9 * B * Co * 4
    # fp32 pack: a neighbouring slot
    f = R.encode_fp32(v)
    fb = R.aggregate_bound(A, K)
    assert _violations(R.decode_fp32(f, Co, Ci).double().numpy()[:, :Co], W, fb) == 0
    g = f.clone()
    j = R._fp32_index(Co, Ci)[17, 9]
    g[1, j], g[1, j + 1] = f[1, j + 1], f[1, j]
    assert _violations(R.decode_fp32(g, Co, Ci).double().numpy()[:, :Co], W, fb) == 2


def test_every_listed_batch_leaves_the_tail_block_short_of_a_full_one():
    """Replacing the tail block's sample count by SB would write past the last sample exactly where B % SB != 0: every
    multi-sample case of the list has such a tail, and its size is the one recorded."""
    for Co, Ci, K, B, sb, tail in R.BF16_PACK_CASES:
        assert (B - 1) % sb + 1 == tail and (sb == 1 or tail < sb)
    assert {c[4] for c in R.BF16_PACK_CASES} == {1, 2, 4, 8}


def test_samples_per_block_query_matches_the_case_list():
    """eat_dyn_pw_pack_samples_per_block is the loop the launch uses; the listed batches are the smallest that reach each value
    (one sample fewer per full block falls back to the next smaller SB)."""
    from efficientat_amd import _lib, build
    build.build()
    q = _lib.lib().eat_dyn_pw_pack_samples_per_block
    for Co, Ci, K, B, sb, tail in R.BF16_PACK_CASES:
        assert q(B, Co, Ci) == sb, (Co, Ci, B)
        if sb > 1:
            assert q(B - tail - sb, Co, Ci) == sb // 2, (Co, Ci, B)
    assert q(1, 16, 4) == 1 and q(9, 1344, 224) == 1
    assert q(68, 960, 160) == 1 and q(69, 960, 160) == 2            # dymn10's widest layer: SB > 1 from B = 69 on
    assert q(1 << 20, 16, 4) == 8
    assert q(0, 16, 4) == 1 and q(4, 0, 4) == 1
