"""DyMN's per-sample weight kernels (csrc/dymn.hip: dyn_aggregate, dyn_pw_pack, dyn_pw_pack_bf16<4> / <0> as hi / lo and plain
bf16 packs, dyn_bank_grad) and the fp32 per-sample 1x1 conv (csrc/conv_pw.hip: eat_pw_conv_dyn_fwd) called directly through
`ops`, against the fp64 oracle tests/dyn_weights_ref.py.

The packs are DECODED (the decoders are written from the layouts' documentation and the consumer kernels, and are held against
independent encoders in tests/test_dyn_weights_ref_cpu.py): every real element within a bound derived from the arithmetic, every
padding element of every sample the bit pattern +0, the `trans` form the same bits.  The batches of the bf16 cases are the
smallest that make a block pack 2, 4 and 8 consecutive samples (register-resident bank tiles, the `b0 + sb` output offset, a
short tail block, the barriers between samples); which branch a case takes is asserted with
eat_dyn_pw_pack_samples_per_block, so a retune of the launch makes the case list fail instead of silently falling back to one
sample per block.  The conv reads a pack encoded on the CPU, so neither kernel can hide behind the other.

The hi part of a hi / lo pack is also held, on its own, to the plain-bf16 bound and to the bits of the plain pack: hi and lo
in each other's slots leave hi + lo unchanged.

Largest errors observed on an MI355X, in units of the bound (`pytest -s` prints them; every pack bound carries the factor 2
for a split fma, which these kernels do not need - 0.5 is a rounding term fully used):
  bf16 packs     hi + lo 0.25, plain / hi 0.50, the same at 1, 2, 4 and 8 samples per block and for K = 3, 4, 5
  fp32 pack      0.37 plain, 0.35 with row_scale          dyn_aggregate  0.41
  pw_conv_dyn    0.14 (the bound is the worst case of a Ci-term sum)
  dyn_bank_grad  0.45 at B = 3 and 7, 0.40 at 262 148 columns, 0.05 sliced over the batch, 0.02 on the two-pass kernels
  pw_conv_dyn_bf16 on the 2-samples-per-block pack: 4.4e-6 of the output's norm (bar 3e-5)
Checked by hand against four deliberately broken builds of the bf16 pack kernel (not kept): the output offset without `+ sb`,
the second barrier of the per-sample loop removed, `nkk = cols >> 5`, hi and lo slots exchanged - the first two fail every
case with more than one sample per block (the missing barrier: those with register-resident bank tiles), the last two fail
every case.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from tests import dyn_weights_ref as R  # noqa: E402

from efficientat_amd import _lib, ops  # noqa: E402
from efficientat_amd._lib import EatHipError  # noqa: E402

DEV = torch.device("cuda:0")


def _ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (a zero bound demands equality)."""
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(r.max())


def _report(kernel, case, ratio):
    print(f"\n[error/bound] {kernel} {case}: {ratio:.3f}")


# ------------------------------------------------------------------------------------------------------------- bf16 packs
@pytest.mark.parametrize("Co,Ci,K,B,sb,tail", R.BF16_PACK_CASES)
def test_bf16_packs_decode_to_the_fp64_aggregate(Co, Ci, K, B, sb, tail):
    assert _lib.lib().eat_dyn_pw_pack_samples_per_block(B, Co, Ci) == sb          # the branch this case is here for
    assert (B - 1) % sb + 1 == tail
    bank, att = R.pack_operands(B, K, Co, Ci)
    bd, ad = bank.to(DEV), att.to(DEV)
    hl_d, p1_d = ops.dyn_pw_pack_bf16(bd, ad, Co, Ci), ops.dyn_pw_pack_b16(bd, ad, Co, Ci)
    # (c) the packs from the bank of the transposed matrices are the same bits
    bt = R.transposed_bank(bank, Co, Ci).to(DEV)
    assert torch.equal(ops.dyn_pw_pack_bf16(bt, ad, Co, Ci, trans=True), hl_d)
    assert torch.equal(ops.dyn_pw_pack_b16(bt, ad, Co, Ci, trans=True), p1_d)
    hi, lo = R.decode_bf16_hilo(hl_d.cpu(), Co, Ci)
    p1 = R.decode_b16(p1_d.cpu(), Co, Ci)
    # (b) padding rows / columns of every sample: +0 in every part
    pad = R.padding_mask(Co, Ci, hi.shape[1], hi.shape[2])
    assert pad.any()
    for part in (hi, lo, p1):
        assert R.is_plus_zero(part)[:, pad].all()
    # the hi part and the plain pack round the same fp32 aggregate
    assert torch.equal(hi.view(torch.int16), p1.view(torch.int16))
    # (a) every real element, sample by sample (chunks keep the fp64 temporaries small)
    W, A = R.aggregate(bank, att)
    W, A = W.reshape(B, Co, Ci), A.reshape(B, Co, Ci)
    r_hilo = r_plain = 0.0
    for s in range(0, B, 128):
        e = min(B, s + 128)
        h, l = hi[s:e, :Co, :Ci].double().numpy(), lo[s:e, :Co, :Ci].double().numpy()
        r_hilo = max(r_hilo, _ratio(h + l, W[s:e], R.hilo_pack_bound(W[s:e], A[s:e], K)))
        r_plain = max(r_plain, _ratio(h, W[s:e], R.b16_pack_bound(W[s:e], A[s:e], K)))
    _report("dyn_pw_pack_bf16 hi+lo", (Co, Ci, K, B, sb), r_hilo)
    _report("dyn_pw_pack_b16 / hi", (Co, Ci, K, B, sb), r_plain)
    assert r_hilo <= 1.0 and r_plain <= 1.0


def test_bf16_pack_feeds_its_consumer_at_two_samples_per_block():
    B, Ci, Co, Fq, T, K = 317, 36, 200, 2, 4, 4
    assert _lib.lib().eat_dyn_pw_pack_samples_per_block(B, Co, Ci) == 2
    bank, att = R.pack_operands(B, K, Co, Ci)
    x = torch.randn(B, Ci, Fq, T, generator=torch.Generator().manual_seed(5))
    W = (att.double() @ bank.double()).view(B, Co, Ci)
    ref = torch.einsum("boi,bis->bos", W, x.double().flatten(2)).view(B, Co, Fq, T)
    got = ops.pw_conv_dyn_bf16(x.to(DEV), ops.dyn_pw_pack_bf16(bank.to(DEV), att.to(DEV), Co, Ci), torch.zeros(Co, device=DEV),
                               Co, ops.ACT_NONE)
    rel = float((got.cpu().double() - ref).norm() / ref.norm())
    _report("pw_conv_dyn_bf16 (relative to the output's norm)", (B, Ci, Co, Fq, T), rel / 3e-5)
    assert rel < 3e-5


# -------------------------------------------------------------------------------------------------------------- fp32 pack
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("Co,Ci", [(7, 4), (200, 36), (72, 260), (16, 256)])
def test_fp32_pack_decodes_to_the_fp64_aggregate(Co, Ci, scaled):
    B, K = 3, 4
    bank, att = R.pack_operands(B, K, Co, Ci)
    rs = torch.rand(Co, generator=torch.Generator().manual_seed(3)) + 0.5 if scaled else None
    rsd = rs.to(DEV) if scaled else None
    bd, ad = bank.to(DEV), att.to(DEV)
    n = R.fp32_pack_len(Co, Ci)
    # the pack inside guard bands of a value no pack holds: its neighbours must come back untouched (16 x 256 has no padding
    # of its own that a misplaced store could hide in)
    guard, mark = 256, 12345.0
    buf = torch.full((guard + B * n + guard,), mark, device=DEV)
    _lib.call("eat_dyn_pw_pack", bd.data_ptr(), ad.data_ptr(), None if rsd is None else rsd.data_ptr(),
              buf.data_ptr() + 4 * guard, B, K, Co, Ci, torch.cuda.current_stream().cuda_stream)
    host = buf.cpu()
    assert bool((host[:guard] == mark).all()) and bool((host[guard + B * n:] == mark).all())
    wp = host[guard:guard + B * n].reshape(B, n).contiguous()
    assert torch.equal(ops.dyn_pw_pack(bd, ad, Co, Ci, rsd).cpu(), wp)
    if Co % 4 == 0:
        bt = R.transposed_bank(bank, Co, Ci).to(DEV)
        assert torch.equal(ops.dyn_pw_pack(bt, ad, Co, Ci, rsd, trans=True).cpu(), wp)
    D = R.decode_fp32(wp, Co, Ci)
    pad = R.padding_mask(Co, Ci, D.shape[1], Ci)
    assert pad.any() == (Co % 16 != 0) and R.is_plus_zero(D)[:, pad].all()
    W, A = R.aggregate(bank, att)
    W, A = W.reshape(B, Co, Ci), A.reshape(B, Co, Ci)
    if scaled:
        s64 = rs.double().numpy()[None, :, None]
        W = W * s64
        bound = R.aggregate_bound(A, K, W, s64)
    else:
        bound = R.aggregate_bound(A, K)
    r = _ratio(D[:, :Co].double().numpy(), W, bound)
    _report("dyn_pw_pack", (Co, Ci, "row_scale" if scaled else "plain"), r)
    assert r <= 1.0


# ---------------------------------------------------------------------------------------------------------- dyn_aggregate
@pytest.mark.parametrize("K", [1, 3, 4, 8])
@pytest.mark.parametrize("N", [5, 256, 257, 262144 + 260])      # one thread block +- 1; the grid-stride loop with a ragged end
def test_dyn_aggregate_matches_fp64(N, K):
    B = 2
    g = torch.Generator().manual_seed(17 * N + K)
    bank, att = torch.randn(K, N, generator=g), torch.softmax(3.0 * torch.randn(B, K, generator=g), dim=-1)
    bd, ad = bank.to(DEV), att.to(DEV)
    worst = 0.0
    for group in (None, 1, 9, 25, 36):                            # no scale; per element; 3 x 3 and 5 x 5 taps; a row of Ci = 36
        if group is None:
            got = ops.dyn_aggregate(bd, ad)
            W, A = R.aggregate(bank, att)
            bound = R.aggregate_bound(A, K)
        else:
            gs = torch.rand((N + group - 1) // group, generator=g) + 0.5
            got = ops.dyn_aggregate(bd, ad, gs.to(DEV), group)
            W, A = R.aggregate(bank, att, gs, group)
            s64 = gs.double().numpy()[np.arange(N) // group][None, :]
            bound = R.aggregate_bound(A, K, W, s64)
        assert got.shape == (B, N)
        r = _ratio(got.cpu().double().numpy(), W, bound)
        assert r <= 1.0, (group, r)
        worst = max(worst, r)
    _report("dyn_aggregate", (N, K), worst)


# ------------------------------------------------------------------------------------- fp32 per-sample conv on an encoded pack
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("act", [0, 1, 2])
@pytest.mark.parametrize("S", [4, 252, 256, 260, 516])          # a 256-column tile +- 4; two tiles, the second 4 wide; three
def test_pw_conv_dyn_on_a_cpu_encoded_pack(S, act, res):
    B, Ci, Co = 3, 36, 200
    g = torch.Generator().manual_seed(1000 * S + 10 * act + res)
    W = torch.randn(B, Co, Ci, generator=g) * Ci ** -0.5
    x, bias = torch.randn(B, Ci, 2, S // 2, generator=g), torch.randn(Co, generator=g)
    r = torch.randn(B, Co, 2, S // 2, generator=g) if res else None
    got = ops.pw_conv_dyn(x.to(DEV), R.encode_fp32(W).to(DEV), bias.to(DEV), Co, act, res=r.to(DEV) if res else None)
    ref, bound = R.pw_conv_dyn(x.flatten(2), W, bias, act, None if r is None else r.flatten(2))
    ratio = _ratio(got.cpu().double().numpy().reshape(B, Co, S), ref, bound)
    _report("pw_conv_dyn", (S, act, res), ratio)
    assert ratio <= 1.0


# ---------------------------------------------------------------------------------------------------------- dyn_bank_grad
def _bank_grad_case(B, K, N):
    g = torch.Generator().manual_seed(7 * B + 3 * K + N)
    return (torch.randn(B, N, generator=g), torch.softmax(3.0 * torch.randn(B, K, generator=g), dim=-1),
            torch.randn(K, N, generator=g))


# fused kernel (K = 4, N % 4 == 0): B < 8 in one slice; a batch sliced over the grid (dbank zero-filled, atomics); more than 64
# column tiles (one slice, plain stores, no zero-fill); 2 B K floats past 48 KiB: the two-pass kernels; K != 4 / N % 4 != 0: two-pass
@pytest.mark.parametrize("B,K,N", [(3, 4, 8), (7, 4, 1000), (40, 4, 1000), (16, 4, 65536 * 4 + 4), (1537, 4, 64), (5, 3, 10)])
def test_dyn_bank_grad_matches_fp64(B, K, N):
    G, att, bank = _bank_grad_case(B, K, N)
    # dbank arrives as NaN: whichever branch runs has to write (or zero-fill and accumulate) every element
    dbank = torch.full((K, N), float("nan"), device=DEV)
    datt = torch.zeros(B, K, device=DEV)
    Gd, ad, bd = G.to(DEV), att.to(DEV), bank.to(DEV)
    _lib.call("eat_dyn_bank_grad", Gd.data_ptr(), ad.data_ptr(), bd.data_ptr(), dbank.data_ptr(), datt.data_ptr(), B, K, N,
              torch.cuda.current_stream().cuda_stream)
    db_ref, da_ref, db_bound, da_bound = R.bank_grad(G, att, bank)
    r_b = _ratio(dbank.cpu().double().numpy(), db_ref, db_bound)
    r_a = _ratio(datt.cpu().double().numpy(), da_ref, da_bound)
    _report("dyn_bank_grad dbank / datt", (B, K, N), max(r_b, r_a))
    assert r_b <= 1.0 and r_a <= 1.0
    db2, da2 = ops.dyn_bank_grad(Gd, ad, bd)
    assert _ratio(db2.cpu().double().numpy(), db_ref, db_bound) <= 1.0
    assert _ratio(da2.cpu().double().numpy(), da_ref, da_bound) <= 1.0


def test_dyn_bank_grad_refuses_what_its_kernels_cannot_hold():
    G, att, bank = _bank_grad_case(2, 9, 8)
    with pytest.raises(EatHipError, match=r"eat_dyn_bank_grad: K=9 > 8"):
        ops.dyn_bank_grad(G.to(DEV), att.to(DEV), bank.to(DEV))
    G, att, bank = _bank_grad_case(3073, 4, 4)                    # B K 4 bytes = 48 KiB + 16
    with pytest.raises(EatHipError, match=r"eat_dyn_bank_grad: batch too large"):
        ops.dyn_bank_grad(G.to(DEV), att.to(DEV), bank.to(DEV))
