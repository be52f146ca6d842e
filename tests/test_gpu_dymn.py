"""GPU parity of the DyMN eval forward (dynamic conv kernel aggregation, DyReLU-B, CoordAtt,
context generator) against the CPU oracle and the stored outputs of the unmodified reference."""
import contextlib
import io
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import eat_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import ops  # noqa: E402
from efficientat_amd.dymn import get_model  # noqa: E402

DEV = torch.device("cuda:0")


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _rel(got, ref):
    got, ref = got.detach().cpu().double().reshape(-1), ref.detach().double().reshape(-1)
    return float((got - ref).norm() / max(1e-30, float(ref.norm())))


@pytest.mark.parametrize("B,C,F_,T", [(2, 16, 64, 500), (3, 40, 16, 125), (2, 80, 8, 63), (3, 160, 4, 32), (1, 5, 3, 7)])
def test_ctx_pool(B, C, F_, T):
    x = _rand(B, C, F_, T, seed=1)
    ref = torch.cat([x.mean(dim=3), x.mean(dim=2)], dim=2).transpose(1, 2)       # (B, F+T, C)
    assert _rel(ops.ctx_pool(x.to(DEV)), ref) < 2e-6


# T = 1; T = 4096 (the last width whose [4][T] column partials fit LDS) and past it (block 0 of a clip longer than ~82 s);
# F + T > 16384 (the backward's gradient table no longer fits LDS either)
@pytest.mark.parametrize("B,C,F_,T", [(3, 5, 7, 1), (2, 3, 1, 9), (2, 3, 5, 4096), (2, 3, 5, 4097), (1, 4, 64, 4500),
                                      (1, 2, 3, 16500)])
def test_ctx_pools_and_their_backward_match_fp64(B, C, F_, T):
    """ctx_pool / ctx_pool_cm and both backward forms (the channel-major one with the main path's dx added) against
    fp64 autograd of the two means."""
    from efficientat_amd.dymn_train import CtxPool
    x = _rand(B, C, F_, T, seed=1)
    xr = x.double().requires_grad_(True)
    ref = torch.cat([xr.mean(dim=3), xr.mean(dim=2)], dim=2)                      # (B, C, F+T)
    L = F_ + T
    dseq = _rand(B, L, C, seed=2)
    ref.backward(dseq.double().transpose(1, 2))
    xd = x.to(DEV).requires_grad_(True)
    seq = CtxPool.apply(xd)
    assert seq.shape == (B, L, C) and _rel(seq, ref.detach().transpose(1, 2)) < 2e-6
    seq.backward(dseq.to(DEV))
    assert _rel(xd.grad, xr.grad) < 2e-6
    cm = ops.ctx_pool_cm(x.to(DEV))
    assert _rel(cm.view(C, B, L), ref.detach().permute(1, 0, 2)) < 2e-6
    add = _rand(B, C, F_, T, seed=3)
    dcm = dseq.permute(2, 0, 1).contiguous().view(1, C, B * L, 1)
    dx = ops.ctx_pool_cm_bwd(dcm.to(DEV), (B, C, F_, T), add=add.to(DEV))
    assert _rel(dx, xr.grad + add.double()) < 2e-6


@pytest.mark.parametrize("H,B,F_,T,stride", [(5, 3, 7, 9, 2), (4, 2, 1, 1, 2), (3, 2, 5, 1, 1), (6, 3, 5, 125, 2),
                                             (4, 3, 3, 63, 2), (3, 2, 8, 4097, 1), (2, 3, 64, 4500, 2)])
def test_ctx_split_and_backward_match_fp64(H, B, F_, T, stride):
    """ctx_split (AvgPool(3, stride 2, pad 1) of both halves for stride 2, odd lengths included; the mean h_c) and its
    backward against fp64 autograd."""
    L = F_ + T
    g = _rand(H, B, L, seed=1)
    gr = g.double().requires_grad_(True)
    pool = (lambda r: r) if stride == 1 else (lambda r: F.avg_pool1d(r, 3, 2, 1, count_include_pad=True))
    hcf, hct, hc = pool(gr[..., :F_]), pool(gr[..., F_:]), gr.mean(-1).t()
    Fo, To = hcf.shape[-1], hct.shape[-1]
    dcf, dct, dc = _rand(H, B, Fo, seed=2), _rand(H, B, To, seed=3), _rand(B, H, seed=4)
    torch.autograd.backward([hcf, hct, hc], [dcf.double(), dct.double(), dc.double()])
    gcf, gct, gc = ops.ctx_split(g.view(1, H, B * L, 1).to(DEV), B, F_, T, stride)
    assert gcf.shape == (1, H, B * Fo, 1) and gct.shape == (1, H, B * To, 1)
    assert _rel(gcf.view(H, B, Fo), hcf.detach()) < 1e-6 and _rel(gct.view(H, B, To), hct.detach()) < 1e-6
    assert _rel(gc, hc.detach()) < 1e-6
    dg = ops.ctx_split_bwd(dcf.reshape(1, H, B * Fo, 1).to(DEV), dct.reshape(1, H, B * To, 1).to(DEV), dc.to(DEV), H, B, F_, T,
                           stride)
    assert _rel(dg.view(H, B, L), gr.grad) < 1e-6


def test_dyn_aggregate_and_pack():
    B, K, Co, Ci = 3, 4, 40, 24
    bank, att = _rand(K, Co * Ci, seed=1), torch.softmax(_rand(B, K, seed=2), dim=-1)
    rs = torch.rand(Co, generator=torch.Generator().manual_seed(3)) + 0.5
    agg = ops.dyn_aggregate(bank.to(DEV), att.to(DEV), rs.to(DEV), Ci)
    ref = (att @ bank).view(B, Co, Ci) * rs[None, :, None]
    assert _rel(agg, ref) < 2e-6
    # per-sample packed weights through the per-sample 1x1 conv
    x = _rand(B, Ci, 8, 63, seed=4)
    wp = ops.dyn_pw_pack(bank.to(DEV), att.to(DEV), Co, Ci, rs.to(DEV))
    bias, res = _rand(Co, seed=5, scale=0.1), _rand(B, Co, 8, 63, seed=6)
    y = ops.pw_conv_dyn(x.to(DEV), wp, bias.to(DEV), Co, ops.ACT_HSWISH, res=res.to(DEV))
    yref = torch.stack([F.hardswish(F.conv2d(x[b:b + 1], ref[b].view(Co, Ci, 1, 1), bias))[0] for b in range(B)]) + res
    assert _rel(y, yref) < 5e-6


@pytest.mark.parametrize("B,C,F_,T,k,s", [(2, 32, 64, 500, 3, 1), (2, 48, 32, 250, 5, 2), (3, 240, 16, 125, 3, 2),
                                          (3, 96, 8, 63, 5, 1), (4, 160, 4, 32, 5, 1),
                                          # planes off the 128-mel / 10 s grid: 0.3 s clips (4x1, 8x2), 40 and 64 mels, 11 s
                                          (3, 16, 4, 1, 5, 1), (3, 24, 8, 2, 3, 1), (2, 24, 5, 125, 3, 1), (2, 24, 3, 63, 5, 1),
                                          (2, 24, 2, 31, 5, 1), (2, 8, 64, 550, 3, 1)])
def test_dw_conv_dyn(B, C, F_, T, k, s):
    x, w = _rand(B, C, F_, T, seed=1), _rand(B, C, k, k, seed=2, scale=0.3)
    bias, coef = _rand(C, seed=3, scale=0.1), _rand(B, C, 4, seed=4)
    z = F.conv2d(x.reshape(1, B * C, F_, T), w.reshape(B * C, 1, k, k), None, s, (k - 1) // 2, 1, B * C)
    z = z.reshape(B, C, *z.shape[2:]) + bias[None, :, None, None]
    Fo, To = z.shape[2], z.shape[3]
    gf, gt = _rand(B, Fo, C, seed=5), _rand(B, To, C, seed=6)
    c = coef[:, :, None, None, :]
    ref = torch.maximum(z * c[..., 0] + c[..., 2], z * c[..., 1] + c[..., 3])
    ref = ref * torch.sigmoid(gf.permute(0, 2, 1))[:, :, :, None] * torch.sigmoid(gt.permute(0, 2, 1))[:, :, None, :]
    got = ops.dw_conv_dyn(x.to(DEV), w.reshape(B, C * k * k).contiguous().to(DEV), bias.to(DEV), coef.contiguous().to(DEV),
                          gf.to(DEV), gt.to(DEV), k, s)
    assert _rel(got, ref) < 5e-6


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def test_dymn10_eval_matches_oracle_and_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "dymn10_ref.npz"))
    sd = synth.synth_state(synth.dymn_shapes(1.0), seed=0)
    for k in g.files:
        if k.startswith("bn/"):
            sd[k[3:]] = torch.from_numpy(g[k])
    temp = float(g["temp_eval"])
    model = _quiet(get_model, width_mult=1.0)
    model.load_state_dict(sd, strict=True)
    for m in model.modules():
        if hasattr(m, "temperature"):
            m.temperature = temp
    model.to(DEV).eval()
    x = O.mel_forward(synth.parity_clips(320000, seed=1234)).unsqueeze(1)
    with torch.no_grad():
        ref_logits, ref_fmaps = O.dymn_forward(sd, x, temperature=temp, return_fmaps=True)
        logits, fmaps = model(x.to(DEV), return_fmaps=True)
        logits2, feat = model(x.to(DEV))
    assert len(fmaps) == 17
    for i, (a, b) in enumerate(zip(fmaps, ref_fmaps)):
        assert a.shape == b.shape
        assert _rel(a, b) < 2e-4, (i, _rel(a, b))
    # synthetic dynamic weights amplify the loud-noise clip (|logit| ~ 1e2): compare relative to the
    # per-sample logit scale, which is <= 1e-3 absolute for the O(1) samples
    scale = np.maximum(1.0, np.abs(g["eval_logits"]).max(axis=1, keepdims=True))
    assert (np.abs(logits.cpu().numpy() - ref_logits.numpy()) / scale).max() < 1e-3
    assert (np.abs(logits.cpu().numpy() - g["eval_logits"]) / scale).max() < 1e-3
    assert (np.abs(logits2.cpu().numpy() - g["eval_logits"]) / scale).max() < 1e-3
    assert feat.shape == (5, 960)


# ----------------------------------------------------------------------------- training step
def test_dyrelu_coordatt_backward():
    from efficientat_amd.dymn_train import DyReluCoordAtt
    B, C, Fo, To = 3, 24, 8, 63
    v, coef = _rand(B, C, Fo, To, seed=1), _rand(B, C, 4, seed=2)
    gf, gt, dout = _rand(B, Fo, C, seed=3), _rand(B, To, C, seed=4), _rand(B, C, Fo, To, seed=5)
    ts = [t.clone().requires_grad_(True) for t in (v, coef, gf, gt)]
    c = ts[1][:, :, None, None, :]
    ref = torch.maximum(ts[0] * c[..., 0] + c[..., 2], ts[0] * c[..., 1] + c[..., 3])
    ref = ref * torch.sigmoid(ts[2].permute(0, 2, 1))[:, :, :, None] * torch.sigmoid(ts[3].permute(0, 2, 1))[:, :, None, :]
    ref.backward(dout)
    td = [t.detach().to(DEV).requires_grad_(True) for t in (v, coef, gf, gt)]
    out = DyReluCoordAtt.apply(*td)
    out.backward(dout.to(DEV))
    assert _rel(out, ref) < 5e-6
    for a, b in zip(td, ts):
        assert _rel(a.grad, b.grad) < 2e-5


def _dyrelu_ca_fp64(z, a, b, coef, gf, gt, dout):
    """fp64 autograd of DyReLU-B * CoordAtt on v = a z + b: gates position-major (B, L, C).  -> out, (dv, dcoef, dgf, dgt)"""
    C = z.shape[1]
    cr, gfr, gtr = (t.double().clone().requires_grad_(True) for t in (coef, gf, gt))
    v = (z.double() * a.double().view(1, C, 1, 1) + b.double().view(1, C, 1, 1)).requires_grad_(True)
    c = cr[:, :, None, None, :]
    ref = torch.maximum(v * c[..., 0] + c[..., 2], v * c[..., 1] + c[..., 3])
    ref = ref * torch.sigmoid(gfr.permute(0, 2, 1))[:, :, :, None] * torch.sigmoid(gtr.permute(0, 2, 1))[:, :, None, :]
    ref.backward(dout.double())
    return ref.detach(), (v.grad, cr.grad, gfr.grad, gtr.grad)


DYRELU2_WIDTHS = [1, 2, 3, 15, 16, 17, 31, 33, 64, 65, 255, 257, 511, 512]     # every cut of EAT_DYRELU2_DISPATCH and its odd edges


@pytest.mark.parametrize("To", DYRELU2_WIDTHS)
def test_dyrelu_ca2_edge_widths_match_fp64(To):
    """eat_dyrelu_ca_fwd2 / _bwd2 (fp32 storage) at every lane layout of the dispatch, with Fo of 1, 2, 3 and 5 rows (the
    clamped last row group of the RU-row unroll) and a plane count that leaves the last wave part-filled."""
    B, C = 2, 37
    for Fo in (1, 2, 3, 5):
        z, coef = _rand(B, C, Fo, To, seed=1), _rand(B, C, 4, seed=2)
        gf, gt, dout = _rand(B, Fo, C, seed=3), _rand(B, To, C, seed=4), _rand(B, C, Fo, To, seed=5)
        a, b = _rand(C, seed=6).abs() + 0.5, _rand(C, seed=7)
        ref, (gv, gc, ggf, ggt) = _dyrelu_ca_fp64(z, a, b, coef, gf, gt, dout)
        zd, cd, ad, bd, dd = (t.to(DEV) for t in (z, coef, a, b, dout))
        gfd, gtd = gf.permute(2, 0, 1).contiguous().to(DEV), gt.permute(2, 0, 1).contiguous().to(DEV)
        out = ops.dyrelu_ca_fwd2(zd, ad, bd, cd, gfd, gtd)
        assert _rel(out, ref) < 5e-6, Fo
        dv, dcoef, dgf, dgt, bnpart = ops.dyrelu_ca_bwd2(dd, zd, ad, bd, cd, gfd, gtd)
        assert _rel(dv, gv) < 2e-5 and _rel(dcoef, gc) < 2e-5, Fo
        assert _rel(dgf, ggf.permute(2, 0, 1)) < 2e-5 and _rel(dgt, ggt.permute(2, 0, 1)) < 2e-5, Fo
        assert _rel(bnpart[..., 0], gv.sum((2, 3))) < 2e-5 and _rel(bnpart[..., 1], (gv * z.double()).sum((2, 3))) < 2e-5, Fo


def test_dyrelu_ca2_refuses_rows_wider_than_512():
    from efficientat_amd._lib import EatHipError
    z, coef = torch.zeros(1, 2, 3, 513, device=DEV), torch.zeros(1, 2, 4, device=DEV)
    gf, gt = torch.zeros(2, 1, 3, device=DEV), torch.zeros(2, 1, 513, device=DEV)
    with pytest.raises(EatHipError):
        ops.dyrelu_ca_fwd2(z, None, None, coef, gf, gt)
    with pytest.raises(EatHipError):
        ops.dyrelu_ca_bwd2(z, z, None, None, coef, gf, gt)


@pytest.mark.parametrize("Fo,To", [(2, 550), (3, 2250), (2, 4500), (1, 10000)])
def test_dyrelu_coordatt_wide_rows(Fo, To):
    """The plane-per-block kernels (eat_dyrelu_ca_fwd / _bwd) of the unfused path on the rows of long clips: 4500 columns
    (block 0 of 90 s) no longer fit one row of column partials per wave in LDS.  Past what fits at all, a clean EatHipError."""
    from efficientat_amd._lib import EatHipError
    from efficientat_amd.dymn_train import DyReluCoordAtt
    B, C = 2, 3
    v, coef = _rand(B, C, Fo, To, seed=1), _rand(B, C, 4, seed=2)
    gf, gt, dout = _rand(B, Fo, C, seed=3), _rand(B, To, C, seed=4), _rand(B, C, Fo, To, seed=5)
    one, zero = torch.ones(C), torch.zeros(C)
    ref, grads = _dyrelu_ca_fp64(v, one, zero, coef, gf, gt, dout)
    td = [t.to(DEV).requires_grad_(True) for t in (v, coef, gf, gt)]
    out = DyReluCoordAtt.apply(*td)
    assert _rel(out, ref) < 5e-6
    if To > 8000:                                  # (Fo + 2 To + 16) floats of LDS: more than 64 KB
        with pytest.raises(EatHipError):
            out.backward(dout.to(DEV))
        return
    out.backward(dout.to(DEV))
    for t, g in zip(td, grads):
        assert _rel(t.grad, g) < 2e-5


def test_dyrelu_coordatt_refuses_gates_that_do_not_fit_lds():
    from efficientat_amd._lib import EatHipError
    from efficientat_amd.dymn_train import DyReluCoordAtt
    v = torch.zeros(1, 1, 1, 17000, device=DEV)
    with pytest.raises(EatHipError):
        DyReluCoordAtt.apply(v, torch.zeros(1, 1, 4, device=DEV), torch.zeros(1, 1, 1, device=DEV),
                             torch.zeros(1, 17000, 1, device=DEV))


@pytest.mark.parametrize("B,C,Fo,To", [(3, 24, 8, 63), (3, 7, 4, 32), (2, 5, 16, 125), (2, 6, 32, 250), (1, 3, 64, 500), (2, 9, 5, 20)])
def test_dyrelu_coordatt_wave_per_plane_forms(B, C, Fo, To):
    """Round-4 forms (channel-major pre-sigmoid gates, one wave per plane, BatchNorm affine on load, BatchNorm-backward sums
    in the epilogue) against fp64 autograd of models/dymn/dy_block.py:172-201 applied to v = a z + b."""
    z, coef = _rand(B, C, Fo, To, seed=1), _rand(B, C, 4, seed=2)
    gf, gt, dout = _rand(B, Fo, C, seed=3), _rand(B, To, C, seed=4), _rand(B, C, Fo, To, seed=5)
    a, b = _rand(C, seed=6).abs() + 0.5, _rand(C, seed=7)
    zr, cr, gfr, gtr = (t.double().clone().requires_grad_(True) for t in (z, coef, gf, gt))
    v = zr * a.double().view(1, C, 1, 1) + b.double().view(1, C, 1, 1)
    v.retain_grad()
    c = cr[:, :, None, None, :]
    ref = torch.maximum(v * c[..., 0] + c[..., 2], v * c[..., 1] + c[..., 3])
    ref = ref * torch.sigmoid(gfr.permute(0, 2, 1))[:, :, :, None] * torch.sigmoid(gtr.permute(0, 2, 1))[:, :, None, :]
    ref.backward(dout.double())
    zd, cd, ad, bd, dd = (t.to(DEV) for t in (z, coef, a, b, dout))
    gfd, gtd = gf.permute(2, 0, 1).contiguous().to(DEV), gt.permute(2, 0, 1).contiguous().to(DEV)     # (C, B, Fo) / (C, B, To)
    out = ops.dyrelu_ca_fwd2(zd, ad, bd, cd, gfd, gtd)
    assert _rel(out, ref) < 5e-6
    dv, dcoef, dgf, dgt, bnpart = ops.dyrelu_ca_bwd2(dd, zd, ad, bd, cd, gfd, gtd)
    assert _rel(dv, v.grad) < 2e-5 and _rel(dcoef, cr.grad) < 2e-5
    assert _rel(dgf, gfr.grad.permute(2, 0, 1)) < 2e-5 and _rel(dgt, gtr.grad.permute(2, 0, 1)) < 2e-5
    assert _rel(bnpart[..., 0], v.grad.sum((2, 3))) < 2e-5
    assert _rel(bnpart[..., 1], (v.grad * z.double()).sum((2, 3))) < 2e-5
    # channel sums of the BatchNorm backward from the partials
    mean, invstd = _rand(C, seed=8), _rand(C, seed=9).abs() + 0.5
    sums, dgam, dbet = ops.bn_bwd_combine_partials(bnpart, bnpart.view(-1)[1:], 2, B, C, 1, mean.to(DEV), invstd.to(DEV))
    xhat = (z.double() - mean.double().view(1, C, 1, 1)) * invstd.double().view(1, C, 1, 1)
    assert _rel(sums[:C], v.grad.sum((0, 2, 3))) < 2e-5 and _rel(sums[C:], (v.grad * xhat).sum((0, 2, 3))) < 2e-5
    assert _rel(dgam, (v.grad * xhat).sum((0, 2, 3))) < 2e-5 and _rel(dbet, v.grad.sum((0, 2, 3))) < 2e-5


@pytest.mark.parametrize("B,C,Fq,T,k,s,act", [(3, 8, 64, 500, 3, 1, 1), (2, 8, 64, 500, 3, 2, 1), (3, 12, 32, 250, 5, 2, 1),
                                              (5, 20, 16, 125, 5, 1, 2), (3, 24, 16, 125, 3, 2, 2), (5, 20, 8, 63, 3, 1, 2),
                                              (3, 16, 8, 63, 5, 2, 2), (7, 12, 4, 32, 5, 1, 2), (2, 6, 6, 40, 3, 1, 0),
                                              # off the 128-mel / 10 s grid: 4x1, 8x2, 5x125, 3x63, 2x31 and 64x550 outputs
                                              (3, 8, 4, 1, 3, 1, 2), (3, 8, 8, 2, 5, 1, 2), (3, 8, 10, 250, 3, 2, 2),
                                              (3, 8, 6, 125, 3, 2, 1), (3, 8, 2, 31, 5, 1, 2), (2, 8, 64, 550, 3, 1, 1)])
def test_dynamic_depthwise_train_kernels(B, C, Fq, T, k, s, act):
    """Round-4 train-mode passes of the dynamic depthwise conv (per-(b,c) taps): forward with the expand BatchNorm +
    activation on load and depth_norm's statistics in the epilogue; merged backward with depth_norm's backward on load -
    against fp64 autograd of  z_d = conv_bc(act(a_e z_e + b_e)),  v = BN_batch(z_d)  (dy_block.py:313-348)."""
    KK = k * k
    z_e, taps = _rand(B, C, Fq, T, seed=1), _rand(B, C * KK, seed=2, scale=0.3)
    a_e, b_e = _rand(C, seed=3).abs() + 0.5, _rand(C, seed=4, scale=0.3)
    gam, bet = _rand(C, seed=5).abs() + 0.5, _rand(C, seed=6)
    actf = {0: lambda t: t, 1: torch.relu, 2: F.hardswish}[act]
    zr, tr = z_e.double().clone().requires_grad_(True), taps.double().clone().requires_grad_(True)
    u = zr * a_e.double().view(1, C, 1, 1) + b_e.double().view(1, C, 1, 1)
    y = actf(u)
    zd_ref = F.conv2d(y.reshape(1, B * C, Fq, T), tr.reshape(B * C, 1, k, k), None, s, (k - 1) // 2, 1, B * C)
    zd_ref = zd_ref.reshape(B, C, *zd_ref.shape[2:])
    Fo, To = zd_ref.shape[2], zd_ref.shape[3]
    mu, var = zd_ref.mean((0, 2, 3)), zd_ref.var((0, 2, 3), unbiased=False)
    invstd = 1.0 / torch.sqrt(var + 1e-3)
    v = (zd_ref - mu.view(1, C, 1, 1)) * (invstd * gam.double()).view(1, C, 1, 1) + bet.double().view(1, C, 1, 1)
    dv = _rand(B, C, Fo, To, seed=7)
    # keep the incoming gradient away from activation kinks of u
    kink = torch.zeros_like(u, dtype=torch.bool)
    for kp in ({1: [0.0], 2: [-3.0, 3.0]}.get(act, [])):
        kink |= (u.detach() - kp).abs() < 1e-3
    v.backward(dv.double())
    # ---- forward
    zd, parts = ops.dw_conv_dyn_stats(z_e.to(DEV), taps.to(DEV), k, s, tf=(a_e.to(DEV), b_e.to(DEV), act))
    assert _rel(zd, zd_ref) < 5e-6
    bn = torch.nn.BatchNorm2d(C, eps=1e-3, momentum=0.01).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(gam); bn.bias.copy_(bet)
    st = ops.bn_state_from_partials(parts, bn, B * Fo * To)
    assert _rel(st[2], mu) < 1e-5 and _rel(st[3], invstd.detach()) < 1e-5
    # ---- backward: the channel sums as the DyReLU kernel would hand them over, then the merged kernel
    vg = dv.double()
    xhat = ((zd_ref - mu.view(1, C, 1, 1)) * invstd.view(1, C, 1, 1)).detach()
    sums = torch.cat([vg.sum((0, 2, 3)), (vg * xhat).sum((0, 2, 3))]).to(DEV)
    g, dw, p3 = ops.dw_conv_dyn_bwd_bn_g(dv.to(DEV), zd, st, ops.ACT_NONE, sums, taps.to(DEV), z_e.to(DEV), a_e.to(DEV),
                                         b_e.to(DEV), act, k, s)
    gu = (zr.grad / a_e.double().view(1, C, 1, 1)).masked_fill(kink, 0.0)            # gradient w.r.t. u
    assert _rel(g.cpu().double().masked_fill(kink, 0.0), gu) < 3e-5
    assert _rel(dw, tr.grad) < 3e-5
    gp = p3[0][:B * C * p3[2]].view(B, C, p3[2]).sum(-1).cpu().double()
    gz = p3[1][:B * C * p3[2]].view(B, C, p3[2]).sum(-1).cpu().double()
    gfull = g.cpu().double()
    assert _rel(gp, gfull.sum((2, 3))) < 1e-5 and _rel(gz, (gfull * z_e.double()).sum((2, 3))) < 1e-5
    # no expand conv: identity transform, the skip connection's gradient added to g
    if s == 1:
        res = _rand(B, C, Fq, T, seed=8)
        one, zero = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        zr2 = z_e.double().clone().requires_grad_(True)
        zd2 = F.conv2d(zr2.reshape(1, B * C, Fq, T), taps.double().reshape(B * C, 1, k, k), None, s, (k - 1) // 2, 1, B * C)
        zd2 = zd2.reshape(B, C, Fo, To)
        mu2, var2 = zd2.mean((0, 2, 3)), zd2.var((0, 2, 3), unbiased=False)
        v2 = (zd2 - mu2.view(1, C, 1, 1)) * (gam.double() / torch.sqrt(var2 + 1e-3)).view(1, C, 1, 1)
        v2.backward(dv.double())
        zd2g, parts2 = ops.dw_conv_dyn_stats(z_e.to(DEV), taps.to(DEV), k, s)
        st2 = ops.bn_state_from_partials(parts2, bn, B * Fo * To)
        xh2 = ((zd2 - mu2.view(1, C, 1, 1)) / torch.sqrt(var2 + 1e-3).view(1, C, 1, 1)).detach()
        sums2 = torch.cat([vg.sum((0, 2, 3)), (vg * xh2).sum((0, 2, 3))]).to(DEV)
        dx, _, _ = ops.dw_conv_dyn_bwd_bn_g(dv.to(DEV), zd2g, st2, ops.ACT_NONE, sums2, taps.to(DEV), z_e.to(DEV), one, zero,
                                            ops.ACT_NONE, k, s, res=res.to(DEV), want_sums=False)
        assert _rel(dx, zr2.grad + res.double()) < 3e-5


# dw shapes: a generic one plus every geometry of the register-resident plane kernels (dw_plane.hip: forward, data and
# per-plane weight gradient), with odd sample counts for the two-planes-per-wave forms
@pytest.mark.parametrize("kind", ["pw", "dw", (7, 8, 63, 3, 1), (5, 16, 125, 5, 1), (6, 8, 63, 5, 2), (9, 16, 125, 3, 2),
                                  (10, 4, 32, 5, 1), (3, 4, 20, 5, 1), (6, 32, 250, 3, 1), (4, 32, 250, 5, 2), (3, 20, 300, 3, 2)])
def test_dynamic_conv_backward(kind):
    from efficientat_amd.dymn_train import DynDwConv, DynPwConv
    B, K = 3, 4
    if kind == "pw":
        Ci, Co, Fq, T = 24, 40, 8, 63
        x, w = _rand(B, Ci, Fq, T, seed=1), _rand(1, 1, K, Co * Ci, seed=2, scale=Ci ** -0.5)
    else:
        C, Fq, T, k, s = (24, 16, 125, 5, 2) if kind == "dw" else kind
        x, w = _rand(B, C, Fq, T, seed=1), _rand(1, 1, K, C * k * k, seed=2, scale=0.3)
        kind = "dw"
    att = torch.softmax(_rand(B, K, seed=3), dim=-1)
    xr, wr, ar = (t.clone().requires_grad_(True) for t in (x, w, att))
    agg = ar @ wr[0, 0]
    if kind == "pw":
        y = torch.stack([F.conv2d(xr[b:b + 1], agg[b].view(Co, Ci, 1, 1))[0] for b in range(B)])
    else:
        y = F.conv2d(xr.reshape(1, B * C, Fq, T), agg.reshape(B * C, 1, k, k), None, s, (k - 1) // 2, 1, B * C)
        y = y.reshape(B, C, *y.shape[2:])
    dz = _rand(*y.shape, seed=4)
    y.backward(dz)
    xd, wd, ad = (t.detach().to(DEV).requires_grad_(True) for t in (x, w, att))
    out = DynPwConv.apply(xd, wd, ad, Co) if kind == "pw" else DynDwConv.apply(xd, wd, ad, k, s)
    out.backward(dz.to(DEV))
    assert _rel(out, y) < 5e-6
    assert _rel(xd.grad, xr.grad) < 2e-5 and _rel(wd.grad, wr.grad) < 2e-5 and _rel(ad.grad, ar.grad) < 2e-5


@pytest.mark.parametrize("prec", ["fp32", "auto"])
def test_dymn10_train_step_matches_oracle(golden_dir, prec):
    """One training step of dymn10 against torch-CPU autograd over the oracle (and the reference's stored loss / logits).
    'fp32': every GEMM on the exact fp32 MFMA - the arithmetic of the reference's CPU path; gradient bars = SURVEY 8c
    (rel-L2 <= 1e-2 per tensor: activation-kink flips).  'auto' (the default of a training step, what bench.py times):
    split bf16 operands from C_in = 40 on put ~1e-5 of relative noise on every such GEMM - about 100x the fp32
    re-association noise, so about 100x as many pre-activations change side at a ReLU / Hardswish kink and the per-tensor
    differences grow from ~1e-3 to ~1e-2 (same mechanism): 5e-2 per tensor, 2e-2 median."""
    g = np.load(os.path.join(golden_dir, "dymn10_ref.npz"))
    sd = synth.synth_state(synth.dymn_shapes(1.0), seed=0)
    for k in g.files:
        if k.startswith("bn/"):
            sd[k[3:]] = torch.from_numpy(g[k])
    temp = float(g["temp_train"])
    x = O.mel_forward(synth.parity_clips(320000, seed=1234)).unsqueeze(1)
    y = torch.from_numpy(g["train_labels"])
    keep = torch.from_numpy(g["drop_keep"].astype(np.float32))
    skip = ("running_mean", "running_var", "num_batches_tracked", "lambdas", "init_v")
    sdr = {k: (v.clone().requires_grad_(True) if not k.endswith(skip) else v.clone()) for k, v in sd.items()}
    stats = {}
    logits_ref, _ = O.dymn_forward(sdr, x, temperature=temp, train=True, stats=stats, drop_mask=keep)
    F.binary_cross_entropy_with_logits(logits_ref, y).backward()

    model = _quiet(get_model, width_mult=1.0)
    model.load_state_dict(sd)
    for m in model.modules():
        if hasattr(m, "temperature"):
            m.temperature = temp
    model.to(DEV).train()
    model.train_precision = prec
    model._drop_mask_override = keep
    logits, emb = model(x.to(DEV))
    loss = F.binary_cross_entropy_with_logits(logits, y.to(DEV))
    loss.backward()
    # round-off floor of this network: the same step on the input with one-ulp noise, against the step above
    ctrl = _quiet(get_model, width_mult=1.0)
    ctrl.load_state_dict(sd)
    for m in ctrl.modules():
        if hasattr(m, "temperature"):
            m.temperature = temp
    ctrl.to(DEV).train()
    ctrl.train_precision = prec
    ctrl._drop_mask_override = keep
    xn = x * (1.0 + 2.0 ** -23 * torch.randn(x.shape, generator=torch.Generator().manual_seed(4321)))
    F.binary_cross_entropy_with_logits(ctrl(xn.to(DEV))[0], y.to(DEV)).backward()
    noise = {n: _rel(pc.grad, p.grad.cpu()) for (n, p), (_, pc) in zip(model.named_parameters(), ctrl.named_parameters())}
    del ctrl
    assert abs(loss.item() - float(g["train_loss"])) < 2e-5              # vs the unmodified reference
    assert np.abs(logits.detach().cpu().numpy() - g["train_logits"]).max() < 1e-3
    gmax = max(float(v.grad.norm()) for v in sdr.values() if getattr(v, "grad", None) is not None)
    rels, bad = [], []
    for name, p in model.named_parameters():
        ref = sdr[name].grad
        assert p.grad is not None, name
        if float(ref.norm()) < 1e-4 * gmax:      # zero-gradient BN biases, cancellation-dominated attention logits
            continue
        r = _rel(p.grad, ref)
        rels.append(r)
        if r > max(1e-2 if prec == "fp32" else 5e-2, 4 * noise[name]):   # the bar yields to 4x the tensor's round-off floor
            bad.append((name, r, noise[name]))
    nmed = float(np.median(list(noise.values())))
    print(f"dymn10 train step [{prec}]: gradient rel-L2 median {np.median(rels):.2e}, max {max(rels):.2e}"
          f"  (one-ulp input noise on the same step: median {nmed:.2e}, max {max(noise.values()):.2e})")
    assert not bad, bad[:8]
    assert float(np.median(rels)) < max(3e-3 if prec == "fp32" else 2e-2, 4 * nmed)
    msd = model.state_dict()
    for k, v in stats.items():
        assert _rel(msd[k], v) < 1e-4, k


@pytest.mark.parametrize("B,C,Fq,T,stride", [(4, 16, 64, 500, 1), (4, 24, 32, 250, 2), (3, 40, 16, 125, 2), (4, 80, 8, 63, 1),
                                             (5, 112, 8, 63, 2), (4, 160, 4, 32, 1)])
def test_context_generator_channel_major(B, C, Fq, T, stride):
    """Round-4 context generator (pools, joint conv + BatchNorm + Hardswish, h_c, pooled halves, conv_f / conv_t) on the
    channel-major sequence against fp64 autograd of models/dymn/dy_block.py:235-254 - outputs, input gradient and every
    parameter gradient."""
    from types import SimpleNamespace
    from efficientat_amd.dymn import ContextGen
    from efficientat_amd.dymn_train import _context_cm
    H, cexp = 32, 48
    torch.manual_seed(0)
    cg = ContextGen(H, C, cexp, stride=stride)
    with torch.no_grad():
        for prm in cg.parameters():
            prm.copy_(_rand(*prm.shape, seed=prm.numel() % 97, scale=0.3) + (1.0 if prm.dim() == 1 and prm.numel() == H else 0.0))
    x = _rand(B, C, Fq, T, seed=1)
    cgr = ContextGen(H, C, cexp, stride=stride).double()
    cgr.load_state_dict({k_: v.double() for k_, v in cg.state_dict().items()})
    cgr.train()
    xr = x.double().clone().requires_grad_(True)
    seq = torch.cat([xr.mean(3), xr.mean(2)], 2).unsqueeze(-1)                         # (B, C, F+T, 1)
    g = F.hardswish(cgr.joint_norm(cgr.joint_conv(seq)))
    h_c = g.mean((2, 3))
    pool = torch.nn.AvgPool2d((3, 1), (stride, 1), (1, 0)) if stride > 1 else torch.nn.Identity()
    g_cf, g_ct = cgr.conv_f(pool(g[:, :, :Fq])), cgr.conv_t(pool(g[:, :, Fq:]))
    d_hc, d_f, d_t = _rand(*h_c.shape, seed=2), _rand(*g_cf.shape, seed=3), _rand(*g_ct.shape, seed=4)
    ((h_c * d_hc).sum() + (g_cf * d_f).sum() + (g_ct * d_t).sum()).backward()
    cg.to(DEV).train()
    blk = SimpleNamespace(context_gen=cg, cnf=SimpleNamespace(stride=stride))
    xd = x.to(DEV).requires_grad_(True)
    with ops.precision("fp32"):
        hc, gf, gt = _context_cm(blk, xd)
    Fo, To = g_cf.shape[2], g_ct.shape[2]
    assert _rel(hc, h_c) < 5e-6
    assert _rel(gf.view(cexp, B, Fo), g_cf[..., 0].permute(1, 0, 2)) < 5e-6
    assert _rel(gt.view(cexp, B, To), g_ct[..., 0].permute(1, 0, 2)) < 5e-6
    loss = (hc * d_hc.to(DEV)).sum() + (gf.view(cexp, B, Fo) * d_f[..., 0].permute(1, 0, 2).to(DEV)).sum() + \
        (gt.view(cexp, B, To) * d_t[..., 0].permute(1, 0, 2).to(DEV)).sum()
    loss.backward()
    assert _rel(xd.grad, xr.grad) < 2e-3                     # Hardswish kinks of the context sequence
    for (n, prm), (_, ref) in zip(cg.named_parameters(), cgr.named_parameters()):
        assert _rel(prm.grad, ref.grad) < 2e-3, n
    assert _rel(cg.joint_norm.running_var, cgr.joint_norm.running_var) < 1e-5


@pytest.mark.parametrize("B,Ci,Co,Fq,T,res", [(3, 48, 144, 8, 63, False), (5, 160, 96, 4, 32, True), (2, 40, 20, 16, 125, False),
                                               (3, 224, 1344, 8, 63, False), (2, 44, 72, 3, 100, True)])
def test_pw_conv_dyn_bf16x3(B, Ci, Co, Fq, T, res):
    """Per-sample-weight 1x1 conv on split bf16 operands (eat_dyn_pw_pack_bf16 + eat_pw_conv_dyn_bf16_fwd) against an
    fp64 evaluation of models/dymn/dy_block.py:111-127 and against the exact-fp32 per-sample kernel."""
    K = 4
    x, bank = _rand(B, Ci, Fq, T, seed=1), _rand(K, Co * Ci, seed=2, scale=Ci ** -0.5)
    att = torch.softmax(_rand(B, K, seed=3), dim=-1)
    r = _rand(B, Co, Fq, T, seed=4) if res else None
    W = (att.double() @ bank.double()).view(B, Co, Ci)
    ref = torch.einsum("boi,bis->bos", W, x.double().flatten(2)).view(B, Co, Fq, T)
    if res:
        ref = ref + r.double()
    xd, bd, ad = x.to(DEV), bank.to(DEV), att.to(DEV)
    zero = torch.zeros(Co, device=DEV)
    rd = r.to(DEV) if res else None
    got = ops.pw_conv_dyn_bf16(xd, ops.dyn_pw_pack_bf16(bd, ad, Co, Ci), zero, Co, ops.ACT_NONE, res=rd)
    exact = ops.pw_conv_dyn(xd, ops.dyn_pw_pack(bd, ad, Co, Ci), zero, Co, ops.ACT_NONE, res=rd)
    assert _rel(got, ref) < 3e-5
    assert _rel(got, exact.cpu()) < 3e-5
    # the packs from the bank of the transposed matrices (the data-gradient form: no transposed bank copy) are the same bits
    if Co % 4 == 0:
        bank_t = bank.view(K, Co, Ci).transpose(1, 2).contiguous().view(K, Ci * Co).to(DEV)
        assert torch.equal(ops.dyn_pw_pack_bf16(bank_t, ad, Co, Ci, trans=True), ops.dyn_pw_pack_bf16(bd, ad, Co, Ci))
        assert torch.equal(ops.dyn_pw_pack(bank_t, ad, Co, Ci, trans=True), ops.dyn_pw_pack(bd, ad, Co, Ci))


@pytest.mark.parametrize("prec", ["fp32", "auto"])
@pytest.mark.parametrize("i,Fq,T", [(0, 64, 500), (1, 64, 500), (3, 32, 250), (5, 16, 125), (12, 8, 63), (13, 4, 32)])
def test_dy_block_train_forward_backward(i, Fq, T, prec):
    """One DY_Block in train mode (stride 1 and 2, with/without expand, with/without residual): output,
    input gradient and every parameter gradient vs torch-CPU autograd over the oracle block; in the exact fp32
    arithmetic and in the default 'auto' arithmetic of a training step (bf16x3 from C_in = 40 on, K-concat late layers)."""
    from efficientat_amd.dymn_train import _block_train as _bt

    def _block_train(blk, x):
        with ops.precision(prec):
            return _bt(blk, x)
    sd = synth.synth_state(synth.dymn_shapes(1.0), seed=0)
    model = _quiet(get_model, width_mult=1.0)
    model.load_state_dict(sd)
    model.to(DEV).train()
    blocks, _ = O.block_table(1.0)
    c, B, temp = blocks[i], 3, 30.0
    H = O.context_dim(c["cexp"], 1.0)
    x = _rand(B, c["cin"], Fq, T, seed=i)
    skip = ("running_mean", "running_var", "num_batches_tracked", "lambdas", "init_v")
    sdr = {k: (v.clone().requires_grad_(True) if not k.endswith(skip) else v.clone())
           for k, v in sd.items() if k.startswith(f"layers.{i}.")}
    xr = x.clone().requires_grad_(True)
    out_ref = O._dy_block(sdr, f"layers.{i}", xr, c, H, True, {}, temp)
    dout = _rand(*out_ref.shape, seed=99)
    out_ref.backward(dout)
    blk = model.layers[i]
    for m in blk.modules():
        if hasattr(m, "temperature"):
            m.temperature = temp
    xd = x.to(DEV).requires_grad_(True)
    out = _block_train(blk, xd)
    out.backward(dout.to(DEV))
    assert _rel(out, out_ref) < (5e-6 if prec == "fp32" else 5e-5)
    # random inputs put a few pre-activations next to a ReLU/Hardswish kink: allow 1 % there
    assert _rel(xd.grad, xr.grad) < 1e-2
    gmax = max(float(v.grad.norm()) for v in sdr.values() if getattr(v, "grad", None) is not None)
    for n, p in blk.named_parameters():
        ref = sdr[f"layers.{i}.{n}"].grad
        if float(ref.norm()) > 1e-4 * gmax:
            assert _rel(p.grad, ref) < 2e-2, (n, _rel(p.grad, ref))


@pytest.mark.parametrize("B,K,N", [(37, 4, 1000), (128, 4, 6400), (5, 4, 1002), (9, 3, 64)])
def test_dyn_bank_grad(B, K, N):
    """dbank = att^T G, datt = G bank^T (gradients of the kernel aggregation, models/dymn/dy_block.py:103-131): the
    one-pass kernel (K = 4, N % 4 == 0) and the two-pass fallback."""
    from efficientat_amd.dymn_train import _bank_grad
    G, att, bank = _rand(B, N, seed=1), torch.softmax(_rand(B, K, seed=2), dim=-1), _rand(K, N, seed=3)
    dbank, datt = _bank_grad(G.to(DEV), att.to(DEV), bank.to(DEV))
    assert _rel(dbank, att.double().t() @ G.double()) < 2e-6
    assert _rel(datt, G.double() @ bank.double().t()) < 2e-6


@pytest.mark.parametrize("R,C", [(64000, 32), (8064, 1344), (1000, 7), (3, 300), (16000, 240)])
def test_col_sum(R, C):
    m = _rand(R, C, seed=1)
    got = ops.col_sum(m.to(DEV))
    assert _rel(got, m.double().sum(0)) < 2e-6


@pytest.mark.parametrize("B,Ci,Co,Fq,T,act,res", [(3, 64, 96, 4, 32, 2, False), (5, 160, 160, 4, 32, 0, True),
                                                   (2, 32, 200, 8, 63, 1, False), (4, 320, 48, 2, 10, 0, False)])
@pytest.mark.parametrize("stream", [0, 15])
def test_pw_conv_kcat(B, Ci, Co, Fq, T, act, res, stream):
    """Dynamic 1x1 conv as one GEMM over the K-concatenated banks with the attention as input scale
    (models/dymn/dy_block.py:103-131) vs the per-sample aggregated-weight formulation; bf16x3 arithmetic; on the LDS-staged
    kernel (stream 0) and on the K-streaming kernel of csrc/conv_pw_stream.hip (stream 15)."""
    K = 4
    if (Fq * T) % 4:
        pytest.skip("K-concat form needs planes of a multiple of 4 positions")
    x, bank = _rand(B, Ci, Fq, T, seed=1), _rand(K, Co * Ci, seed=2, scale=Ci ** -0.5)
    att = torch.softmax(_rand(B, K, seed=3), dim=-1)
    rs, bias = torch.rand(Co, generator=torch.Generator().manual_seed(4)) + 0.5, _rand(Co, seed=5, scale=0.1)
    r = _rand(B, Co, Fq, T, seed=6) if res else None
    W = (att.double() @ bank.double()).view(B, Co, Ci) * rs.double()[None, :, None]
    ref = torch.einsum("boi,bist->bost", W, x.double()) + bias.double()[None, :, None, None]
    ref = [ref, F.relu(ref), F.hardswish(ref)][act]
    if res:
        ref = ref + r.double()
    wp = ops.kcat_pack(bank.to(DEV), Co, Ci, rs.to(DEV))
    prev = ops.pw_stream_mode(stream)
    try:
        got = ops.pw_conv_kcat(x.to(DEV), wp, bias.to(DEV), att.to(DEV), Co, act, res=None if r is None else r.to(DEV))
    finally:
        ops.pw_stream_mode(prev)
    assert _rel(got, ref) < 3e-5


@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_dymn_captured_step_reproduces_its_gradients_on_every_replay(storage):
    """A captured training step (graphs.GraphedTrainStep) of a dynamic network must produce, on EVERY replay, the gradients of the
    eager step on the same parameters and input (learning rate 0: nothing moves between replays).  Guards the zero-initialised
    accumulators of the step inside a hipGraph: with `hipMemsetAsync` nodes (ROCm 7.0) the batch-sliced bank gradients of the small
    DynamicConv layers and the column sums were not re-zeroed reliably from the second replay on - silent accumulation of the
    previous replay's values, and a NaN loss in ~1 of 20 fresh processes of the dymn20 bench leg; they are kernels now."""
    from efficientat_amd.graphs import GraphedTrainStep
    sd = synth.synth_state(synth.dymn_shapes(1.0), seed=0)
    B = 16
    x = O.mel_forward(synth.parity_clips(320000, seed=31)[[0, 2, 3, 4]]).unsqueeze(1).repeat(4, 1, 1, 1)
    x = (x * (1.0 + 0.01 * _rand(B, 1, 1, 1, seed=3))).to(DEV)
    y = (torch.rand(B, 527, generator=torch.Generator().manual_seed(5)) < 0.01).float().to(DEV)
    keep = (torch.rand(B, 1280, generator=torch.Generator().manual_seed(6)) < 0.8).float()

    def build():
        m = _quiet(get_model, width_mult=1.0)
        m.load_state_dict(sd)
        for mod in m.modules():
            if hasattr(mod, "temperature"):
                mod.temperature = 30.0
        m.to(DEV).train()
        m._drop_mask_override = keep.to(DEV)           # (on the device: a host-to-device copy is not capturable)
        if storage == "bf16":
            m.train_precision, m.act_storage = "bf16", "bf16"
        return m
    ref = build()
    logits, _ = ref(x)
    F.binary_cross_entropy_with_logits(logits, y).backward()
    ref_g = {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
    gmax = max(float(g.norm()) for g in ref_g.values())
    model = build()
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    step = GraphedTrainStep(model, opt, F.binary_cross_entropy_with_logits, x, y)
    tol = 2e-3 if storage == "fp32" else 3e-2          # atomics order (fp32) / rounding-boundary flips between two bf16 evaluations
    for r in range(4):
        step(step.x, step.y)
        torch.cuda.synchronize()
        worst = (0.0, None)
        for n, p in model.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), (r, n)
            if float(ref_g[n].norm()) < 1e-3 * gmax:
                continue
            e = _rel(p.grad, ref_g[n].cpu())
            if e > worst[0]:
                worst = (e, n)
        assert worst[0] < tol, (r, worst)
