"""GPU tests of the step's small dense-algebra and finalize kernels at the smallest shapes that cross their internal
cuts (csrc/se_train.hip: the chunk ring of gemm_tile, the k-slice cut, col_sum_tile; csrc/train_fuse.hip: the j slices
of gram_bn_finalize_g, 4 / 16 waves per tile in expand_bwd_wcat; csrc/stem_train.hip: the two-level sums of the stem
finalizes).  References are fp64 on the CPU, built as tests/test_gpu_train_fuse.py builds them, with its bars."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import ops  # noqa: E402

DEV = torch.device("cuda:0")
ACTS = [lambda t: t, F.relu, F.hardswish]


def _rand(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _rel(got, ref, floor=1e-30):
    """|got - ref| / max(|ref|, floor); floor: the size of the terms a reference that cancels to zero is made of."""
    got = got.detach().cpu().double().reshape(-1)
    ref = ref.detach().cpu().double().reshape(-1)
    return float((got - ref).norm() / max(floor, float(ref.norm())))


def _bn_train_ref(z, gamma, beta, eps=1e-3):
    """fp64 training BatchNorm over (B, C, F, T) written out (F.batch_norm refuses one value per channel)."""
    mean = z.mean((0, 2, 3))
    var = z.var((0, 2, 3), unbiased=False)
    u = (z - mean.view(1, -1, 1, 1)) * (var.view(1, -1, 1, 1) + eps).rsqrt() * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)
    return u, mean, var


def _running_ref(mean, var, n, momentum=0.01):
    unbiased = var * n / (n - 1) if n > 1 else var
    return momentum * mean, (1.0 - momentum) + momentum * unbiased


# (1, 8, 2, 10): smallest; (33, 40, 10, 128): ragged 32-tiles on every axis; (9, 515, 129, 128): one block walks C in 9 chunks -
# every slot of the chunk ring is refilled, the last chunk is ragged, nothing a multiple of 4; (9, 1027, 129, 128): C just over
# 1024, where the contraction over C is split across blocks - 5 ragged k slices (k_lo > 0 on the ring, the slices behind dh,
# slice_sum_kernel with the ReLU gate); (257, 72, 24, 504): K = B just over 256 - the fifth chunk is fetched into the first
# chunk's registers while the tile is running
@pytest.mark.parametrize("B,C,Cr,S", [(1, 8, 2, 10), (33, 40, 10, 128), (9, 515, 129, 128), (9, 1027, 129, 128),
                                      (257, 72, 24, 504)])
def test_se_gate_mlp_backward_at_the_tile_and_chunk_edges(B, C, Cr, S):
    pool = _rand(B, C, seed=1) * S * 0.5
    W1, b1 = _rand(Cr, C, seed=2, scale=C ** -0.5), _rand(Cr, seed=3, scale=0.1)
    W2, b2 = _rand(C, Cr, seed=4, scale=Cr ** -0.5), _rand(C, seed=5, scale=0.1)
    ds = _rand(B, C, seed=6)
    pr = pool.double().requires_grad_(True)
    W1r, b1r, W2r, b2r = (t.double().requires_grad_(True) for t in (W1, b1, W2, b2))
    h_ref = F.relu(F.linear(pr / S, W1r, b1r))
    s_ref = torch.sigmoid(F.linear(h_ref, W2r, b2r))
    (s_ref * ds.double()).sum().backward()
    h = ops.linear(pool.to(DEV), W1.to(DEV), b1.to(DEV), ops.ACT_RELU, 1.0 / S)
    scale = ops.linear(h, W2.to(DEV), b2.to(DEV), ops.ACT_SIGMOID)
    args = (ds.to(DEV), scale, h, pool.to(DEV), W1.to(DEV), W2.to(DEV), S)
    out = ops.se_mlp_bwd(*args)
    errs = [_rel(got, ref) for got, ref in zip(out, (W1r.grad, b1r.grad, W2r.grad, b2r.grad, pr.grad))]
    print("se_mlp_bwd rel errors (dW1, db1, dW2, db2, gadd):", errs)
    assert max(errs) < 2e-5, errs
    again = ops.se_mlp_bwd(*args)
    assert all(torch.equal(p, q) for p, q in zip(out, again))               # fixed summation order


# (3, 33, 7, 5): small and ragged; (37, 130, 515, 10): dfeat's contraction over H in one block, 9 chunks through the ring;
# (5, 33, 1027, 10): H just over 1024 - dfeat's contraction split into 5 ragged k slices and summed by slice_sum_kernel
@pytest.mark.parametrize("B,C,H,N,drop", [(3, 33, 7, 5, True), (37, 130, 515, 10, False), (5, 33, 1027, 10, True)])
def test_classifier_head_backward_at_the_tile_and_chunk_edges(B, C, H, N, drop):
    feat = _rand(B, C, seed=1)
    W1, b1 = _rand(H, C, seed=2, scale=C ** -0.5), _rand(H, seed=3, scale=0.1)
    W2, b2 = _rand(N, H, seed=4, scale=H ** -0.5), _rand(N, seed=5, scale=0.1)
    mask = ((torch.rand(B, H, generator=torch.Generator().manual_seed(6)) < 0.8).float() / 0.8) if drop else None
    dl = _rand(B, N, seed=7)
    fr, W1r, b1r, W2r, b2r = (t.double().requires_grad_(True) for t in (feat, W1, b1, W2, b2))
    u_ref = F.linear(fr, W1r, b1r)
    near = (u_ref.detach().abs() - 3.0).abs() < 1e-4                     # Hardswish' jumps at +-3
    h2_ref = F.hardswish(u_ref) * (mask.double() if drop else 1.0)
    (F.linear(h2_ref, W2r, b2r) * dl.double()).sum().backward()
    u = u_ref.detach().float().to(DEV)
    h2 = h2_ref.detach().float().to(DEV)
    args = (dl.to(DEV), h2, u, mask.to(DEV) if drop else None, feat.to(DEV), W1.to(DEV), W2.to(DEV))
    dW1, db1, dW2, db2, dfeat = ops.mlp_head_bwd(*args)
    tol = 1e-3 if bool(near.any()) else 2e-5
    errs = [_rel(dW2, W2r.grad), _rel(db2, b2r.grad), _rel(dW1, W1r.grad), _rel(db1, b1r.grad), _rel(dfeat, fr.grad)]
    print("mlp_head_bwd rel errors (dW2, db2, dW1, db1, dfeat):", errs)
    assert errs[0] < 2e-5 and errs[1] < 2e-5
    assert max(errs[2:]) < tol
    assert all(torch.equal(p, q) for p, q in zip((dW1, db1, dW2, db2, dfeat), ops.mlp_head_bwd(*args)))


# Ci below the 64 columns of a pass and not a multiple of the four j slices (4, 5, 24), one pass exactly (64), three passes
# (192); Co odd and not a multiple of 4 or 8
@pytest.mark.parametrize("Co,Ci", [(1, 4), (7, 5), (33, 24), (130, 64), (250, 192)])
def test_gram_bn_state_from_small_and_ragged_gram_matrices(Co, Ci):
    B, F_, T = 2, 4, 8
    n = B * F_ * T
    x = (_rand(B, Ci, F_, T, seed=1) + 0.5 * _rand(1, Ci, 1, 1, seed=2)).double()
    W = _rand(Co, Ci, seed=3, scale=Ci ** -0.5)
    gamma, beta = torch.rand(Co, generator=torch.Generator().manual_seed(4)) + 0.5, _rand(Co, seed=5, scale=0.3)
    sx = x.sum((0, 2, 3))
    xc = x - (sx / n).view(1, Ci, 1, 1)
    G = torch.einsum("bift,bjft->ij", xc, xc).float()                     # the centred Gram matrix, as the kernel reads it
    Wd_, Gd_ = W.double(), G.double()
    mean_ref = Wd_ @ (sx.float().double() / n)
    var_ref = ((Wd_ @ Gd_) * Wd_).sum(1) / n
    is_ref = (var_ref + 1e-3).rsqrt()
    a_ref = gamma.double() * is_ref
    b_ref = beta.double() - mean_ref * a_ref
    rm_ref, rv_ref = _running_ref(mean_ref, var_ref, n)

    def run():
        bn = torch.nn.BatchNorm2d(Co, eps=1e-3, momentum=0.01).to(DEV).train()
        with torch.no_grad():
            bn.weight.copy_(gamma)
            bn.bias.copy_(beta)
        Tm, st = ops.gram_bn_state_g(G.to(DEV), W.to(DEV), sx.float().to(DEV), bn, n, centered=True)
        return (Tm, *st, bn.running_mean, bn.running_var)

    Tm, a, b, mean, invstd, rm, rv = run()
    errs = [_rel(Tm, Wd_ @ Gd_), _rel(mean, mean_ref), _rel(invstd, is_ref), _rel(a, a_ref), _rel(b, b_ref), _rel(rm, rm_ref),
            _rel(rv, rv_ref)]
    print("gram_bn_state_g rel errors (Tm, mean, invstd, a, b, running_mean, running_var):", errs)
    assert errs[0] < 1e-6
    assert errs[1] < 1e-5 and errs[2] < 2e-5 and errs[3] < 1e-5 and errs[4] < 1e-4
    assert errs[5] < 1e-5 and errs[6] < 2e-5                              # (updated exactly once)
    assert all(torch.equal(p, q) for p, q in zip((Tm, a, b, mean, invstd, rm, rv), run()))


# Co / 4 = 6 k-steps (4 waves per tile, 2 steps per wave, one wave idle), 18 (ragged last wave, ragged 16-tiles of Ci), 241 (16
# waves per tile, a wave has 16 steps: its one round of loads is full, Co not a multiple of 64 for c0's row groups)
@pytest.mark.parametrize("mode", ["fp32", "auto"])
@pytest.mark.parametrize("B,Ci,Co,F_,T,act", [(2, 8, 24, 4, 32, 1), (2, 20, 72, 4, 32, 2), (2, 160, 964, 4, 8, 2)])
def test_expand_backward_through_the_packed_operands(B, Ci, Co, F_, T, act, mode):
    exact, shift = mode == "fp32", 0.5
    x = _rand(B, Ci, F_, T, seed=1) + shift * _rand(1, Ci, 1, 1, seed=2)
    W = _rand(Co, Ci, seed=3, scale=Ci ** -0.5)
    gamma, beta = torch.rand(Co, generator=torch.Generator().manual_seed(4)) + 0.5, _rand(Co, seed=5, scale=0.3)
    dy = _rand(B, Co, F_, T, seed=6)
    xr, Wr = x.double().requires_grad_(True), W.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z_ref = F.conv2d(xr, Wr[:, :, None, None])
    u_ref, mean_ref, var_ref = _bn_train_ref(z_ref, gr, br)
    near = (u_ref.detach().abs() < 1e-3) if act == 1 else ((u_ref.detach().abs() - 3.0).abs() < 1e-3)
    dy = dy * (~near).float()
    u_leaf = u_ref.detach().requires_grad_(True)
    (ACTS[act](u_leaf) * dy.double()).sum().backward()
    g_ref = u_leaf.grad                                                   # dy * act'(u)
    (ACTS[act](u_ref) * dy.double()).sum().backward()

    xd, Wd = x.to(DEV), W.to(DEV)
    bn = torch.nn.BatchNorm2d(Co, eps=1e-3, momentum=0.01).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    n = B * F_ * T
    sx = xd.double().sum((0, 2, 3)).float().contiguous()
    G = ops.gram(xd, exact=exact, sx=sx)
    Tm, (a, b, mean, invstd) = ops.gram_bn_state_g(G, Wd, sx, bn, n, centered=True)
    with ops.precision(mode):
        z = ops.pw_conv(xd, ops.pw_prepack(Wd), torch.zeros(Co, device=DEV), Co, ops.ACT_NONE)
        g, gparts = ops.act_grad_sum(dy.to(DEV), z, a, b, act)
        Gx = ops.pw_conv_wgrad(g, xd, exact=exact)
        dW, dgam, dbet, wcat, c0 = ops.expand_bwd_coef_cat(Wd, Gx, Tm, sx, gparts, a, mean, invstd, n, centered=True)
        dx = ops.pw_conv_cat(g, xd, wcat, c0, Ci, ops.ACT_NONE)
    # e1 = a (m2 invstd mu - m1) in fp64 (csrc/train_fuse.hip (3)), c0 = e1 W
    is_ref = (var_ref.detach() + 1e-3).rsqrt()
    xhat = (z_ref.detach() - mean_ref.detach().view(1, -1, 1, 1)) * is_ref.view(1, -1, 1, 1)
    m1, m2 = g_ref.sum((0, 2, 3)) / n, (g_ref * xhat).sum((0, 2, 3)) / n
    e1 = gamma.double() * is_ref * (m2 * is_ref * mean_ref.detach() - m1)
    tol = (2e-5 if exact else 1e-4) * max(1.0, shift / 5.0)
    errs = [_rel(dW, Wr.grad), _rel(dgam, gr.grad), _rel(dbet, br.grad), _rel(dx, xr.grad), _rel(c0, e1 @ W.double())]
    print("expand backward rel errors (dW, dgamma, dbeta, dx, c0):", errs)
    assert max(errs) < tol, errs


# 1, 3 and 40 block partials (fewer than a group of the finalize sums, not a multiple of one); C * 10 entries per partial:
# 30 (less than a block's 32), 160, 210 (ragged last block)
@pytest.mark.parametrize("B,C,F_,T", [(1, 3, 2, 2), (3, 16, 9, 21), (5, 21, 128, 40)])
def test_stem_finalize_sums_over_few_and_ragged_partials(B, C, F_, T):
    x = _rand(B, 1, F_, T, seed=1) * 0.6 + 0.1
    W = _rand(C, 1, 3, 3, seed=2, scale=1.0 / 3)
    gamma, beta = torch.rand(C, generator=torch.Generator().manual_seed(4)) + 0.5, _rand(C, seed=5, scale=0.5)
    Wr = W.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    z_ref = F.conv2d(x.double(), Wr, stride=2, padding=1)
    u_ref, mean_ref, var_ref = _bn_train_ref(z_ref, gr, br)
    dy = _rand(*z_ref.shape, seed=6)
    near = (u_ref.detach().abs() - 3.0).abs() < 1e-3            # Hardswish' jumps at +-3: round-off of u flips a few elements
    dy = dy * (~near).float()
    u_leaf = u_ref.detach().requires_grad_(True)
    (F.hardswish(u_leaf) * dy.double()).sum().backward()
    g_ref = u_leaf.grad
    (F.hardswish(u_ref) * dy.double()).sum().backward()

    xd, Wd = x.to(DEV), W.reshape(C, 9).to(DEV)
    bn = torch.nn.BatchNorm2d(C, eps=1e-3, momentum=0.01).to(DEV).train()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    n = z_ref.numel() // C
    Tm, sp = ops.stem_gram(xd, Wd)
    Tm2, sp2 = ops.stem_gram(xd, Wd)
    assert torch.equal(Tm, Tm2) and torch.equal(sp, sp2)                      # fixed reduction order
    patches = F.unfold(x.double(), 3, padding=1, stride=2)                    # (B, 9, L)
    G9 = torch.einsum("bil,bjl->ij", patches, patches)
    e_tm, e_sp = _rel(Tm, W.reshape(C, 9).double() @ G9), _rel(sp, patches.sum((0, 2)))
    a, b, mean, invstd = ops.gram_bn_state(Tm, Wd, sp, bn, n)
    rm_ref, rv_ref = _running_ref(mean_ref.detach(), var_ref.detach(), n)
    e_state = [_rel(mean, mean_ref), _rel(invstd, (var_ref + 1e-3).rsqrt()), _rel(bn.running_mean, rm_ref), _rel(bn.running_var, rv_ref)]
    dy2 = _rand(*dy.shape, seed=9)
    bargs = ((dy - dy2).to(DEV), xd, Wd, a, b, ops.ACT_HSWISH)
    Gx, gparts = ops.stem_bwd(*bargs, dy2=dy2.to(DEV))                        # two summands, added on load
    Gx2, gparts2 = ops.stem_bwd(*bargs, dy2=dy2.to(DEV))
    assert torch.equal(Gx, Gx2) and torch.equal(gparts[0], gparts2[0])
    Gx_ref = torch.einsum("bcl,bkl->ck", g_ref.reshape(B, C, -1), patches)
    e_gx, e_s1 = _rel(Gx, Gx_ref), _rel(gparts[0], g_ref.sum((0, 2, 3)))
    dW, dgam, dbet = ops.expand_bwd_coef(Wd, Gx, Tm, sp, gparts, a, mean, invstd, n, need_dx=False)[:3]
    # with one output position per channel (n = 1) z - mean = 0: dW and dgamma are differences that cancel to zero; measure
    # them against the terms they are made of
    a_ref = (gamma.double() * (var_ref.detach() + 1e-3).rsqrt())
    e_dw = _rel(dW, Wr.grad, floor=1e-30 if n > 1 else float((a_ref[:, None] * Gx_ref).norm()))
    e_dg = _rel(dgam, gr.grad, floor=1e-30 if n > 1 else float(g_ref.abs().sum()))
    e_db = _rel(dbet, br.grad)
    print("stem rel errors (Tm, sp, mean, invstd, running_mean, running_var, Gx, s1, dW, dgamma, dbeta):",
          [e_tm, e_sp] + e_state + [e_gx, e_s1, e_dw, e_dg, e_db])
    assert e_tm < 1e-5 and e_sp < 1e-5
    assert e_state[0] < 1e-5 and e_state[1] < 2e-5 and e_state[2] < 1e-5 and e_state[3] < 2e-5
    assert e_gx < 2e-5 and e_s1 < 2e-5
    assert e_dw < 2e-5 and e_dg < 2e-5 and e_db < 2e-5
