"""The fp64 Adam / AdamW reference (oracle/adam_ref.py) that the FusedAdam kernel tests check against, itself checked against
torch.optim.Adam / AdamW (single-tensor path) on float64 CPU parameters - no GPU needed."""
import pytest
import torch

from oracle.adam_ref import adam_step


def _run_reference(params, grads_per_step, lr, betas, eps, wd, decoupled):
    """Per-parameter state as torch keeps it: a parameter's step counts the steps on which it had a gradient."""
    p = [x.clone() for x in params]
    st = [None] * len(p)
    for grads in grads_per_step:
        for i, g in enumerate(grads):
            if g is None:
                continue
            if st[i] is None:
                st[i] = [torch.zeros_like(p[i]), torch.zeros_like(p[i]), 0]
            m, v, t = st[i]
            p[i], m1, v1, _ = adam_step(p[i], g, m, v, t + 1, lr, betas[0], betas[1], eps, wd, decoupled)
            st[i] = [m1, v1, t + 1]
    return p, st


@pytest.mark.parametrize("decoupled,wd", [(False, 0.0), (False, 3e-2), (True, 3e-2)])
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.0, 0.99)])
def test_fp64_adam_reference_matches_torch(decoupled, wd, betas):
    gen = torch.Generator().manual_seed(0)
    shapes = [(5,), (3, 4), (7,)]
    params = [torch.randn(s, generator=gen, dtype=torch.float64) for s in shapes]
    steps = []
    for it in range(6):
        grads = [torch.randn(s, generator=gen, dtype=torch.float64) * 10.0 ** (it - 2) for s in shapes]
        if it < 3:
            grads[2] = None                              # first gradient on the fourth step: its own t starts at 1
        if it == 4:
            grads[0] = None                              # skips a step: its t stays behind the others'
        steps.append(grads)
    lr, eps = 2e-3, 1e-8
    tp = [x.clone().requires_grad_(True) for x in params]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls(tp, lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
    for grads in steps:
        for x, g in zip(tp, grads):
            x.grad = None if g is None else g.clone()
        opt.step()
    ref, st = _run_reference(params, steps, lr, betas, eps, wd, decoupled)
    for i, x in enumerate(tp):
        s = opt.state[x]
        assert float(s["step"]) == st[i][2]
        torch.testing.assert_close(ref[i], x.detach(), rtol=1e-12, atol=1e-15)
        torch.testing.assert_close(st[i][0], s["exp_avg"], rtol=1e-12, atol=1e-15)
        torch.testing.assert_close(st[i][1], s["exp_avg_sq"], rtol=1e-12, atol=1e-15)
    assert [t for _, _, t in st] == [5, 6, 3]


def test_fp64_adam_reference_grad_scale_multiplies_before_the_l2_term():
    p, g, m, v = (torch.tensor([0.5, -2.0]), torch.tensor([1.0, 3.0]), torch.zeros(2), torch.zeros(2))
    a = adam_step(p, g, m, v, 1, 1e-3, 0.9, 0.999, 1e-8, weight_decay=0.1, decoupled=False, grad_scale=0.25)
    b = adam_step(p, g * 0.25, m, v, 1, 1e-3, 0.9, 0.999, 1e-8, weight_decay=0.1, decoupled=False)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
    assert torch.equal(a[3]["g1"], g.double() * 0.25 + 0.1 * p.double())
