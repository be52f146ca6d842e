"""`efficientat_amd.optim.FusedAdam` (one launch of eat_adam_multi over every parameter) against torch.optim.Adam / AdamW - the
optimizer of the reference's training loop (ex_audioset.py:86-91, 197-199)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd.optim import FusedAdam  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = [(1,), (3,), (527,), (16, 1, 3, 3), (960, 160, 1, 1), (1280, 960), (4097,), (4096,), (2, 4095)]


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).to(DEV).requires_grad_(True) for s in SHAPES]


@pytest.mark.parametrize("decoupled,wd", [(False, 0.0), (False, 1e-2), (True, 1e-2)])
@pytest.mark.parametrize("capturable", [False, True])
def test_fused_adam_matches_torch(decoupled, wd, capturable):
    pa, pb = _params(0), _params(0)
    ref_cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    ref = ref_cls(pa, lr=8e-4, weight_decay=wd, fused=True)       # the kernel whose expression types eat_adam_multi mirrors
    lr = torch.tensor(8e-4, device=DEV) if capturable else 8e-4
    opt = FusedAdam(pb, lr=lr, weight_decay=wd, decoupled=decoupled, capturable=capturable)
    g = torch.Generator().manual_seed(1)
    for it in range(7):
        for a, b in zip(pa, pb):
            gr = torch.randn(a.shape, generator=g).to(DEV) * (10.0 ** (it - 3))
            a.grad, b.grad = gr.clone(), gr.clone()
        ref.step()
        opt.step()
        for a, b in zip(pa, pb):
            assert torch.allclose(a, b, rtol=2e-6, atol=1e-7), (it, a.shape, float((a - b).abs().max()))
    for a, b in zip(pa, pb):
        sa, sb = ref.state[a], opt.state[b]
        # (the first moment is a difference of terms up to 1e3 times its own size here: round-off relative to the TERMS)
        assert torch.allclose(sa["exp_avg"], sb["exp_avg"], rtol=2e-6, atol=2e-6 * float(sa["exp_avg"].abs().max()))
        assert torch.allclose(sa["exp_avg_sq"], sb["exp_avg_sq"], rtol=2e-6, atol=1e-20)
        assert float(sb["step"]) == 7.0


def test_fused_adam_in_a_captured_graph_follows_the_eager_optimizer():
    pa, pb = _params(3), _params(3)
    ref = torch.optim.Adam(pa, lr=1e-3, fused=True)
    lr = torch.tensor(1e-3, device=DEV)
    opt = FusedAdam(pb, lr=lr, capturable=True)
    grads = [torch.zeros_like(p) for p in pb]
    for p, gr in zip(pb, grads):
        p.grad = gr
    opt.step()                                              # builds state + table outside the capture (zero gradients: no-op on p)
    for p in pa:
        p.grad = torch.zeros_like(p)
    ref.step()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            opt.step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.Generator().manual_seed(4)
    for it in range(5):
        if it == 3:
            lr.fill_(2e-4)                                  # a scheduler writing the tensor learning rate between replays
            for grp in ref.param_groups:
                grp["lr"] = 2e-4
        for a, gr in zip(pa, grads):
            v = torch.randn(a.shape, generator=g).to(DEV)
            a.grad.copy_(v)
            gr.copy_(v)
        ref.step()
        graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(pa, pb):
        assert torch.allclose(a, b, rtol=2e-6, atol=1e-7), float((a - b).abs().max())
    assert float(opt.state[pb[0]]["step"]) == 6.0


# ---------------------------------------------------------------------------------------------------------------------------
# against the fp64 reference (oracle/adam_ref.py), one step at a time: before every step() the fp32 p, g, exp_avg, exp_avg_sq
# and each parameter's step go to the host, the reference takes the same step from them in fp64, and the kernel's fp32 result
# must lie within `adam_step_bound` of it - a few 2^-24 relative to the magnitudes of the terms of each line of the update
# (the subnormal range: 2^-150 absolute on v).  Errors do not accumulate across steps, so the bound stays tight over many.

import io  # noqa: E402

import numpy as np  # noqa: E402

from efficientat_amd import _lib  # noqa: E402
from oracle.adam_ref import adam_step, adam_step_bound  # noqa: E402


def _groups_of(opt):
    return {p: g for g in opt.param_groups for p in g["params"]}


def _before(opt, ps):
    """Host copies of what the next step reads, per parameter (None: no gradient, the parameter must not move)."""
    out = []
    for p in ps:
        st = opt.state.get(p)
        z = torch.zeros(p.shape)
        out.append(dict(p=p.detach().cpu().clone(), g=None if p.grad is None else p.grad.detach().cpu().clone(),
                        m=st["exp_avg"].cpu().clone() if st else z, v=st["exp_avg_sq"].cpu().clone() if st else z,
                        t=int(float(st["step"])) + 1 if st else 1))
    return out


def _check_step(opt, ps, before, grad_scale=1.0, what=""):
    grp = _groups_of(opt)
    for i, (p, b) in enumerate(zip(ps, before)):
        if b["g"] is None:
            assert torch.equal(p.detach().cpu(), b["p"]), (what, i, "a parameter without gradient moved")
            continue
        g = grp[p]
        kw = dict(weight_decay=g["weight_decay"], decoupled=g["decoupled"], grad_scale=grad_scale)
        b1, b2 = g["betas"]
        p1, m1, v1, terms = adam_step(b["p"], b["g"], b["m"], b["v"], b["t"], float(g["lr"]), b1, b2, g["eps"], **kw)
        bounds = adam_step_bound(p1, m1, v1, terms, b1, b2, **kw)
        st = opt.state[p]
        assert float(st["step"]) == b["t"], (what, i, float(st["step"]), b["t"])
        for name, got, ref, bound in (("p", p, p1, bounds[0]), ("exp_avg", st["exp_avg"], m1, bounds[1]),
                                      ("exp_avg_sq", st["exp_avg_sq"], v1, bounds[2])):
            got = got.detach().cpu().double()
            assert torch.isfinite(got).all(), (what, i, name, "inf / NaN")
            err = (got - ref).abs()
            bad = err > bound
            if bad.any():
                j = int(torch.argmax(err / bound.clamp_min(1e-300)))
                raise AssertionError(f"{what}: parameter {i} {tuple(p.shape)} {name}[{j}] = {got.flatten()[j].item()!r}, fp64 "
                                     f"{ref.flatten()[j].item()!r}, |err| {err.flatten()[j].item():.3e} > bound "
                                     f"{bound.flatten()[j].item():.3e} ({int(bad.sum())} of {bad.numel()} elements, t={b['t']})")


def _grads(ps, gen, scale=1.0, skip=()):
    for i, p in enumerate(ps):
        p.grad = None if i in skip else (torch.randn(p.shape, generator=gen) * scale).to(DEV)


def _run_checked(opt, ps, steps, gen, scale=1.0, grad_scale=1.0, skip=lambda it: (), what=""):
    for it in range(steps):
        _grads(ps, gen, scale(it) if callable(scale) else scale, skip(it))
        b = _before(opt, ps)
        opt.step(grad_scale=grad_scale) if grad_scale != 1.0 else opt.step()
        torch.cuda.synchronize()
        _check_step(opt, ps, b, grad_scale, f"{what} step {it}")


SIZES = [1, 3, 4, 4095, 4096, 4097, 8191, 8193, (1 << 20) + 4099, 0]


@pytest.mark.parametrize("decoupled,wd", [(False, 0.0), (False, 1e-2), (True, 1e-2)])
@pytest.mark.parametrize("capturable", [False, True])
def test_fused_adam_matches_fp64_reference_across_sizes(decoupled, wd, capturable):
    gen = torch.Generator().manual_seed(10)
    ps = [torch.randn(n, generator=gen).to(DEV) for n in SIZES]
    lr = torch.tensor(1e-3, device=DEV) if capturable else 1e-3
    opt = FusedAdam(ps, lr=lr, weight_decay=wd, decoupled=decoupled, capturable=capturable)
    _run_checked(opt, ps, 4, gen, scale=lambda it: 10.0 ** (it - 2), what=f"decoupled={decoupled} wd={wd}")


def test_fused_adam_many_tiny_parameters_in_one_group():
    gen = torch.Generator().manual_seed(11)
    sizes = [1 + (i * 7) % 9 for i in range(1200)] + [4096 * 3 + 5]
    ps = [torch.randn(n, generator=gen).to(DEV) for n in sizes]
    opt = FusedAdam(ps, lr=3e-3, weight_decay=1e-2)
    _run_checked(opt, ps, 3, gen, what="1200 tiny")


def test_fused_adam_group_of_empty_parameters_is_a_no_op_like_torch():
    ps = [torch.zeros(0, device=DEV), torch.zeros(0, 5, device=DEV)]
    ref_ps = [p.clone() for p in ps]
    opt, ref = FusedAdam(ps, lr=1e-3), torch.optim.Adam(ref_ps, lr=1e-3, foreach=False)
    for _ in range(2):
        for p, q in zip(ps, ref_ps):
            p.grad, q.grad = torch.zeros_like(p), torch.zeros_like(q)
        opt.step()
        ref.step()
    torch.cuda.synchronize()
    for p, q in zip(ps, ref_ps):
        assert float(opt.state[p]["step"]) == float(ref.state[q]["step"]) == 2.0
    cap = FusedAdam([torch.zeros(0, device=DEV)], lr=torch.tensor(1e-3, device=DEV), capturable=True)
    cap.param_groups[0]["params"][0].grad = torch.zeros(0, device=DEV)
    cap.step()
    cap.step()
    assert float(cap.state[cap.param_groups[0]["params"][0]]["step"]) == 2.0


@pytest.mark.parametrize("offset", [1, 64])
def test_fused_adam_parameters_that_are_views_of_one_buffer(offset):
    """offset 1 float: every view starts 4 bytes past a 16-byte boundary although its length is a multiple of 4 (the scalar
    path); offset 64 floats: the 256-byte-aligned gradient views of the data-parallel reducer (the float4 path)."""
    gen = torch.Generator().manual_seed(12)
    lens = [4, 8, 4096, 4100, 8192, 12]
    starts = np.cumsum([offset] + [(n + 63) // 64 * 64 for n in lens[:-1]])
    total = int(starts[-1]) + lens[-1] + 64
    flat, gflat = torch.randn(total, generator=gen).to(DEV), torch.zeros(total, device=DEV)
    ps = [flat[s:s + n] for s, n in zip(starts, lens)]
    assert all((p.data_ptr() % 16 == 0) == (offset % 4 == 0) for p in ps)
    opt = FusedAdam(ps, lr=2e-3, weight_decay=1e-2)
    for it in range(3):
        gflat.copy_(torch.randn(total, generator=gen))
        for p, s in zip(ps, starts):
            p.grad = gflat[s:s + p.numel()]
        b = _before(opt, ps)
        opt.step()
        torch.cuda.synchronize()
        _check_step(opt, ps, b, what=f"offset {offset} step {it}")


HYPER = {
    "adam_l2": dict(weight_decay=1e-2),
    "adamw": dict(weight_decay=5e-2, decoupled=True),
    "beta1_0": dict(betas=(0.0, 0.99)),
    "eps_1e-30": dict(eps=1e-30),
    "adam_l2_grad_scale": dict(weight_decay=1e-1, grad_scale=0.37),
    "adamw_grad_scale": dict(weight_decay=1e-1, decoupled=True, grad_scale=4.0),
}


@pytest.mark.parametrize("case", list(HYPER))
def test_fused_adam_hyper_parameters_against_fp64(case):
    kw = dict(HYPER[case])
    grad_scale = kw.pop("grad_scale", 1.0)
    gen = torch.Generator().manual_seed(13)
    ps = [torch.randn(n, generator=gen).to(DEV) for n in (7, 4096, 5000)]
    opt = FusedAdam(ps, lr=1e-3, **kw)
    _run_checked(opt, ps, 4, gen, grad_scale=grad_scale, what=case)


@pytest.mark.parametrize("capturable", [False, True])
def test_fused_adam_at_a_large_step(capturable):
    """t >= 1e4 (bias corrections within 1e-4 of 1), reached through load_state_dict with random moments."""
    gen = torch.Generator().manual_seed(14)
    ps = [torch.randn(n, generator=gen).to(DEV) for n in (5, 4100)]
    lr = torch.tensor(1e-3, device=DEV) if capturable else 1e-3
    opt = FusedAdam(ps, lr=lr, weight_decay=1e-2, capturable=capturable)
    sd = opt.state_dict()
    sd["state"] = {i: dict(step=torch.tensor(20000.0), exp_avg=torch.randn(p.shape, generator=gen) * 1e-2,
                           exp_avg_sq=torch.rand(p.shape, generator=gen) * 1e-4) for i, p in enumerate(ps)}
    opt.load_state_dict(sd)
    _run_checked(opt, ps, 3, gen, what="t=2e4")
    assert float(opt.state[ps[0]]["step"]) == 20003.0


@pytest.mark.parametrize("scale,eps", [(0.0, 1e-8), (1e-20, 1e-8), (1e-20, 1e-30), (1e18, 1e-8)])
def test_fused_adam_gradient_magnitudes(scale, eps):
    """Exact zeros, 1e-20 (v = (1 - b2) g^2 ~ 1e-43 is subnormal in fp32: it must not be flushed, and with eps = 1e-30 the
    denominator is sqrt(v) itself), 1e18; mixed signs, a quarter of the elements exactly zero.  |g| / scale is kept in
    [0.5, 2]: a smaller g would put (1 - b2) g^2 below the smallest fp32 subnormal, where v stored in fp32 is 0 whatever the
    kernel does (and with eps = 1e-30 the step is then m / 1e-30 - the limit of fp32 moments, not of this kernel)."""
    gen = torch.Generator().manual_seed(15)
    ps = [torch.randn(n, generator=gen).to(DEV) for n in (3, 4096, 4097)]
    opt = FusedAdam(ps, lr=1e-3, eps=eps)
    for it in range(3):
        for p in ps:
            mag = 0.5 * 4.0 ** torch.rand(p.shape, generator=gen)
            g = torch.where(torch.rand(p.shape, generator=gen) < 0.5, -mag, mag) * scale
            g[torch.rand(p.shape, generator=gen) < 0.25] = 0.0
            p.grad = g.to(DEV)
        b = _before(opt, ps)
        opt.step()
        torch.cuda.synchronize()
        _check_step(opt, ps, b, what=f"|g|~{scale} eps={eps} step {it}")
    if scale == 1e-20:
        v = opt.state[ps[1]]["exp_avg_sq"]
        assert (v[ps[1].grad != 0] > 0).all(), "subnormal second moments flushed to zero"


@pytest.mark.parametrize("kind", ["float", "cuda_0dim", "cuda_1elem", "cpu_tensor", "cpu_float64"])
def test_fused_adam_learning_rate_forms(kind):
    lr = {"float": 2e-3, "cuda_0dim": torch.tensor(2e-3, device=DEV), "cuda_1elem": torch.tensor([2e-3], device=DEV),
          "cpu_tensor": torch.tensor(2e-3), "cpu_float64": torch.tensor(2e-3, dtype=torch.float64)}[kind]
    gen = torch.Generator().manual_seed(16)
    ps = [torch.randn(n, generator=gen).to(DEV) for n in (6, 4100)]
    opt = FusedAdam(ps, lr=lr, capturable=kind.startswith("cuda"))
    _run_checked(opt, ps, 2, gen, what=kind)


@pytest.mark.parametrize("lr", [torch.tensor(1e-3, dtype=torch.float64), torch.tensor(1e-3, dtype=torch.float16),
                                torch.tensor([1e-3, 2e-3])], ids=["float64", "float16", "numel2"])
def test_fused_adam_rejects_a_learning_rate_tensor_it_cannot_read(lr):
    p = torch.randn(8, device=DEV)
    opt = FusedAdam([p], lr=lr.to(DEV))
    p.grad = torch.ones_like(p)
    before = p.clone()
    with pytest.raises(_lib.EatHipError):
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(p, before)


def test_fused_adam_several_parameter_groups():
    gen = torch.Generator().manual_seed(17)
    ps = [torch.randn(n, generator=gen).to(DEV) for n in (5, 4097, 300, 8, 9000)]
    opt = FusedAdam([dict(params=ps[:2], lr=3e-3, weight_decay=1e-2),
                     dict(params=ps[2:4], lr=1e-4, betas=(0.5, 0.9), decoupled=True, weight_decay=0.2),
                     dict(params=ps[4:], eps=1e-6)], lr=1e-3)
    _run_checked(opt, ps, 3, gen, what="groups")


def _count_launches(monkeypatch):
    calls = []
    real = _lib.call

    def counting(name, *args):
        if name == "eat_adam_multi":
            calls.append(args)
        return real(name, *args)
    monkeypatch.setattr(_lib, "call", counting)
    return calls


def test_fused_adam_parameters_without_gradient_keep_their_own_step(monkeypatch):
    """torch's per-parameter step: a parameter whose first gradient comes on step 3 takes t = 1 there; one that skips a step
    stays one behind.  Eager mode still issues one launch per group (the table's step offsets)."""
    gen = torch.Generator().manual_seed(18)
    ps = [torch.randn(n, generator=gen).to(DEV) for n in (4, 4097, 33, 8192)]
    opt = FusedAdam(ps, lr=1e-3, weight_decay=1e-2)
    calls = _count_launches(monkeypatch)
    skip = {0: (1,), 1: (1, 2), 2: (), 3: (3,), 4: ()}
    _run_checked(opt, ps, 5, gen, skip=lambda it: skip[it], what="skips")
    assert len(calls) == 5
    assert [int(float(opt.state[p]["step"])) for p in ps] == [5, 3, 4, 4]


def test_fused_adam_capturable_refuses_a_shared_counter_that_would_be_wrong():
    ps = [torch.randn(n, device=DEV) for n in (4, 9)]
    opt = FusedAdam(ps, lr=torch.tensor(1e-3, device=DEV), capturable=True)
    ps[0].grad = torch.ones_like(ps[0])
    opt.step()
    ps[1].grad = torch.ones_like(ps[1])
    with pytest.raises(_lib.EatHipError, match="first"):
        opt.step()                                        # ps[1] would start at the group's counter (1), not at t = 1
    opt2 = FusedAdam([p.clone() for p in ps], lr=torch.tensor(1e-3, device=DEV), capturable=True)
    sd = opt2.state_dict()
    sd["state"] = {i: dict(step=torch.tensor(float(3 + i)), exp_avg=torch.zeros(p.shape), exp_avg_sq=torch.zeros(p.shape))
                   for i, p in enumerate(ps)}
    with pytest.raises(_lib.EatHipError, match="different steps"):
        opt2.load_state_dict(sd)


# ---- state-dict round trips ------------------------------------------------------------------------------------------------

def _make(capturable, decoupled, seed=20, cls=FusedAdam):
    gen = torch.Generator().manual_seed(seed)
    ps = [torch.randn(n, generator=gen).to(DEV) for n in (3, 4096, 4101, 17)]
    lr = torch.tensor(8e-4, device=DEV) if capturable else 8e-4
    if cls is FusedAdam:
        return ps, FusedAdam(ps, lr=lr, weight_decay=1e-2, decoupled=decoupled, capturable=capturable)
    tcls = torch.optim.AdamW if decoupled else torch.optim.Adam
    return ps, tcls(ps, lr=lr, weight_decay=1e-2, capturable=capturable, fused=True)


def _steps(opt, ps, first, n):
    for it in range(first, first + n):
        gen = torch.Generator().manual_seed(1000 + it)
        for p in ps:
            p.grad = (torch.randn(p.shape, generator=gen) * 10.0 ** (it % 3 - 1)).to(DEV)
        opt.step()
    torch.cuda.synchronize()


def _saved(opt):
    buf = io.BytesIO()
    torch.save(opt.state_dict(), buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("capturable", [False, True])
@pytest.mark.parametrize("stepped", [False, True], ids=["fresh", "already_stepped"])
def test_fused_adam_resume_is_bit_identical(decoupled, capturable, stepped):
    """k steps, state_dict -> torch.save / torch.load -> a FusedAdam (fresh, or one that has already taken steps of its own:
    its chunk table then holds the addresses of moment buffers the load replaces) -> m more steps == k + m steps."""
    k, m = 3, 3
    ps_a, a = _make(capturable, decoupled)
    _steps(a, ps_a, 0, k + m)
    ps_b, b = _make(capturable, decoupled)
    _steps(b, ps_b, 0, k)
    sd = _saved(b)
    ps_c, c = _make(capturable, decoupled)
    if stepped:
        _steps(c, ps_c, 50, 2)                           # other values, other moments: all overwritten by the load
    for p, q in zip(ps_c, ps_b):
        p.data.copy_(q)
    c.load_state_dict(sd)
    _steps(c, ps_c, k, m)
    for p, q in zip(ps_a, ps_c):
        assert torch.equal(p, q), float((p - q).abs().max())
    for p, q in zip(ps_a, ps_c):
        sa, sc = a.state[p], c.state[q]
        assert torch.equal(sa["exp_avg"], sc["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sc["exp_avg_sq"])
        assert float(sc["step"]) == k + m


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("capturable", [False, True])
def test_fused_adam_state_dict_round_trips_with_torch(decoupled, capturable):
    """torch -> FusedAdam and FusedAdam -> torch (through torch.save / torch.load): the next steps agree with torch's fused
    Adam, and every parameter's `step` advances by exactly one per step() (no step tensor shared between parameters)."""
    k, m = 3, 3
    ps_t, t = _make(capturable, decoupled, cls=None)
    _steps(t, ps_t, 0, k)
    ps_f, f = _make(capturable, decoupled)
    for p, q in zip(ps_f, ps_t):
        p.data.copy_(q)
    f.load_state_dict(_saved(t))
    ps_u, u = _make(capturable, decoupled, cls=None)       # FusedAdam -> torch
    for p, q in zip(ps_u, ps_f):
        p.data.copy_(q)
    u.load_state_dict(_saved(f))
    assert u.param_groups[0]["decoupled_weight_decay"] == decoupled
    for it in range(k, k + m):
        _steps(t, ps_t, it, 1)
        _steps(f, ps_f, it, 1)
        _steps(u, ps_u, it, 1)
        for opt, ps in ((f, ps_f), (u, ps_u)):
            assert [float(opt.state[p]["step"]) for p in ps] == [it + 1.0] * len(ps), (type(opt).__name__, it)
            for a, b in zip(ps_t, ps):
                assert torch.allclose(a, b, rtol=2e-6, atol=1e-7), (type(opt).__name__, it, float((a - b).abs().max()))


def test_fused_adam_load_into_a_captured_optimizer_writes_the_graphs_buffers():
    ps, opt = _make(True, False)
    grads = [torch.zeros_like(p) for p in ps]
    for p, g in zip(ps, grads):
        p.grad = g
    opt.step()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            opt.step()
    torch.cuda.current_stream().wait_stream(s)
    held = [(opt.state[p]["exp_avg"].data_ptr(), opt.state[p]["exp_avg_sq"].data_ptr()) for p in ps]
    ps_r, ref = _make(True, False)
    _steps(ref, ps_r, 0, 3)
    for p, q in zip(ps, ps_r):
        p.data.copy_(q)
    opt.load_state_dict(_saved(ref))
    assert [(opt.state[p]["exp_avg"].data_ptr(), opt.state[p]["exp_avg_sq"].data_ptr()) for p in ps] == held
    assert float(opt.state[ps[0]]["step"]) == 3.0
    for it in range(3, 5):
        gen = torch.Generator().manual_seed(1000 + it)
        for g in grads:
            g.copy_((torch.randn(g.shape, generator=gen) * 10.0 ** (it % 3 - 1)).to(DEV))
        graph.replay()
        _steps(ref, ps_r, it, 1)
    for p, q in zip(ps, ps_r):
        assert torch.equal(p, q), float((p - q).abs().max())
    assert float(opt.state[ps[0]]["step"]) == 5.0


def test_fused_adam_checkpoint_gives_torch_one_step_tensor_per_parameter():
    """A capturable FusedAdam keeps every parameter's step as a view of one counter; its state_dict() must not hand those
    views out: torch's Adam loading them would share one step tensor and advance it once per parameter per step()."""
    ps, opt = _make(True, False)
    _steps(opt, ps, 0, 5)
    for sd in (opt.state_dict(), _saved(opt)):
        qs, ref = _make(True, False, cls=None)
        ref.load_state_dict(sd)
        _steps(ref, qs, 5, 1)
        assert [float(ref.state[q]["step"]) for q in qs] == [6.0] * len(qs)
    assert [float(opt.state[p]["step"]) for p in ps] == [5.0] * len(ps)
