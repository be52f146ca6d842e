"""The four kernels of csrc/attn_head.hip alone against the fp64 restatement of tests/attn_head_ref.py, and the head
Function captured in a graph.

Every operand is a view into a larger NaN-filled buffer, starting on an odd 4-byte word, with NaN directly behind its last
element; with a row pitch Tp > T the pad columns of the input `p` are NaN as well: a read outside an operand, or of a pad
column, turns a sum into NaN.  Outputs are NaN-filled views whose guard bands must still be NaN afterwards while every element
of the output itself - the zero pad columns (and pad rows) of `dp` and `xm` included - must have been written.

Inputs (attn_head_ref.pool_inputs): logits 1.5 N(0, 1) clamped to |q| <= 12 with 5 % replaced by +-(20 + 10 U), so that both
clamp bounds are hit in the forward and in the backward and no logit lies where fp32 and fp64 put the sigmoid on different
sides of a bound; bias 0.3 N, head_w 0.1 + U, g N(0, 1); one case runs without a bias.

Bar: rel-L2 <= 2e-5 per output tensor, the project's per-op bar.  The reference's own fp32 torch composition lies at
0.2-1.8e-7 against fp64 on these inputs for out, dp, dbias and dhead_w, so the bar leaves two orders of magnitude to any
sane summation order, and an indexing or divisor error lies above 1e-3.  The composition's error is printed beside the
kernel's.  out, xm, dy and dp must be bit-equal across two calls."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, ops  # noqa: E402
from efficientat_amd.mn_train import AttentionPoolHead  # noqa: E402
from tests import attn_head_ref as R  # noqa: E402

DEV = torch.device("cuda:0")
BAR = 2e-5
GUARD = 67            # odd: the view behind it starts on an odd word
NAN = float("nan")

POOL_SHAPES = [(1, 1, 1, 1), (2, 3, 50, 7), (3, 4, 527, 32), (2, 4, 10, 33), (2, 4, 10, 100), (1, 2, 64, 4), (5, 4, 200, 10),
               (64, 4, 527, 32)]
POOL_CASES = [(s, ops.pitch4(s[3])) for s in POOL_SHAPES] + [((3, 4, 527, 32), 36)]
MEAN_SHAPES = [(1, 4, 1, 1), (2, 8, 2, 7), (3, 96, 4, 32), (2, 16, 3, 33), (1, 960, 4, 32)]


def _guarded(x, word=1):
    """x (CPU fp32 tensor) as a device view that starts `word` 4-byte words into a NaN buffer, NaN right behind it."""
    n = x.numel()
    buf = torch.full((word + n + GUARD,), NAN, device=DEV, dtype=torch.float32)
    view = buf[word:word + n].view(x.shape)
    view.copy_(x)
    assert view.data_ptr() % 16 == (4 * word) % 16 and bool(torch.isnan(buf[word + n:]).all())
    return view


class _Out:
    """A NaN-filled output view between two NaN guard bands."""

    def __init__(self, *shape):
        n = int(np.prod(shape))
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), NAN, device=DEV, dtype=torch.float32)
        self.view = self.buf[GUARD:GUARD + n].view(shape)

    def check(self, name):
        assert bool(torch.isnan(self.buf[:GUARD]).all()) and bool(torch.isnan(self.buf[GUARD + self.n:]).all()), \
            f"a guard band of {name} was written"
        assert not bool(torch.isnan(self.view).any()), f"an element of {name} was not written, or a sum read outside its operand"
        return self.view.clone()


def _rel(got, ref):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


def _composition_fp32(p, bias, head_w, g, H):
    """The reference's torch composition (attention_pooling.py:41-56) in fp32 on the CPU, with autograd: out, dp, dbias, dhead_w."""
    B, N, T = p.shape
    K = N // (2 * H)
    p = p.clone().requires_grad_(True)
    b = (bias if bias is not None else torch.zeros(N)).clone().requires_grad_(True)
    hw = head_w.clone().view(1, H, 1).requires_grad_(True)
    q = (p + b.view(1, N, 1)).transpose(1, 2).reshape(B, T, 2, H, K).permute(2, 0, 3, 1, 4)
    att, val = torch.clamp(torch.sigmoid(q[0]), 1e-7, 1.0 - 1e-7), q[1]
    att = att / att.sum(dim=2, keepdim=True)
    out = ((att * val).sum(dim=2) * hw).sum(dim=1)
    dp, db, dhw = torch.autograd.grad(out, (p, b, hw), g)
    return out.detach(), dp, db, dhw.reshape(-1)


_REFS = {}


def _pool_case(shape, with_bias):
    """Inputs and fp64 references of one shape: computed once, shared by the pitches of that shape, never modified."""
    key = (shape, with_bias)
    if key not in _REFS:
        B, H, K, T = shape
        p, bias, hw, g = R.pool_inputs(B, H, K, T, seed=1000 * K + T, with_bias=with_bias)
        out, o, s = R.attn_pool(p, bias, hw, H)
        dp, db, dhw = R.attn_pool_bwd(g, p, bias, hw, H)
        comp = _composition_fp32(p, bias, hw, g, H)
        cerr = [_rel(a, r) for a, r in zip(comp, (out, dp, db, dhw))]
        _REFS[key] = dict(p=p, bias=bias, hw=hw, g=g, out=out, o=o, s=s, dp=dp, db=db, dhw=dhw, cerr=cerr)
    return _REFS[key]


def _run_pool(c, shape, Tp, Np=None):
    """Forward + backward through the launchers on guarded operands -> dict of outputs (clones), guards checked."""
    B, H, K, T = shape
    N = 2 * H * K
    Np = N if Np is None else Np
    p = _guarded(R.pad(c["p"], Tp, NAN))
    bias = None if c["bias"] is None else _guarded(c["bias"])
    hw, g = _guarded(c["hw"]), _guarded(c["g"])
    out, o, s = _Out(B, K), _Out(B, H, K), _Out(B, H, K)
    r = ops.attn_pool(p, bias, hw, H, T, 1e-7, save=True, out=out.view, o=o.view, s=s.view)
    assert r[0] is out.view and r[1] is o.view and r[2] is s.view
    dp, db, dhw = _Out(B, Np, Tp), _Out(N), _Out(H)
    r = ops.attn_pool_bwd(g, p, bias, hw, o.view, s.view, H, T, 1e-7, Np=Np, dp=dp.view,
                          dbias=db.view if bias is not None else None, dhead_w=dhw.view)
    assert r[0] is dp.view and r[2] is dhw.view and (r[1] is db.view if bias is not None else r[1] is None)
    torch.cuda.synchronize()
    res = dict(out=out.check("out"), o=o.check("o"), s=s.check("s"), dp=dp.check("dp"), dhw=dhw.check("dhead_w"))
    if bias is not None:
        res["db"] = db.check("dbias")
    else:
        assert bool(torch.isnan(db.buf).all()), "dbias was written without a bias"
    return res


@pytest.mark.parametrize("shape,Tp", POOL_CASES, ids=[f"{'x'.join(map(str, s))}-Tp{tp}" for s, tp in POOL_CASES])
def test_pool_forward_and_backward(shape, Tp):
    B, H, K, T = shape
    N = 2 * H * K
    with_bias = shape != (2, 3, 50, 7)                      # one case has bias = NULL
    c = _pool_case(shape, with_bias)
    a, b = _run_pool(c, shape, Tp), _run_pool(c, shape, Tp)
    for k in ("out", "o", "s", "dp"):
        assert torch.equal(a[k], b[k]), f"{k} differs between two calls"
    assert bool((a["dp"][:, :, T:] == 0).all()), "pad columns of dp must be written as zeros"
    errs = {"out": _rel(a["out"], c["out"]), "o": _rel(a["o"], c["o"]), "s": _rel(a["s"], c["s"]),
            "dp": _rel(a["dp"][:, :, :T], c["dp"]), "dhead_w": _rel(a["dhw"], c["dhw"])}
    if with_bias:
        errs["dbias"] = _rel(a["db"], c["db"])
    names = ("out", "dp", "dbias", "dhead_w")
    print(f"ATTK pool {shape} Tp={Tp}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()) + " | fp32 torch composition: "
          + ", ".join(f"{k} {v:.2e}" for k, v in zip(names, c["cerr"])) + f" (bar {BAR:.0e})")
    q = c["p"].double()[:, :H * K] + (c["bias"].double()[:H * K].view(1, -1, 1) if with_bias else 0.0)
    if B * H * K * T >= 1000:
        assert bool((q > 16.2).any()) and bool((q < -16.2).any()), "both clamp bounds must be hit"
    for k, v in errs.items():
        assert v <= BAR, (k, v)


def test_pool_backward_writes_zero_pad_rows():
    """dp with more rows per sample than 2 H K (the data-gradient GEMM wants a multiple of 4): rows [N, Np) are zeros."""
    for shape, Np in (((1, 1, 1, 1), 4), ((3, 1, 5, 7), 12), ((2, 3, 3, 33), 20)):
        B, H, K, T = shape
        N, Tp = 2 * H * K, ops.pitch4(T)
        c = _pool_case(shape, True)
        a = _run_pool(c, shape, Tp, Np=Np)
        assert bool((a["dp"][:, N:] == 0).all()) and bool((a["dp"][:, :, T:] == 0).all())
        assert _rel(a["dp"][:, :N, :T], c["dp"]) <= BAR and _rel(a["db"], c["db"]) <= BAR and _rel(a["dhw"], c["dhw"]) <= BAR


@pytest.mark.parametrize("shape", MEAN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_frequency_mean_forward_and_backward(shape):
    B, C, F, T = shape
    rng = np.random.default_rng(C * 100 + T)
    y = torch.from_numpy((0.75 + rng.standard_normal(shape) + 0.05 * np.arange(T)).astype(np.float32))
    for Tp in sorted({ops.pitch4(T), T, T + 5}):
        dxm = torch.from_numpy(rng.standard_normal((B, C, T)).astype(np.float32))
        res = []
        for _ in range(2):
            xm, dy = _Out(B, C, Tp), _Out(B, C, F, T)
            assert ops.freq_mean(_guarded(y), Tp, out=xm.view) is xm.view
            assert ops.freq_mean_bwd(_guarded(R.pad(dxm, Tp, NAN)), F, T, out=dy.view) is dy.view
            torch.cuda.synchronize()
            res.append((xm.check("xm"), dy.check("dy")))
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
        xm, dy = res[0]
        assert bool((xm[:, :, T:] == 0).all()), "pad columns of xm must be written as zeros"
        e1, e2 = _rel(xm[:, :, :T], R.freq_mean(y)), _rel(dy, R.freq_mean_bwd(dxm, F))
        print(f"ATTK mean {shape} Tp={Tp}: xm {e1:.2e}, dy {e2:.2e} (bar {BAR:.0e})")
        assert e1 <= BAR and e2 <= BAR


def test_c_abi_refuses_bad_arguments():
    x = torch.zeros(64, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    p = x.data_ptr()
    with pytest.raises(_lib.EatHipError, match="Tp=3 is shorter than T=4"):
        _lib.call("eat_freq_mean_fwd", p, p, 1, 1, 1, 4, 3, st)
    with pytest.raises(_lib.EatHipError, match="missing operand"):
        _lib.call("eat_freq_mean_bwd", None, p, 1, 1, 1, 4, 4, st)
    with pytest.raises(_lib.EatHipError, match="need B, H, K, T >= 1"):
        _lib.call("eat_attn_pool_fwd", p, None, p, 1e-7, p, None, None, 1, 0, 1, 4, 4, st)
    with pytest.raises(_lib.EatHipError, match="eps=0.7 lies outside"):
        _lib.call("eat_attn_pool_fwd", p, None, p, 0.7, p, None, None, 1, 1, 1, 4, 4, st)
    with pytest.raises(_lib.EatHipError, match="only bias and dbias are optional"):
        _lib.call("eat_attn_pool_bwd", p, p, None, p, 1e-7, p, p, p, None, p, None, 1, 1, 1, 4, 4, 2, st)
    with pytest.raises(_lib.EatHipError, match="Np=1 rows per sample"):
        _lib.call("eat_attn_pool_bwd", p, p, None, p, 1e-7, p, p, p, None, p, p, 1, 1, 1, 4, 4, 1, st)
    torch.cuda.synchronize()


def _head_inputs(B, C, F, T, H, K, seed):
    g = torch.Generator().manual_seed(seed)
    N = 2 * H * K
    y = torch.randn(B, C, F, T, generator=g)
    w = torch.randn(N, C, generator=g) * 0.5
    w[:H * K] *= 3.0
    b = torch.randn(N, generator=g) * 0.3
    hw = 0.1 + torch.rand(1, H, 1, generator=g)
    go = torch.randn(B, K, generator=g)
    return y, w, b, hw, go


@pytest.mark.parametrize("geo", [(3, 16, 2, 10, 4, 5), (2, 8, 3, 5, 1, 3)], ids=["T10-N40", "T5-N6-padded-rows"])
def test_head_function_against_fp64_and_captured_in_a_graph(geo):
    """AttentionPoolHead forward + backward on static buffers, captured in `torch.cuda.graph` on one stream; two replays with
    different buffer contents against the eager result on the same contents (bit-equal for out and dy, which have no
    cross-block accumulation; the parameter gradients within the bar) and against the fp64 head."""
    B, C, F, T, H, K = geo
    sets = [_head_inputs(B, C, F, T, H, K, seed) for seed in (5, 6, 7)]
    y, w, b, hw, go = (t.clone().to(DEV) for t in sets[0])
    for t in (y, w, b, hw):
        t.requires_grad_(True)

    def step():
        out = AttentionPoolHead.apply(y, w, b, hw, H, 1e-7)
        return (out,) + torch.autograd.grad(out, (y, w, b, hw), go)

    with ops.precision("fp32"):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static = step()
        for vals in sets[1:]:
            with torch.no_grad():
                for dst, src in zip((y, w, b, hw, go), vals):
                    dst.copy_(src)
            graph.replay()
            torch.cuda.synchronize()
            got = [t.clone() for t in static]
            eager = step()
            torch.cuda.synchronize()
            assert torch.equal(got[0], eager[0]), "out: replay and eager differ"
            assert torch.equal(got[1], eager[1]), "dy: replay and eager differ"
            ref = (R.head(*vals[:4], H),) + R.head_bwd(vals[4], *vals[:4], H)
            for name, a, e, r in zip(("out", "dy", "dw", "db", "dhead_w"), got, eager, ref):
                r = r.reshape(a.shape)
                print(f"ATTK head {geo} {name}: replay {_rel(a, r):.2e}, eager {_rel(e, r):.2e} (bar {BAR:.0e})")
                assert _rel(a, r) <= BAR and _rel(e, r) <= BAR, name
