"""The kernels of csrc/sed.hip alone against the restatements of tests/sed_ref.py, and `mn_train.FrameHead` against fp64
autograd of the same maths.

Every operand is a view into a larger poisoned buffer (NaN for floats, a huge negative number for integer tables) that
starts on an odd 4-byte word; outputs are NaN-filled views between NaN guard bands that must still be NaN afterwards while
every element of the output itself, pads included, must have been written (`_guarded` / `_Out` as in
test_gpu_attn_head_kernels.py).

eat_sed_targets: exact equality with the brute-force rasteriser, which enumerates every output sample.
eat_frame_bce_fwd_bwd, eat_frame_grad_pad, eat_frame_hidden_fwd / _bwd: rel-L2 <= 2e-5 against fp64, the project's bar for
fp32-stored, fp64-inside kernels; pads bitwise 0; two calls bit-identical; counts exact.
FrameHead: under `ops.precision("fp32")` the same 2e-5 (the bar test_head_function_against_fp64_and_captured_in_a_graph holds
`AttentionPoolHead` to on the same conv kernels).  The other modes have no bar there; theirs follow from the formats: a
split-operand product (bf16x3, and 'auto' from C_in = 40) keeps 16 mantissa bits per operand and drops the lo x lo term,
<= 2^-16 + 2 x 2^-17 = 3.1e-5 relative per product, and the longest chain (dy) passes four GEMMs: 1.25e-4.  Plain bf16 rounds
both operands to 8 bits, <= 2 x 2^-9 = 3.9e-3 per product, four GEMMs: 1.6e-2."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, ops  # noqa: E402
from efficientat_amd.mn_train import FrameHead  # noqa: E402
from tests import sed_ref as R  # noqa: E402

DEV = torch.device("cuda:0")
BAR = 2e-5
HEAD_BARS = {"fp32": BAR, "auto": 1.25e-4, "bf16x3": 1.25e-4, "bf16": 1.6e-2}
GUARD = 67
NAN = float("nan")
POISON = -(2 ** 30)


def _guarded(x, word=1):
    """x (CPU tensor) as a device view that starts `word` words into a poisoned buffer, poison right behind it."""
    x = torch.as_tensor(x)
    n = x.numel()
    fill = NAN if x.is_floating_point() else POISON
    buf = torch.full((word + n + GUARD,), fill, device=DEV, dtype=x.dtype)
    view = buf[word:word + n].view(x.shape)
    view.copy_(x)
    return view


class _Out:
    """A NaN-filled fp32 output view between two NaN guard bands (int64: the poison value)."""

    def __init__(self, *shape, dtype=torch.float32, fill=NAN):
        n = int(np.prod(shape))
        self.n, self.fill = n, fill
        self.buf = torch.full((GUARD + n + GUARD,), fill, device=DEV, dtype=dtype)
        self.view = self.buf[GUARD:GUARD + n].view(shape)

    def _is_fill(self, t):
        return torch.isnan(t) if self.fill != self.fill else t == self.fill

    def check(self, name, nan_ok=False):
        assert bool(self._is_fill(self.buf[:GUARD]).all()) and bool(self._is_fill(self.buf[GUARD + self.n:]).all()), \
            f"a guard band of {name} was written"
        if not nan_ok:
            assert not bool(self._is_fill(self.view).any()), f"an element of {name} was not written, or a sum read outside"
        return self.view.clone()


def _rel(got, ref):
    got = torch.as_tensor(got).detach().cpu().double().flatten()
    ref = torch.as_tensor(ref).detach().cpu().double().flatten()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


# ---------------------------------------------------------------------------------------------------- eat_sed_targets
CASES = R.target_cases()
_BRUTE = {}


def _brute(case):
    if case["name"] not in _BRUTE:
        _BRUTE[case["name"]] = R.targets_brute(*R.case_args(case))
    return _BRUTE[case["name"]]


def _target_operands(c):
    bank = dict(events=_guarded(torch.from_numpy(c["events"])), event_offsets=_guarded(torch.from_numpy(c["eo"]), word=2),
                lengths=_guarded(torch.from_numpy(c["lengths"].astype(np.int32))), classes=[str(k) for k in range(c["K"])])
    tables = [_guarded(torch.from_numpy(c[k])) for k in ("idx", "start", "shift", "mix")]
    return bank, tables


def _run_targets(c, bank, tables):
    out = _Out(len(c["mix"]), c["K"], c["Tp"])
    r = ops.sed_targets(bank, *tables, c["L"], c["R"], c["T"], c["Tp"], out=out.view)
    assert r.data_ptr() == out.view.data_ptr()
    torch.cuda.synchronize()
    y = out.check("y", nan_ok=True)
    return y


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_targets_equal_the_brute_force_reference(case):
    ref = _brute(case)
    bank, tables = _target_operands(case)
    y = _run_targets(case, bank, tables)
    got = y.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "NaN rows differ"
    assert np.array_equal(got, ref, equal_nan=True), f"{int((got != ref).sum() - np.isnan(ref).sum())} elements differ"
    assert torch.equal(y.view(torch.int32), _run_targets(case, bank, tables).view(torch.int32)), "two calls differ"


def test_targets_replayed_from_a_graph_equal_the_eager_result():
    case = CASES[3]                                                          # wave-mixed rows, a crop, 0.3f
    bank, tables = _target_operands(case)
    out = torch.full((len(case["mix"]), case["K"], case["Tp"]), NAN, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.sed_targets(bank, *tables, case["L"], case["R"], case["T"], case["Tp"], out=out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.sed_targets(bank, *tables, case["L"], case["R"], case["T"], case["Tp"], out=out)
    out.fill_(NAN)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), _brute(case), equal_nan=True)


# ---------------------------------------------------------------------------------------------------- eat_frame_bce_fwd_bwd
BCE_SHAPES = [(1, 1, 1, 4, 4), (2, 5, 7, 8, 8), (3, 527, 32, 32, 528), (2, 10, 33, 36, 12), (64, 527, 32, 32, 528)]
_BCE = {}


def _bce_case(shape):
    """Logits 4 N(0, 1) with 5 % at +-(25 .. 30) and the corners at +-30; targets of density 0.1, a tenth of them soft (0.3f,
    0.5: wave-mixed frames).  Pad columns of z and y are NaN: a read of one turns a sum into NaN."""
    if shape not in _BCE:
        B, K, T, Tp, Kp = shape
        g = torch.Generator().manual_seed(100 * K + T)
        z = 4.0 * torch.randn(B, K, Tp, generator=g)
        big = torch.rand(B, K, Tp, generator=g) < 0.05
        z = torch.where(big, torch.sign(z) * (25.0 + 5.0 * torch.rand(B, K, Tp, generator=g)), z).clamp(-30.0, 30.0)
        z[0, 0, 0], z[-1, -1, T - 1] = 30.0, -30.0
        u = torch.rand(B, K, Tp, generator=g)
        y = (u < 0.1).float()
        y = torch.where(u < 0.005, torch.full_like(y, 0.5), torch.where(u < 0.01, torch.full_like(y, float(np.float32(0.3))), y))
        z[:, :, T:], y[:, :, T:] = NAN, NAN
        perm = torch.randperm(B, generator=g).to(torch.int32)
        lam = torch.rand(B, generator=g) * 0.5 + 0.5
        nf = torch.randint(0, T + 1, (B,), generator=g).to(torch.int32)
        nf[0] = 0 if B > 1 else T                                           # a row without frames
        if B > 1:
            nf[1] = T
        _BCE[shape] = dict(z=z, y=y, perm=perm, lam=lam, nf=nf)
    return _BCE[shape]


def _run_bce(shape, c, perm, nframes, want_counts=False, thr=None, sums=None, nan_ok=False):
    B, K, T, Tp, Kp = shape
    z, y = _guarded(c["z"]), _guarded(c["y"])
    p = _guarded(c["perm"]) if perm else None
    l = _guarded(c["lam"]) if perm else None
    nf = None if nframes is None else _guarded(nframes)
    sums = torch.zeros(1, device=DEV) if sums is None else sums
    dl, db = _Out(B, Kp, Tp), _Out(K)
    rows = _Out(B * T, K)
    counts = _Out(K, 3, dtype=torch.int64, fill=POISON) if want_counts else None
    if counts is not None:
        counts.view.zero_()                                                  # (the kernel adds to them)
    ws = torch.empty(K + 1, device=DEV, dtype=torch.float64)
    _lib.call("eat_frame_bce_fwd_bwd", z.data_ptr(), y.data_ptr(), None if p is None else p.data_ptr(),
              None if l is None else l.data_ptr(), None if nf is None else nf.data_ptr(),
              None if thr is None else thr.data_ptr(), B, K, T, Tp, Kp, sums.data_ptr(), dl.view.data_ptr(), db.view.data_ptr(),
              None if counts is None else counts.view.data_ptr(), rows.view.data_ptr(), ws.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dict(loss=sums.clone(), dl=dl.check("dlogits", nan_ok), db=db.check("dbias", nan_ok), rows=rows.check("rows"),
                counts=None if counts is None else counts.check("counts", nan_ok=True))


@pytest.mark.parametrize("nframes", ["all", "ragged", "none"])
@pytest.mark.parametrize("perm", [False, True], ids=["plain", "mixup"])
@pytest.mark.parametrize("shape", BCE_SHAPES, ids=["x".join(map(str, s)) for s in BCE_SHAPES])
def test_frame_bce_against_fp64(shape, perm, nframes):
    B, K, T, Tp, Kp = shape
    c = _bce_case(shape)
    nf = {"all": None, "ragged": c["nf"], "none": torch.zeros(B, dtype=torch.int32)}[nframes]
    zn, yn = np.nan_to_num(c["z"].numpy()), np.nan_to_num(c["y"].numpy())
    loss, dl, db = R.frame_bce(zn, yn, T, Kp, c["perm"].numpy() if perm else None, c["lam"].numpy() if perm else None,
                               None if nf is None else nf.numpy())
    got = _run_bce(shape, c, perm, nf)
    again = _run_bce(shape, c, perm, nf, sums=got["loss"].clone())
    for k in ("dl", "db", "rows"):
        assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), f"{k}: two calls differ"
    nb = np.full(B, T) if nf is None else nf.numpy()
    M = K * int(nb.sum())
    g_dl = got["dl"].cpu()
    assert not bool(g_dl[:, K:].view(torch.int32).any()), "pad rows of dlogits are not bitwise 0"
    for b in range(B):
        assert not bool(g_dl[b, :, int(nb[b]):].view(torch.int32).any()), "columns [n_b, Tp) of dlogits are not bitwise 0"
    assert torch.equal(got["rows"].cpu().view(B, T, K).view(torch.int32),
                       c["z"][:, :, :T].transpose(1, 2).contiguous().view(torch.int32)), "rows are not the transposed logits"
    if M == 0:
        assert got["loss"].item() == 0.0 and not bool(g_dl.view(torch.int32).any()) and not bool(got["db"].cpu().view(torch.int32).any())
        return
    e_loss = abs(got["loss"].item() - loss) / abs(loss)
    e_sum = abs(again["loss"].item() - 2.0 * loss) / abs(2.0 * loss)
    e_dl, e_db = _rel(g_dl, dl), _rel(got["db"], db)
    print(f"SEDK bce {shape} perm={perm} nframes={nframes}: loss {e_loss:.2e}, two calls {e_sum:.2e}, dlogits {e_dl:.2e}, "
          f"dbias {e_db:.2e} (bar {BAR:.0e})")
    assert e_loss <= BAR and e_sum <= BAR and e_dl <= BAR and e_db <= BAR


@pytest.mark.parametrize("nframes", ["all", "ragged"])
@pytest.mark.parametrize("shape", BCE_SHAPES, ids=["x".join(map(str, s)) for s in BCE_SHAPES])
def test_frame_bce_counts_are_exact(shape, nframes):
    B, K, T, Tp, Kp = shape
    c = _bce_case(shape)
    nf = None if nframes == "all" else c["nf"]
    zn, yn = np.nan_to_num(c["z"].numpy()), np.nan_to_num(c["y"].numpy())
    thr, gap = R.midway_thresholds(zn, T)
    print(f"SEDK counts {shape}: smallest |s - thr| = {gap:.2e}")
    assert gap >= 1e-6, "a sigmoid value lies at its threshold: the comparison would be undefined across implementations"
    ref = R.frame_counts(zn, yn, thr, T, None if nf is None else nf.numpy())
    d_thr = _guarded(torch.from_numpy(thr))
    got = _run_bce(shape, c, False, nf, want_counts=True, thr=d_thr)["counts"].cpu().numpy()
    assert np.array_equal(got, ref)
    assert ref[:, 0].sum() + ref[:, 2].sum() > 0 or B * K * T < 8            # (the case has positives to count)


def test_frame_bce_bad_perm_poisons_its_row_only_and_counts_refuse_perm():
    shape = (3, 5, 7, 8, 8)
    B, K, T, Tp, Kp = shape
    c = {}
    g = torch.Generator().manual_seed(3)
    c["z"] = torch.randn(B, K, Tp, generator=g)
    c["y"] = (torch.rand(B, K, Tp, generator=g) < 0.3).float()
    c["perm"], c["lam"] = torch.tensor([2, 7, 0], dtype=torch.int32), torch.tensor([0.7, 0.6, 0.9])
    got = _run_bce(shape, c, True, None, nan_ok=True)
    dl = got["dl"].cpu()
    assert bool(torch.isnan(dl[1, :K, :T]).all()) and not bool(dl[1, K:].view(torch.int32).any()) and not bool(torch.isnan(dl[0]).any()) and not bool(torch.isnan(dl[2]).any())
    assert not bool(dl[1, :, T:].view(torch.int32).any()) and bool(torch.isnan(got["loss"]).all())
    ok = dict(c, perm=torch.tensor([2, 1, 0], dtype=torch.int32))
    _, ref, _ = R.frame_bce(c["z"].numpy(), c["y"].numpy(), T, Kp, ok["perm"].numpy(), c["lam"].numpy())
    assert _rel(dl[[0, 2]], ref[[0, 2]]) <= BAR                               # the other rows are what they were
    z = c["z"].to(DEV)
    with pytest.raises(_lib.EatHipError, match="perm given"):
        ops.frame_bce_fwd_bwd(z, c["y"].to(DEV), T, perm=c["perm"].to(DEV), lam=c["lam"].to(DEV),
                              counts=torch.zeros((K, 3), device=DEV, dtype=torch.int64), thr=torch.full((K,), 0.5, device=DEV))
    # every optional output may be left out
    dl2, db2 = ops.frame_bce_fwd_bwd(z, c["y"].to(DEV), T, grad=False)
    assert dl2 is None and db2 is None
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- grad_pad, hidden layer
HID_SHAPES = [(1, 1, 4, 1, 4), (2, 5, 8, 7, 8), (3, 1280, 1280, 32, 32), (2, 10, 12, 33, 36), (64, 1280, 1280, 32, 32)]


@pytest.mark.parametrize("keep", [False, True], ids=["nokeep", "keep"])
@pytest.mark.parametrize("shape", HID_SHAPES, ids=["x".join(map(str, s)) for s in HID_SHAPES])
def test_hidden_layer_forward_and_backward(shape, keep):
    """(B, H, Hp, T, Tp).  z1 holds the kinks -3 and 3 exactly and values either side; pad rows and columns of dh are NaN."""
    B, H, Hp, T, Tp = shape
    g = torch.Generator().manual_seed(7 * H + T)
    z1 = 2.5 * torch.randn(B, Hp, Tp, generator=g)
    z1.view(-1)[:6] = torch.tensor([-3.0, 3.0, -3.0000002, 3.0000002, -2.9999998, 2.9999998])[:min(6, z1.numel())]
    dh = torch.randn(B, Hp, Tp, generator=g)
    kp = None
    if keep:
        kp = (torch.rand(B, Hp, generator=g) < 0.8).float() / 0.8
    h = ops.frame_hidden_fwd(_guarded(z1), None if kp is None else _guarded(kp))
    torch.cuda.synchronize()
    assert _rel(h, R.hidden_fwd(z1.numpy(), None if kp is None else kp.numpy())) <= BAR
    dh_p = dh.clone()
    dh_p[:, H:], dh_p[:, :, T:] = NAN, NAN
    ref_dz, ref_db = R.hidden_bwd(dh.numpy(), z1.numpy(), None if kp is None else kp.numpy(), H, T)
    outs = []
    for _ in range(2):
        dz, db = ops.frame_hidden_bwd(_guarded(dh_p), _guarded(z1), None if kp is None else _guarded(kp), H, T)
        torch.cuda.synchronize()
        outs.append((dz.cpu(), db.cpu()))
    dz, db = outs[0]
    assert torch.equal(dz.view(torch.int32), outs[1][0].view(torch.int32)) and torch.equal(db.view(torch.int32), outs[1][1].view(torch.int32))
    assert not bool(dz[:, H:].view(torch.int32).any()) and not bool(dz[:, :, T:].view(torch.int32).any()), "pads of dz1 are not bitwise 0"
    e_dz, e_db = _rel(dz, ref_dz), _rel(db, ref_db)
    print(f"SEDK hidden {shape} keep={keep}: dz1 {e_dz:.2e}, db1 {e_db:.2e} (bar {BAR:.0e})")
    assert e_dz <= BAR and e_db <= BAR
    assert db.shape == (H,)


@pytest.mark.parametrize("shape", [(1, 1, 4, 1, 4), (2, 5, 8, 7, 8), (3, 527, 528, 32, 32), (2, 10, 12, 33, 36)],
                         ids=lambda s: "x".join(map(str, s)))
def test_grad_pad_re_establishes_the_pads_and_sums_the_bias(shape):
    """(B, K, Kp, T, Tp): the pad columns of g hold NaN, which must not reach dl or db."""
    B, K, Kp, T, Tp = shape
    g = torch.randn(B, K, Tp, generator=torch.Generator().manual_seed(K + T))
    gp = g.clone()
    gp[:, :, T:] = NAN
    out = _Out(B, Kp, Tp)
    dl, db = ops.frame_grad_pad(_guarded(gp), T, Kp, out=out.view)
    torch.cuda.synchronize()
    dl = out.check("dl").cpu()
    assert torch.equal(dl[:, :K, :T].contiguous().view(torch.int32), g[:, :, :T].contiguous().view(torch.int32))
    assert not bool(dl[:, K:].view(torch.int32).any()) and not bool(dl[:, :, T:].view(torch.int32).any())
    assert _rel(db, g[:, :, :T].double().sum(dim=(0, 2))) <= BAR


# ---------------------------------------------------------------------------------------------------- FrameHead
HEAD_GEOS = [(2, 16, 2, 7, 12, 5), (1, 8, 1, 1, 4, 1), (3, 960, 4, 32, 1280, 527)]
_HEAD = {}


def _head_case(geo, keep):
    """Inputs and the fp64 gradients of one geometry: computed once, shared by the precision modes, never modified.  The
    upstream gradient is random, with non-zero pad columns that must not reach any gradient."""
    key = (geo, keep)
    if key not in _HEAD:
        B, C, Fq, T, H, K = geo
        g = torch.Generator().manual_seed(C + T)
        y = torch.randn(B, C, Fq, T, generator=g)
        w1 = torch.randn(H, C, generator=g) * (2.0 / C ** 0.5)
        b1 = torch.randn(H, generator=g) * 0.5
        w2 = torch.randn(K, H, generator=g) * (1.0 / H ** 0.5)
        b2 = torch.randn(K, generator=g) * 0.3
        kp = (torch.rand(B, H, generator=g) < 0.8).float() / 0.8 if keep else None
        go = torch.randn(B, K, ops.pitch4(T), generator=g)
        ref = R.head_grads(y, w1, b1, w2, b2, kp, go[:, :, :T])
        _HEAD[key] = dict(ins=(y, w1, b1, w2, b2), keep=kp, go=go, ref=ref)
    return _HEAD[key]


def _head_step(ins, kp, go):
    z = FrameHead.apply(*ins, kp)
    return (z,) + torch.autograd.grad(z, ins, go)


@pytest.mark.parametrize("mode", ["fp32", "auto", "bf16x3", "bf16"])
@pytest.mark.parametrize("keep", [False, True], ids=["nokeep", "keep"])
@pytest.mark.parametrize("geo", HEAD_GEOS, ids=["x".join(map(str, g)) for g in HEAD_GEOS])
def test_frame_head_against_fp64_autograd(geo, keep, mode):
    B, C, Fq, T, H, K = geo
    c = _head_case(geo, keep)
    ins = [t.clone().to(DEV).requires_grad_(True) for t in c["ins"]]
    kp = None if c["keep"] is None else c["keep"].to(DEV)
    with ops.precision(mode):
        got = _head_step(ins, kp, c["go"].to(DEV))
    torch.cuda.synchronize()
    assert got[0].shape == (B, K, ops.pitch4(T))
    bar = HEAD_BARS[mode]
    for name, a, r in zip(("logits", "dy", "dw1", "db1", "dw2", "db2"), (got[0][:, :, :T],) + got[1:], c["ref"]):
        e = _rel(a, r.reshape(a.shape))
        print(f"SEDK head {geo} keep={keep} {mode}: {name} {e:.2e} (bar {bar:.1e})")
        assert e <= bar, (name, e, bar)


def test_frame_head_captured_and_replayed_with_equal_bits():
    geo = HEAD_GEOS[0]
    c0, c1 = _head_case(geo, True), _head_case((2, 16, 2, 7, 12, 5), False)
    ins = [t.clone().to(DEV).requires_grad_(True) for t in c0["ins"]]
    kp, go = c0["keep"].to(DEV), c0["go"].to(DEV)
    with ops.precision("fp32"):
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                _head_step(ins, kp, go)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static = _head_step(ins, kp, go)
        with torch.no_grad():
            ins[0].copy_(c1["ins"][0] * 0.5 + 0.25)                           # other contents in the static buffers
            go.copy_(c1["go"].flip(0))
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in static]
        eager = _head_step(ins, kp, go)
        torch.cuda.synchronize()
    for name, a, e in zip(("logits", "dy", "dw1", "db1", "dw2", "db2"), got, eager):
        if name in ("dw1", "dw2"):                                            # (the weight-gradient kernels may add across blocks)
            assert _rel(a, e) <= BAR, name
        else:
            assert torch.equal(a, e), f"{name}: replay and eager differ"
