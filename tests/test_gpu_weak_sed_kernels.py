"""The kernels of csrc/weak_sed.hip alone against the restatements of tests/weak_sed_ref.py.

Every operand is a view into a larger poisoned buffer (NaN for floats, a huge negative number for integer tables, 0xFF for
the strong bytes) that starts on an odd 4-byte word; outputs are NaN-filled views between NaN guard bands that must still
be NaN afterwards while every element of the output itself, pads included, must have been written (`_guarded` / `_Out` as in
test_gpu_sed_kernels.py).

eat_sed_clip_targets: exact equality with the brute force, which enumerates the samples of every crop window.
eat_weak_frame_bce_fwd_bwd: rel-L2 <= 2e-5 against the fp64 closed form, the project's bar for fp32-stored, fp64-inside
kernels (BAR of test_gpu_sed_kernels.py); pads bitwise 0; two calls bit-identical."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, ops  # noqa: E402
from tests import sed_ref as R  # noqa: E402
from tests import weak_sed_ref as W  # noqa: E402

DEV = torch.device("cuda:0")
BAR = 2e-5
GUARD = 67
NAN = float("nan")
POISON = -(2 ** 30)


def _guarded(x, word=1):
    """x (CPU tensor) as a device view that starts `word` words into a poisoned buffer, poison right behind it."""
    x = torch.as_tensor(x)
    n = x.numel()
    fill = NAN if x.is_floating_point() else (255 if x.dtype == torch.uint8 else POISON)
    buf = torch.full((word + n + GUARD,), fill, device=DEV, dtype=x.dtype)
    view = buf[word:word + n].view(x.shape)
    view.copy_(x)
    return view


class _Out:
    """A NaN-filled fp32 output view between two NaN guard bands (int32: the poison value)."""

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


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------- eat_sed_clip_targets
CASES = R.target_cases()
_BRUTE = {}


def _brute(case, kind):
    """(w, framed): the targets are enumerated once per case, the flags per `strong` operand."""
    if case["name"] not in _BRUTE:
        _BRUTE[case["name"]] = W.clip_targets_brute(case["events"], case["eo"], case["lengths"], case["K"], case["idx"],
                                                    case["start"], case["mix"], case["L"])[0]
    strong = W.strong_vectors(len(case["lengths"]))[kind]
    return _BRUTE[case["name"]], W.framed_brute(case["lengths"], case["idx"], case["start"], strong)


def _target_operands(c, kind):
    strong = W.strong_vectors(len(c["lengths"]))[kind]
    bank = dict(events=_guarded(torch.from_numpy(c["events"])), event_offsets=_guarded(torch.from_numpy(c["eo"]), word=2),
                lengths=_guarded(torch.from_numpy(c["lengths"].astype(np.int32))), classes=[str(k) for k in range(c["K"])])
    if strong is not None:
        bank["strong"] = _guarded(torch.from_numpy(strong), word=3)
    tables = [_guarded(torch.from_numpy(c[k])) for k in ("idx", "start", "mix")]
    return bank, tables


def _run_clip_targets(c, bank, tables):
    B = len(c["mix"])
    w, fr = _Out(B, c["K"]), _Out(B, dtype=torch.int32, fill=POISON)
    r = ops.sed_clip_targets(bank, *tables, c["L"], out=w.view, framed_out=fr.view)
    assert r[0].data_ptr() == w.view.data_ptr() and r[1].data_ptr() == fr.view.data_ptr()
    torch.cuda.synchronize()
    return w.check("w", nan_ok=True), fr.check("framed")


@pytest.mark.parametrize("kind", ["mixed", "ones", "null"])
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_clip_targets_equal_the_brute_force_reference(case, kind):
    ref_w, ref_f = _brute(case, kind)
    bank, tables = _target_operands(case, kind)
    w, fr = _run_clip_targets(case, bank, tables)
    got = w.cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(ref_w)), "NaN rows differ"
    assert np.array_equal(got, ref_w, equal_nan=True), f"{int((got != ref_w).sum() - np.isnan(ref_w).sum())} elements differ"
    assert np.array_equal(fr.cpu().numpy(), ref_f)
    w2, fr2 = _run_clip_targets(case, bank, tables)
    assert torch.equal(_bits(w), _bits(w2)) and torch.equal(fr, fr2), "two calls differ"
    # against the strong-label kernel: NaN rows (and framed = 0) exactly where it makes NaN rows; where the frames cover the
    # window, an unmixed sample's clip target is the maximum of its frame targets
    shift = _guarded(torch.from_numpy(case["shift"]))
    y = ops.sed_targets(bank, tables[0], tables[1], shift, tables[2], case["L"], case["R"], case["T"], case["Tp"])
    torch.cuda.synchronize()
    y = y.cpu().numpy()[:, :, :case["T"]]
    nan_rows = np.isnan(y).any(axis=(1, 2))
    assert np.array_equal(nan_rows, np.isnan(got).all(axis=1)) and np.array_equal(nan_rows, np.isnan(got).any(axis=1))
    assert not fr.cpu().numpy()[nan_rows].any()
    if case["T"] * case["R"] >= case["L"]:
        plain = (case["idx"][1::2] == -1) & ~nan_rows
        assert np.array_equal(got[plain], y[plain].max(axis=2))


def test_clip_targets_replayed_from_a_graph_equal_the_eager_result():
    case = CASES[3]                                                          # wave-mixed rows, a crop, 0.3f
    bank, tables = _target_operands(case, "mixed")
    B = len(case["mix"])
    w = torch.full((B, case["K"]), NAN, device=DEV)
    fr = torch.full((B,), POISON, device=DEV, dtype=torch.int32)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.sed_clip_targets(bank, *tables, case["L"], out=w, framed_out=fr)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.sed_clip_targets(bank, *tables, case["L"], out=w, framed_out=fr)
    w.fill_(NAN)
    fr.fill_(POISON)
    graph.replay()
    torch.cuda.synchronize()
    ref_w, ref_f = _brute(case, "mixed")
    assert np.array_equal(w.cpu().numpy(), ref_w, equal_nan=True) and np.array_equal(fr.cpu().numpy(), ref_f)


# ---------------------------------------------------------------------------------------------------- the fused loss
# (B, K, T, Tp, Kp): the smallest shapes at which each mechanism can fail.  A row is walked by a group of 32 lanes for
# T <= 32 and of 64 above, in strides of the group: 32 | 33 and 63 | 64 | 65 lie either side of both; 257 is past one
# block's span; B = 9 at T <= 32 is more rows than a block has groups (8), B = 5 at T = 33 more than it has waves (4).
SHAPES = [(1, 1, 1, 1, 1), (1, 1, 1, 4, 1), (2, 3, 3, 3, 3), (2, 3, 3, 4, 4), (3, 2, 63, 64, 4), (3, 2, 64, 64, 2),
          (2, 2, 65, 68, 4), (5, 3, 32, 32, 4), (5, 2, 33, 36, 2), (9, 1, 5, 8, 1), (2, 1, 257, 260, 1)]
FLAGS = ["all", "none", "mixed", "cross"]
_LOSS = {}


def _loss_case(shape):
    """Logits uniform in [-8, 8] (P stays inside (eps, 1 - eps)); frame targets of density 0.2, a tenth of them soft; clip
    targets 0 / 1 / soft.  Pad columns of z and y are NaN: a read of one turns a sum into NaN."""
    if shape not in _LOSS:
        B, K, T, Tp, Kp = shape
        g = torch.Generator().manual_seed(1000 * B + 10 * K + T)
        z = 16.0 * torch.rand(B, K, Tp, generator=g) - 8.0
        u = torch.rand(B, K, Tp, generator=g)
        y = (u < 0.2).float()
        y = torch.where(u < 0.01, torch.full_like(y, 0.5), torch.where(u < 0.02, torch.full_like(y, float(np.float32(0.3))), y))
        z[:, :, T:], y[:, :, T:] = NAN, NAN
        v = torch.rand(B, K, generator=g)
        w = torch.where(v < 0.1, torch.full_like(v, float(np.float32(0.3))), (v < 0.5).float())
        perm = ((torch.arange(B) + 1) % B).to(torch.int32)                   # a rotation: row b pairs with b + 1
        lam = torch.rand(B, generator=g) * 0.5 + 0.5
        _LOSS[shape] = dict(z=z, y=y, w=w, perm=perm, lam=lam)
    return _LOSS[shape]


def _flags(kind, B):
    if kind == "all":
        return torch.ones(B, dtype=torch.int32)
    if kind == "none":
        return torch.zeros(B, dtype=torch.int32)
    f = (torch.arange(B) % 2 == 0).to(torch.int32) * 7                        # mixed (any non-zero value counts); with the
    return f                                                                  # rotation, a framed row meets an unframed one


def _run_loss(shape, c, framed, perm, ww, eps=1e-7, sums=None, nan_ok=False):
    B, K, T, Tp, Kp = shape
    z, y, w, fr = _guarded(c["z"]), _guarded(c["y"]), _guarded(c["w"]), _guarded(framed)
    p = _guarded(c["perm"]) if perm else None
    l = _guarded(c["lam"]) if perm else None
    sums = torch.zeros(3, device=DEV) if sums is None else sums
    dl, db, cp = _Out(B, Kp, Tp), _Out(K), _Out(B, K)
    ws = torch.full((2 * K + 1 + GUARD,), NAN, device=DEV, dtype=torch.float64)
    _lib.call("eat_weak_frame_bce_fwd_bwd", z.data_ptr(), y.data_ptr(), w.data_ptr(), fr.data_ptr(),
              None if p is None else p.data_ptr(), None if l is None else l.data_ptr(), float(ww), float(eps), B, K, T, Tp, Kp,
              sums.data_ptr(), dl.view.data_ptr(), db.view.data_ptr(), cp.view.data_ptr(), ws.data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[2 * K + 1:]).all()), "the workspace was written past the 2 K + 1 doubles the header states"
    return dict(sums=sums.clone(), dl=dl.check("dlogits", nan_ok), db=db.check("dbias", nan_ok), cp=cp.check("clip_prob"))


def _close(got, ref, bar=BAR):
    """|got - ref| relative to |ref|, absolute where the reference is exactly 0."""
    return abs(got - ref) <= bar * abs(ref) if ref != 0.0 else got == 0.0


@pytest.mark.parametrize("ww", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_weak_frame_bce_against_the_fp64_closed_form(shape, flags, ww):
    B, K, T, Tp, Kp = shape
    c = _loss_case(shape)
    perm = flags == "cross" or shape == (2, 3, 3, 4, 4)
    framed = _flags(flags, B)
    zn, yn = np.nan_to_num(c["z"].numpy()), np.nan_to_num(c["y"].numpy())
    ref = W.loss_closed(zn, yn, c["w"].numpy(), framed.numpy(), T, Tp, Kp, c["perm"].numpy() if perm else None,
                        c["lam"].numpy() if perm else None, ww)
    got = _run_loss(shape, c, framed, perm, ww)
    again = _run_loss(shape, c, framed, perm, ww, sums=got["sums"].clone())
    for k in ("dl", "db", "cp"):
        assert torch.equal(_bits(got[k]), _bits(again[k])), f"{k}: two calls differ"
    g_dl = got["dl"].cpu()
    assert not bool(_bits(g_dl[:, K:]).any()), "pad rows of dlogits are not bitwise 0"
    assert not bool(_bits(g_dl[:, :, T:]).any()), "pad columns of dlogits are not bitwise 0"
    s, s2 = got["sums"].cpu().tolist(), again["sums"].cpu().tolist()
    want = (ref["loss"], ref["frame"], ref["clip"])
    e_dl = _rel(g_dl, ref["dl"]) if np.any(ref["dl"]) else float(g_dl.abs().max())
    e_db = _rel(got["db"], ref["db"]) if np.any(ref["db"]) else float(got["db"].abs().max())
    e_cp = _rel(got["cp"], ref["P"])
    print(f"WSEDK loss {shape} flags={flags} ww={ww} perm={perm}: sums {s} / {want}, dlogits {e_dl:.2e}, dbias {e_db:.2e}, "
          f"clip_prob {e_cp:.2e} (bar {BAR:.0e})")
    assert all(_close(a, r) for a, r in zip(s, want)) and all(_close(a, 2.0 * r) for a, r in zip(s2, want))
    assert e_dl <= BAR and e_db <= BAR and e_cp <= BAR
    f_eff = framed.numpy() != 0
    if perm:
        f_eff = f_eff & f_eff[c["perm"].numpy()]
    if not f_eff.any():
        assert s[1] == 0.0, "L_f must be exactly 0 without a framed row"
    if ww == 0.0:
        assert not bool(_bits(g_dl[torch.from_numpy(~f_eff)]).any()), "an unframed row has a gradient at weak_weight = 0"
    else:                                                                     # the frame part is exactly absent: the
        only = W.loss_closed(zn, yn, c["w"].numpy(), np.zeros(B, np.int32), T, Tp, Kp, c["perm"].numpy() if perm else None,
                             c["lam"].numpy() if perm else None, ww)["dl"]    # unframed rows carry the clip gradient alone
        rows = torch.from_numpy(~f_eff)
        if rows.any():
            assert _rel(g_dl[rows], only[~f_eff]) <= BAR


@pytest.mark.parametrize("shape", [(5, 3, 32, 32, 4), (2, 2, 65, 68, 4), (9, 1, 5, 8, 1)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("perm", [False, True], ids=["plain", "mixup"])
def test_all_framed_at_weight_zero_is_the_strong_label_frame_bce(shape, perm):
    B, K, T, Tp, Kp = shape
    c = _loss_case(shape)
    got = _run_loss(shape, c, torch.ones(B, dtype=torch.int32), perm, 0.0)
    z, y = np.nan_to_num(c["z"].numpy()), np.nan_to_num(c["y"].numpy())
    sums = torch.zeros(1, device=DEV)
    dl, db = ops.frame_bce_fwd_bwd(torch.from_numpy(z).to(DEV), torch.from_numpy(y).to(DEV), T,
                                   perm=c["perm"].to(DEV) if perm else None, lam=c["lam"].to(DEV) if perm else None, sums=sums,
                                   Kp=Kp, dbias=True)
    torch.cuda.synchronize()
    assert _rel(got["dl"], dl) <= BAR and _rel(got["db"], db) <= BAR
    assert abs(got["sums"][1].item() - sums.item()) <= BAR * abs(sums.item())
    assert got["sums"][0].item() == got["sums"][1].item()


@pytest.mark.parametrize("wv", [0.0, 1.0])
def test_saturated_rows_are_finite_and_match_the_closed_form(wv):
    """z = +40 everywhere: P = 1, clamped to 1 - eps; z = -800 everywhere: S1 = 0, the gradient is exactly 0 and the clip loss
    is -(w log eps + (1 - w) log1p(-eps)).  Unframed rows, so the clip term stands alone."""
    shape = (2, 2, 5, 8, 2)
    B, K, T, Tp, Kp = shape
    eps = float(np.float32(1e-7))
    fr = torch.zeros(B, dtype=torch.int32)
    for zv in (40.0, -800.0):
        c = dict(z=torch.full((B, K, Tp), zv), y=torch.zeros(B, K, Tp), w=torch.full((B, K), wv))
        c["z"][:, :, T:], c["y"][:, :, T:] = NAN, NAN
        got = _run_loss(shape, c, fr, False, 1.0)
        ref = W.loss_closed(np.nan_to_num(c["z"].numpy()), np.zeros((B, K, Tp)), c["w"].numpy(), fr.numpy(), T, Tp, Kp)
        dl = got["dl"].cpu()
        assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(got["sums"]).all()) and bool(torch.isfinite(got["db"]).all())
        assert float(dl.abs().max()) <= 1.0 / eps
        if zv < 0:
            assert not bool(_bits(dl).any()) and not bool(_bits(got["db"].cpu()).any()), "S1 = 0: the gradient is exactly 0"
            assert not bool(_bits(got["cp"].cpu()).any())
            want = -(wv * np.log(eps) + (1.0 - wv) * np.log1p(-eps))
        else:
            assert _rel(dl, ref["dl"]) <= BAR if np.any(ref["dl"]) else not bool(dl.any())
            assert bool((got["cp"].cpu() == 1.0).all())
            want = -(wv * np.log(1.0 - eps) + (1.0 - wv) * np.log(eps))
        assert ref["clip"] == pytest.approx(want, rel=1e-12)
        assert _close(got["sums"][2].item(), want) and got["sums"][1].item() == 0.0
        assert _close(got["sums"][0].item(), want)


def test_a_bad_perm_entry_poisons_its_row_only_and_optional_outputs_may_be_left_out():
    shape = (3, 5, 7, 8, 8)
    B, K, T, Tp, Kp = shape
    g = torch.Generator().manual_seed(3)
    c = dict(z=torch.randn(B, K, Tp, generator=g), y=(torch.rand(B, K, Tp, generator=g) < 0.3).float(),
             w=(torch.rand(B, K, generator=g) < 0.5).float(), perm=torch.tensor([2, 7, 0], dtype=torch.int32),
             lam=torch.tensor([0.7, 0.6, 0.9]))
    fr = torch.ones(B, dtype=torch.int32)
    for ww in (1.0, 0.0):
        got = _run_loss(shape, c, fr, True, ww, nan_ok=True)
        dl = got["dl"].cpu()
        assert bool(torch.isnan(dl[1, :K, :T]).all()) and not bool(_bits(dl[1, K:]).any()) and not bool(_bits(dl[1, :, T:]).any())
        assert not bool(torch.isnan(dl[0]).any()) and not bool(torch.isnan(dl[2]).any())
        assert bool(torch.isnan(got["sums"]).all()) and not bool(torch.isnan(got["cp"]).any())
        ok = c["perm"].clone()
        ok[1] = 1                                                             # (every row framed: N_f is what it was)
        ref = W.loss_closed(c["z"].numpy(), c["y"].numpy(), c["w"].numpy(), fr.numpy(), T, Tp, Kp, ok.numpy(), c["lam"].numpy(), ww)
        assert _rel(dl[[0, 2]], ref["dl"][[0, 2]]) <= BAR                     # the other rows are what they were
    # every optional output may be left out; the pooled probabilities alone are one launch
    z, y, w, f = (t.to(DEV) for t in (c["z"], c["y"], c["w"], fr))
    cp = torch.full((B, K), NAN, device=DEV)
    dl2, db2 = ops.weak_frame_bce_fwd_bwd(z, y, w, f, T, grad=False, clip_prob=cp)
    assert dl2 is None and db2 is None
    dl3, db3 = ops.weak_frame_bce_fwd_bwd(z, y, w, f, T, Kp=Kp, dbias=True)
    torch.cuda.synchronize()
    ref = W.loss_closed(c["z"].numpy(), c["y"].numpy(), c["w"].numpy(), fr.numpy(), T, Tp, Kp)
    assert _rel(cp, ref["P"]) <= BAR and _rel(dl3, ref["dl"]) <= BAR and _rel(db3, ref["db"]) <= BAR


def test_loss_replayed_from_a_graph_serves_every_mixture_of_flags():
    """One captured call; the flags change in their static buffer between replays, an all-weak batch included."""
    shape = (5, 3, 32, 32, 4)
    B, K, T, Tp, Kp = shape
    c = _loss_case(shape)
    z, y, w = (torch.nan_to_num(c[k]).to(DEV) for k in ("z", "y", "w"))
    fr = torch.ones(B, device=DEV, dtype=torch.int32)
    sums = torch.zeros(3, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.weak_frame_bce_fwd_bwd(z, y, w, fr, T, sums=sums, Kp=Kp)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dl, _ = ops.weak_frame_bce_fwd_bwd(z, y, w, fr, T, sums=sums, Kp=Kp)
    for kind in ("all", "none", "mixed"):
        flags = _flags(kind, B)
        fr.copy_(flags)
        sums.zero_()
        graph.replay()
        torch.cuda.synchronize()
        ref = W.loss_closed(z.cpu().numpy(), y.cpu().numpy(), w.cpu().numpy(), flags.numpy(), T, Tp, Kp)
        assert _rel(dl, ref["dl"]) <= BAR and all(_close(a, r) for a, r in zip(sums.cpu().tolist(),
                                                                                (ref["loss"], ref["frame"], ref["clip"])))
