"""Every (entry point, route) pair of the forward 1x1 convolutions against an fp64 evaluation of the same formula.

The eleven `eat_pw_conv_*_fwd` entry points fill one request (csrc/eat_common.h: PwFwdReq) and share one route
(csrc/pw_fwd_plan.h): generic plane-size kernel, fp32 LDS kernel, bf16 LDS kernel, x-resident expand kernel, K-streaming
kernel, or the answer 1 where no kernel has the statistics epilogue.  The shapes are the smallest at which a mis-filled
request field shows; each is also a row of the route table in tests/pw_fwd_plan_check.cpp, so its route is pinned there.
Tolerances are the ones the older tests use for the same arithmetic: tests/test_gpu_parity.py (fp32 / bf16x3 / bf16 packs),
tests/test_gpu_train_fuse.py (epilogue partials), tests/test_gpu_bf16_store.py (bf16 storage).
Reference call sites: models/mn/block_types.py:138-181, models/dymn/dy_block.py:103-131."""
import pytest
import torch

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, ops  # noqa: E402
from tests.test_gpu_bf16_store import _assert_is_rounding_of  # noqa: E402

DEV = torch.device("cuda:0")
# max-abs error over the reference's scale, by weight pack: tests/test_gpu_parity.py test_pw_conv / test_pw_conv_bf16
TOL = {"f32": 5e-6, "x3": 3e-5, "b16": 1.5e-2}
POOL_TOL = {"f32": 5e-5, "x3": 20 * 3e-5, "b16": 20 * 1.5e-2}
B16_REL = 2e-5          # bf16 storage, fp32 result against fp64 on the rounded operands: tests/test_gpu_bf16_store.py
PART_REL = 1e-5         # statistics partials against the sums of y as stored: tests/test_gpu_bf16_store.py
GSTAT_TOL = 2e-6        # BatchNorm-backward sums: tests/test_gpu_train_fuse.py


def _case(id, entry, B, Ci, Co, S, pack="f32", act=0, **opt):
    return dict(id=id, entry=entry, B=B, Ci=Ci, Co=Co, S=S, pack=pack, act=act, **opt)


# options: scale / res / pool (bool), tf = activation of the on-load transform, c1 = channels of the first of two sources,
# nbank = K-concat banks (Ci = channels of x), per_sample, x16 / y16 = bf16 storage, stats, gstat = activation of the
# BatchNorm-backward epilogue, mode = eat_pw_stream_mode for the call, rc = the expected answer
CASES = [
    # fp32 LDS kernel: pipelined with a partial m-tile and a column tile that spans samples; NS > 4 (not pipelined); two row
    # chunks (MT = 9 -> 5 + 4); three stages of an 8-tile block (more than 64 KB of LDS)
    _case("f32-pipe", "fwd", 2, 8, 24, 60, act=1, res=True, pool=True),
    _case("f32-nopipe", "fwd", 6, 72, 24, 16, scale=True),
    _case("f32-two-row-chunks", "fwd", 2, 8, 136, 64, act=2),
    _case("f32-lds-above-64k", "fwd", 2, 48, 128, 64, act=1),
    # generic plane size (S = 3 x 5): the three packs, per-sample weights, the statistics entry points' answer 1
    _case("generic-f32", "fwd", 2, 8, 24, 15, act=2, scale=True, res=True, pool=True),
    _case("generic-b16", "bf16", 2, 8, 24, 15, "b16", act=1, scale=True, res=True, pool=True),
    _case("generic-x3", "bf16", 2, 8, 24, 15, "x3", act=2, scale=True, res=True, pool=True),
    _case("generic-dyn", "dyn", 2, 8, 24, 15, act=1, per_sample=True, res=True),
    _case("generic-stats", "stats", 2, 8, 24, 15, stats=True, rc=1),
    _case("generic-gstats", "gstats", 2, 8, 24, 15, stats=True, gstat=1, rc=1),
    # bf16 LDS kernel: two stages (both NPROD), one stage (>= 512 blocks of two 48 KB stages)
    _case("b16lds-two-stages-x3", "bf16", 2, 40, 48, 64, "x3", act=1, res=True),
    _case("b16lds-two-stages-b16", "bf16", 2, 40, 48, 64, "b16", act=1, res=True),
    _case("b16lds-one-stage", "bf16", 8, 32, 128, 16384, "x3", res=True),
    # x-resident expand kernel (stream mode bit 0): one and four k chunks, Co = 2 Ci and 8 Ci (the row-split loop)
    _case("expand-32-64", "bf16", 2, 32, 64, 64, "x3", mode=3),
    _case("expand-32-256", "bf16", 2, 32, 256, 64, "x3", act=2, mode=3),
    _case("expand-128-256", "bf16", 2, 128, 256, 64, "b16", act=2, mode=3),
    _case("expand-128-1024", "bf16", 2, 128, 1024, 64, "x3", mode=3),
    # K-streaming kernel at the default mode; 7 m-tiles must stay on the LDS kernel
    _case("kstream-160-40-x3", "bf16", 2, 160, 40, 64, "x3", scale=True, res=True, pool=True),
    _case("kstream-160-40-b16", "bf16", 2, 160, 40, 64, "b16", scale=True, res=True),
    _case("kstream-not-7-tiles", "bf16", 2, 160, 112, 64, "x3", scale=True, res=True),
    # K-concat: LDS kernel (bit 3 off) and K-streaming kernel (bit 3 on)
    _case("kcat-lds", "kcat", 3, 32, 48, 8, "x3", act=1, nbank=4, res=True, mode=2),
    _case("kcat-kstream", "kcat", 3, 32, 48, 8, "x3", act=1, nbank=4, res=True, mode=10),
    # on-load transform
    _case("tf-f32", "tf", 2, 16, 24, 64, "f32", tf=2, res=True),
    _case("tf-f32-scale", "tf", 2, 16, 24, 64, "f32", act=1, tf=1, scale=True),
    _case("tf-x3", "tf", 2, 16, 24, 64, "x3", tf=2, res=True),
    _case("tf-x3-scale", "tf", 2, 16, 24, 64, "x3", act=1, tf=1, scale=True),
    # two sources
    _case("cat-f32", "cat", 2, 20, 24, 64, "f32", act=1, c1=8, res=True),
    _case("cat-x3", "cat", 2, 40, 24, 64, "x3", c1=32, res=True),
    _case("cat-b16", "cat", 2, 40, 24, 64, "b16", c1=32),
    # per-sample weights on the LDS kernels (two tiles per sample)
    _case("dyn-f32", "dyn", 3, 16, 24, 260, act=2, per_sample=True, res=True),
    _case("dyn-x3", "dyn_bf16", 3, 16, 24, 260, "x3", act=2, per_sample=True, res=True),
    # statistics epilogue: shared and per-sample packs (per-sample: two tiles per sample, the second partial)
    _case("stats-f32", "stats", 3, 16, 24, 260, stats=True),
    _case("stats-x3-tf-scale", "stats", 3, 16, 24, 260, "x3", stats=True, tf=2, scale=True),
    _case("stats-b16", "stats", 3, 16, 24, 260, "b16", stats=True),
    _case("stats-f32-per-sample", "stats", 3, 16, 24, 260, stats=True, per_sample=True),
    _case("stats-x3-per-sample", "stats", 3, 16, 24, 260, "x3", stats=True, per_sample=True),
    # BatchNorm-backward epilogue
    _case("gstats-f32", "gstats", 3, 16, 24, 260, stats=True, gstat=1),
    _case("gstats-x3", "gstats", 3, 16, 24, 260, "x3", stats=True, gstat=2),
    # bf16 storage: the three combinations, two sources, the gz form
    _case("b16-f32-to-b16", "b16", 2, 32, 64, 64, "b16", act=2, y16=True),
    _case("b16-b16-to-f32", "b16", 2, 32, 64, 64, "b16", x16=True, stats=True, res=True),
    _case("b16-b16-to-b16", "b16", 2, 32, 64, 64, "b16", x16=True, y16=True, stats=True),
    _case("b16-two-sources", "b16", 2, 40, 24, 64, "b16", x16=True, c1=32, res=True),
    _case("b16-gz", "b16", 2, 32, 64, 64, "b16", x16=True, y16=True, stats=True, gstat=1),
    # per-sample weights with bf16 storage: both directions, with and without statistics, S = 8 and two tiles per sample
    _case("dyn-b16-out-s8-stats", "dyn_b16", 3, 16, 24, 8, "b16", per_sample=True, y16=True, stats=True),
    _case("dyn-b16-out-s264", "dyn_b16", 3, 16, 24, 264, "b16", act=1, per_sample=True, y16=True),
    _case("dyn-b16-in-s264-stats", "dyn_b16", 3, 16, 24, 264, "b16", per_sample=True, x16=True, stats=True, res=True),
    _case("dyn-b16-in-s8", "dyn_b16", 3, 16, 24, 8, "b16", act=2, per_sample=True, x16=True),
]


def _rand(*shape, seed, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _urand(*shape, seed, lo=0.5):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)) + lo


def make_inputs(c):
    """Seeded operands of a case on the GPU.  K-concat: Ci is the channel count of x, the reduction axis has nbank * Ci rows."""
    B, Ci, Co, S = c["B"], c["Ci"], c["Co"], c["S"]
    nbank, c1 = c.get("nbank", 1), c.get("c1", 0)
    K = nbank * Ci
    i = {}
    cx = c1 if c1 else Ci
    i["x"] = _rand(B, cx, S, seed=1).to(DEV)
    if c.get("x16"):
        i["x"] = i["x"].bfloat16()
    if c1:
        i["x2"] = _rand(B, Ci - c1, S, seed=11).to(DEV)
    i["bias"] = (torch.zeros(Co) if c.get("stats") or c["entry"] == "dyn_b16" else _rand(Co, seed=3, scale=0.1)).to(DEV)
    if c.get("per_sample"):
        bank = _rand(3, Co * Ci, seed=2, scale=Ci ** -0.5).to(DEV)
        if c["pack"] == "b16":      # one-hot attention: the aggregated weights are the bank's, their bf16 rounding is unambiguous
            att = torch.eye(3)[torch.arange(B) % 3].to(DEV)
        else:
            att = torch.softmax(_rand(B, 3, seed=4), dim=-1).to(DEV)
        i["W"] = torch.einsum("bk,kn->bn", att.double(), bank.double()).view(B, Co, Ci)
        pack = {"f32": ops.dyn_pw_pack, "x3": ops.dyn_pw_pack_bf16, "b16": ops.dyn_pw_pack_b16}[c["pack"]]
        i["wp"] = pack(bank, att, Co, Ci)
    else:
        W = _rand(Co, K, seed=2, scale=K ** -0.5).to(DEV)
        i["W"] = W.double()
        i["wp"] = ops._pw_prepack_fp32(W) if c["pack"] == "f32" else ops.pw_prepack_bf16(W, None, split=c["pack"] == "x3")
    if c.get("scale") or nbank > 1:
        i["scale"] = _urand(B, K, seed=5, lo=0.25).to(DEV)
    if c.get("res"):
        i["res"] = _rand(B, Co, S, seed=6).to(DEV)
    if c.get("tf") is not None:
        i["tf_a"], i["tf_b"] = _urand(Ci, seed=7).to(DEV), _rand(Ci, seed=8, scale=0.3).to(DEV)
    if c.get("gstat") is not None:
        z = (_rand(B, Co, S, seed=9) * 1.5 + _rand(1, Co, 1, seed=10)).to(DEV)
        i["gz"] = z.bfloat16() if c.get("y16") else z
        i["g_a"], i["g_b"] = _urand(Co, seed=12).to(DEV), _rand(Co, seed=13, scale=0.5).to(DEV)
    return i


def run(c, i):
    """One call of the case's entry point on poisoned outputs -> dict(rc, y, pool, part)."""
    B, Ci, Co, S, act = c["B"], c["Ci"], c["Co"], c["S"], c["act"]
    p = lambda name: i[name].data_ptr() if name in i else None      # noqa: E731
    wmode = {"f32": 0, "b16": 1, "x3": 2}[c["pack"]]
    y = torch.full((B, Co, S), float("nan"), device=DEV, dtype=torch.bfloat16 if c.get("y16") else torch.float32)
    pool = torch.zeros(B, Co, device=DEV) if c.get("pool") else None
    part = None
    if c.get("stats"):
        tiles = int(_lib.lib().eat_pw_conv_stat_tiles(B, S, 1 if c.get("per_sample") else 0))
        part = torch.full((tiles, 2, Co), float("nan"), device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    yp, pp, sp = y.data_ptr(), None if pool is None else pool.data_ptr(), None if part is None else part.data_ptr()
    e = c["entry"]
    prev = ops.pw_stream_mode(c["mode"]) if "mode" in c else None
    try:
        if e == "fwd":
            rc = _lib.call_rc("eat_pw_conv_fwd", p("x"), p("wp"), p("bias"), p("scale"), p("res"), yp, pp, B, Ci, Co, S, act, st)
        elif e == "bf16":
            rc = _lib.call_rc("eat_pw_conv_bf16_fwd", p("x"), p("wp"), p("bias"), p("scale"), p("res"), yp, pp, B, Ci, Co, S, act,
                              1 if wmode == 2 else 0, st)
        elif e == "tf":
            rc = _lib.call_rc("eat_pw_conv_tf_fwd", p("x"), p("tf_a"), p("tf_b"), c["tf"], p("wp"), wmode, p("bias"), p("scale"),
                              p("res"), yp, B, Ci, Co, S, act, st)
        elif e == "cat":
            rc = _lib.call_rc("eat_pw_conv_cat_fwd", p("x"), c["c1"], p("x2"), Ci - c["c1"], p("wp"), wmode, p("bias"), p("res"), yp,
                              B, Co, S, act, st)
        elif e == "dyn":
            rc = _lib.call_rc("eat_pw_conv_dyn_fwd", p("x"), p("wp"), p("bias"), p("res"), yp, B, Ci, Co, S, act, st)
        elif e == "dyn_bf16":
            rc = _lib.call_rc("eat_pw_conv_dyn_bf16_fwd", p("x"), p("wp"), p("bias"), p("res"), yp, B, Ci, Co, S, act, st)
        elif e == "kcat":
            rc = _lib.call_rc("eat_pw_conv_kcat_fwd", p("x"), p("wp"), p("bias"), p("scale"), p("res"), yp, B, Ci, c["nbank"], Co, S,
                              act, st)
        elif e == "stats":
            rc = _lib.call_rc("eat_pw_conv_stats_fwd", p("x"), p("wp"), wmode, 1 if c.get("per_sample") else 0, p("tf_a"), p("tf_b"),
                              c.get("tf") or 0, p("scale"), p("bias"), yp, sp, B, Ci, Co, S, st)
        elif e == "gstats":
            rc = _lib.call_rc("eat_pw_conv_gstats_fwd", p("x"), p("wp"), wmode, p("bias"), yp, p("gz"), p("g_a"), p("g_b"), c["gstat"],
                              sp, B, Ci, Co, S, st)
        elif e == "b16":
            rc = _lib.call_rc("eat_pw_conv_b16_fwd", p("x"), 1 if c.get("x16") else 0, p("x2"), c.get("c1", 0), p("wp"), p("bias"),
                              p("tf_a"), p("tf_b"), c.get("tf") or 0, p("scale"), p("res"), yp, 1 if c.get("y16") else 0, sp, p("gz"),
                              p("g_a"), p("g_b"), c.get("gstat") or 0, B, Ci, Co, S, act, st)
        else:
            rc = _lib.call_rc("eat_pw_conv_dyn_b16_fwd", p("x"), 1 if c.get("x16") else 0, p("wp"), p("bias"), p("res"), yp,
                              1 if c.get("y16") else 0, sp, B, Ci, Co, S, act, st)
    finally:
        if prev is not None:
            ops.pw_stream_mode(prev)
    torch.cuda.synchronize()
    return dict(rc=rc, y=y, pool=pool, part=part)


def reference(c, i):
    """fp64 evaluation of the case's formula -> y (B, Co, S) float64 before any storage rounding.  Plain-bf16 products with bf16
    storage are evaluated on the rounded operands (tests/test_gpu_bf16_store.py)."""
    nbank, act = c.get("nbank", 1), c["act"]
    x = i["x"].double()
    if "x2" in i:
        x = torch.cat([x, i["x2"].double()], dim=1)
    if c.get("tf") is not None:
        u = i["tf_a"].double()[None, :, None] * x + i["tf_b"].double()[None, :, None]
        x = [u, u.clamp_min(0), u * (u + 3).clamp(0, 6) / 6][c["tf"]]
    x = x.repeat(1, nbank, 1)
    if "scale" in i:
        x = x * i["scale"].double()[:, :, None]
    W = i["W"]
    if c.get("x16") or c.get("y16"):
        x, W = x.float().bfloat16().double(), W.float().bfloat16().double()
    y = torch.einsum("boi,bis->bos" if W.dim() == 3 else "oi,bis->bos", W, x) + i["bias"].double()[None, :, None]
    y = [y, y.clamp_min(0), y * (y + 3).clamp(0, 6) / 6][act]
    if "res" in i:
        y = y + i["res"].double()
    return y


def _rel(got, ref):
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    return float((got - ref).norm() / max(1e-30, float(ref.norm())))


def _close(got, ref, rel, what):
    scale = max(1e-6, float(ref.abs().max()))
    err = float((got.double() - ref).abs().max())
    assert err <= rel * scale, f"{what}: max-abs err {err:.3e} vs scale {scale:.3e} (rel tol {rel})"


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_entry_point_on_its_route(c):
    i = make_inputs(c)
    out = run(c, i)
    assert out["rc"] == c.get("rc", 0)
    y, part = out["y"], out["part"]
    if out["rc"] == 1:                       # no kernel with the epilogue: nothing launched, nothing written
        assert bool(torch.isnan(y).all()) and bool(torch.isnan(part).all())
        return
    ref = reference(c, i)
    wide16 = c.get("x16") or c.get("y16")
    if c.get("y16"):
        _assert_is_rounding_of(y, ref.float(), c["id"])
    elif wide16:
        assert _rel(y, ref) < B16_REL, _rel(y, ref)
    else:
        _close(y, ref, TOL[c["pack"]], c["id"])
    if out["pool"] is not None:
        _close(out["pool"], ref.sum(2), POOL_TOL[c["pack"]], c["id"] + " pool")
    if part is None:
        return
    assert not bool(torch.isnan(part).any())
    # the statistics are those of the conv output z = W x + bias as stored; a residual is added behind them (fp32 y only)
    yd = y.double() - i["res"].double() if "res" in i else y.double()
    if c.get("gstat") is None:               # sums of z and z^2 over the tiles
        s = part.double().sum(0)
        assert _rel(s[0], yd.sum((0, 2))) < PART_REL and _rel(s[1], (yd ** 2).sum((0, 2))) < PART_REL
        return
    # BatchNorm-backward sums of g = y act'(g_a z + g_b) over (y as stored, z), finished by eat_bn_bwd_sums_from_tiles
    Co = c["Co"]
    mean, invstd = _rand(Co, seed=14, scale=0.3).to(DEV), _urand(Co, seed=15).to(DEV)
    sums = ops._gstat_finish(part.view(-1), part.shape[0], Co, (i["g_a"], i["g_b"], mean, invstd), None)
    zd = i["gz"].double()
    u = i["g_a"].double()[None, :, None] * zd + i["g_b"].double()[None, :, None]
    d = {0: torch.ones_like(u), 1: (u > 0).double(), 2: ((u >= -3) & (u <= 3)).double() * (u / 3 + 0.5) + (u > 3).double()}[c["gstat"]]
    g = yd * d
    s0 = g.sum((0, 2))
    s1 = invstd.double() * (g * (zd - mean.double()[None, :, None])).sum((0, 2))
    n0, n1 = float(g.abs().sum((0, 2)).max()), float((g * zd).abs().sum((0, 2)).max()) * float(invstd.max())
    assert float((sums[:Co] - s0).abs().max()) < GSTAT_TOL * n0 and float((sums[Co:] - s1).abs().max()) < GSTAT_TOL * n1
