"""The branches of the DyMN training step (efficientat_amd/dymn_train.py) that the rest of the suite does not pin: a backward
after a second forward re-ran the pack plan, a step without the pack plan (switched off, or captured before it exists), the
loud error after a partial backward, both sides of the size cut in `Linear.backward`, bf16 storage declined by a frozen
`depth_norm`, the skip gradient of a fused block without expand conv, and the per-(tile, sample) weight-gradient kernel behind
EAT_DYMN_WIDE_WGRAD=0.

Every test counts the library's entry points (`_Calls`) and pins the ones that tell its branch apart.  Where two runs of the
same exact-fp32 arithmetic are compared (the kernels add with atomics, so the summation order differs), the bars are those of
tests/test_gpu_train_paths.py: gradient rel-L2 median below 1e-3 (round-off is ~1e-5), maximum below 2e-2 (one activation-kink
flip moves a tensor by up to ~1e-2), over the tensors whose norm is at least 1e-4 of the largest."""
import collections
import contextlib
import copy
import io
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import eat_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, ops  # noqa: E402
from efficientat_amd.dymn import get_model  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 3


class _Calls:
    """with _Calls() as n: ...  ->  n[entry point] = calls made through efficientat_amd._lib inside the block."""

    def __enter__(self):
        self.n, self.saved = collections.Counter(), (_lib.call, _lib.call_rc)

        def call(name, *a):
            self.n[name] += 1
            return self.saved[0](name, *a)

        def call_rc(name, *a):
            self.n[name] += 1
            return self.saved[1](name, *a)
        _lib.call, _lib.call_rc = call, call_rc
        return self.n

    def __exit__(self, *exc):
        _lib.call, _lib.call_rc = self.saved


def _dymn10(prec="fp32"):
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        m = get_model(width_mult=1.0)
    m.classifier[4].p = 0.0
    m.to(DEV).train()
    m.train_precision = prec
    return m


def _data(T=200):
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(B, 1, 128, T, generator=g) * 3.0 - 4.0).to(DEV)
    y = (torch.rand(B, 527, generator=g) < 0.1).float().to(DEV)
    return x, y


def _n_fused(model, x):
    """Number of blocks on the merged plan, by the conditions of dymn_train._block_train_fused."""
    f, t = ops.conv_out(x.shape[2], 3, 2), ops.conv_out(x.shape[3], 3, 2)
    n = 0
    for blk in model.layers:
        k, stride, cexp = blk.cnf.kernel, blk.cnf.stride, blk.cnf.expanded_channels
        fo, to = ops.conv_out(f, k, stride), ops.conv_out(t, k, stride)
        n += bool(to <= 512 and ops.dw_bwd_merged_ok((B, cexp, fo, to), (B, cexp, f, t), k, stride))
        f, t = fo, to
    return n


def _packs(n):
    return (n["eat_pw_prepack"] + n["eat_pw_prepack_bf16"], n["eat_pw_prepack_t"] + n["eat_pw_prepack_bf16_t"])


def _assert_grads(model, ref_g, med_bar=1e-3, max_bar=2e-2):
    gmax = max(float(v.norm()) for v in ref_g.values())
    rels = []
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        if float(ref_g[n].norm()) >= 1e-4 * gmax:
            rels.append((float((p.grad - ref_g[n]).norm() / ref_g[n].norm()), n))
    rels.sort()
    print(f"gradient rel-L2 median {rels[len(rels) // 2][0]:.2e} max {rels[-1][0]:.2e} ({rels[-1][1]}) over {len(rels)} tensors")
    assert rels[len(rels) // 2][0] < med_bar and rels[-1][0] < max_bar, (rels[len(rels) // 2], rels[-1])


def test_backward_after_a_second_forward_packs_its_own_operands():
    """Two forwards before one backward: the second re-runs the pack plan, so the static 1x1 convs of the first pass must not
    read the plan's views in their backward - each packs its transposed matrix itself (three per merged block's context
    generator and the last conv); the backward of a single pass packs none.  Same weights in both passes: same gradients."""
    model = _dymn10()
    ref = copy.deepcopy(model)
    x, y = _data()
    n_static = 3 * _n_fused(model, x) + 1
    assert n_static > 1
    logits, _ = ref(x)
    with _Calls() as n:
        F.binary_cross_entropy_with_logits(logits, y).backward()
    assert _packs(n) == (0, 0), n
    ref_g = {k: p.grad.detach().clone() for k, p in ref.named_parameters()}
    logits, _ = model(x)
    model(x)
    with _Calls() as n:
        F.binary_cross_entropy_with_logits(logits, y).backward()
    assert _packs(n) == (0, n_static), n
    _assert_grads(model, ref_g)


def _case(env, prec="fp32"):
    """tests/dymn_paths_case.py in a process of its own (the switches are read at import) -> its JSON line."""
    e = dict(os.environ, PYTHONPATH=ROOT, **env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "dymn_paths_case.py"), prec], capture_output=True, text=True,
                       timeout=300, env=e, cwd=ROOT)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["finite"] and out["gmax"] > 0, out
    return collections.Counter(out["calls"])


def test_step_without_the_pack_plan_packs_every_matrix_by_itself():
    """EAT_DYMN_PLAN=0: no one-launch pack, one per-matrix pack per static 1x1 conv and direction."""
    model = _dymn10()
    x, _ = _data()
    n_static = 3 * _n_fused(model, x) + 1
    n = _case({"EAT_DYMN_PLAN": "0"})
    assert n["eat_pw_prepack_multi"] == 0 and _packs(n) == (n_static, n_static), n


def test_capture_whose_first_call_precedes_the_pack_plan():
    """GraphedTrainStep(warmup=0): the captured forward is the model's first, the plan does not exist and cannot be built while
    the stream captures - every pack is a launch of its own inside the graph.  Replays reproduce the eager gradients (bound of
    tests/test_gpu_dymn_geometry.py::test_dymn_captured_step_on_the_unfused_path_reproduces_its_gradients: 2e-3)."""
    from efficientat_amd.graphs import GraphedTrainStep
    model = _dymn10()
    ref = copy.deepcopy(model)
    x, y = _data()
    n_static = 3 * _n_fused(model, x) + 1
    F.binary_cross_entropy_with_logits(ref(x)[0], y).backward()
    ref_g = {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
    with _Calls() as n:
        step = GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=0.0), F.binary_cross_entropy_with_logits, x, y, warmup=0)
    assert n["eat_pw_prepack_multi"] == 0 and _packs(n) == (n_static, n_static), n
    gmax = max(float(v.norm()) for v in ref_g.values())
    for r in range(2):
        step(step.x, step.y)
        torch.cuda.synchronize()
        for k, p in model.named_parameters():
            if float(ref_g[k].norm()) >= 1e-3 * gmax:
                assert float((p.grad - ref_g[k]).norm() / ref_g[k].norm()) < 2e-3, (r, k)


def test_partial_backward_makes_the_next_forward_fail_loudly():
    """torch.autograd.grad w.r.t. a parameter of the last block's main path only: that block's input gradient is handed to its
    context path, whose backward never runs.  The next forward of the model says so; the one after works again."""
    model = _dymn10()
    x, y = _data()
    assert _n_fused(model, x) == len(model.layers)
    logits, _ = model(x)
    loss = F.binary_cross_entropy_with_logits(logits, y)
    (g,) = torch.autograd.grad(loss, [model.layers[-1].proj_norm.weight])
    assert torch.isfinite(g).all() and float(g.norm()) > 0
    with pytest.raises(_lib.EatHipError, match="EAT_DYMN_FUSED_DW"):
        model(x)
    logits, _ = model(x)
    F.binary_cross_entropy_with_logits(logits, y).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


@pytest.mark.parametrize("M", [4096, 4092, 4098])
def test_linear_backward_on_both_sides_of_its_size_cut(M):
    """`Linear.backward` takes the weight gradient of M >= 4096 rows (M % 4 == 0) through the 1x1 weight-gradient GEMM and of
    fewer through the linear kernel; against torch on the CPU in fp64.  Bar: every output element is an fp32-accumulated sum of
    at most M products, whose error is bounded by M * 2^-24 = 2.5e-4 of the sum of magnitudes (measured: ~1e-6)."""
    from efficientat_amd.dymn_train import Linear
    K, N = 16, 32
    g = torch.Generator().manual_seed(M)
    x, w, b, dy = (torch.randn(*s, generator=g) for s in ((M, K), (N, K), (N,), (M, N)))
    xd, wd, bd = (t.to(DEV).requires_grad_(True) for t in (x, w, b))
    with ops.precision("fp32"):
        out = Linear.apply(xd, wd, bd)
    with _Calls() as n:
        out.backward(dy.to(DEV))
    wgrad = sum(v for k, v in n.items() if k.startswith("eat_pw_conv_wgrad"))
    wide = M >= 4096 and M % 4 == 0
    assert (wgrad, n["eat_linear_fwd"]) == ((1, 1) if wide else (0, 2)), n
    xr, wr, br = (t.double().requires_grad_(True) for t in (x, w, b))
    F.linear(xr, wr, br).backward(dy.double())
    bar = M * 2.0 ** -24
    for name, got, ref in (("out", out, F.linear(xr, wr, br)), ("dx", xd.grad, xr.grad), ("dw", wd.grad, wr.grad), ("db", bd.grad, br.grad)):
        e = float((got.detach().double().cpu() - ref.detach()).norm() / ref.detach().norm())
        print(f"Linear M={M} {name}: rel-L2 {e:.2e}")
        assert e < bar, (name, e)


def test_frozen_depth_norm_keeps_a_block_on_fp32_storage():
    """act_storage = 'bf16' with every depth_norm in eval(): the bf16-storage kernels take their statistics from the values as
    stored, which a frozen BatchNorm does not have - every merged block stays on fp32 storage.  Control: the same step with
    training depth_norms stores some blocks in bf16 at this geometry."""
    x, y = _data(T=500)
    for freeze in (False, True):
        model = _dymn10("bf16")
        model.act_storage = "bf16"
        if freeze:
            for blk in model.layers:
                blk.depth_norm.eval()
        n_fused = _n_fused(model, x)
        with _Calls() as n:
            logits, _ = model(x)
            F.binary_cross_entropy_with_logits(logits, y).backward()
        assert n["eat_dyrelu_ca_fwd2"] + n["eat_dyrelu_ca_fwd2_b16"] == n_fused > 0, n
        if not freeze:
            assert n["eat_dyrelu_ca_fwd2_b16"] > 0 and n["eat_dyrelu_ca_bwd2_b16"] == n["eat_dyrelu_ca_fwd2_b16"], n
            continue
        assert n["eat_dyrelu_ca_fwd2_b16"] == 0 and n["eat_dyrelu_ca_bwd2_b16"] == 0, n
        assert n["eat_dw_conv_dyn_fwd_stats_b16"] == 0 and n["eat_pw_conv_dyn_b16_fwd"] == 0, n
        for blk in model.layers:
            assert int(blk.depth_norm.num_batches_tracked) == 0 and int(blk.proj_norm.num_batches_tracked) == 1
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())


def test_fused_block_without_expand_conv_adds_the_skip_gradient_once():
    """Block 0 (no expand conv, residual) on the merged plan: the skip gradient enters the merged depthwise backward as its
    `res` operand.  Against torch-CPU autograd over the oracle block: dx to the bar of
    test_gpu_dymn.py::test_dy_block_train_forward_backward (1e-2: activation kinks); a skip gradient dropped or added twice
    is an error of exactly |dout|, so the error is also held below a tenth of that."""
    from efficientat_amd.dymn_train import _block_train
    sd = synth.synth_state(synth.dymn_shapes(1.0), seed=0)
    with contextlib.redirect_stdout(io.StringIO()):
        model = get_model(width_mult=1.0)
    model.load_state_dict(sd)
    model.to(DEV).train()
    blocks, _ = O.block_table(1.0)
    c, temp = blocks[0], 30.0
    assert c["cexp"] == c["cin"] and model.layers[0].use_res_connect
    x = torch.randn(B, c["cin"], 64, 200, generator=torch.Generator().manual_seed(1))
    skip = ("running_mean", "running_var", "num_batches_tracked", "lambdas", "init_v")
    sdr = {k: (v.clone().requires_grad_(True) if not k.endswith(skip) else v.clone()) for k, v in sd.items() if k.startswith("layers.0.")}
    xr = x.clone().requires_grad_(True)
    out_ref = O._dy_block(sdr, "layers.0", xr, c, O.context_dim(c["cexp"], 1.0), True, {}, temp)
    dout = torch.randn(*out_ref.shape, generator=torch.Generator().manual_seed(99))
    out_ref.backward(dout)
    blk = model.layers[0]
    for m in blk.modules():
        if hasattr(m, "temperature"):
            m.temperature = temp
    xd = x.to(DEV).requires_grad_(True)
    with _Calls() as n, ops.precision("fp32"):
        out = _block_train(blk, xd)
        out.backward(dout.to(DEV))
    assert n["eat_dyrelu_ca_fwd2"] == 1 and n["eat_dw_conv_dyn_bwd_bn_g"] == 1 and n["eat_ctx_pool_cm_bwd"] == 1, n
    err = float((xd.grad.cpu().double() - xr.grad.double()).norm())
    print(f"block 0: |dx - ref| = {err:.3e}, |ref| = {float(xr.grad.norm()):.3e}, |dout| = {float(dout.norm()):.3e}")
    assert err < 1e-2 * float(xr.grad.double().norm()), err
    assert err < 0.1 * float(dout.double().norm()), err


def test_wide_wgrad_switched_off_takes_the_per_sample_tile_kernel():
    """EAT_DYMN_WIDE_WGRAD=0 on fp32 storage: the per-sample weight gradients of the dynamic 1x1 convs run on
    eat_pw_conv_dyn_wgrad (two per block with expand conv, one for block 0), none on the wide-tile kernel."""
    model = _dymn10()
    n_dyn = sum(2 if blk.has_expand else 1 for blk in model.layers)
    n = _case({"EAT_DYMN_WIDE_WGRAD": "0"})
    assert n["eat_pw_conv_dyn_wgrad"] == n_dyn and n["eat_pw_conv_dyn_wgrad_b16"] == 0, n
    n = _case({})
    assert n["eat_pw_conv_dyn_wgrad"] + n["eat_pw_conv_dyn_wgrad_b16"] == n_dyn and n["eat_pw_conv_dyn_wgrad_b16"] > 0, n
