"""The branches of the monolithic MN training plan (efficientat_amd/mn_train.py) that the released configurations at their
usual input sizes never take: a stem whose consumer has an expand conv (the pre-activation tensor is written, the stem hands
channel sums to the block), a residual block without expand conv that is not the stem's consumer, planes the merged
depthwise backward / the two-source data-gradient GEMM do not take, a backward after the pack plan was re-run by a second
forward, and a capture whose first call precedes the pack plan.

Reference: the SAME model through `forward_train_modular` - one autograd Function per layer, torch autograd between them,
none of the plan's fusions.  Both sides run exact-fp32 arithmetic on the same function in different summation orders, which
is the situation of `__graft_entry__.smoke()` (fp32 plan vs fp32 CPU oracle), so its bars apply: loss to 1e-4 relative,
gradient rel-L2 median below 1e-3 (round-off is ~1e-5) and maximum below 2e-2 (one activation-kink flip moves a tensor by
up to ~1e-2), over the tensors whose norm is at least 1e-4 of the largest.

Every test counts the library's entry points during the plan's step (`_Calls`) and pins the ones that tell its branch apart,
so a changed threshold or geometry predicate turns the test red instead of quietly moving it onto the common path."""
import collections
import contextlib
import copy
import io

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, mn_train  # noqa: E402
from efficientat_amd.mn import MN, InvertedResidualConfig, get_model  # noqa: E402
from efficientat_amd.mn_train import forward_train_modular  # noqa: E402

DEV = torch.device("cuda:0")


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


def _custom():
    row = [(16, 3, 64, 24, False, "RE", 2),       # first block WITH expand conv: the stem writes z0 and hands over channel sums
           (24, 3, 24, 24, False, "RE", 1),       # residual, no expand conv, not the stem's consumer
           (24, 5, 72, 40, True, "HS", 2),
           (40, 3, 120, 40, True, "HS", 1)]
    return MN([InvertedResidualConfig(*r, 1, 1.0) for r in row], 64, num_classes=10, head_type="mlp", dropout=0.0)


def _mn10():
    with contextlib.redirect_stdout(io.StringIO()):
        return get_model(width_mult=1.0)


def _pair(make):
    torch.manual_seed(0)
    m = make()
    for p in m.classifier.parameters():           # (the head's N(0, 0.01) init leaves gradients near the fp32 floor)
        if p.dim() == 2:
            torch.nn.init.normal_(p, 0, 0.2)
    if isinstance(m.classifier[4], torch.nn.Dropout):
        m.classifier[4].p = 0.0
    m.to(DEV).train()
    m.train_precision = "fp32"
    return m, copy.deepcopy(m)


def _step(model, x, y):
    """One forward + backward of the plan -> (loss, logits, entry-point counts)."""
    with _Calls() as n:
        logits, _ = model(x)
        loss = F.binary_cross_entropy_with_logits(logits, y)
        loss.backward()
    return float(loss), logits.detach(), n


def _rels(model, ref_g, floor=1e-4):
    gmax = max(float(v.norm()) for v in ref_g.values())
    return {n: float((p.grad - ref_g[n]).norm() / ref_g[n].norm()) for n, p in model.named_parameters()
            if float(ref_g[n].norm()) >= floor * gmax}


def _data(B, Fm, T, n_cls):
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(B, 1, Fm, T, generator=g) * 3.0 - 4.0).to(DEV)
    y = (torch.rand(B, n_cls, generator=g) < 0.1).float().to(DEV)
    return x, y


def _reference_grads(ref, x, y):
    logits, _ = forward_train_modular(ref, x)
    loss = F.binary_cross_entropy_with_logits(logits, y)
    loss.backward()
    return float(loss), {n: p.grad.detach().clone() for n, p in ref.named_parameters()}


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


@pytest.mark.parametrize("make,shape", [(_custom, (6, 64, 200)), (_custom, (3, 64, 99)), (_mn10, (4, 40, 99)), (_mn10, (3, 128, 301))],
                         ids=["custom", "custom_odd_planes", "mn10_40x99", "mn10_128x301"])
def test_plan_matches_the_per_layer_functions(make, shape):
    model, ref = _pair(make)
    x, y = _data(*shape, model.classifier[5].out_features)
    loss_ref, ref_g = _reference_grads(ref, x, y)
    loss, _, n = _step(model, x, y)
    assert abs(loss - loss_ref) < 1e-4 * max(1.0, abs(loss_ref)), (loss, loss_ref)
    _assert_grads(model, ref_g)
    if make is _custom:
        # the stem wrote its pre-activation tensor; block 1 (residual, no expand conv, not the stem's consumer) took the
        # separate depthwise passes, the other three the merged kernel
        assert n["eat_stem_gram"] == 0 and n["eat_bn_stats_partial"] == 1 and n["eat_stem_bwd"] == 0, n
        assert n["eat_dw_conv_dgrad"] == 1 and n["eat_dw_conv_wgrad"] == 2 and n["eat_dw_conv_bwd_bn_g"] == 3, n
    elif shape[2] == 99:
        # 20 x 50 ... 2 x 4 planes: the statistics epilogue of the 1x1 convs and the two-source data-gradient GEMM decline most
        assert n["eat_bn_stats"] > 0 and n["eat_pw_conv_cat_fwd"] < 14 and n["eat_expand_bwd_coef"] == 15, n
    # running statistics after the step, to round-off: the variance relative to itself, the mean in units of the layer's standard
    # deviation (the mean of a conv that follows a zero-mean BatchNorm output is itself round-off: no relative error to speak of)
    for (n, a), (_, b) in zip(model.named_modules(), ref.named_modules()):
        if isinstance(a, torch.nn.BatchNorm2d):
            var = b.running_var.double()
            assert float((a.running_var.double() - var).norm()) <= 1e-3 * float(var.norm()), n
            assert float((a.running_mean.double() - b.running_mean.double()).norm()) <= 1e-3 * float(var.sqrt().norm()), n
            assert int(a.num_batches_tracked) == int(b.num_batches_tracked) == 1, n


def test_backward_after_a_second_forward_packs_its_own_operands():
    """Two forwards before one backward: the second re-runs the pack plan, so the first pass's backward must not read the
    plan's views.  The weights are the same in both, so the gradients are those of the single pass."""
    model, ref = _pair(_mn10)
    x, y = _data(3, 128, 200, 527)
    _, ref_g = _reference_grads(ref, x, y)
    logits, _ = model(x)
    model(x)
    with _Calls() as n:
        F.binary_cross_entropy_with_logits(logits, y).backward()
    assert n["eat_pw_prepack_t"] + n["eat_pw_prepack_bf16_t"] == 16, n       # 15 project convs + the last conv, one by one
    _assert_grads(model, ref_g)


def test_plan_without_the_merged_depthwise_backward(monkeypatch):
    """The merged depthwise backward covers every plane a test can afford (it declines from 2^27 elements per sample), so its
    geometry predicate is switched off here: every block takes the BatchNorm-backward pass of its own (with and without SE
    gate) and the depthwise backward from dz_d, which run on any geometry."""
    monkeypatch.setattr(mn_train.ops, "dw_bwd_merged_ok", lambda *a: False)
    model, ref = _pair(_mn10)
    x, y = _data(3, 128, 200, 527)
    loss_ref, ref_g = _reference_grads(ref, x, y)
    loss, _, n = _step(model, x, y)
    assert n["eat_dw_conv_bwd_bn_g"] == 0 and n["eat_dw_conv_bwd_g"] == 14 and n["eat_dw_conv_dgrad"] == 1, n
    assert n["eat_se_bn_bwd_partials"] == 8, n
    assert abs(loss - loss_ref) < 1e-4 * max(1.0, abs(loss_ref)), (loss, loss_ref)
    _assert_grads(model, ref_g)


def _median(v):
    v = sorted(v)
    return v[len(v) // 2]


def test_bf16_storage_with_frozen_project_batchnorm():
    """act_storage='bf16' with every project BatchNorm in eval() (depthwise / expand ones training): the project conv reads the
    bf16-stored z_d / y_d without a statistics epilogue and leaves an fp32 z_p.  bf16 round-off is amplified by the net, so - as
    in test_gpu_configs.py::test_mn40_train_step_bf16_tracks_oracle (b) - the criterion is "not further from the fp32 evaluation
    than the same bf16 arithmetic on fp32 storage is" (x 1.25 + 1 %), loss to 2 %; no gradient tensor off by its own norm."""
    runs = {}
    x, y = _data(4, 128, 1000, 527)
    for tag, prec, storage in (("fp32", "fp32", "fp32"), ("bf16", "bf16", "fp32"), ("stored", "bf16", "bf16")):
        model, _ = _pair(_mn10)
        model.train_precision, model.act_storage = prec, storage
        for blk in model.features[1:-1]:
            blk.block[blk.i_proj][1].eval()
        before = {k: v.clone() for k, v in model.state_dict().items() if ".running_" in k}
        loss, _, n = _step(model, x, y)
        runs[tag] = (loss, {k: p.grad.detach().clone() for k, p in model.named_parameters()}, model, n)
        for blk in model.features[1:-1]:                                    # frozen: buffers untouched
            bn = blk.block[blk.i_proj][1]
            assert int(bn.num_batches_tracked) == 0 and torch.equal(bn.running_var, torch.ones_like(bn.running_var))
        assert any(not torch.equal(v, model.state_dict()[k]) for k, v in before.items())    # (the others trained)
    n = runs["stored"][3]
    # every block on bf16 storage (15 depthwise convs / merged backwards), no statistics epilogue in any project conv:
    # 15 depthwise + 1 last-conv finalize launches only (the fp32-storage run has the same count: same frozen layers)
    assert n["eat_dw_conv_fwd_stats_b16"] == 15 and n["eat_dw_conv_bwd_bn_g_b16"] == 15, n
    assert n["eat_bn_finalize_partials"] == runs["bf16"][3]["eat_bn_finalize_partials"] == 16, n
    ref_g = runs["fp32"][1]
    far = {t: _rels(runs[t][2], ref_g) for t in ("bf16", "stored")}
    print(f"vs fp32: bf16 operands median {_median(far['bf16'].values()):.2e} max {max(far['bf16'].values()):.2e}; "
          f"+ bf16 storage median {_median(far['stored'].values()):.2e} max {max(far['stored'].values()):.2e}")
    assert abs(runs["stored"][0] - runs["fp32"][0]) < 2e-2 * abs(runs["fp32"][0])
    assert _median(far["stored"].values()) < 1.25 * _median(far["bf16"].values()) + 1e-2
    assert max(far["stored"].values()) < 1.0, max(far["stored"].items(), key=lambda kv: kv[1])


def test_bf16_storage_backward_sums_from_the_data_gradient_epilogue(monkeypatch):
    """mn40 at 40 clips on bf16 storage: the depthwise outputs of the first wide blocks pass _GSTATS_MIN_ELEMS, so the channel
    sums of their BatchNorm backward leave the project data-gradient GEMM's epilogue.  Reference: the same step with the
    threshold out of reach (the reduce pass, which the bf16-storage tests of test_gpu_configs.py pin on the oracle).  Same
    arithmetic, another summation order - the situation and the bound (5e-2 per tensor on bf16 storage) of
    test_gpu_trainloop.py::test_mn_captured_step_reproduces_its_gradients_on_every_replay; the forward is the same code."""
    x, y = _data(40, 128, 1000, 527)
    runs = {}
    for tag in ("epilogue", "reduce"):
        if tag == "reduce":
            monkeypatch.setattr(mn_train, "_GSTATS_MIN_ELEMS", 1 << 62)
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            model = get_model(width_mult=4.0)
        model.classifier[4].p = 0.0
        model.to(DEV).train()
        model.train_precision, model.act_storage = "bf16", "bf16"
        loss, logits, n = _step(model, x, y)
        runs[tag] = (loss, logits, n, model)
    ne, nr = runs["epilogue"][2], runs["reduce"][2]
    moved = nr["eat_bn_act_bwd_reduce_b16"] - ne["eat_bn_act_bwd_reduce_b16"]
    assert moved > 0 and nr["eat_bn_bwd_sums_from_tiles"] == 0 and ne["eat_bn_bwd_sums_from_tiles"] > 0, (ne, nr)
    assert abs(runs["epilogue"][0] - runs["reduce"][0]) < 1e-5 * abs(runs["reduce"][0])
    ref_g = {k: p.grad for k, p in runs["reduce"][3].named_parameters()}
    rels = _rels(runs["epilogue"][3], ref_g, floor=1e-3)
    print(f"{moved} reduce passes moved into the epilogue; gradient rel-L2 median {_median(rels.values()):.2e} max {max(rels.values()):.2e}")
    assert max(rels.values()) < 5e-2, max(rels.items(), key=lambda kv: kv[1])


def test_capture_whose_first_call_precedes_the_pack_plan():
    """GraphedTrainStep(warmup=0): the captured forward is the model's first, the plan does not exist yet and every weight
    pack is a launch of its own inside the graph.  Replays reproduce the eager gradients (bound of
    test_gpu_trainloop.py::test_mn_captured_step_reproduces_its_gradients_on_every_replay, fp32 storage: 2e-3)."""
    from efficientat_amd.graphs import GraphedTrainStep
    model, ref = _pair(_mn10)
    ref.train_precision = model.train_precision = "auto"
    x, y = _data(4, 128, 200, 527)
    F.binary_cross_entropy_with_logits(ref(x)[0], y).backward()
    ref_g = {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
    with _Calls() as n:
        step = GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=0.0), F.binary_cross_entropy_with_logits, x, y, warmup=0)
    assert n["eat_pw_prepack_multi"] == 0 and n["eat_pw_prepack"] + n["eat_pw_prepack_bf16"] == 30, n    # (no plan: 14 + 15 + 1 packs)
    gmax = max(float(v.norm()) for v in ref_g.values())
    for r in range(2):
        step(step.x, step.y)
        torch.cuda.synchronize()
        for n, p in model.named_parameters():
            if float(ref_g[n].norm()) >= 1e-3 * gmax:
                assert float((p.grad - ref_g[n]).norm() / ref_g[n].norm()) < 2e-3, (r, n)
