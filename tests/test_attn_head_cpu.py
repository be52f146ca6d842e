"""CPU checks of the attention-pooling head: the fp64 restatement of tests/attn_head_ref.py against the oracle and torch
autograd over it, the operand refusals of the four launchers, and fine-tuning from a checkpoint of another head."""
import contextlib
import io

import pytest
import torch

from efficientat_amd import ops
from efficientat_amd._lib import EatHipError
from oracle import eat_oracle as O
from tests import attn_head_ref as R


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _rel(got, ref):
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ reference agreement
@pytest.mark.parametrize("B,C,F,T,H,K", [(1, 4, 1, 1, 1, 1), (2, 8, 2, 7, 3, 5), (3, 12, 4, 32, 4, 11), (2, 6, 3, 10, 4, 50)])
def test_reference_agrees_with_the_oracle_and_its_autograd(B, C, F, T, H, K):
    g = torch.Generator().manual_seed(B * 100 + T)
    N = 2 * H * K
    y = torch.randn(B, C, F, T, generator=g, dtype=torch.float64).requires_grad_(True)
    w = (torch.randn(N, C, generator=g, dtype=torch.float64) * 2.0).requires_grad_(True)      # logits wide enough to hit the clamp
    w.data[:H * K] *= 6.0
    b = (torch.randn(N, generator=g, dtype=torch.float64) * 0.3).requires_grad_(True)
    hw = (0.1 + torch.rand(1, H, 1, generator=g, dtype=torch.float64)).requires_grad_(True)
    sd = {"classifier.subspace_proj.weight": w, "classifier.subspace_proj.bias": b, "classifier.head_weight": hw}
    logits, feat = O._attention_head(sd, y, num_heads=H)
    out = R.head(y.detach(), w.detach(), b.detach(), hw.detach(), H)
    assert out.shape == logits.shape == (B, K)
    assert _rel(out, logits.detach()) <= 1e-12
    assert _rel(R.freq_mean(y.detach()).mean(dim=2), feat.detach()) <= 1e-12
    gout = torch.randn(B, K, generator=g, dtype=torch.float64)
    dy, dw, db, dhw = torch.autograd.grad(logits, (y, w, b, hw), gout)
    got = R.head_bwd(gout, y.detach(), w.detach(), b.detach(), hw.detach(), H)
    for name, a, r in zip(("dy", "dw", "db", "dhead_w"), got, (dy, dw, db, dhw.reshape(-1))):
        assert a.shape == r.shape, name
        assert _rel(a, r) <= 1e-12, (name, _rel(a, r))
    if T > 1:       # the clamp was active somewhere, on both sides of the reference's formula
        p = torch.einsum("nc,bct->bnt", w.detach(), R.freq_mean(y.detach())) + b.detach().view(1, N, 1)
        sig = torch.sigmoid(p[:, :H * K])
        assert bool((sig > 1 - 1e-7).any()) or bool((sig < 1e-7).any())


def test_reference_pool_inputs_hit_both_clamp_bounds_and_keep_clear_of_them():
    p, bias, hw, g = R.pool_inputs(3, 4, 50, 32, seed=1)
    q = (p.double() + bias.double().view(1, -1, 1))[:, :200]
    assert bool((q > 19.9).any()) and bool((q < -19.9).any())
    assert not bool(((q.abs() > 12.001) & (q.abs() < 19.999)).any())
    assert g.shape == (3, 50) and hw.shape == (4,) and float(hw.min()) >= 0.1


# ------------------------------------------------------------------------------------------------ operand refusals
def _pool_args(B=2, H=3, K=5, T=7, Tp=8):
    N = 2 * H * K
    return dict(p=torch.zeros(B, N, Tp), bias=torch.zeros(N), head_w=torch.ones(H), H=H, T=T)


def _bwd_args(B=2, H=3, K=5, T=7, Tp=8):
    a = _pool_args(B, H, K, T, Tp)
    a.update(g=torch.zeros(B, K), o=torch.zeros(B, H, K), s=torch.ones(B, H, K))
    return a


@pytest.mark.parametrize("fn,make", [(ops.attn_pool, _pool_args), (ops.attn_pool_bwd, _bwd_args)], ids=["fwd", "bwd"])
def test_pool_launchers_refuse_bad_operands_without_a_gpu(fn, make):
    name = fn.__name__
    for key in ("p", "bias", "head_w"):
        a = make()
        a[key] = a[key].double()
        with pytest.raises(EatHipError, match=f"{name}: {key} must be a contiguous float32"):
            fn(**a)
    a = make()
    a["p"] = torch.zeros(2, 8, 30).transpose(1, 2)                      # (2, 30, 8), strided
    with pytest.raises(EatHipError, match=f"{name}: p must be a contiguous float32"):
        fn(**a)
    a = make()
    a["head_w"] = torch.ones(4)
    with pytest.raises(EatHipError, match=f"{name}: head_w must be .* of 3 elements"):
        fn(**a)
    a = make()
    a["bias"] = torch.zeros(31)
    with pytest.raises(EatHipError, match=f"{name}: bias must be .* of 30 elements"):
        fn(**a)
    a = make()
    a["T"] = 9
    with pytest.raises(EatHipError, match=f"{name}: Tp=8 is shorter than T=9"):
        fn(**a)
    a = make()
    a["H"] = 4
    with pytest.raises(EatHipError, match=f"{name}: p has 30 rows per sample"):
        fn(**a)
    with pytest.raises(EatHipError, match=f"{name}: p must live on the GPU"):    # well-formed CPU operands: no CPU path
        fn(**make())


def test_pool_backward_refuses_its_own_operands_without_a_gpu():
    for key, n in (("g", 10), ("o", 30), ("s", 30)):
        a = _bwd_args()
        a[key] = a[key].double()
        with pytest.raises(EatHipError, match=f"attn_pool_bwd: {key} must be a contiguous float32 tensor of {n} elements"):
            ops.attn_pool_bwd(**a)
    a = _bwd_args()
    a["g"] = torch.zeros(2, 6)
    with pytest.raises(EatHipError, match="attn_pool_bwd: g must be .* of 10 elements"):
        ops.attn_pool_bwd(**a)
    with pytest.raises(EatHipError, match="attn_pool_bwd: Np=28 is smaller than 2 H K = 30"):
        ops.attn_pool_bwd(Np=28, **_bwd_args())
    with pytest.raises(EatHipError, match="attn_pool_bwd: dp must be .* of 480 elements"):
        ops.attn_pool_bwd(dp=torch.zeros(2, 30, 7), **_bwd_args())


def test_frequency_mean_launchers_refuse_bad_operands_without_a_gpu():
    y = torch.zeros(2, 3, 4, 7)
    with pytest.raises(EatHipError, match="freq_mean: y must be a contiguous float32"):
        ops.freq_mean(y.double())
    with pytest.raises(EatHipError, match="freq_mean: y must be a contiguous float32"):
        ops.freq_mean(y.transpose(2, 3))
    with pytest.raises(EatHipError, match="freq_mean: Tp=6 is shorter than T=7"):
        ops.freq_mean(y, Tp=6)
    with pytest.raises(EatHipError, match="freq_mean: y must be a non-empty"):
        ops.freq_mean(y[0])
    with pytest.raises(EatHipError, match="freq_mean: out must be .* of 48 elements"):
        ops.freq_mean(y, out=torch.zeros(2, 3, 7))
    with pytest.raises(EatHipError, match="freq_mean: y must live on the GPU"):
        ops.freq_mean(y)
    d = torch.zeros(2, 3, 8)
    with pytest.raises(EatHipError, match="freq_mean_bwd: dxm must be a contiguous float32"):
        ops.freq_mean_bwd(d.double(), 4, 7)
    with pytest.raises(EatHipError, match="freq_mean_bwd: dxm must be a contiguous float32"):
        ops.freq_mean_bwd(torch.zeros(2, 8, 3).transpose(1, 2), 4, 7)
    with pytest.raises(EatHipError, match="freq_mean_bwd: Tp=8 is shorter than T=9"):
        ops.freq_mean_bwd(d, 4, 9)
    with pytest.raises(EatHipError, match="freq_mean_bwd: dxm must live on the GPU"):
        ops.freq_mean_bwd(d, 4, 7)
    assert [ops.pitch4(t) for t in (1, 4, 10, 32, 33)] == [4, 4, 12, 32, 36]


def test_the_attn_header_parses_is_disjoint_from_the_other_headers_and_is_bound():
    import ctypes
    import os
    from efficientat_amd import _lib, build
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "eat_attn.h")) as f:
        protos = _lib.parse_prototypes(f.read())
    assert protos == _lib.ATTN_PROTOTYPES
    assert set(protos) == {"eat_freq_mean_fwd", "eat_freq_mean_bwd", "eat_attn_pool_fwd", "eat_attn_pool_bwd"}
    assert protos["eat_freq_mean_fwd"] == protos["eat_freq_mean_bwd"] == (I, [P, P, I, I, I, I, I, P])
    assert protos["eat_attn_pool_fwd"] == (I, [P, P, P, D, P, P, P, I, I, I, I, I, P])
    assert protos["eat_attn_pool_bwd"] == (I, [P, P, P, P, D, P, P, P, P, P, P, I, I, I, I, I, I, P])
    for other in (_lib.PROTOTYPES, _lib.TAG_PROTOTYPES, _lib.EMBED_PROTOTYPES):
        assert not set(protos) & set(other)
    assert "attn_head.hip" in build.SOURCES
    build.build()
    for name, (restype, args) in protos.items():
        fn = getattr(_lib.lib(), name)
        assert list(fn.argtypes) == args and fn.restype is restype, name
    # argument checks that return before anything touches the device
    with pytest.raises(EatHipError, match="eat_freq_mean_fwd: missing operand"):
        _lib.call("eat_freq_mean_fwd", None, None, 1, 1, 1, 1, 1, None)
    with pytest.raises(EatHipError, match="eat_attn_pool_fwd: missing operand"):
        _lib.call("eat_attn_pool_fwd", None, None, None, 1e-7, None, None, None, 1, 1, 1, 1, 1, None)


# ------------------------------------------------------------------------------------------------ loader
def test_a_checkpoint_of_another_head_initialises_the_trunk_of_an_attention_head_model(tmp_path):
    from efficientat_amd.finetune import load_init_checkpoint
    from efficientat_amd.mn import get_model
    torch.manual_seed(0)
    src = _quiet(get_model, num_classes=527, head_type="mlp")
    path = str(tmp_path / "as.pt")
    torch.save(src.state_dict(), path)
    torch.manual_seed(1)
    dst = _quiet(get_model, num_classes=50, head_type="multihead_attention_pooling")
    before = {k: v.clone() for k, v in dst.state_dict().items()}
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        dropped = load_init_checkpoint(dst, path)
    assert "Loading weights for classifier only implemented for head types 'mlp' and 'fully_convolutional'" in out.getvalue()
    ssd = src.state_dict()
    assert sorted(dropped) == sorted(k for k in ssd if k.startswith("classifier.")) and len(dropped) == 4
    n_feat = 0
    for k, v in dst.state_dict().items():
        if k.startswith("features."):
            assert torch.equal(v, ssd[k]), k
            n_feat += 1
        else:
            assert k.startswith("classifier.") and torch.equal(v, before[k]), k      # the head keeps its fresh initialisation
    assert n_feat == sum(k.startswith("features.") for k in ssd) > 100
    head = dst.classifier
    assert torch.equal(head.head_weight, torch.full((1, 4, 1), 0.25)) and bool((head.subspace_proj.bias == 0).all())
    assert 0.005 < float(head.subspace_proj.weight.detach().std()) < 0.02


def test_a_checkpoint_of_another_head_and_another_width_is_still_refused(tmp_path):
    from efficientat_amd.finetune import load_init_checkpoint
    from efficientat_amd.mn import get_model
    path = str(tmp_path / "as05.pt")
    torch.save(_quiet(get_model, num_classes=527, width_mult=0.5).state_dict(), path)
    dst = _quiet(get_model, num_classes=50, width_mult=1.0, head_type="multihead_attention_pooling")
    before = {k: v.clone() for k, v in dst.state_dict().items()}
    with pytest.raises(ValueError, match="does not fit head 'multihead_attention_pooling'"):
        _quiet(load_init_checkpoint, dst, path)
    assert all(torch.equal(v, before[k]) for k, v in dst.state_dict().items())
    # a trunk with tensors the model does not have (or without some it has) is no fit either
    sd = _quiet(get_model, num_classes=527).state_dict()
    sd["features.99.weight"] = torch.zeros(1)
    torch.save(sd, path)
    with pytest.raises(ValueError, match="unexpected"):
        _quiet(load_init_checkpoint, dst, path)
    del sd["features.99.weight"], sd["features.0.0.weight"]
    torch.save(sd, path)
    with pytest.raises(ValueError, match="features.0.0.weight"):
        _quiet(load_init_checkpoint, dst, path)
    assert all(torch.equal(v, before[k]) for k, v in dst.state_dict().items())
