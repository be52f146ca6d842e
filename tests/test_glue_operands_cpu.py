"""ops.kd_loss_fwd_bwd / ops.mixup_fwd refuse the operands their kernels cannot take - by name, from tensor metadata alone and
BEFORE the residency check of the batch, so every refusal is shown here with CPU tensors: no launch, no GPU.  (The kernels
read perm as int32 and teacher_idx as int64 and gather rows by them: a tensor of another type or length is an out-of-bounds
read.)  A well-formed CPU call passes all of them and stops at "must live on the GPU"."""
import pytest
import torch

from efficientat_amd import ops
from efficientat_amd._lib import EatHipError

B, C, N = 4, 6, 5


def _kd(**over):
    a = dict(logits=torch.zeros(B, C), y=torch.zeros(B, C), perm=torch.arange(B, dtype=torch.int32), lam=torch.ones(B),
             teacher=torch.full((N, C), 0.5), teacher_idx=torch.zeros(B, dtype=torch.int64), kd_lambda=0.1, sums=torch.zeros(3))
    a.update(over)
    return a


def _mix(**over):
    a = dict(x=torch.zeros(B, 2, 3), perm=torch.arange(B, dtype=torch.int32), lam=torch.ones(B))
    a.update(over)
    return a


KD_REFUSALS = [
    ("logits", dict(logits=torch.zeros(B * C))),
    ("logits", dict(logits=torch.zeros(B, C, 1))),
    ("y", dict(y=torch.zeros(B, C + 1))),
    ("y", dict(y=torch.zeros(C, B))),
    ("y", dict(y=torch.zeros(B * C))),
    ("perm", dict(perm=torch.arange(B))),                                     # int64: what torch.randperm returns
    ("perm", dict(perm=torch.arange(B + 1, dtype=torch.int32))),
    ("perm", dict(perm=torch.arange(2 * B, dtype=torch.int32)[::2])),
    ("lam", dict(lam=torch.ones(B - 1))),
    ("lam", dict(lam=torch.ones(B, dtype=torch.float64))),
    ("lam", dict(lam=torch.ones(2 * B)[::2])),
    ("perm and lam", dict(perm=None)),
    ("perm and lam", dict(lam=None)),
    ("teacher", dict(teacher=torch.zeros(N, C + 1))),                         # a table of another width
    ("teacher", dict(teacher=torch.zeros(0, C))),
    ("teacher", dict(teacher=torch.zeros(N * C))),
    ("teacher", dict(teacher=torch.zeros(N, C, dtype=torch.float64))),
    ("teacher", dict(teacher=torch.zeros(C, N).t())),
    ("teacher_idx", dict(teacher_idx=torch.zeros(B, dtype=torch.int32))),
    ("teacher_idx", dict(teacher_idx=torch.zeros(B + 1, dtype=torch.int64))),
    ("teacher_idx", dict(teacher_idx=torch.zeros(2 * B, dtype=torch.int64)[::2])),
    ("teacher_idx", dict(teacher_idx=None)),                                  # required: teacher given, kd_lambda < 1
    ("teacher_idx", dict(teacher=None, teacher_idx=torch.zeros(B, dtype=torch.int32))),
    ("sums", dict(sums=torch.zeros(2))),
    ("sums", dict(sums=torch.zeros(3, dtype=torch.float64))),
    ("sums", dict(sums=torch.zeros(6)[::2])),
    ("kd_lambda", dict(kd_lambda=-0.01)),
    ("kd_lambda", dict(kd_lambda=1.01)),
    ("kd_lambda", dict(kd_lambda=float("nan"))),
]


@pytest.mark.parametrize("name,over", KD_REFUSALS, ids=[f"{n}-{i}" for i, (n, _) in enumerate(KD_REFUSALS)])
def test_kd_loss_wrapper_refuses_by_operand_name(name, over):
    with pytest.raises(EatHipError, match=rf"kd_loss_fwd_bwd: {name}\b"):
        ops.kd_loss_fwd_bwd(**_kd(**over))


MIX_REFUSALS = [
    ("x", dict(x=torch.zeros(0, 3))),
    ("x", dict(x=torch.zeros(()))),
    ("perm", dict(perm=torch.arange(B))),
    ("perm", dict(perm=torch.arange(B - 1, dtype=torch.int32))),
    ("perm", dict(perm=torch.arange(2 * B, dtype=torch.int32)[::2])),
    ("perm", dict(perm=None)),
    ("lam", dict(lam=torch.ones(B + 1))),
    ("lam", dict(lam=torch.ones(B, dtype=torch.float16))),
    ("lam", dict(lam=None)),
]


@pytest.mark.parametrize("name,over", MIX_REFUSALS, ids=[f"{n}-{i}" for i, (n, _) in enumerate(MIX_REFUSALS)])
def test_mixup_wrapper_refuses_by_operand_name(name, over):
    with pytest.raises(EatHipError, match=rf"mixup_fwd: .*\b{name}\b"):
        ops.mixup_fwd(**_mix(**over))


@pytest.mark.parametrize("over", [dict(), dict(perm=None, lam=None), dict(teacher=None, teacher_idx=None),
                                  dict(teacher_idx=None, kd_lambda=1.0), dict(kd_lambda=0.0), dict(sums=torch.zeros(5))])
def test_a_well_formed_cpu_call_gets_as_far_as_the_residency_check(over):
    """The metadata checks come first AND pass: what stops a well-formed call on CPU tensors is the batch's device."""
    with pytest.raises(EatHipError, match="logits must live on the GPU"):
        ops.kd_loss_fwd_bwd(**_kd(**over))


def test_a_well_formed_cpu_mixup_gets_as_far_as_the_residency_check():
    with pytest.raises(EatHipError, match="x must live on the GPU"):
        ops.mixup_fwd(**_mix())
