"""fp64 reference of one Adam / AdamW step - the update `eat_adam_multi` applies (csrc/train_glue.hip), elementwise on CPU
tensors, no chunking.  Names follow the kernel comment:

    g' = g * grad_scale (+ wd * p, Adam's L2 form);  AdamW: p *= 1 - lr * wd
    m = m + (1 - b1) (g' - m);  v = b2 v + (1 - b2) g'^2;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)

`t` is the step being taken (1 on a parameter's first update: torch's `state["step"]` after its increment).
`grad_scale` multiplies the gradient.  `adam_step_bound` is a first-order bound on how far an fp32 evaluation of the same
step (from the same fp32 inputs) may lie from this one."""
import math

import torch

U = 2.0 ** -24                    # unit round-off of fp32
SUBNORMAL_HALF_ULP = 2.0 ** -150  # absolute round-off of an fp32 result in the subnormal range


def adam_step(p, g, m, v, t, lr, beta1, beta2, eps, weight_decay=0.0, decoupled=False, grad_scale=1.0):
    """One step from fp32 (or any) p, g, m, v; returns the float64 (p', m', v') and a dict of the intermediate terms."""
    p, g, m, v = (x.detach().to("cpu", torch.float64) for x in (p, g, m, v))
    lr, b1, b2, eps, wd = float(lr), float(beta1), float(beta2), float(eps), float(weight_decay)
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    step_size, bc2_sqrt = lr / bc1, math.sqrt(bc2)
    g1 = g * float(grad_scale)
    if decoupled:
        p_in = p * (1.0 - lr * wd)
    else:
        p_in = p
        if wd != 0.0:
            g1 = g1 + wd * p
    m1 = m + (1.0 - b1) * (g1 - m)
    v1 = b2 * v + (1.0 - b2) * g1 * g1
    denom = v1.sqrt() / bc2_sqrt + eps
    upd = step_size * m1 / denom
    p1 = p_in - upd
    terms = dict(p=p, g=g, m=m, g1=g1, p_in=p_in, denom=denom, upd=upd, step_size=step_size, bc2_sqrt=bc2_sqrt)
    return p1, m1, v1, terms


def adam_step_bound(p1, m1, v1, terms, beta1, beta2, decoupled=False, grad_scale=1.0, weight_decay=0.0):
    """Bounds (float64 tensors, elementwise) on |p' - p'_ref|, |m' - m'_ref|, |v' - v'_ref| for an fp32 evaluation of the
    step from the same fp32 inputs: each rounding contributes U times the magnitude of the term it rounds, propagated to
    first order through the later lines, and the sum is doubled (slack for second-order terms; still a few U relative to the
    magnitudes of the terms, so a kernel that drops a factor or a term of the update is far outside it)."""
    b1, b2, wd = float(beta1), float(beta2), float(weight_decay)
    p, g, m, g1 = terms["p"], terms["g"], terms["m"], terms["g1"]
    # g' = fl(g * s) [+ fl(. + wd p)]
    err_g = U * (g * float(grad_scale)).abs()
    if not decoupled and wd != 0.0:
        err_g = err_g + U * g1.abs()
    # m' = fma(fl(1 - b1), fl(g' - m), m): rounding of the weight, of the difference, of the fma
    err_m = (1.0 - b1) * (err_g + 2 * U * (g1.abs() + m.abs())) + U * m1.abs()
    # v' = fl32(b2 v + (1 - b2) g'^2) evaluated in fp64: one fp32 rounding (absolute below the normal range) + g's error
    err_v = U * v1.abs() + SUBNORMAL_HALF_ULP + (1.0 - b2) * (2 * g1.abs() * err_g + err_g * err_g)
    # denom = fl(sqrt(v')) / sqrt(bc2) + eps: |sqrt(a) - sqrt(b)| <= |a - b| / sqrt(b), + the sqrtf rounding
    sv = v1.sqrt()
    err_sqrt = torch.where(v1 > 0, err_v / sv.clamp_min(1e-300), err_v.sqrt()) + U * sv
    err_denom = err_sqrt / terms["bc2_sqrt"]
    denom = terms["denom"]
    err_upd = terms["step_size"] * err_m / denom + terms["upd"].abs() * err_denom / denom
    # p' = fl(fl(p * (1 - lr wd)) - upd)
    err_p = U * p1.abs() + err_upd + (U * terms["p_in"].abs() if decoupled else 0.0)
    return 2 * err_p, 2 * err_m, 2 * err_v
