"""numpy / fp64 torch restatements of include/eat_weak_sed.h for the weak-label SED tests; no tests here.

`clip_targets_brute` enumerates the samples of each crop window and looks them up in a per-class occupancy array of the
clip (no interval arithmetic).  `loss_autograd` is the loss exactly as the header defines it, in fp64 torch under autograd;
`loss_closed` is the closed-form gradient next to it, with the clamp passed straight through, the only form that is defined
on saturated rows.  tests/test_weak_sed_cpu.py holds one against the other where both are defined (|z| <= 8, P inside
(eps, 1 - eps)); the GPU tests compare the kernel with the closed form."""
import numpy as np
import torch

from tests.sed_ref import _mix, _slot_ok


# ---------------------------------------------------------------------------------------------------- clip targets
def _clip_activity(ev, lengths, K, i, st, L):
    occ = np.zeros((K, int(lengths[i])), dtype=bool)
    for c, on, off in ev:
        occ[c, on:off] = True
    return occ[:, st:st + min(int(lengths[i]) - st, L)].any(axis=1).astype(np.float64)      # every sample of the crop window


def _slots(idx, start, lengths, b):
    """-> (i0, i1, whether `sed_slot` accepts every slot in use) of sample b."""
    i0, i1 = int(idx[2 * b]), int(idx[2 * b + 1])
    return i0, i1, _slot_ok(i0, int(start[2 * b]), lengths) and (i1 == -1 or _slot_ok(i1, int(start[2 * b + 1]), lengths))


def framed_brute(lengths, idx, start, strong=None):
    """-> framed (B,) int32: every slot in use is accepted and names a clip with strong != 0 (None: every clip is strong)."""
    framed = np.zeros(len(idx) // 2, dtype=np.int32)
    for b in range(len(framed)):
        i0, i1, ok = _slots(idx, start, lengths, b)
        framed[b] = int(ok and all(strong is None or strong[i] != 0 for i in (i0, i1) if i != -1))
    return framed


def clip_targets_brute(events, eo, lengths, K, idx, start, mix, L, strong=None):
    """-> (w (B, K) float32, framed (B,) int32) of eat_sed_clip_targets; strong (N,) or None (every clip is strong)."""
    B = len(mix)
    w = np.zeros((B, K), dtype=np.float32)
    for b in range(B):
        i0, i1, ok = _slots(idx, start, lengths, b)
        if not ok:
            w[b] = np.nan
            continue
        a0 = _clip_activity(events[eo[i0]:eo[i0 + 1]], lengths, K, i0, int(start[2 * b]), L)
        if i1 == -1:
            w[b] = a0
        else:
            a1 = _clip_activity(events[eo[i1]:eo[i1 + 1]], lengths, K, i1, int(start[2 * b + 1]), L)
            w[b] = _mix(mix[b], a0, a1)
    return w, framed_brute(lengths, idx, start, strong)


def strong_vectors(n):
    """The `strong` operands the clip-target tests add to a case of n clips: mixed values, all ones, NULL."""
    mixed = (np.arange(n) % 3 != 1).astype(np.uint8)
    mixed[0] = 3 if n > 2 else mixed[0]                                         # (any non-zero value counts as strong)
    return {"mixed": mixed, "ones": np.ones(n, dtype=np.uint8), "null": None}


# ---------------------------------------------------------------------------------------------------- the fused loss
def _operands(z, y, w, framed, T, perm, lam):
    """fp64 torch operands over the columns t < T: (z, ty, tw, f (B,) bool)."""
    z = torch.as_tensor(np.asarray(z, dtype=np.float64))[:, :, :T]
    y = torch.as_tensor(np.asarray(y, dtype=np.float64))[:, :, :T]
    w = torch.as_tensor(np.asarray(w, dtype=np.float64))
    f = torch.as_tensor(np.asarray(framed) != 0)
    if perm is not None:
        pm = torch.as_tensor(np.asarray(perm, dtype=np.int64))
        l = torch.as_tensor(np.asarray(lam, dtype=np.float32).astype(np.float64))
        y = l.view(-1, 1, 1) * y + (1.0 - l.view(-1, 1, 1)) * y[pm]
        w = l.view(-1, 1) * w + (1.0 - l.view(-1, 1)) * w[pm]
        f = f & f[pm]
    return z, y, w, f


def _sigmoid(z):
    """(p, 1 - p) in the branch form of the kernels: no cancellation at either end."""
    e = torch.exp(-z.abs())
    a, b = 1.0 / (1.0 + e), e / (1.0 + e)
    return torch.where(z >= 0, a, b), torch.where(z >= 0, b, a), e


def loss_autograd(z, y, w, framed, T, perm=None, lam=None, weak_weight=1.0, eps=1e-7):
    """The loss as defined, fp64 torch, and d loss / d z by autograd -> (loss, L_f, L_c, dz (B, K, T), P (B, K))."""
    z, ty, tw, f = _operands(z, y, w, framed, T, perm, lam)
    z = z.clone().requires_grad_(True)
    B, K, _ = z.shape
    eps, ww = float(np.float32(eps)), float(np.float32(weak_weight))
    el = torch.clamp(z, min=0.0) - z * ty + torch.log1p(torch.exp(-z.abs()))
    n_f = K * T * int(f.sum())
    l_f = (el * f.view(B, 1, 1)).sum() / n_f if n_f else torch.zeros((), dtype=torch.float64)
    p = torch.sigmoid(z)
    s1, s2 = p.sum(dim=2), (p * p).sum(dim=2)
    P = torch.where(s1 > 0, s2 / s1, torch.zeros_like(s1))
    pc = P.clamp(eps, 1.0 - eps)
    l_c = (-(tw * torch.log(pc) + (1.0 - tw) * torch.log1p(-pc))).sum() / (B * K)
    loss = l_f + ww * l_c
    (dz,) = torch.autograd.grad(loss, z)
    return float(loss.detach()), float(l_f.detach()), float(l_c.detach()), dz.numpy(), P.detach().numpy()


def loss_closed(z, y, w, framed, T, Tp=None, Kp=None, perm=None, lam=None, weak_weight=1.0, eps=1e-7):
    """The closed form of the header -> dict(loss, frame, clip, dl (B, Kp, Tp), db (K), P (B, K)), numpy fp64."""
    z, ty, tw, f = _operands(z, y, w, framed, T, perm, lam)
    B, K, _ = z.shape
    Tp, Kp = T if Tp is None else Tp, K if Kp is None else Kp
    eps, ww = float(np.float32(eps)), float(np.float32(weak_weight))
    p, q, e = _sigmoid(z)
    el = torch.clamp(z, min=0.0) - z * ty + torch.log1p(e)
    fm = f.view(B, 1, 1).to(torch.float64)
    n_f = K * T * int(f.sum())
    l_f = float((el * fm).sum() / n_f) if n_f else 0.0
    s1, s2 = p.sum(dim=2), (p * p).sum(dim=2)
    live = s1 > 0
    safe = torch.where(live, s1, torch.ones_like(s1))
    P = torch.where(live, s2 / safe, torch.zeros_like(s1))
    pc = P.clamp(eps, 1.0 - eps)
    l_c = float((-(tw * torch.log(pc) + (1.0 - tw) * torch.log1p(-pc))).sum() / (B * K))
    g = ((pc - tw) / (pc * (1.0 - pc)) / safe / (B * K)).unsqueeze(2) * ((2.0 * p - P.unsqueeze(2)) * p * q)
    g = torch.where(live.unsqueeze(2), g, torch.zeros_like(g))
    d = ww * g
    if n_f:
        d = d + fm * (p - ty) / n_f
    dl = np.zeros((B, Kp, Tp), dtype=np.float64)
    dl[:, :K, :T] = d.numpy()
    return dict(loss=l_f + ww * l_c, frame=l_f, clip=l_c, dl=dl, db=dl[:, :K].sum(axis=(0, 2)), P=P.numpy())


# ---------------------------------------------------------------------------------------------------- a bank with weak clips
def weaken_bank(path, every=3):
    """Mark every `every`-th clip of a bank directory written by `sed_ref.synth_bank` weak (clips 1, 1 + every, ...): its
    events become one whole-clip event per class it holds, and strong.npy is written -> (strong, events, event_offsets)."""
    import os
    lengths = np.load(os.path.join(path, "lengths.npy"))
    events = np.load(os.path.join(path, "events.npy"))
    eo = np.load(os.path.join(path, "event_offsets.npy"))
    n = len(lengths)
    strong = np.ones(n, dtype=np.uint8)
    strong[1::every] = 0
    out, new_eo = [], [0]
    for i in range(n):
        mine = events[eo[i]:eo[i + 1]]
        if strong[i]:
            out.extend(tuple(int(v) for v in r) for r in mine)
        else:
            out.extend((int(c), 0, int(lengths[i])) for c in sorted(set(mine[:, 0].tolist())))
        new_eo.append(len(out))
    events = np.asarray(out, dtype=np.int32).reshape(-1, 3)
    new_eo = np.asarray(new_eo, dtype=np.int64)
    np.save(os.path.join(path, "events.npy"), events)
    np.save(os.path.join(path, "event_offsets.npy"), new_eo)
    np.save(os.path.join(path, "strong.npy"), strong)
    return strong, events, new_eo
