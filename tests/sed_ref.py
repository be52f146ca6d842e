"""numpy / fp64 restatements of include/eat_sed.h, of `mn_train.FrameHead` and of `sed.evaluate_frames`, for the SED tests.

The rasteriser of eat_sed_targets exists twice: `targets_brute` enumerates every output sample of every frame and looks its
source sample up in a per-class occupancy array of the clip (no interval arithmetic at all); `targets_closed` intersects
each event with the at most two runs of window positions a frame shows.  tests/test_sed_cpu.py holds one against the other;
the GPU tests compare the kernel with the brute force."""
import numpy as np
import torch
import torch.nn.functional as F


# ---------------------------------------------------------------------------------------------------- targets
def _mix(l32, a0, a1):
    """(float)(l a_0 + (1 - l) a_1) with l the fp32 mix value, the sum in fp64, rounded once."""
    l = np.float64(np.float32(l32))
    return np.float32(l * a0 + (1.0 - l) * a1)


def _slot_ok(i, st, lengths):
    return 0 <= i < len(lengths) and lengths[i] >= 1 and 0 <= st < lengths[i]


def _activity_brute(ev, lengths, K, i, st, sh, L, R, T):
    occ = np.zeros((K, int(lengths[i])), dtype=bool)
    for c, on, off in ev:
        occ[c, on:off] = True
    w = min(int(lengths[i]) - st, L)
    a = np.zeros((K, T), dtype=np.float64)
    for t in range(T):
        p = (np.arange(t * R, min((t + 1) * R, L), dtype=np.int64) - sh) % L   # every output sample of the frame
        p = p[p < w]
        if p.size:
            a[:, t] = occ[:, st + p].any(axis=1)
    return a


def _activity_closed(ev, lengths, K, i, st, sh, L, R, T):
    w = min(int(lengths[i]) - st, L)
    s = sh % L
    a = np.zeros((K, T), dtype=np.float64)
    for t in range(T):
        n0, n1 = t * R, min((t + 1) * R, L)
        if n0 >= n1:
            continue
        runs = [(max(n0, s) - s, min(n1 - s, w)), (n0 - s + L, min(min(n1, s) - s + L, w))]
        for c, on, off in ev:
            for lo, hi in runs:
                if lo < hi and on - st < hi and off - st > lo:
                    a[c, t] = 1.0
    return a


def _targets(activity, events, eo, lengths, K, idx, start, shift, mix, L, R, T, Tp):
    B = len(mix)
    y = np.zeros((B, K, Tp), dtype=np.float32)
    for b in range(B):
        i0, i1 = int(idx[2 * b]), int(idx[2 * b + 1])
        ok = _slot_ok(i0, int(start[2 * b]), lengths) and (i1 == -1 or _slot_ok(i1, int(start[2 * b + 1]), lengths))
        if not ok:
            y[b, :, :T] = np.nan
            continue
        a0 = activity(events[eo[i0]:eo[i0 + 1]], lengths, K, i0, int(start[2 * b]), int(shift[2 * b]), L, R, T)
        if i1 == -1:
            y[b, :, :T] = a0
        else:
            a1 = activity(events[eo[i1]:eo[i1 + 1]], lengths, K, i1, int(start[2 * b + 1]), int(shift[2 * b + 1]), L, R, T)
            y[b, :, :T] = _mix(mix[b], a0, a1)
    return y


def targets_brute(*a):
    return _targets(_activity_brute, *a)


def targets_closed(*a):
    return _targets(_activity_closed, *a)


def targets_windows(events, eo, lengths, K, L, R, T):
    """Frame activity (W, T, K) bool and frame counts (W,) of the non-overlapping windows of L samples that tile every clip,
    by enumeration: frame t of window q of clip i owns the clip's samples [q L + t R, min(q L + (t + 1) R, q L + L, length))."""
    rows, nf = [], []
    for i, n in enumerate(lengths):
        occ = np.zeros((K, int(n)), dtype=bool)
        for c, on, off in events[eo[i]:eo[i + 1]]:
            occ[c, on:off] = True
        for q in range(-(-int(n) // L)):
            valid = min(L, int(n) - q * L)
            a = np.zeros((T, K), dtype=bool)
            for t in range(T):
                lo, hi = q * L + t * R, min(q * L + min((t + 1) * R, L), int(n))
                if lo < hi:
                    a[t] = occ[:, lo:hi].any(axis=1)
            rows.append(a)
            nf.append(-(-valid // R))
    return np.stack(rows), np.asarray(nf, dtype=np.int64)


# ---------------------------------------------------------------------------------------------------- frame BCE
def sigmoid32(z):
    """The fp32 sigmoid of eat_detect_stitch, 1 / (1 + exp(-v)), in numpy fp32."""
    z = np.asarray(z, dtype=np.float32)
    with np.errstate(over="ignore"):
        return (np.float32(1.0) / (np.float32(1.0) + np.exp(-z, dtype=np.float32))).astype(np.float32)


def frame_bce(z, y, T, Kp, perm=None, lam=None, nframes=None):
    """fp64 restatement of eat_frame_bce_fwd_bwd on z, y (B, K, Tp) numpy -> (loss, dlogits (B, Kp, Tp), dbias (K))."""
    z, y = np.asarray(z, dtype=np.float64), np.asarray(y, dtype=np.float64)
    B, K, Tp = z.shape
    nb = np.full(B, T, dtype=np.int64) if nframes is None else np.clip(np.asarray(nframes, dtype=np.int64), 0, T)
    M = K * int(nb.sum())
    t = y
    if perm is not None:
        l = np.asarray(lam, dtype=np.float32).astype(np.float64).reshape(B, 1, 1)
        t = l * y + (1.0 - l) * y[np.asarray(perm)]
    live = (np.arange(Tp).reshape(1, 1, Tp) < nb.reshape(B, 1, 1)) & np.ones((B, K, Tp), dtype=bool)
    l_el = np.maximum(z, 0.0) - z * t + np.log1p(np.exp(-np.abs(z)))
    sg = np.where(z >= 0, 1.0 / (1.0 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1.0 + np.exp(-np.abs(z))))
    dl = np.zeros((B, Kp, Tp), dtype=np.float64)
    if M == 0:
        return 0.0, dl, np.zeros(K)
    dl[:, :K] = np.where(live, (sg - t) / M, 0.0)
    return float(np.where(live, l_el, 0.0).sum() / M), dl, dl[:, :K].sum(axis=(0, 2))


def frame_counts(z, y, thr, T, nframes=None):
    """(K, 3) int64 (tp, fp, fn) over the frames t < n_b: sigmoid32(z) >= thr[c] against y > 0.5."""
    B, K, Tp = z.shape
    nb = np.full(B, T, dtype=np.int64) if nframes is None else np.clip(np.asarray(nframes, dtype=np.int64), 0, T)
    live = np.broadcast_to(np.arange(Tp).reshape(1, 1, Tp) < nb.reshape(B, 1, 1), z.shape)
    p = sigmoid32(z) >= np.asarray(thr, dtype=np.float32).reshape(1, K, 1)
    g = np.asarray(y, dtype=np.float32) > 0.5
    return np.stack([(live & p & g).sum(axis=(0, 2)), (live & p & ~g).sum(axis=(0, 2)), (live & ~p & g).sum(axis=(0, 2))],
                    axis=1).astype(np.int64)


def midway_thresholds(z, T):
    """One threshold per class, midway between two adjacent distinct fp32 sigmoid values of that class's logits (columns
    < T), and the smallest |s - thr| over the class: a tie at the threshold would be undefined across sigmoid
    implementations."""
    B, K, _ = z.shape
    thr, gap = np.zeros(K, dtype=np.float32), np.inf
    for c in range(K):
        s = np.unique(sigmoid32(z[:, c, :T]).astype(np.float64))
        if len(s) < 2:
            thr[c] = np.float32(min(max(s[0] * 0.5, 1e-3), 1.0))
        else:
            j = len(s) // 2
            d = np.diff(s)
            j = min(max(j, 1), len(s) - 1)
            j = int(np.argmax(d[max(0, j - 3):j + 3]) + max(0, j - 3)) + 1   # the widest gap near the median
            thr[c] = np.float32(0.5 * (s[j - 1] + s[j]))
        gap = min(gap, float(np.abs(s - np.float64(thr[c])).min()))
    return thr, gap


# ---------------------------------------------------------------------------------------------------- hidden layer
def hswish_grad(u):
    """The derivative of eat_mlp_head_bwd: 0 below -3, u / 3 + 1 / 2 on [-3, 3], 1 above."""
    return np.where(u < -3.0, 0.0, np.where(u <= 3.0, u / 3.0 + 0.5, 1.0))


def hidden_fwd(z1, keep):
    z1 = np.asarray(z1, dtype=np.float64)
    k = 1.0 if keep is None else np.asarray(keep, dtype=np.float64)[:, :, None]
    return z1 * np.clip(z1 + 3.0, 0.0, 6.0) / 6.0 * k


def hidden_bwd(dh, z1, keep, H, T):
    dh, z1 = np.asarray(dh, dtype=np.float64), np.asarray(z1, dtype=np.float64)
    k = 1.0 if keep is None else np.asarray(keep, dtype=np.float64)[:, :, None]
    dz = dh * k * hswish_grad(z1)
    dz[:, H:] = 0.0
    dz[:, :, T:] = 0.0
    return dz, dz[:, :H].sum(axis=(0, 2))


# ---------------------------------------------------------------------------------------------------- the frame head
def head(y, w1, b1, w2, b2, keep=None):
    """The mlp head per time column of the frequency mean, torch, any dtype: y (B, C, F, T) -> frame logits (B, K, T)."""
    xm = y.mean(dim=2)                                                        # (B, C, T)
    h = F.hardswish(torch.einsum("hc,bct->bht", w1, xm) + b1.view(1, -1, 1))
    if keep is not None:
        h = h * keep.unsqueeze(2)
    return torch.einsum("kh,bht->bkt", w2, h) + b2.view(1, -1, 1)


def head_grads(y, w1, b1, w2, b2, keep, g):
    """fp64 autograd of `head` -> (logits, dy, dw1, db1, dw2, db2) for an upstream gradient g (B, K, T)."""
    ts = [t.detach().double().requires_grad_(True) for t in (y, w1, b1, w2, b2)]
    z = head(*ts, None if keep is None else keep.double())
    return (z.detach(),) + torch.autograd.grad(z, ts, g.double())


def frame_bce_torch(z, y):
    """Mean BCE-with-logits over every (b, c, t) of frame logits z against targets y (B, K, T), torch, any dtype."""
    return F.binary_cross_entropy_with_logits(z, y)


def oracle_frame_step(O, sd, x, y, keep, dtype):
    """One strong-label step under torch-CPU autograd over the oracle: the trunk's last feature map, `head` with the keep
    factor `keep` (B, H) and the frame BCE -> (loss, frame logits (B, K, T), {name: gradient})."""
    sdr = {k: (v.clone().to(dtype).requires_grad_(True) if v.is_floating_point() and "running" not in k
               else (v.clone().to(dtype) if v.is_floating_point() else v.clone())) for k, v in sd.items()}
    _, fmaps = O.mn_forward(sdr, x.to(dtype), train=True, stats={}, return_fmaps=True)
    z = head(fmaps[-1], sdr["classifier.2.weight"], sdr["classifier.2.bias"], sdr["classifier.5.weight"],
             sdr["classifier.5.bias"], keep.to(dtype))
    loss = frame_bce_torch(z, y.to(dtype))
    loss.backward()
    return loss.detach(), z.detach(), {k: v.grad for k, v in sdr.items() if getattr(v, "grad", None) is not None}


# ---------------------------------------------------------------------------------------------------- evaluation
def segment_scores(counts):
    """The definitions of `sed.segment_scores`, restated: micro from the summed counts, macro over the classes with a
    reference or a predicted segment, empty ratios 0."""
    c = np.asarray(counts, dtype=np.float64)
    out = {}
    tp, fp, fn = c.sum(0)
    out["micro_f1"] = 2 * tp / (2 * tp + fp + fn) if 2 * tp + fp + fn > 0 else float("nan")
    out["micro_precision"] = (tp / (tp + fp) if tp + fp > 0 else 0.0) if 2 * tp + fp + fn > 0 else float("nan")
    out["micro_recall"] = (tp / (tp + fn) if tp + fn > 0 else 0.0) if 2 * tp + fp + fn > 0 else float("nan")
    f, p, r = [], [], []
    for tp, fp, fn in c:
        if 2 * tp + fp + fn > 0:
            f.append(2 * tp / (2 * tp + fp + fn))
            p.append(tp / (tp + fp) if tp + fp > 0 else 0.0)
            r.append(tp / (tp + fn) if tp + fn > 0 else 0.0)
    for name, v in (("macro_f1", f), ("macro_precision", p), ("macro_recall", r)):
        out[name] = float(np.mean(v)) if v else float("nan")
    return out


# ---------------------------------------------------------------------------------------------------- a synthetic bank
def synth_bank(path, n_clips=12, K=5, sr=32000, seed=0, lo_s=0.5, hi_s=4.0):
    """Write a small strong-label bank directory: `n_clips` clips of lo_s .. hi_s seconds of tones and noise, up to 4 events
    per clip, one clip without events -> (lengths, events, event_offsets) as written."""
    import os
    rng = np.random.RandomState(seed)
    os.makedirs(path, exist_ok=True)
    lengths = rng.randint(int(lo_s * sr), int(hi_s * sr) + 1, size=n_clips).astype(np.int64)
    waves, events, eo = [], [], [0]
    for i, n in enumerate(lengths):
        t = np.arange(n) / sr
        x = 0.05 * rng.randn(n)
        mine = []
        for _ in range(0 if i == 3 else rng.randint(1, 5)):
            c = int(rng.randint(K))
            on = int(rng.randint(0, n - 1))
            off = int(min(n, on + rng.randint(1, max(2, n // 2))))
            x[on:off] += 0.3 * np.sin(2 * np.pi * (300.0 + 400.0 * c) * t[on:off])
            mine.append((c, on, off))
        events.extend(sorted(mine))
        eo.append(len(events))
        waves.append(x.astype(np.float32))
    events = np.asarray(events, dtype=np.int32).reshape(-1, 3)
    eo = np.asarray(eo, dtype=np.int64)
    np.save(os.path.join(path, "waves.npy"), np.concatenate(waves))
    np.save(os.path.join(path, "lengths.npy"), lengths)
    np.save(os.path.join(path, "events.npy"), events)
    np.save(os.path.join(path, "event_offsets.npy"), eo)
    with open(os.path.join(path, "names.txt"), "w") as f:
        f.write("\n".join(f"clip{i:02d}.wav" for i in range(n_clips)) + "\n")
    with open(os.path.join(path, "classes.txt"), "w") as f:
        f.write("\n".join(f"class{c}" for c in range(K)) + "\n")
    return lengths, events, eo


# ---------------------------------------------------------------------------------------------------- target cases
def _bank(clips, K):
    """[(length, [(class, on, off)])] -> (events (E, 3) int32, eo (N + 1) int64, lengths (N) int64, K)."""
    ev, eo, lengths = [], [0], []
    for n, mine in clips:
        ev.extend(sorted(mine))
        eo.append(len(ev))
        lengths.append(n)
    return np.asarray(ev, dtype=np.int32).reshape(-1, 3), np.asarray(eo, dtype=np.int64), np.asarray(lengths, dtype=np.int64), K


def _case(name, bank, rows, L, R, T, Tp):
    """rows: [(i0, start0, shift0, i1, start1, shift1, mix)] -> the operands of one eat_sed_targets call."""
    events, eo, lengths, K = bank
    B = len(rows)
    idx, start, shift = (np.zeros(2 * B, dtype=np.int32) for _ in range(3))
    mix = np.ones(B, dtype=np.float32)
    for b, (i0, s0, h0, i1, s1, h1, m) in enumerate(rows):
        idx[2 * b:2 * b + 2], start[2 * b:2 * b + 2], shift[2 * b:2 * b + 2], mix[b] = (i0, i1), (s0, s1), (h0, h1), m
    return dict(name=name, events=events, eo=eo, lengths=lengths, K=K, idx=idx, start=start, shift=shift, mix=mix, L=L, R=R,
                T=T, Tp=Tp)


def case_args(c):
    return (c["events"], c["eo"], c["lengths"], c["K"], c["idx"], c["start"], c["shift"], c["mix"], c["L"], c["R"], c["T"],
            c["Tp"])


def target_cases():
    """The smallest geometries at which the rasteriser can go wrong (R, L, T are arguments: none needs real audio).
    Small bank, R = 8: clip 0 fills L = 100 exactly - an event ending on a frame boundary (frame 2 stays 0), an event of one
    sample, two overlapping events of one class, an event at the clip's end that a roll wraps to the front; clip 1 is
    shorter than L (its padding stays 0 and rolls); clip 2 is longer (a crop leaves an event wholly outside); clip 3 has no
    events; clip 4 is one sample long."""
    small = _bank([(100, [(0, 8, 16), (1, 37, 38), (2, 10, 30), (2, 20, 50), (3, 95, 100)]),
                   (40, [(0, 0, 5), (4, 30, 40)]),
                   (250, [(1, 0, 20), (2, 120, 180), (3, 240, 250), (4, 99, 101)]),
                   (64, []),
                   (1, [(0, 0, 1)])], 5)
    L = 100
    rows = [(0, 0, 0, -1, 0, 0, 1.0), (0, 0, 1, -1, 0, 0, 1.0), (0, 0, -1, -1, 0, 0, 1.0),
            (0, 0, L - 1, -1, 0, 0, 1.0), (0, 0, -(L - 1), -1, 0, 0, 1.0), (0, 0, 10, -1, 0, 0, 1.0),      # (3, 95, 100) wraps
            (1, 0, 0, -1, 0, 0, 1.0), (1, 0, 70, -1, 0, 0, 1.0), (1, 0, -3, 0, 0, 5, 0.5),
            (2, 100, 0, -1, 0, 0, 1.0), (2, 0, 7, 1, 0, -20, np.float32(0.3)), (2, 150, -9, 3, 0, 0, 1.0),
            (3, 0, 13, -1, 0, 0, 1.0), (4, 0, 50, 2, 95, 0, 0.5), (3, 0, 0, 0, 0, 0, np.float32(0.3)),
            (99, 0, 0, -1, 0, 0, 1.0), (0, 0, 0, 77, 0, 0, 0.5), (0, 0, 3, -1, 0, 0, 1.0)]                 # rows 15, 16: NaN
    cases = [_case(f"R8-L100-rows{j}", small, rows[j:j + 3], 100, 8, 14, 16) for j in range(0, len(rows), 3)]
    cases.append(_case("R8-L100-B1", small, rows[5:6], 100, 8, 14, 16))
    rows64 = [(0, 0, 0, -1, 0, 0, 1.0), (2, 186, 63, 0, 36, -63, np.float32(0.3)), (1, 0, 33, 3, 0, 0, 0.5)]
    cases.append(_case("R8-L64", small, rows64, 64, 8, 8, 8))
    one = _bank([(100, [(0, 8, 16), (0, 12, 40), (0, 99, 100)]), (30, [])], 1)
    cases.append(_case("K1-B1", one, [(0, 0, -2, 1, 0, 0, np.float32(0.3))], 100, 8, 14, 16))
    rng = np.random.RandomState(4)
    clips = []
    for n in (327680, 100000, 500000):
        mine = [(0, 0, 1), (526, n - 1, n)]
        for _ in range(20):
            on = int(rng.randint(0, n - 1))
            mine.append((int(rng.randint(527)), on, int(min(n, on + rng.randint(1, 60000)))))
        clips.append((n, mine))
    big = _bank(clips, 527)
    Lb = 327680
    cases.append(_case("R10240-K527", big, [(0, 0, 4000, -1, 0, 0, 1.0), (2, 100000, -3999, 1, 0, 17, np.float32(0.3)),
                                            (1, 0, 0, 0, 0, -(Lb - 1), 0.5)], Lb, 10240, 32, 32))
    return cases
