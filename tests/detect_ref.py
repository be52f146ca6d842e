"""numpy / fp64 restatements of sound event detection (include/eat_detect.h, efficientat_amd/detection.py): the stitch of
overlapping windows, the running median with periodic reflection, the double-threshold event list and the frame-level head.
Plain loops over recordings, classes and frames; nothing here shares code with the package.

A recording table `rec` is a list of rows (first window, window count, goff, G)."""
import numpy as np


def stitch_ref(p, rec, Hf, T, wt):
    """p (N_w, K, Tp) logits -> prob (K, G_total) float64: prob[k, goff + g] = sum_q wt[j] s(p[first + q, k, j]) / sum_q wt[j],
    j = g - q Hf, over the recording's windows with 0 <= j < T.  A frame no window covers is NaN."""
    p = np.asarray(p, dtype=np.float64)
    wt = np.asarray(wt, dtype=np.float64)
    K = p.shape[1]
    G_total = sum(r[3] for r in rec)
    out = np.full((K, G_total), np.nan)
    for first, count, goff, G in rec:
        for g in range(G):
            num, den = np.zeros(K), 0.0
            for q in range(count):
                j = g - q * Hf
                if 0 <= j < T:
                    num += wt[j] / (1.0 + np.exp(-p[first + q, :, j]))
                    den += wt[j]
            if den > 0:
                out[:, goff + g] = num / den
    return out


def reflect_index(j, G):
    """rho(j): u = j mod 2 G; u if u < G else 2 G - 1 - u."""
    u = j % (2 * G)
    return u if u < G else 2 * G - 1 - u


def median_ref(x, rec, m):
    """Running median of odd width m along time of x (K, G_total), per row and per recording, sample i + d read at
    rho(i + d) of the recording -> the dtype of x: every output is one of the inputs."""
    x = np.asarray(x)
    assert m % 2 == 1 and m >= 1
    h = m // 2
    out = np.empty_like(x)
    for _, _, goff, G in rec:
        idx = np.array([[reflect_index(i + d, G) for d in range(-h, h + 1)] for i in range(G)])      # (G, m)
        seg = x[:, goff:goff + G]
        out[:, goff:goff + G] = np.sort(seg[:, idx], axis=2)[:, :, h]
    return out


def timeline_events(v, hi, lo, max_gap, min_len):
    """One timeline -> [(onset, offset)]: runs of v >= lo that reach hi; runs whose gap (end of one to start of the next) is
    at most max_gap frames are merged; merged events shorter than min_len are dropped.  A plain state machine."""
    runs, start, hit = [], None, False
    for i in range(len(v) + 1):
        active = i < len(v) and v[i] >= lo
        if active:
            if start is None:
                start, hit = i, False
            if v[i] >= hi:
                hit = True
        elif start is not None:
            if hit:
                runs.append((start, i))
            start = None
    merged = []
    for on, off in runs:
        if merged and on - merged[-1][1] <= max_gap:
            merged[-1] = (merged[-1][0], off)
        else:
            merged.append((on, off))
    return [(on, off) for on, off in merged if off - on >= min_len]


def events_ref(filt, rec, hi, lo, max_gap=0, min_len=0):
    """filt (K, G_total) float32 -> (ev_i (E, 4) int32: recording, class, onset, offset; peak (E,) float32; mean (E,) float64),
    sorted by (recording, class, onset).  hi, lo: K values each, compared as float32."""
    filt = np.asarray(filt, dtype=np.float32)
    K = filt.shape[0]
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float32), (K,))
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float32), (K,))
    ev, peak, mean = [], [], []
    for i, (_, _, goff, G) in enumerate(rec):
        for k in range(K):
            v = filt[k, goff:goff + G]
            for on, off in timeline_events(v, hi[k], lo[k], max_gap, min_len):
                ev.append((i, k, on, off))
                peak.append(v[on:off].max())
                s = 0.0
                for t in range(on, off):
                    s += float(v[t])
                mean.append(s / (off - on))
    return (np.asarray(ev, dtype=np.int32).reshape(-1, 4), np.asarray(peak, dtype=np.float32), np.asarray(mean, dtype=np.float64))


def frame_logits_ref(model, y):
    """The head of `model` on every time column of the frequency mean of y (B, C, F, T), in fp64 on the host -> (B, K, T)."""
    import torch
    import torch.nn.functional as F
    with torch.no_grad():
        xm = y.detach().double().cpu().mean(dim=2)                         # (B, C, T)
        cls = model.classifier
        if model.head_type == "mlp":
            w1, b1, w2, b2 = (t.detach().double().cpu() for t in (cls[2].weight, cls[2].bias, cls[5].weight, cls[5].bias))
            h = F.hardswish(torch.einsum("hc,bct->bht", w1, xm) + b1.view(1, -1, 1))
            return (torch.einsum("kh,bht->bkt", w2, h) + b2.view(1, -1, 1)).numpy()
        conv, bn = cls[0], cls[1]
        w = conv.weight.detach().double().cpu().flatten(1)
        z = torch.einsum("kc,bct->bkt", w, xm)
        g, b, mu, var = (t.detach().double().cpu().view(1, -1, 1) for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))
        return ((z - mu) / torch.sqrt(var + bn.eps) * g + b).numpy()
