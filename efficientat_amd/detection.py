"""Sound event detection with an MN / DyMN: WHEN each class sounds in a recording of any length.

The trunk's last feature map keeps a time axis, one column per r mel frames (r = 32: 320 ms at the default geometry),
and the heads are linear or pointwise over that axis before they pool it away.  `frame_logits` runs the head per column
instead: mean over frequency (`ops.freq_mean`), then the head's Linear layers as 1x1 convs over the time positions on the
MFMA conv kernels.  `EADetector` cuts every recording into overlapping windows whose length and hop are whole frames,
runs them in chunks through ``AugmentMelSTFT.forward_windows``, the model and `frame_logits` into one (N_w, K, Tp) logits
buffer, and then launches, once per call for all recordings and classes (include/eat_detect.h, csrc/detect.hip):

stitch   prob[k, g] = weighted mean over the windows that hold frame g of sigmoid(logit)      `ops.detect_stitch`
median   running median along time with reflection at the recording's own ends               `ops.detect_median`
         (widths that differ between classes: `ops.detect_median_bank`, include/eat_median_bank.h)
events   double-threshold binarisation, gap merging, minimum length -> sorted event list     `ops.detect_events`

Geometry (host, integers / fp64): R = r hop_size samples per frame (10240), frame_s = R / sample_rate; window W and
window hop Hs are positive multiples of R samples, T = W / R frames per window, Hf = Hs / R with 1 <= Hf <= T.  A
recording of n samples has G = ceil(n / R) frames, frame g centred at g frame_s (the column-centre convention of
`embeddings.segment_plan`), and windows at q Hs, q < n_w = 1 if n <= W else 1 + ceil((n - W) / Hs), window q holding
min(W, n - q Hs) samples and the rest zeros.  Column j of window q is frame q Hf + j; it exists iff that is < G.
"""
import contextlib
import io
from collections import namedtuple

import numpy as np
import torch

from . import mn as _mn
from . import ops
from .embeddings import model_maps
from .mn import get_model as get_mobilenet
from .preprocess import AugmentMelSTFT
from .tagger import load_waveform
from .utils import NAME_TO_WIDTH

MAX_MEDIAN = ops._DETECT_MAX_M

Geometry = namedtuple("Geometry", "r R frame_s W Hs T Hf")


def frame_geometry(r, hop_size, sample_rate, clip_seconds, hop_seconds):
    """-> Geometry(r, R, frame_s, W, Hs, T, Hf) of windows of clip_seconds every hop_seconds over a last map of cumulative
    time stride r.  Both lengths must be positive multiples of R = r hop_size samples and Hs <= W, else ValueError."""
    r, hop_size, sample_rate = int(r), int(hop_size), int(sample_rate)
    if r < 1 or hop_size < 1 or sample_rate < 1:
        raise ValueError(f"frame_geometry: need r, hop_size, sample_rate >= 1 (got {r}, {hop_size}, {sample_rate})")
    R = r * hop_size
    out = []
    for name, seconds in (("clip_seconds", clip_seconds), ("hop_seconds", hop_seconds)):
        samples = float(seconds) * sample_rate
        n = int(round(samples)) if np.isfinite(samples) else 0
        if n < 1 or abs(samples - n) > 1e-6 * max(1.0, abs(samples)) or n % R:
            raise ValueError(f"{name}={seconds} is {samples:.6g} samples at {sample_rate} Hz: it must be a positive multiple of "
                             f"R = {R} samples (one frame of the last feature map = {R / sample_rate:.6g} s)")
        out.append(n)
    W, Hs = out
    if Hs > W:
        raise ValueError(f"hop_seconds={hop_seconds} exceeds clip_seconds={clip_seconds}: the windows of R = {R} samples per "
                         f"frame would leave frames uncovered")
    return Geometry(r, R, R / sample_rate, W, Hs, W // R, Hs // R)


def frame_plan(n, geo):
    """Windows and frames of a recording of n samples -> (n_w, valid (n_w,) int64, G)."""
    n = int(n)
    if n < 1:
        raise ValueError("frame_plan: an empty recording")
    n_w = 1 if n <= geo.W else 1 + -(-(n - geo.W) // geo.Hs)
    valid = np.minimum(geo.W, n - np.arange(n_w, dtype=np.int64) * geo.Hs)
    return n_w, valid, -(-n // geo.R)


def ms_to_frames(ms, frame_s):
    """Milliseconds -> frames, rounded to nearest (halves up)."""
    ms = float(ms)
    if not np.isfinite(ms) or ms < 0:
        raise ValueError(f"a duration in ms must be finite and not negative (got {ms})")
    return int(np.floor(ms / (1000.0 * frame_s) + 0.5))


def median_frames(median_ms, frame_s):
    """Width of the median filter in frames: `ms_to_frames`, made odd by rounding up; outside [1, 31]: ValueError."""
    m = ms_to_frames(median_ms, frame_s)
    m += 1 - m % 2
    if not 1 <= m <= MAX_MEDIAN:
        raise ValueError(f"median_ms={median_ms} is {m} frames of {1000.0 * frame_s:.6g} ms: the filter takes 1 to {MAX_MEDIAN}")
    return m


def median_frames_per_class(median_ms, frame_s, K):
    """Per-class widths of the median filter in frames -> (K,) int32: `median_frames` of a scalar for every class, or of one
    value per class.  A value `median_frames` refuses: ValueError naming the class; another shape: ValueError."""
    ms = np.asarray(median_ms, dtype=np.float64)
    if ms.ndim == 0:
        return np.full(int(K), median_frames(float(ms), frame_s), dtype=np.int32)
    if ms.shape != (int(K),):
        raise ValueError(f"median_ms must be a scalar or hold one value per class, K = {int(K)} (got shape {ms.shape})")
    out = np.empty(int(K), dtype=np.int32)
    for k, v in enumerate(ms.tolist()):
        try:
            out[k] = median_frames(v, frame_s)
        except ValueError as e:
            raise ValueError(f"class {k}: {e}") from None
    return out


def thresholds(threshold, low_threshold, K):
    """-> (hi, lo) float32 numpy arrays of K values from scalars or length-K arrays; low_threshold None: lo = hi.
    0 < lo <= hi <= 1 in every class, else ValueError."""
    hi = np.asarray(threshold, dtype=np.float32)
    lo = hi if low_threshold is None else np.asarray(low_threshold, dtype=np.float32)
    out = []
    for name, v in (("threshold", hi), ("low_threshold", lo)):
        if v.ndim == 0:
            v = np.full(K, v, dtype=np.float32)
        if v.shape != (K,):
            raise ValueError(f"{name} must be a scalar or hold one value per class, K = {K} (got shape {v.shape})")
        out.append(np.ascontiguousarray(v))
    hi, lo = out
    if not bool(((lo > 0) & (lo <= hi) & (hi <= 1)).all()):
        raise ValueError("thresholds need 0 < low_threshold <= threshold <= 1 in every class")
    return hi, lo


# ---------------------------------------------------------------------------------------------------- frame-level head
def _head_packs(model):
    """Packed 1x1 layers of the frame-level head, kept in the dict of the model's `_FoldCache` (dropped with it on
    train() / eval() and on every change of a folded tensor) under their own key of the head tensors' versions and the
    EAT_PW_MODE in force."""
    W = model._cache.get(model._fold_sources(), model._build_folded)
    cls = model.classifier
    if model.head_type == "mlp":
        src = [cls[2].weight, cls[2].bias, cls[5].weight, cls[5].bias]
    else:
        src = [cls[0].weight, cls[1].weight, cls[1].bias, cls[1].running_mean, cls[1].running_var]
    key = (_mn._PW_MODE,) + tuple((t.data_ptr(), t._version) for t in src)
    hit = W.get("detect_head")
    if hit is not None and hit[0] == key:
        return hit[1]
    with torch.no_grad():
        if model.head_type == "mlp":
            w1, b1, w2, b2 = (t.detach().float() for t in src)
            H = w1.shape[0]
            Hp = ops.pitch4(H)                 # the second conv contracts over the hidden rows: C_in % 4 == 0
            if Hp != H:                        # zero rows (hswish(0) = 0) against zero columns: nothing changes
                w1 = torch.cat((w1, w1.new_zeros((Hp - H, w1.shape[1]))))
                b1 = torch.cat((b1, b1.new_zeros(Hp - H)))
                w2 = torch.cat((w2, w2.new_zeros((w2.shape[0], Hp - H))), dim=1)
            packs = ((_mn._pack_pw(w1.contiguous(), None, b1.contiguous()), Hp, ops.ACT_HSWISH),
                     (_mn._pack_pw(w2.contiguous(), None, b2.contiguous()), w2.shape[0], ops.ACT_NONE))
        else:
            if "fc_head" in W:
                wf, bf = W["fc_head"]
            else:
                s, b = _mn._fold(cls[0], cls[1])
                wf, bf = (cls[0].weight.flatten(1) * s.view(-1, 1)).contiguous(), b.contiguous()
            packs = ((_mn._pack_pw(wf, None, bf), wf.shape[0], ops.ACT_NONE),)
    W["detect_head"] = (key, packs)
    return packs


def check_model(model):
    """What `frame_logits` needs of a model -> (C of the last map, r of the last map, K classes).  TypeError for anything
    without `_forward_impl(x, return_fmaps=True)` (an ensemble included), ValueError for the attention-pooling head."""
    try:
        channels, strides = model_maps(model)
    except TypeError as e:
        raise TypeError(str(e).replace("EmbeddingExtractor", "detection")) from None
    head = getattr(model, "head_type", None)
    if head == "multihead_attention_pooling":
        raise ValueError("detection: the multihead_attention_pooling head has no frame-level logits (its attention is "
                         "normalised over the whole clip); use a model with the 'mlp' or 'fully_convolutional' head")
    if head == "mlp":
        K = model.classifier[5].out_features
    elif head == "fully_convolutional":
        K = model.classifier[0].out_channels
    else:
        raise ValueError(f"detection: head_type {head!r} has no frame-level plan ('mlp' and 'fully_convolutional' do)")
    return channels[-1], strides[-1], K


def frame_logits(model, y, out=None):
    """Frame-level logits of the last feature map y (B, C, F', T) of an eval `model._forward_impl(x, return_fmaps=True)`
    -> p (B, K, Tp), Tp = `ops.pitch4(T)`: the model's head applied to every time column of the frequency mean.

    mlp                  fc2 hswish(fc1 xm + b1) + b2 as two 1x1 convs over the Tp positions
    fully_convolutional  the folded conv + BatchNorm; linear, so the mean of p over the T columns is the clip logits
    Columns [T, Tp) of p hold the head's answer to a zero column: callers must not read them.  out: a contiguous fp32
    buffer of B K Tp elements to store into."""
    C, _, K = check_model(model)
    if model.training:
        raise ValueError("frame_logits needs the model in eval mode (model.eval()): the head of a training forward uses "
                         "batch statistics and dropout")
    if not isinstance(y, torch.Tensor) or y.dim() != 4 or y.shape[1] != C or y.numel() < 1:
        raise ValueError(f"frame_logits: y must be the model's last feature map (B, {C}, F, T), got "
                         f"{tuple(getattr(y, 'shape', ()))}")
    with torch.no_grad():
        y = y.contiguous().float()
        B = y.shape[0]
        xm = ops.freq_mean(y)
        Tp = xm.shape[2]
        x = xm.view(B, C, 1, Tp)
        packs = _head_packs(model)
        for pack, Co, act in packs[:-1]:
            x = _mn._pw(x, pack, Co, act)
        pack, Co, act = packs[-1]
        if out is None:
            out = torch.empty((B, K, Tp), device=y.device, dtype=torch.float32)
        ops.pw_conv_into(x, pack, Co, act, out)
    return out.view(B, K, Tp)


# ---------------------------------------------------------------------------------------------------- the detector
class EADetector:
    """Sound events of recordings of any length.  `window_size` / `hop_size` are the STFT window and hop in samples, as in
    `tagger.EATagger`.

    model          an MN or DyMN with the 'mlp' or 'fully_convolutional' head (eval mode) instead of a released name
    batch_windows  windows per mel + forward + head chunk
    clip_seconds   window length, hop_seconds: window hop; both whole multiples of one frame R / sample_rate (0.32 s)
    taper          weights of a window's columns where windows overlap: 'triangle' (min(j + 1, T - j): a column near a
                   window's edge has seen less context) or 'uniform'
    labels         list of class names; None: the class index names the event"""

    def __init__(self, model_name=None, *, model=None, device="cuda", sample_rate=32000, window_size=800, hop_size=320,
                 n_mels=128, batch_windows=64, clip_seconds=10.24, hop_seconds=5.12, taper="triangle", labels=None):
        if model is None and model_name is None:
            raise ValueError("Please provide a model name or a model")
        if not 1 <= batch_windows <= 65535:
            raise ValueError(f"batch_windows must lie in [1, 65535] (got {batch_windows})")
        given = model is not None
        if model is not None:
            C, r, K = check_model(model)
        if given and model.training:
            raise ValueError("EADetector needs the model in eval mode (model.eval()): the frame logits of a training forward "
                             "depend on the batch")
        if taper not in ("uniform", "triangle"):
            raise ValueError(f"taper must be 'uniform' or 'triangle' (got {taper!r})")
        if not given:
            if not torch.cuda.is_available():
                raise RuntimeError("EADetector needs a GPU: efficientat_amd has no CPU path")
            model = get_mobilenet(width_mult=NAME_TO_WIDTH(model_name), pretrained_name=model_name)
            C, r, K = check_model(model)
        self.geometry = frame_geometry(r, hop_size, sample_rate, clip_seconds, hop_seconds)
        if labels is not None and len(labels) != K:
            raise ValueError(f"labels holds {len(labels)} names, the model has {K} classes")
        if not torch.cuda.is_available():
            raise RuntimeError("EADetector needs a GPU: efficientat_amd has no CPU path")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device == "cuda" else torch.device(device)
        self.sample_rate, self.window_size, self.hop_size, self.n_mels = int(sample_rate), window_size, hop_size, n_mels
        self.batch_windows, self.taper, self.num_classes = int(batch_windows), taper, K
        self.labels = None if labels is None else list(labels)
        self.model = model
        self.model.to(self.device)
        self.model.eval()
        with contextlib.redirect_stdout(io.StringIO()):          # (the "FMAX is None" notice of the constructor)
            self.mel = AugmentMelSTFT(n_mels=n_mels, sr=sample_rate, win_length=window_size, hopsize=hop_size)
        self.mel.to(self.device)
        self.mel.eval()
        self._wt = torch.from_numpy(ops.detect_weights(self.geometry.T, taper).astype(np.float32)).to(self.device)

    # -- host-only ---------------------------------------------------------------------------------------------------
    @property
    def frame_s(self):
        return self.geometry.frame_s

    def load_waveform(self, audio_path):
        """`tagger.load_waveform` at this detector's sample rate, on its device."""
        return load_waveform(audio_path, self.sample_rate, self.device)

    def _flatten(self, waves):
        if torch.is_tensor(waves) and waves.dim() == 2:
            waves = list(waves)
        elif torch.is_tensor(waves) and waves.dim() == 1:
            waves = [waves]
        if len(waves) == 0:
            raise ValueError("no recordings")
        ts = [torch.as_tensor(w, dtype=torch.float32).reshape(-1) for w in waves]
        lengths = [int(t.numel()) for t in ts]
        if min(lengths) < 1:
            raise ValueError("an empty recording")
        flat = torch.cat([t.to(self.device) for t in ts]) if len(ts) > 1 else ts[0].to(self.device).contiguous()
        return flat, lengths

    def plan(self, lengths):
        """-> (window starts in the flat buffer (N_w,) int64, valid samples (N_w,), `ops.DetectTable`)."""
        geo, starts, valids, rows, base, first, goff = self.geometry, [], [], [], 0, 0, 0
        for n in lengths:
            n_w, valid, G = frame_plan(n, geo)
            starts.append(base + np.arange(n_w, dtype=np.int64) * geo.Hs)
            valids.append(valid)
            rows.append((first, n_w, goff, G))
            base, first, goff = base + n, first + n_w, goff + G
        return np.concatenate(starts), np.concatenate(valids), ops.detect_table(np.asarray(rows, dtype=np.int64))

    # -- device ------------------------------------------------------------------------------------------------------
    def window_logits(self, flat, starts, valids):
        """Every window through mel, forward and `frame_logits`, in chunks of `batch_windows` -> (N_w, K, Tp)."""
        if self.model.training:
            raise ValueError("EADetector needs the model in eval mode (model.eval())")
        geo = self.geometry
        d_start, d_valid = (t.to(self.device) for t in ops.check_windows(starts, valids, geo.W, flat.numel()))
        n_total, P = int(d_start.numel()), None
        with torch.no_grad():
            for q0 in range(0, n_total, self.batch_windows):
                q1 = min(q0 + self.batch_windows, n_total)
                spec = self.mel.forward_windows(flat, d_start[q0:q1], d_valid[q0:q1], geo.W)
                y = self.model._forward_impl(spec.unsqueeze(1), return_fmaps=True)[1][-1]
                if y.shape[3] != geo.T:
                    raise RuntimeError(f"the model's last feature map of a {geo.W}-sample window is {y.shape[3]} columns wide, "
                                       f"the frame plan promises T = {geo.T} (r = {geo.r})")
                if P is None:
                    P = torch.empty((n_total, self.num_classes, ops.pitch4(geo.T)), device=self.device, dtype=torch.float32)
                frame_logits(self.model, y, out=P[q0:q1])
        return P

    def timelines(self, waves, median=1):
        """-> (prob (K, G_total), filt (K, G_total) or None with median = 1, table, lengths): the stitched probabilities of
        all recordings side by side, and their running median of `median` frames: a scalar, or one odd width in [1, 31] per
        class.  Widths that are the same in every class run `ops.detect_median` (none at width 1); widths that differ run
        one `ops.detect_median_bank` of one slice, which copies the classes of width 1."""
        m = np.asarray(median)
        if m.ndim > 0:
            widths = ops.median_width_table(m, self.num_classes)             # (refuses a float, even or out-of-range width)
            median = int(m.flat[0]) if bool((m == m.flat[0]).all()) else None
        flat, lengths = self._flatten(waves)
        starts, valids, table = self.plan(lengths)
        table.dev(self.device)                                   # (uploaded ahead of the forward)
        P = self.window_logits(flat, starts, valids)
        prob = ops.detect_stitch(P, table, self.geometry.Hf, self.geometry.T, self._wt)
        if median is None:
            filt = ops.detect_median_bank(prob, table, widths)[0]
        else:
            filt = ops.detect_median(prob, table, median) if median != 1 else None
        return prob, filt, table, lengths

    def frame_probs(self, waves):
        """waves: (B, L) tensor or list of 1-D waveforms of any lengths at `sample_rate` -> per recording (probs (G, K) fp32
        device view of the shared timeline buffer, times_s (G,) float64 numpy: the frames' centres g frame_s)."""
        prob, _, table, _ = self.timelines(waves)
        out = []
        for _, _, goff, G in table.cpu.tolist():
            out.append((prob[:, goff:goff + G].t(), np.arange(G, dtype=np.float64) * self.geometry.frame_s))
        return out

    def detect(self, waves, threshold=0.5, low_threshold=None, median_ms=960, min_duration_ms=0, max_gap_ms=0):
        """-> per recording a list of (label or class index, onset_s, offset_s, peak, mean), sorted by class, then onset.
        threshold / low_threshold: scalars or one value per class (low_threshold None: the same as threshold); a run of
        frames at or above low_threshold is an event if it reaches threshold.  median_ms: a scalar or one value per class
        (`median_frames_per_class`; see `timelines`).  Runs at most max_gap_ms apart are merged,
        then events shorter than min_duration_ms are dropped; ms become frames by rounding to nearest, median_ms then odd
        by rounding up.  onset_s = onset frame_s; offset_s = min(offset R, n) / sample_rate: inside the recording."""
        geo = self.geometry
        hi, lo = thresholds(threshold, low_threshold, self.num_classes)
        m = median_frames(median_ms, geo.frame_s) if np.ndim(median_ms) == 0 else \
            median_frames_per_class(median_ms, geo.frame_s, self.num_classes)
        min_len, max_gap = ms_to_frames(min_duration_ms, geo.frame_s), ms_to_frames(max_gap_ms, geo.frame_s)
        d_hi, d_lo = torch.from_numpy(hi).to(self.device), torch.from_numpy(lo).to(self.device)
        prob, filt, table, lengths = self.timelines(waves, m)
        ev_i, ev_f = ops.detect_events(prob if filt is None else filt, table, d_hi, d_lo, max_gap, min_len)
        ev_i, ev_f = ev_i.cpu().numpy(), ev_f.cpu().numpy()                # the event list's one copy
        return self.event_lists(ev_i, ev_f, lengths)

    def event_lists(self, ev_i, ev_f, lengths):
        """(E, 4) / (E, 2) host arrays of `ops.detect_events` -> per recording the list `detect` returns."""
        geo, out = self.geometry, [[] for _ in lengths]
        for (i, k, on, off), (peak, mean) in zip(ev_i.tolist(), ev_f.tolist()):
            name = self.labels[k] if self.labels is not None else k
            out[i].append((name, on * geo.frame_s, min(off * geo.R, lengths[i]) / self.sample_rate, peak, mean))
        return out

    def detect_audio(self, path, **kw):
        """`detect` of one WAV file (decoded, down-mixed and resampled by `tagger.load_waveform`) -> its event list."""
        return self.detect([self.load_waveform(path)], **kw)[0]
