"""Audio embeddings from an MN / DyMN: a fixed-size vector per recording (scene embedding) or one vector every
`hop_ms` milliseconds (timestamp embeddings).

The original project advertises its models as embedding extractors but ships no embedding code, so the definition is
this module's.  A forward in eval mode with ``return_fmaps=True`` gives n_maps feature maps x_l (B, C_l, F_l, T_l): the
stem, every block and the last 1x1 conv (17 for the MobileNetV3 table).  An embedding has D = sum C_l components,
map l at [off_l, off_l + C_l):

scene embedding       e[b, off_l + c] = mean over (f, t) of x_l[b, c, f, t]
timestamp embeddings  the same mean over f and over the columns t of map l that belong to timestamp k (`segment_plan`)

Both are one launch of ``eat_embed_pool`` (include/eat_embed.h, csrc/embed.hip) per chunk of windows, for every map and
every timestamp at once; nothing is pooled on the host.  Recordings are cut into non-overlapping windows of
`clip_seconds` exactly as the long-recording tagger cuts them (`tagger.window_plan` with hop = window), and all
recordings of a call share one window table and ``AugmentMelSTFT.forward_windows``.
"""
import contextlib
import io
import math

import numpy as np
import torch

from . import ops
from .mn import get_model as get_mobilenet
from .preprocess import AugmentMelSTFT
from .tagger import _get_ensemble_model, load_waveform, window_plan
from .utils import NAME_TO_WIDTH


def segment_plan(T_mel, T_l, r_l, frame_ms, hop_ms=50.0, width_ms=160.0):
    """Which columns of each feature map belong to each timestamp -> (lo (n_maps, n) int32, hi (n_maps, n) int32,
    timestamps_ms (n,) float64), host only, all arithmetic in fp64.

    n = floor((T_mel - 1) frame_ms / hop_ms) + 1 and timestamps_ms[k] = k hop_ms.  Timestamp k is centred at mel frame
    m = k hop_ms / frame_ms and owns the frames [a, b) = [m - w / 2, m + w / 2), w = width_ms / frame_ms.  Column j of a
    map with cumulative time stride r is centred at mel frame j r (every conv of the trunk has an odd kernel and 'same'
    padding), and the segment is the set of columns whose centre lies in [a, b):
    lo = clamp(ceil(a / r), 0, T_l), hi = clamp(ceil(b / r), 0, T_l).  Where that set is empty (r > w on the deep maps,
    or a window that ends before the map does) it is the single nearest column
    j* = clamp(floor(m / r + 0.5), 0, T_l - 1).  Segments overlap wherever width_ms exceeds hop_ms and are never empty."""
    T_l, r_l = [int(t) for t in T_l], [float(r) for r in r_l]
    if T_mel < 1 or len(T_l) != len(r_l) or len(T_l) < 1 or min(T_l) < 1 or min(r_l) <= 0:
        raise ValueError(f"segment_plan: need T_mel >= 1 and one T_l >= 1 and one stride > 0 per map (got {T_mel}, {T_l}, {r_l})")
    if not (frame_ms > 0 and hop_ms > 0 and width_ms > 0):
        raise ValueError(f"segment_plan: frame_ms, hop_ms and width_ms must be positive (got {frame_ms}, {hop_ms}, {width_ms})")
    frame_ms, hop_ms, width_ms = float(frame_ms), float(hop_ms), float(width_ms)
    n = int(math.floor((T_mel - 1) * frame_ms / hop_ms)) + 1
    timestamps = np.arange(n, dtype=np.float64) * hop_ms
    m = timestamps / frame_ms
    half = 0.5 * (width_ms / frame_ms)
    a, b = m - half, m + half
    lo = np.empty((len(T_l), n), dtype=np.int32)
    hi = np.empty((len(T_l), n), dtype=np.int32)
    for l, (T, r) in enumerate(zip(T_l, r_l)):
        lo_l = np.clip(np.ceil(a / r), 0, T)
        hi_l = np.clip(np.ceil(b / r), 0, T)
        near = np.clip(np.floor(m / r + 0.5), 0, T - 1)
        empty = hi_l <= lo_l
        lo[l] = np.where(empty, near, lo_l)
        hi[l] = np.where(empty, near + 1, hi_l)
    return lo, hi, timestamps


def window_weights(lengths, W):
    """Windows per recording and their weights in the recording's scene embedding -> (counts list, weights (sum counts)
    float64).  A recording of n samples has the windows of `tagger.window_plan` with hop = window = W samples; window q
    holds valid_q = clamp(n - q W, 0, W) samples and weighs valid_q / W, normalised over the recording: valid_q / n.
    A recording of at most W samples is one zero-padded window of weight 1."""
    counts, weights = [], []
    for n in lengths:
        _, valid, _ = window_plan(int(n), W, W, 1)
        w = valid.astype(np.float64) / W
        counts.append(len(valid))
        weights.append(w / w.sum())
    return counts, np.concatenate(weights)


def model_maps(model):
    """(C_l, r_l) of the feature maps that `model._forward_impl(x, return_fmaps=True)` returns in eval mode: channel counts
    and cumulative time strides - the stem's stride, doubled at each block whose depthwise conv has stride 2
    (`dw_stride`: a dilated tail keeps stride 1)."""
    if not callable(getattr(model, "_forward_impl", None)):
        raise TypeError(f"EmbeddingExtractor needs a model with _forward_impl(x, return_fmaps=True) returning "
                        f"(logits, feature maps) - an efficientat_amd MN or DyMN; {type(model).__name__} has none")
    if hasattr(model, "features"):                       # MN
        stem, blocks, last = model.features[0], list(model.features[1:-1]), model.features[-1]
    elif hasattr(model, "layers") and hasattr(model, "in_c"):       # DyMN
        stem, blocks, last = model.in_c, list(model.layers), model.out_c
    else:
        raise TypeError(f"EmbeddingExtractor needs a model with _forward_impl(x, return_fmaps=True) and the stem / block "
                        f"/ last-conv layout of an efficientat_amd MN or DyMN; {type(model).__name__} has another")
    stride = stem[0].stride
    r = int(stride[1] if isinstance(stride, (tuple, list)) else stride)
    channels, strides = [stem[0].out_channels], [r]
    for blk in blocks:
        r *= int(blk.dw_stride)
        channels.append(blk.cnf.out_channels)
        strides.append(r)
    channels.append(last.out_channels)
    strides.append(r)
    return channels, strides


class EmbeddingExtractor:
    """Scene and timestamp embeddings of recordings of any length.  The arguments up to `n_mels` are those of
    `tagger.EATagger`; `window_size` / `hop_size` are the STFT window and hop in samples.

    model          an MN or DyMN (eval mode) instead of a released name; anything without
                   `_forward_impl(x, return_fmaps=True)` - an ensemble included - raises TypeError, a model in training
                   mode ValueError
    batch_windows  windows per mel + forward + pooling chunk
    layers         "all", or a list of feature-map indices (0 = stem, 1..15 = blocks, 16 = last conv): the embedding is
                   the concatenation of the chosen maps' channel means, in the given order
    clip_seconds   length of the non-overlapping windows a recording is cut into"""

    def __init__(self, model_name=None, ensemble=None, device="cuda", sample_rate=32000, window_size=800, hop_size=320,
                 n_mels=128, *, model=None, batch_windows=64, layers="all", clip_seconds=10.0):
        if not torch.cuda.is_available():
            raise RuntimeError("EmbeddingExtractor needs a GPU: efficientat_amd has no CPU path")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device == "cuda" else torch.device(device)
        self._sample_rate, self.window_size, self.hop_size, self.n_mels = sample_rate, window_size, hop_size, n_mels
        if not 1 <= batch_windows <= 65535:
            raise ValueError(f"batch_windows must lie in [1, 65535] (got {batch_windows})")
        self.batch_windows, self.clip_seconds = int(batch_windows), float(clip_seconds)
        given = model is not None
        if model is not None:
            self.model = model
        elif ensemble is not None:
            self.model = _get_ensemble_model(ensemble)
        elif model_name is not None:
            self.model = get_mobilenet(width_mult=NAME_TO_WIDTH(model_name), pretrained_name=model_name)
        else:
            raise ValueError("Please provide a model name or an ensemble of models")
        channels, strides = model_maps(self.model)
        if given and self.model.training:
            raise ValueError("EmbeddingExtractor needs the model in eval mode (model.eval()): the feature maps of a training "
                             "forward depend on the batch")
        self.model.to(self.device)
        self.model.eval()
        if isinstance(layers, str):
            if layers != "all":
                raise ValueError(f"layers must be 'all' or a list of feature-map indices (got '{layers}')")
            self.layers = list(range(len(channels)))
        else:
            self.layers = [int(i) for i in layers]
            if len(self.layers) < 1 or any(not 0 <= i < len(channels) for i in self.layers):
                raise ValueError(f"layers must name feature maps in [0, {len(channels)}) (got {list(layers)})")
        self._channels = [channels[i] for i in self.layers]
        self._strides = [strides[i] for i in self.layers]
        self._n_maps = len(channels)
        self.W = int(self.clip_seconds * sample_rate)
        if self.W < 1:
            raise ValueError(f"clip_seconds={clip_seconds} is shorter than one sample")
        self.T_mel = 1 + (self.W - 1) // hop_size
        self.frame_ms = 1000.0 * hop_size / sample_rate
        with contextlib.redirect_stdout(io.StringIO()):          # (the "FMAX is None" notice of the constructor)
            self.mel = AugmentMelSTFT(n_mels=n_mels, sr=sample_rate, win_length=window_size, hopsize=hop_size)
        self.mel.to(self.device)
        self.mel.eval()

    # -- host-only ---------------------------------------------------------------------------------------------------
    @property
    def sample_rate(self):
        return self._sample_rate

    @property
    def scene_embedding_size(self):
        return sum(self._channels)

    @property
    def timestamp_embedding_size(self):
        return sum(self._channels)

    def load_waveform(self, audio_path):
        """`tagger.load_waveform` at this extractor's sample rate, on its device."""
        return load_waveform(audio_path, self._sample_rate, self.device)

    def _flatten(self, waves):
        if torch.is_tensor(waves) and waves.dim() == 2:
            waves = list(waves)
        if len(waves) == 0:
            raise ValueError("no recordings")
        ts = [torch.as_tensor(w, dtype=torch.float32).reshape(-1) for w in waves]
        lengths = [int(t.numel()) for t in ts]
        if min(lengths) < 1:
            raise ValueError("an empty recording")
        flat = torch.cat([t.to(self.device) for t in ts]) if len(ts) > 1 else ts[0].to(self.device).contiguous()
        return flat, lengths

    # -- device ------------------------------------------------------------------------------------------------------
    def _pool_windows(self, flat, lengths, plan):
        """Every window of every recording through mel, forward and ONE pooling launch per chunk of `batch_windows` ->
        (emb (N_total, n_seg, D), window counts, valid samples per window).  plan: None = the scene segment (0, T_l), or a
        function of the maps' widths -> (lo, hi)."""
        if self.model.training:
            raise ValueError("EmbeddingExtractor needs the model in eval mode (model.eval())")
        offsets, valids, counts, base = [], [], [], 0
        for n in lengths:
            s, v, _ = window_plan(n, self.W, self.W, 1)
            offsets.append(s + base)                             # hop = window: every window starts inside its recording
            valids.append(v)
            counts.append(len(s))
            base += n
        valids = np.concatenate(valids)
        d_start, d_valid = (t.to(self.device) for t in ops.check_windows(np.concatenate(offsets), valids, self.W, flat.numel()))
        n_total, emb, tables = int(d_start.numel()), None, None
        with torch.no_grad():
            for q0 in range(0, n_total, self.batch_windows):
                q1 = min(q0 + self.batch_windows, n_total)
                spec = self.mel.forward_windows(flat, d_start[q0:q1], d_valid[q0:q1], self.W)
                fmaps = self.model._forward_impl(spec.unsqueeze(1), return_fmaps=True)[1]
                if len(fmaps) != self._n_maps:
                    raise RuntimeError(f"the model returned {len(fmaps)} feature maps, its layout promises {self._n_maps}")
                fmaps = [fmaps[i].contiguous() for i in self.layers]
                if [m.shape[1] for m in fmaps] != self._channels:
                    raise RuntimeError("the feature maps' channel counts differ from the model's layout")
                if tables is None:
                    widths = [m.shape[3] for m in fmaps]
                    if plan is None:
                        tables = (np.zeros((len(fmaps), 1), dtype=np.int32), np.asarray(widths, dtype=np.int32).reshape(-1, 1))
                    else:
                        tables = plan(widths)
                    emb = torch.empty((n_total, tables[0].shape[1], sum(self._channels)), device=self.device, dtype=torch.float32)
                ops.embed_pool(fmaps, tables[0], tables[1], out=emb[q0:q1])
        return emb, counts, valids

    def scene_embeddings(self, waves):
        """waves: (B, L) tensor or list of 1-D waveforms of any lengths at `sample_rate` -> (B, D) fp32 on the device.  A
        recording's embedding is the mean of its windows' scene embeddings weighted by the share of the window that the
        recording fills (`window_weights`); a recording of at most `clip_seconds` is one zero-padded window."""
        flat, lengths = self._flatten(waves)
        emb, counts, _ = self._pool_windows(flat, lengths, None)
        emb = emb[:, 0, :]
        if max(counts) == 1:
            return emb
        _, weights = window_weights(lengths, self.W)
        # (recordings x windows) weight matrix, block diagonal: one small GEMM instead of a host loop over recordings
        mix = np.zeros((len(counts), emb.shape[0]), dtype=np.float32)
        row = 0
        for i, c in enumerate(counts):
            mix[i, row:row + c] = weights[row:row + c]
            row += c
        return torch.from_numpy(mix).to(self.device) @ emb

    def timestamp_embeddings(self, waves, hop_ms=50.0, width_ms=160.0):
        """-> per recording (emb (n_i, D) fp32 device tensor, timestamps_ms (n_i,) numpy float64): one embedding every hop_ms,
        each the mean over the feature-map columns within width_ms around it (`segment_plan`).  The plan is that of a full
        window; window q's timestamps are offset by q clip_seconds 1000, and of a recording's last window only the
        timestamps centred on a mel frame that the recording reaches (frame < 1 + (valid - 1) // hop_size) are kept.
        Pooling does NOT cross window boundaries: a timestamp near a window's edge averages only the columns of its own
        window.  clip_seconds 1000 must be a multiple of hop_ms."""
        clip_ms = self.clip_seconds * 1000.0
        ratio = clip_ms / float(hop_ms) if hop_ms > 0 else 0.0
        if hop_ms <= 0 or abs(ratio - round(ratio)) > 1e-9 or round(ratio) < 1:
            raise ValueError(f"clip_seconds * 1000 = {clip_ms} must be a multiple of hop_ms = {hop_ms}")
        flat, lengths = self._flatten(waves)
        stamps = []

        def plan(widths):
            lo, hi, t = segment_plan(self.T_mel, widths, self._strides, self.frame_ms, hop_ms, width_ms)
            stamps.append(t)
            return lo, hi

        emb, counts, valids = self._pool_windows(flat, lengths, plan)
        t_ms = stamps[0]
        n = len(t_ms)
        centre = t_ms / self.frame_ms
        out, row = [], 0
        for c in counts:
            frames = 1 + (int(valids[row + c - 1]) - 1) // self.hop_size
            keep = int(np.count_nonzero(centre < frames))
            total = (c - 1) * n + keep
            times = (np.arange(c, dtype=np.float64)[:, None] * clip_ms + t_ms[None, :]).reshape(-1)[:total]
            out.append((emb[row:row + c].reshape(c * n, -1)[:total], times))
            row += c
        return out
