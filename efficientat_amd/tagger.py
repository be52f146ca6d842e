"""Batched long-recording tagger: the reference's ``windowed_inference.py`` (``EATagger.tag_audio_window``) without its
per-window host loop.

The reference decodes and resamples on the host, zero-pads a copy of the waveform and then, per window, runs one mel call,
one forward at batch 1, one sigmoid, one device->host copy and a numpy argsort.  Here every recording of a call goes into
one flat device buffer with one window table; the windows run in chunks of `batch_windows` through
``AugmentMelSTFT.forward_windows`` (``eat_mel_windows_fwd``: the zero tail is a property of the window descriptor, no padded
copy) and the model into one (N_total, C) logits buffer; one ``eat_tag_topk`` launch ranks all rows and one device->host
copy brings the result back.  Files at another sample rate are dequantised, down-mixed and resampled on the device
(``eat_resample_mono``, the `scipy.signal.resample_poly` of ``audio_io.load_audio``).

Deviations from the reference, all deliberate: fp32 throughout (no autocast, the project's stance everywhere); equal
probabilities rank by ascending class index (`np.argsort(p)[::-1]` leaves ties unspecified); a recording so short
that the reference computes n_windows <= 0 and tags nothing (at most window - hop samples) is tagged as one zero-padded
window; no host RNG draws.
"""
import contextlib
import importlib.util
import io
import math
import os

import numpy as np
import torch

from . import ops
from .mn import get_model as get_mobilenet
from .preprocess import AugmentMelSTFT
from .utils import NAME_TO_WIDTH

_HERE = os.path.dirname(os.path.abspath(__file__))
_PLANS = {}


def resample_plan(src_rate, dst_rate):
    """-> (up, down, taps): the rational factors of dst_rate / src_rate and the FIR of `scipy.signal.resample_poly(x, up,
    down)` (its default window ('kaiser', 5.0)), designed in fp64 and rounded to fp32 once per rate pair:
    taps = firwin(2 half + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up, half = 10 max(up, down)."""
    key = (int(src_rate), int(dst_rate))
    if key not in _PLANS:
        from scipy.signal import firwin
        if key[0] < 1 or key[1] < 1:
            raise ValueError(f"resample_plan: sample rates must be positive (got {key})")
        g = math.gcd(*key)
        up, down = key[1] // g, key[0] // g
        half = 10 * max(up, down)
        taps = firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
        _PLANS[key] = (up, down, torch.from_numpy(taps.astype(np.float32)))
    return _PLANS[key]


def window_plan(n_samples, window_size_s, hop_length_s, sample_rate=32000):
    """-> (starts, valids, W): window i covers samples [i H, i H + W) of the recording, of which valid_i =
    clamp(n_samples - i H, 0, W) exist and the rest read as zero; W = int(window_size_s sr), H = int(hop_length_s sr),
    n = max(1, ceil((n_samples - W) / H) + 1).  Wherever the reference tags anything this is its window set
    (windowed_inference.py:93-103: pad, then slice).  For a recording of at most W - H samples the reference computes
    n <= 0 and tags nothing; here it is tagged as ONE zero-padded window."""
    W, H = int(window_size_s * sample_rate), int(hop_length_s * sample_rate)
    if W < 1 or H < 1:
        raise ValueError(f"window_plan: window and hop must be at least one sample (got {W}, {H})")
    n = max(1, int(math.ceil((n_samples - W) / H)) + 1)
    starts = np.arange(n, dtype=np.int64) * H
    valids = np.clip(n_samples - starts, 0, W).astype(np.int32)
    return starts, valids, W


def load_waveform(audio_path, sample_rate, device):
    """WAV file -> mono fp32 waveform at `sample_rate` on the device: decoded on the host (scipy.io.wavfile), int16 and
    float32 frames uploaded as they are, other sample types converted to float32 as `audio_io.load_audio` does;
    dequantised, down-mixed and resampled on the device."""
    from scipy.io import wavfile
    src_sr, data = wavfile.read(audio_path)
    if data.dtype == np.uint8:
        data = (data.astype(np.float32) - 128.0) / 128.0
    elif data.dtype != np.int16 and np.issubdtype(data.dtype, np.integer):
        data = data.astype(np.float32) / float(2 ** (8 * data.dtype.itemsize - 1))
    elif data.dtype != np.int16:
        data = data.astype(np.float32)
    if data.shape[0] < 1:
        raise ValueError(f"{audio_path}: no audio frames")
    frames = torch.from_numpy(np.ascontiguousarray(data)).to(device)
    if src_sr == sample_rate and frames.dtype == torch.float32 and frames.dim() == 1:
        return frames                                        # nothing to do: no launch
    if src_sr == sample_rate:
        up, down, taps = 1, 1, torch.ones(1)                 # dequantise + down-mix alone: one tap of 1.0
    else:
        up, down, taps = resample_plan(src_sr, sample_rate)
    return ops.resample_mono(frames, up, down, taps.to(device))


def _get_ensemble_model(names):
    """`models.ensemble.get_ensemble_model` of the drop-in tree (dropin/models/ensemble.py), loaded by path: the drop-in
    tree is laid out to shadow the reference's top-level `models` package and is not itself a package."""
    path = os.path.join(_HERE, os.pardir, "dropin", "models", "ensemble.py")
    spec = importlib.util.spec_from_file_location("efficientat_amd._dropin_ensemble", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.get_ensemble_model(names)


class EATagger:
    """Tags long recordings window by window.  The first seven arguments are the reference's
    (windowed_inference.py:40-47); `window_size` / `hop_size` are the STFT window and hop in samples.

    model        any module whose forward(x) returns (logits, _) - MN, DyMN, EnsemblerModel - instead of a released name
    labels       list of class names; None: the class index is the tag name
    batch_windows  windows per mel + forward chunk
    top_k        tags per window (the reference lists 10)"""

    def __init__(self, model_name=None, ensemble=None, device="cuda", sample_rate=32000, window_size=800, hop_size=320,
                 n_mels=128, *, model=None, labels=None, batch_windows=64, top_k=10):
        if not torch.cuda.is_available():
            raise RuntimeError("EATagger needs a GPU: efficientat_amd has no CPU path")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device == "cuda" else torch.device(device)
        self.sample_rate, self.window_size, self.hop_size, self.n_mels = sample_rate, window_size, hop_size, n_mels
        if not 1 <= batch_windows <= 65535:
            raise ValueError(f"batch_windows must lie in [1, 65535] (got {batch_windows})")
        self.batch_windows, self.top_k = int(batch_windows), int(top_k)
        self.labels = None if labels is None else list(labels)
        if model is not None:
            self.model = model
        elif ensemble is not None:
            self.model = _get_ensemble_model(ensemble)
        elif model_name is not None:
            self.model = get_mobilenet(width_mult=NAME_TO_WIDTH(model_name), pretrained_name=model_name)
        else:
            raise ValueError("Please provide a model name or an ensemble of models")
        self.model.to(self.device)
        self.model.eval()
        with contextlib.redirect_stdout(io.StringIO()):          # (the "FMAX is None" notice of the constructor)
            self.mel = AugmentMelSTFT(n_mels=n_mels, sr=sample_rate, win_length=window_size, hopsize=hop_size)
        self.mel.to(self.device)
        self.mel.eval()

    # -- host-only ---------------------------------------------------------------------------------------------------
    def window_plan(self, n_samples, window_size_s, hop_length_s):
        """`window_plan` at this tagger's sample rate -> (starts, valids, W)."""
        return window_plan(n_samples, window_size_s, hop_length_s, self.sample_rate)

    # -- device ------------------------------------------------------------------------------------------------------
    def _tag_flat(self, flat, lengths, window_size, hop_length, return_probs):
        """flat: the recordings back to back in one fp32 device buffer, lengths: their sample counts."""
        starts, offsets, valids, counts, base = [], [], [], [], 0
        for n in lengths:
            s, v, W = self.window_plan(n, window_size, hop_length)
            starts.append(s)
            # a start beyond the recording's end (hop > window) belongs to a window with valid 0, which reads nothing:
            # it is anchored at the recording's first sample so that every descriptor points into the buffer
            offsets.append(np.where(v > 0, s + base, base))
            valids.append(v)
            counts.append(len(s))
            base += n
        d_start, d_valid = (t.to(self.device) for t in
                            ops.check_windows(np.concatenate(offsets), np.concatenate(valids), W, flat.numel()))
        n_total = int(d_start.numel())
        logits = None
        with torch.no_grad():
            for lo in range(0, n_total, self.batch_windows):
                hi = min(lo + self.batch_windows, n_total)
                spec = self.mel.forward_windows(flat, d_start[lo:hi], d_valid[lo:hi], W)
                out = self.model(spec.unsqueeze(1))[0].float()
                if logits is None:
                    logits = torch.empty((n_total, out.shape[1]), device=self.device, dtype=torch.float32)
                logits[lo:hi] = out
            ranked = ops.tag_topk(logits, min(self.top_k, logits.shape[1]), return_probs=return_probs)
        prob, index = ranked[0].cpu().numpy(), ranked[1].cpu().numpy()      # the one device->host copy (it synchronises)
        probs = ranked[2].cpu().numpy() if return_probs else None
        results, row = [], 0
        for s, n in zip(starts, counts):
            r = {"start": s / self.sample_rate, "end": (s + W) / self.sample_rate,
                 "index": index[row:row + n], "prob": prob[row:row + n]}
            if return_probs:
                r["probs"] = probs[row:row + n]
            results.append(r)
            row += n
        return results

    def tag_waveforms(self, waves, window_size=20.0, hop_length=10.0, return_probs=False):
        """waves: list of 1-D float tensors / arrays at `sample_rate` -> per recording a dict of `start`, `end` (n,) seconds,
        `index` (n, k) int32, `prob` (n, k) and, with return_probs, `probs` (n, C), n = the recording's windows."""
        if len(waves) == 0:
            return []
        ts = [torch.as_tensor(w, dtype=torch.float32).reshape(-1) for w in waves]
        lengths = [int(t.numel()) for t in ts]
        if min(lengths) < 1:
            raise ValueError("tag_waveforms: an empty recording")
        flat = torch.cat([t.to(self.device) for t in ts]) if len(ts) > 1 else ts[0].to(self.device).contiguous()
        return self._tag_flat(flat, lengths, window_size, hop_length, return_probs)

    def load_waveform(self, audio_path):
        """`load_waveform` at this tagger's sample rate, on its device."""
        return load_waveform(audio_path, self.sample_rate, self.device)

    def tag_audio_window(self, audio_path, window_size=20.0, hop_length=10.0):
        """The reference's call (windowed_inference.py:71-124) -> list of {'start', 'end', 'tags': [{'tag', 'probability'}
        x top_k]}, one entry per window."""
        wave = self.load_waveform(audio_path)
        r = self._tag_flat(wave, [int(wave.numel())], window_size, hop_length, False)[0]
        name = (lambda c: self.labels[c]) if self.labels is not None else (lambda c: c)
        return [{"start": float(s), "end": float(e),
                 "tags": [{"tag": name(int(c)), "probability": p} for c, p in zip(ci, pi)]}
                for s, e, ci, pi in zip(r["start"], r["end"], r["index"], r["prob"])]
