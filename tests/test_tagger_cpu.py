"""Host side of the long-recording tagger (efficientat_amd/tagger.py): the window table against a literal emulation of the
reference's pad-then-slice loop, the resampler's FIR and output length against scipy, the closed form that
`eat_resample_mono` evaluates against `scipy.signal.resample_poly`, and the second header include/eat_tag.h."""
import ctypes
import math
import os

import numpy as np
import pytest
from scipy.signal import firwin, resample_poly

from efficientat_amd import _lib, build, ops, tagger

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SR = 32000


def _reference_windows(n_samples, window_size_s, hop_length_s, sr=SR):
    """windowed_inference.py:93-103 on a waveform of ones: pad with zeros, slice -> [(start, end, valid samples)]."""
    waveform = np.ones(n_samples, dtype=np.float32)
    window_size = int(window_size_s * sr)
    hop_length = int(hop_length_s * sr)
    n_windows = int(np.ceil((waveform.shape[0] - window_size) / hop_length)) + 1
    waveform = np.pad(waveform, (0, n_windows * hop_length + window_size - waveform.shape[0]))
    out = []
    for i in range(n_windows):
        start = i * hop_length
        end = start + window_size
        piece = waveform[start:end]
        assert piece.shape[0] == window_size
        valid = int(piece.sum())
        assert bool((piece[:valid] == 1).all()) and bool((piece[valid:] == 0).all())      # the zeros are a tail
        out.append((start, end, valid))
    return out


# 50000 at window 0.5 s / hop 1.0 s: ceil(34000 / 32000) = 2 hops, and the third window starts at 64000 >= 50000: with a
# hop H > window W the last valid is 0 exactly when n_samples - W lies in ((m - 1) H, m H - W] ... (m H - n <= 0), i.e. for
# n_samples in (W + (m - 1) H, m H]; 50000 lies in (48000, 64000].
@pytest.mark.parametrize("n_samples,win_s,hop_s", [(137600, 1.0, 0.75), (32000, 1.0, 0.75), (80000, 1.0, 0.75),
                                                   (100000, 0.5, 1.0), (50000, 0.5, 1.0), (64000, 0.5, 1.0),
                                                   (48000, 0.5, 1.0), (48001, 0.5, 1.0), (20000, 1.0, 0.75)])
def test_window_plan_is_the_reference_window_set(n_samples, win_s, hop_s):
    starts, valids, W = tagger.window_plan(n_samples, win_s, hop_s, SR)
    ref = _reference_windows(n_samples, win_s, hop_s)
    assert W == int(win_s * SR) and len(ref) >= 1
    assert [(int(s), int(s) + W, int(v)) for s, v in zip(starts, valids)] == ref
    assert starts.dtype == np.int64 and valids.dtype == np.int32


def test_window_plan_named_cases():
    starts, valids, W = tagger.window_plan(137600, 1.0, 0.75, SR)
    assert len(starts) == 6 and int(valids[-1]) == 17600 and list(valids[:5]) == [32000] * 5
    starts, valids, W = tagger.window_plan(32000, 1.0, 0.75, SR)
    assert list(starts) == [0] and list(valids) == [32000]
    starts, valids, W = tagger.window_plan(80000, 1.0, 0.75, SR)
    assert (80000 - W) % 24000 == 0 and list(starts) == [0, 24000, 48000] and list(valids) == [32000] * 3
    starts, valids, W = tagger.window_plan(50000, 0.5, 1.0, SR)
    assert list(starts) == [0, 32000, 64000] and list(valids) == [16000, 16000, 0]
    starts, valids, W = tagger.window_plan(48001, 0.5, 1.0, SR)            # one sample past the 0-valid range
    assert list(valids) == [16000, 16000, 0]
    starts, valids, W = tagger.window_plan(48000, 0.5, 1.0, SR)
    assert list(valids) == [16000, 16000]


def test_window_plan_tags_a_short_recording_as_one_padded_window():
    """OUR rule where the reference tags nothing: its n_windows = ceil((n - W) / H) + 1 is <= 0 for n <= W - H (8000 here).
    Between W - H and W (20000) the reference already pads one window, and the plan is that window."""
    assert _reference_windows(20000, 1.0, 0.75) == [(0, 32000, 20000)]
    starts, valids, W = tagger.window_plan(20000, 1.0, 0.75, SR)
    assert list(starts) == [0] and list(valids) == [20000] and W == 32000
    for n in (8000, 5000, 1):
        assert int(np.ceil((n - 32000) / 24000)) + 1 <= 0
        starts, valids, W = tagger.window_plan(n, 1.0, 0.75, SR)
        assert list(starts) == [0] and list(valids) == [n] and W == 32000
    assert _reference_windows(8001, 1.0, 0.75) == [(0, 32000, 8001)]
    with pytest.raises(ValueError, match="at least one sample"):
        tagger.window_plan(1000, 0.0, 1.0, SR)


RATES = [44100, 48000, 22050, 16000, 8000]


@pytest.mark.parametrize("src", RATES)
def test_resample_plan_is_the_filter_of_resample_poly(src):
    up, down, taps = tagger.resample_plan(src, SR)
    g = math.gcd(src, SR)
    assert (up, down) == (SR // g, src // g)
    half = 10 * max(up, down)
    h = firwin(2 * half + 1, 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    assert taps.numel() == 2 * half + 1 and taps.numel() % 2 == 1
    assert np.array_equal(taps.numpy(), h.astype(np.float32))
    assert tagger.resample_plan(src, SR)[2] is taps                       # designed once per rate pair
    for n_in in (1, 2, 441, 1000, 4411):
        assert ops.resampled_length(n_in, up, down) == len(resample_poly(np.zeros(n_in), up, down))


def _closed_form(m, up, down, h):
    """y[j] = sum_i m[i] h[j down - i up + half], the sum `eat_resample_mono` evaluates, in fp64 with the kernel's bounds."""
    half = (len(h) - 1) // 2
    n_out = -(-len(m) * up // down)
    y = np.zeros(n_out)
    for j in range(n_out):
        c = j * down
        lo = 0 if c - half <= 0 else (c - half + up - 1) // up
        hi = min((c + half) // up, len(m) - 1)
        i = np.arange(lo, hi + 1)
        t = c - i * up + half
        assert t.size == 0 or (t.min() >= 0 and t.max() < len(h))
        y[j] = float(np.dot(m[i], h[t]))
    return y


@pytest.mark.parametrize("src,n_in", [(44100, 1), (44100, 441), (44100, 1000), (48000, 999), (22050, 500), (16000, 300),
                                      (8000, 77)])
def test_the_resampler_sum_is_resample_poly(src, n_in):
    up, down, taps = tagger.resample_plan(src, SR)
    m = np.random.default_rng(src + n_in).uniform(-1, 1, n_in)
    h = firwin(taps.numel(), 1.0 / max(up, down), window=("kaiser", 5.0)) * up
    want = resample_poly(m, up, down)
    got = _closed_form(m, up, down, h)
    assert got.shape == want.shape
    assert float(np.abs(got - want).max()) < 1e-13                       # fp64 round-off of a reordered sum of <= 28 terms


_VOCABULARY = {ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_longlong}


def test_the_tag_header_parses_and_is_disjoint_from_the_main_header():
    P, I, LL = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong
    with open(os.path.join(ROOT, "include", "eat_tag.h")) as f:
        protos = _lib.parse_prototypes(f.read())
    assert protos == _lib.TAG_PROTOTYPES
    assert set(protos) == {"eat_mel_windows_fwd", "eat_tag_topk", "eat_resample_mono"}
    for name, (restype, args) in protos.items():
        assert set(args) <= _VOCABULARY and restype is I, name
    assert not set(protos) & set(_lib.PROTOTYPES)
    assert len(_lib.PROTOTYPES) == 139 and set(_lib.exported_symbols()) == set(_lib.PROTOTYPES)
    assert set(_lib.SIGNATURES) == set(_lib.PROTOTYPES)
    # order-sensitive literals, written from the header by hand
    assert protos["eat_mel_windows_fwd"][1] == [P, LL, P, P, I, I, P, I, I, I, P, P, P, P, I, I, P, I, P]
    assert protos["eat_tag_topk"][1] == [P, I, I, I, P, P, P, P]
    assert protos["eat_resample_mono"][1] == [P, I, LL, I, I, I, P, I, P, LL, P]


def test_the_library_exports_and_binds_the_tag_entry_points():
    build.build()
    h = _lib.lib()
    for name, (restype, args) in _lib.TAG_PROTOTYPES.items():
        fn = getattr(h, name)
        assert list(fn.argtypes) == args and fn.restype is restype, name
    assert "tag.hip" in build.SOURCES
    # argument checks that return before anything touches the device
    with pytest.raises(_lib.EatHipError, match="1 <= k <= min"):
        _lib.call("eat_tag_topk", None, 4, 10, 11, None, None, None, None)
    with pytest.raises(_lib.EatHipError, match="1 <= k <= min"):
        _lib.call("eat_tag_topk", None, 4, 100, 65, None, None, None, None)
    with pytest.raises(_lib.EatHipError, match="must be odd"):
        _lib.call("eat_resample_mono", None, 1, 441, 1, 320, 441, None, 8820, None, 320, None)
    with pytest.raises(_lib.EatHipError, match=r"ceil\(n_in \* up / down\) = 320"):
        _lib.call("eat_resample_mono", None, 1, 441, 1, 320, 441, None, 8821, None, 321, None)
    for bad in ((0, 441, 1), (320, 0, 1), (320, 441, 0)):
        with pytest.raises(_lib.EatHipError, match="need up, down, channels"):
            _lib.call("eat_resample_mono", None, 1, 441, bad[2], bad[0], bad[1], None, 8821, None, 320, None)
    with pytest.raises(_lib.EatHipError, match="at most 65535"):
        _lib.call("eat_mel_windows_fwd", None, 10, None, None, 65536, 9600, None, 800, 1024, 320, None, None, None, None,
                  128, 12, None, 30, None)
    with pytest.raises(_lib.EatHipError, match="bad geometry"):
        _lib.call("eat_mel_windows_fwd", None, 10, None, None, 0, 9600, None, 800, 1024, 320, None, None, None, None,
                  128, 12, None, 30, None)


def test_window_descriptors_are_validated_on_the_host():
    s, v = ops.check_windows([0, 5, 10], [4, 4, 0], 4, 10)
    assert s.dtype.is_floating_point is False and s.tolist() == [0, 5, 10] and v.tolist() == [4, 4, 0]
    for start, valid, match in (([0], [5], "valid length"), ([0], [-1], "valid length"), ([-1], [2], "outside the waveform"),
                                ([7], [4], "outside the waveform"), ([], [], "one .start, valid. pair"),
                                ([0, 1], [1], "one .start, valid. pair")):
        with pytest.raises(_lib.EatHipError, match=match):
            ops.check_windows(start, valid, 4, 10)
