"""The three kernels of the long-recording tagger (include/eat_tag.h) on their own.

eat_mel_windows_fwd   torch.equal with `eat_mel_fwd` on the materialised (zero-padded, sliced, contiguous) windows.  The
                      waveform is a view of a larger buffer whose other elements are NaN - one in front (the view starts
                      on an odd 4-byte word), three between the two recordings, and the buffer ends with the last sample -
                      and `out` is pre-filled with NaN: a read past `valid` or outside the buffer, or a row left unwritten,
                      turns the case red.
eat_tag_topk          probs within 1e-6 of the fp64 sigmoid (fp32 exp + divide on values <= 1 stays below 5e-7); index and
                      prob EQUAL to a stable numpy sort of the device's own probs by (descending p, ascending index).
eat_resample_mono     against `scipy.signal.resample_poly` in fp64 on the dequantised channel mean:
                      e_hip <= 3 e_ref32 + 1e-6, e_ref32 = scipy's own float32 run against fp64 (the form of the bar in
                      tests/test_gpu_mel_geometry.py).
Each case prints its figures (`TAGK ...`, visible with pytest -s) before it asserts.
"""
import contextlib
import io

import numpy as np
import pytest
import torch
from scipy.signal import resample_poly

from oracle import synth

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, ops, tagger  # noqa: E402
from efficientat_amd.preprocess import AugmentMelSTFT  # noqa: E402

DEV = torch.device("cuda:0")
NAN = float("nan")


# ------------------------------------------------------------------------------------------------- mel windows
N_A, GAP, N_B = 16803, 3, 10753          # recording A, NaN elements between the two, recording B
B0 = N_A + GAP                           # first sample of B in the view (even, A starts at 0; the VIEW starts on an odd word)
N_WAVE = B0 + N_B
L = 9600

_RIG = {}


def _rig():
    """-> (host waveform with NaN gap, device view at an odd element of a NaN buffer that ends with the last sample)."""
    if not _RIG:
        clips = synth.parity_clips(N_A + N_B, seed=11)
        host = torch.full((N_WAVE,), NAN)
        host[:N_A] = clips[0, :N_A]                           # noise
        host[B0:] = clips[4, N_A:]                            # AM noise + tone
        buf = torch.full((1 + N_WAVE,), NAN, device=DEV)
        buf[1:] = host.to(DEV)
        view = buf[1:]
        assert view.is_contiguous() and view.data_ptr() % 8 == 4 and view.numel() == N_WAVE
        _RIG.update(host=host, buf=buf, view=view, mels={})
    return _RIG


def _mel(n_mels=128, hop=320):
    mels = _rig()["mels"]
    if (n_mels, hop) not in mels:
        with contextlib.redirect_stdout(io.StringIO()):
            mels[(n_mels, hop)] = AugmentMelSTFT(n_mels=n_mels, hopsize=hop, freqm=0, timem=0).to(DEV).eval()
    return mels[(n_mels, hop)]


def _materialise(host, wins, length):
    x = torch.zeros((len(wins), length))
    for r, (s, v) in enumerate(wins):
        x[r, :v] = host[s:s + v]
    assert bool(torch.isfinite(x).all()), "the case itself reads a NaN: start / valid reach outside a recording"
    return x


FULL = L
MEL_CASES = {
    # (start, valid) in the view's coordinates
    "even_starts": [(0, FULL), (2400, FULL), (4800, FULL), (7200, FULL)],
    "odd_starts_H2401": [(0, FULL), (2401, FULL), (4802, FULL), (7203, FULL)],            # the last ends with recording A
    "tail_of_a_recording": [(9604, N_A - 9604), (12005, N_A - 12005), (7203, FULL)],
    "valid_inside_a_frame": [(0, 5000), (1, 5001), (2401, 4798), (2400, 1152), (2400, 1153), (3, 1152), (3, 1153),
                             (0, L - 1), (1, L - 1)],
    "valid_in_the_first_reflect_region": [(N_A - 300, 300), (N_A - 1, 1), (5, 511), (6, 512), (7, 513), (0, 2), (1, 2)],
    "valid_zero": [(N_A, 0), (0, 0), (N_WAVE, 0), (7203, FULL)],
    "two_recordings": [(7203, FULL), (B0, FULL), (B0 + 1153, FULL), (B0 + 1, 1152), (12005, N_A - 12005),
                       (B0 + 10000, 753), (B0 + 1001, 9600)],                               # B ends the buffer
}


@pytest.mark.parametrize("name", list(MEL_CASES))
def test_mel_windows_equal_mel_fwd_on_the_materialised_windows(name):
    rig, mel, wins = _rig(), _mel(), MEL_CASES[name]
    T = 1 + (L - 1) // 320
    out = torch.full((len(wins), 128, T), NAN, device=DEV)
    got = mel.forward_windows(rig["view"], [s for s, _ in wins], [v for _, v in wins], L, out=out)
    assert got.data_ptr() == out.data_ptr()
    want = mel(_materialise(rig["host"], wins, L).to(DEV))
    torch.cuda.synchronize()
    print(f"TAGK mel {name}: {len(wins)} windows, finite {bool(torch.isfinite(got).all())}, "
          f"max|diff| {float((got - want).abs().nan_to_num(nan=9e9).max()):.3e}")
    assert bool(torch.isfinite(got).all()), name
    assert torch.equal(got, want), name


@pytest.mark.parametrize("n_mels,hop,length", [(40, 441, L), (128, 320, 32000)], ids=["mels40_hop441", "two_blocks_T100"])
def test_mel_windows_other_geometry_and_more_than_one_block(n_mels, hop, length):
    """40 mels / hop 441 (fast and edge frames alternate, one partial 64-lane round); 1 s windows: T = 100 frames, two
    blocks along the time axis, the second one wholly past `valid` (both recordings are shorter than 1 s)."""
    rig, mel = _rig(), _mel(n_mels, hop)
    if length == L:
        wins = MEL_CASES["two_recordings"] + MEL_CASES["valid_inside_a_frame"][:4] + [(N_A, 0)]
    else:
        wins = [(0, N_A), (1, N_A - 1), (B0, N_B), (B0 + 1, 9999), (B0 + 10000, 753), (N_A, 0)]   # full ones: test_gpu_tagger.py
    T = 1 + (length - 1) // hop
    out = torch.full((len(wins), n_mels, T), NAN, device=DEV)
    got = mel.forward_windows(rig["view"], [s for s, _ in wins], [v for _, v in wins], length, out=out)
    want = mel(_materialise(rig["host"], wins, length).to(DEV))
    torch.cuda.synchronize()
    print(f"TAGK mel n_mels={n_mels} hop={hop} L={length}: max|diff| {float((got - want).abs().nan_to_num(nan=9e9).max()):.3e}")
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want)


def test_mel_windows_device_descriptors_and_even_view():
    """Descriptor tensors that already live on the device (slices of a validated table, as the tagger passes them), and the
    same windows through a view that starts on an EVEN word: the parity of every address flips, the bits do not."""
    rig, mel = _rig(), _mel()
    wins = MEL_CASES["two_recordings"] + MEL_CASES["odd_starts_H2401"]
    want = mel(_materialise(rig["host"], wins, L).to(DEV))
    s, v = ops.check_windows([s for s, _ in wins], [v for _, v in wins], L, N_WAVE)
    ds, dv = s.to(DEV), v.to(DEV)
    got = torch.cat([mel.forward_windows(rig["view"], ds[:5], dv[:5], L), mel.forward_windows(rig["view"], ds[5:], dv[5:], L)])
    assert torch.equal(got, want)
    even = torch.full((2 + N_WAVE,), NAN, device=DEV)
    even[2:] = rig["view"]
    assert even[2:].data_ptr() % 8 == 0
    assert torch.equal(mel.forward_windows(even[2:], s, v, L), want)


def test_mel_windows_argument_checks_raise():
    rig, mel = _rig(), _mel()
    good = mel.forward_windows(rig["view"], [0], [L], L)
    for start, valid, match in (([0], [L + 1], "valid length"), ([0], [-1], "valid length"), ([-2], [10], "outside the waveform"),
                                ([N_WAVE - 5], [6], "outside the waveform"), ([N_WAVE + 1], [0], "outside the waveform"),
                                ([0, 1], [L], "one .start, valid. pair")):
        with pytest.raises(_lib.EatHipError, match=match):
            mel.forward_windows(rig["view"], start, valid, L)
    with pytest.raises(_lib.EatHipError, match="too short"):
        mel.forward_windows(rig["view"], [0], [513], 513)
    with pytest.raises(_lib.EatHipError, match="flat"):
        mel.forward_windows(rig["view"][:2 * L].view(2, L), [0], [L], L)
    with pytest.raises(_lib.EatHipError, match="out must be"):
        mel.forward_windows(rig["view"], [0], [L], L, out=torch.empty(5, device=DEV))
    with pytest.raises(RuntimeError, match="evaluation only"):
        _mel().train().forward_windows(rig["view"], [0], [L], L)
    mel.eval()
    w2, st, cnt = mel._device_tables(mel.fmin, mel.fmax, DEV)
    s, v = (t.to(DEV) for t in ops.check_windows([0], [L], L, N_WAVE))
    scratch = torch.empty(128 * 31, device=DEV)

    def raw(n, length, t):
        _lib.call("eat_mel_windows_fwd", rig["view"].data_ptr(), N_WAVE, s.data_ptr(), v.data_ptr(), n, length,
                  mel.window.data_ptr(), 800, 1024, 320, mel._twiddle.data_ptr(), w2.data_ptr(), st.data_ptr(), cnt.data_ptr(),
                  128, w2.shape[0], scratch.data_ptr(), t, ops._stream())

    with pytest.raises(_lib.EatHipError, match="does not match"):
        raw(1, L, 31)
    with pytest.raises(_lib.EatHipError, match="at most 65535"):
        raw(65536, L, 30)
    with pytest.raises(_lib.EatHipError, match="bad geometry"):
        raw(0, L, 30)
    assert torch.equal(mel.forward_windows(rig["view"], [0], [L], L), good)      # still usable afterwards


# ------------------------------------------------------------------------------------------------------- top-k
def _logits(N, C, seed):
    rng = np.random.default_rng(seed)
    z = rng.uniform(-12.0, 12.0, (N, C)).astype(np.float32)
    extremes = np.array([50.0, -50.0, 88.0, -88.0], dtype=np.float32)[:max(0, min(4, C - 2))]
    z[0, C - len(extremes):] = extremes                                    # saturated probabilities: ties at 1 and near 0
    dup = 0 if N == 1 else 1
    if C >= 4:
        z[dup, C // 2:C // 2 + C // 4] = z[dup, :C // 4][::-1]             # exact duplicates, the copies at higher indices
    if N >= 3:
        z[2, :] = z[2, 0]                                                  # a row of equal values: index order alone
    return z


def _ranked(p, k):
    """Stable numpy sort of a row by (descending p, ascending index)."""
    order = np.lexsort((np.arange(p.shape[0]), -p.astype(np.float64)))
    return order[:k]


TOPK_CASES = sorted({(N, C, k) for C in (1, 10, 63, 64, 65, 527) for N in (1, 3) for k in (1, 10, min(C, 64)) if k <= C}
                    | {(9, 527, 10), (130, 20, 20)})                       # + a tail wave of the last block, + many blocks


@pytest.mark.parametrize("N,C,k", TOPK_CASES, ids=[f"N{n}_C{c}_k{k}" for n, c, k in TOPK_CASES])
def test_tag_topk_is_a_stable_sort_of_the_device_probabilities(N, C, k):
    z = _logits(N, C, seed=1000 * C + 10 * N + k)
    prob, index, probs = (t.cpu().numpy() for t in ops.tag_topk(torch.from_numpy(z).to(DEV), k, return_probs=True))
    exact = 1.0 / (1.0 + np.exp(-z.astype(np.float64)))
    e = float(np.abs(probs.astype(np.float64) - exact).max())
    print(f"TAGK topk N={N} C={C} k={k}: max|p - sigmoid64| {e:.3e}")
    assert probs.shape == (N, C) and prob.shape == (N, k) and index.shape == (N, k) and index.dtype == np.int32
    assert np.isfinite(probs).all() and e <= 1e-6
    for r in range(N):
        want = _ranked(probs[r], k)
        assert index[r].tolist() == want.tolist(), (r, index[r], want)
        assert np.array_equal(prob[r], probs[r][want]), r
    if N >= 3:
        assert index[2].tolist() == list(range(k))                          # all equal: ascending class index
    prob2, index2 = (t.cpu().numpy() for t in ops.tag_topk(torch.from_numpy(z).to(DEV), k))      # probs_all = NULL
    assert np.array_equal(index2, index) and np.array_equal(prob2, prob)


def test_tag_topk_argument_checks_raise():
    z = torch.zeros((2, 100), device=DEV)
    for k in (0, 65, 101):
        with pytest.raises(_lib.EatHipError, match="1 <= k <= min"):
            ops.tag_topk(z, k)
    with pytest.raises(_lib.EatHipError, match="1 <= k <= min"):
        ops.tag_topk(z[:, :5].contiguous(), 6)
    with pytest.raises(_lib.EatHipError, match=r"\(N, C\)"):
        ops.tag_topk(z[0], 1)
    with pytest.raises(_lib.EatHipError, match="must live on the GPU"):
        ops.tag_topk(z.cpu(), 1)


# --------------------------------------------------------------------------------------------------- resampler
def _frames(n_in, channels, i16, seed):
    rng = np.random.default_rng(seed)
    shape = (n_in, channels) if channels > 1 else (n_in,)
    if i16:
        data = rng.integers(-32768, 32768, shape).astype(np.int16)
        mono = data.astype(np.float64) / 32768.0
    else:
        data = rng.uniform(-1.0, 1.0, shape).astype(np.float32)
        mono = data.astype(np.float64)
    return data, (mono.mean(axis=1) if channels > 1 else mono)


def _resample_check(src, data, mono, label, tail=None):
    up, down, taps = tagger.resample_plan(src, 32000)
    got = ops.resample_mono(torch.from_numpy(data).to(DEV), up, down, taps.to(DEV)).cpu().numpy().astype(np.float64)
    exact = resample_poly(mono, up, down)
    ref32 = resample_poly(mono.astype(np.float32), up, down)
    assert ref32.dtype == np.float32 and got.shape == exact.shape, (got.shape, exact.shape)
    if tail:
        got, exact, ref32 = got[-tail:], exact[-tail:], ref32[-tail:]
    e_hip = float(np.abs(got - exact).max())
    e_ref = float(np.abs(ref32.astype(np.float64) - exact).max())
    print(f"TAGK resample {label}: n_out={got.shape[0]} e_hip={e_hip:.3e} e_ref32={e_ref:.3e}")
    assert np.isfinite(got).all()
    assert e_hip <= 3.0 * e_ref + 1e-6, (label, e_hip, e_ref)


RESAMPLE_CASES = ([(44100, n, ch, i16) for n in (1, 441, 1000, 4411) for ch, i16 in ((1, False), (2, True))]
                  + [(48000, 999, 1, False), (16000, 300, 1, False), (22050, 500, 1, False), (8000, 77, 3, False),
                     (44100, 1000, 1, True)])


@pytest.mark.parametrize("src,n_in,channels,i16", RESAMPLE_CASES,
                         ids=[f"{s}_n{n}_ch{c}_{'i16' if i else 'f32'}" for s, n, c, i in RESAMPLE_CASES])
def test_resample_mono_matches_resample_poly(src, n_in, channels, i16):
    data, mono = _frames(n_in, channels, i16, seed=src + n_in)
    _resample_check(src, data, mono, f"{src} n_in={n_in} ch={channels} i16={i16}")


def test_resample_mono_long_recording_needs_64_bit_indices():
    """160 s of mono int16 at 44.1 kHz (14 MB): the only size at which a 32-bit j * down wraps (5.12e6 x 441 > 2^31);
    compared on the last 2000 outputs."""
    data, mono = _frames(160 * 44100, 1, True, seed=5)
    assert (160 * 32000 - 1) * 441 > 2 ** 31
    _resample_check(44100, data, mono, "44100 160 s", tail=2000)


def test_resample_mono_argument_checks_raise():
    up, down, taps = tagger.resample_plan(44100, 32000)
    x = torch.zeros(441, device=DEV)
    t = taps.to(DEV)
    with pytest.raises(_lib.EatHipError, match="must be odd"):
        ops.resample_mono(x, up, down, t[:-1].contiguous())
    with pytest.raises(_lib.EatHipError, match="need up, down, channels"):
        ops.resample_mono(x, 0, down, t)
    with pytest.raises(_lib.EatHipError, match="need up, down, channels"):
        ops.resample_mono(x[:0], up, down, t)
    with pytest.raises(_lib.EatHipError, match="int16 / float32"):
        ops.resample_mono(x.double(), up, down, t)
    out = torch.empty(321, device=DEV)
    with pytest.raises(_lib.EatHipError, match="ceil"):
        _lib.call("eat_resample_mono", x.data_ptr(), 0, 441, 1, up, down, t.data_ptr(), t.numel(), out.data_ptr(), 321,
                  ops._stream())
