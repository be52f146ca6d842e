"""The fused log-mel kernel (csrc/mel.hip, `eat_mel_fwd`) beyond its default geometry, against the fp64 oracle.

tests/test_gpu_parity.py pins the kernel at win 800 / hop 320 / 32 kHz / 128 mels and full-length clips.  Here: every
code path that only other inputs reach - clips so short that a frame reflects on both sides, T of 1 and 2, odd hops (fast
and edge frames alternating), other windows, sample rates and mel counts (partial 64-lane rounds, empty mel rows), masks at
the edges of both axes and across tile / block / lane-round boundaries, the fixed-shape tables of the captured trainers,
the large-LDS branches of the entry point, its argument checks and a wave at a 4-byte-aligned address.

Bars (those of test_gpu_parity.py::test_mel_matches_oracle, every cell of every clip compared, no exclusions):
    ref32 = oracle in fp32, exact = oracle in fp64, per clip
    e_hip = max|got - exact| <= 3 * max|ref32 - exact| + 2e-5      and      max|got - ref32| < 1e-4
Input: the noise and the AM-noise + tone clips of synth.parity_clips (energy in every band).
Each case prints its figures (`MELGEOM ...`, visible with pytest -s) before it asserts.
"""
import contextlib
import io

import numpy as np
import pytest
import torch

from oracle import eat_oracle as O
from oracle import synth
from tests import mel_cases as MC

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import _lib, ops  # noqa: E402
from efficientat_amd.preprocess import AugmentMelSTFT, band_table, kaldi_mel_basis  # noqa: E402

DEV = torch.device("cuda:0")
MASKED = np.float32(0.9)            # (0 + 4.5) / 5 in fp32


def _module(geom, train=False, **kw):
    g = MC.full_geom(geom)
    with contextlib.redirect_stdout(io.StringIO()):
        mel = AugmentMelSTFT(n_mels=g["n_mels"], sr=g["sr"], win_length=g["win_length"], hopsize=g["hopsize"],
                             fmin=g["fmin"], fmax=g["fmax"], freqm=0, timem=0, **kw).to(DEV)
    return mel.train() if train else mel.eval()


_WAVES = {}


def _wave(L, B=2, sr=32000):
    """(B, L): rows 0 and 4 (noise, AM noise + tone) of parity_clips, further seeds for B > 2."""
    key = (L, B, sr)
    if key not in _WAVES:
        rows = [synth.parity_clips(L, seed=100 + s, sr=sr)[[0, 4]] for s in range((B + 1) // 2)]
        _WAVES[key] = torch.cat(rows)[:B].contiguous()
    return _WAVES[key]


def _oracle(wave, geom, **kw):
    g = MC.full_geom(geom)
    g.update(kw)
    return O.mel_forward(wave, **g), O.mel_forward(wave, dtype=torch.float64, **g)


def _check(got, refs, label):
    """The two bars of the module docstring -> (worst e_hip / e_ref, worst |got - ref32|)."""
    ref32, exact = refs
    got = got.detach().cpu()
    assert got.shape == ref32.shape, (label, got.shape, ref32.shape)
    assert bool(torch.isfinite(got).all()), label
    e_hip = (got.double() - exact).abs().amax(dim=(1, 2))
    e_ref = (ref32.double() - exact).abs().amax(dim=(1, 2))
    d32 = (got - ref32).abs().amax(dim=(1, 2))
    ratio = float((e_hip / e_ref.clamp_min(1e-30)).max())
    print(f"MELGEOM {label} e_hip={float(e_hip.max()):.3e} e_ref={float(e_ref.max()):.3e} "
          f"ratio={ratio:.3f} d32={float(d32.max()):.3e}")
    assert torch.all(e_hip <= 3.0 * e_ref + 2e-5), (label, e_hip.tolist(), e_ref.tolist())
    assert float(d32.max()) < 1e-4, (label, d32.tolist())
    return ratio, float(d32.max())


def _launch(mel, x, tables=None, fmask=(0, 0), tmask=(0, 0), out=None):
    """ops.mel_fwd with the module's own (eval) tables unless others are given."""
    if tables is None:
        tables = mel._device_tables(mel.fmin, mel.fmax, x.device)
    else:
        mel._device_tables(mel.fmin, mel.fmax, x.device)            # twiddles
    return ops.mel_fwd(x, mel.window, mel._twiddle, *tables, mel.n_fft, mel.hopsize, mel.n_mels, fmask, tmask, out=out)


# ------------------------------------------------------------------------------------------------- geometries
@pytest.mark.parametrize("group,cid,L,B,geom", MC.ALL, ids=[f"{c[0]}-{c[1]}" for c in MC.ALL])
def test_mel_geometry_matches_fp64_oracle(group, cid, L, B, geom):
    g = MC.full_geom(geom)
    wave = _wave(L, B, g["sr"])
    mel = _module(geom)
    T = MC.frames(L, g["hopsize"])
    got = mel(wave.to(DEV))
    assert got.shape == (B, g["n_mels"], T)
    if cid in MC.EMPTY_ROWS:                            # the band_cnt == 0 path must really run in these cases
        cnt = mel._device_tables(mel.fmin, mel.fmax, DEV)[2].cpu()
        assert int((cnt == 0).sum()) >= 1, cnt.tolist()
    _check(got, _oracle(wave, geom), f"{group} {cid}")


def test_mel_out_buffer_in_trainer_layout():
    """out= as the (B, 1, n_mels, T) buffer the trainers hand in: filled completely, same bits as the allocating call."""
    L, B = 20481, 3
    wave = _wave(L, B)
    mel = _module({})
    x = wave.to(DEV)
    T = MC.frames(L, 320)
    out = torch.full((B, 1, 128, T), float("nan"), device=DEV)
    r = mel(x, out=out)
    assert r.data_ptr() == out.data_ptr() and r.shape == out.shape
    assert torch.equal(out[:, 0], mel(x))
    _check(out[:, 0], _oracle(wave, {}), "batch out_B1FT")


# ------------------------------------------------------------------------------------------------------ masks
_FM = [(0, 1), (127, 128), (63, 65), (0, 128)]
_TM = [(0, 1), (99, 100), (15, 17), (63, 65), (0, 100)]
MASK_CASES = ([(f, (0, 0)) for f in _FM] + [((0, 0), t) for t in _TM]
              + [((63, 65), (15, 17)), ((0, 1), (99, 100)), ((127, 128), (63, 65)), ((5, 5), (0, 0)), ((0, 0), (5, 5)),
                 ((5, 5), (5, 5))])


class _MaskRig:
    """L=32000 (T=100), 128 mels: the wave, the unmasked launches and both launchers, built once."""

    def __init__(self, n_mels=128):
        self.geom = dict(n_mels=n_mels)
        self.wave = _wave(32000)
        self.x = self.wave.to(DEV)
        self.mel = _module(self.geom)
        self.static = _module(self.geom)
        self.static.static_tables(DEV)
        self.static.stage_tables(self.static.fmin, self.static.fmax)
        self.launchers = {
            "ops": lambda f, t: _launch(self.mel, self.x, fmask=f, tmask=t),
            "static": lambda f, t: self.static.forward_static(self.x, fmask=f, tmask=t),
        }
        self.base = {k: fn((0, 0), (0, 0)).cpu() for k, fn in self.launchers.items()}

    def check(self, fmask, tmask):
        refs = _oracle(self.wave, self.geom, freq_mask=fmask, time_mask=tmask)
        n_mels, T = self.base["ops"].shape[1:]
        m = torch.zeros(n_mels, T, dtype=torch.bool)
        m[fmask[0]:fmask[1], :] = True
        m[:, tmask[0]:tmask[1]] = True
        assert int(m.sum()) == (fmask[1] - fmask[0]) * T + (tmask[1] - tmask[0]) * n_mels \
            - (fmask[1] - fmask[0]) * (tmask[1] - tmask[0])
        for name, fn in self.launchers.items():
            got = fn(fmask, tmask).cpu()
            _check(got, refs, f"masks {name} n_mels={n_mels} f={fmask} t={tmask}")
            assert bool((got[:, m].numpy() == MASKED).all()), (name, fmask, tmask)
            assert torch.equal(got[:, ~m], self.base[name][:, ~m]), (name, fmask, tmask)   # bit-identical elsewhere


_RIGS = {}


def _rig(n_mels):
    if n_mels not in _RIGS:
        _RIGS[n_mels] = _MaskRig(n_mels)
    return _RIGS[n_mels]


@pytest.mark.parametrize("fmask,tmask", MASK_CASES, ids=[f"f{f[0]}-{f[1]}_t{t[0]}-{t[1]}" for f, t in MASK_CASES])
def test_mel_masks_at_edges_and_boundaries(fmask, tmask):
    _rig(128).check(fmask, tmask)


def test_mel_mask_of_the_single_row_of_a_second_round():
    """65 mels: row 64 is the only row of the second 64-lane round."""
    _rig(65).check((64, 65), (0, 0))


# ---------------------------------------------------------------------------------------------- static tables
# (n_mels, a draw with the widest band of the jitter space (brute force, tests/test_host_cpu.py), the static P).  The
# width at one draw can differ by a pair between hosts (a filter's last non-zero is an fp32 value next to zero, and the
# host's log decides its sign), so only P is pinned.
STATIC = [(128, (0, 15952), 15), (40, (0, 15750), 40)]


@pytest.mark.parametrize("n_mels,widest,P", STATIC, ids=["mels128", "mels40"])
def test_mel_static_tables_match_dynamic_tables_and_oracle(n_mels, widest, P):
    """forward_static + stage_tables (fixed-shape table, band starts clamped to 512 - 2P) against the fp64 oracle and
    against the tight table of the same (fmin, fmax).  A wider table only adds zero weights in front of and behind a
    band - fmaf(0, p, acc) == acc for finite p - and keeps every start even, so the two must agree to the bit."""
    geom = dict(n_mels=n_mels)
    L = 20480
    wave = _wave(L)
    x = wave.to(DEV)
    mel = _module(geom, train=True)
    assert (mel.fmin_aug_range, mel.fmax_aug_range) == (10, 2000)
    dev_tables = mel.static_tables(DEV)
    assert mel._static["P"] == P and dev_tables[0].shape == (P, n_mels, 2)
    assert P - 2 <= band_table(kaldi_mel_basis(n_mels, 1024, 32000, *widest))[0].shape[0] <= P
    draws = [(0, 14001), (0, 16000), (9, 14001), (9, 16000), widest, (9, 14001)]
    results = {}
    for fmin, fmax in draws:
        mel.stage_tables(fmin, fmax)
        got = mel.forward_static(x)
        dyn = _launch(mel, x, tables=mel._device_tables(fmin, fmax, DEV))
        assert torch.equal(got, dyn), (fmin, fmax, float((got - dyn).abs().max()))
        _check(got, _oracle(wave, geom, fmin=float(fmin), fmax=float(fmax)), f"static n_mels={n_mels} ({fmin},{fmax})")
        results[(fmin, fmax)] = got.clone()
    # ring ordering: two tables staged back to back (two slots of the pinned ring, one device table) - the launch
    # that follows sees the second one
    a, b = (0, 16000), (9, 14001)
    assert not torch.equal(results[a], results[b])
    mel.stage_tables(*a)
    mel.stage_tables(*b)
    assert torch.equal(mel.forward_static(x), results[b])
    mel.stage_tables(*b)
    mel.stage_tables(*a)
    assert torch.equal(mel.forward_static(x), results[a])
    for _ in range(5):                                   # more stagings than the ring has slots
        mel.stage_tables(*b)
        mel.stage_tables(*a)
    mel.stage_tables(*b)
    assert torch.equal(mel.forward_static(x), results[b])


# ------------------------------------------------------------------------------------------------ LDS branches
def test_mel_large_lds_request_and_its_limit():
    L = 20480
    wave = _wave(L)
    x = wave.to(DEV)
    mel = _module({})
    basis = kaldi_mel_basis(128, 1024, 32000, mel.fmin, mel.fmax)
    tight = _launch(mel, x)
    _check(tight, _oracle(wave, {}), "lds tight")
    # 64 pairs x 128 mels: ~97 KB of LDS, more than the 64 KB a kernel gets without asking
    wide = tuple(t.to(DEV) for t in band_table(basis, pairs=64))
    assert wide[0].shape == (64, 128, 2)
    assert torch.equal(_launch(mel, x, tables=wide), tight)
    # 160 pairs: more than the 160 KB of a CU - an error code, and no launch
    huge = tuple(t.to(DEV) for t in band_table(basis, pairs=160))
    out = torch.full_like(tight, float("nan"))
    with pytest.raises(_lib.EatHipError, match="too large for LDS"):
        _launch(mel, x, tables=huge, out=out)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert torch.equal(_launch(mel, x), tight)          # and the small request still works afterwards


# --------------------------------------------------------------------------------------------- argument checks
def test_mel_argument_checks_raise_and_leave_the_kernel_usable():
    L = 1537
    wave = _wave(L)
    x = wave.to(DEV)
    mel = _module({})
    good = mel(x)
    _check(good, _oracle(wave, {}), "args valid")
    T = MC.frames(L, 320)

    def still_fine():
        assert torch.equal(mel(x), good)

    with pytest.raises(_lib.EatHipError, match="too short"):
        mel(x[:, :513].contiguous())
    still_fine()
    with pytest.raises(_lib.EatHipError, match="n_fft=1024"):
        _module({}, n_fft=512)(x)
    still_fine()
    with pytest.raises(_lib.EatHipError, match="n_mels=257"):
        _module(dict(n_mels=257))(x)
    still_fine()
    with pytest.raises(_lib.EatHipError, match="bad geometry"):
        _module(dict(win_length=1025))(x)
    still_fine()
    for bad in (torch.empty(2 * 128 * T - 1, device=DEV), torch.empty(2 * 128 * T + 1, device=DEV),
                torch.empty((2, 128, T), device=DEV, dtype=torch.float64),
                torch.empty((2, 128, T), device=DEV, dtype=torch.float16)):
        with pytest.raises(_lib.EatHipError, match="out must be"):
            mel(x, out=bad)
        still_fine()
    w2, st, cnt = mel._device_tables(mel.fmin, mel.fmax, DEV)
    for tables in ((w2[:, :127].contiguous(), st, cnt), (w2, st[:127], cnt), (w2, st, cnt[:127]),
                   _module(dict(n_mels=64))._device_tables(0.0, 15000.0, DEV)):
        with pytest.raises(_lib.EatHipError, match="band table"):
            _launch(mel, x, tables=tables)
        still_fine()
    # ops.mel_fwd derives T from L and hop, so a wrong T only reaches the entry point directly; it checks that itself
    scratch = torch.empty(2 * 128 * (T + 1), device=DEV)
    with pytest.raises(_lib.EatHipError, match="does not match"):
        _lib.call("eat_mel_fwd", x.data_ptr(), 2, L, mel.window.data_ptr(), 800, 1024, 320, mel._twiddle.data_ptr(),
                  w2.data_ptr(), st.data_ptr(), cnt.data_ptr(), 128, w2.shape[0], scratch.data_ptr(), T + 1, 0, 0, 0, 0,
                  ops._stream())
    still_fine()


# --------------------------------------------------------------------------------------------------- alignment
@pytest.mark.parametrize("L,B,hop", [(20480, 3, 320), (20481, 3, 320), (22050, 2, 441)],
                         ids=["evenL", "oddL", "oddhop"])
def test_mel_wave_at_a_4_byte_aligned_address(L, B, hop):
    """A contiguous (B, L) view that starts at an odd element of a flat buffer: the interior fast path loads (x[j], x[j+1])
    as one 8-byte word, which is only valid at an 8-byte-aligned ADDRESS - the kernel decides that per frame from the
    address, so such frames take the edge path and every bit stays the same."""
    geom = dict(hopsize=hop)
    wave = _wave(L, B)
    mel = _module(geom)
    aligned = wave.to(DEV)
    assert aligned.data_ptr() % 8 == 0
    flat = torch.zeros(B * L + 2, device=DEV)
    flat[1:1 + B * L] = aligned.reshape(-1)
    odd = flat[1:1 + B * L].view(B, L)
    assert odd.is_contiguous() and odd.data_ptr() % 8 == 4
    want = mel(aligned)
    got = mel(odd)
    assert torch.equal(got, want)
    _check(got, _oracle(wave, geom), f"align L={L} B={B} hop={hop}")
