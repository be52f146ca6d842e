"""Sound event detection at model level (efficientat_amd/detection.py, detect.py) on small seeded random-init models with
perturbed BatchNorm statistics and 7 classes: the frame-level head against its fp64 restatement on the device's own feature
map, the detector end to end against the kernels called by hand and against tests/detect_ref.py, the command line, and the
launch list behind the trunk."""
import contextlib
import io
import json

import numpy as np
import pytest
import torch
from scipy.io import wavfile

from oracle import synth

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

import efficientat_amd.mn as mn_mod  # noqa: E402
from efficientat_amd import detect, detection, ops  # noqa: E402
from efficientat_amd.dymn import get_model as get_dymn  # noqa: E402
from efficientat_amd.mn import get_model  # noqa: E402
from tests import detect_ref as R  # noqa: E402

DEV = torch.device("cuda:0")
SR, K = 32000, 7
_CACHE = {}


def _model(name):
    """mn05 (mlp head), mn05_fc (fully_convolutional), dymn04 (mlp): random init, every BatchNorm's statistics and affine and
    the head's biases perturbed so that folding them matters."""
    if name not in _CACHE:
        torch.manual_seed(23)
        with contextlib.redirect_stdout(io.StringIO()):
            if name == "mn05":
                m = get_model(width_mult=0.5, num_classes=K, head_type="mlp")
            elif name == "mn05_fc":
                m = get_model(width_mult=0.5, num_classes=K, head_type="fully_convolutional")
            else:
                m = get_dymn(width_mult=0.4, num_classes=K)
        g = torch.Generator().manual_seed(29)
        with torch.no_grad():
            for mod in m.modules():
                if isinstance(mod, torch.nn.BatchNorm2d):
                    mod.running_mean.copy_(0.1 * torch.randn(mod.running_mean.shape, generator=g))
                    mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=g))
                    mod.weight.copy_(0.8 + 0.4 * torch.rand(mod.weight.shape, generator=g))
                    mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
            if m.head_type == "mlp":
                m.classifier[2].bias.copy_(0.1 * torch.randn(m.classifier[2].bias.shape, generator=g))
                m.classifier[5].bias.copy_(torch.linspace(-0.6, 0.6, K))
        _CACHE[name] = m.to(DEV).eval()
    return _CACHE[name]


def _last_map(model, B, T_mel, seed):
    x = torch.randn((B, 1, 128, T_mel), generator=torch.Generator().manual_seed(seed)).to(DEV)
    with torch.no_grad():
        logits, fmaps = model._forward_impl(x, return_fmaps=True)
    return logits, fmaps[-1]


# ------------------------------------------------------------------------------------------------ frame_logits
@pytest.mark.parametrize("pw_mode", ["fp32", "auto"])
@pytest.mark.parametrize("T_mel,T", [(30, 1), (300, 10), (1000, 32)])
@pytest.mark.parametrize("name", ["mn05", "mn05_fc", "dymn04"])
def test_frame_logits_against_fp64(name, T_mel, T, pw_mode, monkeypatch):
    """rel-L2 <= 2e-5 with EAT_PW_MODE=fp32 (the bar of tests/test_gpu_attn_head_kernels.py for the same conv path),
    |delta| <= 1e-3 in the default mode (the project's logit bar); the fully_convolutional head's column mean is the model's
    own clip logits within the same bars."""
    monkeypatch.setattr(mn_mod, "_PW_MODE", pw_mode)
    model = _model(name)
    for B in (1, 5):
        clip, y = _last_map(model, B, T_mel, seed=T_mel + B)
        assert y.shape[0] == B and y.shape[3] == T and bool(torch.isfinite(y).all())
        p = detection.frame_logits(model, y)
        Tp = ops.pitch4(T)
        assert p.shape == (B, K, Tp) and p.dtype == torch.float32 and p.is_cuda
        assert torch.equal(p, detection.frame_logits(model, y))
        buf = torch.full((B + 2, K, Tp), float("nan"), device=DEV)
        assert torch.equal(detection.frame_logits(model, y, out=buf[1:B + 1]), p)
        assert bool(torch.isnan(buf[0]).all()) and bool(torch.isnan(buf[B + 1]).all())
        want = R.frame_logits_ref(model, y)
        got = p[:, :, :T].double().cpu().numpy()
        rel = float(np.linalg.norm(got - want) / np.linalg.norm(want))
        err = float(np.abs(got - want).max())
        print(f"frame_logits {name} T={T} B={B} {pw_mode}: rel-L2 {rel:.3e}, max |delta| {err:.3e}, max |ref| {float(np.abs(want).max()):.3f}")
        assert bool(torch.isfinite(p).all())
        if pw_mode == "fp32":
            assert rel <= 2e-5
        else:
            assert err <= 1e-3
        if model.head_type == "fully_convolutional":
            mean = p[:, :, :T].double().mean(dim=2).cpu().numpy()
            ref = clip.double().cpu().numpy()
            rel_c, err_c = float(np.linalg.norm(mean - ref) / np.linalg.norm(ref)), float(np.abs(mean - ref).max())
            print(f"frame_logits {name} T={T} B={B} {pw_mode}: column mean vs clip logits rel-L2 {rel_c:.3e}, max |delta| {err_c:.3e}")
            if pw_mode == "fp32":
                assert rel_c <= 2e-5
            else:
                assert err_c <= 1e-3


def test_head_packs_live_in_the_models_fold_cache():
    model = _model("mn05")
    _, y = _last_map(model, 1, 300, seed=1)
    detection.frame_logits(model, y)
    W = model._cache.val
    packs = W["detect_head"][1]
    detection.frame_logits(model, y)
    assert model._cache.val["detect_head"][1] is packs                     # cached
    model.train()
    model.eval()                                                           # the fold cache is dropped: so are the head's packs
    _last_map(model, 1, 300, seed=1)
    assert "detect_head" not in model._cache.val
    p = detection.frame_logits(model, y)
    assert model._cache.val["detect_head"][1] is not packs
    with torch.no_grad():
        model.classifier[5].bias.add_(1.0)                                 # a version bump of a head tensor alone
    try:
        q = detection.frame_logits(model, y)
        assert float((q - p - 1.0)[:, :, :10].abs().max()) < 1e-5
    finally:
        with torch.no_grad():
            model.classifier[5].bias.sub_(1.0)


# ------------------------------------------------------------------------------------------------ end to end
def _recordings():
    clips = synth.parity_clips(800000, seed=77)                            # 25 s
    return [clips[1].clone(), clips[3][:100000].clone()]                   # ... and 3.1 s: shorter than one window


def _close(got, want):
    """Two forwards of one input differ by fp32 ulps of the activations (the trunk's squeeze-excitation sums are atomic): the
    bar tests/test_gpu_embed.py gives two runs of one computation, 2e-5 (|want| + mean |want|)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and bool((np.abs(got - want) <= 2e-5 * (np.abs(want) + np.abs(want).mean())).all())


@pytest.mark.parametrize("taper", ["triangle", "uniform"])
def test_detector_is_its_kernels_called_by_hand(taper, monkeypatch):
    """`frame_probs` is torch.equal to `ops.detect_stitch` called by hand on the detector's own logits buffer, and the mel of
    the windows is torch.equal to the mel of the materialised (sliced, zero-padded) windows.  The trunk between the two is
    run by hand on the same chunks as well, but two forwards of one input are not bit-identical by contract (the
    squeeze-excitation sums of the eval plan are atomic), so that leg is held to `_close` and its bit-equality is printed
    (measured: bit-equal on both tapers).  `detect` is `events_ref` on the device's own filtered timeline."""
    model = _model("mn05")
    det = detection.EADetector(model=model, batch_windows=3, taper=taper)
    geo = det.geometry
    assert (geo.W, geo.Hs, geo.T, geo.Hf, geo.R) == (327680, 163840, 32, 16, 10240)
    recs = _recordings()
    lengths = [int(r.numel()) for r in recs]
    starts, valids, table = det.plan(lengths)
    assert table.cpu.tolist() == [[0, 4, 0, 79], [4, 1, 79, 10]]

    seen = []
    inner = det.window_logits
    monkeypatch.setattr(det, "window_logits", lambda *a: seen.append(inner(*a)) or seen[-1])
    res = det.frame_probs(recs)
    P = seen[-1]                                                           # the detector's own (N_w, K, Tp) logits
    assert P.shape == (5, K, 32)
    wt = torch.from_numpy(ops.detect_weights(32, taper).astype(np.float32)).to(DEV)
    prob = ops.detect_stitch(P, table, 16, 32, wt)
    assert len(res) == 2
    for (pr, t), (_, _, goff, G), n in zip(res, table.cpu.tolist(), lengths):
        assert pr.shape == (G, K) and pr.is_cuda and t.dtype == np.float64 and np.array_equal(t, np.arange(G) * 0.32)
        assert torch.equal(pr, prob[:, goff:goff + G].t())
        assert (G - 1) * geo.R < n <= G * geo.R
    # the same chunks of MATERIALISED windows through mel, forward and frame_logits by hand
    flat = torch.cat(recs)
    wins = torch.zeros((5, geo.W))
    for w, (s, v) in enumerate(zip(starts, valids)):
        wins[w, :v] = flat[s:s + v]
    by_hand = []
    d_start, d_valid = (t.to(DEV) for t in ops.check_windows(starts, valids, geo.W, flat.numel()))
    with torch.no_grad():
        for q0 in (0, 3):
            spec = det.mel(wins[q0:q0 + 3].to(DEV))
            assert torch.equal(spec, det.mel.forward_windows(flat.to(DEV), d_start[q0:q0 + 3], d_valid[q0:q0 + 3], geo.W))
            y = model._forward_impl(spec.unsqueeze(1), return_fmaps=True)[1][-1]
            assert y.shape[3] == 32
            by_hand.append(detection.frame_logits(model, y))
    P2 = torch.cat(by_hand)
    dP = float((P2 - P).abs().max())
    prob2 = ops.detect_stitch(P2, table, 16, 32, wt)
    dp = float((prob2 - prob).abs().max())
    print(f"detector vs by hand ({taper}): logits bit-equal {torch.equal(P2, P)} (max |delta| {dP:.3e}), "
          f"probabilities bit-equal {torch.equal(prob2, prob)} (max |delta| {dp:.3e})")
    assert _close(P2.cpu().numpy(), P.cpu().numpy())
    assert _close(prob2.cpu().numpy(), prob.cpu().numpy())

    # detect == events_ref on the device's own filt
    hi = np.linspace(0.45, 0.6, K).astype(np.float32)
    for kw, m, gap, mlen in ((dict(median_ms=960), 3, 0, 0), (dict(median_ms=0, max_gap_ms=640, min_duration_ms=960), 1, 2, 3),
                             (dict(median_ms=2240, max_gap_ms=320), 7, 1, 0)):
        found = det.detect(recs, threshold=hi, low_threshold=0.42, **kw)
        P = seen[-1]
        filt = ops.detect_median(ops.detect_stitch(P, table, 16, 32, wt), table, m).cpu().numpy()
        ev, peak, mean = R.events_ref(filt, table.cpu.tolist(), hi, np.float32(0.42), gap, mlen)
        n_ev = [int((ev[:, 0] == i).sum()) for i in range(2)]
        print(f"detect ({taper}, {kw}): {n_ev} events")
        assert [len(f) for f in found] == n_ev and sum(n_ev) > 0
        flat_found = [e for f in found for e in f]
        for (label, on_s, off_s, pk, mn), (i, k, on, off), p_ref, m_ref in zip(flat_found, ev.tolist(), peak, mean):
            assert label == k and on_s == on * 0.32 and off_s == min(off * 10240, lengths[i]) / SR
            assert on_s < off_s <= lengths[i] / SR
            assert pk == float(p_ref) and abs(mn - m_ref) <= 2 * float(np.spacing(np.float32(m_ref)))


def test_labels_single_waveform_and_dymn():
    names = [f"class {k}" for k in range(K)]
    det = detection.EADetector(model=_model("dymn04"), labels=names, clip_seconds=5.12, hop_seconds=2.56)
    wave = _recordings()[1]
    found = det.detect([wave], threshold=0.5, median_ms=0)
    again = det.detect(wave.to(DEV), threshold=0.5, median_ms=0)          # a single 1-D waveform is one recording
    assert len(found) == 1 and len(again) == 1 and len(found[0]) > 0
    assert {e[0] for e in found[0]} <= set(names)
    (pr, t), = det.frame_probs([wave])
    assert pr.shape == (10, K) and float(pr.min()) > 0 and float(pr.max()) < 1
    model = _model("mn05")
    model.train()
    try:
        with pytest.raises(ValueError, match="eval mode"):
            detection.EADetector(model=model)
    finally:
        model.eval()
    det = detection.EADetector(model=model, clip_seconds=0.32, hop_seconds=0.32)     # T = 1: one column per window
    assert det.geometry.T == 1
    (pr, t), = det.frame_probs([wave[:25000]])
    assert pr.shape == (3, K) and bool(torch.isfinite(pr).all())
    with pytest.raises(ValueError, match="the filter takes 1 to 31"):
        det.detect([wave], median_ms=20000)
    with pytest.raises(ValueError, match="0 < low_threshold <= threshold <= 1"):
        det.detect([wave], threshold=0.3, low_threshold=0.5)
    with pytest.raises(ValueError, match="empty recording"):
        det.detect([torch.zeros(0)])


# ------------------------------------------------------------------------------------------------ the program
def test_command_line(tmp_path, capsys):
    model = _model("mn05")
    ckpt = str(tmp_path / "mn05.pt")
    torch.save(model.state_dict(), ckpt)
    paths = []
    for i, rec in enumerate(_recordings()):
        pcm = (rec.clamp(-1, 1) * 32767).to(torch.int16).numpy()
        paths.append(str(tmp_path / f"clip{i}.wav"))
        wavfile.write(paths[-1], SR, pcm)
    common = ["--audio_path", *paths, "--checkpoint", ckpt, "--width", "0.5", "--threshold", "0.5", "--low_threshold", "0.45"]
    assert detect.main(common + ["--json"]) == 0
    lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert [ln["audio_path"] for ln in lines] == paths
    assert sum(len(ln["events"]) for ln in lines) > 0
    for ln, dur in zip(lines, (25.0, 3.125)):
        for e in ln["events"]:
            assert set(e) == {"label", "onset", "offset", "peak", "mean"}
            assert 0 <= e["onset"] < e["offset"] <= dur and 0.4499 <= e["mean"] <= e["peak"] <= 1.0 and e["peak"] >= 0.5
    out = str(tmp_path / "events.tsv")
    assert detect.main(common + ["--out", out, "--max_gap_ms", "320"]) == 0
    with open(out) as f:
        rows = [ln.rstrip("\n").split("\t") for ln in f]
    assert rows[0] == ["filename", "onset", "offset", "event_label"] and len(rows) > 1
    body = [(r[0], float(r[1]), float(r[2]), r[3]) for r in rows[1:]]
    assert all(len(r) == 4 for r in rows) and all(on < off for _, on, off, _ in body)
    assert {r[0] for r in body} <= {"clip0.wav", "clip1.wav"}
    assert body == sorted(body, key=lambda r: (r[0], r[1], r[2], r[3]))
    print(f"detect program: {len(body)} TSV rows, {sum(len(ln['events']) for ln in lines)} JSON events")


# ------------------------------------------------------------------------------------------------ launch list
_BLAS = ("Cijk_", "rocblas", "hipblas", "Tensile")


def _kernels(fn):
    """Names of the device activities `fn` launches, in launch order (torch.profiler)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    ev.sort(key=lambda e: e.time_range.start)
    return [e.name for e in ev]


def test_no_torch_elementwise_op_and_no_vendor_gemm_behind_the_trunk():
    """One `detect` of a recording that fits one chunk under torch.profiler.  From the trunk's last kernel (the one ahead of
    the frequency mean) to the event list every launch is a kernel of this library, except the documented scan between the two
    event launches (torch.cumsum) and the device->host copies of the total and of the event list: no `at::native` elementwise
    kernel, no BLAS kernel, no memset."""
    det = detection.EADetector(model=_model("mn05"))
    wave = _recordings()[0].to(DEV)
    run = lambda: det.detect([wave], threshold=0.5, low_threshold=0.45)
    assert len(run()[0]) > 0
    names = _kernels(run)
    i = [k for k, n in enumerate(names) if "freq_mean_fwd_kernel" in n]
    assert len(i) == 1 and i[0] >= 1, names
    tail = names[i[0] - 1:]
    print("detect launch list behind the trunk:", tail)
    ours = ("freq_mean_fwd_kernel", "detect_stitch_kernel", "detect_median_kernel", "detect_events_kernel")
    for want in ours:
        assert any(want in n for n in tail), want
    assert sum("detect_events_kernel" in n for n in tail) == 2
    assert not [n for n in tail if "elementwise" in n.lower()], tail
    assert not [n for n in names if any(b in n for b in _BLAS)]
    assert not [n for n in tail if n.startswith("Memset")], tail
    # whatever is not ours between the two event launches is the scan (and the copy of its last element)
    e = [k for k, n in enumerate(tail) if "detect_events_kernel" in n]
    between = tail[e[0] + 1:e[1]]
    assert between and all("scan" in n.lower() or n.startswith("Memcpy") for n in between), between
    foreign = [n for n in tail[:e[0]] if n.startswith("Mem") or "at::" in n]
    assert not foreign, foreign
