"""PSDS at model level: `sed.evaluate_psds` against `EADetector.detect` at every grid threshold followed by the numpy
restatement's criteria and curve (tests/psds_ref.py), for both scenarios; `score_sed --psds`; `evaluate_events`, which now shares
its chunk walk, against a direct `ops.event_score` walk; and the launch list of a chunk.  All counts are compared for exact
equality."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import detection, ops, score_sed, sed  # noqa: E402
from efficientat_amd.mn import get_model  # noqa: E402
from efficientat_amd.preprocess import AugmentMelSTFT  # noqa: E402
from tests import psds_ref as P  # noqa: E402
from tests.event_score_ref import class_rows  # noqa: E402

DEV = torch.device("cuda:0")
SR, K, WIDTH = 32000, 3, 0.5
SECONDS = (3.0, 12.0, 5.3, 7.77)
CLASSES = ["alarm", "dog", "speech"]
POST = dict(median_ms=960, min_duration_ms=640, max_gap_ms=320)
LOW_RATIO = 0.8


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _mel():
    return _quiet(AugmentMelSTFT, freqm=0, timem=0).to(DEV).eval()


def _waves():
    """Noise with tone bursts that come and go, so that the frame probabilities of a random model move in time."""
    rng = np.random.RandomState(3)
    out = []
    for s in SECONDS:
        n = int(round(s * SR))
        t = np.arange(n) / SR
        x = 0.03 * rng.randn(n)
        for _ in range(int(2 + s)):
            a, d = rng.randint(0, n - 1), rng.randint(SR // 4, 2 * SR)
            x[a:a + d] += rng.uniform(0.1, 0.5) * np.sin(2 * np.pi * rng.uniform(150, 6000) * t[a:a + d])
        out.append(x.astype(np.float32))
    return out


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    """A narrow random mlp-head MN whose frame probabilities straddle 0.5 in every class (prepared as in
    tests/test_gpu_event_eval.py), four clips of 3 - 12 s, and a bank the test writes: the reference events are the model's
    own events at 0.5 / 0.4, moved by up to 0.3 s at either end, every other one with a copy under the next class (so that
    detections lie over other classes' references) and those of one class per clip filed under the next class alone, plus one
    event nothing finds; clip 2 has none."""
    torch.manual_seed(31)
    model = _quiet(get_model, width_mult=WIDTH, num_classes=K, head_type="mlp").to(DEV).eval()
    waves = _waves()
    det = detection.EADetector(model=model)
    with torch.no_grad():
        g = torch.Generator().manual_seed(29)
        for mod in model.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.copy_(0.1 * torch.randn(mod.running_mean.shape, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=g))
                mod.weight.copy_(0.8 + 0.4 * torch.rand(mod.weight.shape, generator=g))
                mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
        starts, valids, _ = det.plan([len(w) for w in waves])
        P_ = det.window_logits(torch.from_numpy(np.concatenate(waves)).to(DEV), starts, valids)
        z = P_[:, :, :det.geometry.T].permute(0, 2, 1).reshape(-1, K).double()
        q = torch.quantile(z, torch.tensor([0.1, 0.5, 0.9], dtype=torch.float64, device=z.device), dim=0)
        spread, med = q[2] - q[0], q[1]
        assert bool(torch.isfinite(z).all()) and float(spread.min()) > 0
        scale = (2.0 / spread).float()                                        # four fifths of the frames within a logit of +- 1
        model.classifier[5].weight.mul_(scale.view(K, 1))
        model.classifier[5].bias.copy_(scale * (model.classifier[5].bias - med.float()))
    found = det.detect([torch.from_numpy(w) for w in waves], threshold=0.5, low_threshold=0.4, **POST)
    rng = np.random.RandomState(5)
    events, eo = [], [0]
    for i, (w, evs) in enumerate(zip(waves, found)):
        n, mine = len(w), []
        for j, (k, on_s, off_s, _, _) in enumerate([] if i == 2 else evs):
            on, off = int(round(on_s * SR)), int(round(off_s * SR))
            if j > 0:
                on, off = on + rng.randint(-9600, 9601), off + rng.randint(-9600, 9601)
            on = min(max(on, 0), n - 1)
            off = min(max(off, on + 1), n)
            if int(k) == (i + 1) % K:                                         # filed under the next class alone: its detections
                mine.append(((int(k) + 1) % K, on, off))                      # are false positives that cross-trigger
                continue
            mine.append((int(k), on, off))
            if j % 2 == 0:
                mine.append(((int(k) + 1) % K, on, off))
        if i == 0:
            mine.append((1, 777, 777 + SR))
        events.extend(sorted(mine))
        eo.append(len(events))
    d = str(tmp_path_factory.mktemp("psds_bank"))
    np.save(os.path.join(d, "waves.npy"), np.concatenate(waves))
    np.save(os.path.join(d, "lengths.npy"), np.asarray([len(w) for w in waves], dtype=np.int64))
    np.save(os.path.join(d, "events.npy"), np.asarray(events, dtype=np.int32).reshape(-1, 3))
    np.save(os.path.join(d, "event_offsets.npy"), np.asarray(eo, dtype=np.int64))
    with open(os.path.join(d, "names.txt"), "w") as f:
        f.write("\n".join(f"clip{i}.wav" for i in range(len(waves))) + "\n")
    with open(os.path.join(d, "classes.txt"), "w") as f:
        f.write("\n".join(CLASSES) + "\n")
    ckpt = os.path.join(d, "model.pt")
    torch.save(model.state_dict(), ckpt)
    hi, lo = sed.threshold_grid(None, LOW_RATIO)
    tensors = [torch.from_numpy(w) for w in waves]
    lists = [det.detect(tensors, threshold=float(hi[v]), low_threshold=float(lo[v]), **POST) for v in range(hi.size)]
    return dict(dir=d, model=model, det=det, waves=waves, events=np.asarray(events, dtype=np.int64).reshape(-1, 3), eo=eo,
                ckpt=ckpt, bank=sed.load_bank(d, device=DEV), lists=lists, hi=hi, lo=lo)


def _want(s, crit):
    """The restatement's criteria on what `detect` listed at every threshold -> (counts (V, K, 4), ct (V, K, K))."""
    ev = s["events"].tolist()
    V = len(s["lists"])
    counts, ct = np.zeros((V, K, 4), dtype=np.int64), np.zeros((V, K, K), dtype=np.int64)
    for v, found in enumerate(s["lists"]):
        for i, evs in enumerate(found):
            rows = {k: [(ev[e][1], ev[e][2]) for e in class_rows(ev, s["eo"], i, k)] for k in range(K)}
            for k in range(K):
                dets = [(int(round(on * SR)), int(round(off * SR))) for kk, on, off, _, _ in evs if kk == k]
                tp, n_det, fp, crossed = P.judge_timeline(dets, rows[k], {c: r for c, r in rows.items() if c != k and r}, *crit)
                counts[v, k] += (tp, n_det, fp, len(crossed))
                for c in crossed:
                    ct[v, k, c] += 1
    return counts, ct


@pytest.mark.parametrize("scenario", [1, 2])
def test_evaluate_psds_equals_detect_and_the_restatement_at_every_threshold(setup, scenario):
    s = setup
    s["model"].train()
    ev = sed.evaluate_psds(s["model"], _mel(), s["bank"], scenario=scenario, low_ratio=LOW_RATIO, **POST)
    assert s["model"].training                                                # the mode is restored
    s["model"].eval()
    assert ev["thresholds"].shape == (49,) and np.array_equal(ev["thresholds"], s["hi"]) and np.array_equal(ev["low_thresholds"], s["lo"])
    sc = sed.PSDS_SCENARIOS[scenario]
    crit = tuple(int(round(1000 * sc[k])) for k in ("dtc", "gtc", "cttc"))
    want, want_ct = _want(s, crit)
    n_ref = np.bincount(s["events"][:, 0], minlength=K)
    print(f"evaluate_psds scenario {scenario}: tp {want[:, :, 0].sum(1).tolist()}\n fp {want[:, :, 2].sum(1).tolist()}\n "
          f"cross-triggers {want_ct.sum((1, 2)).tolist()}\n psds {ev['psds']}")
    assert ev["counts"].dtype == np.int64
    assert np.array_equal(ev["counts"], np.stack([want[:, :, 0], want[:, :, 2], n_ref[None] - want[:, :, 0]], axis=2))
    assert np.array_equal(ev["n_det"], want[:, :, 1]) and np.array_equal(ev["ct"], want_ct)
    assert want[:, :, 0].sum() > 0 and want[:, :, 2].sum() > 0 and (want_ct.sum() > 0) == (scenario == 2)
    assert len({tuple(w) for w in want.reshape(49, -1).tolist()}) > 5         # the thresholds see different event lists
    ref_seconds = [sum(off - on for c, on, off in s["events"].tolist() if c == k) / SR for k in range(K)]
    total = sum(len(w) for w in s["waves"]) / SR
    assert np.array_equal(ev["n_ref"], n_ref) and ev["ref_seconds"].tolist() == pytest.approx(ref_seconds, rel=1e-12)
    assert ev["total_seconds"] == pytest.approx(total, rel=1e-12) and ev["n_clips"] == len(SECONDS) and ev["eval_s"] > 0
    psds, _, _ = P.curve_ref(want[:, :, 0], want[:, :, 2], want_ct, n_ref, ref_seconds, total, sc["alpha_ct"], sc["alpha_st"], 100.0)
    # both are fp64 sums of fewer than 10^4 terms (rounding about 1e-12): 1e-9 leaves three decades
    assert np.isfinite(psds) and abs(ev["psds"] - psds) <= 1e-9 * abs(psds)
    assert ev["settings"]["scenario"] == scenario and ev["settings"]["dtc"] == sc["dtc"] and ev["settings"]["cttc"] == sc["cttc"]
    # the chunking does not matter.  The split is 28 s long, so a single false positive is 128 per hour and only the points
    # without any lie inside e_max = 100: the curve is compared once more over a range that holds all of them
    wide = 3600.0 * 50 / total
    one = sed.evaluate_psds(s["model"], _mel(), s["bank"], scenario=scenario, low_ratio=LOW_RATIO, batch_clips=1, e_max=wide, **POST)
    assert np.array_equal(one["counts"], ev["counts"]) and np.array_equal(one["ct"], ev["ct"])
    psds_wide, bx, _ = P.curve_ref(want[:, :, 0], want[:, :, 2], want_ct, n_ref, ref_seconds, total, sc["alpha_ct"], sc["alpha_st"], wide)
    print(f" psds over [0, {wide:.0f}]: {one['psds']} ({len(bx)} breakpoints)")       # (more than the two ends: the curve has steps inside)
    assert len(bx) > 2 and abs(one["psds"] - psds_wide) <= 1e-9 * abs(psds_wide) and psds_wide != 0 and one["settings"]["e_max"] == wide
    # explicit criteria override the scenario's
    other = sed.PSDS_SCENARIOS[3 - scenario]
    over = sed.evaluate_psds(s["model"], _mel(), s["bank"], scenario=3 - scenario, dtc=sc["dtc"], gtc=sc["gtc"], cttc=sc["cttc"],
                             alpha_ct=sc["alpha_ct"], alpha_st=sc["alpha_st"], low_ratio=LOW_RATIO, batch_clips=3, **POST)
    assert other["dtc"] != sc["dtc"] and np.array_equal(over["counts"], ev["counts"]) and over["psds"] == ev["psds"]


def test_score_sed_prints_the_same_psds(setup, capsys):
    common = ["--checkpoint", setup["ckpt"], "--bank", setup["dir"], "--width", str(WIDTH), "--json", "--low_ratio", str(LOW_RATIO),
              "--min_duration_ms", "640", "--max_gap_ms", "320"]

    def run(extra):
        assert score_sed.main(common + extra) == 0
        return json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])

    plain, line = run([]), run(["--psds", "1,2"])
    assert not [k for k in plain if "psds" in k]                              # without the flag: the line as it was
    assert list(line) == list(plain) + ["psds_scenario1", "psds_scenario2", "psds_eval_s"]
    assert {k: v for k, v in line.items() if k in plain and k != "event_eval_s"} == \
        {k: v for k, v in plain.items() if k != "event_eval_s"}
    for scenario in (1, 2):
        ev = sed.evaluate_psds(setup["model"], _mel(), setup["bank"], scenario=scenario, low_ratio=LOW_RATIO, **POST)
        assert line[f"psds_scenario{scenario}"] == ev["psds"]
    custom = run(["--dtc", "0.5", "--gtc", "0.5", "--e_max", "50"])
    ev = sed.evaluate_psds(setup["model"], _mel(), setup["bank"], scenario=1, dtc=0.5, gtc=0.5, e_max=50.0, low_ratio=LOW_RATIO, **POST)
    assert custom["psds"] == ev["psds"] and "psds_scenario1" not in custom
    with pytest.raises(SystemExit):
        _quiet(score_sed.parse_args, ["--checkpoint", "a", "--bank", "b", "--psds", "3"])


def test_evaluate_events_still_equals_a_direct_event_score_walk(setup):
    s = setup
    ev = sed.evaluate_events(s["model"], _mel(), s["bank"], low_ratio=LOW_RATIO, batch_clips=3, **POST)
    det, mel = detection.EADetector(model=s["model"]), _mel()
    det.mel = mel
    geo = det.geometry
    lengths = [len(w) for w in s["waves"]]
    c = sed.collar_samples(200, SR)
    refs = ops.event_refs(s["bank"]["events"].cpu(), torch.from_numpy(sed.event_tolerances(s["bank"]["events"], c, 0.2)),
                          s["bank"]["event_offsets"].cpu(), K)
    with torch.no_grad():
        starts, valids, table = det.plan(lengths)
        logits = det.window_logits(s["bank"]["waves"], starts, valids)
        prob = ops.detect_stitch(logits, table, geo.Hf, geo.T, det._wt)
        filt = ops.detect_median(prob, table, detection.median_frames(POST["median_ms"], geo.frame_s))
        cnt = ops.event_score(filt, table, lengths, geo.R, refs, c, s["hi"], s["lo"],
                              detection.ms_to_frames(POST["max_gap_ms"], geo.frame_s),
                              detection.ms_to_frames(POST["min_duration_ms"], geo.frame_s)).sum(0).cpu().numpy().astype(np.int64)
    tp, n_est = cnt[:, :, 0].T, cnt[:, :, 1].T
    n_ref = np.bincount(s["events"][:, 0], minlength=K)
    assert np.array_equal(ev["counts"], np.stack([tp, n_est - tp, n_ref[None] - tp], axis=2)) and tp.sum() > 0
    assert ev["n_ref"] == len(s["events"]) and ev["n_clips"] == len(SECONDS) and ev["threshold"] == 0.5


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


def test_one_psds_count_launch_per_chunk(setup):
    mel = _mel()
    for batch_clips, chunks in ((len(SECONDS), 1), (3, 2)):
        names = _kernels(lambda: sed.evaluate_psds(setup["model"], mel, setup["bank"], scenario=2, low_ratio=LOW_RATIO,
                                                   batch_clips=batch_clips, **POST))
        assert sum("psds_count_kernel" in n for n in names) == chunks, names
        assert sum("detect_median_kernel" in n for n in names) == chunks and not [n for n in names if "event_score_kernel" in n]


def test_finetune_sed_psds_eval_prints_the_score_of_the_model_it_saves(setup, tmp_path):
    from efficientat_amd import finetune_sed
    save = str(tmp_path / "sed.pt")
    argv = ["--train_bank", setup["dir"], "--valid_bank", setup["dir"], "--batch_size", "4", "--clip_frames", "3", "--n_epochs", "1",
            "--lr", "1e-3", "--warm_up_len", "1", "--model_width", str(WIDTH), "--no_graph", "--max_steps", "2", "--json",
            "--low_ratio", str(LOW_RATIO), "--min_duration_ms", "640", "--max_gap_ms", "320", "--save", save]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        finetune_sed.main(argv + ["--psds_eval", "--psds", "2", "--e_max", "5000"])
    line = json.loads(buf.getvalue().strip().splitlines()[-1])
    assert list(line)[-2:] == ["psds_scenario2", "psds_eval_s"] and not [k for k in line if k.startswith("event_")]
    model = _quiet(get_model, width_mult=WIDTH, num_classes=K)
    model.load_state_dict(torch.load(save, map_location="cpu", weights_only=True))
    ev = sed.evaluate_psds(model.to(DEV).eval(), _mel(), setup["bank"], scenario=2, e_max=5000.0, low_ratio=LOW_RATIO, **POST)
    assert line["psds_scenario2"] == pytest.approx(ev["psds"], abs=0, nan_ok=True)
    with pytest.raises(SystemExit):                                           # the PSDS flags ask for --psds_eval
        _quiet(finetune_sed.parse_args, ["--train_bank", "a", "--valid_bank", "b", "--psds", "1"])
