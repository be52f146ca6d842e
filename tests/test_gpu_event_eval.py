"""Event-based scoring at model level: `sed.evaluate_events` against `EADetector.detect` at every grid threshold followed by
the numpy restatement's matching (tests/event_score_ref.py), its scores and threshold choice against the counts, the chunking,
and the programs around it: `finetune_sed --event_eval`, `score_sed`, `detect --thresholds_file`.  All counts are compared
for exact equality."""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch
from scipy.io import wavfile

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import detect, detection, finetune_sed, score_sed, sed  # noqa: E402
from efficientat_amd.mn import get_model  # noqa: E402
from efficientat_amd.preprocess import AugmentMelSTFT  # noqa: E402
from tests import event_score_ref as R  # noqa: E402
from tests.sed_ref import segment_scores as scores_ref  # noqa: E402

DEV = torch.device("cuda:0")
SR, K, RS, WIDTH = 32000, 3, 10240, 0.5
SECONDS = (3.0, 12.0, 5.3, 7.77, 10.24, 4.1)
CLASSES = ["alarm", "dog", "speech"]
POST = dict(median_ms=960, min_duration_ms=640, max_gap_ms=320)
LOW_RATIO, COLLAR_MS, PCT = 0.8, 200, 0.2
# the JSON line of `finetune_sed --json` before event scoring existed: without --event_eval it is still exactly this
PARENT_KEYS = ["what", "model", "classes", "steps", "epochs", "batch_size", "clip_samples", "launch", "threshold", "train_loss",
               "clips_per_s", "n_frames", "eval_s", "checkpoint", "frame_mAP", "frame_ROC", "micro_f1", "micro_precision",
               "micro_recall", "macro_f1", "macro_precision", "macro_recall", "val_loss"]


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
    """A narrow random mlp-head MN whose frame probabilities straddle 0.5 in every class, six clips of 3 - 12 s, and a bank the
    test writes: the reference events are the model's own events at 0.5 / 0.4 - a clip's first and a third of the others kept
    on the frame grid, the rest moved off it by up to 0.3 s at either end - plus two events the model does not find; clip 3 has none."""
    torch.manual_seed(31)
    model = _quiet(get_model, width_mult=WIDTH, num_classes=K, head_type="mlp").to(DEV).eval()
    waves = _waves()
    det = detection.EADetector(model=model)
    with torch.no_grad():
        # (BatchNorm statistics and affines perturbed as in tests/test_gpu_detect.py: the trunk of a fresh model is degenerate)
        g = torch.Generator().manual_seed(29)
        for mod in model.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.copy_(0.1 * torch.randn(mod.running_mean.shape, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=g))
                mod.weight.copy_(0.8 + 0.4 * torch.rand(mod.weight.shape, generator=g))
                mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
        # per class, scale and shift the output layer so that the window logits have median 0 and four fifths of them lie
        # within +- 1:
        # probabilities that straddle 0.5 and spread over the grid of thresholds
        starts, valids, _ = det.plan([len(w) for w in waves])
        P = det.window_logits(torch.from_numpy(np.concatenate(waves)).to(DEV), starts, valids)
        z = P[:, :, :det.geometry.T].permute(0, 2, 1).reshape(-1, K).double()
        q = torch.quantile(z, torch.tensor([0.1, 0.5, 0.9], dtype=torch.float64, device=z.device), dim=0)
        spread, med = q[2] - q[0], q[1]
        print(f"event bank: window logits 10 % to 90 % spread {spread.tolist()}, median {med.tolist()}")
        assert bool(torch.isfinite(z).all()) and float(spread.min()) > 0
        scale = (2.0 / spread).float()                                        # four fifths of the frames within a logit of +- 1
        model.classifier[5].weight.mul_(scale.view(K, 1))
        model.classifier[5].bias.copy_(scale * (model.classifier[5].bias - med.float()))
    found = det.detect([torch.from_numpy(w) for w in waves], threshold=0.5, low_threshold=0.4, **POST)
    rng = np.random.RandomState(5)
    events, eo = [], [0]
    for i, (w, evs) in enumerate(zip(waves, found)):
        n, mine = len(w), []
        for j, (k, on_s, off_s, _, _) in enumerate([] if i == 3 else evs):
            on, off = int(round(on_s * SR)), int(round(off_s * SR))
            if j > 0 and rng.rand() > 1 / 3:
                on, off = on + rng.randint(-9600, 9601), off + rng.randint(-9600, 9601)
            on = min(max(on, 0), n - 1)
            mine.append((int(k), on, min(max(off, on + 1), n)))
        if i in (0, 1):
            mine.append((i, 777, 777 + SR))
        events.extend(sorted(mine))
        eo.append(len(events))
    d = str(tmp_path_factory.mktemp("event_bank"))
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
    return dict(dir=d, model=model, det=det, waves=waves, events=np.asarray(events, dtype=np.int64).reshape(-1, 3), eo=eo,
                ckpt=ckpt, bank=sed.load_bank(d, device=DEV))


def _evaluate(s, **kw):
    return sed.evaluate_events(s["model"], _mel(), s["bank"], low_ratio=LOW_RATIO, collar_ms=COLLAR_MS, offset_pct=PCT,
                               threshold=0.5, **POST, **kw)


def test_evaluate_events_equals_detect_and_the_restatement_at_every_threshold(setup):
    s = setup
    s["model"].train()
    ev = _evaluate(s)
    assert s["model"].training                                                # the mode is restored
    s["model"].eval()
    hi, lo = ev["thresholds"], ev["low_thresholds"]
    assert hi.shape == (49,) and np.array_equal(hi, sed.threshold_grid()[0]) and np.array_equal(lo, sed.threshold_grid(None, 0.8)[1])
    c = 6400
    tol = R.tolerances(s["events"], c, PCT)
    waves = [torch.from_numpy(w) for w in s["waves"]]
    want = np.zeros((49, K, 3), dtype=np.int64)
    for v in range(49):
        found = s["det"].detect(waves, threshold=float(hi[v]), low_threshold=float(lo[v]), **POST)
        for i, evs in enumerate(found):
            for k in range(K):
                ests = [(int(round(on * SR)), int(round(off * SR))) for kk, on, off, _, _ in evs if kk == k]
                rows = R.class_rows(s["events"].tolist(), s["eo"], i, k)
                tp = len(R.match_ref_outer([(s["events"][e][1], s["events"][e][2]) for e in rows], [tol[e] for e in rows], ests, c))
                want[v, k] += (tp, len(ests) - tp, len(rows) - tp)
    print(f"evaluate_events: tp {want[:, :, 0].sum(1).tolist()}\n fp {want[:, :, 1].sum(1).tolist()}\n fn {want[:, :, 2].sum(1).tolist()}")
    assert ev["counts"].dtype == np.int64 and np.array_equal(ev["counts"], want)
    assert want[24, :, 0].sum() > 0 and want[:, :, 1].sum() > 0 and want[:, :, 2].sum() > 0
    assert len({tuple(w) for w in want.reshape(49, -1).tolist()}) > 5         # the thresholds see different event lists
    assert ev["n_clips"] == len(SECONDS) and ev["n_ref"] == len(s["events"]) and ev["eval_s"] > 0

    # scores, the reported threshold and the per-class choice, recomputed from the counts on the host
    assert ev["threshold"] == 0.5 and ev["threshold_index"] == 24
    for v in range(49):
        ref = scores_ref(want[v])
        for name in sed.SCORE_NAMES:
            assert ev["grid"][name][v] == pytest.approx(ref[name], abs=1e-15, nan_ok=True)
            if v == 24:
                assert ev[name] == pytest.approx(ref[name], abs=1e-15, nan_ok=True)
    best = []
    for k in range(K):
        f = [2 * a / (2 * a + b + m) if 2 * a + b + m else -1.0 for a, b, m in want[:, k].tolist()]
        best.append(f.index(max(f)))
    assert ev["best_index"].tolist() == best
    assert ev["best_threshold"].dtype == np.float32 and np.array_equal(ev["best_threshold"], hi[best])
    assert np.array_equal(ev["best_low_threshold"], lo[best])
    assert ev["macro_f1_best"] == pytest.approx(scores_ref(want[best, np.arange(K)])["macro_f1"], abs=1e-15)
    assert ev["macro_f1_best"] >= ev["macro_f1"]
    off_grid = _evaluate(s, thresholds=[0.3, 0.62, 0.9])                      # 0.5 is not on this grid: the nearest is reported
    assert off_grid["threshold"] == float(np.float32(0.62)) and off_grid["threshold_index"] == 1
    assert np.array_equal(off_grid["counts"][0], want[14])                    # 0.3 = 15 / 50


def test_counts_do_not_depend_on_the_chunking(setup):
    one, all_ = _evaluate(setup, batch_clips=1), _evaluate(setup, batch_clips=len(SECONDS))
    assert np.array_equal(one["counts"], all_["counts"]) and one["counts"][:, :, 0].sum() > 0
    assert np.array_equal(_evaluate(setup, batch_clips=4)["counts"], one["counts"])


@pytest.fixture(scope="module")
def program(setup, tmp_path_factory):
    out = tmp_path_factory.mktemp("event_prog")
    points, save = str(out / "points" / "ops.json"), str(out / "sed.pt")
    argv = ["--train_bank", setup["dir"], "--valid_bank", setup["dir"], "--batch_size", "4", "--clip_frames", "3", "--n_epochs", "1",
            "--lr", "1e-3", "--warm_up_len", "1", "--model_width", str(WIDTH), "--no_graph", "--max_steps", "2", "--json"]
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        finetune_sed.main(argv + ["--event_eval", "--save_thresholds", points, "--save", save, "--low_ratio", str(LOW_RATIO),
                                  "--min_duration_ms", "640", "--max_gap_ms", "320"])
    line = json.loads(buf.getvalue().strip().splitlines()[-1])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        finetune_sed.main(argv)
    plain = json.loads(buf.getvalue().strip().splitlines()[-1])
    return dict(line=line, plain=plain, points=points, save=save)


def test_finetune_sed_event_eval_prints_its_keys_and_writes_operating_points(setup, program):
    line, plain = program["line"], program["plain"]
    assert list(plain) == PARENT_KEYS                                         # without --event_eval: the line as it was
    assert list(line) == PARENT_KEYS + list(finetune_sed.EVENT_KEYS) and line["steps"] == 2
    assert line["thresholds_file"] == program["points"] and line["event_threshold"] == 0.5
    assert (line["event_collar_ms"], line["event_offset_pct"]) == (200.0, 0.2) and len(line["event_best_threshold"]) == K
    assert all(0 < t < 1 for t in line["event_best_threshold"]) and line["event_eval_s"] > 0
    pts = sed.load_operating_points(program["points"], classes=CLASSES, n_classes=K)
    assert pts["threshold"].tolist() == line["event_best_threshold"]
    assert (pts["median_ms"], pts["min_duration_ms"], pts["max_gap_ms"], pts["taper"]) == (960.0, 640.0, 320.0, "triangle")
    assert (pts["window_size"], pts["hop_length"]) == (10.24, 5.12) and pts["scoring"]["low_ratio"] == LOW_RATIO
    with pytest.raises(SystemExit):
        _quiet(finetune_sed.parse_args, ["--train_bank", "a", "--valid_bank", "b", "--save_thresholds", "f"])


def test_score_sed_agrees_with_evaluate_events(setup, program, capsys):
    points = os.path.join(os.path.dirname(program["save"]), "scored.json")
    assert score_sed.main(["--checkpoint", program["save"], "--bank", setup["dir"], "--width", str(WIDTH), "--json",
                           "--low_ratio", str(LOW_RATIO), "--min_duration_ms", "640", "--max_gap_ms", "320", "--threshold", "0.4",
                           "--save_thresholds", points]) == 0
    line = json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])
    model = _quiet(get_model, width_mult=WIDTH, num_classes=K)
    model.load_state_dict(torch.load(program["save"], map_location="cpu", weights_only=True))
    ev = sed.evaluate_events(model.to(DEV).eval(), _mel(), setup["bank"], low_ratio=LOW_RATIO, threshold=0.4, **POST)
    assert line["event_threshold"] == float(np.float32(0.4)) == ev["threshold"]
    for name in sed.SCORE_NAMES:
        assert line["event_" + name] == pytest.approx(ev[name], abs=0, nan_ok=True), name
    assert line["event_macro_f1_best"] == pytest.approx(ev["macro_f1_best"], abs=0, nan_ok=True)
    assert line["event_best_threshold"] == [float(v) for v in ev["best_threshold"]]
    assert (line["n_clips"], line["n_ref"], line["classes"]) == (len(SECONDS), len(setup["events"]), K)
    assert np.array_equal(sed.load_operating_points(points, classes=CLASSES)["threshold"], ev["best_threshold"])


def test_detect_takes_its_defaults_from_a_thresholds_file(setup, tmp_path, capsys):
    ev = _evaluate(setup)
    ev["best_threshold"] = np.asarray([0.42, 0.5, 0.58], dtype=np.float32)    # (distinct per class, whatever the scores chose)
    ev["best_low_threshold"] = np.asarray([0.3, 0.5, 0.4], dtype=np.float32)
    points = str(tmp_path / "ops.json")
    sed.save_operating_points(points, ev, CLASSES)
    paths = []
    for i, w in enumerate(setup["waves"][:3]):
        paths.append(str(tmp_path / f"clip{i}.wav"))
        wavfile.write(paths[-1], SR, w)
    common = ["--audio_path", *paths, "--checkpoint", setup["ckpt"], "--width", str(WIDTH), "--json"]

    def run(extra):
        assert detect.main(common + extra) == 0
        lines = [json.loads(ln) for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
        return [[(e["label"], e["onset"], e["offset"], e["peak"], e["mean"]) for e in ln["events"]] for ln in lines]

    det = detection.EADetector(model=setup["model"], labels=CLASSES)
    waves = [det.load_waveform(p) for p in paths]
    pts = sed.load_operating_points(points)
    want = det.detect(waves, threshold=pts["threshold"], low_threshold=pts["low_threshold"], **POST)
    got = run(["--thresholds_file", points])
    assert got == [[tuple(e) for e in evs] for evs in want] and sum(len(g) for g in got) > 0
    # an explicit flag still wins over the file
    want = det.detect(waves, threshold=0.45, median_ms=320, min_duration_ms=640, max_gap_ms=320)
    assert run(["--thresholds_file", points, "--threshold", "0.45", "--median_ms", "320"]) == [[tuple(e) for e in evs] for evs in want]
    # the class count must match the model
    ev["best_threshold"], ev["best_low_threshold"] = ev["best_threshold"][:2], ev["best_low_threshold"][:2]
    sed.save_operating_points(points, ev, CLASSES[:2])
    with pytest.raises(SystemExit, match="holds 2 classes, the model 3"):
        detect.main(common + ["--thresholds_file", points])
