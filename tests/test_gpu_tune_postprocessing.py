"""Per-class median tuning end to end: the two-class case of tests/tune_case.py through the kernels (`sed._sweep_timelines`),
then on a model - `sed.tune_postprocessing` against one `sed.evaluate_events` per width, `detect` with per-class widths
against one `detect` per width, and the programs: `score_sed --tune_median / --operating_points`, `detect --thresholds_file`
with `class_median_ms`, and the key sets of the runs without the new flags.  Counts are integers and compared for equality."""
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

from efficientat_amd import detect, detection, finetune_sed, ops, score_sed, sed  # noqa: E402
from efficientat_amd.mn import get_model  # noqa: E402
from efficientat_amd.preprocess import AugmentMelSTFT  # noqa: E402
from tests import tune_case as C  # noqa: E402

DEV = torch.device("cuda:0")
SR, K, WIDTH = 32000, 3, 0.5
SECONDS = (3.0, 12.0, 5.3, 7.77, 10.24, 4.1)
CLASSES = ["alarm", "dog", "speech"]
LOW_RATIO = 0.8
GRID_MS = [0.0, 960.0, 1600.0, 2240.0, 4160.0]                                # 1, 3, 5, 7 and 13 frames of 320 ms
FRAMES = [1, 3, 5, 7, 13]
# the JSON lines of the two programs as they were before --tune_median and --operating_points existed
SCORE_KEYS = ["what", "checkpoint", "classes", "n_clips", "n_ref"] + list(finetune_sed.EVENT_KEYS)
FINETUNE_KEYS = ["what", "model", "classes", "steps", "epochs", "batch_size", "clip_samples", "launch", "threshold", "train_loss",
                 "clips_per_s", "n_frames", "eval_s", "checkpoint", "frame_mAP", "frame_ROC", "micro_f1", "micro_precision",
                 "micro_recall", "macro_f1", "macro_precision", "macro_recall", "val_loss"] + list(finetune_sed.EVENT_KEYS)
TUNED_KEYS = ["macro_f1_tuned", "macro_f1_best_single", "best_single_median_ms", "best_median_ms"]


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _mel():
    return _quiet(AugmentMelSTFT, freqm=0, timem=0).to(DEV).eval()


# ------------------------------------------------------------------------------------------------ the two-class case
def test_no_single_width_serves_both_classes():
    prob, rec, nsamp, ref, ro = C.build()
    table = ops.detect_table(rec)
    refs = ops.event_refs(torch.from_numpy(ref), torch.from_numpy(sed.event_tolerances(ref, C.COLLAR, C.PCT)), torch.from_numpy(ro), C.K)
    widths = ops.median_width_table(np.repeat(np.asarray(C.WIDTHS)[:, None], C.K, axis=1), C.K)
    hi, lo = sed.threshold_grid([0.5])
    res = sed._sweep_timelines(torch.from_numpy(prob).to(DEV), table, nsamp, C.R, refs, C.COLLAR, widths, hi, lo, 0, 0)
    assert res.shape == (len(C.WIDTHS), C.K, 1, 2) and res.dtype == torch.int64 and res.is_cuda
    res = res.cpu().numpy()
    got = {m: tuple(tuple(int(v) for v in res[j, k, 0]) for k in range(C.K)) for j, m in enumerate(C.WIDTHS)}
    print(f"(tp, n_est) per width and class: {got}")
    assert got == C.EXPECTED
    counts = C.counts_grid(res)
    at, best_j, best_v, b_hi, _ = sed.pick_operating_points(counts, hi, lo, 0.5, 1)
    assert [C.WIDTHS[j] for j in best_j] == [5, 3] and best_v.tolist() == [0, 0] and b_hi.tolist() == [0.5, 0.5]
    tuned = sed.tuned_scores(counts, hi, lo, 0.5, 1)
    assert tuned["macro_f1_tuned"] == 1.0 and tuned["macro_f1_best_single"] == 0.5
    single = [sed.segment_scores(counts[j, 0])["macro_f1"] for j in range(len(C.WIDTHS))]
    assert max(single) == 0.5 and single[-1] == 0.0 and single[0] == pytest.approx(1 / 3, abs=1e-15)


# ------------------------------------------------------------------------------------------------ on a model
def _waves():
    """Noise with tone bursts that come and go, so that the frame probabilities of a random model move in time."""
    rng = np.random.RandomState(11)
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
    """A narrow random mlp-head MN rescaled per class so that its frame probabilities straddle 0.5, six clips of 3 - 12 s, and a
    bank whose reference events are the model's own at a 3-frame median and 0.5 / 0.4, some moved off the frame grid, plus
    two events the model does not find."""
    torch.manual_seed(37)
    model = _quiet(get_model, width_mult=WIDTH, num_classes=K, head_type="mlp").to(DEV).eval()
    waves = _waves()
    det = detection.EADetector(model=model)
    with torch.no_grad():
        g = torch.Generator().manual_seed(41)                                 # (the trunk of a fresh model is degenerate)
        for mod in model.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.copy_(0.1 * torch.randn(mod.running_mean.shape, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=g))
                mod.weight.copy_(0.8 + 0.4 * torch.rand(mod.weight.shape, generator=g))
                mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
        starts, valids, _ = det.plan([len(w) for w in waves])
        P = det.window_logits(torch.from_numpy(np.concatenate(waves)).to(DEV), starts, valids)
        z = P[:, :, :det.geometry.T].permute(0, 2, 1).reshape(-1, K).double()
        q = torch.quantile(z, torch.tensor([0.1, 0.5, 0.9], dtype=torch.float64, device=z.device), dim=0)
        spread, med = q[2] - q[0], q[1]
        assert bool(torch.isfinite(z).all()) and float(spread.min()) > 0
        scale = (2.0 / spread).float()                                        # four fifths of the frames within a logit of +- 1
        model.classifier[5].weight.mul_(scale.view(K, 1))
        model.classifier[5].bias.copy_(scale * (model.classifier[5].bias - med.float()))
    found = det.detect([torch.from_numpy(w) for w in waves], threshold=0.5, low_threshold=0.4, median_ms=960)
    rng = np.random.RandomState(5)
    events, eo = [], [0]
    for i, (w, evs) in enumerate(zip(waves, found)):
        n, mine = len(w), []
        for j, (k, on_s, off_s, _, _) in enumerate(evs):
            on, off = int(round(on_s * SR)), int(round(off_s * SR))
            if j > 0 and rng.rand() > 1 / 3:
                on, off = on + rng.randint(-9600, 9601), off + rng.randint(-9600, 9601)
            on = min(max(on, 0), n - 1)
            mine.append((int(k), on, min(max(off, on + 1), n)))
        if i in (0, 1):
            mine.append((i, 777, 777 + SR))
        events.extend(sorted(mine))
        eo.append(len(events))
    d = str(tmp_path_factory.mktemp("tune_bank"))
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
    return dict(dir=d, model=model, det=det, waves=waves, ckpt=ckpt, bank=sed.load_bank(d, device=DEV))


def _tune(s, **kw):
    return sed.tune_postprocessing(s["model"], _mel(), s["bank"], median_grid_ms=GRID_MS, median_ms=960, low_ratio=LOW_RATIO, **kw)


@pytest.fixture(scope="module")
def tuned(setup):
    return _tune(setup)


def test_every_width_of_the_grid_counts_what_evaluate_events_counts(setup, tuned):
    s, t = setup, tuned
    assert t["median_frames"].tolist() == FRAMES and t["median_ms_grid"].tolist() == [320.0 * m for m in FRAMES]
    assert t["counts_grid"].shape == (len(FRAMES), 49, K, 3) and t["counts_grid"].dtype == np.int64
    assert t["class_f1_grid"].shape == (len(FRAMES), 49, K)
    n_est = []
    for j, ms in enumerate(t["median_ms_grid"].tolist()):
        ev = sed.evaluate_events(s["model"], _mel(), s["bank"], median_ms=ms, low_ratio=LOW_RATIO)
        assert np.array_equal(t["counts_grid"][j], ev["counts"]), f"width {FRAMES[j]}"
        n_est.append(int(ev["counts"][:, :, :2].sum()))
        if FRAMES[j] == 3:                                                    # the reference width: evaluate_events' own result
            assert np.array_equal(t["counts"], ev["counts"]) and t["macro_f1_best"] == ev["macro_f1_best"]
            assert all(t[k] == pytest.approx(ev[k], abs=0, nan_ok=True) for k in sed.SCORE_NAMES)
            assert t["threshold"] == ev["threshold"] == 0.5 and t["n_ref"] == ev["n_ref"] and t["n_clips"] == len(SECONDS)
            assert {k: v for k, v in t["settings"].items() if k != "frame_ms"} == ev["settings"] and t["settings"]["frame_ms"] == 320.0
    print(f"tune_postprocessing: estimated events per width {dict(zip(FRAMES, n_est))}, true positives "
          f"{t['counts_grid'][:, :, :, 0].sum(axis=(1, 2)).tolist()}")
    assert t["counts_grid"][:, :, :, 0].sum() > 0                             # some true positive exists
    assert len(set(n_est)) > 1                                                # and the widths see different event lists
    # the choice and the figures, recomputed from the counts
    want = sed.tuned_scores(t["counts_grid"], t["thresholds"], t["low_thresholds"], 0.5, 1, LOW_RATIO)
    for key in ("best_median_index", "best_index", "best_threshold", "best_low_threshold"):
        assert np.array_equal(t[key], want[key]), key
    assert t["best_median_frames"].tolist() == [FRAMES[j] for j in t["best_median_index"]]
    assert t["best_median_ms"].tolist() == [320.0 * m for m in t["best_median_frames"]]
    assert t["macro_f1_tuned"] == want["macro_f1_tuned"] and t["macro_f1_best_single"] == want["macro_f1_best_single"]
    if bool((np.bincount(s["bank"]["events"][:, 0].cpu().numpy(), minlength=K) > 0).all()):
        # every class has references, so every point averages the same classes: a wider choice cannot score less
        assert t["macro_f1_tuned"] >= t["macro_f1_best_single"] >= t["macro_f1_best"]
    assert t["best_single_median_ms"] == 320.0 * FRAMES[want["best_single_index"]]


def test_the_grid_does_not_depend_on_the_chunking(setup, tuned):
    for batch_clips in (1, 4):
        assert np.array_equal(_tune(setup, batch_clips=batch_clips)["counts_grid"], tuned["counts_grid"]), batch_clips


def test_detect_with_per_class_widths_lists_each_class_as_at_its_own_width(setup):
    det = setup["det"]
    waves = [torch.from_numpy(w) for w in setup["waves"]]
    ms = [2240.0, 0.0, 960.0]                                                 # 7, 1 and 3 frames
    kw = dict(threshold=[0.5, 0.45, 0.55], low_threshold=[0.4, 0.45, 0.3])
    got = det.detect(waves, median_ms=np.asarray(ms), **kw)
    n = 0
    for k in range(K):
        one = det.detect(waves, median_ms=ms[k], **kw)
        for g, o in zip(got, one):
            mine = [e for e in g if e[0] == k]
            assert mine == [e for e in o if e[0] == k], k
            n += len(mine)
    assert n > 0
    assert det.detect(waves, median_ms=[960.0] * K, **kw) == det.detect(waves, median_ms=960, **kw)
    with pytest.raises(ValueError, match="class 1"):
        det.detect(waves, median_ms=[960.0, 99999.0, 0.0])


def test_evaluate_psds_with_equal_per_class_widths_is_the_scalar_call(setup):
    a = sed.evaluate_psds(setup["model"], _mel(), setup["bank"], scenario=2, median_ms=960, low_ratio=LOW_RATIO)
    b = sed.evaluate_psds(setup["model"], _mel(), setup["bank"], scenario=2, median_ms=[960.0] * K, low_ratio=LOW_RATIO)
    assert np.array_equal(a["counts"], b["counts"]) and np.array_equal(a["ct"], b["ct"]) and np.array_equal(a["n_det"], b["n_det"])
    assert a["psds"] == pytest.approx(b["psds"], abs=0, nan_ok=True) and a["counts"][:, :, 0].sum() > 0
    assert b["settings"]["class_median_ms"] == [960.0] * K and b["settings"]["median_ms"] == a["settings"]["median_ms"] == 960.0
    assert "class_median_ms" not in a["settings"]
    # unequal widths: every class is counted as at its own width (tp, fp and n_det of a class do not depend on the others)
    ms = [4160.0, 0.0, 960.0]
    c = sed.evaluate_psds(setup["model"], _mel(), setup["bank"], scenario=2, median_ms=ms, low_ratio=LOW_RATIO)
    for k in range(K):
        one = a if ms[k] == 960.0 else sed.evaluate_psds(setup["model"], _mel(), setup["bank"], scenario=2, median_ms=ms[k],
                                                         low_ratio=LOW_RATIO)
        assert np.array_equal(c["counts"][:, k], one["counts"][:, k]) and np.array_equal(c["n_det"][:, k], one["n_det"][:, k]), k
    assert not np.array_equal(c["n_det"], a["n_det"]) and c["settings"]["class_median_ms"] == ms


# ------------------------------------------------------------------------------------------------ the programs
def _json_line(capsys):
    return json.loads([ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")][-1])


def test_score_sed_tunes_saves_and_scores_the_saved_points(setup, tuned, tmp_path, capsys):
    points = str(tmp_path / "ops.json")
    base = ["--checkpoint", setup["ckpt"], "--bank", setup["dir"], "--width", str(WIDTH), "--json", "--low_ratio", str(LOW_RATIO)]
    assert score_sed.main(base) == 0
    plain = _json_line(capsys)
    assert list(plain) == SCORE_KEYS                                          # without the new flags: the line as it was
    assert score_sed.main(base + ["--tune_median", "--median_grid_ms", ",".join(str(v) for v in GRID_MS),
                                  "--save_thresholds", points]) == 0
    line = _json_line(capsys)
    assert list(line) == SCORE_KEYS + TUNED_KEYS
    assert {k: v for k, v in line.items() if k not in TUNED_KEYS + ["event_eval_s", "thresholds_file", "event_best_threshold"]} == \
        {k: v for k, v in plain.items() if k not in ("event_eval_s", "thresholds_file", "event_best_threshold")}
    assert line["macro_f1_tuned"] == tuned["macro_f1_tuned"] and line["macro_f1_best_single"] == tuned["macro_f1_best_single"]
    assert line["best_median_ms"] == tuned["best_median_ms"].tolist()
    assert line["event_best_threshold"] == [float(v) for v in tuned["best_threshold"]]
    pts = sed.load_operating_points(points, classes=CLASSES)
    assert pts["class_median_ms"].tolist() == line["best_median_ms"] and pts["median_ms"] == 960.0
    assert pts["threshold"].tolist() == line["event_best_threshold"]
    # the saved file, scored as it stands on the split it was tuned on: exactly the tuned figure
    assert score_sed.main(base + ["--operating_points", points, "--psds", "1"]) == 0
    at = _json_line(capsys)
    assert at["macro_f1_at_ops"] == line["macro_f1_tuned"]
    assert list(at) == SCORE_KEYS[:5] + list(finetune_sed.EVENT_KEYS) + [k + "_at_ops" for k in sed.SCORE_NAMES] + \
        ["operating_points", "eval_s_at_ops", "psds_scenario1", "psds_eval_s"]
    res = sed.score_operating_points(setup["model"], _mel(), setup["bank"], pts, batch_clips=4)
    assert res["macro_f1"] == tuned["macro_f1_tuned"] and res["counts"].shape == (K, 3) and res["n_clips"] == len(SECONDS)
    j, v = tuned["best_median_index"], tuned["best_index"]
    assert bool((v >= 0).all()) and np.array_equal(res["counts"], tuned["counts_grid"][j, v, np.arange(K)])
    ps = sed.evaluate_psds(setup["model"], _mel(), setup["bank"], scenario=1, median_ms=pts["class_median_ms"], low_ratio=LOW_RATIO)
    assert at["psds_scenario1"] == pytest.approx(ps["psds"], abs=0, nan_ok=True)   # PSDS ran at the file's widths

    # detect --thresholds_file runs with the file's widths; an explicit --median_ms wins for all classes
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
    kw = dict(threshold=pts["threshold"], low_threshold=pts["low_threshold"])
    want = det.detect(waves, median_ms=pts["class_median_ms"], **kw)
    assert run(["--thresholds_file", points]) == [[tuple(e) for e in evs] for evs in want] and sum(len(e) for e in want) > 0
    want = det.detect(waves, median_ms=4160, **kw)
    assert run(["--thresholds_file", points, "--median_ms", "4160"]) == [[tuple(e) for e in evs] for evs in want]


def test_finetune_sed_event_eval_without_the_new_flags_prints_the_keys_it_printed(setup, capsys):
    argv = ["--train_bank", setup["dir"], "--valid_bank", setup["dir"], "--batch_size", "4", "--clip_frames", "3", "--n_epochs", "1",
            "--lr", "1e-3", "--warm_up_len", "1", "--model_width", str(WIDTH), "--no_graph", "--max_steps", "1", "--json",
            "--event_eval"]
    finetune_sed.main(argv)
    assert list(_json_line(capsys)) == FINETUNE_KEYS


def test_finetune_sed_tune_median_adds_its_keys_and_writes_class_median_ms(setup, tmp_path, capsys):
    points = str(tmp_path / "ops.json")
    finetune_sed.main(["--train_bank", setup["dir"], "--valid_bank", setup["dir"], "--batch_size", "4", "--clip_frames", "3",
                       "--n_epochs", "1", "--lr", "1e-3", "--warm_up_len", "1", "--model_width", str(WIDTH), "--no_graph",
                       "--max_steps", "1", "--json", "--event_eval", "--tune_median", "--median_grid_ms", "0,1600",
                       "--save_thresholds", points])
    line = _json_line(capsys)
    assert list(line) == FINETUNE_KEYS + TUNED_KEYS and len(line["best_median_ms"]) == K
    assert set(line["best_median_ms"]) <= {320.0, 960.0, 1600.0} and line["best_single_median_ms"] in (320.0, 960.0, 1600.0)
    pts = sed.load_operating_points(points, classes=CLASSES)
    assert pts["class_median_ms"].tolist() == line["best_median_ms"] and pts["threshold"].tolist() == line["event_best_threshold"]
    assert pts["scores"]["macro_f1_tuned"] == pytest.approx(line["macro_f1_tuned"], abs=0, nan_ok=True)
