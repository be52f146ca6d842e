"""Per-epoch validation of `python -m efficientat_amd.train_dp` (--eval_every / --eval_only / --eval_dump) on the synthetic
AudioSet stand-in with an odd test-set size (301 clips: the shards of two ranks have a tail)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
from tests import rank_metrics_ref as R  # noqa: E402

N_TEST = 301
DEV = torch.device("cuda:0")


def _env():
    env = dict(os.environ, EAT_SYNTH_AUDIOSET="1", EAT_SYNTH_AUDIOSET_TRAIN="64", EAT_SYNTH_AUDIOSET_TEST=str(N_TEST),
               PYTHONPATH=ROOT)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def _json(r):
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def _run(args, tmp_path, ranks=1):
    if ranks == 1:
        cmd = [sys.executable, "-m", "efficientat_amd.train_dp"]
    else:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ranks}", "--master-addr",
               "127.0.0.1", "--master-port", str(port), "-m", "efficientat_amd.train_dp", "--backend", "gloo"]
    return subprocess.run(cmd + args, capture_output=True, text=True, timeout=900, env=_env(), cwd=str(tmp_path))


def _test_set():
    os.environ["EAT_SYNTH_AUDIOSET"] = "1"                    # explicit opt-in to the synthetic stand-in
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    from datasets import audioset
    return audioset._SyntheticAudioSet(("eval", N_TEST, 527 << 12))   # this size whatever the module was imported with


def _checkpoint(path):
    import contextlib
    import io
    from efficientat_amd.mn import get_model
    torch.manual_seed(4)
    with contextlib.redirect_stdout(io.StringIO()):
        m = get_model(width_mult=0.5)
    torch.save(m.state_dict(), path)


def _eager_logits(ck):
    import contextlib
    import io
    from efficientat_amd.mn import get_model
    from efficientat_amd.preprocess import AugmentMelSTFT
    with contextlib.redirect_stdout(io.StringIO()):
        m = get_model(width_mult=0.5)
        mel = AugmentMelSTFT(freqm=0, timem=0).to(DEV).eval()
    m.load_state_dict(torch.load(ck, map_location="cpu"))
    m.to(DEV).eval()
    ds = _test_set()
    out = []
    with torch.no_grad():
        for i0 in range(0, N_TEST, 50):
            x = torch.stack([torch.from_numpy(ds[i][0]) for i in range(i0, min(N_TEST, i0 + 50))]).to(DEV)
            y_hat, _ = m(mel(x.reshape(x.shape[0], -1)).unsqueeze(1))
            out.append(y_hat.cpu())
    return torch.cat(out).numpy(), ds.targets()


def _check_metrics_of_dump(ev, dump):
    logits, targets = np.load(os.path.join(dump, "logits.npy")), np.load(os.path.join(dump, "targets.npy"))
    assert logits.shape == (N_TEST, 527) and targets.shape == (N_TEST, 527)
    ap, auc = R.ap_auc(logits, targets)
    assert abs(ev["mAP"] - ap.mean()) < 1e-9, (ev, ap.mean())
    assert np.isnan(ev["ROC"]) == np.isnan(auc.mean()) and (np.isnan(ev["ROC"]) or abs(ev["ROC"] - auc.mean()) < 1e-9)
    return logits, targets


@pytest.fixture(scope="module")
def one_rank(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("eval1")
    ck = str(tmp / "ck.pt")
    _checkpoint(ck)
    r = _run(["--eval_only", "--checkpoint", ck, "--model_width", "0.5", "--batch_size", "40", "--num_workers", "2",
              "--eval_dump", str(tmp / "dump"), "--json"], tmp)
    return ck, _json(r), str(tmp / "dump")


def test_eval_only_one_gpu_reports_every_clip_and_the_metric_of_its_dump(one_rank):
    ck, line, dump = one_rank
    ev = line["eval"]
    assert line["mode"] == "eval_only" and ev["n_clips"] == N_TEST and ev["clips_per_s"] > 0 and np.isfinite(ev["val_loss"])
    logits, targets = _check_metrics_of_dump(ev, dump)
    ref, ref_t = _eager_logits(ck)
    scale = float(np.abs(ref).max())
    assert float(np.abs(logits - ref).max()) <= 1e-4 * scale, float(np.abs(logits - ref).max())
    assert np.array_equal(targets, ref_t)
    bce = torch.nn.functional.binary_cross_entropy_with_logits(torch.from_numpy(logits).double(), torch.from_numpy(targets).double())
    assert abs(ev["val_loss"] - float(bce)) < 1e-5


def test_eval_only_two_gloo_ranks_gather_in_test_set_order(one_rank, tmp_path):
    _, _, dump1 = one_rank
    ck = one_rank[0]
    r = _run(["--eval_only", "--checkpoint", ck, "--model_width", "0.5", "--batch_size", "32", "--num_workers", "1",
              "--eval_dump", str(tmp_path / "dump"), "--json"], tmp_path, ranks=2)
    if r.returncode != 0 and "gloo" in r.stderr and "not supported" in r.stderr.lower():
        pytest.skip("this torch build's gloo does not gather device tensors: " + r.stderr[-300:])
    line = _json(r)
    ev = line["eval"]
    assert line["n_gpus"] == 2 and ev["n_clips"] == N_TEST
    logits, targets = _check_metrics_of_dump(ev, str(tmp_path / "dump"))
    l1, t1 = np.load(os.path.join(dump1, "logits.npy")), np.load(os.path.join(dump1, "targets.npy"))
    assert np.array_equal(targets, t1)
    assert float(np.abs(logits - l1).max()) <= 1e-5 * float(np.abs(l1).max())


@pytest.mark.parametrize("graph", [False, True])
def test_eval_every_epoch_does_not_perturb_training(tmp_path, graph):
    """Two one-step epochs with an evaluation after each: the same final parameters as without evaluation, eager and
    captured (the captured step replays after an eager eval pass; no RNG is consumed, BatchNorm statistics unchanged)."""
    base = ["--model_width", "0.5", "--batch_size", "8", "--num_workers", "1", "--n_epochs", "2", "--epoch_len", "8",
            "--max_steps", "2", "--max_lr", "5e-3", "--json"] + ([] if graph else ["--no_graph"])
    plain = _json(_run(base, tmp_path))
    ev = _json(_run(base + ["--eval_every", "1", "--eval_batch_size", "64"], tmp_path))
    print("param_abs_sum", plain["param_abs_sum"], ev["param_abs_sum"])
    assert "eval" not in plain and plain["steps"] == ev["steps"] == 2
    assert [e["epoch"] for e in ev["eval"]] == [0, 1] and all(e["n_clips"] == N_TEST for e in ev["eval"])
    assert ev["param_abs_sum"] == pytest.approx(plain["param_abs_sum"], rel=5e-8, abs=0)
    assert ev["eval"][0]["mAP"] != ev["eval"][1]["mAP"]             # the second evaluation saw the trained weights
