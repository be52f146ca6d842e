"""ESC-50 fine-tuning end to end (efficientat_amd/finetune.py, finetune_esc50.py): the trainers against the reference's loss
expression, the captured step against the eager one, the program on a synthetic ESC-50 folder, and a learning check."""
import contextlib
import csv
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import ops  # noqa: E402
from efficientat_amd.esc50 import draw_augment  # noqa: E402
from efficientat_amd.finetune import CETrainer, GraphedCETrainer, evaluate_accuracy  # noqa: E402
from efficientat_amd.optim import FusedAdam  # noqa: E402
from efficientat_amd.preprocess import AugmentMelSTFT  # noqa: E402
from efficientat_amd.train_loop import mixup  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _model(name="mn10", seed=0, dropout_off=True, B=None):
    torch.manual_seed(seed)
    if name.startswith("dymn"):
        from efficientat_amd.dymn import get_model
        m = _quiet(get_model, num_classes=50, width_mult=1.0)
    else:
        from efficientat_amd.mn import get_model
        m = _quiet(get_model, num_classes=50, width_mult=1.0)
    m = m.to(DEV).train()
    m.train_precision = "fp32"
    if dropout_off and B is not None and name.startswith("mn"):
        m._drop_mask_override = torch.full((B, m.classifier[2].out_features), 0.8, device=DEV)
    return m


def _mel():
    return _quiet(AugmentMelSTFT, freqm=0, timem=0).to(DEV).train()


def _bank(n, L, seed=0):
    g = torch.Generator().manual_seed(seed)
    bank = (torch.randn(n, L, generator=g) * 0.1).float()
    t = torch.arange(L) / 32000.0
    cls = torch.arange(n, dtype=torch.int32) % 50
    for i in range(n):
        bank[i] += 0.3 * torch.sin(2 * np.pi * (200.0 + 150.0 * float(cls[i])) * t)
    return bank.to(DEV), bank.double().mean(1).to(DEV), cls.to(DEV)


def test_ce_trainer_step_matches_the_reference_loss_expression():
    """A CETrainer step (augment -> mel -> mix-up -> model -> eat_softmax_ce_fwd_bwd -> backward) against the same HIP model's
    logits fed to ex_esc50.py:109-112's two F.cross_entropy terms: same loss, same gradient of every parameter."""
    B, L = 16, 160000
    bank, mean, cls = _bank(40, L)
    batch = list(range(3, 3 + B))
    res = {}
    for tag in ("kernel", "reference"):
        m = _model(B=B)
        mel = _mel()
        torch.manual_seed(21); np.random.seed(21)
        if tag == "kernel":
            tr = CETrainer(m, mel, FusedAdam(m.parameters(), lr=1e-3), bank, mean, cls, mixup_alpha=0.3)
            loss = tr.loss_and_backward(batch)
        else:
            draws = draw_augment(batch, bank.shape[0], 12, True, True)
            x, y = ops.wave_augment(bank, mean, cls, *draws, 50)
            spec = mel(x).unsqueeze(1)
            rn, lam = mixup(B, 0.3)
            spec = ops.mixup_fwd(spec, rn.to(DEV, torch.int32), lam.to(DEV))
            y_hat, _ = m(spec)
            lam = lam.to(DEV)
            loss = (F.cross_entropy(y_hat, y, reduction="none") * lam
                    + F.cross_entropy(y_hat, y[rn.to(DEV)], reduction="none") * (1. - lam)).mean()
            loss.backward()
        torch.cuda.synchronize()
        res[tag] = (float(loss.detach()), {n: p.grad.detach().cpu().double() for n, p in m.named_parameters()})
    lk, lr_ = res["kernel"][0], res["reference"][0]
    assert abs(lk - lr_) <= 1e-5 * max(1.0, abs(lr_)), (lk, lr_)
    # per tensor, relative to its own largest gradient, plus an absolute floor of 1e-6 of the model's largest gradient: a bias
    # in front of a BatchNorm has a gradient that is round-off (~1e-7 of the largest one, measured), which differs by its own size
    gmax = max(float(g.abs().max()) for g in res["reference"][1].values())
    worst = 0.0
    for n, gr in res["reference"][1].items():
        gk = res["kernel"][1][n]
        scale = float(gr.abs().max())
        err = float((gk - gr).abs().max())
        worst = max(worst, err / (1e-4 * scale + 1e-6 * gmax))
        assert err <= 1e-4 * scale + 1e-6 * gmax, (n, err, scale, gmax)
    print(f"loss {lk:.6f} / {lr_:.6f}; worst per-tensor max|dgrad| / (1e-4 max|grad| + 1e-6 gmax) {worst:.2e}")


def _run_trainer(graphed, steps=3, B=6, L=32000, lr=1e-3, name="mn10", dropout_off=True):
    bank, mean, cls = _bank(30, L, seed=2)
    m = _model(name, B=B, dropout_off=dropout_off)
    mel = _mel()
    opt = FusedAdam(m.parameters(), lr=torch.tensor(lr, device=DEV), capturable=True)
    kw = dict(mixup_alpha=0.3)
    tr = GraphedCETrainer(m, mel, opt, bank, mean, cls, B, **kw) if graphed else CETrainer(m, mel, opt, bank, mean, cls, **kw)
    torch.manual_seed(11); np.random.seed(11)
    losses = []
    for s in range(steps):
        batch = torch.randperm(30)[:B].tolist()
        losses.append(float(tr.step(batch)))
    torch.cuda.synchronize()
    return tr, m, losses


def test_graphed_ce_trainer_follows_the_eager_trainer():
    """Three seeded steps, captured vs eager: the tolerances of test_graphed_kd_trainer_follows_the_eager_trainer."""
    res = {}
    for graphed in (False, True):
        tr, m, losses = _run_trainer(graphed)
        rm = torch.cat([b.detach().float().reshape(-1) for n, b in m.named_buffers() if n.endswith("running_mean")]).cpu()
        res[graphed] = (losses, torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu(), tr.epoch_stats(), rm)
    le, lg = res[False][0], res[True][0]
    assert all(abs(a - b) < 2e-5 * max(1.0, abs(a)) for a, b in zip(le, lg)), (le, lg)
    d = (res[False][1] - res[True][1]).abs()
    frac = float((d > 1e-4).float().mean())
    print(f"losses {le} / {lg}; params max |eager - graph| {float(d.max()):.2e}, fraction above 1e-4 {frac:.2e}")
    assert float(d.max()) <= 6.1e-3 and frac < 0.02, (float(d.max()), frac)
    se, sg = res[False][2]["train_loss"], res[True][2]["train_loss"]
    assert abs(se - sg) < 2e-5 * max(1.0, abs(se)) and abs(se - np.mean(le)) < 1e-5 * max(1.0, abs(se))
    # the capture's warm-up steps must not leak into the BatchNorm running statistics (restored after the capture)
    drm = float((res[False][3] - res[True][3]).abs().max())
    print(f"running_mean max |eager - graph| {drm:.2e} (max |rm| {float(res[False][3].abs().max()):.2e})")
    assert drm < 1e-4 * max(1.0, float(res[False][3].abs().max())), drm


class _CountingGraph:
    def __init__(self, g):
        self.g, self.n = g, 0

    def replay(self):
        self.n += 1
        self.g.replay()


def test_graphed_ce_trainer_lr0_replay_and_partial_batch():
    """lr = 0: a replay leaves every parameter bit-identical (the warm-up of the capture is undone too); a partial batch takes
    the eager step and does not replay."""
    B = 6
    tr, m, _ = _run_trainer(True, steps=0, lr=0.0, B=B, dropout_off=False)
    before = [p.detach().clone() for p in m.parameters()]
    tr.graph = _CountingGraph(tr.graph)
    torch.manual_seed(3); np.random.seed(3)
    loss = float(tr.step(list(range(B))))
    torch.cuda.synchronize()
    assert tr.graph.n == 1 and np.isfinite(loss)
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
    loss = float(tr.step(list(range(B - 2))))
    torch.cuda.synchronize()
    assert tr.graph.n == 1 and np.isfinite(loss) and tr.steps == 2
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))


def test_dymn10_eager_and_captured_steps():
    for graphed in (False, True):
        tr, m, losses = _run_trainer(graphed, steps=1, B=4, name="dymn10")
        assert np.isfinite(losses).all(), losses
        if graphed:
            m.update_params(3)
            tr.recapture()
            torch.manual_seed(1); np.random.seed(1)
            assert np.isfinite(float(tr.step([0, 1, 2, 3])))
        torch.cuda.synchronize()


def test_mn10_overfits_one_batch_of_tones():
    """Learning: one fixed batch of class-specific tones (no augmentation, no mix-up), 40 captured steps at lr 1e-3.  Measured
    on one MI355X: 3.919 -> 0.0009; the bar leaves a 50x margin on the final loss."""
    B, L = 8, 32000
    t = torch.arange(L) / 32000.0
    cls = torch.tensor([0, 7, 13, 21, 28, 35, 42, 49], dtype=torch.int32)
    bank = torch.stack([0.4 * torch.sin(2 * np.pi * (150.0 + 250.0 * float(c)) * t) for c in cls]).float()
    m = _model(B=B, dropout_off=False)
    mel = _mel()
    opt = FusedAdam(m.parameters(), lr=torch.tensor(1e-3, device=DEV), capturable=True)
    tr = GraphedCETrainer(m, mel, opt, bank.to(DEV), bank.double().mean(1).to(DEV), cls.to(DEV), B, mixup_alpha=0,
                          gain_augment=0, roll=False, wavmix=False)
    torch.manual_seed(0); np.random.seed(0)
    losses = [float(tr.step(list(range(B)))) for _ in range(40)]
    ev = evaluate_accuracy(m, mel, bank.to(DEV), cls.to(DEV), B)
    print(f"losses {losses[0]:.4f} -> {losses[-1]:.4f}; eval accuracy {ev['accuracy']:.3f}, val_loss {ev['val_loss']:.4f}")
    assert losses[0] > 3.5 and losses[-1] < 0.05, losses


def _synthetic_esc50(root, n_per_class_fold=1, seconds=0.5):
    os.makedirs(os.path.join(root, "meta"))
    os.makedirs(os.path.join(root, "audio_32k"))
    from scipy.io import wavfile
    rng = np.random.default_rng(0)
    n = int(32000 * seconds)
    t = np.arange(n) / 32000.0
    rows = []
    for fold in range(1, 6):
        for c in range(50):
            for k in range(n_per_class_fold):
                name = f"{fold}-{c}{k}-A-{c}.wav"
                x = 0.3 * np.sin(2 * np.pi * (150.0 + 120.0 * c) * t) + 0.05 * rng.standard_normal(n)
                wavfile.write(os.path.join(root, "audio_32k", name), 32000, (x * 32767).astype(np.int16))
                rows.append((name, fold, c))
    with open(os.path.join(root, "meta", "esc50.csv"), "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["filename", "fold", "target", "category", "esc10", "src_file", "take"])
        for r in rows:
            w.writerow([r[0], r[1], r[2], "x", "False", "x", "A"])


def _program(args, timeout=420):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, "-m", "efficientat_amd.finetune_esc50"] + args, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-4000:]
    return json.loads(p.stdout.strip().splitlines()[-1]), p.stderr


def test_program_on_a_synthetic_esc50_folder(tmp_path):
    data = str(tmp_path / "esc50")
    _synthetic_esc50(data)
    out, dump = str(tmp_path / "out"), str(tmp_path / "dump")
    line, err = _program(["--data", data, "--n_epochs", "2", "--batch_size", "32", "--json", "--out", out, "--eval_dump", dump,
                          "--lr", "1e-3", "--warm_up_len", "1"])
    print(err[-1500:])
    print(json.dumps(line))
    for k in ("accuracy", "val_loss", "train_loss", "clips_per_s", "eval_clips_per_s"):
        assert np.isfinite(line[k]), k
    assert line["launch"] == "hipGraph replay" and line["steps"] == 2 * 7
    logits = np.load(os.path.join(dump, "logits.npy")).astype(np.float64)
    targets = np.load(os.path.join(dump, "targets.npy")).astype(np.float64)
    assert logits.shape == (50, 50) and targets.shape == (50, 50)
    acc = float((logits.argmax(1) == targets.argmax(1)).mean())
    lse = logits.max(1) + np.log(np.exp(logits - logits.max(1, keepdims=True)).sum(1))
    ce = (targets * (lse[:, None] - logits)).sum(1)
    val_loss = float(np.mean([ce[s:s + 32].mean() for s in range(0, 50, 32)]))
    assert abs(acc - line["accuracy"]) <= 1e-6 and abs(val_loss - line["val_loss"]) <= 1e-6, (acc, val_loss, line)
    assert os.listdir(out) == [f"mn10_esc50_epoch_1_acc_{int(round(line['accuracy'] * 1000))}.pt"]
    line, _ = _program(["--data", data, "--n_epochs", "1", "--batch_size", "32", "--json", "--no_graph", "--max_steps", "2"])
    assert line["launch"] == "eager" and line["steps"] == 2 and np.isfinite(line["accuracy"])
