"""DCASE20 fine-tuning end to end (efficientat_amd/finetune.py SceneCETrainer / GraphedSceneCETrainer, finetune_dcase20.py):
the eager step against the reference's expressions written in torch ops, the captured step against the eager one across
applied and unapplied MixStyle steps, the grouped accuracy, and the program on two synthetic banks."""
import contextlib
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

from efficientat_amd import dcase20, ops, train_loop  # noqa: E402
from efficientat_amd.finetune import GraphedSceneCETrainer, SceneCETrainer, evaluate_accuracy  # noqa: E402
from efficientat_amd.optim import FusedAdam  # noqa: E402
from efficientat_amd.preprocess import AugmentMelSTFT  # noqa: E402
from efficientat_amd.train_loop import mixup  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, L, B, C = 12, 32000, 4, 10                                                  # 1 s clips: 100 mel frames


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _model(name="mn10", seed=0, dropout_off=True, batch=B):
    torch.manual_seed(seed)
    if name.startswith("dymn"):
        from efficientat_amd.dymn import get_model
    else:
        from efficientat_amd.mn import get_model
    m = _quiet(get_model, num_classes=C, width_mult=1.0).to(DEV).train()
    m.train_precision = "fp32"
    if dropout_off and name.startswith("mn"):
        m._drop_mask_override = torch.full((batch, m.classifier[2].out_features), 0.8, device=DEV)
    return m


def _mel():
    return _quiet(AugmentMelSTFT, freqm=0, timem=0).to(DEV).train()


def _bank(n=N, seed=0):
    g = torch.Generator().manual_seed(seed)
    bank = (torch.randn(n, L, generator=g) * 0.1).float()
    t = torch.arange(L) / 32000.0
    cls = torch.arange(n, dtype=torch.int32) % C
    for i in range(n):
        bank[i] += 0.3 * torch.sin(2 * np.pi * (200.0 + 150.0 * float(cls[i])) * t)
    return bank.to(DEV), bank.double().mean(1).to(DEV), cls.to(DEV)


def _states():
    return torch.get_rng_state(), np.random.get_state()


def _same_states(a, b):
    return torch.equal(a[0], b[0]) and a[1][0] == b[1][0] and np.array_equal(a[1][1], b[1][1]) and a[1][2:] == b[1][2:]


def _torch_mixstyle(x, perm, lam, eps=1e-6):
    """dropin/helpers/utils.py `mixstyle` past its draws."""
    lmda = lam.to(x.device).reshape(-1, 1, 1, 1)
    perm = perm.to(x.device)
    mu = x.mean(dim=[1, 3], keepdim=True).detach()
    sig = (x.var(dim=[1, 3], keepdim=True) + eps).sqrt().detach()
    return (x - mu) / sig * (sig * lmda + sig[perm] * (1 - lmda)) + (mu * lmda + mu[perm] * (1 - lmda))


def _compare(res):
    """The bounds of test_gpu_finetune.py::test_ce_trainer_step_matches_the_reference_loss_expression."""
    lk, lr_ = res["kernel"][0], res["reference"][0]
    assert abs(lk - lr_) <= 1e-5 * max(1.0, abs(lr_)), (lk, lr_)
    gmax = max(float(g.abs().max()) for g in res["reference"][1].values())
    worst = 0.0
    for n, gr in res["reference"][1].items():
        gk = res["kernel"][1][n]
        scale = float(gr.abs().max())
        err = float((gk - gr).abs().max())
        worst = max(worst, err / (1e-4 * scale + 1e-6 * gmax))
        assert err <= 1e-4 * scale + 1e-6 * gmax, (n, err, scale, gmax)
    print(f"loss {lk:.6f} / {lr_:.6f}; worst per-tensor max|dgrad| / (1e-4 max|grad| + 1e-6 gmax) {worst:.2e}")
    assert _same_states(res["kernel"][2], res["reference"][2])                 # the same host draws were consumed


@pytest.mark.parametrize("branch", ["mixstyle", "mixup"])
def test_scene_trainer_step_matches_the_reference_expressions(branch):
    """An eager SceneCETrainer step against ex_dcase20.py:99-123 in torch ops on the same HIP model: wave_augment -> mel ->
    torch MixStyle with the same draws -> F.cross_entropy on the soft targets (mixstyle_p = 1: no mix-up draw is consumed),
    and the mix-up branch (mixstyle_p = 0) with its two F.cross_entropy terms.  Same loss, same gradients, same RNG state."""
    bank, mean, cls = _bank()
    batch = [5, 0, 11, 7]
    kw = dict(mixstyle_p=1.0, mixstyle_alpha=0.4) if branch == "mixstyle" else dict(mixstyle_p=0.0, mixup_alpha=0.3)
    res = {}
    for tag in ("kernel", "reference"):
        m = _model()
        mel = _mel()
        torch.manual_seed(21); np.random.seed(21)
        if tag == "kernel":
            tr = SceneCETrainer(m, mel, FusedAdam(m.parameters(), lr=1e-3), bank, mean, cls, **kw)
            loss = tr.loss_and_backward(batch)
        else:
            draws = dcase20.draw_augment(batch, N, 12, True, True)
            x, y = ops.wave_augment(bank, mean, cls, *draws, C)
            spec = mel(x).unsqueeze(1)
            if branch == "mixstyle":
                on, perm, lam = dcase20.draw_mixstyle(B, 1.0, 0.4)
                assert on
                y_hat, _ = m(_torch_mixstyle(spec, perm, lam))
                loss = F.cross_entropy(y_hat, y, reduction="none").mean()
            else:
                rn, lam = mixup(B, 0.3)
                spec = ops.mixup_fwd(spec, rn.to(DEV, torch.int32), lam.to(DEV))
                y_hat, _ = m(spec)
                lam = lam.to(DEV)
                loss = (F.cross_entropy(y_hat, y, reduction="none") * lam
                        + F.cross_entropy(y_hat, y[rn.to(DEV)], reduction="none") * (1. - lam)).mean()
            loss.backward()
        torch.cuda.synchronize()
        res[tag] = (float(loss.detach()), {n: p.grad.detach().cpu().double() for n, p in m.named_parameters()}, _states())
    _compare(res)


def test_unapplied_mixstyle_step_is_the_plain_step_without_mixup_draws():
    """mixstyle_p > 0 and the coin says no: plain CE on the unmixed spec, and still no mix-up draw (ex_dcase20.py:104-107)."""
    bank, mean, cls = _bank()
    batch = [1, 2, 3, 4]
    res = {}
    for tag in ("kernel", "reference"):
        m = _model()
        mel = _mel()
        torch.manual_seed(5); np.random.seed(5)
        if tag == "kernel":
            tr = SceneCETrainer(m, mel, FusedAdam(m.parameters(), lr=1e-3), bank, mean, cls, mixstyle_p=1e-9)
            assert tr.mixup_alpha == 0
            loss = tr.loss_and_backward(batch)
        else:
            x, y = ops.wave_augment(bank, mean, cls, *dcase20.draw_augment(batch, N, 12, True, True), C)
            spec = mel(x).unsqueeze(1)
            assert dcase20.draw_mixstyle(B, 1e-9, 0.4) == (False, None, None)
            y_hat, _ = m(spec)
            loss = F.cross_entropy(y_hat, y)
            loss.backward()
        torch.cuda.synchronize()
        res[tag] = (float(loss.detach()), {n: p.grad.detach().cpu().double() for n, p in m.named_parameters()}, _states())
    _compare(res)


class _CountingGraph:
    def __init__(self, g):
        self.g, self.n = g, 0

    def replay(self):
        self.n += 1
        self.g.replay()


def _run_trainer(graphed, monkeypatch, steps=6, lr=1e-3, name="mn10", seed=13, **kw):
    bank, mean, cls = _bank(seed=2)
    m = _model(name)
    mel = _mel()
    opt = FusedAdam(m.parameters(), lr=torch.tensor(lr, device=DEV), capturable=True)
    coins, captures = [], []
    real_draw, real_capture = dcase20.draw_mixstyle, train_loop.capture

    def draw(*a):
        r = real_draw(*a)
        coins.append(r[0])
        return r

    def capture(*a, **k):
        captures.append(1)
        return real_capture(*a, **k)

    monkeypatch.setattr(dcase20, "draw_mixstyle", draw)
    monkeypatch.setattr(train_loop, "capture", capture)
    tr = (GraphedSceneCETrainer(m, mel, opt, bank, mean, cls, B, **kw) if graphed
          else SceneCETrainer(m, mel, opt, bank, mean, cls, **kw))
    if graphed:
        tr.graph = _CountingGraph(tr.graph)
    torch.manual_seed(seed); np.random.seed(seed)
    losses = []
    for s in range(steps):
        batch = torch.randperm(N)[:B].tolist()
        losses.append(float(tr.step(batch)))
    torch.cuda.synchronize()
    return tr, m, losses, coins, captures


def test_graphed_scene_trainer_follows_the_eager_trainer(monkeypatch):
    """Six seeded steps with mixstyle_p = 0.5, captured vs eager, at the tolerances of
    test_gpu_finetune.py::test_graphed_ce_trainer_follows_the_eager_trainer.  The coin falls both ways; the captured trainer
    replays ONE graph through applied and unapplied steps.

    lr = 1e-4, not that test's 1e-3: its bounds ask for rounding-level agreement of two trajectories, and that can be asked
    only while the trajectories are comparable at all.  The training step is not bit-repeatable (atomic adds in the weight
    gradients), and Adam turns an ulp of difference into steps of +-lr in parameters whose gradient is noise.  Measured on one
    MI355X on this bank (batch 4, six steps, seed 13) with the EXISTING ESC-50 trainers: two EAGER runs of CETrainer differ in
    the step losses by 0, 0, 0, 5.6e-7, 1.5e-5, 1.9e-4 (relative) at lr 1e-3 - the sixth step is past the 2e-5 bound without
    any captured step involved - and CETrainer against GraphedCETrainer by at most 4.2e-7 at lr 1e-4.  At lr 1e-3 this
    test's own pair differed by 4.4e-5 ... 6.6e-4 at the sixth step from run to run; at 1e-4 by at most 5.2e-7."""
    res = {}
    for graphed in (False, True):
        tr, m, losses, coins, captures = _run_trainer(graphed, monkeypatch, lr=1e-4, mixstyle_p=0.5, mixstyle_alpha=0.4)
        assert len(coins) == 6 and True in coins and False in coins, coins
        if graphed:
            assert len(captures) == 1 and tr.graph.n == 6 and tr._perm is None
        rm = torch.cat([b.detach().float().reshape(-1) for n, b in m.named_buffers() if n.endswith("running_mean")]).cpu()
        res[graphed] = (losses, torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu(), tr.epoch_stats(), rm, list(coins))
        if graphed:                                                           # a partial batch takes the eager step
            m._drop_mask_override = m._drop_mask_override[:3]
            loss = float(tr.step([0, 1, 2]))
            torch.cuda.synchronize()
            assert np.isfinite(loss) and tr.graph.n == 6 and tr.steps == 1 and len(captures) == 1
    assert res[False][4] == res[True][4]
    le, lg = res[False][0], res[True][0]
    assert all(abs(a - b) < 2e-5 * max(1.0, abs(a)) for a, b in zip(le, lg)), (le, lg)
    d = (res[False][1] - res[True][1]).abs()
    frac = float((d > 1e-4).float().mean())
    print(f"coins {res[True][4]}; losses {le} / {lg}; params max |eager - graph| {float(d.max()):.2e}, "
          f"fraction above 1e-4 {frac:.2e}")
    assert float(d.max()) <= 6.1e-3 and frac < 0.02, (float(d.max()), frac)
    se, sg = res[False][2]["train_loss"], res[True][2]["train_loss"]
    assert abs(se - sg) < 2e-5 * max(1.0, abs(se)) and abs(se - np.mean(le)) < 1e-5 * max(1.0, abs(se))
    drm = float((res[False][3] - res[True][3]).abs().max())
    print(f"running_mean max |eager - graph| {drm:.2e} (max |rm| {float(res[False][3].abs().max()):.2e})")
    assert drm < 1e-4 * max(1.0, float(res[False][3].abs().max())), drm


def test_graphed_unapplied_step_passes_the_spec_through(monkeypatch):
    """The captured MixStyle with the flag at 0 hands the model the log-mel bit for bit; with the flag at 1 it does not."""
    tr, m, _, _, _ = _run_trainer(True, monkeypatch, steps=0, lr=0.0, mixstyle_p=0.5)
    seen = {}
    for coin in (False, True):
        monkeypatch.setattr(dcase20, "draw_mixstyle", lambda b, p, a, coin=coin: (
            (True, torch.tensor([1, 2, 3, 0]), torch.full((b,), 0.25)) if coin else (False, None, None)))
        torch.manual_seed(3); np.random.seed(3)
        tr.step([0, 1, 2, 3])
        torch.cuda.synchronize()
        seen[coin] = torch.equal(tr._ms_out, tr.spec)
    assert seen == {False: True, True: False}


def test_mixup_branch_when_mixstyle_is_off(monkeypatch):
    """mixstyle_p = 0, mixup_alpha = 0.3: the captured step keeps the mix-up rings, draws no MixStyle coin and follows the
    eager trainer."""
    out = {}
    for graphed in (False, True):
        tr, m, losses, coins, _ = _run_trainer(graphed, monkeypatch, steps=2, mixstyle_p=0.0, mixup_alpha=0.3)
        assert coins == [] and tr.mixup_alpha == 0.3
        if graphed:
            assert tr._perm is not None and not hasattr(tr, "_ms_perm")
        out[graphed] = (losses, _states())
    assert all(abs(a - b) < 2e-5 * max(1.0, abs(a)) for a, b in zip(*[out[g][0] for g in (False, True)])), out
    assert _same_states(out[False][1], out[True][1])


def test_evaluate_accuracy_by_group():
    bank, mean, cls = _bank(n=11, seed=4)
    m, mel = _model(batch=4), _mel()
    groups = torch.tensor([0, 1, 2, 0, 1, 2, 0, 0, 4, 4, 1], dtype=torch.int32)   # (group 3 has no clip)
    plain = evaluate_accuracy(m, mel, bank, cls, 4, C)
    grouped = evaluate_accuracy(m, mel, bank, cls, 4, C, keep_outputs=True, groups=(groups.to(DEV), 5))
    assert set(plain) == {"accuracy", "val_loss", "n_clips", "eval_s", "clips_per_s"}
    assert grouped["accuracy"] == plain["accuracy"] and abs(grouped["val_loss"] - plain["val_loss"]) <= 1e-9
    hit = (grouped["logits"].cpu().numpy().argmax(1) == cls.cpu().numpy())
    got = grouped["accuracy_by_group"]
    assert len(got) == 5 and np.isnan(got[3])
    for k in (0, 1, 2, 4):
        assert abs(got[k] - hit[groups.numpy() == k].mean()) <= 1e-12, (k, got)
    assert abs(plain["accuracy"] - hit.mean()) <= 1e-12
    assert m.training and mel.training
    for bad in ((groups[:-1], 5), (groups, 0), (groups, 4), (groups.float(), 5)):
        with pytest.raises(ValueError):
            evaluate_accuracy(m, mel, bank, cls, 4, C, groups=bad)


def test_dymn10_eager_and_captured_steps(monkeypatch):
    for graphed in (False, True):
        tr, m, losses, coins, _ = _run_trainer(graphed, monkeypatch, steps=1, name="dymn10", mixstyle_p=1.0)
        assert np.isfinite(losses).all() and coins == [True], (losses, coins)
        if graphed:
            m.update_params(3)
            tr.recapture()
            torch.manual_seed(1); np.random.seed(1)
            assert np.isfinite(float(tr.step([0, 1, 2, 3])))
        torch.cuda.synchronize()


def _synthetic_bank(path, n, seed, devices):
    rng = np.random.default_rng(seed)
    t = np.arange(L) / 32000.0
    scene = np.arange(n) % C
    x = np.stack([0.3 * np.sin(2 * np.pi * (150.0 + 120.0 * c) * t) + 0.05 * rng.standard_normal(L) for c in scene])
    os.makedirs(path)
    np.save(os.path.join(path, "waves.npy"), np.rint(np.clip(x, -1, 1) * 32767).astype(np.int16))
    labels = np.stack([scene, np.arange(n) % len(devices), np.arange(n) % 2], 1).astype(np.int32)
    np.save(os.path.join(path, "labels.npy"), labels)
    with open(os.path.join(path, "names.txt"), "w") as f:
        f.write("".join(f"audio/clip{i}.wav\n" for i in range(n)))
    with open(os.path.join(path, "classes.json"), "w") as f:
        json.dump(dict(scene=[f"scene{c}" for c in range(C)], device=devices, city=["lyon", "vienna"]), f)
    return labels


def _program(args, timeout=420):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, "-m", "efficientat_amd.finetune_dcase20"] + args, cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-4000:]
    return json.loads(p.stdout.strip().splitlines()[-1]), p.stderr


def test_program_on_two_synthetic_banks(tmp_path):
    devices = ["a", "b", "s1"]
    train, test = str(tmp_path / "train"), str(tmp_path / "test")
    _synthetic_bank(train, 20, 0, devices)
    labels = _synthetic_bank(test, 11, 1, devices)
    out, dump = str(tmp_path / "out"), str(tmp_path / "dump")
    banks = ["--train_bank", train, "--test_bank", test]
    line, err = _program(banks + ["--n_epochs", "2", "--batch_size", "8", "--json", "--out", out, "--eval_dump", dump,
                                  "--lr", "1e-3", "--warm_up_len", "1", "--mixstyle_p", "0.6"])
    print(err[-1500:])
    print(json.dumps(line))
    for k in ("accuracy", "val_loss", "train_loss", "clips_per_s", "eval_clips_per_s"):
        assert np.isfinite(line[k]), k
    assert line["what"] == "efficientat_amd.finetune_dcase20" and line["model"] == "mn10_as" and line["mixstyle_p"] == 0.6
    assert line["launch"] == "hipGraph replay" and line["steps"] == 2 * 3 and line["epochs"] == 2 and line["batch_size"] == 8
    logits = np.load(os.path.join(dump, "logits.npy")).astype(np.float64)
    targets = np.load(os.path.join(dump, "targets.npy")).astype(np.float64)
    assert logits.shape == (11, C) and targets.shape == (11, C)
    assert np.array_equal(np.load(os.path.join(dump, "devices.npy")), labels[:, 1])
    hit = logits.argmax(1) == targets.argmax(1)
    lse = logits.max(1) + np.log(np.exp(logits - logits.max(1, keepdims=True)).sum(1))
    ce = (targets * (lse[:, None] - logits)).sum(1)
    val_loss = float(np.mean([ce[s:s + 8].mean() for s in range(0, 11, 8)]))
    assert abs(float(hit.mean()) - line["accuracy"]) <= 1e-6 and abs(val_loss - line["val_loss"]) <= 1e-6, (val_loss, line)
    assert list(line["accuracy_by_device"]) == devices
    for k, d in enumerate(devices):
        assert np.isfinite(line["accuracy_by_device"][d])
        assert abs(float(hit[labels[:, 1] == k].mean()) - line["accuracy_by_device"][d]) <= 1e-6, (d, line)
    assert os.listdir(out) == [f"mn10_dcase_epoch_1_acc_{int(round(line['accuracy'] * 1000))}.pt"]
    assert line["checkpoint"] == os.listdir(out)[0]
    line, _ = _program(banks + ["--n_epochs", "1", "--batch_size", "8", "--json", "--no_graph", "--max_steps", "2",
                                "--mixstyle_p", "0.6"])
    assert line["launch"] == "eager" and line["steps"] == 2 and np.isfinite(line["accuracy"]) and line["checkpoint"] is None
