"""OpenMIC fine-tuning end to end (efficientat_amd/finetune.py, finetune_openmic.py): the trainers against the reference's loss
expression, the captured step against the eager one, the evaluation against the reference's `_test` expression, and the
program on a synthetic bank.  Model sizes, clip length and tolerances are those of tests/test_gpu_finetune.py."""
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

from efficientat_amd import ops  # noqa: E402
from efficientat_amd.finetune import GraphedMaskedBCETrainer, MaskedBCETrainer, evaluate_masked  # noqa: E402
from efficientat_amd.openmic import draw_augment  # noqa: E402
from efficientat_amd.optim import FusedAdam  # noqa: E402
from efficientat_amd.preprocess import AugmentMelSTFT  # noqa: E402
from efficientat_amd.train_loop import mixup  # noqa: E402
from tests.openmic_ref import masked_ap_auc  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 32000


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _model(seed=0, dropout_off=True, B=None):
    from efficientat_amd.mn import get_model
    torch.manual_seed(seed)
    m = _quiet(get_model, num_classes=20, width_mult=1.0).to(DEV).train()
    m.train_precision = "fp32"
    if dropout_off and B is not None:
        m._drop_mask_override = torch.full((B, m.classifier[2].out_features), 0.8, device=DEV)
    return m


def _mel():
    return _quiet(AugmentMelSTFT, freqm=0, timem=0).to(DEV).train()


def _bank_cpu(n, seed=0):
    """n clips of 1 s: noise plus the tones of the clip's instruments; soft labels, a sixth of them not annotated - half of
    the positives, so that a class's annotated prevalence (0.2) is not its prevalence (1/3).  Every class keeps annotated
    positives and negatives (the masked ROC of `_test` is then a number)."""
    g = torch.Generator().manual_seed(seed)
    bank = (torch.randn(n, L, generator=g) * 0.1).float()
    t = torch.arange(L) / 32000.0
    i, c = torch.meshgrid(torch.arange(n), torch.arange(20), indexing="ij")
    pos = (i + c) % 3 == 0
    lab = torch.where(pos, 0.55 + 0.45 * torch.rand(n, 20, generator=g), 0.45 * torch.rand(n, 20, generator=g))
    mask = ((i + c) % 6 != 0).float()
    for k in range(n):
        for cc in torch.nonzero(pos[k]).flatten().tolist():
            bank[k] += 0.05 * torch.sin(2 * np.pi * (200.0 + 150.0 * cc) * t)
    return bank, torch.cat([lab, mask], 1).float()


def _bank(n, seed=0):
    bank, yy = _bank_cpu(n, seed)
    return bank.to(DEV), bank.double().mean(1).to(DEV), yy.to(DEV)


def test_masked_bce_trainer_step_matches_the_reference_loss_expression():
    """A MaskedBCETrainer step (augment + label rows -> mel -> mix-up -> model -> eat_masked_bce_fwd_bwd -> backward) against
    the same HIP model's logits fed to the literal lines of ex_openmic.py:102-121: same loss, same gradient of every parameter."""
    B = 16
    bank, mean, bank_y = _bank(40)
    batch = list(range(3, 3 + B))
    res = {}
    for tag in ("kernel", "reference"):
        m = _model(B=B)
        mel = _mel()
        torch.manual_seed(21); np.random.seed(21)
        if tag == "kernel":
            tr = MaskedBCETrainer(m, mel, FusedAdam(m.parameters(), lr=1e-3), bank, mean, bank_y, mixup_alpha=0.3)
            loss = tr.loss_and_backward(batch)
        else:
            idx, shift, amp, mix = (t.to(DEV) for t in draw_augment(batch, bank.shape[0], 12, True, True))
            assert bool((idx[1::2] >= 0).any()) and bool((idx[1::2] < 0).any())       # mixed and unmixed rows in the batch
            x, _ = ops.wave_augment(bank, mean, None, idx, shift, amp, mix, 0)
            y = ops.openmic_targets(bank_y, idx, mix)
            x = mel(x).unsqueeze(1)
            bs = B
            y_mask = y[:, 20:]
            y = y[:, :20] > 0.5
            y = y.float()
            rn_indices, lam = mixup(bs, 0.3)
            lam = lam.to(x.device)
            x = ops.mixup_fwd(x, rn_indices.to(DEV, torch.int32), lam)
            y_hat, _ = m(x)
            y_mix = y * lam.reshape(bs, 1) + y[rn_indices.to(DEV)] * (1. - lam.reshape(bs, 1))
            samples_loss = F.binary_cross_entropy_with_logits(y_hat, y_mix, reduction="none")
            samples_loss = y_mask.float() * samples_loss
            loss = samples_loss.mean()
            loss.backward()
        torch.cuda.synchronize()
        res[tag] = (float(loss.detach()), {n: p.grad.detach().cpu().double() for n, p in m.named_parameters()})
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


def _run_trainer(graphed, steps=3, B=6, lr=1e-3, dropout_off=True):
    bank, mean, bank_y = _bank(30, seed=2)
    m = _model(B=B, dropout_off=dropout_off)
    mel = _mel()
    opt = FusedAdam(m.parameters(), lr=torch.tensor(lr, device=DEV), capturable=True)
    kw = dict(mixup_alpha=0.3)
    tr = (GraphedMaskedBCETrainer(m, mel, opt, bank, mean, bank_y, B, **kw) if graphed
          else MaskedBCETrainer(m, mel, opt, bank, mean, bank_y, **kw))
    torch.manual_seed(11); np.random.seed(11)
    losses = []
    for s in range(steps):
        batch = torch.randperm(30)[:B].tolist()
        losses.append(float(tr.step(batch)))
    torch.cuda.synchronize()
    return tr, m, losses


def test_graphed_masked_bce_trainer_follows_the_eager_trainer():
    """Three seeded steps, captured vs eager: the tolerances of test_graphed_ce_trainer_follows_the_eager_trainer."""
    res = {}
    for graphed in (False, True):
        tr, m, losses = _run_trainer(graphed)
        if graphed:
            assert tr.y.shape == (6, 40)
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
    drm = float((res[False][3] - res[True][3]).abs().max())
    assert drm < 1e-4 * max(1.0, float(res[False][3].abs().max())), drm


class _CountingGraph:
    def __init__(self, g):
        self.g, self.n = g, 0

    def replay(self):
        self.n += 1
        self.g.replay()


def test_graphed_masked_bce_trainer_lr0_replay_and_partial_batch():
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


def test_evaluate_masked_is_the_reference_test_expression():
    """12 clips at batch 5 (the last batch is short): val_loss against the literal lines of `_test` (ex_openmic.py:170-192) on
    logits recomputed here with the same modules, the probabilities against their sigmoid, mAP / ROC against the fp64 oracle
    (pinned to sklearn's sample_weight in tests/test_openmic_cpu.py) on evaluate_masked's own probabilities, and away from
    the unmasked metric.  Measured on one MI355X: this briefly trained model scores the 12 clips of a class with one or two
    distinct values in eval mode, so the metric here is mostly tie groups; rankings are tests/test_gpu_openmic_kernels.py's."""
    bank, mean, bank_y = _bank(12, seed=4)
    m, mel = _model(seed=1), _mel()
    # (training steps first: with the BatchNorm running statistics of its initialisation the eval-mode model scores every
    # clip alike - one tie group per class - so the statistics are brought close to the data's, 1 - 0.9^30 = 96 %)
    tr = MaskedBCETrainer(m, mel, FusedAdam(m.parameters(), lr=1e-3), bank, mean, bank_y, mixup_alpha=0)
    torch.manual_seed(2); np.random.seed(2)
    for _ in range(30):
        tr.step(list(range(12)))
    state = torch.random.get_rng_state()
    ev = evaluate_masked(m, mel, bank, bank_y, 5, keep_outputs=True)
    assert m.training and mel.training and torch.equal(torch.random.get_rng_state(), state)
    m.eval(); mel.eval()
    losses, outputs = [], []
    for s in range(0, 12, 5):
        y = bank_y[s:s + 5]
        y_mask = y[:, 20:]
        y = y[:, :20] > 0.5
        y = y.float()
        with torch.no_grad():
            y_hat, _ = m(mel(bank[s:s + 5]).unsqueeze(1))
        samples_loss = F.binary_cross_entropy_with_logits(y_hat.double(), y.double(), reduction="none")
        samples_loss = y_mask.double() * samples_loss
        losses.append(samples_loss.mean().cpu().numpy())
        outputs.append(torch.sigmoid(y_hat.double()).cpu().numpy())
    val_loss, outputs = float(np.stack(losses).mean()), np.concatenate(outputs)
    probs, targets = ev["probs"].cpu().numpy(), ev["targets"].cpu().numpy()
    print(f"val_loss {ev['val_loss']:.7f} / {val_loss:.7f}, mAP {ev['mAP']:.6f}, ROC {ev['ROC']:.6f}")
    assert abs(ev["val_loss"] - val_loss) <= 1e-6 * max(1.0, val_loss)
    assert np.abs(probs - outputs).max() <= 2.0 ** -24
    np.testing.assert_array_equal(targets, torch.cat([(bank_y[:, :20] > 0.5).float(), bank_y[:, 20:]], 1).cpu().numpy())
    print("distinct scores per class:", [int(np.unique(probs[:, c]).size) for c in range(20)])
    ap, auc = masked_ap_auc(probs, targets[:, :20], targets[:, 20:])
    assert np.isfinite(ap).all() and np.isfinite(auc).all()
    assert abs(ev["mAP"] - ap.mean()) <= 1e-9 and abs(ev["ROC"] - auc.mean()) <= 1e-9 and ev["n_clips"] == 12
    ap_all, _ = masked_ap_auc(probs, targets[:, :20], np.ones_like(probs))
    assert abs(ev["mAP"] - ap_all.mean()) > 0.05                                   # the mask reached the metric
    # a class without annotated positives: the plain mean is NaN, as the reference's
    bank_y[:, 3] = 0.0
    ev = evaluate_masked(m, mel, bank, bank_y, 5)
    assert np.isnan(ev["ROC"]) and np.isfinite(ev["mAP"]) and np.isfinite(ev["val_loss"])
    # what sklearn refuses (here: a mask entry of 0.5) is the reference's `except ValueError`: NaN
    bank_y[0, 25] = 0.5
    ev = evaluate_masked(m, mel, bank, bank_y, 5)
    assert np.isnan(ev["mAP"]) and np.isnan(ev["ROC"]) and np.isfinite(ev["val_loss"])


def test_program_on_a_synthetic_bank(tmp_path):
    bank, yy = _bank_cpu(12, seed=6)
    for split in ("train", "test"):
        d = tmp_path / split
        d.mkdir()
        np.save(d / "waves.npy", np.rint(bank.clamp(-1, 1).numpy() * 32767.0).astype(np.int16))
        np.save(d / "targets.npy", yy.numpy())
        (d / "names.txt").write_text("\n".join(f"clip{i}" for i in range(12)) + "\n")
    out = str(tmp_path / "out")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, "-m", "efficientat_amd.finetune_openmic", "--train_bank", str(tmp_path / "train"),
                        "--test_bank", str(tmp_path / "test"), "--batch_size", "4", "--n_epochs", "2", "--max_steps", "3",
                        "--json", "--out", out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=420)
    assert p.returncode == 0, p.stderr[-4000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    print(p.stderr[-800:])
    print(json.dumps(line))
    for k in ("train_loss", "val_loss", "mAP", "clips_per_s"):
        assert np.isfinite(line[k]), k
    assert line["launch"] == "hipGraph replay" and line["steps"] == 3 and line["epochs"] == 1
    assert os.listdir(out) == [f"mn10_openmic_epoch_0_mAP_{int(round(line['mAP'] * 1000))}.pt"]
