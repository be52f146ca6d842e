"""FSD50K fine-tuning end to end (efficientat_amd/finetune.py, finetune_fsd50k.py): the trainers against the reference's loss
expression, the captured step against the eager one, the evaluation at a fixed length and at every clip's own against the
reference's `_test` expression and the CPU oracle, and the program on a synthetic ragged bank.  Model sizes, clip length and
tolerances are those of tests/test_gpu_openmic.py."""
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

from efficientat_amd import fsd50k, ops  # noqa: E402
from efficientat_amd.finetune import BCETrainer, GraphedBCETrainer, evaluate_multilabel  # noqa: E402
from efficientat_amd.optim import FusedAdam  # noqa: E402
from efficientat_amd.preprocess import AugmentMelSTFT  # noqa: E402
from efficientat_amd.train_loop import mixup  # noqa: E402
from tests import rank_metrics_ref as R  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 32000
NC = 200


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _model(seed=0, dropout_off=True, B=None):
    from efficientat_amd.mn import get_model
    torch.manual_seed(seed)
    m = _quiet(get_model, num_classes=NC, width_mult=1.0).to(DEV).train()
    m.train_precision = "fp32"
    if dropout_off and B is not None:
        m._drop_mask_override = torch.full((B, m.classifier[2].out_features), 0.8, device=DEV)
    return m


def _mel():
    return _quiet(AugmentMelSTFT, freqm=0, timem=0).to(DEV).train()


def _bank_cpu(n, seed=0, lens=None):
    """n clips of 0.3 s - 2.5 s (about half of them longer than the 1 s clip length of these tests), laid out back to back:
    noise with a per-clip offset plus tones of some of the clip's classes; every class has positives and negatives."""
    g = torch.Generator().manual_seed(seed)
    if lens is None:
        lens = torch.randint(9600, 80000, (n,), generator=g).tolist()
        lens[0], lens[1] = L, L + 1
    t = torch.arange(max(lens)) / 32000.0
    i, c = torch.meshgrid(torch.arange(n), torch.arange(NC), indexing="ij")
    y = ((i + c) % 3 == 0).float()
    clips = []
    for k in range(n):
        x = torch.randn(lens[k], generator=g) * 0.1 + 0.02 * (k % 5 - 2)
        for cc in torch.nonzero(y[k, :20]).flatten().tolist():
            x += 0.05 * torch.sin(2 * np.pi * (200.0 + 150.0 * cc) * t[:lens[k]])
        clips.append(x.float())
    return clips, y


def _bank(n, seed=0, lens=None):
    clips, y = _bank_cpu(n, seed, lens)
    lengths = torch.tensor([len(x) for x in clips], dtype=torch.int64)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), lengths.cumsum(0)[:-1]])
    return dict(waves=torch.cat(clips).to(DEV), offsets=offsets.to(DEV), lengths=lengths.to(torch.int32).to(DEV),
                clip_sum=torch.stack([x.double().sum() for x in clips]).to(DEV), bank_y=y.to(DEV), lengths_cpu=lengths,
                names=[f"clip{i}" for i in range(n)])


def test_bce_trainer_step_matches_the_reference_loss_expression():
    """A BCETrainer step (ragged gather + labels -> mel -> mix-up -> model -> eat_masked_bce_fwd_bwd -> backward) against the
    same HIP model's logits fed to the literal lines of ex_fsd50k.py:102-115: same loss, same gradient of every parameter."""
    B = 16
    bank = _bank(40)
    batch = list(range(3, 3 + B))
    res = {}
    for tag in ("kernel", "reference"):
        m = _model(B=B)
        mel = _mel()
        torch.manual_seed(21); np.random.seed(21)
        if tag == "kernel":
            tr = BCETrainer(m, mel, FusedAdam(m.parameters(), lr=1e-3), bank, clip_samples=L, mixup_alpha=0.3)
            loss = tr.loss_and_backward(batch)
        else:
            draws = fsd50k.draw_augment(batch, bank["lengths_cpu"], L, 12, True, True)
            idx, start = draws[0], draws[1]
            assert bool((idx[1::2] >= 0).any()) and bool((idx[1::2] < 0).any()) and bool((start > 0).any())
            x, yy = ops.wave_augment_ragged(bank, *draws, L)
            y = yy[:, :NC]
            x = mel(x).unsqueeze(1)
            bs = B
            rn_indices, lam = mixup(bs, 0.3)
            lam = lam.to(x.device)
            x = ops.mixup_fwd(x, rn_indices.to(DEV, torch.int32), lam)
            y_hat, _ = m(x)
            y_mix = y * lam.reshape(bs, 1) + y[rn_indices.to(DEV)] * (1. - lam.reshape(bs, 1))
            samples_loss = F.binary_cross_entropy_with_logits(y_hat, y_mix, reduction="none")
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


N_RUN = 30


def _run_trainer(graphed, steps=3, B=6, lr=1e-3, dropout_off=True):
    bank = _bank(N_RUN, seed=2)
    m = _model(B=B, dropout_off=dropout_off)
    mel = _mel()
    opt = FusedAdam(m.parameters(), lr=torch.tensor(lr, device=DEV), capturable=True)
    kw = dict(clip_samples=L, mixup_alpha=0.3)
    tr = GraphedBCETrainer(m, mel, opt, bank, B, **kw) if graphed else BCETrainer(m, mel, opt, bank, **kw)
    torch.manual_seed(11); np.random.seed(11)
    losses = []
    for s in range(steps):
        batch = torch.randperm(N_RUN)[:B].tolist()
        losses.append(float(tr.step(batch)))
    torch.cuda.synchronize()
    return tr, m, losses


@pytest.mark.parametrize("B", [6, 16])
def test_graphed_bce_trainer_follows_the_eager_trainer(B):
    """Three seeded steps, captured vs eager, at the tolerances of test_graphed_masked_bce_trainer_follows_the_eager_trainer;
    the first batch holds a long clip and a wave-mixed pair of long clips."""
    lengths = _bank(N_RUN, seed=2)["lengths_cpu"]
    torch.manual_seed(11); np.random.seed(11)
    idx, start, _, _, _ = fsd50k.draw_augment(torch.randperm(N_RUN)[:B].tolist(), lengths, L)
    long_ = torch.where(idx >= 0, lengths[idx.clamp(min=0).long()], 0) > L
    assert bool(long_.any()) and bool((long_[0::2] & long_[1::2]).any()), (idx, lengths)
    res = {}
    for graphed in (False, True):
        tr, m, losses = _run_trainer(graphed, B=B)
        if graphed:
            assert tr.y.shape == (B, 2 * NC) and tr.wave.shape == (B, L)
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


def test_graphed_bce_trainer_lr0_replay_and_partial_batch():
    """lr = 0: replays leave every parameter bit-identical (the warm-up of the capture is undone too) and each replay
    reproduces the eager trainer's gradients for the same draws; a partial batch takes the eager step and does not replay."""
    B = 6
    tr, m, _ = _run_trainer(True, steps=0, lr=0.0, B=B)
    before = [p.detach().clone() for p in m.parameters()]
    tr.graph = _CountingGraph(tr.graph)
    me = _model(B=B)
    me.load_state_dict(m.state_dict())
    eager = BCETrainer(me, _mel(), FusedAdam(me.parameters(), lr=0.0), tr.bank, clip_samples=L, mixup_alpha=0.3)
    for rep, batch in enumerate(([0, 1, 2, 3, 4, 5], [7, 1, 9, 20, 3, 11])):
        torch.manual_seed(3 + rep); np.random.seed(3 + rep)
        loss = float(tr.step(batch))
        torch.cuda.synchronize()
        assert tr.graph.n == rep + 1 and np.isfinite(loss)
        assert all(torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))
        torch.manual_seed(3 + rep); np.random.seed(3 + rep)
        le = float(eager.loss_and_backward(batch))
        assert abs(loss - le) < 2e-5 * max(1.0, abs(le)), (loss, le)
        gmax = max(float(p.grad.abs().max()) for p in me.parameters())
        for (n, pg), pe in zip(m.named_parameters(), me.parameters()):
            err = float((pg.grad - pe.grad).abs().max())
            assert err <= 1e-4 * float(pe.grad.abs().max()) + 1e-6 * gmax, (rep, n, err)
        eager.opt.zero_grad()
    m._drop_mask_override = m._drop_mask_override[:B - 2].clone()       # (the eager step's batch: the captured graph keeps its own)
    loss = float(tr.step(list(range(B - 2))))
    torch.cuda.synchronize()
    assert tr.graph.n == 2 and np.isfinite(loss) and tr.steps == 3
    assert all(torch.equal(a, p.detach()) for a, p in zip(before, m.parameters()))


def test_evaluate_multilabel_fixed_length_is_the_reference_test_expression(monkeypatch):
    """12 clips at batch 5 (the last batch is short): the crops handed to the gather are draw_eval_crops' under the caller's
    seed, val_loss equals the literal lines of `_test` (ex_fsd50k.py:162-178) on batches padded / cropped on the host, mAP /
    ROC equal the fp64 oracle on evaluate_multilabel's own logits, and the caller's RNG state is unchanged."""
    bank = _bank(12, seed=4)
    lengths = bank["lengths_cpu"]
    assert bool((lengths > L).any()) and bool((lengths < L).any())
    m, mel = _model(seed=1), _mel()
    tr = BCETrainer(m, mel, FusedAdam(m.parameters(), lr=1e-3), bank, clip_samples=L, mixup_alpha=0)
    torch.manual_seed(2); np.random.seed(2)
    for _ in range(30):                              # (BatchNorm running statistics close to the data's: test_gpu_openmic.py)
        tr.step(list(range(12)))
    seen = []
    real = ops.wave_augment_ragged
    monkeypatch.setattr(ops, "wave_augment_ragged", lambda bank, idx, start, *a, **k: (seen.append((idx.clone(), start.clone())),
                                                                                       real(bank, idx, start, *a, **k))[1])
    state = torch.random.get_rng_state()
    ev = evaluate_multilabel(m, mel, bank, 5, clip_samples=L, keep_outputs=True)
    assert m.training and mel.training and torch.equal(torch.random.get_rng_state(), state)
    with torch.random.fork_rng(devices=[]):
        crops = fsd50k.draw_eval_crops(lengths, L)
    assert bool((crops > 0).any())
    assert torch.equal(torch.cat([s[0::2] for _, s in seen]), crops) and [len(i) for i, _ in seen] == [10, 10, 4]
    assert torch.equal(torch.cat([i[0::2] for i, _ in seen]), torch.arange(12, dtype=torch.int32))
    m.eval(); mel.eval()
    waves, offs = bank["waves"].cpu(), bank["offsets"].tolist()
    rows = []
    for k in range(12):
        x = waves[offs[k] + int(crops[k]):offs[k] + int(lengths[k])][:L]
        rows.append(torch.cat([x, torch.zeros(L - len(x))]))
    xb = torch.stack(rows).to(DEV)
    losses, outputs = [], []
    for s in range(0, 12, 5):
        y = bank["bank_y"][s:s + 5]
        with torch.no_grad():
            y_hat, _ = m(mel(xb[s:s + 5]).unsqueeze(1))
        losses.append(F.binary_cross_entropy_with_logits(y_hat.double(), y.double()).cpu().numpy())
        outputs.append(y_hat.float().cpu().numpy())
    val_loss, outputs = float(np.stack(losses).mean()), np.concatenate(outputs)
    logits, targets = ev["logits"].cpu().numpy(), ev["targets"].cpu().numpy()
    print(f"val_loss {ev['val_loss']:.7f} / {val_loss:.7f}, mAP {ev['mAP']:.6f}, ROC {ev['ROC']:.6f}")
    assert abs(ev["val_loss"] - val_loss) <= 1e-6 * max(1.0, val_loss)
    np.testing.assert_allclose(logits, outputs, rtol=0, atol=1e-5)     # the same kernels on the same batches
    np.testing.assert_array_equal(targets, bank["bank_y"].cpu().numpy())
    ap, auc = R.ap_auc(logits, targets)
    assert np.isfinite(ap).all() and np.isfinite(auc).all()
    assert abs(ev["mAP"] - ap.mean()) <= 1e-9 and abs(ev["ROC"] - auc.mean()) <= 1e-9 and ev["n_clips"] == 12
    # a class with one label value only: the plain mean is NaN where the reference's roc_auc_score raises
    bank["bank_y"][:, 3] = 0.0
    ev = evaluate_multilabel(m, mel, bank, 5, clip_samples=L)
    assert np.isnan(ev["ROC"]) and np.isfinite(ev["mAP"]) and np.isfinite(ev["val_loss"])


def test_evaluate_multilabel_variable_length_matches_the_oracle():
    """Clips of 9 600, 47 777 and 400 000 samples (30, 150 and 1250 frames), each at its own length as a view of the flat
    buffer - the second and third start at odd samples: every logit row against oracle/eat_oracle.py's mel + MN on that clip
    alone within 1e-3 (the project's logits bar, __graft_entry__.smoke), val_loss = the mean of the per-clip losses."""
    from oracle import eat_oracle as O
    from oracle import synth
    lens = [9600, 47777, 400000]
    bank = _bank(3, seed=8, lens=lens)
    assert bank["offsets"].tolist() == [0, 9600, 57377]
    x_cal = O.mel_forward(synth.parity_clips(64000, seed=3)).unsqueeze(1)
    sd = synth.calibrate(synth.synth_state(synth.mn_shapes(1.0, num_classes=NC), seed=0), O.mn_forward, x_cal)
    m = _model()
    m.load_state_dict(sd)
    mel = _mel()
    state = torch.random.get_rng_state()
    ev = evaluate_multilabel(m, mel, bank, 64, clip_samples=L, variable_length=True, keep_outputs=True)
    assert m.training and mel.training and torch.equal(torch.random.get_rng_state(), state) and ev["n_clips"] == 3
    logits = ev["logits"].cpu()
    waves, y = bank["waves"].cpu(), bank["bank_y"].cpu()
    losses = []
    for k, (o, n) in enumerate(zip(bank["offsets"].tolist(), lens)):
        with torch.no_grad():
            ref, _ = O.mn_forward(sd, O.mel_forward(waves[o:o + n].unsqueeze(0)).unsqueeze(1))
        err = float((logits[k] - ref[0]).abs().max())
        print(f"{n} samples: max |logits - oracle| {err:.2e} (|logits| max {float(ref.abs().max()):.2f})")
        assert err <= 1e-3, (n, err)
        losses.append(float(F.binary_cross_entropy_with_logits(logits[k].double(), y[k].double())))
    assert abs(ev["val_loss"] - np.mean(losses)) <= 1e-6 * max(1.0, np.mean(losses))


def test_program_on_a_synthetic_bank(tmp_path):
    clips, y = _bank_cpu(12, seed=6)
    for split in ("train", "valid"):
        d = tmp_path / split
        d.mkdir()
        np.save(d / "waves.npy", np.rint(torch.cat(clips).clamp(-1, 1).numpy() * 32767.0).astype(np.int16))
        np.save(d / "lengths.npy", np.array([len(x) for x in clips], dtype=np.int64))
        np.save(d / "targets.npy", y.numpy().astype(np.uint8))
        (d / "names.txt").write_text("\n".join(f"clip{i}" for i in range(12)) + "\n")
    out = str(tmp_path / "out")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    base = [sys.executable, "-m", "efficientat_amd.finetune_fsd50k", "--batch_size", "4", "--clip_seconds", "1", "--json"]
    banks = ["--train_bank", str(tmp_path / "train"), "--valid_bank", str(tmp_path / "valid")]
    train_keys = {"what", "mode", "model", "steps", "epochs", "batch_size", "launch", "eval", "mAP", "ROC", "val_loss",
                  "train_loss", "clips_per_s", "eval_clips_per_s", "checkpoint"}
    ckpt = None
    for extra, launch, mode in ((["--out", out], "hipGraph replay", "1 s"),
                                (["--variable_eval_length", "--no_graph"], "eager", "variable length")):
        p = subprocess.run(base + ["--train"] + banks + ["--n_epochs", "2", "--max_steps", "3"] + extra, cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=420)
        assert p.returncode == 0, p.stderr[-4000:]
        line = json.loads(p.stdout.strip().splitlines()[-1])
        print(p.stderr[-600:])
        print(json.dumps(line))
        assert set(line) == train_keys
        for k in ("train_loss", "val_loss", "mAP", "ROC", "clips_per_s", "eval_clips_per_s"):
            assert np.isfinite(line[k]), k
        assert (line["launch"], line["steps"], line["epochs"], line["eval"], line["mode"]) == (launch, 3, 1, mode, "train")
        if "--out" in extra:
            ckpt = f"mn10_fsd50k_epoch_0_mAP_{int(round(line['mAP'] * 1000))}.pt"
            assert os.listdir(out) == [ckpt] and line["checkpoint"] == ckpt
    p = subprocess.run(base + ["--eval_bank", str(tmp_path / "valid"), "--init_checkpoint", os.path.join(out, ckpt)], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=420)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = p.stdout.strip().splitlines()
    line = json.loads(lines[-1])
    assert set(line) == {"what", "mode", "model", "eval", "mAP", "ROC", "val_loss", "n_clips", "eval_clips_per_s"}
    assert line["mode"] == "evaluate" and line["n_clips"] == 12 and np.isfinite(line["mAP"]) and np.isfinite(line["ROC"])
    assert "  mAP: {:.3f}".format(line["mAP"]) in lines and "  ROC: {:.3f}".format(line["ROC"]) in lines
