"""Strong-label SED at model level: one training step through `forward_train_frames` and the fused frame BCE against
torch-CPU autograd over the oracle; the captured trainer against the eager one, `evaluate_frames` against a numpy
restatement and the `finetune_sed` program on a synthetic bank, and its checkpoint in `EADetector`."""
import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import eat_oracle as O
from oracle import synth

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import detection, ops, sed  # noqa: E402
from efficientat_amd.mn import get_model  # noqa: E402
from efficientat_amd.mn_train import FrameHead, forward_train_frames  # noqa: E402
from efficientat_amd.optim import FusedAdam  # noqa: E402
from efficientat_amd.preprocess import AugmentMelSTFT  # noqa: E402
from tests import sed_ref as R  # noqa: E402
from tests.openmic_ref import masked_ap_auc  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = ("classifier.2.weight", "classifier.2.bias", "classifier.5.weight", "classifier.5.bias")
ATOL = 1e-9                                                               # the bound of tests/test_gpu_openmic_kernels.py
K, RS = 5, 10240
L = 3 * RS


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def _rel(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm())


# ------------------------------------------------------------------------------------------------ one training step
def test_one_training_step_matches_autograd_over_the_oracle():
    """Synthetic mn10 (calibrated), 5 clips of 3 s: frame logits (5, 527, 10); targets of density 0.02; Dropout replaced by
    its expectation on both sides.  Loss 1e-4 relative, frame logits 1e-3 of scale; parameter gradients at the
    whole-network bars (rel-L2 max 5e-2, median 1.5e-2; tensors whose norm is below 1e-4 of the largest are skipped - at
    most 16 of them, the fp32 oracle alone skips 15 of the 174, and never a head tensor); the four head tensors at 1e-3, or
    4x the oracle's own fp32-vs-fp64 figure where that exceeds 2.5e-4 (printed)."""
    wave = synth.parity_clips(96000, seed=3)
    x = O.mel_forward(wave).unsqueeze(1)
    sd = synth.calibrate(synth.synth_state(synth.mn_shapes(1.0), seed=0), O.mn_forward, x)
    B, T = x.shape[0], 10
    y = (torch.rand(B, 527, T, generator=torch.Generator().manual_seed(8)) < 0.02).float()
    keep = torch.full((B, 1280), 0.8) / 0.8                                   # the expectation of the dropout factor
    loss_ref, z_ref, gref = R.oracle_frame_step(O, sd, x, y, keep, torch.float32)
    _, _, gref64 = R.oracle_frame_step(O, sd, x, y, keep, torch.float64)
    assert z_ref.shape == (B, 527, T)

    model = _quiet(get_model, width_mult=1.0)
    model.load_state_dict(sd)
    model.to(DEV).train()
    model.train_precision = "fp32"
    model._drop_mask_override = torch.full((B, 1280), 0.8, device=DEV)
    z = forward_train_frames(model, x.to(DEV))
    Tp = ops.pitch4(T)
    assert z.shape == (B, 527, Tp)
    yp = torch.zeros(B, 527, Tp)
    yp[:, :, :T] = y
    loss = sed.frame_bce_loss(z, yp.to(DEV), T)
    loss.backward()
    torch.cuda.synchronize()
    print(f"sed step: loss {loss.item():.6f} (oracle {loss_ref.item():.6f})")
    assert abs(loss.item() - loss_ref.item()) < 1e-4 * max(1.0, abs(loss_ref.item()))
    assert float((z.detach().cpu()[:, :, :T] - z_ref).abs().max()) < 1e-3 * max(1.0, float(z_ref.abs().max()))
    gmax = max(float(v.norm()) for v in gref.values())
    rels, skipped = [], []
    for name, p in model.named_parameters():
        assert p.grad is not None, name
        if float(gref[name].norm()) < 1e-4 * gmax:
            skipped.append(name)
            continue
        rels.append(_rel(p.grad, gref[name].reshape(p.grad.shape)))
    print(f"sed step: gradient rel-L2 max {max(rels):.2e}, median {float(np.median(rels)):.2e} over {len(rels)} tensors, "
          f"{len(skipped)} skipped")
    assert len(skipped) <= 16 and not set(skipped) & set(HEAD), skipped
    assert max(rels) < 5e-2 and float(np.median(rels)) < 1.5e-2, (max(rels), float(np.median(rels)))
    params = dict(model.named_parameters())
    for name in HEAD:
        own = _rel(gref[name], gref64[name])
        bar = 1e-3 if own <= 2.5e-4 else 4.0 * own
        r = _rel(params[name].grad, gref[name].reshape(params[name].grad.shape))
        print(f"sed step: {name} rel-L2 {r:.2e} (bar {bar:.2e}; the oracle's fp32 vs fp64: {own:.2e})")
        assert r <= bar, (name, r, bar)


# ------------------------------------------------------------------------------------------------ trainers on a synthetic bank
@pytest.fixture(scope="module")
def bank_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("sed_bank"))
    lengths, events, eo = R.synth_bank(d, n_clips=12, K=K, seed=0)
    return d, lengths, events, eo


def _model(seed=0, B=None):
    torch.manual_seed(seed)
    m = _quiet(get_model, num_classes=K, width_mult=1.0).to(DEV).train()
    m.train_precision = "fp32"
    if B is not None:
        m._drop_mask_override = torch.full((B, m.classifier[2].out_features), 0.8, device=DEV)
    return m


def _mel():
    return _quiet(AugmentMelSTFT, freqm=0, timem=0).to(DEV).train()


def _run_trainer(bank, graphed, steps=3, B=4):
    m, mel = _model(B=B), _mel()
    opt = FusedAdam(m.parameters(), lr=torch.tensor(1e-3, device=DEV), capturable=True)
    kw = dict(clip_samples=L, mixup_alpha=0.3)
    tr = sed.GraphedFrameBCETrainer(m, mel, opt, bank, B, **kw) if graphed else sed.FrameBCETrainer(m, mel, opt, bank, **kw)
    torch.manual_seed(11); np.random.seed(11)
    losses = []
    for _ in range(steps):
        losses.append(float(tr.step(torch.randperm(12)[:B].tolist())))
    torch.cuda.synchronize()
    return tr, m, losses


class _CountingGraph:
    def __init__(self, g):
        self.g, self.n = g, 0

    def replay(self):
        self.n += 1
        self.g.replay()


def test_graphed_trainer_follows_the_eager_trainer_and_a_partial_batch_runs_eagerly(bank_dir):
    """Three seeded steps, captured vs eager, at the tolerances of test_graphed_bce_trainer_follows_the_eager_trainer
    (tests/test_gpu_fsd50k.py); then a partial batch, which must not replay."""
    bank = sed.load_bank(bank_dir[0], device=DEV)
    B = 4
    res = {}
    for graphed in (False, True):
        tr, m, losses = _run_trainer(bank, graphed, B=B)
        if graphed:
            assert tr.y.shape == (B, K * ops.pitch4(3)) and tr.wave.shape == (B, L) and (tr.R, tr.T) == (RS, 3)
            gtr, gm = tr, m
        rm = torch.cat([b.detach().float().reshape(-1) for n, b in m.named_buffers() if n.endswith("running_mean")]).cpu()
        res[graphed] = (losses, torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu(), tr.epoch_stats(), rm)
    le, lg = res[False][0], res[True][0]
    assert all(np.isfinite(le)) and all(abs(a - b) < 2e-5 * max(1.0, abs(a)) for a, b in zip(le, lg)), (le, lg)
    d = (res[False][1] - res[True][1]).abs()
    frac = float((d > 1e-4).float().mean())
    print(f"losses {le} / {lg}; params max |eager - graph| {float(d.max()):.2e}, fraction above 1e-4 {frac:.2e}")
    assert float(d.max()) <= 6.1e-3 and frac < 0.02, (float(d.max()), frac)
    se, sg = res[False][2]["train_loss"], res[True][2]["train_loss"]
    assert abs(se - sg) < 2e-5 * max(1.0, abs(se)) and abs(se - np.mean(le)) < 1e-5 * max(1.0, abs(se))
    drm = float((res[False][3] - res[True][3]).abs().max())
    assert drm < 1e-4 * max(1.0, float(res[False][3].abs().max())), drm
    # a partial batch takes the eager path
    gtr.graph = _CountingGraph(gtr.graph)
    gm._drop_mask_override = gm._drop_mask_override[:B - 1].clone()
    before = gtr.steps
    loss = float(gtr.step([0, 5, 7]))
    torch.cuda.synchronize()
    assert gtr.graph.n == 0 and np.isfinite(loss) and gtr.steps == before + 1


def test_evaluate_frames_equals_a_numpy_restatement(bank_dir):
    d, lengths, events, eo = bank_dir
    bank = sed.load_bank(d, device=DEV)
    m, mel = _model(seed=4), _mel()
    with torch.no_grad():
        m.classifier[5].bias.add_(torch.linspace(-0.5, 0.5, K, device=DEV))
        m.classifier[5].weight.mul_(30.0)                                 # (logits that spread around the threshold)
    thr = np.asarray([0.5, 0.45, 0.55, 0.5, 0.4], dtype=np.float32)
    ev = sed.evaluate_frames(m, mel, bank, batch_windows=5, threshold=thr, clip_samples=L, keep_outputs=True)
    assert m.training and mel.training                                        # the modes are restored
    T = 3
    truth, nf = R.targets_windows(events, eo, lengths, K, L, RS, T)
    W = truth.shape[0]
    assert W == int(sum(-(-int(n) // L) for n in lengths)) and W > 12       # some clips take several windows
    rows = ev["rows"].cpu().numpy().reshape(W, T, K)
    live = (np.arange(T).reshape(1, T) < nf.reshape(W, 1))
    assert ev["n_clips"] == 12 and ev["n_frames"] == int(nf.sum()) and int(nf.sum()) < W * T
    assert np.array_equal(ev["truth"].cpu().numpy().reshape(W, T, K) > 0.5, truth)
    assert np.array_equal(ev["weight"].cpu().numpy().reshape(W, T, K)[:, :, 0] > 0.5, live)
    s = R.sigmoid32(rows)
    assert np.abs(s - thr.reshape(1, 1, K)).min() >= 1e-6, "a sigmoid value lies at its threshold"
    pred = s >= thr.reshape(1, 1, K)
    lv = live[:, :, None]
    counts = np.stack([(lv & pred & truth).sum((0, 1)), (lv & pred & ~truth).sum((0, 1)), (lv & ~pred & truth).sum((0, 1))], 1)
    assert np.array_equal(ev["counts"], counts) and counts.sum() > 0
    ref = R.segment_scores(counts)
    for k, v in ref.items():
        assert ev[k] == pytest.approx(v, abs=1e-12, nan_ok=True), k
    wt = np.broadcast_to(lv, rows.shape).reshape(W * T, K).astype(np.float64)
    ap, auc = masked_ap_auc(rows.reshape(W * T, K), truth.reshape(W * T, K).astype(np.float64), wt)
    print(f"evaluate_frames: mAP {ev['frame_mAP']:.6f} / {ap.mean():.6f}, ROC {ev['frame_ROC']:.6f} / {auc.mean():.6f}, "
          f"counts {counts.tolist()}")
    assert abs(ev["frame_mAP"] - ap.mean()) <= ATOL
    assert (np.isnan(auc.mean()) and np.isnan(ev["frame_ROC"])) or abs(ev["frame_ROC"] - auc.mean()) <= ATOL
    z64 = rows.astype(np.float64)
    el = np.maximum(z64, 0) - z64 * truth + np.log1p(np.exp(-np.abs(z64)))
    assert ev["val_loss"] == pytest.approx(float((el * lv).sum() / (K * nf.sum())), rel=2e-5)


def test_program_runs_an_epoch_and_its_checkpoint_loads_into_the_detector(bank_dir, tmp_path):
    d = bank_dir[0]
    save = str(tmp_path / "out" / "sed.pt")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, "-m", "efficientat_amd.finetune_sed", "--train_bank", d, "--valid_bank", d,
                        "--batch_size", "4", "--clip_frames", "3", "--n_epochs", "1", "--lr", "1e-3", "--warm_up_len", "1",
                        "--threshold", "0.4", "--json", "--save", save], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=420)
    assert p.returncode == 0, p.stderr[-4000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    print(p.stderr[-400:])
    print(json.dumps(line))
    from efficientat_amd.finetune_sed import METRICS
    assert set(METRICS) <= set(line) and {"train_loss", "steps", "n_frames", "checkpoint", "launch", "clip_samples"} <= set(line)
    assert (line["steps"], line["epochs"], line["classes"], line["clip_samples"], line["launch"]) == (3, 1, K, L,
                                                                                                      "hipGraph replay")
    assert all(np.isfinite(line[k]) for k in ("train_loss", "val_loss", "frame_mAP"))
    state = torch.load(save, map_location="cpu", weights_only=True)
    model = _quiet(get_model, num_classes=K, width_mult=1.0)
    model.load_state_dict(state)                                              # a plain state dict in the reference's layout
    det = detection.EADetector(model=model.eval(), clip_seconds=3 * 0.32, hop_seconds=0.32,
                               labels=[f"class{c}" for c in range(K)])
    assert det.num_classes == K
    g = torch.Generator().manual_seed(9)
    events = det.detect([0.1 * torch.randn(40000, generator=g)], threshold=0.3, median_ms=320)
    assert len(events) == 1 and all(e[0].startswith("class") for e in events[0])
    # the eval frame head and the training frame head agree on a fixed last map (no dropout: eval-equivalent conditions),
    # at the 1e-3 of scale that test_eval_matches_oracle_and_golden holds the attention head to
    model = det.model
    ymap = torch.randn(3, 960, 4, 7, generator=g).to(DEV)
    with torch.no_grad():
        p_eval = detection.frame_logits(model, ymap)
        cls = model.classifier
        with ops.precision(model.train_precision):
            p_train = FrameHead.apply(ymap, cls[2].weight, cls[2].bias, cls[5].weight, cls[5].bias, None)
    torch.cuda.synchronize()
    assert p_eval.shape == p_train.shape == (3, K, 8)
    err = float((p_eval[:, :, :7] - p_train[:, :, :7]).abs().max())
    scale = max(1.0, float(p_train[:, :, :7].abs().max()))
    print(f"frame head eval vs train: max abs {err:.2e} (scale {scale:.2f})")
    assert err < 1e-3 * scale
