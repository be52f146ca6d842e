"""Weak-label SED at model level: `sed.weak_frame_loss` under autograd, the captured trainer against the eager one on a bank
that mixes strong and weak clips (one graph for a mixed, an all-weak and an all-strong batch), and the `finetune_sed` program
with `--weak_weight` on that bank, its checkpoint in `EADetector`."""
import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # collected but skipped on the CPU-only build container
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import detection, ops, sed  # noqa: E402
from efficientat_amd.mn import get_model  # noqa: E402
from efficientat_amd.optim import FusedAdam  # noqa: E402
from efficientat_amd.preprocess import AugmentMelSTFT  # noqa: E402
from tests import sed_ref as R  # noqa: E402
from tests import weak_sed_ref as W  # noqa: E402

DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, RS = 5, 10240
L = 3 * RS
WW = 0.5
# clips 1, 4, 7, 10 of the bank are weak (`weak_sed_ref.weaken_bank`)
BATCHES = [[0, 1, 2, 4], [1, 4, 7, 10], [0, 2, 3, 5]]                          # mixed, all weak, all strong
FRAMED = [[1, 0, 1, 0], [0, 0, 0, 0], [1, 1, 1, 1]]


def _quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


# ------------------------------------------------------------------------------------------------ the loss under autograd
def test_weak_frame_loss_hands_the_kernel_gradient_to_autograd():
    B, Kc, T, Tp = 3, 4, 7, 8
    g = torch.Generator().manual_seed(5)
    z = (6.0 * torch.rand(B, Kc, Tp, generator=g) - 3.0).to(DEV).requires_grad_(True)
    y = (torch.rand(B, Kc, Tp, generator=g) < 0.3).float().to(DEV)
    w = (torch.rand(B, Kc, generator=g) < 0.5).float().to(DEV)
    framed = torch.tensor([1, 0, 1], dtype=torch.int32, device=DEV)
    perm = torch.tensor([1, 2, 0], dtype=torch.int32, device=DEV)
    lam = torch.tensor([0.7, 0.6, 0.9], device=DEV)
    sums = torch.zeros(3, device=DEV, dtype=torch.float64)
    loss = sed.weak_frame_loss(z, y, w, framed, T, perm, lam, WW, sums)
    (loss * 3.0).backward()
    step = torch.zeros(3, device=DEV)
    dl, _ = ops.weak_frame_bce_fwd_bwd(z.detach(), y, w, framed, T, perm, lam, WW, sums=step)
    torch.cuda.synchronize()
    assert torch.equal(z.grad, dl * 3.0)
    ref = W.loss_closed(z.detach().cpu().numpy(), y.cpu().numpy(), w.cpu().numpy(), framed.cpu().numpy(), T, Tp, Kc,
                        perm.cpu().numpy(), lam.cpu().numpy(), WW)
    assert loss.item() == step[0].item() and loss.item() == pytest.approx(ref["loss"], rel=2e-5)
    assert sums.cpu().tolist() == step.double().cpu().tolist()
    assert sums[0].item() == pytest.approx(sums[1].item() + WW * sums[2].item(), rel=1e-6)
    assert float((z.grad.cpu().double() / 3.0 - torch.from_numpy(ref["dl"])).norm()) <= 2e-5 * float(np.linalg.norm(ref["dl"]))


# ------------------------------------------------------------------------------------------------ trainers on a synthetic bank
@pytest.fixture(scope="module")
def bank_dirs(tmp_path_factory):
    """(a bank with a third of its clips weak, the same clips all strong - the validation split)."""
    weak, strong = str(tmp_path_factory.mktemp("weak_bank")), str(tmp_path_factory.mktemp("strong_bank"))
    R.synth_bank(weak, n_clips=12, K=K, seed=0)
    R.synth_bank(strong, n_clips=12, K=K, seed=0)
    flags, events, eo = W.weaken_bank(weak)
    assert flags.tolist() == [1, 0, 1] * 4 and len(events) == eo[-1]
    return weak, strong


def _model(seed=0, B=None):
    torch.manual_seed(seed)
    m = _quiet(get_model, num_classes=K, width_mult=1.0).to(DEV).train()
    m.train_precision = "fp32"
    if B is not None:
        m._drop_mask_override = torch.full((B, m.classifier[2].out_features), 0.8, device=DEV)
    return m


def _mel():
    return _quiet(AugmentMelSTFT, freqm=0, timem=0).to(DEV).train()


def _run_trainer(bank, graphed, B=4):
    """Three seeded steps on BATCHES.  Without wave-mix a sample's frame truth is its own clip's, so the batches are what
    their names say; the log-mel mix-up still pairs framed rows with unframed ones in the mixed batch."""
    m, mel = _model(B=B), _mel()
    opt = FusedAdam(m.parameters(), lr=torch.tensor(1e-3, device=DEV), capturable=True)
    kw = dict(clip_samples=L, mixup_alpha=0.3, wavmix=False, weak_weight=WW)
    tr = (sed.GraphedWeakFrameTrainer(m, mel, opt, bank, B, **kw) if graphed else sed.WeakFrameTrainer(m, mel, opt, bank, **kw))
    torch.manual_seed(11); np.random.seed(11)
    losses, terms, framed = [], [], []
    for batch in BATCHES:
        before = tr.sums.clone()
        losses.append(float(tr.step(batch)))
        terms.append((tr.sums - before).cpu().tolist())
        if graphed:
            framed.append(tr.framed.cpu().tolist())
    torch.cuda.synchronize()
    return tr, m, losses, terms, framed


class _CountingGraph:
    def __init__(self, g):
        self.g, self.n = g, 0

    def replay(self):
        self.n += 1
        self.g.replay()


def test_graphed_weak_trainer_follows_the_eager_trainer_on_every_mixture_of_clips(bank_dirs):
    """Captured vs eager at the tolerances of test_graphed_trainer_follows_the_eager_trainer_and_a_partial_batch_runs_eagerly
    (tests/test_gpu_sed.py); the one captured graph serves a mixed, an all-weak and an all-strong batch; then a partial batch,
    which must not replay."""
    bank = sed.load_bank(bank_dirs[0], device=DEV)
    assert sed.n_weak(bank) == 4
    B = 4
    res = {}
    for graphed in (False, True):
        tr, m, losses, terms, framed = _run_trainer(bank, graphed, B=B)
        assert tr.STATS == ("train_loss", "train_frame_loss", "train_clip_loss")
        if graphed:
            assert tr.w.shape == (B, K) and tr.framed.shape == (B,) and tr.y.shape == (B, K * ops.pitch4(3))
            assert framed == FRAMED, framed                                   # the static flags, filled inside the graph
            gtr, gm = tr, m
        rm = torch.cat([b.detach().float().reshape(-1) for n, b in m.named_buffers() if n.endswith("running_mean")]).cpu()
        res[graphed] = (losses, torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu(), tr.epoch_stats(), rm, terms)
    le, lg = res[False][0], res[True][0]
    assert all(np.isfinite(le)) and all(abs(a - b) < 2e-5 * max(1.0, abs(a)) for a, b in zip(le, lg)), (le, lg)
    d = (res[False][1] - res[True][1]).abs()
    frac = float((d > 1e-4).float().mean())
    print(f"losses {le} / {lg}; terms {res[True][4]}; params max |eager - graph| {float(d.max()):.2e}, fraction above 1e-4 "
          f"{frac:.2e}")
    assert float(d.max()) <= 6.1e-3 and frac < 0.02, (float(d.max()), frac)
    for which in (False, True):
        t = res[which][4]
        assert t[1][1] == 0.0 and t[1][2] > 0.0, "the all-weak batch has no frame term"
        assert t[2][1] > 0.0 and all(s[2] > 0.0 for s in t)                   # (the mixed batch's frame term depends on
        #                                                                       which rows the mix-up pairs)
        for total, frame, clip in t:
            assert total == pytest.approx(frame + WW * clip, rel=1e-5)
    se, sg = res[False][2], res[True][2]
    for k in ("train_loss", "train_frame_loss", "train_clip_loss"):
        assert abs(se[k] - sg[k]) < 2e-5 * max(1.0, abs(se[k])), k
    assert abs(se["train_loss"] - np.mean(le)) < 1e-5 * max(1.0, abs(se["train_loss"]))
    for s in (se, sg):
        assert s["train_loss"] == pytest.approx(s["train_frame_loss"] + WW * s["train_clip_loss"], rel=1e-5)
    drm = float((res[False][3] - res[True][3]).abs().max())
    assert drm < 1e-4 * max(1.0, float(res[False][3].abs().max())), drm
    # a partial batch takes the eager path
    gtr.graph = _CountingGraph(gtr.graph)
    gm._drop_mask_override = gm._drop_mask_override[:B - 1].clone()
    before = gtr.steps
    loss = float(gtr.step([0, 4, 7]))
    torch.cuda.synchronize()
    assert gtr.graph.n == 0 and np.isfinite(loss) and gtr.steps == before + 1


def test_program_trains_on_weak_clips_and_its_checkpoint_loads_into_the_detector(bank_dirs, tmp_path):
    weak, strong = bank_dirs
    save = str(tmp_path / "out" / "weak_sed.pt")
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, "-m", "efficientat_amd.finetune_sed", "--train_bank", weak, "--valid_bank", strong, "--batch_size", "4",
           "--clip_frames", "3", "--n_epochs", "1", "--lr", "1e-3", "--warm_up_len", "1", "--max_steps", "2", "--json", "--save",
           save]
    # without --weak_weight: the argument error, before anything is built
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=420)
    assert p.returncode == 2 and "--weak_weight" in p.stderr and "strong.npy" in p.stderr, p.stderr[-2000:]
    assert not os.path.exists(save)
    p = subprocess.run(cmd + ["--weak_weight", "1"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=420)
    assert p.returncode == 0, p.stderr[-4000:]
    line = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(line))
    assert {"weak_weight", "n_weak", "train_frame_loss", "train_clip_loss", "train_loss", "val_loss", "frame_mAP"} <= set(line)
    assert (line["steps"], line["classes"], line["clip_samples"], line["launch"]) == (2, K, L, "hipGraph replay")
    assert (line["weak_weight"], line["n_weak"]) == (1.0, 4)
    assert all(np.isfinite(line[k]) for k in ("train_loss", "train_frame_loss", "train_clip_loss", "val_loss"))
    assert line["train_loss"] == pytest.approx(line["train_frame_loss"] + line["train_clip_loss"], rel=1e-5)
    state = torch.load(save, map_location="cpu", weights_only=True)
    model = _quiet(get_model, num_classes=K, width_mult=1.0)
    model.load_state_dict(state)                                              # a plain state dict in the reference's layout
    det = detection.EADetector(model=model.eval(), clip_seconds=3 * 0.32, hop_seconds=0.32,
                               labels=[f"class{c}" for c in range(K)])
    assert det.num_classes == K
    events = det.detect([0.1 * torch.randn(40000, generator=torch.Generator().manual_seed(9))], threshold=0.3, median_ms=320)
    assert len(events) == 1 and all(e[0].startswith("class") for e in events[0])
