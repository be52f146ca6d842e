"""f1: the device-side training-loop glue (efficientat_amd/train_loop.py, csrc/train_glue.hip) against the torch-op
formulation the reference's loop uses (ex_audioset.py:142-189), written out here on CPU tensors as the oracle."""
import contextlib
import io

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

from efficientat_amd import ops  # noqa: E402
from efficientat_amd.mn import get_model  # noqa: E402
from efficientat_amd.preprocess import AugmentMelSTFT  # noqa: E402
from efficientat_amd.train_loop import KDTrainer, kd_loss  # noqa: E402

DEV = torch.device("cuda:0")


def _reference_loss(y_hat, y, rn, lam, teacher_probs, indices, kd_lambda):
    """ex_audioset.py:142-189 verbatim in meaning, on CPU tensors."""
    bs = y_hat.shape[0]
    distillation_loss = nn.BCEWithLogitsLoss(reduction="none")
    if rn is not None:
        y_mix = y * lam.reshape(bs, 1) + y[rn] * (1. - lam.reshape(bs, 1))
    else:
        y_mix = y
    label_loss = F.binary_cross_entropy_with_logits(y_hat, y_mix, reduction="none").mean()
    if kd_lambda > 0 and teacher_probs is not None:
        unknown = indices == -1
        soft = teacher_probs[indices]
        if rn is not None:
            st = distillation_loss(y_hat, soft).mean(dim=1) * lam.reshape(bs) + \
                distillation_loss(y_hat, soft[rn]).mean(dim=1) * (1. - lam.reshape(bs))
        else:
            st = distillation_loss(y_hat, soft)
            st = st.mean(dim=1)
        st = torch.where(unknown, torch.zeros_like(st), st).mean()
        label_loss = kd_lambda * label_loss
        st = (1 - kd_lambda) * st
    else:
        st = torch.tensor(0.)
    return label_loss + st, label_loss, st


@pytest.mark.parametrize("mix,kd", [(True, True), (True, False), (False, True), (False, False)])
def test_fused_kd_loss_and_gradient(mix, kd):
    g = torch.Generator().manual_seed(3)
    B, C, N = 9, 527, 40
    z = (torch.randn(B, C, generator=g) * 3).requires_grad_(True)
    y = (torch.rand(B, C, generator=g) < 0.01).float()
    rn = torch.randperm(B, generator=g) if mix else None
    lam = (torch.rand(B, generator=g) * 0.5 + 0.5) if mix else None
    teacher = torch.sigmoid(torch.randn(N, C, generator=g) * 2 - 5)
    idx = torch.randint(0, N, (B,), generator=g)
    idx[2] = -1
    idx[7] = -1
    kd_lambda = 0.1 if kd else 1.0
    loss, lab, st = _reference_loss(z, y, rn, lam, teacher if kd else None, idx, 0.1 if kd else 0.0)
    loss.backward()
    zd = z.detach().to(DEV).requires_grad_(True)
    sums = torch.zeros(3, device=DEV)
    got = kd_loss(zd, y.to(DEV), None if rn is None else rn.to(DEV, torch.int32), None if lam is None else lam.to(DEV),
                  teacher.to(DEV) if kd else None, idx.to(DEV) if kd else None, kd_lambda, sums)
    got.backward()
    assert abs(got.item() - loss.item()) < 2e-6 * max(1.0, abs(loss.item()))
    s = sums.cpu()
    assert abs(s[1].item() - lab.detach().item()) < 2e-6 and abs(s[2].item() - float(st.detach())) < 2e-6
    assert float((zd.grad.cpu() - z.grad).abs().max()) < 1e-8 + 1e-5 * float(z.grad.abs().max())


@pytest.mark.parametrize("shape", [(5, 1, 128, 1000), (3, 1, 7, 9)])
def test_mixup_kernel(shape):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(*shape, generator=g)
    rn, lam = torch.randperm(shape[0], generator=g), torch.rand(shape[0], generator=g)
    ref = x * lam.reshape(-1, 1, 1, 1) + x[rn] * (1. - lam.reshape(-1, 1, 1, 1))
    got = ops.mixup_fwd(x.to(DEV), rn.to(DEV, torch.int32), lam.to(DEV))
    assert float((got.cpu() - ref).abs().max()) < 1e-6


def test_kd_trainer_step_equals_the_reference_loop_formulation():
    """One KDTrainer.step (device glue) vs the same step spelled as the reference loop does (torch ops, same host RNG
    seeds -> same mix-up pairs): identical loss and parameter updates."""
    from efficientat_amd.train_loop import mixup
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        mel = AugmentMelSTFT(freqm=0, timem=0).to(DEV)
        m1, m2 = get_model(width_mult=0.4), get_model(width_mult=0.4)
    with torch.no_grad():
        for mod in m1.modules():
            if isinstance(mod, nn.Conv2d):
                fan_in = mod.weight.shape[1] * mod.weight.shape[2] * mod.weight.shape[3]
                mod.weight.normal_(0, (2.0 / fan_in) ** 0.5)
            elif isinstance(mod, nn.Linear):
                mod.weight.normal_(0, mod.weight.shape[1] ** -0.5)
    m2.load_state_dict(m1.state_dict())
    m1.to(DEV).train()
    m2.to(DEV).train()
    mel.train()
    B, N = 6, 20
    g = torch.Generator().manual_seed(5)
    wave = (0.1 * torch.randn(B, 1, 64000, generator=g)).to(DEV)
    y = (torch.rand(B, 527, generator=g) < 0.01).float().to(DEV)
    names = [f"f{i}" for i in range(B)]
    f2i = {f"f{i}": i for i in range(B) if i != 3}
    tlogits = torch.randn(N, 527, generator=g) * 2 - 5
    keep = torch.ones(B, m1.classifier[2].out_features, device=DEV)
    m1._drop_mask_override = m2._drop_mask_override = keep
    p0 = [p.detach().clone() for p in m1.parameters()]
    o1 = torch.optim.SGD(m1.parameters(), lr=1e-3)
    o2 = torch.optim.SGD(m2.parameters(), lr=1e-3)
    tr = KDTrainer(m1, mel, o1, teacher_preds=tlogits, fname_to_index=f2i, kd_lambda=0.1, mixup_alpha=0.3)
    torch.manual_seed(11); np.random.seed(11)
    l1 = tr.step(wave, names, y)
    # the reference formulation (ex_audioset.py:139-199) on the same modules
    torch.manual_seed(11); np.random.seed(11)
    teacher = torch.sigmoid(tlogits / 1.0)
    x = mel(wave.reshape(B, -1)).unsqueeze(1)
    rn, lam = mixup(B, 0.3)
    lam = lam.to(DEV)
    x = x * lam.reshape(B, 1, 1, 1) + x[rn] * (1. - lam.reshape(B, 1, 1, 1))
    y_hat, _ = m2(x)
    y_mix = y * lam.reshape(B, 1) + y[rn] * (1. - lam.reshape(B, 1))
    label_loss = F.binary_cross_entropy_with_logits(y_hat, y_mix, reduction="none").mean()
    indices = torch.tensor([f2i.get(f, -1) for f in names], dtype=torch.int64)
    soft = teacher[indices].to(DEV)
    bce = nn.BCEWithLogitsLoss(reduction="none")
    st = bce(y_hat, soft).mean(dim=1) * lam.reshape(B) + bce(y_hat, soft[rn]).mean(dim=1) * (1. - lam.reshape(B))
    st[indices == -1] = st[indices == -1] * 0
    loss = 0.1 * label_loss + 0.9 * st.mean()
    loss.backward()
    o2.step()
    assert abs(l1.item() - loss.item()) < 1e-5 * max(1.0, abs(loss.item()))
    # the parameter UPDATES (= -lr * gradient) agree like gradients do (activation-kink budget of test_gpu_train.py)
    d1 = [(p.detach() - q).double() for p, q in zip(m1.parameters(), p0)]
    d2 = [(p.detach() - q).double() for p, q in zip(m2.parameters(), p0)]
    dmax = max(float(d.norm()) for d in d2)
    rels = [float((a - b).norm() / b.norm()) for a, b in zip(d1, d2) if float(b.norm()) > 1e-5 * dmax]
    assert len(rels) > 50 and max(rels) < 5e-2 and float(np.median(rels)) < 1e-2, (max(rels), float(np.median(rels)))
    stats = tr.epoch_stats()
    assert abs(stats["train_loss"] - loss.item()) < 1e-5 and tr.steps == 0


# ------------------------------------------------------------------------------------------------ f2: input staging
def test_device_prefetcher_delivers_the_loader_batches_in_order():
    """DevicePrefetcher (efficientat_amd/input_pipeline.py): pinned, double-buffered H2D on a copy stream must hand out
    exactly the DataLoader's batches (datasets/audioset.py:138-161 tuple layout, file names passed through), in order,
    while the consumer keeps the compute stream busy; slots are recycled only after the consumer moved on."""
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dropin", "datasets", "audioset.py")
    os.environ["EAT_SYNTH_AUDIOSET"] = "1"                                          # explicit opt-in to the synthetic stand-in
    spec = importlib.util.spec_from_file_location("eat_dropin_audioset", path)    # (not `import datasets`: the
    audioset = importlib.util.module_from_spec(spec)                                 #  HuggingFace package has that name)
    spec.loader.exec_module(audioset)
    from torch.utils.data import DataLoader, Subset
    from efficientat_amd.input_pipeline import DevicePrefetcher

    ds = Subset(audioset.get_training_set(add_index=True), list(range(22)))       # 22 clips: a ragged last batch
    loader = DataLoader(ds, batch_size=4, shuffle=False, num_workers=0)
    want = [(w.clone(), list(n), y.clone(), i.clone()) for w, n, y, i in loader]
    assert want[0][0].shape == (4, 1, 320000) and want[-1][0].shape[0] == 2
    got = []
    burn = torch.randn(2048, 2048, device=DEV)
    for depth in (1, 2, 3):
        got.clear()
        for w, n, y, i in DevicePrefetcher(loader, DEV, depth=depth):
            assert w.is_cuda and y.is_cuda and i.is_cuda and isinstance(n[0], str)
            for _ in range(4):
                burn = torch.tanh(burn @ burn * 1e-3)                                # compute-stream work between batches
            got.append((w.float().sum(dim=(1, 2)), list(n), y.clone(), i.clone(), w[:, 0, 12345].clone()))
        assert len(got) == len(want)
        for (ws, n, y, i, probe), (w0, n0, y0, i0) in zip(got, want):
            assert n == n0
            assert torch.equal(y.cpu(), y0) and torch.equal(i.cpu(), i0)
            assert torch.equal(probe.cpu(), w0[:, 0, 12345])
            assert torch.allclose(ws.cpu(), w0.sum(dim=(1, 2)), rtol=1e-4, atol=1e-3)


# ------------------------------------------------------------------------------------------------ configs[4]: the captured KD step
def _kd_setup(seed=3, width=0.5):
    torch.manual_seed(seed)                      # (before the constructor: the Linear layers keep their default init)
    with contextlib.redirect_stdout(io.StringIO()):
        m = get_model(width_mult=width)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.Conv2d):
                fan_in = mod.weight.shape[1] * mod.weight.shape[2] * mod.weight.shape[3]
                mod.weight.normal_(0, (2.0 / fan_in) ** 0.5)
            if isinstance(mod, nn.Dropout):
                mod.p = 0.0
    return m.to(DEV).train()


def _kd_batch(step, B, L):
    g = torch.Generator().manual_seed(50 + step)
    x = (0.1 * torch.randn(B, 1, L, generator=g)).clamp_(-1, 1).to(DEV)
    y = (torch.rand(B, 527, generator=g) < 0.01).float().to(DEV)
    return x, ["syn%07d" % (3 * step + i) for i in range(B)], y


@pytest.mark.parametrize("masks", [False, True])
def test_graphed_kd_trainer_follows_the_eager_trainer(masks):
    """GraphedKDTrainer (mel + mixup + forward + KD loss + backward + Adam as ONE hipGraph replay; the batch, the mixup draw,
    the teacher rows and the mel basis enter through static buffers) against the eager KDTrainer on the same seeds, three
    steps with three different batches: same losses, same parameters up to what round-off in a gradient does to an Adam step.
    masks=True: SpecAugment masks are scalar launch arguments, so the mel runs eagerly in front of the graph."""
    from efficientat_amd.train_loop import GraphedKDTrainer
    B, L = 6, 32000
    g = torch.Generator().manual_seed(5)
    tlogits = torch.randn(40, 527, generator=g) * 2 - 5
    f2i = {"syn%07d" % i: i % 40 for i in range(0, 30, 2)}
    res = {}
    for tag in ("eager", "graph"):
        m = _kd_setup()
        with contextlib.redirect_stdout(io.StringIO()):
            mel = AugmentMelSTFT(freqm=16 if masks else 0, timem=20 if masks else 0).to(DEV).train()
        opt = torch.optim.Adam(m.parameters(), lr=1e-3, capturable=True, fused=True)
        kw = dict(teacher_preds=tlogits, fname_to_index=f2i, kd_lambda=0.1, mixup_alpha=0.3)
        tr = KDTrainer(m, mel, opt, **kw) if tag == "eager" else GraphedKDTrainer(m, mel, opt, B, L, **kw)
        if tag == "graph":
            assert tr.mel_in_graph == (not masks)
        torch.manual_seed(11); np.random.seed(11)
        losses = [float(tr.step(*_kd_batch(s, B, L))) for s in range(3)]
        torch.cuda.synchronize()
        rm = torch.cat([b.detach().float().reshape(-1) for n, b in m.named_buffers() if n.endswith("running_mean")]).cpu()
        res[tag] = (losses, torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu(), tr.epoch_stats(), rm)
    le, lg = res["eager"][0], res["graph"][0]
    assert all(abs(a - b) < 2e-5 * max(1.0, abs(a)) for a, b in zip(le, lg)), (le, lg)
    d = (res["eager"][1] - res["graph"][1]).abs()
    frac = float((d > 1e-4).float().mean())
    print(f"masks={masks}: losses {le} / {lg}; params max |eager - graph| {float(d.max()):.2e}, fraction above 1e-4 {frac:.2e}, "
          f"bit-identical: {bool((d == 0).all())}")
    # Adam moves a weight by <= lr per step whatever the gradient's size: an element whose gradient is round-off can differ
    # by 2 lr per step between two runs - bounded here; the bulk must agree
    assert float(d.max()) <= 6.1e-3 and frac < 0.02, (float(d.max()), frac)
    se, sg = res["eager"][2], res["graph"][2]
    assert all(abs(se[k] - sg[k]) < 2e-5 * max(1.0, abs(se[k])) for k in se), (se, sg)
    # the capture's warm-up steps must not leak into the BatchNorm running statistics (restored after the capture)
    assert float((res["eager"][3] - res["graph"][3]).abs().max()) < 1e-4 * max(1.0, float(res["eager"][3].abs().max()))


def test_int16_waveform_transport():
    """f2: 16-bit PCM over PCIe (`Int16Waveform` / `to_int16` on the host, `eat_wave_i16_to_f32` on the device) - exact
    against the host formula, and a training step fed int16 equals the step fed the dequantised floats."""
    from efficientat_amd.input_pipeline import I16_SCALE, to_int16
    from efficientat_amd.train_loop import GraphedKDTrainer
    g = torch.Generator().manual_seed(2)
    for n in (320000 * 3, 1003, 8, 5):
        w = (0.4 * torch.randn(n, generator=g)).clamp_(-1.2, 1.2)
        q = to_int16(w)
        assert q.dtype == torch.int16 and int(q.abs().max()) <= 32767
        got = ops.wave_i16_to_f32(q.to(DEV), scale=1.0 / I16_SCALE).cpu()
        assert torch.equal(got, q.float() * (1.0 / I16_SCALE))
        assert float((got - w.clamp(-1, 1)).abs().max()) <= 0.5 / I16_SCALE + 1e-7
    assert np.array_equal(to_int16(w.numpy()), q.numpy())
    B, L = 4, 32000
    outs = []
    for as_int in (True, False):
        m = _kd_setup(seed=4)
        with contextlib.redirect_stdout(io.StringIO()):
            mel = AugmentMelSTFT(freqm=0, timem=0).to(DEV).train()
        tr = GraphedKDTrainer(m, mel, torch.optim.Adam(m.parameters(), lr=1e-3, capturable=True, fused=True), B, L, mixup_alpha=0.3)
        x, names, y = _kd_batch(0, B, L)
        q = to_int16(x.cpu()).to(DEV)
        torch.manual_seed(1); np.random.seed(1)
        loss = tr.step(q if as_int else q.float() * (1.0 / I16_SCALE), names, y)
        outs.append(float(loss))
    assert abs(outs[0] - outs[1]) < 1e-6 * max(1.0, abs(outs[1])), outs


def _run_case(args, ok, skip=None, timeout=900):
    import os
    import subprocess
    import sys
    case = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kd_dp_case.py")
    for attempt in range(3):
        r = subprocess.run([sys.executable, case] + args, capture_output=True, text=True, timeout=timeout)
        if ok in r.stdout or r.returncode >= 0:
            break                                   # (a run killed by a signal is repeated, a wrong result is a failure at once)
    if skip and skip in r.stdout:
        pytest.skip(r.stdout[-300:])
    assert ok in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    print(r.stdout[-1500:])


def test_kd_step_two_rank_gradients_are_the_mean_of_the_shards():
    """tests/kd_dp_case.py two_rank: the KD step under `enable_data_parallel` on two ranks == mean over the ranks of the
    per-shard single-process gradients (ex_pl_audioset.py:287-293 semantics for the loop of ex_audioset.py:139-196)."""
    _run_case(["two_rank"], "KD_TWO_RANK_OK", skip="KD_TWO_RANK_SKIP")


def test_graphed_kd_trainer_with_captured_rccl_all_reduce():
    """tests/kd_dp_case.py graph_rccl: the captured KD step with the bucketed RCCL all-reduce inside the hipGraph (one rank,
    forced bucketing) follows the eager trainer."""
    _run_case(["graph_rccl"], "KD_GRAPH_RCCL_OK")


def test_train_dp_program_runs_on_one_gpu(tmp_path):
    """`python -m efficientat_amd.train_dp` end to end on the synthetic AudioSet stand-in: sharded sampler -> DataLoader ->
    DevicePrefetcher (int16 transport) -> GraphedKDTrainer, a few steps, JSON line with a finite loss."""
    import json
    import os
    import pickle
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    g = torch.Generator().manual_seed(1)
    np.save(tmp_path / "teacher.npy", (torch.randn(64, 527, generator=g) * 2 - 5).numpy())
    with open(tmp_path / "f2i.pkl", "wb") as f:
        pickle.dump({"syn%07d" % i: i % 64 for i in range(0, 4096, 2)}, f)
    env = dict(os.environ, EAT_SYNTH_AUDIOSET="1", EAT_SYNTH_AUDIOSET_TRAIN="64", PYTHONPATH=root)
    # (third run: a dynamic network on the 16-bit surface - bf16 GEMM operands + bf16 storage of the blocks' wide tensors - in
    #  the captured KD step: `--precision bf16 --act_storage bf16`, ex_pl_audioset.py:287-293)
    for extra in (["--model_width", "0.5", "--transport", "int16"], ["--model_width", "0.5", "--no_graph"],
                  ["--model_name", "dymn10_as", "--precision", "bf16", "--act_storage", "bf16", "--transport", "int16"]):
        r = subprocess.run([sys.executable, "-m", "efficientat_amd.train_dp", "--batch_size", "8", "--num_workers", "2",
                            "--n_epochs", "1", "--epoch_len", "64", "--max_steps", "4",
                            "--teacher_preds", str(tmp_path / "teacher.npy"), "--fname_to_index", str(tmp_path / "f2i.pkl"),
                            "--json"] + extra, capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == 4 and np.isfinite(line["final"]["train_loss"]) and line["final"]["distillation_loss"] > 0, line


def test_train_dp_program_two_ranks_end_to_end(tmp_path):
    """`torch.distributed.run --nproc-per-node 2 -m efficientat_amd.train_dp` on the one GPU (both ranks on cuda:0, gloo
    collectives on device tensors, eager trainer): the per-rank sampler shards, the broadcast of rank 0's weights, the bucketed
    gradient exchange and Adam keep the two replicas IDENTICAL over a few KD steps (the spread of a parameter digest over the
    ranks is exactly 0) - BASELINE configs[4]'s loop with N > 1, minus RCCL (which needs one GPU per rank)."""
    import json
    import os
    import pickle
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    g = torch.Generator().manual_seed(1)
    np.save(tmp_path / "teacher.npy", (torch.randn(64, 527, generator=g) * 2 - 5).numpy())
    with open(tmp_path / "f2i.pkl", "wb") as f:
        pickle.dump({"syn%07d" % i: i % 64 for i in range(0, 4096, 2)}, f)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, EAT_SYNTH_AUDIOSET="1", EAT_SYNTH_AUDIOSET_TRAIN="64", PYTHONPATH=root)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), "-m", "efficientat_amd.train_dp", "--backend", "gloo", "--no_graph",
                        "--batch_size", "6", "--num_workers", "1", "--n_epochs", "1", "--epoch_len", "64", "--max_steps", "3",
                        "--model_width", "0.5", "--teacher_preds", str(tmp_path / "teacher.npy"),
                        "--fname_to_index", str(tmp_path / "f2i.pkl"), "--json"],
                       capture_output=True, text=True, timeout=900, env=env, cwd=str(tmp_path))
    if r.returncode != 0 and "gloo" in r.stderr and "not supported" in r.stderr.lower():
        pytest.skip("this torch build's gloo does not reduce device tensors: " + r.stderr[-300:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["steps"] == 3 and np.isfinite(line["final"]["train_loss"]), line
    assert line["param_abs_sum_spread_over_ranks"] == 0.0, line          # the replicas took the same averaged step


def test_graphed_kd_trainer_with_dymn_and_recapture():
    """DyMN under the captured KD step: the DynamicConv temperatures are launch constants, so the step is re-captured after
    `update_params(epoch)` (ex_audioset.py:131-133; here T = 30 -> 1) - the losses of the re-captured trainer follow an eager
    trainer that saw the same schedule, and a trainer that is NOT re-captured keeps computing with the old temperature.
    (DyMN's bank-gradient kernels accumulate with atomics: run-to-run noise of ~1e-6 per step, which Adam's normalisation
    amplifies - hence lr = 1e-4 and a 3e-4 bar where the MN test holds 2e-5.)"""
    from efficientat_amd.dymn import get_model as get_dymn
    from efficientat_amd.train_loop import GraphedKDTrainer
    B, L = 4, 32000
    res = {}
    for tag in ("eager", "graph", "stale"):
        torch.manual_seed(2)
        with contextlib.redirect_stdout(io.StringIO()):
            m = get_dymn(width_mult=0.4).to(DEV).train()
            mel = AugmentMelSTFT(freqm=0, timem=0).to(DEV).train()
        with torch.no_grad():                                      # attention logits of O(1): the temperature matters
            for n_, p_ in m.named_parameters():
                if ".residuals.0.weight" in n_:
                    p_.normal_(0, 0.5)
        for mod in m.modules():
            if isinstance(mod, nn.Dropout):
                mod.p = 0.0
        opt = torch.optim.Adam(m.parameters(), lr=1e-4, capturable=True, fused=True)
        tr = KDTrainer(m, mel, opt, mixup_alpha=0.3) if tag == "eager" else GraphedKDTrainer(m, mel, opt, B, L, mixup_alpha=0.3)
        torch.manual_seed(11); np.random.seed(11)
        losses = []
        for i, epoch in enumerate((0, 40)):
            with contextlib.redirect_stdout(io.StringIO()):
                m.update_params(epoch)                              # T = 30, then T = 1 (dy_block.py:133-139)
            if tag == "graph":
                tr.recapture()
            losses += [float(tr.step(*_kd_batch(2 * i + s, B, L))) for s in range(2)]
        res[tag] = losses
    print(res)
    assert all(abs(a - b) < 3e-4 * max(1.0, abs(a)) for a, b in zip(res["eager"], res["graph"])), res
    assert all(abs(a - b) < 3e-4 * max(1.0, abs(a)) for a, b in zip(res["eager"][:2], res["stale"][:2])), res
    assert abs(res["stale"][2] - res["eager"][2]) > 10 * abs(res["graph"][2] - res["eager"][2]) + 1e-5, res   # old temperature


@pytest.mark.parametrize("prec,storage", [("auto", "fp32"), ("bf16", "bf16")])
def test_mn_captured_step_reproduces_its_gradients_on_every_replay(prec, storage):
    """graphs.GraphedTrainStep on mn10 at learning rate 0: every replay must reproduce the gradients of the eager step on the same
    parameters and input - the zero-initialised accumulators (weight-gradient workspaces, fp64 BatchNorm sums, SE / head pools)
    and the copy / fill nodes of the captured step must behave on replay 2, 3, ... exactly as on replay 1 (see
    test_gpu_dymn.py::test_dymn_captured_step_reproduces_its_gradients_on_every_replay for the defect this guards against)."""
    import contextlib
    import io
    from efficientat_amd.graphs import GraphedTrainStep
    from efficientat_amd.mn import get_model
    from oracle import synth
    B = 16
    sd = synth.synth_state(synth.mn_shapes(1.0), seed=0)
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(B, 1, 128, 1000, generator=g) * 3.0 - 4.0).to(DEV)
    y = (torch.rand(B, 527, generator=g) < 0.01).float().to(DEV)
    keep = (torch.rand(B, 1280, generator=g) < 0.8).float().to(DEV)

    def build():
        with contextlib.redirect_stdout(io.StringIO()):
            m = get_model(width_mult=1.0)
        m.load_state_dict(sd)
        m.to(DEV).train()
        m.train_precision, m.act_storage = prec, storage
        m._drop_mask_override = keep
        return m
    ref = build()
    logits, _ = ref(x)
    F.binary_cross_entropy_with_logits(logits, y).backward()
    ref_g = {n: p.grad.detach().clone() for n, p in ref.named_parameters()}
    gmax = max(float(v.norm()) for v in ref_g.values())
    model = build()
    step = GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=0.0), F.binary_cross_entropy_with_logits, x, y)
    tol = 2e-3 if storage == "fp32" else 5e-2
    for r in range(4):
        step(step.x, step.y)
        torch.cuda.synchronize()
        worst = (0.0, None)
        for n, p in model.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), (r, n)
            if float(ref_g[n].norm()) < 1e-3 * gmax:
                continue
            e = float((p.grad - ref_g[n]).norm() / ref_g[n].norm())
            if e > worst[0]:
                worst = (e, n)
        assert worst[0] < tol, (r, worst)


@pytest.mark.parametrize("name", ["mn10", "mn40_bf16", "dymn20_bf16"])
def test_training_steps_read_no_uninitialised_memory(name):
    """tools/uninit_hunt.py in a child process: every `torch.empty` filled with NaN (torch.utils.deterministic.
    fill_uninitialized_memory), three eager training steps and six replays of the captured step (graphs.GraphedTrainStep, the
    fills are captured too: every replay re-poisons) - loss, gradients and parameters must stay finite.  A kernel that reads
    what neither it nor its producer wrote - or an accumulator that is not re-zeroed on replay - turns this red on EVERY run
    instead of in one fresh process out of twenty."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "uninit_hunt.py"), name, "8"], capture_output=True, text=True,
                       timeout=900, cwd=root)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith(("step ", "graph step "))]
    assert len(lines) == 9, r.stdout[-2000:]
    for ln in lines:
        assert "loss nan" not in ln and "loss inf" not in ln, ln
        if ln.startswith("step "):                      # eager: "... non-finite grads 0 []; params 0 []"
            assert "non-finite grads 0 []; params 0 []" in ln, ln
        else:                                           # captured: "... non-finite params 0 []; grads []"
            assert "non-finite params 0 []; grads []" in ln, ln


def _fused_adam(m):
    from efficientat_amd.optim import FusedAdam
    return FusedAdam(m.parameters(), lr=torch.tensor(1e-3, device=DEV), capturable=True)


def _kd_trainer(tag, opt_for, tlogits, f2i, B, L):
    from efficientat_amd.train_loop import GraphedKDTrainer
    m = _kd_setup()
    with contextlib.redirect_stdout(io.StringIO()):
        mel = AugmentMelSTFT(freqm=0, timem=0).to(DEV).train()
    opt = opt_for(m)
    kw = dict(teacher_preds=tlogits, fname_to_index=f2i, kd_lambda=0.1, mixup_alpha=0.3)
    return m, opt, (KDTrainer(m, mel, opt, **kw) if tag == "eager" else GraphedKDTrainer(m, mel, opt, B, L, **kw))


def _kd_teacher():
    g = torch.Generator().manual_seed(5)
    return torch.randn(40, 527, generator=g) * 2 - 5, {"syn%07d" % i: i % 40 for i in range(0, 30, 2)}


def _assert_trainers_agree(le, lg, pe, pg):
    # the tolerances of test_graphed_kd_trainer_follows_the_eager_trainer
    assert all(abs(a - b) < 2e-5 * max(1.0, abs(a)) for a, b in zip(le, lg)), (le, lg)
    d = (pe - pg).abs()
    frac = float((d > 1e-4).float().mean())
    assert float(d.max()) <= 6.1e-3 and frac < 0.02, (float(d.max()), frac)


def test_graphed_kd_trainer_with_fused_adam_follows_the_eager_trainer():
    """train_dp's default: GraphedKDTrainer with FusedAdam(capturable=True, tensor lr) - the capture's warm-up steps create
    the optimizer state and its step counter, which the trainer must put back to zero - against the eager KDTrainer."""
    B, L = 6, 32000
    tlogits, f2i = _kd_teacher()
    res = {}
    for tag in ("eager", "graph"):
        m, opt, tr = _kd_trainer(tag, _fused_adam, tlogits, f2i, B, L)
        torch.manual_seed(11); np.random.seed(11)
        losses = [float(tr.step(*_kd_batch(s, B, L))) for s in range(3)]
        torch.cuda.synchronize()
        res[tag] = (losses, torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu(), tr.epoch_stats())
        assert {float(opt.state[p]["step"]) for p in m.parameters()} == {3.0}, tag
    _assert_trainers_agree(res["eager"][0], res["graph"][0], res["eager"][1], res["graph"][1])
    se, sg = res["eager"][2], res["graph"][2]
    assert all(abs(se[k] - sg[k]) < 2e-5 * max(1.0, abs(se[k])) for k in se), (se, sg)


def test_graphed_kd_trainer_with_fused_adam_resumes_from_a_checkpoint():
    """4 graphed steps with a checkpoint (model + optimizer state, torch.save) taken after the second; a new model, FusedAdam
    and trainer (whose constructor has already captured its step) load it and take steps 3 and 4: the same losses and
    parameters as the uninterrupted run.  (Both continue from the one checkpoint: two uninterrupted runs differ already, by
    the round-off of the atomics in backward that Adam turns into +-lr moves, more than the trainer tolerance by step 4.)"""
    B, L = 6, 32000
    tlogits, f2i = _kd_teacher()
    m, opt, tr = _kd_trainer("graph", _fused_adam, tlogits, f2i, B, L)
    torch.manual_seed(11); np.random.seed(11)
    full = [float(tr.step(*_kd_batch(s, B, L))) for s in range(2)]
    buf = io.BytesIO()
    torch.save(dict(model=m.state_dict(), opt=opt.state_dict()), buf)
    rng = torch.get_rng_state(), np.random.get_state()
    full += [float(tr.step(*_kd_batch(s, B, L))) for s in range(2, 4)]
    torch.cuda.synchronize()
    p_full = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu()
    del m, opt, tr

    m, opt, tr = _kd_trainer("graph", _fused_adam, tlogits, f2i, B, L)
    buf.seek(0)
    ck = torch.load(buf, weights_only=False)
    m.load_state_dict(ck["model"])
    opt.load_state_dict(ck["opt"])
    for i, p in enumerate(m.parameters()):                # the captured step's own buffers now hold the checkpoint
        for k in ("exp_avg", "exp_avg_sq"):
            assert torch.equal(opt.state[p][k].cpu(), ck["opt"]["state"][i][k].cpu()), (i, k)
        assert float(opt.state[p]["step"]) == 2.0
    torch.set_rng_state(rng[0]); np.random.set_state(rng[1])
    part = [float(tr.step(*_kd_batch(s, B, L))) for s in range(2, 4)]
    torch.cuda.synchronize()
    p_part = torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu()
    _assert_trainers_agree(full[2:], part, p_full, p_part)
    assert {float(opt.state[p]["step"]) for p in m.parameters()} == {4.0}
