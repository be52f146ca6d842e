"""CPU tests of bench.py's options: `--full` is off by default and the options that only make sense with its measurements
refuse to run without it; `dump_outputs` (--dump-outputs) writes float32 / float64 .npy files within its byte budget, cut
to the same seeded sample of elements on every call."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_plain_run_is_the_default():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not a.full and a.dump_outputs is None and a.reps is None and a.steps == 7 and a.warmup == 2
    a = bench.parse_args(["--full", "--kernel-table", "--calibrate-traffic", "--dump-outputs", "d"])
    assert a.full and a.kernel_table and a.calibrate_traffic and a.dump_outputs == "d"


@pytest.mark.parametrize("flag", ["--kernel-table", "--calibrate-traffic"])
def test_full_only_options_need_full(flag, capsys):
    with pytest.raises(SystemExit) as e:
        bench.parse_args([flag])
    assert e.value.code == 2
    assert "--full" in capsys.readouterr().err


def _read(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_within_budget_and_reproducible(tmp_path):
    g = torch.Generator().manual_seed(0)
    arrays = {"loss": torch.tensor([0.25]), "params": torch.arange(300_000, dtype=torch.float32).reshape(600, 500),
              "grads": torch.randn(200_000, generator=g, dtype=torch.float64), "bn_stats": torch.randn(7, 5, generator=g)}
    budget = 1_000_000
    bench.dump_outputs(str(tmp_path / "a"), arrays, budget=budget)
    bench.dump_outputs(str(tmp_path / "b"), arrays, budget=budget)
    a, b = _read(tmp_path / "a"), _read(tmp_path / "b")
    assert sorted(a) == ["bn_stats", "grads", "loss", "params"]
    assert sum(v.nbytes for v in a.values()) <= budget
    assert a["params"].dtype == np.float32 and a["grads"].dtype == np.float64
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    # small arrays whole, large ones a sample of their own elements, in order
    assert np.array_equal(a["loss"], [0.25]) and np.array_equal(a["bn_stats"], arrays["bn_stats"].numpy())
    # params[i] == i: the sample is a strictly increasing set of element positions
    assert 0 < a["params"].size < 300_000 and a["params"].ndim == 1
    assert np.all(np.diff(a["params"]) > 0) and a["params"][0] >= 0 and a["params"][-1] < 300_000


def test_dump_outputs_under_budget_writes_everything(tmp_path):
    x = torch.arange(10_000, dtype=torch.float32).reshape(100, 100)
    bench.dump_outputs(str(tmp_path), {"params": x})
    assert np.array_equal(np.load(tmp_path / "params.npy"), x.numpy())
