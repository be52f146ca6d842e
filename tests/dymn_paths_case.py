"""One eager dymn10 train step in a process of its own, for the switches efficientat_amd/dymn_train.py reads from the
environment at import (tests/test_gpu_dymn_paths.py sets them): prints one JSON line with the number of calls per library
entry point and the largest gradient norm.  argv[1]: train_precision."""
import collections
import contextlib
import io
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from efficientat_amd import _lib  # noqa: E402
from efficientat_amd.dymn import get_model  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        model = get_model(width_mult=1.0)
    model.classifier[4].p = 0.0
    model.to(dev).train()
    model.train_precision = sys.argv[1]
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(3, 1, 128, 200, generator=g) * 3.0 - 4.0).to(dev)
    y = (torch.rand(3, 527, generator=g) < 0.1).float().to(dev)
    calls, real = collections.Counter(), (_lib.call, _lib.call_rc)

    def call(name, *a):
        calls[name] += 1
        return real[0](name, *a)

    def call_rc(name, *a):
        calls[name] += 1
        return real[1](name, *a)
    _lib.call, _lib.call_rc = call, call_rc
    logits, _ = model(x)
    F.binary_cross_entropy_with_logits(logits, y).backward()
    torch.cuda.synchronize()
    grads = [p.grad for p in model.parameters()]
    ok = all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    print(json.dumps({"calls": dict(calls), "finite": ok, "gmax": max(float(g.norm()) for g in grads)}))


if __name__ == "__main__":
    main()
