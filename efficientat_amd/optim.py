"""The optimizer of the reference's training loop on the HIP path: `torch.optim.Adam` / `AdamW` (ex_audioset.py:86-91) with the
same constructor arguments and state-dict layout (`exp_avg`, `exp_avg_sq`, `step` per parameter), whose `step()` is ONE launch
of `eat_adam_multi` over every parameter (+ a one-thread counter kernel in the capturable form) instead of torch's multi-tensor
chunks.  SURVEY 8(f) row f1 / K17 allow torch's fused optimizer; this is the in-library form of the same update."""
from collections import defaultdict

import numpy as np
import torch

from . import _lib

_CHUNK = 4096
_TORCH_ONLY = ("amsgrad", "maximize", "differentiable", "foreach", "fused")


def _from_torch_group(group, own):
    """A parameter group of torch's Adam / AdamW (or of this optimizer) in this optimizer's keys, in place: torch's
    `decoupled_weight_decay` -> `decoupled` (a checkpoint with neither keeps `own["decoupled"]`), torch-only switches dropped
    (the ones that change the update must be off)."""
    dwd = group.pop("decoupled_weight_decay", None)
    if "decoupled" not in group:
        group["decoupled"] = bool(own["decoupled"]) if dwd is None else bool(dwd)
    elif dwd is not None and bool(dwd) != bool(group["decoupled"]):
        raise ValueError(f"FusedAdam: parameter group with decoupled={group['decoupled']} and decoupled_weight_decay={dwd}")
    for k in _TORCH_ONLY:
        if group.pop(k, False) and k in ("amsgrad", "maximize", "differentiable"):
            raise ValueError(f"FusedAdam: {k}=True is not supported")
    group.setdefault("capturable", bool(own["capturable"]))


def _one_step(sts, gi):
    """The common step of a capturable group's parameter states (one counter per group)."""
    steps = {float(st["step"]) for st in sts}
    if len(steps) != 1:
        raise _lib.EatHipError(f"FusedAdam(capturable=True): the loaded states of group {gi} are at different steps "
                               f"{sorted(steps)} - a capturable group shares one step counter")
    return steps.pop()


class FusedAdam(torch.optim.Optimizer):
    """Adam (decoupled=False: L2 weight decay, `torch.optim.Adam`) or AdamW (decoupled=True).  fp32 CUDA parameters with fp32
    gradients; `capturable=True` keeps the step counter on the device (required inside a hipGraph capture); `lr` may be a
    0-dim / 1-element float32 CUDA tensor that a scheduler writes (then it is read on the device).  No amsgrad / maximize.

    Every parameter keeps its own `step` as in torch: eager parameters that skipped steps (no gradient) are updated in the same
    launch with their own bias corrections (the chunk table's `pad` field holds their step offset).  A capturable group shares
    ONE counter on the device (every `state[p]["step"]` is a view of it): all its parameters must take every step, so a
    parameter without state joining a group after its first step, or one with state that skips a step, is an error.

    `step(grad_scale=s)` MULTIPLIES the gradients by s (torch's fused-Adam kwarg of that name divides by it).

    `state_dict()` / `load_state_dict()` use torch's layout and exchange checkpoints with `torch.optim.Adam` / `AdamW` in both
    directions (`decoupled` <-> torch's `decoupled_weight_decay`; `state_dict()` hands out an independent `step` tensor per
    parameter).  `capturable` and a tensor `lr` belong to this optimizer, not to the checkpoint: a load keeps them (the loaded
    rate is written into the existing lr tensor).  Once a step has been captured into a graph, a load copies the loaded moments
    and steps into the buffers the graph holds."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, capturable=False):
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"invalid betas {betas}")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled=decoupled,
                                      capturable=capturable))
        self._tables = {}
        self._spare = {}
        self._counters = {}
        self._captured = []
        self._layouts = {}
        self._in_graph = False                              # a step() has been captured into a graph

    def __setstate__(self, state):
        super().__setstate__(state)
        for k in ("_tables", "_spare", "_counters", "_layouts"):
            self.__dict__.setdefault(k, {})
        self.__dict__.setdefault("_captured", [])
        self.__dict__.setdefault("_in_graph", False)
        for group in self.param_groups:
            _from_torch_group(group, self.defaults)

    def state_dict(self):
        sd = super().state_dict()
        # an independent `step` per parameter (the capturable ones are views of the group's counter: a checkpoint loaded
        # into torch's Adam would otherwise advance one shared tensor once per parameter), torch's name of the decay mode
        state = {k: {n: (t.detach().clone() if n == "step" and torch.is_tensor(t) else t) for n, t in st.items()}
                 for k, st in sd["state"].items()}
        groups = [dict(g, decoupled_weight_decay=bool(g["decoupled"])) for g in sd["param_groups"]]
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, state_dict):
        own = [dict(capturable=g["capturable"], decoupled=g["decoupled"], lr=g["lr"]) for g in self.param_groups]
        live = {p: st for p, st in self.state.items() if st} if self._in_graph else None
        saved = state_dict["param_groups"]
        if len(saved) != len(own):
            raise ValueError("loaded state dict has a different number of parameter groups")
        groups = []
        for sg, o in zip(saved, own):
            sg = dict(sg)
            _from_torch_group(sg, o)
            sg["capturable"] = o["capturable"]             # where this optimizer keeps its counters, not the checkpoint's
            groups.append(sg)
        super().load_state_dict(dict(state_dict, param_groups=groups))
        with torch.no_grad():
            for g, o in zip(self.param_groups, own):
                if torch.is_tensor(o["lr"]) and g["lr"] is not o["lr"]:
                    o["lr"].fill_(float(g["lr"]))          # a scheduler (or a captured graph) holds this tensor
                    g["lr"] = o["lr"]
            if live is not None:
                self._load_in_place(live)
                return
            # the chunk tables hold the old moment buffers' addresses, the counters the old steps
            self._tables, self._layouts, self._counters = {}, {}, {}
            for gi, g in enumerate(self.param_groups):
                sts = [self.state[p] for p in g["params"] if self.state.get(p)]
                if not g["capturable"]:
                    for st in sts:
                        st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
                elif sts:
                    ctr = self._counters[gi] = torch.full((1,), _one_step(sts, gi), dtype=torch.float32, device=g["params"][0].device)
                    for st in sts:
                        st["step"] = ctr[0]

    def _load_in_place(self, live):
        """load_state_dict after a capture: the graph holds the addresses of the moment buffers, of the counters and of the
        chunk tables - the loaded values go into those buffers and nothing is rebuilt."""
        loaded, self.state = self.state, defaultdict(dict, live)
        steps = {}
        for gi, g in enumerate(self.param_groups):
            for p in g["params"]:
                new = loaded.get(p)
                if new and p not in live:
                    raise _lib.EatHipError("FusedAdam: the loaded state holds a parameter that had no state when the step was "
                                           "captured - the captured graph cannot update it")
                for k in ("exp_avg", "exp_avg_sq"):
                    if new and p in live and new[k].shape != live[p][k].shape:
                        raise _lib.EatHipError(f"FusedAdam: loaded {k} {tuple(new[k].shape)} for a parameter "
                                               f"{tuple(live[p][k].shape)}")
            sts = [loaded.get(p) or dict(step=0.0) for p in g["params"] if p in live]
            if sts and g["capturable"]:
                if gi not in self._counters:
                    raise _lib.EatHipError(f"FusedAdam: group {gi} has state but no step counter")
                steps[gi] = _one_step(sts, gi)
        for gi, step in steps.items():
            self._counters[gi].fill_(step)
        for p, old in live.items():
            new = loaded.get(p)
            for k in ("exp_avg", "exp_avg_sq"):
                if new:
                    old[k].copy_(new[k])
                else:
                    old[k].zero_()
            if not old["step"].is_cuda:                    # (capturable: a view of the group's counter, written above)
                old["step"] = torch.tensor(float(new["step"]) if new else 0.0, dtype=torch.float32)

    def _state(self, p, capturable):
        st = self.state[p]
        if not st:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.EatHipError("FusedAdam: run one eager step before capturing (the moment buffers and the step counter "
                                       "must exist outside the graph - a captured initialisation would re-run on every replay)")
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device if capturable else "cpu")
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    def _table(self, gi, ps, offs):
        """Chunk table of a parameter group (device tensor), rebuilt when a parameter, a moment buffer or a gradient moved, or
        the parameters' step offsets (`offs`, int32 per parameter: the table's `pad`) changed.  (None, 0) when every parameter
        has 0 elements.  Outside a capture the upload is a synchronous copy; inside a stream capture (the gradients of a
        captured step live at new addresses) it goes through a pinned buffer allocated by the first eager step - the captured
        copy node re-reads that buffer on every replay, so it is used for ONE capture only (`_spare`)."""
        key = (tuple((p.data_ptr(), p.grad.data_ptr()) for p in ps), offs.tobytes())
        cached = self._tables.get(gi)
        if cached is not None and cached[0] == key:
            return cached[1], cached[2]
        # the chunk layout depends on the parameters and their moment buffers only: offsets / lengths / parameter and moment
        # addresses are built once per such set, a rebuild (gradients at new addresses: an eager data-parallel step hands out
        # a fresh bucket buffer every pass) only adds the gradients' base addresses - vectorised, no Python loop over ~1500
        # chunks
        lay = self._layouts.get(gi)
        pkey = tuple((p.data_ptr(), self.state[p]["exp_avg"].data_ptr(), self.state[p]["exp_avg_sq"].data_ptr()) for p in ps)
        if lay is None or lay[0] != pkey:
            idx, offsets, lens = [], [], []
            for i, p in enumerate(ps):
                st = self.state[p]
                if p.dtype != torch.float32 or not p.is_cuda:
                    raise _lib.EatHipError("FusedAdam: fp32 CUDA parameters and gradients only")
                if not p.is_contiguous():
                    raise _lib.EatHipError("FusedAdam: parameters and gradients must be contiguous")
                for k in ("exp_avg", "exp_avg_sq"):
                    t = st[k]
                    if t.dtype != torch.float32 or t.device != p.device or t.shape != p.shape or not t.is_contiguous():
                        raise _lib.EatHipError(f"FusedAdam: state {k} of a parameter {tuple(p.shape)} is {t.dtype} "
                                               f"{tuple(t.shape)} on {t.device} (fp32, contiguous, the parameter's shape)")
                n = p.numel()
                o = np.arange(0, n, _CHUNK, dtype=np.int64)
                idx.append(np.full(o.shape, i, dtype=np.int64))
                offsets.append(o)
                lens.append(np.minimum(_CHUNK, n - o))
            idx, offsets, lens = np.concatenate(idx), np.concatenate(offsets), np.concatenate(lens).astype(np.int32)
            boffs = (4 * offsets).astype(np.uint64)
            pb = np.array([k[0] for k in pkey], dtype=np.uint64)[idx] + boffs
            mb = np.array([k[1] for k in pkey], dtype=np.uint64)[idx] + boffs
            vb = np.array([k[2] for k in pkey], dtype=np.uint64)[idx] + boffs
            lay = self._layouts[gi] = (pkey, idx, boffs, lens, pb, mb, vb)
        _, idx, boffs, lens, pb, mb, vb = lay
        if not lens.shape[0]:
            return None, 0                                     # only 0-element parameters: nothing to launch
        for p in ps:
            if p.grad.dtype != torch.float32 or not p.grad.is_contiguous() or p.grad.shape != p.shape:
                raise _lib.EatHipError("FusedAdam: fp32 contiguous gradients of the parameter's shape only")
        gb = np.array([k[1] for k in key[0]], dtype=np.uint64)[idx] + boffs
        tab = np.zeros((lens.shape[0],), dtype=[("p", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<i4"), ("pad", "<i4")])
        tab["p"], tab["g"], tab["m"], tab["v"], tab["n"], tab["pad"] = pb, gb, mb, vb, lens, offs[idx]
        recs = tab
        raw = torch.from_numpy(tab.view(np.uint8).copy())
        if torch.cuda.is_current_stream_capturing():
            spare = self._spare.get(gi)
            if not spare or spare[0].numel() != raw.numel():
                raise _lib.EatHipError("FusedAdam: the gradients moved inside a stream capture and no staging buffer is left - run "
                                       "one eager step with this set of parameters before capturing, and capture once per optimizer")
            host, dev_tab = spare
            self._spare[gi] = None
            host.copy_(raw)
            dev_tab.copy_(host, non_blocking=True)
            self._tables[gi] = (key, dev_tab, len(recs))
            self._captured.append((host, dev_tab))      # the graph's copy node re-reads them on every replay: never freed
        else:
            dev_tab = raw.to(ps[0].device)
            self._tables[gi] = (key, dev_tab, len(recs))
            if not self._spare.get(gi):                                # staging for the next capture (same parameters => same size)
                self._spare[gi] = (torch.empty_like(raw).pin_memory(), torch.empty_like(dev_tab))
        return dev_tab, len(recs)

    @staticmethod
    def _lr(lr):
        """(device pointer, 0) for a float32 CUDA tensor of one element, (None, value) for a float or a CPU tensor."""
        if not torch.is_tensor(lr):
            return None, float(lr)
        if lr.numel() != 1:
            raise _lib.EatHipError(f"FusedAdam: a tensor lr must hold one element, not {lr.numel()}")
        if not lr.is_cuda:
            return None, float(lr)
        if lr.dtype != torch.float32:
            raise _lib.EatHipError(f"FusedAdam: a CUDA tensor lr is read on the device as float32, not {lr.dtype}")
        return lr.data_ptr(), 0.0

    @torch.no_grad()
    def step(self, closure=None, grad_scale=1.0):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        capturing = torch.cuda.is_current_stream_capturing()
        for gi, group in enumerate(self.param_groups):
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            cap = bool(group["capturable"])
            if capturing:
                if not cap:
                    raise _lib.EatHipError("FusedAdam: capturable=False bakes the step into the launch - a captured step needs "
                                           "capturable=True")
                self._in_graph = True
            fresh = [not self.state.get(p) for p in ps]
            sts = [self._state(p, cap) for p in ps]
            lr_ptr, lr_val = self._lr(group["lr"])
            if cap:
                # one counter per group on the device: every parameter's `step` is a view of it
                ctr = self._counters.get(gi)
                if ctr is None:
                    if capturing:
                        raise _lib.EatHipError("FusedAdam: run one eager step before capturing")
                    steps = {float(st["step"]) for st in sts}
                    if len(steps) != 1:
                        raise _lib.EatHipError(f"FusedAdam(capturable=True): the parameters of group {gi} are at different "
                                               f"steps {sorted(steps)} - a capturable group shares one step counter")
                    ctr = self._counters[gi] = torch.full((1,), steps.pop(), dtype=torch.float32, device=ps[0].device)
                    for st in sts:
                        st["step"] = ctr[0]
                elif any(fresh):
                    raise _lib.EatHipError(f"FusedAdam(capturable=True): {sum(fresh)} parameter(s) of group {gi} got their first "
                                           "gradient after the group's first step - a capturable group shares one step counter, "
                                           "so every parameter must take every step")
                if len(ps) != len(group["params"]) and any(p.grad is None and self.state.get(p) for p in group["params"]):
                    raise _lib.EatHipError(f"FusedAdam(capturable=True): a parameter of group {gi} with state has no gradient - "
                                           "its step would advance with the group's shared counter without an update")
                offs = np.zeros((len(ps),), dtype=np.int32)
                step_ptr, step_val = ctr.data_ptr(), 0.0
            else:
                steps = np.array([float(st["step"]) for st in sts])
                base = steps.min()
                offs = (steps - base).astype(np.int32)
                step_ptr, step_val = None, float(base)
            tab, n = self._table(gi, ps, offs)
            b1, b2 = group["betas"]
            if n:
                _lib.call("eat_adam_multi", tab.data_ptr(), n, lr_ptr, lr_val, step_ptr, step_val, float(b1), float(b2),
                          float(group["eps"]), float(group["weight_decay"]), 1 if group["decoupled"] else 0, float(grad_scale),
                          torch.cuda.current_stream().cuda_stream)
            elif cap:
                ctr += 1                                  # 0-element parameters only: no update, the steps still advance
            if not cap:
                for st in sts:
                    st["step"] = st["step"] + 1
        return loss
