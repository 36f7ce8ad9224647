"""Exponential moving average (EMA) of the weights, updated on the device right after the optimizer step.

    ema = ModelEMA(model, decay=0.999, warmup=True, guard=None)
    ... optimizer.step(); ema.update()         # two launches on the current stream; capturable into a HIP graph
    ema.swap(); validate(model); ema.swap()    # the averaged weights in place: same parameter addresses, no second model

One update is umi_ema_pre + umi_ema_multi (include/unetmi.h): the first advances a device block of UMI_EMA_LEN doubles -- the
decay d_t of this update, with the warm-up d_t = min(d, (1 + t) / (10 + t)) of timm.ModelEmaV2 / mean teacher, and the fp32
weight w_f = (float)(1 - d_t) --, the second applies e <- e + w_f * (p - e) to every shadow in one launch, as three separate
fp32 roundings.  `ema_state_update_numpy` and `ema_update_numpy` are the NumPy statements of the two; the device results equal
them bit for bit.  A `umi.optim.GradGuard` gates the update on the device: a step the guard skipped leaves the shadows and the
update count untouched, also inside a replayed graph.

`Trainer(..., ema=...)` (keyword-only, after `resume`; singe_train / multi_task_train): None / False = nothing of this runs; True,
a float (the decay), `dict(decay=0.999, warmup=True, validate=True)` or a ready `umi.ema.ModelEMA` = an exponential moving average
of the parameters that require a gradient (buffers are not averaged: the averaged model is the averaged parameters plus the live
BatchNorm running statistics, as `AveragedModel(use_buffers=False)`); anything else raises ValueError.  The shadows are copies of
the parameters taken before the first step.  `ema.update()` (two launches, `umi_ema_pre` + `umi_ema_multi`) follows
`optimizer.step()` inside the step body, so a captured step contains it; in the deferred data-parallel path it follows `flush()` +
`optimizer.step()` after each replay.  The `grad_guard` block gates it on the device: a skipped step leaves the shadows' bits and
the update count alone, eagerly and in a replay.  With `validate=True` (the default) the validation phase runs on the averaged
weights IN PLACE: `ema.swap()` exchanges parameters and shadows after the data-parallel phase's BatchNorm broadcast (one launch;
the parameter versions are bumped, so `ops.PackCache` and the eval graphs re-pack), and swaps back after the best-model decision
-- loss, score, `best_model`, `epochN.pt` and `best.pt` are those of the averaged weights (what is validated is what is saved, and
what train() returns), `last_epoch.pt` keeps the live weights; under `async_checkpoints` the best files then come from a host copy
of the best-model arena taken while the average is swapped in, not from the copy behind `last_epoch.pt`.  `validate=False` only
maintains the average (`trainer.ema`: `averaged()`, `copy_to(model)`, `state_dict()`).  One line per epoch goes to `logs.txt` after
the training phase, on rank 0: `EMA on epoch N: decay D, updates U` (D = the decay of the last update).  The shadows and the state
block are part of the run state (umi/run_state.py: `ema.shadow.<name>`, `ema.state`): `resume` and `snapshot_run_state()` /
`restore_run_state()` carry them, a resumed run stays bit-identical, a run-state file written with `ema` and read without it (or
the reverse) raises before anything is modified, and the data-parallel replica check covers them.  With 'multi_task_loss_ratio'
train() raises NotImplementedError before the first step.
"""
import collections

import numpy as np
import torch

from . import lib as L

# the state block of include/unetmi.h: EMA["DECAY"] etc. = the UMI_EMA_* slot indices
EMA_LEN = L.UMI_EMA_LEN
EMA = {k[len("UMI_EMA_"):]: v for k, v in L.ENUMS.items() if k.startswith("UMI_EMA_") and k != "UMI_EMA_LEN"}
STATE_KEY = "_ema_state"


def ema_state_update_numpy(state, skip):
    """The arithmetic of umi_ema_pre in float64: `state` (the UMI_EMA_LEN doubles of a state block) after one more update, or
    after an update that the guard skipped (`skip`: only ACTIVE changes).  Returns a new array."""
    st = np.array(state, dtype=np.float64)
    if skip:
        st[EMA["ACTIVE"]] = 0.0
        return st
    t, d = st[EMA["UPDATES"]], st[EMA["DECAY"]]
    if st[EMA["WARMUP"]] != 0.0:
        w = (np.float64(1.0) + t) / (np.float64(10.0) + t)
        d = w if w < d else d
    st[EMA["LAST"]] = d
    st[EMA["WEIGHT"]] = np.float64(np.float32(np.float64(1.0) - d))
    st[EMA["ACTIVE"]] = 1.0
    st[EMA["UPDATES"]] = t + 1.0
    return st


def ema_update_numpy(e, p, w_f):
    """The arithmetic of umi_ema_multi: e + w_f * (p - e) in float32, three roundings (NumPy has no fused multiply-add).
    Returns a new float32 array."""
    e, p, w = np.asarray(e, dtype=np.float32), np.asarray(p, dtype=np.float32), np.float32(w_f)
    with np.errstate(all="ignore"):
        return e + w * (p - e)


class ModelEMA:
    """fp32 shadows of the parameters of `model_or_params` that require a gradient, in `named_parameters()` order (an iterable
    of parameters, or of (name, parameter) pairs, is taken as it comes), created as copies of the parameters.

    Buffers are NOT shadowed: the averaged model is the averaged parameters plus the live BatchNorm running statistics, the
    choice of `torch.optim.swa_utils.AveragedModel(use_buffers=False)`.

        update()         one more update on the current stream.  Capturable: the state block, the descriptor tables and their
                         staging buffers are allocated by the first eager update (the warm-up step), never inside a capture;
                         at most two captures share the tables, as for a umi.optim optimizer
        swap()           exchanges parameters and shadows in place and bumps the parameters' versions, so `ops.PackCache` and
                         `GraphedEval.refresh()` re-pack; `swapped` tells which side is live; update() while swapped raises
        averaged()       name -> tensor holding the average right now (the shadows, or the parameters while swapped)
        copy_to(model)   the average into `model`'s parameters of the same names
        state_dict() / load_state_dict()   the average by parameter name plus the state doubles under '_ema_state'
                         (`model.load_state_dict(ema.state_dict(), strict=False)` gives the averaged model)
        sync_host()      the state block read back, as a dict (one small copy; for logs)
        tensors()        name -> tensor of every shadow and the state block, for umi.snapshot.Snapshot and the fingerprint

    CPU parameters take a torch statement of the same three float32 operations, with the state machine in NumPy float64."""

    def __init__(self, model_or_params, decay=0.999, warmup=True, guard=None):
        if not (0.0 <= float(decay) < 1.0):
            raise ValueError(f"ModelEMA: decay must be in [0, 1), not {decay!r}")
        if isinstance(model_or_params, torch.nn.Module):
            named = [(n, p) for n, p in model_or_params.named_parameters() if p.requires_grad]
        else:
            named = [(it if isinstance(it, (tuple, list)) else (str(i), it)) for i, it in enumerate(model_or_params)]
            named = [(n, p) for n, p in named if p.requires_grad]
        if len({n for n, _ in named}) != len(named):
            raise ValueError("ModelEMA: parameter names repeat")
        devs = {p.device for _, p in named}
        if len(devs) > 1:
            raise ValueError(f"ModelEMA: the parameters live on several devices ({sorted(map(str, devs))})")
        for n, p in named:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError(f"ModelEMA: parameter {n} is not a contiguous fp32 tensor")
        self.device = devs.pop() if devs else torch.device("cpu")
        self.cuda = self.device.type == "cuda"
        if self.cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("umi.ema.ModelEMA: built inside a HIP-graph capture; build it before the warm-up step")
        if guard is not None and not self.cuda:
            raise ValueError("ModelEMA: a GradGuard lives on the device; CPU parameters take guard=None")
        self.names = [n for n, _ in named]
        self.params = [p for _, p in named]
        self.shadows = [p.detach().clone(memory_format=torch.contiguous_format) for p in self.params]
        st = np.zeros(EMA_LEN, dtype=np.float64)
        st[EMA["DECAY"]], st[EMA["WARMUP"]] = float(decay), 1.0 if warmup else 0.0
        self.state = torch.from_numpy(st).to(self.device)
        self.guard = guard
        self.swapped = False
        self._tables = {}

    # ---- the update --------------------------------------------------------------------------------------------------------
    def _rows(self):
        return [(p.data_ptr(), 0, s.data_ptr(), 0, p.numel()) for p, s in zip(self.params, self.shadows)]

    @torch.no_grad()
    def update(self):
        if self.swapped:
            raise RuntimeError("umi.ema.ModelEMA: update() while swapped (the parameters hold the average); swap() back first")
        if not self.cuda:
            st = ema_state_update_numpy(self.state.numpy(), False)
            self.state.numpy()[:] = st
            w = torch.tensor(st[EMA["WEIGHT"]], dtype=torch.float32)
            for p, s in zip(self.params, self.shadows):
                s.add_((p.detach() - s).mul_(w))                   # subtract, multiply, add: one float32 rounding each
            return self
        from . import ops, optim
        with torch.cuda.device(self.device):
            cap = torch.cuda.is_current_stream_capturing()
            ptr, n, blocks = optim._table(self._tables, ("ema",), cap, self._rows())
            guard = None if self.guard is None else self.guard._device_state().data_ptr()
            stream = ops._stream()
            L.call("umi_ema_pre", self.state.data_ptr(), guard, stream)
            L.call("umi_ema_multi", ptr, n, blocks, self.state.data_ptr(), stream)
        return self

    @torch.no_grad()
    def swap(self):
        if not self.cuda:
            for p, s in zip(self.params, self.shadows):
                keep = p.detach().clone()
                p.copy_(s)                                          # (bumps the version)
                s.copy_(keep)
        else:
            from . import ops, optim
            with torch.cuda.device(self.device):
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("umi.ema.ModelEMA: swap() cannot run inside a HIP-graph capture")
                ptr, n, blocks = optim._table(self._tables, ("ema",), False, self._rows())
                L.call("umi_ema_swap_multi", ptr, n, blocks, ops._stream())
            for p in self.params:
                optim._bump(p)
        self.swapped = not self.swapped
        return self

    # ---- the average as named tensors ----------------------------------------------------------------------------------------
    def averaged(self):
        side = self.params if self.swapped else self.shadows
        return collections.OrderedDict((n, t.detach()) for n, t in zip(self.names, side))

    @torch.no_grad()
    def copy_to(self, model):
        own = dict(model.named_parameters())
        missing = [n for n in self.names if n not in own]
        if missing:
            raise KeyError(f"ModelEMA.copy_to: the model has no parameter {missing[0]!r}")
        for n, t in self.averaged().items():
            if own[n] is not t and own[n].data_ptr() != t.data_ptr():
                own[n].copy_(t)
        return model

    def tensors(self):
        out = collections.OrderedDict(("shadow." + n, s) for n, s in zip(self.names, self.shadows))
        out["state"] = self.state
        return out

    def state_dict(self):
        out = collections.OrderedDict((n, t.clone()) for n, t in self.averaged().items())
        out[STATE_KEY] = self.state.clone()
        return out

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        if list(state_dict) != self.names + [STATE_KEY]:
            raise ValueError("ModelEMA.load_state_dict: the keys are not this average's parameter names plus "
                             f"{STATE_KEY!r}, in order")
        live = self.averaged()
        for n, t in live.items():
            if state_dict[n].shape != t.shape or state_dict[n].dtype != t.dtype:
                raise ValueError(f"ModelEMA.load_state_dict: {n} is {tuple(state_dict[n].shape)} {state_dict[n].dtype}, "
                                 f"not {tuple(t.shape)} {t.dtype}")
        st = state_dict[STATE_KEY]
        if st.shape != self.state.shape or st.dtype != torch.float64:
            raise ValueError(f"ModelEMA.load_state_dict: {STATE_KEY!r} is not {EMA_LEN} doubles")
        for n, t in live.items():
            t.copy_(state_dict[n])
        self.state.copy_(st)
        return self

    def sync_host(self):
        st = self.state.cpu().numpy()
        return dict(decay=float(st[EMA["DECAY"]]), warmup=bool(st[EMA["WARMUP"]]), updates=int(st[EMA["UPDATES"]]),
                    last=float(st[EMA["LAST"]]), weight=float(st[EMA["WEIGHT"]]), active=bool(st[EMA["ACTIVE"]]))
