"""Fused multi-tensor optimizers behind the torch.optim façade.

`SGD` / `Adam` subclass `torch.optim.SGD` / `torch.optim.Adam`: same constructor, `param_groups`, `state` and
`state_dict()` layout (`momentum_buffer`; `step` / `exp_avg` / `exp_avg_sq`), so the reference's call sites
(train.py:341-347 builds the optimizer, Trainer.py:719-725 drives it and rewrites `param_group['lr']` for the poly
schedule) work unchanged.  `step()` updates every parameter of a group with ONE libunetmi launch
(umi_optim_sgd_multi / umi_optim_adam_multi) that follows torch's operation order, instead of torch's 4-10 foreach
launches per group.

`AdamW` subclasses `torch.optim.AdamW` the same way and shares `Adam.step`: decoupled weight decay (umi_optim_adamw_multi*), also
what `Adam(..., decoupled_weight_decay=True)` runs.  `device_schedule(schedule=...)` puts a linear warm-up + cosine / poly /
constant decay into the device block (`schedule_lr` is the rule on the host); `decay_groups` splits a model's parameters into the
decayed and the not decayed group.

`GradGuard` + `optimizer.grad_guard(guard)`: a non-finite check that skips the step, global gradient-norm clipping and a
dynamic loss scale, decided on the device inside the step (so a captured HIP graph keeps deciding).

Parameters must live on the MI355X; there is no CPU path here (the CPU oracle uses torch.optim itself).
"""
import math

import numpy as np
import torch

from . import lib as L
from . import ops


def _bump(p):
    # the kernels write through raw pointers: tell autograd (and ops.PackCache) that the parameter changed
    torch.autograd.graph.increment_version(p)


class _Table:
    """Device descriptor table of one param group, rebuilt only when a pointer changes.

    The upload is stream-capture safe: the pinned staging buffers and the device buffer are allocated once (outside any
    capture: `umi.graphs.GraphedStep` warms up first) and reused, and the copy is a kernel (`umi_table_upload`) reading the
    device-mapped pinned buffer, i.e. an ordinary kernel node of the graph.  That node re-reads the pinned buffer at every
    replay, so an optimizer that was captured into a graph must not also be stepped eagerly afterwards (GraphedStep owns
    it)."""

    def __init__(self):
        self.key, self.dev, self.blocks, self.n = None, None, 0, 0
        self.host, self.events, self.turn = [None, None], [None, None], 0
        self.captured = set()                            # staging buffers a captured graph replays from

    def _ensure(self, nbytes):
        if self.dev is None or self.dev.numel() < nbytes:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("umi.optim: first optimizer step inside a HIP-graph capture; run a warm-up step first "
                                   "(umi.graphs.GraphedStep does)")
            cap = max(nbytes, 16384)
            self.dev = torch.empty(cap, dtype=torch.uint8, device="cuda")
            self.host = [torch.empty(cap, dtype=torch.uint8).pin_memory() for _ in range(2)]
            self.events = [None, None]

    def get(self, rows):
        key = tuple(rows)
        if key != self.key:
            blk = L.fn("umi_optim_block_elems")()
            arr = np.zeros(len(rows), dtype=ops.OPTIM_DESC)
            b0 = 0
            for i, (p, g, s0, s1, n) in enumerate(rows):
                arr[i] = (p, g, s0, s1, n, b0, 0)
                b0 += (n + blk - 1) // blk
            raw = arr.view(np.uint8).reshape(-1)                 # 48 B per row: a multiple of 16
            self._ensure(raw.size)
            capturing = torch.cuda.is_current_stream_capturing()
            self.turn ^= 1                               # two staging buffers: the previous upload may still be in flight
            if capturing:
                # a captured upload node re-reads ITS staging buffer at every replay: a third capture (a third batch shape)
                # would overwrite the buffer the first graph still replays from, and that graph would step the parameters
                # with another graph's gradient addresses.  Trainer(graph=True) captures two shapes (full and ragged batch).
                if self.turn in self.captured:
                    raise RuntimeError("umi.optim: more than two HIP-graph captures share this optimizer's descriptor table "
                                       "(two staging buffers); use one optimizer per set of captured shapes")
                self.captured.add(self.turn)
            ev = self.events[self.turn]
            if ev is not None and not capturing:
                ev.synchronize()
            self.host[self.turn].numpy()[:raw.size] = raw
            L.call("umi_table_upload", self.host[self.turn].data_ptr(), self.dev.data_ptr(), raw.size, ops._stream())
            if not capturing:
                self.events[self.turn] = torch.cuda.Event()
                self.events[self.turn].record()
            self.key, self.blocks, self.n = key, b0, len(rows)
        return self.dev.data_ptr(), self.n, self.blocks


def _table(tabs, key, cap, rows, also=()):
    """Descriptor table for (key, capturing?).  A step captured into a HIP graph gets its own table: the captured upload node
    re-reads its pinned staging buffer at every replay, so eager steps (other gradient addresses) must not share it.  The
    capture-side buffers are allocated during the eager warm-up step, never inside the capture."""
    if not cap:
        for k in (key,) + tuple(also):
            tabs.setdefault(k + (True,), _Table())._ensure(len(rows) * ops.OPTIM_DESC.itemsize)
    return tabs.setdefault(key + (cap,), _Table()).get(rows)


_HYPER = np.dtype(L.STRUCTS["umi_optim_hyper"])


# the guard block of include/unetmi.h: UMI_GUARD_LEN doubles, GUARD["SCALE"] etc. = the UMI_GUARD_* slot indices
GUARD_LEN = L.UMI_GUARD_LEN
GUARD = {k[len("UMI_GUARD_"):]: v for k, v in L.ENUMS.items() if k.startswith("UMI_GUARD_") and k != "UMI_GUARD_LEN"}


def guard_update_numpy(state, S, K):
    """The arithmetic of umi_grad_guard_finalize in float64: `state` (the UMI_GUARD_LEN doubles of a guard block) after a step
    whose gradients have the sum of squares S and K non-finite elements.  Returns a new array."""
    st = np.array(state, dtype=np.float64)
    d = st[GUARD["SCALE"]]
    with np.errstate(all="ignore"):
        norm = np.sqrt(np.float64(S)) / d
    st[GUARD["NORM"]], st[GUARD["NONFINITE"]] = norm, K
    skip = K > 0
    st[GUARD["SKIP"]] = 1.0 if skip else 0.0
    if not skip:
        clip = np.float64(1.0)
        if st[GUARD["MAX_NORM"]] > 0:
            r = st[GUARD["MAX_NORM"]] / (norm + 1e-6)
            clip = r if r < 1.0 else np.float64(1.0)
        st[GUARD["COEF"]] = clip / d
        st[GUARD["CLIPPED"]] += clip < 1.0
    else:
        st[GUARD["COEF"]] = 0.0
        st[GUARD["SKIPPED"]] += 1
    st[GUARD["STEPS"]] += 1
    if st[GUARD["GROWTH_INTERVAL"]] > 0:                        # torch.amp.GradScaler.update
        if skip:
            d = max(d * st[GUARD["BACKOFF"]], st[GUARD["MIN_SCALE"]])
            st[GUARD["STREAK"]] = 0
        else:
            st[GUARD["STREAK"]] += 1
            if st[GUARD["STREAK"]] >= st[GUARD["GROWTH_INTERVAL"]]:
                d = min(d * st[GUARD["GROWTH"]], st[GUARD["MAX_SCALE"]])
                st[GUARD["STREAK"]] = 0
        st[GUARD["SCALE"]] = d
    return st


class GradGuard:
    """Device-side guard of the optimizer step (include/unetmi.h, "Guarded optimizer step").

        guard = GradGuard(max_norm=1.0, dynamic_scale=True, init_scale=2.0 ** 8)
        optimizer.grad_guard(guard)            # umi.optim.SGD / Adam; before any HIP-graph capture
        guard.attach(model)                    # only needed for a loss scale other than 1: the model's tape applies it

    Every `optimizer.step()` then makes one extra pass over all gradients of all param groups (sum of squares in float64 and a
    count of inf / NaN), and one small kernel decides: a step with a non-finite gradient is SKIPPED (parameters, momentum /
    Adam moments and Adam's step count keep their bits; the learning-rate schedule still advances: it counts batches); otherwise
    the gradients are clipped to the global L2 norm `max_norm` (as torch.nn.utils.clip_grad_norm_, error_if_nonfinite=False)
    and the loss scale divided out.  Unlike torch's in-place clip, `p.grad` is NOT rewritten: the coefficient is applied as the
    update kernel reads the gradient, so `p.grad` after the step still holds what the backward pass produced (times the
    dynamic scale, if one is attached).

    dynamic_scale=True follows torch.amp.GradScaler: the factor d (initially init_scale) is multiplied by backoff_factor after
    a skipped step and by growth_factor after growth_interval clean steps in a row, within [min_scale, max_scale].  It rides on
    top of the static per-shape loss scale of fp16 mode (umi.graph.default_loss_scale): `attach(model)` hands the model's tape
    a device view of d, the tape multiplies the seed gradient by it, parameter gradients leave the tape carrying it, and the
    update removes it.  With dynamic_scale=False d stays at init_scale.

    Under umi.ddp the check runs in step(), i.e. after grad_sync: every rank sees the same reduced gradients and takes the same
    decisions, without any extra communication.

    `read()` synchronises once and returns
        norm, nonfinite   of the LAST step: global gradient norm (loss scale divided out; inf / nan as computed) and the number of
                          non-finite gradient elements
        scale             the factor the NEXT backward pass will use
        steps, skipped, clipped   running totals since the guard was created."""

    def __init__(self, max_norm=None, dynamic_scale=False, init_scale=1.0, growth_interval=2000, growth_factor=2.0,
                 backoff_factor=0.5, min_scale=2.0 ** -24, max_scale=2.0 ** 24):
        if max_norm is not None and not max_norm > 0:
            raise ValueError("GradGuard: max_norm must be positive (None: no clipping)")
        if not (init_scale > 0 and math.isfinite(init_scale)):
            raise ValueError("GradGuard: init_scale must be positive and finite")
        if dynamic_scale and not (growth_interval >= 1 and growth_factor > 1.0 and 0.0 < backoff_factor < 1.0
                                  and 0.0 < min_scale <= max_scale):
            raise ValueError("GradGuard: need growth_interval >= 1, growth_factor > 1, 0 < backoff_factor < 1, "
                             "0 < min_scale <= max_scale")
        st = np.zeros(GUARD_LEN, dtype=np.float64)
        st[GUARD["SCALE"]], st[GUARD["COEF"]] = init_scale, 1.0 / init_scale
        st[GUARD["MAX_NORM"]] = 0.0 if max_norm is None else float(max_norm)
        st[GUARD["GROWTH_INTERVAL"]] = float(growth_interval) if dynamic_scale else 0.0
        st[GUARD["GROWTH"]], st[GUARD["BACKOFF"]] = growth_factor, backoff_factor
        st[GUARD["MIN_SCALE"]], st[GUARD["MAX_SCALE"]] = min_scale, max_scale
        self.initial = st
        self.state, self._host, self._ws = None, None, None

    def _device_state(self):
        """The device block, filled once (umi_table_upload from a pinned copy of the initial values)."""
        if self.state is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("umi.optim.GradGuard: first use inside a HIP-graph capture; run a warm-up step first")
            self._host = torch.empty(GUARD_LEN, dtype=torch.float64).pin_memory()
            self._host.numpy()[:] = self.initial
            self.state = torch.empty(GUARD_LEN, dtype=torch.float64, device="cuda")
            L.call("umi_table_upload", self._host.data_ptr(), self.state.data_ptr(), GUARD_LEN * 8, ops._stream())
            torch.cuda.current_stream().synchronize()
        return self.state

    def _workspace(self, total_blocks):
        """Partials workspace for `total_blocks` rows; allocated outside any capture (the eager warm-up step), like _Table._ensure."""
        need = L.fn("umi_grad_guard_ws_bytes")(total_blocks)
        if self._ws is None or self._ws.numel() * 8 < need:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("umi.optim.GradGuard: the partials workspace must be allocated before a HIP-graph capture; "
                                   "run a warm-up step first (umi.graphs.GraphedStep does)")
            self._ws = torch.empty(max(need // 8, 2048), dtype=torch.float64, device="cuda")
        return self._ws

    def attach(self, model):
        """Hands `model` the dynamic loss-scale factor: tapes built for it from now on multiply the seed gradient by
        (static loss scale) * d and divide input gradients by the same value.  Call before the first step and before any capture."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("umi.optim.GradGuard: attach() cannot run inside a HIP-graph capture")
        model._umi_dyn_scale = self._device_state()[GUARD["SCALE"]]
        return self

    def read(self):
        st = self.initial if self.state is None else self.state.cpu().numpy()
        return dict(norm=float(st[GUARD["NORM"]]), nonfinite=int(st[GUARD["NONFINITE"]]), skipped=int(st[GUARD["SKIPPED"]]),
                    clipped=int(st[GUARD["CLIPPED"]]), steps=int(st[GUARD["STEPS"]]), scale=float(st[GUARD["SCALE"]]))


class _Guarded:
    """Mixin: the guarded form of step() (see GradGuard)."""

    def grad_guard(self, guard):
        """Attach a GradGuard (None detaches).  Must happen before this optimizer's step is captured into a HIP graph: the
        captured launches are the unguarded ones."""
        captured = any(t.captured for t in self.__dict__.get("_umi_tables", {}).values())
        if captured or (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()):
            raise RuntimeError("umi.optim: grad_guard() after (or inside) a HIP-graph capture of this optimizer's step; attach "
                               "the guard before the GraphedStep is built")
        if guard is not None:
            if not isinstance(guard, GradGuard):
                raise TypeError("umi.optim: grad_guard() takes a GradGuard")
            if any(float(g.get("dampening", 0.0)) != 0.0 for g in self.param_groups):
                raise ValueError("umi.optim: a GradGuard needs dampening == 0 (a skipped first step cannot reproduce "
                                 "buf = clone(grad))")
        self._umi_guard = guard
        return self

    @property
    def guard(self):
        return self.__dict__.get("_umi_guard")

    def _guarded_step(self, groups):
        """groups: [(gi, tables, launch)], tables = [(ptr, n_desc, blocks, tag)], launch(table, guard_ptr) issues the update of
        one table.  One partials pass per table into disjoint rows, ONE finalize (the norm is global over all param groups, as
        in torch.nn.utils.clip_grad_norm_), then per group: guarded hyper_pre, guarded updates, poly rule."""
        total = sum(t[2] for _, tables, _ in groups for t in tables)
        if total == 0:
            return
        guard = self._umi_guard
        st = guard._device_state().data_ptr()
        ws = guard._workspace(total)
        stream, off = ops._stream(), 0
        for _, tables, _ in groups:
            for ptr, n, blocks, _ in tables:
                L.call("umi_grad_norm_partials", ptr, n, blocks, off, ws.data_ptr(), ws.numel() * 8, stream)
                off += blocks
        L.call("umi_grad_guard_finalize", ws.data_ptr(), total, st, stream)
        hyper = self.device_hyper
        for gi, tables, launch in groups:
            if not tables:
                continue
            if hyper is not None:
                L.call("umi_optim_hyper_pre_guarded", hyper[gi][0].data_ptr(), int("betas" in self.param_groups[gi]), st, stream)
            for table in tables:
                launch(table, st)
            if hyper is not None:
                self._advance_schedule(gi)


SCHEDULE_KINDS = {k[len("UMI_SCHED_"):].lower(): v for k, v in L.ENUMS.items() if k.startswith("UMI_SCHED_") and v != 0}


def check_schedule(spec, what="schedule", max_iterations=None):
    """A schedule dict -> dict(kind, max_iterations, warmup, power, final_ratio, iter_num), all checked; ValueError otherwise.
    `max_iterations`: the default for a dict that leaves it out or gives None (Trainer: num_epochs * len(train loader))."""
    if not isinstance(spec, dict):
        raise ValueError(f"{what} takes a dict(kind=, max_iterations=, warmup=0, power=0.9, final_ratio=0.0, iter_num=0), "
                         f"not {spec!r}")
    extra = set(spec) - {"kind", "max_iterations", "warmup", "power", "final_ratio", "iter_num"}
    if extra:
        raise ValueError(f"{what}: unknown keys {sorted(extra)}")
    kind = spec.get("kind")
    if kind not in SCHEDULE_KINDS:
        raise ValueError(f"{what}: kind must be one of {sorted(SCHEDULE_KINDS)}, not {kind!r}")
    mx = spec.get("max_iterations")
    mx = max_iterations if mx is None else mx
    out = dict(kind=kind, max_iterations=mx, warmup=spec.get("warmup", 0), power=spec.get("power", 0.9),
               final_ratio=spec.get("final_ratio", 0.0), iter_num=spec.get("iter_num", 0))
    for k, v in out.items():
        if k != "kind" and (isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v)):
            raise ValueError(f"{what}: {k} must be a finite number, not {v!r}")
    if not out["max_iterations"] > 0:
        raise ValueError(f"{what}: max_iterations must be positive, not {out['max_iterations']!r}")
    if out["warmup"] < 0:
        raise ValueError(f"{what}: warmup must not be negative, not {out['warmup']!r}")
    if not 0.0 <= out["final_ratio"] <= 1.0:
        raise ValueError(f"{what}: final_ratio must be in [0, 1], not {out['final_ratio']!r}")
    if not out["power"] > 0:
        raise ValueError(f"{what}: power must be positive, not {out['power']!r}")
    if out["iter_num"] < 0:
        raise ValueError(f"{what}: iter_num must not be negative, not {out['iter_num']!r}")
    return out


def schedule_lr(k, base_lr, kind, max_iterations, warmup=0, power=0.9, final_ratio=0.0):
    """The learning rate of step k (counted from 0) under the warm-up + decay rule of include/unetmi.h
    (umi_optim_hyper_schedule), in Python doubles and in the kernel's operation order:

        lr(k) = base_lr * (w(k) * (final_ratio + (1 - final_ratio) * s(k)))
        w(k)  = min(1, (k + 1) / warmup) if warmup > 0 else 1
        x     = min(k, max_iterations) / max_iterations
        s(k)  = poly: (1 - x) ** power    cosine: 0.5 * (1 + cos(pi * x))    constant: 1"""
    w = min(1.0, (k + 1) / warmup) if warmup > 0 else 1.0
    x = min(k, max_iterations) / max_iterations
    if kind == "poly":
        s = (1.0 - x) ** power
    elif kind == "cosine":
        s = 0.5 * (1.0 + math.cos(math.pi * x))
    elif kind == "constant":
        s = 1.0
    else:
        raise ValueError(f"schedule_lr: kind must be one of {sorted(SCHEDULE_KINDS)}, not {kind!r}")
    return base_lr * (w * (final_ratio + (1.0 - final_ratio) * s))


def decay_groups(model, weight_decay, no_decay_names=("position_embeddings",)):
    """Two param groups over the trainable parameters of `model`, each parameter exactly once: [decayed, not decayed].
    Not decayed (weight_decay=0): parameters with ndim <= 1 (biases; BatchNorm / GroupNorm / LayerNorm scales and shifts) and
    parameters whose name ends in one of `no_decay_names`; every other one gets `weight_decay`."""
    decay, rest, seen = [], [], set()
    for name, p in model.named_parameters():
        if not p.requires_grad or id(p) in seen:
            continue
        seen.add(id(p))
        (rest if p.ndim <= 1 or name.endswith(tuple(no_decay_names)) else decay).append(p)
    return [dict(params=decay, weight_decay=weight_decay), dict(params=rest, weight_decay=0.0)]


class _DeviceHyper:
    """Mixin: learning rate (and Adam's step count) kept in device memory, so that a step captured into a HIP graph keeps
    following the schedule when it is replayed (reference Trainer.py:719-726 rewrites the LR after every step; a captured
    kernel argument would freeze it -- and torch.optim.Adam's bias corrections with it).

        opt.device_schedule()                                          constant LR (Adam: the step count advances on device)
        opt.device_schedule(poly=dict(base_lr=.., max_iterations=.., power=0.9, iter_num=0))
                                                                       + the reference's poly rule, applied by step() itself
        opt.device_schedule(schedule=dict(kind='cosine' | 'poly' | 'constant', max_iterations=.., warmup=0, power=0.9,
                                          final_ratio=0.0, iter_num=0))
                                                                       + linear warm-up and decay (`schedule_lr`), applied by
                                                                       step() itself; each param group's base LR is its own
                                                                       `lr` at this call, and step k runs on rule(k): no lag

    From then on `step()` reads the LR from the device block and ignores later edits of `param_groups[i]['lr']`;
    `sync_host()` copies lr / iteration / Adam step back into `param_groups` and `state` (it synchronises; `state_dict()`
    calls it).  Eager and graph-replayed steps are interchangeable in this mode: nothing step-dependent is a kernel argument."""

    def device_schedule(self, poly=None, schedule=None):
        if poly is not None and schedule is not None:
            raise ValueError("umi.optim: device_schedule() takes poly= or schedule=, not both")
        if schedule is not None:
            schedule = check_schedule(schedule, "device_schedule(schedule=...)")
        return self._build_hyper(poly, schedule, [float(group["lr"]) for group in self.param_groups])

    def _build_hyper(self, poly, schedule, base_lrs):
        """The blocks of device_schedule(); `base_lrs`: the schedule's base LR per param group."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("umi.optim: call device_schedule() before the HIP-graph capture")
        blocks = []
        for group, base in zip(self.param_groups, base_lrs):
            h = np.zeros(1, dtype=_HYPER)
            h["lr"] = float(group["lr"])
            if poly is not None:
                h["base_lr"], h["max_iter"] = float(poly["base_lr"]), float(poly["max_iterations"])
                h["power"], h["iter"] = float(poly.get("power", 0.9)), float(poly.get("iter_num", 0))
            if schedule is not None:
                rule = {k: schedule[k] for k in ("kind", "max_iterations", "warmup", "power", "final_ratio")}
                h["base_lr"], h["max_iter"], h["power"] = base, float(rule["max_iterations"]), float(rule["power"])
                h["iter"], h["kind"] = float(schedule["iter_num"]), SCHEDULE_KINDS[rule["kind"]]
                h["warmup"], h["final_ratio"] = float(rule["warmup"]), float(rule["final_ratio"])
                h["lr"] = schedule_lr(float(schedule["iter_num"]), base, **rule)
            if "betas" in group:
                h["beta1"], h["beta2"] = (float(b) for b in group["betas"])
                steps = {float(self.state[p]["step"]) for p in group["params"] if len(self.state.get(p, {}))}
                if len(steps) > 1:
                    raise RuntimeError("umi.optim: device_schedule() needs one common Adam step count per param group")
                h["adam_t"] = steps.pop() if steps else 0.0
            host = torch.empty(_HYPER.itemsize, dtype=torch.uint8).pin_memory()
            host.numpy()[:] = h.view(np.uint8).reshape(-1)
            dev = torch.empty(_HYPER.itemsize, dtype=torch.uint8, device="cuda")
            L.call("umi_table_upload", host.data_ptr(), dev.data_ptr(), _HYPER.itemsize, ops._stream())
            blocks.append((dev, host))
        torch.cuda.current_stream().synchronize()
        self._umi_hyper, self._umi_poly, self._umi_sched = blocks, poly is not None, schedule
        return self

    @property
    def device_hyper(self):
        return self.__dict__.get("_umi_hyper")

    def _advance_schedule(self, gi):
        """After the update of group `gi` (device block present): the installed learning-rate rule, if any."""
        if self._umi_poly:
            L.call("umi_optim_hyper_poly", self._umi_hyper[gi][0].data_ptr(), ops._stream())
        elif self._umi_sched is not None:
            L.call("umi_optim_hyper_schedule", self._umi_hyper[gi][0].data_ptr(), ops._stream())

    def sync_host(self):
        """Device block -> param_groups[i]['lr'] (and Adam state['step']); returns the list of blocks as numpy records."""
        out = []
        if self.device_hyper is None or torch.cuda.is_current_stream_capturing():
            return out
        for group, (dev, _) in zip(self.param_groups, self._umi_hyper):
            h = dev.cpu().numpy().view(_HYPER)[0]
            group["lr"] = float(h["lr"])
            if "betas" in group:
                for p in group["params"]:
                    st = self.state.get(p)
                    if st is not None and "step" in st:
                        st["step"].fill_(float(h["adam_t"]))
            out.append(h)
        return out

    def push_lr(self):
        """param_groups[i]['lr'] -> the device block's learning rate, written in place (a captured graph holds the block's
        address), so an LR set on the host between steps -- e.g. by a torch lr_scheduler after sync_host() -- is what the next
        eager or replayed step uses."""
        if self.device_hyper is None:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("umi.optim: push_lr() cannot run inside a HIP-graph capture")
        for group, (dev, _) in zip(self.param_groups, self._umi_hyper):
            dev[:8].copy_(torch.tensor([float(group["lr"])], dtype=torch.float64).view(torch.uint8))   # Hyper.lr, offset 0

    def state_dict(self):
        self.sync_host()
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """Loading a state dict rewrites param_groups[i]['lr'] and Adam's step counts on the host; with a device schedule active
        the device block is what step() reads, so it is rebuilt from the loaded values (the poly rule keeps its base_lr /
        max_iterations / power and the ITERATION COUNT of the block: pass iter_num to device_schedule() to resume elsewhere).
        A schedule= rule keeps its settings, each group's base LR and the iteration count of the block likewise, and the
        block's LR is the rule's at that count, not the loaded one: the rule owns the LR."""
        blocks = self.sync_host() if self.device_hyper is not None else []
        super().load_state_dict(state_dict)
        if self.device_hyper is not None:
            if self._umi_sched is not None and len(blocks) == len(self.param_groups):
                self._build_hyper(None, dict(self._umi_sched, iter_num=float(blocks[0]["iter"])),
                                  [float(h["base_lr"]) for h in blocks])
                return
            poly = None
            if self._umi_poly and blocks:
                h = blocks[0]
                poly = dict(base_lr=float(h["base_lr"]), max_iterations=float(h["max_iter"]), power=float(h["power"]),
                            iter_num=float(h["iter"]))
            self.device_schedule(poly=poly)


def _check(p):
    if not p.is_cuda:
        raise RuntimeError("umi.optim: parameters must be on the MI355X (device 'cuda'); use torch.optim on the CPU")
    if p.dtype != torch.float32 or p.grad.dtype != torch.float32 or p.grad.is_sparse:
        raise RuntimeError("umi.optim: dense fp32 parameters and gradients only")
    if not p.is_contiguous():
        raise RuntimeError("umi.optim: parameters must be contiguous")


class SGD(_DeviceHyper, _Guarded, torch.optim.SGD):
    """torch.optim.SGD(lr, momentum, dampening, weight_decay, nesterov) with a single-launch step."""

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        guarded = [] if self.guard is not None else None
        for gi, group in enumerate(self.param_groups):
            if group.get("maximize") or group.get("differentiable"):
                raise NotImplementedError("umi.optim.SGD: maximize / differentiable are not supported")
            mom = float(group["momentum"])
            rows = {True: [], False: []}             # first step of a momentum buffer? -> rows
            touched = []
            for p in group["params"]:
                if p.grad is None:
                    continue
                _check(p)
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                first, buf = False, None
                if mom != 0.0:
                    st = self.state[p]
                    buf = st.get("momentum_buffer")
                    if buf is None:
                        buf = st["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
                        first = True
                rows[first].append((p.data_ptr(), g.data_ptr(), 0 if buf is None else buf.data_ptr(), 0, p.numel()))
                touched.append((p, g))
            tabs = self.__dict__.setdefault("_umi_tables", {})
            cap = torch.cuda.is_current_stream_capturing()       # a captured table-upload node re-reads its own staging buffers
            hyper = self.device_hyper
            if guarded is not None:
                if float(group["dampening"]) != 0.0:
                    raise ValueError("umi.optim.SGD: a GradGuard needs dampening == 0")
                tables = [_table(tabs, (gi, first), cap, rr, also=((gi, False),)) + (first,) for first, rr in rows.items() if rr]

                def launch(table, st, group=group, mom=mom, hp=hyper[gi][0].data_ptr() if hyper is not None else None):
                    ptr, n, blocks, first = table
                    L.call("umi_optim_sgd_multi_guarded", ptr, n, blocks, hp, float(group["lr"]), mom, 0.0,
                           float(group["weight_decay"]), int(bool(group["nesterov"])), int(first), st, ops._stream())
                guarded.append((gi, tables, launch))
                for p, _ in touched:
                    _bump(p)
                continue
            if hyper is not None:
                L.call("umi_optim_hyper_pre", hyper[gi][0].data_ptr(), 0, ops._stream())
            for first, rr in rows.items():
                if not rr:
                    continue
                ptr, n, blocks = _table(tabs, (gi, first), cap, rr, also=((gi, False),))   # the step after a first step
                if hyper is not None:
                    L.call("umi_optim_sgd_multi_dev", ptr, n, blocks, hyper[gi][0].data_ptr(), mom, float(group["dampening"]),
                           float(group["weight_decay"]), int(bool(group["nesterov"])),
                           int(first), ops._stream())
                else:
                    L.call("umi_optim_sgd_multi", ptr, n, blocks, float(group["lr"]), mom, float(group["dampening"]),
                           float(group["weight_decay"]), int(bool(group["nesterov"])), int(first),
                           ops._stream())
            if hyper is not None:
                self._advance_schedule(gi)
            for p, _ in touched:
                _bump(p)
        if guarded:
            self._guarded_step(guarded)
        return loss


class Adam(_DeviceHyper, _Guarded, torch.optim.Adam):
    """torch.optim.Adam(lr, betas, eps, weight_decay) (no amsgrad) with a single-launch step: L2 weight decay, or with
    `decoupled_weight_decay=True` torch's AdamW rule (the umi_optim_adamw_* entry points)."""

    @torch.no_grad()
    def step(self, closure=None):
        me = "umi.optim." + type(self).__name__
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        guarded = [] if self.guard is not None else None
        if guarded is not None and self.device_hyper is None:
            # the host cannot know whether a step was skipped: Adam's step count has to advance on the device
            raise RuntimeError(f"{me}: a guarded step needs the device-side step count; call "
                               "optimizer.device_schedule() first (umi.graphs.GraphedStep(optimizers=[...]) does)")
        for gi, group in enumerate(self.param_groups):
            if group.get("amsgrad") or group.get("maximize") or group.get("differentiable") or group.get("capturable"):
                raise NotImplementedError(f"{me}: amsgrad / maximize / differentiable / capturable are not supported")
            if isinstance(group["lr"], torch.Tensor):
                raise NotImplementedError(f"{me}: tensor learning rates are not supported")
            b1, b2 = (float(b) for b in group["betas"])
            # decoupled: p *= 1 - lr * wd before the update instead of g += wd * p inside it (torch.optim.AdamW)
            decoupled = bool(group.get("decoupled_weight_decay"))
            fam = "umi_optim_adamw_multi" if decoupled else "umi_optim_adam_multi"
            hyper = self.device_hyper
            cap = torch.cuda.is_current_stream_capturing()
            if cap and hyper is None:
                # torch.optim.Adam refuses capture unless capturable=True; here the host-side `step += 1` and the bias
                # corrections baked into kernel arguments would silently repeat step t on every replay
                raise RuntimeError(f"{me}: a captured step needs the device-side step count; call "
                                   "optimizer.device_schedule() before capturing (umi.graphs.GraphedStep(optimizers=[...]) does)")
            by_step = {}
            touched = []
            for p in group["params"]:
                if p.grad is None:
                    continue
                _check(p)
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                st = self.state[p]
                if len(st) == 0:
                    if cap:
                        raise RuntimeError(f"{me}: first step inside a HIP-graph capture; run a warm-up step first")
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)            # host scalar, as torch keeps it
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                if hyper is None:
                    st["step"] += 1
                    t = int(st["step"].item()) if not st["step"].is_cuda else int(st["step"])
                else:
                    t = 0                                # the device block counts; sync_host() refreshes state['step']
                by_step.setdefault(t, []).append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(),
                                                  st["exp_avg_sq"].data_ptr(), p.numel()))
                touched.append((p, g))
            tabs = self.__dict__.setdefault("_umi_tables", {})
            eps, wd = float(group["eps"]), float(group["weight_decay"])
            if guarded is not None:
                tables = [_table(tabs, (gi, slot), cap, rr) + (slot,) for slot, (t, rr) in enumerate(sorted(by_step.items()))]

                def launch(table, st, fam=fam, decoupled=decoupled, b1=b1, b2=b2, eps=eps, wd=wd, hp=hyper[gi][0].data_ptr()):
                    ptr, n, blocks, _ = table
                    host = (0.0, 0.0) if decoupled else (0.0,)         # (lr,) step_size: the block's are used
                    L.call(fam + "_guarded", ptr, n, blocks, hp, *host, b1, b2, 1.0, eps, wd, st, ops._stream())
                guarded.append((gi, tables, launch))
                for p, _ in touched:
                    _bump(p)
                continue
            if hyper is not None and touched:
                L.call("umi_optim_hyper_pre", hyper[gi][0].data_ptr(), 1, ops._stream())
            for slot, (t, rr) in enumerate(sorted(by_step.items())):
                ptr, n, blocks = _table(tabs, (gi, slot), cap, rr)
                if hyper is not None:
                    L.call(fam + "_dev", ptr, n, blocks, hyper[gi][0].data_ptr(), b1, b2, eps, wd, ops._stream())
                    continue
                bc1 = 1.0 - b1 ** t
                bc2 = 1.0 - b2 ** t
                lr = float(group["lr"])
                L.call(fam, ptr, n, blocks, *((lr,) if decoupled else ()), lr / bc1, b1, b2, math.sqrt(bc2), eps, wd,
                       ops._stream())
            if hyper is not None and touched:
                self._advance_schedule(gi)
            for p, _ in touched:
                _bump(p)
        if guarded:
            self._guarded_step(guarded)
        return loss


class AdamW(_DeviceHyper, _Guarded, torch.optim.AdamW):
    """torch.optim.AdamW(lr, betas, eps, weight_decay) (decoupled weight decay, no amsgrad) with a single-launch step: the step
    of `Adam` on the umi_optim_adamw_* entry points.  Same `state_dict()` layout as torch's."""

    step = Adam.step
