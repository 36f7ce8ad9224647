"""Gradient accumulation: one optimizer step over the mean gradient of a WINDOW of micro-batches, summed on the device.

    acc = GradAccumulator(model, steps=4)
    for x, y in loader:
        loss(model(x), y).backward()           # with optimizer.zero_grad() before it: every micro-batch has its own gradient
        if acc.add():                          # two launches on the current stream; capturable into a HIP graph
            optimizer.step()                   # .grad now holds the mean gradient of the window

One add() is umi_grad_accum_pre + umi_grad_accum_multi (include/unetmi.h): the first advances a device block of UMI_ACCUM_LEN
doubles -- how many micro-batches the open window holds, whether this call is its first and its last, and the fp32 factor
(float)(1 / r) --, the second walks every gradient in one launch: the first call of a window MOVES the gradient into its fp32
accumulator (the accumulator is not read, so nobody ever zeroes it), a middle call adds, and the last call writes
(acc + g) * (float)(1 / r) into the gradient itself, so the optimizer, the guard's norm pass, the reducer and the weight average read
what they read without accumulation.  The gradient of a window of r micro-batches is

    float32(1 / r) * (((g1 + g2) + g3) + ... + gr)          in float32, in arrival order

`accumulate_numpy` is that statement in NumPy, `accum_state_update_numpy` the state machine; the device results equal them bit
for bit (where the statement gives a NaN, a NaN: IEEE 754 leaves the payload of a computed NaN to the implementation).  A window of
one launches the pass, which returns before any access: the gradient keeps its bits.  "First" lives in the device block and not in
a kernel argument, so under graph capture one captured micro-step serves every non-final position of a window.

`Trainer(..., accumulate=k)` (keyword-only; None or 1 = off: nothing of this is built, allocated or launched; an int >= 2 = on;
True, 0, negatives and floats raise ValueError).  A window is k consecutive training batches of one epoch; the last window of an
epoch may be shorter and steps with 1 / r of what it saw; a window never spans two epochs.  A micro-step is forward, loss,
zero_grad, backward, add(last=False); the final step is the same with add(last=True) and then grad_sync, optimizer.step() and the
EMA update.  `train_step(inputs, labels, last=None)`: None follows the Trainer's own window count (the epoch loop passes True for
the last batch of the loader), an explicit True closes the window early.  `iter_num`, both learning-rate rules, Adam's step count,
the guard's `steps` and the EMA's update count all count OPTIMIZER steps; `max_iterations` defaults to
num_epochs * ceil(len(train loader) / k) and `lr_schedule`'s default follows it; epoch losses stay the mean over batches.  One line
in `logs.txt` per run gives k and the optimizer steps per epoch.  BatchNorm statistics and running averages are per MICRO-batch,
as with any accumulation loop: k micro-batches of B images are not one batch of k * B images for a model with BatchNorm (they are
for GroupNorm / LayerNorm models).  Dropout counters advance per forward.
Graph mode holds at most two graphs per batch shape: the micro-step (without the optimizer) and the final step (with it), each by
the existing rule -- first occurrence eager, second captured.  The ragged last batch of an epoch is always a final step, so the
optimizer's descriptor table is captured at most twice.
The guard decides nothing new: a non-finite value of any micro-batch reaches the sum and the window's one guarded step skips;
clipping uses the norm of the mean gradient; the dynamic loss scale is written by the guarded step alone, so it is constant inside
a window and moves once per window.
Data parallel: one set of bucket collectives per optimizer step.  Every step runs with the reducer in deferred mode (the tape fills
the buckets and launches nothing), add() works on the bucket views, and `reducer.flush()` and the step follow the final add().  This
gives up the overlap of the collectives with the final backward pass.  `global_batch=True` raises NotImplementedError, and so does
the count-ratio loop ('multi_task_loss_ratio').
Run state: nothing new is stored.  Windows end with the epoch, so the run-state file is always written with the window closed;
`snapshot_run_state()` inside an open window raises RuntimeError, `restore_run_state()` closes the window (`reset()`), and a file
written under another k is caught by the `max_iterations` check.
"""
import numpy as np
import torch

from . import lib as L

# the state block of include/unetmi.h: ACCUM["COUNT"] etc. = the UMI_ACCUM_* slot indices
ACCUM_LEN = L.UMI_ACCUM_LEN
ACCUM = {k[len("UMI_ACCUM_"):]: v for k, v in L.ENUMS.items() if k.startswith("UMI_ACCUM_") and k != "UMI_ACCUM_LEN"}


def accum_state_update_numpy(state, last):
    """The arithmetic of umi_grad_accum_pre in float64: `state` (the UMI_ACCUM_LEN doubles of a block) after one more call.
    Returns a new array."""
    st = np.array(state, dtype=np.float64)
    j = st[ACCUM["COUNT"]]
    st[ACCUM["FIRST"]] = 1.0 if j == 0.0 else 0.0
    st[ACCUM["LAST"]] = 1.0 if last else 0.0
    st[ACCUM["SCALE"]] = np.float64(np.float32(np.float64(1.0) / (j + np.float64(1.0))))
    st[ACCUM["COUNT"]] = 0.0 if last else j + 1.0
    st[ACCUM["MICRO"]] += 1.0
    st[ACCUM["WINDOWS"]] += 1.0 if last else 0.0
    return st


def accumulate_numpy(grads, r=None):
    """The gradient of a window: float32(1 / r) * (((g1 + g2) + g3) + ... + gr) in float32, in arrival order, r = len(grads)
    unless given.  A window of one returns the input's bits (a copy).  Returns a new float32 array."""
    grads = [np.asarray(g, dtype=np.float32) for g in grads]
    r = len(grads) if r is None else int(r)
    if r < 1 or r != len(grads):
        raise ValueError(f"accumulate_numpy: a window of {r} micro-batches over {len(grads)} gradients")
    if r == 1:
        return grads[0].copy()
    with np.errstate(all="ignore"):
        acc = grads[0]
        for g in grads[1:]:
            acc = acc + g
        return acc * np.float32(np.float64(1.0) / np.float64(r))


class GradAccumulator:
    """fp32 accumulators for the gradients of the parameters of `model_or_params` that require one (a module, or an iterable
    of parameters), closed every `steps` calls.

        add(last=None)   after backward(): this micro-batch's gradients into the window.  `last` None = "the `steps`-th call of
                         the window"; True closes the window now: every gradient then holds the window's mean.  Returns whether
                         the window closed.  Reads each parameter's current `.grad`, or -- where the model has a gradient sink
                         (`umi.ddp.GradReducer`) whose buckets the backward pass has just filled -- its bucket view.
                         Capturable: the accumulators, the state block, the descriptor tables and their staging buffers are
                         allocated by the first eager add() (the warm-up step), never inside a capture; an eager step and each
                         captured graph get their own table (micro and final calls keep separate ones, so one micro-step graph
                         and two final-step graphs fit the two staging buffers of a table)
        position         host count of the open window (0: closed)
        note(last)       a replayed graph ran add(last) on the device: the host count follows
        reset()          host count and the device COUNT back to 0 (an open window is dropped)
        read()           dict(count, windows, micro) of the device block; one synchronisation

    The set of parameters that have a gradient must not change inside a window (RuntimeError).  CPU tensors and gradients that are
    not fp32 take a torch composite with the same arithmetic order (add in arrival order, then mul_(1 / r))."""

    def __init__(self, model_or_params, steps):
        if isinstance(steps, bool) or not isinstance(steps, int) or steps < 1:
            raise ValueError(f"GradAccumulator: steps must be a positive int, not {steps!r}")
        self.model = model_or_params if isinstance(model_or_params, torch.nn.Module) else None
        params = model_or_params.parameters() if self.model is not None else model_or_params
        self.params = [p for p in params if p.requires_grad]
        devs = {p.device for p in self.params}
        if len(devs) > 1:
            raise ValueError(f"GradAccumulator: the parameters live on several devices ({sorted(map(str, devs))})")
        self.device = devs.pop() if devs else torch.device("cpu")
        self.cuda = self.device.type == "cuda"
        if self.cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("umi.accum.GradAccumulator: built inside a HIP-graph capture; build it before the warm-up step")
        self.steps, self.position = steps, 0
        self.state, self._host = None, None                   # device block and its pinned source (CPU: a NumPy block)
        self.arena, self.accs = None, None                    # one flat fp32 arena; per parameter a view into its slot
        self._tables, self._live = {}, None                   # descriptor tables; the parameters of the open window

    # ---- allocation (first use, never inside a capture) ----------------------------------------------------------------------
    def _device_state(self):
        if self.state is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("umi.accum.GradAccumulator: first add() inside a HIP-graph capture; run a warm-up step first")
            from . import ops
            self._host = torch.zeros(ACCUM_LEN, dtype=torch.float64).pin_memory()
            self.state = torch.empty(ACCUM_LEN, dtype=torch.float64, device=self.device)
            L.call("umi_table_upload", self._host.data_ptr(), self.state.data_ptr(), ACCUM_LEN * 8, ops._stream())
            torch.cuda.current_stream().synchronize()
        return self.state

    def _accumulators(self, grads):
        """One arena, a 16-byte aligned slot of n + 3 (rounded up to whole quads) floats per parameter.  The accumulator is the
        view into its slot that shares the gradient's offset into a 16-byte line (bucket views of a reducer start anywhere), so
        the kernel takes its 16-byte walk."""
        if self.accs is None:
            if self.cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("umi.accum.GradAccumulator: first add() inside a HIP-graph capture; run a warm-up step first")
            offs, total = [], 0
            for p in self.params:
                offs.append(total)
                total += (p.numel() + 3 + 3) // 4 * 4
            self.arena = torch.empty(max(total, 4), dtype=torch.float32, device=self.device)
            self.accs = []
            for p, g, off in zip(self.params, grads, offs):
                lead = 0 if g is None or g.dtype != torch.float32 else (g.data_ptr() % 16) // 4
                self.accs.append(self.arena[off + lead:off + lead + p.numel()].view(p.shape))
        return self.accs

    # ---- one micro-batch -----------------------------------------------------------------------------------------------------
    def _grads(self):
        sink = getattr(self.model, "_umi_grad_sink", None) if self.model is not None else None
        if sink is not None and sink._marked:                 # the tape has just filled the buckets (deferred mode)
            return [sink.buffer_for(p) if sink.buffer_for(p) is not None else p.grad for p in self.params]
        return [p.grad for p in self.params]

    @torch.no_grad()
    def add(self, last=None):
        last = self.position + 1 >= self.steps if last is None else bool(last)
        grads = self._grads()
        live = tuple(i for i, g in enumerate(grads) if g is not None)
        if self.position and live != self._live:
            raise RuntimeError("umi.accum.GradAccumulator: the set of parameters that have a gradient changed inside a window "
                               f"({len(self._live)} at its first micro-batch, {len(live)} now)")
        self._live = live
        for i in live:
            g = grads[i]
            if g.is_sparse or not g.is_contiguous():
                raise RuntimeError("umi.accum.GradAccumulator: dense contiguous gradients only (the mean is written in place)")
        accs = self._accumulators(grads)
        fused = [i for i in live if self.cuda and grads[i].dtype == torch.float32]
        rest = [i for i in live if not (self.cuda and grads[i].dtype == torch.float32)]
        if rest:
            if self.cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("umi.accum.GradAccumulator: gradients that are not fp32 cannot be accumulated inside a HIP-graph "
                                   "capture (their factor is a host value)")
            first, r = self.position == 0, self.position + 1
            for i in rest:
                g = grads[i]
                a = accs[i] if g.dtype == torch.float32 else self._wide(i, g)
                if first and last:
                    continue
                if first:
                    a.copy_(g)
                elif not last:
                    a.add_(g)
                else:
                    g.copy_(a.add(g).mul_(1.0 / r))                # the accumulator is not written
        if self.cuda:
            from . import ops, optim
            with torch.cuda.device(self.device):
                st = self._device_state().data_ptr()
                cap = torch.cuda.is_current_stream_capturing()
                rows = [(0, grads[i].data_ptr(), accs[i].data_ptr(), 0, grads[i].numel()) for i in fused]
                ptr, n, blocks = optim._table(self._tables, ("accum", last), cap, rows) if rows else (None, 0, 0)
                stream = ops._stream()
                L.call("umi_grad_accum_pre", st, int(last), stream)
                L.call("umi_grad_accum_multi", ptr, n, blocks, st, stream)
        else:
            if self.state is None:
                self.state = np.zeros(ACCUM_LEN, dtype=np.float64)
            self.state = accum_state_update_numpy(self.state, last)
        self.note(last)
        return last

    def _wide(self, i, g):
        """Accumulator of a gradient that is not fp32 (the float64 CPU oracle): its own tensor, in the gradient's dtype."""
        wide = self.__dict__.setdefault("_wide_accs", {})
        a = wide.get(i)
        if a is None or a.dtype != g.dtype or a.shape != g.shape:
            a = wide[i] = torch.empty_like(g, memory_format=torch.contiguous_format)
        return a

    def note(self, last):
        self.position = 0 if last else self.position + 1

    def reset(self):
        self.position, self._live = 0, None
        if self.state is None:
            return self
        if not self.cuda:
            self.state[ACCUM["COUNT"]] = 0.0
            return self
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("umi.accum.GradAccumulator: reset() cannot run inside a HIP-graph capture")
        self.state[ACCUM["COUNT"]] = 0.0                       # in place: captured graphs hold the block's address
        return self

    def read(self):
        st = np.zeros(ACCUM_LEN) if self.state is None else self.state if not self.cuda else self.state.cpu().numpy()
        return dict(count=int(st[ACCUM["COUNT"]]), windows=int(st[ACCUM["WINDOWS"]]), micro=int(st[ACCUM["MICRO"]]))
