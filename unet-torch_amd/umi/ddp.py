"""Data-parallel gradient exchange: one process per GPU, bucketed sum-all-reduce over RCCL/xGMI.

The reference has no multi-GPU path; this is new functionality with standard
DDP semantics: every rank holds a full replica, the global batch is split evenly, gradients are
averaged.  By default BatchNorm statistics and the Dice sums stay per-replica, as in torch DDP -- which makes N ranks
x B/N images a different model from one process on the B images.  `GradReducer(..., global_batch=True)` closes that gap:

  * training-mode BatchNorm layers (all go through Tape.conv_bn) normalise with the statistics of the WHOLE batch: each
    rank reduces its partial rows to float64 sums, ONE all-reduce per layer carries [sums | sums of squares | pixel count],
    and the finalize kernel runs from the global sums and the global count (running statistics included);
  * their backward adds the two sums sum(dz), sum(dz * xhat) over the ranks (carried as float64) and applies them with the global
    count.  The gradients of gamma and beta that go into the buckets stay the LOCAL sums: the bucket all-reduce with its
    1 / world already turns them into the gradient of the global loss;
  * `loss.calc_loss(..., 'dice_bce_mc')` becomes the loss of the whole batch (global Dice sums and pixel count), reported on
    every rank, and its backward is world x the gradient of that loss w.r.t. this rank's logits, so the AVERAGED parameter
    gradient is the gradient of the global loss.

With the switch on, equal shards are required (a rank whose count is not 1 / world of the total raises), the batch-coupled
losses 'Tversky', 'TopK' and 'BCE_HEM' raise NotImplementedError instead of silently staying per-replica, and a sync
collective cannot be captured into a HIP graph: deferred / GraphedStep mode raises RuntimeError (a group of one launches no
collective and is exempt).  Eval mode is untouched.  The switch is per process: the loss has no model argument, so it asks
`active_batch_sync()`; `GradReducer.close()` turns it off again.  Cost: 2 small launches more per BatchNorm layer forward, a
launch and a collective more per layer each way when world > 1; the latency of those collectives over xGMI is unmeasured
on hardware.

Overlap: the tape's hand-written backward (umi/graph.py) writes each parameter gradient straight
into its slot of a flat fp32 bucket and tells the reducer; buckets are filled in reverse execution
order (outc, up4, ... inc), and a bucket's `all_reduce(async_op=True)` is issued the moment its last
gradient kernel has been enqueued.  torch's RCCL process group runs it on its own HIP stream, so
the decoder buckets travel over xGMI while the encoder backward is still computing; `finish()`
makes the compute stream wait for the outstanding collectives (no host sync).  The 1/world factor
is folded into the wgrad kernels' output scale, so the collective is a plain SUM.

`Trainer(..., data_parallel=...)` (Trainer.py) drives all of this behind the reference's Trainer API.  The scheme rests on the
replicas being bit-identical: `check_replicas(model)` folds the parameters into one 64-bit word on the device
(`fingerprint`, umi_fingerprint_multi; `fingerprint_numpy` is the definition) and compares the words of the ranks.

`sync()` also supports models that do not use the tape (e.g. the CPU oracle in the gloo tests):
it then reduces `p.grad` through the same buckets after backward.
"""
import torch
import torch.distributed as dist


class _Bucket:
    __slots__ = ("flat", "views", "pending", "work", "params")

    def __init__(self):
        self.flat, self.views, self.pending, self.work, self.params = None, {}, 0, None, []


_ACTIVE_SYNC = None


def active_batch_sync():
    """The BatchSync of the GradReducer(global_batch=True) of this process, or None."""
    return _ACTIVE_SYNC


def set_active_batch_sync(sync):
    """Which BatchSync loss.calc_loss uses (None: per-replica losses).  GradReducer(global_batch=True) and close() call this; a
    process that holds several reducers (an A/B measurement) switches by hand."""
    global _ACTIVE_SYNC
    _ACTIVE_SYNC = sync


class BatchSync:
    """The collectives of global-batch mode: the hook Tape.conv_bn reads from the model (`_umi_batch_sync`) and
    loss.calc_loss from active_batch_sync().  A group of one launches nothing."""

    def __init__(self, reducer):
        self.reducer, self.world, self.group = reducer, reducer.world, reducer.group

    def all_reduce(self, vec):
        """In-place SUM of a small statistics vector over the group."""
        if self.world == 1:
            return vec
        if self.reducer.deferred or (vec.is_cuda and torch.cuda.is_current_stream_capturing()):
            raise RuntimeError("global_batch: a statistics all-reduce cannot run in deferred / GraphedStep mode (collectives are "
                               "not captured into a HIP graph); use the eager step with global_batch=True")
        dist.all_reduce(vec, op=dist.ReduceOp.SUM, group=self.group)
        return vec

    def check_count(self, total, local):
        """Equal shards only: `total` (the all-reduced count) must be world x this rank's count.  Returns the global count."""
        want = self.world * int(local)
        if self.world > 1:
            got = float(total)                                     # one host read
            if got != float(want):
                raise RuntimeError(f"global_batch needs equal shards: this rank holds {int(local)} of {got:.0f} rows, "
                                   f"not 1/{self.world} of them")
        return want

    def reduce_counted(self, vec, local, tape=None):
        """All-reduce [sums ... | count] in place; returns the global count.  The count is read back (a host sync) for the first
        layer of a tape only: every layer of one forward sees the same split of the batch."""
        self.all_reduce(vec)
        if tape is not None and tape._shards_checked:
            return self.world * int(local)
        if tape is not None:
            tape._shards_checked = True
        return self.check_count(vec[-1] if self.world > 1 else None, local)

    def reduce_bn_bwd(self, sum_dz, sum_dzx, local):
        """The group's (sum dz, sum dz * xhat, count) for stage 3 of a BatchNorm backward.  The inputs are left alone (they are
        the LOCAL gradients of beta and gamma); the sums travel as float64."""
        if self.world == 1:
            return sum_dz, sum_dzx, int(local)
        C = sum_dz.numel()
        g = torch.cat([sum_dz.reshape(-1), sum_dzx.reshape(-1)]).double()
        g = self.all_reduce(g).float()
        return g[:C], g[C:], self.world * int(local)


class GradReducer:
    def __init__(self, model, world_size=None, bucket_mb=32.0, group=None, global_batch=False):
        self.group = group
        self.world = world_size if world_size is not None else dist.get_world_size(group)
        params = [p for p in model.parameters() if p.requires_grad]
        self.params = params
        cap = int(bucket_mb * (1 << 20)) // 4
        self.buckets, cur, n = [], _Bucket(), 0
        for p in reversed(params):                      # reverse execution order
            if n and n + p.numel() > cap:
                self._seal(cur, n)
                cur, n = _Bucket(), 0
            cur.params.append(p)
            n += p.numel()
        if n:
            self._seal(cur, n)
        self.where = {id(p): b for b in self.buckets for p in b.params}
        self.grad_scale = 1.0 / self.world              # folded into the wgrad output scale by the tape
        self._marked = False
        # deferred mode (`flush()`): the tape only fills the buckets and launches nothing, so forward + backward can be
        # captured into a HIP graph (umi.graphs.GraphedStep); the collectives are issued after the replay.  Trades the
        # overlap with the backward pass (~0.1 ms per 16 MB bucket over xGMI) for a step whose ~350 launches no longer
        # depend on the host
        self.deferred = False
        self.reset()
        model._umi_grad_sink = self
        self.model = model
        self.batch_sync = None
        if global_batch:
            self.batch_sync = model._umi_batch_sync = BatchSync(self)
            set_active_batch_sync(self.batch_sync)
        if self.world > 1:
            self.broadcast_parameters(model)

    def close(self):
        """Detach from the model (and turn global-batch mode off for this process)."""
        for name, mine in (("_umi_grad_sink", self), ("_umi_batch_sync", self.batch_sync)):
            if mine is not None and self.model.__dict__.get(name) is mine:
                delattr(self.model, name)
        if self.batch_sync is not None and _ACTIVE_SYNC is self.batch_sync:
            set_active_batch_sync(None)

    def reopen(self):
        """Attach again after close(), with the same buckets: gradient addresses a captured HIP graph holds stay valid (a
        Trainer whose train() is called a second time).  Rank 0's replica is broadcast again, as at construction."""
        self.model._umi_grad_sink = self
        if self.batch_sync is not None:
            self.model._umi_batch_sync = self.batch_sync
            set_active_batch_sync(self.batch_sync)
        self.deferred = False
        self.reset()
        if self.world > 1:
            self.broadcast_parameters(self.model)
        return self

    def _seal(self, b, numel):
        p0 = b.params[0]
        b.flat = torch.zeros(numel, dtype=torch.float32, device=p0.device)
        off = 0
        for p in b.params:
            b.views[id(p)] = b.flat[off:off + p.numel()].view(p.shape)
            off += p.numel()
        self.buckets.append(b)

    def broadcast_parameters(self, model):
        """Identical replicas: rank 0's parameters and buffers win (as torch DDP does at construction)."""
        with torch.no_grad():
            for t in list(model.parameters()) + list(model.buffers()):
                dist.broadcast(t, 0, group=self.group)

    def reset(self):
        for b in self.buckets:
            b.pending, b.work = len(b.params), None
        self._marked = False

    # ---- tape-facing API -------------------------------------------------------------------
    def buffer_for(self, p):
        b = self.where.get(id(p))
        return None if b is None else b.views[id(p)]

    def mark_ready(self, p):
        b = self.where.get(id(p))
        if b is None:
            return
        self._marked = True
        b.pending -= 1
        if b.pending == 0:
            self._launch(b)

    def _launch(self, b):
        if self.deferred:
            return
        if self.world > 1 and b.work is None:
            b.work = dist.all_reduce(b.flat, op=dist.ReduceOp.SUM, group=self.group, async_op=True)

    def flush(self):
        """Deferred mode, after the (replayed) backward filled the buckets: all-reduce them, make the stream wait, and point
        every .grad at its bucket slot (autograd left copies of the un-reduced values there)."""
        for b in self.buckets:
            if self.world > 1:
                # one collective at a time, in bucket order: RCCL runs them back to back on its stream either way (the call
                # returns once enqueued and makes the compute stream wait); several concurrent 32 MB gloo all-reduces, as used
                # by the one-GPU rehearsal, take seconds
                dist.all_reduce(b.flat, op=dist.ReduceOp.SUM, group=self.group)
            for p in b.params:
                p.grad = b.views[id(p)]
        self.reset()

    def finish(self):
        """Called at the end of the tape backward: flush stragglers, make the stream wait."""
        if self.deferred:
            return
        for b in self.buckets:
            if b.pending > 0 and b.pending < len(b.params):
                self._launch(b)                         # some parameter of this bucket got no gradient
            if b.work is not None:
                b.work.wait()
                b.work = None

    # ---- step-facing API --------------------------------------------------------------------
    def sync(self):
        """After loss.backward(): gradients are averaged when this returns (stream-ordered)."""
        if self._marked:
            self.finish()
            # autograd stores a COPY of each gradient (AccumulateGrad clones a tensor it cannot steal).  The tape's backward
            # ends with finish(), so that copy is taken after the all-reduce and already holds the reduced values; .grad is
            # re-pointed at the bucket slots anyway: no copy, and the slots are stable, so the fused optimizer's pointer table
            # never changes
            for b in self.buckets:
                for p in b.params:
                    if p.grad is not None:
                        p.grad = b.views[id(p)]
            self.reset()
            return
        # generic path: the model's backward did not go through the tape
        for b in self.buckets:
            for p in b.params:
                v = b.views[id(p)]
                if p.grad is None:
                    v.zero_()
                else:
                    v.copy_(p.grad)
            b.flat.mul_(self.grad_scale)
            self._launch(b)
        for b in self.buckets:
            if b.work is not None:
                b.work.wait()
                b.work = None
            for p in b.params:
                if p.grad is not None:
                    p.grad.copy_(b.views[id(p)])
        self.reset()


# ---- replica fingerprint ---------------------------------------------------------------------------------------------------
# The scheme rests on every rank holding bit-identical parameters.  fingerprint() folds a list of tensors into one 64-bit word
# (umi_fingerprint_multi, include/unetmi.h: one read of the tensors, 8 bytes read back); check_replicas() compares the words
# of the ranks.  fingerprint_numpy() is the definition, in NumPy.
_FP_G = 0x9E3779B97F4A7C15
_FP_MASK = (1 << 64) - 1


def _fp_mix(z):
    """mix() of include/unetmi.h on a Python int (mod 2^64)."""
    z &= _FP_MASK
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & _FP_MASK
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & _FP_MASK
    return z ^ (z >> 31)


def _fp_words(a):
    import numpy as np
    a = np.ascontiguousarray(a)
    if a.nbytes % 4:
        raise ValueError(f"fingerprint: a tensor of {a.nbytes} bytes is not a whole number of 32-bit words")
    return a.reshape(-1).view(np.uint8).view(np.uint32)


def fingerprint_numpy(arrays, chunk=1 << 22):
    """F = sum_t mix(H_t + G (t + 1)),  H_t = sum_i mix(w_i + G (i + 1)) over the 32-bit words of array t; all mod 2^64."""
    import numpy as np
    G = np.uint64(_FP_G)
    F = 0
    with np.errstate(over="ignore"):
        for t, a in enumerate(arrays):
            w, H = _fp_words(a), 0
            for i0 in range(0, w.size, chunk):
                part = w[i0:i0 + chunk].astype(np.uint64)
                z = part + G * np.arange(i0 + 1, i0 + 1 + part.size, dtype=np.uint64)
                z ^= z >> np.uint64(30)
                z *= np.uint64(0xBF58476D1CE4E5B9)
                z ^= z >> np.uint64(27)
                z *= np.uint64(0x94D049BB133111EB)
                z ^= z >> np.uint64(31)
                H = (H + int(z.sum(dtype=np.uint64))) & _FP_MASK
            F = (F + _fp_mix(H + _FP_G * (t + 1))) & _FP_MASK
    return F


class FingerprintPlan:
    """The launch of umi_fingerprint_multi over a fixed list of device tensors: descriptor table, scratch and result word are
    allocated once; launch() only enqueues (two kernels on the current stream), word() reads the 8 bytes back."""

    def __init__(self, tensors):
        import numpy as np
        from . import lib as L, ops
        if not tensors or not all(t.is_cuda and t.device == tensors[0].device for t in tensors):
            raise ValueError("fingerprint: needs device tensors that live on one device")
        self.tensors = [t.detach().contiguous() for t in tensors]                 # (a copy of a non-contiguous one is kept alive)
        blk = L.fn("umi_optim_block_elems")()
        arr = np.zeros(len(self.tensors), dtype=ops.OPTIM_DESC)
        b0 = 0
        for i, t in enumerate(self.tensors):
            nbytes = t.numel() * t.element_size()
            if nbytes % 4:
                raise ValueError(f"fingerprint: a tensor of {nbytes} bytes is not a whole number of 32-bit words")
            arr[i] = (t.data_ptr(), 0, 0, 0, nbytes // 4, b0, 0)
            b0 += (nbytes // 4 + blk - 1) // blk
        self.device, self.blocks, self.bytes = self.tensors[0].device, b0, 4 * int(arr["n"].sum())
        with torch.cuda.device(self.device):
            self.table = torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).to(self.device)
            self.ws = torch.empty(max(b0, 1), dtype=torch.int64, device=self.device)
            self.out = torch.empty(1, dtype=torch.int64, device=self.device)

    def launch(self):
        from . import lib as L, ops
        with torch.cuda.device(self.device):
            L.call("umi_fingerprint_multi", self.table.data_ptr(), len(self.tensors), self.blocks, self.ws.data_ptr(),
                   self.ws.numel() * 8, self.out.data_ptr(), ops._stream())
        return self

    def word(self):
        return int(self.out.item()) & _FP_MASK


def fingerprint(tensors):
    """The fingerprint of a list of tensors: device tensors through the HIP kernel (all on one device), CPU tensors through the
    NumPy statement.  The same bits either way."""
    tensors = list(tensors)
    if not any(t.is_cuda for t in tensors):
        return fingerprint_numpy([t.detach().contiguous().numpy() for t in tensors])
    return FingerprintPlan(tensors).launch().word()


def check_replicas(model, group=None, buffers=False, extra=()):
    """Every rank fingerprints its parameters (and buffers, when they are meant to be identical too: global_batch; and `extra`,
    further tensors that must agree, such as the shadows of a weight average), the words are all-gathered, and EVERY rank raises
    RuntimeError when they differ.  Returns this rank's word."""
    tensors = list(model.parameters()) + (list(model.buffers()) if buffers else []) + list(extra)
    word = fingerprint(tensors)
    world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
    if world == 1:
        return word
    dev = tensors[0].device if tensors else torch.device("cpu")
    mine = torch.tensor([word - (1 << 64) if word >> 63 else word], dtype=torch.int64, device=dev)
    got = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(got, mine, group=group)
    words = [int(g.item()) & _FP_MASK for g in got]
    if len(set(words)) > 1:
        raise RuntimeError("data parallel: the replicas differ (fingerprint of the parameters%s per rank: %s)"
                           % (" and buffers" if buffers else "", ", ".join(f"{r}: {w:#018x}" for r, w in enumerate(words))))
    return word
