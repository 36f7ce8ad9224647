"""The Trainer under data parallel.  `DataParallelRun(trainer, spec)` exists only when `data_parallel` is given.

`Trainer(..., data_parallel=...)` (keyword-only): None / False = one process, unchanged; True, a dict of
`umi.ddp.GradReducer` arguments (which may also hold `check_replicas`, default True), or a ready GradReducer = one run over the
ranks of a process group (one process per GPU; `dict(world_size=1)` needs no group).  The reducer is built at the start of
train() and closed by it if it built it; `data_parallel` with a user-set `grad_sync` raises ValueError, True without an
initialised process group RuntimeError, unequal `len(dataloader['train'])` over the ranks ValueError on every rank before the
first step.  Covers singe_train and multi_task_train (multi_task_trainRatio raises NotImplementedError).  Step: backward,
`reducer.sync()`, `optimizer.step()`; with graph=True and more than one rank the graph holds forward + loss + backward captured in
the reducer's deferred mode, and `reducer.flush()` + `optimizer.step()` follow each replay (under `global_batch=True` the step
stays eager, one log line says why: collectives are not captured).  Once per phase the ranks all-reduce one float64 vector (loss
sum, score sum, step count, per-task sums): epoch figures are global sums over global step counts -- validation shards may be
unequal or empty --, every rank holds the same floats and takes the same best-model and early-stop decisions.  Validation runs on
rank 0's BatchNorm running statistics (broadcast before the phase; under `global_batch` they agree anyway) and each rank's own
batches (no collective inside a validation step).  Rank 0 alone writes `logs.txt`, checkpoints and `total.png`, prints and shows
the progress bar; `best_model` is kept on every rank, so train() returns the best weights everywhere.  With `check_replicas`
the parameters' device fingerprint (`umi.ddp.check_replicas`) is compared across the ranks after the reducer's broadcast and at
the end of every training phase (buffers included under `global_batch`): one read of the parameters and 8 bytes read back per
epoch; RuntimeError on every rank if they differ.  The Trainer does not reseed: augmentation and dropout seeds are the caller's
business, and the same seed on every rank gives the same masks on every rank.
"""
import torch
import torch.distributed as dist

from . import ddp


class DataParallelRun:
    def __init__(self, trainer, spec):
        # the spec, then -- from begin() to end() -- the umi.ddp.GradReducer, whether begin() built it, the replica check, this
        # rank, and a line for the log
        self.t, self.spec = trainer, spec
        self.reducer, self.own, self.check, self.rank, self.note = None, False, False, 0, None
        self.built = None             # the reducer begin() built, kept for a later train(): captured graphs hold its addresses

    @staticmethod
    def world_of(spec):
        """The world size a `data_parallel` spec asks for; None: that of a process group that is not initialised."""
        if isinstance(spec, dict):
            world, group = spec.get("world_size"), spec.get("group")
        else:
            world, group = getattr(spec, "world", None), getattr(spec, "group", None)
        if world is None and dist.is_available() and dist.is_initialized():
            world = dist.get_world_size(group)
        return world

    def begin(self):
        """Start of train(): argument checks, equal step counts, the reducer (whose constructor broadcasts rank 0's replica), the
        first replica check."""
        t, spec = self.t, self.spec
        if t.grad_sync is not None:
            raise ValueError("Trainer(data_parallel=...) runs the gradient exchange itself; do not set trainer.grad_sync as well")
        if t._ratio_loop():
            raise NotImplementedError("multi_task_trainRatio under data_parallel: its alpha and count-ratio sums are not reduced "
                                      "over the ranks")
        world = self.world_of(spec)
        if isinstance(spec, ddp.GradReducer):
            kw, check, group = None, True, spec.group
        else:
            if spec is not True and not isinstance(spec, dict):
                raise TypeError("data_parallel takes None / False, True, a dict of umi.ddp.GradReducer arguments (plus "
                                f"check_replicas) or a GradReducer, not {spec!r}")
            kw = {} if spec is True else dict(spec)
            check, group = bool(kw.pop("check_replicas", True)), kw.get("group")
            if world is None or (world > 1 and not (dist.is_available() and dist.is_initialized())):
                raise RuntimeError("Trainer(data_parallel=...) over more than one rank needs an initialised process group "
                                   "(torch.distributed.init_process_group, one process per GPU)")
        self.rank = dist.get_rank(group) if world > 1 else 0
        if world > 1:                         # before anything is touched: a rank with fewer steps would leave the others waiting
            mine = torch.tensor([len(t.dataloader['train'])], dtype=torch.int64, device=t._model_device())
            lens = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(lens, mine, group=group)
            lens = [int(v.item()) for v in lens]
            if len(set(lens)) > 1:
                raise ValueError(f"data_parallel needs the same number of training steps on every rank, got {lens} (per rank); "
                                 "use a DistributedSampler with drop_last, or equal shards")
        if kw is None:
            self.reducer, self.own = spec, False
        elif self.built is not None:
            self.reducer, self.own = self.built.reopen(), True
        else:
            self.reducer = self.built = ddp.GradReducer(t.model, **kw)
            self.own = True
        self.check = check and world > 1
        t.grad_sync = self.reducer.sync
        if t.graph and world > 1 and self.reducer.batch_sync is not None:
            self.note = ("data_parallel: graph=True runs eagerly under global_batch=True (the statistics all-reduce of "
                         "every BatchNorm layer and of the loss is a collective, and collectives are not captured)")
        self.verify()

    def verify(self):
        """The replicas still agree, bit for bit (one word per rank); the EMA's tensors included."""
        if self.check:
            ema = self.t._ema
            ddp.check_replicas(self.t.model, self.reducer.group, buffers=self.reducer.batch_sync is not None,
                               extra=() if ema is None else list(ema.tensors().values()))

    def end(self):
        """End of train(), also on an error: hand the model back as it came (a reducer built here is closed, so the
        global-batch switch does not leak into later code)."""
        if self.reducer is None:
            return
        if self.t.grad_sync == self.reducer.sync:
            self.t.grad_sync = None
        if self.own:
            self.reducer.close()
        elif self.reducer.batch_sync is not None:
            ddp.set_active_batch_sync(self.reducer.batch_sync)     # as the caller's reducer had it (validation turns it off)
        self.reducer, self.own = None, False

    def phase(self, train):
        """Before a phase.  Validation: what is validated is what rank 0 saves -- without global_batch the BatchNorm running
        statistics differ per rank, so rank 0's buffers are broadcast; and the loss is each rank's own (the shards may be unequal
        or empty, so no collective may sit inside a validation step), reduced once afterwards."""
        if self.reducer.batch_sync is not None:
            ddp.set_active_batch_sync(self.reducer.batch_sync if train else None)
        elif not train and self.reducer.world > 1:
            with torch.no_grad():
                for b in self.t.model.buffers():
                    dist.broadcast(b, 0, group=self.reducer.group)

    def reduce(self, sums):
        """One all-reduce per phase: the float64 sums (losses, score, step count) of all ranks, so every rank derives the same
        epoch figures and the same model selection and early stop from them."""
        if self.reducer.world == 1:
            return sums
        vec = torch.tensor(sums, dtype=torch.float64, device=self.t._model_device())
        dist.all_reduce(vec, op=dist.ReduceOp.SUM, group=self.reducer.group)
        return vec.tolist()
