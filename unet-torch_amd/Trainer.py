"""Training loop: drop-in for the reference `Trainer.py` on the hot-path model types.

Keeps `Trainer(model, model_type, dtype, device, output_save_dir, dataloaders, batch_size,
optimizer, patience, num_epochs, loss_function, accuracy_metric, lr_scheduler=None,
start_epoch=1)` and `.train()` (reference Trainer.py:12-50, :113-129), and the behaviour of
`singe_train` (Trainer.py:663-829): per-batch order  to(device)/type -> forward -> calc_loss ->
zero_grad -> backward -> step -> poly-LR with the pre-increment `iter_num` (:719-726); model
selection on `val_score < best_val_score` (:752); early stop on `counter > patience` (:768);
files `logs.txt`, `models/{epochN,best,last_epoch}.pt`, `total.png`.

Differences, all host-side: the step body is factored into `train_step` and the running loss is
accumulated on the device and read back once per epoch instead of a `.item()` sync every step
(Trainer.py:727).
`Trainer(..., graph=True)` (keyword-only, or env UMI_TRAINER_GRAPH=1) replays the whole step from a captured HIP graph
(umi.graphs.GraphedStep) when the model runs on the MI355X and the optimizer is a `umi.optim` one: the first step of a batch
shape runs eagerly, the second is captured and replayed, ragged last batches run eagerly.  The poly learning-rate rule
(:722-725) then advances inside the step from a device-resident block (`optimizer.device_schedule`), because a captured
kernel argument would freeze it; `param_groups[i]['lr']` is refreshed from the device when it is printed or saved.
`multi_task_train` (Trainer.py:831-992; model types 'multi_task*' with a plain loss name): two-headed models
(`Model.UNet_multitask`, `VisionTransformerMultitask`), batches `(inputs, (label1, label2))`, both outputs through
`F.relu` (:883-884), loss = loss1 + loss2 (:885-890), model selection on the validation LOSS (:926).
`multi_task_trainRatio` (Trainer.py:1174-1366; loss_function 'multi_task_loss_ratio' on the 'multi_task*' model types): the
same two-headed step with `loss.multi_task_ratio_loss` (per-task MSE of the ReLU'd heads, error r of the per-image count
ratio, loss = (L1 + L2) * (1 + 10 r) from epoch 6 on), and the reference's bookkeeping: alpha = part1 / part2 per epoch, the
per-task epoch losses divided by the step count twice, no validation record, checkpoint or early stop before epoch 6, then
`lr_scheduler.step(0.0)` when a scheduler is given.  The sums are kept on the device and read back once per phase.  In graph
mode the epoch gate is a device flag the loss kernel reads (rewritten in place at the start of each epoch, so the graphs of
the full and the ragged batch serve both gate values), and an LR change made by a scheduler object is written into the device
LR block in place (umi.optim push_lr), so the captured step sees it.
`Trainer(..., batch_transform=tf)` (keyword-only; `umi.augment.TrainTransform` or any callable of its signature): the loaders
then yield RAW batches -- uint8 / float32 HWC (or HW) images and a label map or a tuple of them, as the reference's
`Dataset.__getitem__` reads them before `transform` -- which are moved to the device as they are and transformed there, with
freshly drawn augmentation parameters in the train phase and none in the validation phase, before the step and outside any
captured graph.
`Trainer(..., grad_guard=...)` (keyword-only; True, a dict of `umi.optim.GradGuard` arguments, or a GradGuard): the optimizer
step skips on a non-finite gradient, clips to `max_norm` and follows a dynamic loss scale, decided on the device (eager and
graph mode alike).  Adam then runs on its device schedule in eager mode too (a skipped step must not advance its step count).
One line per epoch goes to `logs.txt`: `Guard on epoch N: skipped S, clipped C, loss scale X` (S and C count that epoch's
steps).  A skipped step's loss still counts in the epoch mean.
`Trainer(..., data_parallel=...)` (keyword-only): None / False = one process, the path above, unchanged; True, a dict of
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
`Trainer(..., val_batch=k)` (keyword-only, after `data_parallel`): None = the validation loop above, one `eval_step` per loader
item, untouched; an int k >= 1 = in singe_train's validation phase (multi_task_train included) loader items go through
`_to_device(train=False)` one by one as before (`batch_transform` included) and are gathered into groups of up to k CONSECUTIVE
items of EQUAL shapes -- a shape change or the end of the loader closes a group early.  One eval-mode forward runs over the
concatenated group; loss and score are then evaluated per item on that item's slice (`loss.calc_loss_items`: the loop over
`calc_loss`, or one `umi_dice_ce_fwd_items` pass for 'dice_bce_mc' on the fused kernels' inputs, same bits; the regression ReLU
and the two heads / per-task losses as in `_forward_loss`; computed once when loss_function == accuracy_metric), and the rows are
added to the running sums [loss, score, task 1, task 2] -- one device vector of the losses' dtype -- by k sequential adds in
item order.  `steps` counts loader items, so the epoch figures, the per-task lists, model selection, early stop, the log lines and
the data-parallel phase reduction see what the item-by-item loop gives them.  With graph=True and device inputs a FULL group
replays from a `umi.graphs.GraphedEval` kept in `_eval_graphs` by group shapes (`_graphs` stays the training graphs): the first
full group of a shape runs eagerly, the second is captured (forward, per-item values, the adds into the running sums), short groups stay eager.
The eval graph holds no weight-pack node: GraphedEval refreshes the model's `ops.PackCache` eagerly before the capture and before
every replay, keyed on the parameter versions the cache tracks, so a replay after a training phase or a `load_state_dict` reads
current weights; BatchNorm running statistics are device tensors the captured kernels re-read.  `multi_task_trainRatio` with
`val_batch` raises NotImplementedError at train() (its validation bookkeeping is its own); a `val_batch` that is not None or a
positive int raises ValueError.
The hard-mask metrics of `loss.SEG_METRICS` ('dice_err_mc', 'iou_err_mc', 'pixel_err_mc', 'dice_err', 'iou_err', 'pixel_err':
1 - Dice / IoU / pixel accuracy of the argmax or threshold mask, lower is better) work as `accuracy_metric` in every validation
path above -- item by item, `val_batch` groups (one counting pass over the group), replayed groups, data parallel; as
`loss_function` they raise ValueError (not differentiable).  `Trainer(..., val_confusion=True)` (keyword-only; the single-output
model types): the validation phase also adds every item's confusion matrix (umi/metrics.py: [K+1, K+1] int64, row = label,
column = prediction, index K = "not a class"; K = the logits' channel count, 2 for one logit) into a static device accumulator
-- inside the captured group function too --, reads it back once after the phase (under data parallel after an int64
all-reduce, exact), appends it to `self.val_confusion_list` and keeps the per-class Dice / IoU of that dataset-level matrix in
`self.val_class_scores`.  When the accuracy metric is a hard-mask one the score comes from the same matrices (one pass).
`logs.txt`, the checkpoints and the other lists do not change; with `val_confusion=False` and another metric name none of
this runs.
The surface-distance metrics of `loss.SURFACE_METRICS` ('hd_mc', 'hd95_mc', 'assd_mc', 'hd', 'hd95', 'assd': Hausdorff distance,
its 95th percentile and the average symmetric surface distance of the argmax or threshold mask's foreground classes, in pixels,
lower is better; umi/surface.py) work as `accuracy_metric` in the same validation paths through `calc_loss` / `calc_loss_items`
(one kernel call per group).  The kernels take contiguous fp32 device logits with at most 8 channels and H, W <= 4096; on those
nothing allocates outside the caching allocator or synchronises, so a full group replays from its GraphedEval like any other.
Every other input (a 9-class model, `loss.METRICS_KERNEL = False`, ...) runs the NumPy statement on host copies, which
synchronises: a group whose first, eager run took that route is never captured and stays eager under `graph=True`
(`_eval_host`, decided by `loss.surface_host_calls()`), with the same scores, at the host's speed.  As `loss_function` they raise
ValueError.  With `val_confusion=True` the
confusion matrices take their own pass next to it.
`Trainer(..., async_checkpoints=True)` (keyword-only; singe_train / multi_task_train with the model on the device, otherwise
ignored): `last_epoch.pt`, `epochN.pt` and `best.pt` come from a `umi.snapshot.Snapshot` of `model.state_dict()` -- the training
stream pays one take() (umi_snapshot_multi: one copy pass into a contiguous arena) per epoch, the device-to-host copy runs on a
side stream and one `umi.snapshot.CheckpointWriter` thread writes the files (`.tmp`, then `os.replace`) beside the next epoch.
`best_model` becomes the views of a second arena (one launch instead of a deepcopy).  train() joins the writer before it
returns, also when it raises, and a write that failed is raised there.  The files hold what the synchronous path writes: same
keys, order, dtypes, shapes and values, every tensor in its own storage (CPU tensors; load with `map_location`).
`Trainer(..., resume=True | path)` (keyword-only; True = `<output_save_dir>/run_state.pt`): after every epoch's validation phase
rank 0 writes the RUN STATE atomically (through the writer when checkpoints are asynchronous): one dict that
`torch.load(weights_only=True)` accepts, with a format number, the epoch just finished and whether the run is over (the last
epoch, or an early stop), the model's state_dict, `optimizer.state_dict()` and the raw bytes of its device hyper blocks, the
GradGuard block, the dropout bases and counters, `best_model`, and under 'host' iter_num, max_iterations, the best scores, the
early-stop counter, every per-epoch list, `val_confusion_list`, `_guard_seen`, and the states of torch's CPU generator, the CUDA
generator of the model's device, Python's `random`, NumPy's global generator and each `dataloaders[phase].generator`.  'word' is
the fingerprint (umi.ddp) of all its state tensors in file order -- the word of the arena they were copied through --,
'host_word' that of the host fields.  At train(), if the file exists, it is checked first -- state-dict keys, shapes and dtypes,
optimizer class and group count, max_iterations, both words recomputed; ValueError or RuntimeError before anything is modified
-- then everything is put back, the generator states last, and the loop continues at the next epoch, or goes straight to its end
if the run was over; no file: a fresh run.  A run cut after any epoch and resumed with new objects, in a new process, gives the
lists, files, weights and optimizer state of the run that was never cut, bit for bit (eager and graph=True, fp32 and fp16, SGD
and Adam on the device poly rule, dropout, a moved dynamic loss scale, multi-task).  Refused with NotImplementedError before the
first step: `resume` with 'multi_task_loss_ratio' (its alpha and gate bookkeeping is its own) and with `data_parallel` over more
than one rank (per-rank generator states are not collected; a world of one works).  `snapshot_run_state()` /
`restore_run_state()` do the same in memory and IN PLACE between steps of a live run (the roll-back after a diverged epoch):
one Snapshot over parameters, buffers, optimizer state, hyper blocks, guard block and dropout counters, the host fields and
generator states beside it; every tensor keeps its address, so under graph=True no graph is captured again, and the parameter
versions are bumped, so the kernel-layout weight copies are re-packed.  With both arguments at their defaults none of this runs.
`Trainer(..., ema=...)` (keyword-only, after `resume`; singe_train / multi_task_train): None / False = nothing of this runs; True,
a float (the decay), `dict(decay=0.999, warmup=True, validate=True)` or a ready `umi.ema.ModelEMA` = an exponential moving average
of the parameters that require a gradient (buffers are not averaged: the averaged model is the averaged parameters plus the live
BatchNorm running statistics, as `AveragedModel(use_buffers=False)`); anything else raises ValueError.  The shadows are copies of
the parameters taken before the first step.  `ema.update()` (two launches, `umi_ema_pre` + `umi_ema_multi`) follows
`optimizer.step()` inside the step body, so a captured step contains it; in the deferred data-parallel path it follows `flush()` +
`optimizer.step()` after each replay.  The `grad_guard` block gates it on the device: a skipped step leaves the shadows' bits and
the update count alone, eagerly and in a replay.  With `validate=True` (the default) the validation phase runs on the averaged
weights IN PLACE: `ema.swap()` exchanges parameters and shadows after `_dp_phase`'s BatchNorm broadcast (one launch; the parameter
versions are bumped, so `ops.PackCache` and the eval graphs re-pack), and swaps back after the best-model decision -- loss, score,
`best_model`, `epochN.pt` and `best.pt` are those of the averaged weights (what is validated is what is saved, and what train()
returns), `last_epoch.pt` keeps the live weights; under `async_checkpoints` the best files then come from a host copy of the
best-model arena taken while the average is swapped in, not from the copy behind `last_epoch.pt`.  `validate=False` only maintains
the average (`trainer.ema`: `averaged()`, `copy_to(model)`, `state_dict()`).  One line per epoch goes to `logs.txt` after the
training phase, on rank 0: `EMA on epoch N: decay D, updates U` (D = the decay of the last update).  The shadows and the state
block are part of `_state_tensors` (`ema.shadow.<name>`, `ema.state`): `resume` and `snapshot_run_state()` / `restore_run_state()`
carry them, a resumed run stays bit-identical, a run-state file written with `ema` and read without it (or the reverse) raises
before anything is modified, and the data-parallel replica check covers them.  With 'multi_task_loss_ratio' train() raises
NotImplementedError before the first step.
`lr_scheduler=True` (what the reference's train.py passes) crashes the reference in its first validation after epoch 5
(`True.step`); here train() raises NotImplementedError before the first step whenever the run would reach that point.
The remaining epoch loops of the reference (uncertainty-weighted multi-task, CLTR, Topo losses) are out of scope and raise.
"""
import copy
import os
import time

import numpy as np
import torch
import torch.nn.functional as F
from tqdm import tqdm

import loss as _loss
from loss import SEG_METRICS, SURFACE_METRICS, calc_loss, calc_loss_items, multi_task_ratio_loss, seg_confusion_items, seg_scores

_SINGLE = ('single', 'TransUnet', 'regression', 'regression_t', 'attention')
_TOPO = ('TopoCount', 'TopoCount2', 'TopoLoss', 'TopoLoss2', 'MyTopoLoss1', 'MyTopoLoss2', 'MyTopoLossGraph',
         'MyTopoLossVR')
_MULTI = ('multi_task', 'multi_task_reg', 'multi_task_regTU')
_OTHER = ('CLTR',)


class Trainer():
    def __init__(self, model, model_type, dtype, device, output_save_dir, dataloaders, batch_size, optimizer,
                 patience, num_epochs, loss_function, accuracy_metric, lr_scheduler=None, start_epoch=1, *, graph=None,
                 batch_transform=None, grad_guard=None, data_parallel=None, val_batch=None, val_confusion=False,
                 async_checkpoints=False, resume=None, ema=None):
        self.model = model
        self.model_type = model_type
        self.dtype = dtype
        self.device = device
        self.output_save_dir = output_save_dir
        self.dataloader = dataloaders
        self.batch_size = batch_size
        self.optimizer = optimizer
        self.patience = patience
        self.num_epochs = num_epochs
        self.loss_function = loss_function
        self.accuracy_metric = accuracy_metric
        self.lr_scheduler = lr_scheduler
        self.start_epoch = start_epoch

        self.phases = ["train", "val"]
        self.iter_num = 0
        self.base_lr = self.optimizer.param_groups[-1]['lr']
        self.max_iterations = self.num_epochs * len(self.dataloader['train'])
        self.best_loss = 1e15
        self.best_val_score = 0 if accuracy_metric in ('dice_score', 'dice_score_mc') else 1e15
        self.best_model = []
        self.early_stop_counter = 0
        self.train_loss_list, self.val_loss_list, self.val_score_list = [], [], []
        self.train_loss_list_1, self.train_loss_list_2, self.val_loss_list_1, self.val_loss_list_2 = [], [], [], []
        self.grad_sync = None         # optional callable run between backward and optimizer.step (DDP)
        self.graph = (os.environ.get("UMI_TRAINER_GRAPH") == "1") if graph is None else bool(graph)
        self._graphs, self._seen_shapes, self._dev_sched, self._side = {}, set(), False, None
        self.batch_transform = batch_transform
        self._guard, self._guard_seen = self._make_guard(grad_guard), (0, 0)
        # multi_task_trainRatio: epoch > 5 (host, and in graph mode a device flag), ratioAccuracy of the last step
        self._ratio_gate, self._gate_dev, self._ratio = False, None, None
        self.alpha, self.alpha_list = None, []
        # data parallel (see the module docstring): the spec, then -- from the start of train() -- the umi.ddp.GradReducer,
        # whether this Trainer built it, the replica check, this rank, and a line for the log
        self._dp_spec = None if data_parallel is False else data_parallel
        self._dp, self._dp_own, self._dp_check, self._rank, self._dp_note = None, False, False, 0, None
        self._dp_built = None         # the reducer train() built, kept for a later train(): captured graphs hold its addresses
        # batched validation (see the module docstring): the group size, the eval graphs by group shapes (`_graphs` stays the
        # training graphs), the shapes that ran eagerly once, and the running sums [loss, score, task 1, task 2] (one vector of
        # the losses' dtype, where the model runs)
        if val_batch is not None and (isinstance(val_batch, bool) or not isinstance(val_batch, int) or val_batch < 1):
            raise ValueError(f"val_batch takes None or a positive int, not {val_batch!r}")
        self.val_batch = val_batch
        self._eval_graphs, self._eval_seen, self._val_sums = {}, set(), None
        self._eval_host = set()       # group shapes whose eager run copied to the host (surface metrics' composite): never captured
        # hard-mask metrics (see the module docstring): the dataset-level matrix of each validation phase, its per-class scores,
        # and the static device accumulator the validation steps add into
        if loss_function in SEG_METRICS:
            raise ValueError(f"loss_function {loss_function!r} is a hard-mask metric: not differentiable, use it as accuracy_metric")
        if loss_function in SURFACE_METRICS:
            raise ValueError(f"loss_function {loss_function!r} is a surface-distance metric: not differentiable, use it as "
                             "accuracy_metric")
        if val_confusion and model_type not in _SINGLE:
            raise ValueError(f"val_confusion covers the single-output model types {_SINGLE}, not {model_type!r}")
        self.val_confusion = bool(val_confusion)
        self.val_confusion_list, self.val_class_scores, self._val_conf = [], None, None

        # snapshots (see the module docstring): checkpoints through a device arena and a writer thread; the run-state file; the
        # in-memory roll-back.  All None / off by default: nothing below runs then.
        self.async_checkpoints = bool(async_checkpoints)
        if resume is None or resume is False:
            self._resume_path = None
        elif resume is True:
            self._resume_path = os.path.join(self.output_save_dir, 'run_state.pt')
        else:
            self._resume_path = os.fspath(resume)
        self._writer, self._ckpt_snap, self._best_snap, self._file_snap, self._run_snap = None, None, None, None, None
        self._run_host, self._total_time, self._best_views, self._ckpt_event = None, 0.0, False, None

        # weight average (see the module docstring): the ModelEMA arguments (or a ready ModelEMA) until the first step, then the
        # ModelEMA; whether the validation phase runs on the averaged weights
        self._ema_spec, self._ema_validate = self._parse_ema(ema)
        self._ema = None

        self.save_dir_model = os.path.join(self.output_save_dir, 'models/')
        os.makedirs(self.save_dir_model, exist_ok=True)

    @staticmethod
    def _parse_ema(spec):
        """`ema` -> (None | dict of ModelEMA arguments | ModelEMA, validate).  ValueError on anything else."""
        if spec is None or spec is False:
            return None, False
        if spec is True:
            return {}, True
        if isinstance(spec, float):
            spec = dict(decay=spec)
        if isinstance(spec, dict):
            kw = dict(spec)
            validate = kw.pop('validate', True)
            if set(kw) - {'decay', 'warmup'} or not isinstance(validate, bool):
                raise ValueError(f"ema takes dict(decay=0.999, warmup=True, validate=True), not {spec!r}")
            if not 0.0 <= float(kw.get('decay', 0.999)) < 1.0:
                raise ValueError(f"ema: decay must be in [0, 1), not {kw['decay']!r}")
            return kw, validate
        if type(spec).__name__ == 'ModelEMA' and hasattr(spec, 'swap'):
            return spec, True
        raise ValueError(f"ema takes None / False, True, a float (the decay), a dict(decay=, warmup=, validate=) or a "
                         f"umi.ema.ModelEMA, not {spec!r}")

    @property
    def ema(self):
        """The umi.ema.ModelEMA of this run (None: `ema` is off, or no step has run yet)."""
        return self._ema

    def _attach_ema(self):
        """Before the first step (and before a run state is read): the shadows as copies of the parameters, which are where
        they train by now; the guard gates the update on the device."""
        if self._ema_spec is None or self._ema is not None:
            return
        if isinstance(self._ema_spec, dict):
            from umi.ema import ModelEMA
            self._attach_guard()
            self._ema = ModelEMA(self.model, guard=self._guard, **self._ema_spec)
        else:
            self._ema = self._ema_spec
            if self._ema.guard is None and self._guard is not None:
                self._attach_guard()
                self._ema.guard = self._guard

    def _ema_tensors(self):
        import collections
        if self._ema is None:
            return collections.OrderedDict()
        return collections.OrderedDict(('ema.' + k, v) for k, v in self._ema.tensors().items())

    def _log_ema(self, say, epoch):
        if self._ema is None or not self._main:
            return
        r = self._ema.sync_host()
        say("EMA on epoch %i: decay %g, updates %i" % (epoch, r["last"], r["updates"]))

    @staticmethod
    def _make_guard(spec):
        if spec is None or spec is False:
            return None
        from umi.optim import GradGuard
        if isinstance(spec, GradGuard):
            return spec
        return GradGuard(**({} if spec is True else dict(spec)))

    def _attach_guard(self):
        """Before the first step: guard -> optimizer and model (whose parameters are on the device by now)."""
        if self._guard is None or getattr(self.optimizer, "guard", None) is self._guard:
            return
        if not hasattr(self.optimizer, "grad_guard"):
            raise TypeError("Trainer(grad_guard=...) needs a umi.optim optimizer")
        self.optimizer.grad_guard(self._guard)
        self._guard.attach(self.model)

    def _device_schedule(self):
        if not self._dev_sched:
            poly = dict(base_lr=self.base_lr, max_iterations=self.max_iterations, power=0.9, iter_num=self.iter_num)
            self.optimizer.device_schedule(poly=poly if self.lr_scheduler else None)
            self._dev_sched = True

    def _log_guard(self, say, epoch):
        if self._guard is None:
            return
        r = self._guard.read()
        say("Guard on epoch %i: skipped %i, clipped %i, loss scale %g"
            % (epoch, r["skipped"] - self._guard_seen[0], r["clipped"] - self._guard_seen[1], r["scale"]))
        self._guard_seen = (r["skipped"], r["clipped"])

    # ---- data parallel ------------------------------------------------------------------
    @property
    def _main(self):
        """Rank 0 (or no data parallel): the rank that writes files and prints."""
        return self._rank == 0

    def _dp_device(self):
        p = next(self.model.parameters(), None)
        return p.device if p is not None else torch.device("cpu")

    def _dp_begin(self):
        """Start of train(): argument checks, equal step counts, the reducer (whose constructor broadcasts rank 0's replica), the
        first replica check."""
        import torch.distributed as dist
        from umi import ddp
        spec = self._dp_spec
        if self.grad_sync is not None:
            raise ValueError("Trainer(data_parallel=...) runs the gradient exchange itself; do not set trainer.grad_sync as well")
        if self._ratio_loop():
            raise NotImplementedError("multi_task_trainRatio under data_parallel: its alpha and count-ratio sums are not reduced "
                                      "over the ranks")
        if isinstance(spec, ddp.GradReducer):
            kw, check, world, group = None, True, spec.world, spec.group
        else:
            if spec is not True and not isinstance(spec, dict):
                raise TypeError("data_parallel takes None / False, True, a dict of umi.ddp.GradReducer arguments (plus "
                                f"check_replicas) or a GradReducer, not {spec!r}")
            kw = {} if spec is True else dict(spec)
            check, world, group = bool(kw.pop("check_replicas", True)), kw.get("world_size"), kw.get("group")
            if world is None or world > 1:
                if not (dist.is_available() and dist.is_initialized()):
                    raise RuntimeError("Trainer(data_parallel=...) over more than one rank needs an initialised process group "
                                       "(torch.distributed.init_process_group, one process per GPU)")
                world = dist.get_world_size(group) if world is None else world
        self._rank = dist.get_rank(group) if world > 1 else 0
        if world > 1:                         # before anything is touched: a rank with fewer steps would leave the others waiting
            mine = torch.tensor([len(self.dataloader['train'])], dtype=torch.int64, device=self._dp_device())
            lens = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(lens, mine, group=group)
            lens = [int(t.item()) for t in lens]
            if len(set(lens)) > 1:
                raise ValueError(f"data_parallel needs the same number of training steps on every rank, got {lens} (per rank); "
                                 "use a DistributedSampler with drop_last, or equal shards")
        if kw is None:
            self._dp, self._dp_own = spec, False
        elif self._dp_built is not None:
            self._dp, self._dp_own = self._dp_built.reopen(), True
        else:
            self._dp = self._dp_built = ddp.GradReducer(self.model, **kw)
            self._dp_own = True
        self._dp_check = check and world > 1
        self.grad_sync = self._dp.sync
        if self.graph and world > 1 and self._dp.batch_sync is not None:
            self._dp_note = ("data_parallel: graph=True runs eagerly under global_batch=True (the statistics all-reduce of "
                             "every BatchNorm layer and of the loss is a collective, and collectives are not captured)")
        self._dp_verify()

    def _dp_verify(self):
        if self._dp_check:
            from umi import ddp
            if self._ema is None:
                ddp.check_replicas(self.model, self._dp.group, buffers=self._dp.batch_sync is not None)
            else:
                ddp.check_replicas(self.model, self._dp.group, buffers=self._dp.batch_sync is not None,
                                   extra=list(self._ema.tensors().values()))

    def _dp_end(self):
        """End of train(), also on an error: hand the model back as it came (a reducer built here is closed, so the
        global-batch switch does not leak into later code)."""
        if self._dp is None:
            return
        if self.grad_sync == self._dp.sync:
            self.grad_sync = None
        if self._dp_own:
            self._dp.close()
        elif self._dp.batch_sync is not None:
            from umi import ddp
            ddp.set_active_batch_sync(self._dp.batch_sync)         # as the caller's reducer had it (validation turns it off)
        self._dp, self._dp_own = None, False

    def _dp_phase(self, train):
        """Before a phase.  Validation: what is validated is what rank 0 saves -- without global_batch the BatchNorm running
        statistics differ per rank, so rank 0's buffers are broadcast; and the loss is each rank's own (the shards may be unequal
        or empty, so no collective may sit inside a validation step), reduced once afterwards."""
        if self._dp is None:
            return
        import torch.distributed as dist
        from umi import ddp
        if self._dp.batch_sync is not None:
            ddp.set_active_batch_sync(self._dp.batch_sync if train else None)
        elif not train and self._dp.world > 1:
            with torch.no_grad():
                for b in self.model.buffers():
                    dist.broadcast(b, 0, group=self._dp.group)

    def _dp_reduce(self, sums):
        """One all-reduce per phase: the float64 sums (losses, score, step count) of all ranks, so every rank derives the same
        epoch figures and the same model selection and early stop from them."""
        if self._dp is None or self._dp.world == 1:
            return sums
        import torch.distributed as dist
        vec = torch.tensor(sums, dtype=torch.float64, device=self._dp_device())
        dist.all_reduce(vec, op=dist.ReduceOp.SUM, group=self._dp.group)
        return vec.tolist()

    # ---- snapshots: asynchronous checkpoints, the run-state file, in-place roll-back ------------------------------------------
    _LISTS = ('train_loss_list', 'val_loss_list', 'val_score_list', 'train_loss_list_1', 'train_loss_list_2', 'val_loss_list_1',
              'val_loss_list_2', 'alpha_list')
    RUN_STATE_FORMAT = 1

    def _resume_refusals(self):
        """Before anything runs: what `resume` does not cover."""
        if self._resume_path is None:
            return
        if self._ratio_loop():
            raise NotImplementedError("resume with multi_task_loss_ratio: the loop's alpha and gate bookkeeping is its own and is "
                                      "not part of the run state")
        spec, world = self._dp_spec, 1
        if spec is not None:
            import torch.distributed as dist
            if isinstance(spec, dict):
                world = spec.get("world_size")
            elif hasattr(spec, "world"):
                world = spec.world
            else:
                world = None
            if world is None:
                world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        if world > 1:
            raise NotImplementedError("resume with data_parallel over more than one rank: the per-rank random-generator states "
                                      "are not collected (a world of one works)")

    def _ckpt_async(self):
        return self.async_checkpoints and self._dp_device().type == "cuda"

    def _writer_get(self):
        if self._writer is None:
            from umi.snapshot import CheckpointWriter
            self._writer = CheckpointWriter()
        return self._writer

    def _writer_close(self):
        w, self._writer = self._writer, None
        if w is not None:
            w.close()

    def _snap_for(self, slot, tensors):
        """The Snapshot kept in attribute `slot` for exactly these live tensors (built again when one of them moved)."""
        from umi.snapshot import Snapshot
        key = tuple((k, v.data_ptr(), v.numel() * v.element_size()) for k, v in tensors.items())
        have = getattr(self, slot)
        if have is None or have[0] != key:
            have = (key, Snapshot(tensors))
            setattr(self, slot, have)
        return have[1]

    def _submit(self, snap, event, obj, path):
        self._writer_get().submit(event, obj, path, snap.hold_host())

    def _save_last(self, path):
        """'last_epoch.pt' after a training phase: one take() on the training stream; the copy to the host and the write run
        beside what follows."""
        snap = self._snap_for('_ckpt_snap', self.model.state_dict())
        snap.take()
        self._ckpt_event = snap.to_host_async()
        self._submit(snap, self._ckpt_event, snap.host_views(), path)

    def _save_best(self, paths):
        """A new best model: `best_model` becomes the views of a second arena (one launch instead of a deepcopy); the files come
        from the host copy that 'last_epoch.pt' of this epoch was taken from (a validation phase changes no weight or buffer)."""
        best = self._snap_for('_best_snap', self.model.state_dict())
        best.take()
        self.best_model, self._best_views = best.views(), True
        if self._ema is not None and self._ema.swapped:
            # the averaged weights are swapped in: this phase DID change the weights, so the files come from a host copy of the
            # arena just taken, not from the one behind 'last_epoch.pt' (which keeps the live weights)
            event = best.to_host_async()
            for path in paths:
                self._submit(best, event, best.host_views(), path)
            return
        snap = self._ckpt_snap[1] if self._ckpt_snap is not None else None
        for path in paths:
            self._submit(snap, self._ckpt_event, snap.host_views(), path)

    def _state_tensors(self, best=True):
        """name -> live tensor of everything a step reads or writes that lives in tensors: parameters and buffers, the optimizer's
        momentum buffers or moments, its device hyper blocks, the guard block, the dropout counters, and (`best`) the best model."""
        import collections
        out = collections.OrderedDict()
        for k, v in self.model.state_dict().items():
            out['model.' + k] = v
        idx = 0
        for group in self.optimizer.param_groups:
            for p in group['params']:
                if p in self.optimizer.state:
                    for k, v in self.optimizer.state[p].items():
                        if torch.is_tensor(v) and k != 'step':         # Adam's step count is a host scalar (see _host_fields)
                            out[f'optim.{idx}.{k}'] = v
                idx += 1
        for gi, (dev, _) in enumerate(getattr(self.optimizer, 'device_hyper', None) or []):
            out[f'hyper.{gi}'] = dev
        if self._guard is not None and self._guard.state is not None:
            out['guard'] = self._guard.state
        for name, m in self.model.named_modules():
            if getattr(m, '_drop_step', None) is not None:
                out['drop.' + name] = m._drop_step
        out.update(self._ema_tensors())
        if best and isinstance(self.best_model, dict):
            for k, v in self.best_model.items():
                out['best.' + k] = v
        return out

    def _rng_get(self):
        import random
        dev = self._dp_device()
        kind, keys, pos, has_gauss, cached = np.random.get_state()
        loaders = {ph: dl.generator.get_state() for ph, dl in self.dataloader.items()
                   if isinstance(getattr(dl, 'generator', None), torch.Generator)}
        return dict(torch_cpu=torch.get_rng_state(), torch_cuda=torch.cuda.get_rng_state(dev) if dev.type == 'cuda' else None,
                    python=random.getstate(), loaders=loaders,
                    numpy=(str(kind), torch.from_numpy(keys.astype(np.int64)), int(pos), int(has_gauss), float(cached)))

    def _rng_set(self, rng):
        import random
        for ph, st in rng['loaders'].items():
            gen = getattr(self.dataloader.get(ph), 'generator', None)
            if isinstance(gen, torch.Generator):
                gen.set_state(st)
        kind, keys, pos, has_gauss, cached = rng['numpy']
        np.random.set_state((kind, keys.numpy().astype(np.uint32), pos, has_gauss, cached))
        version, words, gauss = rng['python']
        random.setstate((version, tuple(words), gauss))
        if rng['torch_cuda'] is not None:
            torch.cuda.set_rng_state(rng['torch_cuda'], self._dp_device())
        torch.set_rng_state(rng['torch_cpu'])

    def _host_fields(self):
        """Everything of the run that lives on the host, as values torch.load(weights_only=True) accepts."""
        groups = [{k: v for k, v in g.items() if k != 'params'} for g in self.optimizer.param_groups]
        steps, idx = {}, 0
        for g in self.optimizer.param_groups:
            for p in g['params']:
                st = self.optimizer.state[p] if p in self.optimizer.state else {}
                if 'step' in st:
                    steps[idx] = float(st['step'])
                idx += 1
        scores = self.val_class_scores
        return dict(iter_num=self.iter_num, max_iterations=self.max_iterations, base_lr=self.base_lr,
                    best_val_score=self.best_val_score, best_loss=self.best_loss, early_stop_counter=self.early_stop_counter,
                    lists={n: list(getattr(self, n)) for n in self._LISTS}, alpha=self.alpha,
                    val_confusion_list=[torch.from_numpy(np.array(m, dtype=np.int64)) for m in self.val_confusion_list],
                    val_class_scores=None if scores is None else {k: torch.from_numpy(np.array(v, dtype=np.float64))
                                                                  for k, v in scores.items()},
                    guard_seen=tuple(self._guard_seen), total_time=float(self._total_time), groups=copy.deepcopy(groups),
                    adam_steps=steps, drop_base={name: int(m._drop_base) for name, m in self.model.named_modules()
                                                 if getattr(m, '_drop_base', None) is not None},
                    rng=self._rng_get())

    def _put_host(self, host):
        """The host fields back, except the generators' states (_rng_set, which goes last)."""
        self.iter_num, self.base_lr = host['iter_num'], host['base_lr']
        self.best_val_score, self.best_loss = host['best_val_score'], host['best_loss']
        self.early_stop_counter, self.alpha = host['early_stop_counter'], host['alpha']
        for n in self._LISTS:
            setattr(self, n, list(host['lists'][n]))
        self.val_confusion_list = [m.numpy().copy() for m in host['val_confusion_list']]
        scores = host['val_class_scores']
        self.val_class_scores = None if scores is None else {k: v.numpy().copy() for k, v in scores.items()}
        self._guard_seen, self._total_time = tuple(host['guard_seen']), host['total_time']

    # -- in memory, in place ---------------------------------------------------------------
    def snapshot_run_state(self):
        """Between two steps of a live run: the whole training state into one device arena (one launch) plus the host fields
        and generator states beside it.  restore_run_state() puts it back IN PLACE: every tensor keeps its address, so graphs
        captured before stay valid and none is captured again."""
        # a deepcopy'd best model is never written to again: the reference is enough.  The views of the asynchronous path show
        # an arena that the next best model overwrites, so that arena is part of the snapshot
        views = self._best_views and isinstance(self.best_model, dict)
        snap = self._snap_for('_run_snap', self._state_tensors(best=views))
        snap.take()
        self._run_host = (self._host_fields(), self.best_model, views)
        return snap

    def restore_run_state(self):
        if self._run_snap is None or self._run_host is None:
            raise RuntimeError("restore_run_state() without a snapshot_run_state() before it")
        (key, snap), (host, best, views) = self._run_snap, self._run_host
        live = self._state_tensors(best=False)
        if views:
            live.update(('best.' + k, v) for k, v in best.items())
        if tuple((k, v.data_ptr(), v.numel() * v.element_size()) for k, v in live.items()) != key:
            raise RuntimeError("restore_run_state(): the state's tensors changed since the snapshot (a tensor moved, or optimizer "
                               "state appeared); take the snapshot after the first step")
        snap.restore()                         # verifies the arena first; bumps the parameter versions (weight re-pack)
        self.best_model = best
        self._put_host(host)
        for g, saved in zip(self.optimizer.param_groups, host['groups']):
            g.update(copy.deepcopy(saved))
        idx = 0
        for g in self.optimizer.param_groups:
            for p in g['params']:
                if idx in host['adam_steps']:
                    self.optimizer.state[p]['step'].fill_(host['adam_steps'][idx])
                idx += 1
        self._rng_set(host['rng'])

    # -- the file --------------------------------------------------------------------------
    @staticmethod
    def _payload_tensors(pl):
        """name -> tensor of a run-state payload, in the order of _state_tensors: what the fingerprint word is taken over."""
        import collections
        out = collections.OrderedDict(('model.' + k, v) for k, v in pl['model'].items())
        for idx in sorted(pl['optimizer']['state']):
            for k, v in pl['optimizer']['state'][idx].items():
                if torch.is_tensor(v) and k != 'step':
                    out[f'optim.{idx}.{k}'] = v
        for gi, h in enumerate(pl['hyper'] or []):
            out[f'hyper.{gi}'] = h
        if pl['guard'] is not None:
            out['guard'] = pl['guard']
        for name, step in pl['drop_step'].items():
            out['drop.' + name] = step
        for k, v in (pl.get('ema') or {}).items():
            out['ema.' + k] = v
        for k, v in (pl['best_model'] or {}).items():
            out['best.' + k] = v
        return out

    @staticmethod
    def _host_word(host):
        """One fingerprint word over the host fields: the tensors among them (bytes, zero-padded to whole words) and the text of
        everything else."""
        from umi.ddp import fingerprint_numpy
        arrays = []

        def walk(o):
            if torch.is_tensor(o):
                raw = o.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy()
                arrays.append(np.concatenate([raw, np.zeros(-raw.size % 4, dtype=np.uint8)]))
                return 'T%d' % (len(arrays) - 1)
            if isinstance(o, dict):
                return [(repr(k), walk(v)) for k, v in o.items()]
            if isinstance(o, (list, tuple)):
                return [walk(v) for v in o]
            return repr(o)
        text = np.frombuffer(repr(walk(host)).encode(), dtype=np.uint8)
        arrays.append(np.concatenate([text, np.zeros(-text.size % 4, dtype=np.uint8)]))
        return fingerprint_numpy(arrays)

    def _write_run_state(self, epoch, over):
        """The run state after `epoch`'s validation phase -> the file, atomically; through the writer when checkpoints are
        asynchronous, otherwise before this returns."""
        import collections
        from umi.snapshot import _own, save_atomic
        live = self._state_tensors()
        snap = self._snap_for('_file_snap', live)
        snap.take()
        event = snap.to_host_async()
        views = snap.host_views()
        osd = self.optimizer.state_dict()
        for idx, st in osd['state'].items():
            osd['state'][idx] = {k: views.get(f'optim.{idx}.{k}', v.detach().cpu() if torch.is_tensor(v) else v)
                                 for k, v in st.items()}
        take = lambda prefix: collections.OrderedDict((k[len(prefix):], v) for k, v in views.items() if k.startswith(prefix))
        model = take('model.')
        meta = getattr(self.model.state_dict(), '_metadata', None)
        if meta is not None:
            model._metadata = meta
        host = self._host_fields()
        pl = dict(format=self.RUN_STATE_FORMAT, epoch=int(epoch), over=bool(over), model=model, optimizer=osd,
                  optimizer_class=type(self.optimizer).__name__, hyper=list(take('hyper.').values()) or None,
                  guard=views.get('guard'), drop_step=dict(take('drop.')), best_model=take('best.') or None, host=host,
                  ema=take('ema.') or None,
                  word=snap.word(), host_word=self._host_word(host))
        assert list(self._payload_tensors(pl)) == list(live)
        if self._ckpt_async():
            self._submit(snap, event, pl, self._resume_path)
        else:
            event.synchronize()
            save_atomic(_own(pl), self._resume_path)

    def _resume_from_file(self):
        """None when there is no file; else the file is checked against this Trainer -- nothing is modified before every check
        has passed -- and put back.  Returns (epoch finished, run over)."""
        path = self._resume_path
        if not os.path.exists(path):
            return None
        from umi import ddp
        if self._graphs or self._eval_graphs:
            raise RuntimeError("resume: this Trainer has captured graphs, which hold the addresses of the optimizer state a file "
                               "would replace; resume with a new Trainer, or roll back in place with restore_run_state()")
        try:
            pl = torch.load(path, map_location='cpu', weights_only=True)
            ok = isinstance(pl, dict) and pl.get('format') == self.RUN_STATE_FORMAT
            tensors = self._payload_tensors(pl) if ok else None
        except Exception as e:
            raise ValueError(f"resume: {path} cannot be read as a run state ({type(e).__name__}: {e})") from e
        if not ok:
            raise ValueError(f"resume: {path} is not a run state of format {self.RUN_STATE_FORMAT}")
        sd = self.model.state_dict()
        if list(pl['model']) != list(sd):
            raise ValueError(f"resume: the model of {path} has other state-dict keys than this model")
        for k, v in sd.items():
            if pl['model'][k].shape != v.shape or pl['model'][k].dtype != v.dtype:
                raise ValueError(f"resume: {k} is {tuple(pl['model'][k].shape)} {pl['model'][k].dtype} in {path}, "
                                 f"{tuple(v.shape)} {v.dtype} in this model")
        if pl['optimizer_class'] != type(self.optimizer).__name__ or \
                len(pl['optimizer']['param_groups']) != len(self.optimizer.param_groups):
            raise ValueError(f"resume: {path} was written with {pl['optimizer_class']} over "
                             f"{len(pl['optimizer']['param_groups'])} param groups, not {type(self.optimizer).__name__} over "
                             f"{len(self.optimizer.param_groups)}")
        host = pl['host']
        if host['max_iterations'] != self.max_iterations:
            raise ValueError(f"resume: {path} belongs to a run of {host['max_iterations']} iterations, this one has "
                             f"{self.max_iterations} (num_epochs or the training loader differ)")
        if (pl['hyper'] or pl['guard'] is not None) and not hasattr(self.optimizer, 'device_schedule'):
            raise ValueError(f"resume: {path} holds device optimizer blocks; this optimizer is not a umi.optim one")
        if pl['guard'] is not None and self._guard is None:
            raise ValueError(f"resume: {path} was written with a grad_guard, this Trainer has none")
        mine, theirs = self._ema_tensors(), pl.get('ema') or {}
        if ['ema.' + k for k in theirs] != list(mine):
            raise ValueError(f"resume: {path} was written {'with' if theirs else 'without'} an `ema`, this Trainer runs "
                             f"{'with another one' if mine and theirs else 'with one' if mine else 'without'}")
        for k, v in theirs.items():
            if v.shape != mine['ema.' + k].shape or v.dtype != mine['ema.' + k].dtype:
                raise ValueError(f"resume: ema.{k} is {tuple(v.shape)} {v.dtype} in {path}, "
                                 f"{tuple(mine['ema.' + k].shape)} {mine['ema.' + k].dtype} in this Trainer")
        dev = self._dp_device()
        words = [t.to(dev) for t in tensors.values()]
        for i, t in enumerate(words):
            if (t.numel() * t.element_size()) % 4:
                raise ValueError(f"resume: tensor {i} of {path} is not a whole number of 32-bit words")
        if ddp.fingerprint(words) != pl['word'] or self._host_word(host) != pl['host_word']:
            raise RuntimeError(f"resume: the contents of {path} do not match its fingerprint word; nothing was restored")
        modules = dict(self.model.named_modules())
        if any(name not in modules for name in list(pl['drop_step']) + list(host['drop_base'])):
            raise ValueError(f"resume: {path} names dropout modules this model does not have")

        # every check passed: put it back
        self.model.load_state_dict(pl['model'])
        self.optimizer.load_state_dict(pl['optimizer'])
        self._put_host(host)
        self.best_model, self._best_views = [], False
        if pl['best_model'] is not None:
            self.best_model = type(pl['best_model'])((k, v.to(dev)) for k, v in pl['best_model'].items())
        if pl['hyper']:
            self._device_schedule()
            for (block, _), raw in zip(self.optimizer.device_hyper, pl['hyper']):
                block.copy_(raw)
        if pl['guard'] is not None:
            self._attach_guard()
            self._guard._device_state().copy_(pl['guard'])
        with torch.no_grad():
            for k, v in theirs.items():
                mine['ema.' + k].copy_(v)
        for name, base in host['drop_base'].items():
            modules[name]._drop_base = int(base)
        for name, step in pl['drop_step'].items():
            modules[name]._drop_step = step.to(dev)
        self._rng_set(host['rng'])             # last: nothing above may consume a draw after this
        return pl['epoch'], pl['over']

    # ------------------------------------------------------------------------------------
    def train(self):
        if self._ema_spec is not None and self._ratio_loop():
            raise NotImplementedError("ema with multi_task_loss_ratio: the count-ratio loop is not covered")
        if not self.async_checkpoints and self._resume_path is None:
            return self._train_dp()
        self._resume_refusals()
        try:
            return self._train_dp()
        finally:
            self._writer_close()              # every queued file is on disk, or its error is raised here

    def _train_dp(self):
        if self._dp_spec is None:
            return self._train()
        try:
            self._dp_begin()
            return self._train()
        finally:
            self._dp_end()

    def _train(self):
        if self.model_type in _SINGLE:
            if self.loss_function in _TOPO:
                raise NotImplementedError("Topo-loss warm-up loop (reference singe_train_wup) is out of scope")
            return self.singe_train()
        if self.model_type in _MULTI:
            if self.loss_function == 'multi_task_loss':
                raise NotImplementedError("uncertainty-weighted multi-task loop (reference multi_task_uc_train) is out of scope")
            if self.loss_function == 'multi_task_loss_ratio':
                if self.val_batch is not None:
                    raise NotImplementedError("multi_task_trainRatio with val_batch: its validation bookkeeping (alpha, the "
                                              "count-ratio sums) is its own and is not batched")
                return self.multi_task_trainRatio()
            return self.multi_task_train()
        if self.model_type in _OTHER:
            raise NotImplementedError(f'model_type "{self.model_type}" (CLTR loop) is out of scope')
        raise ValueError('Invalid model_type "%s"' % self.model_type)

    # ------------------------------------------------------------------------------------
    def _transform_batch(self, inputs, labels, train):
        """Raw batch -> network batch with self.batch_transform, on self.device."""
        from umi.augment import no_augmentation
        multi = isinstance(labels, (list, tuple))
        inputs = inputs.to(self.device)
        maps = [l.to(self.device) for l in labels] if multi else labels.to(self.device)
        params = None if train else no_augmentation(inputs.shape[0])       # None: the transform draws them
        inputs, out = self.batch_transform(inputs, maps, params)
        return inputs, (tuple(out) if multi else out)

    def _to_device(self, inputs, labels, train=True):
        if self.batch_transform is not None:
            inputs, labels = self._transform_batch(inputs, labels, train)
        if isinstance(labels, (list, tuple)):                    # multi-task batches: labels = (label1, label2)
            return inputs.to(self.device).type(self.dtype), tuple(l.to(self.device).type(self.dtype) for l in labels)
        return inputs.to(self.device).type(self.dtype), labels.to(self.device).type(self.dtype)

    def _ratio_loop(self):
        return self.model_type in _MULTI and self.loss_function == 'multi_task_loss_ratio'

    def _forward_loss(self, inputs, labels):
        if self._ratio_loop():                                   # reference Trainer.py:1226-1249
            o1, o2 = self.model(inputs)
            gate = self._ratio_gate if self._gate_dev is None else self._gate_dev
            loss, loss1, loss2, self._ratio = multi_task_ratio_loss(o1, o2, labels[0], labels[1], gate)
            self._task_losses = [loss1, loss2]
            return (o1, o2), loss
        if self.model_type in _MULTI:                            # reference Trainer.py:882-890
            outs = tuple(F.relu(o) for o in self.model(inputs))
            self._task_losses = [calc_loss(o, l, loss_type=self.loss_function) for o, l in zip(outs, labels)]
            return outs, self._task_losses[0] + self._task_losses[1]
        out = self.model(inputs)
        if self.model_type in ('regression', 'regression_t'):
            out = F.relu(out)
        return out, calc_loss(out, labels, loss_type=self.loss_function)

    def _step_body(self, inputs, labels, deferred=False):
        with torch.set_grad_enabled(True):
            _, loss = self._forward_loss(inputs, labels)
            self.optimizer.zero_grad()
            loss.backward()
            if deferred:                      # captured data-parallel step: flush() and optimizer.step() follow each replay
                return loss
            if self.grad_sync is not None:
                self.grad_sync()
            self.optimizer.step()
            if self._ema is not None:         # inside the step: a captured step contains the update
                self._ema.update()
        return loss

    def _graph_capable(self, inputs):
        if not (self.graph and inputs.is_cuda and hasattr(self.optimizer, "device_schedule")):
            return False
        if self._dp is not None:              # collectives are never captured: global-batch statistics need the eager step
            return self._dp.world == 1 or self._dp.batch_sync is None
        return self.grad_sync is None

    def train_step(self, inputs, labels):
        """One optimisation step (reference Trainer.py:700-726).  Returns the detached loss tensor."""
        inputs, labels = self._to_device(inputs, labels)
        self._attach_guard()
        self._attach_ema()
        if self._graph_capable(inputs):
            return self._graphed_train_step(inputs, labels)
        guarded_adam = self._guard is not None and "betas" in self.optimizer.param_groups[0]
        if guarded_adam:
            self._device_schedule()           # the step count advances on the device, and the poly rule with it
        loss = self._step_body(inputs, labels)
        if self.lr_scheduler and not guarded_adam:
            lr_ = self.base_lr * (1.0 - self.iter_num / self.max_iterations) ** 0.9
            for group in self.optimizer.param_groups:
                group['lr'] = lr_
        self.iter_num += 1
        return loss.detach()

    def _graphed_train_step(self, inputs, labels):
        from umi.graphs import GraphedStep
        self._device_schedule()
        if self._side is None:
            self._side = torch.cuda.Stream()
        flat = [inputs] + (list(labels) if isinstance(labels, (list, tuple)) else [labels])
        multi = isinstance(labels, (list, tuple))
        ratio = self._ratio_loop()
        key = tuple(tuple(t.shape) for t in flat)
        if ratio and self._gate_dev is None:       # the gate as a device flag: a captured kernel argument would freeze it
            self._gate_dev = torch.full((), float(self._ratio_gate), dtype=torch.float32, device=inputs.device)

        # data parallel over more than one rank: the graph holds forward + loss + backward with the reducer in deferred mode (the
        # tape fills the gradient buckets and launches no collective); the all-reduce and the optimizer step follow each replay
        deferred = self._dp is not None and self._dp.world > 1

        def body(x, *ys, deferred=False):
            loss = self._step_body(x, tuple(ys) if multi else ys[0], deferred)
            extra = (self._task_losses if multi else []) + ([self._ratio] if ratio else [])
            return (loss.detach(),) + tuple(t.detach() for t in extra)

        gs = self._graphs.get(key)
        if gs is None and key in self._seen_shapes:
            if deferred:
                self._dp.deferred = True
            try:                                                    # 2nd step of a shape: capture, replay
                gs = self._graphs[key] = GraphedStep((lambda *a: body(*a, deferred=True)) if deferred else body, flat, warmup=0,
                                                     optimizers=[self.optimizer])
            finally:
                if deferred:
                    self._dp.deferred = False                       # first steps of other shapes and ragged batches stay eager
        if gs is not None:
            outs = gs(*flat)
            if deferred:
                self._dp.flush()
                self.optimizer.step()
                if self._ema is not None:
                    self._ema.update()
        else:
            # first step of a batch shape (allocations, weight-pack caches) or a ragged batch: eager, on the side stream; its
            # outputs are detached, so no autograd graph of it survives into a later capture (umi/graphs.py)
            self._seen_shapes.add(key)
            self._side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self._side):
                outs = body(*flat)
            torch.cuda.current_stream().wait_stream(self._side)
        if multi:
            self._task_losses = [o.clone() for o in outs[1:3]]
        if ratio:
            self._ratio = outs[3].clone()
        self.iter_num += 1
        return outs[0].clone()            # the static output buffer is overwritten by the next replay

    def eval_step(self, inputs, labels):
        inputs, labels = self._to_device(inputs, labels, train=False)
        with torch.no_grad():
            out, loss = self._forward_loss(inputs, labels)
            if self.model_type in _MULTI:                        # the reference reports no validation score there (:853)
                return loss.detach(), torch.zeros((), device=loss.device)
            if self.val_confusion or self.accuracy_metric in SEG_METRICS:
                score = self._seg_scores(out, labels, 1, loss.reshape(1))[0]
            else:
                score = calc_loss(out, labels, loss_type=self.accuracy_metric)
        return loss.detach(), score.detach()

    # ---- hard-mask metrics ---------------------------------------------------------------
    def _seg_scores(self, out, labels, items, loss):
        """The [items] scores of a validation step with a hard-mask accuracy metric and / or val_confusion: ONE counting pass
        gives the per-item matrices; they are added into the static accumulator `_val_conf` (val_confusion) and scored.  No host
        synchronisation: part of what a GraphedEval captures.  `loss`: the [items] losses, the score when the names agree."""
        name = self.accuracy_metric
        seg = name in SEG_METRICS
        counts = seg_confusion_items(out, labels, items, SEG_METRICS[name][2] if seg else None)
        if self.val_confusion:
            if self._val_conf is None or (self._val_conf.shape, self._val_conf.device) != (counts.shape[1:], counts.device):
                if self._val_conf is not None and bool(self._val_conf.any()):
                    raise ValueError(f"val_confusion: the class count changed inside a validation phase ({self._val_conf.shape[0] - 1} "
                                     f"-> {counts.shape[1] - 1})")
                self._val_conf = torch.zeros_like(counts[0])             # only ever in an eager step (the first of a shape)
                self._eval_graphs, self._eval_seen = {}, set()           # (graphs hold the old accumulator's address)
            self._val_conf.add_(counts.sum(dim=0))
        if seg:
            return seg_scores(counts, name)
        return loss if name == self.loss_function else calc_loss_items(out, labels, items, loss_type=name)

    def _read_confusion(self):
        """After a validation phase: the dataset-level matrix (summed over the ranks under data parallel: int64, exact) to the
        host, once; per-class Dice / IoU of it."""
        from umi import metrics
        dp = self._dp is not None and self._dp.world > 1
        if dp:                                # a rank with an empty shard has no accumulator yet: agree on the size first
            import torch.distributed as dist
            size = torch.tensor([0 if self._val_conf is None else self._val_conf.shape[0]], dtype=torch.int64,
                                device=self._dp_device())
            dist.all_reduce(size, op=dist.ReduceOp.MAX, group=self._dp.group)
            if self._val_conf is None and int(size):
                self._val_conf = torch.zeros((int(size), int(size)), dtype=torch.int64, device=self._dp_device())
        if self._val_conf is None:
            return
        total = self._val_conf.clone()
        if dp:
            dist.all_reduce(total, op=dist.ReduceOp.SUM, group=self._dp.group)
        matrix = total.cpu().numpy()
        self.val_confusion_list.append(matrix)
        per_class = metrics.class_scores_numpy(matrix)
        self.val_class_scores = {"dice": per_class["dice"], "iou": per_class["iou"]}

    # ---- batched validation (val_batch=k) ------------------------------------------------
    def _val_group_fn(self, items):
        """The function of one validation group of `items` loader items laid end to end: f(x, *labels) runs ONE eval-mode
        forward, evaluates loss and score per item on that item's slice (loss.calc_loss_items), adds the rows [loss, score,
        task 1, task 2] to the running sums `self._val_sums` by `items` sequential adds in item order, and returns the
        [items, 4] rows.  No host synchronisation, one stream: it is what a umi.graphs.GraphedEval captures."""
        multi = self.model_type in _MULTI
        relu = self.model_type in ('regression', 'regression_t')

        def group(x, *ys):
            with torch.no_grad():
                if multi:                                        # as _forward_loss / eval_step: no validation score there
                    outs = tuple(F.relu(o) for o in self.model(x))
                    t1, t2 = (calc_loss_items(o, l, items, loss_type=self.loss_function) for o, l in zip(outs, ys))
                    loss, score = t1 + t2, torch.zeros_like(t1)
                else:
                    out = self.model(x)
                    if relu:
                        out = F.relu(out)
                    loss = calc_loss_items(out, ys[0], items, loss_type=self.loss_function)
                    if self.val_confusion or self.accuracy_metric in SEG_METRICS:
                        score = self._seg_scores(out, ys[0], items, loss)
                    else:
                        score = loss if self.accuracy_metric == self.loss_function else \
                            calc_loss_items(out, ys[0], items, loss_type=self.accuracy_metric)
                    t1 = t2 = torch.zeros_like(loss)
                rows = torch.stack([v.detach() for v in (loss, score, t1, t2)], dim=1)
                if self._val_sums is None or (self._val_sums.dtype, self._val_sums.device) != (rows.dtype, rows.device):
                    # the first group ever (always an eager one): sums of the losses' own dtype, as `loss_sum + loss` keeps them
                    self._val_sums = torch.zeros_like(rows[0])
                    self._eval_graphs, self._eval_seen = {}, set()       # (graphs hold the old vector's address)
                for i in range(items):                           # item order, one add each: the sums of the item-by-item loop
                    self._val_sums.add_(rows[i])
            return rows
        return group

    def _run_val_group(self, group):
        """group: [(inputs, labels)] of equal shapes, already through _to_device(train=False)."""
        items = len(group)
        multi = isinstance(group[0][1], (list, tuple))
        x = torch.cat([g[0] for g in group]) if items > 1 else group[0][0]
        if multi:
            ys = [torch.cat([g[1][j] for g in group]) if items > 1 else group[0][1][j] for j in range(len(group[0][1]))]
        else:
            ys = [torch.cat([g[1] for g in group]) if items > 1 else group[0][1]]
        flat, key = [x] + ys, None
        if self.graph and x.is_cuda and items == self.val_batch:
            key = tuple(tuple(t.shape) for t in flat)
            ge = self._eval_graphs.get(key)
            if ge is None and self._eval_capture_ok(key):        # 2nd full group of a shape: capture (nothing executes), replay
                from umi.graph import pack_cache_of
                from umi.graphs import GraphedEval
                ge = self._eval_graphs[key] = GraphedEval(self._val_group_fn(items), flat, pack_cache=pack_cache_of(self.model))
            if ge is not None:
                ge(*flat)
                return
        host = _loss.surface_host_calls()
        self._val_group_fn(items)(*flat)                         # 1st full group of a shape (allocations, pack entries), short
        if key is not None:                                      # groups, graph=False, CPU models: eager
            self._eval_note_eager(key, host)

    def _eval_note_eager(self, key, host_calls_before):
        """After the eager run of a full group of shapes `key`: seen once, or -- when a surface metric copied to the host in it
        (loss.surface_host_calls() moved) -- never to be captured."""
        if _loss.surface_host_calls() != host_calls_before:
            self._eval_host.add(key)
        else:
            self._eval_seen.add(key)

    def _eval_capture_ok(self, key):
        """Whether the next full group of shapes `key` may be captured: it ran eagerly once, without a host copy, and a surface
        metric would still take the kernels."""
        if key in self._eval_host or key not in self._eval_seen:
            return False
        return not (self.accuracy_metric in SURFACE_METRICS and not _loss.METRICS_KERNEL)

    def _validate_batched(self, bar, epoch, use_cuda, total_mem):
        """The validation phase under val_batch=k: loader items gathered into groups of up to k consecutive items of equal
        shapes (a shape change or the end of the loader closes a group early).  Returns (loss_sum, score_sum, steps,
        task_sums) as the item-by-item loop keeps them; `steps` counts loader items."""
        group, shapes, steps = [], None, 0
        if self._val_sums is not None:
            self._val_sums.zero_()

        def flush():
            if group:
                self._run_val_group(group)
                del group[:]

        for inputs, labels in bar:
            bar.set_description(f"Epoch {epoch}")
            steps += 1
            inputs, labels = self._to_device(inputs, labels, train=False)
            ls = labels if isinstance(labels, (list, tuple)) else (labels,)
            sh = (tuple(inputs.shape),) + tuple(tuple(l.shape) for l in ls)
            if group and sh != shapes:
                flush()
            shapes = sh
            group.append((inputs, labels))
            if len(group) == self.val_batch:
                flush()
                if not use_cuda or steps // 50 > (steps - self.val_batch) // 50:    # no device sync on every group
                    mem = f'{torch.cuda.memory_reserved() / 1E9 if use_cuda else 0:.3g}G/' + total_mem
                    bar.set_postfix(loss=float(self._val_sums[0]) / steps, memory=mem)
        flush()
        if not steps:
            return None, None, 0, [0.0, 0.0]
        sums = self._val_sums.clone()
        multi = self.model_type in _MULTI
        return sums[0], sums[1], steps, ([sums[2], sums[3]] if multi else [0.0, 0.0])

    # ------------------------------------------------------------------------------------
    def _check_ratio_scheduler(self):
        """The reference calls `self.lr_scheduler.step(val_score)` in the first validation after epoch 5 (Trainer.py:1282-1284);
        a truthy lr_scheduler without .step (train.py passes True) dies there with AttributeError."""
        if self.lr_scheduler and not callable(getattr(self.lr_scheduler, "step", None)) \
                and max(self.start_epoch, 6) <= self.num_epochs:
            raise NotImplementedError(
                f"multi_task_loss_ratio with lr_scheduler={self.lr_scheduler!r}: the reference loop calls lr_scheduler.step() "
                "in the first validation after epoch 5 and crashes there (AttributeError); pass a scheduler object, or None "
                "/ False, or stop at epoch 5")

    def _scheduler_step(self):
        """lr_scheduler.step(0.0) (the reference's val_score, Trainer.py:1284).  With the LR on the device (graph mode) the
        host copy is refreshed first and the scheduler's result is written back into the device block in place."""
        if self._dev_sched:
            self.optimizer.sync_host()
        self.lr_scheduler.step(0.0)
        if self._dev_sched:
            self.optimizer.push_lr()

    def multi_task_trainRatio(self):
        """Reference Trainer.multi_task_trainRatio (Trainer.py:1174-1366), see the module docstring."""
        self._check_ratio_scheduler()
        os.makedirs(self.output_save_dir, exist_ok=True)
        log = open(os.path.join(self.output_save_dir, "logs.txt"), 'a')

        def say(msg, echo=True):
            if echo:
                print(msg)
            log.write(msg + "\n")

        total_time = 0.0
        for epoch in range(self.start_epoch, self.num_epochs + 1):
            log.write('Epoch {}/{}\n'.format(epoch, self.num_epochs) + '-' * 10 + "\n")
            since = time.time()
            self._ratio_gate = epoch > 5
            if self._gate_dev is not None:
                self._gate_dev.fill_(float(self._ratio_gate))
            for phase in self.phases:
                train = phase == 'train'
                if train:
                    if self._dev_sched:
                        self.optimizer.sync_host()
                    for group in self.optimizer.param_groups:
                        print("LR", group['lr'])
                        log.write(f"LR {group['lr']}\n")
                    since = time.time()
                self.model.train(train)

                # device sums: loss, loss1, loss2 (fp64, as the reference's float += .item()), part1 = sum of loss1 + loss2
                # (fp64) and part2 = sum of fp32(loss1 + loss2) * ratioAccuracy (fp32, a tensor in the reference too)
                sums, steps = None, 0
                with tqdm(self.dataloader[phase], unit="batch") as bar:
                    for inputs, labels in bar:
                        bar.set_description(f"Epoch {epoch}")
                        steps += 1
                        loss = self.train_step(inputs, labels) if train else self.eval_step(inputs, labels)[0]
                        l1, l2 = (t.detach().double() for t in self._task_losses)
                        s12 = l1 + l2
                        acc = [loss.double(), l1, l2, s12, s12.float() * self._ratio.detach()]
                        sums = acc if sums is None else [a + b for a, b in zip(sums, acc)]
                loss_sum, sum1, sum2, part1, part2 = torch.stack([v.double() for v in sums]).tolist()
                epoch_loss = loss_sum / steps
                loss1_epoch = sum1 / steps / steps                  # divided by batch_step twice (Trainer.py:1275-1278)
                loss2_epoch = sum2 / steps / steps

                if not train:
                    if epoch <= 5:                                  # Trainer.py:1280-1281: nothing recorded yet
                        continue
                    if self.lr_scheduler:
                        self._scheduler_step()
                    self.val_loss_list.append(epoch_loss)
                    self.val_loss_list_1.append(loss1_epoch)
                    self.val_loss_list_2.append(loss2_epoch)
                    say("Val loss on epoch %i: %f" % (epoch, epoch_loss))
                    say("Val score on epoch %i: %f" % (epoch, 0.0))
                    if epoch_loss < self.best_val_score:
                        self.early_stop_counter = 0
                        self.best_val_score = epoch_loss
                        self.best_loss = epoch_loss
                        say("saving best model")
                        self.best_model = copy.deepcopy(self.model.state_dict())
                        torch.save(self.best_model, os.path.join(self.save_dir_model, 'epoch{}.pt'.format(epoch)))
                        torch.save(self.best_model, os.path.join(self.save_dir_model, 'best.pt'))
                    else:
                        self.early_stop_counter += 1
                    if self.early_stop_counter > self.patience:
                        say("Early stopping")
                        return self._finish(log, say)
                    continue

                elapsed = time.time() - since
                self.train_loss_list.append(epoch_loss)
                self.train_loss_list_1.append(loss1_epoch)
                self.train_loss_list_2.append(loss2_epoch)
                # alpha = (part1 / n) / (part2 / n) with the reference's roundings: part2 and the quotient are fp32 tensors
                with np.errstate(divide='ignore', invalid='ignore'):
                    self.alpha = float(np.float32(part1 / steps) / (np.float32(part2) / np.float32(steps)))
                self.alpha_list.append(self.alpha)
                say("Alpha on epoch %i: %f" % (epoch, self.alpha))
                say("Train loss on epoch %i: %f" % (epoch, epoch_loss))
                self._log_guard(say, epoch)
                total_time += elapsed
                self.meanTimePerEpoch = total_time / epoch
                torch.save(self.model.state_dict(), os.path.join(self.save_dir_model, 'last_epoch.pt'))

            elapsed = time.time() - since
            say('{:.0f}m {:.0f}s\n'.format(elapsed // 60, elapsed % 60))
        return self._finish(log, say)

    def multi_task_train(self):
        return self.singe_train()                                # same epoch loop; the differences are flagged `multi` below

    def singe_train(self):
        multi = self.model_type in _MULTI
        os.makedirs(self.output_save_dir, exist_ok=True)
        main = self._main                     # data parallel: rank 0 alone writes files, prints and shows the progress bar
        first_epoch, resumed = self.start_epoch, None
        if self._resume_path is not None:
            if self._dp is not None and self._dp.world > 1:
                raise NotImplementedError("resume with data_parallel over more than one rank")
            self._attach_ema()                          # its tensors are part of the run state
            resumed = self._resume_from_file()          # raises before anything is modified; None: a fresh run
        log = open(os.path.join(self.output_save_dir, "logs.txt") if main else os.devnull, 'a')

        def say(msg, echo=True):
            if echo and main:
                print(msg)
            log.write(msg + "\n")

        if self._dp_note:
            say(self._dp_note)

        use_cuda = torch.cuda.is_available()
        total_mem = f'{torch.cuda.get_device_properties(0).total_memory / 1E9 if use_cuda else 0:.3g}G'
        total_time = 0.0
        if resumed is not None:
            say("Resumed after epoch %i from %s" % (resumed[0], self._resume_path))
            if resumed[1]:                              # the run was over: only its end is left to do
                return self._finish(log, say)
            first_epoch, total_time = resumed[0] + 1, self._total_time
        for epoch in range(first_epoch, self.num_epochs + 1):
            log.write('Epoch {}/{}\n'.format(epoch, self.num_epochs) + '-' * 10 + "\n")
            since = time.time()
            for phase in self.phases:
                train = phase == 'train'
                if train:
                    if self._dev_sched:
                        self.optimizer.sync_host()          # the LR lives on the device in graph mode
                    for group in self.optimizer.param_groups:
                        if main:
                            print("LR", group['lr'])
                        log.write(f"LR {group['lr']}\n")
                    since = time.time()
                self.model.train(train)
                self._dp_phase(train)
                averaged = not train and self._ema is not None and self._ema_validate
                if averaged:                  # validate, select and save the averaged weights, in place (after the broadcast)
                    self._ema.swap()
                if not train and self._val_conf is not None:
                    self._val_conf.zero_()

                loss_sum, score_sum, steps = None, None, 0
                task_sums = [0.0, 0.0]
                with tqdm(self.dataloader[phase], unit="batch", disable=not main) as bar:
                    if not train and self.val_batch is not None:
                        loss_sum, score_sum, steps, task_sums = self._validate_batched(bar, epoch, use_cuda, total_mem)
                        bar = ()
                    for inputs, labels in bar:
                        bar.set_description(f"Epoch {epoch}")
                        steps += 1
                        if train:
                            loss = self.train_step(inputs, labels)
                        else:
                            loss, score = self.eval_step(inputs, labels)
                            score_sum = score if score_sum is None else score_sum + score
                        loss_sum = loss if loss_sum is None else loss_sum + loss
                        if multi:
                            task_sums = [s_ + l_.detach() for s_, l_ in zip(task_sums, self._task_losses)]
                        if steps % 50 == 0 or not use_cuda:     # avoid a device sync on every step
                            mem = f'{torch.cuda.memory_reserved() / 1E9 if use_cuda else 0:.3g}G/' + total_mem
                            bar.set_postfix(loss=float(loss_sum) / steps, memory=mem)
                if self._dp is not None:
                    # global sums over global step counts (a rank's validation shard may be shorter, or empty)
                    loss_sum, score_sum, steps, *task_sums = self._dp_reduce(
                        [float(loss_sum) if steps else 0.0, float(score_sum) if score_sum is not None else 0.0, float(steps),
                         float(task_sums[0]), float(task_sums[1])])
                epoch_loss = float(loss_sum) / steps

                if train:
                    elapsed = time.time() - since
                    say('Training Time for this epoch: {:.0f}m {:.0f}s\n'.format(elapsed // 60, elapsed % 60))
                    self.train_loss_list.append(epoch_loss)
                    if multi:
                        self.train_loss_list_1.append(float(task_sums[0]) / steps)
                        self.train_loss_list_2.append(float(task_sums[1]) / steps)
                    say("Train loss on epoch %i: %f" % (epoch, epoch_loss))
                    self._log_guard(say, epoch)
                    self._log_ema(say, epoch)
                    total_time += elapsed
                    self._total_time = total_time
                    self.meanTimePerEpoch = total_time / epoch
                    say('Curent mean training time per epoch: {:.0f}m {:.0f}s\n'.format(
                        self.meanTimePerEpoch // 60, self.meanTimePerEpoch % 60))
                    if main and self._ckpt_async():
                        self._save_last(os.path.join(self.save_dir_model, 'last_epoch.pt'))
                    elif main:
                        torch.save(self.model.state_dict(), os.path.join(self.save_dir_model, 'last_epoch.pt'))
                    self._dp_verify()                       # the replicas still agree, bit for bit (one word per rank)
                    continue

                val_score = float(score_sum) / steps
                if self.val_confusion:
                    self._read_confusion()
                if multi:
                    self.val_loss_list_1.append(float(task_sums[0]) / steps)
                    self.val_loss_list_2.append(float(task_sums[1]) / steps)
                self.val_loss_list.append(epoch_loss)
                self.val_score_list.append(val_score)
                say("Val loss on epoch %i: %f" % (epoch, epoch_loss))
                say("Val score on epoch %i: %f" % (epoch, val_score))
                selector = epoch_loss if multi else val_score   # multi-task: best model by validation loss (:926)
                if selector < self.best_val_score:
                    self.early_stop_counter = 0
                    self.best_val_score = selector
                    self.best_loss = epoch_loss
                    say("saving best model")
                    if self._ckpt_async():
                        self._save_best([os.path.join(self.save_dir_model, n) for n in ('epoch{}.pt'.format(epoch), 'best.pt')]
                                        if main else [])
                    else:
                        self.best_model = copy.deepcopy(self.model.state_dict())  # on every rank: train() returns it everywhere
                        self._best_views = False
                    if main and not self._ckpt_async():
                        torch.save(self.best_model, os.path.join(self.save_dir_model, 'epoch{}.pt'.format(epoch)))
                        torch.save(self.best_model, os.path.join(self.save_dir_model, 'best.pt'))
                else:
                    self.early_stop_counter += 1
                if averaged:                  # the live weights back, bit for bit
                    self._ema.swap()
                stop = self.early_stop_counter > self.patience
                if self._resume_path is not None and main:
                    self._write_run_state(epoch, stop or epoch == self.num_epochs)
                if stop:
                    say("Early stopping")
                    return self._finish(log, say)

            elapsed = time.time() - since
            say('{:.0f}m {:.0f}s\n'.format(elapsed // 60, elapsed % 60))
        return self._finish(log, say)

    def _finish(self, log, say):
        say('Best val loss: {:4f}'.format(self.best_loss))
        say('Best val score: {:4f}'.format(self.best_val_score))
        log.close()
        if self._main:
            self.plot_loss_functions('total')
        self._dp_end()
        if self.best_model:
            self.model.load_state_dict(self.best_model)     # load best model weights
        return self.model

    def plot_loss_functions(self, name):
        """Train/val loss curves -> <output_save_dir>/<name>.png (reference Trainer.py:52-111)."""
        import matplotlib
        matplotlib.use("Agg", force=False)
        import matplotlib.pyplot as plt
        fig, ax = plt.subplots(figsize=(8, 5))
        ep = range(1, len(self.train_loss_list) + 1)
        ax.plot(ep, self.train_loss_list, label='train loss')
        if self.val_loss_list:
            ax.plot(range(1, len(self.val_loss_list) + 1), self.val_loss_list, label='validation loss')
        ax.set_xlabel('epoch')
        ax.set_ylabel('loss')
        ax.legend()
        fig.savefig(os.path.join(self.output_save_dir, name + '.png'))
        plt.close(fig)
