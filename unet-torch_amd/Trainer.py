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
`Trainer(..., data_parallel=...)` (keyword-only; None / False, True, a dict of `umi.ddp.GradReducer` arguments or a GradReducer):
one run over the ranks of a process group, with a device replica check; rank 0 writes the files.  See umi/dp_run.py.
`Trainer(..., val_batch=k)` (keyword-only; None or an int >= 1): validation over groups of k loader items in one forward, replayed
from a graph under graph=True, every figure as the item-by-item loop gives it.  See umi/val_batch.py.
`Trainer(..., val_confusion=True)` (keyword-only; the single-output model types) keeps each validation phase's confusion matrix in
`val_confusion_list` and its per-class scores in `val_class_scores`; the hard-mask metrics of `loss.SEG_METRICS` and the
surface-distance metrics of `loss.SURFACE_METRICS` work as `accuracy_metric` in every validation path.  See umi/val_batch.py.
`Trainer(..., async_checkpoints=True)` (keyword-only): the checkpoint files come from one device snapshot per epoch and a writer
thread.  `Trainer(..., resume=True | path)` (keyword-only): the run state is written after every epoch and a cut run continues
from it, bit for bit; `snapshot_run_state()` / `restore_run_state()` roll a live run back in place.  See umi/run_state.py.
`Trainer(..., ema=...)` (keyword-only; None / False, True, a float, `dict(decay=0.999, warmup=True, validate=True)` or a
`umi.ema.ModelEMA`): an exponential moving average of the weights, updated inside the step and, with `validate`, validated and
saved in place of the live weights.  See umi/ema.py.
`Trainer(..., lr_schedule=dict(kind='cosine' | 'poly' | 'constant', warmup=0, power=0.9, final_ratio=0.0, max_iterations=None))`
(keyword-only; not together with a truthy `lr_scheduler`): linear warm-up and decay per step, `umi.optim.schedule_lr`, with each
param group's own `lr` as its base and `iter_num` counted across epochs (and carried by `resume`).  `max_iterations` defaults to
num_epochs * len(train loader).  With a `umi.optim` optimizer the rule always lives in the device block
(`optimizer.device_schedule(schedule=...)`), eager or replayed; with a torch optimizer the Trainer writes
`param_groups[i]['lr']` on the host before each step.
`Trainer(..., accumulate=k)` (keyword-only; None or 1: off, nothing of it is built; an int >= 2): one optimizer step over the mean
gradient of a window of k consecutive training batches of an epoch (the last window of an epoch may be shorter), summed on the
device by `umi.accum.GradAccumulator` in one launch per micro-batch; `train_step(inputs, labels, last=None)` steps on the last
micro-batch of a window.  `iter_num`, both learning-rate rules, Adam's step count, the guard's `steps` and the EMA's updates count
optimizer steps, `max_iterations` defaults to num_epochs * ceil(len(train loader) / k), epoch losses stay means over batches;
BatchNorm statistics are per micro-batch.  One line in `logs.txt` per run: `Gradient accumulation: K micro-batches per optimizer
step, S optimizer steps per epoch`.  See umi/accum.py.
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

from loss import SEG_METRICS, SURFACE_METRICS, calc_loss, multi_task_ratio_loss

_SINGLE = ('single', 'TransUnet', 'regression', 'regression_t', 'attention')
_TOPO = ('TopoCount', 'TopoCount2', 'TopoLoss', 'TopoLoss2', 'MyTopoLoss1', 'MyTopoLoss2', 'MyTopoLossGraph',
         'MyTopoLossVR')
_MULTI = ('multi_task', 'multi_task_reg', 'multi_task_regTU')
_OTHER = ('CLTR',)


class Trainer():
    def __init__(self, model, model_type, dtype, device, output_save_dir, dataloaders, batch_size, optimizer,
                 patience, num_epochs, loss_function, accuracy_metric, lr_scheduler=None, start_epoch=1, *, graph=None,
                 batch_transform=None, grad_guard=None, data_parallel=None, val_batch=None, val_confusion=False,
                 async_checkpoints=False, resume=None, ema=None, lr_schedule=None, accumulate=None):
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
        # gradient accumulation: micro-batches per optimizer step (0: off), the umi.accum.GradAccumulator (built by the first
        # step, and only when on) and the host count of the open window.  Every count below is in OPTIMIZER steps
        self._accum_k, self._accum, self._window = self._parse_accumulate(accumulate), None, 0
        if self._accum_k:
            self.max_iterations = self.num_epochs * -(-len(self.dataloader['train']) // self._accum_k)
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
        # warm-up + decay rule: the checked dict (None: off) and each param group's base LR
        self._lr_schedule, self._sched_base = None, [g['lr'] for g in self.optimizer.param_groups]
        if lr_schedule is not None:
            if lr_scheduler:
                raise ValueError("lr_schedule and lr_scheduler are two learning-rate rules: pass one of them")
            from umi.optim import check_schedule
            if isinstance(lr_schedule, dict) and 'iter_num' in lr_schedule:
                raise ValueError("lr_schedule: iter_num is the Trainer's own count (Trainer.iter_num), not a setting")
            self._lr_schedule = check_schedule(lr_schedule, "Trainer(lr_schedule=...)", max_iterations=self.max_iterations)
            del self._lr_schedule['iter_num']
        self._guard, self._guard_seen = self._make_guard(grad_guard), (0, 0)
        # multi_task_trainRatio: epoch > 5 (host, and in graph mode a device flag), ratioAccuracy of the last step
        self._ratio_gate, self._gate_dev, self._ratio = False, None, None
        self.alpha, self.alpha_list = None, []
        self._total_time = 0.0
        # the collaborators.  Data parallel exists only when asked for; validation and run state are built on first use
        # (_validation(), _run_state()), so a run with every keyword at its default loads neither module
        self._dp = None
        if data_parallel is not None and data_parallel is not False:
            from umi.dp_run import DataParallelRun
            self._dp = DataParallelRun(self, data_parallel)
        if val_batch is not None and (isinstance(val_batch, bool) or not isinstance(val_batch, int) or val_batch < 1):
            raise ValueError(f"val_batch takes None or a positive int, not {val_batch!r}")
        self.val_batch = val_batch
        if loss_function in SEG_METRICS:
            raise ValueError(f"loss_function {loss_function!r} is a hard-mask metric: not differentiable, use it as accuracy_metric")
        if loss_function in SURFACE_METRICS:
            raise ValueError(f"loss_function {loss_function!r} is a surface-distance metric: not differentiable, use it as "
                             "accuracy_metric")
        if val_confusion and model_type not in _SINGLE:
            raise ValueError(f"val_confusion covers the single-output model types {_SINGLE}, not {model_type!r}")
        self.val_confusion = bool(val_confusion)
        self.val_confusion_list, self.val_class_scores, self._val = [], None, None
        self.async_checkpoints = bool(async_checkpoints)
        self._resume, self._run = resume, None
        if resume is not None and resume is not False:
            self._run_state()                 # the path is resolved here
        # weight average: the ModelEMA arguments (or a ready ModelEMA) until the first step, then the ModelEMA; whether the
        # validation phase runs on the averaged weights
        self._ema_spec, self._ema_validate = self._parse_ema(ema)
        self._ema = None

        self.save_dir_model = os.path.join(self.output_save_dir, 'models/')
        os.makedirs(self.save_dir_model, exist_ok=True)

    def _validation(self):
        if self._val is None:
            from umi.val_batch import Validation
            self._val = Validation(self)
        return self._val

    def _run_state(self):
        if self._run is None:
            from umi.run_state import RunState
            self._run = RunState(self, self._resume)
        return self._run

    _LISTS = ('train_loss_list', 'val_loss_list', 'val_score_list', 'train_loss_list_1', 'train_loss_list_2', 'val_loss_list_1',
              'val_loss_list_2', 'alpha_list')
    RUN_STATE_FORMAT = 1

    def snapshot_run_state(self):
        """The whole training state into one device arena, between two steps of a live run (umi/run_state.py)."""
        if self._window:
            raise RuntimeError(f"snapshot_run_state() inside an open accumulation window ({self._window} of {self._accum_k} "
                               "micro-batches): the accumulators are not part of the run state; close the window first")
        return self._run_state().snapshot()

    def restore_run_state(self):
        """The state of the last snapshot_run_state() back, in place."""
        self._run_state().restore()
        if self._accum_k:                     # an open window is dropped: the snapshot was taken with the window closed
            self._window = 0
            if self._accum is not None:
                self._accum.reset()

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

    @staticmethod
    def _parse_accumulate(k):
        """`accumulate` -> micro-batches per optimizer step, 0 for off (None or 1).  ValueError on anything else."""
        if k is None:
            return 0
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError(f"accumulate takes None or an int >= 1 (1 = off), not {k!r}")
        return 0 if k == 1 else k

    @property
    def accumulator(self):
        """The umi.accum.GradAccumulator of this run (None: `accumulate` is off, or no step has run yet)."""
        return self._accum

    def _attach_accum(self):
        """Before the first step of a run with `accumulate`: the accumulator over the model's parameters."""
        if self._accum_k and self._accum is None:
            from umi.accum import GradAccumulator
            self._accum = GradAccumulator(self.model, self._accum_k)

    def _accum_refusals(self):
        if not self._accum_k:
            return
        if self._ratio_loop():
            raise NotImplementedError("accumulate with multi_task_loss_ratio: the count-ratio loop is not covered")
        spec = None if self._dp is None else self._dp.spec
        if (isinstance(spec, dict) and spec.get("global_batch")) or getattr(spec, "batch_sync", None) is not None:
            raise NotImplementedError("accumulate with data_parallel global_batch=True: the statistics collectives of every "
                                      "micro-batch are not covered")

    def _log_accum(self, say):
        if self._accum_k:
            say("Gradient accumulation: %i micro-batches per optimizer step, %i optimizer steps per epoch"
                % (self._accum_k, -(-len(self.dataloader['train']) // self._accum_k)))

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
        if not self._dev_sched and self._lr_schedule is not None:
            self.optimizer.device_schedule(schedule=dict(self._lr_schedule, iter_num=self.iter_num))
            self._dev_sched = True
        if not self._dev_sched:
            poly = dict(base_lr=self.base_lr, max_iterations=self.max_iterations, power=0.9, iter_num=self.iter_num)
            self.optimizer.device_schedule(poly=poly if self.lr_scheduler else None)
            self._dev_sched = True

    def _schedule_on_device(self, on_device):
        """lr_schedule with a umi.optim optimizer: the rule lives in the device block, in the eager step too."""
        return self._lr_schedule is not None and on_device and hasattr(self.optimizer, "device_schedule")

    def _host_schedule(self):
        """lr_schedule with a torch optimizer: the LR of step `iter_num` into every param group, before the step."""
        from umi.optim import schedule_lr
        for group, base in zip(self.optimizer.param_groups, self._sched_base):
            group['lr'] = schedule_lr(self.iter_num, base, **self._lr_schedule)

    def _log_guard(self, say, epoch):
        if self._guard is None:
            return
        r = self._guard.read()
        say("Guard on epoch %i: skipped %i, clipped %i, loss scale %g"
            % (epoch, r["skipped"] - self._guard_seen[0], r["clipped"] - self._guard_seen[1], r["scale"]))
        self._guard_seen = (r["skipped"], r["clipped"])

    @property
    def _main(self):
        """Rank 0 (or no data parallel): the rank that writes files and prints."""
        return self._dp is None or self._dp.rank == 0

    def _model_device(self):
        p = next(self.model.parameters(), None)
        return p.device if p is not None else torch.device("cpu")

    def _ckpt_async(self):
        return self.async_checkpoints and self._model_device().type == "cuda"

    # ------------------------------------------------------------------------------------
    def train(self):
        if self._ema_spec is not None and self._ratio_loop():
            raise NotImplementedError("ema with multi_task_loss_ratio: the count-ratio loop is not covered")
        self._accum_refusals()
        if not self.async_checkpoints and self._run is None:
            return self._train_dp()
        run = self._run_state()
        run.refusals()
        try:
            return self._train_dp()
        finally:
            run.close()                       # every queued file is on disk, or its error is raised here

    def _train_dp(self):
        if self._dp is None:
            return self._train()
        try:
            self._dp.begin()
            return self._train()
        finally:
            self._dp.end()

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

    def _activated(self, inputs):
        """The model's outputs as the losses take them: both heads of a multi-task model through ReLU, as a tuple (reference
        Trainer.py:882-884), a regression model's output through ReLU, any other output as it is."""
        out = self.model(inputs)
        if self.model_type in _MULTI:
            return tuple(F.relu(o) for o in out)
        return F.relu(out) if self.model_type in ('regression', 'regression_t') else out

    def _forward_loss(self, inputs, labels):
        if self._ratio_loop():                                   # reference Trainer.py:1226-1249
            o1, o2 = self.model(inputs)
            gate = self._ratio_gate if self._gate_dev is None else self._gate_dev
            loss, loss1, loss2, self._ratio = multi_task_ratio_loss(o1, o2, labels[0], labels[1], gate)
            self._task_losses = [loss1, loss2]
            return (o1, o2), loss
        out = self._activated(inputs)
        if self.model_type in _MULTI:                            # reference Trainer.py:885-890
            self._task_losses = [calc_loss(o, l, loss_type=self.loss_function) for o, l in zip(out, labels)]
            return out, self._task_losses[0] + self._task_losses[1]
        return out, calc_loss(out, labels, loss_type=self.loss_function)

    def _accum_step_body(self, inputs, labels, deferred, last):
        """A step of a run with `accumulate`: the micro-step (forward, loss, zero_grad, backward, add) and, on the `last`
        micro-batch of a window, the tail of _step_body on the window's mean gradient.  Under a reducer every backward pass runs
        in its deferred mode, so a window costs one set of collectives."""
        reducer = None if self._dp is None else self._dp.reducer
        with torch.set_grad_enabled(True):
            _, loss = self._forward_loss(inputs, labels)
            self.optimizer.zero_grad()
            if reducer is not None:
                reducer.deferred = True       # the tape fills the buckets and launches nothing
            try:
                loss.backward()
            finally:
                if reducer is not None:
                    reducer.deferred = False
            filled = reducer is not None and reducer._marked
            self._accum.add(last=last)        # on the bucket views where the tape filled them, else on .grad
            if not last:
                if filled:
                    reducer.reset()
                return loss
            if deferred:                      # captured data-parallel step: flush() and optimizer.step() follow each replay
                return loss
            if filled:
                reducer.flush()               # the window's collectives; .grad -> the bucket slots
            elif self.grad_sync is not None:
                self.grad_sync()
            self.optimizer.step()
            if self._ema is not None:
                self._ema.update()
        return loss

    def _step_body(self, inputs, labels, deferred=False, last=True):
        if self._accum is not None:
            return self._accum_step_body(inputs, labels, deferred, last)
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
        reducer = None if self._dp is None else self._dp.reducer     # of a data-parallel train() in progress
        if reducer is not None:               # collectives are never captured: global-batch statistics need the eager step
            return reducer.world == 1 or reducer.batch_sync is None
        return self.grad_sync is None

    def train_step(self, inputs, labels, *, last=None):
        """One optimisation step (reference Trainer.py:700-726).  Returns the detached loss tensor.
        With `accumulate`: one micro-batch; the optimizer steps when it is the `last` of its window (None: the Trainer's own
        count, every `accumulate`-th call; True closes the window now).  Without it `last` is not looked at."""
        inputs, labels = self._to_device(inputs, labels)
        self._attach_guard()
        self._attach_ema()
        if self._accum_k:
            self._attach_accum()
            return self._accum_train_step(inputs, labels, self._window + 1 >= self._accum_k if last is None else bool(last))
        if self._graph_capable(inputs):
            return self._graphed_train_step(inputs, labels)
        guarded_adam = self._guard is not None and "betas" in self.optimizer.param_groups[0]
        if guarded_adam or self._schedule_on_device(inputs.is_cuda):
            self._device_schedule()           # the step count advances on the device, and the LR rule with it
        elif self._lr_schedule is not None:
            self._host_schedule()
        loss = self._step_body(inputs, labels)
        if self.lr_scheduler and not guarded_adam:
            lr_ = self.base_lr * (1.0 - self.iter_num / self.max_iterations) ** 0.9
            for group in self.optimizer.param_groups:
                group['lr'] = lr_
        self.iter_num += 1
        return loss.detach()

    def _accum_train_step(self, inputs, labels, last):
        """train_step of a run with `accumulate`: iter_num and the learning-rate rules move with the optimizer step."""
        if self._graph_capable(inputs):
            loss = self._graphed_train_step(inputs, labels, last)
            self._window = 0 if last else self._window + 1
            self._accum.position = self._window               # (a replay does not pass through add())
            return loss
        guarded_adam = self._guard is not None and "betas" in self.optimizer.param_groups[0]
        if guarded_adam or self._schedule_on_device(inputs.is_cuda):
            self._device_schedule()
        elif self._lr_schedule is not None:
            self._host_schedule()
        loss = self._step_body(inputs, labels, last=last)
        self._window = 0 if last else self._window + 1
        if last:
            if self.lr_scheduler and not guarded_adam:
                lr_ = self.base_lr * (1.0 - self.iter_num / self.max_iterations) ** 0.9
                for group in self.optimizer.param_groups:
                    group['lr'] = lr_
            self.iter_num += 1
        return loss.detach()

    def _graphed_train_step(self, inputs, labels, last=True):
        from umi.graphs import GraphedStep
        self._device_schedule()
        if self._side is None:
            self._side = torch.cuda.Stream()
        flat = [inputs] + (list(labels) if isinstance(labels, (list, tuple)) else [labels])
        multi = isinstance(labels, (list, tuple))
        ratio = self._ratio_loop()
        key = tuple(tuple(t.shape) for t in flat)
        if self._accum is not None:           # two graphs per batch shape: the micro-step and the final step
            key += (("final",) if last else ("micro",),)
        if ratio and self._gate_dev is None:       # the gate as a device flag: a captured kernel argument would freeze it
            self._gate_dev = torch.full((), float(self._ratio_gate), dtype=torch.float32, device=inputs.device)

        # data parallel over more than one rank: the graph holds forward + loss + backward with the reducer in deferred mode (the
        # tape fills the gradient buckets and launches no collective); the all-reduce and the optimizer step follow each replay
        reducer = None if self._dp is None else self._dp.reducer
        deferred = reducer is not None and reducer.world > 1

        def body(x, *ys, deferred=False):
            loss = self._step_body(x, tuple(ys) if multi else ys[0], deferred, last)
            extra = (self._task_losses if multi else []) + ([self._ratio] if ratio else [])
            return (loss.detach(),) + tuple(t.detach() for t in extra)

        gs = self._graphs.get(key)
        if gs is None and key in self._seen_shapes:
            if deferred:
                reducer.deferred = True
            try:                                                    # 2nd step of a shape: capture, replay
                gs = self._graphs[key] = GraphedStep((lambda *a: body(*a, deferred=True)) if deferred else body, flat, warmup=0,
                                                     optimizers=[self.optimizer])
            finally:
                if deferred:
                    reducer.deferred = False                        # first steps of other shapes and ragged batches stay eager
        if gs is not None:
            outs = gs(*flat)
            if deferred and last:
                reducer.flush()
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
        if last:
            self.iter_num += 1
        return outs[0].clone()            # the static output buffer is overwritten by the next replay

    def eval_step(self, inputs, labels):
        inputs, labels = self._to_device(inputs, labels, train=False)
        with torch.no_grad():
            out, loss = self._forward_loss(inputs, labels)
            if self.model_type in _MULTI:                        # the reference reports no validation score there (:853)
                return loss.detach(), torch.zeros((), device=loss.device)
            if self.val_confusion or self.accuracy_metric in SEG_METRICS:
                score = self._validation().seg_scores(out, labels, 1, loss.reshape(1))[0]
            else:
                score = calc_loss(out, labels, loss_type=self.accuracy_metric)
        return loss.detach(), score.detach()

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

    def _open_log(self):
        """(log, say): `logs.txt` opened for appending, and say(msg, echo=True), which writes a line to it and prints it.  Data
        parallel: rank 0 alone writes files and prints."""
        os.makedirs(self.output_save_dir, exist_ok=True)
        main = self._main
        log = open(os.path.join(self.output_save_dir, "logs.txt") if main else os.devnull, 'a')

        def say(msg, echo=True):
            if echo and main:
                print(msg)
            log.write(msg + "\n")
        return log, say

    def _print_lr(self, log):
        if self._schedule_on_device(self._model_device().type == "cuda"):
            self._device_schedule()           # the LR of the next step is the rule's, before the first step too
        elif self._lr_schedule is not None and not self._dev_sched:
            self._host_schedule()
        if self._dev_sched:
            self.optimizer.sync_host()        # the LR lives on the device in graph mode
        for group in self.optimizer.param_groups:
            if self._main:
                print("LR", group['lr'])
            log.write(f"LR {group['lr']}\n")

    def _save_best_sync(self, epoch):
        """A new best model without a snapshot: a deepcopy on every rank (train() returns it everywhere), the files on rank 0."""
        self.best_model = copy.deepcopy(self.model.state_dict())
        if self._run is not None:
            self._run.best_views = False
        if self._main:
            torch.save(self.best_model, os.path.join(self.save_dir_model, 'epoch{}.pt'.format(epoch)))
            torch.save(self.best_model, os.path.join(self.save_dir_model, 'best.pt'))

    def multi_task_trainRatio(self):
        """Reference Trainer.multi_task_trainRatio (Trainer.py:1174-1366), see the module docstring."""
        self._check_ratio_scheduler()
        log, say = self._open_log()
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
                    self._print_lr(log)
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
                        self._save_best_sync(epoch)
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
        main = self._main                     # data parallel: rank 0 alone writes files, prints and shows the progress bar
        dp = self._dp if self._dp is not None and self._dp.reducer is not None else None     # train() began one
        resume = self._run is not None and self._run.resume_path is not None
        first_epoch, resumed = self.start_epoch, None
        if resume:
            self._attach_ema()                          # its tensors are part of the run state
            resumed = self._run.resume()                # raises before anything is modified; None: a fresh run
        log, say = self._open_log()
        if dp is not None and dp.note:
            say(dp.note)
        self._log_accum(say)

        use_cuda = torch.cuda.is_available()
        total_mem = f'{torch.cuda.get_device_properties(0).total_memory / 1E9 if use_cuda else 0:.3g}G'
        total_time = 0.0
        if resumed is not None:
            say("Resumed after epoch %i from %s" % (resumed[0], self._run.resume_path))
            if resumed[1]:                              # the run was over: only its end is left to do
                return self._finish(log, say)
            first_epoch, total_time = resumed[0] + 1, self._total_time
        for epoch in range(first_epoch, self.num_epochs + 1):
            log.write('Epoch {}/{}\n'.format(epoch, self.num_epochs) + '-' * 10 + "\n")
            since = time.time()
            for phase in self.phases:
                train = phase == 'train'
                if train:
                    self._print_lr(log)
                    since = time.time()
                self.model.train(train)
                if dp is not None:
                    dp.phase(train)
                averaged = not train and self._ema is not None and self._ema_validate
                if averaged:                  # validate, select and save the averaged weights, in place (after the broadcast)
                    self._ema.swap()
                if not train and self._val is not None and self._val.conf is not None:
                    self._val.conf.zero_()

                loss_sum, score_sum, steps = None, None, 0
                task_sums = [0.0, 0.0]
                with tqdm(self.dataloader[phase], unit="batch", disable=not main) as bar:
                    if not train and self.val_batch is not None:
                        loss_sum, score_sum, steps, task_sums = self._validation().validate(bar, epoch, use_cuda, total_mem)
                        bar = ()
                    for inputs, labels in bar:
                        bar.set_description(f"Epoch {epoch}")
                        steps += 1
                        if train and self._accum_k:          # a window never spans two epochs
                            loss = self.train_step(inputs, labels, last=True if steps == len(self.dataloader[phase]) else None)
                        elif train:
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
                if dp is not None:
                    # global sums over global step counts (a rank's validation shard may be shorter, or empty)
                    loss_sum, score_sum, steps, *task_sums = dp.reduce(
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
                        self._run_state().save_last(os.path.join(self.save_dir_model, 'last_epoch.pt'))
                    elif main:
                        torch.save(self.model.state_dict(), os.path.join(self.save_dir_model, 'last_epoch.pt'))
                    if dp is not None:
                        dp.verify()                         # the replicas still agree, bit for bit (one word per rank)
                    continue

                val_score = float(score_sum) / steps
                if self.val_confusion:
                    self._validation().read_confusion()
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
                        self._run_state().save_best([os.path.join(self.save_dir_model, n)
                                                     for n in ('epoch{}.pt'.format(epoch), 'best.pt')] if main else [])
                    else:
                        self._save_best_sync(epoch)
                else:
                    self.early_stop_counter += 1
                if averaged:                  # the live weights back, bit for bit
                    self._ema.swap()
                stop = self.early_stop_counter > self.patience
                if resume and main:
                    self._run.write(epoch, stop or epoch == self.num_epochs)
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
        if self._dp is not None:
            self._dp.end()                    # the reducer is closed before the best weights are loaded
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
