"""The Trainer's validation beyond the item-by-item loop: groups of `val_batch` items in one forward, their graph replay, the
hard-mask confusion accumulator.  `Validation(trainer)` is built on first use (Trainer._validation()); it reads `val_batch`,
`val_confusion`, `graph` and the metric names from the Trainer.

`Trainer(..., val_batch=k)` (keyword-only, after `data_parallel`): None = the validation loop of singe_train, one `eval_step` per
loader item, untouched; an int k >= 1 = in singe_train's validation phase (multi_task_train included) loader items go through
`_to_device(train=False)` one by one as before (`batch_transform` included) and are gathered into groups of up to k CONSECUTIVE
items of EQUAL shapes -- a shape change or the end of the loader closes a group early.  One eval-mode forward runs over the
concatenated group; loss and score are then evaluated per item on that item's slice (`loss.calc_loss_items`: the loop over
`calc_loss`, or one `umi_dice_ce_fwd_items` pass for 'dice_bce_mc' on the fused kernels' inputs, same bits; the regression ReLU
and the two heads / per-task losses as in `_forward_loss`; computed once when loss_function == accuracy_metric), and the rows are
added to the running sums [loss, score, task 1, task 2] -- one device vector of the losses' dtype -- by k sequential adds in
item order.  `steps` counts loader items, so the epoch figures, the per-task lists, model selection, early stop, the log lines and
the data-parallel phase reduction see what the item-by-item loop gives them.  With graph=True and device inputs a FULL group
replays from a `umi.graphs.GraphedEval` kept in `graphs` by group shapes (the Trainer's `_graphs` stays the training graphs): the
first full group of a shape runs eagerly, the second is captured (forward, per-item values, the adds into the running sums),
short groups stay eager.
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
all-reduce, exact), appends it to `trainer.val_confusion_list` and keeps the per-class Dice / IoU of that dataset-level matrix in
`trainer.val_class_scores`.  When the accuracy metric is a hard-mask one the score comes from the same matrices (one pass).
`logs.txt`, the checkpoints and the other lists do not change; with `val_confusion=False` and another metric name none of
this runs.
The surface-distance metrics of `loss.SURFACE_METRICS` ('hd_mc', 'hd95_mc', 'assd_mc', 'hd', 'hd95', 'assd': Hausdorff distance,
its 95th percentile and the average symmetric surface distance of the argmax or threshold mask's foreground classes, in pixels,
lower is better; umi/surface.py) work as `accuracy_metric` in the same validation paths through `calc_loss` / `calc_loss_items`
(one kernel call per group).  The kernels take contiguous fp32 device logits with at most 8 channels and H, W <= 4096; on those
nothing allocates outside the caching allocator or synchronises, so a full group replays from its GraphedEval like any other.
Every other input (a 9-class model, `loss.METRICS_KERNEL = False`, ...) runs the NumPy statement on host copies, which
synchronises: a group whose first, eager run took that route is never captured and stays eager under `graph=True`
(`host`, decided by `loss.surface_host_calls()`), with the same scores, at the host's speed.  As `loss_function` they raise
ValueError.  With `val_confusion=True` the
confusion matrices take their own pass next to it.
"""
import torch

import loss as _loss
from loss import SEG_METRICS, SURFACE_METRICS, calc_loss_items, seg_confusion_items, seg_scores


class Validation:
    def __init__(self, trainer):
        # the eval graphs by group shapes, the shapes that ran eagerly once, the group shapes whose eager run copied to the host
        # (surface metrics' composite: never captured), the running sums [loss, score, task 1, task 2] (one vector of the losses'
        # dtype, where the model runs), and the static device accumulator of the confusion matrices
        self.t = trainer
        self.graphs, self.seen, self.host, self.sums, self.conf = {}, set(), set(), None, None

    # ---- hard-mask metrics ---------------------------------------------------------------
    def seg_scores(self, out, labels, items, loss):
        """The [items] scores of a validation step with a hard-mask accuracy metric and / or val_confusion: ONE counting pass
        gives the per-item matrices; they are added into the static accumulator `conf` (val_confusion) and scored.  No host
        synchronisation: part of what a GraphedEval captures.  `loss`: the [items] losses, the score when the names agree."""
        name = self.t.accuracy_metric
        seg = name in SEG_METRICS
        counts = seg_confusion_items(out, labels, items, SEG_METRICS[name][2] if seg else None)
        if self.t.val_confusion:
            if self.conf is None or (self.conf.shape, self.conf.device) != (counts.shape[1:], counts.device):
                if self.conf is not None and bool(self.conf.any()):
                    raise ValueError(f"val_confusion: the class count changed inside a validation phase ({self.conf.shape[0] - 1} "
                                     f"-> {counts.shape[1] - 1})")
                self.conf = torch.zeros_like(counts[0])                  # only ever in an eager step (the first of a shape)
                self.graphs, self.seen = {}, set()                       # (graphs hold the old accumulator's address)
            self.conf.add_(counts.sum(dim=0))
        if seg:
            return seg_scores(counts, name)
        return loss if name == self.t.loss_function else calc_loss_items(out, labels, items, loss_type=name)

    def read_confusion(self):
        """After a validation phase: the dataset-level matrix (summed over the ranks under data parallel: int64, exact) to the
        host, once; per-class Dice / IoU of it."""
        from . import metrics
        t = self.t
        reducer = t._dp.reducer if t._dp is not None else None
        dp = reducer is not None and reducer.world > 1
        if dp:                                # a rank with an empty shard has no accumulator yet: agree on the size first
            import torch.distributed as dist
            size = torch.tensor([0 if self.conf is None else self.conf.shape[0]], dtype=torch.int64, device=t._model_device())
            dist.all_reduce(size, op=dist.ReduceOp.MAX, group=reducer.group)
            if self.conf is None and int(size):
                self.conf = torch.zeros((int(size), int(size)), dtype=torch.int64, device=t._model_device())
        if self.conf is None:
            return
        total = self.conf.clone()
        if dp:
            dist.all_reduce(total, op=dist.ReduceOp.SUM, group=reducer.group)
        matrix = total.cpu().numpy()
        t.val_confusion_list.append(matrix)
        per_class = metrics.class_scores_numpy(matrix)
        t.val_class_scores = {"dice": per_class["dice"], "iou": per_class["iou"]}

    # ---- batched validation (val_batch=k) ------------------------------------------------
    def group_fn(self, items):
        """The function of one validation group of `items` loader items laid end to end: f(x, *labels) runs ONE eval-mode
        forward, evaluates loss and score per item on that item's slice (loss.calc_loss_items), adds the rows [loss, score,
        task 1, task 2] to the running sums `self.sums` by `items` sequential adds in item order, and returns the
        [items, 4] rows.  No host synchronisation, one stream: it is what a umi.graphs.GraphedEval captures."""
        t = self.t

        def group(x, *ys):
            with torch.no_grad():
                out = t._activated(x)
                if isinstance(out, tuple):                       # two heads, as _forward_loss / eval_step: no validation score
                    t1, t2 = (calc_loss_items(o, l, items, loss_type=t.loss_function) for o, l in zip(out, ys))
                    loss, score = t1 + t2, torch.zeros_like(t1)
                else:
                    loss = calc_loss_items(out, ys[0], items, loss_type=t.loss_function)
                    if t.val_confusion or t.accuracy_metric in SEG_METRICS:
                        score = self.seg_scores(out, ys[0], items, loss)
                    else:
                        score = loss if t.accuracy_metric == t.loss_function else \
                            calc_loss_items(out, ys[0], items, loss_type=t.accuracy_metric)
                    t1 = t2 = torch.zeros_like(loss)
                rows = torch.stack([v.detach() for v in (loss, score, t1, t2)], dim=1)
                if self.sums is None or (self.sums.dtype, self.sums.device) != (rows.dtype, rows.device):
                    # the first group ever (always an eager one): sums of the losses' own dtype, as `loss_sum + loss` keeps them
                    self.sums = torch.zeros_like(rows[0])
                    self.graphs, self.seen = {}, set()           # (graphs hold the old vector's address)
                for i in range(items):                           # item order, one add each: the sums of the item-by-item loop
                    self.sums.add_(rows[i])
            return rows
        return group

    def run_group(self, group):
        """group: [(inputs, labels)] of equal shapes, already through _to_device(train=False)."""
        items = len(group)
        multi = isinstance(group[0][1], (list, tuple))
        x = torch.cat([g[0] for g in group]) if items > 1 else group[0][0]
        if multi:
            ys = [torch.cat([g[1][j] for g in group]) if items > 1 else group[0][1][j] for j in range(len(group[0][1]))]
        else:
            ys = [torch.cat([g[1] for g in group]) if items > 1 else group[0][1]]
        flat, key = [x] + ys, None
        if self.t.graph and x.is_cuda and items == self.t.val_batch:
            key = tuple(tuple(v.shape) for v in flat)
            ge = self.graphs.get(key)
            if ge is None and self.capture_ok(key):              # 2nd full group of a shape: capture (nothing executes), replay
                from .graph import pack_cache_of
                from .graphs import GraphedEval
                ge = self.graphs[key] = GraphedEval(self.group_fn(items), flat, pack_cache=pack_cache_of(self.t.model))
            if ge is not None:
                ge(*flat)
                return
        host = _loss.surface_host_calls()
        self.group_fn(items)(*flat)                              # 1st full group of a shape (allocations, pack entries), short
        if key is not None:                                      # groups, graph=False, CPU models: eager
            self.note_eager(key, host)

    def note_eager(self, key, host_calls_before):
        """After the eager run of a full group of shapes `key`: seen once, or -- when a surface metric copied to the host in it
        (loss.surface_host_calls() moved) -- never to be captured."""
        if _loss.surface_host_calls() != host_calls_before:
            self.host.add(key)
        else:
            self.seen.add(key)

    def capture_ok(self, key):
        """Whether the next full group of shapes `key` may be captured: it ran eagerly once, without a host copy, and a surface
        metric would still take the kernels."""
        if key in self.host or key not in self.seen:
            return False
        return not (self.t.accuracy_metric in SURFACE_METRICS and not _loss.METRICS_KERNEL)

    def validate(self, bar, epoch, use_cuda, total_mem):
        """The validation phase under val_batch=k: loader items gathered into groups of up to k consecutive items of equal
        shapes (a shape change or the end of the loader closes a group early).  Returns (loss_sum, score_sum, steps,
        task_sums) as the item-by-item loop keeps them; `steps` counts loader items."""
        t = self.t
        group, shapes, steps, multi = [], None, 0, False
        if self.sums is not None:
            self.sums.zero_()

        def flush():
            if group:
                self.run_group(group)
                del group[:]

        for inputs, labels in bar:
            bar.set_description(f"Epoch {epoch}")
            steps += 1
            inputs, labels = t._to_device(inputs, labels, train=False)
            multi = isinstance(labels, (list, tuple))
            ls = labels if multi else (labels,)
            sh = (tuple(inputs.shape),) + tuple(tuple(l.shape) for l in ls)
            if group and sh != shapes:
                flush()
            shapes = sh
            group.append((inputs, labels))
            if len(group) == t.val_batch:
                flush()
                if not use_cuda or steps // 50 > (steps - t.val_batch) // 50:       # no device sync on every group
                    mem = f'{torch.cuda.memory_reserved() / 1E9 if use_cuda else 0:.3g}G/' + total_mem
                    bar.set_postfix(loss=float(self.sums[0]) / steps, memory=mem)
        flush()
        if not steps:
            return None, None, 0, [0.0, 0.0]
        sums = self.sums.clone()
        return sums[0], sums[1], steps, ([sums[2], sums[3]] if multi else [0.0, 0.0])
