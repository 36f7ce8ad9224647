"""The Trainer's snapshots: asynchronous checkpoints, the run-state file, the in-place roll-back.  `RunState(trainer, resume)`
is built on first use (Trainer._run_state()); with `async_checkpoints` and `resume` at their defaults none of this runs.

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
versions are bumped, so the kernel-layout weight copies are re-packed.
"""
import collections
import copy
import os

import numpy as np
import torch


def optim_walk(opt):
    """(index, parameter, its state or {}) over the optimizer's parameters, numbered as `optimizer.state_dict()` numbers them."""
    idx = 0
    for group in opt.param_groups:
        for p in group['params']:
            yield idx, p, (opt.state[p] if p in opt.state else {})
            idx += 1


def _moments(states):
    """(index, state) pairs -> 'index.key' -> tensor; Adam's step count is a host scalar (see host_fields)."""
    return {f'{idx}.{k}': v for idx, st in states for k, v in st.items() if torch.is_tensor(v) and k != 'step'}


def _drop_steps(model):
    return {name: m._drop_step for name, m in model.named_modules() if getattr(m, '_drop_step', None) is not None}


# The sections of the run state in file order: (prefix, name -> live tensor of a Trainer, name -> tensor of a payload).  The
# fingerprint word is taken over the tensors in this order.
SECTIONS = (
    ('model.', lambda t: t.model.state_dict(), lambda pl: pl['model']),
    ('optim.', lambda t: _moments((i, st) for i, _, st in optim_walk(t.optimizer)),
     lambda pl: _moments((i, pl['optimizer']['state'][i]) for i in sorted(pl['optimizer']['state']))),
    ('hyper.', lambda t: {str(gi): dev for gi, (dev, _) in enumerate(getattr(t.optimizer, 'device_hyper', None) or [])},
     lambda pl: {str(gi): h for gi, h in enumerate(pl['hyper'] or [])}),
    ('guard', lambda t: {'': t._guard.state} if t._guard is not None and t._guard.state is not None else {},
     lambda pl: {'': pl['guard']} if pl['guard'] is not None else {}),
    ('drop.', lambda t: _drop_steps(t.model), lambda pl: pl['drop_step']),
    ('ema.', lambda t: t._ema.tensors() if t._ema is not None else {}, lambda pl: pl.get('ema') or {}),
    ('best.', lambda t: t.best_model if isinstance(t.best_model, dict) else {}, lambda pl: pl['best_model'] or {}),
)


def _tensors(source, side, best=True):
    return collections.OrderedDict((prefix + k, v) for prefix, *get in SECTIONS if best or prefix != 'best.'
                                   for k, v in get[side](source).items())


def payload_tensors(pl):
    """name -> tensor of a run-state payload, in the order of state_tensors: what the fingerprint word is taken over."""
    return _tensors(pl, 1)


def tensor_key(tensors):
    """What identifies a set of live tensors: (name, address, bytes) of each."""
    return tuple((k, v.data_ptr(), v.numel() * v.element_size()) for k, v in tensors.items())


def host_word(host):
    """One fingerprint word over the host fields: the tensors among them (bytes, zero-padded to whole words) and the text of
    everything else."""
    from .ddp import fingerprint_numpy
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


class RunState:
    def __init__(self, trainer, resume=None):
        self.t = trainer
        if resume is None or resume is False:
            self.resume_path = None
        elif resume is True:
            self.resume_path = os.path.join(trainer.output_save_dir, 'run_state.pt')
        else:
            self.resume_path = os.fspath(resume)
        # the writer thread; the Snapshots (key, Snapshot) of 'last_epoch.pt', the best model, the file and the roll-back; the
        # roll-back's host side; whether `best_model` is the views of an arena; the event of 'last_epoch.pt''s host copy
        self.writer, self.snaps, self.run_host, self.best_views, self.ckpt_event = None, {}, None, False, None

    def refusals(self):
        """Before anything runs: what `resume` does not cover."""
        t = self.t
        if self.resume_path is None:
            return
        if t._ratio_loop():
            raise NotImplementedError("resume with multi_task_loss_ratio: the loop's alpha and gate bookkeeping is its own and is "
                                      "not part of the run state")
        if t._dp is not None and (t._dp.world_of(t._dp.spec) or 1) > 1:      # no process group: one rank
            raise NotImplementedError("resume with data_parallel over more than one rank: the per-rank random-generator states "
                                      "are not collected (a world of one works)")

    def close(self):
        w, self.writer = self.writer, None
        if w is not None:
            w.close()

    def snap_for(self, slot, tensors):
        """The Snapshot kept under `slot` for exactly these live tensors (built again when one of them moved)."""
        from .snapshot import Snapshot
        key = tensor_key(tensors)
        have = self.snaps.get(slot)
        if have is None or have[0] != key:
            have = self.snaps[slot] = (key, Snapshot(tensors))
        return have[1]

    def submit(self, snap, event, obj, path):
        if self.writer is None:
            from .snapshot import CheckpointWriter
            self.writer = CheckpointWriter()
        self.writer.submit(event, obj, path, snap.hold_host())

    def save_last(self, path):
        """'last_epoch.pt' after a training phase: one take() on the training stream; the copy to the host and the write run
        beside what follows."""
        snap = self.snap_for('ckpt', self.t.model.state_dict())
        snap.take()
        self.ckpt_event = snap.to_host_async()
        self.submit(snap, self.ckpt_event, snap.host_views(), path)

    def save_best(self, paths):
        """A new best model: `best_model` becomes the views of a second arena (one launch instead of a deepcopy); the files come
        from the host copy that 'last_epoch.pt' of this epoch was taken from (a validation phase changes no weight or buffer)."""
        t = self.t
        best = self.snap_for('best', t.model.state_dict())
        best.take()
        t.best_model, self.best_views = best.views(), True
        if t._ema is not None and t._ema.swapped:
            # the averaged weights are swapped in: this phase DID change the weights, so the files come from a host copy of the
            # arena just taken, not from the one behind 'last_epoch.pt' (which keeps the live weights)
            event = best.to_host_async()
            for path in paths:
                self.submit(best, event, best.host_views(), path)
            return
        snap = self.snaps['ckpt'][1] if 'ckpt' in self.snaps else None
        for path in paths:
            self.submit(snap, self.ckpt_event, snap.host_views(), path)

    def state_tensors(self, best=True):
        """name -> live tensor of everything a step reads or writes that lives in tensors: parameters and buffers, the optimizer's
        momentum buffers or moments, its device hyper blocks, the guard block, the dropout counters, and (`best`) the best model."""
        return _tensors(self.t, 0, best)

    def rng_get(self):
        import random
        dev = self.t._model_device()
        kind, keys, pos, has_gauss, cached = np.random.get_state()
        loaders = {ph: dl.generator.get_state() for ph, dl in self.t.dataloader.items()
                   if isinstance(getattr(dl, 'generator', None), torch.Generator)}
        return dict(torch_cpu=torch.get_rng_state(), torch_cuda=torch.cuda.get_rng_state(dev) if dev.type == 'cuda' else None,
                    python=random.getstate(), loaders=loaders,
                    numpy=(str(kind), torch.from_numpy(keys.astype(np.int64)), int(pos), int(has_gauss), float(cached)))

    def rng_set(self, rng):
        import random
        for ph, st in rng['loaders'].items():
            gen = getattr(self.t.dataloader.get(ph), 'generator', None)
            if isinstance(gen, torch.Generator):
                gen.set_state(st)
        kind, keys, pos, has_gauss, cached = rng['numpy']
        np.random.set_state((kind, keys.numpy().astype(np.uint32), pos, has_gauss, cached))
        version, words, gauss = rng['python']
        random.setstate((version, tuple(words), gauss))
        if rng['torch_cuda'] is not None:
            torch.cuda.set_rng_state(rng['torch_cuda'], self.t._model_device())
        torch.set_rng_state(rng['torch_cpu'])

    def host_fields(self):
        """Everything of the run that lives on the host, as values torch.load(weights_only=True) accepts."""
        t = self.t
        groups = [{k: v for k, v in g.items() if k != 'params'} for g in t.optimizer.param_groups]
        scores = t.val_class_scores
        return dict(iter_num=t.iter_num, max_iterations=t.max_iterations, base_lr=t.base_lr,
                    best_val_score=t.best_val_score, best_loss=t.best_loss, early_stop_counter=t.early_stop_counter,
                    lists={n: list(getattr(t, n)) for n in t._LISTS}, alpha=t.alpha,
                    val_confusion_list=[torch.from_numpy(np.array(m, dtype=np.int64)) for m in t.val_confusion_list],
                    val_class_scores=None if scores is None else {k: torch.from_numpy(np.array(v, dtype=np.float64))
                                                                  for k, v in scores.items()},
                    guard_seen=tuple(t._guard_seen), total_time=float(t._total_time), groups=copy.deepcopy(groups),
                    adam_steps={idx: float(st['step']) for idx, _, st in optim_walk(t.optimizer) if 'step' in st},
                    drop_base={name: int(m._drop_base) for name, m in t.model.named_modules()
                               if getattr(m, '_drop_base', None) is not None},
                    rng=self.rng_get())

    def put_host(self, host):
        """The host fields back, except the generators' states (rng_set, which goes last)."""
        t = self.t
        t.iter_num, t.base_lr = host['iter_num'], host['base_lr']
        t.best_val_score, t.best_loss = host['best_val_score'], host['best_loss']
        t.early_stop_counter, t.alpha = host['early_stop_counter'], host['alpha']
        for n in t._LISTS:
            setattr(t, n, list(host['lists'][n]))
        t.val_confusion_list = [m.numpy().copy() for m in host['val_confusion_list']]
        scores = host['val_class_scores']
        t.val_class_scores = None if scores is None else {k: v.numpy().copy() for k, v in scores.items()}
        t._guard_seen, t._total_time = tuple(host['guard_seen']), host['total_time']

    # -- in memory, in place ---------------------------------------------------------------
    def snapshot(self):
        """Between two steps of a live run: the whole training state into one device arena (one launch) plus the host fields
        and generator states beside it.  restore() puts it back IN PLACE: every tensor keeps its address, so graphs captured
        before stay valid and none is captured again."""
        # a deepcopy'd best model is never written to again: the reference is enough.  The views of the asynchronous path show
        # an arena that the next best model overwrites, so that arena is part of the snapshot
        views = self.best_views and isinstance(self.t.best_model, dict)
        snap = self.snap_for('run', self.state_tensors(best=views))
        snap.take()
        self.run_host = (self.host_fields(), self.t.best_model, views)
        return snap

    def restore(self):
        t = self.t
        if 'run' not in self.snaps or self.run_host is None:
            raise RuntimeError("restore_run_state() without a snapshot_run_state() before it")
        (key, snap), (host, best, views) = self.snaps['run'], self.run_host
        live = self.state_tensors(best=False)
        if views:
            live.update(('best.' + k, v) for k, v in best.items())
        if tensor_key(live) != key:
            raise RuntimeError("restore_run_state(): the state's tensors changed since the snapshot (a tensor moved, or optimizer "
                               "state appeared); take the snapshot after the first step")
        snap.restore()                         # verifies the arena first; bumps the parameter versions (weight re-pack)
        t.best_model = best
        self.put_host(host)
        for g, saved in zip(t.optimizer.param_groups, host['groups']):
            g.update(copy.deepcopy(saved))
        for idx, _, st in optim_walk(t.optimizer):
            if idx in host['adam_steps']:
                st['step'].fill_(host['adam_steps'][idx])
        self.rng_set(host['rng'])

    # -- the file --------------------------------------------------------------------------
    def write(self, epoch, over):
        """The run state after `epoch`'s validation phase -> the file, atomically; through the writer when checkpoints are
        asynchronous, otherwise before this returns."""
        from .snapshot import _own, save_atomic
        t = self.t
        live = self.state_tensors()
        snap = self.snap_for('file', live)
        snap.take()
        event = snap.to_host_async()
        views = snap.host_views()
        osd = t.optimizer.state_dict()
        for idx, st in osd['state'].items():
            osd['state'][idx] = {k: views.get(f'optim.{idx}.{k}', v.detach().cpu() if torch.is_tensor(v) else v)
                                 for k, v in st.items()}
        take = lambda prefix: collections.OrderedDict((k[len(prefix):], v) for k, v in views.items() if k.startswith(prefix))
        model = take('model.')
        meta = getattr(t.model.state_dict(), '_metadata', None)
        if meta is not None:
            model._metadata = meta
        host = self.host_fields()
        pl = dict(format=t.RUN_STATE_FORMAT, epoch=int(epoch), over=bool(over), model=model, optimizer=osd,
                  optimizer_class=type(t.optimizer).__name__, hyper=list(take('hyper.').values()) or None,
                  guard=views.get('guard'), drop_step=dict(take('drop.')), best_model=take('best.') or None, host=host,
                  ema=take('ema.') or None,
                  word=snap.word(), host_word=host_word(host))
        assert list(payload_tensors(pl)) == list(live)
        if t._ckpt_async():
            self.submit(snap, event, pl, self.resume_path)
        else:
            event.synchronize()
            save_atomic(_own(pl), self.resume_path)

    def resume(self):
        """None when there is no file; else the file is checked against this Trainer -- nothing is modified before every check
        has passed -- and put back.  Returns (epoch finished, run over)."""
        t, path = self.t, self.resume_path
        if not os.path.exists(path):
            return None
        from . import ddp
        if t._graphs or (t._val is not None and t._val.graphs):
            raise RuntimeError("resume: this Trainer has captured graphs, which hold the addresses of the optimizer state a file "
                               "would replace; resume with a new Trainer, or roll back in place with restore_run_state()")
        try:
            pl = torch.load(path, map_location='cpu', weights_only=True)
            ok = isinstance(pl, dict) and pl.get('format') == t.RUN_STATE_FORMAT
            tensors = payload_tensors(pl) if ok else None
        except Exception as e:
            raise ValueError(f"resume: {path} cannot be read as a run state ({type(e).__name__}: {e})") from e
        if not ok:
            raise ValueError(f"resume: {path} is not a run state of format {t.RUN_STATE_FORMAT}")
        sd = t.model.state_dict()
        if list(pl['model']) != list(sd):
            raise ValueError(f"resume: the model of {path} has other state-dict keys than this model")
        for k, v in sd.items():
            if pl['model'][k].shape != v.shape or pl['model'][k].dtype != v.dtype:
                raise ValueError(f"resume: {k} is {tuple(pl['model'][k].shape)} {pl['model'][k].dtype} in {path}, "
                                 f"{tuple(v.shape)} {v.dtype} in this model")
        if pl['optimizer_class'] != type(t.optimizer).__name__ or \
                len(pl['optimizer']['param_groups']) != len(t.optimizer.param_groups):
            raise ValueError(f"resume: {path} was written with {pl['optimizer_class']} over "
                             f"{len(pl['optimizer']['param_groups'])} param groups, not {type(t.optimizer).__name__} over "
                             f"{len(t.optimizer.param_groups)}")
        host = pl['host']
        if host['max_iterations'] != t.max_iterations:
            raise ValueError(f"resume: {path} belongs to a run of {host['max_iterations']} iterations, this one has "
                             f"{t.max_iterations} (num_epochs or the training loader differ)")
        if (pl['hyper'] or pl['guard'] is not None) and not hasattr(t.optimizer, 'device_schedule'):
            raise ValueError(f"resume: {path} holds device optimizer blocks; this optimizer is not a umi.optim one")
        if pl['guard'] is not None and t._guard is None:
            raise ValueError(f"resume: {path} was written with a grad_guard, this Trainer has none")
        mine, theirs = t._ema.tensors() if t._ema is not None else {}, pl.get('ema') or {}
        if list(theirs) != list(mine):
            raise ValueError(f"resume: {path} was written {'with' if theirs else 'without'} an `ema`, this Trainer runs "
                             f"{'with another one' if mine and theirs else 'with one' if mine else 'without'}")
        for k, v in theirs.items():
            if v.shape != mine[k].shape or v.dtype != mine[k].dtype:
                raise ValueError(f"resume: ema.{k} is {tuple(v.shape)} {v.dtype} in {path}, "
                                 f"{tuple(mine[k].shape)} {mine[k].dtype} in this Trainer")
        dev = t._model_device()
        words = [v.to(dev) for v in tensors.values()]
        for i, v in enumerate(words):
            if (v.numel() * v.element_size()) % 4:
                raise ValueError(f"resume: tensor {i} of {path} is not a whole number of 32-bit words")
        if ddp.fingerprint(words) != pl['word'] or host_word(host) != pl['host_word']:
            raise RuntimeError(f"resume: the contents of {path} do not match its fingerprint word; nothing was restored")
        modules = dict(t.model.named_modules())
        if any(name not in modules for name in list(pl['drop_step']) + list(host['drop_base'])):
            raise ValueError(f"resume: {path} names dropout modules this model does not have")

        # every check passed: put it back
        t.model.load_state_dict(pl['model'])
        t.optimizer.load_state_dict(pl['optimizer'])
        self.put_host(host)
        t.best_model, self.best_views = [], False
        if pl['best_model'] is not None:
            t.best_model = type(pl['best_model'])((k, v.to(dev)) for k, v in pl['best_model'].items())
        if pl['hyper']:
            t._device_schedule()
            for (block, _), raw in zip(t.optimizer.device_hyper, pl['hyper']):
                block.copy_(raw)
        if pl['guard'] is not None:
            t._attach_guard()
            t._guard._device_state().copy_(pl['guard'])
        with torch.no_grad():
            for k, v in theirs.items():
                mine[k].copy_(v)
        for name, base in host['drop_base'].items():
            modules[name]._drop_base = int(base)
        for name, step in pl['drop_step'].items():
            modules[name]._drop_step = step.to(dev)
        self.rng_set(host['rng'])              # last: nothing above may consume a draw after this
        return pl['epoch'], pl['over']
