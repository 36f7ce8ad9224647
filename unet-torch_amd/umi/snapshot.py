"""Snapshots of a training state: every tensor copied into one contiguous arena by one pass (umi_snapshot_multi,
include/unetmi.h), with the arena's integrity word -- the replica fingerprint of umi.ddp -- formed on the way.

    layout(word_counts)        where each tensor's slot starts in the arena, in 32-bit words
    snapshot_numpy(arrays)     the NumPy statement: (arena as uint32, F); the device arena and word equal it with ==
    Snapshot(tensors)          table, workspace, result word and arena allocated once; take() / verify() / restore() /
                               to_host_async() / views() / host_views()
    CheckpointWriter()         one background thread that turns host views into files, atomically

A slot is 16-byte aligned and 4 * ceil(n / 4) words long; the pad words are zeros, so the arena's bytes are a function of the
tensors alone.  A checkpoint file, a best-model copy and an in-place roll-back are all taken from such an arena: the training
stream pays one take(), the device-to-host copy runs on a side stream and the file is written by the writer's thread.
CPU tensors run the NumPy statement with torch copies behind the same interface.
"""
import collections
import os
import queue
import threading

import torch

from .ddp import _FP_MASK, fingerprint_numpy


def layout(word_counts):
    """(offsets, total_words): tensor i of word_counts[i] 32-bit words starts `offsets[i]` words into the arena; every offset is
    a multiple of 4 (16 bytes) and a slot is 4 * ceil(n / 4) words."""
    offsets, at = [], 0
    for n in word_counts:
        n = int(n)
        if n < 0:
            raise ValueError(f"snapshot: a negative word count {n}")
        offsets.append(at)
        at += 4 * ((n + 3) // 4)
    return offsets, at


def _words(a):
    import numpy as np
    a = np.ascontiguousarray(a)
    if a.nbytes % 4:
        raise ValueError(f"snapshot: a tensor of {a.nbytes} bytes is not a whole number of 32-bit words")
    return a.reshape(-1).view(np.uint8).view(np.uint32)


def snapshot_numpy(arrays):
    """(arena, F): the arena of `arrays` as a uint32 array (slots as layout() places them, zeros in the pads) and the word
    umi.ddp.fingerprint_numpy(arrays)."""
    import numpy as np
    words = [_words(a) for a in arrays]
    offsets, total = layout([w.size for w in words])
    arena = np.zeros(total, dtype=np.uint32)
    for w, off in zip(words, offsets):
        arena[off:off + w.size] = w
    return arena, fingerprint_numpy(arrays)


class _Done:
    """The event of a copy that has already happened (CPU snapshots)."""

    def synchronize(self):
        pass

    def query(self):
        return True


class Snapshot:
    """One arena for a fixed set of tensors (a list, or a dict such as a state_dict: views() then carries its names).

    The snapshot ALIASES the live tensors -- restore() writes through them, at their addresses, so captured HIP graphs stay
    valid -- which is why a non-contiguous tensor is refused rather than copied.  All tensors live on one device (the
    kernels), or all on the CPU (the NumPy statement)."""

    def __init__(self, tensors, device=None):
        import numpy as np
        if isinstance(tensors, dict):
            self._metadata = getattr(tensors, "_metadata", None)
            self.names, tensors = list(tensors.keys()), list(tensors.values())
        else:
            tensors = list(tensors)
            self.names = list(range(len(tensors)))
        self.tensors = [t.detach() for t in tensors]
        for i, t in enumerate(self.tensors):
            if (t.numel() * t.element_size()) % 4:
                raise ValueError(f"snapshot: tensor {i} has {t.numel() * t.element_size()} bytes, not a whole number of 32-bit words")
            if not t.is_contiguous():
                raise ValueError(f"snapshot: tensor {i} is not contiguous (the snapshot aliases the live tensor; a copy could "
                                 "not be restored into)")
        devs = {t.device for t in self.tensors}
        if len(devs) > 1:
            raise ValueError(f"snapshot: the tensors live on several devices ({sorted(map(str, devs))})")
        self.device = devs.pop() if devs else torch.device(device if device is not None else "cpu")
        if device is not None and torch.device(device).type != self.device.type:
            raise ValueError(f"snapshot: the tensors live on {self.device}, not on {device}")
        self.cuda = self.device.type == "cuda"
        self.counts = [t.numel() * t.element_size() // 4 for t in self.tensors]
        self.offsets, self.total_words = layout(self.counts)
        self.bytes = 4 * sum(self.counts)
        self.arena = torch.zeros(4 * self.total_words, dtype=torch.uint8, device=self.device)
        self._host, self._inflight, self._word = None, None, None
        self._holds, self._held = 0, threading.Condition()
        if not self.cuda:
            return
        from . import lib as L, ops
        blk = L.fn("umi_optim_block_elems")()
        base = self.arena.data_ptr()
        assert base % 16 == 0
        fwd, chk = np.zeros(len(self.tensors), dtype=ops.OPTIM_DESC), np.zeros(len(self.tensors), dtype=ops.OPTIM_DESC)
        b0 = 0
        for i, (t, n, off) in enumerate(zip(self.tensors, self.counts, self.offsets)):
            fwd[i] = (t.data_ptr(), 0, base + 4 * off, 0, n, b0, 0)
            chk[i] = (base + 4 * off, 0, 0, 0, n, b0, 0)               # the fingerprint pass reads p, n and blk0 only
            b0 += (n + blk - 1) // blk
        self.blocks = b0
        with torch.cuda.device(self.device):
            self.table, self.table_chk = (torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(self.device) for a in (fwd, chk))
            self.ws = torch.empty(max(b0, 1), dtype=torch.int64, device=self.device)
            self.out = torch.zeros(2, dtype=torch.int64, device=self.device)      # [word of take(), word of verify()]

    # ---- the copy ----------------------------------------------------------------------------------------------------------
    def take(self):
        """Enqueue the copy of every tensor into the arena on the current stream (two launches: the copy with its block
        partials, the finalize pass).  Waits -- on the device -- for a to_host_async() copy of the previous arena."""
        if not self.cuda:
            import numpy as np
            arena, self._word = snapshot_numpy([t.reshape(-1).view(torch.uint8).numpy() for t in self.tensors])
            self.arena.copy_(torch.from_numpy(arena.view(np.uint8)))
            return self
        from . import lib as L, ops
        with torch.cuda.device(self.device):
            if self._inflight is not None:
                torch.cuda.current_stream().wait_event(self._inflight)
                self._inflight = None
            L.call("umi_snapshot_multi", self.table.data_ptr(), len(self.tensors), self.blocks, self.ws.data_ptr(),
                   self.ws.numel() * 8, self.out.data_ptr(), ops._stream())
        self._word = None
        return self

    def word(self):
        """The fingerprint word of the last take() (8 bytes read back)."""
        if self._word is None:
            self._word = int(self.out[0].item()) & _FP_MASK
        return self._word

    def _arena_word(self):
        if not self.cuda:
            import numpy as np
            a = self.arena.numpy().view(np.uint32)
            return fingerprint_numpy([a[off:off + n] for off, n in zip(self.offsets, self.counts)])
        from . import lib as L, ops
        with torch.cuda.device(self.device):
            L.call("umi_fingerprint_multi", self.table_chk.data_ptr(), len(self.tensors), self.blocks, self.ws.data_ptr(),
                   self.ws.numel() * 8, self.out.data_ptr() + 8, ops._stream())
        return int(self.out[1].item()) & _FP_MASK

    def verify(self):
        """Whether the arena still holds what take() put there: the fingerprint pass over the arena's slots against the word
        stored at take()."""
        return self._arena_word() == self.word()

    def restore(self):
        """Arena -> the live tensors, in place.  Raises RuntimeError and writes nothing when verify() fails."""
        if self._word is None and not self.cuda:
            raise RuntimeError("snapshot: restore() before take()")
        if not self.verify():
            raise RuntimeError("snapshot: the arena no longer matches the word of its take(); nothing was restored")
        if not self.cuda:
            for t, v in zip(self.tensors, self.views().values()):
                t.copy_(v)
        else:
            from . import lib as L, ops
            with torch.cuda.device(self.device):
                L.call("umi_restore_multi", self.table.data_ptr(), len(self.tensors), self.blocks, ops._stream())
        for t in self.tensors:                # written through raw pointers: tell autograd and ops.PackCache (optim._bump)
            torch.autograd.graph.increment_version(t)
        return self

    # ---- the way to a file -------------------------------------------------------------------------------------------------
    def hold_host(self):
        """Marks the host copy as in use and returns the callable that releases it; to_host_async() waits (on the host) until
        every hold is released, so a writer never clones from a buffer that is being overwritten."""
        with self._held:
            self._holds += 1
        released = []

        def release():
            with self._held:
                if not released:
                    released.append(True)
                    self._holds -= 1
                    self._held.notify_all()
        return release

    def to_host_async(self):
        """Copy the arena into the (pinned) host buffer on a side stream; returns the event of that copy.  The next take()
        makes its stream wait for it, so an arena in flight is never overwritten."""
        with self._held:
            while self._holds:
                self._held.wait()
        if not self.cuda:
            if self._host is None:
                self._host = torch.empty_like(self.arena)
            self._host.copy_(self.arena)
            return _Done()
        with torch.cuda.device(self.device):
            if self._host is None:
                self._host = torch.empty(self.arena.numel(), dtype=torch.uint8).pin_memory()
                self._copy_stream = torch.cuda.Stream()
            self._copy_stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(self._copy_stream):
                self._host.copy_(self.arena, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
        self._inflight = ev
        return ev

    def _views_of(self, flat):
        out = collections.OrderedDict()
        for name, t, n, off in zip(self.names, self.tensors, self.counts, self.offsets):
            out[name] = flat[4 * off:4 * (off + n)].view(t.dtype).view(t.shape)
        if getattr(self, "_metadata", None) is not None:
            out._metadata = self._metadata
        return out

    def views(self):
        """name -> view into the arena with the source's dtype and shape (a later take() changes what they show)."""
        return self._views_of(self.arena)

    def host_views(self):
        """The same over the host copy of to_host_async()."""
        if self._host is None:
            raise RuntimeError("snapshot: host_views() before to_host_async()")
        return self._views_of(self._host)


def _own(obj):
    """`obj` with every tensor cloned into a storage of its own (so torch.save writes that tensor's bytes, not the arena's)."""
    if isinstance(obj, torch.Tensor):
        return obj.detach().clone()
    if isinstance(obj, dict):
        out = type(obj)((k, _own(v)) for k, v in obj.items())
        if hasattr(obj, "_metadata"):
            out._metadata = obj._metadata
        return out
    if isinstance(obj, (list, tuple)):
        return type(obj)(_own(v) for v in obj)
    return obj


def save_atomic(obj, path):
    """torch.save to path + '.tmp', then os.replace: a reader sees the old file or the new one, never a part of one."""
    tmp = path + ".tmp"
    try:
        torch.save(obj, tmp)
        os.replace(tmp, path)
    except BaseException:
        try:
            os.remove(tmp)
        except OSError:
            pass
        raise


class CheckpointWriter:
    """One background thread with a queue.  A job is (event, object, path): the thread waits for the event (the device-to-host
    copy), clones every tensor of the object into its own storage, releases the host buffer, and writes the file atomically.
    join() waits for all jobs and re-raises the first error of the thread."""

    def __init__(self):
        self._q, self._error, self._last = queue.Queue(), None, {}
        self._thread = threading.Thread(target=self._run, name="umi-checkpoint-writer", daemon=True)
        self._thread.start()

    def _run(self):
        while True:
            job = self._q.get()
            if job is None:
                self._q.task_done()
                return
            event, obj, path, release, done = job
            try:
                if self._error is None:
                    if event is not None:
                        event.synchronize()
                    own = _own(obj)
                    if release is not None:
                        release()
                        release = None
                    save_atomic(own, path)
            except BaseException as e:          # kept for join(): a lost checkpoint must not be silent
                if self._error is None:
                    self._error = e
            finally:
                if release is not None:
                    release()
                done.set()
                self._q.task_done()

    def submit(self, event, obj, path, release=None):
        """Enqueue one file.  `obj`: any nest of dicts / lists / tuples whose tensors are host views; `release`: called once
        the tensors are cloned (Snapshot.hold_host()).  Waits for the previous job on the same path."""
        if not self._thread.is_alive():
            raise RuntimeError("CheckpointWriter: submit() after close()")
        prev = self._last.get(path)
        if prev is not None:
            prev.wait()
        done = self._last[path] = threading.Event()
        self._q.put((event, obj, path, release, done))

    def join(self):
        self._q.join()
        self._last = {}
        err, self._error = self._error, None
        if err is not None:
            raise err

    def close(self):
        """join(), then end the thread."""
        try:
            self.join()
        finally:
            if self._thread.is_alive():
                self._q.put(None)
                self._thread.join()
