"""Deferred parameter-gradient fills of a tape (umi/graph.py, umi/graph_tu.py).

A deferred fill is a parameter gradient whose CONTENT is only written (with `=`) by a grouped launch at the next flush.  Until
then the buffer must not be added to or handed to the gradient sink, and what the launch will read must not be overwritten.
The ops record an item (`defer` / `open`), `Tape._set_pgrad` asks `pending` and parks what has to wait (`park_add`,
`park_ready`), `flush` runs everything and leaves the object empty.
"""
import weakref


class Deferred:
    def __init__(self, tape):
        self.tape = weakref.proxy(tape)     # (the tape owns this object: no reference cycle, its tensors go when it goes)
        self.marks = False      # the tape flushes at marked points of the backward pass (TUTape.flush_mark)
        self._kinds = {}        # name -> (run, each, on), in flush order
        self._items = {}        # name -> {group key: [items]}, groups in first-recorded order
        self._fills = []        # [lo, hi) address ranges of the unfilled buffers (gradients may be views into them)
        self._reads = set()     # data_ptr of every tensor a deferred launch, or another consumer still to come, reads
        self._adds = []         # (destination, addend): second contributions to a parameter whose gradient is a deferred fill
        self._ready = []        # parameters whose bucket slot (gradient sink) is a deferred fill: mark_ready after it

    def register(self, kind, run, each=None, on=None):
        """A deferred kind; the kinds flush in the order they were registered.  `run(key, items, tape)` is the grouped launch
        of one group.  With `each(key, item, tape)` the group runs item by item when it has fewer than two items or `run`
        returns False (the grouped kernel refused).  `on(tape)`: false = this kind is not deferred now, its ops run at once."""
        self._kinds[kind] = (run, each, on)
        self._items[kind] = {}

    def open(self, kind, key=None, fills=(), reads=()):
        """The live item list of `kind`'s group `key`, for a callee that records its item itself (ops.conv_wgrad(defer=...)),
        or None where the kind is off.  The group's launch writes the tensors in `fills` and reads those in `reads`."""
        on = self._kinds[kind][2]
        if on is not None and not on(self.tape):
            return None
        for t in fills:
            self._fills.append((t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()))
        for t in reads:
            self._reads.add(t.data_ptr())
        return self._items[kind].setdefault(key, [])

    def defer(self, kind, key, item, fills=(), reads=()):
        """Record `item` for `kind`'s grouped launch at the next flush; False (nothing recorded) where the kind is off."""
        items = self.open(kind, key, fills, reads)
        if items is not None:
            items.append(item)
        return items is not None

    def pending(self, t):
        a = t.data_ptr()
        return any(lo <= a < hi for lo, hi in self._fills)

    def hold(self, t):          # `t` has another reader still to come: accumulate into a fresh tensor (TUTape._give)
        self._reads.add(t.data_ptr())

    def held(self, t):
        return t.data_ptr() in self._reads

    def park_add(self, dst, src):
        self._adds.append((dst, src))

    def park_ready(self, p):
        self._ready.append(p)

    def flush(self):
        """Run every deferred fill recorded so far, kind by kind, then the parked second contributions, then hand the filled
        bucket slots to the gradient sink."""
        for kind, (run, each, _) in self._kinds.items():
            groups, self._items[kind] = self._items[kind], {}
            for key, items in groups.items():
                if not items:
                    continue
                if each is None:
                    run(key, items, self.tape)
                elif len(items) < 2 or not run(key, items, self.tape):
                    for it in items:
                        each(key, it, self.tape)
        for dst, src in self._adds:
            dst.add_(src)
        for p in self._ready:
            self.tape.grad_sink.mark_ready(p)
        self._fills, self._reads, self._adds, self._ready = [], set(), [], []
