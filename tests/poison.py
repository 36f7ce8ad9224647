"""Make unwritten device memory visible to whole-model tests.

The tapes (umi/graph.py, umi/graph_tu.py) allocate every activation, gradient, mask and partial-sum tensor with
`torch.empty`, share one grow-only scratch buffer (`umi.ops.workspace`) between all layers and, under a `GradReducer`, write
parameter gradients straight into long-lived bucket slots.  The caching allocator usually hands a step the very tensor the
previous step (or test) used in the same role, so a path that reads what nobody wrote this step still sees plausible values.
Inside `poisoned(byte)` every such byte starts as `byte` instead: 0xFF is NaN in fp16 / fp32 / fp64, 255 in uint8 masks and
-1 in integer tensors; 0x00 is the benign twin.  A step whose results differ between the two read unwritten memory.

Not reachable from Python, and therefore outside what this helper can show: the static device scratch of the 2-D row
reduction (`g_red_scratch` in the library).

Plain module imported by the tests that need it -- not a conftest, no fixtures."""
import contextlib
import sys

import torch

_PATCHED = ("empty", "empty_like", "empty_strided")


def fill_bytes(t, byte, _empty=torch.empty):
    """Set every byte of the storage behind `t` to `byte` (on the current stream for a device tensor).  Through the storage,
    so 0-dim, empty, bool and non-dense strided tensors need no special case."""
    nbytes = t.untyped_storage().nbytes()
    if nbytes:
        _empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage(), 0, (nbytes,)).fill_(byte)
    return t


@contextlib.contextmanager
def poisoned(byte, cpu_too=False):
    """For the duration: every CUDA tensor returned by torch.empty / empty_like / empty_strided has all its bytes set to
    `byte`, and the buffer `umi.ops.workspace` returns is re-filled with `byte` on every call (each call site of the tapes
    requests, fills and consumes the workspace within one Python call).  cpu_too: also fill CPU tensors (the helper's own CPU
    test).
    The originals are restored on exit, also on error."""
    byte = int(byte)
    assert 0 <= byte <= 255
    real = {n: getattr(torch, n) for n in _PATCHED}

    def wrap(fn):
        def alloc(*a, **k):
            t = fn(*a, **k)
            if isinstance(t, torch.Tensor) and t.layout == torch.strided and (t.is_cuda or (cpu_too and t.device.type == "cpu")):
                fill_bytes(t, byte, real["empty"])
            return t
        alloc.__name__, alloc.__wrapped__ = fn.__name__, fn
        return alloc

    from umi import ops
    real_ws = ops.workspace

    def workspace(nbytes, device):
        return fill_bytes(real_ws(nbytes, device), byte, real["empty"])

    def sites(fn):
        # umi.ops itself and every module that imported the function by name (umi.ops_tu, ...)
        return [m for n, m in list(sys.modules.items())
                if m is not None and n.startswith("umi.") and m.__dict__.get("workspace") is fn]
    try:
        for n in _PATCHED:
            setattr(torch, n, wrap(real[n]))
        for m in sites(real_ws):
            m.workspace = workspace
        yield
    finally:
        for n in _PATCHED:
            setattr(torch, n, real[n])
        for m in sites(workspace):                  # (also a module first imported inside the block)
            m.workspace = real_ws


def poison_buckets(reducer, byte):
    """Fill every bucket of a umi.ddp.GradReducer with `byte`: a slot no launch rewrites this step stays visible."""
    for b in reducer.buckets:
        fill_bytes(b.flat, int(byte))
