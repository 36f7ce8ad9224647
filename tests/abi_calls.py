"""The C-ABI calls of libunetmi by parameter name: one spelling for a test's table of calls and for a census that records them.

`params(entry)` are the (name, kind) pairs of include/unetmi.h, kind in {"int", "float", "ptr"}.  `key(entry, values, batch)` is what
a call "is", batch aside: the entry point, every integer and float scalar by name and, for every address, whether it is null.
  * `N` (and the loss kernels' image count) is dropped; `M`, `P`, `rows` and `count` are divided by the batch (rows per image);
  * `ws_bytes` / `nbytes` are dropped: they are the capacity of a grow-only scratch buffer, i.e. the history of the process;
  * `stream` is dropped: every caller passes torch's current stream.
`Recorder` wraps the binding's three doors (umi.lib.call / supported / fn) and keeps every call that goes through them."""
import ctypes
import re

PER_IMAGE = ("M", "P", "rows", "count")
DROPPED = ("N", "ws_bytes", "nbytes", "stream")

_names = {}


def _header_names():
    if not _names:
        from umi import build
        with open(build.HEADER) as f:
            text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
        for m in re.finditer(r"\b(umi_\w+)\s*\(([^()]*)\)\s*;", text):
            ps = [p.strip() for p in m.group(2).split(",")]
            _names[m.group(1)] = [] if ps == ["void"] else [re.search(r"(\w+)$", p).group(1) for p in ps]
    return _names


def params(entry):
    """[(name, kind)] of an entry point, in call order."""
    from umi import lib
    _, argtypes = lib.SIGNATURES[entry]
    names = _header_names()[entry]
    assert len(names) == len(argtypes), entry
    kind = {ctypes.c_void_p: "ptr", ctypes.c_float: "float", ctypes.c_double: "float"}
    return [(n, kind.get(t, "int")) for n, t in zip(names, argtypes)]


def _null(v):
    if isinstance(v, ctypes.c_void_p):
        v = v.value
    return v is None or v == 0


def key(entry, values, batch):
    """values: {parameter name: scalar value, or for an address anything whose truth says "not null"} (a recorded call passes
    the raw arguments, a table row passes True / None)."""
    scal, null = [], []
    for name, kind in params(entry):
        if name in DROPPED:
            continue
        v = values[name]
        if kind == "ptr":
            if _null(v):
                null.append(name)
        elif name in PER_IMAGE:
            assert v % batch == 0, (entry, name, v, batch)
            scal.append((name, v / batch if kind == "float" else int(v) // batch))
        else:
            scal.append((name, float(v) if kind == "float" else int(v)))
    return (entry, tuple(scal), tuple(null))


def show(k):
    entry, scal, null = k
    return f"{entry}({', '.join(f'{n}={v:g}' if isinstance(v, float) else f'{n}={v}' for n, v in scal)}" \
           f"{'; null: ' + ' '.join(null) if null else ''})"


class Recorder:
    """Wraps umi.lib.call / supported / fn with `monkeypatch`; `calls` is [(entry, {name: raw argument}, status)]."""

    def __init__(self, monkeypatch):
        from umi import lib
        self.calls = []
        self.on = True
        call0, sup0, fn0 = lib.call, lib.supported, lib.fn
        rec = self

        def note(name, args, st):
            if rec.on and name in lib.SIGNATURES:
                rec.calls.append((name, dict(zip((n for n, _ in params(name)), args)), st))

        def call(name, *args):
            note(name, args, 0)
            return call0(name, *args)

        def supported(name, *args):
            ok = sup0(name, *args)
            note(name, args, 0 if ok else lib.UMI_ERR_UNSUPPORTED)
            return ok

        def fn(name):
            f = fn0(name)

            def wrapped(*args):
                st = f(*args)
                note(name, args, st)
                return st
            return wrapped

        monkeypatch.setattr(lib, "call", call)
        monkeypatch.setattr(lib, "supported", supported)
        monkeypatch.setattr(lib, "fn", fn)
