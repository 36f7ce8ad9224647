"""ctypes binding of libunetmi.so (declared in include/unetmi.h).

The product path has NO CPU or eager-PyTorch fallback: if the shared library is
missing and cannot be built, importing this module raises.
"""
import ctypes
import os
import re

from . import build as _build

# the closed type map of include/unetmi.h; a parameter or field with a `*` is an address
_SCALAR = {"int": ctypes.c_int, "long": ctypes.c_long, "long long": ctypes.c_longlong, "unsigned": ctypes.c_uint,
           "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double, "umi_stream_t": ctypes.c_void_p}
_TYPE_WORDS = {w for t in _SCALAR for w in t.split()} | {"const", "void", "char", "short", "signed", "struct", "enum"}


def _refuse(decl, why="cannot parse"):
    raise ValueError(f"unetmi.h: {why}: {decl!r}")


def _ctype(text, decl):
    """ctypes type of the type part of a parameter / field declaration."""
    if "*" in text:
        return ctypes.c_void_p if re.fullmatch(r"[\w\s*]+", text) else _refuse(decl)
    t = " ".join(w for w in text.split() if w != "const")
    return _SCALAR[t] if t in _SCALAR else _refuse(decl, f"unknown type {t!r} in")


def _declarator(text, decl):
    """'const float* part' -> ('const float*', 'part', None);  'pad2_[2]' -> ('', 'pad2_', 2)."""
    m = re.fullmatch(r"(.*?)(\w+) ?(?:\[ ?(\d+) ?\])?", text.strip())
    if not m or m.group(2) in _TYPE_WORDS:             # e.g. a bit-field, a parameter without a name
        _refuse(decl, f"cannot parse {text.strip()!r} in")
    return m.group(1).strip(), m.group(2), m.group(3) and int(m.group(3))


def _fields(body, decl):
    out = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        first, *more = stmt.split(",")                 # `long st, sk, sn;`: the later declarators share the first one's base type
        base, name, n = _declarator(first, decl)
        for ptr, name, n in [("*" in base, name, n)] + [("*" in t, *_declarator(t, decl)[1:]) for t in more]:
            t = _ctype(base.replace("*", " ") + "*" * ptr, decl)
            out.append((name, t * n if n else t))
    return out


def _param(text, decl):
    base, _, n = _declarator(text, decl)
    return _ctype(base, decl) if n is None else _refuse(decl, f"array parameter {text.strip()!r} in")


def parse_header(text):
    """(enums, structs, signatures) of a header written like include/unetmi.h: {name: int}, {name: ctypes.Structure subclass},
    {name: (restype, [argtypes])}.  Strict: a declaration that is not fully understood raises and is quoted, nothing is guessed."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)          # include guard, #include, #ifdef __cplusplus
    text, wrapped = re.subn(r'extern\s+"C"\s*\{', "", text)
    enums, structs, sigs = {}, {}, {}
    *pieces, rest = text.split(";")
    decl = ""
    for piece in pieces:                                        # declarations end at a `;` outside braces
        decl += piece
        if decl.count("{") > decl.count("}"):
            decl += ";"
            continue
        decl, d = "", " ".join(decl.split())
        if re.fullmatch(r"typedef void ?\* ?umi_stream_t", d):
            continue
        m = re.fullmatch(r"enum (?:\w+ )?\{(.*)\}", d)
        if m:
            for item in filter(None, (i.strip() for i in m.group(1).split(","))):
                e = re.fullmatch(r"(\w+) = (-?\d+)", item) or _refuse(d, f"cannot parse enumerator {item!r} in")
                enums[e.group(1)] = int(e.group(2))
            continue
        m = re.fullmatch(r"typedef struct (\w+) \{([^{}]*)\} \1", d)
        if m:
            structs[m.group(1)] = type(m.group(1), (ctypes.Structure,), {"_fields_": _fields(m.group(2), d)})
            continue
        m = re.fullmatch(r"([\w *]+?) ?\b(umi_\w+) ?\(([^()]*)\)", d) or _refuse(d)
        ret = m.group(1).replace(" ", "")
        res = ctypes.c_char_p if ret == "constchar*" else _refuse(d, "unsupported return type in") if "*" in ret \
            else _ctype(m.group(1), d)
        params = [] if m.group(3).strip() == "void" else m.group(3).split(",")
        sigs[m.group(2)] = (res, [_param(p, d) for p in params])
    if (decl + rest).strip() != "}" * wrapped:
        _refuse(" ".join((decl + rest).split()))
    return enums, structs, sigs


with open(_build.HEADER) as _f:
    ENUMS, STRUCTS, SIGNATURES = parse_header(_f.read())          # the header is the only statement of the C ABI
# UMI_F32, UMI_F16, UMI_OK, UMI_ERR_*, and the conv flags under their short names CONV_*
globals().update({k.replace("UMI_CONV_", "CONV_"): v for k, v in ENUMS.items()})
_ERR = {v: k for k, v in ENUMS.items() if k.startswith("UMI_ERR_")}


def _load():
    alt = os.environ.get("UMI_LIB_OVERRIDE")          # tuning aid: A/B two builds of libunetmi on one box
    if alt:
        if not os.path.exists(alt):
            raise RuntimeError(f"UMI_LIB_OVERRIDE={alt} does not exist")
        return ctypes.CDLL(alt)
    path = _build.LIB
    if not os.path.exists(path) or (_build.stale() and os.path.exists(_build.HIPCC)):
        if not os.path.exists(_build.HIPCC):
            raise RuntimeError(
                f"libunetmi.so not found at {path} and hipcc is unavailable: the HIP extension is "
                "required, there is no CPU fallback (run `python __graft_entry__.py build`).")
        _build.build_lib()
    return ctypes.CDLL(path)


_lib = _load()

for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(_lib, _name)          # AttributeError here == header/library mismatch: fail loudly
    _fn.restype = _res
    _fn.argtypes = _args


def check(status: int, what: str):
    if status != 0:
        raise RuntimeError(f"libunetmi: {what} failed with "
                           f"{_ERR.get(status, 'hipError_t ' + str(status))}")


def call(name, *args):
    """Run a status-returning entry point; raises on any non-zero status.  (One Python frame around the ctypes call: an eager
    step makes about 350 of these.)"""
    st = getattr(_lib, name)(*args)
    if st:
        check(st, name)


def supported(name, *args):
    """The same for an entry point that may answer UMI_ERR_UNSUPPORTED ("nothing was launched, run the separate passes"):
    False then, True when it ran."""
    st = getattr(_lib, name)(*args)
    if st and st != UMI_ERR_UNSUPPORTED:
        check(st, name)
    return not st


def fn(name):
    return getattr(_lib, name)


lib = _lib
