"""The C-ABI shared library loads (no GPU needed) and exports every symbol include/unetmi.h declares."""
import ctypes
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(REPO, "include", "unetmi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(umi_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    from umi import build, lib
    names = _declared()
    assert len(names) >= 15
    cdll = ctypes.CDLL(build.LIB)
    missing = [n for n in names if not hasattr(cdll, n)]
    assert not missing, f"declared in unetmi.h but not exported: {missing}"
    assert set(lib.SIGNATURES) == set(names), set(lib.SIGNATURES) ^ set(names)
    assert lib.fn("umi_arch")() == b"gfx950"
    assert lib.fn("umi_version")() >= 1


def test_bad_arguments_return_status_not_crash():
    from umi import lib
    # null pointers / non-positive sizes are rejected before any launch (no GPU touched)
    assert lib.fn("umi_bn_finalize")(None, 0, 0, 0.0, None, None, 1e-5, 0.1, None, None, None, None, None) == -1
    assert lib.fn("umi_conv_fwd")(None, 0, None, None, None, None, 0, None, 1, 1, 1, 1, 1, 3, 3, 1, 1, 1, 1, 0, 0, 1, 1,
                                  0, 0, 0, None) == -1
    assert lib.fn("umi_pool2_fwd")(None, 0, None, None, 0, 0, 0, 0, 0, 0, None) == -1


# ---- the binding is derived from the header: umi.lib.parse_header ---------------------------------------------------------

def _header():
    return open(os.path.join(REPO, "include", "unetmi.h")).read()


def _layout(cls):
    return ctypes.sizeof(cls), [(n, getattr(cls, n).offset, getattr(cls, n).size) for n, _ in cls._fields_]


def test_parse_prototypes():
    from ctypes import c_char_p, c_double, c_float, c_int, c_long, c_longlong, c_size_t, c_uint, c_void_p
    from umi.lib import parse_header
    enums, structs, sigs = parse_header("""
        typedef void* umi_stream_t;          /* hipStream_t */
        /* every mapped type, a comment with a ; and a ( in it */
        size_t umi_all(int a, long b, long long c, unsigned d, size_t e, float f, double g, umi_stream_t s,
                       const void* p, const float *q, unsigned char* m, umi_wgrad_pending* out);   // trailing
        const char* umi_name(void);
        int umi_none ( void ) ;
        double umi_pp(const void* const* xs, float* const* outs, const int* n /* host */, long long* sums);
    """)
    assert enums == {} and structs == {}
    assert sigs == {
        "umi_all": (c_size_t, [c_int, c_long, c_longlong, c_uint, c_size_t, c_float, c_double, c_void_p,
                               c_void_p, c_void_p, c_void_p, c_void_p]),
        "umi_name": (c_char_p, []),
        "umi_none": (c_int, []),
        "umi_pp": (c_double, [c_void_p] * 4),
    }
    assert list(sigs) == ["umi_all", "umi_name", "umi_none", "umi_pp"]


def test_parse_struct_grouped_and_array_fields():
    from umi.lib import parse_header
    _, structs, sigs = parse_header("""
        typedef struct umi_t {
            const float* p;      /* a pointer */
            long a, b, c;
            float x;
            int n[3];
            double pad2_[2];
            float *u, v;
        } umi_t;                 /* 80 bytes */
    """)
    assert sigs == {} and list(structs) == ["umi_t"]
    t = structs["umi_t"]
    assert issubclass(t, ctypes.Structure) and t.__name__ == "umi_t"
    assert [(n, c) for n, c in t._fields_] == [
        ("p", ctypes.c_void_p), ("a", ctypes.c_long), ("b", ctypes.c_long), ("c", ctypes.c_long), ("x", ctypes.c_float),
        ("n", ctypes.c_int * 3), ("pad2_", ctypes.c_double * 2), ("u", ctypes.c_void_p), ("v", ctypes.c_float)]
    assert _layout(t) == (80, [("p", 0, 8), ("a", 8, 8), ("b", 16, 8), ("c", 24, 8), ("x", 32, 4), ("n", 36, 12),
                               ("pad2_", 48, 16), ("u", 64, 8), ("v", 72, 4)])


def test_parse_enum_negative_values_and_comments():
    from umi.lib import parse_header
    enums, _, _ = parse_header("""
        enum { UMI_OK = 0, UMI_ERR_BADARG = -1,   /* a comment, with = 5 in it */
               UMI_ERR_UNSUPPORTED = -2,          // another
               UMI_CONV_F32_MFMA = 16             /* the last one, no comma */ };
        enum umi_named { UMI_X = 7, };
    """)
    assert enums == {"UMI_OK": 0, "UMI_ERR_BADARG": -1, "UMI_ERR_UNSUPPORTED": -2, "UMI_CONV_F32_MFMA": 16, "UMI_X": 7}


_REFUSED = {
    "unknown type": ("int umi_f(uint8_t x);", "uint8_t"),
    "unknown field type": ("typedef struct umi_t { int a; short b; } umi_t;", "short"),
    "function pointer parameter": ("int umi_f(int n, int (*cb)(int), umi_stream_t s);", "(*cb)"),
    "bit-field": ("typedef struct umi_t { int a : 3; int b; } umi_t;", "a : 3"),
    "nested struct": ("typedef struct umi_t { int a; struct { int x; } in; } umi_t;", "struct { int x; }"),
    "prototype matched in part": ("int umi_f(int a) __attribute__((unused));", "__attribute__"),
    "struct by value": ("int umi_f(umi_wgrad_pending p);", "umi_wgrad_pending p"),
    "parameter without a name": ("int umi_f(int, long n);", "int umi_f(int, long n)"),
    "array parameter": ("int umi_f(int n[3]);", "n[3]"),
    "pointer return": ("float* umi_f(int n);", "float* umi_f"),
    "void return": ("void umi_f(int n);", "void umi_f"),
    "enumerator without a value": ("enum { UMI_A = 0, UMI_B };", "UMI_B"),
    "another typedef": ("typedef int umi_int;", "typedef int umi_int"),
    "function that is not umi_*": ("int other(int n);", "other"),
    "missing semicolon at the end": ("int umi_f(int n);\nint umi_g(int n)", "umi_g"),
}


def test_parse_refuses_what_it_does_not_understand():
    import pytest
    from umi.lib import parse_header
    for what, (text, quoted) in _REFUSED.items():
        with pytest.raises(ValueError) as e:
            parse_header("int umi_before(int a);\n" + text + "\nint umi_after(int a);\n")
        assert quoted in str(e.value), (what, str(e.value))


def test_binding_follows_the_header():
    from umi.lib import SIGNATURES, STRUCTS, parse_header
    src = _header()
    assert parse_header(src)[2] == SIGNATURES and list(parse_header(src)[1]) == list(STRUCTS)
    # one argument type
    a = src.index("int umi_pool2_bwd(")
    b = src.index("int lddp", a)
    assert b < src.index(";", a)
    sigs = parse_header(src[:b] + "long lddp" + src[b + len("int lddp"):])[2]
    pos = [(n, i) for n in SIGNATURES for i, (x, y) in enumerate(zip(SIGNATURES[n][1], sigs[n][1])) if x is not y]
    assert pos == [("umi_pool2_bwd", 1)] and sigs["umi_pool2_bwd"][1][1] is ctypes.c_long
    assert all(sigs[n][0] is SIGNATURES[n][0] and len(sigs[n][1]) == len(SIGNATURES[n][1]) for n in SIGNATURES)
    # one inserted struct field: the later fields move, the earlier ones and the other structs do not
    a = src.index("typedef struct umi_optim_desc {")
    b = src.index("long n;", a)
    structs = parse_header(src[:b] + "long extra; " + src[b:])[1]
    size0, f0 = _layout(STRUCTS["umi_optim_desc"])
    size1, f1 = _layout(structs["umi_optim_desc"])
    assert f1[:4] == f0[:4] and f1[4] == ("extra", 32, 8) and size1 == size0 + 8
    assert f1[5:] == [(n, off + 8, sz) for n, off, sz in f0[4:]]
    assert all(_layout(structs[n]) == _layout(STRUCTS[n]) for n in STRUCTS if n != "umi_optim_desc")


def test_struct_layouts_match_the_compiler(tmp_path):
    """sizeof / offsetof of every struct of unetmi.h as the host compiler of the build lays them out, against the ctypes classes."""
    import subprocess
    from umi import build
    from umi.lib import STRUCTS
    assert sorted(STRUCTS) == ["umi_optim_desc", "umi_optim_hyper", "umi_pack_desc", "umi_wgrad_pending", "umi_wstd_desc"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "unetmi.h"', 'int main(void) {']
    for name, cls in STRUCTS.items():
        lines.append(f'    printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'    printf("{name}.{f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));' for f, _ in cls._fields_]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.check_call([build.HIPCC, "-x", "c++", "-I", os.path.dirname(build.HEADER), str(src), "-o", str(exe)])
    got = subprocess.check_output([str(exe)], text=True).split("\n")
    want = []
    for name, cls in STRUCTS.items():
        size, fields = _layout(cls)
        want.append(f"{name} {size}")
        want += [f"{name}.{f} {off} {sz}" for f, off, sz in fields]
    assert got == want + [""]


def test_optim_hyper_size_is_the_library_s():
    import numpy as np
    from umi import lib, optim
    assert ctypes.sizeof(lib.STRUCTS["umi_optim_hyper"]) == lib.fn("umi_optim_hyper_bytes")() == 96
    assert optim._HYPER == np.dtype(lib.STRUCTS["umi_optim_hyper"])


def test_constants_come_from_the_header():
    from umi import lib
    assert (lib.UMI_F32, lib.UMI_F16, lib.UMI_OK) == (0, 1, 0)
    assert (lib.UMI_ERR_BADARG, lib.UMI_ERR_UNSUPPORTED, lib.UMI_ERR_WORKSPACE) == (-1, -2, -3)
    assert (lib.CONV_UPSAMPLE2, lib.CONV_FORCE_GENERIC, lib.CONV_DGRAD_STRIDED, lib.CONV_ACCUMULATE, lib.CONV_F32_MFMA) == \
        (1, 2, 4, 8, 16)
    assert lib.ENUMS == lib.parse_header(_header())[0]


def test_call_and_supported():
    import pytest
    from umi import lib
    lay, rows = ctypes.c_int(-1), ctypes.c_int(-1)
    plan = (2, 32, 32, 64, 64, 3, 3, 1, 1, 64, 64, lib.UMI_F16, lib.UMI_F16)          # host only: nothing is launched
    assert lib.call("umi_conv_fwd_plan", *plan, 0, 0, ctypes.addressof(lay), ctypes.addressof(rows)) is None
    assert lay.value == 1 and rows.value > 0
    assert lib.supported("umi_conv_fwd_plan", *plan, 0, 0, None, None) is True
    assert lib.supported("umi_conv_fwd_plan", *plan, lib.CONV_ACCUMULATE, 0, None, None) is False      # 3x3: UMI_ERR_UNSUPPORTED
    with pytest.raises(RuntimeError, match="umi_conv_fwd_plan failed with UMI_ERR_UNSUPPORTED"):
        lib.call("umi_conv_fwd_plan", *plan, lib.CONV_ACCUMULATE, 0, None, None)
    bad = (None, 0, None, None, 0, 0, 0, 0, 0, 0, None)
    with pytest.raises(RuntimeError, match="umi_pool2_fwd failed with UMI_ERR_BADARG"):
        lib.call("umi_pool2_fwd", *bad)
    with pytest.raises(RuntimeError, match="umi_pool2_fwd failed with UMI_ERR_BADARG"):
        lib.supported("umi_pool2_fwd", *bad)
    with pytest.raises(ctypes.ArgumentError):
        lib.call("umi_pool2_fwd", None, 1.5, *bad[2:])                       # int ldx: the header's argtypes are installed
