"""The grid of host-side dispatch queries whose answers tests/golden/dispatch_table.npz pins, shared by tests/test_dispatch_table.py
and tools/gen_dispatch_table.py.  Pure host code of libunetmi: no GPU is touched.

  plan         umi_conv_fwd_plan -> (status, layout, stat_rows) over every axis below (493,920 queries)
  wgrad_ws     umi_conv_wgrad_ws_bytes over channels x geometry x shape x flags {0, FORCE_GENERIC} x dtype {F16, F32}
  gather_rows  umi_conv_gather_bnred_rows over channels x geometry x shape x flags {0, DGRAD_STRIDED}, fp16, ld = C
  head_rows    umi_head_dgrad_bnred_rows over channels x shape x ldda x dtype {F16, F32}
  head_ws      umi_head_bwd_fused_ws_bytes over channels x shape

Output sizes follow the C rule of the library, (H + 2 pad - R) / stride + 1 with the division truncating toward zero.  Every
point lies below the 31-bit source-image limit of the tap-gather kernel."""
import ctypes
import itertools

import numpy as np

F32, F16 = 0, 1
CHANNELS = (1, 2, 3, 4, 8, 16, 24, 32, 64, 96, 128, 256, 512, 1024)
GEOMETRIES = ((1, 1, 1, 0), (3, 3, 1, 1), (2, 2, 2, 0), (7, 7, 2, 3), (3, 3, 2, 1), (16, 16, 16, 0), (1, 1, 2, 0))   # R, S, stride, pad
FLAGS = (0, 1, 2, 4, 8)
DTYPES = ((F16, F16), (F16, F32), (F32, F32))                # (in, out)
SHAPES = ((1, 8, 8), (2, 16, 24), (2, 64, 64), (16, 512, 512))   # N, H, W
LD_EXTRA = (0, 8, 4)                                         # ldx = Ci + e, ldy = Co + e
HAS_BIAS = (0, 1)


def _out(h, pad, r, stride):
    return int((h + 2 * pad - r) / stride) + 1               # C division


def tables(fn):
    """fn(name) -> the ctypes function of that name (umi.lib.fn).  Returns {name: array}."""
    plan, lay, rows = fn("umi_conv_fwd_plan"), ctypes.c_int(), ctypes.c_int()
    p_lay, p_rows = ctypes.byref(lay), ctypes.byref(rows)
    out = []
    for ci, co, (r, s, st, pad), fl, (din, dout), (n, h, w), e, hb in itertools.product(
            CHANNELS, CHANNELS, GEOMETRIES, FLAGS, DTYPES, SHAPES, LD_EXTRA, HAS_BIAS):
        lay.value, rows.value = -7, -7
        status = plan(n, h, w, ci, co, r, s, st, pad, ci + e, co + e, din, dout, fl, hb, p_lay, p_rows)
        out.append((status, lay.value, rows.value))
    t = {"plan": np.asarray(out, np.int32)}

    ws, gather = fn("umi_conv_wgrad_ws_bytes"), fn("umi_conv_gather_bnred_rows")
    a, b = [], []
    for ci, co, (r, s, st, pad), (n, h, w) in itertools.product(CHANNELS, CHANNELS, GEOMETRIES, SHAPES):
        ho, wo = _out(h, pad, r, st), _out(w, pad, s, st)
        a.append([ws(n, ho, wo, ci, co, r, s, dt, fl) for fl in (0, 2) for dt in (F16, F32)])
        b.append([gather(n, h, w, ci, co, r, s, st, pad, ho, wo, ci, co, F16, fl) for fl in (0, 4)])
    t["wgrad_ws"], t["gather_rows"] = np.asarray(a, np.int64), np.asarray(b, np.int32)

    hrows, hws = fn("umi_head_dgrad_bnred_rows"), fn("umi_head_bwd_fused_ws_bytes")
    a, b = [], []
    for ci, co, (n, h, w) in itertools.product(CHANNELS, CHANNELS, SHAPES):
        a.append([hrows(n * h * w, ci, co, co + e, dt) for e in LD_EXTRA for dt in (F16, F32)])
        b.append(hws(n * h * w, ci, co))
    t["head_rows"], t["head_ws"] = np.asarray(a, np.int32), np.asarray(b, np.int64)
    return t
