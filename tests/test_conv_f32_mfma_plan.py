"""Host-side contract of the opt-in fp32 matrix-core 3x3 path (UMI_CONV_F32_MFMA = 16, compute_dtype "fp32_mfma"): where the
plan names it, and that the flag is IGNORED -- the answer is the flag-less one -- wherever the new kernels do not apply.  Pure host
code of libunetmi: no GPU is touched.  The flag-less answers themselves are pinned by tests/test_dispatch_table.py."""
import ctypes
import itertools

import pytest

from tests.dispatch_grid import F16, F32, GEOMETRIES, SHAPES

F32_MFMA, UPSAMPLE2, FORCE_GENERIC, DGRAD_STRIDED, ACCUMULATE = 16, 1, 2, 4, 8
ELIGIBLE = (8, 16, 24, 32, 64, 96, 128, 512, 1024)
NARROW = (1, 2, 3, 4)
UNSUPPORTED = -2


def _plan(n, h, w, ci, co, geo=(3, 3, 1, 1), flags=0, din=F32, dout=F32, ldx=None, ldy=None, has_bias=0):
    from umi import lib
    r, s, st, pad = geo
    lay, rows = ctypes.c_int(-7), ctypes.c_int(-7)
    status = lib.fn("umi_conv_fwd_plan")(n, h, w, ci, co, r, s, st, pad, ldx or ci, ldy or co, din, dout, flags, has_bias,
                                         ctypes.byref(lay), ctypes.byref(rows))
    return status, lay.value, rows.value


def test_compute_dtype_names():
    import torch
    import Model
    assert Model._resolve_dtype("fp32_mfma") is torch.float32
    assert Model._resolve_dtype("fp32") is torch.float32 and Model._resolve_dtype("fp16") is torch.float16
    with pytest.raises(ValueError):
        Model._resolve_dtype("fp33")
    from umi import lib
    assert lib.CONV_F32_MFMA == F32_MFMA
    assert Model._resolve_conv_flags("fp32_mfma")[0] == F32_MFMA
    assert Model._resolve_conv_flags("fp32")[0] == 0 and Model._resolve_conv_flags("fp16")[0] == 0


def test_plan_names_the_new_path_on_eligible_problems():
    differs = 0
    for ci, co, (n, h, w), e in itertools.product(ELIGIBLE, ELIGIBLE, SHAPES, (0, 4, 8)):
        status, lay, rows = _plan(n, h, w, ci, co, flags=F32_MFMA, ldx=ci + e, ldy=co + e)
        # layout 0: umi_pack_kn's [tap][k][n]; one statistics row per 8 x 32 pixel tile
        assert (status, lay) == (0, 0), (ci, co, n, h, w, e)
        assert rows == n * -(-h // 8) * -(-w // 32) >= 1, (ci, co, n, h, w, e)
        plain = _plan(n, h, w, ci, co, flags=0, ldx=ci + e, ldy=co + e)
        assert plain[0] == 0
        differs += plain[2] != rows
    assert differs > 0          # the generic kernel reports one row per 64 pixels: the plan's answer shows which path it names


def _assert_ignored(flags_extra=0, **kw):
    with_flag = _plan(flags=F32_MFMA | flags_extra, **kw)
    assert with_flag == _plan(flags=flags_extra, **kw), (flags_extra, kw)
    return with_flag


def test_flag_is_ignored_on_narrow_channels():
    for (n, h, w), c, wide in itertools.product(SHAPES, NARROW, (8, 64)):
        _assert_ignored(n=n, h=h, w=w, ci=c, co=wide)
        _assert_ignored(n=n, h=h, w=w, ci=wide, co=c)


def test_flag_is_ignored_with_an_fp16_side():
    for (n, h, w), c, (din, dout) in itertools.product(SHAPES, (8, 64, 128), ((F16, F16), (F16, F32))):
        _assert_ignored(n=n, h=h, w=w, ci=c, co=c, din=din, dout=dout)


def test_flag_is_ignored_with_a_bias():
    for (n, h, w), c in itertools.product(SHAPES, (8, 64)):
        _assert_ignored(n=n, h=h, w=w, ci=c, co=2 * c, has_bias=1)


def test_flag_is_ignored_on_every_other_geometry():
    for geo, (n, h, w), c, dt in itertools.product(GEOMETRIES, SHAPES, (8, 64, 128), (F32, F16)):
        if geo == (3, 3, 1, 1):
            continue
        _assert_ignored(n=n, h=h, w=w, ci=c, co=c, geo=geo, din=dt, dout=dt)


@pytest.mark.parametrize("other", [UPSAMPLE2, FORCE_GENERIC, DGRAD_STRIDED])
def test_flag_is_ignored_beside_the_other_flags(other):
    for geo, (n, h, w), c in itertools.product(GEOMETRIES, SHAPES, (8, 64)):
        _assert_ignored(other, n=n, h=h, w=w, ci=c, co=c, geo=geo)


def test_flag_is_ignored_on_a_row_stride_that_is_no_multiple_of_four():
    for (n, h, w), c in itertools.product(SHAPES, (8, 64)):
        _assert_ignored(n=n, h=h, w=w, ci=c, co=c, ldx=c + 2)
        _assert_ignored(n=n, h=h, w=w, ci=c, co=c, ldy=c + 2)


def test_accumulate_stays_unsupported():
    for (n, h, w), c in itertools.product(SHAPES, (8, 64)):
        got = _assert_ignored(ACCUMULATE, n=n, h=h, w=w, ci=c, co=c)
        assert got[0] == UNSUPPORTED


def test_wgrad_workspace():
    from umi import lib
    ws = lib.fn("umi_conv_wgrad_ws_bytes")
    for (n, h, w), ci, co in itertools.product(SHAPES, ELIGIBLE, ELIGIBLE):
        got = ws(n, h, w, ci, co, 3, 3, F32, F32_MFMA)
        assert got > 0 and got % (9 * ci * co * 4) == 0, (n, h, w, ci, co)          # whole slabs [tap][ci][co]
        assert got >= ws(n, h, w, ci, co, 3, 3, F32, 0)          # the call may still find the flag refused (row strides)
        assert ws(n, h, w, ci, co, 3, 3, F16, F32_MFMA) == ws(n, h, w, ci, co, 3, 3, F16, 0)
        assert ws(n, h, w, ci, co, 3, 3, F32, F32_MFMA | FORCE_GENERIC) == ws(n, h, w, ci, co, 3, 3, F32, FORCE_GENERIC)
    for c in NARROW:
        assert ws(2, 16, 24, c, 64, 3, 3, F32, F32_MFMA) == ws(2, 16, 24, c, 64, 3, 3, F32, 0)
        assert ws(2, 16, 24, 64, 64, 1, 1, F32, F32_MFMA) == ws(2, 16, 24, 64, 64, 1, 1, F32, 0)
