"""Host-side contract of the opt-in fp32 matrix-core pointwise path (UMI_CONV_F32_MFMA_1X1 = 32, compute_dtype "fp32_mfma_gemm"):
where the plan names it, and that the flag is IGNORED -- the answer is the flag-less one -- wherever the new kernels do not apply,
independently of the 3x3 flag (16).  Pure host code of libunetmi: no GPU is touched.  The flag-less answers themselves are pinned by
tests/test_dispatch_table.py, the 3x3 flag's by tests/test_conv_f32_mfma_plan.py."""
import ctypes
import itertools

import pytest

from tests.dispatch_grid import F16, F32, GEOMETRIES, SHAPES

F32_MFMA, F32_GEMM, UPSAMPLE2, FORCE_GENERIC, DGRAD_STRIDED, ACCUMULATE = 16, 32, 1, 2, 4, 8
ELIGIBLE = (8, 16, 24, 32, 64, 96, 128, 512, 768, 1024, 3072)
NARROW = (1, 2, 3, 4)
UNSUPPORTED = -2
POINTWISE = (1, 1, 1, 0)


def _plan(n, h, w, ci, co, geo=POINTWISE, flags=0, din=F32, dout=F32, ldx=None, ldy=None, has_bias=0):
    from umi import lib
    r, s, st, pad = geo
    lay, rows = ctypes.c_int(-7), ctypes.c_int(-7)
    status = lib.fn("umi_conv_fwd_plan")(n, h, w, ci, co, r, s, st, pad, ldx or ci, ldy or co, din, dout, flags, has_bias,
                                         ctypes.byref(lay), ctypes.byref(rows))
    return status, lay.value, rows.value


def test_names_and_constants():
    import torch
    import Model
    from umi import lib
    assert lib.CONV_F32_MFMA_1X1 == F32_GEMM and lib.CONV_F32_MFMA == F32_MFMA
    assert Model._resolve_dtype("fp32_mfma_gemm") is torch.float32
    with pytest.raises(ValueError, match="fp32_mfma_gemm"):
        Model._resolve_dtype("fp33")
    assert Model._resolve_conv_flags("fp32_mfma_gemm") == (F32_MFMA, F32_GEMM)
    assert Model._resolve_conv_flags("fp32_mfma") == (F32_MFMA, 0)
    assert Model._resolve_conv_flags("fp32") == (0, 0) and Model._resolve_conv_flags("fp16") == (0, 0)


def test_the_tape_helper_returns_the_flag_that_fits_the_geometry():
    import torch
    from umi import graph
    t = graph.Tape(torch.float32, training=True, record=False)
    assert t._fk(1, 1, 1, 0, 64, 64) == 0 and t._fk(3, 3, 1, 1, 64, 64) == 0           # no mode set: no flags
    t.conv3x3_flags, t.conv1x1_flags = F32_MFMA, F32_GEMM
    assert t._fk(3, 3, 1, 1, 64, 3) == F32_MFMA and t._fk(3, 3, 1, 1, 3, 64) == 0
    assert t._fk(1, 1, 1, 0, 64, 128) == F32_GEMM
    assert t._fk(1, 1, 1, 0, 64, 3) == 0 and t._fk(1, 1, 1, 0, 3, 64) == 0
    for geo in GEOMETRIES:
        if geo not in (POINTWISE, (3, 3, 1, 1)):
            assert t._fk(*geo, 64, 64) == 0, geo
    t.conv1x1_flags = 0                                                                  # "fp32_mfma": the 3x3 flag alone
    assert t._fk(3, 3, 1, 1, 64, 64) == F32_MFMA and t._fk(1, 1, 1, 0, 64, 64) == 0


def test_plan_names_the_new_path_on_eligible_problems():
    differs = 0
    for ci, co, (n, h, w), e, hb in itertools.product(ELIGIBLE, ELIGIBLE, SHAPES, (0, 4, 8), (0, 1)):
        status, lay, rows = _plan(n, h, w, ci, co, flags=F32_GEMM, ldx=ci + e, ldy=co + e, has_bias=hb)
        # layout 0: umi_pack_kn's [1][Ci][Co]; one statistics row per 128 consecutive output rows
        assert (status, lay) == (0, 0), (ci, co, n, h, w, e, hb)
        assert rows == -(-(n * h * w) // 128) >= 1, (ci, co, n, h, w, e, hb)
        plain = _plan(n, h, w, ci, co, flags=0, ldx=ci + e, ldy=co + e, has_bias=hb)
        assert plain[0] == 0
        differs += plain[2] != rows
    assert differs > 0          # the generic kernel reports one row per 64 pixels: the plan's answer shows which path it names


def _assert_ignored(flags_extra=0, flag=F32_GEMM, **kw):
    with_flag = _plan(flags=flag | flags_extra, **kw)
    assert with_flag == _plan(flags=flags_extra, **kw), (flags_extra, kw)
    return with_flag


def test_flag_is_ignored_on_narrow_channels():
    for (n, h, w), c, wide in itertools.product(SHAPES, NARROW, (8, 64)):
        _assert_ignored(n=n, h=h, w=w, ci=c, co=wide)
        _assert_ignored(n=n, h=h, w=w, ci=wide, co=c)


def test_flag_is_ignored_with_an_fp16_side():
    for (n, h, w), c, (din, dout) in itertools.product(SHAPES, (8, 64, 128), ((F16, F16), (F16, F32))):
        _assert_ignored(n=n, h=h, w=w, ci=c, co=c, din=din, dout=dout)


def test_flag_is_ignored_on_every_other_geometry():
    for geo, (n, h, w), c, dt in itertools.product(GEOMETRIES, SHAPES, (8, 64, 128), (F32, F16)):
        if geo == POINTWISE:
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


def test_the_two_flags_are_independent():
    both = F32_MFMA | F32_GEMM
    for (n, h, w), ci, co, hb in itertools.product(SHAPES, (3, 8, 64, 96), (4, 8, 64, 128), (0, 1)):
        kw = dict(n=n, h=h, w=w, ci=ci, co=co, has_bias=hb)
        assert _plan(flags=both, geo=(3, 3, 1, 1), **kw) == _plan(flags=F32_MFMA, geo=(3, 3, 1, 1), **kw)
        assert _plan(flags=both, geo=POINTWISE, **kw) == _plan(flags=F32_GEMM, geo=POINTWISE, **kw)
        # each flag alone on the other geometry: ignored
        assert _plan(flags=F32_GEMM, geo=(3, 3, 1, 1), **kw) == _plan(flags=0, geo=(3, 3, 1, 1), **kw)
        assert _plan(flags=F32_MFMA, geo=POINTWISE, **kw) == _plan(flags=0, geo=POINTWISE, **kw)
    ws = _ws()
    for (n, h, w), c in itertools.product(SHAPES, (8, 64, 96)):
        assert ws(n, h, w, c, c, 3, 3, F32, both) == ws(n, h, w, c, c, 3, 3, F32, F32_MFMA)
        assert ws(n, h, w, c, c, 1, 1, F32, both) == ws(n, h, w, c, c, 1, 1, F32, F32_GEMM)


def _ws():
    from umi import lib
    return lib.fn("umi_conv_wgrad_ws_bytes")


def _split_slabs(m, ci, co):
    """The split rule as include/unetmi.h states it."""
    ti, tj = (64 if ci <= 64 else 128), (64 if co <= 64 else 128)
    tiles = -(-ci // ti) * -(-co // tj)
    chunks = -(-m // 32)
    want = max(1, min(-(-512 // tiles), -(-chunks // 4)))
    per = -(-chunks // want)
    return -(-chunks // per)


def test_wgrad_workspace():
    ws = _ws()
    grew = 0
    for (n, h, w), ci, co in itertools.product(SHAPES, ELIGIBLE, ELIGIBLE):
        got, plain = ws(n, h, w, ci, co, 1, 1, F32, F32_GEMM), ws(n, h, w, ci, co, 1, 1, F32, 0)
        slabs = _split_slabs(n * h * w, ci, co) * ci * co * 4                          # whole slabs [1][ci][co]
        assert got == max(plain, slabs) > 0, (n, h, w, ci, co)       # the call may still find the flag refused (row strides)
        grew += got > plain
        assert ws(n, h, w, ci, co, 1, 1, F16, F32_GEMM) == ws(n, h, w, ci, co, 1, 1, F16, 0)
        assert ws(n, h, w, ci, co, 3, 3, F32, F32_GEMM) == ws(n, h, w, ci, co, 3, 3, F32, 0)
        assert ws(n, h, w, ci, co, 1, 1, F32, F32_GEMM | FORCE_GENERIC) == ws(n, h, w, ci, co, 1, 1, F32, FORCE_GENERIC)
    assert grew > 0
    for c in NARROW:
        assert ws(2, 16, 24, c, 64, 1, 1, F32, F32_GEMM) == ws(2, 16, 24, c, 64, 1, 1, F32, 0)
        assert ws(2, 16, 24, 64, c, 1, 1, F32, F32_GEMM) == ws(2, 16, 24, 64, c, 1, 1, F32, 0)
