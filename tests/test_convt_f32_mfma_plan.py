"""Host-side contract of the opt-in fp32 matrix-core ConvTranspose2d(2, 2) path (UMI_CONV_F32_MFMA_2X2 = 64, compute_dtype
"fp32_mfma_convt"): where the plan names it, and that the flag is IGNORED -- the answer is the flag-less one -- wherever the new
kernels do not apply, independently of the 3x3 flag (16) and the pointwise flag (32).  Pure host code of libunetmi: no GPU is touched.
The flag-less answers themselves are pinned by tests/test_dispatch_table.py, the two older flags' by tests/test_conv_f32_mfma_plan.py
and tests/test_gemm_f32_mfma_plan.py."""
import ctypes
import itertools

import pytest

from tests.dispatch_grid import F16, F32, GEOMETRIES, SHAPES

F32_MFMA, F32_GEMM, F32_CONVT, UPSAMPLE2, FORCE_GENERIC, DGRAD_STRIDED, ACCUMULATE = 16, 32, 64, 1, 2, 4, 8
ELIGIBLE = (8, 16, 24, 40, 64, 96, 136, 512, 1024)
NARROW = (1, 2, 3, 4)
UNSUPPORTED = -2
TWO = (2, 2, 2, 0)
ODD_SHAPES = ((1, 9, 8), (2, 16, 23), (1, 7, 7))           # N, H, W of the input of a 2x2 / stride-2 convolution


def _plan(n, h, w, ci, co, geo=TWO, flags=0, din=F32, dout=F32, ldx=None, ldy=None, has_bias=0):
    from umi import lib
    r, s, st, pad = geo
    lay, rows = ctypes.c_int(-7), ctypes.c_int(-7)
    status = lib.fn("umi_conv_fwd_plan")(n, h, w, ci, co, r, s, st, pad, ldx or ci, ldy or co, din, dout, flags, has_bias,
                                         ctypes.byref(lay), ctypes.byref(rows))
    return status, lay.value, rows.value


def test_names_and_constants(monkeypatch):
    import torch
    import Model
    from umi import lib
    assert lib.CONV_F32_MFMA_2X2 == F32_CONVT and lib.CONV_F32_MFMA_1X1 == F32_GEMM and lib.CONV_F32_MFMA == F32_MFMA
    assert Model._resolve_dtype("fp32_mfma_convt") is torch.float32
    with pytest.raises(ValueError) as e:
        Model._resolve_dtype("fp33")
    for mode in ("fp16", "fp32", "fp32_mfma", "fp32_mfma_gemm", "fp32_mfma_attn", "fp32_mfma_convt"):
        assert mode in str(e.value)
    assert Model._resolve_convt_flags("fp32_mfma_convt") == F32_CONVT
    for mode in ("fp16", "fp32", "fp32_mfma", "fp32_mfma_gemm", "fp32_mfma_attn"):
        assert Model._resolve_convt_flags(mode) == 0, mode
    # the top of the cumulative chain: "fp32_mfma_attn" plus the new flag
    assert Model._resolve_conv_flags("fp32_mfma_convt") == Model._resolve_conv_flags("fp32_mfma_attn") == (F32_MFMA, F32_GEMM)
    assert Model._resolve_attn_flags("fp32_mfma_convt") == Model._resolve_attn_flags("fp32_mfma_attn") == lib.UMI_ATTN_F32_MFMA
    monkeypatch.setenv("UMI_COMPUTE_DTYPE", "fp32_mfma_convt")
    assert Model._resolve_dtype(None) is torch.float32 and Model._resolve_convt_flags(None) == F32_CONVT
    monkeypatch.setenv("UMI_COMPUTE_DTYPE", "fp32_mfma_attn")
    assert Model._resolve_convt_flags(None) == 0


def test_the_tape_carries_the_flag_apart_from_the_geometry_helper():
    import torch
    from umi import graph
    t = graph.Tape(torch.float32, training=True, record=False)
    assert t.convt_flags == 0
    t.convt_flags = F32_CONVT
    for geo in GEOMETRIES:                                  # Tape._fk's answers do not change: conv_transpose2x2 adds the flag itself
        assert t._fk(*geo, 64, 64) == 0, geo


def test_plan_names_the_new_paths_on_eligible_problems():
    for ci, co, (n, h, w), e, hb, up in itertools.product(ELIGIBLE, ELIGIBLE, SHAPES, (0, 4, 8), (0, 1), (0, UPSAMPLE2)):
        kw = dict(n=n, h=h, w=w, ci=ci, co=co, ldx=ci + e, ldy=co + e, has_bias=hb)
        # layout 0: umi_pack_kn's [4][K][N]; these kernels write no statistics
        assert _plan(flags=F32_CONVT | up, **kw) == (0, 0, 0), (kw, up)
        plain = _plan(flags=up, **kw)
        assert plain[0] == 0 and plain[2] >= 1, (kw, up)    # every flag-less path reports rows: the answer shows which is named


def _assert_ignored(flags_extra=0, flag=F32_CONVT, **kw):
    with_flag = _plan(flags=flag | flags_extra, **kw)
    assert with_flag == _plan(flags=flags_extra, **kw), (flags_extra, kw)
    return with_flag


def test_flag_is_ignored_on_narrow_channels():
    for (n, h, w), c, wide, up in itertools.product(SHAPES, NARROW, (8, 64), (0, UPSAMPLE2)):
        _assert_ignored(up, n=n, h=h, w=w, ci=c, co=wide)
        _assert_ignored(up, n=n, h=h, w=w, ci=wide, co=c)


def test_flag_is_ignored_with_an_fp16_side():
    for (n, h, w), c, (din, dout), up in itertools.product(SHAPES, (8, 64, 128), ((F16, F16), (F16, F32)), (0, UPSAMPLE2)):
        _assert_ignored(up, n=n, h=h, w=w, ci=c, co=c, din=din, dout=dout)


def test_flag_is_ignored_on_every_other_geometry():
    for geo, (n, h, w), c, dt, up in itertools.product(GEOMETRIES, SHAPES, (8, 64, 128), (F32, F16), (0, UPSAMPLE2)):
        if geo == TWO:
            continue
        _assert_ignored(up, n=n, h=h, w=w, ci=c, co=c, geo=geo, din=dt, dout=dt)


def test_flag_is_ignored_on_an_odd_image_without_upsample():
    """The data gradient's geometry is H == 2 Ho and W == 2 Wo: a 2x2 / stride-2 convolution that drops a row or a column is not it.
    (With UPSAMPLE2 the image is the ConvT's input: any size is taken.)"""
    for (n, h, w), c in itertools.product(ODD_SHAPES, (8, 64)):
        _assert_ignored(n=n, h=h, w=w, ci=c, co=c)
        assert _plan(n, h, w, c, c, flags=F32_CONVT | UPSAMPLE2) == (0, 0, 0)


@pytest.mark.parametrize("other", [FORCE_GENERIC, DGRAD_STRIDED])
def test_flag_is_ignored_beside_the_other_flags(other):
    for geo, (n, h, w), c, up in itertools.product(GEOMETRIES, SHAPES, (8, 64), (0, UPSAMPLE2)):
        _assert_ignored(other | up, n=n, h=h, w=w, ci=c, co=c, geo=geo)


def test_flag_is_ignored_on_a_row_stride_that_is_no_multiple_of_four():
    for (n, h, w), c, up in itertools.product(SHAPES, (8, 64), (0, UPSAMPLE2)):
        _assert_ignored(up, n=n, h=h, w=w, ci=c, co=c, ldx=c + 2)
        _assert_ignored(up, n=n, h=h, w=w, ci=c, co=c, ldy=c + 2)


def test_accumulate_stays_unsupported():
    for (n, h, w), c, up in itertools.product(SHAPES, (8, 64), (0, UPSAMPLE2)):
        got = _assert_ignored(ACCUMULATE | up, n=n, h=h, w=w, ci=c, co=c)
        assert got[0] == UNSUPPORTED


def test_the_three_flags_are_pairwise_independent():
    own = {(3, 3, 1, 1): F32_MFMA, (1, 1, 1, 0): F32_GEMM, TWO: F32_CONVT}
    every = F32_MFMA | F32_GEMM | F32_CONVT
    for (n, h, w), ci, co, hb in itertools.product(SHAPES, (3, 8, 64, 96), (4, 8, 64, 128), (0, 1)):
        kw = dict(n=n, h=h, w=w, ci=ci, co=co, has_bias=hb)
        for geo, mine in own.items():
            named = _plan(flags=mine, geo=geo, **kw)
            assert _plan(flags=every, geo=geo, **kw) == named
            for other in own.values():
                if other != mine:
                    assert _plan(flags=mine | other, geo=geo, **kw) == named          # a second flag changes nothing
                    assert _plan(flags=other, geo=geo, **kw) == _plan(flags=0, geo=geo, **kw)     # alone on another geometry: ignored
        assert _plan(flags=every | UPSAMPLE2, **kw) == _plan(flags=F32_CONVT | UPSAMPLE2, **kw)
    ws = _ws()
    for (n, h, w), c in itertools.product(SHAPES, (8, 64, 96)):
        for (r, s, _, _), mine in own.items():
            assert ws(n, h, w, c, c, r, s, F32, every) == ws(n, h, w, c, c, r, s, F32, mine)
            for other in own.values():
                if other != mine:
                    assert ws(n, h, w, c, c, r, s, F32, other) == ws(n, h, w, c, c, r, s, F32, 0)


def _ws():
    from umi import lib
    return lib.fn("umi_conv_wgrad_ws_bytes")


def _split_slabs(m, ci, co):
    """The split rule as include/unetmi.h states it: the four taps count as tiles."""
    ti, tj = (64 if ci <= 64 else 128), (64 if co <= 64 else 128)
    tiles = 4 * -(-ci // ti) * -(-co // tj)
    chunks = -(-m // 32)
    want = max(1, min(-(-512 // tiles), -(-chunks // 4)))
    per = -(-chunks // want)
    return -(-chunks // per)


def test_wgrad_workspace():
    ws = _ws()
    grew = 0
    for (n, ho, wo), ci, co in itertools.product(SHAPES, ELIGIBLE, ELIGIBLE):
        got, plain = ws(n, ho, wo, ci, co, 2, 2, F32, F32_CONVT), ws(n, ho, wo, ci, co, 2, 2, F32, 0)
        slabs = _split_slabs(n * ho * wo, ci, co) * 4 * ci * co * 4                     # whole slabs [4][ci][co]
        assert got == max(plain, slabs) > 0, (n, ho, wo, ci, co)     # the call may still find the flag refused (row strides)
        grew += got > plain
        assert ws(n, ho, wo, ci, co, 2, 2, F16, F32_CONVT) == ws(n, ho, wo, ci, co, 2, 2, F16, 0)
        assert ws(n, ho, wo, ci, co, 3, 3, F32, F32_CONVT) == ws(n, ho, wo, ci, co, 3, 3, F32, 0)
        assert ws(n, ho, wo, ci, co, 1, 1, F32, F32_CONVT) == ws(n, ho, wo, ci, co, 1, 1, F32, 0)
        assert ws(n, ho, wo, ci, co, 2, 2, F32, F32_CONVT | FORCE_GENERIC) == ws(n, ho, wo, ci, co, 2, 2, F32, FORCE_GENERIC)
    assert grew > 0
    for c in NARROW:
        assert ws(2, 16, 24, c, 64, 2, 2, F32, F32_CONVT) == ws(2, 16, 24, c, 64, 2, 2, F32, 0)
        assert ws(2, 16, 24, 64, c, 2, 2, F32, F32_CONVT) == ws(2, 16, 24, 64, c, 2, 2, F32, 0)
