"""The fp32 VALU kernel family of csrc/generic_kernels.hip -- what compute_dtype="fp32" runs on, and the in-library yardstick of
every faster path -- against the float64 statement of tests/valu_f32_ref.py (itself pinned on the CPU by
tests/test_valu_f32_ref.py), kernel by kernel, through umi.ops with fp32 tensors and flags = 0 as the tape calls them.

Two kinds of case per operation.
  Exact.  Small-integer operands (the builders of tests/test_gpu_exact.py): every product and every partial sum stays below
  2^24, so fp32 is exact in ANY order and the kernel must reproduce the float64 result bit for bit -- indexing, tile edges, halo,
  K tails, split-K chunk edges, strides and slices at zero tolerance.  Every such test first asserts the precondition on the
  reference alone: the magnitude sum (which bounds every partial sum of every grouping) is below 2^24.
  Rounding.  Standard-normal operands against float64 inside a bound DERIVED from the arithmetic, never from what the kernels
  return.  u = 2^-24, gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, 3.1 / 3.4: n rounded
  operations on a term, in any summation order, perturb it by at most gamma_n):
    contractions      |got - ref| <= gamma_{K+3} * m element by element; K = the products per output (R*S*Ci forward, R*S*Co for a
                      data gradient, Ci for the transposed convolution whose outputs each see one tap, the pixel count for a weight
                      gradient, whose bar is doubled for the merged split-K partial sums as tests/test_gpu_conv_f32_mfma.py doubles
                      its own); the 3 further roundings are the transform's fma, the bias add and out_scale;
                      m = sum (|v| |scale| + |shift|) |w| (+ |bias|) over the same terms;
    statistics rows   gamma_64 * sum |term|: a row is 64 pixels, 4 added per thread then 16 partial sums (conv_generic_kernel's
                      epilogue), and the rows are added in float64 here;
    colsum            gamma_n * sum |x|, n = the rows of one split of colsum_plan (colsum1_kernel adds them in fp32: a quarter per
                      row lane, then the four lanes; the splits are added in double);
    BatchNorm sums    gamma_257 * sum |dz| and gamma_258 * sum |dz xhat|: one stage-1 block of 256 rows in fp32 (bn_bwd_reduce1_kernel)
                      plus the fma / the final cast, later stages in double;
    BatchNorm apply   8 u * |scale| (|dz| + |c1| + |xhat c2|): umi_bn_dz (csrc/common.h) and its caller round 8 times -- 1 / count,
                      c1 = sum_dz / count, c2 = sum_dzx / count, y - mean, * rstd, dz - c1, the fma, the product with scale -- and
                      no term passes through more than 6 of them (gamma_6 < 8 u).
  Every rounding check prints the fraction of its bound it used.

The ReLU mask z > floor of the BatchNorm backward is a discontinuity.  The reference forms z in float64 from the SAME fp32 y, scale
and shift: the product of two fp32 values is exact in float64, the sum is then rounded once to 53 bits where the kernel's fmaf
rounds it once to 24, and rounding is monotone and keeps the sign of z - floor for the floors in use (0 and -inf).  The masks
agree by construction and no case is left out.

There is no fp32 umi_bn_stats: the separate statistics pass exists for fp16 producers without a statistics epilogue and refuses
UMI_F32 (ops.bn_stats returns None); the fp32 statistics come from conv_generic_kernel's epilogue, pinned here with the forward.
For fp16 storage see tests/test_gpu_kernels.py."""
import pytest
import torch

from tests import valu_f32_ref as R
from tests.test_gpu_exact import _int_tx, _ints

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXACT = 2 ** 24
F64 = torch.float64
NINF = float("-inf")
SENT = -5.0                      # outside every slice: must survive
STAT_ROW_TERMS = 64              # fp32 additions behind one statistics row (GBP pixels)
BN_BLOCK_ROWS = 256              # BNB_RPB


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from umi import lib, ops
    return lib, ops


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) * (i + 1) for i, k in enumerate(key)) + 11)


def _itx(C, g):
    """_int_tx (scales 1, -1, 2; integer shifts; ReLU) with every third channel consumed without a floor."""
    t = _int_tx(C, g)
    t[2::3, 3] = NINF
    return t


def _ntx(C, g):
    """tests/test_gpu_kernels.py's _tx (a few negative scales), every third channel without a floor."""
    t = torch.empty(C, 4)
    t[:, 0] = 0.3 * torch.randn(C, generator=g)
    t[:, 1] = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.15, -1.0, 1.0)
    t[:, 2] = 0.2 * torch.randn(C, generator=g)
    t[:, 3] = 0.0
    t[2::3, 3] = NINF
    return t


def _vals(shape, g, exact, lo=-2, hi=2):
    return _ints(shape, lo, hi, g) if exact else torch.randn(shape, generator=g)


def _tx(C, g, exact):
    return _itx(C, g) if exact else _ntx(C, g)


def _dev(t):
    return None if t is None else t.to(DEV)


def _sliced(t, pad, dtype=None):
    """`t` on the device as an interior channel slice of a buffer `2 * pad` channels wider (pad = 0: dense); (buffer, view)."""
    t = t if dtype is None else t.to(dtype)
    if not pad:
        d = t.contiguous().to(DEV, copy=True)
        return d, d
    buf = torch.full(t.shape[:-1] + (t.shape[-1] + 2 * pad,), SENT, dtype=t.dtype, device=DEV)
    view = buf[..., pad:pad + t.shape[-1]]
    view.copy_(t.to(DEV))
    return buf, view


def _outside_untouched(buf, pad):
    return pad == 0 or bool((buf[..., :pad] == SENT).all() and (buf[..., buf.shape[-1] - pad:] == SENT).all())


def _within(name, got, ref, bound):
    """|got - ref| <= bound element by element (equality where the bound is zero); prints the largest fraction used."""
    err = (got.detach().cpu().to(F64) - ref).abs()
    assert torch.isfinite(err).all(), name
    zero = bound <= 0
    assert (err[zero] == 0).all(), name
    frac = (err[~zero] / bound[~zero]).max().item() if (~zero).any() else 0.0
    print(f"[valu_f32] {name}: {frac:.4f} of the bound")
    assert frac <= 1.0, (name, frac)


def _same(name, got, ref, bound, exact):
    if exact:
        assert torch.equal(got.detach().cpu().to(F64), ref), name
    else:
        _within(name, got, ref, bound)


def _cdiv(a, b):
    return -(-a // b)


# ---- configuration classes: what the coverage test of the last section reduces a call to ------------------------------------------------
def _k_cls(K):
    """a contraction depth walked 16 at a time, staged 4 at a time"""
    return (K % 4 == 0, K % 16 == 0, K > 16)


def _c_cls(C):
    """a channel count tiled by 64, owned 4 per thread"""
    return (C % 4 == 0, C % 64 == 0, C > 64)


def _p_cls(P):
    return (P % 64 == 0, P > 64)


def _conv_key(kind, K, stride, pad, Ci, Co, P, islice, oslice, tx, bias, stats, off=None):
    return ("conv", kind, K, stride, pad, _k_cls(Ci), _c_cls(Co), _p_cls(P), bool(islice), bool(oslice), bool(tx), bool(bias),
            bool(stats), off)


def wgrad_plan(P, Ci, Co, RS):
    """wgrad_generic_plan (csrc/generic_kernels.hip): aim for 2,048 workgroups, at least 256 pixels per split, chunks a multiple of
    the 16-pixel K step.  Returns (splits, chunk)."""
    tiles = _cdiv(Ci, 64) * _cdiv(Co, 64) * RS
    want = max(1, min(_cdiv(2048, tiles), (P + 255) // 256))
    chunk = _cdiv(_cdiv(P, want), 16) * 16
    return _cdiv(P, chunk), chunk


def _wgrad_key(K, stride, pad, Ci, Co, P, xslice, dyslice, txa, txb, order):
    splits, chunk = wgrad_plan(P, Ci, Co, K * K)
    return ("wgrad", K, stride, pad, _c_cls(Ci), _c_cls(Co), P % 16 == 0, splits > 1, P % chunk == 0, bool(xslice), bool(dyslice),
            bool(txa), bool(txb), order)


def _pool_key(op, H, W, C, xslice, oslice, tx, acc=None):
    return ("pool", op, H % 2, W % 2, C % 4 == 0, C > 4, bool(xslice), bool(oslice), bool(tx), acc)


def _ct(C):
    return 64 if C >= 64 else 1 << (C.bit_length() - 1)


def _bn_key(op, M, C, daslice, yslice):
    return ("bn", op, M % BN_BLOCK_ROWS == 0, M > BN_BLOCK_ROWS, _ct(C), C % _ct(C) == 0, C > 64, bool(daslice), bool(yslice))


def colsum_plan(M, C):
    """colsum_plan (csrc/generic_kernels.hip): (splits, rows per split)."""
    ctiles = _cdiv(C, 64)
    want = max(1, min(_cdiv(1024, ctiles), (M + 31) // 32))
    rps = _cdiv(M, want)
    return _cdiv(M, rps), rps


def _colsum_key(M, C, sliced):
    return ("colsum", _c_cls(C), colsum_plan(M, C)[0] > 1, bool(sliced))


# =============================================================================================================================
# a. convolution forward, conv_generic_kernel<float, float, false, false>
# =============================================================================================================================
def _f(N, H, W, Ci, Co, K=3, stride=1, pad=1, tx=True, bias=False, stats=True, ipad=0, opad=0):
    return (N, H, W, Ci, Co, K, stride, pad, tx, bias, stats, ipad, opad)


FWD_SHAPES = [
    (1, 16, 64, 64, 64), (2, 16, 32, 64, 128), (1, 8, 32, 512, 1024), (1, 8, 32, 1024, 512),
    (2, 11, 37, 96, 128),        # ragged pixel tile
    (1, 20, 45, 48, 72),         # partial channel tile
    (1, 9, 7, 8, 8),             # fewer than 64 pixels
    (1, 1, 1, 8, 16),            # all halo
    (3, 2, 3, 16, 8),
    (2, 37, 29, 1, 64), (1, 16, 48, 3, 64),          # the stem: Ci not a multiple of 4 or 16
]
# what the fp32 training steps of test_model_calls_are_covered call beyond the tables of this section
MODEL_FWD = [
    _f(2, 32, 32, 1, 64, tx=False),                                                   # inc.c1
    _f(2, 16, 16, 64, 128, tx=False), _f(2, 22, 36, 64, 128, tx=False), _f(2, 4, 4, 256, 512, tx=False),      # Down.c1 reads the pool
    _f(2, 16, 16, 128, 128, opad=64), _f(2, 22, 36, 128, 128, opad=64), _f(2, 4, 4, 512, 512, opad=256),      # Down.c2 -> concat half
    _f(2, 2, 2, 1024, 1024),                                                          # down4.c2
    _f(2, 32, 32, 64, 4, K=1, pad=0, bias=True, stats=False),                         # the 4-class head
    _f(2, 32, 32, 2, 64, K=1, pad=0, tx=False, stats=False), _f(2, 32, 32, 4, 64, K=1, pad=0, tx=False, stats=False),   # its data gradient
    # 3x3 data gradients (the forward kernel without transform or statistics), dense and from the concat gradient's halves
    _f(2, 22, 36, 128, 64, tx=False, stats=False), _f(2, 4, 4, 512, 512, tx=False, stats=False),
    _f(2, 32, 32, 64, 64, tx=False, stats=False, ipad=32), _f(2, 8, 8, 256, 256, tx=False, stats=False, ipad=128),
    _f(2, 4, 4, 512, 512, tx=False, stats=False, ipad=256), _f(2, 5, 9, 512, 512, tx=False, stats=False, ipad=256),
]
HEAD_SHAPES = [(2, 16, 24, 64, 2), (1, 9, 7, 64, 3), (1, 8, 8, 16, 1)]       # 1x1 with bias: Co not a multiple of 4
FWD_CASES = (
    [_f(*s) for s in FWD_SHAPES] + [_f(*s, tx=False, stats=False) for s in FWD_SHAPES]
    + [_f(*s, K=1, pad=0, bias=True, stats=False) for s in HEAD_SHAPES]
    + [_f(*s, K=1, pad=0, tx=False, bias=True, stats=False) for s in HEAD_SHAPES[:1]]
    # interior channel slices of wider buffers on either side and on both
    + [_f(2, 11, 37, 24, 40, ipad=4, opad=4), _f(2, 11, 37, 24, 40, tx=False, stats=False, ipad=4, opad=4),
       _f(1, 16, 64, 64, 64, opad=32), _f(1, 8, 32, 128, 64, ipad=0, opad=32), _f(2, 16, 24, 64, 2, K=1, pad=0, bias=True, stats=False, ipad=4)]
    # stride 2
    + [_f(2, 11, 13, 16, 24, stride=2, stats=False), _f(2, 11, 13, 16, 24, K=1, stride=2, pad=0, tx=False, stats=False),
       _f(2, 11, 13, 128, 64, stride=2), _f(2, 11, 13, 128, 64, K=1, stride=2, pad=0, stats=False)]
    + MODEL_FWD
)


def _fwd_id(c):
    return "-".join(str(int(v)) if isinstance(v, (bool, int)) else str(v) for v in c)


def _is_generic(ops, x, y, K, stride, pad, P, flags=0, has_bias=False):
    """The plan names the generic layout: unpacked-k weights (layout 0) and one statistics row per 64-pixel tile."""
    return ops.conv_plan(x, y, K, K, stride, pad, flags, has_bias) == (0, _cdiv(P, 64))


def _run_conv(ops, case, exact, pack_ref=R.pack_conv_fwd, pack_dev="pack_conv_fwd", in_dtype=None, flags=0, name="fwd"):
    N, H, W, Ci, Co, K, stride, pad, use_tx, use_bias, stats, ipad, opad = case
    g = _gen(*case, exact)
    x = _vals((N, H, W, Ci), g, exact)
    if in_dtype is not None:
        x = x.to(in_dtype)
    # the OIHW weight of this forward form; for a data gradient (pack_conv_dgrad) the same tensor read as [out = Ci][in = Co]
    w = _vals((Co, Ci, K, K) if pack_dev != "pack_conv_dgrad" else (Ci, Co, K, K), g, exact, -1, 1)
    b = _vals((Co,), g, exact, -3, 3) if use_bias else None
    t = _tx(Ci, g, exact) if use_tx else None
    Ho, Wo = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    P = N * Ho * Wo
    xbuf, xd = _sliced(x, ipad)
    ybuf, y = _sliced(torch.full((N, Ho, Wo, Co), float("nan")), opad)
    assert _is_generic(ops, xd, y, K, stride, pad, P, flags, use_bias)
    wp = getattr(ops, pack_dev)(w.to(DEV), x.dtype)
    assert torch.equal(wp.cpu().float().view(K * K, Ci, Co), pack_ref(w if in_dtype is None else w.to(in_dtype).float()))
    ref, mag = R.conv_fwd(x, t, wp.cpu(), b, K, K, stride, pad, Co)
    if exact:
        assert mag.max().item() < EXACT and (not stats or (ref * ref).sum((0, 1, 2)).max().item() < EXACT)
    part = ops.conv_fwd(xd, _dev(t), wp, _dev(b), y, K, K, stride, pad, want_stats=stats, flags=flags)
    tag = f"{name} {_fwd_id(case)}"
    _same(tag, y, ref, R.gamma(K * K * Ci + 3) * mag, exact)
    assert _outside_untouched(ybuf, opad) and _outside_untouched(xbuf, ipad)
    if stats:
        rows = part.view(-1, 2, Co)
        assert rows.shape[0] == _cdiv(P, 64)
        tot = rows.cpu().to(F64).sum(0)
        s, q, sa = R.conv_stats(y.cpu())                                # of the STORED output
        _same(tag + " sum", tot[0], s, R.gamma(STAT_ROW_TERMS) * sa, exact)
        _same(tag + " sumsq", tot[1], q, R.gamma(STAT_ROW_TERMS) * q, exact)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "rounding"])
@pytest.mark.parametrize("case", FWD_CASES, ids=_fwd_id)
def test_conv_forward(case, exact):
    """3x3, the 1- and 3-channel stem, the biased 1x1 head and the stride-2 forms: output and statistics rows."""
    lib, ops = _gpu()
    _run_conv(ops, case, exact)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "rounding"])
def test_conv_forward_half_in_float_out(exact):
    """conv_generic_kernel<half_t, float>: fp16 activations and fp16-packed weights to fp32 logits on the head shape.  The narrow
    head kernel would take this call, so the generic one is asked for by flag; its plan row count (one per 64 pixels) is asserted."""
    lib, ops = _gpu()
    case = _f(2, 16, 24, 64, 2, K=1, pad=0, bias=True, stats=False)
    N, H, W, Ci, Co = case[:5]
    g = _gen(*case, exact)
    x = _vals((N, H, W, Ci), g, exact).half()
    w = _vals((Co, Ci, 1, 1), g, exact, -1, 1)
    b = _vals((Co,), g, exact, -3, 3)
    t = _tx(Ci, g, exact)
    xd = x.to(DEV)
    y = torch.full((N, H, W, Co), float("nan"), device=DEV)
    assert _is_generic(ops, xd, y, 1, 1, 0, N * H * W, lib.CONV_FORCE_GENERIC, True)
    wp = ops.pack_conv_fwd(w.to(DEV), torch.float16)
    assert torch.equal(wp.cpu().view(1, Ci, Co), R.pack_conv_fwd(w).half())
    ref, mag = R.conv_fwd(x, t, wp.cpu(), b, 1, 1, 1, 0, Co)
    if exact:
        assert mag.max().item() < EXACT
    ops.conv_fwd(xd, t.to(DEV), wp, b.to(DEV), y, 1, 1, 1, 0, flags=lib.CONV_FORCE_GENERIC)
    _same("fwd half->float", y, ref, R.gamma(Ci + 3) * mag, exact)


# =============================================================================================================================
# b. transposed convolution 2x2 / stride 2 (UPS = true): forward scatter, data gradient, weight and bias gradient
# =============================================================================================================================
MODEL_UPS = [(2, 16, 16, 128, 64), (2, 22, 36, 128, 64), (2, 2, 2, 1024, 512), (2, 2, 4, 1024, 512)]   # (test_model_calls_are_covered)
UPS_SHAPES = [(2, 5, 6, 128, 64), (1, 16, 16, 64, 128), (2, 9, 7, 256, 128), (1, 8, 16, 1024, 512)] + MODEL_UPS
UPS_PLACEMENTS = [((0, 0), (0, 0)), ((0, 0), (1, 1)), ((1, 0), (1, 1)), ((0, 1), (1, 1)), ((0, 0), (1, 0)), ((0, 0), (0, 1))]


def _ups_key(shape, off, extra):
    N, H, W, Ci, Co = shape
    return _conv_key("ups", 2, 2, 0, Ci, Co, N * H * W, False, True, True, True, False, (off != (0, 0), extra != (0, 0)))


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "rounding"])
@pytest.mark.parametrize("place", UPS_PLACEMENTS, ids=lambda p: f"off{p[0][0]}{p[0][1]}-extra{p[1][0]}{p[1][1]}")
@pytest.mark.parametrize("shape", UPS_SHAPES, ids=_fwd_id)
def test_conv_transpose_forward_scatter(shape, place, exact):
    """With bias, into the upper channel half of a concat buffer whose map is `extra` larger than 2H x 2W (the odd-size skips of
    Up), at up_offset `off`: the other half and the border the scatter does not reach keep their sentinel."""
    lib, ops = _gpu()
    N, H, W, Ci, Co = shape
    off, extra = place
    g = _gen(*shape, *off, *extra, exact)
    x, w, b, t = _vals((N, H, W, Ci), g, exact), _vals((Ci, Co, 2, 2), g, exact, -1, 1), _vals((Co,), g, exact, -3, 3), _tx(Ci, g, exact)
    oH, oW = 2 * H + extra[0], 2 * W + extra[1]
    cat = torch.full((N, oH, oW, 2 * Co), SENT, device=DEV)
    dest = cat[..., Co:]
    xd = x.to(DEV)
    assert _is_generic(ops, xd, dest, 2, 2, 0, N * H * W, lib.CONV_UPSAMPLE2, True)
    wp = ops.pack_convT_fwd(w.to(DEV), torch.float32)
    assert torch.equal(wp.cpu().view(4, Ci, Co), R.pack_convT_fwd(w))
    ref, mag, written = R.convT_fwd(x, t, wp.cpu(), b, off, (oH, oW), Co)
    if exact:
        assert mag.max().item() < EXACT
    ops.conv_fwd(xd, t.to(DEV), wp, b.to(DEV), dest, 2, 2, 2, 0, flags=lib.CONV_UPSAMPLE2, up_offset=off)
    got = cat.cpu()
    assert (got[..., :Co] == SENT).all() and (got[..., Co:][~written] == SENT).all()
    _same(f"convT fwd {_fwd_id(shape)}", got[..., Co:][written], ref[written], R.gamma(Ci + 3) * mag[written], exact)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "rounding"])
@pytest.mark.parametrize("gslice", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("shape", UPS_SHAPES, ids=_fwd_id)
def test_conv_transpose_gradients(shape, gslice, exact):
    """The three calls of Tape.conv_transpose2x2's backward in fp32: the data gradient (a 2x2 / stride-2 forward over the upsampled
    map's gradient on pack_convT_dgrad), the weight gradient (conv_wgrad with the operands swapped, written in the parameter's
    (Cin, Cout, 2, 2) order) and the bias gradient (colsum).  The gradient is the concat buffer's upper channel half, or a
    dense crop of it."""
    lib, ops = _gpu()
    N, H, W, Ci, Co = shape
    g = _gen(*shape, exact, 5)
    x, w, t = _vals((N, H, W, Ci), g, exact), _vals((Ci, Co, 2, 2), g, exact, -1, 1), _tx(Ci, g, exact)
    gup = _vals((N, 2 * H, 2 * W, Co), g, exact, -1, 1)
    if gslice:
        gbuf = torch.full((N, 2 * H, 2 * W, 2 * Co), SENT, device=DEV)
        gd = gbuf[..., Co:]
        gd.copy_(gup.to(DEV))
    else:
        gd = gup.to(DEV)
    xd, td = x.to(DEV), t.to(DEV)
    P = N * H * W
    # data gradient
    dx = torch.full((N, H, W, Ci), float("nan"), device=DEV)
    assert _is_generic(ops, gd, dx, 2, 2, 0, P)
    wpd = ops.pack_convT_dgrad(w.to(DEV), torch.float32)
    assert torch.equal(wpd.cpu().view(4, Co, Ci), R.pack_convT_dgrad(w))
    ref, mag = R.conv_fwd(gup, None, wpd.cpu(), None, 2, 2, 2, 0, Ci)
    if exact:
        assert mag.max().item() < EXACT
    ops.conv_fwd(gd, None, wpd, None, dx, 2, 2, 2, 0)
    _same(f"convT dgrad {_fwd_id(shape)}", dx, ref, R.gamma(4 * Co + 3) * mag, exact)
    # weight gradient: x = the gradient map (Cout channels), dy = the transposed convolution's input with its transform
    gw = torch.full((Ci, Co, 2, 2), float("nan"), device=DEV)
    refw, magw = R.conv_wgrad(gup, None, x, t, 2, 2, 2, 0, gw.numel(), Co * 4, 4, 1, 0.5)
    if exact:
        assert magw.max().item() < EXACT
    ops.conv_wgrad(gd, None, xd, td, gw, Co * 4, 4, 1, 0.5, 2, 2, 2, 0)
    _same(f"convT wgrad {_fwd_id(shape)}", gw.view(-1), refw, 2 * R.gamma(P + 3) * magw, exact)
    # bias gradient
    gb = torch.full((Co,), float("nan"), device=DEV)
    refb, magb = R.colsum(gup, 0.5)
    if exact:
        assert magb.max().item() < EXACT
    ops.colsum(gd, gb, 0.5)
    _same(f"convT bias {_fwd_id(shape)}", gb, refb, R.gamma(colsum_plan(4 * P, Co)[1]) * magb, exact)


# =============================================================================================================================
# c. data gradients
# =============================================================================================================================
# forward widths (N, H, W, Ci, Co): the gradient maps Co -> Ci channels
DGRAD_CASES = [(2, 11, 37, 96, 128), (1, 8, 32, 512, 1024), (1, 20, 45, 48, 72), (1, 9, 7, 8, 8)]


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "rounding"])
@pytest.mark.parametrize("case", DGRAD_CASES, ids=_fwd_id)
def test_conv3x3_data_gradient(case, exact):
    """The forward kernel on pack_conv_dgrad's rotated / transposed panel = the data gradient of the 3x3 / pad-1 convolution."""
    lib, ops = _gpu()
    N, H, W, Ci, Co = case
    _run_conv(ops, _f(N, H, W, Co, Ci, tx=False, stats=False), exact, R.pack_conv_dgrad, "pack_conv_dgrad", name="dgrad")


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "rounding"])
@pytest.mark.parametrize("chan", [(16, 24), (128, 64)], ids=_fwd_id)
@pytest.mark.parametrize("hw", [(11, 13), (12, 12)], ids=_fwd_id)
@pytest.mark.parametrize("geom", [(3, 1), (1, 0)], ids=_fwd_id)
def test_strided_data_gradient(geom, hw, chan, exact):
    """conv_generic_kernel<float, float, false, true>: the stride-2 data gradients (a pixel takes tap (r, s) where (h + pad - r,
    w + pad - s) is twice an output position), called as the TransUNet tape calls them."""
    lib, ops = _gpu()
    from umi.graph_tu import TUTape
    (K, pad), (H, W), (Ci, Co) = geom, hw, chan
    N = 2
    Ho, Wo = (H + 2 * pad - K) // 2 + 1, (W + 2 * pad - K) // 2 + 1
    g = _gen(K, pad, H, W, Ci, Co, exact)
    w, dy = _vals((Co, Ci, K, K), g, exact, -1, 1), _vals((N, Ho, Wo, Co), g, exact, -1, 1)
    dyd = dy.to(DEV)
    dx = torch.full((N, H, W, Ci), float("nan"), device=DEV)
    assert ops.conv_plan(dyd, dx, K, K, 2, pad, lib.CONV_DGRAD_STRIDED)[0] == 0
    wpd = ops.pack_conv_dgrad_strided(w.to(DEV), torch.float32)
    assert torch.equal(wpd.cpu().view(K * K, Co, Ci), R.pack_conv_dgrad_strided(w))
    ref, mag = R.conv_dgrad_strided(dy, wpd.cpu(), K, K, 2, pad, (H, W), Ci)
    if exact:
        assert mag.max().item() < EXACT
    TUTape._strided_dgrad(dyd, wpd, dx, K, K, 2, pad)
    _same(f"dgrad strided {K}-{pad}-{H}-{W}-{Ci}-{Co}", dx, ref, R.gamma(K * K * Co + 3) * mag, exact)


# =============================================================================================================================
# d. weight gradient, wgrad_generic_kernel<float> and its split-K reduction
# =============================================================================================================================
def _w(N, H, W, Ci, Co, K=3, stride=1, pad=1, txa=True, txb=False, order="oihw", xpad=0, dypad=0, splits=None):
    return (N, H, W, Ci, Co, K, stride, pad, txa, txb, order, xpad, dypad, splits)


MODEL_WGRAD = [                  # (test_model_calls_are_covered; dypad: the gradient is a half of a concat buffer's gradient)
    _w(2, 32, 32, 1, 64, txa=False), _w(2, 44, 72, 1, 64, txa=False),
    _w(2, 32, 32, 64, 64), _w(2, 32, 32, 64, 64, dypad=32), _w(2, 44, 72, 64, 64), _w(2, 44, 72, 64, 64, dypad=32),
    _w(2, 32, 32, 128, 64), _w(2, 44, 72, 128, 64),
    _w(2, 16, 16, 64, 128, txa=False), _w(2, 22, 36, 64, 128, txa=False),
    _w(2, 16, 16, 128, 128), _w(2, 16, 16, 128, 128, dypad=64), _w(2, 22, 36, 128, 128), _w(2, 22, 36, 128, 128, dypad=64),
    _w(2, 11, 18, 128, 256, txa=False), _w(2, 11, 18, 256, 256), _w(2, 11, 18, 256, 256, dypad=128),
    _w(2, 4, 4, 256, 512, txa=False), _w(2, 4, 4, 512, 512, dypad=256), _w(2, 5, 9, 512, 512, dypad=256),
    _w(2, 2, 2, 512, 1024, txa=False), _w(2, 2, 2, 1024, 1024),
    _w(2, 32, 32, 64, 4, K=1, pad=0), _w(2, 44, 72, 64, 4, K=1, pad=0), _w(2, 44, 72, 64, 2, K=1, pad=0),
    # the transposed convolution's (operands swapped: x = the upsampled map's gradient, a concat half)
    _w(2, 32, 32, 64, 128, K=2, stride=2, pad=0, txa=False, txb=True, xpad=32),
    _w(2, 44, 72, 64, 128, K=2, stride=2, pad=0, txa=False, txb=True, xpad=32),
    _w(2, 22, 36, 128, 256, K=2, stride=2, pad=0, txa=False, txb=True, xpad=64),
]
WGRAD_CASES = [
    _w(2, 20, 45, 32, 64), _w(1, 16, 64, 64, 128),
    _w(1, 10, 40, 72, 24),                                   # partial tiles on both sides
    _w(1, 8, 32, 1024, 512, splits=1), _w(1, 8, 32, 512, 1024, splits=1),
    _w(2, 37, 29, 1, 64, txa=False, splits=9),               # the stem: nine splits, the last one ragged
    _w(4, 64, 64, 16, 16, splits=64),                        # many splits
    _w(2, 11, 13, 16, 24, stride=2), _w(2, 11, 13, 16, 24, K=1, stride=2, pad=0),
    _w(2, 20, 45, 32, 64, txb=True), _w(1, 10, 40, 72, 24, txb=True, order="iohw"), _w(1, 16, 64, 64, 128, txa=False, order="iohw"),
    _w(2, 11, 37, 24, 40, xpad=4, dypad=4), _w(2, 16, 24, 64, 2, K=1, pad=0), _w(1, 9, 7, 64, 3, K=1, pad=0),
] + MODEL_WGRAD


def _wgrad_strides(order, Ci, Co, KK):
    """(s_co, s_ci, s_t) of a (Co, Ci, K, K) parameter, or of the transposed convolution's (Ci, Co, K, K) one"""
    return (Ci * KK, KK, 1) if order == "oihw" else (KK, Co * KK, 1)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "rounding"])
@pytest.mark.parametrize("case", WGRAD_CASES, ids=_fwd_id)
def test_conv_weight_gradient(case, exact):
    """out_scale = 0.5; the direct form, and the deferred form the tape uses (its record reports the library's split count, which
    must be the documented plan's, and its grouped reduction must give the same bits)."""
    lib, ops = _gpu()
    N, H, W, Ci, Co, K, stride, pad, use_a, use_b, order, xpad, dypad, want_splits = case
    g = _gen(*case[:10], exact)
    Ho, Wo = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    P = N * Ho * Wo
    x, dy = _vals((N, H, W, Ci), g, exact), _vals((N, Ho, Wo, Co), g, exact, -1, 1)
    ta, tb = _tx(Ci, g, exact) if use_a else None, _tx(Co, g, exact) if use_b else None
    s_co, s_ci, s_t = _wgrad_strides(order, Ci, Co, K * K)
    numel = Ci * Co * K * K
    ref, mag = R.conv_wgrad(x, ta, dy, tb, K, K, stride, pad, numel, s_co, s_ci, s_t, 0.5)
    if exact:
        assert mag.max().item() < EXACT
    splits, chunk = wgrad_plan(P, Ci, Co, K * K)
    if want_splits is not None:
        assert splits == want_splits
    if want_splits == 9:
        assert P % chunk != 0                                           # a ragged last chunk
    xbuf, xd = _sliced(x, xpad)
    dybuf, dyd = _sliced(dy, dypad)
    gw = torch.full((numel,), float("nan"), device=DEV)
    ops.conv_wgrad(xd, _dev(ta), dyd, _dev(tb), gw, s_co, s_ci, s_t, 0.5, K, K, stride, pad)
    _same(f"wgrad {_fwd_id(case[:10])}", gw, ref, 2 * R.gamma(P + 3) * mag, exact)
    gw2 = torch.full((numel,), float("nan"), device=DEV)
    pending = []
    ops.conv_wgrad(xd, _dev(ta), dyd, _dev(tb), gw2, s_co, s_ci, s_t, 0.5, K, K, stride, pad, defer=pending)
    assert len(pending) == 1 and (pending[0][0].splits, pending[0][0].RS, pending[0][0].Ci, pending[0][0].Co) == (splits, K * K, Ci, Co)
    ops.wgrad_reduce_flush(pending)
    assert torch.equal(gw2, gw)
    assert _outside_untouched(xbuf, xpad) and _outside_untouched(dybuf, dypad)


# =============================================================================================================================
# e. MaxPool2d(2) forward and backward
# =============================================================================================================================
POOL_SIZES = [(2, 16, 24), (1, 9, 7), (3, 33, 31), (1, 2, 2)]
POOL_CHANNELS = [1, 2, 3, 6, 64, 72]
MODEL_POOL = [((2, 11, 18), 256)]                    # ((N, H, W), C) of test_model_calls_are_covered
POOL_CASES = [(size, C) for size in POOL_SIZES for C in POOL_CHANNELS] + MODEL_POOL
POOL_VARIANTS = [(use_tx, xs, os_) for use_tx in (False, True) for xs in (False, True) for os_ in (False, True)]


def _run_pool(ops, size, C, use_tx, xslice, oslice, exact=True):
    """xslice: the pooled tensor is a channel slice; oslice: the forward's output / the backward's destination is one."""
    N, H, W = size
    g = _gen(N, H, W, C, use_tx, xslice, oslice, exact)
    x = _vals((N, H, W, C), g, exact)
    t = _itx(C, g) if use_tx else None
    dp, old = _vals((N, H // 2, W // 2, C), g, exact, -3, 3), _vals((N, H, W, C), g, exact, -3, 3)
    xpad, opad = 4 if xslice else 0, 4 if oslice else 0
    xbuf, xd = _sliced(x, xpad)
    ybuf, y = _sliced(torch.full((N, H // 2, W // 2, C), float("nan")), opad)
    ops.pool2_fwd(xd, _dev(t), y)
    assert torch.equal(y.cpu().to(F64), R.pool2_fwd(x, t)) and _outside_untouched(ybuf, opad)
    dpbuf, dpd = _sliced(dp, xpad if oslice else 0)
    for acc in (0, 1):
        dabuf, da = _sliced(old if acc else torch.full((N, H, W, C), float("nan")), opad)
        ops.pool2_bwd(dpd, xd, _dev(t), da, acc)
        ref = R.pool2_bwd(dp, x, t, old, acc)
        assert ref.abs().max().item() < EXACT
        # (accumulate on non-integer data: one fp32 addition, i.e. the float64 sum rounded once)
        assert torch.equal(da.cpu(), ref.float()) and _outside_untouched(dabuf, opad)
    assert _outside_untouched(xbuf, xpad) and _outside_untouched(dpbuf, xpad if oslice else 0)


@pytest.mark.parametrize("size,C", POOL_CASES, ids=lambda v: _fwd_id(v) if isinstance(v, tuple) else str(v))
def test_pool2_is_exact_on_integer_data(size, C):
    """pool2_fwd_kernel<float> / pool2_bwd_kernel<float>: a selection, so exact cases only.  Integer data is full of ties (torch's
    first-maximum rule must hold), negative scales reverse the ordering, an odd last row / column is dropped forward and gets a
    zero gradient backward; accumulate 0 and 1; dense and channel slices."""
    lib, ops = _gpu()
    for use_tx, xslice, oslice in POOL_VARIANTS:
        _run_pool(ops, size, C, use_tx, xslice, oslice)


def test_pool2_normal_data_is_bitwise():
    lib, ops = _gpu()
    _run_pool(ops, (3, 33, 31), 72, False, True, False, exact=False)
    _run_pool(ops, (3, 33, 31), 72, False, False, True, exact=False)


# =============================================================================================================================
# f. BatchNorm + ReLU backward: umi_bn_bwd_reduce / umi_bn_bwd_apply / umi_bn_bwd_apply_count
# =============================================================================================================================
MODEL_BN = [(2048, 64), (512, 128)]                  # (M, C) of test_model_calls_are_covered
BN_ROWS = [1, 255, 256, 257, 70000]
BN_SLICES = [(4, 4), (0, 0), (0, 4), (4, 0)]         # channels of padding on either side of (the gradient, y)
BN_CASES = ([(M, C) for M in BN_ROWS for C in (1, 2, 3, 24, 64, 72)] + [(M, 1024) for M in BN_ROWS[:4]]
            + MODEL_BN)


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "rounding"])
@pytest.mark.parametrize("M,C", BN_CASES)
def test_batchnorm_backward(M, C, exact):
    """Stage-1 blocks of 256 rows with a ragged last block, every branch of the channel-lane ladder (CT = 1 ... 64) and channel
    counts above 64, on channel slices (ld = C + 8) and dense.  Exact: integer y / gradient, integer mean and shift, scales 1 / -1 / 2,
    rstd = 1/2, and for the apply stage sums that are multiples of a power-of-two count, so every intermediate is exact."""
    lib, ops = _gpu()
    g = _gen(M, C, exact)
    y, da = _vals((1, 1, M, C), g, exact, -3, 3), _vals((1, 1, M, C), g, exact, -2, 2)
    if exact:
        t = _itx(C, g)
        t[:, 0] = _ints((C,), -1, 1, g)
        rstd = torch.full((C,), 0.5)
    else:
        t = _ntx(C, g)
        rstd = 0.5 + torch.rand(C, generator=g)
    s, q, sa, qa = R.bn_bwd_reduce(da, y, t, rstd)
    if exact:
        assert sa.max().item() < EXACT and 2 * qa.max().item() < EXACT        # (xhat comes in halves)
    td, rd = t.to(DEV), rstd.to(DEV)
    count = 4096                                       # the apply stage alone: over a count that is not this tensor's row count
    if exact:
        cs, cq = count * _ints((C,), -3, 3, g), count * _ints((C,), -2, 2, g)
    else:
        cs, cq = count * torch.randn(C, generator=g), count * torch.randn(C, generator=g)
    refc, magc = R.bn_bwd_apply(da, y, t, rstd, cs, cq, count)
    if exact:
        assert magc.max().item() < 2 ** 12             # half-integers of a few bits: every step of umi_bn_dz is exact
    for dapad, ypad in BN_SLICES:
        tag = f"{M}x{C} ld+{2 * dapad}/{2 * ypad}"
        ybuf, yd = _sliced(y, ypad)
        dabuf, dad = _sliced(da, dapad)
        gs, gq = ops.bn_bwd(dad, yd, td, rd)           # reduce + apply as Tape.conv_bn's backward runs them
        _same(f"bn sum_dz {tag}", gs, s, R.gamma(BN_BLOCK_ROWS + 1) * sa, exact)
        _same(f"bn sum_dzx {tag}", gq, q, R.gamma(BN_BLOCK_ROWS + 2) * qa, exact)
        if not exact:
            ref, mag = R.bn_bwd_apply(da, y, t, rstd, gs.cpu(), gq.cpu(), M)       # from the sums the kernel was given
            _within(f"bn apply {tag}", dad, ref, 8 * R.U * mag)
        assert _outside_untouched(dabuf, dapad) and _outside_untouched(ybuf, ypad)
        dabuf, dad = _sliced(da, dapad)
        ops.bn_bwd_apply(dad, yd, td, rd, cs.to(DEV), cq.to(DEV), count=count)
        _same(f"bn apply_count {tag}", dad, refc, 8 * R.U * magc, exact)
        assert _outside_untouched(dabuf, dapad)


def test_no_fp32_statistics_pass():
    """umi_bn_stats refuses fp32 storage: the fp32 statistics are the convolution epilogue's (test_conv_forward)."""
    lib, ops = _gpu()
    assert ops.bn_stats(torch.zeros(1, 16, 16, 64, device=DEV)) is None


# =============================================================================================================================
# g. colsum and materialize_nchw
# =============================================================================================================================
MODEL_COLSUM = [(32, 512, 512)]  # (test_model_calls_are_covered)
COLSUM_CASES = [(4 * 37 * 29, 2, 0), (2 * 16 * 16, 4, 0), (1001, 2, 0), (4 * 37 * 29, 2, 6), (5000, 64, 0), (777, 768, 0), (300, 3072, 0),
                (100, 72, 8), (1001, 1, 0), (4 * 37 * 29, 3, 0), (300, 1, 4), (31, 3, 2)] + MODEL_COLSUM


@pytest.mark.parametrize("exact", [True, False], ids=["exact", "rounding"])
@pytest.mark.parametrize("M,C,pad", COLSUM_CASES)
def test_colsum(M, C, pad, exact):
    """colsum1_kernel<float> (the fp32 bias gradients of the head and the transposed convolutions) over the table of
    test_colsum_paths plus C = 1 and 3; pad: the tensor is the lower channel slice of a wider buffer."""
    lib, ops = _gpu()
    g = _gen(M, C, pad, exact)
    buf = _vals((1, 1, M, C + pad), g, exact)
    x = buf[..., :C]
    ref, mag = R.colsum(x, 0.25)
    if exact:
        assert 4 * mag.max().item() < EXACT
    out = torch.full((C,), float("nan"), device=DEV)
    ops.colsum(buf.to(DEV)[..., :C], out, 0.25)
    _same(f"colsum {M}x{C}+{pad}", out, ref, R.gamma(colsum_plan(M, C)[1]) * mag, exact)


@pytest.mark.parametrize("use_tx", [False, True])
def test_materialize_nchw(use_tx):
    """materialize_nchw_kernel<float> on a channel slice: the transform is one fma, exact on integer data."""
    lib, ops = _gpu()
    g = _gen(3, use_tx)
    x = _ints((2, 9, 7, 6), -2, 2, g)
    t = _itx(6, g) if use_tx else None
    xbuf, xd = _sliced(x, 4)
    assert torch.equal(ops.materialize_nchw(xd, _dev(t)).cpu().to(F64), R.materialize_nchw(x, t))


# =============================================================================================================================
# h. the calls of the fp32 training step are the configurations pinned above
# =============================================================================================================================
def _allowed():
    ok = set()
    for (N, H, W, Ci, Co, K, stride, pad, tx, bias, stats, ipad, opad) in FWD_CASES:
        P = N * ((H + 2 * pad - K) // stride + 1) * ((W + 2 * pad - K) // stride + 1)
        ok.add(_conv_key("fwd", K, stride, pad, Ci, Co, P, ipad, opad, tx, bias, stats))
    for (N, H, W, Ci, Co) in DGRAD_CASES:
        ok.add(_conv_key("fwd", 3, 1, 1, Co, Ci, N * H * W, 0, 0, False, False, False))
    for shape in UPS_SHAPES:
        N, H, W, Ci, Co = shape
        for off, extra in UPS_PLACEMENTS:
            ok.add(_ups_key(shape, off, extra))
        for gslice in (False, True):
            ok.add(_conv_key("fwd", 2, 2, 0, Co, Ci, N * H * W, gslice, False, False, False, False))
            ok.add(_wgrad_key(2, 2, 0, Co, Ci, N * H * W, gslice, False, False, True, "oihw"))
            ok.add(_colsum_key(4 * N * H * W, Co, gslice))
    for (N, H, W, Ci, Co, K, stride, pad, txa, txb, order, xpad, dypad, _) in WGRAD_CASES:
        P = N * ((H + 2 * pad - K) // stride + 1) * ((W + 2 * pad - K) // stride + 1)
        ok.add(_wgrad_key(K, stride, pad, Ci, Co, P, xpad, dypad, txa, txb, order))
    for (N, H, W), C in POOL_CASES:
        for use_tx, xslice, oslice in POOL_VARIANTS:
            ok.add(_pool_key("fwd", H, W, C, xslice, oslice, use_tx))
            ok |= {_pool_key("bwd", H, W, C, xslice, oslice, use_tx, acc) for acc in (0, 1)}
    for M, C in BN_CASES:
        ok |= {_bn_key(op, M, C, dp, yp) for op in ("reduce+apply", "apply_count") for dp, yp in BN_SLICES}
    for M, C, pad in COLSUM_CASES:
        ok.add(_colsum_key(M, C, pad))
    return ok


def _ld(t):
    from umi.ops import _nhwc
    return _nhwc(t)[4]


def _sl(t):
    return _ld(t) > t.shape[3]


def test_model_calls_are_covered(monkeypatch):
    """One training step each of UNet(1, 2, 64), UNet(3, 4, 64) and UNet_multitask(1, 2, 64) under compute_dtype="fp32", batch 2, on a
    32 x 32 and on a 44 x 72 input: every call into the kernels of this file reduces to a configuration of the tables above
    (operation, R / stride / pad, the tile-residue classes of Ci, Co and P, slice or dense, transform, bias, statistics, offset)."""
    lib, ops = _gpu()
    import Model
    import loss as L
    from oracle import recipe
    seen = {}                                        # configuration -> the first call that had it, as a row for the tables

    def wrap(name, key):
        orig = getattr(ops, name)

        def f(*a, **k):
            kk = key(*a, **k)
            if kk is not None:
                seen.setdefault(*kk)
            return orig(*a, **k)
        monkeypatch.setattr(ops, name, f)

    def pad_of(t):
        return (_ld(t) - t.shape[3]) // 2

    def conv_key(x, tx, wp, bias, y, R_, S_, stride, pad, want_stats=False, flags=0, up_offset=(0, 0)):
        assert x.dtype == y.dtype == torch.float32 and R_ == S_ and not (flags & ~lib.CONV_UPSAMPLE2)
        N, H, W, Ci = x.shape
        Co = y.shape[3]
        if flags & lib.CONV_UPSAMPLE2:
            extra = (y.shape[1] - 2 * H, y.shape[2] - 2 * W)
            return (_conv_key("ups", 2, 2, 0, Ci, Co, N * H * W, _sl(x), _sl(y), tx is not None, bias is not None, want_stats,
                              (tuple(up_offset) != (0, 0), extra != (0, 0))),
                    f"UPS ({N}, {H}, {W}, {Ci}, {Co}) offset {tuple(up_offset)} extra {extra}")
        return (_conv_key("fwd", R_, stride, pad, Ci, Co, N * y.shape[1] * y.shape[2], _sl(x), _sl(y), tx is not None,
                          bias is not None, want_stats),
                f"_f({N}, {H}, {W}, {Ci}, {Co}, K={R_}, stride={stride}, pad={pad}, tx={tx is not None}, bias={bias is not None}, "
                f"stats={want_stats}, ipad={pad_of(x)}, opad={pad_of(y)})")

    def wgrad_key(x, txa, dy, txb, dW, s_co, s_ci, s_t, out_scale, R_, S_, stride, pad, flags=0, defer=None):
        assert x.dtype == dy.dtype == torch.float32 and R_ == S_ and flags == 0 and s_t == 1
        (N, H, W, Ci), Co = x.shape, dy.shape[3]
        order = {_wgrad_strides("oihw", Ci, Co, R_ * S_): "oihw", _wgrad_strides("iohw", Ci, Co, R_ * S_): "iohw"}[(s_co, s_ci, s_t)]
        return (_wgrad_key(R_, stride, pad, Ci, Co, dy.shape[0] * dy.shape[1] * dy.shape[2], _sl(x), _sl(dy), txa is not None,
                           txb is not None, order),
                f"_w({N}, {H}, {W}, {Ci}, {Co}, K={R_}, stride={stride}, pad={pad}, txa={txa is not None}, txb={txb is not None}, "
                f"order=\"{order}\", xpad={pad_of(x)}, dypad={pad_of(dy)})")

    def rows(t):
        return t.shape[0] * t.shape[1] * t.shape[2]

    def bn_key(da, y, tx, rstd, partials=None, apply=True):
        assert y.dtype == torch.float32 and partials is None and apply
        return _bn_key("reduce+apply", rows(y), y.shape[3], _sl(da), _sl(y)), f"BN ({rows(y)}, {y.shape[3]})"

    def bn_apply_key(da, y, tx, rstd, sum_dz, sum_dzx, count=None):
        if count is None:
            return None                                  # (the second half of bn_bwd, counted there)
        return _bn_key("apply_count", rows(y), y.shape[3], _sl(da), _sl(y)), f"BN ({rows(y)}, {y.shape[3]})"

    def pool_fwd_key(x, tx, y):
        return (_pool_key("fwd", x.shape[1], x.shape[2], x.shape[3], _sl(x), _sl(y), tx is not None),
                f"POOL ({tuple(x.shape[:3])}, {x.shape[3]})")

    def pool_bwd_key(dp, x, tx, da, acc):
        return (_pool_key("bwd", x.shape[1], x.shape[2], x.shape[3], _sl(x), _sl(da), tx is not None, int(bool(acc))),
                f"POOL ({tuple(x.shape[:3])}, {x.shape[3]})")

    wrap("conv_fwd", conv_key)
    wrap("conv_wgrad", wgrad_key)
    wrap("pool2_fwd", pool_fwd_key)
    wrap("pool2_bwd", pool_bwd_key)
    wrap("bn_bwd", bn_key)
    wrap("bn_bwd_apply", bn_apply_key)
    wrap("colsum", lambda x, out, s: (_colsum_key(rows(x), x.shape[3], _sl(x)), f"COLSUM ({rows(x)}, {x.shape[3]}, {_ld(x) - x.shape[3]})"))
    for name in ("bn_stats", "pool2_bwd_bnred", "conv_dgrad_bnred", "conv_gather_bnred", "head_dgrad_bnred", "conv_wgrad_bnapply",
                 "convT_wgrad_bias", "conv3x3_fwd_act"):            # the fp16 fusions: none may take an fp32 call
        orig = getattr(ops, name)

        def g(*a, _orig=orig, _name=name, **k):
            r = _orig(*a, **k)
            assert r is None or r is False, f"{_name} took a call of the fp32 step"
            return r
        monkeypatch.setattr(ops, name, g)

    for make, cin, ncls in ((Model.UNet, 1, 2), (Model.UNet, 3, 4), (Model.UNet_multitask, 1, 2)):
        for H, W in ((32, 32), (44, 72)):
            L.CLASS_NUMBER = ncls
            torch.manual_seed(0)
            m = make(cin, ncls, 64, False, compute_dtype="fp32").to(DEV).train()
            x, lab = recipe.synthetic_batch(2, cin, H, W, ncls, seed=3)
            out = m(x.to(DEV))
            outs = out if isinstance(out, tuple) else (out,)
            sum(L.calc_loss(o, lab.to(DEV), loss_type="dice_bce_mc") for o in outs).backward()
            torch.cuda.synchronize()
            assert all(torch.isfinite(p.grad).all() for p in m.parameters())
    assert len(seen) > 20
    ok = _allowed()
    missing = sorted(f"{v}    # {k}" for k, v in seen.items() if k not in ok)
    print(f"[valu_f32] the fp32 steps made {len(seen)} distinct configurations")
    assert not missing, "\n".join(missing)
