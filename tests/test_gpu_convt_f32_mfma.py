"""The opt-in fp32 matrix-core ConvTranspose2d(2, 2) kernels (csrc/convt_mfma_f32.hip, UMI_CONV_F32_MFMA_2X2, compute_dtype
"fp32_mfma_convt"): the forward (UMI_CONV_UPSAMPLE2), the data gradient (a 2x2 / stride-2 convolution) and the weight gradient.

Exactness: small-integer operands built as tests/test_gpu_exact.py builds them, so every product and partial sum is exact in
fp32 whatever the order and the kernels must reproduce torch's fp32 conv_transpose2d / conv2d and their autograd on the CPU BIT FOR
BIT -- the scatter with its offsets, K chunks that straddle a tap's end, masking of ragged row tiles and partial channel tiles,
the bias, split slabs and their reduction at zero tolerance.  Each test first asserts on the reference alone that exactness holds
(everything below 2^24).
Rounding: on standard-normal data the error against float64 stays within the bound of ANY summation order of K' fused products,
gamma_2K' * (|a| * |b|), gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, 3.1 / 3.4;
the bound of tests/test_gpu_conv_f32_mfma.py); K' = Cin + 1 forward (the bias is one more addition), 4 Ci data gradient, N Ho Wo
weight gradient -- derived from the arithmetic, not from what the kernels give.
Whole networks: the bodies and bars of the existing fp32 parity tests under "fp32_mfma_convt"; one step on poisoned memory."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

if __name__ == "__main__":                                   # the HIP-graph case runs this file as a child process
    _REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_REPO, os.path.join(_REPO, "unet-torch_amd")]

from oracle import recipe, ref_unet
from tests.test_gpu_exact import _apply, _int_tx, _ints
from tests.test_gpu_gemm_f32_mfma import _Spy, _gamma
from tests.test_gpu_unet import _is_dead_bias, _oracle_run, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXACT = 2 ** 24
TWO = (2, 2, 2, 0)


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from umi import lib, ops
    return lib, ops


def _dev(t):
    return None if t is None else t.to(DEV)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _on_new_path(lib, ops, x, y, up, has_bias=False):
    """The plan names the fp32 matrix-core 2x2 kernels: layout 0 and no statistics rows, where the flag-less plan reports some."""
    extra = lib.CONV_UPSAMPLE2 if up else 0
    return (ops.conv_plan(x, y, *TWO, lib.CONV_F32_MFMA_2X2 | extra, has_bias) == (0, 0)
            and ops.conv_plan(x, y, *TWO, extra, has_bias)[1] >= 1)


def _up(lib, ops, xd, td, wd, bd, dest, flags, off=(0, 0)):
    ops.conv_fwd(xd, td, lambda l: ops.pack_convT_fwd(wd, torch.float32, k8=bool(l)), bd, dest, *TWO,
                 flags=lib.CONV_UPSAMPLE2 | flags, up_offset=off)


def _dgrad(lib, ops, gd, wd, dx, flags):
    ops.conv_fwd(gd, None, lambda l: ops.pack_convT_dgrad(wd, torch.float32, k8=bool(l)), None, dx, *TWO, flags=flags)


def _wgrad(ops, gd, txa, ad, txb, gw, scale, flags, defer=None):
    Co, Ci = gw.shape[:2]                                      # ConvTranspose2d's [in][out][2][2]: in = the channels of `ad`
    ops.conv_wgrad(gd, txa, ad, txb, gw, Ci * 4, 4, 1, scale, *TWO, flags=flags, defer=defer)


# ---- forward ---------------------------------------------------------------------------------------------------------------------
# N, h, w, Cin, Cout, transform on load, bias, (dY, dX) extra output rows / columns, extra channels in front of the slice
FWD_CASES = [
    (1, 32, 32, 1024, 512, True, True, (0, 0), 512),      # the deepest level at full width, into the upper half of a concat buffer
    (2, 16, 24, 128, 64, True, True, (0, 0), 64),
    (2, 5, 7, 24, 40, True, True, (3, 2), 8),             # ragged rows, taps that straddle 32-column tiles, offset (1, 1)
    (3, 2, 3, 16, 8, True, False, (1, 0), 4),
    (1, 9, 33, 96, 136, False, True, (0, 0), 0),
    (1, 1, 1, 8, 8, False, True, (0, 0), 0),
    (2, 64, 64, 64, 32, True, True, (0, 0), 32),
]
_fwd_cache = {}


def _fwd_case(case):
    """(x, weight, transform, bias, reference), built once per case and shared (never modified)."""
    if case in _fwd_cache:
        return _fwd_cache[case]
    N, h, w, Cin, Cout, use_tx, use_bias = case[:7]
    g = torch.Generator().manual_seed(sum(case[:5]))
    x = _ints((N, h, w, Cin), -2, 2, g)
    wt = _ints((Cin, Cout, 2, 2), -1, 1, g)
    t = _int_tx(Cin, g) if use_tx else None
    b = _ints((Cout,), -3, 3, g) if use_bias else None
    a = _nchw(_apply(x, t) if use_tx else x)
    ref = _nhwc(F.conv_transpose2d(a, wt, b, stride=2))
    # exactness holds: the magnitude sums bound every partial sum of every order
    assert F.conv_transpose2d(a.abs(), wt.abs(), b.abs() if use_bias else None, stride=2).max().item() < EXACT
    _fwd_cache[case] = (x, wt, t, b, ref)
    return _fwd_cache[case]


@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_is_exact_on_integer_data_and_writes_only_its_window(case):
    lib, ops = _gpu()
    N, h, w, Cin, Cout, use_tx, use_bias, (dY, dX), front = case
    x, wt, t, b, ref = _fwd_case(case)
    oy, ox = dY // 2, dX // 2                                  # centred like F.pad in the reference's Up.forward
    buf = torch.full((N, 2 * h + dY, 2 * w + dX, front + Cout), float("nan"), device=DEV)
    dest, xd = buf[..., front:], x.to(DEV)
    assert _on_new_path(lib, ops, xd, dest, True, has_bias=use_bias)
    _up(lib, ops, xd, _dev(t), wt.to(DEV), _dev(b), dest, lib.CONV_F32_MFMA_2X2, off=(oy, ox))
    got = buf.cpu()
    assert torch.equal(got[:, oy:oy + 2 * h, ox:ox + 2 * w, front:], ref)
    # everything else still holds NaN: the other channels of the buffer, the rows and columns outside the window
    written = torch.zeros(got.shape, dtype=torch.bool)
    written[:, oy:oy + 2 * h, ox:ox + 2 * w, front:] = True
    assert torch.isnan(got[~written]).all().item() and not torch.isnan(got[written]).any().item()


# ---- data gradient ---------------------------------------------------------------------------------------------------------------
# N, Ho, Wo, Ci, Co in the call's own naming: Ci = the ConvT's Cout (channels of g), Co = the ConvT's Cin
DGRAD_CASES = [(1, 32, 32, 512, 1024), (2, 16, 24, 64, 128), (2, 5, 7, 40, 24), (1, 9, 33, 136, 96), (1, 1, 1, 8, 8)]
_dgrad_cache = {}


def _dgrad_case(case):
    if case in _dgrad_cache:
        return _dgrad_cache[case]
    N, Ho, Wo, Ci, Co = case
    g = torch.Generator().manual_seed(sum(case) + 1)
    wt = _ints((Co, Ci, 2, 2), -1, 1, g)                       # ConvTranspose2d weight [Cin][Cout][2][2]
    gup = _ints((N, 2 * Ho, 2 * Wo, Ci), -1, 1, g)
    xr = torch.zeros(N, Co, Ho, Wo, requires_grad=True)
    F.conv_transpose2d(xr, wt, None, stride=2).backward(_nchw(gup))
    ref = _nhwc(xr.grad)
    assert F.conv2d(_nchw(gup).abs(), wt.abs(), None, 2).max().item() < EXACT
    _dgrad_cache[case] = (wt, gup, ref)
    return _dgrad_cache[case]


@pytest.mark.parametrize("case", DGRAD_CASES)
def test_data_gradient_is_exact_on_integer_data(case):
    lib, ops = _gpu()
    N, Ho, Wo, Ci, Co = case
    wt, gup, ref = _dgrad_case(case)
    gd = gup.to(DEV)
    dx = torch.full((N, Ho, Wo, Co), float("nan"), device=DEV)
    assert _on_new_path(lib, ops, gd, dx, False)
    _dgrad(lib, ops, gd, wt.to(DEV), dx, lib.CONV_F32_MFMA_2X2)
    assert torch.equal(dx.cpu(), ref)


def test_data_gradient_on_channel_slices_of_wider_buffers():
    """ldx = Ci + 8, ldy = Co + 4: g is a slice of a buffer whose other columns are NaN; nothing outside the output slice is written."""
    lib, ops = _gpu()
    case = (2, 5, 7, 40, 24)
    N, Ho, Wo, Ci, Co = case
    wt, gup, ref = _dgrad_case(case)
    gbuf = torch.full((N, 2 * Ho, 2 * Wo, Ci + 8), float("nan"), device=DEV)
    gbuf[..., 4:4 + Ci] = gup.to(DEV)
    ybuf = torch.full((N, Ho, Wo, Co + 4), float("nan"), device=DEV)
    gd, dx = gbuf[..., 4:4 + Ci], ybuf[..., :Co]
    assert _on_new_path(lib, ops, gd, dx, False)
    _dgrad(lib, ops, gd, wt.to(DEV), dx, lib.CONV_F32_MFMA_2X2)
    assert torch.equal(dx.cpu(), ref) and torch.isnan(ybuf[..., Co:]).all().item()


# ---- weight gradient -------------------------------------------------------------------------------------------------------------
WGRAD_CASES = DGRAD_CASES + [(4, 64, 64, 64, 128)]             # the last: many splits
_wgrad_cache = {}


def _wgrad_case(case, use_txb, use_txa=False):
    """(g, the ConvT's input, its transform, transform of g, reference * 0.5): out_scale = 1 / loss scale, a power of two."""
    key = (case, use_txb, use_txa)
    if key in _wgrad_cache:
        return _wgrad_cache[key]
    N, Ho, Wo, Ci, Co = case
    g = torch.Generator().manual_seed(sum(case) + 2)
    gup = _ints((N, 2 * Ho, 2 * Wo, Ci), -1, 1, g)
    a = _ints((N, Ho, Wo, Co), -2, 2, g)
    tb = _int_tx(Co, g) if use_txb else None
    ta = _int_tx(Ci, g) if use_txa else None
    act = _apply(a, tb) if use_txb else a
    gact = _apply(gup, ta) if use_txa else gup
    wr = torch.zeros(Co, Ci, 2, 2, requires_grad=True)
    F.conv_transpose2d(_nchw(act), wr, None, stride=2).backward(_nchw(gact))
    # exactness holds for any grouping of the pixels: the sum of the products' magnitudes is below 2^24
    assert act.abs().max().item() * gact.abs().max().item() * N * Ho * Wo < EXACT
    _wgrad_cache[key] = (gup, a, tb, ta, wr.grad * 0.5)
    return _wgrad_cache[key]


def _split_slabs(m, ci, co):
    """The split rule as include/unetmi.h states it: the four taps count as tiles."""
    ti, tj = (64 if ci <= 64 else 128), (64 if co <= 64 else 128)
    tiles = 4 * -(-ci // ti) * -(-co // tj)
    chunks = -(-m // 32)
    want = max(1, min(-(-512 // tiles), -(-chunks // 4)))
    per = -(-chunks // want)
    return -(-chunks // per)


def _wgrad_on_new_path(lib, case):
    N, Ho, Wo, Ci, Co = case
    ws = lib.fn("umi_conv_wgrad_ws_bytes")
    return ws(N, Ho, Wo, Ci, Co, 2, 2, lib.UMI_F32, lib.CONV_F32_MFMA_2X2) >= _split_slabs(N * Ho * Wo, Ci, Co) * 4 * Ci * Co * 4


@pytest.mark.parametrize("use_txb", [True, False])
@pytest.mark.parametrize("case", WGRAD_CASES)
def test_weight_gradient_is_exact_immediate_and_deferred(case, use_txb):
    """Incl. the split slabs and their fixed-order reduction, out_scale = 0.5; the deferred sink gives the immediate call's bits."""
    lib, ops = _gpu()
    N, Ho, Wo, Ci, Co = case
    gup, a, tb, _, ref = _wgrad_case(case, use_txb)
    gd, ad, td = gup.to(DEV), a.to(DEV), _dev(tb)
    assert _on_new_path(lib, ops, gd, ad, False) and _wgrad_on_new_path(lib, case)
    if case == WGRAD_CASES[-1]:
        assert _split_slabs(N * Ho * Wo, Ci, Co) >= 32
    now = torch.full((Co, Ci, 2, 2), float("nan"), device=DEV)
    later = torch.full((Co, Ci, 2, 2), float("nan"), device=DEV)
    _wgrad(ops, gd, None, ad, td, now, 0.5, lib.CONV_F32_MFMA_2X2)
    pending = []
    _wgrad(ops, gd, None, ad, td, later, 0.5, lib.CONV_F32_MFMA_2X2, defer=pending)
    assert len(pending) == 1                                   # recorded, not launched
    ops.wgrad_reduce_flush(pending)
    assert torch.equal(now.cpu(), ref) and torch.equal(later.cpu(), now.cpu())


def test_weight_gradient_with_a_transform_on_both_sides():
    lib, ops = _gpu()
    case = (2, 5, 7, 40, 24)
    N, Ho, Wo, Ci, Co = case
    gup, a, tb, ta, ref = _wgrad_case(case, True, True)
    gw = torch.full((Co, Ci, 2, 2), float("nan"), device=DEV)
    _wgrad(ops, gup.to(DEV), ta.to(DEV), a.to(DEV), tb.to(DEV), gw, 0.5, lib.CONV_F32_MFMA_2X2)
    assert torch.equal(gw.cpu(), ref)


# ---- rounding on real data -------------------------------------------------------------------------------------------------------
def _ratio(got, ref64, mag64, K):
    """Largest |got - ref| / (gamma_2K * sum |a b|) over the tensor (the bound holds elementwise: every ratio <= 1)."""
    return ((got.double() - ref64).abs() / (_gamma(K) * mag64)).max().item()


@pytest.mark.parametrize("case", [(1, 16, 16, 256, 128), (2, 8, 8, 64, 32)])
def test_rounding_on_normal_data(case):
    lib, ops = _gpu()
    N, h, w, Cin, Cout = case
    f = lib.CONV_F32_MFMA_2X2
    g = torch.Generator().manual_seed(sum(case))
    x, wt, b = torch.randn(N, h, w, Cin, generator=g), torch.randn(Cin, Cout, 2, 2, generator=g), torch.randn(Cout, generator=g)
    gup = torch.randn(N, 2 * h, 2 * w, Cout, generator=g)
    x64, w64, b64, g64 = _nchw(x.double()), wt.double(), b.double(), _nchw(gup.double())
    xd, wd, gd = x.to(DEV), wt.to(DEV), gup.to(DEV)
    # forward: K' = Cin + 1
    ref, mag = F.conv_transpose2d(x64, w64, b64, stride=2), F.conv_transpose2d(x64.abs(), w64.abs(), b64.abs(), stride=2)
    y = torch.empty(N, 2 * h, 2 * w, Cout, device=DEV)
    assert _on_new_path(lib, ops, xd, y, True, has_bias=True)
    _up(lib, ops, xd, None, wd, b.to(DEV), y, f)
    r = _ratio(_nchw(y.cpu()), ref, mag, Cin + 1)
    print(f"forward {case}: largest error / bound = {r:.4f}")
    assert r <= 1.0
    # data gradient: K' = 4 Ci, Ci = the ConvT's Cout
    ref, mag = F.conv2d(g64, w64, None, 2), F.conv2d(g64.abs(), w64.abs(), None, 2)
    dx = torch.empty(N, h, w, Cin, device=DEV)
    assert _on_new_path(lib, ops, gd, dx, False)
    _dgrad(lib, ops, gd, wd, dx, f)
    r = _ratio(_nchw(dx.cpu()), ref, mag, 4 * Cout)
    print(f"data gradient {case}: largest error / bound = {r:.4f}")
    assert r <= 1.0
    # weight gradient: K' = N Ho Wo
    taps = gup.double().view(N, h, 2, w, 2, Cout)
    ref = torch.einsum("nhwi,nhrwso->iors", x.double(), taps)
    mag = torch.einsum("nhwi,nhrwso->iors", x.double().abs(), taps.abs())
    gw = torch.empty(Cin, Cout, 2, 2, device=DEV)
    assert _wgrad_on_new_path(lib, (N, h, w, Cout, Cin))
    _wgrad(ops, gd, None, xd, None, gw, 1.0, f)
    r = _ratio(gw.cpu(), ref, mag, N * h * w)
    print(f"weight gradient {case}: largest error / bound = {r:.4f}")
    assert r <= 1.0


# ---- determinism, batch independence, ignore rule --------------------------------------------------------------------------------
def _trio(lib, ops, x, wt, b, gup, flags):
    """(forward of x, data gradient of gup, weight gradient of the pair) of one ConvTranspose2d, computed on the device under `flags`.
    gup may have one row more than twice x's: the 2x2 / stride-2 calls then drop it."""
    N, h, w, Cin = x.shape
    Cout = wt.shape[1]
    xd, wd, gd = x.to(DEV), wt.to(DEV), gup.to(DEV)
    y = torch.empty(N, 2 * h, 2 * w, Cout, device=DEV)
    _up(lib, ops, xd, None, wd, _dev(b), y, flags)
    dx = torch.empty(N, h, w, Cin, device=DEV)
    _dgrad(lib, ops, gd, wd, dx, flags)
    gw = torch.empty(Cin, Cout, 2, 2, device=DEV)
    _wgrad(ops, gd, None, xd, None, gw, 1.0, flags)
    return y.cpu(), dx.cpu(), gw.cpu()


def _normal(N, h, w, Cin, Cout, seed, gh=None, gw=None):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, h, w, Cin, generator=g), torch.randn(Cin, Cout, 2, 2, generator=g), torch.randn(Cout, generator=g),
            torch.randn(N, gh or 2 * h, gw or 2 * w, Cout, generator=g))


def test_two_calls_give_identical_bits():
    lib, ops = _gpu()
    x, wt, b, gup = _normal(2, 9, 21, 96, 136, 11)
    assert _on_new_path(lib, ops, x.to(DEV), torch.empty(2, 18, 42, 136, device=DEV), True, has_bias=True)
    first, second = (_trio(lib, ops, x, wt, b, gup, lib.CONV_F32_MFMA_2X2) for _ in range(2))
    for a, c in zip(first, second):
        assert torch.isfinite(a).all().item() and torch.equal(a, c)


def test_image_0_of_a_batch_equals_the_same_image_alone():
    """48 + 48 rows: both images share the row tile of a workgroup."""
    lib, ops = _gpu()
    x, wt, b, gup = _normal(2, 6, 8, 24, 40, 12)
    both = _trio(lib, ops, x, wt, b, gup, lib.CONV_F32_MFMA_2X2)
    alone = _trio(lib, ops, x[:1], wt, b, gup[:1], lib.CONV_F32_MFMA_2X2)
    assert torch.equal(both[0][:1], alone[0]) and torch.equal(both[1][:1], alone[1])


def test_flag_is_ignored_on_pointers_that_are_not_16_byte_aligned():
    """Channel slices that start 8 bytes into a pixel (ld % 4 == 0, so the plan names the new kernels): every call equals the
    flag-less one bit for bit."""
    lib, ops = _gpu()
    x, wt, b, gup = _normal(2, 4, 7, 16, 8, 15)
    xbuf, gbuf = torch.zeros(2, 4, 7, 20, device=DEV), torch.zeros(2, 8, 14, 12, device=DEV)
    xbuf[..., 2:18], gbuf[..., 2:10] = x.to(DEV), gup.to(DEV)
    xd, gd, wd, bd = xbuf[..., 2:18], gbuf[..., 2:10], wt.to(DEV), b.to(DEV)
    assert xd.data_ptr() % 16 == 8 and gd.data_ptr() % 16 == 8
    outs = []
    for f in (0, lib.CONV_F32_MFMA_2X2):
        ybuf, dbuf = torch.zeros(2, 8, 14, 12, device=DEV), torch.zeros(2, 4, 7, 20, device=DEV)
        y, dx, gw = ybuf[..., 2:10], dbuf[..., 2:18], torch.empty(16, 8, 2, 2, device=DEV)
        if f:
            assert _on_new_path(lib, ops, xd, y, True, True) and _on_new_path(lib, ops, gd, dx, False)
        _up(lib, ops, xd, None, wd, bd, y, f)
        _dgrad(lib, ops, gd, wd, dx, f)
        _wgrad(ops, gd, None, xd, None, gw, 1.0, f)
        outs.append((ybuf.cpu(), dbuf.cpu(), gw.cpu()))
    for a, c in zip(*outs):
        assert torch.isfinite(a).all().item() and a.abs().sum().item() > 0 and torch.equal(a, c)


@pytest.mark.parametrize("what", ["cin4", "force_generic", "odd_h"])
def test_flag_is_ignored_on_the_device(what):
    """Cin = 4 with the flag, an eligible shape under FORCE_GENERIC | F32_MFMA_2X2, and a 2x2 / stride-2 convolution over 9 rows (the
    data gradient's and the weight gradient's calls): bit-identical to the same calls without the flag."""
    lib, ops = _gpu()
    base = lib.CONV_FORCE_GENERIC if what == "force_generic" else 0
    gh = 9 if what == "odd_h" else None
    x, wt, b, gup = _normal(2, 4, 7, 4 if what == "cin4" else 16, 8, 13, gh=gh)
    f = lib.CONV_F32_MFMA_2X2
    gd, dx = gup.to(DEV), torch.empty(2, 4, 7, x.shape[3], device=DEV)
    xd, y = x.to(DEV), torch.empty(2, 8, 14, 8, device=DEV)
    assert ops.conv_plan(gd, dx, *TWO, base | f) == ops.conv_plan(gd, dx, *TWO, base)
    if what == "odd_h":
        # premise: the same call over 8 rows is taken, and so is the forward (it has no odd image)
        assert _on_new_path(lib, ops, torch.empty(2, 8, 14, 8, device=DEV), dx, False) and _on_new_path(lib, ops, xd, y, True, True)
    else:
        up = lib.CONV_UPSAMPLE2
        assert ops.conv_plan(xd, y, *TWO, base | up | f, True) == ops.conv_plan(xd, y, *TWO, base | up, True)
    plain = _trio(lib, ops, x, wt, b, gup, base)
    flagged = _trio(lib, ops, x, wt, b, gup, base | lib.CONV_F32_MFMA_2X2)
    for i, (a, c) in enumerate(zip(plain, flagged)):
        if what == "odd_h" and i == 0:
            continue                                           # (the forward has no odd image: it is on the new kernel)
        assert torch.isfinite(a).all().item() and torch.equal(a, c), i


def test_a_forward_call_with_statistics_is_unsupported_and_writes_nothing():
    lib, ops = _gpu()
    x, wt, b, _ = _normal(1, 4, 4, 16, 8, 14)
    xd, bd = x.to(DEV), b.to(DEV)
    wp = ops.pack_convT_fwd(wt.to(DEV), torch.float32)
    y = torch.full((1, 8, 8, 8), float("nan"), device=DEV)
    part = torch.full((64,), float("nan"), device=DEV)
    assert _on_new_path(lib, ops, xd, y, True, has_bias=True)
    flags = lib.CONV_UPSAMPLE2 | lib.CONV_F32_MFMA_2X2
    st = lib.fn("umi_conv_fwd")(xd.data_ptr(), 16, None, wp.data_ptr(), bd.data_ptr(), y.data_ptr(), 8, part.data_ptr(),
                                1, 4, 4, 16, 8, 2, 2, 2, 0, 4, 4, 0, 0, 8, 8, lib.UMI_F32, lib.UMI_F32, flags, ops._stream())
    assert st == lib.UMI_ERR_UNSUPPORTED
    assert torch.isnan(y).all().item() and torch.isnan(part).all().item()
    st = lib.fn("umi_conv_fwd")(xd.data_ptr(), 16, None, wp.data_ptr(), bd.data_ptr(), y.data_ptr(), 8, None,
                                1, 4, 4, 16, 8, 2, 2, 2, 0, 4, 4, 0, 0, 8, 8, lib.UMI_F32, lib.UMI_F32, flags, ops._stream())
    assert st == 0 and torch.isfinite(y).all().item()


# ---- whole networks --------------------------------------------------------------------------------------------------------------
def _check_spy(spy, lib, mode):
    """Under "fp32_mfma_convt" every 2x2 call between multiples of 8 channels carries the flag and no other call does; the two older
    flags sit where they sat.  Under any other mode no call carries it."""
    f3, f1, f2 = lib.CONV_F32_MFMA, lib.CONV_F32_MFMA_1X1, lib.CONV_F32_MFMA_2X2
    kinds = set()
    for c in spy.calls:
        kind, geo, cin, cout, flags = c[0], c[1:5], c[5], c[6], c[7]
        want = 0
        if geo == (1, 1, 1, 0) and cin % 8 == 0 and cout % 8 == 0:
            want = f1
        elif geo == (3, 3, 1, 1) and cin % 8 == 0:
            want = f3
        elif geo == TWO and cin % 8 == 0 and cout % 8 == 0 and mode == "fp32_mfma_convt":
            want = f2
            kinds.add((kind, bool(flags & lib.CONV_UPSAMPLE2)))
        assert flags & (f3 | f1 | f2) == want, c
    if mode == "fp32_mfma_convt":
        assert kinds == {("fwd", True), ("fwd", False), ("wgrad", False)}, kinds
    else:
        assert any(c[1:5] == TWO for c in spy.calls)


@pytest.mark.parametrize("name", ["unet_1_2_8", "unet_3_4_8"])
def test_unet_fp32_mfma_convt_parity(golden_dir, name, monkeypatch):
    """tests/test_gpu_unet.py::test_unet_fp32_parity under compute_dtype="fp32_mfma_convt", same bars: logits rtol 1e-4 vs the
    REFERENCE's logits, argmax identical off near-ties, loss / grads / 3 SGD steps / eval-mode logits vs the oracle."""
    lib, _ = _gpu()
    import Model
    import loss as L
    spy = _Spy(monkeypatch)
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    ref, x, lab = _oracle_run(g, 3)
    ncls = int(g["ncls"])
    L.CLASS_NUMBER = ncls
    m = Model.UNet(int(g["cin"]), ncls, int(g["feat"]), False, compute_dtype="fp32_mfma_convt")
    m.load_state_dict(ref.state_dict())
    m.to(DEV).train()
    ref.train()
    xd, labd = x.to(DEV), lab.to(DEV)
    opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    ropt = torch.optim.SGD(ref.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    for step in range(3):
        logits = m(xd)
        loss = L.calc_loss(logits, labd, loss_type="dice_bce_mc")
        opt.zero_grad()
        loss.backward()
        rlogits = ref(x)
        rloss = ref_unet.dice_bce_mc(rlogits, lab, ncls)
        ropt.zero_grad()
        rloss.backward()
        if step == 0:
            _check_spy(spy, lib, "fp32_mfma_convt")
            gl = torch.from_numpy(g["logits"])
            np.testing.assert_allclose(logits.detach().cpu().numpy(), g["logits"], rtol=1e-4, atol=1e-4 * gl.abs().max().item())
            top2 = torch.topk(gl, 2, dim=1).values
            safe = (top2[:, 0] - top2[:, 1]) > 1e-4 * gl.abs().max()
            am = logits.argmax(1).cpu()
            assert (am == torch.from_numpy(g["argmax"]).long())[safe].all()
            assert abs(loss.item() - float(g["loss0"])) < 1e-5
        assert abs(loss.item() - float(g[f"loss{step}"])) < 5e-5, step
        for (k, p), (_, rp) in zip(m.named_parameters(), ref.named_parameters()):
            assert rel_err(p.grad, rp.grad) < (2e-3 if step == 0 else 8e-2), (step, k)
        opt.step()
        ropt.step()
    for k, v in m.state_dict().items():
        rv = ref.state_dict()[k]
        if "num_batches" in k:
            assert int(v) == int(rv) == 3
        else:
            assert rel_err(v.float(), rv.float()) < 1e-3, k
    m.eval()
    with torch.no_grad():
        ev = m(xd)
    np.testing.assert_allclose(ev.cpu().numpy(), g["eval_logits"], rtol=2e-3,
                               atol=2e-3 * float(np.abs(g["eval_logits"]).max()))


def test_no_call_carries_the_flag_under_fp32_mfma_attn(golden_dir, monkeypatch):
    lib, _ = _gpu()
    import Model
    import loss as L
    spy = _Spy(monkeypatch)
    g = np.load(os.path.join(golden_dir, "unet_1_2_8.npz"))
    ref, x, lab = _oracle_run(g, 1)
    L.CLASS_NUMBER = int(g["ncls"])
    m = Model.UNet(int(g["cin"]), int(g["ncls"]), int(g["feat"]), False, compute_dtype="fp32_mfma_attn")
    m.load_state_dict(ref.state_dict())
    m.to(DEV).train()
    L.calc_loss(m(x.to(DEV)), lab.to(DEV), loss_type="dice_bce_mc").backward()
    _check_spy(spy, lib, "fp32_mfma_attn")


VARIANTS = [("unet_multitask_1_2_8", "UNet_multitask", "RefUNetMultitask", True),
            ("unet_multitask_1_2_8_s10", "UNet_multitask", "RefUNetMultitask", False),
            ("unet_attention_1_2_8", "UNet_attention", "RefUNetAttention", True),
            ("unet_attention_1_2_8_s16", "UNet_attention", "RefUNetAttention", False)]


@pytest.mark.parametrize("name,pcls,rcls,screened", VARIANTS)
def test_variant_fp32_mfma_convt_step0(golden_dir, name, pcls, rcls, screened, monkeypatch):
    """Step 0 of tests/test_gpu_unet.py::test_unet_multitask_parity[fp32] / test_unet_attention_parity[fp32] (fixtures on screened
    seeds: 2e-3 for every gradient tensor, the bars of tests/test_gpu_conv_f32_mfma.py) and of test_variant_unpicked_seeds (3e-2 for
    every tensor, 2e-3 for the median) under "fp32_mfma_convt"."""
    lib, _ = _gpu()
    import Model
    import loss as L
    spy = _Spy(monkeypatch)
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    cin, ncls, feat = int(g["cin"]), int(g["ncls"]), int(g["feat"])
    B, H, W, seed = int(g["B"]), int(g["H"]), int(g["W"]), int(g["seed"])
    ref = getattr(ref_unet, rcls)(cin, ncls, feat, False)
    ref.load_state_dict(recipe.fill_state_dict(ref.state_dict(), seed=seed))
    x, lab1 = recipe.synthetic_batch(B, cin, H, W, ncls, seed=seed)
    _, lab2 = recipe.synthetic_batch(B, cin, H, W, ncls, seed=seed + 100)
    L.CLASS_NUMBER = ncls
    m = getattr(Model, pcls)(cin, ncls, feat, False, compute_dtype="fp32_mfma_convt")
    m.load_state_dict(ref.state_dict())
    m.to(DEV).train()
    attention = pcls == "UNet_attention"
    if attention and screened:
        ref.double()                                           # as test_unet_attention_parity[fp32] runs its oracle
        rx = x.double()
    else:
        rx = x
    ref.train()
    out, rout = m(x.to(DEV)), ref(rx)
    if isinstance(out, tuple):
        loss = L.calc_loss(out[0], lab1.to(DEV), loss_type="dice_bce_mc") + L.calc_loss(out[1], lab2.to(DEV), loss_type="dice_bce_mc")
        rloss = ref_unet.dice_bce_mc(rout[0], lab1, ncls) + ref_unet.dice_bce_mc(rout[1], lab2, ncls)
        pairs = [(out[0], g["logits1"]), (out[1], g["logits2"])]
    else:
        loss = L.calc_loss(out, lab1.to(DEV), loss_type="dice_bce_mc")
        rloss = ref_unet.dice_bce_mc(rout, lab1, ncls)
        pairs = [(out, g["logits"])]
    loss.backward()
    rloss.backward()
    _check_spy(spy, lib, "fp32_mfma_convt")
    for o, gl in pairs:
        np.testing.assert_allclose(o.detach().cpu().numpy(), gl, rtol=1e-4, atol=1e-4 * float(np.abs(gl).max()))
    assert abs(loss.item() - float(g["loss0"])) < 1e-4
    named = list(zip(m.named_parameters(), ref.named_parameters()))
    if screened:
        for (k, p), (_, rp) in named:
            if attention and _is_dead_bias(k):
                assert float(p.grad.abs().max()) < 1e-6 and float(rp.grad.abs().max()) < 1e-6, k
            else:
                assert rel_err(p.grad, rp.grad) < 2e-3, k
    else:
        errs = {k: rel_err(p.grad, rp.grad) for (k, p), (_, rp) in named if rp.grad.abs().max() > 1e-6}
        print(name, "grad rel-L2: median", float(np.median(list(errs.values()))), "worst", max(errs.items(), key=lambda kv: kv[1]))
        assert max(errs.values()) < 3e-2, max(errs.items(), key=lambda kv: kv[1])
        assert float(np.median(list(errs.values()))) < 2e-3


# ---- poisoned memory -------------------------------------------------------------------------------------------------------------
POISON_CASE = dict(model=("UNet", 1, 2, 8), dtype="fp32_mfma_convt", shape=(1, 1, 44, 72))      # 5x9 / 2x4 levels: padded skips


def test_step_is_invariant_to_prior_memory_contents(monkeypatch):
    """tests/test_gpu_poisoned_step.py's method on one UNet(1, 2, 8) step under the new mode: zero-filled against 0xFF-filled
    memory, bit for bit and finite."""
    lib, _ = _gpu()
    from tests import test_gpu_poisoned_step as P
    spy = _Spy(monkeypatch)
    master = P._master(POISON_CASE)
    x, labs = P._batch(POISON_CASE)
    a0 = P._run(POISON_CASE, master, x, labs, 0x00, steps=1)
    _check_spy(spy, lib, "fp32_mfma_convt")                    # premise: the step ran the three new kernels
    a1 = P._run(POISON_CASE, master, x, labs, 0x00, steps=1)
    b = P._run(POISON_CASE, master, x, labs, 0xFF, steps=1)
    assert len(a0) > 4
    P._check_invariance(a0, a1, b)


def _graph_child():
    """Child-process body of the test below (stream capture is sensitive to what ran before it in the process).  The eager run does
    two steps: the GraphedStep's warm-up step and its one replay."""
    from tests import test_gpu_poisoned_step as P
    master = P._master(POISON_CASE)
    x, labs = P._batch(POISON_CASE)
    a0 = P._run(POISON_CASE, master, x, labs, 0x00, steps=2)
    b = P._graphed_run(POISON_CASE, master, x, labs, 0xFF, replays=1)
    assert "step1.loss" in b and any(k.startswith("step1.grad.") for k in b)
    a0 = {k: a0[k] for k in b}                               # (the warm-up step's own tensors are not visible from outside)
    d = P._first_difference(a0, b)
    assert d is None, "the graph replay on 0xFF-filled memory differs from the eager run on zero-filled memory at " + d
    P._assert_finite(b)
    print("POISONED_GRAPH_OK", len(b), float(b["step1.loss"]))


def test_graphed_step_is_invariant_to_prior_memory_contents():
    """The same step captured by umi.graphs.GraphedStep and replayed on 0xFF-filled memory, against the eager run on zero-filled
    memory: logits, loss, gradients, parameters, momentum and BatchNorm buffers, bit for bit and finite."""
    _gpu()
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "POISONED_GRAPH_OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])


if __name__ == "__main__":
    _graph_child()
