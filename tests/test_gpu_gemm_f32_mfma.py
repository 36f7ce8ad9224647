"""The opt-in fp32 matrix-core pointwise kernels (csrc/gemm_mfma_f32.hip, UMI_CONV_F32_MFMA_1X1, compute_dtype "fp32_mfma_gemm").

Exactness: small-integer operands built as tests/test_gpu_exact.py builds them, so every product and partial sum is exact in
fp32 whatever the order and the kernels must reproduce torch's fp32 linear / conv2d on the CPU BIT FOR BIT -- indexing, K
chunks, masking of ragged row tiles and partial channel tiles, the bias, split slabs, their reduction and the statistics
epilogue at zero tolerance.  Each test first asserts on the reference alone that exactness holds (everything below 2^24).
Rounding: on standard-normal data the error against float64 stays within the bound of ANY summation order of K' fused products,
gamma_2K' * (|a| * |b|), gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, 3.1 / 3.4;
the bound of tests/test_gpu_conv_f32_mfma.py); K' = Ci + 1 with a bias (one more addition), M for the weight gradient -- derived
from the arithmetic, not from what the kernels give.
Whole networks: the bodies and bars of the existing fp32 parity tests under "fp32_mfma_gemm"."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import recipe, ref_transunet, ref_unet
from tests.test_gpu_exact import _apply, _int_tx, _ints
from tests.test_gpu_transunet import product_config
from tests.test_gpu_unet import _is_dead_bias, rel_err
from tests.test_oracle_golden import sig

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXACT = 2 ** 24


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from umi import lib, ops
    return lib, ops


def _on_new_path(lib, ops, x, y, flags=None, has_bias=False):
    """The plan names the fp32 matrix-core pointwise kernel: layout 0 and one statistics row per 128 output rows."""
    N, H, W, _ = x.shape
    lay, rows = ops.conv_plan(x, y, 1, 1, 1, 0, lib.CONV_F32_MFMA_1X1 if flags is None else flags, has_bias)
    return lay == 0 and rows == -(-(N * H * W) // 128)


def _fwd(lib, ops, xd, td, wd, bd, y, flags, pack=None, stats=True):
    pack = pack or ops.pack_conv_fwd
    return ops.conv_fwd(xd, td, lambda l: pack(wd, torch.float32, k8=bool(l)), bd, y, 1, 1, 1, 0, want_stats=stats, flags=flags)


# N, H, W, Ci, Co, transform on load, bias
FWD_CASES = [
    (1, 14, 14, 768, 3072, False, True),     # fc1
    (1, 14, 14, 3072, 768, False, True),     # fc2
    (1, 14, 14, 768, 2304, False, True),     # fused qkv
    (1, 14, 14, 1024, 768, False, True),     # patch embedding
    (2, 16, 24, 64, 256, True, False),       # trunk 1x1 with a transform
    (1, 8, 8, 1024, 256, True, False),
    (2, 11, 37, 96, 136, True, False),       # ragged M tile, partial channel tiles
    (1, 9, 7, 8, 8, True, False),            # smallest channels
    (1, 1, 1, 16, 24, False, True),          # one row
    (3, 2, 3, 24, 40, False, False),
    (1, 33, 5, 32, 32, True, False),         # gate widths
    (2, 64, 64, 32, 64, True, False),        # 64 statistics rows
]
_fwd_cache = {}


def _fwd_case(case):
    """(x, w, transform, bias, reference), built once per case and shared (never modified)."""
    if case in _fwd_cache:
        return _fwd_cache[case]
    N, H, W, Ci, Co, use_tx, use_bias = case
    g = torch.Generator().manual_seed(sum(case[:5]))
    x = _ints((N, H, W, Ci), -2, 2, g)
    w = _ints((Co, Ci, 1, 1), -1, 1, g)
    t = _int_tx(Ci, g) if use_tx else None
    b = _ints((Co,), -3, 3, g) if use_bias else None
    a = _apply(x, t) if use_tx else x
    ref = F.linear(a, w.view(Co, Ci), b).contiguous()
    # exactness holds: the magnitude sums bound every partial sum of every order, the statistics sums are integers below 2^24
    mag = F.linear(a.abs(), w.view(Co, Ci).abs(), b.abs() if use_bias else None)
    assert mag.max().item() < EXACT and (ref * ref).sum((0, 1, 2)).max().item() < EXACT
    _fwd_cache[case] = (x, w, t, b, ref)
    return _fwd_cache[case]


def _check_stats(part, ref, Co):
    rows = part.view(-1, 2, Co)
    assert rows.shape[0] == -(-ref[..., 0].numel() // 128)
    s = rows.sum(0).cpu()
    assert torch.equal(s[0], ref.sum((0, 1, 2))) and torch.equal(s[1], (ref * ref).sum((0, 1, 2)))


def _dev(t):
    return None if t is None else t.to(DEV)


@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_and_statistics_are_exact_on_integer_data(case):
    lib, ops = _gpu()
    N, H, W, Ci, Co, use_tx, use_bias = case
    x, w, t, b, ref = _fwd_case(case)
    xd = x.to(DEV)
    y = torch.full((N, H, W, Co), float("nan"), device=DEV)
    assert _on_new_path(lib, ops, xd, y, has_bias=use_bias)
    part = _fwd(lib, ops, xd, _dev(t), w.to(DEV), _dev(b), y, lib.CONV_F32_MFMA_1X1)
    assert torch.equal(y.cpu(), ref)
    _check_stats(part, ref, Co)
    # each row of the partials covers 128 consecutive output rows
    r0 = ref.reshape(-1, Co)[:128]
    assert torch.equal(part.view(-1, 2, Co)[0, 0].cpu(), r0.sum(0))


def test_forward_on_channel_slices_of_wider_buffers():
    """ldx = Ci + 4, ldy = Co + 8: the operands are slices of concat buffers; nothing outside the output slice is written."""
    lib, ops = _gpu()
    case = (2, 11, 37, 96, 136, True, False)
    N, H, W, Ci, Co = case[:5]
    x, w, t, _, ref = _fwd_case(case)
    xbuf = torch.full((N, H, W, Ci + 4), 7.0, device=DEV)
    xbuf[..., 4:] = x.to(DEV)
    ybuf = torch.full((N, H, W, Co + 8), -5.0, device=DEV)
    xd, y = xbuf[..., 4:], ybuf[..., :Co]
    assert _on_new_path(lib, ops, xd, y)
    part = _fwd(lib, ops, xd, t.to(DEV), w.to(DEV), None, y, lib.CONV_F32_MFMA_1X1)
    assert torch.equal(y.cpu(), ref)
    assert (ybuf[..., Co:] == -5.0).all().item()
    _check_stats(part, ref, Co)


@pytest.mark.parametrize("case", FWD_CASES)
def test_data_gradient_is_exact_on_integer_data(case):
    """dgrad = the same kernel on the transposed weight panel (the forward cases without their bias), against autograd of conv2d."""
    lib, ops = _gpu()
    N, H, W, Ci, Co = case[:5]                                 # forward widths: the gradient maps Co -> Ci channels
    g = torch.Generator().manual_seed(sum(case[:5]) + 1)
    w = _ints((Co, Ci, 1, 1), -1, 1, g)
    dy = _ints((N, H, W, Co), -1, 1, g)
    xr = torch.zeros(N, Ci, H, W, requires_grad=True)
    F.conv2d(xr, w).backward(dy.permute(0, 3, 1, 2))
    ref = xr.grad.permute(0, 2, 3, 1).contiguous()
    assert F.linear(dy.abs(), w.view(Co, Ci).t().abs()).max().item() < EXACT
    dx = torch.full((N, H, W, Ci), float("nan"), device=DEV)
    dyd = dy.to(DEV)
    assert _on_new_path(lib, ops, dyd, dx)
    _fwd(lib, ops, dyd, None, w.to(DEV), None, dx, lib.CONV_F32_MFMA_1X1, pack=ops.pack_conv_dgrad, stats=False)
    assert torch.equal(dx.cpu(), ref)


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------
WGRAD_CASES = [(1, 14, 14, 768, 3072), (1, 14, 14, 3072, 768), (24, 14, 14, 64, 128), (2, 16, 24, 64, 256), (1, 8, 8, 1024, 256),
               (2, 11, 37, 96, 136), (1, 9, 7, 8, 8), (4, 64, 64, 8, 16), (1, 33, 5, 24, 40), (2, 32, 32, 768, 96)]
_wgrad_cache = {}


def _wgrad_case(case):
    if case in _wgrad_cache:
        return _wgrad_cache[case]
    N, H, W, Ci, Co = case
    g = torch.Generator().manual_seed(sum(case))
    x = _ints((N, H, W, Ci), -2, 2, g)
    dy = _ints((N, H, W, Co), -1, 1, g)
    t = _int_tx(Ci, g)
    a = _apply(x, t).reshape(-1, Ci)
    d = dy.reshape(-1, Co)
    ref = (d.t() @ a).view(Co, Ci, 1, 1)
    # exactness holds for any grouping of the rows: the sum of the products' magnitudes is below 2^24
    assert (d.abs().t() @ a.abs()).max().item() < EXACT
    _wgrad_cache[case] = (x, dy, t, ref * 0.5)                 # out_scale = 1 / loss scale: a power of two
    return _wgrad_cache[case]


def _split_slabs(m, ci, co):
    """The split rule as include/unetmi.h states it."""
    ti, tj = (64 if ci <= 64 else 128), (64 if co <= 64 else 128)
    tiles = -(-ci // ti) * -(-co // tj)
    chunks = -(-m // 32)
    want = max(1, min(-(-512 // tiles), -(-chunks // 4)))
    per = -(-chunks // want)
    return -(-chunks // per)


def _wgrad_on_new_path(lib, case):
    N, H, W, Ci, Co = case
    ws = lib.fn("umi_conv_wgrad_ws_bytes")
    return ws(N, H, W, Ci, Co, 1, 1, lib.UMI_F32, lib.CONV_F32_MFMA_1X1) >= _split_slabs(N * H * W, Ci, Co) * Ci * Co * 4


@pytest.mark.parametrize("case", WGRAD_CASES)
def test_weight_gradient_is_exact_on_integer_data(case):
    """Incl. the split slabs and their fixed-order reduction, with the transform on x and out_scale = 0.5."""
    lib, ops = _gpu()
    N, H, W, Ci, Co = case
    x, dy, t, ref = _wgrad_case(case)
    xd, dyd = x.to(DEV), dy.to(DEV)
    assert _on_new_path(lib, ops, xd, dyd) and _wgrad_on_new_path(lib, case)
    gw = torch.full((Co, Ci, 1, 1), float("nan"), device=DEV)
    ops.conv_wgrad(xd, t.to(DEV), dyd, None, gw, Ci, 1, 1, 0.5, 1, 1, 1, 0, flags=lib.CONV_F32_MFMA_1X1)
    assert torch.equal(gw.cpu(), ref)


def test_weight_gradient_of_a_channel_slice_of_a_wider_gradient_buffer():
    """lddy = 3 Co: the per-projection call of the fused q/k/v gradient."""
    lib, ops = _gpu()
    case = (2, 11, 37, 96, 136)
    N, H, W, Ci, Co = case
    x, dy, t, ref = _wgrad_case(case)
    buf = torch.full((N, H, W, 3 * Co), 9.0, device=DEV)
    buf[..., Co:2 * Co] = dy.to(DEV)
    dyd, xd = buf[..., Co:2 * Co], x.to(DEV)
    assert _on_new_path(lib, ops, xd, dyd) and _wgrad_on_new_path(lib, case)
    gw = torch.full((Co, Ci, 1, 1), float("nan"), device=DEV)
    ops.conv_wgrad(xd, t.to(DEV), dyd, None, gw, Ci, 1, 1, 0.5, 1, 1, 1, 0, flags=lib.CONV_F32_MFMA_1X1)
    assert torch.equal(gw.cpu(), ref)


def test_weight_gradient_through_the_deferred_sink_equals_the_immediate_call():
    lib, ops = _gpu()
    case = (2, 16, 24, 64, 256)
    N, H, W, Ci, Co = case
    x, dy, t, ref = _wgrad_case(case)
    xd, dyd, td = x.to(DEV), dy.to(DEV), t.to(DEV)
    assert _on_new_path(lib, ops, xd, dyd) and _wgrad_on_new_path(lib, case)
    now = torch.full((Co, Ci, 1, 1), float("nan"), device=DEV)
    later = torch.full((Co, Ci, 1, 1), float("nan"), device=DEV)
    ops.conv_wgrad(xd, td, dyd, None, now, Ci, 1, 1, 0.5, 1, 1, 1, 0, flags=lib.CONV_F32_MFMA_1X1)
    pending = []
    ops.conv_wgrad(xd, td, dyd, None, later, Ci, 1, 1, 0.5, 1, 1, 1, 0, flags=lib.CONV_F32_MFMA_1X1, defer=pending)
    assert len(pending) == 1                                   # recorded, not launched
    ops.wgrad_reduce_flush(pending)
    assert torch.equal(now.cpu(), ref) and torch.equal(later.cpu(), now.cpu())


# ---- rounding on real data -------------------------------------------------------------------------------------------------------
U = 2.0 ** -24


def _gamma(K):
    return 2 * K * U / (1 - 2 * K * U)


def _ratio(got, ref64, mag64, K):
    """Largest |got - ref| / (gamma_2K * sum |a b|) over the tensor (the bound holds elementwise: every ratio <= 1)."""
    return ((got.double() - ref64).abs() / (_gamma(K) * mag64)).max().item()


@pytest.mark.parametrize("case", [(1, 14, 14, 768, 3072), (1, 14, 14, 3072, 768)])
def test_forward_and_data_gradient_rounding_on_normal_data(case):
    lib, ops = _gpu()
    N, H, W, Ci, Co = case
    g = torch.Generator().manual_seed(sum(case))
    x, w, b = torch.randn(N, H, W, Ci, generator=g), torch.randn(Co, Ci, 1, 1, generator=g), torch.randn(Co, generator=g)
    dy = torch.randn(N, H, W, Co, generator=g)
    x64, w64, b64, dy64 = x.double(), w.double().view(Co, Ci), b.double(), dy.double()
    ref, mag = F.linear(x64, w64, b64), F.linear(x64.abs(), w64.abs(), b64.abs())
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
    y = torch.empty(N, H, W, Co, device=DEV)
    assert _on_new_path(lib, ops, xd, y, has_bias=True)
    _fwd(lib, ops, xd, None, wd, b.to(DEV), y, lib.CONV_F32_MFMA_1X1, stats=False)
    r_fwd = _ratio(y.cpu(), ref, mag, Ci + 1)
    print(f"forward {case}: largest error / bound = {r_fwd:.4f}")
    assert r_fwd <= 1.0
    # data gradient: Co -> Ci channels, K = Co
    refd, magd = F.linear(dy64, w64.t()), F.linear(dy64.abs(), w64.t().abs())
    dx = torch.empty(N, H, W, Ci, device=DEV)
    assert _on_new_path(lib, ops, dyd, dx)
    _fwd(lib, ops, dyd, None, wd, None, dx, lib.CONV_F32_MFMA_1X1, pack=ops.pack_conv_dgrad, stats=False)
    r_dg = _ratio(dx.cpu(), refd, magd, Co)
    print(f"data gradient {case}: largest error / bound = {r_dg:.4f}")
    assert r_dg <= 1.0


@pytest.mark.parametrize("case", [(2, 32, 32, 64, 128), (24, 14, 14, 64, 96)])
def test_weight_gradient_rounding_on_normal_data(case):
    lib, ops = _gpu()
    N, H, W, Ci, Co = case
    g = torch.Generator().manual_seed(sum(case))
    x, dy = torch.randn(N, H, W, Ci, generator=g), torch.randn(N, H, W, Co, generator=g)
    a64, d64 = x.double().reshape(-1, Ci), dy.double().reshape(-1, Co)
    ref, mag = (d64.t() @ a64).view(Co, Ci, 1, 1), (d64.abs().t() @ a64.abs()).view(Co, Ci, 1, 1)
    xd, dyd = x.to(DEV), dy.to(DEV)
    assert _on_new_path(lib, ops, xd, dyd) and _wgrad_on_new_path(lib, case)
    gw = torch.empty(Co, Ci, 1, 1, device=DEV)
    ops.conv_wgrad(xd, None, dyd, None, gw, Ci, 1, 1, 1.0, 1, 1, 1, 0, flags=lib.CONV_F32_MFMA_1X1)
    r = _ratio(gw.cpu(), ref, mag, N * H * W)
    print(f"weight gradient {case}: largest error / bound = {r:.4f}")
    assert r <= 1.0


# ---- determinism, ignore rule ----------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bits():
    lib, ops = _gpu()
    N, H, W, Ci, Co = 2, 19, 45, 96, 136
    g = torch.Generator().manual_seed(11)
    x, w, dy = torch.randn(N, H, W, Ci, generator=g), torch.randn(Co, Ci, 1, 1, generator=g), torch.randn(N, H, W, Co, generator=g)
    b = torch.randn(Co, generator=g)
    xd, wd, dyd, bd = x.to(DEV), w.to(DEV), dy.to(DEV), b.to(DEV)
    outs = []
    for _ in range(2):
        y, gw = torch.empty(N, H, W, Co, device=DEV), torch.empty(Co, Ci, 1, 1, device=DEV)
        assert _on_new_path(lib, ops, xd, y, has_bias=True)
        part = _fwd(lib, ops, xd, None, wd, bd, y, lib.CONV_F32_MFMA_1X1)
        ops.conv_wgrad(xd, None, dyd, None, gw, Ci, 1, 1, 1.0, 1, 1, 1, 0, flags=lib.CONV_F32_MFMA_1X1)
        outs.append((y.cpu(), part.cpu(), gw.cpu()))
    for a, b_ in zip(*outs):
        assert torch.equal(a, b_)


@pytest.mark.parametrize("Ci,flags", [(3, 0), (64, 2)])
def test_flag_is_ignored_on_the_device(Ci, flags):
    """Ci = 3 with the flag, and an eligible shape under FORCE_GENERIC | F32_MFMA_1X1: bit-identical to the same call without the
    flag, forward, statistics and weight gradient."""
    lib, ops = _gpu()
    N, H, W, Co = 2, 13, 37, 64
    g = torch.Generator().manual_seed(Ci)
    x, w, dy = torch.randn(N, H, W, Ci, generator=g), torch.randn(Co, Ci, 1, 1, generator=g), torch.randn(N, H, W, Co, generator=g)
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
    outs = []
    for f in (flags, flags | lib.CONV_F32_MFMA_1X1):
        y, gw = torch.empty(N, H, W, Co, device=DEV), torch.empty(Co, Ci, 1, 1, device=DEV)
        assert ops.conv_plan(xd, y, 1, 1, 1, 0, f) == ops.conv_plan(xd, y, 1, 1, 1, 0, flags)
        part = _fwd(lib, ops, xd, None, wd, None, y, f)
        ops.conv_wgrad(xd, None, dyd, None, gw, Ci, 1, 1, 1.0, 1, 1, 1, 0, flags=f)
        outs.append((y.cpu(), part.cpu(), gw.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_both_flags_on_a_3x3_call_equal_the_3x3_flag_alone():
    lib, ops = _gpu()
    N, H, W, Ci, Co = 2, 13, 37, 24, 40
    g = torch.Generator().manual_seed(5)
    x, w, dy = torch.randn(N, H, W, Ci, generator=g), torch.randn(Co, Ci, 3, 3, generator=g), torch.randn(N, H, W, Co, generator=g)
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
    outs = []
    for f in (lib.CONV_F32_MFMA, lib.CONV_F32_MFMA | lib.CONV_F32_MFMA_1X1):
        y, gw = torch.empty(N, H, W, Co, device=DEV), torch.empty(Co, Ci, 3, 3, device=DEV)
        assert ops.conv_plan(xd, y, 3, 3, 1, 1, f) == ops.conv_plan(xd, y, 3, 3, 1, 1, lib.CONV_F32_MFMA)
        part = ops.conv_fwd(xd, None, lambda l: ops.pack_conv_fwd(wd, torch.float32, k8=bool(l)), None, y, 3, 3, 1, 1,
                            want_stats=True, flags=f)
        ops.conv_wgrad(xd, None, dyd, None, gw, Ci * 9, 9, 1, 1.0, 3, 3, 1, 1, flags=f)
        outs.append((y.cpu(), part.cpu(), gw.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---- whole networks ----------------------------------------------------------------------------------------------------------------
class _Spy:
    """Records (kind, R, S, stride, pad, input channels, output channels, flags) of every ops.conv_fwd / ops.conv_wgrad call."""

    def __init__(self, monkeypatch):
        from umi import ops
        self.calls = []
        fwd, wgrad = ops.conv_fwd, ops.conv_wgrad

        def conv_fwd(x, tx, wp, bias, y, R, S, stride, pad, want_stats=False, flags=0, up_offset=(0, 0)):
            self.calls.append(("fwd", R, S, stride, pad, x.shape[3], y.shape[3], flags))
            return fwd(x, tx, wp, bias, y, R, S, stride, pad, want_stats=want_stats, flags=flags, up_offset=up_offset)

        def conv_wgrad(x, txa, dy, txb, dW, s_co, s_ci, s_t, out_scale, R, S, stride, pad, flags=0, defer=None):
            self.calls.append(("wgrad", R, S, stride, pad, x.shape[3], dy.shape[3], flags))
            return wgrad(x, txa, dy, txb, dW, s_co, s_ci, s_t, out_scale, R, S, stride, pad, flags=flags, defer=defer)

        monkeypatch.setattr(ops, "conv_fwd", conv_fwd)
        monkeypatch.setattr(ops, "conv_wgrad", conv_wgrad)

    def check(self, lib):
        f3, f1 = lib.CONV_F32_MFMA, lib.CONV_F32_MFMA_1X1
        kinds = {f3: set(), f1: set()}
        for c in self.calls:
            kind, geo, cin, cout, flags = c[0], c[1:5], c[5], c[6], c[7]
            want = 0
            if geo == (1, 1, 1, 0) and cin % 8 == 0 and cout % 8 == 0:
                want = f1
            elif geo == (3, 3, 1, 1) and cin % 8 == 0:
                want = f3
            assert flags & (f3 | f1) == want, c
            if want:
                kinds[want].add(kind)
        assert kinds[f3] == {"fwd", "wgrad"} and kinds[f1] == {"fwd", "wgrad"}, kinds


@pytest.mark.parametrize("name,ncls", [("transunet_small", 2), ("transunet_small_rgb4", 4)])
def test_transunet_small_fp32_mfma_gemm_parity(golden_dir, name, ncls, monkeypatch):
    """tests/test_gpu_transunet.py::test_transunet_small_fp32_parity under compute_dtype="fp32_mfma_gemm", same bars."""
    lib, _ = _gpu()
    import loss as L
    from TransUnet.vit_seg_modeling import VisionTransformer
    spy = _Spy(monkeypatch)
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    cfg = ref_transunet.small_config(ncls)
    img, B, cin, seed = int(g["img"]), int(g["B"]), int(g["cin"]), int(g["seed"])
    ref = ref_transunet.RefTransUNet(cfg, img)
    ref.load_state_dict(recipe.fill_state_dict(ref.state_dict(), seed=seed, negative_gamma=False))
    x, lab = recipe.synthetic_batch(B, cin, img, img, ncls, seed=seed)
    L.CLASS_NUMBER = ncls
    m = VisionTransformer(product_config(cfg, img), img_size=img, num_classes=ncls, compute_dtype="fp32_mfma_gemm")
    m.load_state_dict(ref.state_dict())
    m.to(DEV).train()
    logits = m(x.to(DEV))
    loss = L.calc_loss(logits, lab.to(DEV), loss_type="dice_bce_mc")
    loss.backward()
    spy.check(lib)
    gl = g["logits"]
    np.testing.assert_allclose(logits.detach().cpu().numpy(), gl, rtol=1e-4, atol=1e-4 * float(np.abs(gl).max()))
    assert abs(loss.item() - float(g["loss0"])) < 2e-5
    ref.train()
    rl = ref_unet.dice_bce_mc(ref(x), lab, ncls)
    rl.backward()
    worst = ("", 0.0)
    for (k, p), (_, rp) in zip(m.named_parameters(), ref.named_parameters()):
        assert p.grad is not None, k
        # key biases have a mathematically zero gradient (softmax is shift invariant): absolute floor 1e-6
        e = (p.grad.detach().double().cpu() - rp.grad.double()).norm().item() / (rp.grad.double().norm().item() + 1e-6 / 3e-3)
        worst = max(worst, (k, e), key=lambda t: t[1])
    assert worst[1] < 3e-3, worst
    # BatchNorm running stats after one step, eval-mode forward
    for k, v in m.state_dict().items():
        if "running" in k:
            assert rel_err(v, ref.state_dict()[k]) < 1e-4, k
    m.eval()
    ref.eval()
    with torch.no_grad():
        ev, rev = m(x.to(DEV)), ref(x)
    assert ((ev.cpu() - rev).abs().max() / rev.abs().max()).item() < 2e-4


def test_transunet_r50_vit_b16_224_fp32_mfma_gemm(golden_dir, monkeypatch):
    """tests/test_gpu_transunet.py::test_transunet_r50_vit_b16_224[fp32] under "fp32_mfma_gemm" (the real 768 / 3072 widths), same
    bars."""
    lib, _ = _gpu()
    import loss as L
    from TransUnet.vit_seg_modeling import VisionTransformer
    spy = _Spy(monkeypatch)
    g = np.load(os.path.join(golden_dir, "transunet_r50_b16_224.npz"))
    cfg = ref_transunet.r50_vit_b16_config(2, 3, dropout_rate=0.0)
    L.CLASS_NUMBER = 2
    m = VisionTransformer(product_config(cfg, 224), img_size=224, num_classes=2, compute_dtype="fp32_mfma_gemm")
    assert len(m.state_dict()) == 409
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=int(g["seed"]), negative_gamma=False))
    m.to(DEV).train()
    x, lab = recipe.synthetic_batch(1, 1, 224, 224, 2, seed=int(g["seed"]))
    logits = m(x.to(DEV))
    loss = L.calc_loss(logits, lab.to(DEV), loss_type="dice_bce_mc")
    loss.backward()
    spy.check(lib)
    s = sig(logits.cpu())
    np.testing.assert_allclose(s[[0, 2]], g["logits_sig"][[0, 2]], rtol=2e-4)
    np.testing.assert_allclose(s[3:], g["logits_sig"][3:], rtol=1e-3, atol=1e-3 * s[0] / 300)
    assert abs(loss.item() - float(g["loss0"])) < 2e-5
    bad = []
    for k, p in m.named_parameters():
        ref_norm = float(g["grad_sig." + k][0])
        assert torch.isfinite(p.grad).all(), k
        if ref_norm < 1e-7:                                    # e.g. key biases: mathematically zero gradient
            continue
        if abs(p.grad.double().norm().item() - ref_norm) > 1e-2 * ref_norm:
            bad.append((k, p.grad.double().norm().item(), ref_norm))
    assert not bad, bad[:5]


def test_unet_attention_fp32_mfma_gemm_step0(golden_dir, monkeypatch):
    """Step 0 of tests/test_gpu_unet.py::test_unet_attention_parity[fp32] under "fp32_mfma_gemm", with the bars of
    tests/test_gpu_conv_f32_mfma.py::test_unet_attention_fp32_mfma_step0."""
    lib, _ = _gpu()
    import Model
    import loss as L
    spy = _Spy(monkeypatch)
    g = np.load(os.path.join(golden_dir, "unet_attention_1_2_8.npz"))
    cin, ncls, feat = int(g["cin"]), int(g["ncls"]), int(g["feat"])
    B, H, W, seed = int(g["B"]), int(g["H"]), int(g["W"]), int(g["seed"])
    ref = ref_unet.RefUNetAttention(cin, ncls, feat, False)
    ref.load_state_dict(recipe.fill_state_dict(ref.state_dict(), seed=seed))
    x, lab = recipe.synthetic_batch(B, cin, H, W, ncls, seed=seed)
    L.CLASS_NUMBER = ncls
    m = Model.UNet_attention(cin, ncls, feat, False, compute_dtype="fp32_mfma_gemm")
    m.load_state_dict(ref.state_dict())
    m.to(DEV).train()
    ref.double().train()
    logits = m(x.to(DEV))
    loss = L.calc_loss(logits, lab.to(DEV), loss_type="dice_bce_mc")
    loss.backward()
    spy.check(lib)
    ref_unet.dice_bce_mc(ref(x.double()), lab, ncls).backward()
    np.testing.assert_allclose(logits.detach().cpu().numpy(), g["logits"], rtol=1e-4, atol=1e-4 * float(np.abs(g["logits"]).max()))
    assert abs(loss.item() - float(g["loss0"])) < 1e-4
    for (k, p), (_, rp) in zip(m.named_parameters(), ref.named_parameters()):
        if _is_dead_bias(k):
            assert float(p.grad.abs().max()) < 1e-6, k
            assert float(rp.grad.abs().max()) < 1e-6, k
        else:
            assert rel_err(p.grad, rp.grad) < 2e-3, k
