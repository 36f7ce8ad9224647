"""The opt-in fp32 matrix-core 3x3 kernels (csrc/conv_mfma_f32.hip, UMI_CONV_F32_MFMA, compute_dtype "fp32_mfma").

Exactness: small-integer operands built as tests/test_gpu_exact.py builds them, so every product and partial sum is exact in
fp32 whatever the order and the kernels must reproduce torch's fp32 conv2d on the CPU BIT FOR BIT -- indexing, halo, tap and
chunk order, masking of partial tiles, split-K slabs, their reduction and the statistics epilogue at zero tolerance.  Each test
first asserts on the reference alone that exactness holds (everything below 2^24).
Rounding: on standard-normal data the error against float64 stays within the bound of ANY summation order of K fused products,
gamma_2K * (|a| * |b|), gamma_n = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, 3.1 / 3.4: a
sum of K products accumulated by fma in any order carries at most K roundings per term; the factor 2 leaves room for merged partial
sums, i.e. the split-K reduction) -- derived from the arithmetic, not from what the kernels give.
Whole network: test_unet_fp32_parity's body and bars under "fp32_mfma"."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import recipe, ref_unet
from tests.test_gpu_exact import _apply, _int_tx, _ints
from tests.test_gpu_unet import _is_dead_bias, _oracle_run, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
EXACT = 2 ** 24


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from umi import lib, ops
    return lib, ops


def _on_new_path(lib, ops, x, y, flags=None):
    """The plan names the fp32 matrix-core kernel: layout 0 and one statistics row per 8 x 32 pixel tile."""
    N, H, W, _ = x.shape
    lay, rows = ops.conv_plan(x, y, 3, 3, 1, 1, lib.CONV_F32_MFMA if flags is None else flags)
    return lay == 0 and rows == N * -(-H // 8) * -(-W // 32)


def _fwd(lib, ops, xd, td, wd, y, flags, pack=None, stats=True):
    pack = pack or ops.pack_conv_fwd
    return ops.conv_fwd(xd, td, lambda l: pack(wd, torch.float32, k8=bool(l)), None, y, 3, 3, 1, 1, want_stats=stats, flags=flags)


# N, H, W, Ci, Co, transform on load
FWD_CASES = [
    (1, 16, 64, 64, 64, True),
    (1, 16, 64, 128, 64, True),
    (2, 16, 32, 64, 128, True),
    (1, 8, 32, 512, 512, True),
    (1, 8, 32, 1024, 512, True),
    (2, 11, 37, 96, 128, True),       # ragged pixel tiles
    (1, 20, 45, 48, 72, True),        # partial channel tiles
    (1, 9, 7, 8, 8, True),            # smallest channels
    (1, 5, 33, 24, 40, False),
    (1, 1, 1, 8, 16, True),           # a single pixel: all halo
    (3, 2, 3, 16, 8, False),
]


def _fwd_case(case):
    N, H, W, Ci, Co, use_tx = case
    g = torch.Generator().manual_seed(sum(case[:5]))
    x = _ints((N, H, W, Ci), -2, 2, g)
    w = _ints((Co, Ci, 3, 3), -1, 1, g)
    t = _int_tx(Ci, g) if use_tx else None
    a = _apply(x, t) if use_tx else x
    ref = F.conv2d(a.permute(0, 3, 1, 2), w, None, 1, 1).permute(0, 2, 3, 1).contiguous()
    # exactness holds: every output and every statistics sum is an integer below 2^24
    assert ref.abs().max().item() < EXACT and (ref * ref).sum((0, 1, 2)).max().item() < EXACT
    return x, w, t, ref


def _check_stats(part, ref, Co):
    s = part.view(-1, 2, Co).sum(0).cpu()
    assert torch.equal(s[0], ref.sum((0, 1, 2))) and torch.equal(s[1], (ref * ref).sum((0, 1, 2)))


@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_and_statistics_are_exact_on_integer_data(case):
    lib, ops = _gpu()
    N, H, W, Ci, Co, use_tx = case
    x, w, t, ref = _fwd_case(case)
    xd, wd = x.to(DEV), w.to(DEV)
    y = torch.full((N, H, W, Co), float("nan"), device=DEV)
    assert _on_new_path(lib, ops, xd, y)
    part = _fwd(lib, ops, xd, t.to(DEV) if use_tx else None, wd, y, lib.CONV_F32_MFMA)
    assert torch.equal(y.cpu(), ref)
    _check_stats(part, ref, Co)


def test_forward_on_channel_slices_of_wider_buffers():
    """ldx = Ci + 4, ldy = Co + 8: the operands are slices of concat buffers; nothing outside the output slice is written."""
    lib, ops = _gpu()
    case = (2, 11, 37, 24, 40, True)
    N, H, W, Ci, Co, _ = case
    x, w, t, ref = _fwd_case(case)
    xbuf = torch.full((N, H, W, Ci + 4), 7.0, device=DEV)
    xbuf[..., 4:] = x.to(DEV)
    ybuf = torch.full((N, H, W, Co + 8), -5.0, device=DEV)
    xd, y = xbuf[..., 4:], ybuf[..., :Co]
    assert _on_new_path(lib, ops, xd, y)
    part = _fwd(lib, ops, xd, t.to(DEV), w.to(DEV), y, lib.CONV_F32_MFMA)
    assert torch.equal(y.cpu(), ref)
    assert (ybuf[..., Co:] == -5.0).all().item()
    _check_stats(part, ref, Co)


@pytest.mark.parametrize("case", [(1, 16, 64, 64, 64), (2, 16, 32, 128, 64), (1, 8, 32, 512, 1024), (2, 11, 37, 128, 96),
                                  (1, 9, 7, 8, 8), (1, 5, 33, 40, 24)])
def test_data_gradient_is_exact_on_integer_data(case):
    """dgrad = the same kernel on the flipped / transposed weight panel, against autograd of conv2d."""
    lib, ops = _gpu()
    N, H, W, Ci, Co = case                                     # forward widths: the gradient maps Co -> Ci channels
    g = torch.Generator().manual_seed(sum(case))
    w = _ints((Co, Ci, 3, 3), -1, 1, g)
    dy = _ints((N, H, W, Co), -1, 1, g)
    xr = torch.zeros(N, Ci, H, W, requires_grad=True)
    F.conv2d(xr, w, None, 1, 1).backward(dy.permute(0, 3, 1, 2))
    ref = xr.grad.permute(0, 2, 3, 1).contiguous()
    assert ref.abs().max().item() < EXACT
    dx = torch.full((N, H, W, Ci), float("nan"), device=DEV)
    dyd = dy.to(DEV)
    assert _on_new_path(lib, ops, dyd, dx)
    _fwd(lib, ops, dyd, None, w.to(DEV), dx, lib.CONV_F32_MFMA, pack=ops.pack_conv_dgrad, stats=False)
    assert torch.equal(dx.cpu(), ref)


def _wgrad_case(case):
    N, H, W, Ci, Co = case
    g = torch.Generator().manual_seed(sum(case))
    x = _ints((N, H, W, Ci), -2, 2, g)
    dy = _ints((N, H, W, Co), -1, 1, g)
    t = _int_tx(Ci, g)
    a = _apply(x, t).permute(0, 3, 1, 2)
    wr = torch.zeros(Co, Ci, 3, 3, requires_grad=True)
    F.conv2d(a, wr, None, 1, 1).backward(dy.permute(0, 3, 1, 2))
    # exactness holds for any grouping of the pixels: the sum of the products' magnitudes is below 2^24
    wa = torch.zeros(Co, Ci, 3, 3, requires_grad=True)
    F.conv2d(a.abs(), wa, None, 1, 1).backward(dy.abs().permute(0, 3, 1, 2))
    assert wa.grad.max().item() < EXACT
    return x, dy, t, wr.grad * 0.5                             # out_scale = 1 / loss scale: a power of two


def _wgrad_on_new_path(lib, case):
    N, H, W, Ci, Co = case
    ws = lib.fn("umi_conv_wgrad_ws_bytes")
    # whole slabs of the new kernel's own split: N * H * ceil(W / 32) items, at least 4 per split, 1,024 workgroups aimed at
    items, tiles = N * H * -(-W // 32), -(-Ci // 64) * -(-Co // 64) * 3
    want = max(1, min(-(-1024 // tiles), -(-items // 4)))
    ips = -(-items // want)
    return ws(N, H, W, Ci, Co, 3, 3, lib.UMI_F32, lib.CONV_F32_MFMA) >= -(-items // ips) * 9 * Ci * Co * 4


WGRAD_CASES = [(2, 32, 64, 64, 64), (1, 32, 32, 128, 64), (2, 16, 32, 256, 256), (1, 16, 16, 1024, 512), (2, 20, 45, 32, 64),
               (1, 9, 7, 8, 8), (4, 64, 64, 8, 16), (1, 5, 33, 24, 40)]


@pytest.mark.parametrize("case", WGRAD_CASES)
def test_weight_gradient_is_exact_on_integer_data(case):
    """Incl. the split-K slabs and their fixed-order reduction, with the transform on x and out_scale = 0.5."""
    lib, ops = _gpu()
    N, H, W, Ci, Co = case
    x, dy, t, ref = _wgrad_case(case)
    xd, dyd = x.to(DEV), dy.to(DEV)
    assert _on_new_path(lib, ops, xd, dyd) and _wgrad_on_new_path(lib, case)
    gw = torch.full((Co, Ci, 3, 3), float("nan"), device=DEV)
    ops.conv_wgrad(xd, t.to(DEV), dyd, None, gw, Ci * 9, 9, 1, 0.5, 3, 3, 1, 1, flags=lib.CONV_F32_MFMA)
    assert torch.equal(gw.cpu(), ref)


def test_weight_gradient_through_the_deferred_sink_equals_the_immediate_call():
    lib, ops = _gpu()
    case = (2, 20, 45, 32, 64)
    N, H, W, Ci, Co = case
    x, dy, t, ref = _wgrad_case(case)
    xd, dyd, td = x.to(DEV), dy.to(DEV), t.to(DEV)
    assert _on_new_path(lib, ops, xd, dyd) and _wgrad_on_new_path(lib, case)
    now = torch.full((Co, Ci, 3, 3), float("nan"), device=DEV)
    later = torch.full((Co, Ci, 3, 3), float("nan"), device=DEV)
    ops.conv_wgrad(xd, td, dyd, None, now, Ci * 9, 9, 1, 0.5, 3, 3, 1, 1, flags=lib.CONV_F32_MFMA)
    pending = []
    ops.conv_wgrad(xd, td, dyd, None, later, Ci * 9, 9, 1, 0.5, 3, 3, 1, 1, flags=lib.CONV_F32_MFMA, defer=pending)
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


@pytest.mark.parametrize("case", [(1, 16, 32, 64, 64), (1, 8, 16, 512, 256)])
def test_forward_and_data_gradient_rounding_on_normal_data(case):
    lib, ops = _gpu()
    N, H, W, Ci, Co = case
    g = torch.Generator().manual_seed(sum(case))
    x, w = torch.randn(N, H, W, Ci, generator=g), torch.randn(Co, Ci, 3, 3, generator=g)
    dy = torch.randn(N, H, W, Co, generator=g)
    x64, w64, dy64 = x.double().permute(0, 3, 1, 2), w.double(), dy.double().permute(0, 3, 1, 2)
    ref = F.conv2d(x64, w64, None, 1, 1).permute(0, 2, 3, 1)
    mag = F.conv2d(x64.abs(), w64.abs(), None, 1, 1).permute(0, 2, 3, 1)
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
    y = torch.empty(N, H, W, Co, device=DEV)
    assert _on_new_path(lib, ops, xd, y)
    _fwd(lib, ops, xd, None, wd, y, lib.CONV_F32_MFMA, stats=False)
    r_fwd = _ratio(y.cpu(), ref, mag, 9 * Ci)
    print(f"forward {case}: largest error / bound = {r_fwd:.4f}")
    assert r_fwd <= 1.0
    # data gradient: Co -> Ci channels, K = 9 Co
    refd = F.conv_transpose2d(dy64, w64, None, 1, 1).permute(0, 2, 3, 1)
    magd = F.conv_transpose2d(dy64.abs(), w64.abs(), None, 1, 1).permute(0, 2, 3, 1)
    dx = torch.empty(N, H, W, Ci, device=DEV)
    assert _on_new_path(lib, ops, dyd, dx)
    _fwd(lib, ops, dyd, None, wd, dx, lib.CONV_F32_MFMA, pack=ops.pack_conv_dgrad, stats=False)
    r_dg = _ratio(dx.cpu(), refd, magd, 9 * Co)
    print(f"data gradient {case}: largest error / bound = {r_dg:.4f}")
    assert r_dg <= 1.0


def test_weight_gradient_rounding_on_normal_data():
    lib, ops = _gpu()
    case = (2, 32, 32, 64, 64)
    N, H, W, Ci, Co = case
    g = torch.Generator().manual_seed(sum(case))
    x, dy = torch.randn(N, H, W, Ci, generator=g), torch.randn(N, H, W, Co, generator=g)
    x64, dy64 = x.double().permute(0, 3, 1, 2), dy.double().permute(0, 3, 1, 2)
    wr = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x64, wr, None, 1, 1).backward(dy64)
    wa = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x64.abs(), wa, None, 1, 1).backward(dy64.abs())
    xd, dyd = x.to(DEV), dy.to(DEV)
    assert _on_new_path(lib, ops, xd, dyd) and _wgrad_on_new_path(lib, case)
    gw = torch.empty(Co, Ci, 3, 3, device=DEV)
    ops.conv_wgrad(xd, None, dyd, None, gw, Ci * 9, 9, 1, 1.0, 3, 3, 1, 1, flags=lib.CONV_F32_MFMA)
    r = _ratio(gw.cpu(), wr.grad, wa.grad, N * H * W)
    print(f"weight gradient {case}: largest error / bound = {r:.4f}")
    assert r <= 1.0


# ---- determinism, ignore rule ----------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bits():
    lib, ops = _gpu()
    N, H, W, Ci, Co = 2, 19, 45, 48, 72
    g = torch.Generator().manual_seed(11)
    x, w, dy = torch.randn(N, H, W, Ci, generator=g), torch.randn(Co, Ci, 3, 3, generator=g), torch.randn(N, H, W, Co, generator=g)
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
    outs = []
    for _ in range(2):
        y, gw = torch.empty(N, H, W, Co, device=DEV), torch.empty(Co, Ci, 3, 3, device=DEV)
        assert _on_new_path(lib, ops, xd, y)
        part = _fwd(lib, ops, xd, None, wd, y, lib.CONV_F32_MFMA)
        ops.conv_wgrad(xd, None, dyd, None, gw, Ci * 9, 9, 1, 1.0, 3, 3, 1, 1, flags=lib.CONV_F32_MFMA)
        outs.append((y.cpu(), part.cpu(), gw.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("Ci,flags", [(3, 0), (64, 2)])
def test_flag_is_ignored_on_the_device(Ci, flags):
    """Ci = 3 (the stem) with the flag, and an eligible shape under FORCE_GENERIC | F32_MFMA: bit-identical to the same call
    without the flag, forward, statistics and weight gradient."""
    lib, ops = _gpu()
    N, H, W, Co = 2, 13, 37, 64
    g = torch.Generator().manual_seed(Ci)
    x, w, dy = torch.randn(N, H, W, Ci, generator=g), torch.randn(Co, Ci, 3, 3, generator=g), torch.randn(N, H, W, Co, generator=g)
    xd, wd, dyd = x.to(DEV), w.to(DEV), dy.to(DEV)
    outs = []
    for f in (flags, flags | lib.CONV_F32_MFMA):
        y, gw = torch.empty(N, H, W, Co, device=DEV), torch.empty(Co, Ci, 3, 3, device=DEV)
        assert ops.conv_plan(xd, y, 3, 3, 1, 1, f) == ops.conv_plan(xd, y, 3, 3, 1, 1, flags)
        part = _fwd(lib, ops, xd, None, wd, y, f)
        ops.conv_wgrad(xd, None, dyd, None, gw, Ci * 9, 9, 1, 1.0, 3, 3, 1, 1, flags=f)
        outs.append((y.cpu(), part.cpu(), gw.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ---- whole network -----------------------------------------------------------------------------------------------------------------
class _Spy:
    """Records (R, S, input channels, flags) of every ops.conv_fwd / ops.conv_wgrad call of the tape."""

    def __init__(self, monkeypatch):
        from umi import ops
        self.calls = []
        fwd, wgrad = ops.conv_fwd, ops.conv_wgrad

        def conv_fwd(x, tx, wp, bias, y, R, S, stride, pad, want_stats=False, flags=0, up_offset=(0, 0)):
            self.calls.append(("fwd", R, S, stride, pad, x.shape[3], flags))
            return fwd(x, tx, wp, bias, y, R, S, stride, pad, want_stats=want_stats, flags=flags, up_offset=up_offset)

        def conv_wgrad(x, txa, dy, txb, dW, s_co, s_ci, s_t, out_scale, R, S, stride, pad, flags=0, defer=None):
            self.calls.append(("wgrad", R, S, stride, pad, x.shape[3], flags))
            return wgrad(x, txa, dy, txb, dW, s_co, s_ci, s_t, out_scale, R, S, stride, pad, flags=flags, defer=defer)

        monkeypatch.setattr(ops, "conv_fwd", conv_fwd)
        monkeypatch.setattr(ops, "conv_wgrad", conv_wgrad)

    def check(self, flag):
        flagged = [c for c in self.calls if c[1:3] == (3, 3) and c[5] % 8 == 0]
        assert {c[0] for c in flagged} == {"fwd", "wgrad"} and len(flagged) >= 3 * 17
        for c in self.calls:
            want = flag if (c[1:5] == (3, 3, 1, 1) and c[5] % 8 == 0) else 0
            assert c[6] & flag == want, c


@pytest.mark.parametrize("name", ["unet_1_2_8", "unet_3_4_8"])
def test_unet_fp32_mfma_parity(golden_dir, name, monkeypatch):
    """tests/test_gpu_unet.py::test_unet_fp32_parity under compute_dtype="fp32_mfma", same bars: logits rtol 1e-4 vs the
    REFERENCE's logits, argmax identical off near-ties, loss / grads / 3 SGD steps / eval-mode logits vs the oracle.  Every 3x3
    convolution call that reads a multiple of 8 channels carries the flag, no other call does."""
    lib, _ = _gpu()
    import Model
    import loss as L
    spy = _Spy(monkeypatch)
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    ref, x, lab = _oracle_run(g, 3)
    ncls = int(g["ncls"])
    L.CLASS_NUMBER = ncls
    m = Model.UNet(int(g["cin"]), ncls, int(g["feat"]), False, compute_dtype="fp32_mfma")
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
            spy.check(lib.CONV_F32_MFMA)
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


def test_unet_multitask_fp32_mfma_step0(golden_dir):
    """Step 0 of tests/test_gpu_unet.py::test_unet_multitask_parity[fp32] under "fp32_mfma", same bars."""
    _gpu()
    import Model
    import loss as L
    g = np.load(os.path.join(golden_dir, "unet_multitask_1_2_8.npz"))
    cin, ncls, feat = int(g["cin"]), int(g["ncls"]), int(g["feat"])
    B, H, W, seed = int(g["B"]), int(g["H"]), int(g["W"]), int(g["seed"])
    ref = ref_unet.RefUNetMultitask(cin, ncls, feat, False)
    ref.load_state_dict(recipe.fill_state_dict(ref.state_dict(), seed=seed))
    x, lab1 = recipe.synthetic_batch(B, cin, H, W, ncls, seed=seed)
    _, lab2 = recipe.synthetic_batch(B, cin, H, W, ncls, seed=seed + 100)
    L.CLASS_NUMBER = ncls
    m = Model.UNet_multitask(cin, ncls, feat, False, compute_dtype="fp32_mfma")
    m.load_state_dict(ref.state_dict())
    m.to(DEV).train()
    ref.train()
    o1, o2 = m(x.to(DEV))
    loss = L.calc_loss(o1, lab1.to(DEV), loss_type="dice_bce_mc") + L.calc_loss(o2, lab2.to(DEV), loss_type="dice_bce_mc")
    loss.backward()
    r1, r2 = ref(x)
    (ref_unet.dice_bce_mc(r1, lab1, ncls) + ref_unet.dice_bce_mc(r2, lab2, ncls)).backward()
    for o, key in ((o1, "logits1"), (o2, "logits2")):
        np.testing.assert_allclose(o.detach().cpu().numpy(), g[key], rtol=1e-4, atol=1e-4 * float(np.abs(g[key]).max()))
    assert abs(loss.item() - float(g["loss0"])) < 1e-4
    for (k, p), (_, rp) in zip(m.named_parameters(), ref.named_parameters()):
        assert rel_err(p.grad, rp.grad) < 2e-3, k


def test_unet_attention_fp32_mfma_step0(golden_dir):
    """Step 0 of tests/test_gpu_unet.py::test_unet_attention_parity[fp32] under "fp32_mfma", same bars."""
    _gpu()
    import Model
    import loss as L
    g = np.load(os.path.join(golden_dir, "unet_attention_1_2_8.npz"))
    cin, ncls, feat = int(g["cin"]), int(g["ncls"]), int(g["feat"])
    B, H, W, seed = int(g["B"]), int(g["H"]), int(g["W"]), int(g["seed"])
    ref = ref_unet.RefUNetAttention(cin, ncls, feat, False)
    ref.load_state_dict(recipe.fill_state_dict(ref.state_dict(), seed=seed))
    x, lab = recipe.synthetic_batch(B, cin, H, W, ncls, seed=seed)
    L.CLASS_NUMBER = ncls
    m = Model.UNet_attention(cin, ncls, feat, False, compute_dtype="fp32_mfma")
    m.load_state_dict(ref.state_dict())
    m.to(DEV).train()
    ref.double().train()
    logits = m(x.to(DEV))
    loss = L.calc_loss(logits, lab.to(DEV), loss_type="dice_bce_mc")
    loss.backward()
    ref_unet.dice_bce_mc(ref(x.double()), lab, ncls).backward()
    np.testing.assert_allclose(logits.detach().cpu().numpy(), g["logits"], rtol=1e-4, atol=1e-4 * float(np.abs(g["logits"]).max()))
    assert abs(loss.item() - float(g["loss0"])) < 1e-4
    for (k, p), (_, rp) in zip(m.named_parameters(), ref.named_parameters()):
        if _is_dead_bias(k):
            assert float(p.grad.abs().max()) < 1e-6, k
            assert float(rp.grad.abs().max()) < 1e-6, k
        else:
            assert rel_err(p.grad, rp.grad) < 2e-3, k
