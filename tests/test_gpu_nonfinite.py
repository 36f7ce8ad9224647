"""NaN / +Inf / -Inf through the FORWARD pass of a training step, against torch's semantics (tests/nonfinite_ref.py).

Kernel level: one small launch per case through the umi.ops / umi.ops_tu wrapper the tapes use, at the smallest shapes that reach
each code form (fp32 and fp16, 16-byte vector and scalar paths).  Step level: one training step of the smallest models of
tests/test_gpu_poisoned_step.py's recipe with a value planted in the input or in a weight: the loss is NaN, every parameter
gradient is non-finite, and a GradGuard skips the step with every parameter and optimizer-state bit in place -- eagerly and
under GraphedStep replay (a child process, as in the poison test).

Values are planted in floating-point data only (nonfinite_ref.plant), never in labels, indices, sizes or strides; no kernel under
test forms an address from floating-point data (the pool backward's `best` is a tap number 0..3, pool3s2's recorded taps 0..8,
the loss kernels index by the label alone), so a failing case fails by comparison, never by a fault.

Not covered on purpose: ONE NaN element under a transform whose rows are finite (eval-mode BatchNorm with finite running
statistics).  umi_tx's clamp returns `lo` there; see DESIGN.md, "Non-finite values in the training step"."""
import copy
import math
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

if __name__ == "__main__":                                   # the HIP-graph case runs this file as a child process
    _REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_REPO, os.path.join(_REPO, "unet-torch_amd")]

from oracle import recipe, ref_transunet, ref_unet
from tests import nonfinite_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 70                                                     # tests/test_gpu_poisoned_step.py
F64 = torch.float64
NAN, INF = R.NAN, R.INF
U32, U16 = 2.0 ** -24, 2.0 ** -11                             # unit roundoff of fp32 / fp16


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: torch.cuda.is_available() is False")
    from umi import lib, ops, ops_tu
    return lib, ops, ops_tu


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _dt(name):
    return torch.float16 if name == "fp16" else torch.float32


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().reshape(-1).view(torch.uint8),
                                                                     b.contiguous().reshape(-1).view(torch.uint8))


# =================================================================================================================================
# BatchNorm statistics -> bn_finalize -> the consumers of tx
# =================================================================================================================================
def _stat_rows(ops, xd):
    """Statistics partials [rows][2][C] of the stored tensor: the fp16 statistics pass where it applies (umi_bn_stats), else one
    row per (image, line) summed in fp32 on the device by torch -- the rows a convolution's statistics epilogue leaves."""
    part = ops.bn_stats(xd) if xd.dtype == torch.float16 else None
    if part is not None:
        return part, "umi_bn_stats"
    xf = xd.float()
    rows = torch.stack([xf.sum(2), (xf * xf).sum(2)], dim=2)                      # [N, H, 2, C]
    return rows.reshape(-1).contiguous(), "rows"


@pytest.mark.parametrize("value", list(R.VALUES))
@pytest.mark.parametrize("C", [16, 64])
@pytest.mark.parametrize("hw", [(9, 13), (16, 16)])
@pytest.mark.parametrize("dt", ["fp32", "fp16"])
def test_bn_statistics_carry_a_nonfinite_value_to_every_consumer(dt, hw, C, value):
    """One NaN / +Inf / -Inf in one channel of a raw tensor: bn_finalize (and the finalize-from-sums form, bit for bit) must
    leave a transform under which that channel reads as NaN in pool2_fwd and conv3x3, with NaN running_var (running_mean NaN,
    or +-Inf for an Inf, as 0.9 * old + 0.1 * mean is in torch) for that channel ONLY; the other channels within
    test_bn_finalize_row_reduction_forms' bars (tests/test_gpu_kernels.py: mean 1e-6, scale 2e-6 relative, shift 1e-5) and, through
    pool2_fwd, within one rounding of the storage format of the float64 value of the device's own transform."""
    lib, ops, _ = _need_gpu()
    dtype = _dt(dt)
    N, (H, W) = 2, hw
    g = _g(100 * C + H)
    shape = (N, H, W, C)
    where = R.positions(shape, channel=C // 2 + 1)["interior"]
    c = where[-1]
    x = R.plant((torch.randn(shape, generator=g) * 2 + 0.5).to(dtype), where, value)
    gamma = 0.5 + torch.rand(C, generator=g)
    gamma[::7] = -gamma[::7]
    beta = 0.1 * torch.randn(C, generator=g)
    rm0, rv0 = 0.2 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    xd = x.to(DEV)
    part, _ = _stat_rows(ops, xd)
    count = N * H * W
    rm, rv = rm0.to(DEV), rv0.to(DEV)
    tx, rstd = ops.bn_finalize(part, C, count, gamma.to(DEV), beta.to(DEV), 1e-5, 0.1, rm, rv)
    rm2, rv2 = rm0.to(DEV), rv0.to(DEV)
    tx2, rstd2 = ops.bn_finalize_sums(ops.bn_stat_sums(part, C, count), C, count, gamma.to(DEV), beta.to(DEV), 1e-5, 0.1, rm2, rv2)
    for a, b in ((tx, tx2), (rstd, rstd2), (rm, rm2), (rv, rv2)):
        assert _bits_equal(a, b)
    others = [k for k in range(C) if k != c]
    want_y, want_rm, want_rv = R.bn_relu_train(x, gamma, beta, 1e-5, True, 0.1, rm0, rv0)
    # the transform row: nothing finite survives in the planted channel, everything is finite elsewhere
    t = tx.cpu()
    assert bool(torch.isnan(t[c, 1:]).all()), t[c]
    assert bool(torch.isfinite(t[others]).all()) and bool((t[others, 3] == 0).all())
    mean, var, _ = R.bn_stats(x)
    scale = gamma.to(F64) / torch.sqrt(var + 1e-5)
    assert (t[others, 0].to(F64) - mean[others]).abs().max().item() < 1e-6 * max(1.0, mean[others].abs().max().item())
    assert (t[others, 1].to(F64) - scale[others]).abs().max().item() < 2e-6 * scale[others].abs().max().item()
    assert (t[others, 2].to(F64) - (beta.to(F64) - mean * scale)[others]).abs().max().item() < 1e-5
    # running statistics: fp32 arithmetic on O(1) values against float64 (the bars above: 1e-6 / 2e-6 relative), non-finite
    # entries exactly as the reference has them
    R.assert_same_nonfinite(rm, want_rm, 1e-6 * max(1.0, R.finite_scale(want_rm)), "running_mean")
    R.assert_same_nonfinite(rv, want_rv, 2e-6 * max(1.0, R.finite_scale(want_rv)), "running_var")
    assert int((~torch.isfinite(rm.cpu())).sum()) == 1 and int(torch.isnan(rv.cpu()).sum()) == 1 and bool(torch.isnan(rv[c]))
    # consumer 1: pool2_fwd with the transform
    y = torch.empty(N, H // 2, W // 2, C, device=DEV, dtype=dtype)
    ops.pool2_fwd(xd, tx, y)
    yc = y.cpu()
    assert bool(torch.isnan(yc[..., c]).all()), "the planted channel is not NaN everywhere after pool2_fwd"
    assert bool(torch.isnan(R.max_pool2(want_y)[..., c]).all())
    dev_act = torch.relu(R.apply_scale_shift(x, t))                               # float64 value of the device's own rows
    want_pool = R.max_pool2(dev_act)
    u = U16 if dtype == torch.float16 else U32
    R.assert_same_nonfinite(yc[..., others], want_pool[..., others], (u + 2 * U32) * R.finite_scale(want_pool[..., others]),
                            "pool2_fwd, other channels")
    # consumer 2: conv3x3 forward with the transform on its input (every output pixel reads the channel: all NaN, as F.conv2d)
    Co = 16
    w = torch.randn(Co, C, 3, 3, generator=g) * (2.0 / (9 * C)) ** 0.5
    want_conv = F.conv2d(want_y.permute(0, 3, 1, 2), w.to(F64), None, 1, 1)
    assert bool(torch.isnan(want_conv).all())
    z = torch.zeros(N, H, W, Co, device=DEV, dtype=dtype)
    wd = w.to(DEV)
    ops.conv_fwd(xd, tx, lambda l: ops.pack_conv_fwd(wd, dtype, k8=bool(l)), None, z, 3, 3, 1, 1)
    assert bool(torch.isnan(z).all()), f"{int(torch.isfinite(z).sum())} of {z.numel()} conv outputs are finite"


def test_eval_bn_tx_marks_non_finite_rows():
    """ops.eval_bn_tx: lo = NaN exactly where scale or shift is not finite (running_var NaN / Inf, running_mean Inf)."""
    _, ops, _ = _need_gpu()
    C = 8
    w, b = torch.linspace(0.5, 1.5, C), torch.linspace(-0.1, 0.1, C)
    rm, rv = torch.zeros(C), torch.ones(C)
    rv[1], rm[2], rv[3], w[4] = NAN, INF, INF, NAN                 # rv = Inf: rstd = 0, scale = 0, shift = beta: finite
    tx, _ = ops.eval_bn_tx(w.to(DEV), b.to(DEV), rm.to(DEV), rv.to(DEV), 1e-5)
    lo = tx[:, 3].cpu()
    assert torch.equal(torch.isnan(lo), torch.tensor([False, True, True, False, True, False, False, False]))
    assert bool((lo[~torch.isnan(lo)] == 0).all()) and not bool(torch.signbit(lo[~torch.isnan(lo)]).any())


# =================================================================================================================================
# MaxPool2d(2)
# =================================================================================================================================
def _pool_input(N, H, W, C, g):
    x = torch.randn(N, H, W, C, generator=g)
    x[0, 0, 1, :] = NAN                                                           # window (0, 0): one NaN
    x[0, 0:2, 2:4, :] = NAN                                                       # window (0, 1): four NaNs
    x[0, 2, 0, :] = INF                                                           # window (1, 0): +Inf among finite values
    x[0, 2:4, 2:4, :] = -INF                                                      # window (1, 1): four -Inf
    x[N - 1, 2 * (H // 2) - 1, 2 * (W // 2) - 1, C - 1] = NAN                     # the last window, last channel: NaN in its last tap
    return x


@pytest.mark.parametrize("hw", [(8, 8), (7, 9)])
@pytest.mark.parametrize("dt,C", [("fp16", 16), ("fp16", 12), ("fp32", 12)])
def test_pool2_windows_with_nonfinite_values(dt, C, hw):
    """pool2_fwd as F.max_pool2d: a window with one NaN and a window of four NaNs give NaN, +Inf wins, four -Inf give -Inf; exact
    (a selection).  fp16 C = 16: pool2_fwd_v8; C = 12 and fp32: the scalar kernel; (7, 9): odd sizes, the tail dropped.
    With a transform: rows as the statistics finalize stores them -- finite pass-through rows (scale > 0, lo = -inf) on the
    channels holding the Inf windows and all-NaN rows (a channel with non-finite statistics) that must read as NaN everywhere.
    pool2_bwd on the same inputs: each window's gradient goes to exactly one of its four positions, the tail gets zeros."""
    _, ops, _ = _need_gpu()
    dtype = _dt(dt)
    N, (H, W) = 2, hw
    Ho, Wo = H // 2, W // 2
    g = _g(7 * C + H)
    x = _pool_input(N, H, W, C, g).to(dtype)
    xd = x.to(DEV)
    dp = torch.randint(1, 4, (N, Ho, Wo, C), generator=g).to(dtype)               # non-zero: the routed position is visible

    def check(xin, tx, want, bar, what):
        xd, td = xin.to(DEV), None if tx is None else tx.to(DEV)
        y = torch.full((N, Ho, Wo, C), 7.0, device=DEV, dtype=dtype)
        ops.pool2_fwd(xd, td, y)
        R.assert_same_nonfinite(y, want, bar, "pool2_fwd " + what)
        da = torch.full((N, H, W, C), 7.0, device=DEV, dtype=dtype)
        ops.pool2_bwd(dp.to(DEV), xd, td, da, False)
        d = da.float().cpu()
        win = d[:, :2 * Ho, :2 * Wo].reshape(N, Ho, 2, Wo, 2, C)
        assert bool(torch.isfinite(d).all())
        assert torch.equal((win != 0).sum((2, 4)), torch.ones(N, Ho, Wo, C, dtype=torch.long)), "not exactly one position per window"
        assert torch.equal(win.sum((2, 4)), dp.float())
        assert float(d[:, 2 * Ho:].abs().sum()) == 0 and float(d[:, :, 2 * Wo:].abs().sum()) == 0

    want = R.max_pool2(x)
    assert math.isnan(want[0, 0, 0, 0]) and math.isnan(want[0, 0, 1, 0]) and want[0, 1, 0, 0] == INF and want[0, 1, 1, 0] == -INF
    assert math.isnan(want[N - 1, Ho - 1, Wo - 1, C - 1])
    check(x, None, want, 0.0, "as stored")
    # with a transform (the NaN elements of x are taken out again: one NaN under finite rows is the documented gap)
    xt = torch.where(torch.isnan(x), torch.zeros_like(x), x)
    tx = torch.zeros(C, 4)
    tx[:, 1], tx[:, 2], tx[:, 3] = 0.5 + torch.rand(C, generator=g), 0.1 * torch.randn(C, generator=g), -INF
    nan_rows = [1, C - 1]
    tx[nan_rows] = NAN
    want = R.max_pool2(R.apply_scale_shift(xt, tx))
    assert bool(torch.isnan(want[..., nan_rows]).all()) and want[0, 1, 0, 0] == INF and want[0, 1, 1, 0] == -INF
    assert int(torch.isnan(want).sum()) == N * Ho * Wo * len(nan_rows)
    u = U16 if dtype == torch.float16 else U32
    check(xt, tx, want, (u + 2 * U32) * R.finite_scale(want), "with a transform")  # one fp32 fma, then the store's rounding


@pytest.mark.parametrize("dt", ["fp32", "fp16"])
def test_pool3s2_nan_window(dt):
    """MaxPool2d(3, 2, 0) of the ResNet root (scalar kernels; fp16 C = 8: the 8-channel kernel with recorded taps): NaN windows as
    F.max_pool2d, and the backward sends each window's gradient to one input position (the sum over the input is the sum of dy)."""
    _, _, T = _need_gpu()
    dtype = _dt(dt)
    g = _g(11)
    N, H, W, C = 2, 9, 11, 8
    x = torch.randn(N, H, W, C, generator=g)
    x[0, 1, 1, :] = NAN
    x[1, 4:7, 4:7, 3] = NAN
    x[1, 8, 10, 7] = INF
    x = x.to(dtype)
    want = R.max_pool3s2(x)
    assert math.isnan(want[0, 0, 0, 0]) and math.isnan(want[1, 2, 2, 3]) and want[1, 3, 4, 7] == INF
    y = torch.empty(N, 4, 5, C, device=DEV, dtype=dtype)
    idx = torch.empty(N, 4, 5, C, device=DEV, dtype=torch.uint8) if dtype == torch.float16 else None
    T.pool3s2_fwd(x.to(DEV), y, idx)
    R.assert_same_nonfinite(y, want, 0.0, "pool3s2_fwd")
    if idx is not None:
        assert int(idx.max()) <= 8
    dy = torch.randint(1, 4, (N, 4, 5, C), generator=g).to(dtype)
    for use_idx in ([False, True] if idx is not None else [False]):
        dx = torch.empty(N, H, W, C, device=DEV, dtype=dtype)
        T.pool3s2_bwd(dy.to(DEV), x.to(DEV), dx, idx if use_idx else None)
        d = dx.float().cpu()
        assert bool(torch.isfinite(d).all()) and torch.equal(d.sum((1, 2)), dy.float().sum((1, 2)))
        # a window holding a NaN routes its gradient to a NaN tap, as torch does
        assert float(d[0, 1, 1, 0]) >= float(dy[0, 0, 0, 0])


# =================================================================================================================================
# GroupNorm (+ residual) + ReLU
# =================================================================================================================================
# bars: tests/test_gpu_kernels_tu.py::test_group_norm_fwd_bwd (fp32 2e-5, fp16 4e-3, times max |ref|)
GN_CASES = [("fp32", 64, 32, 2e-5), ("fp16", 64, 32, 4e-3), ("fp16", 12, 3, 4e-3)]     # fp16 C = 64: the f16v kernels; C = 12: generic


@pytest.mark.parametrize("relu,with_res", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("dt,C,G,tol", GN_CASES)
def test_group_norm_nonfinite(dt, C, G, tol, relu, with_res):
    """One NaN in one (image, group): that group NaN, every other group as the reference; a NaN only in `res`: that element."""
    _, _, T = _need_gpu()
    dtype = _dt(dt)
    N, H, W = 2, 7, 9
    g = _g(C + 2 * relu + with_res)
    x0 = (torch.randn(N, H, W, C, generator=g) * 2 + 0.5).to(dtype)
    res0 = torch.randn(N, H, W, C, generator=g).to(dtype) if with_res else None
    gamma, beta = 0.5 + torch.rand(C, generator=g), 0.1 * torch.randn(C, generator=g)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    where = (1, 3, 4, C // 2 + 1)
    plans = [("x", R.plant(x0, where, "nan"), res0)]
    if with_res:
        plans.append(("res", x0, R.plant(res0, where, "nan")))
    for name, x, res in plans:
        want = R.group_norm(x, G, gamma, beta, 1e-6, res, relu)
        cg = C // G
        n_nan = H * W * cg if name == "x" else 1
        assert int(torch.isnan(want).sum()) == n_nan and math.isnan(want[where])
        y = torch.empty(N, H, W, C, device=DEV, dtype=dtype)
        T.gn_fwd(x.to(DEV), gd, bd, G, 1e-6, relu, None if res is None else res.to(DEV), y)
        R.assert_same_nonfinite(y, want, tol * R.finite_scale(want), f"gn_fwd, NaN in {name}")


# =================================================================================================================================
# add2_relu
# =================================================================================================================================
# bars: tests/test_gpu_kernels_tu.py::test_add2_relu_fwd_bwd_vector_and_scalar_paths (fp16 2e-3, fp32 1e-6, times max(1, max |ref|))
@pytest.mark.parametrize("C,dt", [(32, "fp16"), (12, "fp16"), (20, "fp32")])      # 32: add2_relu_fwd_v8; 12 and fp32: scalar
def test_add2_relu_nonfinite(C, dt):
    """relu(a' + b') with a NaN or +Inf in a, in b, or in both.  Operands consumed as stored (tx None) per element; +Inf also under
    finite pass-through rows (lo = -inf); a NaN under a transform as the tape produces it: rows from bn_finalize of the operand
    itself with `lo += -inf` (BatchNorm without ReLU, umi/graph.py conv_bn), which make the whole channel NaN."""
    _, ops, _ = _need_gpu()
    dtype = _dt(dt)
    tol = 2e-3 if dtype == torch.float16 else 1e-6
    N, H, W = 2, 7, 9
    g = _g(C)
    a0, b0 = (torch.randn(N, H, W, C, generator=g).to(dtype) for _ in range(2))
    pa, pb = (0, 0, 0, 0), (N - 1, H - 1, W - 1, C - 1)
    t = torch.zeros(C, 4)
    t[:, 1], t[:, 2], t[:, 3] = 0.5 + torch.rand(C, generator=g), 0.3 * torch.randn(C, generator=g), -INF

    def run(a, ta, b, tb):
        y = torch.empty(N, H, W, C, device=DEV, dtype=dtype)
        ops.add2_relu(a.to(DEV), None if ta is None else ta.to(DEV), b.to(DEV), None if tb is None else tb.to(DEV), y)
        return y

    for value in ("nan", "+inf"):
        for a, b in ((R.plant(a0, pa, value), b0), (a0, R.plant(b0, pb, value)), (R.plant(a0, pa, value), R.plant(b0, pb, value)),
                     (R.plant(a0, pa, value), R.plant(b0, pa, value))):
            want = R.add2_relu(a, None, b, None)
            assert not bool(torch.isfinite(want[pa]) and torch.isfinite(want[pb]))
            R.assert_same_nonfinite(run(a, None, b, None), want, tol * max(1.0, R.finite_scale(want)), f"{value}, as stored")
            if value == "+inf":
                want = R.add2_relu(a, t, b, t)
                R.assert_same_nonfinite(run(a, t, b, t), want, tol * max(1.0, R.finite_scale(want)), "+inf, finite rows")
    # -Inf + +Inf = NaN inside the sum
    a, b = R.plant(a0, pa, "+inf"), R.plant(b0, pa, "-inf")
    want = R.add2_relu(a, None, b, None)
    assert math.isnan(want[pa])
    R.assert_same_nonfinite(run(a, None, b, None), want, tol * max(1.0, R.finite_scale(want)), "+inf + -inf")
    # a NaN under batch statistics: the whole channel, in a and in b
    for value in ("nan", "+inf"):
        a = R.plant(a0, (1, 3, 4, 5), value)
        ad = a.to(DEV)
        af = ad.float()
        part = torch.stack([af.sum(2), (af * af).sum(2)], dim=2).reshape(-1).contiguous()
        gamma, beta = (0.5 + torch.rand(C, generator=g)), 0.1 * torch.randn(C, generator=g)
        ta, _ = ops.bn_finalize(part, C, N * H * W, gamma.to(DEV), beta.to(DEV), 1e-5, 0.1, None, None)
        ta[:, 3] += ops.NEG_INF
        tac = ta.cpu()
        assert bool(torch.isnan(tac[5, 1:]).all()) and bool((tac[[k for k in range(C) if k != 5], 3] == -INF).all())
        bn_a = R.bn_relu_train(a, gamma, beta, 1e-5, relu_on=False)[0]
        for swap in (False, True):
            want = torch.relu(bn_a + R.apply_scale_shift(b0, t))
            assert bool(torch.isnan(want[..., 5]).all()) and int(torch.isnan(want).sum()) == N * H * W
            y = run(b0, t, a, ta) if swap else run(a, ta, b0, t)
            # finite entries: the transform rows carry bn_finalize's own error (scale 2e-6, shift 1e-5: test_bn_finalize_row_
            # reduction_forms) on top of the kernel's bar
            R.assert_same_nonfinite(y, want, (tol + 2e-5) * max(1.0, R.finite_scale(want)), f"{value} under batch statistics")


# =================================================================================================================================
# LayerNorm, GELU, attention, the loss: pinned as they are
# =================================================================================================================================
def test_layer_norm_and_gelu_keep_a_nan():
    """ln_fwd: one NaN in one row makes that row NaN and no other (bar 2e-5: test_layer_norm_gelu_pool_bilinear_fp32); gelu_fwd: that
    element (bar 2e-6, same test)."""
    _, _, T = _need_gpu()
    g = _g(2)
    B, N, C = 2, 37, 96
    x = R.plant(torch.randn(B, 1, N, C, generator=g), (1, 0, 20, 70), "nan")
    gamma, beta = 0.5 + torch.rand(C, generator=g), 0.1 * torch.randn(C, generator=g)
    want = R.layer_norm(x, gamma, beta, 1e-6)
    assert int(torch.isnan(want).sum()) == C and bool(torch.isnan(want[1, 0, 20]).all())
    y = torch.empty_like(x, device=DEV)
    T.ln_fwd(x.to(DEV), gamma.to(DEV), beta.to(DEV), 1e-6, y)
    R.assert_same_nonfinite(y, want, 2e-5 * R.finite_scale(want), "ln_fwd")
    u = R.plant(torch.randn(B, 1, N, C, generator=g) * 2, (0, 0, 3, 5), "nan")
    u[1, 0, 7, 9] = INF
    o = torch.empty_like(u, device=DEV)
    T.gelu_fwd(u.to(DEV), o)
    want = R.gelu(u)
    assert int(torch.isnan(want).sum()) == 1 and want[1, 0, 7, 9] == INF
    R.assert_same_nonfinite(o, want, 2e-6 * R.finite_scale(want), "gelu_fwd")


# bars: tests/test_gpu_kernels_tu.py::test_attention_fwd_bwd (fp32 2e-5, fp16 3e-3, times max |ref|); tests/attn_dropout_cases.py BARS_F32
ATTN_CASES = [("fp32", 50, 4, 16, 0, 0, 2e-5), ("fp16", 196, 3, 64, 0, 1, 3e-3), ("fp32", 196, 3, 64, 1, 2, 2e-5)]


@pytest.mark.parametrize("which", ["q", "k", "v"])
@pytest.mark.parametrize("dt,N,heads,D,flags,kernel,tol", ATTN_CASES)
def test_attention_forward_keeps_a_nan(dt, N, heads, D, flags, kernel, tol, which):
    """One NaN in one query / key / value of image 1, head 1: the scalar, fp16 matrix-core and fp32 matrix-core kernels (named by
    umi_attn_plan) give NaN where softmax attention does -- one output row for a query, the whole (image, head) for a key, that
    head's column of the value for a value -- and leave every other (image, head) within the bar."""
    lib, _, T = _need_gpu()
    dtype = _dt(dt)
    g = _g(3)
    B, C = 2, heads * D
    q, k, v = (torch.randn(B, 1, N, C, generator=g).to(dtype) for _ in range(3))
    ts = dict(q=q, k=k, v=v)
    ts[which] = R.plant(ts[which], (1, 0, N // 2, D + 3), "nan")
    q, k, v = ts["q"], ts["k"], ts["v"]
    want = R.attention(q, k, v, heads)
    nan = torch.isnan(want)
    assert not bool(nan[0].any()) and not bool(nan[1, 0, :, :D].any()) and not bool(nan[1, 0, :, 2 * D:].any())
    assert int(nan.sum()) == {"q": D, "k": N * D, "v": N}[which]
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    o = torch.empty(B, 1, N, C, device=DEV, dtype=dtype)
    assert T.attn_plan(qd, kd, vd, o, heads, flags) == kernel
    T.attn_fwd(qd, kd, vd, o, heads, flags)
    R.assert_same_nonfinite(o, want, tol * R.finite_scale(want), f"attn_fwd, NaN in {which}")


@pytest.mark.parametrize("C", [2, 4])
def test_dice_ce_nan_logit(C):
    """umi_dice_ce_fwd / _bwd at 2 x C x 33 x 31: one NaN logit gives a NaN loss and, through the global Dice sums, a NaN in EVERY
    dlogits entry, as torch's gradient."""
    _need_gpu()
    import loss as L
    g = _g(5 + C)
    x = torch.randn(2, C, 33, 31, generator=g)
    lab = torch.randint(0, C, (2, 33, 31), generator=g).float()
    x = R.plant(x, (1, C - 1, 16, 15), "nan")
    want_loss, want_grad = R.dice_bce_mc_with_grad(x, lab, C)
    assert math.isnan(float(want_loss)) and bool(torch.isnan(want_grad).all())
    L.CLASS_NUMBER = C
    xd = x.to(DEV).requires_grad_(True)
    loss = L.calc_loss(xd, lab.to(DEV), loss_type="dice_bce_mc")
    loss.backward()
    assert math.isnan(float(loss))
    assert bool(torch.isnan(xd.grad).all()), f"{int((~torch.isnan(xd.grad)).sum())} of {xd.grad.numel()} dlogits entries are not NaN"


# =================================================================================================================================
# One training step
# =================================================================================================================================
STEP_CASES = {
    "unet8_fp32_32x32": dict(model=("UNet", 1, 2, 8), dtype="fp32", shape=(2, 1, 32, 32)),
    "unet8_fp16_32x32": dict(model=("UNet", 1, 2, 8), dtype="fp16", shape=(2, 1, 32, 32)),
    "unet64_fp16_64x64": dict(model=("UNet", 1, 2, 64), dtype="fp16", shape=(2, 1, 64, 64)),          # MFMA forms, fused backward
    "attention64_fp16_64x64": dict(model=("UNet_attention", 1, 2, 64), dtype="fp16", shape=(2, 1, 64, 64)),
    "unet64_fp32_mfma_32x48": dict(model=("UNet", 1, 2, 64), dtype="fp32_mfma", shape=(2, 1, 32, 48)),
    "transunet_small_fp16": dict(model=("TransUNet", "small", 64), dtype="fp16", shape=(2, 1, 64, 64)),
    "transunet_small_fp32": dict(model=("TransUNet", "small", 64), dtype="fp32", shape=(2, 1, 64, 64)),
}
GRAPH_CASE = "unet64_fp16_64x64"
PLANTS = ("nan_pixel", "inf_pixel", "nan_weight")
# (d) the fp16 overflow plant: output channel 3 of that conv times a power of two chosen on the float64 oracle.  The fp16 modes of
# the U-Net family; TransUNet's ResNet convolutions standardise their weights, so no power of two moves their output
# (tests/test_nonfinite_ref.py::test_no_power_of_two_overflows_a_standardised_convolution asserts that on the oracle)
OVERFLOW_CASES = ("unet8_fp16_32x32", "unet64_fp16_64x64", "attention64_fp16_64x64")
STEP_PARAMS = [(n, p) for n in STEP_CASES for p in PLANTS] + [(n, "overflow") for n in OVERFLOW_CASES]


def _weight_key(case):
    """The first conv of the second encoder block / of the second ResNet stage."""
    if case["model"][0] == "TransUNet":
        return "transformer.embeddings.hybrid_model.body.block2.unit1.conv1.weight"
    return "down1.maxpool_conv.1.double_conv.0.weight"


def _master(case):
    """tests/test_gpu_poisoned_step.py's recipe: the case's network on the CPU with seeded weights."""
    from tests.test_gpu_poisoned_step import _master as recipe_master
    return recipe_master(case)


def _oracle(case, state):
    """The CPU oracle of the case in float64 holding `state`."""
    kind = case["model"][0]
    if kind == "TransUNet":
        ref = ref_transunet.RefTransUNet(ref_transunet.small_config(2), case["model"][2])
    else:
        ref = {"UNet": ref_unet.RefUNet, "UNet_attention": ref_unet.RefUNetAttention}[kind](*case["model"][1:], False)
    ref.load_state_dict(state)
    return ref.double().train()


def _overflow_power(case, x, state):
    """(d): the smallest power of two that puts the oracle's pre-normalisation maximum of output channel 3 above 2^17 while every
    other tensor of its forward stays below 2^14; both conditions are asserted there (nonfinite_ref.overflow_power), on the CPU."""
    assert case["dtype"] == "fp16" and case["model"][0] != "TransUNet"
    return R.overflow_power(ref_unet, lambda: _oracle(case, state), x.double(), _weight_key(case))


def _planted(case, plant, x, state, k=None):
    """(x, state) with the plant applied to copies; k: the power of two of the overflow plant."""
    x, state = x.clone(), {k: v.clone() for k, v in state.items()}
    B, _, H, W = x.shape
    if plant == "nan_pixel":
        x[B - 1, 0, H // 2 + 1, W // 2 - 2] = NAN
    elif plant == "inf_pixel":
        x[B - 1, 0, H // 2 + 1, W // 2 - 2] = INF
    else:
        w = state[_weight_key(case)]
        assert w.is_floating_point() and w.dim() == 4
        if plant == "overflow":
            w[3] *= 2.0 ** k
        else:
            w[3, 1, 0, 0] = NAN
    return x, state


def _premise_on_the_oracle(case, x, lab, state):
    ref = _oracle(case, state)
    loss = ref_unet.dice_bce_mc(ref(x.double()), lab, 2)
    loss.backward()
    assert math.isnan(float(loss.detach())), "premise: the oracle's loss is not NaN"
    clean = [k for k, p in ref.named_parameters() if p.grad is None or not bool(torch.isnan(p.grad).any())]
    assert not clean, f"premise: oracle gradients without a NaN: {clean[:6]}"


def _opt_state(m, opt):
    out = {"param." + k: p.detach().clone() for k, p in m.named_parameters()}
    for k, p in m.named_parameters():
        for name in ("momentum_buffer", "exp_avg", "exp_avg_sq"):
            v = opt.state.get(p, {}).get(name)
            if v is not None:
                out[f"{name}.{k}"] = v.detach().clone()
    if opt.device_hyper is not None:
        for i, h in enumerate(opt.sync_host()):
            out[f"adam_t.{i}"] = torch.tensor(float(h["adam_t"]))
    return out


def _assert_same_state(before, after):
    assert list(before) == list(after)
    changed = [k for k in before if not _bits_equal(before[k], after[k])]
    assert not changed, f"a skipped step changed {len(changed)} tensors: {changed[:6]}"


def _make_opt(kind, m):
    from umi import optim as uo
    if kind == "adam":
        opt = uo.Adam(m.parameters(), lr=1e-3, weight_decay=1e-4)
        opt.device_schedule()
    else:
        opt = uo.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    guard = uo.GradGuard()                                    # no clipping, fixed scale
    opt.grad_guard(guard)
    return opt, guard


def _step(m, opt, x, lab):
    import loss as L
    loss = L.calc_loss(m(x), lab, loss_type="dice_bce_mc")
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
    return loss.detach()


def _guarded_steps(case, master, x_clean, lab, plant, kind, k=None):
    """A clean step (applied: the optimizer state holds values), then the planted one.  Returns what the assertions need."""
    import loss as L
    L.CLASS_NUMBER = 2
    torch.manual_seed(SEED)
    m = copy.deepcopy(master).to(DEV).train()
    opt, guard = _make_opt(kind, m)
    xc, labd = x_clean.to(DEV), lab.to(DEV)
    loss0 = _step(m, opt, xc, labd)
    r0 = guard.read()
    assert math.isfinite(float(loss0)) and r0["nonfinite"] == 0 and r0["skipped"] == 0 and r0["steps"] == 1
    xp, state = _planted(case, plant, x_clean, {n: v.detach().cpu() for n, v in m.state_dict().items()}, k)
    if plant in ("nan_weight", "overflow"):
        with torch.no_grad():
            dict(m.named_parameters())[_weight_key(case)].copy_(state[_weight_key(case)])
    before = _opt_state(m, opt)
    loss = _step(m, opt, xp.to(DEV), labd)
    torch.cuda.synchronize()
    return m, opt, guard, before, loss


@pytest.mark.parametrize("name,plant", STEP_PARAMS)
def test_step_reports_nan_and_the_guard_skips_it(name, plant):
    """(a) NaN at one input pixel, (b) +Inf at one input pixel, (c) NaN in one element of the first conv of the second encoder
    block (TransUNet: of the second ResNet stage).  Premise on the float64 oracle: its loss is NaN and every parameter gradient
    holds a NaN.  (d), fp16 U-Net family: output channel 3 of that conv times the power of two chosen (and its two conditions
    asserted) on the oracle, whose own loss stays finite: the expectation is torch's fp16 behaviour, the channel overflows to
    +-Inf in the fp16 store and the loss is NaN.  On the device: 1. the loss is NaN; 2. every parameter's gradient holds a non-finite element; 3. the GradGuard
    counts them and skips the step, and every parameter, momentum buffer, Adam moment and Adam's step count keeps its bits."""
    _need_gpu()
    case = STEP_CASES[name]
    master = _master(case)
    B, C, H, W = case["shape"]
    x, lab = recipe.synthetic_batch(B, C, H, W, 2, seed=SEED)
    k = None
    if plant == "overflow":
        k = _overflow_power(case, x, master.state_dict())                      # asserts both conditions before any launch
        ref = _oracle(case, _planted(case, plant, x, master.state_dict(), k)[1])
        assert math.isfinite(float(ref_unet.dice_bce_mc(ref(x.double()), lab, 2).detach()))
    else:
        xp, state = _planted(case, plant, x, master.state_dict())
        _premise_on_the_oracle(case, xp, lab, state)
    for kind in ("sgd", "adam"):
        m, opt, guard, before, loss = _guarded_steps(case, master, x, lab, plant, kind, k)
        assert math.isnan(float(loss)), f"{kind}: the loss of the planted step is {float(loss)!r}, not NaN"
        finite = [k for k, p in m.named_parameters() if p.grad is None or bool(torch.isfinite(p.grad).all())]
        assert not finite, f"{kind}: {len(finite)} parameter gradients are finite: {finite[:6]}"
        r = guard.read()
        assert r["nonfinite"] > 0 and r["skipped"] == 1 and r["steps"] == 2, r
        _assert_same_state(before, _opt_state(m, opt))


def _graph_child():
    """GraphedStep of UNet(1,2,64) fp16 with a guarded SGD: warm-up and first replay on the clean batch (applied), then a replay
    per plant -- (a), (b) on the planted input, (c), (d) on the planted weight, copied into the parameter before the replay and taken
    out again after it -- : NaN loss, non-finite gradients everywhere, skipped, every bit in place; then a clean replay is applied
    again."""
    import loss as L
    from umi.graphs import GraphedStep
    case = STEP_CASES[GRAPH_CASE]
    L.CLASS_NUMBER = 2
    master = _master(case)
    B, C, H, W = case["shape"]
    x, lab = recipe.synthetic_batch(B, C, H, W, 2, seed=SEED)
    k = _overflow_power(case, x, master.state_dict())
    torch.manual_seed(SEED)
    m = copy.deepcopy(master).to(DEV).train()
    opt, guard = _make_opt("sgd", m)
    wparam = dict(m.named_parameters())[_weight_key(case)]
    xd, labd = x.to(DEV), lab.to(DEV)
    gs = GraphedStep(lambda xx, ll: _step(m, opt, xx, ll), [xd, labd], warmup=1)
    loss = gs(xd, labd)
    r = guard.read()
    assert math.isfinite(float(loss)) and r["skipped"] == 0 and r["steps"] == 2, r
    skipped = 0
    for plant in PLANTS + ("overflow",):
        keep = wparam.detach().clone()
        xp, state = _planted(case, plant, x, {_weight_key(case): keep.cpu()}, k)
        with torch.no_grad():
            wparam.copy_(state[_weight_key(case)])
        before = _opt_state(m, opt)
        loss = gs(xp.to(DEV), labd)
        torch.cuda.synchronize()
        skipped += 1
        assert math.isnan(float(loss)), (plant, float(loss))
        finite = [k for k, p in m.named_parameters() if bool(torch.isfinite(p.grad).all())]
        assert not finite, (plant, finite[:6])
        r = guard.read()
        assert r["nonfinite"] > 0 and r["skipped"] == skipped, (plant, r)
        _assert_same_state(before, _opt_state(m, opt))
        with torch.no_grad():
            wparam.copy_(keep)
    # (BatchNorm's running statistics are module buffers, not optimizer state: the planted steps left NaN in them, which only
    #  eval mode reads; the training step after them uses batch statistics and is applied)
    before = _opt_state(m, opt)
    loss = gs(xd, labd)
    r = guard.read()
    assert math.isfinite(float(loss)) and r["nonfinite"] == 0 and r["skipped"] == skipped, r
    assert not _bits_equal(before["param.inc.double_conv.0.weight"], _opt_state(m, opt)["param.inc.double_conv.0.weight"])
    print("NONFINITE_GRAPH_OK", r)


def test_graphed_step_reports_nan_and_the_guard_skips_it():
    """The same through umi.graphs.GraphedStep replay, in a fresh child process (stream capture is sensitive to what ran before
    it in the process); the child's exit status is checked."""
    _need_gpu()
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "NONFINITE_GRAPH_OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])


if __name__ == "__main__":
    _graph_child()
