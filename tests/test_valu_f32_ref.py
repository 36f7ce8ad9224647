"""tests/valu_f32_ref.py against torch's own float64 operators, on the CPU: the float64 statement that tests/test_gpu_valu_f32.py
holds the fp32 VALU kernels to is itself pinned here, to `==` on small-integer data (the builders of tests/test_gpu_exact.py) and
to 1e-12 of the result's scale on standard-normal data (two float64 summation orders of at most ~10^4 terms differ by ~10^-13)."""
import pytest
import torch
import torch.nn.functional as F

from tests import valu_f32_ref as R
from tests.test_gpu_exact import _apply, _int_tx, _ints

F64 = torch.float64


def _gen(*key):
    return torch.Generator().manual_seed(sum(int(k) for k in key) + 7)


def _norm_tx(C, g, floor=0.0):
    t = torch.empty(C, 4)
    t[:, 0] = 0.3 * torch.randn(C, generator=g)
    t[:, 1] = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0)
    t[:, 2] = 0.2 * torch.randn(C, generator=g)
    t[:, 3] = floor
    return t


def _data(shape, g, ints, lo=-2, hi=2):
    return _ints(shape, lo, hi, g) if ints else torch.randn(shape, generator=g)


def _tx_of(C, g, ints, floor=0.0):
    t = _int_tx(C, g) if ints else _norm_tx(C, g)
    t[:, 3] = floor
    return t


def _act(x, t):
    """the transform by torch, float64 (for integer data the same values as test_gpu_exact._apply where floor = 0)"""
    if t is None:
        return x.to(F64)
    return torch.maximum(x.to(F64) * t[:, 1].to(F64) + t[:, 2].to(F64), t[:, 3].to(F64))


def _same(got, ref, ints):
    if ints:
        assert torch.equal(got, ref.to(F64))
    else:
        assert (got - ref).abs().max().item() <= 1e-12 * max(ref.abs().max().item(), 1.0)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def test_transform_matches_the_integer_builder():
    g = _gen(1)
    x, t = _ints((2, 3, 5, 7), -2, 2, g), _int_tx(7, g)
    a, m = R.apply_tx(x, t)
    assert torch.equal(a, _apply(x, t).to(F64))
    assert torch.equal(m, x.abs().to(F64) * t[:, 1].abs() + t[:, 2].abs()) and (m >= a.abs()).all()
    a, m = R.apply_tx(x, None)
    assert torch.equal(a, x.to(F64)) and torch.equal(m, x.abs().to(F64))


CONV = [  # N, H, W, Ci, Co, R, stride, pad, tx floor (None: no transform), bias
    (2, 11, 13, 5, 7, 3, 1, 1, 0.0, False),
    (1, 9, 7, 8, 3, 3, 1, 1, float("-inf"), True),
    (2, 6, 5, 4, 2, 1, 1, 0, None, True),
    (1, 1, 1, 3, 4, 3, 1, 1, 0.0, False),
    (2, 11, 13, 6, 5, 3, 2, 1, 0.0, False),
    (2, 11, 13, 6, 5, 1, 2, 0, None, False),
    (1, 12, 12, 3, 4, 3, 2, 1, None, True),
    (1, 8, 6, 4, 3, 2, 2, 0, 0.0, False),      # the transposed convolution's data gradient form
]


@pytest.mark.parametrize("ints", [True, False])
@pytest.mark.parametrize("case", CONV)
def test_conv_forward_and_packing(case, ints):
    N, H, W, Ci, Co, K, stride, pad, floor, has_bias = case
    g = _gen(*case[:8], ints)
    x = _data((N, H, W, Ci + 3), g, ints)[..., 2:2 + Ci]            # a channel slice of a wider buffer
    w = _data((Co, Ci, K, K), g, ints, -1, 1)
    b = _data((Co,), g, ints, -3, 3) if has_bias else None
    t = _tx_of(Ci, g, ints, floor) if floor is not None else None
    ref = _nhwc(F.conv2d(_nchw(_act(x, t)), w.to(F64), b.to(F64) if has_bias else None, stride, pad))
    y, mag = R.conv_fwd(x, t, R.pack_conv_fwd(w), b, K, K, stride, pad, Co)
    _same(y, ref, ints)
    mref = _nhwc(F.conv2d(_nchw(R.apply_tx(x, t)[1]), w.to(F64).abs(), b.to(F64).abs() if has_bias else None, stride, pad))
    _same(mag, mref, ints)
    assert (mag >= y.abs() * (1 - 1e-12)).all()
    s, q, sa = R.conv_stats(y)
    _same(s, ref.sum((0, 1, 2)), ints)
    _same(q, (ref * ref).sum((0, 1, 2)), ints)
    _same(sa, ref.abs().sum((0, 1, 2)), ints)


@pytest.mark.parametrize("ints", [True, False])
@pytest.mark.parametrize("case", [(2, 11, 13, 5, 7, 3, 1), (1, 9, 7, 8, 3, 3, 1), (2, 6, 5, 4, 2, 1, 0), (1, 1, 1, 3, 4, 3, 1)])
def test_stride1_data_gradient_is_the_forward_on_the_rotated_panel(case, ints):
    N, H, W, Ci, Co, K, pad = case
    g = _gen(*case, ints)
    w = _data((Co, Ci, K, K), g, ints, -1, 1)
    dy = _data((N, H + 2 * pad - K + 1, W + 2 * pad - K + 1, Co), g, ints, -1, 1)
    xr = torch.zeros(N, Ci, H, W, dtype=F64, requires_grad=True)
    F.conv2d(xr, w.to(F64), None, 1, pad).backward(_nchw(dy.to(F64)))
    dx, mag = R.conv_fwd(dy, None, R.pack_conv_dgrad(w), None, K, K, 1, K - 1 - pad, Ci)
    _same(dx, _nhwc(xr.grad), ints)
    assert (mag >= dx.abs() * (1 - 1e-12)).all()


@pytest.mark.parametrize("ints", [True, False])
@pytest.mark.parametrize("case", [(2, 11, 13, 6, 5, 3, 2, 1), (2, 11, 13, 6, 5, 1, 2, 0), (1, 12, 12, 3, 4, 3, 2, 1),
                                  (1, 12, 12, 3, 4, 1, 2, 0), (1, 7, 9, 2, 3, 3, 3, 1)])
def test_strided_data_gradient(case, ints):
    N, H, W, Ci, Co, K, stride, pad = case
    g = _gen(*case, ints)
    w = _data((Co, Ci, K, K), g, ints, -1, 1)
    xr = torch.zeros(N, Ci, H, W, dtype=F64, requires_grad=True)
    yr = F.conv2d(xr, w.to(F64), None, stride, pad)
    dy = _data(tuple(_nhwc(yr).shape), g, ints, -1, 1)
    yr.backward(_nchw(dy.to(F64)))
    dx, mag = R.conv_dgrad_strided(dy, R.pack_conv_dgrad_strided(w), K, K, stride, pad, (H, W), Ci)
    _same(dx, _nhwc(xr.grad), ints)
    ar = torch.zeros(N, Ci, H, W, dtype=F64, requires_grad=True)
    F.conv2d(ar, w.to(F64).abs(), None, stride, pad).backward(_nchw(dy.to(F64).abs()))
    _same(mag, _nhwc(ar.grad), ints)


CONVT = [  # N, H, W, Cin, Cout, extra rows, extra columns, offset
    (2, 5, 6, 8, 4, 0, 0, (0, 0)),
    (1, 3, 4, 5, 6, 1, 1, (0, 0)),
    (2, 3, 4, 5, 6, 2, 1, (1, 0)),
    (1, 4, 3, 4, 3, 1, 2, (0, 1)),
]


@pytest.mark.parametrize("ints", [True, False])
@pytest.mark.parametrize("case", CONVT)
def test_conv_transpose_trio(case, ints):
    """Forward = F.conv_transpose2d then F.pad by the offset; its data gradient = the 2x2 / stride-2 forward on pack_convT_dgrad
    of the cropped gradient; its weight gradient = conv_wgrad with the operands swapped, written in (Cin, Cout, 2, 2) order."""
    N, H, W, Cin, Cout, eh, ew, off = case
    g = _gen(*case[:7], *off, ints)
    x = _data((N, H, W, Cin), g, ints)
    w = _data((Cin, Cout, 2, 2), g, ints, -1, 1)
    b = _data((Cout,), g, ints, -3, 3)
    t = _tx_of(Cin, g, ints)
    oH, oW = 2 * H + eh, 2 * W + ew
    wr, br = w.to(F64).requires_grad_(True), b.to(F64).requires_grad_(True)
    ar = _act(x, t).requires_grad_(True)
    up = F.conv_transpose2d(_nchw(ar), wr, br, stride=2)
    ref = _nhwc(F.pad(up, (off[1], oW - 2 * W - off[1], off[0], oH - 2 * H - off[0])))
    y, mag, written = R.convT_fwd(x, t, R.pack_convT_fwd(w), b, off, (oH, oW), Cout)
    _same(y, ref, ints)
    inside = torch.zeros(N, oH, oW, dtype=torch.bool)
    inside[:, off[0]:off[0] + 2 * H, off[1]:off[1] + 2 * W] = True
    assert torch.equal(written, inside) and (mag[~written] == 0).all() and (mag >= y.abs() * (1 - 1e-12)).all()
    # an offset that pushes the scatter past the destination: those positions are dropped
    y2, _, wr2 = R.convT_fwd(x, t, R.pack_convT_fwd(w), b, (eh + 1, -1), (oH, oW), Cout)
    full = _nhwc(F.pad(up.detach(), (-1, oW - 2 * W + 1, eh + 1, -1)))
    assert torch.equal(wr2, _nhwc(F.pad(torch.ones(N, 1, 2 * H, 2 * W), (-1, oW - 2 * W + 1, eh + 1, -1)))[..., 0] > 0)
    _same(y2, full, ints)
    # gradients of the cropped map
    gup = _data((N, oH, oW, Cout), g, ints, -1, 1)
    gc = gup[:, off[0]:off[0] + 2 * H, off[1]:off[1] + 2 * W].contiguous()
    up.backward(_nchw(gc.to(F64)))
    dx, _ = R.conv_fwd(gc, None, R.pack_convT_dgrad(w), None, 2, 2, 2, 0, Cin)
    _same(dx, ar.grad, ints)
    dW, _ = R.conv_wgrad(gc, None, x, t, 2, 2, 2, 0, w.numel(), Cout * 4, 4, 1, 0.5)
    _same(dW.view(Cin, Cout, 2, 2), 0.5 * wr.grad, ints)
    db, dbm = R.colsum(gc, 0.5)
    _same(db, 0.5 * br.grad, ints)
    _same(dbm, 0.5 * gc.to(F64).abs().sum((0, 1, 2)), ints)


WGRAD = [  # N, H, W, Ci, Co, R, stride, pad, txa, txb
    (2, 11, 13, 5, 7, 3, 1, 1, True, False),
    (1, 9, 7, 8, 3, 3, 1, 1, True, True),
    (2, 6, 5, 4, 2, 1, 1, 0, False, False),
    (2, 11, 13, 6, 5, 3, 2, 1, True, False),
    (1, 12, 12, 3, 4, 1, 2, 0, False, True),
]


@pytest.mark.parametrize("ints", [True, False])
@pytest.mark.parametrize("case", WGRAD)
def test_weight_gradient(case, ints):
    N, H, W, Ci, Co, K, stride, pad, use_a, use_b = case
    g = _gen(*case, ints)
    x = _data((N, H, W, Ci), g, ints)
    ta = _tx_of(Ci, g, ints) if use_a else None
    tb = _tx_of(Co, g, ints, float("-inf")) if use_b else None
    wr = torch.zeros(Co, Ci, K, K, dtype=F64, requires_grad=True)
    yr = F.conv2d(_nchw(_act(x, ta)), wr, None, stride, pad)
    dy = _data(tuple(_nhwc(yr).shape), g, ints, -1, 1)
    yr.backward(_nchw(_act(dy, tb)))
    dW, mag = R.conv_wgrad(x, ta, dy, tb, K, K, stride, pad, wr.numel(), Ci * K * K, K * K, 1, 0.25)
    _same(dW.view(Co, Ci, K, K), 0.25 * wr.grad, ints)
    assert (mag >= dW.abs() * (1 - 1e-12)).all()
    mr = torch.zeros(Co, Ci, K, K, dtype=F64, requires_grad=True)
    F.conv2d(_nchw(R.apply_tx(x, ta)[1]), mr, None, stride, pad).backward(_nchw(R.apply_tx(dy, tb)[1]))
    _same(mag.view(Co, Ci, K, K), 0.25 * mr.grad, ints)
    # another destination order, with room between the elements: untouched elements keep the fill
    dW2, _ = R.conv_wgrad(x, ta, dy, tb, K, K, stride, pad, 2 * wr.numel(), 2 * K * K, 2 * Co * K * K, 2, 0.25, fill=-7.0)
    v = dW2.view(Ci, Co, K * K, 2)
    _same(v[..., 0].reshape(Ci, Co, K, K), 0.25 * wr.grad.permute(1, 0, 2, 3), ints)
    assert (v[..., 1] == -7.0).all()


@pytest.mark.parametrize("ints", [True, False])
@pytest.mark.parametrize("shape", [(2, 16, 24, 6), (1, 9, 7, 3), (3, 33, 31, 2), (1, 2, 2, 1)])
@pytest.mark.parametrize("use_tx", [False, True])
def test_pool2(shape, use_tx, ints):
    """F.max_pool2d and its autograd (first maximum takes the gradient: integer data is full of ties); negative scales in the
    transform reverse the ordering."""
    N, H, W, C = shape
    g = _gen(*shape, use_tx, ints)
    x = _data(shape, g, ints)
    t = _tx_of(C, g, ints, float("-inf")) if use_tx else None
    ar = _nchw(_act(x, t)).clone().requires_grad_(True)
    pr = F.max_pool2d(ar, 2)
    dp = _data((N, H // 2, W // 2, C), g, ints, -3, 3)
    pr.backward(_nchw(dp.to(F64)))
    _same(R.pool2_fwd(x, t), _nhwc(pr.detach()), True)                     # a selection: bit for bit on any data
    old = _data(shape, g, ints, -3, 3)
    _same(R.pool2_bwd(dp, x, t, old, False), _nhwc(ar.grad), True)
    _same(R.pool2_bwd(dp, x, t, old, True), _nhwc(ar.grad) + old.to(F64), True)


@pytest.mark.parametrize("ints", [True, False])
@pytest.mark.parametrize("M,C", [(1, 3), (257, 2), (300, 5)])
def test_batchnorm_backward(M, C, ints):
    """BatchNorm (batch statistics) + ReLU composed in float64 and differentiated: the reduce stage's two sums are the gradients of
    beta and gamma, the apply stage's result is the gradient of the BatchNorm's input."""
    g = _gen(M, C, ints)
    y = (_ints((1, 1, M, C), -3, 3, g) if ints else torch.randn(1, 1, M, C, generator=g)).to(F64)
    da = _data((1, 1, M, C), g, ints, -2, 2)
    gam = (_ints((C,), 1, 2, g) * torch.tensor([1.0, -1.0])[torch.randint(0, 2, (C,), generator=g)]).to(F64)
    bet = _data((C,), g, ints, -1, 1).to(F64)
    bet = torch.where(bet == 0, torch.ones_like(bet), bet)       # (M = 1: z = beta exactly; keep it off the ReLU's kink)
    eps = 1e-5
    yr, gr, br = y.clone().requires_grad_(True), gam.clone().requires_grad_(True), bet.clone().requires_grad_(True)
    mean, var = yr.mean((0, 1, 2)), yr.var((0, 1, 2), unbiased=False)
    xh = (yr - mean) / torch.sqrt(var + eps)
    torch.relu(xh * gr + br).backward(da.to(F64))
    # the kernels' inputs: tx = (mean, gamma * rstd, beta - mean * gamma * rstd, 0) and rstd, here in float64
    rstd = 1.0 / torch.sqrt(var.detach() + eps)
    tx = torch.stack([mean.detach(), gam * rstd, bet - mean.detach() * gam * rstd, torch.zeros(C, dtype=F64)], 1)
    s, q, sa, qa = R.bn_bwd_reduce(da, y, tx, rstd)
    tol = 1e-12 * max(1.0, da.abs().sum().item())
    assert (s - br.grad).abs().max().item() <= tol and (q - gr.grad).abs().max().item() <= tol * max(1.0, xh.abs().max().item())
    assert (sa >= s.abs() * (1 - 1e-12)).all() and (qa >= q.abs() * (1 - 1e-12)).all()
    dz, mag = R.bn_bwd_apply(da, y, tx, rstd, s, q, M)
    assert (dz - yr.grad).abs().max().item() <= 1e-11 * max(1.0, mag.max().item())
    assert (mag >= dz.abs() * (1 - 1e-12)).all()
    # count != M: the sums are divided by the count that is passed
    dz2, _ = R.bn_bwd_apply(da, y, tx, rstd, 2 * s, 2 * q, 2 * M)
    assert (dz2 - dz).abs().max().item() <= 1e-12 * max(1.0, mag.max().item())
    if ints:                                    # the sums themselves, term by term, on integer statistics
        tx_i = torch.tensor([[1.0, 1.0, -1.0, 0.0], [0.0, -1.0, 1.0, 0.0], [-1.0, 2.0, 1.0, float("-inf")]])[:C]
        if C <= 3:
            z = y * tx_i[:, 1].to(F64) + tx_i[:, 2].to(F64)
            dzi = torch.where(z > tx_i[:, 3].to(F64), da.to(F64), torch.zeros((), dtype=F64))
            xi = (y - tx_i[:, 0].to(F64)) * 2.0
            si, qi, sai, qai = R.bn_bwd_reduce(da, y, tx_i, torch.full((C,), 2.0))
            assert torch.equal(si, dzi.sum((0, 1, 2))) and torch.equal(qi, (dzi * xi).sum((0, 1, 2)))
            assert torch.equal(sai, dzi.abs().sum((0, 1, 2))) and torch.equal(qai, (dzi * xi).abs().sum((0, 1, 2)))


@pytest.mark.parametrize("ints", [True, False])
def test_colsum_and_materialize(ints):
    g = _gen(11, ints)
    x = _data((2, 5, 7, 9), g, ints)[..., 1:7]
    s, m = R.colsum(x, 0.25)
    _same(s, 0.25 * x.to(F64).sum((0, 1, 2)), ints)
    _same(m, 0.25 * x.to(F64).abs().sum((0, 1, 2)), ints)
    t = _tx_of(6, g, ints)
    _same(R.materialize_nchw(x, t), _nchw(_act(x, t)).contiguous(), True)
    _same(R.materialize_nchw(x, None), _nchw(x.to(F64)).contiguous(), True)


def test_gamma():
    assert R.gamma(1) == R.U / (1 - R.U) and R.gamma(100) > 100 * R.U
