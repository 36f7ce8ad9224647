"""tests/nonfinite_ref.py against torch.nn.functional (float64, CPU) on inputs with planted NaN / +Inf / -Inf, its comparison
helper against hand-made disagreements, and the premise of the whole exercise: with a NaN-dropping max in place of torch.relu /
F.max_pool2d a small network's loss stays FINITE on an input that makes torch's loss NaN.  No GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import nonfinite_ref as R

F64 = torch.float64
BAR = 1e-12                                    # float64 against float64: both sides round at 2^-53 on O(1..10) values
PLACES = ("first", "last", "interior", "channel", "image")


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _cases():
    return [(p, v) for p in PLACES for v in R.VALUES]


def _x(shape, seed, place, value, **kw):
    x = (torch.randn(shape, generator=_g(seed), dtype=F64) * 2 + 0.5)
    return x if place is None else R.plant(x, R.positions(shape, **kw)[place], value)


def _affine(C, seed):
    g = _g(seed)
    gamma = 0.5 + torch.rand(C, generator=g, dtype=F64)
    gamma[::7] = -gamma[::7]
    return gamma, 0.1 * torch.randn(C, generator=g, dtype=F64)


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def test_positions_and_plant():
    shape = (2, 5, 7, 6)
    pos = R.positions(shape)
    x = torch.zeros(shape)
    assert int(torch.isnan(R.plant(x, pos["first"], "nan")).sum()) == 1 and math.isnan(R.plant(x, pos["first"], "nan")[0, 0, 0, 0])
    assert R.plant(x, pos["last"], "+inf")[1, 4, 6, 5] == R.INF
    assert R.plant(x, pos["interior"], "-inf")[1, 2, 3, 3] == -R.INF
    ch = R.plant(x, pos["channel"], "nan")
    assert bool(torch.isnan(ch[..., 3]).all()) and int(torch.isnan(ch).sum()) == 2 * 5 * 7
    im = R.plant(x, pos["image"], "+inf")
    assert bool(torch.isinf(im[1]).all()) and not bool(torch.isinf(im[0]).any())
    assert not bool(torch.isnan(x).any())                                     # plant copies
    with pytest.raises(TypeError):
        R.plant(torch.zeros(3, dtype=torch.int64), (0,), "nan")               # labels / indices are never planted


def test_assert_same_nonfinite_accepts_and_rejects():
    want = torch.tensor([1.0, R.NAN, R.INF, -R.INF, 2.0], dtype=F64)
    R.assert_same_nonfinite(want.clone(), want, 0.0)
    R.assert_same_nonfinite(want + torch.tensor([1e-3, 0, 0, 0, -1e-3], dtype=F64), want, 1.1e-3)
    for bad in ([1.0, 0.0, R.INF, -R.INF, 2.0],          # a NaN swallowed
                [R.NAN, R.NAN, R.INF, -R.INF, 2.0],      # a NaN invented
                [1.0, R.NAN, 65504.0, -R.INF, 2.0],      # +Inf saturated
                [1.0, R.NAN, R.INF, R.INF, 2.0],         # the sign of an Inf
                [1.0, R.NAN, R.INF, -R.INF, R.INF],      # an Inf where a finite value belongs
                [1.0, R.NAN, R.INF, -R.INF, 2.1]):       # past the bar
        with pytest.raises(AssertionError):
            R.assert_same_nonfinite(torch.tensor(bad, dtype=F64), want, 1e-3)
    assert R.finite_scale(want) == 2.0


# ---- references against torch.nn.functional ------------------------------------------------------------------------------------
@pytest.mark.parametrize("place,value", [(None, None)] + _cases())
def test_bn_relu_train(place, value):
    shape = (2, 9, 13, 16)
    x = _x(shape, 1, place, value)
    gamma, beta = _affine(16, 2)
    rm0, rv0 = 0.2 * torch.randn(16, generator=_g(3), dtype=F64), 0.5 + torch.rand(16, generator=_g(4), dtype=F64)
    rm, rv = rm0.clone(), rv0.clone()
    want = _nhwc(F.relu(F.batch_norm(_nchw(x), rm, rv, gamma, beta, True, 0.1, 1e-5)))
    got, grm, grv = R.bn_relu_train(x, gamma, beta, 1e-5, True, 0.1, rm0, rv0)
    R.assert_same_nonfinite(got, want, BAR, "y")
    R.assert_same_nonfinite(grm, rm, BAR, "running_mean")
    R.assert_same_nonfinite(grv, rv, BAR, "running_var")
    if place in ("first", "last", "interior"):                  # the contract: that channel NaN everywhere, the others as before
        c = R.positions(shape)[place][-1]
        clean = R.bn_relu_train(_x(shape, 1, None, None), gamma, beta, 1e-5)[0]
        others = [k for k in range(16) if k != c]
        assert bool(torch.isnan(got[..., c]).all()) and torch.equal(got[..., others], clean[..., others])
        # running_var is NaN; running_mean is NaN for a NaN and +-Inf for an Inf (0.9 * old + 0.1 * (+-Inf)), as in torch
        assert bool(torch.isnan(grv[c])) and int(torch.isnan(grv).sum()) == 1
        assert int((~torch.isfinite(grm)).sum()) == 1
        assert bool(torch.isnan(grm[c])) if value == "nan" else float(grm[c]) == R.VALUES[value]


@pytest.mark.parametrize("place,value", [(None, None)] + _cases())
def test_bn_relu_eval(place, value):
    shape = (2, 5, 6, 8)
    x = _x(shape, 5, place, value)
    gamma, beta = _affine(8, 6)
    rm, rv = 0.2 * torch.randn(8, generator=_g(7), dtype=F64), 0.5 + torch.rand(8, generator=_g(8), dtype=F64)
    want = _nhwc(F.relu(F.batch_norm(_nchw(x), rm, rv, gamma, beta, False, 0.1, 1e-5)))
    got = R.bn_relu_eval(x, gamma, beta, rm, rv, 1e-5)
    R.assert_same_nonfinite(got, want, BAR)
    if place in ("first", "last", "interior") and value == "nan":
        assert int(torch.isnan(got).sum()) == 1                 # per element: one NaN in, one NaN out


@pytest.mark.parametrize("hw", [(6, 8), (7, 9), (9, 13), (2, 3)])
@pytest.mark.parametrize("place,value", [(None, None)] + _cases())
def test_max_pool2(hw, place, value):
    shape = (2,) + hw + (4,)
    x = _x(shape, 9, place, value)
    R.assert_same_nonfinite(R.max_pool2(x), _nhwc(F.max_pool2d(_nchw(x), 2)), 0.0)


def test_max_pool2_windows():
    x = torch.zeros(1, 4, 4, 1, dtype=F64)
    x[0, 0, 1, 0] = R.NAN                                        # one NaN among finite values
    x[0, 0:2, 2:4, 0] = R.NAN                                    # four NaNs
    x[0, 2, 0, 0] = R.INF                                        # +Inf among finite values
    x[0, 2:4, 2:4, 0] = -R.INF                                   # four -Inf
    y = R.max_pool2(x)[0, :, :, 0]
    assert math.isnan(y[0, 0]) and math.isnan(y[0, 1]) and y[1, 0] == R.INF and y[1, 1] == -R.INF
    R.assert_same_nonfinite(R.max_pool2(x), _nhwc(F.max_pool2d(_nchw(x), 2)), 0.0)


@pytest.mark.parametrize("place,value", [(None, None)] + _cases())
def test_max_pool3s2(place, value):
    x = _x((2, 9, 11, 4), 10, place, value)
    R.assert_same_nonfinite(R.max_pool3s2(x), _nhwc(F.max_pool2d(_nchw(x), 3, 2, 0)), 0.0)


@pytest.mark.parametrize("relu_on,with_res", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("place,value", [(None, None)] + _cases())
def test_group_norm(relu_on, with_res, place, value):
    shape, G = (2, 5, 7, 16), 4
    x = _x(shape, 11, place, value)
    res = torch.randn(shape, generator=_g(12), dtype=F64) if with_res else None
    gamma, beta = _affine(16, 13)
    want = F.group_norm(_nchw(x), G, gamma, beta, 1e-6)
    if with_res:
        want = want + _nchw(res)
    want = _nhwc(F.relu(want) if relu_on else want)
    got = R.group_norm(x, G, gamma, beta, 1e-6, res, relu_on)
    R.assert_same_nonfinite(got, want, BAR)
    if place == "interior":                                      # that (image, group) NaN, every other group as before
        n, c = R.positions(shape)[place][0], R.positions(shape)[place][-1]
        nan = torch.isnan(got)
        cg = 16 // G
        assert bool(nan[n, :, :, c // cg * cg:(c // cg + 1) * cg].all()) and int(nan.sum()) == 5 * 7 * cg


def test_group_norm_nan_in_res_only():
    shape = (2, 5, 7, 16)
    x, res = _x(shape, 14, None, None), R.plant(torch.randn(shape, generator=_g(15), dtype=F64), (1, 2, 3, 5), "nan")
    gamma, beta = _affine(16, 16)
    got = R.group_norm(x, 4, gamma, beta, 1e-6, res, True)
    R.assert_same_nonfinite(got, _nhwc(F.relu(F.group_norm(_nchw(x), 4, gamma, beta, 1e-6) + _nchw(res))), BAR)
    assert int(torch.isnan(got).sum()) == 1 and math.isnan(got[1, 2, 3, 5])


@pytest.mark.parametrize("place,value", [(None, None)] + _cases())
def test_layer_norm_and_gelu(place, value):
    shape = (2, 1, 11, 24)
    x = _x(shape, 17, place, value)
    gamma, beta = _affine(24, 18)
    R.assert_same_nonfinite(R.layer_norm(x, gamma, beta, 1e-6), F.layer_norm(x, (24,), gamma, beta, 1e-6), BAR)
    # F.gelu(-inf) is 0 * -inf = NaN in torch's own arithmetic too: the reference is the same expression
    R.assert_same_nonfinite(R.gelu(x), F.gelu(x), BAR)


@pytest.mark.parametrize("place,value", [(None, None)] + _cases())
def test_add2_relu(place, value):
    shape = (2, 3, 5, 12)
    a, b = _x(shape, 19, place, value), _x(shape, 20, None, None)
    t = torch.zeros(12, 4, dtype=F64)
    t[:, 1], t[:, 2], t[:, 3] = 0.5 + torch.rand(12, generator=_g(21), dtype=F64), 0.3, -R.INF
    for fa, fb, ta, tb in ((a, b, t, None), (b, a, None, t), (a, a, t, t)):
        want = F.relu((fa if ta is None else fa * t[:, 1] + t[:, 2]) + (fb if tb is None else fb * t[:, 1] + t[:, 2]))
        R.assert_same_nonfinite(R.add2_relu(fa, ta, fb, tb), want, BAR)


@pytest.mark.parametrize("which", ["q", "k", "v"])
@pytest.mark.parametrize("value", list(R.VALUES))
def test_attention(which, value):
    B, N, heads, D = 2, 13, 2, 8
    g = _g(22)
    q, k, v = (torch.randn(B, 1, N, heads * D, generator=g, dtype=F64) for _ in range(3))
    planted = dict(q=q, k=k, v=v)
    planted[which] = R.plant(planted[which], (1, 0, 5, 9), value)          # image 1, token 5, head 1
    q, k, v = planted["q"], planted["k"], planted["v"]
    sp = lambda t: t.reshape(B, N, heads, D).permute(0, 2, 1, 3)
    want = F.scaled_dot_product_attention(sp(q), sp(k), sp(v)).permute(0, 2, 1, 3).reshape(B, 1, N, heads * D)
    got = R.attention(q, k, v, heads)
    R.assert_same_nonfinite(got, want, BAR)
    assert not bool(torch.isnan(got[0]).any()) and not bool(torch.isnan(got[1, 0, :, :D]).any())   # other image / head untouched
    if which == "q" and value == "nan":
        assert bool(torch.isnan(got[1, 0, 5, D:]).all()) and int(torch.isnan(got).sum()) == D      # that query's row only


@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("value", [None] + list(R.VALUES))
def test_dice_bce_mc(C, value):
    g = _g(23)
    x = torch.randn(2, C, 9, 7, generator=g, dtype=F64)
    lab = torch.randint(0, C, (2, 9, 7), generator=g)
    if value is not None:
        x = R.plant(x, (1, C - 1, 4, 3), value)
    xr = x.clone().requires_grad_(True)
    p = torch.softmax(xr, 1)
    dice = sum(1 - (2 * (p[:, c] * (lab == c)).sum() + 1e-5) / ((p[:, c] ** 2).sum() + (lab == c).sum() + 1e-5) for c in range(C))
    want = 0.5 * F.cross_entropy(xr, lab) + 0.5 * dice / C
    want.backward()
    loss, grad = R.dice_bce_mc_with_grad(x, lab, C)
    R.assert_same_nonfinite(loss, want.detach(), BAR, "loss")
    R.assert_same_nonfinite(grad, xr.grad, BAR, "dlogits")
    if value in ("nan", "+inf"):                                 # (-inf is an ordinary logit: probability 0)
        assert math.isnan(float(loss)) and bool(torch.isnan(grad).all())     # the global Dice sums carry it to every pixel


# ---- the premise -----------------------------------------------------------------------------------------------------------------
def _rehearsal(plant):
    g = _g(24)
    x = torch.randn(2, 1, 16, 16, generator=g, dtype=F64)
    lab = torch.randint(0, 2, (2, 16, 16), generator=g)
    C = 8
    ws = [torch.randn(C, 1, 3, 3, generator=g, dtype=F64) * (2 / 9) ** 0.5,
          torch.randn(C, C, 3, 3, generator=g, dtype=F64) * (2 / (9 * C)) ** 0.5,
          torch.randn(2, C, 1, 1, generator=g, dtype=F64) * (2 / C) ** 0.5]
    if plant == "nan_pixel":
        x = R.plant(x, (1, 0, 7, 9), "nan")
    elif plant == "inf_pixel":
        x = R.plant(x, (1, 0, 7, 9), "+inf")
    elif plant == "inf_weight_channel":
        ws[1] = R.plant(ws[1], (3,), "+inf")
    torch_loss = R.rehearsal_loss(x, lab, ws, torch.relu, lambda t: F.max_pool2d(t, 2))
    dropping = R.rehearsal_loss(x, lab, ws, R.nan_dropping_relu, R.nan_dropping_pool2)
    return float(torch_loss), float(dropping)


def test_premise_nan_dropping_max_hides_what_torch_reports():
    """Recorded premise: clamps and maxima that return their non-NaN operand (fmaxf, `f > m ? f : m`) turn a channel whose
    BatchNorm statistics are NaN into exact zeros, and the loss stays finite where torch.relu / F.max_pool2d give NaN."""
    clean_t, clean_d = _rehearsal(None)
    assert math.isfinite(clean_t) and clean_t == clean_d          # on finite data the two forms are the same function
    for plant in ("nan_pixel", "inf_pixel", "inf_weight_channel"):
        t, d = _rehearsal(plant)
        assert math.isnan(t), (plant, t)
        assert math.isfinite(d) and 0.0 < d < 2.0, (plant, d)


# ---- the fp16 overflow plant -------------------------------------------------------------------------------------------------------
def test_overflow_power_is_the_smallest_and_leaves_the_rest_small():
    from oracle import recipe, ref_unet
    key = "down1.maxpool_conv.1.double_conv.0.weight"

    def make():
        ref = ref_unet.RefUNet(1, 2, 8, False)
        ref.load_state_dict(recipe.fill_state_dict(ref.state_dict(), seed=70))
        return ref.double().train()
    x = recipe.synthetic_batch(2, 1, 32, 32, 2, seed=70)[0].double()
    k = R.overflow_power(ref_unet, make, x, key)
    assert 8 <= k <= 20                                            # O(1..30) activations to 2^17
    assert ref_unet.F is F                                        # the recorder is gone again
    pre0, rest0 = R.oracle_forward_maxima(ref_unet, make(), x, key, 3)
    assert 2.0 ** 17 / 2 ** k < pre0 * 2 <= 2 * 2.0 ** 17 / 2 ** (k - 1) and rest0 < 2.0 ** 14
    with pytest.raises(AssertionError):                           # a bound nothing can meet is reported, not waved through
        R.overflow_power(ref_unet, make, x, key, below=1e-3)


def test_no_power_of_two_overflows_a_standardised_convolution():
    """Why the TransUNet cases carry no overflow plant: its ResNet convolutions standardise their weights per output channel, so
    a power of two on a channel of the stored weight leaves the forward where it was."""
    from oracle import recipe, ref_transunet
    key = "transformer.embeddings.hybrid_model.body.block2.unit1.conv1.weight"
    ref = ref_transunet.RefTransUNet(ref_transunet.small_config(2), 64)
    ref.load_state_dict(recipe.fill_state_dict(ref.state_dict(), seed=70, negative_gamma=False))
    ref = ref.double().train()
    x = recipe.synthetic_batch(2, 1, 64, 64, 2, seed=70)[0].double()
    with torch.no_grad():
        base = ref(x)
        for k in (8, 17, 40):
            w = dict(ref.named_parameters())[key]
            keep = w[3].clone()
            w[3] *= 2.0 ** k
            out = ref(x)
            w[3] = keep
            # (the eps of the standardisation is the only thing that does not scale: 1e-5 against a variance of O(1e-2))
            assert float((out - base).abs().max()) <= 1e-2 * float(base.abs().max()), k
            assert float(out.abs().max()) < 2.0 ** 14
