"""What the training step's kernels owe a NaN or an Inf in their floating-point input: torch's result.

Float64 references built from plain torch tensor arithmetic on the CPU (sums, products, torch.relu, torch.amax: IEEE semantics,
NaN-propagating), in the kernels' calling convention -- NHWC activations `[N, H, W, C]`, per-channel parameters `[C]`, the
consumer transform `tx` = rows (mean, scale, shift, lo).  tests/test_nonfinite_ref.py pins them against torch.nn.functional on
planted inputs; tests/test_gpu_nonfinite.py holds the kernels to them.

The contract ("Non-finite values in the training step"):
  * training-mode BatchNorm: one NaN or +-Inf in a channel makes the batch statistics of that channel NaN, and with them every
    element of the channel and its running statistics; other channels are untouched;
  * GroupNorm: the same per (image, group); LayerNorm: per row;
  * ReLU keeps NaN (torch.relu), +Inf stays +Inf, -Inf becomes 0;
  * MaxPool: a window holding a NaN gives NaN; otherwise the maximum (+Inf wins, four -Inf give -Inf);
  * softmax attention, GELU and the dice_bce_mc loss propagate by their arithmetic.
Eval-mode BatchNorm (finite running statistics, one NaN element) is stated here too (`bn_relu_eval`) but NOT yet met by the
kernels' clamp: see DESIGN.md, "left out on purpose".

Values are only ever planted in floating-point DATA (`plant` refuses anything else): never in labels, indices, sizes, strides."""
import math

import torch

F64 = torch.float64
NAN, INF = float("nan"), float("inf")
VALUES = {"nan": NAN, "+inf": INF, "-inf": -INF}


# ---- planting ---------------------------------------------------------------------------------------------------------------
def positions(shape, channel=None, image=None):
    """name -> index (a tuple for Tensor.__setitem__) into an NHWC (or any >= 2-D, channels-last) tensor of `shape`: the first
    element, the last one, one interior element, a whole channel and a whole image."""
    nd = len(shape)
    c = shape[-1] // 2 if channel is None else channel
    n = shape[0] - 1 if image is None else image
    return {
        "first": (0,) * nd,
        "last": tuple(s - 1 for s in shape),
        "interior": tuple(s // 2 for s in shape[:-1]) + (c,),
        "channel": (Ellipsis, c),
        "image": (n,),
    }


def plant(t, where, value):
    """A copy of the floating-point tensor `t` with `value` (a float or a key of VALUES) at index `where`."""
    if not t.is_floating_point():
        raise TypeError("non-finite values are planted in floating-point data only, got " + str(t.dtype))
    v = VALUES[value] if isinstance(value, str) else float(value)
    out = t.clone()
    out[where] = v
    return out


# ---- the comparison ---------------------------------------------------------------------------------------------------------
def assert_same_nonfinite(got, want, bar, what=""):
    """isnan(got) == isnan(want) element-wise; got == want wherever want is +-Inf; finite entries within `bar` (absolute: the
    caller passes the bar of the kernel's existing float64 test, e.g. tol * max |finite want|)."""
    got, want = got.detach().to(F64).cpu(), want.detach().to(F64).cpu()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    gn, wn = torch.isnan(got), torch.isnan(want)
    if not torch.equal(gn, wn):
        bad = (gn != wn).nonzero()
        i = tuple(int(k) for k in bad[0])
        raise AssertionError(f"{what}: NaN pattern differs at {len(bad)} of {got.numel()} elements, first {i}: "
                             f"got {got[i].item()!r}, want {want[i].item()!r}")
    wi = torch.isinf(want)
    if bool(wi.any()):
        ne = (got[wi] != want[wi])
        assert not bool(ne.any()), f"{what}: {int(ne.sum())} of {int(wi.sum())} infinite entries differ: got {got[wi][ne][:4]}"
    fin = ~(wn | wi)
    if bool(fin.any()):
        err = (got[fin] - want[fin]).abs()                      # (an Inf in `got` where `want` is finite gives err = inf)
        worst = err.max().item()
        assert worst <= bar, f"{what}: finite entries differ by {worst!r} > bar {bar!r}"


def finite_scale(want):
    """max |finite entries of want| (0 for none): the scale the relative bars of the existing tests multiply."""
    w = want.detach().to(F64)
    w = w[torch.isfinite(w)]
    return float(w.abs().max()) if w.numel() else 0.0


# ---- references -------------------------------------------------------------------------------------------------------------
def relu(v):
    return torch.relu(v)


def apply_scale_shift(x, tx):
    """v * scale + shift of the transform rows, float64, WITHOUT the clamp (`lo` is how the kernels express the ReLU; the
    reference applies torch.relu where lo == 0)."""
    t = tx.to(F64)
    return x.to(F64) * t[:, 1] + t[:, 2]


def bn_stats(x):
    """(mean, biased variance, count) per channel of an NHWC tensor, float64."""
    x = x.to(F64)
    dims = tuple(range(x.dim() - 1))
    count = x.numel() // x.shape[-1]
    mean = x.sum(dims) / count
    var = ((x - mean) ** 2).sum(dims) / count
    return mean, var, count


def bn_relu_train(x, gamma, beta, eps, relu_on=True, momentum=0.1, running_mean=None, running_var=None):
    """Training-mode BatchNorm (+ ReLU) of NHWC `x`: (y, new running_mean, new running_var) -- the running statistics only when
    given (new = (1 - momentum) * old + momentum * batch statistic, the variance unbiased, as nn.BatchNorm2d)."""
    mean, var, count = bn_stats(x)
    y = (x.to(F64) - mean) / torch.sqrt(var + eps) * gamma.to(F64) + beta.to(F64)
    if relu_on:
        y = relu(y)
    rm = rv = None
    if running_mean is not None:
        rm = (1 - momentum) * running_mean.to(F64) + momentum * mean
        unb = var * count / (count - 1) if count > 1 else var
        rv = (1 - momentum) * running_var.to(F64) + momentum * unb
    return y, rm, rv


def bn_relu_eval(x, gamma, beta, running_mean, running_var, eps, relu_on=True):
    """Eval-mode BatchNorm (+ ReLU): per element, so one NaN element stays one NaN element."""
    y = (x.to(F64) - running_mean.to(F64)) / torch.sqrt(running_var.to(F64) + eps) * gamma.to(F64) + beta.to(F64)
    return relu(y) if relu_on else y


def max_pool2(x):
    """MaxPool2d(2) of NHWC `x` (odd H / W: the last row / column is dropped): NaN if the window holds one."""
    N, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    w = x.to(F64)[:, :2 * Ho, :2 * Wo].reshape(N, Ho, 2, Wo, 2, C)
    return torch.amax(w, dim=(2, 4))


def max_pool3s2(x):
    """MaxPool2d(3, stride 2, padding 0) of NHWC `x`."""
    N, H, W, C = x.shape
    w = x.to(F64).unfold(1, 3, 2).unfold(2, 3, 2)               # [N, Ho, Wo, C, 3, 3]
    return torch.amax(w, dim=(4, 5))


def group_norm(x, groups, gamma, beta, eps, res=None, relu_on=False):
    """[relu](GroupNorm(x) [+ res]) of NHWC `x`; statistics per (image, group of C / groups consecutive channels)."""
    N, H, W, C = x.shape
    g = x.to(F64).reshape(N, H * W, groups, C // groups)
    mean = g.mean(dim=(1, 3), keepdim=True)
    var = ((g - mean) ** 2).mean(dim=(1, 3), keepdim=True)
    y = ((g - mean) / torch.sqrt(var + eps)).reshape(N, H, W, C) * gamma.to(F64) + beta.to(F64)
    if res is not None:
        y = y + res.to(F64)
    return relu(y) if relu_on else y


def layer_norm(x, gamma, beta, eps):
    """LayerNorm over the last dimension."""
    x = x.to(F64)
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * gamma.to(F64) + beta.to(F64)


def add2_relu(a, txa, b, txb):
    """relu(a' + b'), a' = a * scale_a + shift_a (tx None: as stored): the attention gate's E."""
    fa = a.to(F64) if txa is None else apply_scale_shift(a, txa)
    fb = b.to(F64) if txb is None else apply_scale_shift(b, txb)
    return relu(fa + fb)


def gelu(x):
    """Exact GELU (F.gelu's default)."""
    x = x.to(F64)
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def attention(q, k, v, heads):
    """softmax(Q K^T / sqrt(D)) V per head; q, k, v: [B, 1, N, heads * D] as the kernels take them."""
    B, _, N, C = q.shape
    D = C // heads
    sp = lambda t: t.to(F64).reshape(B, N, heads, D).permute(0, 2, 1, 3)
    s = sp(q) @ sp(k).transpose(-1, -2) / math.sqrt(D)
    s = s - s.amax(-1, keepdim=True)                            # (amax propagates NaN: the row is NaN either way)
    e = torch.exp(s)
    p = e / e.sum(-1, keepdim=True)
    return (p @ sp(v)).permute(0, 2, 1, 3).reshape(B, 1, N, C)


def dice_bce_mc(logits, labels, n_classes, eps=1e-5):
    """'dice_bce_mc': 0.5 * cross entropy + 0.5 * mean_c (1 - (2 A_c + eps) / (B_c + T_c + eps)) with the sums over batch and
    pixels.  logits [N, C, H, W] (float64 in, differentiable), labels [N, H, W] class indices (never planted)."""
    t = labels.long()
    x = logits.to(F64)
    ls = x - torch.logsumexp(x, dim=1, keepdim=True)
    ce = -ls.gather(1, t.unsqueeze(1)).mean()
    p = torch.exp(ls)
    dice = 0.0
    for c in range(n_classes):
        tc = (t == c).to(F64)
        dice = dice + 1.0 - (2.0 * (p[:, c] * tc).sum() + eps) / ((p[:, c] * p[:, c]).sum() + tc.sum() + eps)
    return 0.5 * ce + 0.5 * dice / n_classes


def dice_bce_mc_with_grad(logits, labels, n_classes):
    """(loss, d loss / d logits) in float64."""
    x = logits.detach().to(F64).clone().requires_grad_(True)
    loss = dice_bce_mc(x, labels, n_classes)
    loss.backward()
    return loss.detach(), x.grad


# ---- the rehearsal: a small Conv-BN-ReLU-pool network whose ReLU and max can be chosen ------------------------------------------
def nan_dropping_relu(v):
    """max(v, 0) as fmaxf evaluates it: the non-NaN operand."""
    return torch.fmax(v, torch.zeros_like(v))


def nan_dropping_pool2(x_nchw):
    """`m = f > m ? f : m` from -inf over the four taps: a NaN never wins."""
    m = torch.full_like(x_nchw[..., ::2, ::2], -INF)
    for dh in (0, 1):
        for dw in (0, 1):
            m = torch.fmax(m, x_nchw[..., dh::2, dw::2])
    return m


def rehearsal_loss(x, labels, weights, relu_fn, pool_fn):
    """Two Conv3x3-BatchNorm(batch statistics)-ReLU-MaxPool(2) blocks and a 1x1 head in float64, then dice_bce_mc.
    x [N, 1, H, W] with H, W multiples of 4; weights = (w1 [C, 1, 3, 3], w2 [C, C, 3, 3], w3 [K, C, 1, 1])."""
    import torch.nn.functional as Fn
    h = x.to(F64)
    for w in weights[:2]:
        h = Fn.conv2d(h, w.to(F64), None, 1, 1)
        mean = h.mean(dim=(0, 2, 3), keepdim=True)
        var = ((h - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
        h = pool_fn(relu_fn((h - mean) / torch.sqrt(var + 1e-5)))
    logits = Fn.conv2d(h, weights[2].to(F64))
    lab = labels[:, ::4, ::4]
    return dice_bce_mc(logits, lab, weights[2].shape[0])


# ---- the fp16 overflow plant: a power of two chosen on the float64 oracle --------------------------------------------------------
class _Recorder:
    """Stands in for `torch.nn.functional` inside an oracle module: every call goes through, and the largest magnitude of every
    tensor it returns is recorded.  The output of the convolution whose weight IS `target` is recorded without channel
    `channel`, whose own maximum goes to `pre`."""

    def __init__(self, real, target, channel):
        self.real, self.target, self.channel, self.seen, self.pre = real, target, channel, [], None

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def call(*a, **k):
            out = fn(*a, **k)
            if torch.is_tensor(out) and out.is_floating_point():
                o = out.detach()
                if name == "conv2d" and len(a) > 1 and a[1] is self.target:
                    assert self.pre is None, "the planted convolution ran twice"
                    self.pre = float(o[:, self.channel].abs().max())
                    o = o.clone()
                    o[:, self.channel] = 0
                self.seen.append((name, float(o.abs().max())))
            return out
        return call


def oracle_forward_maxima(oracle_module, ref, x, weight_key, channel):
    """One training-mode forward of the float64 oracle `ref` (a class of `oracle_module`, e.g. oracle.ref_unet) on `x`:
    (max |pre-normalisation output channel `channel`| of the convolution holding `weight_key`, max |anything else|), where
    "anything else" is the input and every tensor a torch.nn.functional call of the forward returns."""
    target = dict(ref.named_parameters())[weight_key]
    rec = _Recorder(oracle_module.F, target, channel)
    oracle_module.F = rec
    try:
        with torch.no_grad():
            ref(x)
    finally:
        oracle_module.F = rec.real
    assert rec.pre is not None, "the forward never ran the convolution of " + weight_key
    return rec.pre, max([float(x.abs().max())] + [m for _, m in rec.seen])


def overflow_power(oracle_module, make_ref, x, weight_key, channel=3, above=2.0 ** 17, below=2.0 ** 14):
    """The smallest k such that multiplying output channel `channel` of `weight_key` by 2^k puts the oracle's pre-normalisation
    maximum of that channel above `above`; both conditions of the plant are ASSERTED on a forward with the scaled weight: that
    maximum is above `above` and every other tensor of the forward stays below `below`.  make_ref() -> a fresh float64 oracle
    in training mode.  The convolution is linear in its weight, so k follows from the unscaled maximum."""
    pre0, _ = oracle_forward_maxima(oracle_module, make_ref(), x, weight_key, channel)
    assert pre0 > 0 and math.isfinite(pre0)
    k = math.floor(math.log2(above / pre0)) + 1
    ref = make_ref()
    with torch.no_grad():
        dict(ref.named_parameters())[weight_key][channel] *= 2.0 ** k
    pre, rest = oracle_forward_maxima(oracle_module, ref, x, weight_key, channel)
    assert pre > above and pre / 2 <= above, f"2^{k} is not the smallest power: the channel's maximum is {pre}"
    assert rest < below, f"another tensor of the oracle's forward reaches {rest} >= {below}"
    return k
