"""The two narrow ends of TransUNet (csrc/narrow_convs.hip) at the shapes the R50-ViT-B/16 models run, and past every edge
of their schedules:
  * root  : ResNetV2's StdConv2d(3, 64, kernel 7, stride 2, pad 3), forward and weight gradient (`root_fwd_kernel`,
            `root_wgrad_kernel`): several passes of the 128-column loop, a ragged last pass, ragged row blocks, the dynamic LDS
            up to its 64-KiB edge (W = 656) and the first width past it (W = 657: the generic kernel);
  * head3 : SegmentationHead Conv2d(C, n_classes, kernel 3, pad 1), fp32 logits + bias with the producer's transform on load
            (`head3x3_fwd_kernel`: the grid-stride loop above 16,384 workgroups) and its weight gradient (`head3x3_wgrad_kernel`:
            one partial row per 2,048 pixels, workgroups that straddle images);
  * the head's data gradient, which runs on `stem3x3_fwd_kernel` with Ci = n_classes and 16 / 8 output channels (runs of 8 / 4
    pixels per thread, also with rows shorter than a run).
Section 1 uses small-integer operands: every product and partial sum is exact in fp16 / fp32 in any order, so the kernels must
equal torch's fp32 convolution / autograd on the CPU bit for bit (each test asserts that premise on the reference).  Section 2
adds one random-data case per forward kernel against float64, elementwise, with a derived bound.  Every output, split
workspace and the unused columns of strided buffers are prefilled with NaN; every case proves from the profiler's kernel
names which kernel ran.  `test_model_calls_are_covered` records every convolution call with at most 4 channels on one side
that the models make at 224 x 224 and 512 x 512 and requires each to appear in the tables, batch aside."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_exact import _apply, _gpu, _int_tx, _ints
from tests.test_gpu_exact_fullsize import _nan, _nan_ws
from tests.test_gpu_tu_fullsize import SUB16, U16, U32, _check, _kernels

pytestmark = pytest.mark.gpu
DEV = "cuda"
CO_ROOT = 64

# ---- the tables --------------------------------------------------------------------------------------------------------
# root: (N, H, W), passes of the 128-column loop, dynamic LDS bytes of the forward (None: past the edge, generic kernel)
ROOT_CASES = [
    ((2, 224, 224), 1, 47376),      # production 224: Wo = 112
    ((1, 512, 512), 2, 59472),      # production 512: Wo = 256, two full passes
    ((2, 37, 261), 2, 48930),       # Wo = 131: the second pass holds 3 pixels; Ho = 19 is ragged for blocks of 4 and of 8 rows
    ((1, 9, 656), 3, 65520),        # the widest accepted width; Wo = 328: three passes, the last ragged; Ho = 5
    ((1, 9, 657), 3, None),         # one past: must not run root_fwd_kernel
]
ROOT_STRIDED = (2, 37, 261)         # again with y / dy as 64-channel slices of 128-wide buffers
# head3: (N, H, W, C, n_classes), sweeps of the forward's grid-stride loop, partial rows of the weight gradient
HEAD_CASES = [
    ((2, 224, 224, 16, 2), 1, 49),        # production 224
    ((1, 512, 512, 16, 2), 1, 128),       # production 512, one image
    ((9, 509, 515, 16, 2), 2, 1152),      # P = 2,359,215 > 2,097,152: a second, partly filled sweep; boundaries inside wavefronts
    ((1, 725, 727, 64, 3), 2, 258),       # 8 lanes per pixel: P = 527,075 is just over that width's sweep of 524,288
    ((3, 37, 41, 16, 4), 1, 3),           # three weight-gradient workgroups; the image boundary (pixel 1,517) inside the first
    ((2, 21, 19, 32, 1), 1, 1),           # one class, 4 lanes per pixel
]
HEAD_STRIDED = (3, 37, 41, 16, 4)   # again with x as a 16-channel slice of a 32-wide NaN-padded buffer
# head data gradient on the stem kernel: (N, H, W, n_classes, Co), pixels per thread
DGRAD_CASES = [
    ((2, 224, 224, 2, 16), 8),            # production 224
    ((1, 512, 512, 2, 16), 8),            # production 512 (two classes, as the models are built)
    ((1, 512, 512, 4, 16), 8),
    ((2, 9, 5, 3, 16), 8),                # W = 5 < 8: a thread's run wraps more than one row
    ((1, 13, 3, 2, 8), 4),                # one lane per pixel, W = 3 < 4
]
# section 2 (random data against float64)
ROOT_RANDOM = (1, 224, 224)
HEAD_RANDOM = (2, 224, 224, 16, 2)


def _ids(cases):
    return ["x".join(map(str, c[0])) for c in cases]


def _wgrad_ref(a, dy, R, stride, pad):
    """Sum over images of conv2d's weight gradient ([Co, Ci, R, R] float64; each image's fp32 sums are exact integers)."""
    out = None
    for n in range(a.shape[0]):
        gw = torch.nn.grad.conv2d_weight(a[n].permute(2, 0, 1)[None], (dy.shape[3], a.shape[3], R, R),
                                         dy[n].permute(2, 0, 1)[None], stride, pad).double()
        out = gw if out is None else out + gw
    return out


def _fwd_pack(ops, wd):
    return lambda lay: ops.pack_conv_fwd(wd, torch.float16, k8=bool(lay))


# ========================================================================================================================
# 1a. Root: forward + weight gradient, exact
# ========================================================================================================================
def _root_exact(shape, passes, lds, strided):
    lib, ops = _gpu()
    N, H, W = shape
    Co = CO_ROOT
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert (Wo + 127) // 128 == passes, "premise: passes of the column loop"
    assert lds == (37632 + 42 * (W + 8) if W <= 656 else None) and (lds is None or lds <= 65536)
    g = torch.Generator().manual_seed(N * 1000003 + H * 1009 + W)
    x = _ints((N, H, W, 3), -2, 2, g)
    w = _ints((Co, 3, 7, 7), -1, 1, g)
    dy = _ints((N, Ho, Wo, Co), -1, 1, g)
    xd = torch.empty(N, H, W, 3, dtype=torch.float16, device=DEV)        # NHWC with ldx = 3, as Tape.input_nchw makes it
    xd.copy_(x)
    wd = w.to(DEV)
    wide = 2 * Co if strided else Co
    ybuf = _nan(N, Ho, Wo, wide)
    y = ybuf[..., wide - Co:]
    dybuf = _nan(N, Ho, Wo, wide)
    dyd = dybuf[..., wide - Co:]
    dyd.copy_(dy)
    gw = _nan(Co, 3, 7, 7, dtype=torch.float32)
    scale = 0.25
    nb = lib.fn("umi_conv_wgrad_ws_bytes")(N, Ho, Wo, 3, Co, 7, 7, lib.UMI_F16, 0)

    def run():
        ops.conv_fwd(xd, None, _fwd_pack(ops, wd), None, y, 7, 7, 2, 3)
        ops.conv_wgrad(xd, None, dyd, None, gw, 3 * 49, 49, 1, scale, 7, 7, 2, 3)
    names = _kernels(run)
    assert ("root_fwd_kernel" in names) == (lds is not None), "premise: the root forward runs up to W = 656 and not past it"
    assert "conv_generic_kernel" in names or lds is not None, "premise: the generic kernel past the edge"
    assert "root_wgrad_kernel" in names, "premise: the root weight-gradient kernel"
    ybuf.fill_(float("nan"))
    gw.fill_(float("nan"))
    _nan_ws(nb)
    run()
    torch.cuda.synchronize()
    # sum |x dy| over all pixels: every fp32 partial sum of the weight gradient is an exact integer
    assert N * Ho * Wo * x.abs().max().item() * dy.abs().max().item() < 2 ** 24
    got = y.float().cpu()
    for n in range(N):
        ref = F.conv2d(x[n].permute(2, 0, 1)[None], w, None, 2, 3)[0].permute(1, 2, 0)
        assert ref.abs().max().item() < 2048               # every output is an fp16 integer
        assert torch.equal(got[n], ref), n
    if strided:
        assert torch.isnan(ybuf[..., :wide - Co]).all(), "the other 64 columns are not the kernel's"
    assert torch.equal(gw.cpu().double(), _wgrad_ref(x, dy, 7, 2, 3) * scale)


@pytest.mark.parametrize("shape,passes,lds", ROOT_CASES, ids=_ids(ROOT_CASES))
def test_root_forward_and_weight_gradient_exact(shape, passes, lds):
    _root_exact(shape, passes, lds, False)


def test_root_exact_on_channel_slices():
    shape, passes, lds = next(c for c in ROOT_CASES if c[0] == ROOT_STRIDED)
    _root_exact(shape, passes, lds, True)


# ========================================================================================================================
# 1b. Segmentation head: forward (fp32 logits + bias, transform on load) + weight gradient, exact
# ========================================================================================================================
def _head_exact(shape, sweeps, rows, strided):
    lib, ops = _gpu()
    N, H, W, C, NC = shape
    P, G = N * H * W, C // 8
    per_sweep = 16384 * 256 // G                             # pixels one sweep of the capped grid covers
    assert (P + per_sweep - 1) // per_sweep == sweeps and (P + 2047) // 2048 == rows, "premise: the schedule this case reaches"
    g = torch.Generator().manual_seed(N * 1000003 + H * 1009 + W + C + NC)
    x = _ints((N, H, W, C), -2, 2, g)
    t = _int_tx(C, g)
    w = _ints((NC, C, 3, 3), -2, 2, g)
    b = _ints((NC,), -3, 3, g)
    dl = _ints((N, H, W, NC), -1, 1, g)
    a = _apply(x, t)
    amax = a.abs().max().item()
    assert amax <= 5
    # sum |terms| of a logit, and of a weight gradient over all pixels: every fp32 partial sum is an exact integer
    assert 9 * C * amax * w.abs().max().item() + b.abs().max().item() < 2 ** 24
    assert P * amax * dl.abs().max().item() < 2 ** 24
    if strided:
        xbuf = _nan(N, H, W, 2 * C)
        xd = xbuf[..., C // 2:C // 2 + C]
        xd.copy_(x)
    else:
        xd = x.half().to(DEV)
    del x
    td, wd, bd, dld = t.to(DEV), w.to(DEV), b.to(DEV), dl.half().to(DEV)
    logits = _nan(N, H, W, NC, dtype=torch.float32)
    gw = _nan(NC, C, 3, 3, dtype=torch.float32)
    scale = 0.5
    nb = lib.fn("umi_conv_wgrad_ws_bytes")(N, H, W, C, NC, 3, 3, lib.UMI_F16, 0)

    def run():
        ops.conv_fwd(xd, td, _fwd_pack(ops, wd), bd, logits, 3, 3, 1, 1)
        ops.conv_wgrad(xd, td, dld, None, gw, C * 9, 9, 1, scale, 3, 3, 1, 1)
    names = _kernels(run)
    assert "head3x3_fwd_kernel" in names and "head3x3_wgrad_kernel" in names, "premise: the narrow head kernels"
    logits.fill_(float("nan"))
    gw.fill_(float("nan"))
    _nan_ws(nb)
    run()
    torch.cuda.synchronize()
    got = logits.cpu()
    assert not torch.isnan(got).any(), "unwritten logits"
    for n in range(N):
        ref = F.conv2d(a[n].permute(2, 0, 1)[None], w, b, 1, 1)[0].permute(1, 2, 0)
        assert torch.equal(got[n], ref), n
    assert torch.equal(gw.cpu().double(), _wgrad_ref(a, dl, 3, 1, 1) * scale)


@pytest.mark.parametrize("shape,sweeps,rows", HEAD_CASES, ids=_ids(HEAD_CASES))
def test_head_forward_and_weight_gradient_exact(shape, sweeps, rows):
    _head_exact(shape, sweeps, rows, False)


def test_head_exact_on_channel_slice():
    shape, sweeps, rows = next(c for c in HEAD_CASES if c[0] == HEAD_STRIDED)
    _head_exact(shape, sweeps, rows, True)


# ========================================================================================================================
# 1c. The head's data gradient on the stem kernel (Ci = n_classes, 16 / 8 output channels), exact
# ========================================================================================================================
@pytest.mark.parametrize("shape,run_len", DGRAD_CASES, ids=_ids(DGRAD_CASES))
def test_head_data_gradient_on_stem_kernel_exact(shape, run_len):
    lib, ops = _gpu()
    N, H, W, NC, Co = shape
    assert 1024 // (256 // (Co // 8)) == run_len, "premise: pixels per thread"
    g = torch.Generator().manual_seed(N * 1000003 + H * 1009 + W + NC + Co)
    w = _ints((NC, Co, 3, 3), -2, 2, g)                      # the head's weight: Co input channels -> NC classes
    dl = _ints((N, H, W, NC), -1, 1, g)
    wd, dld = w.to(DEV), dl.half().to(DEV)
    dx = _nan(N, H, W, Co)
    run = lambda: ops.conv_fwd(dld, None, lambda lay: ops.pack_conv_dgrad(wd, torch.float16, k8=bool(lay)), None, dx, 3, 3, 1, 1)
    names = _kernels(run)
    assert "stem3x3_fwd_kernel" in names, "premise: the stem kernel serves the head's data gradient"
    dx.fill_(float("nan"))
    run()
    torch.cuda.synchronize()
    got = dx.float().cpu()
    for n in range(N):
        ref = F.conv_transpose2d(dl[n].permute(2, 0, 1)[None], w, None, 1, 1)[0].permute(1, 2, 0)
        assert ref.abs().max().item() < 2048                 # every output is an fp16 integer
        assert torch.equal(got[n], ref), n


# ========================================================================================================================
# 2. Random data against float64, elementwise: |y - ref| <= (a |ref| + b s) u + floor with s = sum |x||w| (+ |bias|).
#    Both kernels are fp32 fmaf chains over exact products of fp16 values, so b = the chain's length n at u = 2^-24.
# ========================================================================================================================
def test_root_forward_random_against_float64():
    """n = 7 * 7 * 3 = 147 fmaf; the fp16 store adds a = 1 at 2^-11 (written as a = 2^13 at u = 2^-24) and half the fp16
    subnormal spacing.  Measured b 0.96, bound 147."""
    lib, ops = _gpu()
    N, H, W = ROOT_RANDOM
    Co = CO_ROOT
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = torch.Generator().manual_seed(147)
    x = torch.randn(N, H, W, 3, generator=g).half()
    w = (torch.randn(Co, 3, 7, 7, generator=g) * 0.1).half().float()
    xd = torch.empty(N, H, W, 3, dtype=torch.float16, device=DEV)
    xd.copy_(x)
    y = _nan(N, Ho, Wo, Co)
    run = lambda: ops.conv_fwd(xd, None, _fwd_pack(ops, w.to(DEV)), None, y, 7, 7, 2, 3)
    assert "root_fwd_kernel" in _kernels(run)
    y.fill_(float("nan"))
    run()
    x64, w64 = x.double().permute(0, 3, 1, 2), w.double()
    ref = F.conv2d(x64, w64, None, 2, 3).permute(0, 2, 3, 1)
    s = F.conv2d(x64.abs(), w64.abs(), None, 2, 3).permute(0, 2, 3, 1)
    _check("root fwd", y.cpu(), ref, s, U16 / U32, 147, U32, SUB16)


def test_head_forward_random_against_float64():
    """Real-valued scale / shift rows and bias.  n = 9 C + log2(C / 8) + 3 (the transform's fmaf, the products' chain, the
    shuffle adds across the C / 8 lanes of a pixel, the bias) = 148 at C = 16; fp32 output, so a = 0 and no floor.  Measured
    b 2.7, bound 148."""
    lib, ops = _gpu()
    N, H, W, C, NC = HEAD_RANDOM
    g = torch.Generator().manual_seed(148)
    x = torch.randn(N, H, W, C, generator=g).half()
    t = torch.stack([torch.zeros(C), torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3, torch.zeros(C)],
                    1).contiguous()
    w = (torch.randn(NC, C, 3, 3, generator=g) * 0.2).half().float()
    b = torch.randn(NC, generator=g)
    y = _nan(N, H, W, NC, dtype=torch.float32)
    xd, td, bd = x.to(DEV), t.to(DEV), b.to(DEV)
    run = lambda: ops.conv_fwd(xd, td, _fwd_pack(ops, w.to(DEV)), bd, y, 3, 3, 1, 1)
    assert "head3x3_fwd_kernel" in _kernels(run)
    y.fill_(float("nan"))
    run()
    t64 = t.double()
    a64 = torch.maximum(x.double() * t64[:, 1] + t64[:, 2], t64[:, 3]).permute(0, 3, 1, 2)
    ref = F.conv2d(a64, w.double(), b.double(), 1, 1).permute(0, 2, 3, 1)
    s = F.conv2d(a64.abs(), w.double().abs(), b.double().abs(), 1, 1).permute(0, 2, 3, 1)
    n = 9 * C + (C // 8).bit_length() - 1 + 3
    assert n == 148
    _check("head fwd", y.cpu(), ref, s, 0, n, U32)


# ========================================================================================================================
# 3. The tables above cover every narrow convolution call the models make (batch aside)
# ========================================================================================================================
def _dtn(t):
    return {torch.float16: "f16", torch.float32: "f32"}[t.dtype]


def _table_keys():
    """(kind, H, W, Ci, Co, R, stride, pad, ldx, ldy, transform, bias, output dtype) of every row of sections 1 - 2."""
    keys = set()
    for (N, H, W), _, _ in ROOT_CASES + [(ROOT_RANDOM, 0, 0)]:
        keys.add(("fwd", H, W, 3, CO_ROOT, 7, 2, 3, 3, CO_ROOT, False, False, "f16"))
    for (N, H, W), _, _ in ROOT_CASES:
        keys.add(("wgrad", H, W, 3, CO_ROOT, 7, 2, 3, 3, CO_ROOT, False, False, "f32"))
    N, H, W = ROOT_STRIDED
    keys.add(("fwd", H, W, 3, CO_ROOT, 7, 2, 3, 3, 2 * CO_ROOT, False, False, "f16"))
    keys.add(("wgrad", H, W, 3, CO_ROOT, 7, 2, 3, 3, 2 * CO_ROOT, False, False, "f32"))
    for (N, H, W, C, NC), _, _ in HEAD_CASES + [(HEAD_RANDOM, 0, 0)]:
        keys.add(("fwd", H, W, C, NC, 3, 1, 1, C, NC, True, True, "f32"))
    for (N, H, W, C, NC), _, _ in HEAD_CASES:
        keys.add(("wgrad", H, W, C, NC, 3, 1, 1, C, NC, True, False, "f32"))
    N, H, W, C, NC = HEAD_STRIDED
    keys.add(("fwd", H, W, C, NC, 3, 1, 1, 2 * C, NC, True, True, "f32"))
    keys.add(("wgrad", H, W, C, NC, 3, 1, 1, 2 * C, NC, True, False, "f32"))
    for (N, H, W, NC, Co), _ in DGRAD_CASES:
        keys.add(("fwd", H, W, NC, Co, 3, 1, 1, NC, Co, False, False, "f16"))
    return keys


@pytest.mark.parametrize("img", [224, 512])
def test_model_calls_are_covered(img, monkeypatch):
    lib, ops = _gpu()
    import loss as L
    from oracle import recipe, ref_transunet
    from TransUnet.vit_seg_modeling import VisionTransformer
    from tests.test_gpu_transunet import product_config
    seen = set()
    fwd0, wgrad0 = ops.conv_fwd, ops.conv_wgrad

    def fwd(x, tx, wp, bias, y, R, S, stride, pad, *a, **k):
        if min(x.shape[3], y.shape[3]) <= 4:
            seen.add(("fwd", x.shape[1], x.shape[2], x.shape[3], y.shape[3], R, stride, pad, ops._nhwc(x)[4], ops._nhwc(y)[4],
                      tx is not None, bias is not None, _dtn(y)))
        return fwd0(x, tx, wp, bias, y, R, S, stride, pad, *a, **k)

    def wgrad(x, txa, dy, txb, dW, s_co, s_ci, s_t, out_scale, R, S, stride, pad, *a, **k):
        if min(x.shape[3], dy.shape[3]) <= 4:
            assert txb is None
            seen.add(("wgrad", x.shape[1], x.shape[2], x.shape[3], dy.shape[3], R, stride, pad, ops._nhwc(x)[4],
                      ops._nhwc(dy)[4], txa is not None, False, _dtn(dW)))
        return wgrad0(x, txa, dy, txb, dW, s_co, s_ci, s_t, out_scale, R, S, stride, pad, *a, **k)

    monkeypatch.setattr(ops, "conv_fwd", fwd)
    monkeypatch.setattr(ops, "conv_wgrad", wgrad)
    cfg = ref_transunet.r50_vit_b16_config(2, 3, dropout_rate=0.0)
    L.CLASS_NUMBER = 2
    torch.manual_seed(0)
    m = VisionTransformer(product_config(cfg, img), img_size=img, num_classes=2, compute_dtype="fp16").to(DEV).train()
    x, lab = recipe.synthetic_batch(1, 1, img, img, 2, seed=1)
    L.calc_loss(m(x.to(DEV)), lab.to(DEV), loss_type="dice_bce_mc").backward()
    torch.cuda.synchronize()

    assert any(k[0] == "fwd" and k[5] == 7 for k in seen), sorted(seen)                                   # the root
    assert any(k[0] == "fwd" and k[5] == 3 and k[4] <= 4 and k[12] == "f32" for k in seen), sorted(seen)  # the head
    assert any(k[0] == "fwd" and k[5] == 3 and k[3] <= 4 and k[4] == 16 for k in seen), sorted(seen)      # its data gradient
    allowed = _table_keys()
    missing = sorted(k for k in seen if k not in allowed)
    assert not missing, f"narrow convolution calls of the model that the tables do not pin: {missing}"
