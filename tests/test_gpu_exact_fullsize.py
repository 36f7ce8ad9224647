"""Exact-arithmetic parity of the matrix-core kernels at the benchmark's own geometry (512 x 512 maps, B = 2 and 16).

tests/test_gpu_exact.py pins every kernel bit for bit on small maps (at most 20 x 64 pixels).  The schedules that only large
maps reach are pinned here with the same construction (small-integer operands: every product and partial sum is exact in
fp16 / fp32 in any order, so the kernels must match the reference exactly):
  * the XCD-aware work order of conv_mfma.hip (`xcd_chunk` = nblk / 8 > 1, with and without a remainder);
  * the per-pixel-tile statistics rows of the forward (EPI 1) and of the data gradient's fused BatchNorm reduction (EPI 2),
    compared row by row, then through the 2-D finalize reduction;
  * the weight-gradient split-K plans at bench sizes (many tiles per split, splits straddling images, a short last split);
  * the ConvTranspose trio at dec3.up, max-pool with its fused reduction, stem and head at 2 x 512 x 512.
Every GPU output and partial-row buffer is filled with NaN before its launch, so a tile that is never written fails.
The CPU reference runs one image at a time (host memory stays bounded).  Two child-process tests run the whole network at
512 x 512 against the oracle and a graph-replayed B = 16 training step against eager, both under UMI_TRACE_GENERIC=1."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_exact import _apply, _gpu, _int_tx, _ints

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# N, H, W, Ci, Co of the forward conv
SHAPES = [
    (2, 512, 512, 64, 64),        # enc0.c2 / dec3.c2
    (2, 512, 512, 128, 64),       # dec3.c1
    (2, 256, 256, 64, 128),       # enc1.c1
    (2, 256, 256, 128, 128),      # enc1.c2 / dec2.c2
    (2, 128, 128, 128, 256),      # two channel blocks: xcd_chunk = 32
    (1, 40, 70, 128, 256),        # xcd_chunk = 3, remainder 6 (ragged tiles)
]


def _nan(*shape, dtype=torch.float16):
    return torch.full(shape, NAN, device=DEV, dtype=dtype)


def _nan_ws(nbytes):
    """The grow-only split-K workspace with every byte 0xFF (an fp32 NaN): a slab that is never written poisons the result."""
    from umi import ops
    ws = ops.workspace(nbytes, torch.device(DEV, torch.cuda.current_device()))     # the key ops uses: x.device
    ws[:max(int(nbytes), 1)].fill_(255)


def _tiles(th, H, W):
    return (H + th - 1) // th, (W + 31) // 32


def _th(rows, N, H, W, Co):
    """TH of the pixel tiles, derived from umi_conv_fwd_plan's row count (and checked against the kernel's choice)."""
    tw = (W + 31) // 32
    th = [t for t in (8, 16) if N * tw * ((H + t - 1) // t) == rows]
    assert th, (rows, N, H, W)
    assert th[0] == (16 if Co % 128 else 8), (th, Co)
    return th[0]


def _tile_sums(v, th):
    """[H, W, C] float64 -> [tiles_y * tiles_x, C] sums over each TH x 32 pixel tile (rows in pt order)."""
    H, W, C = v.shape
    ty, tx = _tiles(th, H, W)
    p = torch.zeros(ty * th, tx * 32, C, dtype=torch.float64)
    p[:H, :W] = v
    return p.view(ty, th, tx, 32, C).sum((1, 3)).reshape(ty * tx, C)


def _check_rows(part, rows, C, a_rows, b_rows):
    """GPU partial rows [rows][2][C] against reference rows, bit for bit (each reference row is an exact fp32 integer sum)."""
    got = part.view(rows, 2, C).cpu()
    want = torch.stack([a_rows, b_rows], 1)
    assert want.abs().max().item() < 2 ** 24
    assert torch.equal(got.double(), want), (got.double() - want).abs().amax((0, 2))


def _conv_fwd(lib, ops, x, tx, w, y, stats):
    """umi_conv_fwd (3x3, stride 1, pad 1) with a NaN-filled partial-row buffer; asserts the matrix-core path."""
    N, H, W, Ci, ldx = ops._nhwc(x)
    _, _, _, Co, ldy = ops._nhwc(y)
    lay, rows = ops.conv_plan(x, y, 3, 3, 1, 1)
    assert lay == 1
    wp = ops.pack_conv_fwd(w, torch.float16, k8=True)
    part = _nan(rows * 2 * Co, dtype=torch.float32) if stats else None
    lib.check(lib.fn("umi_conv_fwd")(x.data_ptr(), ldx, ops._ptr(tx), wp.data_ptr(), None, y.data_ptr(), ldy, ops._ptr(part),
                                     N, H, W, Ci, Co, 3, 3, 1, 1, H, W, 0, 0, H, W, lib.UMI_F16, lib.UMI_F16, 0, ops._stream()),
              "umi_conv_fwd")
    return part, rows


def _fwd_exact(x_img, t, w, y, part, rows, N, H, W, Co):
    """Compare y and the statistics rows against the CPU conv, one image at a time; returns float64 (sum, sum of squares)."""
    th = _th(rows, N, H, W, Co)
    per = rows // N
    s1 = torch.zeros(Co, dtype=torch.float64)
    s2 = torch.zeros(Co, dtype=torch.float64)
    for n in range(N):
        a = x_img(n)
        if t is not None:
            a = _apply(a, t)
        ref = F.conv2d(a.permute(2, 0, 1)[None], w, None, 1, 1)[0].permute(1, 2, 0).contiguous()
        assert ref.abs().max().item() < 2048                      # every output is an fp16 integer
        assert torch.equal(y[n].float().cpu(), ref), n
        if part is not None:
            r = ref.double()
            ra, rb = _tile_sums(r.abs(), th), _tile_sums(r * r, th)
            assert ra.max().item() < 2 ** 24 and rb.max().item() < 2 ** 24     # every partial sum of a row is exact in fp32
            _check_rows(part[n * per * 2 * Co:(n + 1) * per * 2 * Co], per, Co, _tile_sums(r, th), rb)
            s1 += r.sum((0, 1))
            s2 += (r * r).sum((0, 1))
    return s1, s2


def _check_finalize(ops, part, Co, count, s1, s2):
    """The GPU rows through umi_bn_finalize against float64 statistics (tolerances of test_bn_finalize_row_reduction_forms)."""
    gamma, beta = torch.ones(Co), torch.zeros(Co)
    rm, rv = torch.zeros(Co, device=DEV), torch.ones(Co, device=DEV)
    tx, rs = ops.bn_finalize(part, Co, float(count), gamma.to(DEV), beta.to(DEV), 1e-5, 0.1, rm, rv)
    tx, rs = tx.cpu(), rs.cpu()
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    assert (tx[:, 0].double() - mean).abs().max().item() < 1e-6 * max(1.0, mean.abs().max().item())
    assert (tx[:, 1].double() - rstd).abs().max().item() < 2e-6 * rstd.abs().max().item()
    assert (tx[:, 2].double() + mean * rstd).abs().max().item() < 1e-5 * max(1.0, (mean * rstd).abs().max().item())
    assert (rs.double() - rstd).abs().max().item() < 2e-6 * rstd.abs().max().item()
    assert (rv.cpu().double() - (0.9 + 0.1 * var * count / (count - 1))).abs().max().item() < 1e-5 * max(1.0, var.max().item())


def _xcd_chunk(N, H, W, Co):
    """(xcd_chunk, ids left in order) of conv_mfma.hip's launch(): tiles of TH x 32 pixels x BN channels, nblk / 8 when n_co > 1."""
    th, bn = (8, 128) if Co % 128 == 0 else (16, 64)
    n_co = (Co + bn - 1) // bn
    nblk = N * ((W + 31) // 32) * ((H + th - 1) // th) * n_co
    return (nblk // 8 if n_co > 1 else 0), nblk % 8


@pytest.mark.parametrize("case", SHAPES)
def test_conv3x3_forward_and_stat_rows_exact_at_bench_size(case):
    """EPI 1 at full size: output with torch.equal, the statistics row of every pixel tile against that tile's sums, then the
    rows through the 2-D finalize reduction."""
    lib, ops = _gpu()
    N, H, W, Ci, Co = case
    if Co == 256:                               # the XCD permutation is non-trivial here (it is the identity for chunk <= 1)
        assert _xcd_chunk(N, H, W, Co) in ((32, 0), (3, 6))
    g = torch.Generator().manual_seed(sum(case) + 1)
    x = _ints((N, H, W, Ci), -1, 1, g)
    w = _ints((Co, Ci, 3, 3), -1, 1, g)
    t = _int_tx(Ci, g) if (Ci, Co) != (128, 128) else None     # 128 -> 128: the form without a transform on load
    xd = x.half().to(DEV)
    y = _nan(N, H, W, Co)
    part, rows = _conv_fwd(lib, ops, xd, t.to(DEV) if t is not None else None, w.to(DEV), y, True)
    torch.cuda.synchronize()
    s1, s2 = _fwd_exact(lambda n: x[n], t, w, y, part, rows, N, H, W, Co)
    _check_finalize(ops, part, Co, N * H * W, s1, s2)


def test_conv3x3_forward_exact_on_b16_concat_buffer():
    """dec3.c1 at the benchmark's batch: B = 16, a 128-channel view of a [16, 512, 512, 128] concat buffer (1 GiB), 8,192
    statistics rows."""
    lib, ops = _gpu()
    N, H, W, Ci, Co = 16, 512, 512, 128, 64
    gd = torch.Generator(device=DEV).manual_seed(16)
    buf = torch.randint(-1, 2, (N, H, W, Ci), generator=gd, device=DEV, dtype=torch.int8).half()
    xd = buf[..., :Ci]
    g = torch.Generator().manual_seed(17)
    w = _ints((Co, Ci, 3, 3), -1, 1, g)
    t = _int_tx(Ci, g)
    y = _nan(N, H, W, Co)
    part, rows = _conv_fwd(lib, ops, xd, t.to(DEV), w.to(DEV), y, True)
    assert rows == 8192
    torch.cuda.synchronize()
    s1, s2 = _fwd_exact(lambda n: xd[n].float().cpu(), t, w, y, part, rows, N, H, W, Co)
    _check_finalize(ops, part, Co, N * H * W, s1, s2)


def _bn_rows(C, g):
    """BatchNorm transform rows {mean, scale, shift, lo = 0} and rstd with dyadic effect: integer mean / shift, scale and rstd
    in {0.5, 1, 2}, so the ReLU mask, xhat and dz * xhat are exact."""
    t = torch.zeros(C, 4)
    t[:, 0] = _ints((C,), -1, 1, g)
    t[:, 1] = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)]
    t[:, 2] = _ints((C,), -1, 1, g)
    rstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)]
    return t, rstd


# the last two: data gradients with 256 output channels, i.e. under the non-trivial XCD permutation (chunk 32; chunk 3 + 6)
@pytest.mark.parametrize("case", SHAPES + [(2, 128, 128, 256, 128), (1, 40, 70, 256, 128)])
def test_conv3x3_dgrad_and_fused_bn_rows_exact_at_bench_size(case):
    """The data gradient (Co -> Ci channels) with the fused stage 1 of the BatchNorm backward (EPI 2): gradient bit for bit,
    and the sum dz / sum dz*xhat row of every pixel tile; the plain data gradient writes the same gradient."""
    lib, ops = _gpu()
    N, H, W, Ci, Co = case
    if Ci == 256:
        assert _xcd_chunk(N, H, W, Ci) in ((32, 0), (3, 6))
    g = torch.Generator().manual_seed(sum(case) + 2)
    w = _ints((Co, Ci, 3, 3), -1, 1, g)
    dy = _ints((N, H, W, Co), -1, 1, g)
    ybn = _ints((N, H, W, Ci), -2, 2, g)
    t, rstd = _bn_rows(Ci, g)
    dyd, ybd, wd = dy.half().to(DEV), ybn.half().to(DEV), w.to(DEV)
    td, rsd = t.to(DEV).contiguous(), rstd.to(DEV)
    lay, rows = ops.conv_plan(dyd, ybd, 3, 3, 1, 1)
    assert lay == 1
    th = _th(rows, N, H, W, Ci)
    wp = ops.pack_conv_dgrad(wd, torch.float16, k8=True)
    da = _nan(N, H, W, Ci)
    part = _nan(rows * 2 * Ci, dtype=torch.float32)
    lib.check(lib.fn("umi_conv_dgrad_bnred")(dyd.data_ptr(), Co, wp.data_ptr(), da.data_ptr(), Ci, ybd.data_ptr(), Ci,
                                             td.data_ptr(), rsd.data_ptr(), part.data_ptr(), N, H, W, Co, Ci, lib.UMI_F16,
                                             ops._stream()), "umi_conv_dgrad_bnred")
    da2 = _nan(N, H, W, Ci)
    ops.conv_fwd(dyd, None, lambda l: wp, None, da2, 3, 3, 1, 1)
    torch.cuda.synchronize()
    assert torch.equal(da, da2)
    per = rows // N
    for n in range(N):
        ref = F.conv_transpose2d(dy[n].permute(2, 0, 1)[None], w, None, 1, 1)[0].permute(1, 2, 0).contiguous()
        assert ref.abs().max().item() < 2048
        assert torch.equal(da[n].float().cpu(), ref), n
        yb = ybn[n].double()
        dz = ref.double() * ((yb * t[:, 1].double() + t[:, 2].double()) > 0)
        dzx = dz * (yb - t[:, 0].double()) * rstd.double()
        ra = _tile_sums(dz.abs(), th)
        rb = _tile_sums(dzx.abs(), th)
        assert ra.max().item() < 2 ** 21 and rb.max().item() < 2 ** 21       # multiples of 1/4: exact in fp32 in any order
        _check_rows(part[n * per * 2 * Ci:(n + 1) * per * 2 * Ci], per, Ci, _tile_sums(dz, th), _tile_sums(dzx, th))


def test_conv3x3_inference_epilogue_exact_at_bench_size():
    """EPI 3: this layer's BatchNorm (integer scale / shift) + ReLU applied to the fp32 accumulators on store."""
    lib, ops = _gpu()
    N, H, W, Ci, Co = 2, 512, 512, 64, 64
    g = torch.Generator().manual_seed(3)
    x = _ints((N, H, W, Ci), -1, 1, g)
    w = _ints((Co, Ci, 3, 3), -1, 1, g)
    t = _int_tx(Ci, g)
    ot = _int_tx(Co, g)
    y = _nan(N, H, W, Co)
    wp = ops.pack_conv_fwd(w.to(DEV), torch.float16, k8=True)
    assert ops.conv3x3_fwd_act(x.half().to(DEV), t.to(DEV), wp, ot.to(DEV), y)
    torch.cuda.synchronize()
    for n in range(N):
        ref = F.conv2d(_apply(x[n], t).permute(2, 0, 1)[None], w, None, 1, 1)[0].permute(1, 2, 0)
        assert ref.abs().max().item() < 2048
        assert torch.equal(y[n].float().cpu(), _apply(ref, ot)), n


def _wgrad_ref(a, dy, R, pad):
    """sum over images of the conv2d weight gradient (float64 accumulation of exact per-image float32 integer sums)."""
    out = None
    for n in range(a.shape[0]):
        gw = torch.nn.grad.conv2d_weight(a[n].permute(2, 0, 1)[None], (dy.shape[3], a.shape[3], R, R),
                                         dy[n].permute(2, 0, 1)[None], 1, pad).double()
        out = gw if out is None else out + gw
    return out


@pytest.mark.parametrize("case", SHAPES[:4] + [(3, 132, 96, 64, 64)])
def test_conv3x3_weight_gradient_exact_at_bench_size(case):
    """Weight gradient with its split-K slabs at the bench's plans (16 tiles per split at 2 x 512^2 x 64 -> 64); the last case
    has 2 tiles per split over 297 tiles: splits straddle two images and the last split is one tile long."""
    lib, ops = _gpu()
    N, H, W, Ci, Co = case
    g = torch.Generator().manual_seed(sum(case) + 4)
    x = _ints((N, H, W, Ci), -1, 1, g)
    dy = _ints((N, H, W, Co), -1, 1, g)
    t = _int_tx(Ci, g)
    a = _apply(x, t)
    assert N * H * W * a.abs().max().item() < 2 ** 24                 # every partial sum is an exact fp32 integer
    ref = _wgrad_ref(a, dy, 3, 1) * 0.5
    gw = _nan(Co, Ci, 3, 3, dtype=torch.float32)
    _nan_ws(lib.fn("umi_conv_wgrad_ws_bytes")(N, H, W, Ci, Co, 3, 3, lib.UMI_F16, 0))
    ops.conv_wgrad(x.half().to(DEV), t.to(DEV), dy.half().to(DEV), None, gw, Ci * 9, 9, 1, 0.5, 3, 3, 1, 1)
    assert torch.equal(gw.cpu().double(), ref)


def test_wgrad_bn_apply_exact_at_bench_size():
    """umi_conv_wgrad_bnapply at 2 x 512^2, 64 -> 64: dz (stage 3 of the BatchNorm backward, formed while staging) and the weight
    gradient are bit-identical to umi_bn_bwd_apply + umi_conv_wgrad, and both equal the float64 reference exactly (c1, c2,
    xhat, gamma * rstd are dyadic: dz is a multiple of 1/4)."""
    lib, ops = _gpu()
    N, H, W, Ci, Co = 2, 512, 512, 64, 64
    M = N * H * W
    g = torch.Generator().manual_seed(5)
    x = _ints((N, H, W, Ci), -1, 1, g)
    txa = torch.zeros(Ci, 4)
    txa[:, 1] = torch.tensor([1.0, -1.0])[torch.randint(0, 2, (Ci,), generator=g)]
    da = _ints((N, H, W, Co), -1, 1, g)
    y = _ints((N, H, W, Co), -1, 1, g)
    tb = torch.zeros(Co, 4)
    tb[:, 1] = torch.tensor([0.5, 1.0])[torch.randint(0, 2, (Co,), generator=g)]
    tb[:, 2] = _ints((Co,), -1, 1, g)
    rstd = torch.tensor([1.0, 2.0])[torch.randint(0, 2, (Co,), generator=g)]
    c1 = _ints((Co,), -1, 1, g)
    c2 = torch.tensor([0.0, 0.5])[torch.randint(0, 2, (Co,), generator=g)]
    sums = torch.stack([c1 * M, c2 * M])                 # M = 2^19: c = sum / M is exact
    a = _apply(x, txa)
    dz = tb[:, 1] * ((y * tb[:, 1] + tb[:, 2] > 0).float() * da - c1 - (y - tb[:, 0]) * rstd * c2)
    assert dz.abs().max().item() <= 4 and torch.equal(dz * 4, (dz * 4).round())
    assert M * a.abs().max().item() * dz.abs().max().item() * 4 < 2 ** 24
    ref = _wgrad_ref(a, dz, 3, 1) * 0.5
    xd, dad, yd = x.half().to(DEV), da.half().to(DEV), y.half().to(DEV)
    txd, tbd, rsd, sd = txa.to(DEV), tb.to(DEV).contiguous(), rstd.to(DEV), sums.to(DEV)
    dz_f = _nan(N, H, W, Co)
    gw_f = _nan(Co, Ci, 3, 3, dtype=torch.float32)
    nb = lib.fn("umi_conv_wgrad_ws_bytes")(N, H, W, Ci, Co, 3, 3, lib.UMI_F16, 0)
    _nan_ws(nb)
    assert ops.conv_wgrad_bnapply(xd, txd, dad, yd, tbd, rsd, sd[0], sd[1], dz_f, gw_f, Ci * 9, 9, 1, 0.5, 3, 3, 1, 1)
    dz_s = dad.clone()
    ops.bn_bwd_apply(dz_s, yd, tbd, rsd, sd[0], sd[1])
    gw_s = _nan(Co, Ci, 3, 3, dtype=torch.float32)
    _nan_ws(nb)
    ops.conv_wgrad(xd, txd, dz_s, None, gw_s, Ci * 9, 9, 1, 0.5, 3, 3, 1, 1)
    torch.cuda.synchronize()
    assert torch.equal(dz_f, dz_s) and torch.equal(gw_f, gw_s)
    assert torch.equal(dz_f.float().cpu(), dz)
    assert torch.equal(gw_f.cpu().double(), ref)


def test_conv_transpose_trio_exact_at_dec3_up():
    """ConvTranspose2d(128 -> 64, 2, 2) at dec3.up (2 x 256^2 -> 512^2): forward scattered into the upper half of a 512^2
    concat buffer (the lower half stays untouched), data gradient from a concat-buffer slice, weight + bias gradient."""
    lib, ops = _gpu()
    N, h, w, Cin, Cout = 2, 256, 256, 128, 64
    g = torch.Generator().manual_seed(6)
    x = _ints((N, h, w, Cin), -1, 1, g)
    wt = _ints((Cin, Cout, 2, 2), -1, 1, g)
    b = _ints((Cout,), -3, 3, g)
    t = _int_tx(Cin, g)
    a = _apply(x, t)
    wd, xd, td = wt.to(DEV), x.half().to(DEV), t.to(DEV)
    buf = _nan(N, 2 * h, 2 * w, 2 * Cout)
    dest = buf[..., Cout:]
    assert ops.conv_plan(xd, dest, 2, 2, 2, 0, lib.CONV_UPSAMPLE2)[0] == 1
    ops.conv_fwd(xd, td, lambda l: ops.pack_convT_fwd(wd, torch.float16, k8=bool(l)), b.to(DEV), dest, 2, 2, 2, 0,
                 flags=lib.CONV_UPSAMPLE2, up_offset=(0, 0))
    dupb = torch.randint(-1, 2, (N, 2 * h, 2 * w, 2 * Cout), generator=torch.Generator(device=DEV).manual_seed(6), device=DEV,
                         dtype=torch.int8).half()
    dupd = dupb[..., Cout:]
    dx = _nan(N, h, w, Cin)
    assert ops.conv_plan(dupd, dx, 2, 2, 2, 0, 0)[0] == 1
    ops.conv_fwd(dupd, None, lambda l: ops.pack_convT_dgrad(wd, torch.float16, k8=bool(l)), None, dx, 2, 2, 2, 0)
    gw = _nan(Cin, Cout, 2, 2, dtype=torch.float32)
    gb = _nan(Cout, dtype=torch.float32)
    _nan_ws(lib.fn("umi_conv_wgrad_ws_bytes")(N, h, w, Cout, Cin, 2, 2, lib.UMI_F16, 0))
    assert ops.convT_wgrad_bias(dupd, xd, td, gw, gb, 1.0)
    torch.cuda.synchronize()
    assert torch.isnan(buf[..., :Cout]).all()
    gw_ref = torch.zeros(Cin, Cout, 2, 2, dtype=torch.float64)
    gb_ref = torch.zeros(Cout, dtype=torch.float64)
    for n in range(N):
        an = a[n].permute(2, 0, 1)[None]
        ref = F.conv_transpose2d(an, wt, b, stride=2)[0].permute(1, 2, 0)
        assert ref.abs().max().item() < 2048
        assert torch.equal(buf[n, ..., Cout:].float().cpu(), ref), n
        dup = dupd[n].float().cpu()
        dref = F.conv2d(dup.permute(2, 0, 1)[None], wt, None, stride=2)[0].permute(1, 2, 0)
        assert dref.abs().max().item() < 2048
        assert torch.equal(dx[n].float().cpu(), dref), n
        gw_ref += torch.einsum("chw,hpwqd->cdpq", a[n].permute(2, 0, 1).double(), dup.double().view(h, 2, w, 2, Cout))
        gb_ref += dup.double().sum((0, 1))
    assert N * h * w * 3 < 2 ** 24
    assert torch.equal(gw.cpu().double(), gw_ref) and torch.equal(gb.cpu().double(), gb_ref)


def test_maxpool_and_fused_bn_reduction_exact_at_bench_size():
    """MaxPool2d(2) of enc0's activated output at 2 x 512^2 x 64 and umi_pool2_bwd_bnred: forward, routed gradient and the
    channel totals of its sum dz / sum dz*xhat rows, exact.  No ties inside a window except where every value clips to 0
    (those windows route a gradient the ReLU mask then zeroes: dz is fully determined)."""
    lib, ops = _gpu()
    N, H, W, C = 2, 512, 512, 64
    g = torch.Generator().manual_seed(7)
    base = torch.rand(N * (H // 2) * (W // 2) * C, 4, generator=g).argsort(1).float()    # a permutation of 0..3 per window
    x = base.view(N, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, H, W, C) + 1.0
    del base
    t = torch.zeros(C, 4)
    t[:, 0] = _ints((C,), 0, 3, g)
    t[:, 1] = torch.tensor([1.0, 2.0])[torch.randint(0, 2, (C,), generator=g)]
    t[:, 2] = _ints((C,), -2, 0, g)
    rstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)]
    dp = _ints((N, H // 2, W // 2, C), -3, 3, g)
    xd, td, rsd, dpd = x.half().to(DEV), t.to(DEV), rstd.to(DEV), dp.half().to(DEV)
    y = _nan(N, H // 2, W // 2, C)
    ops.pool2_fwd(xd, td, y)
    rows = lib.fn("umi_pool2_bwd_bnred_stat_rows")(N, H, W, C)
    assert rows > 0
    part = _nan(rows * 2 * C, dtype=torch.float32)
    da = _nan(N, H, W, C)
    lib.check(lib.fn("umi_pool2_bwd_bnred")(dpd.data_ptr(), C, xd.data_ptr(), C, td.data_ptr(), rsd.data_ptr(), da.data_ptr(),
                                            C, 0, part.data_ptr(), N, H, W, C, lib.UMI_F16, ops._stream()), "umi_pool2_bwd_bnred")
    torch.cuda.synchronize()
    s1 = torch.zeros(C, dtype=torch.float64)
    s2 = torch.zeros(C, dtype=torch.float64)
    bound = 0.0
    for n in range(N):
        act = _apply(x[n], t).permute(2, 0, 1)[None].requires_grad_(True)
        ref = F.max_pool2d(act, 2)
        ref.backward(dp[n].permute(2, 0, 1)[None])
        assert torch.equal(y[n].float().cpu(), ref.detach()[0].permute(1, 2, 0)), n
        a4 = act.detach()[0].view(C, H // 2, 2, W // 2, 2)
        mx = a4.amax((2, 4), keepdim=True)
        unique = ((a4 == mx).sum((2, 4), keepdim=True) == 1).expand_as(a4).reshape(C, H, W).permute(1, 2, 0)
        assert unique.float().mean().item() > 0.5
        dref = act.grad[0].permute(1, 2, 0)
        got = da[n].float().cpu()
        assert torch.equal(got[unique], dref[unique]) and not torch.isnan(got).any(), n
        xn = x[n].double()
        dz = dref.double() * ((xn * t[:, 1].double() + t[:, 2].double()) > 0)
        dzx = dz * (xn - t[:, 0].double()) * rstd.double()
        s1 += dz.sum((0, 1))
        s2 += dzx.sum((0, 1))
        bound += dzx.abs().sum((0, 1)).max().item() + dz.abs().sum((0, 1)).max().item()
    assert bound < 2 ** 22                                 # multiples of 1/2: every partial sum is exact in fp32
    got = part.view(rows, 2, C).cpu().double().sum(0)
    assert torch.equal(got[0], s1) and torch.equal(got[1], s2)


def test_stem_and_head_exact_at_bench_size():
    """First conv (1 -> 64: forward, statistics, weight gradient) and the OutConv head (64 -> 2: fp32 logits with bias, data
    and weight gradient) at 2 x 512 x 512."""
    lib, ops = _gpu()
    N, H, W, C, ncls = 2, 512, 512, 64, 2
    g = torch.Generator().manual_seed(8)
    x = _ints((N, H, W, 1), -1, 1, g)
    w = _ints((C, 1, 3, 3), -1, 1, g)
    dy = _ints((N, H, W, C), -1, 1, g)
    xd, wd = x.half().to(DEV), w.to(DEV)
    y = _nan(N, H, W, C)
    _, rows = ops.conv_plan(xd, y, 3, 3, 1, 1)
    part = _nan(rows * 2 * C, dtype=torch.float32)
    wp = ops.pack_conv_fwd(wd, torch.float16, k8=False)
    lib.check(lib.fn("umi_conv_fwd")(xd.data_ptr(), 1, None, wp.data_ptr(), None, y.data_ptr(), C, part.data_ptr(), N, H, W, 1, C,
                                     3, 3, 1, 1, H, W, 0, 0, H, W, lib.UMI_F16, lib.UMI_F16, 0, ops._stream()), "umi_conv_fwd")
    gw = _nan(C, 1, 3, 3, dtype=torch.float32)
    _nan_ws(lib.fn("umi_conv_wgrad_ws_bytes")(N, H, W, 1, C, 3, 3, lib.UMI_F16, 0))
    ops.conv_wgrad(xd, None, dy.half().to(DEV), None, gw, 9, 9, 1, 0.25, 3, 3, 1, 1)
    torch.cuda.synchronize()
    s1 = torch.zeros(C, dtype=torch.float64)
    s2 = torch.zeros(C, dtype=torch.float64)
    for n in range(N):
        ref = F.conv2d(x[n].permute(2, 0, 1)[None], w, None, 1, 1)[0].permute(1, 2, 0)
        assert torch.equal(y[n].float().cpu(), ref), n
        s1 += ref.double().sum((0, 1))
        s2 += ref.double().square().sum((0, 1))
    assert s2.max().item() < 2 ** 24                       # sum |ref| <= sum ref^2 here: every row partial sum is exact
    got = part.view(rows, 2, C).cpu().double().sum(0)
    assert torch.equal(got[0], s1) and torch.equal(got[1], s2)
    assert N * H * W < 2 ** 24
    assert torch.equal(gw.cpu().double(), _wgrad_ref(x, dy, 3, 1) * 0.25)

    a = _ints((N, H, W, C), -1, 1, g)
    t = _int_tx(C, g)
    wo = _ints((ncls, C, 1, 1), -2, 2, g)
    b = _ints((ncls,), -3, 3, g)
    dl = _ints((N, H, W, ncls), -2, 2, g)
    act = _apply(a, t)
    assert N * H * W * act.abs().max().item() * 2 < 2 ** 24
    ad, td, wod, dld = a.half().to(DEV), t.to(DEV), wo.to(DEV), dl.half().to(DEV)
    logits = _nan(N, H, W, ncls, dtype=torch.float32)
    ops.conv_fwd(ad, td, lambda l: ops.pack_conv_fwd(wod, torch.float16, k8=bool(l)), b.to(DEV), logits, 1, 1, 1, 0)
    da = _nan(N, H, W, C)
    ops.conv_fwd(dld, None, lambda l: ops.pack_conv_dgrad(wod, torch.float16, k8=bool(l)), None, da, 1, 1, 1, 0)
    gwo = _nan(ncls, C, 1, 1, dtype=torch.float32)
    _nan_ws(lib.fn("umi_conv_wgrad_ws_bytes")(N, H, W, C, ncls, 1, 1, lib.UMI_F16, 0))
    ops.conv_wgrad(ad, td, dld, None, gwo, C, 1, 1, 2.0, 1, 1, 1, 0)
    torch.cuda.synchronize()
    for n in range(N):
        an = act[n].permute(2, 0, 1)[None]
        assert torch.equal(logits[n].cpu(), F.conv2d(an, wo, b)[0].permute(1, 2, 0)), n
        dref = F.conv_transpose2d(dl[n].permute(2, 0, 1)[None], wo)[0].permute(1, 2, 0)
        assert torch.equal(da[n].float().cpu(), dref), n
    assert torch.equal(gwo.cpu().double(), _wgrad_ref(act, dl, 1, 0) * 2.0)


def _generic_lines(err):
    return [l for l in err.splitlines() if "[umi generic" in l]


def test_unet_fp16_feat64_at_512():
    """UNet(1,2,64) fp16 at 1 x 1 x 512 x 512 against the CPU oracle, with every bound of
    tests/test_gpu_unet.py::test_unet_fp16_feat64_benchmark_widths unchanged and no conv on the generic kernels."""
    _gpu()
    env = dict(os.environ, UMI_TRACE_GENERIC="1")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_fp16_feat64.py"), "1", "2", "--size", "512",
                        "--batch", "1"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert not _generic_lines(r.stderr), _generic_lines(r.stderr)[:8]
    m = json.loads([l for l in r.stdout.splitlines() if l.startswith("FP16_FEAT64 ")][-1][len("FP16_FEAT64 "):])
    print(m)
    assert m["grads_finite"]
    assert m["logits_max_err_over_scale_vs_fp32_oracle"] < 2e-2 and m["logits_max_err_over_scale_vs_fp16_oracle"] < 1e-2
    assert abs(m["loss"] - m["loss_fp32_oracle"]) < 5e-3 and abs(m["loss"] - m["loss_fp16_oracle"]) < 5e-3
    assert m["argmax_mismatch_clear"] == 0 and m["pixels_clear_of_near_ties"] > 0.5 * m["pixels"]
    gq, fl = m["grad_rel_l2_vs_fp16_oracle"], m["grad_rel_l2_fp16_oracle_self_noise_floor"]
    assert gq["median"] < 1.5 * fl["median"] + 0.01 and gq["worst"] < 2.0 * fl["worst"] + 0.02, (gq, fl)
    assert gq["median"] < 0.25 and gq["worst"] < 0.5, gq
    assert m["grad_cosine_vs_fp32_oracle"]["worst"] > 0.9, m["grad_cosine_vs_fp32_oracle"]


def test_graphed_step_matches_eager_at_bench_scale():
    """The benchmark's step (UNet(1,2,64) fp16, B = 16, 512 x 512) captured in a HIP graph and replayed follows the eager
    trajectory bit for bit (losses and every weight), stays finite, and runs no conv on the generic VALU kernels."""
    _gpu()
    env = dict(os.environ, UMI_TRACE_GENERIC="1")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_graphed_step.py"), "--features", "64", "--size",
                        "512", "--batch", "16"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "GRAPHED_STEP_OK" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert not _generic_lines(r.stderr), _generic_lines(r.stderr)[:8]
