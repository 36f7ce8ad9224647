"""Every kernel call of one UNet(c, k, 64) fp16 training step at 2 x 512 x 512, pinned at the arguments the step passes.

tests/test_gpu_exact_fullsize.py pins the matrix-core kernels at the benchmark's geometry down to the 128^2 level, on dense tensors
and with an output scale of its own.  The step itself (tests/test_gpu_unet_step_calls.py records it) runs other calls: the encoder's
second convolutions write into the lower half of a concat buffer (ldy = 2 Co) and take their gradient from a slice of the concat
gradient (lddy = 2 Co), the max-pool reads and accumulates into such slices, the encoder's first convolutions read a pooled
(already activated) tensor without a transform, every weight gradient leaves its kernel multiplied by 1 / loss scale = 2^-16 and
has its split-K reduction deferred, and the backward pass runs on the fused kernels (umi_head_bwd_fused, umi_conv_gather_bnred,
umi_pool2_bwd_bnred with accumulate = 1, umi_conv_wgrad_bnapply with and without a stored dz, umi_conv_wgrad_bias).

The construction is that of test_gpu_exact_fullsize.py: small-integer (or dyadic) operands, so that every product and every partial
sum is exact in fp16 / fp32 in any order and the kernels must reproduce the CPU reference bit for bit; outputs, partial-row buffers
and the unused halves of strided buffers prefilled with NaN, split-K workspaces with 0xFF bytes; one image at a time on the CPU.
Per-tile statistics rows are compared row by row where the row -> pixels map is the kernel's tile grid (3x3 kernels, the tap-gather
kernel), as exact channel totals where it is a grid-stride loop (head, max-pool, stem); then through umi_bn_finalize /
umi_bn_bwd_from_partials against float64.  Every exactness premise is asserted on the CPU data.

Each case states the calls it pins as `specs`: (entry point, scalar arguments by name, null addresses), rows per image.  A test
records its own C-ABI calls and asserts that it made every call its case lists; the census derives the pinned keys from the same
lists."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import abi_calls as A
from tests.test_gpu_exact import _apply, _gpu, _int_tx, _ints
from tests.test_gpu_exact_fullsize import _bn_rows, _check_finalize, _check_rows, _nan, _nan_ws, _th, _tile_sums, _wgrad_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16 = 0, 1                     # UMI_F32, UMI_F16 (asserted against the header in _start)
N = 2
OUT_SCALE = 2.0 ** -16              # 1 / umi.graph.default_loss_scale(fp16, 2 * 512 * 512): what the tape's weight gradients carry
GUARD = 4096


# ========================================================================================================================
# call specs
# ========================================================================================================================
def _spec(entry, nulls=(), **scal):
    return (entry, scal, tuple(nulls))


def key_of(spec):
    entry, scal, nulls = spec
    vals = dict(scal)
    for name, kind in A.params(entry):
        if kind == "ptr":
            vals[name] = None if name in nulls else True
    return A.key(entry, vals, 1)


def _conv_rows(H, Co):
    """Statistics rows per image of the 3x3 matrix-core kernels: tiles of TH x 32 pixels, TH = 8 with 128-channel blocks, else 16."""
    th = 8 if Co % 128 == 0 else 16
    return ((H + th - 1) // th) * ((H + 31) // 32)


def spec_conv_fwd(H, Ci, Co, ldx, ldy, tx, stats, R=3, up=False, bias=False, out32=False):
    stride, pad = {3: (1, 1), 2: (2, 0), 1: (1, 0)}[R]
    nulls = [n for n, given in (("tx", tx), ("bias", bias), ("stat_part", stats)) if not given]
    return _spec("umi_conv_fwd", nulls, ldx=ldx, ldy=ldy, H=H, W=H, Ci=Ci, Co=Co, R=R, S=R, stride=stride, pad=pad, Ho=H, Wo=H,
                 off_h=0, off_w=0, out_H=2 * H if up else H, out_W=2 * H if up else H, in_dtype=F16,
                 out_dtype=F32 if out32 else F16, flags=1 if up else 0)


def spec_pack(kind, wshape, k8):
    from umi import ops
    T, K, Nn, st, sk, sn, flip = ops._pack_args(kind, tuple(wshape))
    return _spec("umi_pack_kn8" if k8 else "umi_pack_kn", T=T, K=K, st=st, sk=sk, sn=sn, flip_t=flip, Kpad=K, Npad=Nn, dtype=F16)


def spec_finalize(rows, C, HW):
    return _spec("umi_bn_finalize", rows=rows, C=C, count=float(HW), eps=1e-5, momentum=0.1)


def spec_from_partials(rows, C):
    return _spec("umi_bn_bwd_from_partials", rows=rows, C=C)


def _start(monkeypatch):
    lib, ops = _gpu()
    assert (lib.UMI_F32, lib.UMI_F16, lib.CONV_UPSAMPLE2) == (F32, F16, 1)
    return lib, ops, A.Recorder(monkeypatch)


def _made(rec, specs):
    """The test made every call its case lists (so the census may count the case's keys as pinned)."""
    seen = {A.key(e, v, N) for e, v, st in rec.calls if st == 0}
    missing = [A.show(key_of(s)) for s in specs if key_of(s) not in seen]
    assert not missing, missing


def _slice_of_nan(v, ld):
    """v ([N, H, W, C] on the CPU) as the lower channels of a NaN-filled [N, H, W, ld] fp16 device buffer: (buffer, view)."""
    C = v.shape[3]
    if ld == C:
        d = v.half().to(DEV)
        return d, d
    buf = _nan(*v.shape[:3], ld)
    buf[..., :C] = v.half().to(DEV)
    return buf, buf[..., :C]


def _rest_is_nan(buf, C):
    return buf.shape[3] == C or bool(torch.isnan(buf[..., C:]).all())


def _check_from_partials(lib, ops, part, C, s1, s2, exact):
    """The rows through umi_bn_bwd_from_partials against the float64 totals: equal where every fp32 partial sum of the totals
    is exact (`exact`), else within 2e-5 of the largest total (the bound tests/test_gpu_unet.py holds this reduction to)."""
    sums = _nan(2, C, dtype=torch.float32)
    rows = part.numel() // (2 * C)
    lib.check(lib.fn("umi_bn_bwd_from_partials")(part.data_ptr(), rows, C, sums[0].data_ptr(), sums[1].data_ptr(), ops._stream()),
              "umi_bn_bwd_from_partials")
    got = sums.cpu().double()
    for g, s in ((got[0], s1), (got[1], s2)):
        if exact:
            assert torch.equal(g, s), (g - s).abs().max().item()
        else:
            assert (g - s).abs().max().item() <= 2e-5 * max(1.0, s.abs().max().item()), (g - s).abs().max().item()


# ========================================================================================================================
# 1. Conv3x3 forward (+ statistics rows) and the plain data gradients, on the step's strides
# ========================================================================================================================
# layer, H (= W), Ci, Co, ldy, transform on load, statistics rows, data gradient (weights [Ci][Co][3][3], rotated packing)
FWD_CASES = [
    ("inc.c2", 512, 64, 64, 128, True, True, False),             # lower half of the 512^2 concat buffer
    ("down1.c1", 256, 64, 128, 128, False, True, False),         # reads the pooled (activated) tensor: no transform
    ("down1.c2", 256, 128, 128, 256, True, True, False),
    ("down2.c1", 128, 128, 256, 256, False, True, False),
    ("down2.c2", 128, 256, 256, 512, True, True, False),
    ("down3.c1", 64, 256, 512, 512, False, True, False),
    ("down3.c2", 64, 512, 512, 1024, True, True, False),
    ("down4.c1", 32, 512, 1024, 1024, False, True, False),
    ("down4.c2", 32, 1024, 1024, 1024, True, True, False),
    ("up1.c1", 64, 1024, 512, 512, True, True, False),           # reads the full-width concat buffer
    ("up1.c2", 64, 512, 512, 512, True, True, False),
    ("up2.c1", 128, 512, 256, 256, True, True, False),
    ("up2.c2", 128, 256, 256, 256, True, True, False),
    ("up3.c1", 256, 256, 128, 128, True, True, False),
    ("up3.c2", 256, 128, 128, 128, True, True, False),
    ("up3.c1 dgrad", 256, 128, 256, 256, False, False, True),    # into the concat gradient (both halves, one dense tensor)
    ("up2.c1 dgrad", 128, 256, 512, 512, False, False, True),
    ("up1.c1 dgrad", 64, 512, 1024, 1024, False, False, True),
    ("down4.c1 dgrad", 32, 1024, 512, 512, False, False, True),  # into the pooled tensor's gradient
    ("down3.c1 dgrad", 64, 512, 256, 256, False, False, True),
]


def specs_fwd(case):
    name, H, Ci, Co, ldy, tx, stats, dgrad = case
    out = [spec_conv_fwd(H, Ci, Co, Ci, ldy, tx, stats),
           spec_pack("conv_dgrad" if dgrad else "conv_fwd", (Ci, Co, 3, 3) if dgrad else (Co, Ci, 3, 3), True)]
    if stats:
        out.append(spec_finalize(_conv_rows(H, Co), Co, H * H))
    return out


@pytest.mark.parametrize("case", FWD_CASES, ids=[c[0].replace(" ", "_") for c in FWD_CASES])
def test_conv3x3_forward_as_the_step_calls_it(case, monkeypatch):
    lib, ops, rec = _start(monkeypatch)
    name, H, Ci, Co, ldy, tx, stats, dgrad = case
    W = H
    g = torch.Generator().manual_seed(H + Ci + 3 * Co + ldy)
    x = _ints((N, H, W, Ci), -1, 1, g)
    w = _ints((Ci, Co, 3, 3) if dgrad else (Co, Ci, 3, 3), -1, 1, g)
    t = _int_tx(Ci, g) if tx else None
    xd = x.half().to(DEV)
    buf = _nan(N, H, W, ldy)
    y = buf[..., :Co]
    lay, rows = ops.conv_plan(xd, y, 3, 3, 1, 1)
    assert lay == 1 and rows == N * _conv_rows(H, Co)             # the matrix-core path, its tile grid
    wp = (ops.pack_conv_dgrad if dgrad else ops.pack_conv_fwd)(w.to(DEV), torch.float16, k8=True)
    part = _nan(rows * 2 * Co, dtype=torch.float32) if stats else None
    lib.call("umi_conv_fwd", xd.data_ptr(), Ci, ops._ptr(t.to(DEV) if tx else None), wp.data_ptr(), None, y.data_ptr(), ldy,
             ops._ptr(part), N, H, W, Ci, Co, 3, 3, 1, 1, H, W, 0, 0, H, W, F16, F16, 0, ops._stream())
    torch.cuda.synchronize()
    assert _rest_is_nan(buf, Co)
    th = _th(rows, N, H, W, Co)
    per = rows // N
    s1 = torch.zeros(Co, dtype=torch.float64)
    s2 = torch.zeros(Co, dtype=torch.float64)
    for n in range(N):
        a = (_apply(x[n], t) if tx else x[n]).permute(2, 0, 1)[None]
        ref = (F.conv_transpose2d(a, w, None, 1, 1) if dgrad else F.conv2d(a, w, None, 1, 1))[0].permute(1, 2, 0).contiguous()
        assert ref.abs().max().item() < 2048                      # every output is an fp16 integer
        assert torch.equal(y[n].float().cpu(), ref), (name, n)
        if stats:
            r = ref.double()
            ra, rb = _tile_sums(r.abs(), th), _tile_sums(r * r, th)
            assert ra.max().item() < 2 ** 24 and rb.max().item() < 2 ** 24     # every partial sum of a row is exact in fp32
            _check_rows(part[n * per * 2 * Co:(n + 1) * per * 2 * Co], per, Co, _tile_sums(r, th), rb)
            s1 += r.sum((0, 1))
            s2 += (r * r).sum((0, 1))
    if stats:
        _check_finalize(ops, part, Co, N * H * W, s1, s2)
    _made(rec, specs_fwd(case))


# ========================================================================================================================
# 2. Conv3x3 data gradient + fused BatchNorm rows (umi_conv_dgrad_bnred) of every second convolution
# ========================================================================================================================
# H, channels of dy (the conv's output), channels of da (its input), lddy: 2 C where dy is the lower half of a concat gradient
DGRAD_CASES = [(512, 64, 64, 64), (256, 128, 128, 128), (128, 256, 256, 256), (64, 512, 512, 512), (32, 1024, 1024, 1024),
               (64, 512, 512, 1024), (128, 256, 256, 512), (256, 128, 128, 256)]


def specs_dgrad(case):
    H, Cy, Ca, lddy = case
    return [_spec("umi_conv_dgrad_bnred", lddy=lddy, ldda=Ca, ldybn=Ca, H=H, W=H, Ci=Cy, Co=Ca, dtype=F16),
            spec_pack("conv_dgrad", (Cy, Ca, 3, 3), True), spec_from_partials(_conv_rows(H, Ca), Ca)]


@pytest.mark.parametrize("case", DGRAD_CASES)
def test_conv3x3_dgrad_bnred_as_the_step_calls_it(case, monkeypatch):
    lib, ops, rec = _start(monkeypatch)
    H, Cy, Ca, lddy = case
    W = H
    g = torch.Generator().manual_seed(sum(case) + 2)
    w = _ints((Cy, Ca, 3, 3), -1, 1, g)
    dy = _ints((N, H, W, Cy), -1, 1, g)
    ybn = _ints((N, H, W, Ca), -2, 2, g)
    t, rstd = _bn_rows(Ca, g)
    dyb, dyd = _slice_of_nan(dy, lddy)
    ybd, td, rsd = ybn.half().to(DEV), t.to(DEV).contiguous(), rstd.to(DEV)
    da = _nan(N, H, W, Ca)
    part = ops.conv_dgrad_bnred(dyd, ops.pack_conv_dgrad(w.to(DEV), torch.float16, k8=True), da, ybd, td, rsd)
    assert part is not None
    part_nan = torch.full_like(part, float("nan"))               # the same launch into a NaN-filled row buffer
    lib.call("umi_conv_dgrad_bnred", dyd.data_ptr(), lddy, ops.pack_conv_dgrad(w.to(DEV), torch.float16, k8=True).data_ptr(),
             da.data_ptr(), Ca, ybd.data_ptr(), Ca, td.data_ptr(), rsd.data_ptr(), part_nan.data_ptr(), N, H, W, Cy, Ca, F16,
             ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(part, part_nan) and _rest_is_nan(dyb, Cy)
    rows = part.numel() // (2 * Ca)
    assert rows == N * _conv_rows(H, Ca)
    th = _th(rows, N, H, W, Ca)
    per = rows // N
    s1 = torch.zeros(Ca, dtype=torch.float64)
    s2 = torch.zeros(Ca, dtype=torch.float64)
    for n in range(N):
        ref = F.conv_transpose2d(dy[n].permute(2, 0, 1)[None], w, None, 1, 1)[0].permute(1, 2, 0).contiguous()
        assert ref.abs().max().item() < 2048
        assert torch.equal(da[n].float().cpu(), ref), n
        yb = ybn[n].double()
        dz = ref.double() * ((yb * t[:, 1].double() + t[:, 2].double()) > 0)
        dzx = dz * (yb - t[:, 0].double()) * rstd.double()
        assert _tile_sums(dz.abs(), th).max().item() < 2 ** 21 and _tile_sums(dzx.abs(), th).max().item() < 2 ** 21
        _check_rows(part_nan[n * per * 2 * Ca:(n + 1) * per * 2 * Ca], per, Ca, _tile_sums(dz, th), _tile_sums(dzx, th))
        s1 += dz.sum((0, 1))
        s2 += dzx.sum((0, 1))
    _check_from_partials(lib, ops, part_nan, Ca, s1, s2, exact=False)
    _made(rec, specs_dgrad(case))


# ========================================================================================================================
# 3. Conv3x3 weight gradient, deferred split-K reduction, at the tape's output scale
# ========================================================================================================================
# layer, H, Ci, Co, lddy, transform on x
WGRAD_CASES = [
    ("up4.c1", 512, 128, 64, 64, True), ("up3.c2", 256, 128, 128, 128, True), ("up3.c1", 256, 256, 128, 128, True),
    ("up2.c2", 128, 256, 256, 256, True), ("up2.c1", 128, 512, 256, 256, True), ("up1.c2", 64, 512, 512, 512, True),
    ("up1.c1", 64, 1024, 512, 512, True), ("down4.c2", 32, 1024, 1024, 1024, True), ("down4.c1", 32, 512, 1024, 1024, False),
    ("down3.c2", 64, 512, 512, 1024, True), ("down3.c1", 64, 256, 512, 512, False), ("down2.c2", 128, 256, 256, 512, True),
    ("down2.c1", 128, 128, 256, 256, False), ("down1.c2", 256, 128, 128, 256, True),
]


def specs_wgrad(case):
    name, H, Ci, Co, lddy, txa = case
    return [_spec("umi_conv_wgrad_deferred", ("txb",) if txa else ("txa", "txb"), ldx=Ci, lddy=lddy, s_co=Ci * 9, s_ci=9, s_t=1,
                  out_scale=OUT_SCALE, H=H, W=H, Ci=Ci, Co=Co, R=3, S=3, stride=1, pad=1, Ho=H, Wo=H, dtype=F16, flags=0)]


@pytest.mark.parametrize("case", WGRAD_CASES, ids=[c[0] for c in WGRAD_CASES])
def test_conv3x3_weight_gradient_deferred_as_the_step_calls_it(case, monkeypatch):
    lib, ops, rec = _start(monkeypatch)
    name, H, Ci, Co, lddy, txa = case
    W = H
    g = torch.Generator().manual_seed(H + Ci + 3 * Co + lddy + 4)
    x = _ints((N, H, W, Ci), -1, 1, g)
    dy = _ints((N, H, W, Co), -1, 1, g)
    t = _int_tx(Ci, g) if txa else None
    a = _apply(x, t) if txa else x
    assert N * H * W * a.abs().max().item() < 2 ** 24                 # every partial sum is an exact fp32 integer
    ref = _wgrad_ref(a, dy, 3, 1) * OUT_SCALE                         # a power of two: exact
    xd = x.half().to(DEV)
    dyb, dyd = _slice_of_nan(dy, lddy)
    gw = _nan(Co, Ci, 3, 3, dtype=torch.float32)
    nb = lib.fn("umi_conv_wgrad_ws_bytes")(N, H, W, Ci, Co, 3, 3, F16, 0)
    ws = torch.full((max(nb, 16),), 255, dtype=torch.uint8, device=DEV)      # the call's own slabs, every byte 0xFF
    pend = ops._WgPending()
    lib.call("umi_conv_wgrad_deferred", xd.data_ptr(), Ci, ops._ptr(t.to(DEV) if txa else None), dyd.data_ptr(), lddy, None,
             gw.data_ptr(), Ci * 9, 9, 1, OUT_SCALE, N, H, W, Ci, Co, 3, 3, 1, 1, H, W, F16, 0, ws.data_ptr(), ws.numel(),
             ctypes.addressof(pend), ops._stream())
    assert pend.part and pend.splits >= 1                             # the split-K reduction was recorded, not run
    ops.wgrad_reduce_group([pend])
    torch.cuda.synchronize()
    assert torch.equal(gw.cpu().double(), ref) and _rest_is_nan(dyb, Co)
    _made(rec, specs_wgrad(case))


# ========================================================================================================================
# 4. Weight gradient fused with stage 3 of the BatchNorm backward (umi_conv_wgrad_bnapply), stored and unstored dz
# ========================================================================================================================
# layer, H, Ci, Co, ldda = ldy, lddz (0: dz is not stored), transform on x
BNAPPLY_CASES = [
    ("up4.c2", 512, 64, 64, 64, 64, True),
    ("inc.c2", 512, 64, 64, 128, 64, True),          # gradient and output are halves of concat buffers, dz is dense
    ("down1.c1", 256, 64, 128, 128, 128, False),     # the pooled input has no transform
    ("inc.c1 cin=1", 512, 1, 64, 64, 0, False),      # the stem: its input takes no gradient, dz is formed on the fly
    ("inc.c1 cin=3", 512, 3, 64, 64, 0, False),
]


def specs_bnapply(case):
    name, H, Ci, Co, ld, lddz, txa = case
    nulls = ([] if txa else ["txa"]) + ([] if lddz else ["dz"])
    return [_spec("umi_conv_wgrad_bnapply", nulls, ldx=Ci, ldda=ld, ldy=ld, lddz=lddz, s_co=Ci * 9, s_ci=9, s_t=1,
                  out_scale=OUT_SCALE, H=H, W=H, Ci=Ci, Co=Co, R=3, S=3, stride=1, pad=1, dtype=F16, flags=0)]


def _dyadic_bn_backward(Co, M, g):
    """(tx rows, rstd, c1, c2, sums) with dyadic effect: dz = scale * (mask * da - c1 - xhat * c2) is a multiple of 1/4."""
    tb = torch.zeros(Co, 4)
    tb[:, 1] = torch.tensor([0.5, 1.0])[torch.randint(0, 2, (Co,), generator=g)]
    tb[:, 2] = _ints((Co,), -1, 1, g)
    rstd = torch.tensor([1.0, 2.0])[torch.randint(0, 2, (Co,), generator=g)]
    c1 = _ints((Co,), -1, 1, g)
    c2 = torch.tensor([0.0, 0.5])[torch.randint(0, 2, (Co,), generator=g)]
    assert M & (M - 1) == 0                                # c = sum / M is exact
    return tb, rstd, c1, c2, torch.stack([c1 * M, c2 * M])


def _dz_ref(da, y, tb, rstd, c1, c2):
    return tb[:, 1] * ((y * tb[:, 1] + tb[:, 2] > 0).float() * da - c1 - (y - tb[:, 0]) * rstd * c2)


@pytest.mark.parametrize("case", BNAPPLY_CASES, ids=[c[0].replace(" ", "_") for c in BNAPPLY_CASES])
def test_wgrad_bnapply_as_the_step_calls_it(case, monkeypatch):
    """The fused call equals umi_bn_bwd_apply + umi_conv_wgrad bit for bit, and both equal the reference."""
    lib, ops, rec = _start(monkeypatch)
    name, H, Ci, Co, ld, lddz, txa = case
    W = H
    M = N * H * W
    g = torch.Generator().manual_seed(H + Ci + Co + ld + 5)
    x = _ints((N, H, W, Ci), -1, 1, g)
    t = None
    if txa:
        t = torch.zeros(Ci, 4)
        t[:, 1] = torch.tensor([1.0, -1.0])[torch.randint(0, 2, (Ci,), generator=g)]
    da = _ints((N, H, W, Co), -1, 1, g)
    y = _ints((N, H, W, Co), -1, 1, g)
    tb, rstd, c1, c2, sums = _dyadic_bn_backward(Co, M, g)
    a = _apply(x, t) if txa else x
    dz = _dz_ref(da, y, tb, rstd, c1, c2)
    assert dz.abs().max().item() <= 4 and torch.equal(dz * 4, (dz * 4).round())
    assert M * a.abs().max().item() * dz.abs().max().item() * 4 < 2 ** 24
    ref = _wgrad_ref(a, dz, 3, 1) * OUT_SCALE
    xd = x.half().to(DEV)
    dab, dad = _slice_of_nan(da, ld)
    yb, yd = _slice_of_nan(y, ld)
    txd = t.to(DEV) if txa else None
    tbd, rsd, sd = tb.to(DEV).contiguous(), rstd.to(DEV), sums.to(DEV)
    dz_f = _nan(N, H, W, Co) if lddz else None
    gw_f = _nan(Co, Ci, 3, 3, dtype=torch.float32)
    nb = lib.fn("umi_conv_wgrad_ws_bytes")(N, H, W, Ci, Co, 3, 3, F16, 0)
    _nan_ws(nb)
    assert ops.conv_wgrad_bnapply(xd, txd, dad, yd, tbd, rsd, sd[0], sd[1], dz_f, gw_f, Ci * 9, 9, 1, OUT_SCALE, 3, 3, 1, 1)
    dz_s = dad.clone()
    ops.bn_bwd_apply(dz_s, yd, tbd, rsd, sd[0], sd[1])
    gw_s = _nan(Co, Ci, 3, 3, dtype=torch.float32)
    _nan_ws(nb)
    ops.conv_wgrad(xd, txd, dz_s, None, gw_s, Ci * 9, 9, 1, OUT_SCALE, 3, 3, 1, 1)
    torch.cuda.synchronize()
    assert torch.equal(gw_f, gw_s)
    assert torch.equal(gw_f.cpu().double(), ref)
    assert torch.equal(dz_s.float().cpu(), dz)
    if lddz:
        assert torch.equal(dz_f, dz_s)
    assert _rest_is_nan(dab, Co) and _rest_is_nan(yb, Co) and torch.equal(dad.float().cpu(), da)     # the inputs are only read
    _made(rec, specs_bnapply(case))


# ========================================================================================================================
# 5. The transposed convolutions: scattered forward, tap-gather data gradient + BatchNorm rows, weight + bias gradient
# ========================================================================================================================
UP_CASES = [(32, 1024, 512), (64, 512, 256), (128, 256, 128), (256, 128, 64)]          # h (= w), Cin, Cout of up1 .. up4


def _gather_rows(h, Cin):
    """Rows per image of umi_conv_gather_bnred at these shapes: one per tile of 256 (128 below 128^2) consecutive output pixels."""
    return h * h // (256 if h >= 128 else 128)


def specs_up(case):
    h, Cin, Cout = case
    geo = dict(R=2, S=2, stride=2, pad=0, Ho=h, Wo=h, dtype=F16, flags=0)
    return [spec_conv_fwd(h, Cin, Cout, Cin, 2 * Cout, True, False, R=2, up=True, bias=True),
            spec_pack("convT_fwd", (Cin, Cout, 2, 2), True), spec_pack("convT_dgrad", (Cin, Cout, 2, 2), True),
            _spec("umi_conv_gather_bnred", ldx=2 * Cout, ldy=Cin, ldybn=Cin, H=2 * h, W=2 * h, Ci=Cout, Co=Cin, **geo),
            spec_from_partials(_gather_rows(h, Cin), Cin),
            _spec("umi_conv_wgrad_bias", ldx=2 * Cout, lddy=Cin, s_co=Cout * 4, s_ci=4, s_t=1, out_scale=OUT_SCALE, H=2 * h,
                  W=2 * h, Ci=Cout, Co=Cin, Ho=h, Wo=h, dtype=F16, flags=0)]


@pytest.mark.parametrize("case", UP_CASES)
def test_conv_transpose_trio_as_the_step_calls_it(case, monkeypatch):
    lib, ops, rec = _start(monkeypatch)
    h, Cin, Cout = case
    w = h
    g = torch.Generator().manual_seed(sum(case) + 6)
    x = _ints((N, h, w, Cin), -1, 1, g)
    wt = _ints((Cin, Cout, 2, 2), -1, 1, g)
    b = _ints((Cout,), -3, 3, g)
    t = _int_tx(Cin, g)
    a = _apply(x, t)
    ybn = _ints((N, h, w, Cin), -2, 2, g)                  # the raw output of the DoubleConv below, for the fused reduction
    tb, rstd = _bn_rows(Cin, g)
    wd, xd, td = wt.to(DEV), x.half().to(DEV), t.to(DEV)
    buf = _nan(N, 2 * h, 2 * w, 2 * Cout)
    dest = buf[..., Cout:]
    assert ops.conv_plan(xd, dest, 2, 2, 2, 0, lib.CONV_UPSAMPLE2, True)[0] == 1
    ops.conv_fwd(xd, td, lambda l: ops.pack_convT_fwd(wd, torch.float16, k8=bool(l)), b.to(DEV), dest, 2, 2, 2, 0,
                 flags=lib.CONV_UPSAMPLE2, up_offset=(0, 0))
    dupb = torch.randint(-1, 2, (N, 2 * h, 2 * w, 2 * Cout), generator=torch.Generator(device=DEV).manual_seed(6), device=DEV,
                         dtype=torch.int8).half()
    dupd = dupb[..., Cout:]                                # the upper half of the concat gradient
    dx = _nan(N, h, w, Cin)
    part = ops.conv_gather_bnred(dupd, ops.pack_convT_dgrad(wd, torch.float16, k8=True), dx, ybn.half().to(DEV),
                                 tb.to(DEV).contiguous(), rstd.to(DEV), 2, 2, 2, 0)
    assert part is not None
    rows = part.numel() // (2 * Cin)
    assert rows == N * _gather_rows(h, Cin)
    gw = _nan(Cin, Cout, 2, 2, dtype=torch.float32)
    gb = _nan(Cout, dtype=torch.float32)
    pending = []
    assert ops.convT_wgrad_bias(dupd, xd, td, gw, gb, OUT_SCALE, defer=pending)
    assert len(pending) == 1
    ops.wgrad_reduce_flush(pending)
    torch.cuda.synchronize()
    assert torch.isnan(buf[..., :Cout]).all()
    per = rows // N
    gw_ref = torch.zeros(Cin, Cout, 2, 2, dtype=torch.float64)
    gb_ref = torch.zeros(Cout, dtype=torch.float64)
    s1 = torch.zeros(Cin, dtype=torch.float64)
    s2 = torch.zeros(Cin, dtype=torch.float64)
    for n in range(N):
        an = a[n].permute(2, 0, 1)[None]
        ref = F.conv_transpose2d(an, wt, b, stride=2)[0].permute(1, 2, 0)
        assert ref.abs().max().item() < 2048
        assert torch.equal(buf[n, ..., Cout:].float().cpu(), ref), n
        dup = dupd[n].float().cpu()
        dref = F.conv2d(dup.permute(2, 0, 1)[None], wt, None, stride=2)[0].permute(1, 2, 0)
        assert dref.abs().max().item() < 2048
        assert torch.equal(dx[n].float().cpu(), dref), n
        yb = ybn[n].double()
        dz = dref.double() * ((yb * tb[:, 1].double() + tb[:, 2].double()) > 0)
        dzx = dz * (yb - tb[:, 0].double()) * rstd.double()

        def chunks(v):
            return v.reshape(per, h * w // per, Cin).sum(1)
        assert chunks(dz.abs()).max().item() < 2 ** 21 and chunks(dzx.abs()).max().item() < 2 ** 21   # multiples of 1/4
        _check_rows(part[n * per * 2 * Cin:(n + 1) * per * 2 * Cin], per, Cin, chunks(dz), chunks(dzx))
        s1 += dz.sum((0, 1))
        s2 += dzx.sum((0, 1))
        gw_ref += torch.einsum("chw,hpwqd->cdpq", a[n].permute(2, 0, 1).double(), dup.double().view(h, 2, w, 2, Cout))
        gb_ref += dup.double().sum((0, 1))
    assert N * h * w * 3 < 2 ** 24 and N * 4 * h * w < 2 ** 24
    assert torch.equal(gw.cpu().double(), gw_ref * OUT_SCALE) and torch.equal(gb.cpu().double(), gb_ref * OUT_SCALE)
    _check_from_partials(lib, ops, part, Cin, s1, s2, exact=False)
    _made(rec, specs_up(case))


# ========================================================================================================================
# 6. Max-pool on concat-buffer slices, its backward accumulating onto the skip's gradient
# ========================================================================================================================
POOL_CASES = [(512, 64), (256, 128), (128, 256), (64, 512)]


def _pool_rows(H, C):
    """umi_pool2_bwd_bnred's rows per image at these sizes (one per workgroup of its grid: 256 lanes x 8 channels x 1 window)."""
    return (H // 2) * (H // 2) * (C // 8) // 256


def specs_pool(case):
    H, C = case
    return [_spec("umi_pool2_fwd", ldx=2 * C, ldy=C, H=H, W=H, C=C, dtype=F16),
            _spec("umi_pool2_bwd_bnred", lddp=C, ldx=2 * C, ldda=2 * C, accumulate=1, H=H, W=H, C=C, dtype=F16),
            spec_from_partials(_pool_rows(H, C), C)]


@pytest.mark.parametrize("case", POOL_CASES)
def test_maxpool_on_concat_slices_with_accumulation(case, monkeypatch):
    """Encoder outputs live in the lower half of the decoder's concat buffer, and the skip's gradient reaches that half of the
    concat gradient first: ldx = ldda = 2 C and accumulate = 1.  Forward, the accumulated gradient and the channel totals of the
    rows exact; the upper halves untouched.  Ties as in test_maxpool_and_fused_bn_reduction_exact_at_bench_size."""
    lib, ops, rec = _start(monkeypatch)
    H, C = case
    W = H
    g = torch.Generator().manual_seed(H + C + 7)
    base = torch.rand(N * (H // 2) * (W // 2) * C, 4, generator=g).argsort(1).float()    # a permutation of 0..3 per window
    x = base.view(N, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(N, H, W, C) + 1.0
    del base
    t = torch.zeros(C, 4)
    t[:, 0] = _ints((C,), 0, 3, g)
    t[:, 1] = torch.tensor([1.0, 2.0])[torch.randint(0, 2, (C,), generator=g)]
    t[:, 2] = _ints((C,), -2, 0, g)
    rstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (C,), generator=g)]
    dp = _ints((N, H // 2, W // 2, C), -3, 3, g)
    # the skip connection's gradient, already there (sparse: the exactness bound below covers the sums of both contributions)
    prior = _ints((N, H, W, C), -1, 1, g) * (torch.rand(N, H, W, C, generator=g) < 0.25)
    xb, xd = _slice_of_nan(x, 2 * C)
    dab, dad = _slice_of_nan(prior, 2 * C)
    td, rsd, dpd = t.to(DEV), rstd.to(DEV), dp.half().to(DEV)
    y = _nan(N, H // 2, W // 2, C)
    ops.pool2_fwd(xd, td, y)
    part = ops.pool2_bwd_bnred(dpd, xd, td, rsd, dad, True)
    assert part is not None
    rows = part.numel() // (2 * C)
    assert rows == N * _pool_rows(H, C)
    part_nan = torch.full_like(part, float("nan"))         # again into NaN-filled rows, onto a fresh copy of the prior gradient
    dab2, dad2 = _slice_of_nan(prior, 2 * C)
    lib.call("umi_pool2_bwd_bnred", dpd.data_ptr(), C, xd.data_ptr(), 2 * C, td.data_ptr(), rsd.data_ptr(), dad2.data_ptr(),
             2 * C, 1, part_nan.data_ptr(), N, H, W, C, F16, ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(part, part_nan) and torch.equal(dad, dad2)
    assert _rest_is_nan(xb, C) and _rest_is_nan(dab, C) and _rest_is_nan(dab2, C)
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
        dref = act.grad[0].permute(1, 2, 0) + prior[n]
        got = dad[n].float().cpu()
        assert torch.equal(got[unique], dref[unique]) and not torch.isnan(got).any(), n
        xn = x[n].double()
        # (a tied window clips to 0 everywhere: the ReLU mask zeroes whatever was routed there, dz is the prior gradient's)
        dz = dref.double() * ((xn * t[:, 1].double() + t[:, 2].double()) > 0)
        dzx = dz * (xn - t[:, 0].double()) * rstd.double()
        s1 += dz.sum((0, 1))
        s2 += dzx.sum((0, 1))
        bound += dzx.abs().sum((0, 1)).max().item() + dz.abs().sum((0, 1)).max().item()
    assert bound < 2 ** 22                                 # multiples of 1/2: every partial sum is exact in fp32
    got = part_nan.view(rows, 2, C).cpu().double().sum(0)
    assert torch.equal(got[0], s1) and torch.equal(got[1], s2)
    _check_from_partials(lib, ops, part_nan, C, s1, s2, exact=True)
    _made(rec, specs_pool(case))


# ========================================================================================================================
# 7. The head: forward, and data gradient + BatchNorm rows + weight gradient in one pass (umi_head_bwd_fused), bias gradient
# ========================================================================================================================
HEAD_CASES = [2, 4]
H0, C0 = 512, 64


def _head_rows():
    return 4096                    # umi_head_dgrad_bnred_rows per image at 512^2 x 64 (asserted in the test)


def specs_head(ncls):
    return [spec_conv_fwd(H0, C0, ncls, C0, ncls, True, False, R=1, bias=True, out32=True),
            spec_pack("conv_fwd", (ncls, C0, 1, 1), False), spec_pack("conv_dgrad", (ncls, C0, 1, 1), False),
            _spec("umi_head_bwd_fused", lddl=ncls, ldda=C0, ldybn=C0, s_co=C0, s_ci=1, out_scale=OUT_SCALE, P=H0 * H0, Ci=ncls,
                  Co=C0, dtype=F16),
            spec_from_partials(_head_rows(), C0),
            _spec("umi_colsum", ldx=ncls, out_scale=OUT_SCALE, M=H0 * H0, C=ncls, dtype=F16)]


@pytest.mark.parametrize("ncls", HEAD_CASES)
def test_head_forward_and_fused_backward_as_the_step_calls_it(ncls, monkeypatch):
    lib, ops, rec = _start(monkeypatch)
    H = W = H0
    C = C0
    g = torch.Generator().manual_seed(80 + ncls)
    ybn = _ints((N, H, W, C), -2, 2, g)                    # the raw output of up4.c2
    t, rstd = _bn_rows(C, g)
    wo = _ints((ncls, C, 1, 1), -1, 1, g)
    b = _ints((ncls,), -3, 3, g)
    dl = _ints((N, H, W, ncls), -1, 1, g)
    act = _apply(ybn, t)
    assert N * H * W * act.abs().max().item() * 2 < 2 ** 24      # multiples of 1/2: the weight gradient's sums are exact
    yd, td, rsd, wod, dld = ybn.half().to(DEV), t.to(DEV).contiguous(), rstd.to(DEV), wo.to(DEV), dl.half().to(DEV)
    logits = _nan(N, H, W, ncls, dtype=torch.float32)
    ops.conv_fwd(yd, td, lambda l: ops.pack_conv_fwd(wod, torch.float16, k8=bool(l)), b.to(DEV), logits, 1, 1, 1, 0)
    da = _nan(N, H, W, C)
    gw = _nan(ncls, C, 1, 1, dtype=torch.float32)
    gb = _nan(ncls, dtype=torch.float32)
    _nan_ws(lib.fn("umi_head_bwd_fused_ws_bytes")(N * H * W, ncls, C))
    part = ops.head_dgrad_bnred(dld, ops.pack_conv_dgrad(wod, torch.float16, k8=False), da, yd, td, rsd, dW=gw, out_scale=OUT_SCALE)
    assert part is not None
    rows = part.numel() // (2 * C)
    assert rows == N * _head_rows()
    ops.colsum(dld, gb, OUT_SCALE)
    torch.cuda.synchronize()
    s1 = torch.zeros(C, dtype=torch.float64)
    s2 = torch.zeros(C, dtype=torch.float64)
    bound = 0.0
    for n in range(N):
        an = act[n].permute(2, 0, 1)[None]
        assert torch.equal(logits[n].cpu(), F.conv2d(an, wo, b)[0].permute(1, 2, 0)), n
        dref = F.conv_transpose2d(dl[n].permute(2, 0, 1)[None], wo)[0].permute(1, 2, 0)
        assert torch.equal(da[n].float().cpu(), dref), n
        yb = ybn[n].double()
        dz = dref.double() * ((yb * t[:, 1].double() + t[:, 2].double()) > 0)
        dzx = dz * (yb - t[:, 0].double()) * rstd.double()
        s1 += dz.sum((0, 1))
        s2 += dzx.sum((0, 1))
        bound += dzx.abs().sum((0, 1)).max().item() + dz.abs().sum((0, 1)).max().item()
    assert bound < 2 ** 22                                 # multiples of 1/2: every partial sum of a row, and of the totals, is exact
    got = part.view(rows, 2, C).cpu().double().sum(0)
    assert torch.equal(got[0], s1) and torch.equal(got[1], s2)
    _check_from_partials(lib, ops, part, C, s1, s2, exact=True)
    assert torch.equal(gw.cpu().double(), _wgrad_ref(act, dl, 1, 0) * OUT_SCALE)
    assert torch.equal(gb.cpu().double(), dl.double().sum((0, 1, 2)) * OUT_SCALE)
    _made(rec, specs_head(ncls))


# ========================================================================================================================
# 8. The stem's forward and statistics rows for one and three input channels
# ========================================================================================================================
STEM_CASES = [1, 3]
STEM_ROWS = 256                    # statistics rows per image of the narrow-input kernel at 512^2 (asserted in the test)


def specs_stem(cin):
    return [spec_conv_fwd(H0, cin, C0, cin, C0, False, True), spec_pack("conv_fwd", (C0, cin, 3, 3), False),
            spec_finalize(STEM_ROWS, C0, H0 * H0)]


@pytest.mark.parametrize("cin", STEM_CASES)
def test_stem_forward_and_rows_as_the_step_calls_it(cin, monkeypatch):
    lib, ops, rec = _start(monkeypatch)
    H = W = H0
    C = C0
    g = torch.Generator().manual_seed(90 + cin)
    x = _ints((N, H, W, cin), -1, 1, g)
    w = _ints((C, cin, 3, 3), -1, 1, g)
    xd = x.half().to(DEV)
    y = _nan(N, H, W, C)
    lay, rows = ops.conv_plan(xd, y, 3, 3, 1, 1)
    assert rows == N * STEM_ROWS                           # (the narrow-input kernel reads the generic weight packing)
    part = _nan(rows * 2 * C, dtype=torch.float32)
    wp = ops.pack_conv_fwd(w.to(DEV), torch.float16, k8=False)
    lib.call("umi_conv_fwd", xd.data_ptr(), cin, None, wp.data_ptr(), None, y.data_ptr(), C, part.data_ptr(), N, H, W, cin, C,
             3, 3, 1, 1, H, W, 0, 0, H, W, F16, F16, 0, ops._stream())
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
    _check_finalize(ops, part, C, N * H * W, s1, s2)
    _made(rec, specs_stem(cin))


# ========================================================================================================================
# 9. Stage 3 of the BatchNorm backward on the halves of concat buffers (the encoder's second convolutions above 64 channels)
# ========================================================================================================================
APPLY_CASES = [(256, 128), (128, 256), (64, 512)]


def specs_apply(case):
    H, C = case
    return [_spec("umi_bn_bwd_apply", ldda=2 * C, ldy=2 * C, M=H * H, C=C, dtype=F16)]


@pytest.mark.parametrize("case", APPLY_CASES)
def test_bn_backward_apply_on_concat_slices(case, monkeypatch):
    lib, ops, rec = _start(monkeypatch)
    H, C = case
    W = H
    g = torch.Generator().manual_seed(H + C + 9)
    da = _ints((N, H, W, C), -1, 1, g)
    y = _ints((N, H, W, C), -1, 1, g)
    tb, rstd, c1, c2, sums = _dyadic_bn_backward(C, N * H * W, g)
    dz = _dz_ref(da, y, tb, rstd, c1, c2)
    assert dz.abs().max().item() <= 4 and torch.equal(dz * 4, (dz * 4).round())       # exact in fp16
    dab, dad = _slice_of_nan(da, 2 * C)
    yb, yd = _slice_of_nan(y, 2 * C)
    sd = sums.to(DEV)
    ops.bn_bwd_apply(dad, yd, tb.to(DEV).contiguous(), rstd.to(DEV), sd[0], sd[1])
    torch.cuda.synchronize()
    assert torch.equal(dad.float().cpu(), dz)
    assert _rest_is_nan(dab, C) and _rest_is_nan(yb, C) and torch.equal(yd.float().cpu(), y)
    _made(rec, specs_apply(case))


# ========================================================================================================================
# 10. The dice_bce_mc loss kernels at 512^2: 512 and 1024 partial rows through the float64 finalize
# ========================================================================================================================
# images, classes, target dtype: the two benchmark configurations as the step calls them (float labels), class-index labels, and
# N = 4: 1,048,576 pixels, the smallest size at which the kernel's row count reaches its cap of 1024
LOSS_CASES = [(2, 2, torch.float32), (2, 4, torch.float32), (2, 4, torch.int64), (4, 2, torch.float32)]
TARGET_CODE = {torch.int64: 0, torch.float32: 1}


def specs_loss(case):
    n, C, tdt = case
    return [_spec("umi_dice_ce_fwd", target_dtype=TARGET_CODE[tdt], C=C, HW=H0 * H0),
            _spec("umi_dice_ce_bwd", target_dtype=TARGET_CODE[tdt], C=C, HW=H0 * H0)]


def _nan_bytes(nbytes):
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("case", LOSS_CASES, ids=[f"{n}x{C}-{str(t)[6:]}" for n, C, t in LOSS_CASES])
def test_dice_ce_kernels_at_bench_size(case, monkeypatch):
    """umi_dice_ce_fwd / umi_dice_ce_bwd against the float64 composite of test_fused_dice_ce_loss_matches_composite, with that test's
    bounds: 2e-6 max(1, |ref|) on the loss and on each of the 3 C + 1 sums, 2e-5 max |grad| on the gradient.  stats, workspace and
    gradient are preset to NaN bytes with guard bytes behind them.  The worst ratios error / bound are printed; measured on an
    MI355X: sums 0.030, loss 0.014, gradient 0.019 (C = 4), and no larger at 1024 rows (N = 4) than at 512."""
    lib, ops, rec = _start(monkeypatch)
    n, C, tdt = case
    HW = H0 * H0
    K = 3 * C + 2
    g = torch.Generator().manual_seed(100 + n + C)
    logits = 3.0 * torch.randn(n, C, HW, generator=g)
    classes = torch.randint(0, C, (n, HW), generator=g)
    ld, td = logits.to(DEV), classes.to(tdt).to(DEV)
    need = lib.fn("umi_dice_ce_ws_bytes")(n, C, HW)
    rows = min(1024, n * HW // 1024)
    assert need == rows * (3 * C + 1) * 4 and rows == (512 if n == 2 else 1024)
    ws, stats, dl = _nan_bytes(need + GUARD), _nan_bytes(K * 4 + GUARD), _nan_bytes(n * C * HW * 4 + GUARD)
    gout = torch.tensor(1.7, device=DEV)
    lib.call("umi_dice_ce_fwd", ld.data_ptr(), td.data_ptr(), TARGET_CODE[tdt], n, C, HW, stats.data_ptr(), ws.data_ptr(), need,
             ops._stream())
    lib.call("umi_dice_ce_bwd", ld.data_ptr(), td.data_ptr(), TARGET_CODE[tdt], stats.data_ptr(), gout.data_ptr(), n, C, HW,
             dl.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert bool((ws[need:] == 0xFF).all()) and bool((stats[K * 4:] == 0xFF).all()) and bool((dl[n * C * HW * 4:] == 0xFF).all())
    assert not bool(torch.isnan(ws[:need].view(torch.float32)).any())               # every row was written
    got = stats[:K * 4].view(torch.float32).cpu().double()
    grad = dl[:n * C * HW * 4].view(torch.float32).view(n, C, HW).cpu().double()
    ref_in = logits.double().requires_grad_(True)
    ce_sum = F.cross_entropy(ref_in, classes, reduction="sum")
    p = torch.softmax(ref_in, 1)
    oh = F.one_hot(classes, C).movedim(-1, 1).double()
    sA, sB, sT = (p * oh).sum((0, 2)), (p * p).sum((0, 2)), oh.sum((0, 2))
    dice = (1 - (2 * sA + 1e-5) / (sB + sT + 1e-5)).sum()
    ref = 0.5 * ce_sum / (n * HW) + 0.5 * dice / C
    (ref * 1.7).backward()
    want = torch.cat([sA, sB, sT, ce_sum[None], ref[None]]).detach()
    ratio = ((got - want).abs() / (2e-6 * want.abs().clamp_min(1.0)))
    gmax = ref_in.grad.abs().max().item()
    gratio = (grad - ref_in.grad).abs().max().item() / (2e-5 * gmax)
    print(f"[loss bound] N={n} C={C} {tdt}: sums worst {ratio[:-1].max().item():.3g}, loss {ratio[-1].item():.3g}, "
          f"gradient {gratio:.3g} (of 1)")
    assert ratio.max().item() < 1.0, ratio.tolist()
    assert torch.isfinite(grad).all() and gratio < 1.0
    _made(rec, specs_loss(case))


def all_specs():
    """Every call these tables pin."""
    out = []
    for cases, fn in ((FWD_CASES, specs_fwd), (DGRAD_CASES, specs_dgrad), (WGRAD_CASES, specs_wgrad), (BNAPPLY_CASES, specs_bnapply),
                      (UP_CASES, specs_up), (POOL_CASES, specs_pool), (HEAD_CASES, specs_head), (STEM_CASES, specs_stem),
                      (APPLY_CASES, specs_apply), (LOSS_CASES, specs_loss)):
        for c in cases:
            out += fn(c)
    return out
