"""The dropout kernels against the NumPy statement of their random stream (tests/dropout_stream.py) and float64 values.

Three hand-kept copies of the generator exist (dropout_kernel in transformer_kernels.hip, dropout8_kernel / dropout8_fused_kernel
in elementwise_tu_f16.hip, the epi 1 / epi 2 epilogue of conv1x1_mfma.hip); the rest of the suite only compares them with each
other.  Here every path's mask bytes must equal `keep_mask(M, C, p, seed, counter)` bit for bit -- the element index is the
dense row * C + col whatever the leading dimensions, the device counter enters as seed + counter * 0x9E3779B9, and the
grid-stride trips past the grid caps (16,384 blocks of 256 threads: 33,554,432 elements on the vector kernel, 4,194,304 on
the scalar one) index like the first -- and every value must be keep ? f(x) / (1 - p) : 0 in float64, elementwise, with the
`|y - ref| <= (a |ref| + b s) u + floor` bounds of tests/test_gpu_tu_fullsize.py (each b states its measured worst case).

Not covered here: element counts of 2^32 and more (an 8 GB fp16 tensor); the high word of the index is pinned on the CPU
statement only (tests/test_dropout_stream.py)."""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

from tests import dropout_stream as D

pytestmark = pytest.mark.gpu
DEV = "cuda"
U16, U32 = 2.0 ** -11, 2.0 ** -24
SUB16 = 2.0 ** -25                   # half the fp16 subnormal spacing: the absolute floor of rounding to fp16
PS = (0.1, 0.25, 0.5)
SEEDS = (12345, 0x7FFFFFF3, 0x9ABCDEF1)          # the last one is >= 2^31
COUNTERS = (None, 0, 1, -2147483643)             # no device counter, then int32 device scalars (the last wraps as uint32)
F16, F32 = torch.float16, torch.float32


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from umi import lib, ops, ops_tu
    return lib, ops, ops_tu


def _nan(*shape, dtype=torch.float16):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _check(name, y, ref, s, a, b, u, floor=0.0):
    """|y - ref| <= (a |ref| + b s) u + floor, elementwise.  Prints the measured b: max over elements of
    (|y - ref| - a |ref| u - floor) / (s u), so that a bound's comment can record its worst case."""
    y = y.double()
    assert torch.isfinite(y).all(), f"{name}: non-finite (unwritten?) elements"
    err = (y - ref).abs()
    lim = (a * ref.abs() + b * s) * u + floor
    bad = err > lim
    used = ((err - a * ref.abs() * u - floor).clamp_min(0) / (s * u).clamp_min(1e-300)).max().item()
    print(f"[bound] {name}: b measured {used:.3g}, bound {b}")
    if bad.any():
        i = bad.nonzero()[0].tolist()
        pytest.fail(f"{name}: {int(bad.sum())} elements out of bound; first at {i}: got {y[tuple(i)].item()!r}, "
                    f"ref {ref[tuple(i)].item()!r}, s {s[tuple(i)].item() if s.dim() else s.item()!r}; measured b {used:.3g}")
    return used


def _kernels(fn):
    """Names of the device kernels `fn` launches (the premise checks: which path ran)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return " ".join(e.name for e in prof.events())


@functools.lru_cache(maxsize=2)
def _uniform(n, eff_seed):
    return D.uniform(n, eff_seed)        # computed once per stream; every p thresholds the same u


def _keep(M, C, p, seed, counter=None):
    """keep_mask(M, C, p, seed, counter) as a device uint8 tensor [M * C]."""
    return torch.from_numpy(D.keep_of(_uniform(M * C, D.effective_seed(seed, counter)), p)).to(DEV)


def _ctr(counter):
    return None if counter is None else torch.tensor([counter], dtype=torch.int32, device=DEV)


def _scale64(p):
    return 1.0 / (1.0 - float(np.float32(p)))          # the kernel receives p as a float


def _assert_mask(tag, mask, M, C, p, seed, counter):
    want = _keep(M, C, p, seed, counter)
    if not torch.equal(mask, want):
        i = int((mask != want).nonzero()[0])
        pytest.fail(f"{tag}: {int((mask != want).sum())} of {M * C} mask bytes differ from the stated stream, first at element "
                    f"{i} (row {i // C}, col {i % C}): got {int(mask[i])}, want {int(want[i])}")
    return want


def _tx_rows(g, C):
    """Consumer transform rows (BatchNorm + ReLU folded): max(v * scale + shift, 0)."""
    return torch.stack([torch.zeros(C, device=DEV), 0.5 + torch.rand(C, generator=g, device=DEV),
                        0.2 * torch.randn(C, generator=g, device=DEV), torch.zeros(C, device=DEV)], 1).contiguous()


def _tx64(x64, tx):
    if tx is None:
        return x64
    t = tx.double()
    return torch.maximum(x64 * t[:, 1] + t[:, 2], t[:, 3])


def _gelu64(u):
    return u * 0.5 * (1 + torch.erf(u / math.sqrt(2)))


def _dgelu64(u):
    return 0.5 * (1 + torch.erf(u / math.sqrt(2))) + u * torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)


def _check_plain(tag, y, x, tx, keep, p):
    """y = keep ? tx(x) / (1 - p) : 0.  fp32 arithmetic: one fmaf for tx, then 1 - p, its reciprocal and the product (a
    rounding each), and the fp32 product is rounded again on the way to fp16: b <= 5 u32 of |ref| next to the output's own
    rounding.  Measured b 0 (fp16: nothing beyond the output's own rounding) / 1.57 (fp32), bound 5.  Dropped elements are
    exactly 0."""
    k = keep.view(x.shape).bool()
    ref = torch.where(k, _tx64(x.double(), tx) * _scale64(p), 0.0)
    assert torch.equal(y[~k], torch.zeros_like(y[~k])), f"{tag}: a dropped element is not exactly 0"
    if y.dtype == F16:
        return _check(tag, y, ref, ref.abs(), U16 / U32, 5, U32, SUB16)
    return _check(tag, y, ref, ref.abs(), 1, 5, U32)


# ========================================================================================================================
# 1. umi_dropout: mask bytes and forward values on the vector fp16 kernel and on the scalar kernel (fp32; fp16 with C % 8)
# ========================================================================================================================
# (dtype, M, C, vector kernel?)
PLAIN_SHAPES = [(F16, 1, 8, True), (F16, 77, 8, True), (F16, 197, 3072, True),
                (F16, 4100, 8192, True),          # 33,587,200 elements: 4,198,400 vectors, past the 16,384 x 256 grid
                (F32, 126, 16, False),
                (F32, 4099, 1027, False),         # 4,209,673 elements, past the scalar kernel's 4,194,304 threads
                (F16, 2050, 2052, False)]         # 4,206,600 elements, C % 8 != 0: fp16 on the scalar kernel, past its grid


@pytest.mark.parametrize("dtype,M,C,vec", PLAIN_SHAPES, ids=lambda v: str(v).replace("torch.", ""))
def test_dropout_mask_is_the_stated_stream_and_values_are_float64(dtype, M, C, vec):
    lib, ops, T = _gpu()
    g = torch.Generator(device=DEV).manual_seed(M + C)
    x = (torch.randn(1, 1, M, C, generator=g, device=DEV) * 2).to(dtype)
    tx = _tx_rows(g, C)
    y, mask = _nan(1, 1, M, C, dtype=dtype), torch.empty(M * C, dtype=torch.uint8, device=DEV)
    names = _kernels(lambda: T.dropout(x, y, mask, False, 0.5, 1))
    assert ("dropout8_kernel" in names) == vec and ("dropout_kernel" in names) != vec, f"premise: which kernel runs: {names}"
    if M * C > 1 << 25:      # the big case: two streams (a reference hash of 33 M elements costs a second)
        combos = [(SEEDS[0], None), (SEEDS[2], COUNTERS[3])]
    else:
        combos = list(itertools.product(SEEDS, COUNTERS))
    worst = 0.0
    for i, ((seed, counter), p) in enumerate(itertools.product(combos, PS)):
        use_tx = tx if i % 2 else None          # both forms at every p: the order is combos x ps, three ps per combo
        y.fill_(float("nan"))
        mask.fill_(7)
        T.dropout(x, y, mask, False, p, seed, use_tx, seed_dev=_ctr(counter))
        tag = f"dropout {M}x{C} p={p} seed={seed:#x} ctr={counter} tx={use_tx is not None}"
        keep = _assert_mask(tag, mask, M, C, p, seed, counter)
        if i < 2 * len(PS) or M * C <= 1 << 20:  # the values do not depend on the stream: every combo only where it is cheap
            worst = max(worst, _check_plain(tag, y, x, use_tx, keep, p))
    print(f"[bound] dropout {M}x{C} {dtype}: worst measured b {worst:.3g}")


def test_every_path_draws_the_same_mask():
    """(M, C, p, seed, counter) fixes the mask: the vector kernel, the scalar kernel in fp32 and in fp16 (a view whose ld % 8
    != 0), the fused kernel and the GEMM epilogue write identical bytes."""
    lib, ops, T = _gpu()
    M, Ci, C = 77, 64, 192
    g = torch.Generator(device=DEV).manual_seed(1)
    x16 = torch.randn(1, 1, M, C, generator=g, device=DEV).half()
    wide = torch.zeros(1, 1, M, C + 4, device=DEV, dtype=F16)
    wide[..., :C] = x16
    xin = torch.randn(1, 1, M, Ci, generator=g, device=DEV).half()
    wp = ops.pack_conv_fwd(torch.randn(C, Ci, 1, 1, generator=g, device=DEV) * Ci ** -0.5, F16, k8=True)
    for p, seed, counter in ((0.1, SEEDS[2], 1), (0.25, SEEDS[0], None), (0.5, SEEDS[1], COUNTERS[3])):
        want = _keep(M, C, p, seed, counter)
        sd = _ctr(counter)
        masks = {}

        def run(name, fn, kernel, absent=None):
            m = masks[name] = torch.full((M * C,), 7, dtype=torch.uint8, device=DEV)
            names = _kernels(lambda: fn(m))
            assert kernel in names and (absent is None or absent not in names), f"premise: {name} runs {kernel}: {names}"
        y16, y32 = torch.empty_like(x16), torch.empty(1, 1, M, C, device=DEV)
        run("vector", lambda m: T.dropout(x16, y16, m, False, p, seed, seed_dev=sd), "dropout8_kernel")
        run("scalar fp32", lambda m: T.dropout(x16.float(), y32, m, False, p, seed, seed_dev=sd), "dropout_kernel", "dropout8")
        run("scalar fp16", lambda m: T.dropout(wide[..., :C], y16, m, False, p, seed, seed_dev=sd), "dropout_kernel", "dropout8")
        run("fused", lambda m: T.dropout_fused(x16, y16, m, False, p, seed, sd, None, True), "dropout8_fused_kernel")
        run("epilogue", lambda m: T.linear_fused(xin, wp, None, torch.empty_like(x16), 2, p, seed, sd, m, aux=x16),
            "conv1x1", "dropout8")
        for name, m in masks.items():
            assert torch.equal(m, want), f"{name}: mask differs from the stated stream at p={p} seed={seed:#x} ctr={counter}"


# ========================================================================================================================
# 2. umi_dropout_fused (GELU before, residual after) and umi_linear_fused (the same tail in the GEMM epilogue)
# ========================================================================================================================
def _check_fused(tag, y, x, aux, gelu, keep, p):
    """y = keep ? f(x) / (1 - p) : 0, + aux; f = GELU or identity.  The bound of test_gelu_fp16_fwd_bwd_ew8 (the output's fp16
    rounding + b u32 of |x|: 1 + erf cancels for x << 0) times 1 / (1 - p), with the residual added: s = keep |x| / (1 - p) +
    |aux|.  b: GELU 1 (as there), 1 - p, the reciprocal, the product, the fp32 add, the second rounding to fp16: 6.
    Measured b 0.24 (GELU), 0.41 (residual), 0.24 (GEMM epilogue), bound 6.  Dropped elements are exactly 0, or exactly aux."""
    k = keep.view(x.shape).bool()
    x64 = x.double()
    sc = _scale64(p)
    ref = torch.where(k, (_gelu64(x64) if gelu else x64) * sc, 0.0)
    s = torch.where(k, x64.abs() * sc, 0.0)
    if aux is not None:
        ref, s = ref + aux.double(), s + aux.double().abs()
        assert torch.equal(y[~k], aux[~k]), f"{tag}: a dropped element is not exactly the residual"
    else:
        assert torch.equal(y[~k], torch.zeros_like(y[~k])), f"{tag}: a dropped element is not exactly 0"
    return _check(tag, y, ref, s, U16 / U32, 6, U32, SUB16)


FUSED_SHAPES = [(77, 64, 192), (300, 256, 128)]          # (M, Ci, Co): a ragged M tile of the GEMM; several tiles


@pytest.mark.parametrize("M,Ci,Co", FUSED_SHAPES)
@pytest.mark.parametrize("gelu,with_add", [(True, False), (False, True), (True, True)])
def test_dropout_fused_mask_and_values(M, Ci, Co, gelu, with_add):
    lib, ops, T = _gpu()
    C = Co
    g = torch.Generator(device=DEV).manual_seed(M + 2 * gelu + with_add)
    x = (torch.randn(1, 1, M, C, generator=g, device=DEV) * 2.5).half()
    x[0, 0, ::7] = (torch.rand(len(x[0, 0, ::7]), C, generator=g, device=DEV) * 20 - 10).half()      # |x| up to 10
    aux = torch.randn(1, 1, M, C, generator=g, device=DEV).half() if with_add else None
    y, mask = _nan(1, 1, M, C), torch.empty(M * C, dtype=torch.uint8, device=DEV)
    names = _kernels(lambda: T.dropout_fused(x, y, mask, False, 0.5, 1, None, aux, gelu))
    assert "dropout8_fused_kernel" in names, f"premise: the fused kernel: {names}"
    worst = 0.0
    for (seed, counter), p in itertools.product(itertools.product(SEEDS, COUNTERS), PS):
        y.fill_(float("nan"))
        mask.fill_(7)
        assert T.dropout_fused(x, y, mask, False, p, seed, _ctr(counter), aux, gelu)
        tag = f"fused {M}x{C} gelu={gelu} add={with_add} p={p} seed={seed:#x} ctr={counter}"
        keep = _assert_mask(tag, mask, M, C, p, seed, counter)
        worst = max(worst, _check_fused(tag, y, x, aux, gelu, keep, p))
    print(f"[bound] fused {M}x{C} gelu={gelu} add={with_add}: worst measured b {worst:.3g}")


@pytest.mark.parametrize("M,Ci,Co", FUSED_SHAPES)
def test_linear_fused_mask_and_values(M, Ci, Co):
    """The GEMM epilogue's mask against the stated stream directly (tests/test_gpu_kernels_tu.py ties it to umi_dropout_fused
    only), and its values against float64 on the fp16 pre-activation the plain GEMM stores (the epilogue's own input)."""
    lib, ops, T = _gpu()
    g = torch.Generator(device=DEV).manual_seed(M + Ci)
    x = torch.randn(1, 1, M, Ci, device=DEV, generator=g).half()
    w = torch.randn(Co, Ci, 1, 1, device=DEV, generator=g) * 2 * Ci ** -0.5
    b = torch.randn(Co, device=DEV, generator=g) * 0.1
    res = torch.randn(1, 1, M, Co, device=DEV, generator=g).half()
    pre = _nan(1, 1, M, Co)
    lay, _ = ops.conv_plan(x, pre, 1, 1, 1, 0, has_bias=True)
    assert lay == 1, "premise: the pointwise matrix-core kernel"
    wp = ops.pack_conv_fwd(w, F16, k8=True)
    ops.conv_fwd(x, None, lambda l: wp, b, pre, 1, 1, 1, 0)
    worst = 0.0
    for (seed, counter), p in itertools.product(itertools.product(SEEDS, COUNTERS), PS):
        for epi in (1, 2):
            yf, y2 = _nan(1, 1, M, Co), (_nan(1, 1, M, Co) if epi == 1 else None)
            mask = torch.full((M * Co,), 7, dtype=torch.uint8, device=DEV)
            assert T.linear_fused(x, wp, b, yf, epi, p, seed, _ctr(counter), mask, aux=res if epi == 2 else None, y2=y2)
            tag = f"linear {M}x{Ci}->{Co} epi={epi} p={p} seed={seed:#x} ctr={counter}"
            keep = _assert_mask(tag, mask, M, Co, p, seed, counter)
            if epi == 1:
                assert torch.equal(yf, pre), f"{tag}: the pre-activation is the plain GEMM's"
                worst = max(worst, _check_fused(tag, y2, pre, None, True, keep, p))
            else:
                worst = max(worst, _check_fused(tag, yf, pre, res, False, keep, p))
    print(f"[bound] linear {M}x{Ci}->{Co}: worst measured b {worst:.3g}")


# ========================================================================================================================
# 3. Leading dimensions: x, y and aux are channel slices of wider buffers; the mask stays dense (e = r * 64 + c)
# ========================================================================================================================
@pytest.mark.parametrize("dtype", [F16, F32], ids=["fp16", "fp32"])
def test_strided_views_keep_the_dense_element_index(dtype):
    lib, ops, T = _gpu()
    M, C, p, seed, counter = 203, 64, 0.25, SEEDS[2], 1
    g = torch.Generator(device=DEV).manual_seed(6)
    xw = (torch.randn(1, 1, M, 192, generator=g, device=DEV) * 2).to(dtype)
    aw = torch.randn(1, 1, M, 192, generator=g, device=DEV).to(dtype)
    x, aux = xw[..., 64:128], aw[..., 128:192]
    tx = _tx_rows(g, C)
    forms = [("plain", None, False, None), ("tx", tx, False, None)]
    if dtype == F16:
        forms += [("gelu", None, True, None), ("add", None, False, aux), ("gelu+add", None, True, aux)]
    for name, txr, gelu, a in forms:
        yw = _nan(1, 1, M, 128, dtype=dtype)
        y = yw[..., 32:96]
        mask = torch.full((M * C + 64,), 7, dtype=torch.uint8, device=DEV)
        if gelu or a is not None:
            names = _kernels(lambda: T.dropout_fused(x, y, mask, False, p, seed, _ctr(counter), a, gelu))
            assert "dropout8_fused_kernel" in names, names
        else:
            names = _kernels(lambda: T.dropout(x, y, mask, False, p, seed, txr, seed_dev=_ctr(counter)))
            assert ("dropout8_kernel" if dtype == F16 else "dropout_kernel") in names, names
        tag = f"strided {name} {dtype}"
        keep = _assert_mask(tag, mask[:M * C], M, C, p, seed, counter)
        assert (mask[M * C:] == 7).all(), f"{tag}: bytes past the mask's M * C were written"
        if gelu or a is not None:
            _check_fused(tag, y, x, a, gelu, keep, p)
        else:
            _check_plain(tag, y, x, txr, keep, p)
        assert torch.isnan(yw[..., :32]).all() and torch.isnan(yw[..., 96:]).all(), f"{tag}: wrote outside the slice"
        # backward through the same views: dx lands in its slice only, the mask is read densely
        gw = torch.randn(1, 1, M, 192, generator=g, device=DEV).to(dtype)
        dxw = _nan(1, 1, M, 128, dtype=dtype)
        before = mask.clone()
        if gelu:
            assert T.dropout_fused(gw[..., 64:128], dxw[..., 32:96], mask, True, p, 0, None, x, True)
        else:
            T.dropout(gw[..., 64:128], dxw[..., 32:96], mask, True, p, 0)
        assert torch.equal(mask, before), f"{tag}: the backward wrote the mask"
        _check_bwd(tag + " bwd", dxw[..., 32:96], gw[..., 64:128], x if gelu else None, keep, p)
        assert torch.isnan(dxw[..., :32]).all() and torch.isnan(dxw[..., 96:]).all(), f"{tag}: backward wrote outside the slice"


# ========================================================================================================================
# 4. Backward: dx = g * mask / (1 - p) (* GELU'(aux)), the mask is only read
# ========================================================================================================================
def _check_bwd(tag, dx, gy, pre, keep, p):
    """dx = keep ? g / (1 - p) : 0, times GELU'(pre) in the fused form.  Plain: the three roundings of the scale and the
    second rounding to fp16, b <= 5 u32 of |ref| as in the forward (measured 0 fp16 / 0.75 fp32).  GELU form: the bound of
    test_gelu_fp16_fwd_bwd_ew8's backward (b u32 of |g| (1 + |pre|): the 1 + erf cancellation and __expf) times 1 / (1 - p);
    b: GELU' 1 (as there), 1 - p, the reciprocal, two products, the second rounding: 6.  Measured b 0.038, bound 6."""
    k = keep.view(gy.shape).bool()
    sc = _scale64(p)
    g64 = gy.double()
    assert torch.equal(dx[~k], torch.zeros_like(dx[~k])), f"{tag}: the gradient of a dropped element is not exactly 0"
    if pre is None:
        ref = torch.where(k, g64 * sc, 0.0)
        if dx.dtype == F16:
            return _check(tag, dx, ref, ref.abs(), U16 / U32, 5, U32, SUB16)
        return _check(tag, dx, ref, ref.abs(), 1, 5, U32)
    u64 = pre.double()
    ref = torch.where(k, g64 * sc * _dgelu64(u64), 0.0)
    return _check(tag, dx, ref, torch.where(k, g64.abs() * sc * (1 + u64.abs()), 0.0), U16 / U32, 6, U32, SUB16)


@pytest.mark.parametrize("dtype,M,C", [(F16, 197, 3072), (F16, 77, 8), (F32, 126, 16), (F16, 126, 20), (F32, 4099, 1027)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_dropout_backward_against_float64_and_mask_untouched(dtype, M, C):
    lib, ops, T = _gpu()
    g = torch.Generator(device=DEV).manual_seed(M * 3 + C)
    gy = torch.randn(1, 1, M, C, generator=g, device=DEV).to(dtype)
    for p in PS:
        keep = _keep(M, C, p, SEEDS[1], 2)
        mask = keep.clone()
        dx = _nan(1, 1, M, C, dtype=dtype)
        names = _kernels(lambda: T.dropout(gy, dx, mask, True, p, 0))
        assert ("dropout8_kernel" in names) == (dtype == F16 and C % 8 == 0), names
        dx.fill_(float("nan"))
        T.dropout(gy, dx, mask, True, p, 0, seed_dev=_ctr(5))          # neither seed nor counter enters the backward
        assert torch.equal(mask, keep), "the backward wrote the mask"
        _check_bwd(f"bwd {M}x{C} {dtype} p={p}", dx, gy, None, keep, p)


@pytest.mark.parametrize("M,C", [(197, 3072), (77, 192)])
def test_gelu_dropout_backward_against_float64_and_mask_untouched(M, C):
    lib, ops, T = _gpu()
    g = torch.Generator(device=DEV).manual_seed(M + C)
    pre = (torch.randn(1, 1, M, C, generator=g, device=DEV) * 2.5).half()
    pre[0, 0, ::7] = (torch.rand(len(pre[0, 0, ::7]), C, generator=g, device=DEV) * 20 - 10).half()
    gy = torch.randn(1, 1, M, C, generator=g, device=DEV).half()
    for p in PS:
        keep = _keep(M, C, p, SEEDS[2], None)
        mask = keep.clone()
        dx = _nan(1, 1, M, C)
        assert T.dropout_fused(gy, dx, mask, True, p, 0, None, pre, True)
        assert torch.equal(mask, keep), "the backward wrote the mask"
        _check_bwd(f"gelu bwd {M}x{C} p={p}", dx, gy, pre, keep, p)


# ========================================================================================================================
# 5. p = 1 (nn.Dropout(1.0) is legal): zeros, or the residual; zero gradients; nothing non-finite; no error
# ========================================================================================================================
@pytest.mark.parametrize("dtype,C", [(F16, 64), (F16, 20), (F32, 16)], ids=["fp16-vector", "fp16-scalar", "fp32"])
def test_p_one_at_op_level(dtype, C):
    lib, ops, T = _gpu()
    M = 77
    g = torch.Generator(device=DEV).manual_seed(C)
    x = (torch.randn(1, 1, M, C, generator=g, device=DEV) * 3).to(dtype)
    x[0, 0, 0, 0] = 0.0                                   # 0 * (1 / (1 - p)) would be NaN if the scale were multiplied in
    aux = torch.randn(1, 1, M, C, generator=g, device=DEV).to(dtype)
    gy = torch.randn(1, 1, M, C, generator=g, device=DEV).to(dtype)
    zero = torch.zeros_like(x)
    for counter in (None, 1):
        y, mask = _nan(1, 1, M, C, dtype=dtype), torch.full((M * C,), 7, dtype=torch.uint8, device=DEV)
        T.dropout(x, y, mask, False, 1.0, SEEDS[2], _tx_rows(g, C), seed_dev=_ctr(counter))
        assert torch.equal(y, zero) and not mask.any()
        dx = _nan(1, 1, M, C, dtype=dtype)
        T.dropout(gy, dx, mask, True, 1.0, 0)
        assert torch.equal(dx, zero)
        if dtype == F16 and C % 8 == 0:
            for gelu, a in ((True, None), (False, aux), (True, aux)):
                y.fill_(float("nan"))
                mask.fill_(7)
                assert T.dropout_fused(x, y, mask, False, 1.0, SEEDS[0], _ctr(counter), a, gelu)
                assert torch.equal(y, zero if a is None else a) and not mask.any()
            dx.fill_(float("nan"))
            assert T.dropout_fused(gy, dx, mask, True, 1.0, 0, None, x, True)
            assert torch.equal(dx, zero)


def _grads_zero_and_finite(tape, acts):
    for a in acts:
        assert a.grad is not None and torch.equal(a.grad, torch.zeros_like(a.grad))
    for _, gp in tape.param_grads.values():
        assert torch.isfinite(gp).all() and not gp.any(), "a parameter gradient behind Dropout(1.0) is not zero"


def test_p_one_through_both_tapes():
    lib, ops, T = _gpu()
    from umi.graph import Tape
    from umi.graph_tu import TUTape
    g = torch.Generator(device=DEV).manual_seed(3)
    ctr = _ctr(1)
    # U-Net tape: dropout of a lazily-activated value
    for dtype in (F16, F32):
        tape = Tape(dtype, training=True, record=True, seed=99, seed_dev=ctr)
        a = tape.input_nhwc(torch.randn(2, 9, 7, 16, generator=g, device=DEV).to(dtype), _tx_rows(g, 16), needs_grad=True)
        o = tape.dropout(a, 1.0)
        assert torch.equal(o.raw, torch.zeros_like(o.raw))
        o.grad = torch.randn(2, 9, 7, 16, generator=g, device=DEV).to(dtype)
        tape.backward()
        _grads_zero_and_finite(tape, [a])
    # TransUNet tape: plain, GELU, residual; then the two linears with their tails in the GEMM epilogue
    M, Ci, Co = 300, 256, 128
    for gelu, with_add in ((False, False), (True, False), (False, True)):
        tape = TUTape(F16, training=True, record=True, seed=99, seed_dev=ctr)
        a = tape.input_nhwc(torch.randn(1, 1, M, Co, generator=g, device=DEV).half(), None, needs_grad=True)
        r = tape.input_nhwc(torch.randn(1, 1, M, Co, generator=g, device=DEV).half(), None, needs_grad=True)
        o = tape.dropout(a, 1.0, gelu=gelu, add=r if with_add else None)
        assert torch.equal(o.raw, r.raw if with_add else torch.zeros_like(o.raw))
        o.grad = gy = torch.randn(1, 1, M, Co, generator=g, device=DEV).half()
        tape.backward()
        _grads_zero_and_finite(tape, [a])
        if with_add:
            assert torch.equal(r.grad, gy)
    w = torch.nn.Parameter(torch.randn(Co, Ci, generator=g, device=DEV) * Ci ** -0.5)
    b = torch.nn.Parameter(torch.randn(Co, generator=g, device=DEV) * 0.1)
    for gelu in (True, False):
        tape = TUTape(F16, training=True, record=True, seed=99, seed_dev=ctr)
        a = tape.input_nhwc(torch.randn(1, 1, M, Ci, generator=g, device=DEV).half(), None, needs_grad=True)
        r = tape.input_nhwc(torch.randn(1, 1, M, Co, generator=g, device=DEV).half(), None, needs_grad=True)
        names = _kernels(lambda: tape.linear_dropout(a, w, b, 1.0, gelu=gelu, add=None if gelu else r))
        assert "dropout8" not in names, f"premise: the tail runs in the GEMM epilogue: {names}"
        tape = TUTape(F16, training=True, record=True, seed=99, seed_dev=ctr)
        o = tape.linear_dropout(a, w, b, 1.0, gelu=gelu, add=None if gelu else r)
        assert torch.equal(o.raw, torch.zeros_like(o.raw) if gelu else r.raw)
        o.grad = gy = torch.randn(1, 1, M, Co, generator=g, device=DEV).half()
        tape.backward()
        _grads_zero_and_finite(tape, [a])
        assert len(tape.param_grads) == 2
        if not gelu:
            assert torch.equal(r.grad, gy)


# ========================================================================================================================
# 6. What the tapes pass: seeds per site, the device step counter, nothing in eval, the fused and unfused routes agree
# ========================================================================================================================
def _record_dropout_calls(monkeypatch, T):
    """Wraps ops_tu.dropout / dropout_fused / linear_fused; every FORWARD launch is recorded as a dict with the mask bytes and
    the counter value read back right after the call; backward launches are counted."""
    from umi.ops import _nhwc
    log = {"fwd": [], "bwd": 0}

    def rows(t):
        N, H, W, C, _ = _nhwc(t)
        return N * H * W, C

    def note(kind, t, mask, p, seed, seed_dev):
        M, C = rows(t)
        log["fwd"].append(dict(kind=kind, M=M, C=C, p=p, seed=seed & 0xFFFFFFFF, mask=mask[:M * C].clone(),
                               counter=None if seed_dev is None else int(seed_dev.item())))

    o_drop, o_fused, o_lin = T.dropout, T.dropout_fused, T.linear_fused

    def dropout(x, y, mask, backward, p, seed, tx=None, seed_dev=None):
        o_drop(x, y, mask, backward, p, seed, tx, seed_dev=seed_dev)
        if backward:
            log["bwd"] += 1
        else:
            note("dropout", x, mask, p, seed, seed_dev)

    def dropout_fused(x, y, mask, backward, p, seed, seed_dev=None, aux=None, gelu=False):
        ok = o_fused(x, y, mask, backward, p, seed, seed_dev, aux, gelu)
        if ok and backward:
            log["bwd"] += 1
        elif ok:
            note("dropout_fused", x, mask, p, seed, seed_dev)
        return ok

    def linear_fused(x, wp8, bias, y, epi, p, seed, seed_dev, mask, aux=None, y2=None):
        ok = o_lin(x, wp8, bias, y, epi, p, seed, seed_dev, mask, aux=aux, y2=y2)
        if ok:
            note("linear_fused", y, mask, p, seed, seed_dev)
        return ok

    monkeypatch.setattr(T, "dropout", dropout)
    monkeypatch.setattr(T, "dropout_fused", dropout_fused)
    monkeypatch.setattr(T, "linear_fused", linear_fused)
    return log


def _two_training_forwards_and_eval(m, x, log, p, sites):
    """Forward + backward, a second training forward, an eval forward; returns the per-site seeds of the first forward."""
    m.train()
    m(x).square().mean().backward()
    first = log["fwd"][:]
    assert log["bwd"] == len(first) == sites, (log["bwd"], len(first), sites)
    with torch.no_grad():
        m(x)
    second = log["fwd"][len(first):]
    for step, calls in ((1, first), (2, second)):
        assert len(calls) == sites
        seeds = [c["seed"] for c in calls]
        assert len(set(seeds)) == len(seeds), f"two dropout sites of one forward share a seed: {seeds}"
        for c in calls:
            assert c["counter"] == step, f"device step counter {c['counter']} in training forward {step}"
            assert c["p"] == p
            want = _keep(c["M"], c["C"], c["p"], c["seed"], c["counter"])
            assert torch.equal(c["mask"], want), f"{c['kind']} {c['M']}x{c['C']} seed {c['seed']:#x}: not the stated stream"
    assert [c["seed"] for c in first] == [c["seed"] for c in second], "the sites' host seeds changed between steps"
    assert not any(torch.equal(a["mask"], b["mask"]) for a, b in zip(first, second)), "a step repeated a mask"
    n, nb = len(log["fwd"]), log["bwd"]
    m.eval()
    with torch.no_grad():
        m(x)
    assert len(log["fwd"]) == n and log["bwd"] == nb, "the eval forward launched a dropout kernel"
    return first


def test_unet_tape_passes_distinct_seeds_and_the_step_counter(monkeypatch):
    lib, ops, T = _gpu()
    import Model
    log = _record_dropout_calls(monkeypatch, T)
    torch.manual_seed(11)
    m = Model.UNet(1, 2, 8, True, True, 0.25, compute_dtype="fp16").to(DEV)
    sites = sum(isinstance(s, torch.nn.Dropout) for s in m.modules())
    assert sites >= 8, "premise: a dropout in every Down and Up"
    x = torch.randn(2, 1, 32, 32, device=DEV)
    first = _two_training_forwards_and_eval(m, x, log, 0.25, sites)
    assert {c["kind"] for c in first} == {"dropout"}


def test_transunet_tape_seeds_counter_and_fused_unfused_routes_agree(monkeypatch):
    lib, ops, T = _gpu()
    import loss as L
    from oracle import recipe, ref_transunet
    from TransUnet.vit_seg_modeling import VisionTransformer
    from tests.test_gpu_transunet import product_config
    log = _record_dropout_calls(monkeypatch, T)
    cfg = ref_transunet.small_config(2)
    cfg["dropout_rate"] = 0.1
    L.CLASS_NUMBER = 2
    x, _ = recipe.synthetic_batch(2, 1, 64, 64, 2, seed=9)
    sites = 1 + 2 * cfg["num_layers"]                       # the embedding's dropout, fc1 and fc2 of every block
    routes = {}
    for off in ("0", "1"):
        monkeypatch.setenv("UMI_NO_LINEAR_FUSION", off)
        log["fwd"].clear()
        log["bwd"] = 0
        torch.manual_seed(11)
        m = VisionTransformer(product_config(cfg, 64), img_size=64, num_classes=2, compute_dtype="fp16")
        m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=9, negative_gamma=False))
        m.to(DEV)
        torch.manual_seed(12)                               # the model draws its dropout base seed on its first training forward
        routes[off] = _two_training_forwards_and_eval(m, x.to(DEV), log, 0.1, sites)
    fused, unfused = routes["0"], routes["1"]
    assert {c["kind"] for c in fused} == {"dropout", "linear_fused"}, "premise: the GEMM epilogues run"
    assert {c["kind"] for c in unfused} == {"dropout", "dropout_fused"}, "premise: the separate kernels run"
    # the same site draws the same seed on either route (the `_drop_count -= 1` of the fall-backs), hence the same mask
    assert [(c["seed"], c["M"], c["C"]) for c in fused] == [(c["seed"], c["M"], c["C"]) for c in unfused]
    for a, b in zip(fused, unfused):
        assert torch.equal(a["mask"], b["mask"])
