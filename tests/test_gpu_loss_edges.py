"""dice_bce, Tversky (binary and multi-class), TopK / BCE_HEM (csrc/binary_losses.hip) and HausdorffDTLoss
(csrc/hausdorff_dt.hip) at their edges, element by element against the float64 statements of tests/loss_f64_ref.py.

Every value comparison is elementwise:  |got - ref| <= (|ref| + b s) u32 + f,  u32 = 2^-24.  `s` is the sum of the magnitudes
of the terms that make up the value before any cancellation (loss_f64_ref names it per loss), `b` the budget for the fp32
roundings inside the kernel in units of u32 of that scale, and f = 2^-126 (gradients only) the smallest normal fp32: where
expf overflows, the kernel's sigmoid is exactly 0 while the float64 one is a subnormal, and no fp32 result carries a relative
error below the normal range.  Each b is the next power of two at or above twice the worst case measured against float64 on
these seeded inputs; BOUNDS states the measurement beside it, and every check prints a `[bound]` line with what it used.

Outputs are prefilled with NaN and workspaces, stats, masks and gradients carry 4,096 guard bytes that must stay untouched.
Misaligned operands are contiguous views one float (the mask: one byte) into their buffer; they go through calc_loss where it
takes them and through the library's entry points where calc_loss would allocate the buffer itself.  Backward passes run with
(0.37 * loss).backward(); test_bare_loss_backward runs each loss once with an upstream gradient of 1.

The selection's reference keys are torch's own device arithmetic (torch.sigmoid, F.binary_cross_entropy_with_logits), and the
selected set must equal the stable argsort's at zero tolerance, no element exempt: the logits come from a coarse grid whose
positive and negative members have different magnitudes and are paired with different targets, so equal keys come from equal
(x, t) only and distinct keys are at least 2^-12 apart (asserted on the float64 keys, here and in test_loss_f64_ref.py)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import loss_f64_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U32 = 2.0 ** -24
TINY = 2.0 ** -126                   # the smallest normal fp32
GUARD = 4096                         # bytes behind every buffer a kernel writes
G = float(np.float32(0.37))          # the upstream gradient, as the fp32 scalar autograd hands to the backward
ALPHA, BETA = 0.4, 0.6               # calc_loss's Tversky weights
DEVICE_FN = {"dice_bce": "_DiceBCE", "Tversky": "_Tversky", "TopK": "_TopKBCE", "BCE_HEM": "_TopKBCE"}

# b of each bound: (bound, worst case measured on the MI355X against float64 over every case of this file).  A measured 0 means
# that no comparison left the output's own rounding |ref| u32.
# tversky_mc.grad is above 32 and explained: the kernel's softmax rounds x_c - max to fp32 before expf, an absolute error of
# |x_c - max| u32 that the exponential turns into a relative one of the same size, and these logits (3 * randn) reach
# |x_c - max| = 23.  The same arithmetic in NumPy float32 with a correctly rounded exp measures 20.6 on the same inputs
# (DESIGN.md), and 3.1 against s_i (1 + max_c |x_c - max|).
BOUNDS = {
    "dice_bce.loss": (0.25, 0.0),
    "dice_bce.grad": (4, 1.99),
    "tversky_bin.loss": (0.25, 0.102),
    "tversky_bin.grad": (8, 2.64),
    "tversky_mc.loss": (0.25, 0.0),
    "tversky_mc.grad": (64, 21.1),
    "selection.loss": (0.25, 0.114),
    "selection.grad": (4, 1.73),
    "hdt.loss": (0.125, 0.053),
    "hdt.grad": (16, 5.12),
}


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    import loss as L
    from umi import lib, ops
    return L, lib, ops


def _check(family, case, got, ref, s, g=1.0, floor=0.0):
    """|got - ref g| <= (|ref g| + b s |g|) u32 + floor, elementwise; prints the b this comparison needed."""
    b = BOUNDS[family][0]
    got, ref, s = torch.as_tensor(got).double().cpu(), torch.as_tensor(ref).double() * g, torch.as_tensor(s).double() * abs(g)
    assert got.shape == ref.shape, (family, case, got.shape, ref.shape)
    assert torch.isfinite(got).all(), f"{family} {case}: non-finite (unwritten?) elements"
    err = (got - ref).abs()
    used = ((err - ref.abs() * U32 - floor).clamp_min(0) / (s * U32).clamp_min(1e-300)).max().item()
    print(f"[bound] {family} {case}: b measured {used:.3g}, bound {b}")
    bad = err > (ref.abs() + b * s) * U32 + floor
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        pytest.fail(f"{family} {case}: {int(bad.sum())} of {bad.numel()} out of bound; first at {i}: got {got[i].item()!r}, "
                    f"ref {ref[i].item()!r}, scale {s[i].item()!r}; measured b {used:.3g}")


def _at(t, off):
    """A contiguous device copy of `t` that starts `off` elements into its buffer."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=DEV)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (off * t.element_size()) % 16
    return v


class _Guarded:
    """`n` elements of `dtype` at element offset `off` of a buffer filled with 0xFF bytes (NaN for floats), GUARD bytes
    behind them; `intact()` tells whether every byte outside the n elements still is 0xFF."""

    def __init__(self, n, dtype=torch.float32, off=0):
        size = torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full(((off + n) * size + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        self.lo, self.hi = off * size, (off + n) * size
        self.t = self.raw[self.lo:self.hi].view(dtype)
        self.ptr = self.t.data_ptr()

    def intact(self):
        return bool((self.raw[:self.lo] == 0xFF).all()) and bool((self.raw[self.hi:] == 0xFF).all())


def _kernels(fn):
    """Names of the device kernels `fn` launches."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return " ".join(e.name for e in prof.events())


def _through_calc_loss(L, lt, x, t, factor, po=0, to=0):
    """(loss, d (factor * loss) / d pred) through calc_loss on the device; the device path must have been taken."""
    xd, td = _at(x, po).requires_grad_(True), _at(t, to)
    v = L.calc_loss(xd, td, loss_type=lt)
    assert type(v.grad_fn).__name__.startswith(DEVICE_FN[lt]), (lt, type(v.grad_fn).__name__)
    (v if factor == 1.0 else factor * v).backward()
    torch.cuda.synchronize()
    return v.detach().cpu(), xd.grad.cpu()


# ========================================================================================================================
# 1. dice_bce and binary Tversky
# ========================================================================================================================
# (B, H, W, pred offset, target offset), offsets in floats
BIN_CASES = [
    (1, 1, 1, 0, 0), (2, 1, 3, 0, 0),        # a single pixel; fewer than four pixels
    (2, 64, 64, 0, 0),                       # vector path, exactly one 4,096-pixel block per image
    (2, 64, 65, 0, 0),                       # vector path, two blocks, the second nearly empty
    (2, 4097, 1, 0, 0),                      # scalar path, two blocks
    (2, 64, 64, 1, 0), (2, 64, 64, 0, 1),    # HW % 4 == 0 but one pointer 4-byte aligned: scalar path
    (300, 1, 7, 0, 0),                       # B * 5 > 1024: second trip of stats_finalize, 300-long loop of bin_coef
]
# hard: smooth logits, 0/1 targets.  edges: image 0 has an all-zero target, the last image an all-one target, image B // 2
# logits in {-100, -30, 30, 100} (saturated sigmoid, expf overflow, log1pf(0)).  soft: targets in [0, 1].  negative: targets
# in [-0.5, 1], the only input on which sum |t| (Dice) and sum t (Tversky) differ.
BIN_CONTENTS = ["hard", "edges", "soft", "negative"]


def _smooth(gen, B, H, W, scale=9.0):
    n = torch.randn(B, 1, H + 8, W + 8, generator=gen)
    return F.avg_pool2d(n, 9, stride=1) * scale


@functools.lru_cache(maxsize=None)
def bin_inputs(B, H, W, content):
    gen = torch.Generator().manual_seed(10007 * B + 101 * H + W + 7 * BIN_CONTENTS.index(content))
    x = _smooth(gen, B, H, W)
    hard = (_smooth(gen, B, H, W)[:, 0] > 0.5).float()
    u = torch.rand(B, H, W, generator=gen)
    sat = torch.tensor([-100.0, -30.0, 30.0, 100.0])[torch.randint(0, 4, (H, W), generator=gen)]
    if content == "hard":
        t = hard
    elif content == "edges":
        t = hard
        x[B // 2, 0] = sat
        t[0] = 0.0
        t[B - 1] = 1.0
    elif content == "soft":
        t = u
    else:
        t = 1.5 * u - 0.5
    return x.contiguous(), t.contiguous()


@functools.lru_cache(maxsize=None)
def bin_ref(lt, B, H, W, content):
    x, t = bin_inputs(B, H, W, content)
    return R.dice_bce(x, t) if lt == "dice_bce" else R.tversky_bin(x, t, ALPHA, BETA)


def _bin_direct(lib, ops, lt, x, t, g, po=0, to=0, do=0):
    """(loss, dpred) from the entry points on poisoned, guarded buffers; dpred `do` floats into its buffer."""
    B, HW = x.shape[0], x[0].numel()
    xd, td = _at(x, po), _at(t, to)
    need = lib.fn("umi_binloss_ws_bytes")(B, 1, HW)
    ws, stats, loss = _Guarded(need, torch.uint8), _Guarded(5 * B, torch.float64), _Guarded(1)
    dpred, gout = _Guarded(x.numel(), off=do), torch.tensor([g], dtype=torch.float32, device=DEV)
    st = ops._stream()
    if lt == "dice_bce":
        lib.call("umi_dice_bce_fwd", xd.data_ptr(), td.data_ptr(), B, HW, stats.ptr, loss.ptr, ws.ptr, need, st)
        lib.call("umi_dice_bce_bwd", xd.data_ptr(), td.data_ptr(), stats.ptr, gout.data_ptr(), B, HW, dpred.ptr, st)
    else:
        lib.call("umi_tversky_fwd", xd.data_ptr(), td.data_ptr(), 1, B, 1, HW, ALPHA, BETA, stats.ptr, loss.ptr, ws.ptr, need, st)
        lib.call("umi_tversky_bwd", xd.data_ptr(), td.data_ptr(), 1, stats.ptr, gout.data_ptr(), B, 1, HW, ALPHA, BETA,
                 dpred.ptr, st)
    torch.cuda.synchronize()
    assert ws.intact() and stats.intact() and loss.intact() and dpred.intact(), "a guard byte was written"
    return loss.t[0].cpu(), dpred.t.view(x.shape).cpu()


def _bin_family(lt):
    return "dice_bce" if lt == "dice_bce" else "tversky_bin"


@pytest.mark.parametrize("content", BIN_CONTENTS)
@pytest.mark.parametrize("case", BIN_CASES, ids=lambda c: "x".join(map(str, c[:3])) + f"+{c[3]}+{c[4]}")
@pytest.mark.parametrize("lt", ["dice_bce", "Tversky"])
def test_binary_losses_against_float64(lt, case, content):
    L, lib, ops = _gpu()
    B, H, W, po, to = case
    x, t = bin_inputs(B, H, W, content)
    if content == "negative":
        assert float(t.min()) < -0.25 and float((t.abs() - t).sum()) > 0.5          # sum |t| != sum t
    ref, fam, tag = bin_ref(lt, B, H, W, content), _bin_family(lt), f"{case} {content}"
    runs = [("calc_loss", _through_calc_loss(L, lt, x, t, G, po, to)), ("direct", _bin_direct(lib, ops, lt, x, t, G, po, to))]
    if case == (2, 64, 64, 0, 0):            # a 4-byte aligned gradient alone: vector forward, scalar backward
        runs.append(("direct, dpred + 1", _bin_direct(lib, ops, lt, x, t, G, do=1)))
    for how, (loss, grad) in runs:
        _check(fam + ".loss", f"{tag} {how}", loss, ref.loss, ref.S)
        _check(fam + ".grad", f"{tag} {how}", grad, ref.grad, ref.scale, g=G, floor=TINY)


# ========================================================================================================================
# 2. multi-class Tversky
# ========================================================================================================================
MC_DTYPES = {torch.int64: 0, torch.float32: 1, torch.uint8: 2, torch.int32: 3}
MC_SMALL = (3, 5, 7)                         # HW = 35 is no multiple of 256: blocks cross image boundaries
MC_BIG = (5, 512, 512)                       # 1,310,720 pixels: past the 1,024-block cap of mc_blocks
MC_GRID = [(C, dt, MC_SMALL) for C in range(2, 9) for dt in MC_DTYPES]
MC_GRID += [(C, dt, shape) for C in (2, 8) for shape in ((1, 1, 1), (2, 1, 63)) for dt in MC_DTYPES]
MC_GRID += [(C, torch.int64, MC_BIG) for C in (2, 8)]
# labels that equal no class, per dtype
MC_OFF_CLASS = {torch.int64: lambda C: [C, C + 3, -1], torch.int32: lambda C: [C, C + 3, -1],
                torch.uint8: lambda C: [C, C + 3, 255], torch.float32: lambda C: [C, C + 3, -1, 1.5, -0.5]}


@functools.lru_cache(maxsize=None)
def mc_inputs(C, shape, off_class_dtype=None):
    """Logits and int64-valued class labels; with `off_class_dtype`, labels of that dtype of which about 40 % match no class."""
    B, H, W = shape
    gen = torch.Generator().manual_seed(977 * C + 31 * B + H + W)
    x = 3.0 * torch.randn(B, C, H, W, generator=gen)
    labels = torch.randint(0, C, shape, generator=gen)
    if off_class_dtype is None:
        return x, labels
    off = torch.tensor(MC_OFF_CLASS[off_class_dtype](C), dtype=torch.float64)
    pick = off[torch.randint(0, len(off), shape, generator=gen)]
    labels = torch.where(torch.rand(shape, generator=gen) < 0.4, pick, labels.double()).to(off_class_dtype)
    return x, labels


@functools.lru_cache(maxsize=None)
def mc_ref(C, shape, off_class_dtype=None):
    return R.tversky_mc(*mc_inputs(C, shape, off_class_dtype), ALPHA, BETA)


def _mc_direct(lib, ops, x, labels, g):
    B, C, HW = x.shape[0], x.shape[1], x[0, 0].numel()
    xd, td, code = x.to(DEV), labels.to(DEV), MC_DTYPES[labels.dtype]
    need = lib.fn("umi_binloss_ws_bytes")(B, C, HW)
    ws, stats, loss, dpred = _Guarded(need, torch.uint8), _Guarded(3 * C, torch.float64), _Guarded(1), _Guarded(x.numel())
    gout, st = torch.tensor([g], dtype=torch.float32, device=DEV), ops._stream()
    lib.call("umi_tversky_fwd", xd.data_ptr(), td.data_ptr(), code, B, C, HW, ALPHA, BETA, stats.ptr, loss.ptr, ws.ptr, need, st)
    lib.call("umi_tversky_bwd", xd.data_ptr(), td.data_ptr(), code, stats.ptr, gout.data_ptr(), B, C, HW, ALPHA, BETA,
             dpred.ptr, st)
    torch.cuda.synchronize()
    assert ws.intact() and stats.intact() and loss.intact() and dpred.intact(), "a guard byte was written"
    return loss.t[0].cpu(), dpred.t.view(x.shape).cpu()


def _mc_compare(L, lib, ops, x, labels, ref, tag):
    for how, (loss, grad) in (("calc_loss", _through_calc_loss(L, "Tversky", x, labels, G)),
                              ("direct", _mc_direct(lib, ops, x, labels, G))):
        _check("tversky_mc.loss", f"{tag} {how}", loss, ref.loss, ref.S)
        _check("tversky_mc.grad", f"{tag} {how}", grad, ref.grad, ref.scale, g=G, floor=TINY)


def _mc_id(v):
    return str(v).replace("torch.", "") if isinstance(v, torch.dtype) else ("x".join(map(str, v)) if isinstance(v, tuple) else str(v))


@pytest.mark.parametrize("C,dtype,shape", MC_GRID, ids=_mc_id)
def test_multiclass_tversky_against_float64(C, dtype, shape):
    L, lib, ops = _gpu()
    x, labels = mc_inputs(C, shape)
    if shape == MC_BIG:
        assert labels.numel() > 1024 * 4 * 256           # more pixels than 1,024 blocks take at 4 per thread
    _mc_compare(L, lib, ops, x, labels.to(dtype), mc_ref(C, shape), f"C={C} {_mc_id(dtype)} {shape}")


@pytest.mark.parametrize("dtype", list(MC_DTYPES), ids=_mc_id)
@pytest.mark.parametrize("C", [2, 8])
def test_multiclass_labels_that_match_no_class_count_nowhere(C, dtype):
    L, lib, ops = _gpu()
    x, labels = mc_inputs(C, MC_SMALL, dtype)
    present = set(labels.double().unique().tolist())
    assert set(float(v) for v in MC_OFF_CLASS[dtype](C)) <= present and labels.dtype == dtype
    _mc_compare(L, lib, ops, x, labels, mc_ref(C, MC_SMALL, dtype), f"C={C} {_mc_id(dtype)} off-class")


# ========================================================================================================================
# 3. TopK / BCE_HEM: the exact selection, through umi_topk_loss_fwd / _bwd so that k and every pointer are free
# ========================================================================================================================
SEL_N = [1, 3, 1023, 1024, 1025, 16384, 16385, 32773]       # 16,384-element blocks; 32773: three blocks, the last one short
SEL_TIES_N, SEL_TIES_K = 32773, (16384, 16387, 32772)       # the tie rank on a block edge, 3 into block 1, one short of all
SEL_MODES = {0: "TopK", 1: "BCE_HEM"}
SEL_SEP = 2.0 ** -12


def sel_ks(N):
    return sorted({1, max(1, N // 2), N})


@functools.lru_cache(maxsize=None)
def sel_inputs(N, flip, seed=0):
    """Logits j/64 (j = 1..192) paired with one target value and -(j/64 - 1/128) paired with the other: |x| differs between
    the two signs, so the mathematically equal pairs (x, 1) / (-x, 0) never occur and equal keys come from equal (x, t)."""
    gen = torch.Generator().manual_seed(5003 * N + 17 * seed + flip)
    j = torch.randint(1, 193, (N,), generator=gen).float()
    pos = torch.rand(N, generator=gen) < 0.5
    x = torch.where(pos, j / 64, -(j / 64 - 1.0 / 128))
    t = (pos != bool(flip)).float()
    return x, t


def sel_tie_inputs(N):
    """All-zero logits: every TopK key is 0.5 and every BCE log 2."""
    return torch.zeros(N), (torch.rand(N, generator=torch.Generator().manual_seed(5)) < 0.5).float()


def sel_digit_inputs(N, e):
    """Logits j 2^-e, j = 0..255 tiled, targets all 1: keys a few fp32 ulps apart around 0.5 (TopK) or log 2 (BCE)."""
    return (torch.arange(N) % 256).float() * 2.0 ** -e, torch.ones(N)


def assert_keys_separated(x, t, mode):
    """The premise of the zero-tolerance comparison, on the float64 keys alone: one key per distinct (x, t), and distinct
    keys at least 2^-12 apart relatively -- far more than the fp32 roundings of either arithmetic can move them."""
    key = R.selection_keys(x, t, mode).numpy()
    pairs = np.stack([x.numpy().astype(np.float64), t.numpy().astype(np.float64)], axis=1)
    uniq, inv = np.unique(pairs, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    ukey = np.zeros(len(uniq))
    ukey[inv] = key
    assert np.allclose(ukey[inv], key, rtol=1e-13, atol=0)       # one key per (x, t), up to float64's own last places
    s = np.sort(ukey)
    if len(s) > 1:
        gap = np.diff(s) / np.maximum(np.abs(s[1:]), np.abs(s[:-1]))
        assert gap.min() >= SEL_SEP, gap.min()


def shared_key_digits(key32):
    """How many leading 8-bit digits of the kernel's order-preserving uint32 map all of the fp32 keys share."""
    u = key32.astype(np.float32).view(np.uint32)
    u = np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)
    return next((p for p in range(4) if len(np.unique(u >> (24 - 8 * p))) > 1), 4)


def _torch_keys(x, t, mode):
    """fp32 keys by torch on the device, smaller = taken first."""
    xd, td = x.to(DEV), t.to(DEV)
    if mode == 0:
        p = torch.sigmoid(xd)
        return torch.where(td.long() == 1, p, 1 - p).cpu().numpy()
    return -F.binary_cross_entropy_with_logits(xd, td, reduction="none").cpu().numpy()


def _want_set(x, t, k, mode):
    return np.sort(np.argsort(_torch_keys(x, t, mode), kind="stable")[:k])


def _new_ws(lib, N):
    return _Guarded(lib.fn("umi_topk_loss_ws_bytes")(N), torch.uint8)


def _sel_fwd(lib, ops, x, t, k, mode, ws, offs=(0, 0, 0)):
    """(loss, mask, device pred, device target, guarded mask) of one forward call on workspace `ws`."""
    N = x.numel()
    xd, td = _at(x, offs[0]), _at(t, offs[1])
    mask, loss = _Guarded(N, torch.uint8, off=offs[2]), _Guarded(1)
    assert xd.data_ptr() % 16 == 4 * offs[0] and td.data_ptr() % 16 == 4 * offs[1] and mask.ptr % 4 == offs[2]
    lib.call("umi_topk_loss_fwd", xd.data_ptr(), td.data_ptr(), N, k, mode, mask.ptr, loss.ptr, ws.ptr, ws.hi, ops._stream())
    torch.cuda.synchronize()
    assert ws.intact() and mask.intact() and loss.intact(), "a guard byte was written"
    return loss.t[0].cpu(), mask.t.cpu().numpy(), xd, td, mask


def _sel_bwd(lib, ops, xd, td, mask, k, g, do=0):
    dpred, gout = _Guarded(xd.numel(), off=do), torch.tensor([g], dtype=torch.float32, device=DEV)
    lib.call("umi_topk_loss_bwd", xd.data_ptr(), td.data_ptr(), mask.ptr, gout.data_ptr(), xd.numel(), k, dpred.ptr, ops._stream())
    torch.cuda.synchronize()
    assert dpred.intact() and mask.intact(), "a guard byte was written"
    return dpred.t.cpu()


def _sel_compare(lib, ops, x, t, k, mode, want, tag, ws=None, offs=(0, 0, 0), do=0):
    """One forward and backward call: the mask is exactly `want`, loss and gradient are the float64 mean over it."""
    ws = ws or _new_ws(lib, x.numel())
    loss, m, xd, td, mask = _sel_fwd(lib, ops, x, t, k, mode, ws, offs)
    assert set(np.unique(m)) <= {0, 1}
    got = np.flatnonzero(m)
    assert np.array_equal(got, want), (tag, got.size, want.size, np.setxor1d(got, want)[:8])
    ref = R.selected_mean(x, t, want)
    _check("selection.loss", tag, loss, ref.loss, ref.S)
    grad = _sel_bwd(lib, ops, xd, td, mask, k, G, do)
    _check("selection.grad", tag, grad, ref.grad, ref.scale, g=G, floor=TINY)
    assert bool((grad[torch.from_numpy(m == 0)] == 0).all()), f"{tag}: a gradient outside the set"
    return ws


def _sel_reuse(lib, ops, ws, x2, t2, k2, mode, tag):
    """A second call with other data on the used workspace `ws` gives the bits of the same call on a fresh one."""
    l1, m1, *_ = _sel_fwd(lib, ops, x2, t2, k2, mode, ws)
    l2, m2, *_ = _sel_fwd(lib, ops, x2, t2, k2, mode, _new_ws(lib, x2.numel()))
    assert np.array_equal(m1, m2) and torch.equal(l1.view(torch.int32), l2.view(torch.int32)), tag


@pytest.mark.parametrize("mode", list(SEL_MODES), ids=SEL_MODES.get)
@pytest.mark.parametrize("N", SEL_N)
def test_selection_takes_the_stable_argsort_set(N, mode):
    _, lib, ops = _gpu()
    flip = SEL_N.index(N) % 2
    x, t = sel_inputs(N, flip)
    x2, t2 = sel_inputs(N, 1 - flip, seed=1)
    assert_keys_separated(x, t, mode)
    for k in sel_ks(N):
        tag = f"{SEL_MODES[mode]} N={N} k={k}"
        ws = _sel_compare(lib, ops, x, t, k, mode, _want_set(x, t, k, mode), tag)
        _sel_reuse(lib, ops, ws, x2, t2, max(1, (2 * k) // 3), mode, tag)


@pytest.mark.parametrize("mode", list(SEL_MODES), ids=SEL_MODES.get)
def test_selection_ties_take_the_first_flat_indices(mode):
    _, lib, ops = _gpu()
    N = SEL_TIES_N
    x, t = sel_tie_inputs(N)
    assert len(np.unique(R.selection_keys(x, t, mode).numpy())) == 1
    x2, t2 = sel_inputs(N, 0, seed=2)
    for k in SEL_TIES_K:
        tag = f"{SEL_MODES[mode]} ties N={N} k={k}"
        ws = _sel_compare(lib, ops, x, t, k, mode, np.arange(k), tag)
        _sel_reuse(lib, ops, ws, x2, t2, k - 5, mode, tag)
        _sel_reuse(lib, ops, ws, x, t, k - 1, mode, tag)         # ties again, where rows and tie_off held other counts


# (mode, e, leading digits all keys share at least): logits j 2^-18 move the TopK key by 16 and the BCE by 32 fp32 ulps per
# step, so two histogram passes see one bin and the third sees 16 resp. 32; at 2^-22 the TopK key moves by one ulp per step
# and three passes see one bin.  The BCE is not run there: torch's BCE and the kernel's may differ in the last place, which a
# one-ulp key spacing would turn into another set.
SEL_DIGIT_CASES = [(0, 18, 2), (1, 18, 2), (0, 22, 3)]


@pytest.mark.parametrize("mode,e,shared", SEL_DIGIT_CASES, ids=lambda v: str(v))
def test_selection_keys_that_differ_in_the_last_digits(mode, e, shared):
    _, lib, ops = _gpu()
    N = 32773
    x, t = sel_digit_inputs(N, e)
    key = _torch_keys(x, t, mode)
    assert shared_key_digits(key) >= shared and len(np.unique(key)) >= 128
    for k in (1, 129, N // 2, N - 1):
        _sel_compare(lib, ops, x, t, k, mode, np.sort(np.argsort(key, kind="stable")[:k]), f"{SEL_MODES[mode]} 2^-{e} k={k}")


# (pred, target offsets in floats, mask offset in bytes, dpred offset in floats)
SEL_OFFSETS = [(1, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 0, 1, 1)]


@pytest.mark.parametrize("offs", SEL_OFFSETS, ids=lambda o: "+".join(map(str, o)))
@pytest.mark.parametrize("mode", list(SEL_MODES), ids=SEL_MODES.get)
@pytest.mark.parametrize("N", [1024, 32773])
def test_selection_on_misaligned_operands(N, mode, offs):
    """A pointer that is not 16-byte (the mask: 4-byte) aligned turns the float4 / uchar4 accesses off: load4's scalar body in
    sel_hist / sel_sum, n4 = 0 in sel_bwd.  _at and _Guarded place the operands; their alignment is asserted here."""
    _, lib, ops = _gpu()
    x, t = sel_inputs(N, 0)
    k = max(1, N // 2)
    _sel_compare(lib, ops, x, t, k, mode, _want_set(x, t, k, mode), f"{SEL_MODES[mode]} N={N} offsets {offs}", None, offs[:3], offs[3])


def test_selection_kernels_of_a_misaligned_call():
    """The path is a runtime argument of the same kernels, so their names cannot tell it; what the profile does show is that
    a misaligned call runs the selection's own kernels and nothing else of the library."""
    _, lib, ops = _gpu()
    x, t = sel_inputs(1024, 0)
    ws = _new_ws(lib, 1024)

    def run():
        _, _, xd, td, mask = _sel_fwd(lib, ops, x, t, 512, 0, ws, (1, 1, 1))
        _sel_bwd(lib, ops, xd, td, mask, 512, G, do=1)
    names = _kernels(run)
    for kern in ("sel_hist_kernel", "sel_pick_kernel", "sel_sum_kernel", "sum_finalize_kernel", "sel_bwd_kernel"):
        assert kern in names, (kern, names)


# ========================================================================================================================
# 4. HausdorffDTLoss
# ========================================================================================================================
# H > 1024: a thread of hdt_col_kernel owns more than one 64-row chunk (j >= 1); 4096: the limit, distances up to
# 4095^2 + 1; 64 / 63 / 65: one chunk exactly, one short, one more
HDT_SHAPES = [(1025, 3), (1100, 5), (2049, 2), (4096, 2), (2, 4096), (3, 1100), (65, 257), (64, 64), (63, 65)]
HDT_ALPHAS = [0.2, 2.0]
# (B, H, W, pred offset): the tail loop alone (N = 35); n4 = 0 on a 4-byte aligned pred; N = 2,100,225 > 2048 * 1024 with
# N % 4 = 1: the grid-stride loop and the tail together
HDT_BWD_CASES = [(1, 5, 7, 0), (2, 64, 64, 1), (3, 1025, 683, 0)]


@functools.lru_cache(maxsize=None)
def hdt_masks(H, W):
    """The foreground images of one shape: 50 % noise, one pixel in the far corner and its complement, stripes 70 thick
    (across the longer axis: horizontal wherever H >= W; starting half a stripe in), and for H > 1024 rows 0..1023
    background / the rest foreground and the reverse (the nearest row of the other class then lies in a chunk of the same
    thread at j + 1, or of another wave)."""
    rng = np.random.default_rng(10007 * H + W)
    rows = np.arange(H)[:, None] + np.zeros((1, W), dtype=np.int64)
    along = rows if H >= W else np.arange(W)[None, :] + np.zeros((H, 1), dtype=np.int64)
    corner = np.zeros((H, W), dtype=bool)
    corner[H - 1, W - 1] = True
    out = [rng.random((H, W)) < 0.5, corner, ~corner, ((along + 35) // 70) % 2 == 1]
    if H > 1024:
        out += [rows >= 1024, rows < 1024]
    return out


@functools.lru_cache(maxsize=None)
def hdt_field_batches(H, W):
    """Per content n one batch of 3: pred masks (content n, all foreground, no foreground), target masks (no foreground,
    content n + 1, all foreground), both rolled by n.  Returns [(pred logits, target, pred field, target field)], the fields
    by SciPy.  Logits are +-[0.25, 6] by the mask; target background is 0 or 0.5 (not > 0.5), foreground 1."""
    rng = np.random.default_rng(H + 4099 * W)
    masks, out = hdt_masks(H, W), []
    full, none = np.ones((H, W), dtype=bool), np.zeros((H, W), dtype=bool)
    for n, m in enumerate(masks):
        pm = np.roll(np.stack([m, full, none]), n, axis=0)[:, None]
        tm = np.roll(np.stack([none, masks[(n + 1) % len(masks)], full]), n, axis=0)[:, None]
        mag = 0.25 + 5.75 * rng.random(pm.shape)
        x = torch.from_numpy(np.where(pm, mag, -mag).astype(np.float32))
        t = torch.from_numpy(np.where(tm, 1.0, np.where(rng.random(tm.shape) < 0.2, 0.5, 0.0)).astype(np.float32))
        out.append((x, t, R.edt_fields(torch.sigmoid(x.double()).numpy()), R.edt_fields(t.numpy())))
    return out


def _smooth_logits(gen, B, H, W):
    x = _smooth(gen, B, H, W)
    return torch.where(x.abs() < 1e-3, torch.full_like(x, 1e-3), x)    # keeps sigmoid(x) > 0.5 clear of its rounding


@functools.lru_cache(maxsize=None)
def hdt_bwd_inputs(B, H, W):
    gen = torch.Generator().manual_seed(7 * B + 13 * H + W)
    x = _smooth_logits(gen, B, H, W).contiguous()
    t = (_smooth_logits(gen, B, H, W) > 1.0).float().contiguous()
    return x, t, R.edt_fields(torch.sigmoid(x.double()).numpy()), R.edt_fields(t.numpy())


@functools.lru_cache(maxsize=None)
def hdt_bwd_ref(B, H, W, alpha):
    x, t, fp_ref, ft_ref = hdt_bwd_inputs(B, H, W)
    return R.hdt(x, t, alpha, fp_ref, ft_ref)


def _ulps(a, b):
    return int((a.view(torch.int32).long() - b.view(torch.int32).long()).abs().max())


def _hdt_fwd(lib, ops, xd, td, alpha):
    """(loss, guarded D, pred field, target field) of one forward call on poisoned, guarded buffers."""
    B, _, H, W = xd.shape
    n = xd.numel()
    need = lib.fn("umi_hdt_ws_bytes")(B, H, W)
    ws, D, fields, loss = _Guarded(need, torch.uint8), _Guarded(n), _Guarded(2 * n), _Guarded(1)
    lib.call("umi_hdt_fwd", xd.data_ptr(), td.data_ptr(), B, 1, H, W, alpha, D.ptr, fields.ptr, loss.ptr, ws.ptr, need, ops._stream())
    torch.cuda.synchronize()
    assert ws.intact() and D.intact() and fields.intact() and loss.intact(), "a guard byte was written"
    f = fields.t.view((2,) + tuple(xd.shape)).cpu()
    return loss.t[0].cpu(), D, f[0], f[1]


def _hdt_check_forward(tag, loss, D, fp, ft, fp_ref, ft_ref, ref):
    fp_ref, ft_ref = torch.from_numpy(fp_ref), torch.from_numpy(ft_ref)
    assert torch.equal(fp.view(torch.int32), fp_ref.view(torch.int32)), (tag, "pred field", (fp - fp_ref).abs().max().item())
    assert torch.equal(ft.view(torch.int32), ft_ref.view(torch.int32)), (tag, "target field", (ft - ft_ref).abs().max().item())
    Dc = D.t.view(fp.shape).cpu()
    assert torch.isfinite(Dc).all()
    ulps = _ulps(Dc, ref.coef.float())
    print(f"[ulps] hdt.D {tag}: {ulps} of 2")
    assert ulps <= 2, (tag, ulps)
    _check("hdt.loss", tag, loss, ref.loss, ref.S)


@pytest.mark.parametrize("alpha", HDT_ALPHAS)
@pytest.mark.parametrize("shape", HDT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_hdt_fields_bit_for_bit_and_loss_against_float64(shape, alpha):
    _, lib, ops = _gpu()
    for n, (x, t, fp_ref, ft_ref) in enumerate(hdt_field_batches(*shape)):
        loss, D, fp, ft = _hdt_fwd(lib, ops, x.to(DEV), t.to(DEV), alpha)
        _hdt_check_forward(f"{shape} alpha={alpha} content {n}", loss, D, fp, ft, fp_ref, ft_ref,
                           R.hdt(x, t, alpha, fp_ref, ft_ref))


@pytest.mark.parametrize("alpha", HDT_ALPHAS)
@pytest.mark.parametrize("case", HDT_BWD_CASES, ids=lambda c: "x".join(map(str, c[:3])) + f"+{c[3]}")
def test_hdt_gradient_against_float64(case, alpha):
    L, lib, ops = _gpu()
    B, H, W, po = case
    x, t, fp_ref, ft_ref = hdt_bwd_inputs(B, H, W)
    ref, tag = hdt_bwd_ref(B, H, W, alpha), f"{case} alpha={alpha}"
    xd, td = _at(x, po), _at(t, 0)
    assert xd.data_ptr() % 16 == 4 * po                  # po = 1: no float4 access is possible, n4 = 0
    loss, D, fp, ft = _hdt_fwd(lib, ops, xd, td, alpha)
    _hdt_check_forward(tag, loss, D, fp, ft, fp_ref, ft_ref, ref)
    dpred, gout = _Guarded(x.numel()), torch.tensor([G], dtype=torch.float32, device=DEV)
    lib.call("umi_hdt_bwd", xd.data_ptr(), td.data_ptr(), D.ptr, gout.data_ptr(), B, 1, H, W, dpred.ptr, ops._stream())
    torch.cuda.synchronize()
    assert dpred.intact() and D.intact(), "a guard byte was written"
    _check("hdt.grad", tag + " direct", dpred.t.view(x.shape).cpu(), ref.grad, ref.scale, g=G, floor=TINY)
    xa = _at(x, po).requires_grad_(True)                 # and through the module, as calc_loss runs it
    v = L.HausdorffDTLoss(alpha)(xa, td)
    assert type(v.grad_fn).__name__.startswith("_HausdorffDT")
    (G * v).backward()
    torch.cuda.synchronize()
    _check("hdt.loss", tag + " module", v.detach().cpu(), ref.loss, ref.S)
    _check("hdt.grad", tag + " module", xa.grad.cpu(), ref.grad, ref.scale, g=G, floor=TINY)


# ========================================================================================================================
# 5. an upstream gradient of exactly 1, once per loss
# ========================================================================================================================
@pytest.mark.parametrize("which", ["dice_bce", "Tversky", "Tversky_mc", "TopK", "BCE_HEM", "HausdorffDTLoss"])
def test_bare_loss_backward(which):
    L, lib, ops = _gpu()
    if which in ("dice_bce", "Tversky"):
        x, t = bin_inputs(2, 64, 65, "hard")
        ref, fam = bin_ref(which, 2, 64, 65, "hard"), _bin_family(which)
        loss, grad = _through_calc_loss(L, which, x, t, 1.0)
    elif which == "Tversky_mc":
        x, t = mc_inputs(3, MC_SMALL)
        ref, fam = mc_ref(3, MC_SMALL), "tversky_mc"
        loss, grad = _through_calc_loss(L, "Tversky", x, t, 1.0)
    elif which in ("TopK", "BCE_HEM"):
        mode, N = (0, 32 * 33) if which == "TopK" else (1, 32 * 33)
        x, t = sel_inputs(N, 0)
        x, t = x.view(2, 1, 16, 33), t.view(2, 16, 33)
        assert_keys_separated(x.reshape(-1), t.reshape(-1), mode)
        k = N // 2 if which == "TopK" else 500
        ref, fam = R.selected_mean(x, t, _want_set(x.reshape(-1), t.reshape(-1), k, mode)), "selection"
        loss, grad = _through_calc_loss(L, which, x, t, 1.0)
        assert bool((grad.reshape(-1)[ref.scale.reshape(-1) == 0] == 0).all())
    else:
        x, t, fp_ref, ft_ref = hdt_bwd_inputs(1, 5, 7)
        ref, fam = hdt_bwd_ref(1, 5, 7, 0.2), "hdt"
        xd = x.to(DEV).requires_grad_(True)
        v = L.calc_loss(xd, t.to(DEV), loss_type="HausdorffDTLoss")
        v.backward()
        loss, grad = v.detach().cpu(), xd.grad.cpu()
    _check(fam + ".loss", f"{which} g=1", loss, ref.loss, ref.S)
    _check(fam + ".grad", f"{which} g=1", grad, ref.grad, ref.scale, floor=TINY)
