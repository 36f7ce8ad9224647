"""The deferred split-K weight-gradient reductions (umi_wgrad_reduce_group / wgrad_reduce_group_kernel) against float64.

Every weight gradient of a training step ends in one of these reductions, 16 per launch.  Here the kernel is driven directly
over synthetic slabs (every form wg_tmode can choose, every split count around the lane and chain boundaries, entries past the
per-entry workgroup cap, tables longer than one launch), through the nine paths of umi_conv_wgrad with and without `defer`,
and through whole models with the A/B knob UMI_NO_WGRAD_REDUCE_GROUP.  Every expectation is exact (integer data against
float64), bit-identical to the documented order (tests/wgrad_reduce_order.py) or inside the a-priori summation bound."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.wgrad_reduce_order import error_bound, reduce_one_chain, reduce_two_chains, reference_f64

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG = -1                  # UMI_ERR_BADARG
SENTINEL = -1234.5678        # neither a multiple of 0.5 (integer data) nor a plausible sum
GUARD = 64                   # floats in front of and behind every dW


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from umi import lib, ops
    return lib, ops


# ---- (a) the grouped kernel on synthetic slabs -------------------------------------------------------------------------------
# The form is chosen per entry by wg_tmode and the kernel's `vec` (csrc/generic_kernels.hip); the cases below were picked from
# this rule, and _form restates it -- if the rule changes, re-choose the cases:
#
#   constexpr int WGT_CO = 32, WGT_CI = 8;
#   wg_tmode(d):  0 = element-wise, 1 = OIHW tiles, 2 = IOHW tiles
#     if (d.Co % WGT_CO || d.Ci % WGT_CI || d.RS > 9 || d.s_t != 1 || (((uintptr_t)d.part) & 15)) return 0;
#     if ((long)(d.Co / WGT_CO) * (d.Ci / WGT_CI) < 512) return 0;
#     if (d.s_ci == d.RS && d.s_co == (long)d.Ci * d.RS) return 1;
#     if (d.s_co == d.RS && d.s_ci == (long)d.Co * d.RS) return 2;
#     return 0;
#   element-wise:  vec = d.Co % 4 == 0 && (((uintptr_t)d.part) & 15) == 0   (float4 form; else the scalar form)
#   workgroups of an entry: tiles = (Co / 32) * (Ci / 8), or ceil(RS * Ci * Co / (vec ? 4 : 1) / 32); at most 4096 (stride loop)
def _strides(layout, RS, Ci, Co):
    """(s_co, s_ci, s_t) of dW[co * s_co + ci * s_ci + t * s_t]."""
    return {"OIHW": (Ci * RS, RS, 1),               # Conv2d
            "IOHW": (RS, Co * RS, 1),               # ConvTranspose2d
            "TOI": (Ci, 1, Co * Ci),                # [t][co][ci]: s_t != 1
            "OIHW+5": (Ci * RS + 5, RS, 1)}[layout]  # rows padded by 5 floats


def _form(shape, layout, misaligned):
    RS, Ci, Co = shape
    s_co, s_ci, s_t = _strides(layout, RS, Ci, Co)
    if not (Co % 32 or Ci % 8 or RS > 9 or s_t != 1 or misaligned) and (Co // 32) * (Ci // 8) >= 512:
        if s_ci == RS and s_co == Ci * RS:
            return "tile-OIHW"
        if s_co == RS and s_ci == Co * RS:
            return "tile-IOHW"
    return "float4" if Co % 4 == 0 and not misaligned else "scalar"


def _workgroups(shape, layout, misaligned):
    RS, Ci, Co = shape
    form = _form(shape, layout, misaligned)
    if form.startswith("tile"):
        return (Co // 32) * (Ci // 8)
    return -(-(RS * Ci * Co // (4 if form == "float4" else 1)) // 32)


CASES = [  # form, (RS, Ci, Co), layout, slab pointer offset by one float
    ("scalar", (9, 5, 3), "OIHW", False),
    ("scalar", (1, 64, 2), "OIHW", False),
    ("scalar", (49, 3, 7), "OIHW", False),
    ("scalar", (9, 16, 8), "OIHW", True),
    ("float4", (9, 16, 24), "OIHW", False),
    ("float4", (9, 64, 64), "OIHW", False),
    ("float4", (1, 72, 136), "OIHW", False),
    ("float4", (4, 64, 128), "IOHW", False),
    ("float4", (9, 256, 512), "TOI", False),
    ("float4", (9, 256, 512), "OIHW+5", False),
    ("tile-OIHW", (9, 256, 512), "OIHW", False),
    ("tile-OIHW", (4, 512, 256), "OIHW", False),
    ("tile-OIHW", (1, 1024, 128), "OIHW", False),
    ("tile-IOHW", (4, 256, 512), "IOHW", False),
    ("tile-IOHW", (1, 128, 1024), "IOHW", False),
    # more than 4,096 workgroups in one entry: the stride loop behind the cap
    ("tile-OIHW", (1, 1040, 1024), "OIHW", False),          # 4,160 tiles
    ("float4", (9, 512, 132), "OIHW", False),               # 4,752 workgroups
    ("scalar", (9, 5000, 3), "OIHW", False),                # 4,219 workgroups
]
STRIDE_LOOP = CASES[-3:]
SPLITS_SMALL = [1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 33]      # around `z + 8 < splits` and the trailing term
SPLITS_LARGE = [1, 9, 25]                                   # Ci * Co >= 131072: the slab set reaches ~120 MB
SCALE = {"int": 0.5, "normal": 0.37}


def _case_id(c):
    return "%s-%dx%dx%d-%s%s" % (c[0], *c[1], c[2], "-off1" if c[3] else "")


def _case_splits():
    out = []
    for c in CASES:
        for s in (SPLITS_LARGE if c[1][1] * c[1][2] >= 131072 else SPLITS_SMALL):
            out.append(pytest.param(c, s, id="%s-s%d" % (_case_id(c), s)))
    return out


def test_cases_reach_the_forms_they_are_listed_under():
    for form, shape, layout, mis in CASES:
        assert _form(shape, layout, mis) == form, (form, shape, layout)
    for _, shape, layout, mis in STRIDE_LOOP:
        assert _workgroups(shape, layout, mis) > 4096
    for form, shape, layout, mis in CASES[:-3]:              # (the two large float4 cases run through the stride loop as well)
        assert _workgroups(shape, layout, mis) <= 4096 or (form, shape) == ("float4", (9, 256, 512))
    assert {c[0] for c in CASES} == {"scalar", "float4", "tile-OIHW", "tile-IOHW"}


class _Entry:
    """One reduction over device slabs of its own: `splits` slabs [RS][Ci][Co], a dW inside a sentinel-filled buffer."""

    def __init__(self, ops, case, splits, kind, seed):
        self.form, (RS, Ci, Co), self.layout, self.misaligned = case
        self.shape, self.splits, self.kind, self.scale = (RS, Ci, Co), splits, kind, SCALE[kind]
        n = splits * RS * Ci * Co
        g = torch.Generator(device=DEV).manual_seed(seed)
        self._flat = torch.empty(n + 4, device=DEV)
        self.part = self._flat[1:1 + n] if self.misaligned else self._flat[:n]
        assert (self.part.data_ptr() % 16 != 0) == self.misaligned
        if kind == "int":
            self.part.copy_(torch.randint(-64, 65, (n,), generator=g, device=DEV))
        else:
            self.part.normal_(generator=g)
        self.strides = _strides(self.layout, RS, Ci, Co)
        s_co, s_ci, s_t = self.strides
        extent = (Co - 1) * s_co + (Ci - 1) * s_ci + (RS - 1) * s_t + 1
        self.buf = torch.full((GUARD + extent + GUARD,), SENTINEL, device=DEV)
        self.pending = ops.wgrad_pending(self.part, self.buf.data_ptr() + 4 * GUARD, s_co, s_ci, s_t, self.scale, splits, RS, Ci, Co)

    def host_part(self):
        return self.part.cpu().numpy().reshape((self.splits,) + self.shape)

    def index(self):
        """Position in `buf` of element [t][ci][co]."""
        RS, Ci, Co = self.shape
        s_co, s_ci, s_t = self.strides
        t, ci, co = np.ogrid[:RS, :Ci, :Co]
        return GUARD + t * s_t + ci * s_ci + co * s_co

    def expected_buffer(self, values):
        """The whole buffer -- guards, gaps between addressed elements and all -- with `values` [RS][Ci][Co] scattered in."""
        out = np.full(self.buf.numel(), SENTINEL, np.float32)
        idx = self.index()
        assert np.unique(idx).size == idx.size
        out[idx] = values
        return out

    def order(self, part):
        return (reduce_one_chain if self.form == "scalar" else reduce_two_chains)(part, self.scale)


def _same_bits(got, want):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    bad = np.flatnonzero(got.view(np.int32) != want.view(np.int32))
    assert bad.size == 0, "%d of %d floats differ, first at %d: got %r, want %r" % (bad.size, got.size, bad[0], got[bad[0]],
                                                                                  want[bad[0]])


@pytest.mark.parametrize("case,splits", _case_splits())
def test_grouped_reduction_on_synthetic_slabs(case, splits):
    """One entry per call.  Integer slabs: equal to float64.  Normal slabs: bit-identical to the documented order and inside
    (splits + 1) * 2^-24 * scale * sum |part| of float64.  The whole sentinel-filled buffer is compared, so a store into a
    gap of a padded / transposed layout or into the guards fails the same assertion."""
    lib, ops = _gpu()
    for kind in ("int", "normal"):
        e = _Entry(ops, case, splits, kind, seed=1000 * splits + sum(case[1]))
        ops.wgrad_reduce_group([e.pending])
        torch.cuda.synchronize()
        got = e.buf.cpu().numpy()
        part = e.host_part()
        ref = reference_f64(part, e.scale)
        if kind == "int":
            assert np.array_equal(ref, ref.astype(np.float32))
            _same_bits(got, e.expected_buffer(ref.astype(np.float32)))
        else:
            _same_bits(got, e.expected_buffer(e.order(part)))
            err = np.abs(got[e.index()].astype(np.float64) - ref)
            bound = error_bound(part, e.scale)
            print(_case_id(case), "splits", splits, "worst err / bound", float((err[bound > 0] / bound[bound > 0]).max()))
            assert (err <= bound).all()
        del e, part, ref


# ---- (b) group composition ------------------------------------------------------------------------------------------------------
GROUP_N = [1, 2, 16, 17, 32, 33, 40]


@pytest.fixture(scope="module", params=["int", "normal"])
def pool(request):
    """40 entries drawn from CASES in a fixed shuffled order (the forms interleave and straddle the chunks of 16; every case
    repeats with other data), each reduced ALONE once: `alone` is that buffer, `exact` the float64 result on integer data."""
    lib, ops = _gpu()
    kind = request.param
    order = np.random.default_rng(7).permutation(len(CASES) * 3)[:max(GROUP_N)] % len(CASES)
    assert {CASES[i][0] for i in order[:16]} == {"scalar", "float4", "tile-OIHW", "tile-IOHW"}
    entries = []
    for pos, ci in enumerate(order):
        case = CASES[ci]
        big = case[1][0] * case[1][1] * case[1][2] > 200000
        splits = (1, 2, 3)[pos % 3] if big else (1, 2, 3, 9, 17)[pos % 5]           # small: bounds the memory
        e = _Entry(ops, case, splits, kind, seed=50 + pos)
        ops.wgrad_reduce_group([e.pending])
        torch.cuda.synchronize()
        e.alone = e.buf.clone()
        e.exact = None
        if kind == "int":
            ref = reference_f64(e.host_part(), e.scale)
            assert np.array_equal(ref, ref.astype(np.float32))
            e.exact = torch.from_numpy(e.expected_buffer(ref.astype(np.float32))).to(DEV)
        entries.append(e)
    yield kind, entries
    del entries[:]
    torch.cuda.empty_cache()


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("n", GROUP_N)
def test_group_of_n_entries_equals_each_entry_alone(pool, n):
    lib, ops = _gpu()
    kind, entries = pool
    for e in entries:
        e.buf.fill_(SENTINEL)
    ops.wgrad_reduce_group([e.pending for e in entries[:n]])
    torch.cuda.synchronize()
    for i, e in enumerate(entries[:n]):
        assert _bits_equal(e.buf, e.alone), (i, e.form, e.shape, e.layout, e.splits)
        if kind == "int":
            assert _bits_equal(e.buf, e.exact), (i, e.form, e.shape, e.layout, e.splits)
    for i, e in enumerate(entries[n:], n):
        assert (e.buf == SENTINEL).all(), (i, "not part of this call")


# ---- (c) deferred versus immediate through the real kernels -------------------------------------------------------------------------
def _ints(shape, lo, hi, gen):
    return torch.randint(lo, hi + 1, shape, generator=gen).float()


def _int_tx(C, gen):
    """Consumer-side transform rows with integer effect: scale in {1, -1, 2}, integer shift, ReLU."""
    t = torch.zeros(C, 4)
    t[:, 1] = torch.tensor([1.0, -1.0, 2.0])[torch.randint(0, 3, (C,), generator=gen)]
    t[:, 2] = _ints((C,), -1, 1, gen)
    return t


def _apply(x, t):
    return torch.clamp_min(x * t[:, 1] + t[:, 2], 0.0)


class _Conv:
    """One Conv2d weight-gradient problem on integer operands (exact in fp16 / fp32 in any order) with its float64 autograd
    reference.  The shapes are the smallest of tests/test_gpu_exact.py and tests/test_gpu_kernels*.py that reach each path."""

    def __init__(self, N, H, W, Ci, Co, R, stride, pad, use_tx, scale, dtype=torch.float16, flags=0):
        self.args = (N, H, W, Ci, Co, R, stride, pad, use_tx, scale, dtype, flags)

    def build(self, ops, seed):
        N, H, W, Ci, Co, R, stride, pad, use_tx, scale, dtype, flags = self.args
        g = torch.Generator().manual_seed(seed)
        x = _ints((N, H, W, Ci), -2, 2, g)
        t = _int_tx(Ci, g) if use_tx else None
        a = (_apply(x, t) if use_tx else x).permute(0, 3, 1, 2).double()
        wr = torch.zeros(Co, Ci, R, R, dtype=torch.float64, requires_grad=True)
        y = F.conv2d(a, wr, None, stride, pad)
        dy = _ints((N, y.shape[2], y.shape[3], Co), -1, 1, g)
        y.backward(dy.permute(0, 3, 1, 2).double())
        self.ref = wr.grad * scale
        assert self.ref.abs().max().item() < 2 ** 24
        xd, dyd = x.to(dtype).to(DEV), dy.to(dtype).to(DEV)
        td = t.to(DEV) if use_tx else None
        self.RS, self.Ci, self.Co = R * R, Ci, Co
        self.dev = (xd, td, dyd)

        def run(gw, defer=None):
            ops.conv_wgrad(xd, td, dyd, None, gw, Ci * R * R, R * R, 1, scale, R, R, stride, pad, flags=flags, defer=defer)
        self.run = run
        self.new = lambda fill: torch.full((Co, Ci, R, R), fill, device=DEV)
        return self


class _ConvT:
    """ConvTranspose2d(2, 2) weight + bias gradient in one pass (convT_wgrad_bias), as in test_gpu_exact.py."""

    def __init__(self, N, h, w, Cin, Cout, scale):
        self.args = (N, h, w, Cin, Cout, scale)

    def build(self, ops, seed):
        N, h, w, Cin, Cout, scale = self.args
        g = torch.Generator().manual_seed(seed)
        x = _ints((N, h, w, Cin), -2, 2, g)
        t = _int_tx(Cin, g)
        a = _apply(x, t).permute(0, 3, 1, 2).double()
        dup = _ints((N, 2 * h, 2 * w, Cout), -1, 1, g)
        wr = torch.zeros(Cin, Cout, 2, 2, dtype=torch.float64, requires_grad=True)
        br = torch.zeros(Cout, dtype=torch.float64, requires_grad=True)
        F.conv_transpose2d(a, wr, br, stride=2).backward(dup.permute(0, 3, 1, 2).double())
        self.ref, self.ref_bias = wr.grad * scale, br.grad * scale
        xd, td, dupd = x.half().to(DEV), t.to(DEV), dup.half().to(DEV)
        self.dev = (dupd, xd, td)                           # d(up), the ConvT's input, its transform
        self.RS, self.Ci, self.Co = 4, Cout, Cin            # the kernel's view: x = d(up), "dy" = the ConvT's input
        self.bias = []

        def run(gw, defer=None):
            gb = torch.full((Cout,), float("nan"), device=DEV)
            assert ops.convT_wgrad_bias(dupd, xd, td, gw, gb, scale, defer=defer)
            self.bias.append(gb)
        self.run = run
        self.new = lambda fill: torch.full((Cin, Cout, 2, 2), fill, device=DEV)
        return self


def _paths(lib):
    """The nine paths of umi_conv_wgrad (csrc/api.hip), in its order of preference."""
    return {
        "conv3x3": lambda: _Conv(2, 20, 45, 32, 64, 3, 1, 1, True, 0.5),          # matrix-core 3x3 (512-thread form by default)
        "pointwise": lambda: _Conv(2, 13, 11, 192, 64, 1, 1, 0, True, 2.0),       # 1x1 matrix-core
        "convT": lambda: _ConvT(1, 16, 16, 128, 64, 0.5),                         # 2x2 / stride 2 with the bias gradient
        "gather": lambda: _Conv(2, 11, 13, 64, 128, 3, 2, 1, True, 1.0),          # strided tap-gather
        "stem": lambda: _Conv(2, 37, 29, 1, 64, 3, 1, 1, False, 0.25),            # Ci <= 4
        "head": lambda: _Conv(2, 37, 29, 64, 2, 1, 1, 0, True, 2.0),              # OutConv: 1x1, Co <= 8
        "root": lambda: _Conv(2, 37, 41, 3, 64, 7, 2, 3, False, 1.0),             # ResNetV2 root 7x7 / s2
        "head3": lambda: _Conv(2, 21, 19, 16, 2, 3, 1, 1, True, 1.0),             # SegmentationHead 3x3, Co <= 4
        "generic-fp32": lambda: _Conv(2, 9, 7, 5, 3, 3, 1, 1, True, 0.5, dtype=torch.float32),
        "generic-forced": lambda: _Conv(1, 12, 12, 128, 64, 3, 1, 1, True, 0.5, flags=lib.CONV_FORCE_GENERIC),
    }


def run_deferred_vs_immediate(names):
    """Each named path once immediately and once with `defer` into ONE list, then one flush."""
    lib, ops = _gpu()
    paths = _paths(lib)
    lst, done = [], []
    for i, name in enumerate(names):
        p = paths[name]().build(ops, seed=300 + i)              # a repeated path gets fresh data
        gw_a, gw_b = p.new(0.0), p.new(float("nan"))
        p.run(gw_a)
        before = len(lst)
        p.run(gw_b, defer=lst)
        torch.cuda.synchronize()
        assert len(lst) == before + 1, (name, "the reduction was not recorded")
        assert torch.isnan(gw_b).all(), (name, "the reduction ran at once")
        pend = lst[-1][0]
        assert (pend.RS, pend.Ci, pend.Co, pend.dW) == (p.RS, p.Ci, p.Co, gw_b.data_ptr()), name
        if isinstance(p, _ConvT):                                # the bias gradient does not wait for the flush
            assert torch.equal(p.bias[1], p.bias[0]) and torch.equal(p.bias[1].cpu().double(), p.ref_bias), name
        done.append((name, p, gw_a, gw_b))
    assert len({d[0].part for d in lst}) == len(lst)             # every call's partial sums are its own
    ops.wgrad_reduce_flush(lst)
    torch.cuda.synchronize()
    assert lst == []
    for name, p, gw_a, gw_b in done:
        assert torch.equal(gw_a, gw_b), name
        assert torch.equal(gw_a.cpu().double(), p.ref), name
    return len(done)


def test_deferred_reduction_equals_immediate_on_every_wgrad_path():
    lib, ops = _gpu()
    names = list(_paths(lib))
    names = names + names[::-1]                                  # 20 entries: two launches, every path on both sides of entry 16
    assert run_deferred_vs_immediate(names) > 16


def test_deferred_reduction_equals_immediate_on_the_256_thread_conv3x3_form():
    """UMI_WGRAD_CLASSIC=1 selects the 256-thread 3x3 kernel; the library reads it once per process, hence the child."""
    _gpu()
    code = ("import sys; sys.path[:0] = [%r, %r]; from tests import test_gpu_wgrad_reduce as t; "
            "print('ran', t.run_deferred_vs_immediate(['conv3x3', 'pointwise', 'conv3x3']))" % (REPO, os.path.join(REPO, "unet-torch_amd")))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, UMI_WGRAD_CLASSIC="1"), cwd=REPO, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "ran 3" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ---- (c') a refused call arms nothing: the sinks are arguments of that call alone ------------------------------------------------
WORKSPACE = -3               # UMI_ERR_WORKSPACE


def test_a_failed_deferred_call_leaves_nothing_armed():
    """umi_conv_wgrad_deferred with a workspace four bytes short: refused before any launch, nothing recorded, dW untouched --
    and the next, immediate call on this thread reduces at once into its own dW."""
    import ctypes
    lib, ops = _gpu()
    p = _paths(lib)["head"]().build(ops, seed=500)
    N, H, W, Ci, Co, R, stride, pad, _, scale, _, flags = p.args
    xd, td, dyd = p.dev
    nb = lib.fn("umi_conv_wgrad_ws_bytes")(N, H, W, Ci, Co, R, R, lib.UMI_F16, flags)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    gw = p.new(SENTINEL)
    pend = ops.wgrad_pending(ws, gw, 1, 1, 1, 1.0, 1, 1, 1, 1)           # stale contents: the call must clear `part`
    st = lib.fn("umi_conv_wgrad_deferred")(xd.data_ptr(), Ci, td.data_ptr(), dyd.data_ptr(), Co, None, gw.data_ptr(), Ci * R * R, R * R,
                                           1, scale, N, H, W, Ci, Co, R, R, stride, pad, H, W, lib.UMI_F16, flags, ws.data_ptr(),
                                           nb - 4, ctypes.addressof(pend), ops._stream())
    torch.cuda.synchronize()
    assert st == WORKSPACE and not pend.part
    assert (gw == SENTINEL).all()
    p.run(gw)                                                            # immediate
    torch.cuda.synchronize()
    assert torch.equal(gw.cpu().double(), p.ref)


def test_a_failed_bias_call_leaves_no_bias_sink_armed():
    """The same for umi_conv_wgrad_bias: refused for its workspace, dbias untouched; the plain weight gradient of the same
    2x2 / stride-2 problem that follows gives the reference dW and writes no bias gradient anywhere near that buffer."""
    lib, ops = _gpu()
    p = _paths(lib)["convT"]().build(ops, seed=501)
    N, h, w, Cin, Cout, scale = p.args
    dupd, xd, td = p.dev
    Ci, Co = Cout, Cin                                                   # the kernel's view: x = d(up), dy = the ConvT's input
    nb = lib.fn("umi_conv_wgrad_ws_bytes")(N, h, w, Ci, Co, 2, 2, lib.UMI_F16, 0)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    gw = p.new(SENTINEL)
    dbias = torch.full((GUARD + Ci + GUARD,), float("nan"), device=DEV)
    st = lib.fn("umi_conv_wgrad_bias")(dupd.data_ptr(), Ci, xd.data_ptr(), Co, td.data_ptr(), gw.data_ptr(), Ci * 4, 4, 1,
                                       dbias.data_ptr() + 4 * GUARD, scale, N, 2 * h, 2 * w, Ci, Co, h, w, lib.UMI_F16, 0,
                                       ws.data_ptr(), nb - 4, None, ops._stream())
    torch.cuda.synchronize()
    assert st == WORKSPACE
    assert torch.isnan(dbias).all() and (gw == SENTINEL).all()
    ops.conv_wgrad(dupd, None, xd, td, gw, Ci * 4, 4, 1, scale, 2, 2, 2, 0)
    torch.cuda.synchronize()
    assert torch.equal(gw.cpu().double(), p.ref)
    assert torch.isnan(dbias).all()


def _head_fused(ops, C, seed):
    """OutConv's fused backward (ops.head_dgrad_bnred with dW) on a 1x8x8 map, 2 logit channels, C feature channels, integer data.
    Returns the partial rows (None: refused), da, dW, the float64 dW and the device operands."""
    g = torch.Generator().manual_seed(seed)
    y = _ints((1, 8, 8, C), -2, 2, g)                                    # the BatchNorm layer's raw output
    t = _int_tx(C, g)
    dl = _ints((1, 8, 8, 2), -1, 1, g)
    wo = _ints((2, C, 1, 1), -1, 1, g)
    ref = torch.einsum("nhwc,nhwk->kc", _apply(y, t).double(), dl.double()).reshape(2, C, 1, 1) * 0.5
    dev = (dl.half().to(DEV), ops.pack_conv_dgrad(wo.to(DEV), torch.float16, k8=False), y.half().to(DEV), t.to(DEV),
           torch.ones(C, device=DEV))
    da = torch.full((1, 8, 8, C), SENTINEL, device=DEV, dtype=torch.float16)
    gw = torch.full((2, C, 1, 1), SENTINEL, device=DEV)
    part = ops.head_dgrad_bnred(dev[0], dev[1], da, dev[2], dev[3], dev[4], dW=gw, out_scale=0.5)
    torch.cuda.synchronize()
    return part, da, gw, ref, dev


def test_head_fusion_at_the_channel_limit():
    """The fused kernel keeps a workgroup's weight-gradient rows in LDS, 256 feature channels at the most: above that the call
    is refused as unsupported before anything is launched (the caller runs the separate kernels), at the limit it runs."""
    lib, ops = _gpu()
    C = 512
    part, da, gw, _, (dl, wp, y, t, rstd) = _head_fused(ops, C, seed=502)
    assert part is None
    assert (da == SENTINEL).all() and (gw == SENTINEL).all()
    # the C call itself, with partial rows of our own: unsupported, and they stay untouched too
    rows = lib.fn("umi_head_dgrad_bnred_rows")(64, 2, C, C, lib.UMI_F16)
    assert rows > 0
    rows_buf = torch.full((rows * 2 * C,), SENTINEL, device=DEV)
    ws = torch.empty(max(lib.fn("umi_head_bwd_fused_ws_bytes")(64, 2, C), 16), dtype=torch.uint8, device=DEV)
    st = lib.fn("umi_head_bwd_fused")(dl.data_ptr(), 2, wp.data_ptr(), da.data_ptr(), C, y.data_ptr(), C, t.data_ptr(), rstd.data_ptr(),
                                      rows_buf.data_ptr(), gw.data_ptr(), C, 1, 0.5, ws.data_ptr(), ws.numel(), 64, 2, C, lib.UMI_F16,
                                      ops._stream())
    torch.cuda.synchronize()
    assert st == -2                                                      # UMI_ERR_UNSUPPORTED
    assert (rows_buf == SENTINEL).all() and (da == SENTINEL).all() and (gw == SENTINEL).all()
    part, da, gw, ref, _ = _head_fused(ops, 256, seed=503)
    assert part is not None and part.numel() % (2 * 256) == 0 and torch.isfinite(part).all()
    assert torch.equal(gw.cpu().double(), ref)
    assert not (da == SENTINEL).any()


# ---- (d) model level: the A/B knob ------------------------------------------------------------------------------------------------
def _unet():
    import Model
    from oracle import recipe
    m = Model.UNet(1, 2, 8, compute_dtype="fp16")
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=5))
    x, _ = recipe.synthetic_batch(2, 1, 64, 64, 2, seed=5)
    return m.to(DEV).train(), (x.to(DEV),), None


def _transunet():
    from oracle import ref_transunet
    from tests.test_gpu_transunet import product_config
    from TransUnet.vit_seg_modeling import VisionTransformer
    torch.manual_seed(3)
    cfg = ref_transunet.small_config(2)
    m = VisionTransformer(product_config(cfg, 64), img_size=64, num_classes=2, compute_dtype="fp16").to(DEV).train()
    x = torch.randn(2, 1, 64, 64, generator=torch.Generator().manual_seed(4))
    return m, (x.to(DEV),), None


def _twice():
    """A module applied twice in one tape (tests/test_gpu_unet.py): the second gradient is parked behind the flush."""
    import Model
    from oracle import recipe
    dc = Model.DoubleConv(16, 16, compute_dtype="fp16")
    dc.load_state_dict(recipe.fill_state_dict(dc.state_dict(), seed=11))
    dc = dc.to(DEV)

    class Twice(Model._UmiModule):
        def __init__(self, block):
            super().__init__()
            self.block = block
            self._compute_dtype = "fp16"

        def forward(self, x):
            return Model._run_tape(self, [x], lambda t, a: Model._build_double_conv(
                t, Model._build_double_conv(t, a, self.block), self.block))

    g = torch.Generator().manual_seed(6)
    x, gy = torch.randn(2, 16, 24, 40, generator=g), torch.randn(2, 16, 24, 40, generator=g)
    return Twice(dc).train(), (x.to(DEV),), gy.to(DEV)


# "nofuse": UMI_BNAPPLY_FUSION=0 (read per call).  By default a 3x3 conv of <= 64 input channels folds the BatchNorm backward
# into its weight-gradient kernel and reduces at once; at these small widths that is most layers.  Without the fusion every
# DoubleConv conv goes through conv_wgrad(defer=...): 18 + 4 ConvTranspose + the head in a U-Net, more than one launch of 16.
@pytest.mark.parametrize("make,nofuse,min_reductions", [(_unet, False, 1), (_unet, True, 17), (_transunet, False, 1),
                                                        (_twice, False, 0), (_twice, True, 2)],
                         ids=["unet", "unet-nofuse", "transunet", "twice", "twice-nofuse"])
def test_model_gradients_do_not_depend_on_the_grouping(monkeypatch, make, nofuse, min_reductions):
    """Forward + backward with the reductions grouped (default) and launched one by one (UMI_NO_WGRAD_REDUCE_GROUP=1, read per
    call): every parameter gradient bit-identical, and two runs of one configuration bit-identical to begin with."""
    lib, ops = _gpu()
    if nofuse:
        monkeypatch.setenv("UMI_BNAPPLY_FUSION", "0")
    m, xs, gy = make()
    state = {k: v.clone() for k, v in m.state_dict().items()}
    flushed = []
    flush = ops.wgrad_reduce_flush
    monkeypatch.setattr(ops, "wgrad_reduce_flush", lambda lst: (flushed.append(len(lst)), flush(lst))[1])

    def grads(knob):
        if knob:
            monkeypatch.setenv("UMI_NO_WGRAD_REDUCE_GROUP", "1")
        else:
            monkeypatch.delenv("UMI_NO_WGRAD_REDUCE_GROUP", raising=False)
        m.load_state_dict(state)
        m.zero_grad(set_to_none=True)
        torch.manual_seed(9)
        del flushed[:]
        y = m(*xs)
        (y.square().mean() if gy is None else y).backward(gy)
        torch.cuda.synchronize()
        out = {k: p.grad.clone() for k, p in m.named_parameters()}
        assert all(torch.isfinite(v).all() for v in out.values())
        return out, sum(flushed)

    g0, n0 = grads(False)
    g1, n1 = grads(False)
    gk, nk = grads(True)
    gk2, _ = grads(True)
    assert n0 == n1 >= min_reductions and nk == 0, (n0, n1, nk)       # the default really groups, the knob really does not
    for k in g0:
        assert torch.equal(g0[k], g1[k]), ("grouped, run to run", k)
        assert torch.equal(gk[k], gk2[k]), ("one by one, run to run", k)
        assert torch.equal(g0[k], gk[k]), ("grouped against one by one", k)


# ---- (e) argument checking ----------------------------------------------------------------------------------------------------------
BAD_FIELDS = [("part", None), ("dW", None), ("splits", 0), ("splits", -1), ("RS", 0), ("RS", -3), ("Ci", 0), ("Ci", -1), ("Co", 0),
              ("Co", -4)]


def test_empty_and_null_tables_are_refused():
    lib, ops = _gpu()
    assert ops.wgrad_reduce_group([], check=False) == BADARG
    e = _Entry(ops, CASES[0], 2, "int", seed=1)
    assert lib.fn("umi_wgrad_reduce_group")(1, None, None) == BADARG
    assert lib.fn("umi_wgrad_reduce_group")(-1, None, None) == BADARG
    torch.cuda.synchronize()
    assert (e.buf == SENTINEL).all()


@pytest.mark.parametrize("field,value", BAD_FIELDS)
@pytest.mark.parametrize("n", [1, 17])
def test_a_bad_entry_anywhere_is_refused_before_anything_is_launched(field, value, n):
    """The bad entry is the LAST of n: with n = 17 it sits in the second chunk of 16, and the 16 valid reductions in front of it
    must not have run."""
    lib, ops = _gpu()
    entries = [_Entry(ops, CASES[i % 8], 2, "int", seed=i) for i in range(n)]
    pend = [e.pending for e in entries]
    setattr(pend[-1], field, value)
    assert ops.wgrad_reduce_group(pend, check=False) == BADARG
    with pytest.raises(RuntimeError, match="UMI_ERR_BADARG"):
        ops.wgrad_reduce_group(pend)
    torch.cuda.synchronize()
    for i, e in enumerate(entries):
        assert (e.buf == SENTINEL).all(), (i, "was written")
