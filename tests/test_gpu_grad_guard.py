"""Guarded optimizer step on the MI355X, kernel level: the multi-tensor norm / non-finite pass, the finalize kernel and the guarded
SGD / Adam updates, on one parameter set built to reach every path of the kernels (sizes around the 4096-element block and the
4-element vector, a run of small tensors for the table's binary search, misaligned gradients, a parameter without a gradient, two
param groups).  The tape and Trainer side runs in child processes (tools/check_grad_guard.py)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = [1, 3, 4, 5, 4095, 4096, 4097, 8191, 12289] + [64 + (i * 37) % 449 for i in range(30)] + [2048, 16384, 20000, 30000]
MISALIGNED = {1000: 43, 5000: 44}          # size -> position: .grad starts one float past a 16-byte boundary
NO_GRAD = 20                               # position of the parameter whose .grad is None
SPLIT = 25                                 # param group 0: positions [0, SPLIT), group 1: the rest


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")


def _grads(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    sizes = list(SIZES)
    for n, pos in sorted(MISALIGNED.items(), key=lambda kv: kv[1]):
        sizes.insert(pos, n)
    return sizes, [torch.randn(n, generator=g) * scale for n in sizes]


def _set_grads(params, grads):
    for i, (p, g) in enumerate(zip(params, grads)):
        if i == NO_GRAD:
            p.grad = None
        elif p.numel() in MISALIGNED:
            if p.grad is None:
                p.grad = torch.empty(p.numel() + 4, device="cuda")[1:1 + p.numel()]
                assert p.grad.data_ptr() % 16 == 4
            p.grad.copy_(g)
        else:
            p.grad = g.to("cuda")


def _make(kind, dev, guard, seed=1):
    """(params, optimizer) of the test's parameter set; `guard`: a GradGuard or None."""
    from umi import optim as uo
    sizes, init = _grads(100 + seed)
    params = [torch.nn.Parameter(v.to("cuda")) for v in init]
    groups = [dict(params=params[:SPLIT]), dict(params=params[SPLIT:])]
    if kind == "adam":
        opt = uo.Adam(groups, lr=2e-3, weight_decay=1e-4)
    else:
        opt = uo.SGD(groups, lr=0.05, momentum=0.9 if kind == "sgd_mom" else 0.0, weight_decay=1e-4 if kind == "sgd_mom" else 0.0)
    if dev:
        opt.device_schedule(poly=dict(base_lr=opt.param_groups[0]["lr"], max_iterations=10, power=0.9))
    if guard is not None:
        opt.grad_guard(guard)
    return params, opt


def _snapshot(params, opt):
    out = [p.detach().clone() for p in params]
    for p in params:
        for k in ("momentum_buffer", "exp_avg", "exp_avg_sq"):
            v = opt.state.get(p, {}).get(k)
            if v is not None:
                out.append(v.detach().clone())
    return out


def _adam_t(opt):
    return [float(h["adam_t"]) for h in opt.sync_host()]


def _same_bits(a, b):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), i


def _state(guard):
    torch.cuda.synchronize()
    return guard.state.cpu().numpy().copy()


def _numel(grads):
    return sum(g.numel() for i, g in enumerate(grads) if i != NO_GRAD)


# ---- norm -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale,d", [(1.0, 1.0), (1e25, 1.0), (3e-3, 0.125)])
def test_norm_against_float64(scale, d):
    """NORM against the correctly rounded float64 sum of the same fp32 gradients' squares (math.fsum).  Squares of fp32 values are
    exact in double and a sum of n non-negative terms in any order is within (n - 1) * 2^-53 relative, so the bar is n * 2^-53
    relative plus 2 ulp for the square root and the division.  At |g| ~ 1e25 an fp32 sum of squares would overflow."""
    _gpu()
    from umi import optim as uo
    _, grads = _grads(7, scale)
    states = []
    for _ in range(2):
        guard = uo.GradGuard(init_scale=d)
        params, opt = _make("sgd_plain", False, guard)
        _set_grads(params, grads)
        opt.step()
        states.append(_state(guard))
    G = uo.GUARD
    flat = np.concatenate([g.numpy().astype(np.float64) for i, g in enumerate(grads) if i != NO_GRAD])
    n = flat.size
    assert n == _numel(grads) and 1.0e5 < n < 1.5e5
    want = math.sqrt(math.fsum(flat * flat)) / d
    tol = n * 2.0 ** -53 + 2 * 2.0 ** -52
    got = states[0][G["NORM"]]
    print("norm", got, "want", want, "rel", abs(got - want) / want, "bar", tol)
    assert abs(got - want) <= tol * want
    assert states[0][G["NONFINITE"]] == 0 and states[0][G["SKIP"]] == 0 and states[0][G["COEF"]] == 1.0 / d
    assert states[0].tobytes() == states[1].tobytes()                     # fixed reduction order: bit-identical runs
    if scale == 1e25:
        with np.errstate(over="ignore"):
            assert not np.isfinite(np.sum((flat * flat).astype(np.float32)))


# ---- non-finite gradients: counted, and the step leaves every bit alone -----------------------------------------------------------

def _pos(size):
    sizes, _ = _grads(0)
    return sizes.index(size)


PLACES = {
    "element_0": (lambda: _pos(12289), 0),
    "last_of_a_full_block": (lambda: _pos(12289), 4095),
    "scalar_tail": (lambda: _pos(8191), 4096 + 4094),                    # second block: cnt = 4095, tail from 4092
    "misaligned_tensor": (lambda: _pos(5000), 4500),
    "last_tensor": (lambda: len(SIZES) + len(MISALIGNED) - 1, 7),
    "second_group_only": (lambda: SPLIT, 1),
}
VALUES = {"+inf": float("inf"), "-inf": float("-inf"), "nan": float("nan")}


def _plant(grads, plan):
    grads = [g.clone() for g in grads]
    for place, value in plan:
        pos, idx = PLACES[place][0](), PLACES[place][1]
        assert pos != NO_GRAD
        grads[pos][idx] = VALUES[value]
    return grads


@pytest.mark.parametrize("plan", [[(p, v)] for p in PLACES for v in VALUES]
                         + [[(p, list(VALUES)[i % 3]) for i, p in enumerate(PLACES)]],
                         ids=lambda plan: "all" if len(plan) > 1 else "%s:%s" % plan[0])
def test_nonfinite_is_counted_and_the_step_is_skipped(plan):
    _gpu()
    from umi import optim as uo
    G = uo.GUARD
    _, clean = _grads(11)
    bad = _plant(_grads(12)[1], plan)
    for kind, dev in (("sgd_mom", False), ("adam", True)):
        guard = uo.GradGuard(max_norm=5.0)
        params, opt = _make(kind, dev, guard)
        _set_grads(params, clean)
        opt.step()                                                       # a clean step first: the state holds values
        before, t0 = _snapshot(params, opt), _adam_t(opt) if dev else None
        st0 = _state(guard)
        assert st0[G["SKIP"]] == 0 and st0[G["STEPS"]] == 1
        _set_grads(params, bad)
        opt.step()
        st = _state(guard)
        assert st[G["NONFINITE"]] == len(plan) and st[G["SKIP"]] == 1 and st[G["COEF"]] == 0
        assert st[G["SKIPPED"]] == st0[G["SKIPPED"]] + 1 == 1 and st[G["STEPS"]] == 2
        _same_bits(_snapshot(params, opt), before)
        if dev:
            assert _adam_t(opt) == t0 == [1.0, 1.0]
        _set_grads(params, clean)                                        # and the step after it is applied again
        opt.step()
        st = _state(guard)
        assert st[G["SKIP"]] == 0 and st[G["NONFINITE"]] == 0 and st[G["SKIPPED"]] == 1
        assert not torch.equal(params[0], before[0])
        if dev:
            assert _adam_t(opt) == [2.0, 2.0]


# ---- update arithmetic: the parent's own kernels on gradients multiplied by float32(COEF) ---------------------------------------

@pytest.mark.parametrize("kind,dev,max_norm,d", [
    ("sgd_mom", False, 1.0, 1.0),          # clipping active (the norm is about 350)
    ("sgd_mom", True, None, 1.0),          # COEF == 1: the same gradients
    ("sgd_mom", False, 1e6, 1.0),          # max_norm above the norm: COEF == 1
    ("sgd_mom", True, 1.0, 4.0),
    ("sgd_plain", False, None, 4.0),       # COEF = 1 / 4
    ("sgd_plain", True, 1.0, 1.0),
    ("adam", True, 1.0, 0.5),
    ("adam", True, None, 1.0),
])
def test_guarded_update_is_the_unguarded_one_on_scaled_gradients(kind, dev, max_norm, d):
    _gpu()
    from umi import optim as uo
    G = uo.GUARD
    guard = uo.GradGuard(max_norm=max_norm, init_scale=d)
    pa, oa = _make(kind, dev, guard)
    pb, ob = _make(kind, dev, None)
    for step in range(3):
        _, grads = _grads(20 + step)
        _set_grads(pa, grads)
        oa.step()
        st = _state(guard)
        cf = np.float32(st[G["COEF"]])
        clip = 1.0 if max_norm is None else min(1.0, max_norm / (st[G["NORM"]] + 1e-6))
        assert st[G["COEF"]] == clip / d and st[G["CLIPPED"]] == (step + 1) * (clip < 1.0) and st[G["SKIP"]] == 0
        assert (cf == 1.0) == (d == 1.0 and max_norm in (None, 1e6))
        _set_grads(pb, grads)
        if cf != 1.0:
            c = torch.tensor(cf, device="cuda")                          # an fp32 scalar: one rounding per element
            for p in pb:
                if p.grad is not None:
                    p.grad.copy_(p.grad * c)
        ob.step()
        if step in (0, 2):
            _same_bits(_snapshot(pa, oa), _snapshot(pb, ob))
    if dev:
        ha, hb = oa.sync_host(), ob.sync_host()
        assert [h.tobytes() for h in ha] == [h.tobytes() for h in hb]


def test_skipped_first_sgd_step_zero_fills_the_momentum_buffers():
    _gpu()
    from umi import optim as uo
    _, clean = _grads(31)
    bad = _plant(_grads(32)[1], [("scalar_tail", "nan")])
    guard_a, guard_b = uo.GradGuard(), uo.GradGuard()
    pa, oa = _make("sgd_mom", False, guard_a)
    pb, ob = _make("sgd_mom", False, guard_b)
    start = _snapshot(pa, oa)
    _set_grads(pa, bad)
    oa.step()
    torch.cuda.synchronize()
    bufs = [oa.state[p]["momentum_buffer"] for p in pa if p.grad is not None]
    assert len(bufs) == len(pa) - 1 and all(int(torch.count_nonzero(b.view(torch.int32))) == 0 for b in bufs)
    _same_bits([p.detach() for p in pa], start)
    _set_grads(pa, clean)
    oa.step()
    _set_grads(pb, clean)
    ob.step()                                                            # the run whose first step is the clean one
    _same_bits([p.detach() for p in pa], [p.detach() for p in pb])
    assert guard_a.read()["skipped"] == 1 and guard_b.read()["skipped"] == 0


def test_no_stray_writes_around_workspace_and_state():
    """The entry points themselves, on buffers with sentinels around them; the workspace starts as NaN, so a row that finalize
    read without partials having written it would show in NORM."""
    _gpu()
    from umi import lib as L
    from umi import ops
    from umi import optim as uo
    G = uo.GUARD
    _, grads = _grads(41)
    gs = [g.to("cuda") for g in grads]
    ps = [torch.zeros_like(g) for g in gs]
    tabs, total = [], 0
    for part in (list(zip(ps, gs))[:SPLIT], list(zip(ps, gs))[SPLIT:]):
        t = uo._Table()
        tabs.append((t, t.get([(p.data_ptr(), g.data_ptr(), 0, 0, g.numel()) for p, g in part])))
        total += tabs[-1][1][2]
    rows_bytes = L.fn("umi_grad_guard_ws_bytes")(total)
    assert rows_bytes % 8 == 0
    PAD, MAGIC = 32, 12345.678
    big = torch.full((PAD + rows_bytes // 8 + PAD,), float("nan"), dtype=torch.float64, device="cuda")
    big[:PAD] = MAGIC
    big[-PAD:] = MAGIC
    ws = big[PAD:PAD + rows_bytes // 8]
    blk = torch.full((PAD + uo.GUARD_LEN + PAD,), MAGIC, dtype=torch.float64, device="cuda")
    state = blk[PAD:PAD + uo.GUARD_LEN]
    state.copy_(torch.from_numpy(uo.GradGuard(max_norm=2.0).initial))
    off = 0
    for _, (ptr, n, blocks) in tabs:
        L.call("umi_grad_norm_partials", ptr, n, blocks, off, ws.data_ptr(), rows_bytes, ops._stream())
        off += blocks
    L.call("umi_grad_guard_finalize", ws.data_ptr(), total, state.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert bool((big[:PAD] == MAGIC).all()) and bool((big[-PAD:] == MAGIC).all())
    assert bool((blk[:PAD] == MAGIC).all()) and bool((blk[-PAD:] == MAGIC).all())
    assert not bool(torch.isnan(ws).any())
    st = state.cpu().numpy()
    flat = np.concatenate([g.numpy().astype(np.float64) for g in grads])
    want = math.sqrt(math.fsum(flat * flat))
    assert abs(st[G["NORM"]] - want) <= (flat.size * 2.0 ** -53 + 2 * 2.0 ** -52) * want
    init = uo.GradGuard(max_norm=2.0).initial
    assert st[G["COEF"]] == 2.0 / (st[G["NORM"]] + 1e-6) < 1.0 and st[G["NONFINITE"]] == 0 and st[G["SKIP"]] == 0
    assert (st[G["SCALE"]], st[G["STREAK"]], st[G["STEPS"]], st[G["SKIPPED"]], st[G["CLIPPED"]]) == (1.0, 0.0, 1.0, 0.0, 1.0)
    assert np.array_equal(st[G["MAX_NORM"]:], init[G["MAX_NORM"]:])
    for g, p in zip(gs, ps):                                             # reads g only
        assert int(torch.count_nonzero(p)) == 0
    for g, g0 in zip(gs, grads):
        assert torch.equal(g.cpu(), g0)


# ---- tape and Trainer: child processes ----------------------------------------------------------------------------------------------

def _run(what, marker):
    _gpu()
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_grad_guard.py"), what],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and marker in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])


def test_dynamic_factor_is_exact_in_fp32():
    """Two guarded SGD steps of the fp32 U-Net with SCALE fixed at 2^-3, 1 and 2^5: bit-identical parameters (every backward
    kernel is linear in the incoming gradient and a power of two scales every intermediate exactly)."""
    _run("exact", "GUARD_EXACT_OK")


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_recovery_from_an_overflowing_scale_eager_and_replayed(kind):
    """fp16, init_scale 2^30: the first steps overflow and are skipped with the parameters untouched, the scale halves until a step
    applies (within 40 steps), the loss falls afterwards; eagerly and under GraphedStep replay, with matching counters, Adam's
    step count == applied steps and the poly block's iteration == all steps."""
    _run("recover_" + kind, "GUARD_RECOVER_OK")


def test_trainer_logs_the_guard_line():
    _run("trainer", "GUARD_TRAINER_OK")
