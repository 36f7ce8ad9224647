"""Guarded optimizer step, host side: the arithmetic of umi_grad_guard_finalize as umi.optim.guard_update_numpy states it, the C
entry points' argument checks and the refusals of umi.optim -- nothing here touches a GPU (tests/test_gpu_grad_guard.py does)."""
import numpy as np
import pytest
import torch

from umi import lib
from umi import optim as uo

G = uo.GUARD


def _state(**kw):
    return uo.GradGuard(**kw).initial.copy()


# ---- scale state machine against torch.amp.GradScaler ---------------------------------------------------------------------------

def _grad_scaler_run(init, interval, bad, steps):
    """(scale, growth tracker, skipped?) after each of `steps` steps of torch's CPU GradScaler; `bad`: steps with an inf gradient."""
    p = torch.nn.Parameter(torch.zeros(3))
    opt = torch.optim.SGD([p], lr=1.0)
    sc = torch.amp.GradScaler("cpu", init_scale=float(init), growth_interval=interval)
    out = []
    for i in range(steps):
        opt.zero_grad()
        sc.scale((p * 1.0).sum()).backward()
        if i in bad:
            p.grad[1] = float("inf")
        before = p.detach().clone()
        sc.step(opt)
        skipped = bool(torch.equal(before, p.detach()))
        sc.update()
        out.append((sc.get_scale(), sc._get_growth_tracker(), skipped))
    return out


@pytest.mark.parametrize("init,interval,bad,steps,scales", [
    (4.0, 3, {3, 6, 7}, 12, [4, 4, 8, 4, 4, 4, 2, 1, 1, 1, 2, 2]),
    (4.0, 3, set(), 6, [4, 4, 8, 8, 8, 16]),                      # no bad step over two intervals
    (4.0, 3, set(range(5)), 5, [2, 1, 0.5, 0.25, 0.125]),         # every step bad
    (1.0, 1, {1, 2}, 6, None),                                    # interval 1: grows on every clean step
])
def test_scale_state_machine_follows_grad_scaler(init, interval, bad, steps, scales):
    ref = _grad_scaler_run(init, interval, bad, steps)
    if scales is not None:
        assert [r[0] for r in ref] == scales
    st = _state(dynamic_scale=True, init_scale=init, growth_interval=interval, min_scale=2.0 ** -100, max_scale=2.0 ** 100)
    for i, (scale, streak, skipped) in enumerate(ref):
        st = uo.guard_update_numpy(st, 4.0, 1 if i in bad else 0)
        assert (st[G["SCALE"]], st[G["STREAK"]], bool(st[G["SKIP"]])) == (scale, streak, skipped), i
        assert skipped == (i in bad)
    assert st[G["STEPS"]] == steps and st[G["SKIPPED"]] == len(bad)


def test_scale_clamps():
    st = _state(dynamic_scale=True, init_scale=4.0, growth_interval=1, min_scale=1.5, max_scale=6.0)
    st = uo.guard_update_numpy(st, 1.0, 0)
    assert st[G["SCALE"]] == 6.0                                  # min(4 * 2, 6)
    st = uo.guard_update_numpy(st, 1.0, 0)
    assert st[G["SCALE"]] == 6.0
    for want in (3.0, 1.5, 1.5):                                  # max(d / 2, 1.5)
        st = uo.guard_update_numpy(st, 1.0, 2)
        assert st[G["SCALE"]] == want
    st = _state(dynamic_scale=False, init_scale=4.0)              # static: the scale never moves
    for k in (0, 3, 0):
        st = uo.guard_update_numpy(st, 1.0, k)
        assert st[G["SCALE"]] == 4.0 and st[G["STREAK"]] == 0.0


# ---- clip coefficient and counters ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_norm", [None, 1.0, 1e-3])
@pytest.mark.parametrize("d", [1.0, 0.25, 8.0])
def test_clip_coefficient_and_counters(max_norm, d):
    g = np.random.default_rng(3).standard_normal(1000).astype(np.float32)
    S = float(np.sum(g.astype(np.float64) ** 2))                  # the gradients carry d: S is of g * d
    st0 = _state(max_norm=max_norm, init_scale=d)
    st = uo.guard_update_numpy(st0, S * d * d, 0)
    norm = np.sqrt(np.float64(S * d * d)) / d
    want = (1.0 if max_norm is None else min(1.0, max_norm / (norm + 1e-6))) / d
    assert st[G["NORM"]] == norm and st[G["COEF"]] == want and st[G["SKIP"]] == 0.0 and st[G["NONFINITE"]] == 0.0
    clipped = max_norm is not None and max_norm / (norm + 1e-6) < 1.0
    assert clipped == (max_norm == 1e-3 or max_norm == 1.0)      # ||g|| is about 31
    assert (st[G["STEPS"]], st[G["SKIPPED"]], st[G["CLIPPED"]]) == (1.0, 0.0, float(clipped))
    assert st[G["SCALE"]] == d
    st2 = uo.guard_update_numpy(st, np.inf, 3)                    # a step with three non-finite elements
    assert st2[G["COEF"]] == 0.0 and st2[G["SKIP"]] == 1.0 and st2[G["NONFINITE"]] == 3.0 and np.isinf(st2[G["NORM"]])
    assert (st2[G["STEPS"]], st2[G["SKIPPED"]], st2[G["CLIPPED"]]) == (2.0, 1.0, float(clipped))
    st3 = uo.guard_update_numpy(st2, np.nan, 1)
    assert np.isnan(st3[G["NORM"]]) and st3[G["SKIPPED"]] == 2.0 and st3[G["COEF"]] == 0.0
    np.testing.assert_array_equal(st0[G["MAX_NORM"]:], st3[G["MAX_NORM"]:])      # the settings are never written


def test_small_norm_is_not_clipped():
    st = uo.guard_update_numpy(_state(max_norm=1.0), 0.25, 0)
    assert st[G["COEF"]] == 1.0 and st[G["CLIPPED"]] == 0.0 and st[G["NORM"]] == 0.5


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------

def test_guard_constants_come_from_the_header():
    names = ["NORM", "NONFINITE", "COEF", "SKIP", "SCALE", "STREAK", "STEPS", "SKIPPED", "CLIPPED", "MAX_NORM",
             "GROWTH_INTERVAL", "GROWTH", "BACKOFF", "MIN_SCALE", "MAX_SCALE", "SPARE"]
    assert [getattr(lib, "UMI_GUARD_" + n) for n in names] == list(range(16))
    assert lib.UMI_GUARD_LEN == uo.GUARD_LEN == 16 and sorted(G, key=G.get) == names
    assert "umi_optim_hyper" in lib.STRUCTS and len(lib.STRUCTS) == 5           # the guard block is an array, not a struct


def test_workspace_size_grows_with_the_blocks():
    ws = lib.fn("umi_grad_guard_ws_bytes")
    assert ws(0) == 0 and ws(-3) == 0
    sizes = [ws(n) for n in (1, 2, 31, 30000)]
    assert sizes == sorted(set(sizes)) and sizes[0] >= 16 and all(b % 8 == 0 for b in sizes)


def test_bad_arguments_return_status_before_any_launch():
    import ctypes
    bad = lib.UMI_ERR_BADARG
    buf = (ctypes.c_double * 66)()
    a = (ctypes.addressof(buf) + 15) & ~15                         # a non-null, 16-byte aligned address that is never followed
    part = lib.fn("umi_grad_norm_partials")
    assert part(None, 1, 1, 0, a, 512, None) == bad
    assert part(a, 1, 1, 0, None, 512, None) == bad
    assert part(a, 0, 1, 0, a, 512, None) == bad
    assert part(a, 1, 0, 0, a, 512, None) == bad
    assert part(a, 1, -1, 0, a, 512, None) == bad
    assert part(a, 1, 1, -1, a, 512, None) == bad
    assert part(a, 1, 1, 0, a + 4, 512, None) == bad and part(a, 1, 1, 0, a + 8, 512, None) == bad      # ws: 16-byte aligned
    assert part(a, 1, 8, 0, a, 16 * 8 - 1, None) == lib.UMI_ERR_WORKSPACE
    assert part(a, 1, 4, 4, a, 16 * 8 - 1, None) == lib.UMI_ERR_WORKSPACE
    fin = lib.fn("umi_grad_guard_finalize")
    assert fin(None, 1, a, None) == bad and fin(a, 1, None, None) == bad and fin(a, 0, a, None) == bad
    assert fin(a, -2, a, None) == bad and fin(a, 1, a + 4, None) == bad and fin(a + 8, 1, a, None) == bad
    pre = lib.fn("umi_optim_hyper_pre_guarded")
    assert pre(None, 1, a, None) == bad and pre(a, 1, None, None) == bad and pre(a + 4, 0, a, None) == bad
    sgd = lib.fn("umi_optim_sgd_multi_guarded")
    ok = (a, 1, 1, None, 0.1, 0.9, 0.0, 0.0, 0, 0, a, None)

    def but(i, v):
        return ok[:i] + (v,) + ok[i + 1:]
    for args in (but(0, None), but(1, 0), but(2, 0), but(2, -1), but(10, None), but(6, 0.1)):      # 6: dampening != 0
        assert sgd(*args) == bad
    adam = lib.fn("umi_optim_adam_multi_guarded")
    ok = (a, 1, 1, None, 1e-3, 0.9, 0.999, 1.0, 1e-8, 0.0, a, None)
    for args in (but(0, None), but(1, 0), but(1, -5), but(2, 0), but(10, None)):
        assert adam(*args) == bad


# ---- host-side refusals -----------------------------------------------------------------------------------------------------------

def _param():
    p = torch.nn.Parameter(torch.zeros(4))
    p.grad = torch.ones(4)
    return p


def test_guard_refuses_dampening():
    with pytest.raises(ValueError, match="dampening"):
        uo.SGD([_param()], lr=0.1, momentum=0.9, dampening=0.1).grad_guard(uo.GradGuard())
    opt = uo.SGD([_param()], lr=0.1, momentum=0.9).grad_guard(uo.GradGuard())
    assert opt.guard is not None and opt.grad_guard(None).guard is None


def test_guarded_adam_needs_the_device_block():
    opt = uo.Adam([_param()], lr=1e-3).grad_guard(uo.GradGuard(max_norm=1.0))
    with pytest.raises(RuntimeError, match=r"device_schedule\(\)"):
        opt.step()


def test_guard_cannot_be_attached_after_a_capture():
    opt = uo.SGD([_param()], lr=0.1)
    t = uo._Table()
    t.captured.add(0)                                              # what _Table.get records when its upload is captured
    opt._umi_tables = {(0, False, True): t}
    with pytest.raises(RuntimeError, match="capture"):
        opt.grad_guard(uo.GradGuard())
    with pytest.raises(TypeError):
        uo.SGD([_param()], lr=0.1).grad_guard(object())


def test_guard_argument_checks_and_initial_read():
    for kw in (dict(max_norm=0.0), dict(max_norm=-1.0), dict(init_scale=0.0), dict(init_scale=float("inf")),
               dict(dynamic_scale=True, growth_interval=0), dict(dynamic_scale=True, backoff_factor=1.0),
               dict(dynamic_scale=True, min_scale=2.0, max_scale=1.0)):
        with pytest.raises(ValueError):
            uo.GradGuard(**kw)
    r = uo.GradGuard(init_scale=8.0).read()                        # before any step: nothing on the device yet
    assert r == dict(norm=0.0, nonfinite=0, skipped=0, clipped=0, steps=0, scale=8.0)
