"""umi.optim.AdamW, the decoupled-decay update kernels and the warm-up + decay schedule kernel on the MI355X.

Tensor sizes are chosen where the update can go wrong, not from a model: 1, 2, 3, 5 and 35 elements (scalar tail only, and a
float4 body with a tail), 4095 / 4096 / 4097 (one block of 4,096, full, and one element into a second block), 8193 (third block)
and 300 x 41; once with aligned gradients, once with gradients that are views 3 floats into a flat buffer (the path without
16-byte accesses).

Bars.  Against torch.optim.AdamW(foreach=True): those of tests/test_gpu_kernels.py::test_optim_adam_matches_torch (the kernel
follows torch's operation order; fma contraction may differ by an ulp of an O(1) intermediate).  The decay factor itself, the
skipped step and the entry-point variants are pinned bit for bit.  Schedule kernel: 1e-12 relative on the double LR (the
device's pow / cos against libm; an off-by-one in k or a missing warm-up term moves the values by more than 1e-3), in units of
the base LR where the rule gives exactly 0; the fp32 fields derived from device pow() within 2 ulp of fp32."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

if __name__ == "__main__":                                  # the child process of the graph-replay case
    _REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_REPO, os.path.join(_REPO, "unet-torch_amd")]

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(1,), (2,), (3,), (5,), (35,), (4095,), (4096,), (4097,), (8193,), (300, 41)]
KWS = [dict(lr=1e-3, weight_decay=1e-2), dict(lr=5e-4, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.1)]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: torch.cuda.is_available() is False")


def _bits(t):
    return t.detach().cpu().contiguous().reshape(-1).view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _block(opt, gi=0):
    from umi import optim as uo
    torch.cuda.synchronize()
    return opt.device_hyper[gi][0].cpu().numpy().view(uo._HYPER)[0].copy()


def _fresh(seed=5):
    gen = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, generator=gen).to(DEV)) for s in SIZES]
    flat = torch.zeros(3 + sum(p.numel() for p in params), device=DEV)
    return gen, params, flat


def _set_grads(params, flat, grads, flat_grads):
    off = 3                                                 # misaligned start: the views are only 4-byte aligned
    for p, g in zip(params, grads):
        g = g.to(DEV)
        if flat_grads:
            v = flat[off:off + p.numel()].view(p.shape)
            v.copy_(g)
            p.grad = v
            off += p.numel()
        else:
            p.grad = g


def _run(make, steps, flat_grads, grads=None, rewrite=True, before_step=None):
    """`steps` steps of make(params) on seeded gradients (or `grads(step, params)`); the LR of every group is rewritten after
    step 2, as a host schedule would.  Returns (params, optimizer)."""
    gen, params, flat = _fresh()
    opt = make(params)
    for s in range(steps):
        drawn = [torch.randn(p.shape, generator=gen) * (0.5 + s) for p in params]
        _set_grads(params, flat, drawn if grads is None else grads(s, params), flat_grads)
        if s == 2 and rewrite:
            for group in opt.param_groups:
                group["lr"] *= 0.7
        if before_step is not None:
            before_step(s, opt, params)
        opt.step()
    torch.cuda.synchronize()
    return params, opt


_REF = {}


def _torch_adamw(i, flat_grads):
    """The reference run, computed once per case and shared: (parameters, optimizer state) on the host."""
    if (i, flat_grads) not in _REF:
        ps, opt = _run(lambda p: torch.optim.AdamW(p, foreach=True, **KWS[i]), 6, flat_grads)
        st = opt.state_dict()["state"]
        _REF[i, flat_grads] = ([p.detach().cpu() for p in ps],
                               {k: {n: v.detach().cpu() for n, v in s.items()} for k, s in st.items()})
    return _REF[i, flat_grads]


def _close(mine, opt, ref, ref_state):
    """None when the run holds the bars of test_optim_adam_matches_torch, else the first miss."""
    for j, (a, b) in enumerate(zip(mine, ref)):
        if not torch.allclose(a.detach().cpu(), b, rtol=5e-6, atol=2e-7):
            return f"parameter {j} {tuple(b.shape)}: max |diff| {(a.detach().cpu() - b).abs().max().item():.3e}"
    st = opt.state_dict()["state"]
    if st.keys() != ref_state.keys():
        return "other parameters have state"
    for k in st:
        if st[k].keys() != ref_state[k].keys() or float(st[k]["step"]) != float(ref_state[k]["step"]):
            return f"state {k}: keys or step count differ ({float(st[k]['step'])} / {float(ref_state[k]['step'])})"
        for name in ("exp_avg", "exp_avg_sq"):
            if not torch.allclose(st[k][name].cpu(), ref_state[k][name], rtol=5e-6, atol=1e-6):
                return f"state {k}.{name}: max |diff| {(st[k][name].cpu() - ref_state[k][name]).abs().max().item():.3e}"
    return None


@pytest.mark.parametrize("flat_grads", [False, True], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("i", [0, 1])
def test_adamw_matches_torch_adamw(i, flat_grads):
    from umi import optim as uo
    ref, ref_state = _torch_adamw(i, flat_grads)
    assert all(float(s["step"]) == 6.0 for s in ref_state.values())
    mine, opt = _run(lambda p: uo.AdamW(p, **KWS[i]), 6, flat_grads)
    assert _close(mine, opt, ref, ref_state) is None, _close(mine, opt, ref, ref_state)
    mine, opt = _run(lambda p: uo.Adam(p, decoupled_weight_decay=True, **KWS[i]), 6, flat_grads)
    assert _close(mine, opt, ref, ref_state) is None, _close(mine, opt, ref, ref_state)
    # L2 decay on the same inputs is another trajectory: the bars tell the two apart
    mine, opt = _run(lambda p: uo.Adam(p, **KWS[i]), 6, flat_grads)
    miss = _close(mine, opt, ref, ref_state)
    assert miss is not None and miss.startswith("parameter"), miss


# ---- exact cases ---------------------------------------------------------------------------------------------------------------

def _zeros(s, params):
    return [torch.zeros(p.shape) for p in params]


@pytest.mark.parametrize("flat_grads", [False, True], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("device_block", [False, True], ids=["host", "dev"])
def test_zero_gradient_step_is_the_decay_factor_alone(flat_grads, device_block):
    from umi import optim as uo
    lr, wd = 1e-3, 0.1
    _, before, _ = _fresh()

    def make(p):
        opt = uo.AdamW(p, lr=lr, weight_decay=wd)
        return opt.device_schedule() if device_block else opt
    after, opt = _run(make, 1, flat_grads, grads=_zeros, rewrite=False)
    factor = np.float32(1.0 - lr * wd)                      # formed in double, ONE rounding to fp32
    assert float(factor) != 1.0 - lr * wd                   # (the rounding is there to be seen)
    for b, a in zip(before, after):
        want = (b.detach().cpu().numpy() * factor).astype(np.float32)
        assert np.array_equal(a.detach().cpu().numpy().view(np.int32), want.view(np.int32)), tuple(b.shape)
        st = opt.state[a]
        assert not bool(st["exp_avg"].any()) and not bool(st["exp_avg_sq"].any())
    assert all(float(s["step"]) == 1.0 for s in opt.state_dict()["state"].values())


@pytest.mark.parametrize("flat_grads", [False, True], ids=["aligned", "unaligned"])
def test_without_weight_decay_adamw_is_adam_bit_for_bit(flat_grads):
    from umi import optim as uo
    a, oa = _run(lambda p: uo.AdamW(p, lr=1e-3, weight_decay=0.0), 3, flat_grads)
    b, ob = _run(lambda p: uo.Adam(p, lr=1e-3, weight_decay=0.0), 3, flat_grads)
    for x, y in zip(a, b):
        assert _same_bits(x, y), tuple(x.shape)
        assert _same_bits(oa.state[x]["exp_avg"], ob.state[y]["exp_avg"])
        assert _same_bits(oa.state[x]["exp_avg_sq"], ob.state[y]["exp_avg_sq"])


@pytest.mark.parametrize("flat_grads", [False, True], ids=["aligned", "unaligned"])
def test_host_dev_and_guarded_entry_points_agree_bit_for_bit(flat_grads):
    """Constant LR, guard inactive (no clipping, scale 1: COEF = 1): the three entry points run the same arithmetic."""
    from umi import optim as uo
    kw = dict(lr=1e-3, weight_decay=0.05)
    guard = uo.GradGuard()
    runs = [_run(lambda p: uo.AdamW(p, **kw), 3, flat_grads, rewrite=False),
            _run(lambda p: uo.AdamW(p, **kw).device_schedule(), 3, flat_grads, rewrite=False),
            _run(lambda p: uo.AdamW(p, **kw).device_schedule().grad_guard(guard), 3, flat_grads, rewrite=False)]
    r = guard.read()
    assert (r["steps"], r["skipped"], r["clipped"], r["scale"]) == (3, 0, 0, 1.0)
    assert float(guard.state.cpu()[uo.GUARD["COEF"]]) == 1.0
    (p0, o0), rest = runs[0], runs[1:]
    for what, (p1, o1) in zip(("dev", "guarded"), rest):
        assert _block(o1)["adam_t"] == 3.0
        for x, y in zip(p0, p1):
            assert _same_bits(x, y), (what, tuple(x.shape))
            assert _same_bits(o0.state[x]["exp_avg"], o1.state[y]["exp_avg"]), (what, tuple(x.shape))
            assert _same_bits(o0.state[x]["exp_avg_sq"], o1.state[y]["exp_avg_sq"]), (what, tuple(x.shape))


@pytest.mark.parametrize("flat_grads", [False, True], ids=["aligned", "unaligned"])
def test_skipped_step_stores_nothing_and_applies_no_decay(flat_grads):
    """Steps: clean, one inf planted (skipped), clean.  After the skipped step p, exp_avg, exp_avg_sq and adam_t keep their
    bits -- no decay either --, and the run ends where a run of the two clean steps alone ends."""
    from umi import optim as uo
    kw = dict(lr=1e-3, weight_decay=0.1)
    gen = torch.Generator().manual_seed(11)
    clean = [[torch.randn(s, generator=gen) for s in SIZES] for _ in range(2)]
    poisoned = [g.clone() for g in clean[1]]
    poisoned[7].view(-1)[4096] = float("inf")               # 4097 elements: the one element of its second block
    seen = {}

    def watch(s, opt, params):
        if s in (1, 2):                                     # before the skipped step, and before the step after it
            seen[s] = ([_bits(p) for p in params], [_bits(opt.state[p][n]) for p in params for n in ("exp_avg", "exp_avg_sq")],
                       _block(opt)["adam_t"], _block(opt)["iter"])
    guard = uo.GradGuard()
    sched = dict(kind="constant", max_iterations=10)
    got, opt = _run(lambda p: uo.AdamW(p, **kw).device_schedule(schedule=sched).grad_guard(guard), 3, flat_grads,
                    grads=lambda s, params: [clean[0], poisoned, clean[1]][s], rewrite=False, before_step=watch)
    assert guard.read()["skipped"] == 1 and guard.read()["steps"] == 3 and guard.read()["nonfinite"] == 0
    assert seen[1][2] == seen[2][2] == 1.0                  # adam_t did not advance ...
    assert (seen[1][3], seen[2][3]) == (1.0, 2.0)           # ... the schedule's count of attempted steps did
    for a, b in zip(seen[1][0] + seen[1][1], seen[2][0] + seen[2][1]):
        assert torch.equal(a, b)
    want, ref = _run(lambda p: uo.AdamW(p, **kw).device_schedule(), 2, flat_grads, grads=lambda s, params: clean[s], rewrite=False)
    assert _block(opt)["adam_t"] == _block(ref)["adam_t"] == 2.0 and _block(opt)["iter"] == 3.0
    for x, y in zip(got, want):
        assert _same_bits(x, y), tuple(x.shape)
        assert _same_bits(opt.state[x]["exp_avg"], ref.state[y]["exp_avg"])
        assert _same_bits(opt.state[x]["exp_avg_sq"], ref.state[y]["exp_avg_sq"])


def test_decay_uses_this_step_s_lr_from_the_block():
    """Zero gradients under a warming-up poly rule: p_{k+1} = fp32(p_k * fp32(1 - lr_k * wd)) with lr_k the double the block
    holds BEFORE step k -- not lr_f, not the LR of the step before, not the base LR."""
    from umi import optim as uo
    base, wd = 1e-2, 0.1
    sched = dict(kind="poly", warmup=4, max_iterations=8)
    _, params, flat = _fresh()
    opt = uo.AdamW(params, lr=base, weight_decay=wd).device_schedule(schedule=sched)
    lrs = []
    for k in range(5):
        _set_grads(params, flat, _zeros(k, params), flat_grads=bool(k % 2))
        lr_k = float(_block(opt)["lr"])
        lrs.append(lr_k)
        assert abs(lr_k - uo.schedule_lr(k, base, **sched)) <= 1e-12 * uo.schedule_lr(k, base, **sched)
        before = [p.detach().cpu().numpy().copy() for p in params]
        opt.step()
        torch.cuda.synchronize()
        factor = np.float32(1.0 - lr_k * wd)
        for b, p in zip(before, params):
            want = (b * factor).astype(np.float32)
            assert np.array_equal(p.detach().cpu().numpy().view(np.int32), want.view(np.int32)), (k, tuple(b.shape))
    assert len({np.float32(1.0 - lr * wd) for lr in lrs}) == 5          # five different factors: the cases tell the LRs apart
    assert lrs[0] == base * (0.25 * 1.0) and lrs[1] > lrs[0]


# ---- the schedule kernel -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("final_ratio", [0.0, 0.01])
@pytest.mark.parametrize("warmup", [0, 3])
@pytest.mark.parametrize("kind", ["cosine", "poly", "constant"])
def test_schedule_kernel_follows_schedule_lr(kind, warmup, final_ratio):
    from umi import optim as uo
    bases, betas = [2e-3, 5e-4], (0.9, 0.999)
    sched = dict(kind=kind, warmup=warmup, max_iterations=16, power=0.9, final_ratio=final_ratio)
    ps = [torch.nn.Parameter(torch.ones(5, device=DEV)) for _ in bases]
    opt = uo.AdamW([dict(params=[p], lr=b) for p, b in zip(ps, bases)], betas=betas, weight_decay=0.01)
    opt.device_schedule(schedule=sched)
    for gi, b in enumerate(bases):                          # as built: the LR of step 0
        h = _block(opt, gi)
        assert h["iter"] == 0.0 and h["base_lr"] == b and h["lr"] == uo.schedule_lr(0, b, **sched)
    ulp2 = 2 * 2.0 ** -23
    for k in range(20):
        for p in ps:
            p.grad = torch.full_like(p, 0.1)
        before = [float(_block(opt, gi)["lr"]) for gi in range(2)]
        opt.step()
        for gi, b in enumerate(bases):
            h = _block(opt, gi)
            assert h["iter"] == float(k + 1) and h["adam_t"] == float(k + 1)
            want = uo.schedule_lr(k + 1, b, **sched)
            assert abs(float(h["lr"]) - want) <= 1e-12 * (abs(want) if want != 0.0 else b), (k, gi, float(h["lr"]), want)
            assert h["lr_f"] == np.float32(before[gi])      # what the update of step k read
            t = k + 1
            assert abs(float(h["step_size_f"]) - before[gi] / (1.0 - betas[0] ** t)) <= ulp2 * before[gi] / (1.0 - betas[0] ** t)
            assert abs(float(h["bc2_sqrt_f"]) - (1.0 - betas[1] ** t) ** 0.5) <= ulp2 * (1.0 - betas[1] ** t) ** 0.5
            assert (h["kind"], h["warmup"], h["final_ratio"], h["max_iter"]) == (uo.SCHEDULE_KINDS[kind], warmup, final_ratio, 16.0)
    opt.sync_host()
    assert [g["lr"] for g in opt.param_groups] == [float(_block(opt, gi)["lr"]) for gi in range(2)]
    # load_state_dict rebuilds the blocks: the rule, every group's base LR and the iteration count stay
    opt.load_state_dict(opt.state_dict())
    for gi, b in enumerate(bases):
        h = _block(opt, gi)
        assert (h["iter"], h["base_lr"], h["adam_t"], h["kind"]) == (20.0, b, 20.0, uo.SCHEDULE_KINDS[kind])
        assert h["lr"] == uo.schedule_lr(20, b, **sched)


# ---- graph replay --------------------------------------------------------------------------------------------------------------

def test_graphed_adamw_with_a_cosine_schedule_follows_the_eager_trajectory():
    """The comparison (and the bars) of tools/check_graphed_schedule.py 'optim', which
    test_graphed_sgd_poly_and_adam_follow_eager_trajectory runs for Adam: replayed steps on the device rule against eager steps
    of the same class with the rule applied on the host.  In a child process, as there: a capture that is refused half way
    belongs in a process of its own."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "graph"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "GRAPHED_ADAMW_OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])


def _child_graph():
    import copy
    import Model
    import loss as L
    from umi import optim as uo
    from umi.graphs import GraphedStep
    L.CLASS_NUMBER = 2
    torch.manual_seed(21)
    base_model = Model.UNet(1, 2, 8, compute_dtype="fp32").to(DEV).train()
    x = torch.randn(2, 1, 32, 32, device=DEV)
    lab = torch.randint(0, 2, (2, 32, 32), device=DEV).float()
    BASE, sched = 2e-3, dict(kind="cosine", warmup=3, max_iterations=10)

    def mk(model):
        return uo.AdamW(uo.decay_groups(model, 1e-2), lr=BASE)

    def step_fn(model, opt):
        def step(xx, yy):
            loss = L.calc_loss(model(xx), yy, loss_type="dice_bce_mc")
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            return loss.detach()
        return step

    m_x = copy.deepcopy(base_model)                         # capture without the device block: refused, not silently wrong
    try:
        GraphedStep(step_fn(m_x, mk(m_x)), [x, lab], warmup=1)
        raise SystemExit("AdamW capture without device_schedule() did not raise")
    except RuntimeError as e:
        assert "device_schedule" in str(e) and "umi.optim.AdamW" in str(e), e
    torch.cuda.synchronize()

    m_g, m_e = copy.deepcopy(base_model), copy.deepcopy(base_model)
    o_g, o_e = mk(m_g), mk(m_e)
    o_g.device_schedule(schedule=sched)
    gs = GraphedStep(step_fn(m_g, o_g), [x, lab], warmup=2, optimizers=[o_g])
    se = step_fn(m_e, o_e)
    losses_g, losses_e = [], []
    for i in range(6):
        if i >= 2:                                          # steps 0, 1 ran inside GraphedStep (eagerly, on the device rule)
            losses_g.append(float(gs(x, lab)))
        for g_ in o_e.param_groups:
            g_["lr"] = uo.schedule_lr(i, BASE, **sched)     # host-side rule: step i runs on rule(i)
        losses_e.append(float(se(x, lab)))
    np.testing.assert_allclose(losses_g, losses_e[2:], rtol=2e-5, atol=1e-6)
    for pg, pe in zip(m_g.parameters(), m_e.parameters()):
        torch.testing.assert_close(pg, pe, rtol=2e-4, atol=2e-6)
    hs = o_g.sync_host()
    assert len(hs) == 2 and all(int(h["iter"]) == 6 and h["adam_t"] == 6.0 for h in hs)
    for g_ in o_g.param_groups:
        assert abs(g_["lr"] - uo.schedule_lr(6, BASE, **sched)) < 1e-12 * BASE + 1e-15, g_["lr"]
    assert all(float(v["step"]) == 6.0 for v in o_g.state_dict()["state"].values())
    print("GRAPHED_ADAMW_OK", losses_g[-1], o_g.param_groups[0]["lr"])


# ---- Trainer -------------------------------------------------------------------------------------------------------------------

EPOCHS = 2


def _seed_everything(seed=5):
    import random
    torch.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)


def _trainer(out_dir, graph, cut_at=None, **flags):
    """UNet(1, 2, 8) at 32 x 48, 8 training images at batch 2 (4 steps per epoch, shuffled by the loader's own generator),
    AdamW over decay_groups, a cosine rule with 3 warm-up steps over the run's 8 steps."""
    import Model
    import loss as L
    from Trainer import Trainer
    from tools import check_resume as C
    from umi import optim as uo
    L.CLASS_NUMBER = 2
    torch.manual_seed(100)
    m = Model.UNet(1, 2, 8, False, compute_dtype="fp32").to(DEV)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(10, 1, 32, 48, generator=g)
    lab = torch.randint(0, 2, (10, 32, 48), generator=g).float()
    train = DataLoader(C.Items(x[:8], lab[:8]), batch_size=2, shuffle=True, generator=torch.Generator().manual_seed(3))
    loaders = {"train": C.CutLoader(train, cut_at), "val": DataLoader(C.Items(x[8:], lab[8:]), batch_size=2)}
    opt = uo.AdamW(uo.decay_groups(m, 1e-2), lr=1e-3)
    os.makedirs(out_dir, exist_ok=True)
    tr = Trainer(m, "single", torch.cuda.FloatTensor, DEV, str(out_dir), loaders, 2, opt, 25, EPOCHS, "dice_bce_mc", "dice_bce_mc",
                 graph=graph, lr_schedule=dict(kind="cosine", warmup=3), **flags)
    return tr, m, opt


def _finished(out_dir, graph, **flags):
    from tools import check_resume as C
    _seed_everything()
    tr, m, opt = _trainer(out_dir, graph, **flags)
    tr.train()
    assert tr.iter_num == 8 and len(tr.train_loss_list) == EPOCHS and len(tr._graphs) == (1 if graph else 0)
    return tr, m, opt, C.summary(tr, m, opt, out_dir)


@pytest.fixture(scope="module")
def graphed_run(tmp_path_factory):
    """The uncut graph=True run, shared by the cases below and left unchanged."""
    return _finished(tmp_path_factory.mktemp("graphed"), True)


def test_trainer_graphed_run_follows_the_eager_run(tmp_path, graphed_run):
    """The comparison tests/test_gpu_graph_lr.py makes between its eager and graphed Trainer runs (tools/check_graphed_schedule.py
    'trainer_mt')."""
    from umi import optim as uo
    tr_e, m_e, o_e, _ = _finished(tmp_path, False)
    tr_g, m_g, o_g, _ = graphed_run
    assert o_e.device_hyper is not None                     # the eager run's rule lived in the device block as well
    for name in ("train_loss_list", "val_loss_list", "val_score_list"):
        np.testing.assert_allclose(getattr(tr_g, name), getattr(tr_e, name), rtol=2e-4, atol=2e-5)
    assert tr_e.iter_num == tr_g.iter_num == 8
    for ge, gg in zip(o_e.param_groups, o_g.param_groups):
        assert abs(ge["lr"] - gg["lr"]) < 1e-12, (ge["lr"], gg["lr"])
        assert abs(gg["lr"] - uo.schedule_lr(8, 1e-3, "cosine", 8, warmup=3)) < 1e-15
    w = [torch.cat([p.detach().flatten() for p in m.parameters()]).double().cpu().numpy() for m in (m_e, m_g)]
    assert np.linalg.norm(w[0] - w[1]) / np.linalg.norm(w[0]) < 1e-5
    # the per-epoch LR lines: the LR of the step that follows (epoch 1: step 0 of the warm-up, not the base LR)
    lines = [l for l in open(os.path.join(tr_g.output_save_dir, "logs.txt")).read().split("\n") if l.startswith("LR ")]
    assert len(lines) == 4 and float(lines[0][3:]) == uo.schedule_lr(0, 1e-3, "cosine", 8, warmup=3)
    assert abs(float(lines[2][3:]) - uo.schedule_lr(4, 1e-3, "cosine", 8, warmup=3)) < 1e-15


def test_trainer_with_guard_and_ema(tmp_path):
    tr, m, opt, _ = _finished(tmp_path, True, grad_guard=dict(max_norm=1.0), ema=True)
    r = tr._guard.read()
    assert r["steps"] == 8 and r["skipped"] == 0
    assert all(bool(torch.isfinite(v).all()) for v in m.state_dict().values())
    assert tr.ema is not None and tr.ema.sync_host()["updates"] == 8
    assert all(int(h["iter"]) == 8 and h["adam_t"] == 8.0 for h in opt.sync_host())


def test_trainer_cut_and_resumed_run_equals_the_whole_run(tmp_path, graphed_run):
    """Cut after epoch 1, resumed with new objects: weights, moments, block bytes, lists and LRs of the run that was never cut,
    bit for bit (the pattern of the Adam case of tests/test_gpu_snapshot.py)."""
    from tools import check_resume as C
    whole = graphed_run[3]
    out = tmp_path / "cut"
    _seed_everything()
    cut, _, _ = _trainer(out, True, cut_at=2, resume=True)
    with pytest.raises(C.Cut):
        cut.train()
    pl = torch.load(out / "run_state.pt", weights_only=True)
    assert pl["epoch"] == 1 and pl["over"] is False and pl["host"]["iter_num"] == 4 and len(pl["hyper"]) == 2
    _seed_everything(999)                                   # the file's generator states must replace these
    tr, m, opt = _trainer(out, True, resume=True)
    tr.train()
    resumed = C.summary(tr, m, opt, out)
    assert tr.iter_num == 8 and resumed["graphs"] == 1
    assert C.same(whole, resumed) is None, C.same(whole, resumed)
    assert len(resumed["hyper"]) == 2 and torch.load(out / "run_state.pt", weights_only=True)["over"] is True


if __name__ == "__main__":
    {"graph": _child_graph}[sys.argv[1]]()
