"""Child-process body of tests/test_gpu_grad_guard.py: the guarded optimizer step through the tape, a captured graph and the Trainer.

  exact          : fp32 U-Net, two guarded SGD steps with the dynamic factor fixed at 2^-3, 1 and 2^5: bit-identical parameters
                   (and gradients that carry exactly that factor).
  recover_<kind> : fp16 U-Net, dynamic scale from 2^30 (sgd | adam): skipped steps leave the parameters alone, the scale halves until
                   a step applies (within 40 steps), the loss then falls; eager and GraphedStep replay agree; Adam's step count
                   == applied steps, the poly block's iteration == all steps.
  trainer        : Trainer(grad_guard=dict(max_norm=1e-3)), eager, graph=True and eager Adam: the guard line in logs.txt per epoch;
                   none without a guard.
"""
import copy, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import numpy as np
import torch
import Model
import loss as L
from oracle import recipe
from umi import optim as uo
from umi.graphs import GraphedStep

DEV = "cuda"
what = sys.argv[1]


def step_fn(model, opt):
    def step(xx, yy):
        loss = L.calc_loss(model(xx), yy, loss_type="dice_bce_mc")
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss.detach()
    return step


def bits(model):
    return torch.cat([p.detach().flatten() for p in model.parameters()]).view(torch.int32).clone()


if what == "exact":
    L.CLASS_NUMBER = 2
    torch.manual_seed(21)
    base = Model.UNet(1, 2, 8, compute_dtype="fp32").to(DEV).train()
    x = torch.randn(2, 1, 32, 32, device=DEV)
    lab = torch.randint(0, 2, (2, 32, 32), device=DEV).float()
    runs = {}
    for d in (2.0 ** -3, 1.0, 2.0 ** 5):
        m = copy.deepcopy(base)
        opt = uo.SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
        guard = uo.GradGuard(init_scale=d, growth_interval=0)
        opt.grad_guard(guard)
        guard.attach(m)
        step = step_fn(m, opt)
        for _ in range(2):
            step(x, lab)
        r = guard.read()
        assert (r["scale"], r["steps"], r["skipped"], r["clipped"]) == (d, 2, 0, 0), r
        runs[d] = (bits(m), [p.grad.detach().clone() for p in m.parameters()], r["norm"])
    assert not torch.equal(runs[1.0][0], bits(base)), "the steps changed nothing"
    for d in (2.0 ** -3, 2.0 ** 5):
        for i, (g, g1) in enumerate(zip(runs[d][1], runs[1.0][1])):
            assert torch.equal(g, g1 * d), ("gradient does not carry the factor exactly", d, i)
        diff = int((runs[d][0] != runs[1.0][0]).sum())
        assert diff == 0, ("parameters differ between dynamic factors", d, diff)
        assert runs[d][2] == runs[1.0][2], (runs[d][2], runs[1.0][2])
    print("GUARD_EXACT_OK", runs[1.0][2])

elif what.startswith("recover_"):
    kind = what[len("recover_"):]
    L.CLASS_NUMBER = 2
    torch.manual_seed(0)
    base = Model.UNet(1, 2, 8, compute_dtype="fp16").to(DEV).train()
    x = torch.randn(2, 1, 64, 64, device=DEV)
    lab = torch.randint(0, 2, (2, 64, 64), device=DEV).float()
    LR = {"sgd": 0.01, "adam": 1e-3}[kind]
    poly = dict(base_lr=LR, max_iterations=400, power=0.9, iter_num=0)
    LIMIT, AFTER, WARM = 40, 10, 2
    out = {}
    for mode in ("eager", "graph"):
        m = copy.deepcopy(base)
        opt = uo.SGD(m.parameters(), lr=LR, momentum=0.9) if kind == "sgd" else uo.Adam(m.parameters(), lr=LR)
        guard = uo.GradGuard(dynamic_scale=True, init_scale=2.0 ** 30, growth_interval=100000)
        opt.grad_guard(guard)
        guard.attach(m)
        start = bits(m)
        if mode == "graph":
            run = GraphedStep(step_fn(m, opt), [x, lab], warmup=WARM, optimizers=[opt], poly=poly)
            r = guard.read()
            assert (r["steps"], r["skipped"]) == (WARM, WARM), r          # the warm-up steps ran eagerly and overflowed
            assert torch.equal(bits(m), start)
            done = WARM
        else:
            opt.device_schedule(poly=poly)
            run, done = step_fn(m, opt), 0
        first, losses, reads = None, [], []
        while first is None or done < first + 1 + AFTER:
            assert done < LIMIT + AFTER + 1
            loss = float(run(x, lab))
            done += 1
            r = guard.read()
            reads.append(r)
            assert r["steps"] == done
            if first is None:
                if r["skipped"] == done:                                   # still overflowing: nothing may have moved
                    assert r["nonfinite"] > 0 and torch.equal(bits(m), start), done
                    assert done < LIMIT, "no step applied within %d steps" % LIMIT
                    continue
                first = done - 1                                           # index of the first applied step
                assert r["steps"] == r["skipped"] + 1 and r["scale"] == 2.0 ** 30 * 0.5 ** r["skipped"], r
                assert r["nonfinite"] == 0 and np.isfinite(r["norm"]) and not torch.equal(bits(m), start)
            else:
                losses.append(loss)
        assert len(losses) == AFTER and all(np.isfinite(losses)), losses
        assert losses[-1] < losses[0], losses
        h = opt.sync_host()[0]
        assert int(h["iter"]) == done, (h["iter"], done)
        if kind == "adam":
            assert int(h["adam_t"]) == r["steps"] - r["skipped"], (h["adam_t"], r)
        out[mode] = dict(first=first, losses=losses, reads=reads[WARM if mode == "eager" else 0:], done=done,
                         w=[p.detach().clone() for p in m.parameters()])
        print(kind, mode, "first applied step", first, "scale", r["scale"], "skipped", r["skipped"], "losses", losses[0], losses[-1])
    e, g = out["eager"], out["graph"]
    assert e["first"] == g["first"] and e["done"] == g["done"]
    for re_, rg in zip(e["reads"], g["reads"]):                           # counters and scale: exactly
        assert all(re_[k] == rg[k] for k in ("steps", "skipped", "clipped", "scale", "nonfinite")), (re_, rg)
    np.testing.assert_allclose(g["losses"], e["losses"], rtol=2e-5, atol=1e-6)
    for pg, pe in zip(g["w"], e["w"]):
        torch.testing.assert_close(pg, pe, rtol=2e-4, atol=2e-6)
    print("GUARD_RECOVER_OK")

elif what == "trainer":
    import re, tempfile
    from torch.utils.data import DataLoader, TensorDataset
    from Trainer import Trainer
    for spec, graph, adam in ((dict(max_norm=1e-3), False, False), (dict(max_norm=1e-3), True, False), (None, False, False),
                              (dict(max_norm=1e-3), False, True)):
        L.CLASS_NUMBER = 2
        torch.manual_seed(0)
        m = Model.UNet(1, 2, 8, False, compute_dtype="fp32")
        m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=21))
        m.to(DEV)
        xs, ls = recipe.synthetic_batch(8, 1, 32, 32, 2, seed=21)
        loaders = {"train": DataLoader(TensorDataset(xs[:6], ls[:6]), batch_size=2, shuffle=False),
                   "val": DataLoader(TensorDataset(xs[6:], ls[6:]), batch_size=1)}
        opt = uo.Adam(m.parameters(), lr=1e-3) if adam else uo.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        with tempfile.TemporaryDirectory() as td:
            tr = Trainer(m, "single", torch.cuda.FloatTensor, DEV, td, loaders, 2, opt, 25, 2, "dice_bce_mc", "dice_bce_mc",
                         lr_scheduler=True, graph=graph, grad_guard=spec)
            tr.train()
            log = open(os.path.join(td, "logs.txt")).read()
        lines = [l for l in log.split("\n") if "Guard" in l or "guard" in l]
        if spec is None:
            assert lines == [], lines
            continue
        if graph:
            assert len(tr._graphs) == 1, "the graph path was not taken"
        got = [re.fullmatch(r"Guard on epoch (\d+): skipped (\d+), clipped (\d+), loss scale (\S+)", l) for l in lines]
        assert len(got) == 2 and all(got), lines
        assert [tuple(int(v) for v in g_.groups()[:3]) for g_ in got] == [(1, 0, 3), (2, 0, 3)], lines
        assert all(float(g_.group(4)) == 1.0 for g_ in got), lines
        assert tr.iter_num == 6 and np.all(np.isfinite(tr.train_loss_list))
        if adam:                                   # eager Adam under a guard runs on the device schedule: t and the poly rule
            h = opt.sync_host()[0]
            assert (int(h["adam_t"]), int(h["iter"])) == (6, 6), h
            assert abs(opt.param_groups[0]["lr"] - 1e-3 * (1.0 - 5 / 6) ** 0.9) < 1e-15, opt.param_groups[0]["lr"]
        print("trainer graph=%s adam=%s ok" % (graph, adam), lines)
    print("GUARD_TRAINER_OK")
