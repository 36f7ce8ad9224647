"""CPU tests of the count-ratio-weighted multi-task loop (reference Trainer.multi_task_trainRatio, Trainer.py:1174-1366) and of
the torch composite of its step loss (loss.multi_task_ratio_loss off the device domain)."""
import os
import re

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader

from oracle import recipe, ref_unet
from tests.test_oracle_golden import _sig_close, sig

FIXTURE = "trainer_multitask_ratio.npz"


def _loaders():
    from tools.gen_golden import PairLabels, multitask_trainer_data
    xs, l1, l2 = multitask_trainer_data()
    return {"train": DataLoader(PairLabels(xs[:4], l1[:4], l2[:4]), batch_size=2, shuffle=False),
            "val": DataLoader(PairLabels(xs[4:], l1[4:], l2[4:]), batch_size=1)}


def _run(tmp_path, lr, patience, scheduler, epochs):
    from Trainer import Trainer
    m = ref_unet.RefUNetMultitask(1, 1, 8, False)
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=22))
    opt = torch.optim.SGD(m.parameters(), lr=lr, momentum=0.9, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, patience=0) if scheduler else None
    tr = Trainer(m, "multi_task_reg", torch.FloatTensor, "cpu", str(tmp_path), _loaders(), 2, opt, patience, epochs,
                 "multi_task_loss_ratio", "mse", lr_scheduler=sched)
    assert tr.train() is m
    return tr, m, opt


@pytest.mark.parametrize("run", ["none", "plateau", "stop"])
def test_trainer_ratio_loop_reproduces_reference_run(golden_dir, tmp_path, run):
    """Product Trainer.multi_task_trainRatio driving the CPU oracle's UNet_multitask == the reference's own loop (fixture):
    per-epoch total and per-task losses (the latter divided by the step count twice), alpha of every epoch, the gate jump at
    epoch 6, no validation record before it, iter_num, the LR (poly rule, plus ReduceLROnPlateau cuts in 'plateau'),
    best_val_score, checkpoint files, early stop ('stop') and the weights."""
    g = np.load(os.path.join(golden_dir, FIXTURE))
    p = lambda k: g[f"{run}_{k}"]
    tr, m, opt = _run(tmp_path, float(p("lr")), int(p("patience")), bool(p("scheduler")), int(p("epochs")))
    for mine, key in ((tr.train_loss_list, "train_loss"), (tr.val_loss_list, "val_loss"),
                      (tr.train_loss_list_1, "train_loss_1"), (tr.train_loss_list_2, "train_loss_2"),
                      (tr.val_loss_list_1, "val_loss_1"), (tr.val_loss_list_2, "val_loss_2")):
        assert len(mine) == len(p(key)), key
        np.testing.assert_allclose(mine, p(key), rtol=0, atol=5e-6, err_msg=key)
    np.testing.assert_allclose(tr.alpha_list, p("alpha"), rtol=1e-5)
    assert tr.alpha == tr.alpha_list[-1]
    assert len(tr.val_loss_list) == len(tr.train_loss_list) - 5 and tr.val_score_list == []
    assert tr.iter_num == int(p("iter_num"))
    assert abs(opt.param_groups[0]["lr"] - float(p("final_lr"))) < 1e-12
    assert abs(tr.best_val_score - float(p("best_val_score"))) < 5e-6
    assert sorted(os.listdir(tmp_path / "models")) == list(p("files"))
    assert (tr.early_stop_counter > tr.patience) == bool(p("early_stop"))
    assert (tmp_path / "total.png").exists()                  # the reference dies in its plot routine; the product plots
    log = (tmp_path / "logs.txt").read_text()
    assert len(re.findall(r"Alpha on epoch \d+", log)) == len(tr.train_loss_list)
    keys = list(p("keys"))
    last = torch.load(tmp_path / "models" / "last_epoch.pt")
    state = m.state_dict()
    for i, k in enumerate(keys):
        _sig_close(sig(last[k].float()), p("last")[i], rtol=5e-4)
        if bool(p("early_stop")):     # after an early stop both load the best model; else the product's best is the last
            _sig_close(sig(state[k].float()), p("final")[i], rtol=5e-4)


def test_ratio_gate_switches_at_epoch_6(golden_dir):
    """The fixture shows the gate: the train loss jumps at epoch 6 in every run (reference Trainer.py:1245-1248)."""
    g = np.load(os.path.join(golden_dir, FIXTURE))
    for run in g["runs"]:
        t = g[f"{run}_train_loss"]
        assert t[5] > 2.5 * t[4], (run, t)


def _restated(o1, o2, l1, l2, gate):
    """fp64 restatement of Trainer.py:1226-1248."""
    o1, o2, l1, l2 = (t.double() for t in (o1, o2, l1, l2))
    r1, r2 = torch.relu(o1)[:, 0], torch.relu(o2)[:, 0]
    L1, L2 = ((r1 - l1) ** 2).mean(), ((r2 - l2) ** 2).mean()
    g1, g2, p1, p2 = l1.sum((1, 2)), l2.sum((1, 2)), r1.sum((1, 2)), r2.sum((1, 2))
    r = (g1 / (g2 + g1) - p1 / (p2 + p1)).abs().mean()
    return ((L1 + L2) * (1 + 10 * r) if gate else L1 + L2), L1, L2, r


def _case(B, H, W, seed, zero_pred=None, zero_label=None):
    gen = torch.Generator().manual_seed(seed)
    o1, o2 = torch.randn(B, 1, H, W, generator=gen), torch.randn(B, 1, H, W, generator=gen)
    l1, l2 = torch.rand(B, H, W, generator=gen), torch.rand(B, H, W, generator=gen)
    if zero_pred is not None:
        o1[zero_pred] = -o1[zero_pred].abs()
        o2[zero_pred] = -o2[zero_pred].abs()
    if zero_label is not None:
        l1[zero_label] = 0
        l2[zero_label] = 0
    return o1, o2, l1, l2


def _grads(fn, o1, o2, l1, l2, gate, up):
    a, b = o1.clone().requires_grad_(True), o2.clone().requires_grad_(True)
    outs = fn(a, b, l1, l2, gate)
    sum(u * o for u, o in zip(up, outs)).backward()
    return [o.detach() for o in outs], a.grad, b.grad


@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 7, 5), (4, 16, 24)])
def test_composite_matches_fp64_restatement(shape, gate):
    import loss as L
    o1, o2, l1, l2 = _case(*shape, seed=sum(shape))
    o1[0, 0, 0, 0] = 0.0                                      # ReLU gradient 0 at an output of exactly 0
    up = [1.0, 0.3, -0.7, 1.9]
    (lo, a1, a2) = _grads(L.multi_task_ratio_loss, o1, o2, l1, l2, gate, up)
    (ro, b1, b2) = _grads(_restated, o1, o2, l1, l2, gate, up)
    for x, y in zip(lo, ro):
        np.testing.assert_allclose(x.item(), y.item(), rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(a1.numpy(), b1.float().numpy(), rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(a2.numpy(), b2.float().numpy(), rtol=2e-5, atol=1e-7)
    assert a1[0, 0, 0, 0] == 0


@pytest.mark.parametrize("kind", ["pred", "label"])
def test_composite_zero_denominator(kind):
    """An image whose ReLU'd outputs (or labels) sum to 0 makes r NaN: with the gate on the loss is NaN and so is every
    gradient of an output > 0; with the gate off the loss and the gradients stay finite (and r is NaN)."""
    import loss as L
    o1, o2, l1, l2 = _case(3, 6, 5, seed=4, **({"zero_pred": 1} if kind == "pred" else {"zero_label": 1}))
    outs, d1, d2 = _grads(L.multi_task_ratio_loss, o1, o2, l1, l2, True, [1.0, 0, 0, 0])
    rout, r1, r2 = _grads(_restated, o1, o2, l1, l2, True, [1.0, 0, 0, 0])
    assert torch.isnan(outs[0]) and torch.isnan(outs[3]) and torch.isfinite(outs[1]) and torch.isfinite(outs[2])
    assert torch.equal(torch.isnan(d1), torch.isnan(r1)) and torch.equal(torch.isnan(d2), torch.isnan(r2))
    assert torch.equal(torch.isnan(d1), o1 > 0)
    outs, d1, d2 = _grads(L.multi_task_ratio_loss, o1, o2, l1, l2, False, [1.0, 0, 0, 0])
    rout, r1, r2 = _grads(_restated, o1, o2, l1, l2, False, [1.0, 0, 0, 0])
    assert torch.isfinite(outs[0]) and torch.isnan(outs[3])
    assert torch.isfinite(d1).all() and torch.isfinite(d2).all()
    np.testing.assert_allclose(d1.numpy(), r1.float().numpy(), rtol=2e-5, atol=1e-8)
    np.testing.assert_allclose(outs[0].item(), rout[0].item(), rtol=2e-6)


def test_composite_raises_and_broadcasts_where_the_reference_does():
    import loss as L
    o1, o2, l1, l2 = _case(2, 4, 4, seed=1)
    with pytest.raises(RuntimeError), pytest.warns(UserWarning):   # C != 1: squeeze(1) keeps the channel, mse fails
        L.multi_task_ratio_loss(torch.randn(2, 3, 4, 4), o2, l1, l2, True)
    with pytest.warns(UserWarning):                           # mse_loss warns on a broadcasting target, as in the reference
        L.multi_task_ratio_loss(o1, o2, l1[:1], l2, False)
    out = L.multi_task_ratio_loss(o1.double(), o2.double(), l1.double(), l2.double(), True)
    assert out[0].dtype == torch.float64


def test_lr_scheduler_true_is_refused_before_any_step(tmp_path):
    """reference train.py passes lr_scheduler=True; the reference loop then dies with AttributeError ('bool' object has no
    attribute 'step') in the first validation after epoch 5.  The product refuses up front, before any step, and only when the
    run would get there."""
    from Trainer import Trainer
    m = ref_unet.RefUNetMultitask(1, 1, 8, False)
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=22))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    tr = Trainer(m, "multi_task_reg", torch.FloatTensor, "cpu", str(tmp_path / "a"), _loaders(), 2, opt, 25, 6,
                 "multi_task_loss_ratio", "mse", lr_scheduler=True)
    with pytest.raises(NotImplementedError, match="lr_scheduler"):
        tr.train()
    assert tr.iter_num == 0 and all(torch.equal(before[k], v) for k, v in m.state_dict().items())
    tr = Trainer(m, "multi_task_reg", torch.FloatTensor, "cpu", str(tmp_path / "b"), _loaders(), 2, opt, 25, 2,
                 "multi_task_loss_ratio", "mse", lr_scheduler=True)
    tr.train()                                                 # stops at epoch 2: the reference never reaches the crash
    assert tr.iter_num == 4 and tr.val_loss_list == [] and len(tr.alpha_list) == 2
    tr = Trainer(m, "multi_task_reg", torch.FloatTensor, "cpu", str(tmp_path / "c"), _loaders(), 2, opt, 25, 7,
                 "multi_task_loss_ratio", "mse", lr_scheduler=True, start_epoch=7)
    with pytest.raises(NotImplementedError):
        tr.train()
    with pytest.raises(NotImplementedError):                  # the uncertainty-weighted loop stays refused
        Trainer(m, "multi_task_reg", torch.FloatTensor, "cpu", str(tmp_path / "d"), _loaders(), 2, opt, 25, 2,
                "multi_task_loss", "mse").train()
