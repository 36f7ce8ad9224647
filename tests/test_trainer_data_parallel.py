"""Trainer(..., data_parallel=...) without a GPU: a world of one on the reference run, two gloo ranks against one process
(global-batch loss, unequal validation shards, shared output directory), early stop, unequal training lengths, the argument
errors, the multi-task loop.

Every multi-process test goes through run_ranks / init_rank of tests/test_global_batch.py: init_process_group, q.get and join
have timeouts and the workers are terminated afterwards."""
import os
import re

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, Dataset, TensorDataset

from oracle import recipe, ref_unet
from tests.test_global_batch import init_rank, run_ranks
from tests.test_oracle_golden import _sig_close, sig

EPOCHS = 2


# ---- world of one on the case of tests/test_host_logic.py::test_trainer_reproduces_reference_run ---------------------------

def _reference_run(out_dir, data_parallel):
    import loss as L
    from Trainer import Trainer
    torch.manual_seed(0)
    L.CLASS_NUMBER = 2
    m = ref_unet.RefUNet(1, 2, 8, False)
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=21))
    xs, ls = recipe.synthetic_batch(6, 1, 32, 32, 2, seed=21)
    loaders = {"train": DataLoader(TensorDataset(xs[:4], ls[:4]), batch_size=2, shuffle=False),
               "val": DataLoader(TensorDataset(xs[4:], ls[4:]), batch_size=1)}
    opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    tr = Trainer(m, "single", torch.FloatTensor, "cpu", str(out_dir), loaders, 2, opt, 25, 2,
                 "dice_bce_mc", "dice_bce_mc", lr_scheduler=True, data_parallel=data_parallel)
    assert tr.train() is m
    return tr, m, opt


def test_world_of_one_is_the_reference_run_and_equals_no_data_parallel(golden_dir, tmp_path):
    from umi import ddp
    g = np.load(os.path.join(golden_dir, "trainer_single.npz"))
    tr, m, opt = _reference_run(tmp_path / "dp", dict(world_size=1))
    assert not torch.distributed.is_initialized()                      # a world of one needs no process group
    np.testing.assert_allclose(tr.train_loss_list, g["train_loss"], rtol=0, atol=5e-6)
    np.testing.assert_allclose(tr.val_loss_list, g["val_loss"], rtol=0, atol=5e-6)
    np.testing.assert_allclose(tr.val_score_list, g["val_score"], rtol=0, atol=5e-6)
    assert tr.iter_num == int(g["iter_num"])
    assert abs(opt.param_groups[0]["lr"] - float(g["final_lr"])) < 1e-12
    assert sorted(os.listdir(tmp_path / "dp" / "models")) == list(g["files"])
    assert (tmp_path / "dp" / "total.png").exists()
    pick = lambda s: re.findall(r"(Epoch \d+/\d+|LR [0-9.e-]+|saving best model)", s)      # noqa: E731
    assert pick((tmp_path / "dp" / "logs.txt").read_text()) == pick(str(g["log"]))
    for k, v in m.state_dict().items():
        _sig_close(sig(v.float()), g["final." + k], rtol=5e-4)
    # the Trainer built the reducer, so it closed it: nothing is left on the model, the hook or the process
    assert not hasattr(m, "_umi_grad_sink") and tr.grad_sync is None and ddp.active_batch_sync() is None
    plain, pm, _ = _reference_run(tmp_path / "plain", None)
    assert tr.train_loss_list == plain.train_loss_list and tr.val_loss_list == plain.val_loss_list
    assert tr.val_score_list == plain.val_score_list
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), pm.state_dict().values()))


# ---- two ranks ---------------------------------------------------------------------------------------------------------------

class TwoConv(torch.nn.Module):
    """BatchNorm-free, fp32: two ranks on 2 + 2 images are then ONE model on the four, given the global-batch loss."""

    def __init__(self, heads=1):
        super().__init__()
        self.a = torch.nn.Conv2d(1, 4, 3, padding=1)
        self.b = torch.nn.ModuleList(torch.nn.Conv2d(4, 2 if heads == 1 else 1, 3, padding=1) for _ in range(heads))

    def forward(self, x):
        h = torch.relu(self.a(x))
        return self.b[0](h) if len(self.b) == 1 else tuple(b(h) for b in self.b)


class Pairs(Dataset):
    def __init__(self, x, l1, l2):
        self.x, self.l1, self.l2 = x, l1, l2

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], (self.l1[i], self.l2[i])


def _data(multi):
    g = torch.Generator().manual_seed(17)
    x = torch.randn(12, 1, 12, 10, generator=g)
    if multi:
        return x, torch.rand(12, 12, 10, generator=g), torch.rand(12, 12, 10, generator=g)
    return x, torch.randint(0, 2, (12, 12, 10), generator=g).float(), None


def _loaders(case, rank, world):
    """Images 0..7 train in steps of four (a rank takes its half of each step), 8..11 validate one by one: rank 0 takes the
    first, rank 1 the other three.  world = 1: everything, in the same order."""
    multi = case == "multi"
    x, l1, l2 = _data(multi)
    if world == 1:
        tr, va = list(range(8)), [8, 9, 10, 11]
    else:
        tr = [4 * k + 2 * rank + j for k in range(2) for j in range(2)]
        va = [8] if rank == 0 else [9, 10, 11]
        if case == "unequal_train" and rank == 1:
            tr = tr[:2]
    ds = (lambda idx: Pairs(x[idx], l1[idx], l2[idx])) if multi else (lambda idx: TensorDataset(x[idx], l1[idx]))
    return {"train": DataLoader(ds(tr), batch_size=4 // world, shuffle=False), "val": DataLoader(ds(va), batch_size=1)}


def _run(case, rank, world, out_dir, data_parallel):
    import loss as L
    from Trainer import Trainer
    L.CLASS_NUMBER = 2
    multi = case == "multi"
    torch.manual_seed(3)
    m = TwoConv(2 if multi else 1)
    before = [p.detach().clone() for p in m.parameters()]
    early = case == "early_stop"
    opt = torch.optim.SGD(m.parameters(), lr=0.0 if early else 0.05, momentum=0.9)
    loss_name = "mse" if multi else "dice_bce_mc"
    tr = Trainer(m, "multi_task" if multi else "single", torch.FloatTensor, "cpu", str(out_dir), _loaders(case, rank, world),
                 4 // world, opt, 0 if early else 25, 5 if early else EPOCHS, loss_name, loss_name, lr_scheduler=not early,
                 data_parallel=data_parallel)
    out = {}
    try:
        tr.train()
    except ValueError as e:
        out["error"] = str(e)
    out.update(train=tr.train_loss_list, val=tr.val_loss_list, score=tr.val_score_list, iter_num=tr.iter_num,
               tasks=[tr.train_loss_list_1, tr.train_loss_list_2, tr.val_loss_list_1, tr.val_loss_list_2],
               untouched=all(torch.equal(a, b) for a, b in zip(before, m.parameters())),
               state={k: v.numpy().copy() for k, v in m.state_dict().items()}, best=bool(tr.best_model))      # (NumPy: it crosses a queue)
    return out


def _worker(rank, world, port, q, case, out_dir):
    dist = init_rank(rank, world, port)
    from umi import ddp
    out = _run(case, rank, world, out_dir, dict(global_batch=case == "single", bucket_mb=0.0001))
    out["closed"] = ddp.active_batch_sync() is None
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def single(tmp_path_factory):
    """The two-rank run and the one-process run of the same four images per step, once for the tests below."""
    shared, alone = tmp_path_factory.mktemp("two_ranks"), tmp_path_factory.mktemp("one_process")
    res = run_ranks(_worker, 2, "single", str(shared))
    return res, _run("single", 0, 1, alone, None), shared, alone


def test_two_ranks_hold_one_set_of_numbers(single):
    res, _, _, _ = single
    a, b = res[0], res[1]
    assert len(a["train"]) == len(a["val"]) == len(a["score"]) == EPOCHS
    for k in ("train", "val", "score", "iter_num"):
        assert a[k] == b[k], k                                       # bit-identical floats: the same decisions everywhere
    assert all(np.array_equal(a["state"][k], b["state"][k]) for k in a["state"])
    assert a["best"] and b["best"] and a["closed"] and b["closed"]


def test_two_ranks_are_the_one_process_run(single):
    res, one, _, _ = single
    for k in ("train", "val", "score"):
        np.testing.assert_allclose(res[0][k], one[k], rtol=0, atol=5e-6)
    assert res[0]["iter_num"] == one["iter_num"] == 2 * EPOCHS
    assert not one["untouched"]                                      # (the run trained)
    for k, v in one["state"].items():
        _sig_close(sig(torch.from_numpy(res[0]["state"][k])), sig(torch.from_numpy(v)), rtol=5e-4)


def test_unequal_validation_shards_reduce_to_the_mean_over_the_four(single):
    """Rank 0 validates one image, rank 1 three: sum of the four losses over the global step count, not a mean of two means."""
    res, one, _, _ = single
    np.testing.assert_allclose(res[1]["val"], one["val"], rtol=0, atol=5e-6)
    np.testing.assert_allclose(res[1]["score"], one["score"], rtol=0, atol=5e-6)


def test_two_ranks_write_one_set_of_files(single):
    _, _, shared, alone = single
    assert sorted(os.listdir(shared / "models")) == sorted(os.listdir(alone / "models"))
    assert sorted(os.listdir(shared)) == sorted(os.listdir(alone)) == ["logs.txt", "models", "total.png"]
    log = (shared / "logs.txt").read_text()
    for e in range(1, EPOCHS + 1):
        assert log.count(f"Epoch {e}/{EPOCHS}\n") == 1
    assert log.count("Train loss on epoch") == EPOCHS and log.count("Best val loss") == 1


def test_early_stop_ends_both_ranks_at_the_same_epoch(tmp_path):
    res = run_ranks(_worker, 2, "early_stop", str(tmp_path))          # (run_ranks asserts that both workers exited)
    for r in (0, 1):
        assert len(res[r]["train"]) == len(res[r]["val"]) == 2, r    # epoch 2 does not improve: counter 1 > patience 0
    assert res[0]["val"] == res[1]["val"]
    assert (tmp_path / "logs.txt").read_text().count("Early stopping") == 1


def test_unequal_training_lengths_raise_on_both_ranks_before_any_step(tmp_path):
    res = run_ranks(_worker, 2, "unequal_train", str(tmp_path))
    for r in (0, 1):
        assert "same number of training steps" in res[r].get("error", ""), res[r].get("error")
        assert "[2, 1]" in res[r]["error"]
        assert res[r]["iter_num"] == 0 and res[r]["untouched"] and res[r]["train"] == []


def test_multi_task_loop_reduces_the_per_task_lists(tmp_path):
    res = run_ranks(_worker, 2, "multi", str(tmp_path / "two"))
    one = _run("multi", 0, 1, tmp_path / "one", None)
    assert res[0]["tasks"] == res[1]["tasks"] and res[0]["train"] == res[1]["train"] and res[0]["val"] == res[1]["val"]
    assert all(len(t) == EPOCHS for t in res[0]["tasks"])
    for got, want in zip(res[0]["tasks"] + [res[0]["train"], res[0]["val"]], one["tasks"] + [one["train"], one["val"]]):
        np.testing.assert_allclose(got, want, rtol=0, atol=5e-6)
    assert min(min(t) for t in one["tasks"]) > 1e-3                  # (not a comparison of zeros)


# ---- argument errors -------------------------------------------------------------------------------------------------------

def _tiny_trainer(tmp_path, **kw):
    from Trainer import Trainer
    m = TwoConv()
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    return Trainer(m, "single", torch.FloatTensor, "cpu", str(tmp_path), _loaders("single", 0, 1), 4, opt, 1, 1, "dice_bce_mc",
                   "dice_bce_mc", **kw), m


def test_argument_errors(tmp_path):
    from umi import ddp
    assert not torch.distributed.is_initialized()
    tr, m = _tiny_trainer(tmp_path, data_parallel=True)
    with pytest.raises(RuntimeError, match="process group"):
        tr.train()
    tr, m = _tiny_trainer(tmp_path, data_parallel=dict(world_size=1))
    tr.grad_sync = lambda: None
    with pytest.raises(ValueError, match="grad_sync"):
        tr.train()
    assert tr.iter_num == 0 and not hasattr(m, "_umi_grad_sink")
    with pytest.raises(TypeError, match="data_parallel"):
        _tiny_trainer(tmp_path, data_parallel="yes")[0].train()
    # a reducer the caller built stays the caller's: attached after train(), global-batch switch as it was
    tr, m = _tiny_trainer(tmp_path)
    red = ddp.GradReducer(m, 1, global_batch=True)
    try:
        tr = _tiny_trainer(tmp_path, data_parallel=red)[0]
        tr.model = m
        tr.optimizer = torch.optim.SGD(m.parameters(), lr=0.1)
        tr.train()
        assert m._umi_grad_sink is red and ddp.active_batch_sync() is red.batch_sync and tr.grad_sync is None
    finally:
        red.close()
    assert ddp.active_batch_sync() is None


def test_ratio_loop_refuses_data_parallel(tmp_path):
    from Trainer import Trainer
    m = TwoConv(2)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    tr = Trainer(m, "multi_task", torch.FloatTensor, "cpu", str(tmp_path), _loaders("multi", 0, 1), 4, opt, 1, 1,
                 "multi_task_loss_ratio", "mse", data_parallel=dict(world_size=1))
    with pytest.raises(NotImplementedError, match="multi_task_trainRatio"):
        tr.train()
    assert tr.iter_num == 0
