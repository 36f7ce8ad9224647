"""Trainer(..., data_parallel=...) on the MI355X: a world of one is the plain Trainer bit for bit (fp32 / fp16, eager / graph), and
two ranks on ONE device (gloo on device tensors, as tests/test_gpu_ddp.py) train through the Trainer -- global-batch statistics
against the one-process Trainer on the four images, the graph-replayed step with its deferred all-reduce against the eager
one, and the replica check catching one changed ulp.

The two ranks run every scenario in one pair of processes (started once per module, with timeouts everywhere)."""
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from tests.test_global_batch import init_rank, run_ranks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPOCHS = 2


def _images(n, S=32):
    """Data generator seed 7 (the seeds of tests/test_gpu_ddp.py): n training images, then 4 validation images."""
    g = torch.Generator().manual_seed(7)
    x = torch.randn(n + 4, 1, S, S, generator=g)
    lab = torch.randint(0, 2, (n + 4, S, S), generator=g).float()
    return x, lab


def _trainer(out_dir, train_idx, val_idx, batch, n_train, mode="fp32", **kw):
    import Model
    import loss as L
    from Trainer import Trainer
    from umi import optim as uo
    L.CLASS_NUMBER = 2
    torch.manual_seed(100)                                            # model seed 100: the same replica wherever this runs
    m = Model.UNet(1, 2, 8, False, compute_dtype=mode).to(DEV)
    x, lab = _images(n_train)
    loaders = {"train": DataLoader(TensorDataset(x[train_idx], lab[train_idx]), batch_size=batch, shuffle=False),
               "val": DataLoader(TensorDataset(x[val_idx], lab[val_idx]), batch_size=2)}
    opt = uo.SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    tr = Trainer(m, "single", torch.cuda.FloatTensor, DEV, str(out_dir), loaders, batch, opt, 25, EPOCHS, "dice_bce_mc",
                 "dice_bce_mc", lr_scheduler=True, **kw)
    return tr, m


def _state(m):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}


# ---- world of one ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_world_of_one_is_the_plain_trainer_bit_for_bit(tmp_path, mode, graph):
    """UNet(1,2,8), 32 x 32, B = 2, 3 steps x 2 epochs, from the same seeds: loss lists, parameters and buffers."""
    from umi import ddp
    runs = []
    for name, dp in (("plain", None), ("dp", dict(world_size=1))):
        tr, m = _trainer(tmp_path / name, list(range(6)), [6, 7], 2, 6, mode, graph=graph, data_parallel=dp)
        tr.train()
        assert tr.iter_num == 3 * EPOCHS and bool(tr._graphs) == graph
        runs.append((tr.train_loss_list, tr.val_loss_list, tr.val_score_list, _state(m)))
        assert not hasattr(m, "_umi_grad_sink") and ddp.active_batch_sync() is None
    a, b = runs
    assert a[:3] == b[:3], (a[:3], b[:3])
    assert all(np.isfinite(v) for v in a[0] + a[1])
    for k in a[3]:
        np.testing.assert_array_equal(a[3][k], b[3][k], err_msg=k)


def test_a_second_train_call_replays_the_same_graphs_into_the_same_buckets(tmp_path):
    """train() closes the reducer it built and a later train() reopens THAT reducer: the captured step keeps writing its
    gradients where the optimizer reads them.  Two calls each, against the plain Trainer, bit for bit."""
    runs = []
    for name, dp in (("plain", None), ("dp", dict(world_size=1))):
        tr, m = _trainer(tmp_path / name, list(range(6)), [6, 7], 2, 6, graph=True, data_parallel=dp)
        tr.lr_scheduler = None                                        # (the poly rule ends with the first call's last step)
        built = lambda: None if tr._dp is None else tr._dp.built      # noqa: E731  (the plain Trainer has no data-parallel run)
        tr.train()
        first = built()
        tr.train()
        assert built() is first and len(tr._graphs) == 1 and tr.iter_num == 6 * EPOCHS
        runs.append((tr.train_loss_list, _state(m)))
    assert runs[0][0] == runs[1][0] and len(runs[0][0]) == 2 * EPOCHS
    for k in runs[0][1]:
        np.testing.assert_array_equal(runs[0][1][k], runs[1][1][k], err_msg=k)


# ---- two ranks on one device -----------------------------------------------------------------------------------------------

def _worker(rank, world, port, q, out_dir):
    dist = init_rank(rank, world, port)
    torch.cuda.set_device(0)
    from umi import ddp
    out = {}
    # (1) global_batch=True: 2 + 2 images, one step per epoch
    tr, m = _trainer(os.path.join(out_dir, "global"), [2 * rank, 2 * rank + 1], [4 + 2 * rank, 5 + 2 * rank], 2, 4,
                     data_parallel=dict(global_batch=True, bucket_mb=0.05))
    tr.train()
    out["global"] = dict(train=tr.train_loss_list, val=tr.val_loss_list, score=tr.val_score_list, state=_state(m),
                         word=ddp.fingerprint(list(m.parameters())), closed=ddp.active_batch_sync() is None)
    # (2) graph=True without global_batch against the eager data-parallel Trainer: 3 steps per epoch, so steps are replayed
    idx = [4 * k + 2 * rank + j for k in range(3) for j in range(2)]
    #     ... and the same pair under a GradGuard that clips every step and carries a loss scale
    guard = dict(max_norm=1e-3, init_scale=4.0)
    for name, graph, gg in (("graph", True, None), ("eager", False, None), ("graph_guard", True, guard), ("eager_guard", False, guard)):
        tr, m = _trainer(os.path.join(out_dir, name), idx, [12 + 2 * rank, 13 + 2 * rank], 2, 12, graph=graph, grad_guard=gg,
                         data_parallel=dict(bucket_mb=0.05))
        tr.train()
        out[name] = dict(train=tr.train_loss_list, val=tr.val_loss_list, state=_state(m), replayed=bool(tr._graphs),
                         iter_num=tr.iter_num, guard=tr._guard.read() if gg else None)
    # (3) one parameter word of rank 1 moves by one ulp: check_replicas raises on BOTH ranks
    out["agree"] = ddp.check_replicas(m)
    if rank == 1:
        with torch.no_grad():
            p = list(m.parameters())[3]
            p.view(-1)[-1:].view(torch.int32).add_(1)
    try:
        ddp.check_replicas(m)
        out["differ"] = "no error"
    except RuntimeError as e:
        out["differ"] = str(e)
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    out_dir = tmp_path_factory.mktemp("two_ranks")
    return run_ranks(_worker, 2, str(out_dir)), out_dir


def test_two_ranks_global_batch_is_the_one_process_trainer_on_the_four_images(two_ranks, tmp_path):
    """Epoch-1 train and validation loss within 1e-4 of the one-process HIP Trainer (B = 4; the validation images in the same
    two batches of two); lists, parameters, buffers and fingerprints identical across the ranks; one set of files."""
    res, out_dir = two_ranks
    a, b = res[0]["global"], res[1]["global"]
    tr, m = _trainer(tmp_path, [0, 1, 2, 3], [4, 5, 6, 7], 4, 4)
    tr.train()
    print("two ranks", a["train"], a["val"], "one process", tr.train_loss_list, tr.val_loss_list)
    assert abs(a["train"][0] - tr.train_loss_list[0]) < 1e-4
    assert abs(a["val"][0] - tr.val_loss_list[0]) < 1e-4
    assert a["train"] == b["train"] and a["val"] == b["val"] and a["score"] == b["score"] and len(a["train"]) == EPOCHS
    for k in a["state"]:
        np.testing.assert_array_equal(a["state"][k], b["state"][k], err_msg=k)   # global_batch: the buffers agree as well
    assert a["word"] == b["word"] and a["closed"] and b["closed"]
    shared = os.path.join(out_dir, "global")
    assert sorted(os.listdir(shared)) == ["logs.txt", "models", "total.png"]
    assert sorted(os.listdir(os.path.join(shared, "models"))) == sorted(os.listdir(tmp_path / "models"))
    log = open(os.path.join(shared, "logs.txt")).read()
    assert all(log.count(f"Epoch {e}/{EPOCHS}\n") == 1 for e in range(1, EPOCHS + 1))


@pytest.mark.parametrize("suffix", ["", "_guard"], ids=["plain", "grad_guard"])
def test_two_ranks_graph_replay_follows_the_eager_data_parallel_trainer(two_ranks, suffix):
    res, _ = two_ranks
    g0, g1, e0 = res[0]["graph" + suffix], res[1]["graph" + suffix], res[0]["eager" + suffix]
    if suffix:                                                       # every step was clipped, none skipped, on either path
        assert g0["guard"] == g1["guard"] and g0["guard"]["clipped"] == e0["guard"]["clipped"] == 3 * EPOCHS
        assert g0["guard"]["skipped"] == 0 and g0["guard"]["scale"] == 4.0
    assert g0["replayed"] and g1["replayed"] and not e0["replayed"]
    assert g0["iter_num"] == e0["iter_num"] == 3 * EPOCHS
    assert g0["train"] == g1["train"] and g0["val"] == g1["val"]
    params = [k for k in g0["state"] if "running_" not in k and "num_batches" not in k]
    for k in params:
        np.testing.assert_array_equal(g0["state"][k], g1["state"][k], err_msg=k)          # replicas identical
        np.testing.assert_allclose(g0["state"][k], e0["state"][k], rtol=1e-6, atol=1e-7, err_msg=k)


def test_check_replicas_raises_on_both_ranks_after_one_ulp(two_ranks):
    res, _ = two_ranks
    assert res[0]["agree"] == res[1]["agree"]
    for r in (0, 1):
        assert "replicas differ" in res[r]["differ"], res[r]["differ"]
        assert "0: 0x" in res[r]["differ"] and "1: 0x" in res[r]["differ"]
