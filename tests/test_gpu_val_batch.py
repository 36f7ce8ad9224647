"""Trainer(val_batch=k) and umi.graphs.GraphedEval on the MI355X.

Every case first asserts its premise: eval graphs exist exactly when graph=True, and the number of umi_dice_ce_fwd_items calls
is the number of groups that ran eagerly or were captured.  Then:
  * exactness: validation lists, best epoch and best.pt of a val_batch=3 run (eager and graph-replayed) `==` the val_batch=None
    run from the same seeds, per model family;
  * stale weights: a graph captured before a training phase (or a load_state_dict) replays on the current weights;
  * ragged tail and shape change run eagerly and the sums still agree;
  * data parallel: a world of one, and two ranks sharing the device (fresh processes);
  * poisoned memory: a replay pair on memory preset to 0x00 and to 0xFF gives identical, finite values."""
import os

import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from tests import poison
from tests.test_global_batch import init_rank, run_ranks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPOCHS, K, N_VAL = 3, 3, 7


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: torch.cuda.is_available() is False")


class _Items(torch.utils.data.Dataset):
    def __init__(self, items):
        self.items = items

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


FAMILIES = {
    # name: (model_type, H, W, loss, two label maps)
    "unet": ("single", 32, 48, "dice_bce_mc", False),
    "multitask": ("multi_task", 32, 48, "mse", True),
    "attention": ("attention", 32, 48, "dice_bce_mc", False),
    "transunet": ("TransUnet", 64, 64, "dice_bce_mc", False),
}


def _model(family, mode):
    import Model
    torch.manual_seed(100)
    if family == "unet":
        return Model.UNet(1, 2, 16, False, compute_dtype=mode)
    if family == "multitask":
        return Model.UNet_multitask(1, 1, 16, False, compute_dtype=mode)
    if family == "attention":
        return Model.UNet_attention(1, 2, 16, False, compute_dtype=mode)
    from oracle import ref_transunet
    from tests.test_gpu_transunet import product_config
    from TransUnet.vit_seg_modeling import VisionTransformer
    return VisionTransformer(product_config(ref_transunet.small_config(2), 64), img_size=64, num_classes=2, compute_dtype=mode)


def _data(family, odd_at=None, n_val=N_VAL, val_from=0):
    """6 training images in batches of 2 and n_val validation items of one image (item `odd_at`: 16 rows taller)."""
    _, H, W, _, pair = FAMILIES[family]
    g = torch.Generator().manual_seed(7)
    n = 6 + 16
    x = torch.randn(n, 1, H, W, generator=g)
    l1 = torch.randint(0, 2, (n, H, W), generator=g).float()
    l2 = 0.5 * torch.randint(0, 3, (n, H, W), generator=g).float()
    val = []
    for i in range(val_from, val_from + n_val):
        a, b, c = x[6 + i:7 + i], l1[6 + i:7 + i], l2[6 + i:7 + i]
        if i == odd_at:
            a, b, c = torch.cat([a, a[:, :, :16]], 2), torch.cat([b, b[:, :16]], 1), torch.cat([c, c[:, :16]], 1)
        val.append((a, (b, c) if pair else b))
    if pair:
        from tools.gen_golden import PairLabels
        train = DataLoader(PairLabels(x[:6], l1[:6], l2[:6]), batch_size=2, shuffle=False)
    else:
        train = DataLoader(TensorDataset(x[:6], l1[:6]), batch_size=2, shuffle=False)
    return {"train": train, "val": DataLoader(_Items(val), batch_size=None, shuffle=False)}


def _trainer(out_dir, family, mode, loaders=None, epochs=EPOCHS, **kw):
    import loss as L
    from Trainer import Trainer
    from umi import optim as uo
    L.CLASS_NUMBER = 2
    m = _model(family, mode).to(DEV)
    opt = uo.SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    mt, _, _, loss, _ = FAMILIES[family]
    os.makedirs(out_dir, exist_ok=True)
    tr = Trainer(m, mt, torch.cuda.FloatTensor, DEV, str(out_dir), loaders or _data(family), 2, opt, 25, epochs, loss, loss,
                 lr_scheduler=True, **kw)
    return tr, m


class _Spy:
    """Counts libunetmi calls by name for the duration."""

    def __enter__(self):
        from umi import lib as L
        self.L, self.real, self.n = L, L.call, {}

        def call(name, *a):
            self.n[name] = self.n.get(name, 0) + 1
            return self.real(name, *a)
        L.call = call
        return self

    def __exit__(self, *exc):
        self.L.call = self.real


def _figures(tr, out_dir):
    best = torch.load(os.path.join(out_dir, "models", "best.pt"), weights_only=True)
    return dict(val=tr.val_loss_list, score=tr.val_score_list, v1=tr.val_loss_list_1, v2=tr.val_loss_list_2,
                best_score=tr.best_val_score, best_loss=tr.best_loss, files=sorted(os.listdir(os.path.join(out_dir, "models"))),
                best={k: v.cpu() for k, v in best.items()})


def _assert_same(a, b):
    for k in ("val", "score", "v1", "v2", "best_score", "best_loss", "files"):
        assert a[k] == b[k], (k, a[k], b[k])
    assert len(a["val"]) == EPOCHS and all(v == v and abs(v) < 1e6 for v in a["val"])
    assert a["best"].keys() == b["best"].keys()
    for k in a["best"]:
        assert torch.equal(a["best"][k], b["best"][k]), k


def _four_runs(tmp_path, family, mode, odd_at=None):
    """val_batch=None and val_batch=3, each with graph=False and graph=True, from the same seeds; premises asserted."""
    fused = FAMILIES[family][3] == "dice_bce_mc"
    n_groups = 3                                             # 3 + 3 + 1 per epoch, or 3 + 1 + 3 with the odd 4th item
    out = {}
    for name, kw in (("items_eager", dict(val_batch=None, graph=False)), ("batched_eager", dict(val_batch=K, graph=False)),
                     ("items_graph", dict(val_batch=None, graph=True)), ("batched_graph", dict(val_batch=K, graph=True))):
        with _Spy() as spy:
            tr, m = _trainer(tmp_path / name, family, mode, loaders=_data(family, odd_at=odd_at), **kw)
            tr.train()
        calls = spy.n.get("umi_dice_ce_fwd_items", 0)
        assert len(tr._graphs) == (1 if kw["graph"] else 0)
        if kw["val_batch"] is None:
            assert calls == 0 and tr._validation().graphs == {}
        elif not kw["graph"]:
            assert tr._validation().graphs == {} and calls == (n_groups * EPOCHS if fused else 0)
        else:
            # the shape's 1st full group runs eagerly, its 2nd is captured (one call each, both in epoch 1), every later one is
            # a replay (no call); the ragged / odd-shaped group runs eagerly in every epoch
            assert len(tr._validation().graphs) == 1 and calls == ((2 + EPOCHS) if fused else 0)
        out[name] = _figures(tr, tmp_path / name)
    return out


def _check(runs):
    _assert_same(runs["batched_eager"], runs["items_eager"])
    _assert_same(runs["batched_graph"], runs["items_graph"])


@pytest.mark.parametrize("family,mode", [("unet", "fp16"), ("unet", "fp32"), ("multitask", "fp16"), ("attention", "fp16"),
                                         ("transunet", "fp16")])
def test_batched_validation_equals_the_item_loop(tmp_path, family, mode):
    """Seven validation items, k = 3, three epochs with training in between: every figure `==`."""
    _need_gpu()
    runs = _four_runs(tmp_path, family, mode)
    print(family, mode, {k: v["val"] for k, v in runs.items()})
    _check(runs)


def test_ragged_tail_and_shape_change_run_eagerly(tmp_path):
    """The 4th item is 48x48: groups 3 | 1 | 3.  Both full groups have one shape, so the second is captured and replayed."""
    _need_gpu()
    _check(_four_runs(tmp_path, "unet", "fp16", odd_at=3))


# ---- stale weights -----------------------------------------------------------------------------------------------------------

def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def test_replay_after_training_and_after_load_state_dict_reads_current_weights(tmp_path):
    _need_gpu()
    tr, m = _trainer(tmp_path, "unet", "fp16", graph=True, val_batch=K)
    start = {k: v.clone() for k, v in m.state_dict().items()}
    items = list(tr.dataloader["val"])[:K]
    group = [tr._to_device(x, l, train=False) for x, l in items]
    flat = [torch.cat([g[0] for g in group]), torch.cat([g[1] for g in group])]

    def grouped():                                  # through the Trainer's own path: eager, capture, replay
        if tr._validation().sums is not None:
            tr._validation().sums.zero_()
        tr._validation().run_group(group)
        return tr._validation().sums.clone()

    def eager():                                    # the same function without a graph
        tr._validation().sums.zero_()
        rows = tr._validation().group_fn(K)(*flat)
        return tr._validation().sums.clone(), rows.clone()

    m.eval()
    v1 = grouped()
    assert tr._validation().graphs == {}
    v2 = grouped()
    assert len(tr._validation().graphs) == 1                # captured and replayed
    ge = next(iter(tr._validation().graphs.values()))
    assert torch.equal(_bits(v1), _bits(v2))
    # a training phase: three steps (eager, captured, replayed), as the epoch between two validation phases
    m.train()
    for x, l in tr.dataloader["train"]:
        tr.train_step(x, l)
    assert len(tr._graphs) == 1
    m.eval()
    replays = []
    real = ge.graph.replay
    ge.graph.replay = lambda: (replays.append(1), real())[1]
    v3 = grouped()
    assert replays == [1]
    e3, rows3 = eager()
    assert torch.equal(_bits(v3), _bits(e3)), (v3, e3)
    assert torch.equal(_bits(ge.static_outputs), _bits(rows3))
    assert not torch.equal(_bits(v3[:1]), _bits(v1[:1])), "the replay still sees the weights of the capture"
    # load_state_dict between two replays: back to the starting weights and running statistics
    m.load_state_dict(start)
    v4 = grouped()
    assert replays == [1, 1]
    assert torch.equal(_bits(v4), _bits(v1)) and not torch.equal(_bits(v4[:1]), _bits(v3[:1]))
    e4, _ = eager()
    assert torch.equal(_bits(v4), _bits(e4))


def test_graphed_predictor_follows_an_optimizer_step():
    _need_gpu()
    import loss as L
    from umi import infer, optim as uo
    L.CLASS_NUMBER = 2
    m = _model("unet", "fp16").to(DEV).train()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 1, 32, 48, generator=g).to(DEV)
    lab = torch.randint(0, 2, (2, 32, 48), generator=g).float().to(DEV)
    pred = infer.GraphedPredictor(m, x)
    assert m.training and not pred.binary
    before = pred(x)
    assert before.dtype == torch.uint8 and torch.equal(before, infer.predict_mask(m, x))
    opt = uo.SGD(m.parameters(), lr=0.5, momentum=0.9)
    for _ in range(3):
        opt.zero_grad()
        L.calc_loss(m(x), lab, loss_type="dice_bce_mc").backward()
        opt.step()
    after = pred(x)
    assert m.training
    assert torch.equal(after, infer.predict_mask(m, x))
    assert not torch.equal(after, before), "three steps at lr 0.5 changed no pixel of the mask: the case shows nothing"
    # another shape falls back to predict_mask; a one-logit model thresholds
    y = torch.randn(1, 1, 48, 32, generator=g).to(DEV)
    assert torch.equal(pred(y), infer.predict_mask(m, y))
    import Model
    torch.manual_seed(1)
    b = Model.UNet(1, 1, 16, False, compute_dtype="fp16").to(DEV)
    bp = infer.GraphedPredictor(b, x)
    assert bp.binary and torch.equal(bp(x), infer.predict_binary_mask(b, x)) and torch.equal(bp(y), infer.predict_binary_mask(b, y))


# ---- data parallel -----------------------------------------------------------------------------------------------------------

def test_world_of_one(tmp_path):
    _need_gpu()
    figs = {}
    for name, kw in (("items", dict(val_batch=None)), ("batched", dict(val_batch=K))):
        tr, m = _trainer(tmp_path / name, "unet", "fp16", graph=True, data_parallel=dict(world_size=1), **kw)
        tr.train()
        assert bool(tr._validation().graphs) == (name == "batched") and len(tr._graphs) == 1
        figs[name] = _figures(tr, tmp_path / name)
    _assert_same(figs["batched"], figs["items"])


def _worker(rank, world, port, q, out_dir):
    dist = init_rank(rank, world, port)
    torch.cuda.set_device(0)
    out = {}
    for name, vb in (("items", None), ("batched", K)):
        # unequal validation shards: rank 0 items 0-6 (3 + 3 + 1), rank 1 items 7-10 (3 + 1)
        loaders = _data("unet", n_val=7 if rank == 0 else 4, val_from=0 if rank == 0 else 7)
        tr, m = _trainer(os.path.join(out_dir, name), "unet", "fp16", loaders=loaders, graph=True, val_batch=vb,
                         data_parallel=dict(bucket_mb=0.05))
        tr.train()
        out[name] = dict(val=tr.val_loss_list, score=tr.val_score_list, train=tr.train_loss_list, best=tr.best_val_score,
                         eval_graphs=len(tr._validation().graphs), graphs=len(tr._graphs))
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_one_device(tmp_path):
    """Two fresh processes share the MI355X: both report the same epoch figures, equal to the val_batch=None run."""
    _need_gpu()
    res = run_ranks(_worker, 2, str(tmp_path))
    a, b = res[0], res[1]
    assert a["batched"]["eval_graphs"] == 1 and a["items"]["eval_graphs"] == 0 and a["batched"]["graphs"] == 1
    assert b["batched"]["eval_graphs"] == 1            # rank 1's one full group per epoch: eager in epoch 1, captured in epoch 2
    for k in ("val", "score", "train", "best"):
        assert a["batched"][k] == b["batched"][k] == a["items"][k] == b["items"][k], k
    assert len(a["batched"]["val"]) == EPOCHS


# ---- poisoned memory ---------------------------------------------------------------------------------------------------------

def test_replay_pair_on_poisoned_memory():
    _need_gpu()
    import loss as L
    from umi import graph as G
    from umi.graphs import GraphedEval
    L.CLASS_NUMBER = 2
    g = torch.Generator().manual_seed(11)
    x = torch.randn(3, 1, 38, 50, generator=g).to(DEV)              # odd pools 19x25, 9x12: the decoder pads
    lab = torch.randint(0, 2, (3, 38, 50), generator=g).float().to(DEV)
    got = {}
    for byte in (0x00, 0xFF):
        m = _model("unet", "fp16").to(DEV).eval()

        def fn(xs, ls):
            out = m(xs)
            return out, L.calc_loss_items(out, ls, 3, loss_type="dice_bce_mc")
        with poison.poisoned(byte), torch.no_grad():
            fn(x, lab)
            ge = GraphedEval(fn, [x, lab], pack_cache=G.pack_cache_of(m))
            pair = []
            for _ in range(2):
                out, vals = ge(x, lab)
                pair.append((out.clone(), vals.clone()))
        torch.cuda.synchronize()
        assert torch.equal(_bits(pair[0][0]), _bits(pair[1][0])) and torch.equal(_bits(pair[0][1]), _bits(pair[1][1]))
        got[byte] = pair[0]
    for a, b in zip(got[0x00], got[0xFF]):
        assert torch.isfinite(b).all() and torch.equal(_bits(a), _bits(b))
