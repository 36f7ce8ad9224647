"""The hard-mask metric kernels (csrc/seg_metrics.hip) on the MI355X against their NumPy statement (umi/metrics.py).

Counts are integers and must be `torch.equal` to `confusion_numpy`; scores must be bit-identical to `scores_numpy` (the kernel
does the same float64 operations in the same order, without contraction).  Shapes: every HW at which the counting pass takes
another path (below one vector, a ragged tail, HW % 4 != 0 -> scalar loads, one block, more than one block), every channel count
with its own instantiation, one and several items / images per item, the four label dtypes, a view that is only 4-byte aligned.
Then the Trainer: the three validation paths (item by item, val_batch groups, replayed groups) must give `==` figures, best.pt
and matrices, and two ranks on one device the figures of one process on the whole set."""
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from tests import poison
from tests.test_global_batch import init_rank, run_ranks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HWS = (1, 3, 4, 5, 1023, 1024, 1025, 4 * 256 * 5 + 1)
SPLITS = ((1, 1), (3, 2), (5, 1))                     # items x images per item
DTYPES = (torch.int64, torch.float32, torch.uint8, torch.int32)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: torch.cuda.is_available() is False")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _labels(rng, shape, K, dtype):
    """Labels over -1 .. K (uint8: 0 .. K and 255; float32: also 0.5 and NaN), so that the not-a-class row is always in play."""
    t = rng.integers(-1, K + 1, shape)
    if dtype == torch.uint8:
        return torch.from_numpy(np.where(t < 0, 255, t).astype(np.uint8))
    if dtype == torch.float32:
        f = t.astype(np.float32)
        f[rng.random(shape) < 0.05] = 0.5
        f[rng.random(shape) < 0.02] = np.nan
        return torch.from_numpy(f)
    return torch.from_numpy(t).to(dtype)


def _check(pred, target, items, K=None, what=""):
    """Kernel counts == statement, kernel scores bit-identical to the statement, for all kinds and both c0."""
    from umi import metrics as M
    want = M.confusion_numpy(pred.numpy(), target.numpy(), items, K)
    got = M.confusion(pred.to(DEV), target.to(DEV), items, K)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), torch.from_numpy(want)), (what, got.cpu(), want)
    for kind in (0, 1, 2):
        for c0 in (0, 1):
            s = M.scores(got, kind, c0)
            assert s.is_cuda and s.dtype == torch.float32
            assert np.array_equal(_bits(s.cpu().numpy()), _bits(M.scores_numpy(want, kind, c0))), (what, kind, c0)
    return got


@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 8])
def test_counts_and_scores_at_the_edge_shapes(C):
    _need_gpu()
    rng = np.random.default_rng(100 + C)
    K = 2 if C == 1 else C
    for hi, HW in enumerate(HWS):
        for si, (items, n) in enumerate(SPLITS):
            dtype = DTYPES[(hi + si) % 4]
            x = torch.from_numpy(rng.standard_normal((items * n, C, HW)).astype(np.float32))
            _check(x, _labels(rng, (items * n, HW), K, dtype), items, what=(C, HW, items, n, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_label_dtype_on_both_load_paths(dtype):
    _need_gpu()
    rng = np.random.default_rng(7)
    for shape in ((4, 3, 8, 12), (4, 3, 7, 9)):            # HW = 96: vector loads; HW = 63: scalar loads
        x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
        _check(x, _labels(rng, (shape[0],) + shape[2:], 3, dtype), 2, what=(shape, dtype))


def test_views_that_are_only_4_byte_aligned():
    """Logits (and labels) that start one element into their storage: HW % 4 == 0, so only the alignment sends them to the
    scalar loads."""
    _need_gpu()
    from umi import metrics as M
    rng = np.random.default_rng(8)
    x = rng.standard_normal((3, 4, 16, 16)).astype(np.float32)
    t = rng.integers(-1, 5, (3, 16, 16)).astype(np.int32)
    want = M.confusion_numpy(x, t, 3)
    xb = torch.empty(x.size + 1, dtype=torch.float32, device=DEV)
    tb = torch.empty(t.size + 1, dtype=torch.int32, device=DEV)
    xv, tv = xb[1:].view(x.shape), tb[1:].view(t.shape)
    xv.copy_(torch.from_numpy(x))
    tv.copy_(torch.from_numpy(t))
    assert xv.data_ptr() % 16 == 4 and tv.data_ptr() % 16 == 4 and xv.is_contiguous()
    aligned = torch.from_numpy(x).to(DEV), torch.from_numpy(t).to(DEV)
    for a, b in ((xv, tv), (xv, aligned[1]), (aligned[0], tv), aligned):
        assert torch.equal(M.confusion(a, b, 3).cpu(), torch.from_numpy(want))


def test_all_keys_uniform_and_one_bin():
    _need_gpu()
    K, HW = 8, 9 * 8 * 29                                   # every (row, column) pair 29 times per image
    col = np.arange(HW) % K
    row = (np.arange(HW) // K) % (K + 1)
    x = np.full((2, K, HW), -1.0, np.float32)
    x[:, col, np.arange(HW)] = 1.0
    t = np.broadcast_to(row, (2, HW)).astype(np.int64)
    got = _check(torch.from_numpy(x), torch.from_numpy(t.copy()), 2, what="uniform")
    assert (got[:, :, :K] == 29).all() and (got[:, :, K] == 0).all()
    x = np.zeros((2, 3, 4100), np.float32)
    x[:, 1] = 1.0
    got = _check(torch.from_numpy(x), torch.ones(2, 4100, dtype=torch.uint8), 1, what="one bin")
    assert got[0, 1, 1] == 8200 and got.sum() == 8200


def test_ties_nan_and_the_binary_cutoff():
    _need_gpu()
    from umi import infer, metrics as M
    rng = np.random.default_rng(9)
    x = rng.integers(0, 3, (2, 4, 1028)).astype(np.float32)               # many exact ties: the first maximum wins
    x[0, 0, ::7] = np.nan                                                # a NaN in channel 0 stays
    x[1, 2, ::5] = np.nan                                                # a NaN elsewhere never wins
    t = rng.integers(0, 4, (2, 1028)).astype(np.int64)
    got = _check(torch.from_numpy(x), torch.from_numpy(t), 1, what="ties")
    cls, _ = M.predict_numpy(x)
    assert (cls[0, ::7] == 0).all() and (cls[1, ::5] != 2).all()
    mask = infer.argmax_mask(torch.from_numpy(x).to(DEV).view(2, 4, 4, 257))
    assert np.array_equal(mask.cpu().numpy().reshape(2, -1), cls)       # the rule IS umi_argmax_mask's
    cut = np.float32(M.SIGMOID_HALF_CUTOFF)
    b = np.array([cut, np.nextafter(cut, np.float32(-1)), np.nextafter(cut, np.float32(1)), 0.0, -0.0, np.nan, np.inf, -np.inf,
                  1.5, -1.5], np.float32)
    b = np.tile(b, 103).reshape(1, 1, -1)
    tb = torch.from_numpy((np.arange(b.size) % 3 == 0).astype(np.float32).reshape(1, -1))
    _check(torch.from_numpy(b), tb, 1, what="cutoff")
    bm = infer.binary_mask(torch.from_numpy(b).to(DEV).view(1, 1, 10, 103))
    assert np.array_equal(bm.cpu().numpy().reshape(-1), M.predict_numpy(b)[0].reshape(-1))


def test_a_single_bin_past_2_to_24():
    """2^24 + 4096 pixels of one item in one bin: a float32 counter would stop at 2^24, and the block partials are int32."""
    _need_gpu()
    from umi import metrics as M
    n = (1 << 24) + 4096
    x = torch.zeros((1, 2, n), dtype=torch.float32, device=DEV)
    x[:, 1] = 1.0
    t = torch.ones((1, n), dtype=torch.uint8, device=DEV)
    got = M.confusion(x, t, 1)
    want = np.zeros((1, 3, 3), np.int64)
    want[0, 1, 1] = n
    assert torch.equal(got.cpu(), torch.from_numpy(want))
    for kind in (0, 1, 2):
        assert np.array_equal(_bits(M.scores(got, kind).cpu().numpy()), _bits(M.scores_numpy(want, kind)))


def test_preset_memory_does_not_matter():
    _need_gpu()
    from umi import metrics as M
    rng = np.random.default_rng(10)
    x = torch.from_numpy(rng.standard_normal((6, 3, 40, 41)).astype(np.float32)).to(DEV)
    t = torch.from_numpy(rng.integers(-1, 4, (6, 40, 41))).to(DEV)
    want = torch.from_numpy(M.confusion_numpy(x.cpu().numpy(), t.cpu().numpy(), 3))
    got = {}
    for byte in (0x00, 0xFF):
        with poison.poisoned(byte):
            c = M.confusion(x, t, 3)
            s = M.scores(c, 0)
            m = M.confusion(torch.full((6, 40, 41), 2, dtype=torch.uint8, device=DEV), t, 3, K=3)
        got[byte] = (c.cpu(), s.cpu(), m.cpu())
    assert torch.equal(got[0x00][0], want)
    for a, b in zip(got[0x00], got[0xFF]):
        assert torch.equal(a, b)
    assert torch.isfinite(got[0xFF][1]).all()


def test_masks_entry_equals_logits_entry():
    _need_gpu()
    from umi import infer, metrics as M
    rng = np.random.default_rng(11)
    for C, H, W in ((2, 16, 20), (5, 9, 7), (8, 4, 257)):
        x = torch.from_numpy(rng.integers(-2, 3, (4, C, H, W)).astype(np.float32)).to(DEV)
        t = torch.from_numpy(rng.integers(-1, C + 1, (4, H, W))).to(DEV)
        mask = infer.argmax_mask(x)
        assert torch.equal(M.confusion(mask, t, 2, K=C), M.confusion(x, t, 2))
    # mask values >= K fall in column K
    m = torch.from_numpy(rng.integers(0, 6, (2, 31, 33)).astype(np.uint8))
    t = torch.from_numpy(rng.integers(0, 5, (2, 31, 33)).astype(np.uint8))
    got = _check(m, t, 2, K=3, what="mask")
    assert got[:, :, 3].sum() > 0


def test_calc_loss_items_is_the_loop_with_the_kernel_on_and_off():
    _need_gpu()
    import loss as L
    rng = np.random.default_rng(12)
    mc = (torch.from_numpy(rng.standard_normal((6, 3, 24, 40)).astype(np.float32)).to(DEV),
          torch.from_numpy(rng.integers(0, 3, (6, 24, 40)).astype(np.float32)).to(DEV))
    bn = (torch.from_numpy(rng.standard_normal((6, 1, 24, 40)).astype(np.float32)).to(DEV),
          torch.from_numpy(rng.integers(0, 2, (6, 24, 40)).astype(np.float32)).to(DEV))
    vals = {}
    try:
        for on in (True, False):
            L.METRICS_KERNEL = on
            for name, (_, _, multi) in L.SEG_METRICS.items():
                p, t = mc if multi else bn
                for items in (1, 2, 3, 6):
                    n = 6 // items
                    got = L.calc_loss_items(p, t, items, loss_type=name)
                    loop = torch.stack([L.calc_loss(p[i * n:(i + 1) * n], t[i * n:(i + 1) * n], loss_type=name) for i in range(items)])
                    assert got.shape == (items,) and got.dtype == torch.float32 and not got.requires_grad
                    assert torch.equal(got, loop), (on, name, items)
                    vals[(on, name, items)] = got.cpu()
    finally:
        L.METRICS_KERNEL = True
    for (on, name, items), v in vals.items():
        assert torch.equal(v, vals[(True, name, items)]), (name, items)          # kernel == composite, bit for bit


def test_the_three_calls_are_capturable():
    _need_gpu()
    from umi import metrics as M
    rng = np.random.default_rng(13)
    x = torch.from_numpy(rng.standard_normal((4, 2, 32, 32)).astype(np.float32)).to(DEV)
    t = torch.from_numpy(rng.integers(0, 2, (4, 32, 32))).to(DEV)
    want = M.scores(M.confusion(x, t, 4), 0).clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = M.scores(M.confusion(x, t, 4), 0)
    x.copy_(-x)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, M.scores(M.confusion(x, t, 4), 0)) and not torch.equal(out, want)
    # the composite of device tensors reads nothing back either (a validation group with METRICS_KERNEL off is captured too)
    M.confusion_composite(x, t, 4)
    torch.cuda.synchronize()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        comp = M.scores_composite(M.confusion_composite(x, t, 4), 0)
    g2.replay()
    torch.cuda.synchronize()
    assert torch.equal(comp, out)


# ---- Trainer ------------------------------------------------------------------------------------------------------------------

EPOCHS, N_VAL = 2, 9


class _Items(torch.utils.data.Dataset):
    def __init__(self, items):
        self.items = items

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _model(family, mode):
    import Model
    torch.manual_seed(100)
    if family == "unet":
        return Model.UNet(1, 2, 8, False, compute_dtype=mode)
    from oracle import ref_transunet
    from tests.test_gpu_transunet import product_config
    from TransUnet.vit_seg_modeling import VisionTransformer
    return VisionTransformer(product_config(ref_transunet.small_config(2), 32), img_size=32, num_classes=2, compute_dtype=mode)


def _data(val_from=0, n_val=N_VAL):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(4 + N_VAL, 1, 32, 32, generator=g)
    lab = torch.randint(0, 2, (4 + N_VAL, 32, 32), generator=g).float()
    val = [(x[4 + i:5 + i], lab[4 + i:5 + i]) for i in range(val_from, val_from + n_val)]
    return {"train": DataLoader(TensorDataset(x[:4], lab[:4]), batch_size=2, shuffle=False),
            "val": DataLoader(_Items(val), batch_size=None, shuffle=False)}


def _train(out_dir, family, mode, loaders=None, lr=0.05, **kw):
    import loss as L
    from Trainer import Trainer
    from umi import optim as uo
    L.CLASS_NUMBER = 2
    m = _model(family, mode).to(DEV)
    opt = uo.SGD(m.parameters(), lr=lr, momentum=0.9, weight_decay=1e-4)
    os.makedirs(out_dir, exist_ok=True)
    tr = Trainer(m, "single" if family == "unet" else "TransUnet", torch.cuda.FloatTensor, DEV, str(out_dir), loaders or _data(), 2,
                 opt, 25, EPOCHS, "dice_bce_mc", "dice_err_mc", lr_scheduler=True, val_confusion=True, **kw)
    tr.train()
    return tr


def _figures(tr, out_dir):
    best = torch.load(os.path.join(out_dir, "models", "best.pt"), weights_only=True)
    return dict(val=tr.val_loss_list, score=tr.val_score_list, train=tr.train_loss_list, best_score=tr.best_val_score,
                files=sorted(os.listdir(os.path.join(out_dir, "models"))), best={k: v.cpu() for k, v in best.items()},
                conf=[m.tolist() for m in tr.val_confusion_list], per_class={k: v.tolist() for k, v in tr.val_class_scores.items()})


@pytest.mark.parametrize("family,mode", [("unet", "fp16"), ("unet", "fp32"), ("transunet", "fp16")])
def test_trainer_paths_agree(tmp_path, family, mode):
    """Nine validation items of 32x32, two epochs with a training phase between: item by item, val_batch=4 (4 + 4 + 1) and
    val_batch=4 replayed must give `==` figures, best.pt and matrices."""
    _need_gpu()
    runs = {}
    for name, kw in (("items", dict(val_batch=None, graph=False)), ("batched", dict(val_batch=4, graph=False)),
                     ("replayed", dict(val_batch=4, graph=True))):
        tr = _train(tmp_path / name, family, mode, **kw)
        assert len(tr._validation().graphs) == (1 if name == "replayed" else 0)
        runs[name] = _figures(tr, tmp_path / name)
    a = runs["items"]
    assert len(a["val"]) == len(a["score"]) == len(a["conf"]) == EPOCHS
    assert all(np.sum(m) == N_VAL * 32 * 32 for m in a["conf"]) and all(0.0 <= s <= 1.0 for s in a["score"])
    assert a["val"] != a["score"] and a["best_score"] == min(a["score"])
    for name in ("batched", "replayed"):
        b = runs[name]
        for k in ("val", "score", "train", "best_score", "files", "conf", "per_class"):
            assert a[k] == b[k], (name, k, a[k], b[k])
        for k in a["best"]:
            assert torch.equal(a["best"][k], b["best"][k]), (name, k)


def _worker(rank, world, port, q, out_dir):
    dist = init_rank(rank, world, port)
    torch.cuda.set_device(0)
    # unequal validation shards: rank 0 items 0-4, rank 1 items 5-8
    loaders = _data(val_from=0 if rank == 0 else 5, n_val=5 if rank == 0 else 4)
    tr = _train(os.path.join(out_dir, f"r{rank}"), "unet", "fp16", loaders=loaders, lr=0.0, val_batch=4, graph=True,
                data_parallel=dict(bucket_mb=0.05))
    q.put((rank, dict(score=tr.val_score_list, val=tr.val_loss_list, conf=[m.tolist() for m in tr.val_confusion_list],
                      per_class={k: v.tolist() for k, v in tr.val_class_scores.items()})))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_agree_on_the_whole_set(tmp_path):
    """Two fresh processes share the MI355X under data_parallel=True, the validation set split 5 + 4: both hold the same scores
    and the same dataset-level matrices, and these are the ones of one process on the whole set.  The learning rate is 0 (both
    ranks and the one process see the same training batches, so the BatchNorm statistics move alike and the weights stay), which
    leaves the comparison on the validation arithmetic: matrices `==`; scores within 1e-6, because one process adds nine fp32
    values <= 1 in fp32 (at most 9 roundings of 6e-8) where the ranks add 5 and 4 and then the two sums in float64."""
    _need_gpu()
    res = run_ranks(_worker, 2, str(tmp_path))
    a, b = res[0], res[1]
    assert a == b and len(a["conf"]) == EPOCHS
    assert all(np.sum(m) == N_VAL * 32 * 32 for m in a["conf"])
    one = _train(tmp_path / "one", "unet", "fp16", loaders=_data(), lr=0.0, val_batch=4, graph=True)
    print("two ranks", a["score"], "one process", one.val_score_list)
    assert [m.tolist() for m in one.val_confusion_list] == a["conf"]
    assert a["per_class"] == {k: v.tolist() for k, v in one.val_class_scores.items()}
    np.testing.assert_allclose(a["score"], one.val_score_list, rtol=0, atol=1e-6)
