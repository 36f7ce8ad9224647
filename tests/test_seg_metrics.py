"""Hard-mask segmentation metrics without a GPU: the NumPy statement (umi/metrics.py) against a brute-force loop and against
the reference's own DiceLoss on the one-hot argmax mask (tests/golden/seg_metrics.npz), the torch composite against the
statement (integers equal, scores bit-identical), the rule's edges, the six names of `calc_loss`, the Trainer, and the C ABI's
refusals.

The golden bar is |delta| <= 1e-6, derived: every per-class count of a case is below 2^24 (the generator asserts it), so the
reference's float32 sums of 0/1 products are exact integers; what is left of its float32 arithmetic is fewer than ten roundings
of values <= 2 at 6e-8 each.  tools/gen_golden_seg_metrics.py checks the same bar when it writes the file."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from oracle import recipe, ref_unet
from tests.test_global_batch import init_rank, run_ranks

NAMES = ("dice_err_mc", "iou_err_mc", "pixel_err_mc", "dice_err", "iou_err", "pixel_err")


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32)).view(np.uint32)


# ---- the statement ------------------------------------------------------------------------------------------------------------

def _brute(pred, target, items, K=None):
    """Pixel by pixel, in Python."""
    pred, target = np.asarray(pred), np.asarray(target)
    mask = pred.dtype == np.uint8
    N = pred.shape[0]
    if not mask:
        C = pred.shape[1]
        K = 2 if C == 1 else C
        pred = pred.reshape(N, C, -1)
    else:
        pred = pred.reshape(N, -1)
    target = target.reshape(N, -1)
    out = np.zeros((items, K + 1, K + 1), np.int64)
    cut = np.float32(-1.7881390590446244e-07)
    for i in range(N):
        for p in range(target.shape[1]):
            if mask:
                col = min(int(pred[i, p]), K)
            elif pred.shape[1] == 1:
                col = 1 if pred[i, 0, p] >= cut else 0
            else:
                col, best = 0, pred[i, 0, p]
                for c in range(1, pred.shape[1]):
                    if pred[i, c, p] > best:
                        col, best = c, pred[i, c, p]
            t = target[i, p]
            row = K
            for c in range(K):
                if t == c:
                    row = c
            out[i // (N // items), row, col] += 1
    return out


def _brute_scores(m, kind, c0):
    K = len(m) - 1
    I = [float(m[c][c]) for c in range(K)]
    Z = [float(sum(int(m[r][c]) for r in range(K + 1))) for c in range(K)]
    Y = [float(sum(int(m[c][j]) for j in range(K + 1))) for c in range(K)]
    if kind == 2:
        return np.float32(1.0 - (float(sum(int(m[c][c]) for c in range(K))) + 1e-5)
                          / (float(sum(int(m[c][j]) for c in range(K) for j in range(K + 1))) + 1e-5))
    s = 0.0
    for c in range(c0, K):
        s += (2.0 * I[c] + 1e-5) / (Z[c] + Y[c] + 1e-5) if kind == 0 else (I[c] + 1e-5) / (Z[c] + Y[c] - I[c] + 1e-5)
    return np.float32(1.0 - s / float(K - c0))


def _cases():
    rng = np.random.default_rng(5)
    out = []
    for C, shape, items in ((2, (4, 5, 7), 2), (3, (3, 6, 5), 3), (5, (2, 3, 9), 1), (8, (2, 4, 4), 2), (1, (4, 5, 6), 2)):
        K = 2 if C == 1 else C
        x = rng.integers(-2, 3, (shape[0], C) + shape[1:]).astype(np.float32) * np.float32(0.5)      # ties on purpose
        for dt in (np.int64, np.float32, np.uint8, np.int32):
            t = rng.integers(-1, K + 1, shape)
            t = np.where(t < 0, 255, t).astype(dt) if dt == np.uint8 else t.astype(dt)
            if dt == np.float32:
                t[rng.random(shape) < 0.1] = 0.5
            out.append((x, t, items, None))
    m = rng.integers(0, 7, (4, 6, 5)).astype(np.uint8)
    out.append((m, rng.integers(0, 5, (4, 6, 5)).astype(np.int64), 2, 4))
    return out


def test_statement_against_a_brute_force_loop():
    from umi import metrics as M
    for x, t, items, K in _cases():
        got = M.confusion_numpy(x, t, items, K)
        assert got.dtype == np.int64 and np.array_equal(got, _brute(x, t, items, K)), (x.shape, t.dtype)
        assert got.sum() == t.size
        for kind in (0, 1, 2):
            for c0 in (0, 1):
                s = M.scores_numpy(got, kind, c0)
                want = np.array([_brute_scores(m.tolist(), kind, c0) for m in got], np.float32)
                assert s.dtype == np.float32 and np.array_equal(_bits(s), _bits(want)), (kind, c0)
    assert M.scores_numpy(got[0], "dice").shape == () and M.scores_numpy(got[0], "iou") == M.scores_numpy(got, 1)[0]
    with pytest.raises(ValueError):
        M.scores_numpy(got, 3)
    with pytest.raises(ValueError):
        M.scores_numpy(got, 0, c0=got.shape[-1] - 1)


def test_composite_equals_the_statement():
    from umi import metrics as M
    for x, t, items, K in _cases():
        want = M.confusion_numpy(x, t, items, K)
        got = M.confusion_composite(torch.from_numpy(x), torch.from_numpy(t), items, K)
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
        for kind in (0, 1, 2):
            for c0 in (0, 1):
                a, b = M.scores_composite(got, kind, c0), M.scores(got, kind, c0)          # CPU counts: scores() is the composite
                assert a.dtype == torch.float32 and np.array_equal(_bits(a.numpy()), _bits(M.scores_numpy(want, kind, c0)))
                assert torch.equal(a, b)
    with pytest.raises(ValueError, match="contiguous fp32 device logits"):
        M.confusion(torch.from_numpy(x), torch.from_numpy(t), items, K)                    # the kernel entry takes no CPU tensor


def test_golden_against_the_reference(golden_dir):
    from umi import metrics as M
    g = np.load(os.path.join(golden_dir, "seg_metrics.npz"))
    assert len(g["cases"]) >= 8
    for name in g["cases"]:
        x, t, ref = g[f"{name}_pred"], g[f"{name}_target"], float(g[f"{name}_dice"])
        counts = M.confusion_numpy(x, t)
        assert counts.max() < (1 << 24)
        mine = float(M.scores_numpy(counts, 0)[0])
        comp = float(M.scores_composite(M.confusion_composite(torch.from_numpy(x), torch.from_numpy(t)), 0)[0])
        print(f"{name}: reference {ref:.8f} statement {mine:.8f} delta {mine - ref:+.2e}")
        assert abs(mine - ref) <= 1e-6 and comp == mine, name


def test_not_a_class_row():
    from umi import metrics as M
    x = np.zeros((1, 3, 1, 6), np.float32)
    x[0, 1] = 1.0                                              # every pixel predicted 1
    for t, rows in ((np.array([-1, 3, 0, 1, 2, 1], np.int64), [3, 3, 0, 1, 2, 1]),
                    (np.array([255, 3, 0, 1, 2, 1], np.uint8), [3, 3, 0, 1, 2, 1]),
                    (np.array([0.5, 1.0, 2.0, -0.0, np.nan, 3.0], np.float32), [3, 1, 2, 0, 3, 3]),
                    (np.array([-7, 1 << 20, 2, 2, 2, 0], np.int32), [3, 3, 2, 2, 2, 0])):
        want = np.zeros((1, 4, 4), np.int64)
        for r in rows:
            want[0, r, 1] += 1
        t = t.reshape(1, 1, 6)
        assert np.array_equal(M.rows_numpy(t, 3).ravel(), rows)
        assert np.array_equal(M.confusion_numpy(x, t), want)
        assert np.array_equal(M.confusion_composite(torch.from_numpy(x), torch.from_numpy(t)).numpy(), want)
    # their predictions still count: Z_1 = 6 although only the labelled pixels enter Y
    s = M.scores_numpy(want, 0)
    I, Z, Y = want[0, 1, 1], want[0, :, 1].sum(), want[0, 1].sum()
    assert Z == 6 and Y < 6 and s.shape == (1,) and I == 0
    # a uint8 mask: values >= K fall in column K
    m = np.array([[0, 1, 2, 3, 200]], np.uint8)
    c = M.confusion_numpy(m, np.array([[0, 1, 2, 0, 1]], np.int64), K=3)
    assert c[0, 0, 3] == 1 and c[0, 1, 3] == 1 and c[0].trace() == 3 and c.sum() == 5


def test_ties_and_nan_rule():
    from umi import metrics as M
    nan = np.nan
    #                 tie 0/1   tie 1/2   all equal  NaN in 0   NaN in 1   NaN in 2    all NaN    -inf tie
    cols = np.array([[1.0, 1.0, 0.0], [0.0, 2.0, 2.0], [3.0, 3.0, 3.0], [nan, 9.0, 9.0], [1.0, nan, 0.5], [0.0, 1.0, nan],
                     [nan, nan, nan], [-np.inf, -np.inf, -np.inf]], np.float32)
    x = cols.T.reshape(1, 3, 1, -1).copy()
    want = [0, 1, 0, 0, 0, 1, 0, 0]
    assert M.predict_numpy(x)[0].ravel().tolist() == want
    assert M.predict_composite(torch.from_numpy(x))[0].ravel().tolist() == want
    finite = ~np.isnan(x).any(axis=1)
    assert np.array_equal(M.predict_numpy(x)[0][finite], torch.argmax(torch.from_numpy(x), dim=1).numpy()[finite])
    # one logit: the cutoff of umi_binary_mask, i.e. torch's fp32 sigmoid >= 0.5; NaN gives 0
    cut = np.float32(M.SIGMOID_HALF_CUTOFF)
    b = np.array([cut, np.nextafter(cut, np.float32(-1)), 0.0, -0.0, nan, np.inf, -np.inf, 1e-3, -1e-3], np.float32)
    want = [1, 0, 1, 1, 0, 1, 0, 1, 0]
    assert M.predict_numpy(b.reshape(1, 1, -1))[0].ravel().tolist() == want
    assert M.predict_composite(torch.from_numpy(b).reshape(1, 1, -1))[0].ravel().tolist() == want
    ok = ~np.isnan(b)
    assert ((torch.sigmoid(torch.from_numpy(b)) >= 0.5).numpy()[ok] == np.array(want, bool)[ok]).all()
    from umi import infer
    assert M.SIGMOID_HALF_CUTOFF == infer.SIGMOID_HALF_CUTOFF


def test_meter():
    from umi import metrics as M
    rng = np.random.default_rng(3)
    x = torch.from_numpy(rng.standard_normal((6, 3, 8, 8)).astype(np.float32))
    t = torch.from_numpy(rng.integers(0, 3, (6, 8, 8)))
    meter = M.ConfusionMeter()
    with pytest.raises(RuntimeError):
        meter.read()
    meter.update(x[:2], t[:2]).update(x[2:], t[2:])
    whole = M.confusion_numpy(x.numpy(), t.numpy())[0]
    r = meter.read()
    assert np.array_equal(r["matrix"], whole) and set(r) == {"matrix", "dice", "iou", "precision", "recall"}
    I, Z, Y = np.diagonal(whole)[:3], whole.sum(0)[:3], whole.sum(1)[:3]
    np.testing.assert_array_equal(r["precision"], I / Z)
    np.testing.assert_array_equal(r["recall"], I / Y)
    assert np.float32(1.0 - r["dice"].sum() / 3) == pytest.approx(float(M.scores_numpy(whole, 0)), abs=1e-7)
    meter.add(M.confusion_composite(x, t, 3))
    assert np.array_equal(meter.read()["matrix"], 2 * whole)
    meter.reset()
    assert meter.read()["matrix"].sum() == 0


# ---- calc_loss ----------------------------------------------------------------------------------------------------------------

def test_the_six_names():
    import loss as L
    from umi import metrics as M
    L.CLASS_NUMBER = 3
    rng = np.random.default_rng(4)
    x = torch.from_numpy(rng.standard_normal((6, 3, 9, 7)).astype(np.float32)).requires_grad_(True)
    t = torch.from_numpy(rng.integers(0, 3, (6, 9, 7)).astype(np.float32))
    b = torch.from_numpy(rng.standard_normal((6, 1, 9, 7)).astype(np.float32))
    tb = torch.from_numpy(rng.integers(0, 2, (6, 9, 7)).astype(np.float32))
    cm, cb = M.confusion_numpy(x.detach().numpy(), t.numpy()), M.confusion_numpy(b.numpy(), tb.numpy())
    want = {"dice_err_mc": M.scores_numpy(cm, 0)[0], "iou_err_mc": M.scores_numpy(cm, 1)[0], "pixel_err_mc": M.scores_numpy(cm, 2)[0],
            "dice_err": M.scores_numpy(cb, 0, 1)[0], "iou_err": M.scores_numpy(cb, 1, 1)[0], "pixel_err": M.scores_numpy(cb, 2)[0]}
    assert tuple(L.SEG_METRICS) == NAMES
    for name in NAMES:
        p, l = (x, t) if name.endswith("_mc") else (b, tb)
        v = L.calc_loss(p, l, loss_type=name)
        assert v.shape == () and v.dtype == torch.float32 and not v.requires_grad and v.grad_fn is None
        assert np.array_equal(_bits(v.numpy()), _bits(want[name])), name
        if not name.endswith("_mc"):                           # binary labels may be (B, 1, H, W) too
            assert torch.equal(L.calc_loss(p, l.unsqueeze(1), loss_type=name), v)
        for items in (1, 2, 3, 6):
            n = 6 // items
            for on in (True, False):
                L.METRICS_KERNEL = on
                try:
                    got = L.calc_loss_items(p, l, items, loss_type=name)
                finally:
                    L.METRICS_KERNEL = True
                loop = torch.stack([L.calc_loss(p[i * n:(i + 1) * n], l[i * n:(i + 1) * n], loss_type=name) for i in range(items)])
                assert got.shape == (items,) and torch.equal(got, loop), (name, items, on)
    # the pixel error is what it says
    acc = (torch.argmax(x.detach(), 1) == t).double().mean().item()
    assert abs(float(want["pixel_err_mc"]) - (1.0 - acc)) < 1e-6
    with pytest.raises(ValueError, match="C >= 2"):
        L.calc_loss(b, tb, loss_type="dice_err_mc")
    with pytest.raises(ValueError, match="one-logit"):
        L.calc_loss(x, t, loss_type="dice_err")
    for name in ("dice_score", "dice_score_mc"):               # the reference's broken branches stay refused
        with pytest.raises(NotImplementedError):
            L.calc_loss(x, t, loss_type=name)
    assert not set(NAMES) & (L._BATCH_COUPLED | L._OUT_OF_SCOPE)


def test_per_replica_under_a_global_batch_switch():
    import loss as L
    from umi import ddp
    rng = np.random.default_rng(6)
    x = torch.from_numpy(rng.standard_normal((2, 2, 5, 5)).astype(np.float32))
    t = torch.from_numpy(rng.integers(0, 2, (2, 5, 5)))
    want = L.calc_loss(x, t, loss_type="iou_err_mc")
    ddp.set_active_batch_sync(object())                        # never touched: the names are values of this replica's pixels
    try:
        assert torch.equal(L.calc_loss(x, t, loss_type="iou_err_mc"), want)
    finally:
        ddp.set_active_batch_sync(None)


# ---- Trainer ------------------------------------------------------------------------------------------------------------------

N_VAL = 7


def _loaders(val_from=0, n_val=N_VAL, batch=None):
    xs, ls = recipe.synthetic_batch(4 + N_VAL, 1, 32, 32, 2, seed=21)
    val = [(xs[4 + i:5 + i], ls[4 + i:5 + i]) for i in range(val_from, val_from + n_val)]

    class Items(torch.utils.data.Dataset):
        def __len__(self):
            return len(val)

        def __getitem__(self, i):
            return val[i]
    return {"train": DataLoader(TensorDataset(xs[:4], ls[:4]), batch_size=2, shuffle=False),
            "val": DataLoader(Items(), batch_size=None, shuffle=False)}


def _run(tmp, loaders=None, epochs=3, metric="dice_err_mc", lr=0.05, **kw):
    import loss as L
    from Trainer import Trainer
    torch.manual_seed(0)
    L.CLASS_NUMBER = 2
    m = ref_unet.RefUNet(1, 2, 8, False)
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=21))
    opt = torch.optim.SGD(m.parameters(), lr=lr, momentum=0.9, weight_decay=1e-4)
    os.makedirs(tmp, exist_ok=True)
    tr = Trainer(m, "single", torch.FloatTensor, "cpu", str(tmp), loaders or _loaders(), 2, opt, 25, epochs, "dice_bce_mc", metric,
                 lr_scheduler=True, **kw)
    tr.train()
    return tr


def test_trainer_selects_the_epoch_with_the_lowest_error(tmp_path):
    tr = _run(tmp_path, val_confusion=True)
    scores = tr.val_score_list
    assert len(scores) == 3 and all(0.0 <= s <= 1.0 for s in scores) and scores != tr.val_loss_list
    assert tr.best_val_score == min(scores)
    log = (tmp_path / "logs.txt").read_text()
    saved = [int(e) for e in re.findall(r"Val score on epoch (\d+): [0-9.]+\nsaving best model", log)]
    running, want = 1e15, []
    for e, s in enumerate(scores, 1):
        if s < running:
            running = s
            want.append(e)
    assert saved == want and f"epoch{want[-1]}.pt" in os.listdir(tmp_path / "models")
    assert "confusion" not in log                              # logs.txt is untouched
    # the matrices count every validation pixel once, and their Dice error is not the mean of the items' errors but close
    assert len(tr.val_confusion_list) == 3
    for m in tr.val_confusion_list:
        assert m.shape == (3, 3) and m.dtype == np.int64 and m.sum() == N_VAL * 32 * 32 and m[2].sum() == 0 and m[:, 2].sum() == 0
    assert set(tr.val_class_scores) == {"dice", "iou"} and tr.val_class_scores["dice"].shape == (2,)
    # the score is the mean over the items of the statement on each item's argmax mask
    from umi import metrics as M
    tr.model.load_state_dict(tr.best_model)
    tr.model.eval()
    with torch.no_grad():
        errs = [float(M.scores_numpy(M.confusion_numpy(tr.model(x).numpy(), l.numpy()), 0)[0]) for x, l in _loaders()["val"]]
    assert abs(np.mean(errs) - tr.best_val_score) < 1e-6


def test_val_batch_gives_the_same_lists(tmp_path):
    a = _run(tmp_path / "a", val_batch=3, val_confusion=True)
    b = _run(tmp_path / "b", val_batch=None, val_confusion=True)
    assert a.train_loss_list == b.train_loss_list
    # hard masks: an item's error is a function of integers, so the lists are `==` unless a batch-1 forward and a slice of a
    # batched forward put a pixel on the other side of a tie, which these logits do not
    assert a.val_score_list == b.val_score_list and a.best_val_score == b.best_val_score
    assert [m.tolist() for m in a.val_confusion_list] == [m.tolist() for m in b.val_confusion_list]
    assert sorted(os.listdir(tmp_path / "a" / "models")) == sorted(os.listdir(tmp_path / "b" / "models"))
    # the old names and the default are the old code: no matrix, no accumulator
    c = _run(tmp_path / "c", metric="dice_bce_mc", val_batch=3)
    assert c.val_confusion_list == [] and c._validation().conf is None and c.val_class_scores is None and c.val_score_list == c.val_loss_list
    # val_confusion with an old metric name: the matrices of the same predictions
    d = _run(tmp_path / "d", metric="dice_bce_mc", val_batch=3, val_confusion=True)
    assert d.val_score_list == c.val_score_list
    assert [m.tolist() for m in d.val_confusion_list] == [m.tolist() for m in a.val_confusion_list]


def test_metric_names_are_no_loss_functions(tmp_path):
    from Trainer import Trainer
    m = torch.nn.Linear(1, 1)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    for name in NAMES:
        with pytest.raises(ValueError, match="not differentiable"):
            Trainer(m, "single", torch.FloatTensor, "cpu", str(tmp_path), {"train": [0], "val": [0]}, 1, opt, 1, 1, name, name)
    with pytest.raises(ValueError, match="val_confusion"):
        Trainer(m, "multi_task", torch.FloatTensor, "cpu", str(tmp_path), {"train": [0], "val": [0]}, 1, opt, 1, 1, "mse", "mse",
                val_confusion=True)


def _worker(rank, world, port, q, out_dir):
    dist = init_rank(rank, world, port)
    # unequal validation shards: rank 0 items 0-2, rank 1 items 3-6; both train on the same batches at lr 0, so the weights stay
    tr = _run(os.path.join(out_dir, f"r{rank}"), loaders=_loaders(0 if rank == 0 else 3, 3 if rank == 0 else 4), epochs=2, lr=0.0,
              val_batch=2, val_confusion=True, data_parallel=True)
    q.put((rank, dict(score=tr.val_score_list, conf=[m.tolist() for m in tr.val_confusion_list],
                      per_class={k: v.tolist() for k, v in tr.val_class_scores.items()})))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_agree(tmp_path):
    res = run_ranks(_worker, 2, str(tmp_path))
    a, b = res[0], res[1]
    assert a == b and len(a["conf"]) == 2
    one = _run(tmp_path / "one", epochs=2, lr=0.0, val_batch=2, val_confusion=True)
    assert a["conf"] == [m.tolist() for m in one.val_confusion_list]
    assert a["per_class"] == {k: v.tolist() for k, v in one.val_class_scores.items()}
    np.testing.assert_allclose(a["score"], one.val_score_list, rtol=0, atol=1e-6)      # 7 fp32 adds of values <= 1 against 3 + 4


# ---- C ABI --------------------------------------------------------------------------------------------------------------------

def test_c_abi_refuses_before_any_launch():
    from umi import lib
    BAD, UNS, WS = lib.UMI_ERR_BADARG, lib.UMI_ERR_UNSUPPORTED, lib.UMI_ERR_WORKSPACE
    assert len(lib.STRUCTS) == 5
    buf = (ctypes.c_char * 4096)()                             # host memory: never dereferenced, nothing is launched
    p = ctypes.addressof(buf)
    p += -p % 16
    logits, cm, cs, wsb = (lib.fn(n) for n in ("umi_confusion_logits", "umi_confusion_masks", "umi_confusion_scores",
                                               "umi_confusion_ws_bytes"))
    need = wsb(2, 1, 3, 64)
    assert need == 2 * 1 * 16 * 4 and wsb(2, 1, 9, 64) == 0 and wsb(0, 1, 3, 64) == 0 and wsb(1, 1 << 20, 2, 1 << 20) == 0
    good = dict(src=p, target=p + 512, dt=0, items=2, n=1, C=3, HW=64, counts=p + 1024, ws=p + 2048, ws_bytes=need)

    def call(fn, **kw):
        a = dict(good, **kw)
        return fn(a["src"], a["target"], a["dt"], a["items"], a["n"], a["C"], a["HW"], a["counts"], a["ws"], a["ws_bytes"], None)
    for fn in (logits, cm):
        for kw in (dict(src=None), dict(target=None), dict(counts=None), dict(ws=None), dict(items=0), dict(items=65536), dict(n=0),
                   dict(HW=0), dict(dt=4), dict(dt=-1), dict(target=p + 516), dict(counts=p + 1028)):
            assert call(fn, **kw) == BAD, (fn, kw)
        assert call(fn, C=9) == UNS and call(fn, n=1 << 16, HW=1 << 15) == UNS
        assert call(fn, ws_bytes=need - 1) == WS
    assert call(logits, C=0) == UNS and call(cm, C=1) == UNS and call(cm, C=0) == UNS
    assert call(logits, C=1, ws_bytes=wsb(2, 1, 2, 64) - 1) == WS
    assert cs(None, 1, 3, 0, 0, p, None) == BAD and cs(p, 1, 3, 0, 0, None, None) == BAD and cs(p, 0, 3, 0, 0, p + 512, None) == BAD
    assert cs(p, 1, 3, 3, 0, p + 512, None) == BAD and cs(p, 1, 3, -1, 0, p + 512, None) == BAD
    assert cs(p, 1, 3, 0, 3, p + 512, None) == BAD and cs(p, 1, 3, 0, -1, p + 512, None) == BAD
    assert cs(p, 1, 1, 0, 0, p + 512, None) == UNS and cs(p, 1, 9, 0, 0, p + 512, None) == UNS
