"""The surface-distance kernels (csrc/surface_metrics.hip) on the MI355X against their NumPy statement (umi/surface.py).

hd, hd95, the counts, the state and the fp32 hd / hd95 scores must be bit-identical to the statement: squared distances are exact
integers, the select is an integer select and the roots and the lerp are the same float64 operations.  assd is a float64 sum of
n non-negative roots, so any summation order stays within n * 2^-53 relative of any other; its fp32 score is within 1 ulp.
Shapes: the smallest at which the kernels can go wrong -- one pixel, one row, one column, one 64-column group, more than one
62-column block of the column pass (65, 70, 200), three 64-row chunks (130), eighteen chunks in a thin image (1100, 3): more than
the column pass's sixteen waves, so a wave owns two chunks; and for the checkerboard (20, 300): 300 surface pixels
per row and side exceed the 256-key tile a select block takes per step, and 20 rows exceed its 16 blocks, so blocks loop both ways.
Then calc_loss / calc_loss_items, a replayed GraphedEval group and the Trainer's three validation paths."""
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from tests import poison

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = ((1, 1), (1, 7), (7, 1), (5, 64), (33, 65), (130, 70), (70, 200))
DTYPES = (torch.int64, torch.float32, torch.uint8, torch.int32)
U53 = 2.0 ** -53


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: torch.cuda.is_available() is False")


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _blobs(rng, B, K, H, W):
    """Class maps of 8x8 blocks with a few flipped pixels: compact regions, several boundaries, every class in play."""
    low = rng.integers(0, K, (B, (H + 7) // 8, (W + 7) // 8))
    m = np.kron(low, np.ones((8, 8), np.int64))[:, :H, :W]
    flip = rng.random((B, H, W)) < 0.03
    return np.where(flip, rng.integers(0, K, (B, H, W)), m)


def _contents(rng, B, K, H, W):
    """name -> (pred uint8 [B, H, W], label int64 [B, H, W])."""
    yy, xx = np.mgrid[:H, :W]
    z = np.zeros((B, H, W), np.int64)
    a, g = _blobs(rng, B, K, H, W), _blobs(rng, B, K, H, W)
    corner_a, corner_g, far = z.copy(), z.copy(), z.copy()
    corner_a[:, 0, 0] = 1
    corner_g[:, -1, -1] = 1
    far[:, 0, 0] = 1                                  # two prediction pixels, one next to the label's: the two ranks of hd95 lie
    far[:, -1, max(W - 2, 0)] = 1                     # in different level-1 bins of the select once the diagonal passes 64
    checker = np.broadcast_to((yy + xx) % 2, (B, H, W)).astype(np.int64)
    notclass = np.where(rng.random((B, H, W)) < 0.2, 255, g)
    return {"blobs": (a, g), "full": (z + 1, z + 1), "full vs blobs": (z + (K - 1), g), "identical": (a, a),
            "corners": (corner_a, corner_g), "far": (far, corner_g), "checker": (checker, 1 - checker),
            "checker vs itself": (checker, checker), "prediction empty": (z, g), "label empty": (a, z), "both empty": (z, z),
            "not a class": (a, notclass)}


_REF = {}


def _reference(key, pred, label, K, c0):
    """The statement of one case, computed once and shared."""
    from umi import surface as S
    if key not in _REF:
        _REF[key] = S.surface_numpy(pred, label, K, c0)
    return _REF[key]


def _check(pred, label, K, c0, key, items=None):
    """Kernel against statement: stats, counts, and the scores of the three kinds under the three empty rules."""
    from umi import surface as S
    pred = np.ascontiguousarray(pred)
    label = label if torch.is_tensor(label) else np.ascontiguousarray(label)
    want_s, want_c = _reference(key, pred, label.numpy() if torch.is_tensor(label) else label, K, c0)
    t = label if torch.is_tensor(label) else torch.from_numpy(label)
    stats, counts = S.surface(torch.from_numpy(pred).to(DEV), t.to(DEV), K, c0)
    assert stats.dtype == torch.float64 and counts.dtype == torch.int64 and stats.shape == want_s.shape
    gs, gc = stats.cpu().numpy(), counts.cpu().numpy()
    assert np.array_equal(gc, want_c), (key, gc, want_c)
    assert np.array_equal(gs[..., 3], want_s[..., 3]), (key, gs[..., 3], want_s[..., 3])
    for k in (0, 1):
        assert np.array_equal(_bits64(gs[..., k]), _bits64(want_s[..., k])), (key, k, gs[..., k], want_s[..., k])
    n = want_c.sum(axis=-1).astype(np.float64)
    assert (np.abs(gs[..., 2] - want_s[..., 2]) <= n * U53 * want_s[..., 2]).all(), (key, gs[..., 2], want_s[..., 2])
    B, (H, W) = pred.shape[0], pred.shape[1:]
    for it in ((1, B) if items is None else items):
        for rule in ("diagonal", "zero", "nan"):
            for kind in ("hd", "hd95", "assd"):
                got = S.surface_scores(stats, it, kind, c0, rule, (H, W))
                assert got.is_cuda and got.dtype == torch.float32 and got.shape == (it,)
                want = S.surface_scores_numpy(want_s, it, kind, c0, rule, (H, W))
                if kind != "assd":
                    assert np.array_equal(_bits32(got.cpu().numpy()), _bits32(want)), (key, it, rule, kind, got, want)
                else:
                    g64, w64 = got.cpu().numpy().astype(np.float64), want.astype(np.float64)
                    ok = (np.isnan(g64) & np.isnan(w64)) | (np.abs(g64 - w64) <= np.spacing(np.abs(want)).astype(np.float64))
                    assert ok.all(), (key, it, rule, got, want)
    return stats, counts


@pytest.mark.parametrize("H,W", SHAPES + ((1100, 3), (20, 300)))
def test_kernels_equal_the_statement(H, W):
    _need_gpu()
    rng = np.random.default_rng(1000 * H + W)
    for B in (1, 3):
        for K in (2, 4):
            for name, (a, g) in _contents(rng, B, K, H, W).items():
                if (H, W) == (20, 300) and not name.startswith("checker"):
                    continue
                _check(a.astype(np.uint8), g, K, 1, (H, W, B, K, name))
    a, g = _contents(rng, 2, 3, H, W)["blobs"]
    _check(a.astype(np.uint8), g, 3, 0, (H, W, "c0 = 0"))           # the background's surface too
    _check(a.astype(np.uint8), g, 3, 2, (H, W, "c0 = 2"))


@pytest.mark.parametrize("dtype", DTYPES)
def test_every_label_dtype_with_labels_that_are_no_class(dtype):
    _need_gpu()
    rng = np.random.default_rng(21)
    B, K, H, W = 2, 3, 33, 65
    a = _blobs(rng, B, K, H, W).astype(np.uint8)
    g = _blobs(rng, B, K, H, W)
    if dtype == torch.float32:
        f = g.astype(np.float32)
        f[rng.random(g.shape) < 0.1] = 1.5
        f[rng.random(g.shape) < 0.05] = np.nan
        label = torch.from_numpy(f)
    elif dtype == torch.uint8:
        label = torch.from_numpy(np.where(rng.random(g.shape) < 0.15, 255, g).astype(np.uint8))
    else:
        label = torch.from_numpy(np.where(rng.random(g.shape) < 0.15, -1, g)).to(dtype)
    _check(a, label, K, 1, ("dtype", str(dtype)))
    stats4, counts4 = _check(a, label.unsqueeze(1), K, 1, ("dtype", str(dtype)))        # labels (B, 1, H, W)
    assert stats4.shape == (B, K, 4) and counts4.shape == (B, K, 2)


def test_preset_memory_and_a_second_run_do_not_matter():
    _need_gpu()
    from umi import surface as S
    rng = np.random.default_rng(22)
    B, K, H, W = 3, 4, 130, 70
    a = torch.from_numpy(_blobs(rng, B, K, H, W).astype(np.uint8)).to(DEV)
    g = torch.from_numpy(_blobs(rng, B, K, H, W)).to(DEV)
    got = []
    for byte in (0x00, 0xFF, 0x00):
        with poison.poisoned(byte):
            stats, counts = S.surface(a, g, K, 1)
            score = S.surface_scores(stats, B, "hd95", 1, "diagonal", (H, W))
        got.append((stats.cpu(), counts.cpu(), score.cpu()))
    want_s, want_c = S.surface_numpy(a.cpu().numpy(), g.cpu().numpy(), K, 1)
    assert torch.equal(got[0][1], torch.from_numpy(want_c))
    for other in got[1:]:
        for x, y in zip(got[0], other):
            assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert torch.isfinite(got[1][0]).all()


def test_inputs_the_kernels_do_not_take_use_the_composite():
    _need_gpu()
    import loss as L
    from umi import surface as S
    rng = np.random.default_rng(23)
    big = torch.from_numpy(_blobs(rng, 2, 3, 40, 96).astype(np.uint8)).to(DEV)
    view = big[:, :, ::2]                                             # a non-contiguous mask
    g = torch.from_numpy(_blobs(rng, 2, 3, 40, 48)).to(DEV)
    assert not S.surface_kernel_ok(view, g, 3) and S.surface_kernel_ok(view.contiguous(), g, 3)
    with pytest.raises(ValueError):
        S.surface(view, g, 3, 1)
    cs, cc = S.surface_composite(view, g, 3, 1)
    ks, kc = S.surface(view.contiguous(), g, 3, 1)
    assert cs.is_cuda and torch.equal(cc, kc) and torch.equal(cs[..., (0, 1, 3)], ks[..., (0, 1, 3)])
    assert torch.allclose(cs[..., 2], ks[..., 2], rtol=1e-12, atol=0)
    # non-contiguous logits through calc_loss: the composite, the same hd95
    x = torch.from_numpy(rng.standard_normal((2, 3, 40, 96)).astype(np.float32)).to(DEV)
    lab = torch.from_numpy(_blobs(rng, 2, 3, 40, 48)).to(DEV)
    xv = x[:, :, :, ::2]
    assert torch.equal(L.calc_loss(xv, lab, loss_type="hd95_mc"), L.calc_loss(xv.contiguous(), lab, loss_type="hd95_mc"))


def test_argument_refusals_launch_nothing():
    """Return codes only: every refusal is decided on the host before any launch."""
    _need_gpu()
    from umi import lib
    f, w = lib.fn("umi_surface_distances"), lib.fn("umi_surface_ws_bytes")
    buf = torch.zeros(1 << 18, dtype=torch.uint8, device=DEV)            # the histograms alone take 64 KiB per (image, class)
    p = buf.data_ptr()
    ok = (p, p, 2, 1, 2, 1, 8, 8, p, p, p, buf.numel(), None)
    assert w(1, 2, 1, 8, 8) > 0 and w(1, 2, 1, 8, 8) <= buf.numel()

    def call(**kw):
        names = ("pred", "target", "dtype", "B", "K", "c0", "H", "W", "stats", "counts", "ws", "ws_bytes", "stream")
        return f(*[kw.get(n, v) for n, v in zip(names, ok)])
    assert call(pred=None) == lib.UMI_ERR_BADARG and call(dtype=4) == lib.UMI_ERR_BADARG and call(c0=2) == lib.UMI_ERR_BADARG
    assert call(stats=p + 4) == lib.UMI_ERR_BADARG and call(B=0) == lib.UMI_ERR_BADARG
    assert call(H=4097) == lib.UMI_ERR_UNSUPPORTED and call(K=9) == lib.UMI_ERR_UNSUPPORTED and call(K=1) == lib.UMI_ERR_UNSUPPORTED
    assert call(B=128, H=4096, W=4096) == lib.UMI_ERR_UNSUPPORTED and w(128, 2, 1, 4096, 4096) == 0
    assert call(ws_bytes=w(1, 2, 1, 8, 8) - 1) == lib.UMI_ERR_WORKSPACE
    sc = lib.fn("umi_surface_scores")
    assert sc(p, 1, 1, 2, 1, 3, 0, 8, 8, p, None) == lib.UMI_ERR_BADARG and sc(p, 1, 1, 2, 1, 0, 3, 8, 8, p, None) == lib.UMI_ERR_BADARG
    assert sc(p, 1, 1, 9, 1, 0, 0, 8, 8, p, None) == lib.UMI_ERR_UNSUPPORTED and sc(p, 1, 1, 2, 2, 0, 0, 8, 8, p, None) == lib.UMI_ERR_BADARG
    torch.cuda.synchronize()
    assert int(buf.sum()) == 0                                        # nothing was written


@pytest.fixture
def device_calls():
    """Counts the calls of umi.surface.surface (the kernel entry) and of the host composite."""
    from umi import surface as S
    calls = {"kernel": 0, "composite": 0}
    real_k, real_c = S.surface, S.surface_composite

    def kernel(*a, **k):
        calls["kernel"] += 1
        return real_k(*a, **k)

    def composite(*a, **k):
        calls["composite"] += 1
        return real_c(*a, **k)
    S.surface, S.surface_composite = kernel, composite
    try:
        yield calls
    finally:
        S.surface, S.surface_composite = real_k, real_c


def _logits(rng, B, C, H, W):
    """Logits whose argmax / threshold mask is a blob map."""
    cls = _blobs(rng, B, max(C, 2), H, W)
    if C == 1:
        return torch.from_numpy(((cls > 0) * 2.0 - 1.0 + 0.1 * rng.standard_normal((B, H, W))).astype(np.float32)[:, None])
    x = 0.1 * rng.standard_normal((B, C, H, W))
    x[np.arange(B)[:, None, None], cls, np.arange(H)[None, :, None], np.arange(W)[None, None, :]] += 1.0
    return torch.from_numpy(x.astype(np.float32))


def test_calc_loss_takes_the_kernels_and_equals_the_statement(device_calls):
    _need_gpu()
    import loss as L
    from umi import metrics as M, surface as S
    rng = np.random.default_rng(24)
    H, W = 40, 72
    mc = (_logits(rng, 6, 3, H, W).to(DEV), torch.from_numpy(_blobs(rng, 6, 3, H, W)).to(DEV))
    bn = (_logits(rng, 6, 1, H, W).to(DEV), torch.from_numpy(_blobs(rng, 6, 2, H, W).astype(np.float32)).to(DEV))
    expected = 0
    for name, (kind, multi) in L.SURFACE_METRICS.items():
        p, t = mc if multi else bn
        K = p.shape[1] if multi else 2
        mask = M.predict_numpy(p.cpu().numpy())[0].astype(np.uint8)
        want_stats, _ = S.surface_numpy(mask, t.cpu().numpy(), K, 1)
        for items in (1, 2, 3, 6):
            n = 6 // items
            got = L.calc_loss_items(p, t, items, loss_type=name)
            loop = torch.stack([L.calc_loss(p[i * n:(i + 1) * n], t[i * n:(i + 1) * n], loss_type=name) for i in range(items)])
            expected += 1 + items
            assert got.shape == (items,) and got.dtype == torch.float32 and got.is_cuda and not got.requires_grad
            assert torch.equal(got, loop), (name, items)
            want = S.surface_scores_numpy(want_stats, items, kind, 1, "diagonal", (H, W))
            if kind != 2:
                assert np.array_equal(_bits32(got.cpu().numpy()), _bits32(want)), (name, items)
            else:
                assert (np.abs(got.cpu().numpy().astype(np.float64) - want) <= np.spacing(want)).all(), (name, items)
        if not multi:                                                 # binary labels (B, 1, H, W)
            assert torch.equal(L.calc_loss(p, t.unsqueeze(1), loss_type=name), L.calc_loss(p, t, loss_type=name))
            expected += 2
    assert device_calls == {"kernel": expected, "composite": 0}
    try:                                                              # the switch sends everything to the host composite
        L.METRICS_KERNEL = False
        off = L.calc_loss_items(mc[0], mc[1], 3, loss_type="hd95_mc")
    finally:
        L.METRICS_KERNEL = True
    assert device_calls == {"kernel": expected, "composite": 1}
    assert torch.equal(off, L.calc_loss_items(mc[0], mc[1], 3, loss_type="hd95_mc"))
    with pytest.raises(ValueError):
        L.calc_loss(bn[0], bn[1], loss_type="hd95_mc")
    with pytest.raises(ValueError):
        L.calc_loss(mc[0], mc[1], loss_type="hd95")


def test_a_graphed_group_replays_to_the_eager_bits():
    _need_gpu()
    import loss as L
    import Model
    from umi import graph as G
    from umi.graphs import GraphedEval
    L.CLASS_NUMBER = 2
    torch.manual_seed(3)
    m = Model.UNet(1, 2, 8, False, compute_dtype="fp16").to(DEV).eval()
    g = torch.Generator().manual_seed(12)
    xs = [torch.randn(3, 1, 38, 50, generator=g).to(DEV) for _ in range(2)]
    lab = torch.randint(0, 2, (3, 38, 50), generator=g).float().to(DEV)

    def fn(x, ls):
        return L.calc_loss_items(m(x), ls, 3, loss_type="hd95_mc")
    with torch.no_grad():
        eager = [fn(x, lab).clone() for x in xs]
        ge = GraphedEval(fn, [xs[0], lab], pack_cache=G.pack_cache_of(m))
        replayed = [ge(x, lab).clone() for x in xs]
    torch.cuda.synchronize()
    for e, r in zip(eager, replayed):
        assert torch.equal(e.view(torch.int32), r.view(torch.int32)), (e, r)
    assert torch.isfinite(eager[0]).all()


# ---- Trainer ------------------------------------------------------------------------------------------------------------------

EPOCHS, N_VAL = 2, 7


class _Items(torch.utils.data.Dataset):
    def __init__(self, items):
        self.items = items

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _data():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(4 + N_VAL, 1, 32, 32, generator=g)
    low = torch.randint(0, 2, (4 + N_VAL, 4, 4), generator=g)
    lab = low.repeat_interleave(8, dim=1).repeat_interleave(8, dim=2).float()
    val = [(x[4 + i:5 + i], lab[4 + i:5 + i]) for i in range(N_VAL)]
    return {"train": DataLoader(TensorDataset(x[:4], lab[:4]), batch_size=2, shuffle=False),
            "val": DataLoader(_Items(val), batch_size=None, shuffle=False)}


def _train(out_dir, **kw):
    import loss as L
    import Model
    from Trainer import Trainer
    from umi import optim as uo
    L.CLASS_NUMBER = 2
    torch.manual_seed(100)
    m = Model.UNet(1, 2, 8, False, compute_dtype="fp16").to(DEV)
    opt = uo.SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    os.makedirs(out_dir, exist_ok=True)
    tr = Trainer(m, "single", torch.cuda.FloatTensor, DEV, str(out_dir), _data(), 2, opt, 25, EPOCHS, "dice_bce_mc", "hd95_mc",
                 lr_scheduler=True, **kw)
    tr.train()
    return tr


def test_nine_classes_stay_eager_under_graph(tmp_path, device_calls):
    """The kernels stop at eight classes: a 9-class model's 'hd95_mc' runs the host composite, which cannot be captured, so under
    graph=True its full validation groups stay eager (no eval graph, no capture error) and add up the item-by-item scores."""
    _need_gpu()
    import warnings
    import loss as L
    import Model
    from Trainer import Trainer
    from umi import optim as uo
    g = torch.Generator().manual_seed(9)
    x = torch.randn(9, 1, 32, 32, generator=g).to(DEV)
    lab = torch.randint(0, 9, (9, 4, 4), generator=g).repeat_interleave(8, dim=1).repeat_interleave(8, dim=2).float().to(DEV)
    items = [(x[i:i + 1], lab[i:i + 1]) for i in range(9)]
    try:
        L.CLASS_NUMBER = 9
        torch.manual_seed(100)
        m = Model.UNet(1, 9, 8, False, compute_dtype="fp16").to(DEV).eval()
        tr = Trainer(m, "single", torch.cuda.FloatTensor, DEV, str(tmp_path), {"train": [0], "val": items}, 2,
                     uo.SGD(m.parameters(), lr=0.05), 25, 1, "dice_bce_mc", "hd95_mc", graph=True, val_batch=3)
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            for i in range(0, 9, 3):                                  # three full groups of one shape: eager, eager, eager
                tr._validation().run_group(items[i:i + 3])
            total = torch.zeros((), device=DEV)
            for xi, li in items:
                total = total + tr.eval_step(xi, li)[1]
        torch.cuda.synchronize()
    finally:
        L.CLASS_NUMBER = 2
    assert any("host copies" in str(w.message) for w in seen)
    assert len(tr._validation().graphs) == 0 and len(tr._validation().host) == 1 and len(tr._validation().seen) == 0
    assert torch.isfinite(total) and float(tr._validation().sums[1]) == float(total)
    assert device_calls["kernel"] == 0 and device_calls["composite"] == 3 + 9


def test_trainer_paths_agree(tmp_path, device_calls):
    """Seven validation items of 32x32, two epochs: item by item, val_batch=3 (3 + 3 + 1) and val_batch=3 replayed give `==`
    lists; val_confusion=True next to the surface metric keeps the scores."""
    _need_gpu()
    runs = {}
    for name, kw in (("items", dict(val_batch=None, graph=False)), ("batched", dict(val_batch=3, graph=False)),
                     ("replayed", dict(val_batch=3, graph=True)), ("confusion", dict(val_batch=3, graph=True, val_confusion=True))):
        tr = _train(tmp_path / name, **kw)
        assert len(tr._validation().graphs) == (0 if name in ("items", "batched") else 1)
        runs[name] = dict(val=tr.val_loss_list, score=tr.val_score_list, best=tr.best_val_score)
    a = runs["items"]
    assert len(a["score"]) == EPOCHS and all(np.isfinite(s) and 0.0 <= s <= 31 * 2 ** 0.5 + 1e-6 for s in a["score"])
    assert a["val"] != a["score"] and a["best"] == min(a["score"])
    for name in ("batched", "replayed", "confusion"):
        assert runs[name] == a, (name, runs[name], a)
    assert device_calls["kernel"] > 0 and device_calls["composite"] == 0
