"""Surface-distance metrics without a GPU: the NumPy statement (umi/surface.py) against values recorded from live SciPy / NumPy
(tests/golden/surface_metrics.npz, written by tools/gen_golden_surface_metrics.py) and, where SciPy is installed, against the live
composition on random pairs; the empty rules, labels that are no class, the six names of `calc_loss`, the Trainer, the meter and
the C ABI's refusals.

hd, hd95, the counts and the states must be bit-identical: squared distances are exact integers, the float64 root is correctly
rounded and the percentile's lerp is spelled out operation for operation.  assd is held to n * 2^-53 relative of math.fsum over the
same roots: all n terms are non-negative, so any summation order stays inside that bound."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from oracle import recipe, ref_unet
from tests.test_global_batch import init_rank, run_ranks

NAMES = ("hd_mc", "hd95_mc", "assd_mc", "hd", "hd95", "assd")
U53 = 2.0 ** -53


def _bits64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def _golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "surface_metrics.npz"))
    for i, (H, W) in enumerate(z["shapes"]):
        lo, hi = z["offsets"][i], z["offsets"][i + 1]
        a = np.unpackbits(z["pred_bits"][lo:hi])[:H * W].reshape(H, W).astype(bool)
        g = np.unpackbits(z["label_bits"][lo:hi])[:H * W].reshape(H, W).astype(bool)
        yield i, a, g, z


def _fsum_assd(a, g):
    """assd of one non-empty pair with exactly rounded sums of the statement's own roots."""
    from umi import surface as S
    sa, sg = S.surface_mask(a), S.surface_mask(g)
    dag = np.sqrt(S.directed_d2(sa, sg).astype(np.float64))
    dga = np.sqrt(S.directed_d2(sg, sa).astype(np.float64))
    return (math.fsum(dag) / len(dag) + math.fsum(dga) / len(dga)) / 2.0, len(dag) + len(dga)


def test_statement_equals_the_recorded_scipy_values(golden_dir):
    from umi import surface as S
    seen = set()
    for i, a, g, z in _golden(golden_dir):
        stats, counts = S.surface_numpy(a[None].astype(np.uint8), g[None].astype(np.int64), 2, 1)
        assert (stats[0, 0] == 0).all() and (counts[0, 0] == 0).all()            # class 0 < c0 is not scored
        assert counts[0, 1].tolist() == z["counts"][i].tolist() and int(stats[0, 1, 3]) == int(z["state"][i]), i
        assert _bits64(stats[0, 1, 0]) == _bits64(z["hd"][i]) and _bits64(stats[0, 1, 1]) == _bits64(z["hd95"][i]), i
        if z["state"][i] == 0:
            exact, n = _fsum_assd(a, g)
            assert abs(stats[0, 1, 2] - exact) <= n * U53 * exact and abs(z["assd"][i] - exact) <= n * U53 * exact, i
        else:
            assert stats[0, 1, 2] == 0.0
        seen.add(int(z["state"][i]))
    assert seen == {0, 1, 2, 3}


def test_statement_equals_live_scipy_on_random_pairs():
    ndi = pytest.importorskip("scipy.ndimage")
    from umi import surface as S
    rng = np.random.default_rng(5)
    st = ndi.generate_binary_structure(2, 1)
    for _ in range(60):
        H, W = rng.integers(1, 40, 2)
        a, g = rng.random((H, W)) < rng.uniform(0.02, 1.0), rng.random((H, W)) < rng.uniform(0.02, 1.0)
        if not (a.any() and g.any()):
            continue
        sa, sg = a ^ ndi.binary_erosion(a, st), g ^ ndi.binary_erosion(g, st)
        assert np.array_equal(sa, S.surface_mask(a)) and np.array_equal(sg, S.surface_mask(g))
        dag, dga = ndi.distance_transform_edt(~sg)[sa], ndi.distance_transform_edt(~sa)[sg]
        assert np.array_equal(_bits64(dag), _bits64(np.sqrt(S.directed_d2(sa, sg).astype(np.float64))))
        S_ = np.hstack([dag, dga])
        stats, counts = S.surface_numpy(a[None].astype(np.uint8), g[None].astype(np.float32), 2, 1)
        assert counts[0, 1].tolist() == [sa.sum(), sg.sum()]
        assert _bits64(stats[0, 1, 0]) == _bits64(S_.max()) and _bits64(stats[0, 1, 1]) == _bits64(np.percentile(S_, 95))
        exact, n = _fsum_assd(a, g)
        assert abs(stats[0, 1, 2] - exact) <= n * U53 * exact


def test_empty_rules_states_and_labels_that_are_no_class():
    from umi import surface as S
    one, zero = np.ones((1, 1, 1), np.uint8), np.zeros((1, 1, 1), np.uint8)
    # 1x1 images: the four states; the diagonal of a 1x1 image is 0
    for a, g, state in ((one, one, 0), (zero, zero, 1), (zero, one, 2), (one, zero, 3)):
        stats, counts = S.surface_numpy(a, g.astype(np.int64), 2, 1)
        assert stats[0, 1].tolist() == [0.0, 0.0, 0.0, float(state)] and counts[0, 1].tolist() == [int(a[0, 0, 0]), int(g[0, 0, 0])]
        for kind in ("hd", "hd95", "assd"):
            assert S.surface_scores_numpy(stats, 1, kind, 1, "diagonal", (1, 1)).tolist() == [0.0]
            assert S.surface_scores_numpy(stats, 1, kind, 1, "zero").tolist() == [0.0]
            v = S.surface_scores_numpy(stats, 1, kind, 1, "nan")[0]
            assert np.isnan(v) if state in (2, 3) else v == 0.0
    # a 4x6 image: an empty side scores the diagonal sqrt(9 + 25), averaged with the other class and image in float64
    a = np.zeros((2, 4, 6), np.uint8)
    a[0, 1:3, 1:4] = 1
    a[1, 0, 0] = 2
    g = np.zeros((2, 4, 6), np.int64)
    g[0, 1:3, 2:5] = 1
    stats, _ = S.surface_numpy(a, g, 3, 1)
    assert stats[:, :, 3].tolist() == [[0.0, 0.0, 1.0], [0.0, 1.0, 3.0]]
    diag = np.sqrt(np.float64(34.0))
    want = np.float32((((stats[0, 1, 0] + 0.0) + 0.0) + diag) / np.float64(4))
    assert S.surface_scores_numpy(stats, 1, "hd", 1, "diagonal", (4, 6)).tolist() == [want]
    assert S.surface_scores_numpy(stats, 2, "hd", 1, "zero").tolist() == [np.float32(stats[0, 1, 0] / 2), 0.0]
    assert np.isnan(S.surface_scores_numpy(stats, 2, "hd", 1, "nan")).tolist() == [False, True]
    with pytest.raises(ValueError):
        S.surface_scores_numpy(stats, 1, "hd", 1, "diagonal")
    with pytest.raises(ValueError):
        S.surface_scores_numpy(stats, 1, "hd", 1, "largest", (4, 6))
    # labels that are no class: 255, 1.5, NaN are outside every G
    lab = np.array([[[1, 1, 255, 255]]], np.uint8)
    pm = np.array([[[1, 1, 1, 1]]], np.uint8)
    stats, counts = S.surface_numpy(pm, lab, 2, 1)
    assert counts[0, 1].tolist() == [4, 2] and stats[0, 1, 0] == 2.0
    f = np.array([[[1.0, 1.5, np.nan, 0.0]]], np.float32)
    stats, counts = S.surface_numpy(pm, f, 2, 1)
    assert counts[0, 1].tolist() == [4, 1] and stats[0, 1, 0] == 3.0
    stats, counts = S.surface_numpy(pm, np.full((1, 1, 4), np.nan, np.float32), 2, 1)
    assert stats[0, 1, 3] == 3.0 and counts[0, 1].tolist() == [4, 0]


def _inputs(rng, B, C, H, W):
    x = torch.from_numpy(rng.standard_normal((B, C, H, W)).astype(np.float32))
    low = rng.integers(0, max(C, 2), (B, (H + 3) // 4, (W + 3) // 4))
    return x, torch.from_numpy(np.kron(low, np.ones((4, 4), np.int64))[:, :H, :W].copy())


def test_the_six_names():
    import loss as L
    from umi import metrics as M, surface as S
    assert tuple(L.SURFACE_METRICS) == NAMES and L.SURFACE_EMPTY == "diagonal"
    assert not set(L.SURFACE_METRICS) & (L._BATCH_COUPLED | L._OUT_OF_SCOPE) and not set(L.SURFACE_METRICS) & set(L.SEG_METRICS)
    rng = np.random.default_rng(3)
    mc, bn = _inputs(rng, 6, 3, 12, 17), _inputs(rng, 6, 1, 12, 17)
    bn = (bn[0], bn[1].float())
    for name, (kind, multi) in L.SURFACE_METRICS.items():
        p, t = mc if multi else bn
        K = 3 if multi else 2
        stats, _ = S.surface_numpy(M.predict_numpy(p.numpy())[0].astype(np.uint8), t.numpy(), K, 1)
        one = L.calc_loss(p, t, loss_type=name)
        assert one.shape == () and one.dtype == torch.float32 and not one.requires_grad
        for items in (1, 2, 3, 6):
            n = 6 // items
            got = L.calc_loss_items(p, t, items, loss_type=name)
            loop = torch.stack([L.calc_loss(p[i * n:(i + 1) * n], t[i * n:(i + 1) * n], loss_type=name) for i in range(items)])
            assert got.shape == (items,) and got.dtype == torch.float32 and torch.equal(got, loop), (name, items)
            assert np.array_equal(got.numpy(), S.surface_scores_numpy(stats, items, kind, 1, "diagonal", (12, 17)))
        if not multi:
            assert torch.equal(L.calc_loss(p, t.unsqueeze(1), loss_type=name), one)          # labels (B, 1, H, W)
        with pytest.raises(ValueError, match="C >= 2" if multi else "one-logit"):
            L.calc_loss(*(bn if multi else mc), loss_type=name)
        with pytest.raises(ValueError, match=r"\(B, C, H, W\)"):
            L.calc_loss(p[:, :, 0], t[:, 0], loss_type=name)
        with pytest.raises(ValueError):
            L.calc_loss(p, t[:, :-1], loss_type=name)
    # the empty rule is read at call time
    p = torch.zeros(1, 2, 5, 5)
    p[:, 0] = 1.0                                                                # predicts background everywhere
    t = torch.zeros(1, 5, 5, dtype=torch.int64)
    t[0, 2, 2] = 1
    try:
        assert float(L.calc_loss(p, t, loss_type="hd95_mc")) == np.float32(np.sqrt(32.0))
        L.SURFACE_EMPTY = "zero"
        assert float(L.calc_loss(p, t, loss_type="hd95_mc")) == 0.0
        L.SURFACE_EMPTY = "nan"
        assert math.isnan(float(L.calc_loss(p, t, loss_type="hd95_mc")))
    finally:
        L.SURFACE_EMPTY = "diagonal"
    # per replica under a global-batch switch; calc_loss_items raises there like every name
    from umi import ddp
    want = L.calc_loss(*mc, loss_type="hd95_mc")
    ddp.set_active_batch_sync(object())
    try:
        assert torch.equal(L.calc_loss(*mc, loss_type="hd95_mc"), want)
    finally:
        ddp.set_active_batch_sync(None)


def test_meter_against_the_statement():
    from umi import surface as S
    rng = np.random.default_rng(4)
    K = 3
    meter = S.SurfaceMeter(K)
    with pytest.raises(RuntimeError):
        meter.read()
    all_stats = []
    for B in (2, 1, 3):
        _, a = _inputs(rng, B, K, 16, 20)
        _, g = _inputs(rng, B, K, 16, 20)
        if B == 1:
            g[:] = 0                                                             # label-empty cases
        meter.add(a.to(torch.uint8), g)
        all_stats.append(S.surface_numpy(a.numpy().astype(np.uint8), g.numpy(), K, 1)[0])
    st = np.concatenate(all_stats)
    got = meter.read()
    assert got["states"].shape == (K, 4) and got["states"][0].tolist() == [0, 0, 0, 0] and got["states"][1:].sum() == 6 * 2
    for c in range(1, K):
        ok = st[:, c, 3] == 0
        assert got["states"][c].tolist() == [int((st[:, c, 3] == s).sum()) for s in range(4)]
        for k, name in enumerate(("hd", "hd95", "assd")):
            np.testing.assert_allclose(got[name][c], st[ok, c, k].mean(), rtol=1e-12)
    assert np.isnan(got["hd"][0])
    meter.reset()
    assert meter.read()["states"].sum() == 0


# ---- Trainer ------------------------------------------------------------------------------------------------------------------

N_VAL = 7


def _loaders(val_from=0, n_val=N_VAL):
    xs, ls = recipe.synthetic_batch(4 + N_VAL, 1, 32, 32, 2, seed=21)
    val = [(xs[4 + i:5 + i], ls[4 + i:5 + i]) for i in range(val_from, val_from + n_val)]

    class Items(torch.utils.data.Dataset):
        def __len__(self):
            return len(val)

        def __getitem__(self, i):
            return val[i]
    return {"train": DataLoader(TensorDataset(xs[:4], ls[:4]), batch_size=2, shuffle=False),
            "val": DataLoader(Items(), batch_size=None, shuffle=False)}


def _run(tmp, loaders=None, lr=0.05, **kw):
    import loss as L
    from Trainer import Trainer
    torch.manual_seed(0)
    L.CLASS_NUMBER = 2
    m = ref_unet.RefUNet(1, 2, 8, False)
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=21))
    opt = torch.optim.SGD(m.parameters(), lr=lr, momentum=0.9, weight_decay=1e-4)
    os.makedirs(tmp, exist_ok=True)
    tr = Trainer(m, "single", torch.FloatTensor, "cpu", str(tmp), loaders or _loaders(), 2, opt, 25, 2, "dice_bce_mc", "hd95_mc",
                 lr_scheduler=True, **kw)
    tr.train()
    return tr


def test_trainer_scores_with_hd95(tmp_path):
    from umi import metrics as M, surface as S
    a = _run(tmp_path / "a", val_batch=None)
    b = _run(tmp_path / "b", val_batch=3)
    c = _run(tmp_path / "c", val_batch=3, val_confusion=True)
    assert len(a.val_score_list) == 2 and a.val_score_list != a.val_loss_list and a.best_val_score == min(a.val_score_list)
    # hard masks: an item's value is a function of integers, so the lists are `==` (the soft loss of a batched forward is not)
    assert a.val_score_list == b.val_score_list == c.val_score_list and a.train_loss_list == b.train_loss_list
    assert len(c.val_confusion_list) == 2 and a.val_confusion_list == []
    # the score is the mean over the items of the statement on each item's argmax mask
    a.model.load_state_dict(a.best_model)
    a.model.eval()
    vals = []
    with torch.no_grad():
        for x, l in _loaders()["val"]:
            mask = M.predict_numpy(a.model(x).numpy())[0].astype(np.uint8)
            vals.append(float(S.surface_scores_numpy(S.surface_numpy(mask, l.numpy(), 2, 1)[0], 1, "hd95", 1, "diagonal", (32, 32))[0]))
    assert abs(np.mean(vals) - a.best_val_score) < 1e-4


def test_surface_names_are_no_loss_functions(tmp_path):
    from Trainer import Trainer
    m = torch.nn.Linear(1, 1)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    for name in NAMES:
        with pytest.raises(ValueError, match="not differentiable"):
            Trainer(m, "single", torch.FloatTensor, "cpu", str(tmp_path), {"train": [0], "val": [0]}, 1, opt, 1, 1, name, name)


def test_groups_that_copy_to_the_host_are_never_captured(tmp_path):
    """The Trainer's capture decision (no device needed): a full validation group is captured only after an eager run in which no
    surface metric took the host composite -- which nine channels do, the kernels stopping at eight -- and only while the
    kernels are switched on."""
    import loss as L
    from Trainer import Trainer
    m = torch.nn.Linear(1, 1)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    tr = Trainer(m, "single", torch.FloatTensor, "cpu", str(tmp_path), {"train": [0], "val": [0]}, 1, opt, 1, 1, "dice_bce_mc",
                 "hd95_mc", graph=True, val_batch=3)
    rng = np.random.default_rng(8)
    key9, key3 = ((3, 9, 8, 8), (3, 8, 8)), ((3, 3, 8, 8), (3, 8, 8))
    assert not tr._validation().capture_ok(key9)                                         # never seen: the first group runs eagerly
    before = L.surface_host_calls()
    x9, t9 = _inputs(rng, 3, 9, 8, 8)
    L.calc_loss_items(x9, t9, 3, loss_type="hd95_mc")                            # CPU tensors: the composite, like 9 channels on a device
    assert L.surface_host_calls() == before + 1
    tr._validation().note_eager(key9, before)
    assert key9 in tr._validation().host and key9 not in tr._validation().seen and not tr._validation().capture_ok(key9)
    now = L.surface_host_calls()
    L.calc_loss_items(x9, t9, 3, loss_type="dice_err_mc")                        # other metrics do not count
    assert L.surface_host_calls() == now
    tr._validation().note_eager(key3, now)
    assert key3 in tr._validation().seen and tr._validation().capture_ok(key3) and not tr._validation().capture_ok(key9)
    try:
        L.METRICS_KERNEL = False                                                 # everything would go to the host: no capture
        assert not tr._validation().capture_ok(key3)
        tr.accuracy_metric = "dice_err_mc"                                       # (its composite captures)
        assert tr._validation().capture_ok(key3)
    finally:
        L.METRICS_KERNEL = True


def _worker(rank, world, port, q, out_dir):
    dist = init_rank(rank, world, port)
    # unequal validation shards: rank 0 items 0-2, rank 1 items 3-6; both train on the same batches at lr 0, so the weights stay
    tr = _run(os.path.join(out_dir, f"r{rank}"), loaders=_loaders(0 if rank == 0 else 3, 3 if rank == 0 else 4), lr=0.0, val_batch=2,
              data_parallel=True)
    q.put((rank, dict(score=tr.val_score_list)))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_agree(tmp_path):
    """Under data_parallel the names stay per replica and the phase reduction averages them: both ranks hold the scores of one
    process on the whole set, within 4e-5: an item's hd95 on 32x32 is at most 31 sqrt(2) < 44, so a running fp32 sum of seven
    stays below 512, every add rounds by at most half an ulp there (1.53e-5), seven of them move the mean by at most 1.53e-5,
    and the ranks' sums of three and four no more."""
    res = run_ranks(_worker, 2, str(tmp_path))
    assert res[0] == res[1] and len(res[0]["score"]) == 2
    one = _run(tmp_path / "one", lr=0.0, val_batch=2)
    np.testing.assert_allclose(res[0]["score"], one.val_score_list, rtol=0, atol=4e-5)


# ---- C ABI --------------------------------------------------------------------------------------------------------------------

def test_c_abi_refuses_before_any_launch():
    from umi import lib
    BAD, UNS, WS = lib.UMI_ERR_BADARG, lib.UMI_ERR_UNSUPPORTED, lib.UMI_ERR_WORKSPACE
    assert len(lib.STRUCTS) == 5                                                 # no new struct in the header
    buf = (ctypes.c_char * 4096)()                                               # host memory: never dereferenced, nothing is launched
    p = ctypes.addressof(buf)
    p += -p % 16
    dist, score, wsb = (lib.fn(n) for n in ("umi_surface_distances", "umi_surface_scores", "umi_surface_ws_bytes"))
    need = wsb(2, 3, 1, 8, 8)
    assert need > 0 and wsb(2, 9, 1, 8, 8) == 0 and wsb(2, 1, 0, 8, 8) == 0 and wsb(0, 3, 1, 8, 8) == 0 and wsb(1, 2, 1, 4097, 8) == 0
    assert wsb(1, 2, 1, 8, 4097) == 0 and wsb(128, 2, 1, 4096, 4096) == 0 and wsb(1, 2, 1, 4096, 4096) > 0
    assert wsb(2, 3, 3, 8, 8) == 0 and wsb(2, 3, -1, 8, 8) == 0
    # only the scored classes take workspace: 12 bytes per pixel and 64 KiB of histograms per (image, class), plus alignment
    assert wsb(2, 3, 0, 8, 8) > need > wsb(2, 3, 2, 8, 8) and wsb(4, 2, 1, 8, 8) == need
    assert 4 * (12 * 64 + 65536) <= need <= 4 * (12 * 64 + 65536) + 6 * 256 + 4 * 8 * 20
    good = dict(pred=p, target=p + 512, dt=0, B=2, K=3, c0=1, H=8, W=8, stats=p + 1024, counts=p + 2048, ws=p + 3072, ws_bytes=need)

    def call(**kw):
        a = dict(good, **kw)
        return dist(a["pred"], a["target"], a["dt"], a["B"], a["K"], a["c0"], a["H"], a["W"], a["stats"], a["counts"], a["ws"],
                    a["ws_bytes"], None)
    for kw in (dict(pred=None), dict(target=None), dict(stats=None), dict(counts=None), dict(ws=None), dict(B=0), dict(H=0), dict(W=0),
               dict(dt=4), dict(dt=-1), dict(target=p + 516), dict(stats=p + 1028), dict(counts=p + 2052), dict(c0=3), dict(c0=-1)):
        assert call(**kw) == BAD, kw
    for kw in (dict(H=4097), dict(W=4097), dict(K=9), dict(K=1), dict(B=128, K=2, H=4096, W=4096), dict(B=1 << 16, K=2, H=1, W=1)):
        assert call(**kw) == UNS, kw
    assert call(ws_bytes=need - 1) == WS
    ok = (p, 2, 1, 3, 1, 0, 0, 8, 8, p + 512, None)

    def sc(**kw):
        names = ("stats", "items", "n", "K", "c0", "kind", "rule", "H", "W", "out", "stream")
        return score(*[kw.get(n, v) for n, v in zip(names, ok)])
    for kw in (dict(stats=None), dict(out=None), dict(items=0), dict(n=0), dict(kind=3), dict(kind=-1), dict(rule=3), dict(rule=-1),
               dict(c0=3), dict(c0=-1), dict(H=0), dict(stats=p + 4)):
        assert sc(**kw) == BAD, kw
    for kw in (dict(K=1), dict(K=9), dict(H=4097)):
        assert sc(**kw) == UNS, kw
