"""umi.ema on the MI355X: umi_ema_pre / umi_ema_multi / umi_ema_swap_multi against the NumPy statements bit for bit at ragged
and misaligned rows, special values, the guard's SKIP word, the update inside a replayed graph, Trainer(ema=...) validating and
saving the averaged weights, resumption and roll-back, and two ranks on one device."""
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from tests.test_global_batch import init_rank, run_ranks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 8                                                    # guard words behind every parameter and every shadow
SENTINEL = 0x7FC5A5A5                                      # a NaN pattern no update produces


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")


def _block():
    from umi import lib
    return lib.fn("umi_optim_block_elems")()


def _tables():
    B = _block()
    return {"ragged": [1, 3, 4, 5, B - 1, B, B + 1, 2 * B + 5], "many_small": [7] * 64}


OFFSETS = [(0, 0)] + [(k, 0) for k in (1, 2, 3)] + [(0, k) for k in (1, 2, 3)] + [(k, k) for k in (1, 2, 3)]   # in floats: 4, 8, 12 B


def _rows(counts, off_p, off_e, seed=0, values=None):
    """Per row: a storage of `off` + n + PAD words filled with SENTINEL, the tensor a view `off` floats (4 * off bytes) into it.
    Returns (parameter views, shadow views, parameter storages, shadow storages) on the device, and the host values."""
    g = np.random.default_rng(seed)
    ps, es, sp, se, host = [], [], [], [], []
    for i, n in enumerate(counts):
        pv = g.standard_normal(n).astype(np.float32) if values is None else values[0][i]
        ev = g.standard_normal(n).astype(np.float32) if values is None else values[1][i]
        for off, val, views, stores in ((off_p, pv, ps, sp), (off_e, ev, es, se)):
            st = torch.full((off + n + PAD,), SENTINEL, dtype=torch.int32, device=DEV)
            assert st.data_ptr() % 16 == 0
            view = st.view(torch.float32)[off:off + n]
            view.copy_(torch.from_numpy(val))
            assert view.data_ptr() % 16 == 4 * off
            views.append(view)
            stores.append(st)
        host.append((pv, ev))
    return ps, es, sp, se, host


def _ema(ps, es, **kw):
    """A ModelEMA over the views `ps` whose shadows ARE the views `es` (the constructor's own copies are aligned)."""
    from umi.ema import ModelEMA
    ema = ModelEMA([p.requires_grad_(True) for p in ps], **kw)
    ema.shadows = list(es)
    return ema


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _outside_intact(stores, offs, counts):
    for st, n in zip(stores, counts):
        raw = st.cpu().numpy()
        assert np.all(raw[:offs] == SENTINEL) and np.all(raw[offs + n:] == SENTINEL), "a word outside the row was written"


@pytest.mark.parametrize("off_p,off_e", OFFSETS, ids=[f"p{4 * a}_e{4 * b}" for a, b in OFFSETS])
@pytest.mark.parametrize("table", ["ragged", "many_small"])
def test_update_and_swap_against_numpy(table, off_p, off_e):
    _gpu()
    from umi.ema import EMA, ema_state_update_numpy, ema_update_numpy
    counts = _tables()[table]
    ps, es, sp, se, host = _rows(counts, off_p, off_e, seed=len(counts))
    ema = _ema(ps, es, decay=0.999, warmup=True)
    st = ema.state.cpu().numpy()
    want = [e for _, e in host]
    p_before = [s.clone() for s in sp]
    for step in range(1, 13):                               # the warm-up moves w_f at every one of them
        ema.update()
        st = ema_state_update_numpy(st, False)
        want = [ema_update_numpy(e, p, st[EMA["WEIGHT"]]) for e, (p, _) in zip(want, host)]
        if step in (1, 12):
            torch.cuda.synchronize()
            assert np.array_equal(ema.state.cpu().numpy(), st)
            for e_dev, e_np in zip(es, want):
                assert torch.equal(e_dev.cpu(), torch.from_numpy(e_np))
            assert all(torch.equal(a, b) for a, b in zip(sp, p_before))            # p and its surroundings: only read
            _outside_intact(se, off_e, counts)
    assert st[EMA["UPDATES"]] == 12 and st[EMA["LAST"]] == 12.0 / 21.0
    # swap: the words change places, exactly n per row; versions move; update() is refused; two swaps restore
    pb, eb = [_bits(p) for p in ps], [_bits(e) for e in es]
    versions = [p._version for p in ema.params]
    ema.swap()
    assert ema.swapped and all(p._version > v for p, v in zip(ema.params, versions))
    assert all(np.array_equal(_bits(p), b) for p, b in zip(ps, eb)) and all(np.array_equal(_bits(e), b) for e, b in zip(es, pb))
    _outside_intact(sp, off_p, counts)
    _outside_intact(se, off_e, counts)
    with pytest.raises(RuntimeError, match="swapped"):
        ema.update()
    assert np.array_equal(ema.state.cpu().numpy(), st)                             # (the refused update launched nothing)
    ema.swap()
    assert not ema.swapped
    assert all(np.array_equal(_bits(p), b) for p, b in zip(ps, pb)) and all(np.array_equal(_bits(e), b) for e, b in zip(es, eb))
    _outside_intact(sp, off_p, counts)
    _outside_intact(se, off_e, counts)


@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "offset_4_bytes"])
def test_special_values_follow_the_float32_statement(off):
    """+-0, denormals, +-inf, NaN and the largest finite value in p and in e, every pair: the bits of the NumPy statement where it
    gives a number, a NaN where it gives a NaN."""
    _gpu()
    from umi.ema import EMA, ema_update_numpy
    tiny = np.float32(1e-45)
    vals = np.array([0.0, -0.0, tiny, -tiny, 1e-39, -1e-39, 1.17549435e-38, np.inf, -np.inf, np.nan, 1.0, -1.0, 3.4028235e38,
                     -3.4028235e38, 1e-30, 0.1], dtype=np.float32)
    p, e = np.repeat(vals, len(vals)), np.tile(vals, len(vals))
    ps, es, sp, se, _ = _rows([p.size], off, off, values=([p], [e]))
    ema = _ema(ps, es, decay=0.999, warmup=True)            # first update: d_t = 0.1, w_f = float32(0.9)
    ema.update()
    w = ema.sync_host()["weight"]
    assert w == float(np.float32(0.9))
    want = ema_update_numpy(e, p, w)
    got = es[0].cpu().numpy()
    nan = np.isnan(want)
    assert nan.any() and (~nan).any() and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    assert np.array_equal(_bits(ps[0]), p.view(np.int32))
    # the swap moves words: NaN payloads and denormals keep their bits
    ema.swap()
    assert np.array_equal(_bits(es[0]), p.view(np.int32)) and np.array_equal(_bits(ps[0]), got.view(np.int32))


def test_a_skipped_step_leaves_the_average_alone():
    _gpu()
    from umi.ema import EMA, ema_state_update_numpy, ema_update_numpy
    from umi.optim import GUARD, GradGuard
    counts = _tables()["ragged"]
    ps, es, sp, se, host = _rows(counts, 0, 1, seed=5)
    guard = GradGuard()
    block = guard._device_state()
    ema = _ema(ps, es, decay=0.999, warmup=True, guard=guard)
    ema.update()
    st1 = ema.state.cpu().numpy()
    assert st1[EMA["UPDATES"]] == 1 and st1[EMA["ACTIVE"]] == 1
    e1 = [_bits(e) for e in es]
    block[GUARD["SKIP"]] = 1.0
    ema.update()
    st2 = ema.state.cpu().numpy()
    keep = [i for i in range(len(st1)) if i != EMA["ACTIVE"]]
    assert st2[EMA["ACTIVE"]] == 0 and np.array_equal(st2[keep].view(np.int64), st1[keep].view(np.int64))
    assert all(np.array_equal(_bits(e), b) for e, b in zip(es, e1))
    _outside_intact(se, 1, counts)
    block[GUARD["SKIP"]] = 0.0
    ema.update()                                            # t was not advanced by the skipped step
    st3 = ema_state_update_numpy(st1, False)
    assert np.array_equal(ema.state.cpu().numpy(), st3) and st3[EMA["UPDATES"]] == 2 and st3[EMA["LAST"]] == 2.0 / 11.0
    for e_dev, b, (p, _) in zip(es, e1, host):
        assert np.array_equal(e_dev.cpu().numpy(), ema_update_numpy(b.view(np.float32), p, st3[EMA["WEIGHT"]]))


# ---- through the Trainer ---------------------------------------------------------------------------------------------------

EMA_KW = dict(decay=0.9, warmup=False)


def _data(n_val=2):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(4 + n_val, 1, 32, 32, generator=g)
    lab = torch.randint(0, 2, (4 + n_val, 32, 32), generator=g).float()
    return x, lab


def _trainer(out_dir, mode="fp32", epochs=2, cut_at=None, val_items=False, **kw):
    """UNet(1, 2, 8) at 32 x 32 -- the smallest U-Net of the GPU tests --, four training images at batch 2, umi.optim.SGD with
    momentum and the poly rule; two validation images in one batch, or (`val_items`) four of them one by one."""
    import Model
    import loss as L
    from Trainer import Trainer
    from tools import check_resume as C
    from umi import optim as uo
    L.CLASS_NUMBER = 2
    torch.manual_seed(100)
    m = Model.UNet(1, 2, 8, False, compute_dtype=mode).to(DEV)
    x, lab = _data(4 if val_items else 2)
    train = DataLoader(TensorDataset(x[:4], lab[:4]), batch_size=2, shuffle=True, generator=torch.Generator().manual_seed(3))
    loaders = {"train": C.CutLoader(train, cut_at), "val": DataLoader(TensorDataset(x[4:], lab[4:]), batch_size=1 if val_items else 2)}
    opt = uo.SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    tr = Trainer(m, "single", torch.cuda.FloatTensor, DEV, str(out_dir), loaders, 2, opt, 25, epochs, "dice_bce_mc", "dice_bce_mc",
                 lr_scheduler=True, **kw)
    return tr, m, opt


def _five_steps(tmp_path, name, graph, nan_at=None, **kw):
    tr, m, opt = _trainer(tmp_path / name, graph=graph, ema=dict(decay=0.99, warmup=True), **kw)
    x, lab = _data()
    m.train()
    shadows = []
    for i in range(5):
        xb = x[2 * (i % 2):2 * (i % 2) + 2].clone()
        if i == nan_at:
            xb[0, 0, 0, 0] = float("nan")                  # a value, not a fault: every gradient of the step is NaN
        tr.train_step(xb, lab[2 * (i % 2):2 * (i % 2) + 2])
        torch.cuda.synchronize()
        shadows.append([_bits(s) for s in tr.ema.shadows])
    return tr, m, shadows


@pytest.mark.parametrize("guarded", [False, True], ids=["plain", "grad_guard"])
def test_update_inside_a_replayed_graph(tmp_path, guarded):
    """The eager first step, the capture and four replays against five eager steps of an identically seeded twin."""
    _gpu()
    from umi.ema import EMA
    kw = dict(grad_guard=dict(max_norm=1.0), nan_at=2) if guarded else {}
    tg, mg, sg = _five_steps(tmp_path, "graph", True, **kw)
    te, me, se = _five_steps(tmp_path, "eager", False, **kw)
    assert len(tg._graphs) == 1 and not te._graphs
    for a, b in zip(tg.ema.shadows, te.ema.shadows):
        assert torch.equal(a, b)
    assert all(torch.equal(a, b) for a, b in zip(mg.parameters(), me.parameters()))
    st = tg.ema.state.cpu().numpy()
    assert np.array_equal(st, te.ema.state.cpu().numpy())
    assert st[EMA["UPDATES"]] == (4 if guarded else 5) and st[EMA["ACTIVE"]] == 1
    moved = [any(not np.array_equal(a, b) for a, b in zip(sg[i], sg[i - 1])) for i in range(1, 5)]
    if guarded:                                             # the planted step (a replay) left every shadow bit alone
        assert moved == [True, False, True, True] and tg._guard.read()["skipped"] == 1
    else:
        assert moved == [True] * 4
    assert not any(torch.isnan(s).any() for s in tg.ema.shadows)


def _files(out):
    d = os.path.join(out, "models")
    return {n: torch.load(os.path.join(d, n), map_location="cpu", weights_only=True) for n in sorted(os.listdir(d))}


def _validating_run(out, **kw):
    """Two epochs with ema validating; every swap() is recorded: the parameters' bits before and after it."""
    tr, m, opt = _trainer(out, val_items=True, ema=dict(EMA_KW), **kw)
    tr._attach_ema()
    swaps, swap = [], tr.ema.swap

    def recorded():
        before = [_bits(p) for p in m.parameters()]
        shadows = [_bits(s) for s in tr.ema.shadows]
        swap()
        swaps.append((before, shadows, [_bits(p) for p in m.parameters()]))
    tr.ema.swap = recorded
    tr.train()
    torch.cuda.synchronize()
    return tr, m, swaps


@pytest.fixture(scope="module")
def eager_items(tmp_path_factory):
    _gpu()
    out = tmp_path_factory.mktemp("eager_items")
    tr, m, swaps = _validating_run(out, graph=False)
    return dict(val=tr.val_loss_list, score=tr.val_score_list, train=tr.train_loss_list, files=_files(out))


@pytest.mark.parametrize("async_ckpt", [False, True], ids=["sync", "async"])
def test_trainer_validates_on_the_averaged_weights(tmp_path, eager_items, async_ckpt):
    _gpu()
    tr, m, swaps = _validating_run(tmp_path, graph=True, val_batch=2, async_checkpoints=async_ckpt)
    assert len(tr._graphs) == 1 and len(tr._validation().graphs) == 1 and len(swaps) == 4 and not tr.ema.swapped
    assert tr.val_loss_list == eager_items["val"] and tr.val_score_list == eager_items["score"]
    assert tr.train_loss_list == eager_items["train"] and len(tr.val_loss_list) == 2
    names = [n for n, _ in m.named_parameters()]
    for ep in (0, 1):
        (live, shadows, swapped_in), (_, _, back) = swaps[2 * ep], swaps[2 * ep + 1]
        assert all(np.array_equal(a, b) for a, b in zip(swapped_in, shadows))      # validation ran on the average ...
        assert all(np.array_equal(a, b) for a, b in zip(back, live))               # ... and the live weights came back, bit for bit
        assert any(not np.array_equal(a, b) for a, b in zip(live, shadows))
    files = _files(tmp_path)
    saved = sorted(int(n[5:-3]) for n in files if n.startswith("epoch"))
    assert saved and {"best.pt", "last_epoch.pt"} <= set(files)
    best_shadows = swaps[2 * (saved[-1] - 1)][1]
    for n, b in zip(names, best_shadows):                                          # what was validated is what was saved
        assert np.array_equal(files["best.pt"][n].numpy().view(np.int32).reshape(-1), b.reshape(-1)), n
    for n, b in zip(names, swaps[2][0]):                                           # last_epoch.pt: the live weights
        assert np.array_equal(files["last_epoch.pt"][n].numpy().view(np.int32).reshape(-1), b.reshape(-1)), n
    assert list(files) == list(eager_items["files"])
    for f in files:                                                                # the files of the eager, synchronous run
        assert list(files[f]) == list(eager_items["files"][f])
        assert all(torch.equal(files[f][k], eager_items["files"][f][k]) for k in files[f]), f
    for n, p in m.named_parameters():                                              # train() returns the best averaged weights
        assert torch.equal(p.detach().cpu(), files["best.pt"][n])
    log = open(tmp_path / "logs.txt").read()
    assert "EMA on epoch 1: decay 0.9, updates 2\n" in log and "EMA on epoch 2: decay 0.9, updates 4\n" in log


def test_fp16_pack_cache_picks_the_swapped_weights_up(tmp_path):
    _gpu()
    import Model
    tr, m, opt = _trainer(tmp_path, mode="fp16", ema=dict(EMA_KW))
    x, lab = _data()
    m.train()
    for i in range(3):
        tr.train_step(x[2 * (i % 2):2 * (i % 2) + 2], lab[2 * (i % 2):2 * (i % 2) + 2])
    m.eval()
    xv = x[4:].to(DEV)
    with torch.no_grad():
        live = m(xv).clone()                                # packs the live weights
        live_sd = {k: v.clone() for k, v in m.state_dict().items()}
        averaged = tr.ema.state_dict()
        tr.ema.swap()
        swapped = m(xv).clone()
        fresh = Model.UNet(1, 2, 8, False, compute_dtype="fp16").to(DEV).eval()
        fresh.load_state_dict(live_sd)                      # the live BatchNorm statistics ...
        res = fresh.load_state_dict(averaged, strict=False)                        # ... under the averaged parameters
        assert res.unexpected_keys == ["_ema_state"]
        assert torch.equal(swapped, fresh(xv)) and not torch.equal(swapped, live)
        tr.ema.swap()
        assert torch.equal(m(xv), live)


def _summary(tr, m, opt, out):
    from tools import check_resume as C
    s = C.summary(tr, m, opt, out)
    s["ema"] = [t.detach().cpu().clone() for t in tr.ema.tensors().values()]
    return s


def test_cut_and_resumed_run_equals_the_whole_run(tmp_path):
    _gpu()
    from tools import check_resume as C
    kw = dict(mode="fp16", epochs=3, graph=True, ema=dict(EMA_KW))
    C_seed = lambda s: (torch.manual_seed(s), np.random.seed(s))
    C_seed(5)
    tr, m, opt = _trainer(tmp_path / "whole", **kw)
    tr.train()
    whole = _summary(tr, m, opt, tmp_path / "whole")
    C_seed(5)
    tr, m, opt = _trainer(tmp_path / "cut", cut_at=2, resume=True, **kw)
    with pytest.raises(C.Cut):
        tr.train()
    assert len(tr.train_loss_list) == 1
    C_seed(999)
    tr, m, opt = _trainer(tmp_path / "cut", resume=True, **kw)                      # new objects: everything from the file
    tr.train()
    resumed = _summary(tr, m, opt, tmp_path / "cut")
    assert C.same(whole, resumed) is None, C.same(whole, resumed)
    assert len(whole["ema"]) == len(resumed["ema"]) and all(C._eq(a, b) for a, b in zip(whole["ema"], resumed["ema"]))
    assert whole["ema"][-1][2] == 6                                                 # UPDATES: two steps, three epochs


def test_roll_back_in_place_carries_the_average(tmp_path):
    _gpu()
    tr, m, opt = _trainer(tmp_path, graph=True, ema=dict(EMA_KW))
    x, lab = _data()
    batches = [(x[0:2], lab[0:2]), (x[2:4], lab[2:4])]

    def epoch():
        m.train()
        for b in batches:
            tr.train_step(*b)
        torch.cuda.synchronize()
        return [_bits(t) for t in tr.ema.tensors().values()]

    epoch(), epoch()
    kept = [_bits(t) for t in tr.ema.tensors().values()]
    snap = tr.snapshot_run_state()
    assert [k for k in snap.names if k.startswith("ema.")] == ["ema." + k for k in tr.ema.tensors()]
    graphs = dict(tr._graphs)
    first = epoch()
    tr.restore_run_state()
    torch.cuda.synchronize()
    assert all(np.array_equal(a, _bits(t)) for a, t in zip(kept, tr.ema.tensors().values()))
    second = epoch()
    assert all(np.array_equal(a, b) for a, b in zip(first, second)) and any(not np.array_equal(a, b) for a, b in zip(first, kept))
    assert len(graphs) == 1 and all(tr._graphs[k] is graphs[k] for k in graphs) and len(tr._graphs) == 1


# ---- two ranks on one device -----------------------------------------------------------------------------------------------

def _worker(rank, world, port, q, out_dir):
    dist = init_rank(rank, world, port)
    torch.cuda.set_device(0)
    import Model
    import loss as L
    from Trainer import Trainer
    from umi import ddp, optim as uo
    L.CLASS_NUMBER = 2
    out = {}
    for name, graph in (("graph", True), ("eager", False)):
        torch.manual_seed(100)
        m = Model.UNet(1, 2, 8, False).to(DEV)
        g = torch.Generator().manual_seed(7)
        x, lab = torch.randn(16, 1, 32, 32, generator=g), torch.randint(0, 2, (16, 32, 32), generator=g).float()
        idx = [4 * k + 2 * rank + j for k in range(3) for j in range(2)]           # three steps of 2 + 2 images per epoch
        val = [12 + 2 * rank, 13 + 2 * rank]
        loaders = {"train": DataLoader(TensorDataset(x[idx], lab[idx]), batch_size=2), "val": DataLoader(TensorDataset(x[val], lab[val]), batch_size=2)}
        opt = uo.SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
        tr = Trainer(m, "single", torch.cuda.FloatTensor, DEV, os.path.join(out_dir, name), loaders, 2, opt, 25, 2, "dice_bce_mc",
                     "dice_bce_mc", lr_scheduler=True, graph=graph, data_parallel=dict(bucket_mb=0.05), ema=dict(EMA_KW))
        tr.train()
        torch.cuda.synchronize()
        tensors = list(tr.ema.tensors().values())
        out[name] = dict(shadows=[t.cpu().numpy() for t in tensors], val=tr.val_loss_list, replayed=bool(tr._graphs),
                         word=ddp.fingerprint(list(m.parameters()) + tensors), updates=tr.ema.sync_host()["updates"])
    # the replica word covers the shadows: one ulp in one shadow of rank 1 and the Trainer's check raises on both ranks
    tr._dp.reducer, tr._dp.check = ddp.GradReducer(m, bucket_mb=0.05), True
    tr._dp.verify()
    if rank == 1:
        tr.ema.shadows[3].view(-1)[-1:].view(torch.int32).add_(1)
    try:
        tr._dp.verify()
        out["differ"] = "no error"
    except RuntimeError as e:
        out["differ"] = str(e)
    tr._dp.reducer.close()
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_keep_identical_averages(tmp_path):
    _gpu()
    res = run_ranks(_worker, 2, str(tmp_path))
    for name in ("graph", "eager"):
        a, b = res[0][name], res[1][name]
        assert a["replayed"] == b["replayed"] == (name == "graph") and a["updates"] == b["updates"] == 6
        assert len(a["shadows"]) == len(b["shadows"]) and a["word"] == b["word"] and a["val"] == b["val"]
        for u, v in zip(a["shadows"], b["shadows"]):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
    for r in (0, 1):
        assert "replicas differ" in res[r]["differ"], res[r]["differ"]
