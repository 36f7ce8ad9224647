"""umi.accum on the MI355X: umi_grad_accum_pre / umi_grad_accum_multi against the NumPy statements bit for bit at ragged and
misaligned rows, an accumulator nobody zeroed, special values, the pass inside replayed graphs, and Trainer(accumulate=k): against
the loop written out, graph against eager, the guard, the device schedule, the weight average, resumption and roll-back, two ranks
on one device, and the small TransUNet."""
import math
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from tests.test_global_batch import init_rank, run_ranks
from tests.test_grad_accum import _same_bits_or_both_nan, _special_grads

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAD = 8                                                    # guard words behind every gradient and every accumulator
SENTINEL = 0x7FC5A5A5                                      # a NaN pattern no pass produces


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")


def _tables():
    from umi import lib
    B = lib.fn("umi_optim_block_elems")()
    assert B == 4096
    g = np.random.default_rng(1)
    return {"ragged": [0, 1, 3, 4, 5, B - 1, B, B + 1, 2 * B + 5], "many_small": [int(n) for n in g.integers(0, 40, 70)]}


OFFSETS = [(0, 0)] + [(k, k) for k in (1, 2, 3)] + [(k, 0) for k in (1, 2, 3)] + [(0, k) for k in (1, 2, 3)] + [(1, 3)]


def _rows(counts, off_g, off_a):
    """Per row: a storage of `off` + n + PAD words filled with SENTINEL, the tensor a view `off` floats (4 * off bytes) into it.
    Returns a GradAccumulator over zero parameters of these lengths whose gradients and accumulators ARE the views, the gradient
    views, the accumulator views and both lists of storages."""
    from umi.accum import GradAccumulator
    gs, accs, sg, sa = [], [], [], []
    for n in counts:
        for off, views, stores in ((off_g, gs, sg), (off_a, accs, sa)):
            st = torch.full((off + n + PAD,), SENTINEL, dtype=torch.int32, device=DEV)
            assert st.data_ptr() % 16 == 0
            view = st.view(torch.float32)[off:off + n]
            assert n == 0 or view.data_ptr() % 16 == 4 * off
            views.append(view)
            stores.append(st)
    params = [torch.zeros(n, device=DEV, requires_grad=True) for n in counts]
    for p, g in zip(params, gs):
        p.grad = g
    acc = GradAccumulator(params, 4)
    acc.accs, acc.arena = list(accs), sa                    # (the accumulator's own arena is aligned to its gradients)
    return acc, gs, accs, sg, sa


def _bits(t):
    t = t.detach().contiguous().reshape(-1)
    return (t.view(torch.int32) if t.element_size() == 4 else t.view(torch.uint8)).cpu().numpy().copy()


def _fill(views, arrays):
    for v, a in zip(views, arrays):
        if a.size:
            v.copy_(torch.from_numpy(a))


def _outside_intact(stores, off, counts):
    for st, n in zip(stores, counts):
        raw = st.cpu().numpy()
        assert np.all(raw[:off] == SENTINEL) and np.all(raw[off + n:] == SENTINEL), "a word outside the row was written"


# ---- kernel level ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("off_g,off_a", OFFSETS, ids=[f"g{4 * a}_a{4 * b}" for a, b in OFFSETS])
@pytest.mark.parametrize("table", ["ragged", "many_small"])
def test_windows_against_numpy(table, off_g, off_a):
    """Windows of 1, 2, 3 and 4 micro-batches, checked after every call."""
    _gpu()
    from umi.accum import ACCUM, accum_state_update_numpy, accumulate_numpy
    counts = _tables()[table]
    acc, gs, accs, sg, sa = _rows(counts, off_g, off_a)
    rng = np.random.default_rng(len(counts) + 16 * off_g + off_a)
    st = np.zeros(8)
    for r in (1, 2, 3, 4):
        seen = []
        for j in range(r):
            grads = [rng.standard_normal(n).astype(np.float32) for n in counts]
            if r == 1:                                     # a NaN payload a move through a float register might quiet
                for g in grads:
                    g.view(np.uint32)[:1] = 0x7FA00001
            _fill(gs, grads)
            seen.append(grads)
            g_before, a_before = [_bits(g) for g in gs], [_bits(a) for a in accs]
            last = j == r - 1
            assert acc.add(last=last) == last
            st = accum_state_update_numpy(st, last)
            torch.cuda.synchronize()
            assert np.array_equal(acc.state.cpu().numpy(), st) and acc.position == st[ACCUM["COUNT"]]
            g_after, a_after = [_bits(g) for g in gs], [_bits(a) for a in accs]
            if not last:                                   # FIRST and ADD: the gradient is only read
                assert all(np.array_equal(u, v) for u, v in zip(g_before, g_after))
                for i in range(len(counts)):
                    run = seen[0][i]
                    for later in seen[1:]:
                        run = run + later[i]
                    assert np.array_equal(a_after[i], run.view(np.int32)), (r, j, i)
            else:                                          # LAST: the accumulator is only read; a window of one touches nothing
                assert all(np.array_equal(u, v) for u, v in zip(a_before, a_after))
                for i in range(len(counts)):
                    want = accumulate_numpy([s[i] for s in seen])
                    assert np.array_equal(g_after[i], want.view(np.int32)), (r, i)
                if r == 1:
                    assert all(np.array_equal(u, v) for u, v in zip(g_before, g_after))
            _outside_intact(sg, off_g, counts)
            _outside_intact(sa, off_a, counts)
    assert acc.read() == dict(count=0, windows=4, micro=10)


@pytest.mark.parametrize("off", [0, 2], ids=["aligned", "offset_8_bytes"])
def test_first_pass_does_not_read_the_accumulator(off):
    """The accumulator preset to 0xFF bytes (NaNs): a window of three on finite gradients gives the finite statement."""
    _gpu()
    from umi.accum import accumulate_numpy
    counts = _tables()["ragged"]
    acc, gs, accs, sg, sa = _rows(counts, off, off)
    for a in accs:
        a.view(torch.int32).fill_(-1)
    rng = np.random.default_rng(3)
    seen = []
    for j in range(3):
        seen.append([rng.standard_normal(n).astype(np.float32) for n in counts])
        _fill(gs, seen[-1])
        acc.add(last=j == 2)
    for i, g in enumerate(gs):
        want = accumulate_numpy([s[i] for s in seen])
        assert np.isfinite(want).all() and np.array_equal(_bits(g), want.view(np.int32))


@pytest.mark.parametrize("off_g,off_a", [(0, 0), (1, 1), (0, 1)], ids=["aligned", "offset_4_bytes", "scalar_walk"])
@pytest.mark.parametrize("r", [2, 3])
def test_special_values_follow_the_float32_statement(r, off_g, off_a):
    """+-0, denormals (not flushed), +-inf, NaN and inf + (-inf), every pair: the bits of the NumPy statement where it gives a
    number, a NaN where it gives a NaN."""
    _gpu()
    from umi.accum import accumulate_numpy
    grads = _special_grads(r, seed=r)
    acc, gs, accs, sg, sa = _rows([grads[0].size], off_g, off_a)
    for j, g in enumerate(grads):
        _fill(gs, [g])
        acc.add(last=j == r - 1)
        if j == 0:                                         # FIRST moves words
            assert np.array_equal(_bits(accs[0]), g.view(np.int32))
    want = accumulate_numpy(grads)
    got = gs[0].cpu().numpy()
    nan = np.isnan(want)
    assert nan.any() and (~nan).any() and _same_bits_or_both_nan(got, want)
    tiny = want[~nan][(want[~nan] != 0) & (np.abs(want[~nan]) < 1.17549435e-38)]
    assert tiny.size                                       # denormal results are in there
    run = grads[0]
    with np.errstate(all="ignore"):
        for g in grads[1:-1]:
            run = run + g
    assert _same_bits_or_both_nan(accs[0].cpu().numpy(), run)                     # LAST left the accumulator alone


def test_replayed_passes():
    """pre(last=0) + multi as one graph, pre(last=1) + multi as another; the sequence 0,0,1, 0,1, 1 replayed with new gradient
    contents written into the same buffers."""
    _gpu()
    from umi.accum import accumulate_numpy
    counts = _tables()["ragged"]
    acc, gs, accs, sg, sa = _rows(counts, 0, 0)
    rng = np.random.default_rng(9)
    _fill(gs, [rng.standard_normal(n).astype(np.float32) for n in counts])
    acc.add(last=False), acc.add(last=True)                # the eager warm-up: every table and the state block exist
    torch.cuda.synchronize()
    graphs = {}
    for last in (False, True):
        graphs[last] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[last]):
            acc.add(last=last)
    acc.reset()
    acc.state.zero_()
    torch.cuda.synchronize()
    seen, closed = [], 0
    for last in (0, 0, 1, 0, 1, 1):
        seen.append([rng.standard_normal(n).astype(np.float32) for n in counts])
        _fill(gs, seen[-1])
        graphs[bool(last)].replay()
        if last:
            torch.cuda.synchronize()
            for i, g in enumerate(gs):
                assert np.array_equal(_bits(g), accumulate_numpy([s[i] for s in seen]).view(np.int32)), (closed, i)
            seen, closed = [], closed + 1
    assert acc.read() == dict(count=0, windows=3, micro=6)
    _outside_intact(sg, 0, counts)
    _outside_intact(sa, 0, counts)
    assert len(acc._tables) == 4                            # eager and captured, micro and final: a table each


# ---- through the Trainer ---------------------------------------------------------------------------------------------------

N_TRAIN = 10                                               # five batches of 2


def _data():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N_TRAIN + 2, 1, 32, 32, generator=g)
    lab = torch.randint(0, 2, (N_TRAIN + 2, 32, 32), generator=g).float()
    return x, lab


def _model(mode="fp32"):
    import Model
    import loss as L
    L.CLASS_NUMBER = 2
    torch.manual_seed(100)
    return Model.UNet(1, 2, 8, False, compute_dtype=mode).to(DEV)


def _train_loader(x, lab):
    return DataLoader(TensorDataset(x[:N_TRAIN], lab[:N_TRAIN]), batch_size=2, shuffle=True, generator=torch.Generator().manual_seed(3))


def _trainer(out_dir, mode="fp32", epochs=2, cut_at=None, inf_at=None, optim="sgd", **kw):
    """UNet(1, 2, 8) at 32 x 32 -- the smallest U-Net of the GPU tests --, ten training images at batch 2, umi.optim.SGD with
    momentum and the poly rule (or AdamW under a cosine rule); two validation images in one batch."""
    from Trainer import Trainer
    from tools import check_resume as C
    from umi import optim as uo
    m = _model(mode)
    x, lab = _data()
    loaders = {"train": C.CutLoader(_train_loader(x, lab), cut_at, inf_at), "val": DataLoader(TensorDataset(x[N_TRAIN:], lab[N_TRAIN:]), batch_size=2)}
    if optim == "sgd":
        opt = uo.SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
        kw.setdefault("lr_scheduler", True)
    else:
        opt = uo.AdamW(uo.decay_groups(m, 1e-2), lr=1e-3)
        kw.setdefault("lr_schedule", dict(kind="cosine", warmup=2))
    os.makedirs(out_dir, exist_ok=True)
    tr = Trainer(m, "single", torch.cuda.FloatTensor, DEV, str(out_dir), loaders, 2, opt, 25, epochs, "dice_bce_mc", "dice_bce_mc", **kw)
    return tr, m, opt


def _last_state(out_dir, m, opt):
    """The state after the last training phase: `last_epoch.pt` (train() loads the best weights at its end) and the momentum."""
    torch.cuda.synchronize()
    sd = torch.load(os.path.join(out_dir, "models", "last_epoch.pt"), map_location="cpu", weights_only=True)
    return list(sd.values()) + [opt.state[p]["momentum_buffer"].cpu() for p in m.parameters()]


@pytest.fixture(scope="module")
def eager_runs(tmp_path_factory):
    """Eager runs of three epochs, k = 2, shared by the cases below and left unchanged: mode -> (lists, state)."""
    _gpu()
    out = {}
    for mode in ("fp32", "fp16"):
        d = tmp_path_factory.mktemp("eager_" + mode)
        tr, m, opt = _trainer(d, mode, epochs=3, accumulate=2)
        tr.train()
        assert tr.iter_num == 9 and not tr._graphs
        out[mode] = (tr.train_loss_list, tr.val_loss_list, _last_state(d, m, opt))
    return out


@pytest.mark.parametrize("k", [2, 3])
def test_eager_trainer_equals_the_loop_written_out(tmp_path, k):
    _gpu()
    from loss import calc_loss
    from umi import optim as uo
    tr, m, opt = _trainer(tmp_path, accumulate=k)
    tr.train()
    got = _last_state(tmp_path, m, opt)
    per_epoch = math.ceil(5 / k)
    assert tr.iter_num == 2 * per_epoch == tr.max_iterations and tr.accumulator.read() == dict(count=0, windows=2 * per_epoch, micro=10)
    # the loop, on a twin from the same seeds
    twin = _model()
    x, lab = _data()
    loader = _train_loader(x, lab)
    topt = uo.SGD(twin.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    it = 0
    twin.train()
    for epoch in range(2):
        batches, kept = list(loader), []
        for i, (xb, yb) in enumerate(batches):
            topt.zero_grad()
            calc_loss(twin(xb.to(DEV)), yb.to(DEV), loss_type="dice_bce_mc").backward()
            kept.append([p.grad.clone() for p in twin.parameters()])
            if len(kept) == k or i == len(batches) - 1:
                for j, p in enumerate(twin.parameters()):
                    total = kept[0][j].clone()
                    for g in kept[1:]:
                        total.add_(g[j])
                    p.grad = total.mul_(1.0 / len(kept))
                topt.step()
                for group in topt.param_groups:
                    group["lr"] = 0.05 * (1.0 - it / tr.max_iterations) ** 0.9
                it += 1
                kept = []
    torch.cuda.synchronize()
    want = [v.cpu() for v in twin.state_dict().values()] + [topt.state[p]["momentum_buffer"].cpu() for p in twin.parameters()]
    assert len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))
    assert opt.param_groups[0]["lr"] == topt.param_groups[0]["lr"]


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_graph_equals_eager_bit_for_bit(tmp_path, eager_runs, mode):
    """Three epochs: the first occurrences run eagerly, the second are captured, the rest are replays; two graphs for the one
    batch shape (the micro-step and the final step)."""
    tr, m, opt = _trainer(tmp_path, mode, epochs=3, accumulate=2, graph=True)
    tr.train()
    assert len(tr._graphs) == 2 and tr.iter_num == 9 and tr.accumulator.read() == dict(count=0, windows=9, micro=15)
    train, val, state = eager_runs[mode]
    assert tr.train_loss_list == train and tr.val_loss_list == val
    got = _last_state(tmp_path, m, opt)
    assert len(got) == len(state) and all(torch.equal(a, b) for a, b in zip(got, state))


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_guard_and_average_over_windows(tmp_path, graph):
    """k = 2, two epochs of five batches stepped by hand; an inf in the input of batch 3, the second micro-batch of the second
    window (under graph=True that window's final step is the capture).  The window's one guarded step skips: parameters, momentum
    and the shadows of the weight average keep their bits; the scale backs off once; the other windows train.  On the clean
    windows the guard's norm is the float64 norm of the mean gradient, within the bar of tests/test_gpu_grad_guard.py (n terms:
    n * 2^-53, plus 2 ulp for the square root and the division)."""
    _gpu()
    tr, m, opt = _trainer(tmp_path, graph=graph, accumulate=2, ema=dict(decay=0.9, warmup=False),
                          grad_guard=dict(max_norm=1.0, dynamic_scale=True, init_scale=2.0 ** 4))
    x, lab = _data()
    m.train()
    params = list(m.parameters())
    n = sum(p.numel() for p in params)
    snap = lambda: [_bits(p) for p in params] + [_bits(opt.state[p]["momentum_buffer"]) for p in params if opt.state[p]] + \
        [_bits(s) for s in tr.ema.shadows]                                                     # noqa: E731
    steps, scale = 0, 16.0
    for epoch in range(2):
        for i in range(5):
            xb = x[2 * i:2 * i + 2].clone()
            planted = (epoch, i) == (0, 3)
            if planted:
                xb[0, 0, 0, 0] = float("inf")
            before = snap() if steps else None
            tr.train_step(xb, lab[2 * i:2 * i + 2], last=True if i == 4 else None)
            torch.cuda.synchronize()
            if i in (0, 2):                                 # a micro-step: nothing but the accumulator moved
                assert tr.iter_num == steps and all(np.array_equal(a, b) for a, b in zip(before or snap(), snap()))
                continue
            steps += 1
            r = tr._guard.read()
            assert tr.iter_num == steps == r["steps"] and tr.ema.sync_host()["updates"] == steps - r["skipped"]
            if planted:
                assert r["skipped"] == 1 and r["nonfinite"] > 0 and r["scale"] == 8.0
                assert all(np.array_equal(a, b) for a, b in zip(before, snap()))
                scale = 8.0
                continue
            assert r["skipped"] == (0 if steps < 2 else 1) and r["scale"] == scale
            assert before is None or any(not np.array_equal(a, b) for a, b in zip(before[:len(params)], snap()[:len(params)]))
            flat = np.concatenate([p.grad.detach().double().cpu().numpy().reshape(-1) for p in params])
            want = math.sqrt(math.fsum(flat * flat)) / scale
            tol = n * 2.0 ** -53 + 2 * 2.0 ** -52
            print("norm", r["norm"], "want", want, "rel", abs(r["norm"] - want) / want, "bar", tol)
            assert flat.size == n and abs(r["norm"] - want) <= tol * want
    assert steps == 6 and len(tr._graphs) == (2 if graph else 0)
    assert all(bool(torch.isfinite(p).all()) for p in params) and all(bool(torch.isfinite(s).all()) for s in tr.ema.shadows)


@pytest.mark.parametrize("k,graph", [(2, True), (3, False)], ids=["k2_graph", "k3_eager"])
def test_device_schedule_counts_optimizer_steps(tmp_path, k, graph):
    """AdamW under lr_schedule=dict(kind='cosine', warmup=2): the block's iteration count, its LR and Adam's step."""
    _gpu()
    from umi import optim as uo
    tr, m, opt = _trainer(tmp_path, optim="adamw", accumulate=k, graph=graph)
    tr.train()
    count = 2 * math.ceil(5 / k)
    assert tr.iter_num == count == tr.max_iterations and len(tr._graphs) == (2 if graph else 0)
    blocks = opt.sync_host()
    assert len(blocks) == 2
    for h, group in zip(blocks, opt.param_groups):
        assert h["iter"] == count and h["adam_t"] == count and h["max_iter"] == count
        assert group["lr"] == uo.schedule_lr(count, 1e-3, "cosine", count, warmup=2)
    assert all(float(v["step"]) == count for v in opt.state_dict()["state"].values())
    assert all(bool(torch.isfinite(p).all()) for p in m.parameters())


def test_cut_and_resumed_run_equals_the_whole_run(tmp_path):
    _gpu()
    from tools import check_resume as C
    kw = dict(epochs=3, graph=True, accumulate=2)
    seed = lambda s: (torch.manual_seed(s), np.random.seed(s))                                 # noqa: E731
    seed(5)
    tr, m, opt = _trainer(tmp_path / "whole", **kw)
    tr.train()
    whole = C.summary(tr, m, opt, tmp_path / "whole")
    seed(5)
    tr, m, opt = _trainer(tmp_path / "cut", cut_at=2, resume=True, **kw)
    with pytest.raises(C.Cut):
        tr.train()
    assert len(tr.train_loss_list) == 1 and tr.iter_num == 3
    # a file of k = 2 (3 steps per epoch) read with k = 3 (2 steps per epoch): the max_iterations check, nothing is modified
    other, _, _ = _trainer(tmp_path / "cut", resume=True, **dict(kw, accumulate=3))
    with pytest.raises(ValueError, match="iterations"):
        other.train()
    assert other.iter_num == 0
    seed(999)
    tr, m, opt = _trainer(tmp_path / "cut", resume=True, **kw)                                 # new objects: everything from the file
    tr.train()
    resumed = C.summary(tr, m, opt, tmp_path / "cut")
    assert tr.iter_num == 9 and C.same(whole, resumed) is None, C.same(whole, resumed)


def test_roll_back_in_place_repeats_the_epoch(tmp_path):
    _gpu()
    tr, m, opt = _trainer(tmp_path, graph=True, accumulate=2)
    x, lab = _data()
    state = lambda: [_bits(p) for p in m.parameters()] + [_bits(b) for b in m.buffers()] + \
        [_bits(opt.state[p]["momentum_buffer"]) for p in m.parameters()]                       # noqa: E731

    def epoch():
        m.train()
        for i in range(5):
            tr.train_step(x[2 * i:2 * i + 2], lab[2 * i:2 * i + 2], last=True if i == 4 else None)
        torch.cuda.synchronize()
        return state()

    epoch(), epoch()
    kept = state()
    tr.snapshot_run_state()
    graphs = dict(tr._graphs)
    first = epoch()
    tr.train_step(x[0:2], lab[0:2])                         # a micro-step opens a window (and moves the BatchNorm statistics)
    assert tr.accumulator.position == 1 and tr.iter_num == 9
    with pytest.raises(RuntimeError, match="open accumulation window"):
        tr.snapshot_run_state()
    tr.restore_run_state()                                  # drops the open window, on the host and in the device block
    torch.cuda.synchronize()
    assert tr.accumulator.position == 0 and tr.accumulator.read()["count"] == 0 and tr.iter_num == 6
    assert all(np.array_equal(a, b) for a, b in zip(kept, state()))
    second = epoch()
    assert all(np.array_equal(a, b) for a, b in zip(first, second)) and any(not np.array_equal(a, b) for a, b in zip(first, kept))
    assert len(graphs) == 2 and all(tr._graphs[k] is graphs[k] for k in graphs) and len(tr._graphs) == 2


# ---- two ranks on one device -----------------------------------------------------------------------------------------------

def _worker(rank, world, port, q, out_dir):
    dist = init_rank(rank, world, port)
    torch.cuda.set_device(0)
    import Model
    import loss as L
    from Trainer import Trainer
    from umi import ddp, optim as uo
    L.CLASS_NUMBER = 2
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda t, *a, **kw: (calls.append(t.numel()), real(t, *a, **kw))[1]
    out = {}
    for name, graph in (("graph", True), ("eager", False)):
        torch.manual_seed(100)
        m = Model.UNet(1, 2, 8, False).to(DEV)
        g = torch.Generator().manual_seed(7)
        x, lab = torch.randn(24, 1, 32, 32, generator=g), torch.randint(0, 2, (24, 32, 32), generator=g).float()
        idx = [4 * b + 2 * rank + j for b in range(5) for j in range(2)]           # five batches of 2 + 2 images per epoch
        val = [20 + 2 * rank, 21 + 2 * rank]
        loaders = {"train": DataLoader(TensorDataset(x[idx], lab[idx]), batch_size=2), "val": DataLoader(TensorDataset(x[val], lab[val]), batch_size=2)}
        opt = uo.SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
        tr = Trainer(m, "single", torch.cuda.FloatTensor, DEV, os.path.join(out_dir, name), loaders, 2, opt, 25, 2, "dice_bce_mc",
                     "dice_bce_mc", lr_scheduler=True, graph=graph, data_parallel=dict(bucket_mb=0.05), accumulate=2)
        verified, buckets = [], []
        begin, verify = tr._dp.begin, tr._dp.verify
        tr._dp.begin = lambda: (begin(), buckets.append(len(tr._dp.reducer.buckets)))
        tr._dp.verify = lambda: (verify(), verified.append(tr._dp.check))           # raises on every rank if the replicas differ
        del calls[:]
        tr.train()
        torch.cuda.synchronize()
        out[name] = dict(weights=[p.detach().cpu().numpy() for p in m.parameters()], val=tr.val_loss_list, train=tr.train_loss_list,
                         graphs=len(tr._graphs), iters=tr.iter_num, calls=list(calls), buckets=buckets[0], verified=list(verified),
                         word=ddp.fingerprint(list(m.parameters())), windows=tr.accumulator.read()["windows"])
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_one_set_of_collectives_per_window(tmp_path):
    _gpu()
    res = run_ranks(_worker, 2, str(tmp_path))
    for name in ("graph", "eager"):
        a, b = res[0][name], res[1][name]
        assert a["graphs"] == b["graphs"] == (2 if name == "graph" else 0) and a["iters"] == b["iters"] == 6 == a["windows"]
        assert a["word"] == b["word"] and a["val"] == b["val"] and a["train"] == b["train"]
        assert all(np.array_equal(u.view(np.uint8), v.view(np.uint8)) for u, v in zip(a["weights"], b["weights"]))
        assert a["buckets"] > 1
        for r in (a, b):
            assert r["verified"] == [True] * 3               # after the broadcast and after each training phase
            grads = [n for n in r["calls"] if n > 5]         # (the Trainer's per-phase reduction carries five doubles)
            assert len(grads) == r["buckets"] * r["iters"] and len(r["calls"]) - len(grads) == 4
    for u, v in zip(res[0]["graph"]["weights"], res[0]["eager"]["weights"]):
        np.testing.assert_allclose(u, v, rtol=1e-6, atol=1e-7)                       # (the bar of the data-parallel Trainer tests)


# ---- the small TransUNet ---------------------------------------------------------------------------------------------------

def _transunet_run(out_dir, graph):
    import loss as L
    from oracle import ref_transunet
    from tests.test_gpu_transunet import product_config
    from Trainer import Trainer
    from TransUnet.vit_seg_modeling import VisionTransformer
    from umi import optim as uo
    L.CLASS_NUMBER = 2
    torch.manual_seed(100)
    np.random.seed(100)
    m = VisionTransformer(product_config(ref_transunet.small_config(2), 64), img_size=64, num_classes=2, compute_dtype="fp16").to(DEV)
    g = torch.Generator().manual_seed(7)
    x, lab = torch.randn(10, 1, 64, 64, generator=g), torch.randint(0, 2, (10, 64, 64), generator=g).float()
    loaders = {"train": DataLoader(TensorDataset(x[:8], lab[:8]), batch_size=2), "val": DataLoader(TensorDataset(x[8:], lab[8:]), batch_size=2)}
    opt = uo.AdamW(uo.decay_groups(m, 1e-2), lr=1e-3)
    os.makedirs(out_dir, exist_ok=True)
    tr = Trainer(m, "TransUnet", torch.cuda.FloatTensor, DEV, str(out_dir), loaders, 2, opt, 25, 3, "dice_bce_mc", "dice_bce_mc",
                 graph=graph, lr_schedule=dict(kind="cosine", warmup=2), accumulate=2)
    tr.train()
    torch.cuda.synchronize()
    sd = torch.load(os.path.join(out_dir, "models", "last_epoch.pt"), map_location="cpu", weights_only=True)
    moments = [v.cpu() for p in m.parameters() for k, v in sorted(opt.state[p].items()) if k != "step"]
    assert tr.iter_num == 6 and len(tr._graphs) == (2 if graph else 0)
    return tr.train_loss_list, tr.val_loss_list, list(sd.values()) + moments, [bytes(h.tobytes()) for h in opt.sync_host()]


def test_transunet_fp16_adamw_graph_equals_eager(tmp_path):
    """The small TransUNet of the GPU tests, fp16, AdamW on the device cosine rule, accumulate=2: three epochs of four batches."""
    _gpu()
    eager = _transunet_run(tmp_path / "eager", False)
    graph = _transunet_run(tmp_path / "graph", True)
    assert eager[0] == graph[0] and eager[1] == graph[1] and eager[3] == graph[3]
    assert len(eager[2]) == len(graph[2]) and all(torch.equal(a, b) for a, b in zip(eager[2], graph[2]))
    assert all(bool(torch.isfinite(t).all()) for t in graph[2])
