"""Gradient accumulation on the CPU: the entry points' argument checks, `accumulate_numpy` against torch's own accumulation rule,
the state machine of umi_grad_accum_pre, and Trainer(accumulate=k) on the CPU oracle -- windows, counters, learning-rate rules,
the meaning of the mean, off is off, refusals, an early close, and two gloo ranks."""
import math
import os

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from tests.test_global_batch import init_rank, run_ranks

EPOCHS = 2


# ---- the header and the entry points ---------------------------------------------------------------------------------------

def test_enum_comes_from_the_header_and_bad_arguments_are_refused():
    import ctypes
    from umi import accum, lib
    assert lib.UMI_ACCUM_LEN == 8 == accum.ACCUM_LEN
    assert accum.ACCUM == dict(COUNT=0, FIRST=1, LAST=2, SCALE=3, WINDOWS=4, MICRO=5, SPARE0=6, SPARE1=7)
    for name in ("umi_grad_accum_pre", "umi_grad_accum_multi"):
        assert name in lib.SIGNATURES
    # nothing below reaches a launch: no GPU is touched
    block = (ctypes.c_double * 10)()
    state = ctypes.addressof(block)
    assert state % 8 == 0
    table = ctypes.addressof((ctypes.c_char * 48)())
    pre, multi = lib.fn("umi_grad_accum_pre"), lib.fn("umi_grad_accum_multi")
    assert pre(None, 0, None) == lib.UMI_ERR_BADARG
    assert pre(state + 4, 1, None) == lib.UMI_ERR_BADARG                                  # a block of doubles, 4 bytes off
    assert multi(None, 1, 1, state, None) == lib.UMI_ERR_BADARG                           # no table, one row
    assert multi(table, 1, 1, None, None) == lib.UMI_ERR_BADARG                           # no state block
    assert multi(table, 1, 1, state + 4, None) == lib.UMI_ERR_BADARG
    assert multi(table, -1, 0, state, None) == lib.UMI_ERR_BADARG
    assert multi(table, 0, -1, state, None) == lib.UMI_ERR_BADARG
    assert multi(None, 0, 0, None, None) == lib.UMI_ERR_BADARG                            # an empty table still needs its block
    assert multi(None, 0, 0, state, None) == lib.UMI_OK                                   # an empty table: nothing to launch
    assert not any(block)


# ---- the statements --------------------------------------------------------------------------------------------------------

SPECIAL = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 1.17549435e-38, np.inf, -np.inf, np.nan, 1.0, -1.0, 3.4028235e38,
                    -3.4028235e38, 1e-30, 0.1, 1 / 3, 7.0], dtype=np.float32)


def _special_grads(r, seed):
    """r gradients: every pair of SPECIAL in the first two (inf + (-inf) among them), the rest drawn from SPECIAL and normals."""
    g = np.random.default_rng(seed)
    n = SPECIAL.size ** 2
    grads = [np.repeat(SPECIAL, SPECIAL.size), np.tile(SPECIAL, SPECIAL.size)][:r]
    while len(grads) < r:
        pick = g.integers(0, SPECIAL.size, n)
        grads.append(np.where(g.random(n) < 0.5, SPECIAL[pick], g.standard_normal(n).astype(np.float32)).astype(np.float32))
    return grads


def _same_bits_or_both_nan(a, b):
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


@pytest.mark.parametrize("r", [1, 2, 3, 4, 7])
def test_statement_is_torch_s_accumulation_rule(r):
    """Cloned fp32 gradients added in order, then mul_(1.0 / r), on the CPU: the same bits (a NaN where torch has a NaN)."""
    from umi.accum import accumulate_numpy
    grads = _special_grads(r, seed=r)
    got = accumulate_numpy(grads)
    acc = torch.from_numpy(grads[0]).clone()
    for g in grads[1:]:
        acc.add_(torch.from_numpy(g).clone())
    acc.mul_(1.0 / r)
    want = acc.numpy()
    assert got.dtype == np.float32 and _same_bits_or_both_nan(got, want)
    nan = np.isnan(want)
    assert (~nan).any() and (nan.any() or r == 1)                    # inf + (-inf) and NaN inputs are in there
    if r == 1:                                                      # the input's bits, NaN payloads included
        odd = grads[0].copy()
        odd.view(np.uint32)[:3] = [0x7FC5A5A5, 0xFFA00001, 0x00000001]
        assert np.array_equal(accumulate_numpy([odd]).view(np.uint32), odd.view(np.uint32))
        assert accumulate_numpy([odd]) is not odd
    with pytest.raises(ValueError):
        accumulate_numpy(grads, r + 1)
    # denormals are kept, not flushed
    tiny = np.full(4, 1e-45, dtype=np.float32)
    assert np.array_equal(accumulate_numpy([tiny, tiny]), np.full(4, 1e-45, dtype=np.float32))        # (2 * 2^-149) / 2


def test_state_machine():
    """umi_grad_accum_pre restated: COUNT, FIRST, LAST, SCALE, WINDOWS and MICRO after each call of last = 0,0,1, 0,1, 1, 0,0,0,1."""
    from umi.accum import ACCUM, ACCUM_LEN, accum_state_update_numpy
    st = np.zeros(ACCUM_LEN)
    seq = [0, 0, 1, 0, 1, 1, 0, 0, 0, 1]
    want = [  # COUNT, FIRST, SCALE (of 1 / r), WINDOWS
        (1, 1, 1, 0), (2, 0, 2, 0), (0, 0, 3, 1), (1, 1, 1, 1), (0, 0, 2, 2), (0, 1, 1, 3), (1, 1, 1, 3), (2, 0, 2, 3), (3, 0, 3, 3),
        (0, 0, 4, 4)]
    for i, (last, (count, first, r, windows)) in enumerate(zip(seq, want)):
        before = st.copy()
        st = accum_state_update_numpy(st, last)
        assert st is not before and st[ACCUM["COUNT"]] == count and st[ACCUM["FIRST"]] == first and st[ACCUM["LAST"]] == last
        assert st[ACCUM["SCALE"]] == float(np.float32(1.0 / r)) and st[ACCUM["WINDOWS"]] == windows and st[ACCUM["MICRO"]] == i + 1
        assert st[ACCUM["SPARE0"]] == st[ACCUM["SPARE1"]] == 0
    assert float(np.float32(1.0 / 3)) != 1.0 / 3                     # SCALE is the fp32 factor, carried as a double


def test_accumulator_cpu_follows_the_statement():
    from umi.accum import GradAccumulator, accumulate_numpy
    torch.manual_seed(2)
    m = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Linear(7, 3))
    m[1].bias.requires_grad_(False)
    acc = GradAccumulator(m, 3)
    assert len(acc.params) == 3 and acc.position == 0 and acc.read() == dict(count=0, windows=0, micro=0)
    for window in (3, 3, 1, 2):
        seen = []
        for j in range(window):
            m.zero_grad()
            m(torch.randn(4, 5)).square().sum().backward()
            seen.append([p.grad.numpy().copy() for p in acc.params])
            closed = acc.add(last=True if (window, j) in ((1, 0), (2, 1)) else None)
            assert closed == (j == window - 1) and acc.position == (0 if closed else j + 1)
            if not closed:                                          # g is not written by FIRST and ADD
                assert all(np.array_equal(p.grad.numpy(), g) for p, g in zip(acc.params, seen[-1]))
        for i, p in enumerate(acc.params):
            assert np.array_equal(p.grad.numpy(), accumulate_numpy([s[i] for s in seen]))
    assert acc.read() == dict(count=0, windows=4, micro=9)
    # the set of parameters with a gradient must not change inside a window; reset() drops an open window
    m.zero_grad()
    m(torch.randn(4, 5)).sum().backward()
    acc.add()
    m[0].bias.grad = None
    with pytest.raises(RuntimeError, match="changed inside a window"):
        acc.add()
    assert acc.position == 1 and acc.reset().position == 0 and acc.read()["count"] == 0
    for bad in (0, -1, True, 2.0):
        with pytest.raises(ValueError):
            GradAccumulator(m, bad)


# ---- Trainer(accumulate=k) on the CPU oracle -------------------------------------------------------------------------------

def _data():
    g = torch.Generator().manual_seed(7)
    return torch.randn(12, 1, 16, 16, generator=g), torch.randint(0, 2, (12, 16, 16), generator=g).float()


def _model():
    import loss as L
    from oracle import ref_unet
    L.CLASS_NUMBER = 2
    torch.manual_seed(100)
    return ref_unet.RefUNet(1, 2, 4, False)


def _trainer(out_dir, epochs=EPOCHS, **kw):
    """RefUNet(1, 2, 4) at 16 x 16 (the model of the Trainer's CPU tests), ten training images = five batches of 2 in the loader's
    own shuffled order, two validation images, torch.optim.SGD with momentum."""
    from Trainer import Trainer
    m = _model()
    x, lab = _data()
    train = DataLoader(TensorDataset(x[:10], lab[:10]), batch_size=2, shuffle=True, generator=torch.Generator().manual_seed(3))
    loaders = {"train": train, "val": DataLoader(TensorDataset(x[10:], lab[10:]), batch_size=2)}
    opt = torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    kw.setdefault("lr_scheduler", True)
    tr = Trainer(m, "single", torch.FloatTensor, "cpu", str(out_dir), loaders, 2, opt, 25, epochs, "dice_bce_mc", "dice_bce_mc", **kw)
    return tr, m, opt


def _state(m, opt):
    return ([p.detach().clone() for p in m.parameters()] + [b.detach().clone() for b in m.buffers()] +
            [opt.state[p]["momentum_buffer"].clone() for p in m.parameters()])


def _by_hand(k, rule):
    """The run of _trainer(accumulate=k) written out: torch's own accumulation rule (clone, add in order, mul_(1 / r)) and the
    learning-rate rule on the optimizer-step count.  Returns (state, LR of every step, LR after each epoch)."""
    from loss import calc_loss
    from umi.optim import schedule_lr
    m = _model()
    x, lab = _data()
    train = DataLoader(TensorDataset(x[:10], lab[:10]), batch_size=2, shuffle=True, generator=torch.Generator().manual_seed(3))
    opt = torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    per_epoch = math.ceil(5 / k)
    max_it, it, lrs, after = EPOCHS * per_epoch, 0, [], []
    m.train()
    for epoch in range(EPOCHS):
        batches, kept = list(train), []
        for i, (xb, yb) in enumerate(batches):
            opt.zero_grad()
            calc_loss(m(xb), yb, loss_type="dice_bce_mc").backward()
            kept.append([p.grad.clone() for p in m.parameters()])
            if len(kept) == k or i == len(batches) - 1:
                for j, p in enumerate(m.parameters()):
                    total = kept[0][j].clone()
                    for g in kept[1:]:
                        total.add_(g[j])
                    p.grad = total.mul_(1.0 / len(kept))
                if rule == "cosine":
                    for group in opt.param_groups:
                        group["lr"] = schedule_lr(it, 0.05, "cosine", max_it, warmup=2)
                lrs.append(opt.param_groups[0]["lr"])
                opt.step()
                if rule == "poly":
                    for group in opt.param_groups:
                        group["lr"] = 0.05 * (1.0 - it / max_it) ** 0.9
                it += 1
                kept = []
        after.append(opt.param_groups[0]["lr"])
        m.eval()                                                    # (the validation phase changes no state)
        m.train()
    return _state(m, opt), lrs, after, it, max_it


@pytest.mark.parametrize("rule", ["poly", "cosine"])
@pytest.mark.parametrize("k", [2, 3])
def test_trainer_windows_and_counters(tmp_path, k, rule):
    """5 batches of 2: windows 2, 2, 1 (k = 2) and 3, 2 (k = 3), two epochs."""
    kw = dict(lr_scheduler=True) if rule == "poly" else dict(lr_scheduler=None, lr_schedule=dict(kind="cosine", warmup=2))
    tr, m, opt = _trainer(tmp_path, accumulate=k, **kw)
    assert tr.accumulator is None and tr.max_iterations == EPOCHS * math.ceil(5 / k)
    after = []
    finish = tr._log_guard                                          # called once per epoch, after the training phase
    tr._log_guard = lambda say, epoch: (after.append(opt.param_groups[0]["lr"]), finish(say, epoch))
    tr.train()
    want, lrs, want_after, it, max_it = _by_hand(k, rule)
    assert tr.iter_num == it == EPOCHS * math.ceil(5 / k) and tr.max_iterations == max_it
    assert after == want_after and len(tr.train_loss_list) == EPOCHS
    log = open(tmp_path / "logs.txt").read()
    assert log.count("Gradient accumulation: %i micro-batches per optimizer step, %i optimizer steps per epoch\n"
                     % (k, math.ceil(5 / k))) == 1
    assert tr.accumulator.read() == dict(count=0, windows=it, micro=10) and tr.accumulator.position == 0


@pytest.mark.parametrize("k", [2, 3])
def test_trainer_equals_the_loop_written_out(tmp_path, k):
    """Parameters, BatchNorm buffers and momentum buffers of the LAST training state (train() loads the best weights at its end, so
    the state is read after the last training phase)."""
    tr, m, opt = _trainer(tmp_path, accumulate=k)
    got = []
    finish = tr._log_guard
    tr._log_guard = lambda say, epoch: (got.append(_state(m, opt)), finish(say, epoch))
    tr.train()
    want = _by_hand(k, "poly")[0]
    assert len(got) == EPOCHS and len(got[-1]) == len(want)
    assert all(torch.equal(a, b) for a, b in zip(got[-1], want))


class _GN(torch.nn.Module):
    """conv + GroupNorm + conv: no batch statistics, so two halves of a batch are the batch."""

    def __init__(self):
        super().__init__()
        self.a, self.n, self.b = torch.nn.Conv2d(1, 8, 3, padding=1), torch.nn.GroupNorm(2, 8), torch.nn.Conv2d(8, 2, 3, padding=1)

    def forward(self, x):
        return self.b(torch.relu(self.n(self.a(x))))


def test_the_mean_of_two_halves_is_the_whole_batch(tmp_path):
    """float64, loss 'CE', plain SGD: one step with accumulate=2 over the halves of a batch of 4 against one step on the batch.  The
    two differ in summation order only (about 1e4 terms x 2^-53); a wrong factor is off by O(1)."""
    import loss as L
    from Trainer import Trainer
    L.CLASS_NUMBER = 2
    g = torch.Generator().manual_seed(11)
    x, lab = torch.randn(4, 1, 16, 16, generator=g, dtype=torch.float64), torch.randint(0, 2, (4, 16, 16), generator=g).double()
    out = []
    for k, bs in ((2, 2), (None, 4)):
        torch.manual_seed(4)
        m = _GN().double()
        loaders = {"train": DataLoader(TensorDataset(x, lab), batch_size=bs), "val": DataLoader(TensorDataset(x, lab), batch_size=4)}
        opt = torch.optim.SGD(m.parameters(), lr=0.1)
        tr = Trainer(m, "single", torch.DoubleTensor, "cpu", str(tmp_path / str(k)), loaders, bs, opt, 25, 1, "CE", "CE", accumulate=k)
        m.train()
        start = [p.detach().clone() for p in m.parameters()]
        for xb, yb in loaders["train"]:
            tr.train_step(xb, yb)
        assert tr.iter_num == 1
        out.append([p.detach().clone() for p in m.parameters()])
        assert all(not torch.equal(a, b) for a, b in zip(start, out[-1]))
    for a, b, s in zip(out[0], out[1], start):
        assert (a - b).norm() <= 1e-9 * b.norm(), ((a - b).norm() / b.norm()).item()
        assert (a - b).norm() <= 1e-6 * (b - s).norm()              # of the update itself, too


def test_off_is_off(tmp_path):
    runs = []
    for name, kw in (("plain", {}), ("none", dict(accumulate=None)), ("one", dict(accumulate=1))):
        tr, m, opt = _trainer(tmp_path / name, **kw)
        tr.train()
        assert tr.accumulator is None and tr.iter_num == 10 == tr.max_iterations
        runs.append((_state(m, opt), tr.train_loss_list, tr.val_loss_list, opt.param_groups[0]["lr"],
                     open(tmp_path / name / "logs.txt").read().replace("\r", "")))
        assert "accumulation" not in runs[-1][4]
    for other in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0][0], other[0])) and runs[0][1:4] == other[1:4]


def test_refusals(tmp_path):
    from Trainer import Trainer

    class Never:
        generator = None

        def __len__(self):
            return 1

        def __iter__(self):
            raise AssertionError("a step ran")

    m = _model()
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    loaders = {"train": Never(), "val": Never()}
    args = (m, "single", torch.FloatTensor, "cpu", str(tmp_path), loaders, 1, opt, 1, 1, "dice_bce_mc", "dice_bce_mc")
    for bad in (0, -1, True, 2.5):
        with pytest.raises(ValueError, match="accumulate"):
            Trainer(*args, accumulate=bad)
    tr = Trainer(m, "multi_task", torch.FloatTensor, "cpu", str(tmp_path), loaders, 1, opt, 1, 1, "multi_task_loss_ratio", "mse",
                 accumulate=2)
    with pytest.raises(NotImplementedError, match="multi_task_loss_ratio"):
        tr.train()
    tr = Trainer(*args, accumulate=2, data_parallel=dict(global_batch=True))
    with pytest.raises(NotImplementedError, match="global_batch"):
        tr.train()
    with pytest.raises(TypeError):                                    # keyword-only: the positionals stay the reference's
        Trainer(*args, None, 1, 2)


def test_early_close_and_open_window_snapshot(tmp_path):
    """train_step(..., last=True) closes a window early and the next call opens a new one; snapshot_run_state() is refused while a
    window is open."""
    tr, m, opt = _trainer(tmp_path, accumulate=3)
    x, lab = _data()
    m.train()
    batch = lambda i: (x[2 * i:2 * i + 2], lab[2 * i:2 * i + 2])
    start = [p.detach().clone() for p in m.parameters()]
    tr.train_step(*batch(0))
    assert tr.iter_num == 0 and tr.accumulator.position == 1 and all(torch.equal(a, p) for a, p in zip(start, m.parameters()))
    with pytest.raises(RuntimeError, match="open accumulation window"):
        tr.snapshot_run_state()
    tr.train_step(*batch(1), last=True)                             # a window of two
    assert tr.iter_num == 1 and tr.accumulator.position == 0 and not any(torch.equal(a, p) for a, p in zip(start, m.parameters()))
    tr.snapshot_run_state()
    mid = [p.detach().clone() for p in m.parameters()]
    for i in (2, 3):                                                # a new window of three opens
        tr.train_step(*batch(i))
        assert tr.iter_num == 1 and tr.accumulator.position == i - 1 and all(torch.equal(a, p) for a, p in zip(mid, m.parameters()))
    tr.restore_run_state()                                          # drops the open window
    assert tr.accumulator.position == 0 and tr.accumulator.read()["count"] == 0
    for i in (2, 3, 4):
        tr.train_step(*batch(i))
    assert tr.iter_num == 2 and tr.accumulator.position == 0
    assert tr.accumulator.read() == dict(count=0, windows=2, micro=7)
    # the same two windows by hand
    from loss import calc_loss
    twin = _model()
    topt = torch.optim.SGD(twin.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    twin.train()
    for window in ((0, 1), (2, 3, 4)):
        kept = []
        for i in window:
            topt.zero_grad()
            calc_loss(twin(batch(i)[0]), batch(i)[1], loss_type="dice_bce_mc").backward()
            kept.append([p.grad.clone() for p in twin.parameters()])
        for j, p in enumerate(twin.parameters()):
            total = kept[0][j].clone()
            for g in kept[1:]:
                total.add_(g[j])
            p.grad = total.mul_(1.0 / len(kept))
        topt.step()
        for group in topt.param_groups:
            group["lr"] = 0.05 * (1.0 - (0 if window == (0, 1) else 1) / tr.max_iterations) ** 0.9
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), twin.parameters()))


# ---- two gloo ranks ----------------------------------------------------------------------------------------------------------

def _worker(rank, world, port, q, out_dir):
    dist = init_rank(rank, world, port)
    import loss as L
    from Trainer import Trainer
    from oracle import ref_unet
    L.CLASS_NUMBER = 2
    calls = []
    real = dist.all_reduce
    dist.all_reduce = lambda t, *a, **kw: (calls.append(t.numel()), real(t, *a, **kw))[1]
    out = {}
    for k in (1, 2):
        torch.manual_seed(100 + rank)                               # the reducer broadcasts rank 0's replica
        m = ref_unet.RefUNet(1, 2, 4, False)
        g = torch.Generator().manual_seed(7)
        x, lab = torch.randn(20, 1, 16, 16, generator=g), torch.randint(0, 2, (20, 16, 16), generator=g).float()
        idx = [4 * b + 2 * rank + j for b in range(4) for j in range(2)]           # four batches of 2 per rank
        val = [16 + 2 * rank, 17 + 2 * rank]
        loaders = {"train": DataLoader(TensorDataset(x[idx], lab[idx]), batch_size=2), "val": DataLoader(TensorDataset(x[val], lab[val]), batch_size=2)}
        opt = torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9)
        tr = Trainer(m, "single", torch.FloatTensor, "cpu", os.path.join(out_dir, str(k)), loaders, 2, opt, 25, EPOCHS, "dice_bce_mc",
                     "dice_bce_mc", lr_scheduler=True, data_parallel=dict(bucket_mb=0.002), accumulate=k)
        buckets = []
        begin = tr._dp.begin
        tr._dp.begin = lambda: (begin(), buckets.append(len(tr._dp.reducer.buckets)))
        del calls[:]
        tr.train()
        out[k] = dict(calls=list(calls), buckets=buckets[0], iters=tr.iter_num,
                      weights=[p.detach().numpy().copy() for p in m.parameters()], val=tr.val_loss_list)
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_two_gloo_ranks_one_set_of_collectives_per_window(tmp_path):
    res = run_ranks(_worker, 2, str(tmp_path))
    for k in (1, 2):
        a, b = res[0][k], res[1][k]
        assert a["iters"] == b["iters"] == EPOCHS * 4 // k and a["val"] == b["val"]
        assert all(np.array_equal(u, v) for u, v in zip(a["weights"], b["weights"]))              # the replicas stay equal
        nb = a["buckets"]
        assert nb > 1
        phases = 2 * EPOCHS                                         # the Trainer's own reduction of each phase's sums
        for r in (a, b):
            assert len(r["calls"]) == nb * r["iters"] + phases
    assert len(res[0][2]["calls"]) - 2 * EPOCHS == (len(res[0][1]["calls"]) - 2 * EPOCHS) // 2    # half the gradient traffic
    assert any(not np.array_equal(u, v) for u, v in zip(res[0][1]["weights"], res[0][2]["weights"]))
