"""Global-batch statistics under data parallel (umi.ddp.GradReducer(global_batch=True)), the parts that need no GPU:
the composite global 'dice_bce_mc' between two gloo ranks, the refusals, the seed screen that makes the two-rank GPU
test's inputs provably discriminating, and the new C entry points.

Every multi-process test gives init_process_group and q.get a timeout and terminates its workers on failure: a mismatched
collective fails the test instead of hanging it."""
import datetime
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import ref_unet

TIMEOUT = 120


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def run_ranks(worker, world, *args):
    """Start `world` processes of worker(rank, world, port, q, *args); returns {rank: payload}.  A worker that raises reports
    ("error", text), which fails the test; whatever happens, no worker outlives the call."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=guarded, args=(worker, r, world, port, q, *args)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=TIMEOUT) for _ in range(world))
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0, p.exitcode
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
            p.join(timeout=10)
    for r, v in res.items():
        assert not (isinstance(v, tuple) and v and v[0] == "error"), (r, v)
    return res


def init_rank(rank, world, port):
    import sys
    import torch.distributed as dist
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [repo, os.path.join(repo, "unet-torch_amd")]
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=TIMEOUT))
    torch.set_num_threads(2)
    return dist


def guarded(fn, rank, world, port, q, *args):
    """Process entry: runs the worker body and reports an exception through the queue instead of dying silently."""
    import traceback
    try:
        fn(rank, world, port, q, *args)
    except BaseException:                                  # noqa: BLE001 -- reported to the parent, which fails the test
        q.put((rank, ("error", traceback.format_exc())))


def _loss_case(C, seed=3):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(4, C, 9, 7, generator=g, dtype=torch.float64)
    t = torch.randint(0, C, (4, 9, 7), generator=g).float()
    return x, t


def _loss_worker(rank, world, port, q):
    dist = init_rank(rank, world, port)
    import loss as L
    from umi import ddp
    red = ddp.GradReducer(torch.nn.Conv2d(1, 1, 1), world, global_batch=True)
    out = {}
    for C in (2, 4):
        L.CLASS_NUMBER = C
        x, t = _loss_case(C)
        xs = x[rank * 2:(rank + 1) * 2].clone().requires_grad_(True)
        loss = L.calc_loss(xs, t[rank * 2:(rank + 1) * 2], loss_type="dice_bce_mc")
        loss.backward()
        out[C] = (loss.item(), xs.grad.numpy())
    # refusals between two ranks: unequal shards (2 + 1 images), and a statistics collective in deferred (graph-replayed) mode
    L.CLASS_NUMBER = 2
    x, t = _loss_case(2)
    n = 2 - rank
    try:
        L.calc_loss(x[:n], t[:n], loss_type="dice_bce_mc")
        out["unequal"] = "no error"
    except RuntimeError as e:
        out["unequal"] = str(e)
    red.deferred = True
    try:
        red.batch_sync.all_reduce(torch.zeros(3, dtype=torch.float64))
        out["deferred"] = "no error"
    except RuntimeError as e:
        out["deferred"] = str(e)
    red.deferred = False
    red.close()
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_global_dice_bce_mc_between_two_gloo_ranks_is_the_one_process_loss():
    """Composite global loss in float64 on 2 + 2 images, C in {2, 4}: the value on every rank and the averaged logit gradients
    (each rank's gradient / world, side by side) equal the one-process loss and gradient on the 4 images to 1e-12; unequal
    shards and a collective in deferred mode raise on both ranks."""
    import loss as L
    res = run_ranks(_loss_worker, 2)
    for C in (2, 4):
        L.CLASS_NUMBER = C
        x, t = _loss_case(C)
        x.requires_grad_(True)
        want = L.calc_loss(x, t, loss_type="dice_bce_mc")
        want.backward()
        got = np.concatenate([res[0][C][1], res[1][C][1]]) / 2
        for r in (0, 1):
            assert abs(res[r][C][0] - want.item()) <= 1e-12 * abs(want.item()), (C, r)
        np.testing.assert_allclose(got, x.grad.numpy(), rtol=0, atol=1e-12 * float(x.grad.abs().max()))
        assert float(x.grad.abs().max()) > 1e-4              # (the comparison is not of zeros)
    L.CLASS_NUMBER = 2
    for r in (0, 1):
        assert "equal shards" in res[r]["unequal"], res[r]["unequal"]
        assert "deferred" in res[r]["deferred"], res[r]["deferred"]


def test_group_of_one_is_legal_and_batch_coupled_losses_refuse():
    """World size 1 needs no process group (no collective is launched); under the switch 'Tversky', 'TopK' and 'BCE_HEM' raise
    NotImplementedError instead of silently staying per-replica, and work again once the reducer is closed."""
    import loss as L
    from umi import ddp
    m = torch.nn.Conv2d(1, 1, 1)
    assert not torch.distributed.is_initialized()
    pred, tgt = torch.randn(2, 1, 8, 8), (torch.rand(2, 1, 8, 8) > 0.5).float()
    off = ddp.GradReducer(m, 1)
    assert ddp.active_batch_sync() is None and not hasattr(m, "_umi_batch_sync")        # off by default
    L.calc_loss(pred, tgt, loss_type="Tversky")
    off.close()
    red = ddp.GradReducer(m, 1, global_batch=True)
    try:
        assert ddp.active_batch_sync() is red.batch_sync is m._umi_batch_sync
        for name in ("Tversky", "TopK", "BCE_HEM"):
            with pytest.raises(NotImplementedError, match="global_batch"):
                L.calc_loss(pred, tgt, loss_type=name)
        L.CLASS_NUMBER = 2
        x, t = _loss_case(2)
        x.requires_grad_(True)
        a = L.calc_loss(x, t, loss_type="dice_bce_mc")
        a.backward()
        ga = x.grad.clone()
        red.deferred = True                                   # a group of one launches no collective: nothing to refuse
        red.batch_sync.all_reduce(torch.zeros(3, dtype=torch.float64))
    finally:
        red.close()
    assert ddp.active_batch_sync() is None and not hasattr(m, "_umi_batch_sync") and not hasattr(m, "_umi_grad_sink")
    x.grad = None
    b = L.calc_loss(x, t, loss_type="dice_bce_mc")
    b.backward()
    assert abs(a.item() - b.item()) <= 1e-14 and float((ga - x.grad).abs().max()) <= 1e-15
    L.calc_loss(pred, tgt, loss_type="Tversky")


# ---- seed screen -------------------------------------------------------------------------------------------------------

def screen_inputs(S=32):
    """Model seed 100, data generator seed 7, 4 images: the seeds and shapes of tests/test_gpu_ddp.py."""
    torch.manual_seed(100)
    ref = ref_unet.RefUNet(1, 2, 8, False)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(4, 1, S, S, generator=g)
    lab = torch.randint(0, 2, (4, S, S), generator=g).float()
    return ref, x, lab


def oracle_step(state, x, lab, dtype, shards):
    """Training-mode logits, loss-averaged gradients and running statistics of the oracle in `dtype`, the batch cut into
    `shards` equal parts that each normalise and lose on their own (1 = the global batch)."""
    n = x.shape[0] // shards
    logits, grads, stats = [], None, None
    for r in range(shards):
        m = ref_unet.RefUNet(1, 2, 8, False).to(dtype)
        m.load_state_dict(state)
        m.train()
        out = m(x[r * n:(r + 1) * n].to(dtype))
        ref_unet.dice_bce_mc(out, lab[r * n:(r + 1) * n], 2).backward()
        logits.append(out.detach())
        gr = [p.grad.double() / shards for p in m.parameters()]
        grads = gr if grads is None else [a + b for a, b in zip(grads, gr)]
        if r == 0:
            stats = {k: v.double().clone() for k, v in m.state_dict().items() if "running_" in k}
    return torch.cat(logits).double(), grads, stats


def rel_l2(a, b):
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def test_seed_screen_per_replica_statistics_miss_the_fp32_bars_tenfold():
    """The gap the switch closes, recomputed from the oracle in float64: per-replica (2 + 2) against global statistics moves the
    training-mode logits by >= 10 x the 1e-4 bar and >= 56 of the 64 averaged gradient tensors by > 10 x the 2e-3 bar (relative
    L2, the metric of tests/test_gpu_unet.py), while the oracle's own fp32 vs fp64 on the global batch is inside both bars: no
    ReLU near-tie in these seeds, so the two-rank GPU test discriminates."""
    ref, x, lab = screen_inputs()
    state = {k: v.double() for k, v in ref.state_dict().items()}
    gl, gg, gs = oracle_step(state, x, lab, torch.float64, 1)
    sl, sg, ss = oracle_step(state, x, lab, torch.float64, 2)
    assert len(gg) == 64
    logit_gap = ((sl - gl).abs().max() / gl.abs().max()).item()
    gaps = [rel_l2(a, b) for a, b in zip(sg, gg)]
    stat_gap = max(((ss[k] - gs[k]).abs().max() / (gs[k].abs().max() + 1e-30)).item() for k in gs)
    fl, fg, _ = oracle_step(state, x, lab, torch.float32, 1)
    f_logit = ((fl - gl).abs().max() / gl.abs().max()).item()
    f_grad = max(rel_l2(a, b) for a, b in zip(fg, gg))
    print(f"per-replica vs global: logits {logit_gap:.3g} of scale, {sum(g > 2e-2 for g in gaps)} of 64 gradients past 2e-2, "
          f"median {float(np.median(gaps)):.3g}, running statistics {stat_gap:.3g}; fp32 vs fp64: logits {f_logit:.3g}, worst "
          f"gradient {f_grad:.3g}")
    assert logit_gap >= 10 * 1e-4
    assert sum(g > 10 * 2e-3 for g in gaps) >= 56
    assert stat_gap > 10 * 1e-5
    assert f_logit < 1e-4 and f_grad < 2e-3


# ---- C ABI ---------------------------------------------------------------------------------------------------------------

NEW_SYMBOLS = ("umi_bn_stat_sums", "umi_bn_finalize_sums", "umi_bn_bwd_apply_count", "umi_conv_wgrad_bnapply_count",
               "umi_dice_ce_sums", "umi_dice_ce_finalize", "umi_dice_ce_bwd_global")


def test_new_entry_points_are_declared_exported_and_reject_bad_arguments():
    """Declared in unetmi.h, exported by the library, and UMI_ERR_BADARG on nulls / non-positive sizes before any launch (no
    GPU is touched here)."""
    import ctypes
    from umi import build, lib
    cdll = ctypes.CDLL(build.LIB)
    for n in NEW_SYMBOLS:
        assert n in lib.SIGNATURES and hasattr(cdll, n), n
    bad = lib.UMI_ERR_BADARG
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)                                        # a non-null address that is never dereferenced
    f = lib.fn
    assert f("umi_bn_stat_sums")(None, 4, 8, p, None) == bad
    assert f("umi_bn_stat_sums")(p, 4, 8, None, None) == bad
    assert f("umi_bn_stat_sums")(p, 0, 8, p, None) == bad
    assert f("umi_bn_stat_sums")(p, 4, 0, p, None) == bad
    assert f("umi_bn_finalize_sums")(None, 8, 4.0, None, None, 1e-5, 0.1, None, None, p, None, None) == bad
    assert f("umi_bn_finalize_sums")(p, 8, 4.0, None, None, 1e-5, 0.1, None, None, None, None, None) == bad
    assert f("umi_bn_finalize_sums")(p, 0, 4.0, None, None, 1e-5, 0.1, None, None, p, None, None) == bad
    assert f("umi_bn_finalize_sums")(p, 8, 0.0, None, None, 1e-5, 0.1, None, None, p, None, None) == bad
    assert f("umi_bn_finalize_sums")(p, 8, float("nan"), None, None, 1e-5, 0.1, None, None, p, None, None) == bad
    for args in ((None, 8, p, 8, p, p, p, p, 4, 4, 8), (p, 8, p, 8, p, p, None, p, 4, 4, 8), (p, 8, p, 8, p, p, p, None, 4, 4, 8),
                 (p, 8, p, 8, p, p, p, p, 0, 4, 8), (p, 8, p, 8, p, p, p, p, 4, 0, 8), (p, 8, p, 8, p, p, p, p, 4, -1, 8),
                 (p, 8, p, 8, p, p, p, p, 4, 4, 0)):
        assert f("umi_bn_bwd_apply_count")(*args, lib.UMI_F16, None) == bad, args
    wg = [p, 8, None, p, 8, p + 64, 8, p, p, p, p, p + 128, 8, p, 72, 9, 1, 1.0, 1, 4, 4, 8, 8, 3, 3, 1, 1, lib.UMI_F16, 0, 16, p, 256, None]
    for i, v in ((0, None), (3, None), (9, None), (10, None), (13, None), (18, 0), (29, 0), (29, -5), (30, None)):
        a = list(wg)
        a[i] = v
        assert f("umi_conv_wgrad_bnapply_count")(*a) == bad, i
    assert f("umi_dice_ce_sums")(None, p, 0, 1, 2, 16, p, p, 256, None) == bad
    assert f("umi_dice_ce_sums")(p, p, 0, 1, 2, 16, None, p, 256, None) == bad
    assert f("umi_dice_ce_sums")(p, p, 0, 0, 2, 16, p, p, 256, None) == bad
    assert f("umi_dice_ce_sums")(p, p, 0, 1, 2, 0, p, p, 256, None) == bad
    assert f("umi_dice_ce_finalize")(None, 2, 16.0, p, None) == bad
    assert f("umi_dice_ce_finalize")(p, 2, 16.0, None, None) == bad
    assert f("umi_dice_ce_finalize")(p, 2, 0.0, p, None) == bad
    assert f("umi_dice_ce_bwd_global")(None, p, 0, p, None, 1.0, 16.0, 1, 2, 16, p, None) == bad
    assert f("umi_dice_ce_bwd_global")(p, p, 0, p, None, 0.0, 16.0, 1, 2, 16, p, None) == bad
    assert f("umi_dice_ce_bwd_global")(p, p, 0, p, None, 1.0, 0.0, 1, 2, 16, p, None) == bad
    assert f("umi_dice_ce_bwd_global")(p, p, 0, p, None, 1.0, 16.0, 1, 2, 16, None, None) == bad
