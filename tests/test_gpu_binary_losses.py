"""'dice_bce', 'Tversky', 'TopK' and 'BCE_HEM' on the MI355X (csrc/binary_losses.hip): device loss and gradient against the
reference (tests/golden/binary_losses.npz) and float64 NumPy at the benchmark's size, the exact selected sets of TopK and
BCE_HEM including the lowest-index tie rule, determinism, argument checks, the composite fallback, and graph-replayed Trainer
steps (child process: stream capture is sensitive to what ran before it in the process)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_FN = {"dice_bce": "_DiceBCE", "Tversky": "_Tversky", "TopK": "_TopKBCE", "BCE_HEM": "_TopKBCE"}


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    import loss as L
    return L


def _run(L, x, t, loss_type, device_path=True):
    """(loss, d loss / d pred) through calc_loss on the device; asserts which path ran."""
    x = x.detach().to(DEV).clone().contiguous().requires_grad_(True)
    t = t.to(DEV).contiguous()
    v = L.calc_loss(x, t, loss_type=loss_type)
    took = type(v.grad_fn).__name__.startswith(DEVICE_FN[loss_type])
    assert took == device_path, (loss_type, type(v.grad_fn).__name__)
    v.backward()
    torch.cuda.synchronize()
    return v.detach().cpu(), x.grad.cpu()


def test_device_losses_match_the_reference_fixtures():
    L = _gpu()
    g = np.load(os.path.join(REPO, "tests", "golden", "binary_losses.npz"))
    for e in (str(s) for s in g["entries"]):
        c, lt = e.split(":")
        loss, grad = _run(L, torch.from_numpy(g[f"{c}_pred"]), torch.from_numpy(g[f"{c}_target"]), lt)
        want = float(g[f"{e}_loss"])
        assert abs(loss.item() - want) <= 2e-6 * abs(want), (e, loss.item(), want)
        gw = g[f"{e}_grad"]
        assert np.abs(grad.numpy() - gw).max() <= 1e-5 * np.abs(gw).max(), e
        if lt in ("TopK", "BCE_HEM"):
            assert np.array_equal(np.flatnonzero(grad.numpy()), np.flatnonzero(gw)), e


def _smooth(gen, B, H, W, scale=9.0):
    n = torch.randn(B, 1, H + 8, W + 8, generator=gen)
    return F.avg_pool2d(n, 9, stride=1) * scale


@pytest.fixture(scope="module")
def full_size():
    gen = torch.Generator().manual_seed(11)
    B, H, W = 16, 512, 512
    x = _smooth(gen, B, H, W)
    t = (_smooth(gen, B, H, W) > 0.5).float()[:, 0]
    t[2] = 0.0
    t[9] = 1.0
    return x, t


def _np_sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _np_bce(x, t):
    return (1.0 - t) * x - (np.minimum(x, 0.0) - np.log1p(np.exp(-np.abs(x))))


def test_full_size_dice_bce_and_tversky_against_float64(full_size):
    L = _gpu()
    x, t = full_size
    xd, td = x.double().numpy()[:, 0], t.double().numpy()
    s = _np_sigmoid(xd)
    B = xd.shape[0]
    num = 2 * (s * td).reshape(B, -1).sum(1) + 1
    den = (np.abs(s) + np.abs(td)).reshape(B, -1).sum(1) + 1
    want = {"dice_bce": 0.5 * _np_bce(xd, td).mean() + 0.5 * (1 - num / den).mean()}
    tp, fp, fn = (s * td).sum(), ((1 - td) * s).sum(), (td * (1 - s)).sum()
    want["Tversky"] = 1 - (tp + 1) / (tp + 0.4 * fp + 0.6 * fn + 1)
    for lt, w in want.items():
        loss, grad = _run(L, x, t, lt)
        assert abs(loss.item() - w) <= 1e-6 * abs(w), (lt, loss.item(), w)
        xc = x.clone().requires_grad_(True)
        L.calc_loss(xc, t, loss_type=lt).backward()                 # the CPU composite
        assert (grad - xc.grad).abs().max() <= 1e-5 * xc.grad.abs().max(), lt


def _selected(grad):
    return np.flatnonzero(grad.numpy().reshape(-1))


def test_full_size_topk_selects_the_stable_argsort_set(full_size):
    L = _gpu()
    x, t = full_size
    N = x.numel()
    k = N // 2
    xd, td = x.to(DEV), t.to(DEV)
    p = torch.sigmoid(xd).reshape(-1)
    key = torch.where(td.reshape(-1).long() == 1, p, 1 - p).cpu().numpy()
    want = np.sort(np.argsort(key, kind="stable")[:k])
    loss, grad = _run(L, x, t, "TopK")
    assert np.array_equal(_selected(grad), want)
    w = _np_bce(x.double().numpy().reshape(-1), t.double().numpy().reshape(-1))[want].mean()
    assert abs(loss.item() - w) <= 1e-6 * w, (loss.item(), w)


def test_full_size_bce_hem_selects_500_at_the_threshold(full_size):
    L = _gpu()
    x, t = full_size
    key = F.binary_cross_entropy_with_logits(x.to(DEV)[:, 0], t.to(DEV), reduction="none").reshape(-1).cpu().numpy()
    ref = np.argsort(-key.astype(np.float64), kind="stable")[:500]
    loss, grad = _run(L, x, t, "BCE_HEM")
    got = _selected(grad)
    assert got.size == 500
    thr = key[ref[-1]]
    diff = np.setxor1d(got, ref)
    ulp = np.abs(key[diff].view(np.int32).astype(np.int64) - np.int64(np.float32(thr).view(np.int32)))
    assert (ulp <= 2).all(), (diff.size, ulp.max() if diff.size else 0)
    w = _np_bce(x.double().numpy().reshape(-1), t.double().numpy().reshape(-1))[got].mean()
    assert abs(loss.item() - w) <= 1e-6 * w, (loss.item(), w)


@pytest.mark.parametrize("shape", [(16, 1, 512, 512), (3, 1, 37, 53)])
def test_ties_take_the_lowest_flat_indices(shape):
    """All-zero logits: every TopK key is 0.5 and every BCE is log 2, so the first k flat indices are taken."""
    L = _gpu()
    B, _, H, W = shape
    x = torch.zeros(shape)
    t = (torch.rand(B, H, W, generator=torch.Generator().manual_seed(5)) < 0.5).float()
    N = x.numel()
    for lt, k in (("TopK", N // 2), ("BCE_HEM", 500)):
        loss, grad = _run(L, x, t, lt)
        assert np.array_equal(_selected(grad), np.arange(k)), lt
        assert abs(loss.item() - np.log(2.0)) <= 1e-7, (lt, loss.item())
        want = (0.5 - t.reshape(-1)[:k]) / k
        assert torch.allclose(grad.reshape(-1)[:k], want, rtol=1e-6, atol=0), lt


def test_multiclass_tversky_against_the_composite_on_the_device():
    L = _gpu()
    gen = torch.Generator().manual_seed(4)
    x = (torch.randn(4, 3, 256, 256, generator=gen) * 3.0).to(DEV)
    for t in (torch.randint(0, 3, (4, 256, 256), generator=gen), torch.randint(0, 3, (4, 256, 256), generator=gen).float()):
        loss, grad = _run(L, x, t, "Tversky")
        xc = x.clone().requires_grad_(True)
        want = L.tversky_composite(xc, t.to(DEV))
        want.backward()
        assert abs(loss.item() - want.item()) <= 2e-6 * abs(want.item()), (loss.item(), want.item())
        assert (grad - xc.grad.cpu()).abs().max() <= 1e-5 * xc.grad.abs().max().item()


def test_two_runs_give_identical_bits():
    L = _gpu()
    gen = torch.Generator().manual_seed(3)
    x = _smooth(gen, 4, 256, 320)
    t = (_smooth(gen, 4, 256, 320) > 0.5).float()[:, 0]
    xm = torch.randn(2, 5, 64, 96, generator=gen)
    tm = torch.randint(0, 5, (2, 64, 96), generator=gen)
    for lt, xx, tt in (("dice_bce", x, t), ("Tversky", x, t), ("TopK", x, t), ("BCE_HEM", x, t), ("Tversky", xm, tm)):
        a, b = _run(L, xx, tt, lt), _run(L, xx, tt, lt)
        for u, v in zip(a, b):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32)), lt


def test_bad_arguments_return_status_without_launching():
    _gpu()
    from umi import lib
    fn = lib.fn
    p = torch.zeros(2, 1, 8, 8, device=DEV)
    d = p.data_ptr()
    stats = torch.zeros(64, dtype=torch.float64, device=DEV)
    st = stats.data_ptr()
    w = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    wp, wn = w.data_ptr(), w.numel()
    db_fwd, db_bwd = fn("umi_dice_bce_fwd"), fn("umi_dice_bce_bwd")
    assert db_fwd(None, d, 2, 64, st, d, wp, wn, None) == -1 and db_fwd(d, d, 0, 64, st, d, wp, wn, None) == -1
    assert db_fwd(d, d, 2, 0, st, d, wp, wn, None) == -1 and db_fwd(d, d, 2, 64, st, d, None, wn, None) == -1
    assert db_fwd(d, d, 2, 1 << 30, st, d, wp, wn, None) == -2
    assert db_fwd(d, d, 2, 64, st, d, wp, fn("umi_binloss_ws_bytes")(2, 1, 64) - 1, None) == -3
    assert db_bwd(d, d, None, None, 2, 64, d, None) == -1 and db_bwd(d, d, st, None, 2, 1 << 30, d, None) == -2
    tv_fwd, tv_bwd = fn("umi_tversky_fwd"), fn("umi_tversky_bwd")
    assert tv_fwd(d, d, 1, 2, 0, 64, 0.4, 0.6, st, d, wp, wn, None) == -1
    assert tv_fwd(d, d, 7, 2, 1, 64, 0.4, 0.6, st, d, wp, wn, None) == -1
    assert tv_fwd(d, d, 1, 2, 9, 64, 0.4, 0.6, st, d, wp, wn, None) == -2
    assert tv_fwd(d, d, 0, 2, 1, 64, 0.4, 0.6, st, d, wp, wn, None) == -2          # C == 1 takes fp32 targets only
    assert tv_fwd(d, d, 1, 2, 3, 64, 0.4, 0.6, st, d, wp, fn("umi_binloss_ws_bytes")(2, 3, 64) - 1, None) == -3
    assert tv_bwd(d, d, 1, st, None, 2, 9, 64, 0.4, 0.6, d, None) == -2 and tv_bwd(d, None, 1, st, None, 2, 3, 64, 0.4, 0.6, d, None) == -1
    mask = torch.empty(128, dtype=torch.uint8, device=DEV)
    m = mask.data_ptr()
    tk_fwd, tk_bwd = fn("umi_topk_loss_fwd"), fn("umi_topk_loss_bwd")
    assert tk_fwd(d, d, 128, 0, 0, m, d, wp, wn, None) == -1 and tk_fwd(d, d, 0, 1, 0, m, d, wp, wn, None) == -1
    assert tk_fwd(d, d, 128, 64, 2, m, d, wp, wn, None) == -1 and tk_fwd(d, d, 128, 64, 0, None, d, wp, wn, None) == -1
    assert tk_fwd(d, d, 128, 129, 0, m, d, wp, wn, None) == -2 and tk_fwd(d, d, 1 << 31, 5, 1, m, d, wp, wn, None) == -2
    assert tk_fwd(d, d, 128, 64, 0, m, d, wp, fn("umi_topk_loss_ws_bytes")(128) - 1, None) == -3
    assert tk_bwd(d, d, None, None, 128, 64, d, None) == -1 and tk_bwd(d, d, m, None, 128, 129, d, None) == -2
    torch.cuda.synchronize()


def test_out_of_domain_shapes_fall_back_to_the_composite():
    L = _gpu()
    gen = torch.Generator().manual_seed(8)
    cases = [("Tversky", torch.randn(2, 9, 16, 16, generator=gen), torch.randint(0, 9, (2, 16, 16), generator=gen)),
             ("TopK", torch.randn(2, 2, 16, 16, generator=gen), (torch.rand(2, 16, 16, generator=gen) < 0.5).float()),
             ("BCE_HEM", torch.randn(1, 1, 16, 16, generator=gen), (torch.rand(1, 16, 16, generator=gen) < 0.5).float()),
             ("dice_bce", torch.randn(2, 1, 16, 16, generator=gen).double(), (torch.rand(2, 16, 16, generator=gen) < 0.5).double())]
    comp = {"Tversky": L.tversky_composite, "TopK": L.topk_composite, "BCE_HEM": L.bce_hem_composite,
            "dice_bce": L.dice_bce_composite}
    for lt, x, t in cases:
        if lt == "BCE_HEM":                                          # 256 < 500 pixels: raises, as the reference does
            with pytest.raises(RuntimeError):
                L.calc_loss(x.to(DEV), t.to(DEV), loss_type=lt)
            continue
        loss, grad = _run(L, x, t, lt, device_path=False)
        xc = x.to(DEV).requires_grad_(True)
        want = comp[lt](xc, t.to(DEV))
        want.backward()
        assert torch.equal(loss, want.detach().cpu()) and torch.equal(grad, xc.grad.cpu()), lt


def test_trainer_graph_mode_replays_the_eager_losses():
    _gpu()
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_binary_loss_graph.py")], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0 and "BINARY_LOSS_GRAPH_OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
