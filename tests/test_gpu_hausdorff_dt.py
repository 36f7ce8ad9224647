"""HausdorffDTLoss on the MI355X (csrc/hausdorff_dt.hip): device fields bit-identical to the reference's scipy fields,
loss / gradient against the reference (tests/golden/hausdorff_dt.npz) and the CPU path, the foreground mask against
torch.sigmoid on the device, determinism, argument checks, and a graph-replayed Trainer step (child process: stream capture
is sensitive to what ran before it in the process)."""
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


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    import loss as L
    return L


def _device(L, x, t, alpha=0.2):
    """(loss, D, pred field, target field, d loss / d pred) from the kernels."""
    x = x.to(DEV).contiguous().requires_grad_(True)
    t = t.to(DEV).contiguous()
    fields = torch.empty((2,) + tuple(x.shape), device=DEV)
    loss, D = L._HausdorffDT.apply(x, t, alpha, fields)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().cpu(), D.cpu(), fields[0].cpu(), fields[1].cpu(), x.grad.cpu()


def _ulp_diff(a, b):
    ai, bi = a.numpy().view(np.int32).astype(np.int64), b.numpy().view(np.int32).astype(np.int64)
    return np.abs(ai - bi).max()


def test_device_fields_loss_and_gradient_match_the_reference():
    L = _gpu()
    g = np.load(os.path.join(REPO, "tests", "golden", "hausdorff_dt.npz"))
    for c in (str(n) for n in g["cases"]):
        x, t = torch.from_numpy(g[f"{c}_pred"]), torch.from_numpy(g[f"{c}_target"])
        loss, D, fp, ft, grad = _device(L, x, t)
        pw, tw = torch.from_numpy(g[f"{c}_pred_dt"]), torch.from_numpy(g[f"{c}_target_dt"])
        assert torch.equal(fp.view(torch.int32), pw.view(torch.int32)), (c, (fp - pw).abs().max().item())
        assert torch.equal(ft.view(torch.int32), tw.view(torch.int32)), (c, (ft - tw).abs().max().item())
        assert _ulp_diff(D, pw ** 0.2 + tw ** 0.2) <= 2, c                 # device powf vs CPU pow
        want = float(g[f"{c}_loss"])
        assert abs(loss.item() - want) <= 1e-6 * abs(want), (c, loss.item(), want)
        gw = g[f"{c}_grad"]
        assert np.abs(grad.numpy() - gw).max() <= 1e-5 * np.abs(gw).max(), c


def test_module_debug_tuple_on_the_device():
    L = _gpu()
    g = np.load(os.path.join(REPO, "tests", "golden", "hausdorff_dt.npz"))
    x, t = torch.from_numpy(g["odd_37x53_pred"]).to(DEV), torch.from_numpy(g["odd_37x53_target"]).to(DEV)
    loss, (dt_field, pred_error, distance, pred_dt, target_dt) = L.HausdorffDTLoss()(x, t, debug=True)
    want = float(g["odd_37x53_loss"])
    assert abs(float(loss) - want) <= 1e-6 * want
    assert np.array_equal(pred_dt, g["odd_37x53_pred_dt"][0, 0]) and np.array_equal(target_dt, g["odd_37x53_target_dt"][0, 0])
    assert dt_field.shape == pred_error.shape == distance.shape == (37, 53)
    assert abs(L.calc_loss(x, t, loss_type="HausdorffDTLoss").item() - want) <= 1e-6 * want


def _smooth_logits(gen, B, H, W):
    n = torch.randn(B, 1, H + 8, W + 8, generator=gen)
    x = F.avg_pool2d(n, 9, stride=1) * 9.0
    return torch.where(x.abs() < 1e-3, torch.full_like(x, 1e-3), x)   # keep the CPU / device sigmoid rounding out of play


def test_full_size_batch_agrees_with_the_cpu_path():
    L = _gpu()
    gen = torch.Generator().manual_seed(7)
    B, H, W = 16, 512, 512
    x = _smooth_logits(gen, B, H, W)
    t = (_smooth_logits(gen, B, H, W) > 1.0).float()
    t[3] = 0.0                                                         # an empty target
    x[5] = x[5].abs()                                                  # an all-foreground prediction
    loss, D, fp, ft, grad = _device(L, x, t)
    for b in (0, 5, 11):                                               # full images, fields bit for bit
        s = torch.sigmoid(x[b:b + 1]).numpy()
        assert np.array_equal(fp[b:b + 1].numpy(), L._distance_field(s)), b
        assert np.array_equal(ft[b:b + 1].numpy(), L._distance_field(t[b:b + 1].numpy())), b
    xc = x.clone().requires_grad_(True)
    lc = L.HausdorffDTLoss()(xc, t)
    lc.backward()
    assert abs(loss.item() - lc.item()) <= 1e-6 * lc.item(), (loss.item(), lc.item())
    assert (grad - xc.grad).abs().max() <= 1e-5 * xc.grad.abs().max()


def test_foreground_mask_is_torch_sigmoid_on_the_device():
    """1x1 images: the prediction field is 1 (all foreground) where sigmoid(x) > 0.5, else 0 (no foreground)."""
    L = _gpu()
    tiny = torch.tensor([0.0, -0.0, 1e-8, -1e-8, 1e-7, -1e-7, 1e-6, -1e-6])
    geo = torch.logspace(-12, -4, 2001)
    x = torch.cat([tiny, geo, -geo, torch.linspace(-1e-6, 1e-6, 4001), torch.linspace(-3e-7, 3e-7, 6001)])
    x = x.float().reshape(-1, 1, 1, 1)
    _, _, fp, _, _ = _device(L, x, torch.zeros_like(x))
    want = (torch.sigmoid(x.to(DEV)) > 0.5).float().cpu()
    assert torch.equal(fp, want), int((fp != want).sum())


def test_two_runs_give_identical_bits():
    L = _gpu()
    gen = torch.Generator().manual_seed(3)
    x = _smooth_logits(gen, 4, 256, 320)
    t = (_smooth_logits(gen, 4, 256, 320) > 0.5).float()
    a, b = _device(L, x, t), _device(L, x, t)
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))


def test_bad_arguments_return_status_without_launching():
    _gpu()
    from umi import lib
    fwd, bwd, ws = lib.fn("umi_hdt_fwd"), lib.fn("umi_hdt_bwd"), lib.fn("umi_hdt_ws_bytes")
    p = torch.zeros(1, 1, 8, 8, device=DEV)
    d, w = p.data_ptr(), torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    args = dict(pred=d, target=d, B=1, C=1, H=8, W=8, alpha=0.2, D=d, fields=None, loss=d, ws=w.data_ptr(), nbytes=w.numel(), st=None)

    def call(**kw):
        a = dict(args, **kw)
        return fwd(a["pred"], a["target"], a["B"], a["C"], a["H"], a["W"], a["alpha"], a["D"], a["fields"], a["loss"], a["ws"],
                   a["nbytes"], a["st"])
    assert call(pred=None) == -1 and call(target=None) == -1 and call(D=None) == -1 and call(loss=None) == -1
    assert call(ws=None) == -1 and call(B=0) == -1 and call(H=0) == -1 and call(W=-3) == -1 and call(C=0) == -1
    assert call(C=2) == -2 and call(H=4097) == -2 and call(W=5000) == -2
    assert call(nbytes=ws(1, 8, 8) - 1) == -3
    assert bwd(None, d, d, None, 1, 1, 8, 8, d, None) == -1 and bwd(d, d, d, None, 0, 1, 8, 8, d, None) == -1
    assert bwd(d, d, d, None, 1, 2, 8, 8, d, None) == -2
    torch.cuda.synchronize()


def test_trainer_graph_mode_replays_the_eager_losses():
    _gpu()
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_hdt_graph.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "HDT_GRAPH_OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
