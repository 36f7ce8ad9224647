"""The count-ratio-weighted multi-task loss on the MI355X (csrc/multitask_ratio.hip through loss.multi_task_ratio_loss) against
an fp64 restatement of the reference lines (Trainer.py:1226-1248), and the product Trainer's multi_task_trainRatio on the HIP
models: against the reference's own run (tests/golden/trainer_multitask_ratio.npz), on a small multi-task TransUNet, and with
graph=True against the eager run (child process, tools/check_multitask_ratio_graph.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import recipe

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: torch.cuda.is_available() is False")


def _restated(o1, o2, l1, l2, gate):
    """fp64 restatement of Trainer.py:1226-1248 (CPU)."""
    o1, o2, l1, l2 = (t.detach().cpu().double() for t in (o1, o2, l1, l2))
    o1.requires_grad_(True)
    o2.requires_grad_(True)
    r1, r2 = torch.relu(o1)[:, 0], torch.relu(o2)[:, 0]
    L1, L2 = ((r1 - l1) ** 2).mean(), ((r2 - l2) ** 2).mean()
    g1, g2, p1, p2 = l1.sum((1, 2)), l2.sum((1, 2)), r1.sum((1, 2)), r2.sum((1, 2))
    r = (g1 / (g2 + g1) - p1 / (p2 + p1)).abs().mean()
    return ((L1 + L2) * (1 + 10 * r) if gate else L1 + L2), L1, L2, r, o1, o2


def _inputs(B, H, W, seed, offset=0, zeros=False):
    """Device o1, o2 (B, 1, H, W) and l1, l2 (B, H, W), fp32 contiguous; offset > 0: views starting `offset` floats into their
    storage (misaligned for 16-byte loads)."""
    gen = torch.Generator().manual_seed(seed)
    o1, o2 = torch.randn(B, 1, H, W, generator=gen), torch.randn(B, 1, H, W, generator=gen)
    l1, l2 = torch.rand(B, H, W, generator=gen) * 2, torch.rand(B, H, W, generator=gen)
    if zeros:
        o1.view(-1)[::3] = 0.0
        o2.view(-1)[1::5] = 0.0
    out = []
    for t in (o1, o2, l1, l2):
        buf = torch.empty(t.numel() + offset, device=DEV)
        v = buf[offset:].view(t.shape)
        v.copy_(t)
        out.append(v)
    return out


def _check(o1, o2, l1, l2, gate, up, gtol=2e-5):
    import loss as L
    a, b = o1.detach().clone().requires_grad_(True), o2.detach().clone().requires_grad_(True)
    outs = L.multi_task_ratio_loss(a, b, l1, l2, gate)
    sum(u * o for u, o in zip(up, outs)).backward()
    *ref, ra, rb = _restated(o1, o2, l1, l2, gate)
    sum(u * o for u, o in zip(up, ref)).backward()
    # r is a difference of two ratios of O(1) built from fp32 per-thread sums: its error is absolute, ~1e-7 of the ratios,
    # and the gated loss carries it times 10 (L1 + L2)
    scale = abs(ref[1].item() + ref[2].item())
    for x, y, atol in zip(outs, ref, (1e-5 * scale, 1e-9, 1e-9, 1e-6)):
        assert x.dtype == torch.float32 and x.shape == ()
        np.testing.assert_allclose(x.item(), y.item(), rtol=2e-6, atol=atol)
    for d, r in ((a.grad, ra.grad), (b.grad, rb.grad)):
        r = r.numpy()
        np.testing.assert_allclose(d.cpu().numpy(), r, rtol=gtol, atol=gtol * max(float(np.abs(r).max()), 1e-30))
    return outs, a.grad, b.grad


@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("HW", [(1, 1), (1, 7), (33, 65), (512, 512)])
@pytest.mark.parametrize("B", [1, 3, 16])
def test_device_loss_matches_fp64_restatement(B, HW, gate):
    """Loss, loss1, loss2, ratio and both output gradients, with random upstream gradients on all four outputs."""
    _need_gpu()
    o1, o2, l1, l2 = _inputs(B, *HW, seed=B * 1000 + HW[0] * 7 + HW[1])
    up = torch.randn(4, generator=torch.Generator().manual_seed(B + HW[1])).tolist()
    _check(o1, o2, l1, l2, gate, up)


@pytest.mark.parametrize("shape", [(3, 33, 65), (2, 16, 16), (16, 64, 64)])
def test_device_loss_misaligned_views_and_exact_zeros(shape):
    """Views one float into their storage (no 16-byte loads), outputs that are exactly 0 (ReLU gradient 0 there)."""
    _need_gpu()
    o1, o2, l1, l2 = _inputs(*shape, seed=sum(shape), offset=1, zeros=True)
    assert o1.data_ptr() % 16 != 0
    _, d1, d2 = _check(o1, o2, l1, l2, True, [1.0, 0.5, -0.25, 2.0])
    assert (d1[o1 == 0] == 0).all() and (d2[o2 == 0] == 0).all()


def test_device_loss_outputs_equal_labels():
    """o == l: both MSEs and r are 0 and s_b = sgn(0) = 0; the gradients are 0 wherever o > 0 as well."""
    _need_gpu()
    import loss as L
    _, _, l1, l2 = _inputs(4, 20, 24, seed=3)
    o1, o2 = l1.unsqueeze(1).clone().requires_grad_(True), l2.unsqueeze(1).clone().requires_grad_(True)
    outs = L.multi_task_ratio_loss(o1, o2, l1, l2, True)
    assert [v.item() for v in outs] == [0.0, 0.0, 0.0, 0.0]
    sum(outs).backward()
    assert (o1.grad == 0).all() and (o2.grad == 0).all()


@pytest.mark.parametrize("kind", ["pred", "label"])
@pytest.mark.parametrize("gate", [False, True])
def test_device_loss_zero_count_images_follow_the_composite(kind, gate):
    """An image whose ReLU'd outputs (or labels) sum to 0 makes r NaN.  The NaN positions of the outputs and gradients are the
    composite's (same fp32 inputs on the CPU); with the gate off the loss and the gradients stay finite."""
    _need_gpu()
    import loss as L
    o1, o2, l1, l2 = _inputs(3, 12, 20, seed=11)
    with torch.no_grad():
        if kind == "pred":
            o1[1].copy_(-o1[1].abs())
            o2[1].copy_(-o2[1].abs())
        else:
            l1[1].zero_()
            l2[1].zero_()
    res = []
    for dev in (True, False):
        a, b = (t.detach().clone() if dev else t.detach().cpu() for t in (o1, o2))
        a.requires_grad_(True)
        b.requires_grad_(True)
        la, lb = (l1, l2) if dev else (l1.cpu(), l2.cpu())
        outs = L.multi_task_ratio_loss(a, b, la, lb, gate)
        outs[0].backward()
        res.append(([v.detach().cpu() for v in outs], a.grad.cpu(), b.grad.cpu()))
    (do, d1, d2), (co, c1, c2) = res
    assert torch.isnan(do[3]) and torch.isnan(co[3])
    for x, y in zip(do, co):
        assert torch.isnan(x) == torch.isnan(y)
    assert torch.equal(torch.isnan(d1), torch.isnan(c1)) and torch.equal(torch.isnan(d2), torch.isnan(c2))
    if not gate:
        assert torch.isfinite(do[0]) and torch.isfinite(d1).all() and torch.isfinite(d2).all()
        np.testing.assert_allclose(d1.numpy(), c1.numpy(), rtol=1e-4, atol=1e-4 * float(c1.abs().max()))
    else:
        assert torch.isnan(do[0]) and torch.isnan(d1).any()


@pytest.fixture
def device_calls():
    """Routes loss.py's device Function through a subclass that counts its forwards; yields the list of calls."""
    import loss as L
    calls = []
    base = L._MultiTaskRatio

    class Counting(base):
        @staticmethod
        def forward(ctx, *args):
            calls.append(1)
            return base.forward(ctx, *args)
    L._MultiTaskRatio = Counting
    try:
        yield calls
    finally:
        L._MultiTaskRatio = base


def test_device_loss_is_deterministic_and_takes_the_device_path(device_calls):
    """Identical inputs give bit-identical outputs and gradients; the device Function runs (counted), also under no_grad."""
    _need_gpu()
    import loss as L
    o1, o2, l1, l2 = _inputs(16, 512, 512, seed=5)
    runs = []
    for _ in range(2):
        a, b = o1.detach().clone().requires_grad_(True), o2.detach().clone().requires_grad_(True)
        outs = L.multi_task_ratio_loss(a, b, l1, l2, True)
        (outs[0] + 0.5 * outs[3]).backward()
        runs.append(torch.cat([torch.stack(outs).detach().flatten(), a.grad.flatten(), b.grad.flatten()]))
    assert torch.equal(runs[0].view(torch.int32), runs[1].view(torch.int32))
    with torch.no_grad():
        outs = L.multi_task_ratio_loss(o1, o2, l1, l2, False)
    assert not outs[0].requires_grad and abs(outs[0].item() - (outs[1] + outs[2]).item()) < 1e-6
    flag = torch.ones((), device=DEV)                       # the gate as a device flag (Trainer graph mode) == the bool
    gated = L.multi_task_ratio_loss(o1, o2, l1, l2, flag)
    assert torch.equal(gated[0], runs[0][0]) and torch.equal(L.multi_task_ratio_loss(o1, o2, l1, l2, flag.zero_())[0], outs[0])
    assert len(device_calls) == 5
    L.multi_task_ratio_loss(o1.cpu(), o2.cpu(), l1.cpu(), l2.cpu(), True)     # CPU tensors: the composite
    assert len(device_calls) == 5


@pytest.mark.parametrize("run", ["none", "plateau"])
def test_trainer_ratio_loop_on_hip_model_follows_reference_run(golden_dir, tmp_path, run):
    """Product Trainer.multi_task_trainRatio driving the HIP `Model.UNet_multitask(1, 1, 8)` against the reference's own run
    of that loop (fixture): 8 epochs across the gate switch, with and without ReduceLROnPlateau.  The first two epochs are held
    to the bound of test_gpu_unet.py::test_trainer_multitask_on_hip_model_follows_reference_run (same model, data and
    optimizer, 2 epochs).  Over 16 SGD steps two fp32 implementations drift apart (ReLU masks of regression heads near 0 flip,
    momentum carries it on): measured 0.2 % at epoch 5 and under 1 % in epochs 6-8 for the train losses and alpha, which are
    held to 5 %.  The validation losses from epoch 6 on are single images weighted by (1 + 10 r), r = |rG - rP| a difference
    of two nearly equal ratios, so that drift shows there as up to 18 % (measured at epoch 8 of 'none'); they are held to 30 %,
    which still sees the gate (a factor of 2 to 5).  The arithmetic of the device loss itself is pinned against fp64 above.
    Step count, LR and checkpoint files are exact."""
    _need_gpu()
    import Model
    from torch.utils.data import DataLoader
    from Trainer import Trainer
    from tools.gen_golden import PairLabels, multitask_trainer_data
    g = np.load(os.path.join(golden_dir, "trainer_multitask_ratio.npz"))
    p = lambda k: g[f"{run}_{k}"]
    m = Model.UNet_multitask(1, 1, 8, False, compute_dtype="fp32")
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=22))
    m.to(DEV)
    xs, l1, l2 = multitask_trainer_data()
    loaders = {"train": DataLoader(PairLabels(xs[:4], l1[:4], l2[:4]), batch_size=2, shuffle=False),
               "val": DataLoader(PairLabels(xs[4:], l1[4:], l2[4:]), batch_size=1)}
    opt = torch.optim.SGD(m.parameters(), lr=float(p("lr")), momentum=0.9, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, patience=0) if bool(p("scheduler")) else None
    tr = Trainer(m, "multi_task_reg", torch.cuda.FloatTensor, DEV, str(tmp_path), loaders, 2, opt, int(p("patience")),
                 int(p("epochs")), "multi_task_loss_ratio", "mse", lr_scheduler=sched)
    tr.train()
    for mine, key in ((tr.train_loss_list, "train_loss"), (tr.val_loss_list, "val_loss"),
                      (tr.train_loss_list_1, "train_loss_1"), (tr.train_loss_list_2, "train_loss_2"),
                      (tr.val_loss_list_1, "val_loss_1"), (tr.val_loss_list_2, "val_loss_2")):
        np.testing.assert_allclose(mine, p(key), rtol=5e-2 if key.startswith("train") else 0.3, err_msg=key)
        if key.startswith("train"):
            np.testing.assert_allclose(mine[:2], p(key)[:2], rtol=2e-4, atol=2e-5, err_msg=key)
    np.testing.assert_allclose(tr.alpha_list, p("alpha"), rtol=5e-2)
    np.testing.assert_allclose(tr.alpha_list[:2], p("alpha")[:2], rtol=2e-4)
    assert tr.iter_num == int(p("iter_num"))
    np.testing.assert_allclose(opt.param_groups[0]["lr"], float(p("final_lr")), rtol=1e-12)
    assert sorted(os.listdir(tmp_path / "models")) == list(p("files"))


def test_trainer_ratio_loop_on_small_multitask_transunet(tmp_path, device_calls):
    """A small VisionTransformerMultitask (1 output map per head) runs the loop for 7 epochs, across the gate switch: the
    losses stay finite, the validation record starts at epoch 6, and the device loss ran."""
    _need_gpu()
    from torch.utils.data import DataLoader
    from oracle import ref_transunet
    from tests.test_gpu_transunet import product_config
    from tools.gen_golden import PairLabels
    from TransUnet import vit_seg_modeling as vsm
    from Trainer import Trainer
    img = 64
    cfg = ref_transunet.small_config(1)
    torch.manual_seed(0)
    m = vsm.VisionTransformerMultitask(product_config(cfg, img), img_size=img, num_classes=1, compute_dtype="fp32").to(DEV)
    xs, l1 = recipe.synthetic_batch(6, 1, img, img, 2, seed=61)
    _, l2 = recipe.synthetic_batch(6, 1, img, img, 3, seed=62)
    loaders = {"train": DataLoader(PairLabels(xs[:4], l1[:4], 0.5 * l2[:4]), batch_size=2, shuffle=False),
               "val": DataLoader(PairLabels(xs[4:], l1[4:], 0.5 * l2[4:]), batch_size=2)}
    opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    tr = Trainer(m, "multi_task_regTU", torch.cuda.FloatTensor, DEV, str(tmp_path), loaders, 2, opt, 25, 7,
                 "multi_task_loss_ratio", "mse", lr_scheduler=None)
    tr.train()
    assert len(tr.train_loss_list) == 7 and len(tr.val_loss_list) == 2 and len(tr.alpha_list) == 7
    for v in tr.train_loss_list + tr.val_loss_list + tr.train_loss_list_1 + tr.train_loss_list_2:
        assert np.isfinite(v), (tr.train_loss_list, tr.val_loss_list)
    assert len(device_calls) == 7 * 2 + 7 * 1            # 2 training and 1 validation step per epoch, all on the device


def test_trainer_ratio_graph_mode_replays_the_eager_run():
    """graph=True against eager over 7 epochs with a ragged last batch, without and with a ReduceLROnPlateau object: every
    per-step loss and the final weights bit for bit across the epoch-5 -> 6 gate switch (child process: stream capture is
    sensitive to what ran before it in the process)."""
    _need_gpu()
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_multitask_ratio_graph.py")],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "MT_RATIO_GRAPH_OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
