"""Global-batch statistics under data parallel (umi.ddp.GradReducer(global_batch=True)) on the GPU:

  * the new entry points against the calls they split (bit for bit) and against float64;
  * whole models in a group of one: the switch on is bit-identical to the switch off;
  * two ranks on ONE GPU (gloo collectives on device tensors, as tests/test_gpu_ddp.py): 2 + 2 images compute the step of one
    process on the 4 images -- against the CPU oracle in fp32 (and NOT with the switch off: the test that fails without the
    feature), against the one-process HIP run in fp16.

Seeds and shapes of the two-rank tests are those screened by tests/test_global_batch.py."""
import math

import numpy as np
import pytest
import torch

from tests.test_global_batch import init_rank, oracle_step, run_ranks, screen_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from umi import lib, ops
    return lib, ops


def _stream():
    return torch.cuda.current_stream().cuda_stream


def rel_err(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


# ---- kernels -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 8, 33, 64])
@pytest.mark.parametrize("rows", [1, 7, 511, 512, 513, 1000])
def test_stat_sums_then_finalize_from_sums_is_bn_finalize(rows, C):
    """rows -> float64 sums -> finalize-from-sums against umi_bn_finalize on the same rows (both sides of RED_MIN_ROWS = 512 and
    of the 128-row slices, ragged channel blocks): transform, 1/std and running statistics bit for bit.  The sums against the
    float64 sum of the rows: n float64 additions in any order are within (n - 1) 2^-53 sum|x| of the exact sum and the
    reference (math.fsum, the exact sum rounded once) within 2^-53 |sum|, so the two are within n 2^-53 sum|x|."""
    lib, ops = _gpu()
    g = torch.Generator().manual_seed(1000 * rows + C)
    part = torch.randn(rows, 2, C, generator=g)
    part[:, 1] = part[:, 1].abs() * 3 + part[:, 0] ** 2
    count = rows * 7
    gamma, beta = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
    pd = part.to(DEV).contiguous().view(-1)
    rm0, rv0 = torch.randn(C, generator=g).to(DEV), (0.5 + torch.rand(C, generator=g)).to(DEV)
    rm_a, rv_a, rm_b, rv_b = rm0.clone(), rv0.clone(), rm0.clone(), rv0.clone()
    tx_a, rs_a = ops.bn_finalize(pd, C, count, gamma, beta, 1e-5, 0.1, rm_a, rv_a)
    sums = ops.bn_stat_sums(pd, C, count)
    assert sums.dtype == torch.float64 and sums.numel() == 2 * C + 1 and sums[-1].item() == count
    tx_b, rs_b = ops.bn_finalize_sums(sums, C, count, gamma, beta, 1e-5, 0.1, rm_b, rv_b)
    for a, b in ((tx_a, tx_b), (rs_a, rs_b), (rm_a, rm_b), (rv_a, rv_b)):
        assert torch.equal(a, b)
    assert not torch.equal(rm_a, rm0)
    p64 = part.numpy().astype(np.float64)
    want = np.array([math.fsum(p64[:, w, c]) for w in (0, 1) for c in range(C)])
    bound = rows * 2.0 ** -53 * np.concatenate([np.abs(p64[:, 0]).sum(0), np.abs(p64[:, 1]).sum(0)])
    err = np.abs(sums[:2 * C].cpu().numpy() - want)
    assert (err <= bound).all(), float((err / bound).max())
    # twice the count (two equal ranks with these sums each): float64 statement of the finalize
    s2 = sums.clone()
    s2 *= 2
    tx_c, rs_c = ops.bn_finalize_sums(s2, C, 2 * count, gamma, beta, 1e-5, 0.1, None, None)
    assert torch.equal(tx_c, tx_a) and torch.equal(rs_c, rs_a)           # 2s / 2n: exact in binary floating point


def _tx(C, gen, lo=0.0):
    t = torch.empty(C, 4)
    t[:, 0] = 0.1 * torch.randn(C, generator=gen)
    t[:, 1] = (0.5 + torch.rand(C, generator=gen)) * torch.where(torch.rand(C, generator=gen) < 0.15, -1.0, 1.0)
    t[:, 2] = 0.2 * torch.randn(C, generator=gen)
    t[:, 3] = lo
    return t


def _dz_f64(y, da, t, rstd, sums, count):
    """Stage 3 of the BatchNorm + ReLU backward in float64 (csrc/common.h umi_bn_dz), and the mask of elements whose ReLU
    decision is clear of fp32 rounding (|z - lo| > 1e-5)."""
    y, da, t, rstd, sums = (v.detach().double().cpu() for v in (y, da, t, rstd, sums))
    z = y * t[:, 1] + t[:, 2]
    dz = torch.where(z > t[:, 3], da, torch.zeros((), dtype=torch.float64))
    xh = (y - t[:, 0]) * rstd
    return t[:, 1] * (dz - sums[0] / count - xh * sums[1] / count), (z - t[:, 3]).abs() > 1e-5


def _dz_bar(ref, dtype):
    """The float64 bar of the BatchNorm backward in tests/test_gpu_kernels.py, 1e-4 max(1, max|ref|); an fp16 result adds the
    half ulp of its storage format, 2^-11 |ref| (+ the smallest subnormal)."""
    bar = torch.full_like(ref, 1e-4 * max(1.0, ref.abs().max().item()))
    return bar + (ref.abs() * 2.0 ** -11 + 2.0 ** -24 if dtype == torch.float16 else 0)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("M,C,ld", [(1 * 37 * 53, 64, 64), (1 * 37 * 53, 64, 80), (3 * 11 * 7, 24, 24), (2 * 9 * 5, 33, 40),
                                    (2 * 24 * 24, 128, 144)])
def test_bn_bwd_apply_count(M, C, ld, dtype):
    """umi_bn_bwd_apply_count: count = M is umi_bn_bwd_apply bit for bit (fp32, the fp16 vector kernel where C % 8 == 0 and
    the scalar one elsewhere, ragged M, channel slices of wider tensors); count = 2 M against float64."""
    lib, ops = _gpu()
    g = torch.Generator().manual_seed(M + C + ld)
    t = _tx(C, g).to(DEV).contiguous()
    rstd = (0.5 + torch.rand(C, generator=g)).to(DEV)
    sums = (torch.randn(2, C, generator=g) * 0.05 * M).to(DEV)
    y = torch.randn(1, 1, M, ld, generator=g).to(dtype).to(DEV)[..., ld - C:]
    da0 = (0.1 * torch.randn(1, 1, M, ld, generator=g)).to(dtype).to(DEV)
    a, b, c = da0.clone(), da0.clone(), da0.clone()
    ops.bn_bwd_apply(a[..., :C], y, t, rstd, sums[0], sums[1])
    ops.bn_bwd_apply(b[..., :C], y, t, rstd, sums[0], sums[1], count=M)
    assert torch.equal(a, b) and not torch.equal(a, da0)
    assert torch.equal(a[..., C:], da0[..., C:])                    # nothing outside the slice was written
    ops.bn_bwd_apply(c[..., :C], y, t, rstd, sums[0], sums[1], count=2 * M)
    assert torch.equal(c[..., C:], da0[..., C:]) and not torch.equal(c, a)
    ref, clear = _dz_f64(y[0, 0], da0[0, 0, :, :C], t, rstd, sums, 2 * M)
    err = (c[0, 0, :, :C].double().cpu() - ref).abs()
    assert clear.float().mean().item() > 0.99
    assert bool((err <= _dz_bar(ref, dtype))[clear].all()), float((err / _dz_bar(ref, dtype))[clear].max())


@pytest.mark.parametrize("shape,strided", [((2, 16, 64, 64, 64), False), ((1, 13, 37, 72, 136), True), ((1, 5, 70, 16, 24), False)])
def test_conv_wgrad_bnapply_count(shape, strided):
    """umi_conv_wgrad_bnapply_count (stage 3 formed while the weight-gradient kernel stages dA): count = N H W is
    umi_conv_wgrad_bnapply bit for bit; count = 2 N H W gives the dz of umi_bn_bwd_apply_count bit for bit (one expression,
    common.h), which is within the float64 bar, and the weight gradient of that dz."""
    lib, ops = _gpu()
    N, H, W, Ci, Co = shape
    M = N * H * W
    g = torch.Generator().manual_seed(sum(shape))

    def slab(c):
        full = torch.randn(N, H, W, c + (16 if strided else 0), generator=g).half().to(DEV)
        return full[..., 8:8 + c] if strided else full

    x, y, da = slab(Ci), slab(Co), slab(Co)
    da.mul_(0.1)
    txa = _tx(Ci, g).to(DEV).contiguous()
    tb = _tx(Co, g).to(DEV).contiguous()
    rstd = (0.5 + torch.rand(Co, generator=g)).to(DEV)
    sums = (torch.randn(2, Co, generator=g) * 0.05 * M).to(DEV)
    args = (Ci * 9, 9, 1, 0.5, 3, 3, 1, 1)
    out = {}
    for key, cnt in (("plain", None), ("m", M), ("2m", 2 * M)):
        dz = torch.full((N, H, W, Co), float("nan"), device=DEV, dtype=torch.float16)
        gw = torch.empty(Co, Ci, 3, 3, device=DEV)
        assert ops.conv_wgrad_bnapply(x, txa, da, y, tb, rstd, sums[0], sums[1], dz, gw, *args, count=cnt)
        out[key] = (dz, gw)
    assert torch.equal(out["plain"][0], out["m"][0]) and torch.equal(out["plain"][1], out["m"][1])
    dz2 = da.clone()
    ops.bn_bwd_apply(dz2, y, tb, rstd, sums[0], sums[1], count=2 * M)
    gw2 = torch.empty(Co, Ci, 3, 3, device=DEV)
    ops.conv_wgrad(x, txa, dz2, None, gw2, *args)
    assert torch.equal(out["2m"][0], dz2.contiguous()) and torch.equal(out["2m"][1], gw2)
    assert not torch.equal(out["2m"][0], out["m"][0])
    ref, clear = _dz_f64(y.reshape(M, Co), da.reshape(M, Co), tb, rstd, sums, 2 * M)
    err = (out["2m"][0].reshape(M, Co).double().cpu() - ref).abs()
    assert bool((err <= _dz_bar(ref, torch.float16))[clear].all())


@pytest.mark.parametrize("shape", [(2, 37, 29, 1, 64), (1, 16, 48, 3, 64)])
def test_stem_wgrad_bnapply_count(shape):
    """The first conv's form (dz = NULL, formed on the fly, never stored): count = N H W is the existing call bit for bit,
    count = 2 N H W is umi_bn_bwd_apply_count + umi_conv_wgrad bit for bit."""
    lib, ops = _gpu()
    N, H, W, Ci, Co = shape
    M = N * H * W
    g = torch.Generator().manual_seed(sum(shape) + 3)
    x = torch.randn(N, H, W, Ci, generator=g).half().to(DEV)
    y = torch.randn(N, H, W, Co, generator=g).half().to(DEV)
    td = _tx(Co, g).to(DEV).contiguous()
    rstd = (0.5 + torch.rand(Co, generator=g)).to(DEV)
    da = (torch.randn(N, H, W, Co, generator=g) * 0.1).half().to(DEV)
    sums = (torch.randn(2, Co, generator=g) * 0.05 * M).to(DEV)
    args = (Ci * 9, 9, 1, 0.25, 3, 3, 1, 1)
    gws = []
    for cnt in (None, M, 2 * M):
        gw = torch.empty(Co, Ci, 3, 3, device=DEV)
        assert ops.conv_wgrad_bnapply(x, None, da, y, td, rstd, sums[0], sums[1], None, gw, *args, count=cnt)
        gws.append(gw)
    assert torch.equal(gws[0], gws[1]) and not torch.equal(gws[0], gws[2])
    dz = da.clone()
    ops.bn_bwd_apply(dz, y, td, rstd, sums[0], sums[1], count=2 * M)
    gw = torch.empty(Co, Ci, 3, 3, device=DEV)
    ops.conv_wgrad(x, None, dz, None, gw, *args)
    assert torch.equal(gw, gws[2])


@pytest.mark.parametrize("HW", [1, 255, 4097])
@pytest.mark.parametrize("C", [1, 2, 8])
def test_split_dice_ce_loss_is_the_fused_loss(C, HW):
    """umi_dice_ce_sums + umi_dice_ce_finalize with the local count leave umi_dice_ce_fwd's stats bit for bit (sums float64, in
    its order); umi_dice_ce_bwd_global with scale 1 and the local count is umi_dice_ce_bwd bit for bit.  With doubled sums, a
    doubled count and scale 2 (two equal ranks) the Dice coefficients and the CE weight are those of the group."""
    lib, ops = _gpu()
    N = 3
    g = torch.Generator().manual_seed(100 * C + HW)
    x = (2 * torch.randn(N, C, HW, generator=g)).to(DEV)
    t = torch.randint(0, C, (N, HW), generator=g).to(DEV)
    K = 3 * C + 1
    ws = ops.workspace(lib.fn("umi_dice_ce_ws_bytes")(N, C, HW), x.device)
    st_a = torch.empty(K + 1, device=DEV)
    lib.check(lib.fn("umi_dice_ce_fwd")(x.data_ptr(), t.data_ptr(), 0, N, C, HW, st_a.data_ptr(), ws.data_ptr(), ws.numel(),
                                        _stream()), "fwd")
    sums = torch.full((K + 1,), float("nan"), dtype=torch.float64, device=DEV)
    lib.check(lib.fn("umi_dice_ce_sums")(x.data_ptr(), t.data_ptr(), 0, N, C, HW, sums.data_ptr(), ws.data_ptr(), ws.numel(),
                                         _stream()), "sums")
    assert bool(torch.isnan(sums[K])) and bool(torch.isfinite(sums[:K]).all())      # exactly 3 C + 1 values written
    st_b = torch.empty(K + 1, device=DEV)
    lib.check(lib.fn("umi_dice_ce_finalize")(sums.data_ptr(), C, float(N * HW), st_b.data_ptr(), _stream()), "finalize")
    assert torch.equal(st_a, st_b)
    assert torch.equal(sums[:K].float(), st_a[:K])
    gout = torch.tensor([0.75], device=DEV)
    d_a, d_b, d_c = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    lib.check(lib.fn("umi_dice_ce_bwd")(x.data_ptr(), t.data_ptr(), 0, st_a.data_ptr(), gout.data_ptr(), N, C, HW,
                                        d_a.data_ptr(), _stream()), "bwd")
    lib.check(lib.fn("umi_dice_ce_bwd_global")(x.data_ptr(), t.data_ptr(), 0, st_b.data_ptr(), gout.data_ptr(), 1.0,
                                               float(N * HW), N, C, HW, d_b.data_ptr(), _stream()), "bwd_global")
    assert torch.equal(d_a, d_b) and (C == 1 or float(d_a.abs().max()) > 0)      # (one class: the gradient is identically 0)
    # two equal ranks: float64 composite of the loss of [x; x] -- its gradient w.r.t. one copy, times the world size 2
    s2 = sums.clone()
    s2[:K] *= 2
    st_c = torch.empty(K + 1, device=DEV)
    lib.check(lib.fn("umi_dice_ce_finalize")(s2.data_ptr(), C, float(2 * N * HW), st_c.data_ptr(), _stream()), "finalize")
    lib.check(lib.fn("umi_dice_ce_bwd_global")(x.data_ptr(), t.data_ptr(), 0, st_c.data_ptr(), None, 2.0, float(2 * N * HW), N,
                                               C, HW, d_c.data_ptr(), _stream()), "bwd_global")
    xx = torch.cat([x, x]).double().cpu().requires_grad_(True)
    tt = torch.cat([t, t]).cpu()
    p = torch.softmax(xx, 1)
    oh = torch.nn.functional.one_hot(tt, C).movedim(-1, 1).double()
    dice = (1 - (2 * (p * oh).sum((0, 2)) + 1e-5) / ((p * p).sum((0, 2)) + oh.sum((0, 2)) + 1e-5)).sum() / C
    loss = 0.5 * torch.nn.functional.cross_entropy(xx, tt) + 0.5 * dice
    loss.backward()
    want = 2 * xx.grad[:N]
    # (the bars of test_fused_dice_ce_loss_matches_composite in tests/test_gpu_kernels.py)
    assert abs(st_c[K].item() - loss.item()) < 2e-6 * max(1.0, abs(loss.item()))
    assert float((d_c.double().cpu() - want).abs().max()) <= 2e-5 * float(want.abs().max())


# ---- whole models, group of one ------------------------------------------------------------------------------------------

def _one_step(m, x, lab, on):
    import loss as L
    from umi import ddp
    red = ddp.GradReducer(m, 1, global_batch=on)
    try:
        assert (ddp.active_batch_sync() is not None) == on
        m.zero_grad(set_to_none=True)
        logits = m(x)
        loss = L.calc_loss(logits, lab, loss_type="dice_bce_mc")
        loss.backward()
        red.sync()
        torch.cuda.synchronize()
        return (logits.detach().clone(), loss.detach().clone(), [p.grad.detach().clone() for p in m.parameters()],
                {k: v.detach().clone() for k, v in m.state_dict().items() if "running_" in k or "num_batches" in k})
    finally:
        red.close()


def _model(kind, mode, S):
    import Model
    torch.manual_seed(11)
    if kind == "unet":
        return Model.UNet(1, 2, 8, False, compute_dtype=mode)
    if kind == "attention":
        return Model.UNet_attention(1, 2, 8, False, compute_dtype=mode)
    from oracle import ref_transunet
    from tests.test_gpu_transunet import product_config
    from TransUnet.vit_seg_modeling import VisionTransformer
    return VisionTransformer(product_config(ref_transunet.small_config(2), S), img_size=S, num_classes=2, compute_dtype=mode)


@pytest.mark.parametrize("kind,mode,H,W", [("unet", "fp32", 32, 32), ("unet", "fp16", 32, 32), ("unet", "fp32_mfma", 32, 32),
                                           ("unet", "fp32", 44, 72), ("unet", "fp16", 44, 72), ("unet", "fp32_mfma", 44, 72),
                                           ("attention", "fp16", 32, 32), ("attention", "fp32", 32, 32),
                                           ("transunet", "fp16", 64, 64)])
def test_group_of_one_switch_on_is_bit_identical_to_off(kind, mode, H, W):
    """One process, world size 1: logits, loss, every gradient and the running statistics after one step are the same bits with
    global_batch on and off -- rows -> sums -> finalize-from-sums, the count variants with count = M and the split loss change
    no arithmetic, and no collective is launched (there is no process group here)."""
    _gpu()
    import loss as L
    assert not torch.distributed.is_initialized()
    L.CLASS_NUMBER = 2
    m = _model(kind, mode, H).to(DEV).train()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3 if kind == "transunet" else 1, H, W, generator=g).to(DEV)
    lab = torch.randint(0, 2, (2, H, W), generator=g).float().to(DEV)
    state = {k: v.clone() for k, v in m.state_dict().items()}
    off = _one_step(m, x, lab, False)
    m.load_state_dict(state)
    on = _one_step(m, x, lab, True)
    assert torch.equal(off[0], on[0]) and torch.equal(off[1], on[1])
    assert len(off[2]) == len(on[2]) > 0 and all(torch.equal(a, b) for a, b in zip(off[2], on[2]))
    assert off[3].keys() == on[3].keys() and len(off[3]) > 0 and all(torch.equal(off[3][k], on[3][k]) for k in off[3])
    assert any(not torch.equal(off[3][k], state[k]) for k in off[3])         # the running statistics did move


# ---- two ranks on one GPU ------------------------------------------------------------------------------------------------

def _two_rank_model(kind, state):
    import Model
    if kind == "transunet_fp16":
        m = _model("transunet", "fp16", 32)
    else:
        m = Model.UNet(1, 2, 8, False, compute_dtype="fp32" if kind == "unet_fp32" else "fp16")
    m.load_state_dict(state)
    return m.to(DEV).train()


def _two_rank_data(kind):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(4, 1, 32, 32, generator=g)
    lab = torch.randint(0, 2, (4, 32, 32), generator=g).float()
    return (x.repeat(1, 3, 1, 1) if kind == "transunet_fp16" else x), lab


def _train(m, red, x, lab, steps, out, tag):
    import loss as L
    from umi import optim as uo
    opt = uo.SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    for step in range(steps):
        logits = m(x)
        loss = L.calc_loss(logits, lab, loss_type="dice_bce_mc")
        opt.zero_grad()
        loss.backward()
        if red is not None:
            red.sync()
        if step == 0:
            out[tag + "logits"] = logits.detach().cpu().numpy()
            out[tag + "loss"] = loss.item()
            out[tag + "grads"] = [p.grad.detach().cpu().numpy().copy() for p in m.parameters()]
            out[tag + "stats"] = {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items() if "running_" in k}
        opt.step()
    torch.cuda.synchronize()
    out[tag + "params"] = [p.detach().cpu().numpy() for p in m.parameters()]


def _rank_worker(rank, world, port, q, kind, state):
    dist = init_rank(rank, world, port)
    import loss as L
    from umi import ddp
    torch.cuda.set_device(0)
    L.CLASS_NUMBER = 2
    x, lab = _two_rank_data(kind)
    xs, ls = x[rank * 2:(rank + 1) * 2].to(DEV), lab[rank * 2:(rank + 1) * 2].to(DEV)
    out = {}
    if kind == "unet_fp32":                              # the switch off: standard per-replica statistics, first step only
        m = _two_rank_model(kind, state)
        red = ddp.GradReducer(m, world, bucket_mb=0.05)
        _train(m, red, xs, ls, 1, out, "off_")
        red.close()
    m = _two_rank_model(kind, state)
    red = ddp.GradReducer(m, world, bucket_mb=0.05, global_batch=True)
    _train(m, red, xs, ls, 2, out, "")
    red.close()
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def _init_state(kind):
    if kind == "transunet_fp16":
        return {k: v.cpu() for k, v in _model("transunet", "fp16", 32).state_dict().items()}
    return screen_inputs()[0].state_dict()


def test_two_ranks_fp32_unet_is_the_oracle_on_the_four_images():
    """UNet(1,2,8) fp32, seeds 100 / 7, 2 + 2 images at 32 x 32, two SGD steps, against the CPU oracle on the four images under
    the fp32 bars of tests/test_gpu_unet.py: first-step logits rtol 1e-4, every averaged gradient tensor within 2e-3 (relative
    L2), running statistics within 1e-5, the loss of the four images on both ranks, replicas identical after both steps.  The
    same run with the switch off misses the logit bar (by 800 x: tests/test_global_batch.py) -- the feature, not the bar."""
    _gpu()
    ref, x, lab = screen_inputs()
    state = ref.state_dict()
    res = run_ranks(_rank_worker, 2, "unet_fp32", state)
    gl, gg, gs = oracle_step({k: v.clone() for k, v in state.items()}, x, lab, torch.float32, 1)
    scale = float(gl.abs().max())
    got = np.concatenate([res[0]["logits"], res[1]["logits"]])
    off = np.concatenate([res[0]["off_logits"], res[1]["off_logits"]])
    print("logits vs oracle, of scale: on", float(np.abs(got - gl.numpy()).max()) / scale, "off",
          float(np.abs(off - gl.numpy()).max()) / scale)
    np.testing.assert_allclose(got, gl.numpy(), rtol=1e-4, atol=1e-4 * scale)
    assert float(np.abs(off - gl.numpy()).max()) > 1e-4 * scale + 1e-4 * float(np.abs(gl.numpy()).max())
    import loss as L
    L.CLASS_NUMBER = 2
    want_loss = L.calc_loss(gl.float(), lab, loss_type="dice_bce_mc").item()
    errs = [rel_err(a, b) for a, b in zip(res[0]["grads"], gg)]
    print("worst gradient", max(errs), "loss", res[0]["loss"], want_loss)
    for r in (0, 1):
        assert abs(res[r]["loss"] - want_loss) < 1e-4
    assert max(errs) < 2e-3, errs
    for k, v in gs.items():
        assert float(np.abs(res[0]["stats"][k] - v.numpy()).max()) <= 1e-5 * max(1.0, float(v.abs().max())), k
    for a, b in zip(res[0]["grads"], res[1]["grads"]):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(res[0]["params"], res[1]["params"]):
        np.testing.assert_array_equal(a, b)
    for k in gs:
        np.testing.assert_array_equal(res[0]["stats"][k], res[1]["stats"][k])


@pytest.mark.parametrize("kind", ["unet_fp16", "transunet_fp16"])
def test_two_ranks_fp16_is_the_one_process_run_on_the_four_images(kind):
    """fp16 UNet(1,2,8) and the small fp16 TransUNet, 2 + 2 images, against the one-process HIP run on the four images under
    the fp16 bars of tests/test_gpu_unet.py: logits within 2e-3 of scale, gradients within 3e-2 relative L2; replicas
    identical after two steps."""
    _gpu()
    import loss as L
    L.CLASS_NUMBER = 2
    state = _init_state(kind)
    res = run_ranks(_rank_worker, 2, kind, state)
    x, lab = _two_rank_data(kind)
    one = {}
    ref_model = _two_rank_model(kind, state)
    _train(ref_model, None, x.to(DEV), lab.to(DEV), 1, one, "")
    got = np.concatenate([res[0]["logits"], res[1]["logits"]])
    e_logit = float(np.abs(got - one["logits"]).max() / np.abs(one["logits"]).max())
    names = [k for k, _ in ref_model.named_parameters()]
    errs = {k: rel_err(a, b) for k, a, b in zip(names, res[0]["grads"], one["grads"])}
    # softmax is invariant to a shift of the keys: the gradient of a key bias is rounding noise on both sides, as in
    # tests/test_gpu_transunet.py (here under 1e-3 of the query bias's gradient; printed)
    noise = {k for k in names if k.endswith("attn.key.bias")}
    gmax = dict(zip(names, (float(np.abs(g).max()) for g in one["grads"])))
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:4]
    print(kind, "logits", e_logit, "loss", res[0]["loss"], one["loss"], "worst gradients", worst,
          "key bias / query bias gradient", [(k, gmax[k] / (gmax[k.replace("key", "query")] + 1e-30)) for k in sorted(noise)])
    assert e_logit < 2e-3
    assert abs(res[0]["loss"] - one["loss"]) < 2e-3 and res[0]["loss"] == res[1]["loss"]
    bad = {k: e for k, e in errs.items() if k not in noise and e >= 3e-2}
    assert not bad and len(errs) - len(noise) > 40, bad
    assert all(np.isfinite(g).all() for g in res[0]["grads"])
    for a, b in zip(res[0]["params"], res[1]["params"]):
        np.testing.assert_array_equal(a, b)
