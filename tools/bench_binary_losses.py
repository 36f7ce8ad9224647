#!/usr/bin/env python3
"""Times 'dice_bce', 'Tversky', 'TopK' and 'BCE_HEM' (csrc/binary_losses.hip) on one MI355X with device events after
warm-up:

  loss : forward + backward of each loss at (16, 1, 512, 512) through calc_loss (the device path) against its torch
         composite (loss.py *_composite) on the same inputs, alternated over several rounds in one process;
  step : a graph-replayed UNet(1, 1, 64) fp16 training step (forward + loss + backward + umi.optim.SGD) at B=16, 512x512,
         with loss 'dice_bce' and 'TopK' against 'BCE', alternated over several rounds.

Prints one JSON line and writes it to --out if given.
Usage:  python tools/bench_binary_losses.py [--only loss|step|all] [--iters 50] [--rounds 3] [--out profiles/x.json]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

DEV = "cuda"
LOSSES = ("dice_bce", "Tversky", "TopK", "BCE_HEM")


def events_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def inputs(B, H, W, seed=0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = F.avg_pool2d(torch.randn(B, 1, H + 8, W + 8, device=DEV, generator=g), 9, stride=1) * 9.0
    t = (F.avg_pool2d(torch.randn(B, 1, H + 8, W + 8, device=DEV, generator=g), 9, stride=1) * 9.0 > 1.0).float()
    return x.contiguous(), t[:, 0].contiguous()


def bench_loss(iters, rounds):
    import loss as L
    B, H, W = 16, 512, 512
    x, t = inputs(B, H, W)
    x.requires_grad_(True)
    comp = {"dice_bce": L.dice_bce_composite, "Tversky": L.tversky_composite, "TopK": L.topk_composite,
            "BCE_HEM": L.bce_hem_composite}
    fns = {}
    for lt in LOSSES:
        def dev(lt=lt):
            x.grad = None
            L.calc_loss(x, t, loss_type=lt).backward()

        def ref(lt=lt):
            x.grad = None
            comp[lt](x, t).backward()
        fns[f"{lt}_device_ms"], fns[f"{lt}_composite_ms"] = dev, ref
    times = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(5):
            fn()
    for _ in range(rounds):                                   # alternate device and composite on the same box
        for k, fn in fns.items():
            times[k].append(events_ms(fn, iters))
    res = {k: statistics.median(v) for k, v in times.items()}
    for lt in LOSSES:
        res[f"{lt}_speedup"] = res[f"{lt}_composite_ms"] / res[f"{lt}_device_ms"]
    N = B * H * W
    # compulsory HBM bytes per forward + backward: every pass reads pred and target (8 B / pixel); the backward writes dpred
    # (4 B); the selection losses make 5 forward passes (4 digit histograms, 1 select-and-sum writing the 1-byte mask) and
    # read the mask again in the backward
    res["bytes_dice_bce"] = res["bytes_Tversky"] = N * (8 + 8 + 4)
    res["bytes_TopK"] = res["bytes_BCE_HEM"] = N * (5 * 8 + 1 + 8 + 1 + 4)
    res["shape"] = [B, 1, H, W]
    return res


def bench_step(iters, rounds):
    import Model
    import loss as L
    from umi import optim as uo
    from umi.graphs import GraphedStep
    B, H, W = 16, 512, 512
    _, t = inputs(B, H, W, seed=1)
    x = torch.randn(B, 1, H, W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
    steps = {}
    for loss_type in ("BCE", "dice_bce", "TopK"):
        torch.manual_seed(0)
        m = Model.UNet(1, 1, 64, compute_dtype="fp16").to(DEV).train()
        opt = uo.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)

        def body(xx, yy, m=m, opt=opt, loss_type=loss_type):
            loss = L.calc_loss(m(xx), yy, loss_type=loss_type)
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss.detach()
        steps[loss_type] = GraphedStep(body, [x, t], warmup=3, optimizers=[opt])
    times = {k: [] for k in steps}
    for _ in range(rounds):
        for k, gs in steps.items():
            for _ in range(3):
                gs(x, t)
            times[k].append(events_ms(lambda gs=gs: gs(x, t), iters))
    res = {f"step_{k}_ms": statistics.median(v) for k, v in times.items()}
    res.update({f"step_{k}_ms_all": v for k, v in times.items()})
    for k in ("dice_bce", "TopK"):
        res[f"step_{k}_delta_ms"] = res[f"step_{k}_ms"] - res["step_BCE_ms"]
    res["step_workload"] = "UNet(1, 1, 64) fp16, B=16, 512x512, graph-replayed, umi.optim.SGD"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="all", choices=("loss", "step", "all"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_binary_losses.py measures on the MI355X"
    res = {"device": torch.cuda.get_device_name(0)}
    if a.only in ("loss", "all"):
        res.update(bench_loss(a.iters, a.rounds))
    if a.only in ("step", "all"):
        res.update(bench_step(max(1, a.iters // 2), a.rounds))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
