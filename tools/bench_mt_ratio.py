#!/usr/bin/env python3
"""Times the count-ratio-weighted multi-task loss (csrc/multitask_ratio.hip) on one MI355X with device events after warm-up:

  loss : forward + backward of loss.multi_task_ratio_loss at (16, 1, 512, 512) per head, gate on, through the device kernels
         against its torch composite (loss.multi_task_ratio_composite) on the same inputs, alternated over several rounds;
  step : a graph-replayed UNet_multitask(1, 1, 64) fp16 training step (forward + loss + backward + umi.optim.SGD) at B=16,
         512x512, with the ratio loss (gate on) against the plain multi-task loss (ReLU + 'mse' per head, summed).

Prints one JSON line and writes it to --out if given.
Usage:  python tools/bench_mt_ratio.py [--only loss|step|all] [--iters 50] [--rounds 3] [--out profiles/x.json]
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
    o1, o2 = (torch.randn(B, 1, H, W, device=DEV, generator=g) for _ in range(2))
    l1, l2 = (torch.rand(B, H, W, device=DEV, generator=g) for _ in range(2))
    return o1, o2, l1, l2


def bench_loss(iters, rounds):
    import loss as L
    B, H, W = 16, 512, 512
    o1, o2, l1, l2 = inputs(B, H, W)
    o1.requires_grad_(True)
    o2.requires_grad_(True)

    def run(fn):
        def go():
            o1.grad = o2.grad = None
            fn(o1, o2, l1, l2, True)[0].backward()
        return go
    fns = {"device_ms": run(L.multi_task_ratio_loss), "composite_ms": run(L.multi_task_ratio_composite)}
    for fn in fns.values():
        for _ in range(5):
            fn()
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            times[k].append(events_ms(fn, iters))
    res = {f"loss_{k}": statistics.median(v) for k, v in times.items()}
    res["loss_speedup"] = res["loss_composite_ms"] / res["loss_device_ms"]
    N = B * H * W
    # compulsory HBM bytes: the forward reads o1, o2, l1, l2 (16 B / pixel); the backward reads them again and writes d1, d2
    res["loss_bytes_fwd"], res["loss_bytes_bwd"] = N * 16, N * 24
    res["loss_shape"] = [B, 1, H, W]
    return res


def bench_step(iters, rounds):
    import Model
    import loss as L
    from umi import optim as uo
    from umi.graphs import GraphedStep
    B, H, W = 16, 512, 512
    _, _, l1, l2 = inputs(B, H, W, seed=1)
    x = torch.randn(B, 1, H, W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))

    def ratio(o1, o2, y1, y2):
        return L.multi_task_ratio_loss(o1, o2, y1, y2, True)[0]

    def plain(o1, o2, y1, y2):
        return L.calc_loss(F.relu(o1), y1, loss_type="mse") + L.calc_loss(F.relu(o2), y2, loss_type="mse")
    steps = {}
    for name, lf in (("mse", plain), ("ratio", ratio)):
        torch.manual_seed(0)
        m = Model.UNet_multitask(1, 1, 64, compute_dtype="fp16").to(DEV).train()
        opt = uo.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)

        def body(xx, y1, y2, m=m, opt=opt, lf=lf):
            loss = lf(*m(xx), y1, y2)
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss.detach()
        steps[name] = GraphedStep(body, [x, l1, l2], warmup=3, optimizers=[opt])
    times = {k: [] for k in steps}
    for _ in range(rounds):
        for k, gs in steps.items():
            for _ in range(3):
                gs(x, l1, l2)
            times[k].append(events_ms(lambda gs=gs: gs(x, l1, l2), iters))
    res = {f"step_{k}_ms": statistics.median(v) for k, v in times.items()}
    res.update({f"step_{k}_ms_all": v for k, v in times.items()})
    res["step_ratio_delta_ms"] = res["step_ratio_ms"] - res["step_mse_ms"]
    res["step_workload"] = "UNet_multitask(1, 1, 64) fp16, B=16, 512x512, graph-replayed, umi.optim.SGD"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="all", choices=("loss", "step", "all"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mt_ratio.py measures on the MI355X"
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
