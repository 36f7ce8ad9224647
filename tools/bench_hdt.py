#!/usr/bin/env python3
"""Times HausdorffDTLoss (csrc/hausdorff_dt.hip) on one MI355X with device events after warm-up:

  loss : forward + backward of the loss alone at (16, 1, 512, 512) (module call + autograd), and the two C entry points
         (umi_hdt_fwd, umi_hdt_bwd) on their own;
  step : a graph-replayed UNet(1, 1, 64) fp16 training step (forward + loss + backward + umi.optim.SGD) at B=16, 512x512,
         with loss 'HausdorffDTLoss' against 'BCE', alternated over several rounds on the same box.

Prints one JSON line and writes it to --out if given.
Usage:  python tools/bench_hdt.py [--only loss|step|all] [--iters 50] [--rounds 3] [--out profiles/hdt_bench.json]
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
    x = F.avg_pool2d(torch.randn(B, 1, H + 8, W + 8, device=DEV, generator=g), 9, stride=1) * 9.0
    t = (F.avg_pool2d(torch.randn(B, 1, H + 8, W + 8, device=DEV, generator=g), 9, stride=1) * 9.0 > 1.0).float()
    return x.contiguous(), t.contiguous()


def bench_loss(iters, rounds):
    import loss as L
    from umi import lib, ops
    B, H, W = 16, 512, 512
    x, t = inputs(B, H, W)
    x.requires_grad_(True)
    mod = L.HausdorffDTLoss()

    def fwd_bwd():
        x.grad = None
        mod(x, t).backward()

    D = torch.empty_like(x)
    loss = torch.empty((), device=DEV)
    ws = ops.workspace(lib.fn("umi_hdt_ws_bytes")(B, H, W), x.device)
    g = torch.ones((), device=DEV)
    dx = torch.empty_like(x)
    st = ops._stream()

    def fwd():
        lib.check(lib.fn("umi_hdt_fwd")(x.data_ptr(), t.data_ptr(), B, 1, H, W, 0.2, D.data_ptr(), None, loss.data_ptr(),
                                        ws.data_ptr(), ws.numel(), st), "umi_hdt_fwd")

    def bwd():
        lib.check(lib.fn("umi_hdt_bwd")(x.data_ptr(), t.data_ptr(), D.data_ptr(), g.data_ptr(), B, 1, H, W, dx.data_ptr(),
                                        st), "umi_hdt_bwd")

    res = {}
    for name, fn in (("loss_fwd_bwd_ms", fwd_bwd), ("umi_hdt_fwd_ms", fwd), ("umi_hdt_bwd_ms", bwd)):
        for _ in range(5):
            fn()
        res[name] = statistics.median(events_ms(fn, iters) for _ in range(rounds))
    N = B * H * W
    # compulsory HBM bytes: fwd reads pred + target twice (column pass, loss partial), writes and re-reads the 2 x 4-byte
    # column tables, writes D; bwd reads pred, target, D and writes dpred
    res["bytes_fwd"] = N * (8 + 8 + 8 + 8 + 4)
    res["bytes_bwd"] = N * 16
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
    for loss_type, lab in (("BCE", t[:, 0].contiguous()), ("HausdorffDTLoss", t)):
        torch.manual_seed(0)
        m = Model.UNet(1, 1, 64, compute_dtype="fp16").to(DEV).train()
        opt = uo.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)

        def body(xx, yy, m=m, opt=opt, loss_type=loss_type):
            loss = L.calc_loss(m(xx), yy, loss_type=loss_type)
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss.detach()
        gs = GraphedStep(body, [x, lab], warmup=3, optimizers=[opt])
        steps[loss_type] = (gs, lab)
    times = {k: [] for k in steps}
    for _ in range(rounds):                                   # alternate the two on the same box
        for k, (gs, lab) in steps.items():
            for _ in range(3):
                gs(x, lab)
            times[k].append(events_ms(lambda gs=gs, lab=lab: gs(x, lab), iters))
    res = {f"step_{k}_ms": statistics.median(v) for k, v in times.items()}
    res.update({f"step_{k}_ms_all": v for k, v in times.items()})
    res["step_delta_ms"] = res["step_HausdorffDTLoss_ms"] - res["step_BCE_ms"]
    res["step_workload"] = "UNet(1, 1, 64) fp16, B=16, 512x512, graph-replayed, umi.optim.SGD"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="all", choices=("loss", "step", "all"))
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_hdt.py measures on the MI355X"
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
