"""Price of global-batch statistics (umi.ddp.GradReducer(global_batch=True)) on one MI355X, in a group of one: the U-Net step
bench.py times and the TransUNet R50-ViT-B/16 step at B=24, 224x224, run eagerly with the switch off and on.

    python tools/bench_global_batch.py [--out profiles/global_batch.json] [--rounds 10] [--steps 25] [--only unet|transunet]
                                       [--parent-lib PATH]

A group of one launches no collective, so on - off is the price of the extra launches alone: per BatchNorm layer the forward
runs rows -> sums, a fill of the count slot and finalize-from-sums instead of one finalize, the loss one launch more.  What
two or more ranks add -- an all-reduce of 2 C + 1 float64 values per BatchNorm layer each way, one of 3 C + 2 for the loss, and
one host read of the count per forward pass and per loss -- needs xGMI between GPUs and is unmeasured on hardware.

Four copies of the step live in ONE process -- switch off (A), switch on, switch off (A', the A/A pair that gives the spread)
and, with --parent-lib, switch off on another build of libunetmi (the parent commit's) -- and are timed alternately,
`--steps` steps per turn (about half a second), `--rounds` turns each; the figure per variant is the median turn, and the fastest
turn is given beside it: the eager steps are issued launch by launch from a host that other work shares, and a disturbed turn
(several ms on a 20 ms step) hits whichever variant is running."""
import argparse
import copy
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import torch  # noqa: E402
import loss as L  # noqa: E402
import Model  # noqa: E402
from umi import ddp, lib as ulib, optim as uo  # noqa: E402


def workloads():
    def unet():
        return Model.UNet(1, 2, 64, compute_dtype="fp16"), (16, 512, 1)

    def transunet():
        from TransUnet.vit_seg_modeling import CONFIGS, VisionTransformer
        cfg = copy.deepcopy(CONFIGS["R50-ViT-B_16"])
        cfg.n_classes, cfg.n_skip, cfg.patches.grid = 2, 3, (224 // 16, 224 // 16)
        return VisionTransformer(cfg, img_size=224, num_classes=2, compute_dtype="fp16"), (24, 224, 3)
    return {"unet": ("UNet(1,2,64) 16x512x512 fp16 (bench.py), eager", unet),
            "transunet": ("TransUNet R50-ViT-B/16 24x224x224 fp16, eager", transunet)}


def other_build(path):
    """Another build of libunetmi with the header's signatures on every symbol it has."""
    cdll = ctypes.CDLL(path)
    for name, (res, args) in ulib.SIGNATURES.items():
        fn = getattr(cdll, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    return cdll


def build(make, on, cdll):
    torch.manual_seed(0)
    model, (B, size, cin) = make()
    model = model.cuda().train()
    red = ddp.GradReducer(model, 1, global_batch=on)
    opt = uo.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.randn(B, cin, size, size, device="cuda", generator=g)
    lab = torch.randint(0, 2, (B, size, size), device="cuda", generator=g).float()
    n_bn = sum(isinstance(m, torch.nn.BatchNorm2d) for m in model.modules())

    def step():
        ddp.set_active_batch_sync(red.batch_sync)                  # the loss's side of the switch is per process
        ulib._lib = cdll
        loss = L.calc_loss(model(x), lab, loss_type="dice_bce_mc")
        opt.zero_grad()
        loss.backward()
        red.sync()
        opt.step()
        return loss
    return step, n_bn, B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "global_batch.json"))
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--only", choices=["unet", "transunet"])
    ap.add_argument("--parent-lib", help="a build of libunetmi from the parent commit: timed with the switch off as a fourth variant")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_global_batch.py needs an MI355X")
    L.CLASS_NUMBER = 2
    own = ulib._lib
    parent = other_build(a.parent_lib) if a.parent_lib else None
    result = {"device": torch.cuda.get_device_name(0), "launch": "eager", "world": 1, "rounds": a.rounds, "steps_per_turn": a.steps,
              "collectives_over_xgmi": "unmeasured on hardware (one GPU per box)", "workloads": {}}
    for key, (label, make) in workloads().items():
        if a.only and key != a.only:
            continue
        variants = {"off_a": build(make, False, own), "on": build(make, True, own), "off_b": build(make, False, own)}
        if parent is not None:
            variants["off_parent_lib"] = build(make, False, parent)
        turns = {k: [] for k in variants}
        losses = {}
        for k, (run, _, _) in variants.items():
            for _ in range(3):
                losses[k] = run()
        for _ in range(a.rounds):
            for k, (run, _, _) in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    run()
                torch.cuda.synchronize()
                turns[k].append((time.perf_counter() - t0) / a.steps * 1e3)
        med = {k: statistics.median(v) for k, v in turns.items()}
        best = {k: min(v) for k, v in turns.items()}
        off = statistics.median(turns["off_a"] + turns["off_b"])
        row = {"workload": label, "batchnorm_layers": variants["on"][1],
               "ms_per_step": {k: round(v, 4) for k, v in med.items()},
               "ms_per_step_fastest_turn": {k: round(v, 4) for k, v in best.items()},
               "ms_per_step_turns": {k: [round(t, 4) for t in v] for k, v in turns.items()},
               "aa_spread_us": round(abs(med["off_a"] - med["off_b"]) * 1e3, 1),
               "switch_on_overhead_us": round((med["on"] - off) * 1e3, 1),
               "switch_on_overhead_us_fastest_turns": round((best["on"] - min(best["off_a"], best["off_b"])) * 1e3, 1),
               # (equal for a model without dropout; every copy of a model with dropout draws its own mask seed)
               "loss_after_warmup": {k: float(v.detach()) for k, v in losses.items()}}
        if parent is not None:
            row["off_minus_parent_lib_us"] = round((off - med["off_parent_lib"]) * 1e3, 1)
        result["workloads"][key] = row
        print(json.dumps({key: row}), flush=True)
        del variants
        ulib._lib = own
        ddp.set_active_batch_sync(None)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
