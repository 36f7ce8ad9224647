"""Cost of the guarded optimizer step (umi.optim.GradGuard) on one MI355X: the U-Net step bench.py times and the TransUNet
R50-ViT-B/16 step at B=24, 224x224, each replayed from a HIP graph with the guard off and on.

    python tools/bench_grad_guard.py [--out profiles/grad_guard.json] [--rounds 6] [--steps 10] [--only unet|transunet]

Three copies of the step live in ONE process -- guard off (A), guard on, guard off (A', the A/A pair that gives the spread) -- and
are timed alternately, `--steps` replays per turn, `--rounds` turns each; the figure per variant is the median turn.  The
expectation the result is compared with: one extra read of the fp32 gradients at a streaming rate of 6 TB/s plus two kernel
boundaries of 2 us each."""
import argparse
import copy
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
from umi import optim as uo  # noqa: E402
from umi.graphs import GraphedStep  # noqa: E402

STREAM_TBS, BOUNDARY_US = 6.0, 2.0


def workloads():
    def unet():
        return Model.UNet(1, 2, 64, compute_dtype="fp16"), (16, 512)

    def transunet():
        from TransUnet.vit_seg_modeling import CONFIGS, VisionTransformer
        cfg = copy.deepcopy(CONFIGS["R50-ViT-B_16"])
        cfg.n_classes, cfg.n_skip, cfg.patches.grid = 2, 3, (224 // 16, 224 // 16)
        return VisionTransformer(cfg, img_size=224, num_classes=2, compute_dtype="fp16"), (24, 224)
    return {"unet": ("UNet(1,2,64) 16x512x512 fp16 (bench.py)", unet), "transunet": ("TransUNet R50-ViT-B/16 24x224x224 fp16", transunet)}


def build(make, guarded):
    torch.manual_seed(0)
    model, (B, size) = make()
    model = model.cuda().train()
    opt = uo.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    guard = None
    if guarded:
        guard = uo.GradGuard(max_norm=1.0, dynamic_scale=True)
        opt.grad_guard(guard)
        guard.attach(model)
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.randn(B, 1, size, size, device="cuda", generator=g)
    lab = torch.randint(0, 2, (B, size, size), device="cuda", generator=g).float()

    def step(xx, yy):
        loss = L.calc_loss(model(xx), yy, loss_type="dice_bce_mc")
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss
    gs = GraphedStep(step, [x, lab], warmup=3)                   # as bench.py captures it
    nbytes = 4 * sum(p.numel() for p in model.parameters() if p.requires_grad)
    return (lambda: gs(x, lab)), guard, nbytes, B


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "grad_guard.json"))
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--only", choices=["unet", "transunet"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_grad_guard.py needs an MI355X")
    L.CLASS_NUMBER = 2
    result = {"device": torch.cuda.get_device_name(0), "launch": "hipgraph", "rounds": a.rounds, "steps_per_turn": a.steps,
              "expectation": f"gradient bytes / {STREAM_TBS} TB/s + 2 x {BOUNDARY_US} us", "workloads": {}}
    for key, (label, make) in workloads().items():
        if a.only and key != a.only:
            continue
        variants = {"off_a": build(make, False), "on": build(make, True), "off_b": build(make, False)}
        turns = {k: [] for k in variants}
        for k, (run, _, _, _) in variants.items():              # the replays' own warm-up
            for _ in range(3):
                run()
        for _ in range(a.rounds):
            for k, (run, _, _, _) in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    run()
                torch.cuda.synchronize()
                turns[k].append((time.perf_counter() - t0) / a.steps * 1e3)
        med = {k: statistics.median(v) for k, v in turns.items()}
        off = statistics.median(turns["off_a"] + turns["off_b"])
        nbytes = variants["on"][2]
        expected_us = nbytes / (STREAM_TBS * 1e12) * 1e6 + 2 * BOUNDARY_US
        result["workloads"][key] = {
            "workload": label, "gradient_bytes": nbytes,
            "ms_per_step": {k: round(v, 4) for k, v in med.items()},
            "ms_per_step_turns": {k: [round(t, 4) for t in v] for k, v in turns.items()},
            "aa_spread_us": round(abs(med["off_a"] - med["off_b"]) * 1e3, 1),
            "guard_overhead_us": round((med["on"] - off) * 1e3, 1),
            "expected_overhead_us": round(expected_us, 1),
            "guard_state": variants["on"][1].read(),
        }
        print(json.dumps({key: result["workloads"][key]}), flush=True)
        del variants
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
