#!/usr/bin/env python3
"""Times the pure-ViT TransUNet's patch gather and its training step on one MI355X, in one process, the variants alternating.

  kernels   umi_patch_rows (csrc/patch_embed.hip), fp32 NCHW image -> fp16 rows, at B = 24 @ 224 x 224 and B = 12 @ 512 x 512
            (C = 3, P = 16), next to a device-to-device copy that moves the same number of bytes (the gather reads 4 and writes 2
            bytes per element; the copy reads and writes 3 bytes per element of an int8 buffer).  Each variant is `--reps` calls
            captured into one HIP graph (the calls take microseconds: launched one by one from Python the window would time the
            host), a window is one replay between two device events; per variant the median of `--windows` windows, every
            variant warmed up first.  Consecutive calls of a graph rotate through `ring` sets of buffers, 1 GB in all, four
            times the 256 MB Infinity Cache, so every call reads from and writes to HBM.  Variants: "patch", "copy",
            "patch_again" (the gather a second time: the A/A measure of spread), and "patch_cached" / "copy_cached", which use
            one set of buffers for every call (a re-read from the cache: not an HBM rate, recorded to show the difference).
            `derived_us` = bytes over 5 TB/s, the expectation DESIGN.md section 3 derives (no measurement went into it);
            `gbps` = bytes over the measured time.
  steps     the fp16 training step (forward + dice_bce_mc + backward + fused SGD) of `ViT-B_16` (n_skip = 0) replayed from a HIP
            graph (umi.graphs.GraphedStep) at the same two shapes, next to `R50-ViT-B_16` in the same process for context: the
            median and every sample of windows of `--steps` replays, the slots "vit", "r50", "vit_again" alternating.

Prints one JSON line; --out writes it (profiles/vit_pure.json is the record README and DESIGN quote).  No GPU: fails.
"""
import argparse
import copy
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import torch  # noqa: E402

DEV = "cuda"
DERIVED_TBPS = 5.0
RING_BYTES = 1 << 30                                  # four times the 256 MB Infinity Cache
SHAPES = [(24, 224), (12, 512)]
C, P = 3, 16


def replay_ms(graph):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    graph.replay()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


def capture(fns, reps):
    """`reps` calls in one HIP graph, call i running fns[i % len(fns)]."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(reps):
            fns[i % len(fns)]()
    return g


def time_kernels(reps, windows):
    from umi import ops_tu
    rows = []
    for B, size in SHAPES:
        n, K = (size // P) ** 2, C * P * P
        nbytes = B * C * size * size * 4 + B * n * K * 2
        ring = RING_BYTES // nbytes + 1                  # buffer sets a graph rotates through: more bytes than the cache holds
        xs = [torch.randn(B, C, size, size, device=DEV) for _ in range(ring)]
        outs = [torch.empty(B * n, K, dtype=torch.float16, device=DEV) for _ in range(ring)]
        srcs = [torch.empty(nbytes // 2, dtype=torch.int8, device=DEV) for _ in range(ring)]
        dsts = [torch.empty(nbytes // 2, dtype=torch.int8, device=DEV) for _ in range(ring)]
        graphs = {"patch": capture([lambda x=x, o=o: ops_tu.patch_rows(x, P, o) for x, o in zip(xs, outs)], reps),
                  "copy": capture([lambda s=s, d=d: d.copy_(s) for s, d in zip(srcs, dsts)], reps),
                  # the same buffers every call: what a re-read from the Infinity Cache costs (not an HBM rate)
                  "patch_cached": capture([lambda: ops_tu.patch_rows(xs[0], P, outs[0])], reps),
                  "copy_cached": capture([lambda: dsts[0].copy_(srcs[0])], reps)}
        graphs["patch_again"] = graphs["patch"]
        for g in graphs.values():
            replay_ms(g)
        samples = {v: [] for v in graphs}
        for _ in range(windows):
            for v, g in graphs.items():                  # the variants alternate
                samples[v].append(replay_ms(g) * 1e3 / reps)
        us = {v: statistics.median(s) for v, s in samples.items()}
        rows.append({"B": B, "size": size, "tokens": B * n, "K": K, "bytes": nbytes, "ring": ring, "ring_bytes": ring * nbytes,
                     "derived_us": round(nbytes / (DERIVED_TBPS * 1e6), 2),
                     "patch_us": round(us["patch"], 2), "copy_us": round(us["copy"], 2), "patch_again_us": round(us["patch_again"], 2),
                     "patch_gbps": round(nbytes / us["patch"] / 1e3, 1), "copy_gbps": round(nbytes / us["copy"] / 1e3, 1),
                     "patch_over_copy": round(us["patch"] / us["copy"], 3),
                     "aa_spread": round(abs(us["patch_again"] / us["patch"] - 1.0), 4),
                     "patch_cached_us": round(us["patch_cached"], 2), "copy_cached_us": round(us["copy_cached"], 2),
                     "samples_us": {v: [round(t, 2) for t in s] for v, s in samples.items()}})
        del xs, outs, srcs, dsts, graphs
    return rows


def time_steps(batch, size, steps, warmup, windows):
    import loss as L
    from TransUnet.vit_seg_modeling import CONFIGS, VisionTransformer
    from umi import optim as umi_optim
    from umi.graphs import GraphedStep
    L.CLASS_NUMBER = 2
    torch.manual_seed(0)
    x = torch.randn(batch, 3, size, size, device=DEV)
    labels = torch.randint(0, 2, (batch, size, size), device=DEV).float()
    runs, first = {}, {}
    for slot, name in (("vit", "ViT-B_16"), ("r50", "R50-ViT-B_16")):
        cfg = copy.deepcopy(CONFIGS[name])
        cfg.n_classes = 2
        if slot == "vit":
            cfg.n_skip = 0
        else:
            cfg.n_skip, cfg.patches.grid = 3, (size // 16, size // 16)
        m = VisionTransformer(cfg, img_size=size, num_classes=2, compute_dtype="fp16").to(DEV).train()
        opt = umi_optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)

        def step(xx, yy, m=m, opt=opt):
            loss = L.calc_loss(m(xx), yy, loss_type="dice_bce_mc")
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss
        gs = GraphedStep(step, [x, labels], warmup=max(1, warmup))
        runs[slot] = lambda gs=gs: gs(x, labels)
        first[slot] = float(runs[slot]().item())
    torch.cuda.synchronize()
    slots = {"vit": runs["vit"], "r50": runs["r50"], "vit_again": runs["vit"]}
    samples = {s: [] for s in slots}
    for _ in range(windows):
        for s, fn in slots.items():
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(steps):
                fn()
            stop.record()
            torch.cuda.synchronize()
            samples[s].append(start.elapsed_time(stop) / steps)
    res = {s: {"median_ms": round(statistics.median(v), 3), "samples_ms": [round(t, 3) for t in v]} for s, v in samples.items()}
    for s in first:
        res[s]["loss_after_warmup"] = first[s]
    res["vit_images_per_s"] = round(batch / res["vit"]["median_ms"] * 1e3, 1)
    res["r50_images_per_s"] = round(batch / res["r50"]["median_ms"] * 1e3, 1)
    res["aa_spread"] = round(abs(res["vit_again"]["median_ms"] / res["vit"]["median_ms"] - 1.0), 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--reps", type=int, default=1000, help="gather / copy calls per captured graph (one timed window)")
    ap.add_argument("--windows", type=int, default=7, help="timed windows per variant / slot, alternating")
    ap.add_argument("--steps", type=int, default=5, help="graph replays per timed step window")
    ap.add_argument("--warmup", type=int, default=2, help="eager warm-up steps before the capture")
    ap.add_argument("--no-step", action="store_true", help="kernel timings only")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "vit_pure.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_vit: needs an MI355X (no device found); nothing is measured on the host")
    res = {"workload": "pure-ViT TransUNet (ViT-B_16, n_skip = 0): the patch gather per call, and the graph-replayed fp16 training step",
           "device": torch.cuda.get_device_name(0), "derived_at_tbps": DERIVED_TBPS, "reps_per_window": a.reps, "windows": a.windows,
           "kernels": time_kernels(a.reps, a.windows)}
    if not a.no_step:
        res["steps_per_window"] = a.steps
        res["steps"] = {f"batch {b} @ {s}x{s}": time_steps(b, s, a.steps, a.warmup, a.windows) for b, s in SHAPES}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
