"""What umi.optim.AdamW and the device learning-rate schedule cost on one MI355X.

    python tools/bench_adamw.py [--out profiles/adamw.json] [--windows 10] [--rounds 5] [--steps 20] [--only update|step]

One process, the variants take turns round by round, medians are reported, and every comparison has its A/A pair (the same graph
or the same configuration measured twice), as the repository's other bench tools do.

update  `optimizer.step()` on the device block over tensors of the parameter shapes of UNet(1,2,64) and of TransUNet
        R50-ViT-B/16, gradients and moments included: 28 B per parameter (p, g, exp_avg, exp_avg_sq read; p and the two moments
        written).  `reps` steps captured into one HIP graph rotate through a ring of parameter sets of more than 1 GB, so every
        pass reads HBM.  Variants: umi.optim.AdamW, umi.optim.Adam with the same (L2) weight decay -- the same bytes, so the
        expected ratio is 1 within the A/A spread --, AdamW again (A/A), and AdamW with a cosine schedule installed: the
        difference to plain AdamW is what umi_optim_hyper_schedule (one thread, one launch per param group) adds behind the step.
        The variants of a set update the same p, g and moment tensors, so placement in HBM cancels out of the comparison.
step    Trainer.train_step of TransUNet R50-ViT-B/16 at B = 24, 224 x 224, fp16, AdamW over decay_groups with
        lr_schedule=dict(kind='cosine', warmup=10): umi.optim.AdamW with graph=True (twice: A/A), umi.optim.AdamW eager, and
        torch.optim.AdamW(foreach=True) eager with the schedule applied on the host -- what a user had before.

No threshold is set on these times.  Scaling over several GPUs is NOT measured here."""
import argparse
import copy
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import torch  # noqa: E402

from tools.bench_trainer_dp import RING_BYTES, capture, param_shapes, replay_ms  # noqa: E402


def _median_rounds(graphs, windows, reps):
    for g in graphs.values():
        replay_ms(g)
    samples = {v: [] for v in graphs}
    for _ in range(windows):
        for v, g in graphs.items():
            samples[v].append(replay_ms(g) * 1e3 / reps)
    return {v: statistics.median(s) for v, s in samples.items()}, samples


def time_update(windows):
    from umi import optim as uo
    rows = {}
    kw = dict(lr=1e-3, weight_decay=1e-2)
    sched = dict(kind="cosine", warmup=10, max_iterations=10 ** 6)
    for name, shapes in param_shapes().items():
        n = sum(int(torch.Size(s).numel()) for s in shapes)
        ring = RING_BYTES // (16 * n) + 1                          # p, g and the two moments per set
        reps = max(20, int(5e10 // (28 * n)))
        reps -= reps % ring                                        # every set the same number of times
        sets = [[torch.randn(s, device="cuda").requires_grad_(True) for s in shapes] for _ in range(ring)]
        for ts in sets:
            for p in ts:
                p.grad = torch.randn_like(p) * 1e-3
        opts = {"adamw": [uo.AdamW(ts, **kw).device_schedule() for ts in sets],
                "adam_l2": [uo.Adam(ts, **kw).device_schedule() for ts in sets],
                "adamw_schedule": [uo.AdamW(ts, **kw).device_schedule(schedule=sched) for ts in sets]}
        # the variants of a set share p and g; after their first step they share the moment tensors as well, so that every
        # variant streams the SAME addresses (two allocations of equal size differ by several per cent in this pass)
        for os_ in opts.values():
            for o in os_:
                o.step()
        for v in ("adam_l2", "adamw_schedule"):
            for o, first in zip(opts[v], opts["adamw"]):
                for p in o.param_groups[0]["params"]:
                    o.state[p]["exp_avg"], o.state[p]["exp_avg_sq"] = first.state[p]["exp_avg"], first.state[p]["exp_avg_sq"]
        graphs = {v: capture([o.step for o in os_], reps) for v, os_ in opts.items()}
        graphs["adamw_again"] = graphs["adamw"]
        us, samples = _median_rounds(graphs, windows, reps)
        aa = abs(us["adamw_again"] / us["adamw"] - 1.0)
        ratio = us["adamw"] / us["adam_l2"]
        row = {"tensors": len(shapes), "parameters": n, "bytes_moved_per_step": 28 * n, "param_groups": 1, "ring": ring,
               "variants_share_tensors": True, "reps_per_graph": reps, "step_us": {k: round(v, 2) for k, v in us.items()},
               "adamw_gbps": round(28 * n / us["adamw"] / 1e3, 1), "adamw_over_adam_l2": round(ratio, 4),
               "aa_spread": round(aa, 4), "ratio_outside_aa_spread": bool(abs(ratio - 1.0) > aa),
               "schedule_kernel_adds_us": round(us["adamw_schedule"] - us["adamw"], 2),
               "aa_spread_us": round(abs(us["adamw_again"] - us["adamw"]), 2),
               "samples_us": {v: [round(t, 2) for t in s] for v, s in samples.items()}}
        rows[name] = row
        print(json.dumps({name: {k: v for k, v in row.items() if k != "samples_us"}}), flush=True)
        del graphs, opts, sets
        torch.cuda.empty_cache()
    return rows


def time_step(rounds, steps, batch=24, size=224):
    import loss as L
    from Trainer import Trainer
    from TransUnet.vit_seg_modeling import CONFIGS, VisionTransformer
    from umi import optim as uo
    cfg = copy.deepcopy(CONFIGS["R50-ViT-B_16"])
    cfg.n_classes, cfg.n_skip, cfg.patches.grid = 2, 3, (size // 16, size // 16)
    L.CLASS_NUMBER = 2
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.randn(batch, 1, size, size, device="cuda", generator=g)
    lab = torch.randint(0, 2, (batch, size, size), device="cuda", generator=g).float()
    tmp = tempfile.mkdtemp(prefix="bench_adamw_step_")
    variants = [("umi_graph_a", uo.AdamW, {}, True), ("umi_eager", uo.AdamW, {}, False),
                ("torch_foreach_eager", torch.optim.AdamW, dict(foreach=True), False), ("umi_graph_b", uo.AdamW, {}, True)]
    trainers = {}
    for name, cls, okw, graph in variants:
        torch.manual_seed(0)
        m = VisionTransformer(cfg, img_size=size, num_classes=2, compute_dtype="fp16").cuda()
        opt = cls(uo.decay_groups(m, 1e-2), lr=1e-3, **okw)
        trainers[name] = Trainer(m, "TransUnet", torch.cuda.FloatTensor, "cuda", os.path.join(tmp, name),
                                 {"train": [(x, lab)] * steps, "val": []}, batch, opt, 10 ** 6, 10 ** 4, "dice_bce_mc",
                                 "dice_bce_mc", graph=graph, lr_schedule=dict(kind="cosine", warmup=10))
    ms = {k: [] for k in trainers}
    for r in range(rounds + 1):                                   # round 0: the eager first step, the capture
        for k, tr in trainers.items():
            tr.model.train()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.train_step(x, lab)
            torch.cuda.synchronize()
            if r:
                ms[k].append((time.perf_counter() - t0) * 1e3 / steps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    graph_ms = statistics.median(ms["umi_graph_a"] + ms["umi_graph_b"])
    row = {"workload": f"Trainer.train_step, TransUNet R50-ViT-B/16 {batch}x{size}x{size} fp16, AdamW over decay_groups, cosine "
                       f"schedule with warm-up; {steps} steps per turn",
           "rounds": rounds, "step_ms": {k: round(v, 3) for k, v in med.items()},
           "step_ms_turns": {k: [round(t, 3) for t in v] for k, v in ms.items()},
           "aa_spread_ms": round(abs(med["umi_graph_a"] - med["umi_graph_b"]), 3), "umi_graph_ms": round(graph_ms, 3),
           "umi_eager_minus_graph_ms": round(med["umi_eager"] - graph_ms, 3),
           "torch_foreach_eager_minus_graph_ms": round(med["torch_foreach_eager"] - graph_ms, 3),
           "graphs_captured": {k: len(tr._graphs) for k, tr in trainers.items()},
           "iterations": {k: tr.iter_num for k, tr in trainers.items()}}
    print(json.dumps({"step": row}), flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "adamw.json"))
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--only", choices=["update", "step"], action="append")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_adamw.py needs an MI355X")
    want = set(a.only or ["update", "step"])
    result = {"device": torch.cuda.get_device_name(0), "scaling_over_several_gpus": "not measured",
              "update": "not measured", "step": "not measured"}
    if "update" in want:
        result["update"] = time_update(a.windows)
    if "step" in want:
        result["step"] = time_step(a.rounds, a.steps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
