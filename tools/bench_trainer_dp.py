"""What Trainer(..., data_parallel=...) costs on one MI355X: the replica fingerprint pass, and a Trainer epoch in a world of one.

    python tools/bench_trainer_dp.py [--out profiles/trainer_data_parallel.json] [--windows 10] [--rounds 6] [--steps 30]
                                     [--only fingerprint|epoch]

fingerprint   umi_fingerprint_multi (umi.ddp.FingerprintPlan: the two launches, no read-back) over tensors of the parameter
              shapes of UNet(1,2,64) and of TransUNet R50-ViT-B/16, next to a device-to-device copy of the same number of bytes
              (the yardstick of profiles/vit_pure.json).  `reps` calls are captured into one HIP graph and rotate through a ring
              of parameter sets of more than 1 GB (four times the 256 MB Infinity Cache), so every pass reads HBM.  The pass reads
              each byte once and writes 8 bytes per 16 KB; the copy reads and writes each byte.  "fingerprint_again" replays the
              same graph: the A/A measure of spread.  "fingerprint_call_ms" is umi.ddp.fingerprint() as the Trainer calls it once
              per epoch: table upload, the two launches and the 8-byte read-back, on a host clock.
epoch         one Trainer epoch (`--steps` training steps and two validation steps, the checkpoint writes included) of
              UNet(1,2,64) at 16 x 512 x 512, fp16, graph=True: data_parallel=None (the path of the parent commit) against
              dict(world_size=1), and None again (A/A).  Three Trainers live in one process and take turns, one epoch a turn.

Scaling over eight GPUs and the latency of the collectives over xGMI cannot be measured on one MI355X and are NOT measured here."""
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

RING_BYTES = 1 << 30


def param_shapes():
    import Model
    from TransUnet.vit_seg_modeling import CONFIGS, VisionTransformer
    cfg = copy.deepcopy(CONFIGS["R50-ViT-B_16"])
    cfg.n_classes, cfg.n_skip, cfg.patches.grid = 2, 3, (224 // 16, 224 // 16)
    models = {"UNet(1,2,64)": lambda: Model.UNet(1, 2, 64),
              "TransUNet R50-ViT-B/16": lambda: VisionTransformer(cfg, img_size=224, num_classes=2)}
    return {k: [tuple(p.shape) for p in make().parameters()] for k, make in models.items()}


def replay_ms(graph):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    graph.replay()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop)


def capture(fns, reps):
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(reps):
            fns[i % len(fns)]()
    return g


def time_fingerprint(windows):
    from umi import ddp
    rows = {}
    for name, shapes in param_shapes().items():
        nbytes = 4 * sum(int(torch.Size(s).numel()) for s in shapes)
        ring = RING_BYTES // nbytes + 1
        reps = max(20, int(1e11 // nbytes))                       # about 100 GB read per window
        sets = [[torch.randn(s, device="cuda") for s in shapes] for _ in range(ring)]
        plans = [ddp.FingerprintPlan(ts) for ts in sets]
        srcs = [torch.empty(nbytes, dtype=torch.int8, device="cuda") for _ in range(ring)]
        dsts = [torch.empty(nbytes, dtype=torch.int8, device="cuda") for _ in range(ring)]
        graphs = {"fingerprint": capture([p.launch for p in plans], reps),
                  "copy": capture([lambda s=s, d=d: d.copy_(s) for s, d in zip(srcs, dsts)], reps)}
        graphs["fingerprint_again"] = graphs["fingerprint"]
        for g in graphs.values():
            replay_ms(g)
        samples = {v: [] for v in graphs}
        for _ in range(windows):
            for v, g in graphs.items():
                samples[v].append(replay_ms(g) * 1e3 / reps)
        us = {v: statistics.median(s) for v, s in samples.items()}
        calls = []
        for i in range(2 + windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            word = ddp.fingerprint(sets[i % ring])
            calls.append((time.perf_counter() - t0) * 1e3)
        assert word == plans[(1 + windows) % ring].word()      # (the graph's last write to that plan's word: the same bits)
        longer = us["fingerprint"] > us["copy"]
        rows[name] = {"tensors": len(shapes), "bytes": nbytes, "blocks": plans[0].blocks, "ring": ring, "reps_per_graph": reps,
                      "fingerprint_us": round(us["fingerprint"], 2), "copy_us": round(us["copy"], 2),
                      "fingerprint_again_us": round(us["fingerprint_again"], 2),
                      "fingerprint_read_gbps": round(nbytes / us["fingerprint"] / 1e3, 1),
                      "copy_gbps_read_plus_write": round(2 * nbytes / us["copy"] / 1e3, 1),
                      "fingerprint_over_copy": round(us["fingerprint"] / us["copy"], 3),
                      "fingerprint_takes_longer_than_the_copy": bool(longer),
                      "aa_spread": round(abs(us["fingerprint_again"] / us["fingerprint"] - 1.0), 4),
                      "fingerprint_call_ms": round(statistics.median(calls[2:]), 3),
                      "samples_us": {v: [round(t, 2) for t in s] for v, s in samples.items()}}
        print(json.dumps({name: {k: v for k, v in rows[name].items() if k != "samples_us"}}), flush=True)
        del sets, plans, srcs, dsts, graphs
        torch.cuda.empty_cache()
    return rows


def time_epoch(rounds, steps):
    import loss as L
    import Model
    from Trainer import Trainer
    from umi import optim as uo
    L.CLASS_NUMBER = 2
    B, S = 16, 512
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.randn(B, 1, S, S, device="cuda", generator=g)
    lab = torch.randint(0, 2, (B, S, S), device="cuda", generator=g).float()
    loaders = {"train": [(x, lab)] * steps, "val": [(x, lab)] * 2}
    tmp = tempfile.mkdtemp(prefix="bench_trainer_dp_")
    trainers = {}
    for name, dp in (("none_a", None), ("world_of_one", dict(world_size=1)), ("none_b", None)):
        torch.manual_seed(0)
        m = Model.UNet(1, 2, 64, compute_dtype="fp16").cuda()
        opt = uo.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        trainers[name] = Trainer(m, "single", torch.cuda.FloatTensor, "cuda", os.path.join(tmp, name), loaders, B, opt, 10 ** 6, 1,
                                 "dice_bce_mc", "dice_bce_mc", lr_scheduler=None, graph=True, data_parallel=dp)
    turns = {k: [] for k in trainers}
    for r in range(rounds + 1):                                   # round 0 warms up: first steps, captures, first writes
        for k, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.train()
            torch.cuda.synchronize()
            if r:
                turns[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in turns.items()}
    base = statistics.median(turns["none_a"] + turns["none_b"])
    row = {"workload": f"Trainer epoch, UNet(1,2,64) {B}x{S}x{S} fp16, graph=True, {steps} training + 2 validation steps, "
                       "checkpoint writes included",
           "rounds": rounds, "epoch_ms": {k: round(v, 2) for k, v in med.items()},
           "epoch_ms_fastest": {k: round(min(v), 2) for k, v in turns.items()},
           "epoch_ms_turns": {k: [round(t, 2) for t in v] for k, v in turns.items()},
           "aa_spread_ms": round(abs(med["none_a"] - med["none_b"]), 2),
           "world_of_one_minus_none_ms": round(med["world_of_one"] - base, 2),
           "world_of_one_over_none": round(med["world_of_one"] / base, 4),
           "graphs_replayed": {k: bool(tr._graphs) for k, tr in trainers.items()},
           "last_train_loss": {k: tr.train_loss_list[-1] for k, tr in trainers.items()}}
    print(json.dumps({"epoch": row}), flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trainer_data_parallel.json"))
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--only", choices=["fingerprint", "epoch"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_trainer_dp.py needs an MI355X")
    result = {"device": torch.cuda.get_device_name(0), "world": 1,
              "eight_gpu_scaling_and_xgmi_collectives": "not measured: one MI355X per machine"}
    if a.only != "epoch":
        result["fingerprint"] = time_fingerprint(a.windows)
    if a.only != "fingerprint":
        result["world_of_one_epoch"] = time_epoch(a.rounds, a.steps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
