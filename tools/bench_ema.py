"""What the weight average (umi.ema) costs on one MI355X.

    python tools/bench_ema.py [--out profiles/ema.json] [--windows 10] [--rounds 6] [--steps 30] [--only update|swap|step|epoch|abi]
                              [--parent-lib PATH/libunetmi.so] [--parent-trainer PATH/Trainer.py] [--label TEXT]

One process, the variants take turns round by round, medians are reported, and every comparison has its A/A pair (the same graph
or the same configuration measured twice), as the repository's other bench tools do.

update  ModelEMA.update() (umi_ema_pre + umi_ema_multi) over tensors of the parameter shapes of UNet(1,2,64) and of TransUNet
        R50-ViT-B/16.  It moves 12 B per parameter (p and the shadow read, the shadow written), so it stands next to ONE
        device-to-device copy that moves the same bytes (a buffer of 6 B per parameter: read once, written once) and next to
        umi.snapshot.Snapshot.take() on the same tensors (8 B per parameter).
          cold  `reps` calls captured into one HIP graph rotate through a ring of parameter sets of more than 1 GB: every pass
                reads HBM.
          hot   right after an optimizer step on ONE parameter set: a graph of `reps` x (umi.optim.SGD.step) against a graph of
                `reps` x (step + update); the difference per repetition is what the update adds behind a step that has just
                written p.
swap    ModelEMA.swap() alone (16 B per parameter), timed with events over the ring.
step    Trainer.train_step of the benchmark's U-Net step (UNet(1,2,64), B = 16, 512 x 512, fp16, graph=True, replayed) with `ema`
        off, off again (A/A) and on.
epoch   Trainer epochs of tools/bench_trainer_dp.py's setting (`--steps` training and two validation steps, checkpoint writes
        included) with `ema` off twice, on (validating: two swaps and an averaged best model per epoch), and -- with
        --parent-trainer -- the Trainer of the parent commit beside them.
abi     with --parent-lib: umi_optim_sgd_multi and umi_snapshot_multi of that library against this commit's, same tables, same
        process, alternating (this commit touches neither kernel).

The cache policy of the kernels is a compile-time choice (UMI_EMA_POLICY in csrc/ema.hip); `--label` names the build that ran,
a build of another policy is measured by running this tool with UMI_LIB_OVERRIDE pointing at it.
Scaling over several GPUs is NOT measured here."""
import argparse
import ctypes
import importlib.util
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
    from umi.ema import ModelEMA
    from umi.snapshot import Snapshot
    rows = {}
    for name, shapes in param_shapes().items():
        n = sum(int(torch.Size(s).numel()) for s in shapes)
        ring = RING_BYTES // (8 * n) + 1                           # p and its shadow per set
        reps = max(20, int(5e10 // (12 * n)))
        sets = [[torch.randn(s, device="cuda").requires_grad_(True) for s in shapes] for _ in range(ring)]
        emas = [ModelEMA(ts, decay=0.999, warmup=False) for ts in sets]
        snaps = [Snapshot(ts) for ts in sets]
        srcs = [torch.empty(6 * n, dtype=torch.int8, device="cuda") for _ in range(ring)]
        dsts = [torch.empty(6 * n, dtype=torch.int8, device="cuda") for _ in range(ring)]
        graphs = {"update": capture([e.update for e in emas], reps),
                  "copy_12B": capture([lambda s=s, d=d: d.copy_(s) for s, d in zip(srcs, dsts)], reps),
                  "snapshot_take": capture([s.take for s in snaps], reps)}
        graphs["update_again"] = graphs["update"]
        us, samples = _median_rounds(graphs, windows, reps)
        row = {"tensors": len(shapes), "parameters": n, "bytes_moved_per_update": 12 * n, "launches_per_update": 2, "ring": ring,
               "reps_per_graph": reps, "cold_us": {k: round(v, 2) for k, v in us.items()},
               "cold_update_gbps": round(12 * n / us["update"] / 1e3, 1), "cold_copy_gbps": round(12 * n / us["copy_12B"] / 1e3, 1),
               "cold_update_over_copy": round(us["update"] / us["copy_12B"], 3),
               "cold_aa_spread": round(abs(us["update_again"] / us["update"] - 1.0), 4),
               "cold_samples_us": {v: [round(t, 2) for t in s] for v, s in samples.items()}}
        del graphs, snaps, srcs, dsts, emas, sets
        torch.cuda.empty_cache()
        # hot: behind an optimizer step on one parameter set
        ps = [torch.randn(s, device="cuda").requires_grad_(True) for s in shapes]
        for p in ps:
            p.grad = torch.randn_like(p) * 1e-3
        opt = uo.SGD(ps, lr=1e-3, momentum=0.9)
        ema = ModelEMA(ps, decay=0.999, warmup=False)
        opt.step()
        ema.update()
        hot_reps = 50

        def both():
            opt.step()
            ema.update()
        graphs = {"step": capture([opt.step], hot_reps), "step_update": capture([both], hot_reps)}
        graphs["step_again"] = graphs["step"]
        us, samples = _median_rounds(graphs, windows, hot_reps)
        row.update({"hot_us": {k: round(v, 2) for k, v in us.items()}, "hot_update_adds_us": round(us["step_update"] - us["step"], 2),
                    "hot_aa_spread_us": round(abs(us["step_again"] - us["step"]), 2),
                    "hot_working_set_bytes": 16 * n,
                    "hot_samples_us": {v: [round(t, 2) for t in s] for v, s in samples.items()}})
        rows[name] = row
        print(json.dumps({name: {k: v for k, v in row.items() if not k.endswith("samples_us")}}), flush=True)
        del graphs, opt, ema, ps
        torch.cuda.empty_cache()
    return rows


def time_swap(windows):
    from umi.ema import ModelEMA
    rows = {}
    for name, shapes in param_shapes().items():
        n = sum(int(torch.Size(s).numel()) for s in shapes)
        ring = RING_BYTES // (8 * n) + 1
        emas = [ModelEMA([torch.randn(s, device="cuda").requires_grad_(True) for s in shapes]) for _ in range(ring)]
        for e in emas:
            e.swap()
        times = []
        for w in range(windows + 1):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for e in emas:
                e.swap()
            stop.record()
            torch.cuda.synchronize()
            if w:
                times.append(start.elapsed_time(stop) * 1e3 / ring)
        us = statistics.median(times)
        rows[name] = {"parameters": n, "bytes_moved": 16 * n, "swap_us": round(us, 2), "gbps": round(16 * n / us / 1e3, 1),
                      "samples_us": [round(t, 2) for t in times]}
        print(json.dumps({name: {"swap_us": rows[name]["swap_us"], "gbps": rows[name]["gbps"]}}), flush=True)
        del emas
        torch.cuda.empty_cache()
    return rows


def _parent_trainer(path):
    spec = importlib.util.spec_from_file_location("Trainer_parent", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Trainer


def _trainers(variants, loaders, epochs, tmp):
    import loss as L
    import Model
    from umi import optim as uo
    L.CLASS_NUMBER = 2
    out = {}
    for name, cls, flags in variants:
        torch.manual_seed(0)
        m = Model.UNet(1, 2, 64, compute_dtype="fp16").cuda()
        opt = uo.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        out[name] = cls(m, "single", torch.cuda.FloatTensor, "cuda", os.path.join(tmp, name), loaders, 16, opt, 10 ** 6, epochs,
                        "dice_bce_mc", "dice_bce_mc", lr_scheduler=None, graph=True, **flags)
    return out


def _batch():
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.randn(16, 1, 512, 512, device="cuda", generator=g)
    return x, torch.randint(0, 2, (16, 512, 512), device="cuda", generator=g).float()


def time_step(rounds, steps):
    from Trainer import Trainer
    x, lab = _batch()
    tmp = tempfile.mkdtemp(prefix="bench_ema_step_")
    trainers = _trainers([("off_a", Trainer, {}), ("ema", Trainer, dict(ema=dict(decay=0.999))), ("off_b", Trainer, {})],
                         {"train": [(x, lab)] * steps, "val": []}, 1, tmp)
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
    base = statistics.median(ms["off_a"] + ms["off_b"])
    aa = abs(med["off_a"] - med["off_b"])
    row = {"workload": f"Trainer.train_step, UNet(1,2,64) 16x512x512 fp16, graph=True, replayed; {steps} steps per turn",
           "rounds": rounds, "step_ms": {k: round(v, 3) for k, v in med.items()},
           "step_ms_turns": {k: [round(t, 3) for t in v] for k, v in ms.items()}, "aa_spread_ms": round(aa, 3),
           "ema_minus_off_ms": round(med["ema"] - base, 3), "ema_minus_off_percent": round(100 * (med["ema"] - base) / base, 2),
           "outside_aa_spread": bool(abs(med["ema"] - base) > aa), "updates": trainers["ema"].ema.sync_host()["updates"]}
    print(json.dumps({"step": row}), flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
    return row


def time_epoch(rounds, steps, epochs, parent):
    from Trainer import Trainer
    x, lab = _batch()
    tmp = tempfile.mkdtemp(prefix="bench_ema_epoch_")
    variants = [("off_a", Trainer, {})]
    if parent:
        variants.append(("parent", _parent_trainer(parent), {}))
    variants += [("ema", Trainer, dict(ema=dict(decay=0.999))), ("off_b", Trainer, {})]
    trainers = _trainers(variants, {"train": [(x, lab)] * steps, "val": [(x, lab)] * 2}, epochs, tmp)
    turns = {k: [] for k in trainers}
    for r in range(rounds + 1):
        for k, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.train()
            torch.cuda.synchronize()
            if r:
                turns[k].append((time.perf_counter() - t0) * 1e3 / epochs)
    med = {k: statistics.median(v) for k, v in turns.items()}
    base = statistics.median(turns["off_a"] + turns["off_b"])
    aa = abs(med["off_a"] - med["off_b"])
    row = {"workload": f"Trainer epoch, UNet(1,2,64) 16x512x512 fp16, graph=True, {steps} training + 2 validation steps, checkpoint "
                       f"writes included; a turn is one train() of {epochs} epochs, figures are per epoch",
           "rounds": rounds, "epoch_ms": {k: round(v, 2) for k, v in med.items()},
           "epoch_ms_turns": {k: [round(t, 2) for t in v] for k, v in turns.items()}, "aa_spread_ms": round(aa, 2),
           "ema_minus_off_ms": round(med["ema"] - base, 2)}
    if parent:
        row["off_minus_parent_ms"] = round(base - med["parent"], 2)
        row["flag_off_inside_aa_spread_of_parent"] = bool(abs(base - med["parent"]) <= max(aa, 0.005 * base))
        row["flag_off_rule"] = "|off - parent| <= max(A/A spread, 0.5 % of the epoch)"
    print(json.dumps({"epoch": row}), flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
    return row


def time_abi(windows, parent_lib):
    """The parent commit's entry points against this commit's on the same tables."""
    import numpy as np
    from umi import lib as L, ops
    from umi.snapshot import Snapshot
    theirs = ctypes.CDLL(parent_lib)
    for fn in ("umi_optim_sgd_multi", "umi_snapshot_multi"):
        getattr(theirs, fn).restype, getattr(theirs, fn).argtypes = L.SIGNATURES[fn]
    shapes = param_shapes()["UNet(1,2,64)"]
    n = sum(int(torch.Size(s).numel()) for s in shapes)
    ps = [torch.randn(s, device="cuda") for s in shapes]
    gs, ms = [torch.randn_like(p) * 1e-3 for p in ps], [torch.zeros_like(p) for p in ps]
    blk = L.fn("umi_optim_block_elems")()
    arr, b0 = np.zeros(len(ps), dtype=ops.OPTIM_DESC), 0
    for i, (p, g, m) in enumerate(zip(ps, gs, ms)):
        arr[i] = (p.data_ptr(), g.data_ptr(), m.data_ptr(), 0, p.numel(), b0, 0)
        b0 += (p.numel() + blk - 1) // blk
    table = torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).cuda()
    snap = Snapshot(ps)
    reps = 50

    def sgd(lib):
        return lambda: lib.umi_optim_sgd_multi(table.data_ptr(), len(ps), b0, 1e-3, 0.9, 0.0, 1e-4, 0, 0, ops._stream())

    def take(lib):
        return lambda: lib.umi_snapshot_multi(snap.table.data_ptr(), len(ps), snap.blocks, snap.ws.data_ptr(), snap.ws.numel() * 8,
                                              snap.out.data_ptr(), ops._stream())
    graphs = {"sgd_this": capture([sgd(L.lib)], reps), "sgd_parent": capture([sgd(theirs)], reps),
              "snapshot_this": capture([take(L.lib)], reps), "snapshot_parent": capture([take(theirs)], reps)}
    graphs["sgd_this_again"] = graphs["sgd_this"]
    us, samples = _median_rounds(graphs, windows, reps)
    row = {"tensors": "UNet(1,2,64) parameters, one set (hot)", "parameters": n, "us": {k: round(v, 2) for k, v in us.items()},
           "aa_spread": round(abs(us["sgd_this_again"] / us["sgd_this"] - 1.0), 4),
           "sgd_this_over_parent": round(us["sgd_this"] / us["sgd_parent"], 4),
           "snapshot_this_over_parent": round(us["snapshot_this"] / us["snapshot_parent"], 4)}
    print(json.dumps({"abi": row}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ema.json"))
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--only", choices=["update", "swap", "step", "epoch", "abi"], action="append")
    ap.add_argument("--parent-lib", help="libunetmi.so of the parent commit")
    ap.add_argument("--parent-trainer", help="Trainer.py of the parent commit, measured beside this one's")
    ap.add_argument("--label", default="", help="names the build that ran (the cache policy of csrc/ema.hip)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ema.py needs an MI355X")
    want = set(a.only or ["update", "swap", "step", "epoch", "abi"])
    result = {"device": torch.cuda.get_device_name(0), "build": a.label, "scaling_over_several_gpus": "not measured"}
    if "update" in want:
        result["update"] = time_update(a.windows)
    if "swap" in want:
        result["swap"] = time_swap(a.windows)
    if "abi" in want and a.parent_lib:
        result["abi"] = time_abi(a.windows, a.parent_lib)
    if "step" in want:
        result["step"] = time_step(a.rounds, a.steps)
    if "epoch" in want:
        result["epoch"] = time_epoch(a.rounds, a.steps, a.epochs, a.parent_trainer)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
