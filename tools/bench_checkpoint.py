"""What the state snapshot costs on one MI355X, and what asynchronous checkpoints give back to a Trainer epoch.

    python tools/bench_checkpoint.py [--out profiles/checkpoint_snapshot.json] [--windows 10] [--rounds 6] [--steps 30]
                                     [--epochs 3] [--only snapshot|epoch] [--parent PATH/Trainer.py]

snapshot   umi.snapshot.Snapshot.take() (umi_snapshot_multi: the copy with its block partials, then the finalize pass; no
           read-back) over tensors of the parameter shapes of UNet(1,2,64) and of TransUNet R50-ViT-B/16, next to ONE
           device-to-device copy of the same number of bytes.  As in tools/bench_trainer_dp.py, `reps` calls are captured into one
           HIP graph and rotate through a ring of parameter sets of more than 1 GB, so every pass reads HBM; "take_again" replays
           the same graph (the A/A spread).  Both passes read and write each byte once.
epoch      Trainer epochs of tools/bench_trainer_dp.py's setting (UNet(1,2,64) at 16 x 512 x 512, fp16, graph=True, `--steps`
           training and two validation steps per epoch, checkpoint writes included): both flags off twice (A/A), the Trainer of
           another commit when `--parent` names its file (loaded beside this one; the library is this commit's),
           async_checkpoints=True, and async_checkpoints=True with resume=True.  The Trainers live in one process and take turns;
           a turn is one train() of `--epochs` epochs, so the files of every epoch but the last are written beside the next
           epoch's steps, and the time train() spends joining the writer at its end is reported on its own ("join_ms").

Scaling over several GPUs is NOT measured here."""
import argparse
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


def time_snapshot(windows):
    from umi.snapshot import Snapshot
    rows = {}
    for name, shapes in param_shapes().items():
        nbytes = 4 * sum(int(torch.Size(s).numel()) for s in shapes)
        ring = RING_BYTES // nbytes + 1
        reps = max(20, int(5e10 // nbytes))                       # about 50 GB read and 50 GB written per window
        sets = [[torch.randn(s, device="cuda") for s in shapes] for _ in range(ring)]
        snaps = [Snapshot(ts) for ts in sets]
        srcs = [torch.empty(nbytes, dtype=torch.int8, device="cuda") for _ in range(ring)]
        dsts = [torch.empty(nbytes, dtype=torch.int8, device="cuda") for _ in range(ring)]
        graphs = {"take": capture([s.take for s in snaps], reps),
                  "copy": capture([lambda s=s, d=d: d.copy_(s) for s, d in zip(srcs, dsts)], reps)}
        graphs["take_again"] = graphs["take"]
        for g in graphs.values():
            replay_ms(g)
        samples = {v: [] for v in graphs}
        for _ in range(windows):
            for v, g in graphs.items():
                samples[v].append(replay_ms(g) * 1e3 / reps)
        us = {v: statistics.median(s) for v, s in samples.items()}
        assert snaps[0].verify() and torch.equal(snaps[0].views()[0], sets[0][0])
        restore = []
        for i in range(2 + windows):                              # restore(): verify (a fingerprint pass, 16 bytes read back), copy
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            snaps[i % ring].restore()
            torch.cuda.synchronize()
            restore.append((time.perf_counter() - t0) * 1e3)
        rows[name] = {"tensors": len(shapes), "bytes": nbytes, "arena_bytes": snaps[0].arena.numel(), "blocks": snaps[0].blocks,
                      "launches_per_take": 2, "ring": ring, "reps_per_graph": reps,
                      "take_us": round(us["take"], 2), "copy_us": round(us["copy"], 2), "take_again_us": round(us["take_again"], 2),
                      "take_gbps_read_plus_write": round(2 * nbytes / us["take"] / 1e3, 1),
                      "copy_gbps_read_plus_write": round(2 * nbytes / us["copy"] / 1e3, 1),
                      "take_over_copy": round(us["take"] / us["copy"], 3),
                      "aa_spread": round(abs(us["take_again"] / us["take"] - 1.0), 4),
                      "restore_call_ms": round(statistics.median(restore[2:]), 3),
                      "samples_us": {v: [round(t, 2) for t in s] for v, s in samples.items()}}
        print(json.dumps({name: {k: v for k, v in rows[name].items() if k != "samples_us"}}), flush=True)
        del sets, snaps, srcs, dsts, graphs
        torch.cuda.empty_cache()
    return rows


def _parent_trainer(path):
    spec = importlib.util.spec_from_file_location("Trainer_parent", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.Trainer


def time_epoch(rounds, steps, epochs, parent):
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
    tmp = tempfile.mkdtemp(prefix="bench_checkpoint_")
    variants = [("off_a", Trainer, {})]
    if parent:
        variants.append(("parent", _parent_trainer(parent), {}))
    variants += [("async", Trainer, dict(async_checkpoints=True)),
                 ("async_resume", Trainer, dict(async_checkpoints=True, resume=True)), ("off_b", Trainer, {})]
    trainers, joins = {}, {}
    for name, cls, flags in variants:
        torch.manual_seed(0)
        m = Model.UNet(1, 2, 64, compute_dtype="fp16").cuda()
        opt = uo.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        tr = trainers[name] = cls(m, "single", torch.cuda.FloatTensor, "cuda", os.path.join(tmp, name), loaders, B, opt, 10 ** 6,
                                  epochs, "dice_bce_mc", "dice_bce_mc", lr_scheduler=None, graph=True, **flags)
        joins[name] = []
        if flags:                                                 # time the join at the end of train() on its own

            def close(name=name, inner=tr._run_state().close):
                t0 = time.perf_counter()
                inner()
                joins[name].append((time.perf_counter() - t0) * 1e3)
            tr._run_state().close = close
    turns = {k: [] for k in trainers}
    for r in range(rounds + 1):                                   # round 0 warms up: first steps, captures, first writes
        for k, tr in trainers.items():
            state = os.path.join(tmp, k, "run_state.pt")
            if os.path.exists(state):
                os.remove(state)                                  # every turn is a fresh run of `epochs` epochs
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.train()
            torch.cuda.synchronize()
            if r:
                turns[k].append((time.perf_counter() - t0) * 1e3 / epochs)
    med = {k: statistics.median(v) for k, v in turns.items()}
    base = statistics.median(turns["off_a"] + turns["off_b"])
    sizes = {k: sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(os.path.join(tmp, k)) for f in fs if f.endswith(".pt"))
             for k in trainers}
    row = {"workload": f"Trainer epoch, UNet(1,2,64) {B}x{S}x{S} fp16, graph=True, {steps} training + 2 validation steps, "
                       f"checkpoint writes included; a turn is one train() of {epochs} epochs, figures are per epoch",
           "rounds": rounds, "epochs_per_turn": epochs, "epoch_ms": {k: round(v, 2) for k, v in med.items()},
           "epoch_ms_fastest": {k: round(min(v), 2) for k, v in turns.items()},
           "epoch_ms_turns": {k: [round(t, 2) for t in v] for k, v in turns.items()},
           "aa_spread_ms": round(abs(med["off_a"] - med["off_b"]), 2),
           "minus_off_ms": {k: round(v - base, 2) for k, v in med.items()},
           "join_ms_per_turn": {k: round(statistics.median(v[1:]), 2) for k, v in joins.items() if len(v) > 1},
           "checkpoint_bytes_on_disk": sizes,
           "last_train_loss": {k: tr.train_loss_list[-1] for k, tr in trainers.items()}}
    if parent:
        row["off_minus_parent_ms"] = round(base - med["parent"], 2)
    print(json.dumps({"epoch": row}), flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "checkpoint_snapshot.json"))
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--epochs", type=int, default=3)
    ap.add_argument("--only", choices=["snapshot", "epoch"])
    ap.add_argument("--parent", help="Trainer.py of another commit, measured beside this one's")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_checkpoint.py needs an MI355X")
    result = {"device": torch.cuda.get_device_name(0), "scaling_over_several_gpus": "not measured"}
    if a.only != "epoch":
        result["snapshot"] = time_snapshot(a.windows)
    if a.only != "snapshot":
        result["epoch"] = time_epoch(a.rounds, a.steps, a.epochs, a.parent)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
