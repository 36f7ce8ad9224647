"""What gradient accumulation (umi.accum) costs on one MI355X.

    python tools/bench_accum.py [--out profiles/grad_accum.json] [--windows 10] [--rounds 4] [--steps 10] [--only passes|step]
                                [--label TEXT]

One process, the variants take turns round by round, medians are reported, and every comparison has its A/A pair (the same graph
or the same configuration measured twice), as tools/bench_ema.py does.

passes  umi_grad_accum_multi over tensors of the parameter shapes of UNet(1,2,64) and of TransUNet R50-ViT-B/16, `reps` calls
        captured into one HIP graph that rotate through a ring of (gradient, accumulator) sets of more than 1 GB, so every pass
        reads HBM (cold buffers).  The pass a call takes is set by the state block it is given, so each of the three is timed
        alone: FIRST (acc = g: 8 B per parameter), ADD (acc += g: 12 B) and LAST (g = (acc + g) * s: 12 B), each next to ONE
        device-to-device copy that moves the same bytes; beside them umi_ema_multi on the same tables (12 B, the same access
        pattern as ADD) and torch._foreach_add_ followed by torch._foreach_mul_ on the same tensors, which is what a loop written
        by hand runs on the last micro-batch.
step    Trainer.train_step of UNet(1,2,64) at 512 x 512, fp16, graph=True, replayed, per IMAGE:
          B = 16 with accumulate off       against   B = 8 with accumulate=2      (both on the matrix-core kernels)
          B = 32 with accumulate off       against   B = 16 with accumulate=2     (32 x 512 x 512 x 64 halves pass the 31-bit limit
                                                                                   of the matrix-core kernels: the VALU fallback)
The cache policy of the kernel is a compile-time choice (UMI_ACCUM_POLICY in csrc/grad_accum.hip); `--label` names the build that
ran.  Data parallel (one set of collectives per window over xGMI) is NOT measured here."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from tools.bench_ema import _median_rounds  # noqa: E402
from tools.bench_trainer_dp import RING_BYTES, capture, param_shapes  # noqa: E402


def _table(gs, accs):
    """Device descriptor table over (gradient, accumulator) pairs; for umi_ema_multi the gradient stands in `p` as well."""
    from umi import lib as L, ops
    blk = L.fn("umi_optim_block_elems")()
    arr, b0 = np.zeros(len(gs), dtype=ops.OPTIM_DESC), 0
    for i, (g, a) in enumerate(zip(gs, accs)):
        arr[i] = (g.data_ptr(), g.data_ptr(), a.data_ptr(), 0, g.numel(), b0, 0)
        b0 += (g.numel() + blk - 1) // blk
    return torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).cuda(), len(gs), b0


def _block(**slots):
    from umi.accum import ACCUM, ACCUM_LEN
    st = np.zeros(ACCUM_LEN)
    for k, v in slots.items():
        st[ACCUM[k]] = v
    return torch.from_numpy(st).cuda()


def time_passes(windows):
    from umi import lib as L, ops
    from umi.ema import EMA, EMA_LEN
    blocks = {"first": _block(FIRST=1, SCALE=1.0), "add": _block(SCALE=0.5), "last": _block(LAST=1, SCALE=float(np.float32(1 / 3)))}
    ema_st = np.zeros(EMA_LEN)
    ema_st[EMA["ACTIVE"]], ema_st[EMA["WEIGHT"]] = 1.0, float(np.float32(0.001))
    ema_block = torch.from_numpy(ema_st).cuda()
    moved = {"first": 8, "add": 12, "last": 12}
    rows = {}
    for name, shapes in param_shapes().items():
        n = sum(int(torch.Size(s).numel()) for s in shapes)
        ring = RING_BYTES // (8 * n) + 1                           # a gradient and its accumulator per set
        reps = max(20, int(5e10 // (12 * n)))
        grads = [[torch.randn(s, device="cuda") * 1e-3 for s in shapes] for _ in range(ring)]
        accs = [[torch.randn(s, device="cuda") * 1e-3 for s in shapes] for _ in range(ring)]
        tables = [_table(g, a) for g, a in zip(grads, accs)]
        srcs = [torch.empty(6 * n, dtype=torch.int8, device="cuda") for _ in range(ring)]
        dsts = [torch.empty(6 * n, dtype=torch.int8, device="cuda") for _ in range(ring)]

        def accum(block):
            return [lambda t=t: L.call("umi_grad_accum_multi", t[0].data_ptr(), t[1], t[2], block.data_ptr(), ops._stream())
                    for t in tables]

        def foreach(g, a):
            torch._foreach_add_(a, g)
            torch._foreach_mul_(a, 0.5)
        graphs = {k: capture(accum(b), reps) for k, b in blocks.items()}
        graphs["ema_multi"] = capture([lambda t=t: L.call("umi_ema_multi", t[0].data_ptr(), t[1], t[2], ema_block.data_ptr(),
                                                          ops._stream()) for t in tables], reps)
        graphs["foreach_add_mul"] = capture([lambda g=g, a=a: foreach(g, a) for g, a in zip(grads, accs)], reps)
        graphs["copy_8B"] = capture([lambda s=s, d=d: d[:4 * n].copy_(s[:4 * n]) for s, d in zip(srcs, dsts)], reps)
        graphs["copy_12B"] = capture([lambda s=s, d=d: d.copy_(s) for s, d in zip(srcs, dsts)], reps)
        graphs["add_again"] = graphs["add"]
        us, samples = _median_rounds(graphs, windows, reps)
        aa = abs(us["add_again"] / us["add"] - 1.0)
        row = {"tensors": len(shapes), "parameters": n, "ring": ring, "reps_per_graph": reps,
               "bytes_moved_per_parameter": dict(moved, ema_multi=12, foreach_add_mul=20),
               "launches": {"first": 1, "add": 1, "last": 1, "ema_multi": 1, "foreach_add_mul": "2 foreach calls"},
               "cold_us": {k: round(v, 2) for k, v in us.items()},
               "cold_gbps": {k: round(moved[k] * n / us[k] / 1e3, 1) for k in moved},
               "over_copy_of_the_same_bytes": {k: round(us[k] / us["copy_%dB" % moved[k]], 3) for k in moved},
               "add_over_ema_multi": round(us["add"] / us["ema_multi"], 4), "cold_aa_spread": round(aa, 4),
               "add_within_twice_aa_spread_of_ema_multi": bool(abs(us["add"] / us["ema_multi"] - 1.0) <= 2 * aa),
               "foreach_over_last": round(us["foreach_add_mul"] / us["last"], 3),
               "cold_samples_us": {v: [round(t, 2) for t in s] for v, s in samples.items()}}
        rows[name] = row
        print(json.dumps({name: {k: v for k, v in row.items() if not k.endswith("samples_us")}}), flush=True)
        del graphs, tables, grads, accs, srcs, dsts
        torch.cuda.empty_cache()
    return rows


def _batch(B):
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.randn(B, 1, 512, 512, device="cuda", generator=g)
    return x, torch.randint(0, 2, (B, 512, 512), device="cuda", generator=g).float()


def _pair(rounds, steps, variants):
    """variants: name -> (B, accumulate).  Turns of `steps` train_steps each, round by round; ms per IMAGE."""
    import loss as L
    import Model
    from Trainer import Trainer
    from umi import optim as uo
    L.CLASS_NUMBER = 2
    tmp = tempfile.mkdtemp(prefix="bench_accum_")
    trainers, batches = {}, {}
    for name, (B, k) in variants.items():
        torch.manual_seed(0)
        m = Model.UNet(1, 2, 64, compute_dtype="fp16").cuda()
        opt = uo.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        batches[name] = _batch(B)
        trainers[name] = Trainer(m, "single", torch.cuda.FloatTensor, "cuda", os.path.join(tmp, name),
                                 {"train": [batches[name]] * steps, "val": []}, B, opt, 10 ** 6, 1, "dice_bce_mc", "dice_bce_mc",
                                 lr_scheduler=None, graph=True, accumulate=k)
    ms = {k: [] for k in trainers}
    for r in range(rounds + 1):                                   # round 0: the eager first steps, the captures
        for name, tr in trainers.items():
            x, lab = batches[name]
            tr.model.train()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                tr.train_step(x, lab)
            torch.cuda.synchronize()
            if r:
                ms[name].append((time.perf_counter() - t0) * 1e3 / (steps * x.shape[0]))
    shutil.rmtree(tmp, ignore_errors=True)
    graphs = {name: len(tr._graphs) for name, tr in trainers.items()}
    del trainers, batches
    torch.cuda.empty_cache()
    return {k: statistics.median(v) for k, v in ms.items()}, ms, graphs


def time_step(rounds, steps):
    """Yields (label, row), pair by pair, so that what has been measured is on disk before the next pair starts."""
    for label, variants in (("b16_against_2x8", {"b16_a": (16, None), "2x8": (8, 2), "b16_b": (16, None)}),
                            ("b32_against_2x16", {"2x16_a": (16, 2), "b32": (32, None), "2x16_b": (16, 2)})):
        med, ms, graphs = _pair(rounds, steps, variants)
        names = list(variants)
        aa = abs(med[names[0]] - med[names[2]])
        base = statistics.median(ms[names[0]] + ms[names[2]])
        row = {"workload": f"Trainer.train_step, UNet(1,2,64) 512x512 fp16, graph=True, replayed; {steps} steps per turn; ms per image",
               "rounds": rounds, "ms_per_image": {k: round(v, 4) for k, v in med.items()},
               "ms_per_image_turns": {k: [round(t, 4) for t in v] for k, v in ms.items()}, "graphs_held": graphs,
               "aa_spread_ms_per_image": round(aa, 4), "middle_over_the_pair": round(med[names[1]] / base, 4)}
        print(json.dumps({label: row}), flush=True)
        yield label, row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "grad_accum.json"))
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--only", choices=["passes", "step"], action="append")
    ap.add_argument("--label", default="policy 1: every 16-byte access non-temporal", help="names the build that ran")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_accum.py needs an MI355X")
    want = set(a.only or ["passes", "step"])
    result = {"device": torch.cuda.get_device_name(0), "build": a.label, "data_parallel_over_xgmi": "not measured",
              "other_cache_policies": "not measured", "passes": "not measured", "step": "not measured"}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    if "passes" in want:
        result["passes"] = time_passes(a.windows)
        write()
    if "step" in want:
        result["step"] = {"b16_against_2x8": "not measured", "b32_against_2x16": "not measured"}
        for label, row in time_step(a.rounds, a.steps):
            result["step"][label] = row
            write()
    write()


if __name__ == "__main__":
    main()
