#!/usr/bin/env python3
"""Times the attention of TransUNet R50-ViT-B/16 (12 heads x 64) with and without attention-probability dropout on one MI355X, in
one process, the variants alternating, and writes profiles/attn_dropout.json.

  kernels   (B, N, heads) = (24, 196, 12) and (12, 1024, 12), one encoder layer's attention on the tape's layout (q / k / v and
            dq / dk / dv channel slices of [B, N, 3C] buffers), for the fp16 matrix-core kernels and the fp32 matrix-core kernels
            (UMI_ATTN_F32_MFMA): the forward launch and the backward pair, per call.  Per variant the median of --windows windows,
            device events around a window of at least --window-s seconds of calls (the count is calibrated per shape and
            operation), every variant warmed up first.  Variants:
              base        umi_attn_fwd_flags / umi_attn_bwd_flags of this build
              parent      the same two entry points of the PARENT commit's library (--parent-lib), same buffers
              base_again  base, timed a second time: the A/A measure of spread
              drop        umi_attn_fwd_dropout / umi_attn_bwd_dropout at p = 0.1 with a device counter
            Every variant is a raw ctypes call with the same arguments, so the host's share is the same for all.
            `parent_vs_base` = base / parent - 1 is the claim "the existing entry points are unchanged": it must lie inside
            `aa_spread`, the largest distance between two timings of the same code (the two base slots: their medians and
            their windows round by round) -> `unchanged`.  `drop_cost` = drop / base: nobody had measured it, no bar.
  step      the graph-replayed training step of the full model at batch 24 @ 224 x 224 (forward + dice_bce_mc + backward + SGD,
            compute dtype fp16) with config.transformer["attention_dropout_rate"] = 0 and = 0.1, alternating, rate 0 timed in
            two slots.  (The rate also drives the output projection's dropout, as in the reference: rate 0.1 pays for both.)

Prints one JSON line.  No GPU: fails."""
import argparse
import copy
import ctypes
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import torch  # noqa: E402

DEV = "cuda"
D = 64
P = 0.1
KERNEL_SHAPES = [(24, 196, 12), (12, 1024, 12)]
VARIANTS = ("base", "parent", "base_again", "drop")


def event_ms(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def reps_for(fn, window_s):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return max(5, math.ceil(window_s * 1e3 / event_ms(fn, 10)))


def entry_points(path=None):
    """The four attention entry points as raw ctypes functions of this build (path None) or of another build of the library,
    under this build's prototypes (those of the two existing ones are unchanged).  Every variant is called the same way, so the
    host's share of a call is the same for all of them."""
    from umi import lib
    if path is None:
        return {n: lib.fn(n) for n in ("umi_attn_fwd_flags", "umi_attn_bwd_flags", "umi_attn_fwd_dropout", "umi_attn_bwd_dropout")}
    other, out = ctypes.CDLL(path), {}
    for name in ("umi_attn_fwd_flags", "umi_attn_bwd_flags"):
        out[name] = getattr(other, name)
        out[name].restype, out[name].argtypes = lib.SIGNATURES[name]
    return out


def time_kernels(window_s, windows, parent_lib):
    from umi import lib, ops_tu
    from umi.ops import _dt, _stream
    libs = {"base": entry_points()}
    libs["base_again"] = libs["drop"] = libs["base"]
    if parent_lib:
        libs["parent"] = entry_points(parent_lib)
    variants = [var for var in VARIANTS if var in libs]
    rows = []
    for family, dtype, flags, kernel in (("fp16 matrix-core", torch.float16, 0, 1), ("fp32 matrix-core", torch.float32, lib.UMI_ATTN_F32_MFMA, 2)):
        for B, N, heads in KERNEL_SHAPES:
            C = heads * D
            qkv = torch.randn(B, 1, N, 3 * C, device=DEV).to(dtype)
            dqkv = torch.empty(B, 1, N, 3 * C, device=DEV, dtype=dtype)
            q, k, v = (qkv[..., i * C:(i + 1) * C] for i in range(3))
            dq, dk, dv = (dqkv[..., i * C:(i + 1) * C] for i in range(3))
            o, dO = torch.empty(B, 1, N, C, device=DEV, dtype=dtype), torch.randn(B, 1, N, C, device=DEV).to(dtype)
            ctr = torch.tensor([3], dtype=torch.int32, device=DEV)
            assert ops_tu.attn_plan(q, k, v, o, heads, flags) == ops_tu.attn_plan(q, k, v, o, heads, flags, dq=dq) == kernel
            lse = ops_tu.attn_fwd(q, k, v, o, heads, flags=flags)
            delta = torch.empty_like(lse)
            st = _stream()
            fwd_args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), 3 * C, o.data_ptr(), C, lse.data_ptr(), B, N, heads, D, _dt(q), flags)
            bwd_args = (q.data_ptr(), k.data_ptr(), v.data_ptr(), 3 * C, o.data_ptr(), dO.data_ptr(), C, lse.data_ptr(), dq.data_ptr(),
                        dk.data_ptr(), dv.data_ptr(), 3 * C, delta.data_ptr(), B, N, heads, D, _dt(q), flags)
            drop_args = (P, 12345, ctr.data_ptr())

            def calls(var):
                e = libs[var]
                if var == "drop":
                    return {"fwd": lambda: e["umi_attn_fwd_dropout"](*fwd_args, *drop_args, st),
                            "bwd": lambda: e["umi_attn_bwd_dropout"](*bwd_args, *drop_args, st)}
                return {"fwd": lambda: e["umi_attn_fwd_flags"](*fwd_args, st), "bwd": lambda: e["umi_attn_bwd_flags"](*bwd_args, st)}
            fns = {var: calls(var) for var in variants}
            row = {"kernels": family, "B": B, "N": N, "heads": heads}
            total = {var: 0.0 for var in variants}
            for op in ("fwd", "bwd"):
                for var in variants:                                      # warm-up; a raw call returns its status
                    if fns[var][op]() != 0:
                        sys.exit(f"bench_attn_dropout: {var} {op} failed at {(B, N, heads)}")
                reps = reps_for(fns["base"][op], window_s)
                samples = {var: [] for var in variants}
                for _ in range(windows):
                    for var in variants:                                  # the variants alternate
                        samples[var].append(event_ms(fns[var][op], reps))
                ms = {var: statistics.median(s) for var, s in samples.items()}
                row[op] = compare(ms, reps, samples)
                for var in variants:
                    total[var] += ms[var]
            row["fwd_bwd"] = compare(total, None)
            rows.append(row)
            del qkv, dqkv, o, dO, lse
    return rows


def compare(ms, reps, samples=None):
    """aa_spread: how far two timings of the SAME code lie apart -- the medians of the two base slots and, per operation, the
    largest gap between their windows of the same round (`samples`).  A parent / base difference of medians inside it is
    `unchanged`."""
    out = {f"{var}_ms": round(t, 5) for var, t in ms.items()}
    spread = abs(ms["base_again"] / ms["base"] - 1.0)
    if samples is not None:
        out["aa_spread_of_medians"] = round(spread, 5)
        spread = max([spread] + [abs(x / y - 1.0) for x, y in zip(samples["base_again"], samples["base"])])
    out["aa_spread"] = round(spread, 5)
    if "parent" in ms:
        diff = ms["base"] / ms["parent"] - 1.0
        out["parent_vs_base"] = round(diff, 5)
        out["unchanged"] = bool(abs(diff) <= spread)
    out["drop_cost"] = round(ms["drop"] / ms["base"], 3)
    if reps is not None:
        out["calls_per_window"] = reps
    return out


def time_step(batch, size, window_s, windows):
    import loss as L
    from TransUnet.vit_seg_modeling import CONFIGS, VisionTransformer
    from umi import optim as umi_optim
    from umi.graphs import GraphedStep
    L.CLASS_NUMBER = 2
    torch.manual_seed(0)
    x = torch.randn(batch, 1, size, size, device=DEV)
    lab = torch.randint(0, 2, (batch, size, size), device=DEV).float()
    steps, state, keep = {}, None, []
    for rate in (0.0, P):
        cfg = copy.deepcopy(CONFIGS["R50-ViT-B_16"])
        cfg.n_classes, cfg.n_skip, cfg.patches.grid = 2, 3, (size // 16, size // 16)
        cfg.transformer["attention_dropout_rate"] = rate
        m = VisionTransformer(cfg, img_size=size, num_classes=2, compute_dtype="fp16")
        if state is None:
            state = {k: v.clone() for k, v in m.state_dict().items()}
        m.load_state_dict(state)                                          # both rates start from the same weights
        m.to(DEV).train()
        opt = umi_optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)

        def step(xx, yy, m=m, opt=opt):
            loss = L.calc_loss(m(xx), yy, loss_type="dice_bce_mc")
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss
        gs = GraphedStep(step, [x, lab], warmup=2)
        keep.append((m, opt, gs))
        steps[rate] = lambda gs=gs: gs(x, lab)
    slots = {"rate_0": steps[0.0], f"rate_{P}": steps[P], "rate_0_again": steps[0.0]}
    reps = reps_for(slots["rate_0"], window_s)
    samples = {slot: [] for slot in slots}
    for _ in range(windows):
        for slot, fn in slots.items():
            samples[slot].append(event_ms(fn, reps))
    res = {slot: {"median_ms": round(statistics.median(s), 3), "samples_ms": [round(t, 3) for t in s]} for slot, s in samples.items()}
    base, drop, again = (res[s]["median_ms"] for s in slots)
    res.update(batch=batch, size=size, steps_per_window=reps, drop_cost=round(drop / base, 4), aa_spread=round(abs(again / base - 1.0), 4),
               final_loss_finite=bool(all(torch.isfinite(fn()).item() for fn in steps.values())))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--windows", type=int, default=5, help="timed windows per variant, alternating")
    ap.add_argument("--window-s", type=float, default=0.5, help="seconds of device work per timed window")
    ap.add_argument("--parent-lib", default=os.path.join(REPO, "tools", "_ab", "libunetmi_parent.so"),
                    help="libunetmi.so built from the parent commit (a second checkout's umi/build.py); '' = skip that comparison")
    ap.add_argument("--no-step", action="store_true", help="skip the full-model step")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "attn_dropout.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_attn_dropout: needs an MI355X (no device found); nothing is measured on the host")
    if a.parent_lib and not os.path.exists(a.parent_lib):
        sys.exit(f"bench_attn_dropout: no parent library at {a.parent_lib} (build the parent commit, or pass --parent-lib '')")
    kernels = time_kernels(a.window_s, a.windows, a.parent_lib)
    res = {"workload": "TransUNet R50-ViT-B/16 attention, 12 heads x 64, one layer's forward and backward per call, without and with "
                       f"attention-probability dropout p = {P}; and the graph-replayed training step at attention_dropout_rate 0 / {P}",
           "device": torch.cuda.get_device_name(0), "windows": a.windows, "window_seconds": a.window_s,
           "parent_library_compared": bool(a.parent_lib), "kernels": kernels}
    if a.parent_lib:
        res["existing_entry_points_outside_the_aa_spread"] = [f"{r['kernels']} {r['B']}x{r['N']}x{r['heads']} {op}" for r in kernels
                                                              for op in ("fwd", "bwd") if not r[op]["unchanged"]]
    if not a.no_step:
        res["step"] = time_step(24, 224, a.window_s, a.windows)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
