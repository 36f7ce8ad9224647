#!/usr/bin/env python3
"""Times the fp32 softmax attention of TransUNet R50-ViT-B/16 (12 heads x 64) on one MI355X with UMI_ATTN_F32_MFMA (the fp32-input
matrix-core kernels of csrc/attention_mfma_f32.hip) and without it (the VALU kernels of csrc/transformer_kernels.hip), in one
process on one box, the variants alternating.

  kernels           (B, N, heads) = (24, 196, 12) and (12, 1024, 12), the attention of one encoder layer at batch 24 @ 224 x 224
                    and batch 12 @ 512 x 512, on the tape's layout (q / k / v and dq / dk / dv channel slices of [B, N, 3C]
                    buffers): the forward launch and the backward pair (both backward kernels together), per call; per variant the
                    median of --windows windows of --reps calls, device events around a window, every variant warmed up first.
                    Variants: "base" (no flag), "mfma" (the flag), "base_again" (no flag, timed a second time: the A/A measure
                    of spread).  TFLOP/s counts the operations the algorithm needs, 4 N^2 64 per (batch, head) forward and 2.5
                    times that backward (S, dP, dV, dK, dQ; the two backward kernels each recompute S and dP, which is not
                    counted), over the call time; `frac_of_f32_peak` = the flagged call's share of the 157.3 TFLOP/s fp32 peak
                    (compute bound: the tensors are read once per 128-token tile).  `mfma_slower_by` = mfma / base - 1,
                    `aa_spread` = |base_again / base - 1|; `loses` = the flagged call is slower than the flag-less one by more
                    than that spread.  `fwd_bwd` is the sum of the two.
  largest_error     largest |result - float64| / max |float64| of o, lse, dq, dk, dv at (2, 196, 3), flagged and flag-less
  steps             the eager training step of the full model (forward + dice_bce_mc loss + backward + SGD) at batch 24 @ 224 and
                    batch 12 @ 512 under compute_dtype "fp32_mfma_gemm" and "fp32_mfma_attn": the median and every sample of windows
                    of --steps steps, the modes alternating, "fp32_mfma_gemm" timed in two slots (the A/A spread); the first-step
                    loss of each mode (dropout 0.1 is on and each model draws its own mask seed, so the two differ by the masks).

Prints one JSON line; --out writes it (profiles/f32_attn_mfma.json is the record README and DESIGN quote).  No GPU: fails.
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
PEAK_F32_TFLOPS = 157.3
D = 64
KERNEL_SHAPES = [(24, 196, 12), (12, 1024, 12)]
STEP_CONFIGS = [(24, 224), (12, 512)]
MODES = ("fp32_mfma_gemm", "fp32_mfma_attn")
VARIANTS = ("base", "mfma", "base_again")


def event_ms(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def compare(ms, gflop):
    slower, spread = ms["mfma"] / ms["base"] - 1.0, abs(ms["base_again"] / ms["base"] - 1.0)
    return {"base_ms": round(ms["base"], 4), "mfma_ms": round(ms["mfma"], 4), "base_again_ms": round(ms["base_again"], 4),
            "base_tflops": round(gflop / ms["base"], 2), "mfma_tflops": round(gflop / ms["mfma"], 2),
            "frac_of_f32_peak": round(gflop / ms["mfma"] / PEAK_F32_TFLOPS, 4), "speedup": round(ms["base"] / ms["mfma"], 3),
            "mfma_slower_by": round(slower, 4), "aa_spread": round(spread, 4), "loses": bool(slower > spread)}


def time_kernels(reps, windows):
    from umi import lib, ops_tu
    rows = []
    for B, N, heads in KERNEL_SHAPES:
        C = heads * D
        qkv, dqkv = torch.randn(B, 1, N, 3 * C, device=DEV), torch.empty(B, 1, N, 3 * C, device=DEV)
        q, k, v = (qkv[..., i * C:(i + 1) * C] for i in range(3))
        dq, dk, dv = (dqkv[..., i * C:(i + 1) * C] for i in range(3))
        o, dO = torch.empty(B, 1, N, C, device=DEV), torch.randn(B, 1, N, C, device=DEV)
        flag = lib.UMI_ATTN_F32_MFMA
        assert ops_tu.attn_plan(q, k, v, o, heads, flag) == ops_tu.attn_plan(q, k, v, o, heads, flag, dq=dq) == 2
        assert ops_tu.attn_plan(q, k, v, o, heads, 0) == ops_tu.attn_plan(q, k, v, o, heads, 0, dq=dq) == 0
        lse = ops_tu.attn_fwd(q, k, v, o, heads, flags=flag)

        def calls(flags):
            return {"fwd": lambda: ops_tu.attn_fwd(q, k, v, o, heads, flags=flags),
                    "bwd": lambda: ops_tu.attn_bwd(q, k, v, o, dO, lse, dq, dk, dv, heads, flags=flags)}
        fns = {"base": calls(0), "mfma": calls(flag), "base_again": calls(0)}
        for var in VARIANTS:                             # warm-up of this shape, every variant
            for f in fns[var].values():
                f()
        torch.cuda.synchronize()
        gflop = {"fwd": 4.0 * N * N * D * B * heads / 1e9}
        gflop["bwd"] = 2.5 * gflop["fwd"]
        row = {"B": B, "N": N, "heads": heads, "fwd_gflop": round(gflop["fwd"], 3), "bwd_gflop": round(gflop["bwd"], 3)}
        total = {var: 0.0 for var in VARIANTS}
        for op in ("fwd", "bwd"):
            samples = {var: [] for var in VARIANTS}
            for _ in range(windows):
                for var in VARIANTS:                     # the variants alternate
                    samples[var].append(event_ms(fns[var][op], reps))
            ms = {var: statistics.median(s) for var, s in samples.items()}
            row[op] = compare(ms, gflop[op])
            for var in VARIANTS:
                total[var] += ms[var]
        row["fwd_bwd"] = compare(total, gflop["fwd"] + gflop["bwd"])
        rows.append(row)
        del qkv, dqkv, o, dO, lse
    return rows


def largest_errors():
    """Against softmax(QK^T/8)V and its autograd in float64 on the host, shape (2, 196, 3) of tests/attn_f32_cases.py."""
    from tests import attn_f32_cases as cases
    from umi import lib, ops_tu
    shape = B, N, heads = 2, 196, 3
    x, ref = cases.case(shape)
    out = {}
    for name, flags in (("mfma", lib.UMI_ATTN_F32_MFMA), ("base", 0)):
        q, k, v, dO = (x[n].to(DEV) for n in ("q", "k", "v", "dO"))
        got = {n: torch.empty_like(q) for n in ("o", "dq", "dk", "dv")}
        got["lse"] = ops_tu.attn_fwd(q, k, v, got["o"], heads, flags=flags)
        ops_tu.attn_bwd(q, k, v, got["o"], dO, got["lse"], got["dq"], got["dk"], got["dv"], heads, flags=flags)
        out[name] = {}
        for n in cases.BARS:
            err, top = cases.error(got[n], ref[n])
            out[name][n] = float(f"{err / top:.3e}")
    return out


def time_steps(batch, size, steps, warmup, windows):
    import loss as L
    from TransUnet.vit_seg_modeling import CONFIGS, VisionTransformer
    from umi import optim as umi_optim
    cfg = copy.deepcopy(CONFIGS["R50-ViT-B_16"])
    cfg.n_classes, cfg.n_skip, cfg.patches.grid = 2, 3, (size // 16, size // 16)
    L.CLASS_NUMBER = 2
    torch.manual_seed(0)
    x = torch.randn(batch, 1, size, size, device=DEV)
    labels = torch.randint(0, 2, (batch, size, size), device=DEV).float()
    runs, state = {}, None
    for mode in MODES:
        m = VisionTransformer(cfg, img_size=size, num_classes=2, compute_dtype=mode)
        if state is None:
            state = {k: v.clone() for k, v in m.state_dict().items()}
        m.load_state_dict(state)                         # the two modes start from the same weights
        m.to(DEV).train()
        opt = umi_optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)

        def step(m=m, opt=opt):
            loss = L.calc_loss(m(x), labels, loss_type="dice_bce_mc")
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss
        runs[mode] = step
    first_loss = {}
    for mode in MODES:
        first_loss[mode] = float(runs[mode]().item())
        for _ in range(max(warmup - 1, 0)):
            runs[mode]()
    torch.cuda.synchronize()
    slots = {"fp32_mfma_gemm": runs[MODES[0]], "fp32_mfma_attn": runs[MODES[1]], "fp32_mfma_gemm_again": runs[MODES[0]]}
    samples = {slot: [] for slot in slots}
    for _ in range(windows):
        for slot, fn in slots.items():
            samples[slot].append(event_ms(fn, steps))
    res = {slot: {"median_ms": round(statistics.median(s), 3), "samples_ms": [round(t, 3) for t in s]} for slot, s in samples.items()}
    for mode in MODES:
        res[mode]["first_step_loss"] = first_loss[mode]
    base, attn, again = (res[s]["median_ms"] for s in slots)
    res["attn_slower_by"], res["aa_spread"] = round(attn / base - 1.0, 4), round(abs(again / base - 1.0), 4)
    res["loses"] = bool(res["attn_slower_by"] > res["aa_spread"])
    res["speedup"] = round(base / attn, 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=2, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=2, help="eager warm-up steps per mode")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per variant / mode, alternating")
    ap.add_argument("--reps", type=int, default=5, help="calls per kernel-level window")
    ap.add_argument("--no-step", action="store_true", help="skip the full-model steps (kernel timings and errors only)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "f32_attn_mfma.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_f32_attn: needs an MI355X (no device found); nothing is measured on the host")
    errors = largest_errors()
    kernels = time_kernels(a.reps, a.windows)
    res = {"workload": "TransUNet R50-ViT-B/16 fp32 softmax attention, 12 heads x 64: one layer's forward and backward per call, "
                       "and the eager training step",
           "device": torch.cuda.get_device_name(0), "peak_f32_tflops": PEAK_F32_TFLOPS, "reps_per_window": a.reps, "windows": a.windows,
           "kernels": kernels, "largest_error_over_max_ref": errors,
           "slower_than_the_aa_spread": [f"{r['B']}x{r['N']}x{r['heads']} {op}" for r in kernels for op in ("fwd", "bwd", "fwd_bwd")
                                         if r[op]["loses"]]}
    if not a.no_step:
        res["steps_per_window"] = a.steps
        res["steps"] = {f"batch {b} @ {s}x{s}": time_steps(b, s, a.steps, a.warmup, a.windows) for b, s in STEP_CONFIGS}
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
