#!/usr/bin/env python3
"""Times the fp32 pointwise convolutions / linears of TransUNet R50-ViT-B/16 at batch 24, 224 x 224 (M = 4,704 tokens) on one MI355X
with UMI_CONV_F32_MFMA_1X1 (the fp32-input matrix-core GEMM of csrc/gemm_mfma_f32.hip) and without it (the LDS-tiled VALU kernels
of csrc/generic_kernels.hip), in one process on one box, the variants alternating.

  per_shape         the four linears of a ViT block, the patch embedding and the trunk's 1x1 convolutions at their three
                    resolutions: forward (with the bias where the layer has one), data gradient and weight gradient, per launch;
                    per variant the median of --windows windows of --reps launches, device events around a window, every shape
                    warmed up first.  Variants: "base" (no flag), "mfma" (the flag), "base_again" (no flag, timed a second time:
                    the A/A measure of spread).  TFLOP/s = 2 * M * Ci * Co over the launch time, `frac` = the flagged call's share
                    of the 157.3 TFLOP/s fp32 peak.  `mfma_slower_by` = mfma / base - 1, `aa_spread` = |base_again / base - 1|;
                    `loses` = the flagged call is slower than the flag-less one by more than that spread.
  rounding          largest |result - float64| / (gamma_2K' * sum |a b|) of forward, data gradient and weight gradient on
                    standard-normal data (the bound and shapes of tests/test_gpu_gemm_f32_mfma.py; float64 on the host)
  step_ms           the eager training step of the full model (forward + dice_bce_mc loss + backward + SGD) under compute_dtype
                    "fp32" and "fp32_mfma_gemm": the median and every sample of windows of --steps steps, the modes alternating

Prints one JSON line; --out writes it (profiles/f32_gemm_mfma.json is the record README and DESIGN quote).  No GPU: fails.
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
import torch.nn.functional as F  # noqa: E402

DEV = "cuda"
PEAK_F32_TFLOPS = 157.3
BATCH, SIZE = 24, 224
MODES = ("fp32", "fp32_mfma_gemm")
VARIANTS = ("base", "mfma", "base_again")
TOKENS = BATCH * (SIZE // 16) ** 2
# (name, N, H, W, Ci, Co, the layer has a bias)
SHAPES = [("qkv", 1, 1, TOKENS, 768, 2304, True), ("attn_out", 1, 1, TOKENS, 768, 768, True), ("fc1", 1, 1, TOKENS, 768, 3072, True),
          ("fc2", 1, 1, TOKENS, 3072, 768, True), ("patch_embedding", BATCH, 14, 14, 1024, 768, True),
          ("trunk56 64->256", BATCH, 56, 56, 64, 256, False), ("trunk56 256->64", BATCH, 56, 56, 256, 64, False),
          ("trunk28 256->128", BATCH, 28, 28, 256, 128, False), ("trunk28 128->512", BATCH, 28, 28, 128, 512, False),
          ("trunk28 512->128", BATCH, 28, 28, 512, 128, False), ("trunk14 512->256", BATCH, 14, 14, 512, 256, False),
          ("trunk14 256->1024", BATCH, 14, 14, 256, 1024, False), ("trunk14 1024->256", BATCH, 14, 14, 1024, 256, False)]


def event_ms(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def time_shapes(reps, windows):
    from umi import lib, ops
    rows = []
    for name, n, h, w, ci, co, has_bias in SHAPES:
        M = n * h * w
        x, dy = torch.randn(n, h, w, ci, device=DEV), torch.randn(n, h, w, co, device=DEV)
        wgt = torch.randn(co, ci, 1, 1, device=DEV) * ci ** -0.5
        bias = torch.randn(co, device=DEV) if has_bias else None
        wp, wpd = ops.pack_conv_fwd(wgt, torch.float32), ops.pack_conv_dgrad(wgt, torch.float32)
        y, dx, gw = torch.empty(n, h, w, co, device=DEV), torch.empty(n, h, w, ci, device=DEV), torch.empty(co, ci, 1, 1, device=DEV)
        assert ops.conv_plan(x, y, 1, 1, 1, 0, lib.CONV_F32_MFMA_1X1, has_bias) == (0, -(-M // 128))       # the new path is named
        assert ops.conv_plan(dy, dx, 1, 1, 1, 0, lib.CONV_F32_MFMA_1X1) == (0, -(-M // 128))

        def calls(flags):
            return {"fwd": lambda: ops.conv_fwd(x, None, lambda _l: wp, bias, y, 1, 1, 1, 0, flags=flags),
                    "dgrad": lambda: ops.conv_fwd(dy, None, lambda _l: wpd, None, dx, 1, 1, 1, 0, flags=flags),
                    "wgrad": lambda: ops.conv_wgrad(x, None, dy, None, gw, ci, 1, 1, 1.0, 1, 1, 1, 0, flags=flags)}
        fns = {"base": calls(0), "mfma": calls(lib.CONV_F32_MFMA_1X1), "base_again": calls(0)}
        for v in VARIANTS:                               # warm-up of this shape, every variant
            for f in fns[v].values():
                f()
        torch.cuda.synchronize()
        gflop = 2.0 * M * ci * co / 1e9
        row = {"layer": name, "M": M, "Ci": ci, "Co": co, "bias": has_bias, "gflop": round(gflop, 3)}
        for op in ("fwd", "dgrad", "wgrad"):
            samples = {v: [] for v in VARIANTS}
            for _ in range(windows):
                for v in VARIANTS:                       # the variants alternate
                    samples[v].append(event_ms(fns[v][op], reps))
            ms = {v: statistics.median(s) for v, s in samples.items()}
            slower, spread = ms["mfma"] / ms["base"] - 1.0, abs(ms["base_again"] / ms["base"] - 1.0)
            row[op] = {"base_ms": round(ms["base"], 4), "mfma_ms": round(ms["mfma"], 4), "base_again_ms": round(ms["base_again"], 4),
                       "base_tflops": round(gflop / ms["base"], 2), "mfma_tflops": round(gflop / ms["mfma"], 2),
                       "frac_of_f32_peak": round(gflop / ms["mfma"] / PEAK_F32_TFLOPS, 4), "speedup": round(ms["base"] / ms["mfma"], 3),
                       "mfma_slower_by": round(slower, 4), "aa_spread": round(spread, 4), "loses": bool(slower > spread)}
        rows.append(row)
        del x, dy, wgt, wp, wpd, y, dx, gw
    return rows


def rounding_ratios():
    """The bound of tests/test_gpu_gemm_f32_mfma.py: any order of K' fused products, gamma_2K' * sum |a b|, u = 2^-24."""
    from umi import lib, ops
    u, flag = 2.0 ** -24, lib.CONV_F32_MFMA_1X1

    def ratio(got, ref, mag, K):
        return round(((got.double().cpu() - ref).abs() / (2 * K * u / (1 - 2 * K * u) * mag)).max().item(), 5)
    out = {}
    for N, H, W, Ci, Co in ((1, 14, 14, 768, 3072), (1, 14, 14, 3072, 768)):
        g = torch.Generator().manual_seed(N + H + W + Ci + Co)
        x, w, b = torch.randn(N, H, W, Ci, generator=g), torch.randn(Co, Ci, 1, 1, generator=g), torch.randn(Co, generator=g)
        dy = torch.randn(N, H, W, Co, generator=g)
        x64, w64, b64, dy64 = x.double(), w.double().view(Co, Ci), b.double(), dy.double()
        y, dx = torch.empty(N, H, W, Co, device=DEV), torch.empty(N, H, W, Ci, device=DEV)
        wd = w.to(DEV)
        ops.conv_fwd(x.to(DEV), None, lambda _l: ops.pack_conv_fwd(wd, torch.float32), b.to(DEV), y, 1, 1, 1, 0, flags=flag)
        ops.conv_fwd(dy.to(DEV), None, lambda _l: ops.pack_conv_dgrad(wd, torch.float32), None, dx, 1, 1, 1, 0, flags=flag)
        key = f"{N}x{H}x{W}x{Ci}->{Co}"
        out["fwd " + key] = ratio(y, F.linear(x64, w64, b64), F.linear(x64.abs(), w64.abs(), b64.abs()), Ci + 1)
        out["dgrad " + key] = ratio(dx, F.linear(dy64, w64.t()), F.linear(dy64.abs(), w64.t().abs()), Co)
    for N, H, W, Ci, Co in ((2, 32, 32, 64, 128), (24, 14, 14, 64, 96)):
        g = torch.Generator().manual_seed(N + H + W + Ci + Co)
        x, dy = torch.randn(N, H, W, Ci, generator=g), torch.randn(N, H, W, Co, generator=g)
        a64, d64 = x.double().reshape(-1, Ci), dy.double().reshape(-1, Co)
        gw = torch.empty(Co, Ci, 1, 1, device=DEV)
        ops.conv_wgrad(x.to(DEV), None, dy.to(DEV), None, gw, Ci, 1, 1, 1.0, 1, 1, 1, 0, flags=flag)
        out[f"wgrad {N}x{H}x{W}x{Ci}->{Co}"] = ratio(gw, (d64.t() @ a64).view(Co, Ci, 1, 1), (d64.abs().t() @ a64.abs()).view(Co, Ci, 1, 1),
                                                     N * H * W)
    out["largest"] = max(out.values())
    return out


def time_steps(steps, warmup, windows):
    import loss as L
    from TransUnet.vit_seg_modeling import CONFIGS, VisionTransformer
    from umi import optim as umi_optim
    cfg = copy.deepcopy(CONFIGS["R50-ViT-B_16"])
    cfg.n_classes, cfg.n_skip, cfg.patches.grid = 2, 3, (SIZE // 16, SIZE // 16)
    L.CLASS_NUMBER = 2
    torch.manual_seed(0)
    x = torch.randn(BATCH, 1, SIZE, SIZE, device=DEV)
    labels = torch.randint(0, 2, (BATCH, SIZE, SIZE), device=DEV).float()
    runs, state = {}, None
    for mode in MODES:
        m = VisionTransformer(cfg, img_size=SIZE, num_classes=2, compute_dtype=mode)
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
    samples = {mode: [] for mode in MODES}
    for _ in range(windows):
        for mode in MODES:
            samples[mode].append(event_ms(runs[mode], steps))
    return {mode: {"median_ms": round(statistics.median(v), 3), "samples_ms": [round(s, 3) for s in v],
                   "first_step_loss": first_loss[mode]} for mode, v in samples.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=2, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=2, help="eager warm-up steps per mode")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per variant / mode, alternating")
    ap.add_argument("--reps", type=int, default=10, help="launches per per-shape window")
    ap.add_argument("--no-step", action="store_true", help="skip the full-model step (per-shape timings and rounding only)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "f32_gemm_mfma.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_f32_gemm: needs an MI355X (no device found); nothing is measured on the host")
    rounding = rounding_ratios()
    shapes = time_shapes(a.reps, a.windows)
    losing = [f"{r['layer']} {op}" for r in shapes for op in ("fwd", "dgrad", "wgrad") if r[op]["loses"]]
    res = {"workload": f"TransUNet R50-ViT-B/16 {SIZE}x{SIZE} batch {BATCH} (M = {TOKENS} tokens): fp32 pointwise shapes, per launch",
           "device": torch.cuda.get_device_name(0), "peak_f32_tflops": PEAK_F32_TFLOPS, "reps_per_window": a.reps, "windows": a.windows,
           "per_shape": shapes, "slower_than_the_aa_spread": losing, "rounding_ratio_to_bound": rounding}
    if not a.no_step:
        steps = time_steps(a.steps, a.warmup, a.windows)
        res["step_ms"], res["steps_per_window"] = steps, a.steps
        res["step_speedup_fp32_over_fp32_mfma_gemm"] = round(steps["fp32"]["median_ms"] / steps["fp32_mfma_gemm"]["median_ms"], 3)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
