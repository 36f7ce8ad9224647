#!/usr/bin/env python3
"""Times the fp32 training step of UNet(1, 2, 64) at 512 x 512, batch 4, on one MI355X under compute_dtype "fp32" (every
convolution on the VALU kernels of csrc/generic_kernels.hip) and "fp32_mfma" (the 3x3 convolutions on the fp32-input matrix-core
kernels of csrc/conv_mfma_f32.hip), in one process on one box, the two modes alternating.

  step_ms           per mode: the median and every sample of a window of --steps eager steps (forward + dice_bce_mc loss + backward
                    + SGD), device events around the window; --warmup steps of each mode run first
  per_layer         the 17 DoubleConv 3x3 shapes that read >= 8 channels (the Ci = 1 stem stays on the generic kernel in both modes):
                    forward (BatchNorm/ReLU on load, statistics epilogue) and weight gradient, per launch, both kernels; TFLOP/s =
                    2 * N * H * W * 9 * Ci * Co over the launch time, `frac` = the matrix-core kernel's share of the 157.3 TFLOP/s
                    fp32 peak (compute-bound at every layer: >= 144 FLOP/B)
  rounding          largest |result - float64| / (gamma_2K * sum |a b|) of forward, data gradient and weight gradient on
                    standard-normal data (the bound and shapes of tests/test_gpu_conv_f32_mfma.py; float64 on the host)
  outputs_agree     the two modes' forward kernels on the same operands at every timed shape: largest difference over largest value

Prints one JSON line; --out writes it (profiles/f32_mfma_step.json is the record README and DESIGN quote).  No GPU: fails.
"""
import argparse
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
CIN, NCLS, FEAT, SIZE, BATCH = 1, 2, 64, 512, 4
MODES = ("fp32", "fp32_mfma")


def double_conv_shapes(cin, f, H, W, B):
    """(name, N, H, W, Ci, Co) of the 18 3x3 convs of the nine DoubleConvs."""
    out, chans = [], [f * 2 ** i for i in range(5)]
    h, w, prev = H, W, cin
    for i, c in enumerate(chans):
        if i:
            h, w = h // 2, w // 2
        out += [(f"enc{i}.c1", B, h, w, prev, c), (f"enc{i}.c2", B, h, w, c, c)]
        prev = c
    for i in range(4):
        c = chans[3 - i]
        h, w = h * 2, w * 2
        out += [(f"dec{i}.c1", B, h, w, 2 * c, c), (f"dec{i}.c2", B, h, w, c, c)]
    return out


def event_ms(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def time_steps(steps, warmup, windows):
    import Model
    import loss as L
    from umi import optim as umi_optim
    L.CLASS_NUMBER = NCLS
    torch.manual_seed(0)
    g = torch.Generator(device=DEV)
    g.manual_seed(1234)
    x = torch.randn(BATCH, CIN, SIZE, SIZE, device=DEV, generator=g)
    labels = torch.randint(0, NCLS, (BATCH, SIZE, SIZE), device=DEV, generator=g).float()
    runs, state = {}, None
    for mode in MODES:
        m = Model.UNet(CIN, NCLS, FEAT, compute_dtype=mode)
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
    out = {mode: {"median_ms": round(statistics.median(v), 3), "samples_ms": [round(s, 3) for s in v],
                  "first_step_loss": first_loss[mode]} for mode, v in samples.items()}
    return out


def time_layers(reps):
    from umi import lib, ops
    rows, worst = [], 0.0
    for name, n, h, w, ci, co in double_conv_shapes(CIN, FEAT, SIZE, SIZE, BATCH):
        if ci % 8:
            continue
        x = torch.randn(n, h, w, ci, device=DEV)
        dy = torch.randn(n, h, w, co, device=DEV)
        wgt = torch.randn(co, ci, 3, 3, device=DEV) * (2.0 / (9 * ci)) ** 0.5
        tx = ops.passthrough_tx(ci, DEV)
        tx[:, 3] = 0.0                                   # BatchNorm-apply + ReLU on load, like the real step
        wp = ops.pack_conv_fwd(wgt, torch.float32)
        gw = torch.empty(co, ci, 3, 3, device=DEV)
        gflop = 2.0 * n * h * w * 9 * ci * co / 1e9
        row = {"conv": name, "N": n, "H": h, "W": w, "Ci": ci, "Co": co, "gflop": round(gflop, 2)}
        ys = {}
        for key, flags in (("fp32", 0), ("fp32_mfma", lib.CONV_F32_MFMA)):
            y = torch.empty(n, h, w, co, device=DEV)
            lay, _ = ops.conv_plan(x, y, 3, 3, 1, 1, flags)
            assert lay == 0

            def fwd():
                ops.conv_fwd(x, tx, lambda _l: wp, None, y, 3, 3, 1, 1, want_stats=True, flags=flags)

            def wgrad():
                ops.conv_wgrad(x, tx, dy, None, gw, ci * 9, 9, 1, 1.0, 3, 3, 1, 1, flags=flags)
            fwd(), wgrad()                               # warm-up of this shape
            torch.cuda.synchronize()
            fms, wms = event_ms(fwd, reps), event_ms(wgrad, reps)
            row[key] = {"fwd_ms": round(fms, 4), "fwd_tflops": round(gflop / fms, 2),
                        "wgrad_ms": round(wms, 4), "wgrad_tflops": round(gflop / wms, 2)}
            ys[key] = y
        row["fwd_frac_of_f32_peak"] = round(row["fp32_mfma"]["fwd_tflops"] / PEAK_F32_TFLOPS, 4)
        worst = max(worst, ((ys["fp32"] - ys["fp32_mfma"]).abs().max() / ys["fp32"].abs().max()).item())
        rows.append(row)
        del x, dy, wgt, wp, gw, ys
    tot = {k: sum(r[k]["fwd_ms"] for r in rows) for k in MODES}
    fl = sum(r["gflop"] for r in rows)
    summary = {k: {"fwd_ms_17_launches": round(tot[k], 3), "fwd_tflops": round(fl / tot[k], 2)} for k in MODES}
    return rows, summary, worst


def rounding_ratios():
    """The bound of tests/test_gpu_conv_f32_mfma.py: any order of K fused products, gamma_2K * sum |a b|, u = 2^-24."""
    from umi import lib, ops
    u = 2.0 ** -24

    def ratio(got, ref, mag, K):
        return round(((got.double().cpu() - ref).abs() / (2 * K * u / (1 - 2 * K * u) * mag)).max().item(), 5)
    out = {}
    for N, H, W, Ci, Co in ((1, 16, 32, 64, 64), (1, 8, 16, 512, 256)):
        g = torch.Generator().manual_seed(N + H + W + Ci + Co)
        x, w = torch.randn(N, H, W, Ci, generator=g), torch.randn(Co, Ci, 3, 3, generator=g)
        dy = torch.randn(N, H, W, Co, generator=g)
        x64, w64, dy64 = x.double().permute(0, 3, 1, 2), w.double(), dy.double().permute(0, 3, 1, 2)
        y, dx = torch.empty(N, H, W, Co, device=DEV), torch.empty(N, H, W, Ci, device=DEV)
        wd = w.to(DEV)
        ops.conv_fwd(x.to(DEV), None, lambda _l: ops.pack_conv_fwd(wd, torch.float32), None, y, 3, 3, 1, 1, flags=lib.CONV_F32_MFMA)
        ops.conv_fwd(dy.to(DEV), None, lambda _l: ops.pack_conv_dgrad(wd, torch.float32), None, dx, 3, 3, 1, 1, flags=lib.CONV_F32_MFMA)
        key = f"{N}x{H}x{W}x{Ci}->{Co}"
        out["fwd " + key] = ratio(y, F.conv2d(x64, w64, None, 1, 1).permute(0, 2, 3, 1),
                                  F.conv2d(x64.abs(), w64.abs(), None, 1, 1).permute(0, 2, 3, 1), 9 * Ci)
        out["dgrad " + key] = ratio(dx, F.conv_transpose2d(dy64, w64, None, 1, 1).permute(0, 2, 3, 1),
                                    F.conv_transpose2d(dy64.abs(), w64.abs(), None, 1, 1).permute(0, 2, 3, 1), 9 * Co)
    N, H, W, Ci, Co = 2, 32, 32, 64, 64
    g = torch.Generator().manual_seed(N + H + W + Ci + Co)
    x, dy = torch.randn(N, H, W, Ci, generator=g), torch.randn(N, H, W, Co, generator=g)
    x64, dy64 = x.double().permute(0, 3, 1, 2), dy.double().permute(0, 3, 1, 2)
    wr = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x64, wr, None, 1, 1).backward(dy64)
    wa = torch.zeros(Co, Ci, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(x64.abs(), wa, None, 1, 1).backward(dy64.abs())
    gw = torch.empty(Co, Ci, 3, 3, device=DEV)
    ops.conv_wgrad(x.to(DEV), None, dy.to(DEV), None, gw, Ci * 9, 9, 1, 1.0, 3, 3, 1, 1, flags=lib.CONV_F32_MFMA)
    out[f"wgrad {N}x{H}x{W}x{Ci}->{Co}"] = ratio(gw, wr.grad, wa.grad, N * H * W)
    out["largest"] = max(out.values())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=3, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=2, help="eager warm-up steps per mode")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per mode, the modes alternating")
    ap.add_argument("--reps", type=int, default=10, help="launches per per-layer timing")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "f32_mfma_step.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_f32: needs an MI355X (no device found); nothing is measured on the host")
    rounding = rounding_ratios()
    layers, layer_sum, agree = time_layers(a.reps)
    steps = time_steps(a.steps, a.warmup, a.windows)
    res = {"workload": f"UNet({CIN},{NCLS},{FEAT}) {SIZE}x{SIZE} batch {BATCH}, eager training step, dice_bce_mc + SGD",
           "device": torch.cuda.get_device_name(0), "peak_f32_tflops": PEAK_F32_TFLOPS,
           "step_ms": steps, "step_speedup_fp32_over_fp32_mfma": round(steps["fp32"]["median_ms"] / steps["fp32_mfma"]["median_ms"], 3),
           "steps_per_window": a.steps, "per_layer_fwd_summary": layer_sum, "per_layer": layers,
           "outputs_agree_rel": agree, "rounding_ratio_to_bound": rounding}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
