#!/usr/bin/env python3
"""Times the fp32 ConvTranspose2d(2, 2) of the four `Up` levels of UNet(., ., 64) at 512 x 512, batch 4, on one MI355X with
UMI_CONV_F32_MFMA_2X2 (the fp32-input matrix-core kernels of csrc/convt_mfma_f32.hip) and without it (the LDS-tiled VALU kernels of
csrc/generic_kernels.hip), in one process on one box, the variants alternating.

  per_level         the four levels (32 x 32 ... 256 x 256 in, 1024 -> 512 ... 128 -> 64 channels) as the tape calls them: the forward
                    (input transform, bias, written into the upper channel half of a concat buffer), the data gradient and the
                    weight gradient (the transform on the ConvT's input), per launch; per variant the median of --windows windows of
                    --reps launches, device events around a window, every level warmed up first.  Variants: "base" (no flag),
                    "mfma" (the flag), "base_again" (no flag, timed a second time: the A/A measure of spread).  TFLOP/s =
                    2 * M * Cin * 4 Cout over the launch time, `frac` = the flagged call's share of the 157.3 TFLOP/s fp32 peak.
                    `mfma_slower_by` = mfma / base - 1, `aa_spread` = |base_again / base - 1|; `loses` = the flagged call does not
                    beat the flag-less one by more than that spread.
  step_ms           the eager training step of UNet(1, 2, 64) at 512 x 512, batch 4 (forward + dice_bce_mc loss + backward + SGD)
                    under compute_dtype "fp32_mfma" and "fp32_mfma_convt", and "fp32_mfma" a second time (A/A): the median and every
                    sample of windows of --steps steps, the modes alternating, with first-step losses
  generic_2x2_calls the 2x2 calls that UMI_TRACE_GENERIC=1 reports on the generic kernels in one UNet(1, 2, 64) step under
                    "fp32_mfma_convt" (expected: none)

Each part runs in a child process of its own under its own time limit, with at most 16 CPU threads; the parent never opens the GPU.
Prints one JSON line; --out writes it (profiles/f32_convt_mfma.json is the record README and DESIGN quote).  No GPU: fails.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]

DEV = "cuda"
PEAK_F32_TFLOPS = 157.3
BATCH, SIZE, FEAT = 4, 512, 64
MODES = ("fp32_mfma", "fp32_mfma_convt", "fp32_mfma_again")
VARIANTS = ("base", "mfma", "base_again")
OPS = ("fwd", "dgrad", "wgrad")
# (name, h = w of the ConvT's input, Cin, Cout)
LEVELS = [("up1", SIZE // 16, 16 * FEAT, 8 * FEAT), ("up2", SIZE // 8, 8 * FEAT, 4 * FEAT), ("up3", SIZE // 4, 4 * FEAT, 2 * FEAT),
          ("up4", SIZE // 2, 2 * FEAT, FEAT)]
LIMITS = {"levels": 240, "step": 420, "trace": 180}          # seconds per part


def event_ms(fn, reps):
    import torch
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def time_levels(reps, windows):
    import torch
    from umi import lib, ops
    flag, up = lib.CONV_F32_MFMA_2X2, lib.CONV_UPSAMPLE2
    rows = []
    for name, hw, cin, cout in LEVELS:
        n, M = BATCH, BATCH * hw * hw
        x, g = torch.randn(n, hw, hw, cin, device=DEV), torch.randn(n, 2 * hw, 2 * hw, cout, device=DEV)
        wgt = torch.randn(cin, cout, 2, 2, device=DEV) * cin ** -0.5
        bias = torch.randn(cout, device=DEV)
        tx = torch.zeros(cin, 4, device=DEV)
        tx[:, 1], tx[:, 2] = torch.rand(cin, device=DEV) + 0.5, torch.randn(cin, device=DEV)      # BatchNorm scale / shift, ReLU
        wp, wpd = ops.pack_convT_fwd(wgt, torch.float32), ops.pack_convT_dgrad(wgt, torch.float32)
        cat = torch.empty(n, 2 * hw, 2 * hw, 2 * cout, device=DEV)
        dest, dx, gw = cat[..., cout:], torch.empty(n, hw, hw, cin, device=DEV), torch.empty(cin, cout, 2, 2, device=DEV)
        assert ops.conv_plan(x, dest, 2, 2, 2, 0, flag | up, True) == (0, 0)         # the new paths are named
        assert ops.conv_plan(g, dx, 2, 2, 2, 0, flag) == (0, 0)

        def calls(f):
            return {"fwd": lambda: ops.conv_fwd(x, tx, lambda _l: wp, bias, dest, 2, 2, 2, 0, flags=up | f),
                    "dgrad": lambda: ops.conv_fwd(g, None, lambda _l: wpd, None, dx, 2, 2, 2, 0, flags=f),
                    "wgrad": lambda: ops.conv_wgrad(g, None, x, tx, gw, cout * 4, 4, 1, 1.0, 2, 2, 2, 0, flags=f)}
        fns = {"base": calls(0), "mfma": calls(flag), "base_again": calls(0)}
        for v in VARIANTS:                               # warm-up of this level, every variant
            for f in fns[v].values():
                f()
        torch.cuda.synchronize()
        gflop = 2.0 * M * cin * 4 * cout / 1e9
        row = {"level": name, "in": f"{hw}x{hw}", "M": M, "Cin": cin, "Cout": cout, "gflop": round(gflop, 3)}
        for op in OPS:
            samples = {v: [] for v in VARIANTS}
            for _ in range(windows):
                for v in VARIANTS:                       # the variants alternate
                    samples[v].append(event_ms(fns[v][op], reps))
            ms = {v: statistics.median(s) for v, s in samples.items()}
            slower, spread = ms["mfma"] / ms["base"] - 1.0, abs(ms["base_again"] / ms["base"] - 1.0)
            row[op] = {"base_ms": round(ms["base"], 4), "mfma_ms": round(ms["mfma"], 4), "base_again_ms": round(ms["base_again"], 4),
                       "base_tflops": round(gflop / ms["base"], 2), "mfma_tflops": round(gflop / ms["mfma"], 2),
                       "frac_of_f32_peak": round(gflop / ms["mfma"] / PEAK_F32_TFLOPS, 4), "speedup": round(ms["base"] / ms["mfma"], 3),
                       "mfma_slower_by": round(slower, 4), "aa_spread": round(spread, 4), "loses": bool(slower > -spread)}
        rows.append(row)
        del x, g, wgt, wp, wpd, cat, dest, dx, gw
    return rows


def _model_and_step(mode, state, x, labels):
    import Model
    import loss as L
    from umi import optim as umi_optim
    m = Model.UNet(1, 2, FEAT, False, compute_dtype=mode)
    if state:
        m.load_state_dict(state)
    m.to(DEV).train()
    opt = umi_optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)

    def step():
        loss = L.calc_loss(m(x), labels, loss_type="dice_bce_mc")
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss
    return m, step


def _batch(batch, size):
    import torch
    import loss as L
    L.CLASS_NUMBER = 2
    torch.manual_seed(0)
    return torch.randn(batch, 1, size, size, device=DEV), torch.randint(0, 2, (batch, size, size), device=DEV).float()


def time_steps(steps, warmup, windows):
    import torch
    x, labels = _batch(BATCH, SIZE)
    runs, state = {}, None
    for mode in MODES:
        m, runs[mode] = _model_and_step(mode.replace("_again", ""), state, x, labels)
        if state is None:                                # every mode starts from the same weights
            state = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
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


def trace_step():
    """One step at 64 x 64, batch 1 (the same 22 layers and four ConvTs, every channel count as at 512 x 512): the library's trace
    lines go to stderr, the parent reads them."""
    import torch
    x, labels = _batch(1, 64)
    _, step = _model_and_step("fp32_mfma_convt", None, x, labels)
    loss = float(step().item())
    torch.cuda.synchronize()
    return {"loss": loss}


def child(part, a):
    import torch
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    if not torch.cuda.is_available():
        sys.exit("bench_f32_convt: needs an MI355X (no device found); nothing is measured on the host")
    if part == "levels":
        res = {"device": torch.cuda.get_device_name(0), "per_level": time_levels(a.reps, a.windows)}
    elif part == "step":
        res = time_steps(a.steps, a.warmup, a.windows)
    else:
        res = trace_step()
    with open(a.child_out, "w") as fh:
        json.dump(res, fh)


def run_part(part, a, env_extra=None):
    """The part in a fresh child under its own time limit; returns (its result, its stderr)."""
    env = dict(os.environ, **(env_extra or {}))
    for k in ("OMP_NUM_THREADS", "MKL_NUM_THREADS"):
        env[k] = str(min(16, int(env.get(k) or 16)))
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, part + ".json")
        cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--child-out", out, "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--windows", str(a.windows), "--reps", str(a.reps)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[part], env=env)
        if p.returncode != 0:
            sys.exit(f"bench_f32_convt: part {part!r} ended with status {p.returncode}; nothing further is run\n{p.stderr[-3000:]}")
        with open(out) as fh:
            return json.load(fh), p.stderr


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=3, help="steps per timed window")
    ap.add_argument("--warmup", type=int, default=2, help="eager warm-up steps per mode")
    ap.add_argument("--windows", type=int, default=5, help="timed windows per variant / mode, alternating")
    ap.add_argument("--reps", type=int, default=10, help="launches per per-level window")
    ap.add_argument("--no-step", action="store_true", help="skip the full-model step and the trace (per-level timings only)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "f32_convt_mfma.json"))
    ap.add_argument("--part", choices=tuple(LIMITS), help=argparse.SUPPRESS)
    ap.add_argument("--child-out", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.part:
        return child(a.part, a)
    levels, _ = run_part("levels", a)
    losing = [f"{r['level']} {op}" for r in levels["per_level"] for op in OPS if r[op]["loses"]]
    res = {"workload": f"UNet(., ., {FEAT}) {SIZE}x{SIZE} batch {BATCH}: the fp32 ConvTranspose2d(2, 2) of the four Up levels, per launch",
           "device": levels["device"], "peak_f32_tflops": PEAK_F32_TFLOPS, "reps_per_window": a.reps, "windows": a.windows,
           "per_level": levels["per_level"], "not_faster_beyond_the_aa_spread": losing}
    for op in OPS:
        res[f"sum_{op}_ms"] = {v: round(sum(r[op][v + "_ms"] for r in levels["per_level"]), 4) for v in VARIANTS}
    if not a.no_step:
        steps, _ = run_part("step", a)
        base, new, again = (steps[m]["median_ms"] for m in MODES)
        res["step_ms"], res["steps_per_window"] = steps, a.steps
        res["step_speedup_fp32_mfma_over_fp32_mfma_convt"] = round(base / new, 3)
        res["step_aa_spread"] = round(abs(again / base - 1.0), 4)
        res["step_slower_beyond_the_aa_spread"] = bool(new / base - 1.0 > abs(again / base - 1.0))
        _, err = run_part("trace", a, {"UMI_TRACE_GENERIC": "1"})
        lines = [ln for ln in err.splitlines() if ln.startswith("[umi generic")]
        res["generic_calls_in_a_step"] = len(lines)
        res["generic_2x2_calls"] = [ln for ln in lines if " R=2 " in ln]
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
