"""Host cost of umi_conv_fwd_plan, two builds of libunetmi alternating (the eager multi-GPU path asks the plan once per
convolution).  CPU only.

    python tools/ab_plan_host.py A.so B.so [runs=5] [calls=1000000]

Each run is a fresh process (UMI_LIB_OVERRIDE) that times `calls` plan queries through ctypes over the layer shapes of the
benchmark's U-Net step (bench.py defaults: batch 16, 512 x 512, 64 features, fp16): forward, data-gradient, transposed-conv and
head problems of every level."""
import ctypes
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def shapes():
    out, N = [], 16
    chans = [(1, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512), (512, 1024), (1024, 1024)]
    for i, (ci, co) in enumerate(chans):
        hw = 512 >> (i // 2)
        out.append((N, hw, hw, ci, co, 3, 3, 1, 1, ci if ci % 8 == 0 else 8, co, 1, 1, 0, 0))          # forward
        out.append((N, hw, hw, co, ci, 3, 3, 1, 1, co, ci if ci % 8 == 0 else 8, 1, 1, 0, 0))          # data gradient
    for lvl, c in enumerate((1024, 512, 256, 128)):
        hw = 32 << lvl
        out.append((N, hw, hw, c, c // 2, 2, 2, 1, 0, c, c, 1, 1, 1, 1))                               # ConvTranspose2d(2, 2) forward
        out.append((N, 2 * hw, 2 * hw, c // 2, c, 2, 2, 2, 0, c, c, 1, 1, 0, 0))                       # ... its data gradient
        out.append((N, 2 * hw, 2 * hw, c, c // 2, 3, 3, 1, 1, c, c // 2, 1, 1, 0, 0))                  # decoder conv on the concat
    out.append((N, 512, 512, 64, 2, 1, 1, 1, 0, 64, 2, 1, 0, 0, 1))                                    # OutConv (fp32 logits, bias)
    out.append((N, 512, 512, 2, 64, 1, 1, 1, 0, 8, 64, 1, 1, 0, 0))                                    # ... its data gradient
    return out


def child(calls):
    sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
    from umi import lib
    plan, lay, rows = lib.fn("umi_conv_fwd_plan"), ctypes.c_int(), ctypes.c_int()
    a, b = ctypes.byref(lay), ctypes.byref(rows)
    sh = shapes()
    assert all(plan(*s, a, b) == 0 for s in sh)
    reps = calls // len(sh)
    t0 = time.perf_counter()
    for _ in range(reps):
        for s in sh:
            plan(*s, a, b)
    print("%.1f" % ((time.perf_counter() - t0) / (reps * len(sh)) * 1e9))


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(int(sys.argv[2]))
        sys.exit(0)
    libs = sys.argv[1:3]
    runs = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    calls = sys.argv[4] if len(sys.argv) > 4 else "1000000"
    ns = {p: [] for p in libs}
    for r in range(runs):
        for p in libs:
            o = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", calls], env=dict(os.environ, UMI_LIB_OVERRIDE=p),
                               capture_output=True, text=True, check=True)
            ns[p].append(float(o.stdout.split()[-1]))
            print("run %d  %-60s %8.1f ns/call" % (r + 1, p, ns[p][-1]), flush=True)
    for p in libs:
        print("%-60s min %.1f  median %.1f  max %.1f ns/call (ctypes overhead included)" % (p, min(ns[p]), statistics.median(ns[p]), max(ns[p])))
