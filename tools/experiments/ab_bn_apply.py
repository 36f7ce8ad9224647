"""Same-process A/B of umi_bn_bwd_apply across builds of libunetmi at the five (M, C) of the bench workload (batch 16).

usage: python tools/experiments/ab_bn_apply.py NAME=LIB.so [NAME=LIB.so ...] [--out FILE]
  e.g. parent=<built checkout of the parent commit>/unet-torch_amd/umi/libunetmi.so new=unet-torch_amd/umi/libunetmi.so
       wgs1024=tools/_ab/libunetmi_wgs1024.so   (python tools/build_variant.py wgs1024 elementwise_f16.hip -DBNA_WGS=1024)

Each timed apply follows a copy that has just written dA (as the step leaves it); y rotates over buffers that together
exceed the Infinity Cache.  Interleaved rounds; per build: median / min of (loop(copy + apply) - loop(copy)) / n, after a
check that every build leaves the same bits as the first."""
import ctypes, os, statistics, sys
from ctypes import c_int, c_long, c_void_p
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
args = sys.argv[1:]
OUT = args[args.index("--out") + 1] if "--out" in args else None
LIBS = dict(a.split("=", 1) for a in args if "=" in a)
assert LIBS, __doc__
DEV = "cuda"


def load(path):
    f = ctypes.CDLL(os.path.join(REPO, path)).umi_bn_bwd_apply
    f.restype = c_int
    f.argtypes = [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_long, c_int, c_int, c_void_p]
    return f


fns = {k: load(p) for k, p in LIBS.items()}
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


g = torch.Generator(device=DEV).manual_seed(7)
ROUNDS, N_IT = 7, 20
for (M, C) in [(16 * 512 * 512, 64), (16 * 256 * 256, 128), (16 * 128 * 128, 256), (16 * 64 * 64, 512), (16 * 32 * 32, 1024)]:
    nbytes = M * C * 2
    ny = max(1, min(20, -(-600_000_000 // nbytes))) if nbytes < 300_000_000 else 1
    ys = [torch.randn(M, C, device=DEV, generator=g).half() for _ in range(ny)]
    src = (0.1 * torch.randn(M, C, device=DEV, generator=g)).half()
    da = torch.empty_like(src)
    t = torch.empty(C, 4, device=DEV)
    t[:, 0] = 0.1 * torch.randn(C, device=DEV, generator=g)
    t[:, 1] = (0.5 + torch.rand(C, device=DEV, generator=g)) * torch.where(torch.rand(C, device=DEV, generator=g) < 0.2, -1.0, 1.0)
    t[:, 2] = 0.2 * torch.randn(C, device=DEV, generator=g)
    t[:, 3] = 0.0
    rstd = 0.5 + torch.rand(C, device=DEV, generator=g)
    sums = torch.randn(2, C, device=DEV, generator=g) * 0.05 * M
    st = torch.cuda.current_stream().cuda_stream

    def call(f, y):
        rc = f(da.data_ptr(), C, y.data_ptr(), C, t.data_ptr(), rstd.data_ptr(), sums[0].data_ptr(), sums[1].data_ptr(), M, C, 1, st)
        assert rc == 0, rc

    ref = None
    for k, f in fns.items():
        da.copy_(src)
        call(f, ys[0])
        torch.cuda.synchronize()
        out = da.view(torch.int16).clone()
        if ref is None:
            ref = out
        same = torch.equal(out, ref)
        assert same, (k, M, C)
    del ref, out

    def loop(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(N_IT):
            da.copy_(src)
            if f is not None:
                call(f, ys[i % ny])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / N_IT         # us per iteration

    for f in list(fns.values()) + [None]:
        loop(f)
    ts = {k: [] for k in fns}
    base = []
    for r in range(ROUNDS):
        base.append(loop(None))
        for k, f in fns.items():
            ts[k].append(loop(f))
    b = statistics.median(base)
    say(f"M={M} C={C} traffic {3 * nbytes / 1e6:.0f} MB  y buffers {ny}  copy alone {b:.1f} us (min {min(base):.1f} max {max(base):.1f}); all builds bit-identical")
    for k in fns:
        med, mn = statistics.median(ts[k]) - b, min(ts[k]) - b
        say(f"    {k:10s} median {med:7.1f} us  min {mn:7.1f} us   {3 * nbytes / med / 1e6:5.2f} TB/s   all: " + " ".join(f"{x - b:.1f}" for x in ts[k]))
    del ys, src, da
if OUT:
    with open(OUT, "w") as fh:
        fh.write("\n".join(lines) + "\n")
