#!/usr/bin/env python3
"""Times the binary inference path's component labelling (csrc/components.hip) on one MI355X.

For each input at (16, 1, 512, 512) -- random masks at the fixture's densities, the checkerboard, the serpentine and all foreground -- after
warm-up, wall time around a device synchronise over at least --min-seconds of calls:

  label_ms        umi.infer.label_components (labels, counts, area, coordinate sums)
  count_ms        umi.infer.count_objects
  mraccuracy_ms   loss.MRAccuracy on device logits and dot maps (threshold + count + dot sums + one read-back)
  host_numpy_ms   the reference's procedure on the same box: device -> host copy of the logits, threshold, and a CPU labelling
                  per image (umi.components, NumPy)
  host_scipy_ms   the same with scipy.ndimage.label where SciPy is installed, else null

--bench also runs `python bench.py --gpus 1 --steps K --warmup W` in a child process and stores its line, next to the newest
recorded line of the parent tree, so that a change in the training step would show; with --parent-tree DIR (a built checkout
of the parent commit) the two trees' bench.py are alternated for --bench-rounds rounds on this box and both are recorded.
Prints one JSON line; --out writes it.
Per-kernel times: run this program under `rocprofv3 --kernel-trace --stats -- python tools/bench_components.py --min-seconds 0.2`.
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda"


def timed_ms(fn, min_seconds, sync=True):
    for _ in range(3):
        fn()
    if sync:
        torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        for _ in range(5):
            fn()
        n += 5
        if sync:
            torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return dt / n * 1e3


def inputs():
    from tools import gen_golden_binary_infer as G
    B, H, W = 16, 512, 512
    out = {}
    for k, d in enumerate(G.DENSITIES):
        out[f"random_d{d}"] = (np.random.default_rng(50 + k).random((B, H, W)) < d).astype(np.uint8)
    out["checkerboard"] = np.broadcast_to((np.indices((H, W)).sum(0) % 2).astype(np.uint8), (B, H, W)).copy()
    out["serpentine"] = np.broadcast_to(G._serpentine(H, W), (B, H, W)).copy()
    out["ones"] = np.ones((B, H, W), dtype=np.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--bench-steps", type=int, default=20)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--parent-tree")
    ap.add_argument("--bench-rounds", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_components.py measures on the MI355X"
    import loss as L
    from umi import components as C, infer
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    res = {"device": torch.cuda.get_device_name(0), "shape": [16, 1, 512, 512], "min_seconds": a.min_seconds, "cases": {}}
    rng = np.random.default_rng(9)
    for name, m in inputs().items():
        md = torch.from_numpy(m).to(DEV)
        logits = torch.where(md.bool(), 1.0, -1.0).unsqueeze(1).contiguous()
        target = torch.from_numpy((rng.random(m.shape) < 0.002).astype(np.float32)).to(DEV)
        counts = infer.label_components(md, check=True)[1].cpu().tolist()

        def host(label):
            pb = (torch.sigmoid(logits.squeeze(1)).cpu().numpy() >= 0.5).astype(np.uint8)
            return [label(pb[b]) for b in range(pb.shape[0])]
        case = {
            "components_per_image": counts[0],
            "label_ms": timed_ms(lambda: infer.label_components(md), a.min_seconds),
            "count_ms": timed_ms(lambda: infer.count_objects(md), a.min_seconds),
            "mraccuracy_ms": timed_ms(lambda: L.MRAccuracy(logits, target), a.min_seconds),
            "host_numpy_ms": timed_ms(lambda: host(C.count_components_numpy), a.min_seconds),
            "host_scipy_ms": None if ndimage is None else timed_ms(
                lambda: host(lambda im: ndimage.label(im, structure=np.ones((3, 3)))[1]), a.min_seconds),
        }
        assert host(C.count_components_numpy) == counts
        res["cases"][name] = case
    worst = max(res["cases"], key=lambda k: res["cases"][k]["label_ms"])
    res["worst_case"] = {"name": worst, "label_ms": res["cases"][worst]["label_ms"]}
    if a.bench:
        def bench(tree):
            cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup)]
            p = subprocess.run(cmd, capture_output=True, text=True, cwd=tree, timeout=900)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
            if p.returncode or not lines:
                raise RuntimeError(f"bench.py in {tree} failed ({p.returncode}): {p.stderr[-2000:]}")
            return json.loads(lines[-1])
        torch.cuda.synchronize()
        res["bench_py_cmd"] = f"python bench.py --gpus 1 --steps {a.bench_steps} --warmup {a.bench_warmup}"
        if a.parent_tree:
            rounds = [(bench(a.parent_tree), bench(REPO)) for _ in range(a.bench_rounds)]
            res["bench_py"] = {"line": rounds[-1][1], "ms_per_step_all": [r[1]["ms_per_step"] for r in rounds]}
            res["bench_py_parent"] = {"note": "the parent commit's tree, alternated with this one on the same box",
                                      "line": rounds[-1][0], "ms_per_step_all": [r[0]["ms_per_step"] for r in rounds]}
        else:
            res["bench_py"] = {"line": bench(REPO)}
            res["bench_py_parent"] = {"note": "not re-measured on this box; boxes of the pool differ by about 6 %"}
        res["bench_py_parent"]["recorded"] = {"BENCH_r03.json ms_per_step": 21.241,
                                              "profiles/r05_binloss_bench_n1.json": "no bench.py line (its graph-replayed "
                                                                                    "UNet(1,1,64) BCE step: 21.97 ms)"}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
