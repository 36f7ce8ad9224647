#!/usr/bin/env python3
"""Times the class-aware component labelling (csrc/components.hip, umi.infer.label_class_components) on one MI355X against
what the binary kernels offer for the same result: K - 1 calls of umi.infer.label_components on `mask == c`, the compare
launches included.

Sizes 512^2 x 16, 768^2 x 1 and 768^2 x 16; K = 3 and K = 4; two mask families:
  blobs    a seeded noise field, box-blurred and thresholded, every blob (8-connected component of the thresholded field) given
           one seeded class;
  pixels   a seeded class per pixel (background with probability 0.5).
Each figure is the time per call from device events around 50 back-to-back calls after warm-up; every measurement is repeated
three times (all three are recorded; `one_pass_ms` is their median, `chain_min_ms` the smallest of the chain's three).
`one_pass_wins` says whether one_pass_ms < chain_min_ms.  `algo_gbps` is (mask bytes read + label bytes written) / one_pass_ms
and `hbm_fraction` that over the 8 TB/s HBM peak: information only, the passes are latency- and atomics-bound, not streaming.

--bench also alternates `python bench.py --gpus 1 --steps K --warmup W` of this tree with that of --parent-tree DIR (a built
checkout of the parent commit) for --bench-rounds rounds, so that a change in the training step would show.
Prints one JSON line; --out writes it.
Per-kernel times: `rocprofv3 --kernel-trace --stats -- python tools/bench_class_components.py --calls 5 --repeats 1`.
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda"
HBM_PEAK = 8.0e12
SIZES = ((16, 512, 512), (1, 768, 768), (16, 768, 768))


def blob_mask(seed, shape, K):
    from umi.components import label_components_numpy
    rng = np.random.default_rng(seed)
    N, H, W = shape
    out = np.zeros(shape, dtype=np.uint8)
    k = 9
    for n in range(N):
        f = rng.standard_normal((H + k - 1, W + k - 1))
        c = np.cumsum(np.cumsum(np.pad(f, ((1, 0), (1, 0))), axis=0), axis=1)
        blur = (c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]) / (k * k)
        lab, cnt, *_ = label_components_numpy(blur > 0.6 * blur.std())
        cls = np.concatenate([[0], rng.integers(1, K, int(cnt[0]))]).astype(np.uint8)
        out[n] = cls[lab]
    return out


def pixel_mask(seed, shape, K):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < 0.5, rng.integers(1, K, shape), 0).astype(np.uint8)


def event_ms(fn, calls, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--bench-steps", type=int, default=30)
    ap.add_argument("--bench-warmup", type=int, default=8)
    ap.add_argument("--parent-tree")
    ap.add_argument("--bench-rounds", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_class_components.py measures on the MI355X"
    from umi import infer
    res = {"device": torch.cuda.get_device_name(0), "calls": a.calls, "repeats": a.repeats, "cases": {}}
    for K in (3, 4):
        for shape in SIZES:
            for family, make in (("blobs", blob_mask), ("pixels", pixel_mask)):
                m = make(1000 * K + shape[0] + shape[1], shape, K)
                md = torch.from_numpy(m).to(DEV)

                def one_pass():
                    return infer.label_class_components(md, K)

                def chain():
                    return [infer.label_components((md == c).view(torch.uint8)) for c in range(1, K)]
                # the two give the same counts before they are timed
                got = one_pass()
                infer.label_class_components(md, K, check=True)
                per_class = torch.stack([o[1] for o in chain()], dim=1)
                assert torch.equal(got[2][:, 1:], per_class)
                one = [event_ms(one_pass, a.calls) for _ in range(a.repeats)]
                ch = [event_ms(chain, a.calls) for _ in range(a.repeats)]
                cnt = event_ms(lambda: infer.count_class_objects(md, K), a.calls)
                one_ms, ch_min = float(np.median(one)), min(ch)
                nbytes = m.size * 5
                res["cases"][f"k{K}_{shape[1]}x{shape[2]}x{shape[0]}_{family}"] = {
                    "components_per_image": float(got[1].float().mean().item()),
                    "one_pass_all_ms": one, "chain_all_ms": ch, "one_pass_ms": one_ms, "chain_min_ms": ch_min,
                    "one_pass_wins": bool(one_ms < ch_min), "count_class_objects_ms": cnt,
                    "algo_gbps": nbytes / (one_ms * 1e-3) / 1e9, "hbm_fraction": nbytes / (one_ms * 1e-3) / HBM_PEAK}
    res["k3_one_pass_wins_everywhere"] = all(v["one_pass_wins"] for k, v in res["cases"].items() if k.startswith("k3_"))
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
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
