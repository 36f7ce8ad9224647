#!/usr/bin/env python3
"""Times the localisation scoring kernels (csrc/matching.hip) on one MI355X.

For each size -- 512x512 with 100 dots, 768x768 with 400 and with 2,000 dots, centres = the dots jittered plus 5 % spurious
ones -- and batch 1 and 16, after warm-up, device events around --replays (>= 20) back-to-back calls:

  crowd_match_ms      umi.matching.crowd_match, 2 sigmas x 10 thresholds (the reference's table)
  distance_match_ms   umi.matching.distance_match, threshold 10
  dot_lists_ms        umi.matching.dot_lists of the float32 dot maps
  numpy_crowd_ms_per_image / numpy_distance_ms_per_image
                      the in-tree NumPy statements on ONE image of the batch, host clock, in the same run (their results are
                      compared with the device's for that image)

The reference's own CrowdMatchingTest is far slower than the NumPy statement (full-image float64 maps per centre); its
recorded wall times are in tests/golden/crowd_matching.npz (cm_<case>_seconds).  Prints one JSON line; --out writes it.
Per-kernel times: run this program under `rocprofv3 --kernel-trace --stats -- python tools/bench_matching.py`.
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda"
SIGMAS = [5, 20]
THRESHOLDS = list(np.arange(0.5, 1, 0.05))
SIZES = [(512, 100), (768, 400), (768, 2000)]


def event_ms(fn, replays):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(replays):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / replays


def make_batch(rng, B, size, n_dots):
    maps = np.zeros((B, size, size), dtype=np.float32)
    n_cent = n_dots + n_dots // 20
    centers = np.zeros((B, n_cent, 2), dtype=np.int32)
    for b in range(B):
        flat = rng.choice(size * size, n_dots, replace=False)
        ys, xs = flat // size, flat % size
        maps[b, ys, xs] = 1
        cx = np.concatenate([np.clip(xs + rng.integers(-8, 9, n_dots), 0, size - 1), rng.integers(0, size, n_cent - n_dots)])
        cy = np.concatenate([np.clip(ys + rng.integers(-8, 9, n_dots), 0, size - 1), rng.integers(0, size, n_cent - n_dots)])
        order = rng.permutation(n_cent)
        centers[b, :, 0], centers[b, :, 1] = cx[order], cy[order]
    return maps, centers, np.full(B, n_cent, dtype=np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_matching.py measures on the MI355X"
    assert a.replays >= 20
    from umi import matching as M
    res = {"device": torch.cuda.get_device_name(0), "replays": a.replays, "sigmas": SIGMAS, "thresholds": len(THRESHOLDS),
           "max_dots": M.MAX_DOTS, "cases": {}}
    rng = np.random.default_rng(10)
    for size, n_dots in SIZES:
        for B in (1, 16):
            maps, centers, c_count = make_batch(rng, B, size, n_dots)
            md, cd, ccd = (torch.from_numpy(x).to(DEV) for x in (maps, centers, c_count))
            dots, g_count = M.dot_lists(md, check=True)
            crowd = M.crowd_match(dots, g_count, cd, ccd, SIGMAS, THRESHOLDS)
            dist = M.distance_match(dots, g_count, cd, ccd, 10)
            hd, hg = M.dot_lists_numpy(maps[:1])
            t0 = time.perf_counter()
            want_c = M.crowd_match_numpy(hd, hg, centers[:1], c_count[:1], SIGMAS, THRESHOLDS)
            t1 = time.perf_counter()
            want_d = M.distance_match_numpy(hd, hg, centers[:1], c_count[:1], 10)
            t2 = time.perf_counter()
            assert np.array_equal(crowd[:1].cpu().numpy(), want_c) and np.array_equal(dist[:1].cpu().numpy(), want_d)
            res["cases"][f"{size}x{size}_dots{n_dots}_batch{B}"] = {
                "centres_per_image": int(c_count[0]),
                "crowd_match_ms": event_ms(lambda: M.crowd_match(dots, g_count, cd, ccd, SIGMAS, THRESHOLDS), a.replays),
                "distance_match_ms": event_ms(lambda: M.distance_match(dots, g_count, cd, ccd, 10), a.replays),
                "dot_lists_ms": event_ms(lambda: M.dot_lists(md), a.replays),
                "numpy_crowd_ms_per_image": (t1 - t0) * 1e3,
                "numpy_distance_ms_per_image": (t2 - t1) * 1e3,
                "tp_fp_sigma5_thresh0.5_image0": crowd[0, 0, 0].cpu().tolist(),
            }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
