#!/usr/bin/env python3
"""Times density-map scoring (umi.infer.score_density_maps, csrc/peaks.hip) on one MI355X against the host round trip it replaces.

The batch: 16 float32 count maps of 512 x 512 and of 768 x 768, each the sum of a few hundred Gaussian bumps (sigma 3), and a
dot map with one dot near most bumps.  In one process, in alternating rounds (device, host, device, host, ...), host clock around
work that ends in a synchronise:

  device_ms              score_density_maps on the device tensors (one device-to-host copy of the integers and sums)
  host_ms                the maps copied to the host + umi.peaks.score_density_numpy, the path a user had before
  aa_spread              per path, (max - min) / median over the rounds of that path: what the same code gives twice
  peak_lists_ms          umi_peak_lists alone (device events around back-to-back calls), also split d = 1 / 3 / 8
  copy_ms                a device-to-device copy of the same maps, the cost of touching the bytes once
  peaks_per_map          what the rule finds

The device dictionaries are compared with the statement's before anything is timed (integers and matching arrays ==).
No threshold is set: the record says whether the device path beats the host round trip by more than the spread, and by how much.
Prints one JSON line; --out writes it (profiles/density_inference.json is the record README quotes).
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
N = 16
SIGMAS, THRESHOLDS = [5, 20], np.arange(0.5, 1, 0.05)


def make_batch(size, bumps, seed):
    """N maps of `bumps` Gaussian bumps (sigma 3, unit mass each, drawn into their 25 x 25 window) and the dot maps."""
    rng = np.random.default_rng(seed)
    r = 12
    off = np.arange(-r, r + 1, dtype=np.float64)
    pred = np.zeros((N, size, size), dtype=np.float64)
    dots = np.zeros((N, size, size), dtype=np.uint8)
    for n in range(N):
        for k in range(bumps):
            cy, cx = rng.uniform(r, size - r - 1, 2)
            iy, ix = int(cy), int(cx)
            g = np.exp(-((off[:, None] + iy - cy) ** 2 + (off[None, :] + ix - cx) ** 2) / 18.0)
            pred[n, iy - r:iy + r + 1, ix - r:ix + r + 1] += g / g.sum()
            if k % 6:
                dots[n, int(np.clip(round(cy) + rng.integers(-2, 3), 0, size - 1)),
                     int(np.clip(round(cx) + rng.integers(-2, 3), 0, size - 1))] = 1
    return pred.astype(np.float32), dots


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


def clock_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def spread(ts):
    return (max(ts) - min(ts)) / float(np.median(ts))


def same(a, b):
    return all(a[k] == b[k] for k in ("GT", "peaks", "G1", "G2", "G3")) and \
        all(np.array_equal(a[k], b[k]) for k in ("arr_prec", "arr_recall", "arr_f1")) and abs(a["Pred"] - b["Pred"]) <= 1e-9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--bumps", type=int, default=300)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_density.py measures on the MI355X"
    assert a.rounds >= 3 and a.replays >= 20
    from umi import infer
    from umi import peaks as P
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "replays": a.replays, "maps": N, "bumps_per_map": a.bumps,
           "sigmas": SIGMAS, "thresholds": len(THRESHOLDS), "cases": {}}
    for size in (512, 768):
        pred, dots = make_batch(size, a.bumps, seed=size)
        pd, gd = torch.from_numpy(pred).to(DEV), torch.from_numpy(dots).to(DEV)

        def device():
            return infer.score_density_maps(pd, gd, SIGMAS, THRESHOLDS, size=size)

        def host():
            return P.score_density_numpy(pd.cpu().numpy(), gd.cpu().numpy(), SIGMAS, THRESHOLDS, size=size)

        got, want = device(), host()
        assert all(same(g, w) for g, w in zip(got, want)), "the device scores differ from the statement's"
        device()
        dev_t, host_t = [], []
        for _ in range(a.rounds):
            dev_t.append(clock_ms(device))
            host_t.append(clock_ms(host))
        case = {"peaks_per_map": [int(g["peaks"]) for g in got], "dots_per_map": [int(g["GT"]) for g in got],
                "device_ms": float(np.median(dev_t)), "host_ms": float(np.median(host_t)),
                "device_ms_rounds": dev_t, "host_ms_rounds": host_t,
                "aa_spread": {"device": spread(dev_t), "host": spread(host_t)}}
        case["host_over_device"] = case["host_ms"] / case["device_ms"]
        case["beats_host_beyond_spread"] = bool(max(dev_t) < min(host_t))
        case["peak_lists_ms"] = {str(d): event_ms(lambda d=d: P.peak_lists(pd, d), a.replays) for d in (1, 3, 8)}
        buf = torch.empty_like(pd)
        case["copy_ms"] = event_ms(lambda: buf.copy_(pd), a.replays)
        case["peak_lists_over_copy"] = case["peak_lists_ms"]["3"] / case["copy_ms"]
        case["map_bytes"] = pd.numel() * 4
        res["cases"][str(size)] = case
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
