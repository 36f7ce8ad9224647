#!/usr/bin/env python3
"""Times the crop datasets' device path (umi.augment CropPool / CropTransform, csrc/crops.hip) on one MI355X against the host
pipeline it replaces and against a plain device-to-device copy of the bytes it writes.

  train   one batch of 24 random 256 x 256 crops (image + int64 labels) out of a pool of 8 uint8 2048 x 2048 x 3 images, every
          third sample rot90 + flip, every third rotated
  grid    the 64 tiles of one 2048 x 2048 x 3 image of that pool with its labels

For each: `device_ms` = the kernels with their tables already on the device, device events around --replays back-to-back calls;
`device_with_draws_ms` (train) = CropTransform called with indices only: host draws, one upload, the kernels, host clock to a
synchronise; `copy_ms` = one device-to-device copy of as many bytes as the call writes (the floor for anything that produces
the batch on the device); `host_ms` = the NumPy statement per sample (or per image) plus the upload of its results, host clock,
one thread, median of 3.  Everything runs in ONE process in alternating rounds (device, copy, device again); the medians over
the rounds are reported, and `aa_spread` = the relative difference between the medians of the two device series of the same
code, the noise below which no difference means anything.  The device results are compared with the statement before anything is timed.
Prints one JSON line; --out writes it (profiles/crop_batches.json is the record README and DESIGN quote).
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = "cuda"
IMAGES, SIZE, C, N, CROP = 8, 2048, 3, 24, 256


def event_ms(fn, replays):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(replays):
        fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / replays


def host_ms(fn, reps=3):
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def rounds_ms(device, copy, rounds, replays):
    """Alternating rounds of (device, copy, device): medians and the A/A spread of the two device series."""
    for _ in range(5):
        device()
        copy()
    torch.cuda.synchronize()
    a, b, c = [], [], []
    for _ in range(rounds):
        a.append(event_ms(device, replays))
        c.append(event_ms(copy, replays))
        b.append(event_ms(device, replays))
    ma, mb = statistics.median(a), statistics.median(b)
    return {"device_ms": statistics.median(a + b), "copy_ms": statistics.median(c), "aa_spread": abs(ma - mb) / ma,
            "device_ms_min_max": [min(a + b), max(a + b)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_crops.py measures on the MI355X"
    assert a.replays >= 20 and a.rounds >= 3
    from umi import augment as A
    rng = np.random.default_rng(30)
    images = [(rng.random((SIZE, SIZE, C)) * 255).astype(np.uint8) for _ in range(IMAGES)]
    labels = [np.kron(rng.integers(0, 4, (SIZE // 16, SIZE // 16)).astype(np.uint8), np.ones((16, 16), np.uint8)) for _ in range(IMAGES)]
    pool = A.CropPool(images, labels).to(DEV)
    tf = A.CropTransform(CROP, True, py_rng=random.Random(31), np_rng=np.random.RandomState(32))
    crops, _ = A.draw_crop_params(pool.sizes, CROP, False, tf.py_rng, None, indices=np.arange(N) % IMAGES)
    params = np.zeros((N, 4), np.int32)
    for n in range(N):
        if n % 3 == 0:
            params[n] = (1, rng.integers(0, 4), rng.integers(0, 2), 0)
        elif n % 3 == 1:
            params[n] = (2, 0, 0, rng.integers(-20, 20))
    geom = A.batch_geometry(params, CROP, CROP)
    res = {"device": torch.cuda.get_device_name(0), "replays": a.replays, "rounds": a.rounds, "pool": [IMAGES, SIZE, SIZE, C],
           "image_dtype": "uint8", "crop": CROP, "cases": {}}

    # ---- train: 24 crops
    def statement():
        out = [A.crop_transform_numpy(images[r[0]], [labels[r[0]]], r, p, CROP) for r, p in zip(crops, params)]
        return np.stack([o[0] for o in out]), np.stack([o[1][0] for o in out])

    cd, pd, gd = (torch.from_numpy(t).to(DEV) for t in (crops, params, geom))
    x, y = tf(pool, cd, pd, gd)
    wx, wy = statement()
    np.testing.assert_array_equal(y.cpu().numpy(), wy)
    err = float(np.abs(x.cpu().numpy() - wx).max())
    assert err <= 2e-6, err
    written = x.numel() * 4 + y.numel() * 8
    src, dst = torch.empty(written, dtype=torch.uint8, device=DEV), torch.empty(written, dtype=torch.uint8, device=DEV)
    case = {"output": list(x.shape), "modes": params[:, 0].tolist(), "max_abs_err_vs_numpy_statement": err, "bytes_written": written,
            "bytes_read_at_least": 2 * N * CROP * CROP * C + N * CROP * CROP}
    case.update(rounds_ms(lambda: tf(pool, cd, pd, gd), lambda: dst.copy_(src), a.rounds, a.replays))
    idx = np.arange(N) % IMAGES
    case["device_with_draws_ms"] = host_ms(lambda: tf(pool, indices=idx), reps=21)
    case["host_ms"] = host_ms(lambda: [torch.from_numpy(t).to(DEV) for t in statement()])
    res["cases"]["train_24_crops_256"] = case

    # ---- grid: the 64 tiles of one image
    def grid_statement():
        gx, (gl,), _ = A.grid_transform_numpy(images[3], [labels[3]], 0, 0, CROP, CROP)
        return gx, gl

    gx, gy = tf.grid(pool, 3, (0, 0))
    wx, wy = grid_statement()
    np.testing.assert_array_equal(gy.cpu().numpy(), wy)
    err = float(np.abs(gx.cpu().numpy() - wx).max())
    assert err <= 2e-6, err
    written = gx.numel() * 4 + gy.numel() * 8
    src, dst = torch.empty(written, dtype=torch.uint8, device=DEV), torch.empty(written, dtype=torch.uint8, device=DEV)
    case = {"output": list(gx.shape), "max_abs_err_vs_numpy_statement": err, "bytes_written": written,
            "bytes_read_at_least": 2 * SIZE * SIZE * C + SIZE * SIZE}
    case.update(rounds_ms(lambda: tf.grid(pool, 3, (0, 0)), lambda: dst.copy_(src), a.rounds, a.replays))
    case["host_ms"] = host_ms(lambda: [torch.from_numpy(t).to(DEV) for t in grid_statement()])
    res["cases"]["grid_2048_tiles_256"] = case

    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
