#!/usr/bin/env python3
"""Times the training-batch transform (umi.augment.TrainTransform, csrc/augment.hip) on one MI355X against the host pipeline it
replaces.

The batch: N = 16 uint8 768 x 768 x 3 images and one uint8 label map each, modes 1 / 2 / 0 in turn (rot90 + flip, rotation, none),
once at the network size (no resize, the normal case) and once with the resize to 512 x 512.  After warm-up, device events
around --replays (>= 20) back-to-back calls with the parameters already on the device:

  device_ms_per_batch          TrainTransform: labels + image
  device_labels_ms             transform_labels alone
  device_image_ms              the image path alone (statistics + normalise, or geometry + per-image cubic resize + z-norm)
  host_scipy_ms_per_batch      the reference's own per-sample pipeline (np.rot90 / np.flip, scipy.ndimage.rotate and zoom, float64
                               statistics) over the 16 samples, one thread, host clock, same run; absent without SciPy
  host_numpy_ms_per_batch      the in-tree NumPy statement (umi.augment.train_transform_numpy) over the 16 samples
  bytes_per_batch              what the device path has to read and write at least, from the shapes (see bytes_moved)

The device results of the run are compared with the NumPy statement before anything is timed: labels exact, image within 2e-6
without a resize; the largest image difference is recorded.
Prints one JSON line; --out writes it (profiles/augment_times.json is the record README and DESIGN quote).
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
N, SIZE, C = 16, 768, 3


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


def bytes_moved(n, size, c, out):
    """Least bytes per batch.  Labels: every output pixel reads one uint8 and writes one int64.  Image without a resize: the
    uint8 image is read twice (statistics, then normalise) and the float32 NCHW tensor written once.  With a resize: the
    augmented uint8 image is written and read, the float64 spline coefficients are written by two prefilter passes (the second
    in place: read + write) and read 16 times per output value, the resized uint8 image is written and read three times
    (statistics twice, normalise), the float32 tensor is written."""
    px, opx = n * size * size, n * out * out
    labels = opx * (1 + 8)
    if out == size:
        image = 2 * px * c + opx * c * 4
    else:
        image = 2 * px * c + px * c * (1 + 8 + 16) + opx * c * (16 * 8 + 1 + 3 + 4)
    return {"labels": labels, "image": image, "total": labels + image}


def make_batch():
    rng = np.random.default_rng(20)
    img = (rng.random((N, SIZE, SIZE, C)) * 255).astype(np.uint8)
    lab = np.kron(rng.integers(0, 4, (N, SIZE // 16, SIZE // 16)).astype(np.uint8), np.ones((1, 16, 16), np.uint8))
    p = np.zeros((N, 4), np.int32)
    for n in range(N):
        if n % 3 == 0:
            p[n] = (1, rng.integers(0, 4), rng.integers(0, 2), 0)
        elif n % 3 == 1:
            p[n] = (2, 0, 0, rng.integers(-20, 20))
    return img, lab, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--out")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_augment.py measures on the MI355X"
    assert a.replays >= 20
    from umi import augment as A
    from umi import infer
    try:
        import scipy
        from tools.gen_golden_augment import reference_transform
    except ImportError:
        scipy = None
    img, lab, p = make_batch()
    geom = A.batch_geometry(p, SIZE, SIZE)
    xd, ld = torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV)
    pd, gd = torch.from_numpy(p).to(DEV), torch.from_numpy(geom).to(DEV)
    res = {"device": torch.cuda.get_device_name(0), "replays": a.replays, "batch": [N, SIZE, SIZE, C], "image_dtype": "uint8",
           "label_maps": 1, "modes": p[:, 0].tolist(), "scipy": None if scipy is None else scipy.__version__, "cases": {}}
    for out in (SIZE, 512):
        tf = A.TrainTransform((out, out), True)
        x, y = tf(xd, ld, pd, gd)
        t0 = time.perf_counter()
        want = [A.train_transform_numpy(img[n], [lab[n]], p[n], (out, out)) for n in range(N)]
        t1 = time.perf_counter()
        np.testing.assert_array_equal(y.cpu().numpy(), np.stack([w[1][0] for w in want]))
        err = float(np.abs(x.cpu().numpy() - np.stack([w[0] for w in want])).max())
        assert err <= (2e-6 if out == SIZE else 0.1), err      # resize: a byte at an exact half-way value may round the other way
        case = {"output": [N, C, out, out], "max_abs_err_vs_numpy_statement": err, "host_numpy_ms_per_batch": (t1 - t0) * 1e3,
                "bytes_per_batch": bytes_moved(N, SIZE, C, out)}
        if scipy is not None:
            t0 = time.perf_counter()
            for n in range(N):
                reference_transform(img[n], lab[n], tuple(int(v) for v in p[n]), (out, out), 1.0, "int64")
            case["host_scipy_ms_per_batch"] = (time.perf_counter() - t0) * 1e3
        case["device_ms_per_batch"] = event_ms(lambda: tf(xd, ld, pd, gd), a.replays)
        case["device_labels_ms"] = event_ms(lambda: A.transform_labels(ld, pd, gd, (out, out)), a.replays)
        if out == SIZE:
            case["device_image_ms"] = event_ms(lambda: A.transform_image(xd, pd, gd), a.replays)
        else:
            case["device_image_ms"] = event_ms(
                lambda: [infer.preprocess(im, input_size=(out, out)) for im in A.apply_geometry(xd, pd, gd)], a.replays)
        case["device_gb_per_s"] = case["bytes_per_batch"]["total"] / case["device_ms_per_batch"] / 1e6
        res["cases"]["no_resize" if out == SIZE else f"resize_to_{out}"] = case
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
