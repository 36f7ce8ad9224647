"""Fixtures for the cubic resize of the reference's `preprocess` (test_mc3serousv5.py:100-113): outputs of SciPy itself,
`scipy.ndimage.zoom(img, (oh / H, ow / W[, 1]), order=3)`, on seeded images -> tests/golden/zoom_cubic.npz.  The inputs are
regenerated from the seeds by the tests (numpy default_rng), only SciPy's outputs are stored."""
import os
import sys

import numpy as np
from scipy.ndimage import zoom

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [  # seed, input shape, (out_h, out_w), dtype
    (1, (37, 53), (64, 64), "uint8"), (2, (100, 80, 3), (64, 96), "uint8"), (3, (64, 48), (128, 96), "float32"),
    (4, (150, 120, 3), (128, 128), "float32"), (5, (17, 19), (33, 7), "uint8"), (6, (90, 70, 1), (64, 64), "uint8"),
    # evaluation sizes whose last sample coordinate rounds above in - 1 (SciPy's last row / column is cval = 0)
    (7, (512, 512, 3), (224, 224), "uint8"), (8, (32, 40), (224, 224), "uint8"), (9, (1000, 1000), (224, 224), "float32"),
    (10, (1080, 1920, 3), (224, 224), "uint8"),
]

# size classes the tests sweep live (oracle against SciPy on the CPU, kernel against the oracle on the GPU); not stored
SWEEP = [  # input shape, (out_h, out_w)
    # one axis zoomed (thin strips): up and down, along H and along W
    ((37, 3), (64, 3)), ((3, 37), (3, 64)), ((97, 2), (31, 2)), ((2, 97), (2, 31)),
    # both axes, HW and HWC with C = 1, 3, 4
    ((41, 29), (19, 67)), ((29, 41, 3), (67, 19)), ((23, 31, 4), (48, 64)), ((64, 80, 1), (24, 30)),
    # n_in == n_out on one axis
    ((33, 47, 4), (33, 20)), ((45, 16, 3), (90, 16)),
    # degenerate axes: 1 pixel in or out, 2 and 3 pixels
    ((1, 9), (1, 20)), ((9, 1), (20, 1)), ((1, 1, 3), (5, 7)), ((9, 11), (1, 1)), ((1, 8, 3), (4, 1)),
    ((2, 3), (7, 5)), ((3, 2), (2, 3)), ((2, 2, 4), (3, 3)), ((7, 9, 1), (2, 3)),
    # last sample coordinate above in - 1 on both axes (58 -> 224, 32 -> 224): last row and column are cval = 0
    ((58, 32, 3), (224, 224)), ((32, 58), (224, 224)),
] + [  # evaluation sizes as strips along H and along W, to 224 (1000, 1920, 2048: last sample out of range) and to 512
    (shape, out) for n in (1000, 1080, 1920, 2048) for o in (224, 512)
    for shape, out in (((n, 2), (o, 2)), ((2, n, 3), (2, o)))
]


def make(seed, shape, dtype):
    rng = np.random.default_rng(seed)
    img = rng.random(shape) * 255.0
    return img.astype(np.uint8) if dtype == "uint8" else (img / 255.0 - 0.3).astype(np.float32)


if __name__ == "__main__":
    import scipy
    out = {"scipy_version": np.array(scipy.__version__)}
    for i, (seed, shape, ohw, dtype) in enumerate(CASES):
        img = make(seed, shape, dtype)
        zf = (ohw[0] / shape[0], ohw[1] / shape[1]) + ((1,) if len(shape) == 3 else ())
        out[f"case{i}"] = zoom(img, zf, order=3)
    np.savez_compressed(os.path.join(REPO, "tests", "golden", "zoom_cubic.npz"), **out)
    print("wrote zoom_cubic.npz", {k: v.shape for k, v in out.items()})
