"""Fixtures for the training-batch transform (umi.augment) -> tests/golden/augment.npz.  Runs on the CPU, needs SciPy.

  rotate     scipy.ndimage.rotate(x, angle, order=0, reshape=False) of the seeded inputs of ROTATE_CASES, with the matrix and
             offset SciPy forms for them (cosdg / sindg, `@`): keys rot_/mat_/off_<name>_<angle>;
  rot_flip   np.flip(np.rot90(x, k), axis) for all 8 (k, axis) of ROT_FLIP_CASES: rf_<name>_<k>_<axis>;
  transform  the reference's whole `transform` (DataLoader.py:636-680, :275-373) written out with SciPy's own rotate and zoom
             for TRANSFORM_CASES and every row of TRANSFORM_PARAMS: tf_<name>_<row>_x and tf_<name>_<row>_label;
  cos_sin    the 40 (cosdg, sindg) pairs of the angles -20 .. 19.

The inputs are regenerated from the seeds by the tests (make / make_label below); only SciPy's outputs are stored.
"""
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANGLES = list(range(-20, 20))

ROTATE_CASES = [  # name, seed, shape, dtype, angles
    ("map17x13", 1, (17, 13), "uint8", ANGLES),
    ("img33", 2, (33, 33, 3), "uint8", ANGLES),
    ("f31x40", 3, (31, 40), "float32", [-20, -7, 3, 19]),            # non-square
    ("img96", 4, (96, 96, 3), "uint8", [-13, 5, 19]),                # more than one workgroup
    ("map130x70", 5, (130, 70), "uint8", [-20, 11]),                 # no multiple of a vector width
    ("img9x11c4", 6, (9, 11, 4), "float32", [-3, 12]),
]
ROT_FLIP_CASES = [("img24", 7, (24, 24, 3), "uint8"), ("map24", 8, (24, 24), "uint8")]
ROT_FLIP = [(k, axis) for k in range(4) for axis in range(2)]

TRANSFORM_CASES = [  # name, seed, image shape, image dtype, input_size, label kind, label_scale, label dtype
    ("bin40", 11, (40, 40, 3), "uint8", (24, 24), "class", 1.0, "int64"),            # Data_Binary with a resize
    ("bin24", 12, (24, 24), "uint8", (24, 24), "class", 1.0, "int64"),               # Data_Binary, HW, no resize
    ("reg40", 13, (40, 40, 3), "uint8", (24, 24), "density", 200.0, "float32"),      # the x 200 regression labels
    ("reg24", 14, (24, 24, 3), "uint8", (24, 24), "density", 200.0, "float32"),
    # 48 -> 24: the last sample coordinate 23 * (47 / 23) rounds above 47, so SciPy's last row and column are 0 (40 -> 24 has none)
    ("bin48", 15, (48, 48, 3), "uint8", (24, 24), "class", 1.0, "int64"),
]
TRANSFORM_PARAMS = [(0, 0, 0, 0), (1, 1, 0, 0), (1, 2, 1, 0), (2, 0, 0, -17), (2, 0, 0, 8)]      # [mode, k, axis, angle]


def make(seed, shape, dtype):
    rng = np.random.default_rng(seed)
    img = rng.random(shape) * 255.0
    return img.astype(np.uint8) if dtype == "uint8" else (img / 255.0 - 0.3).astype(np.float32)


def make_label(seed, shape, kind):
    """A uint8 class map with values 0 .. 3 in 4 x 4 cells, or a float32 density map."""
    rng = np.random.default_rng(1000 + seed)
    H, W = shape[:2]
    if kind == "class":
        cells = rng.integers(0, 4, size=((H + 3) // 4, (W + 3) // 4)).astype(np.uint8)
        return np.kron(cells, np.ones((4, 4), dtype=np.uint8))[:H, :W].copy()
    return (rng.random((H, W)) ** 8).astype(np.float32)


def reference_transform(image, label, p, input_size, label_scale, label_dtype):
    """The reference's `transform` for one sample with the draws given: p = [mode, k, axis, angle]."""
    from scipy import ndimage
    from scipy.ndimage import zoom
    mode, k, axis, angle = p
    if mode == 1:
        image, label = (np.flip(np.rot90(a, k), axis=axis).copy() for a in (image, label))
    elif mode == 2:
        image, label = (ndimage.rotate(a, angle, order=0, reshape=False) for a in (image, label))
    height, width = input_size
    y, x = image.shape[:2]
    if x != width or y != height:
        image = zoom(image, (width / x, height / y) + ((1,) if image.ndim == 3 else ()), order=3)
        label = zoom(label, (width / x, height / y), order=0)
    z = (image - np.mean(image, axis=(0, 1))) / np.std(image, axis=(0, 1))          # float64 for uint8 and float32 inputs alike
    z = z[None] if z.ndim == 2 else z.transpose((2, 0, 1))[::-1]                    # HW: one channel; HWC: CHW, channels reversed
    return np.ascontiguousarray(z.astype(np.float32)), (label.astype(np.float32) * np.float32(label_scale)).astype(label_dtype)


def scipy_geometry(angle, shape):
    """Matrix and offset as scipy.ndimage.rotate(reshape=False) forms them (ndimage/_interpolation.py)."""
    from scipy import special
    c, s = special.cosdg(angle), special.sindg(angle)
    rot_matrix = np.array([[c, s], [-s, c]])
    plane = np.asarray(shape[:2])
    out_center = rot_matrix @ ((plane - 1) / 2)
    in_center = (plane - 1) / 2
    return rot_matrix, in_center - out_center


if __name__ == "__main__":
    import scipy
    from scipy import ndimage, special
    out = {"scipy_version": np.array(scipy.__version__),
           "cos_sin": np.array([[special.cosdg(a), special.sindg(a)] for a in ANGLES], dtype=np.float64)}
    for name, seed, shape, dtype, angles in ROTATE_CASES:
        x = make(seed, shape, dtype)
        for a in angles:
            m, off = scipy_geometry(a, shape)
            out[f"mat_{name}_{a}"], out[f"off_{name}_{a}"] = m, off
            out[f"rot_{name}_{a}"] = ndimage.rotate(x, a, order=0, reshape=False)
    for name, seed, shape, dtype in ROT_FLIP_CASES:
        x = make(seed, shape, dtype)
        for k, axis in ROT_FLIP:
            out[f"rf_{name}_{k}_{axis}"] = np.flip(np.rot90(x, k), axis=axis).copy()
    for name, seed, shape, dtype, size, kind, scale, ldt in TRANSFORM_CASES:
        img, lab = make(seed, shape, dtype), make_label(seed, shape, kind)
        for i, p in enumerate(TRANSFORM_PARAMS):
            out[f"tf_{name}_{i}_x"], out[f"tf_{name}_{i}_label"] = reference_transform(img, lab, p, size, scale, ldt)
    path = os.path.join(REPO, "tests", "golden", "augment.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")
