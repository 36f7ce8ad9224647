"""Fixtures for the binary-model inference path (umi.infer.binary_mask / zoom_nearest / label_components, loss.MRAccuracy)
-> tests/golden/binary_infer.npz.  Runs on the CPU.

  masks   the patterns of masks(), stored with np.packbits, and per mask from
          scipy.ndimage.label(mask, structure=np.ones((3, 3))): the count, the area vector, the flat index of each label's first
          pixel, the integer coordinate sums sum_y / sum_x and an int64 checksum of the label map (sum of
          label[p] * (p mod 65521 + 1)) -- not the map itself;
  zoom    scipy.ndimage.zoom(order=0) of seeded 0/1 byte masks and float maps for ZOOM_CASES (inputs are regenerated from the
          seeds); byte outputs packed, outputs of more than 2**20 pixels as the same checksum;
  mr      the reference's own loss.MRAccuracy on the batches of mr_case(name), which the tests regenerate from the seeds.

The reference counts components with cv2.connectedComponents(connectivity=8).  OpenCV is not installed where this runs, so
the stand-in cv2 module handed to the reference has that one function built on the SciPy call above (n + 1 labels including the
background, as OpenCV returns): the recorded MRAccuracy values are the reference's arithmetic on SciPy's component counts.
"""
import os
import struct
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUTOFF = struct.unpack("<f", struct.pack("<I", 0xB43FFFFE))[0]         # umi.infer.SIGMOID_HALF_CUTOFF

DENSITIES = (0.05, 0.3, 0.5, 0.6)
RANDOM_SIZES = ((1, 1), (1, 7), (33, 65), (257, 385), (512, 512))


def _spiral(n):
    """One-pixel-wide square spiral with one-pixel gaps on an n x n grid: a single long winding component."""
    m = np.zeros((n, n), dtype=np.uint8)
    y = x = 0
    dy, dx = 0, 1
    m[0, 0] = 1
    while True:
        steps = 0
        while _can_move(m, y, x, dy, dx, n):
            y, x = y + dy, x + dx
            m[y, x] = 1
            steps += 1
        if steps == 0:
            return m
        dy, dx = dx, -dy                          # turn right


def _can_move(m, y, x, dy, dx, n):
    ny, nx = y + dy, x + dx
    ay, ax = ny + dy, nx + dx
    return 0 <= ny < n and 0 <= nx < n and not m[ny, nx] and not (0 <= ay < n and 0 <= ax < n and m[ay, ax])


def _serpentine(h, w):
    """Full rows every second line, joined alternately at the right and left end: one component that crosses every vertical
    seam on every second row and every horizontal seam."""
    m = np.zeros((h, w), dtype=np.uint8)
    m[::2] = 1
    m[1::4, -1] = 1
    m[3::4, 0] = 1
    return m


def _ring_blob(n):
    yy, xx = np.mgrid[:n, :n]
    r2 = (yy - n // 2) ** 2 + (xx - n // 2) ** 2
    return (((r2 <= (n * 0.45) ** 2) & (r2 >= (n * 0.35) ** 2)) | (r2 <= (n * 0.1) ** 2)).astype(np.uint8)


def _diagonals(n, anti):
    yy, xx = np.mgrid[:n, :n]
    d = (yy + xx) if anti else (yy - xx)
    return (d % 7 == 0).astype(np.uint8)


def _comb(h, w):
    m = np.zeros((h, w), dtype=np.uint8)
    m[0] = 1
    m[:, ::2] = 1
    return m


def _isolated(h, w):
    m = np.zeros((h, w), dtype=np.uint8)
    m[::2, ::2] = 1
    return m


def masks():
    """name -> uint8 0/1 mask, in a fixed order."""
    out = {}
    k = 0
    for d in DENSITIES:
        for shape in RANDOM_SIZES:
            out[f"random_d{d}_{shape[0]}x{shape[1]}"] = (np.random.default_rng(1000 + k).random(shape) < d).astype(np.uint8)
            k += 1
    out["zeros_257x385"] = np.zeros((257, 385), dtype=np.uint8)
    out["ones_257x385"] = np.ones((257, 385), dtype=np.uint8)
    out["ones_512x512"] = np.ones((512, 512), dtype=np.uint8)
    out["checkerboard_64x64"] = (np.indices((64, 64)).sum(0) % 2).astype(np.uint8)
    out["checkerboard_257x385"] = (np.indices((257, 385)).sum(0) % 2 == 0).astype(np.uint8)
    out["isolated_512x512"] = _isolated(512, 512)
    out["isolated_257x385"] = _isolated(257, 385)
    out["spiral_257"] = _spiral(257)
    out["serpentine_512x512"] = _serpentine(512, 512)
    out["serpentine_257x385"] = _serpentine(257, 385)
    out["diagonals_main_300"] = _diagonals(300, False)
    out["diagonals_anti_300"] = _diagonals(300, True)
    out["comb_200x333"] = _comb(200, 333)
    out["ring_blob_400"] = _ring_blob(400)
    return out


def checksum(a):
    """int64: sum of a[p] * (p mod 65521 + 1) over flat indices p."""
    v = np.asarray(a).astype(np.int64).ravel()
    return np.int64((v * (np.arange(v.size, dtype=np.int64) % 65521 + 1)).sum())


# ---- nearest resize -----------------------------------------------------------------------------------------------------------
ZOOM_CASES = [  # seed, input (H, W), (out_h, out_w), dtype
    (1, (37, 53), (64, 64), "uint8"), (2, (64, 48), (17, 19), "uint8"), (3, (17, 19), (33, 7), "float32"),
    (4, (512, 512), (224, 224), "uint8"),            # last sample coordinate above in - 1: last row and column are 0
    (5, (512, 512), (768, 768), "uint8"), (6, (512, 512), (1000, 1000), "uint8"), (7, (512, 512), (2048, 2048), "uint8"),
    (8, (512, 512), (1080, 1920), "uint8"), (9, (100, 80), (64, 96), "float32"), (10, (1, 9), (1, 20), "uint8"),
    (11, (9, 11), (1, 1), "uint8"), (12, (2, 3), (7, 5), "float32"),
]


def zoom_input(seed, shape, dtype):
    r = np.random.default_rng(seed).random(shape)
    return (r < 0.5).astype(np.uint8) if dtype == "uint8" else (r - 0.3).astype(np.float32)


def zoom_nearest_numpy(a, out_hw):
    """The rule of scipy.ndimage.zoom(a, (oh / H, ow / W), order=0), restated: output size round(in * zoom); sample coordinate
    x = i * ((in - 1) / (out - 1)) in float64 (0 when out == 1); source index floor(x + 0.5); an output whose coordinate exceeds
    in - 1 on either axis is 0 (mode 'constant')."""
    H, W = a.shape[-2:]
    oh, ow = int(round(H * (out_hw[0] / H))), int(round(W * (out_hw[1] / W)))

    def axis(n_in, n_out):
        x = np.arange(n_out, dtype=np.float64) * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
        return np.minimum(np.floor(x + 0.5).astype(np.int64), n_in - 1), x > n_in - 1
    iy, zy = axis(H, oh)
    ix, zx = axis(W, ow)
    out = a[..., iy, :][..., ix].copy()
    out[..., zy, :] = 0
    out[..., zx] = 0
    return out


# ---- MRAccuracy ---------------------------------------------------------------------------------------------------------------
MR_CASES = ("plain", "empty_gt_nonempty_pred", "both_empty", "threshold")


def _blobs(rng, B, H, W, cell):
    low = rng.standard_normal((B, H // cell, W // cell))
    return np.kron(low, np.ones((cell, cell))) + 0.3 * rng.standard_normal((B, H, W))


def mr_case(name):
    """(pred (B, 1, H, W) float32 logits, target (B, H, W) float32 dot map) of one MRAccuracy case, from fixed seeds."""
    rng = np.random.default_rng(4242 + MR_CASES.index(name))
    B, H, W = 3, 64, 64
    pred = (_blobs(rng, B, H, W, 8) - 0.8).astype(np.float32)
    target = (rng.random((B, H, W)) < 0.004).astype(np.float32)
    if name == "empty_gt_nonempty_pred":
        target[1] = 0
    elif name == "both_empty":
        target[0] = 0
        pred[0] = -3.0
        target[2] = 0
    elif name == "threshold":
        on = _blobs(rng, B, H, W, 4) > 0.5
        nxt = np.nextafter(np.float32(CUTOFF), np.float32(-1))            # just below the cut-off: sigmoid < 0.5
        pred = np.where(on, np.float32(CUTOFF), nxt).astype(np.float32)
        pred[0][on[0] & (rng.random((H, W)) < 0.5)] = 0.0
        pred[1][~on[1] & (rng.random((H, W)) < 0.5)] = -1e-6
        pred[2][on[2] & (rng.random((H, W)) < 0.3)] = -0.0
    return pred[:, None], target


def _reference_mraccuracy():
    from scipy import ndimage
    from tools import gen_golden
    cv2 = types.ModuleType("cv2")

    def connectedComponents(img, connectivity=8):
        assert connectivity == 8 and img.ndim == 2 and img.dtype == np.uint8
        labels, n = ndimage.label(img, structure=np.ones((3, 3)))
        return n + 1, labels
    cv2.connectedComponents = connectedComponents
    sys.modules["cv2"] = cv2
    _, ref_loss, _ = gen_golden.import_reference()
    ref_loss.cv2 = cv2
    return ref_loss.MRAccuracy


def main():
    import scipy
    import torch
    from scipy import ndimage
    sys.path[:0] = [REPO]
    out = {"scipy_version": np.array(scipy.__version__), "mask_names": np.array(list(masks()))}
    for name, m in masks().items():
        lab, n = ndimage.label(m, structure=np.ones((3, 3)))
        idx = np.arange(1, n + 1)
        yy, xx = np.mgrid[:m.shape[0], :m.shape[1]]
        flat = np.arange(m.size).reshape(m.shape)
        out[f"mask_{name}_bits"] = np.packbits(m)
        out[f"mask_{name}_shape"] = np.array(m.shape)
        out[f"mask_{name}_count"] = np.int64(n)
        z = np.zeros(0)
        out[f"mask_{name}_area"] = (ndimage.sum(m, lab, idx) if n else z).astype(np.int32)
        out[f"mask_{name}_first"] = (ndimage.minimum(flat, lab, idx) if n else z).astype(np.int32)
        out[f"mask_{name}_sum_y"] = (ndimage.sum(yy, lab, idx) if n else z).astype(np.int64)
        out[f"mask_{name}_sum_x"] = (ndimage.sum(xx, lab, idx) if n else z).astype(np.int64)
        out[f"mask_{name}_checksum"] = checksum(lab)
        assert n == 0 or np.all(np.diff(out[f"mask_{name}_first"]) > 0), name      # SciPy numbers by first pixel
    for i, (seed, shape, ohw, dtype) in enumerate(ZOOM_CASES):
        z = ndimage.zoom(zoom_input(seed, shape, dtype), (ohw[0] / shape[0], ohw[1] / shape[1]), order=0)
        out[f"zoom{i}_shape"] = np.array(z.shape)
        if z.size > 2 ** 20:
            out[f"zoom{i}_checksum"] = checksum(z)
            out[f"zoom{i}_sum"] = np.int64(z.astype(np.int64).sum())
        elif dtype == "uint8":
            out[f"zoom{i}_bits"] = np.packbits(z)
        else:
            out[f"zoom{i}"] = z
    ref = _reference_mraccuracy()
    for name in MR_CASES:
        pred, target = mr_case(name)
        out[f"mr_{name}"] = np.float64(ref(torch.from_numpy(pred), torch.from_numpy(target)))
    path = os.path.join(REPO, "tests", "golden", "binary_infer.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes;",
          {n: int(out[f"mask_{n}_count"]) for n in masks()}, {n: float(out[f"mr_{n}"]) for n in MR_CASES})


if __name__ == "__main__":
    main()
