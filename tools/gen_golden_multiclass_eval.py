#!/usr/bin/env python3
"""Generate tests/golden/multiclass_eval.npz: SciPy's per-class component labelling of seeded class-valued masks and what the
reference's own CrowdMatching.py returns on seeded multi-class scoring cases.  Runs on the CPU.

Nothing but RESULTS is stored; the masks and dot maps come from the seeded functions below, which the tests import to rebuild
the very same inputs.

  labelling   per mask of label_cases() and per class c = 1 .. K - 1, from scipy.ndimage.label(mask == c, np.ones((3, 3))):
              lab_<name>_count (K,), and per class lab_<name>_c<c>_area / _first / _sum_y / _sum_x (one entry per label, in
              SciPy's order = the raster order of first pixels); lab_<name>_checksum is the checksum (sum of
              label[p] * (p mod 65521 + 1)) of the GLOBAL label map, built here by merging the per-class maps and renumbering
              the components of all classes by first pixel.
  scoring     per image of score_case(name) and per class, on the plane (dot map == c) and the centroid list of that class
              (round half to even of sum / area of the SciPy labels, in integers, label order):
              sc_<name>_<n>_c<c>_prec / _recall / _f1   CrowdMatchingTest(plane, (x, y), SIGMAS, THRESHOLDS, 'Coordinates')
              sc_<name>_<n>_c<c>_gmae  (3, 3)           GMAE(L, plane, e_dot) for L = 1, 2, 3, e_dot[y, x] = 1 per centre
              sc_<name>_<n>_c<c>_count (6,)             GT, Pred and countAccuracyMetric(GT, Pred) on Python ints
              sc_<name>_<n>_ratio (6,) / _ratio3 (9,)   see below; NaNs all through where the expression raises
                                                        ZeroDivisionError

The reference module is imported from the reference checkout next to empty stand-in `cv2` and `skimage` modules, as
tools/gen_golden_crowd_matching.py does.  The two ratio blocks are a few arithmetic lines of the reference's
test_mc3serousv5.py (Results2Class.compareImages :499-501 with :518-523, Results3Class.compareImages :226-228 and :242-252).
That file cannot be imported -- it loads a .npy from an absolute path and imports staintools at import time -- so the values
are recorded by evaluating the same expressions here, on the recorded counts as Python ints (`_ratio_block`, `_ratio3_block`),
with the reference's own countAccuracyMetric for the four ratio metrics.  The reference's ground-truth counts are numpy.uint64
(np.sum of a uint8 image), whose abs(gt - pred) wraps when the prediction is larger; ints do not, and that is what is recorded.
A ground truth without a dot of class 1 or 2 records the ratio nan (numpy's 0 / 0).

Run in the build container: python tools/gen_golden_multiclass_eval.py
"""
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGMAS = [10, 20]                                  # Results2Class.sigma_list, test_mc3serousv5.py:400
THRESHOLDS = list(np.arange(0.5, 1, 0.05))         # :401


# ---- labelling cases -----------------------------------------------------------------------------------------------------------
def random_classes(seed, shape, K, density):
    """Per pixel: background with probability 1 - density, else a uniform class 1 .. K - 1."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(shape) < density, rng.integers(1, K, shape), 0).astype(np.uint8)


def tiling_2x2(h, w):
    """Classes 1..4 on a 2 x 2 tiling: no two equal values touch, every pixel is its own component (h * w of them)."""
    yy, xx = np.mgrid[:h, :w]
    return (1 + (yy % 2) * 2 + (xx % 2)).astype(np.uint8)


def checkerboard(h, w):
    """Classes 1 and 2 on a checkerboard: two components, each joined through diagonals only."""
    return (1 + np.indices((h, w)).sum(0) % 2).astype(np.uint8)


def rings(n, K, width):
    """Concentric square rings `width` pixels wide of the classes 1 .. K - 1 in turn (Chebyshev distance from the centre)."""
    yy, xx = np.mgrid[:n, :n]
    d = np.maximum(np.abs(yy - n // 2), np.abs(xx - n // 2)) // width
    return (1 + d % (K - 1)).astype(np.uint8)


def stripes(h, w, K, width, vertical):
    """Stripes `width` pixels wide of the classes 1 .. K - 1 in turn, running across the whole image."""
    yy, xx = np.mgrid[:h, :w]
    return (1 + ((xx if vertical else yy) // width) % (K - 1)).astype(np.uint8)


def serpentine(h, w):
    """Class 1: full rows every second line, joined alternately at the right and left end (one component crossing every seam);
    class 2 fills the gaps between them, which the joints cut into one component per gap row."""
    m = np.full((h, w), 2, dtype=np.uint8)
    m[::2] = 1
    m[1::4, -1] = 1
    m[3::4, 0] = 1
    return m


def blob_classes(seed, shape, K, n_blobs, rmin=2, rmax=6):
    """Discs of random radius and class 1 .. K - 1 on a background of 0; a later disc overwrites an earlier one."""
    rng = np.random.default_rng(seed)
    H, W = shape
    m = np.zeros(shape, dtype=np.uint8)
    yy, xx = np.mgrid[:H, :W]
    cy, cx = rng.integers(0, H, n_blobs), rng.integers(0, W, n_blobs)
    rad, cls = rng.integers(rmin, rmax + 1, n_blobs), rng.integers(1, K, n_blobs)
    for y, x, r, c in zip(cy, cx, rad, cls):
        y0, y1, x0, x1 = max(y - r, 0), min(y + r + 1, H), max(x - r, 0), min(x + r + 1, W)
        sel = (yy[y0:y1, x0:x1] - y) ** 2 + (xx[y0:y1, x0:x1] - x) ** 2 <= r * r
        m[y0:y1, x0:x1][sel] = c
    return m, cy, cx, cls


def label_cases():
    """name -> (uint8 class mask (H, W), K), in a fixed order."""
    out = {}
    k = 0
    for K in (2, 3, 4, 8):
        for d in (0.1, 0.5, 0.9):
            for shape in ((33, 65), (150, 190)):
                out[f"random_k{K}_d{d}_{shape[0]}x{shape[1]}"] = (random_classes(2000 + k, shape, K, d), K)
                k += 1
    out["tiling_6x6"] = (tiling_2x2(6, 6), 5)
    out["tiling_64x70"] = (tiling_2x2(64, 70), 5)
    out["checkerboard_65x67"] = (checkerboard(65, 67), 3)
    out["checkerboard_130x128"] = (checkerboard(130, 128), 3)
    out["rings_200_k3"] = (rings(200, 3, 3), 3)
    out["rings_257_k4"] = (rings(257, 4, 1), 4)
    for vertical in (False, True):
        v = "v" if vertical else "h"
        out[f"stripes1_{v}_130x200"] = (stripes(130, 200, 4, 1, vertical), 4)
        out[f"stripes64_{v}_200x260"] = (stripes(200, 260, 3, 64, vertical), 3)
    out["serpentine_130x131"] = (serpentine(130, 131), 3)
    out["serpentine_257x64"] = (serpentine(257, 64), 3)
    out["blobs_k4_512"] = (blob_classes(77, (512, 512), 4, 400)[0], 4)
    out["narrow_k4_300x17"] = (random_classes(78, (300, 17), 4, 0.6), 4)
    out["one_pixel_k3"] = (np.array([[2]], dtype=np.uint8), 3)
    out["zeros_k3_70x70"] = (np.zeros((70, 70), dtype=np.uint8), 3)
    return out


def checksum(a):
    """int64: sum of a[p] * (p mod 65521 + 1) over flat indices p."""
    v = np.asarray(a).astype(np.int64).ravel()
    return np.int64((v * (np.arange(v.size, dtype=np.int64) % 65521 + 1)).sum())


# ---- scoring cases -------------------------------------------------------------------------------------------------------------
SCORE_CASES = {  # name: (seed, K, (H, W), images, blobs per image, spurious dots per image)
    "k3_64": (301, 3, (64, 64), 2, 14, 3),
    "k3_96x130": (302, 3, (96, 130), 2, 40, 6),
    "k3_256": (303, 3, (256, 256), 1, 180, 20),
    "k4_64": (304, 4, (64, 64), 2, 16, 3),
    "k4_256": (305, 4, (256, 256), 1, 240, 25),
    "k4_512": (306, 4, (512, 512), 1, 330, 30),
    "k3_more_pred": (307, 3, (96, 130), 1, 50, 0),       # most dots dropped: predictions outnumber the ground truth
    "k3_no_gt_12": (308, 3, (64, 64), 1, 12, 0),         # no dot at all: the ground-truth ratio is nan
    "k3_no_pred_12": (309, 3, (64, 64), 1, 10, 2),       # an empty prediction: the predicted ratio raises ZeroDivisionError
}


def score_case(name):
    """(mask uint8 (N, H, W) class values, gt_dots uint8 (N, H, W) whose value is the class of the dot, K)."""
    seed, K, (H, W), N, n_blobs, n_spur = SCORE_CASES[name]
    rng = np.random.default_rng(seed)
    masks, dots = [], []
    for n in range(N):
        m, cy, cx, cls = blob_classes(int(rng.integers(1 << 30)), (H, W), K, n_blobs)
        g = np.zeros((H, W), dtype=np.uint8)
        keep = rng.random(n_blobs) < (0.2 if name == "k3_more_pred" else 0.85)
        wrong = rng.random(n_blobs) < 0.1
        dy, dx = rng.integers(-3, 4, n_blobs), rng.integers(-3, 4, n_blobs)
        for i in np.flatnonzero(keep):
            c = int(cls[i]) if not wrong[i] else 1 + int(cls[i]) % (K - 1)
            g[np.clip(cy[i] + dy[i], 0, H - 1), np.clip(cx[i] + dx[i], 0, W - 1)] = c
        sy, sx, sc = rng.integers(0, H, n_spur), rng.integers(0, W, n_spur), rng.integers(1, K, n_spur)
        g[sy, sx] = sc
        if name == "k3_no_gt_12":
            g[:] = 0
        if name == "k3_no_pred_12":
            m[:] = 0
        masks.append(m)
        dots.append(g)
    return np.stack(masks), np.stack(dots), K


def round_half_even(s, a):
    q, r = divmod(int(s), int(a))
    return q + (2 * r > a or (2 * r == a and q % 2 == 1))


def _ratio_block(ref, cell_gt, immune_gt, cell_pred, immune_pred):
    """Results2Class.compareImages :499-501 and :518-523: GT, Pred, round(AbsDiff, 4), Accuracy, AccuracyRelative,
    AccuracyRelativePD."""
    ratioGT = immune_gt / (cell_gt + immune_gt) if cell_gt + immune_gt else float("nan")
    try:
        ratioPred = immune_pred / (cell_pred + immune_pred)
    except ZeroDivisionError:
        return np.full(6, np.nan)
    abs_diff_ratio, ratioAccuracy, ratioAccuracyRelative, ratioAccuracyRelativePD = ref.countAccuracyMetric(ratioGT, ratioPred)
    return np.array([ratioGT, ratioPred, round(abs_diff_ratio, 4), ratioAccuracy, ratioAccuracyRelative, ratioAccuracyRelativePD],
                    dtype=np.float64)


def _ratio3_block(gt, pred, smoothening_factor=1e-6):
    """Results3Class.compareImages :226-228 and :242-252: cell / immune / tumor accuracy, then GTImmo, PredImmo, AccuracyImmo,
    GTImmoTummor, PredImmoTummor, AccuracyImmoTummor."""
    (cellCountGT, immuneCountGt, tumorCountGT), (cellCountPred, immuneCountPred, tumorCountPred) = gt, pred
    cellAccuracy = round(abs(cellCountGT - cellCountPred) / (cellCountGT + smoothening_factor), 4)
    immuneAccuracy = round(abs(immuneCountGt - immuneCountPred) / (immuneCountGt + smoothening_factor), 4)
    tumorAccuracy = round(abs(tumorCountGT - tumorCountPred) / (tumorCountGT + smoothening_factor), 4)
    ratioImmoGT = immuneCountGt / (immuneCountGt + tumorCountGT + cellCountGT + smoothening_factor)
    ratioImmoPred = immuneCountPred / (immuneCountPred + tumorCountPred + cellCountPred + smoothening_factor)
    ratioImmoTummorGT = immuneCountGt / (immuneCountGt + tumorCountGT + smoothening_factor)
    ratioImmoTummorPred = immuneCountPred / (immuneCountPred + tumorCountPred + smoothening_factor)
    return np.array([cellAccuracy, immuneAccuracy, tumorAccuracy, ratioImmoGT, ratioImmoPred,
                     round(abs(ratioImmoGT - ratioImmoPred), 4), ratioImmoTummorGT, ratioImmoTummorPred,
                     round(abs(ratioImmoTummorGT - ratioImmoTummorPred), 4)], dtype=np.float64)


def _class_stats(m, c):
    from scipy import ndimage
    lab, n = ndimage.label(m == c, structure=np.ones((3, 3)))
    idx = np.arange(1, n + 1)
    yy, xx = np.mgrid[:m.shape[0], :m.shape[1]]
    flat = np.arange(m.size).reshape(m.shape)
    z = np.zeros(0)
    on = (m == c).astype(np.int64)
    return (lab, n, (ndimage.sum(on, lab, idx) if n else z).astype(np.int32), (ndimage.minimum(flat, lab, idx) if n else z).astype(np.int64),
            (ndimage.sum(yy, lab, idx) if n else z).astype(np.int64), (ndimage.sum(xx, lab, idx) if n else z).astype(np.int64))


def main():
    import scipy
    sys.path[:0] = [REPO]
    from tools.gen_golden_crowd_matching import _reference
    ref = _reference()
    out = {"scipy_version": np.array(scipy.__version__), "label_names": np.array(list(label_cases())),
           "score_names": np.array(list(SCORE_CASES)), "sigmas": np.array(SIGMAS, dtype=np.float64),
           "thresholds": np.array(THRESHOLDS)}
    for name, (m, K) in label_cases().items():
        counts = np.zeros(K, dtype=np.int64)
        merged, firsts = [], []
        for c in range(1, K):
            lab, n, area, first, sy, sx = _class_stats(m, c)
            assert n == 0 or np.all(np.diff(first) > 0), name                  # SciPy numbers by first pixel
            counts[c] = n
            out[f"lab_{name}_c{c}_area"], out[f"lab_{name}_c{c}_first"] = area, first.astype(np.int32)
            out[f"lab_{name}_c{c}_sum_y"], out[f"lab_{name}_c{c}_sum_x"] = sy, sx
            merged.append(lab)
            firsts.append(first)
        allfirst = np.concatenate(firsts)
        number = np.empty(allfirst.size, dtype=np.int64)
        number[np.argsort(allfirst)] = np.arange(1, allfirst.size + 1)
        glob = np.zeros(m.shape, dtype=np.int64)
        at = 0
        for lab, f in zip(merged, firsts):
            glob += np.concatenate([[0], number[at:at + f.size]])[lab]
            at += f.size
        out[f"lab_{name}_count"] = counts
        out[f"lab_{name}_shape"] = np.array(m.shape + (K,))
        out[f"lab_{name}_checksum"] = checksum(glob)
    for name in SCORE_CASES:
        masks, dots, K = score_case(name)
        t0 = time.perf_counter()
        for n in range(masks.shape[0]):
            gts, preds = [], []
            for c in range(1, K):
                _, cnt, area, _, sy, sx = _class_stats(masks[n], c)
                x = np.array([round_half_even(s, a) for s, a in zip(sx, area)], dtype=np.int64)
                y = np.array([round_half_even(s, a) for s, a in zip(sy, area)], dtype=np.int64)
                plane = np.zeros(dots[n].shape, dtype=np.float64)
                plane[dots[n] == c] = 1
                e_dot = np.zeros_like(plane)
                for e in range(len(y)):
                    e_dot[y[e], x[e]] = 1
                gt, pred = int(plane.sum()), int(cnt)
                p, r, f = ref.CrowdMatchingTest(plane.copy(), (x.copy(), y.copy()), SIGMAS, THRESHOLDS, inputType='Coordinates')
                key = f"sc_{name}_{n}_c{c}"
                out[key + "_prec"], out[key + "_recall"], out[key + "_f1"] = p, r, f
                out[key + "_gmae"] = np.array([ref.GMAE(L, plane, e_dot) for L in (1, 2, 3)], dtype=np.float64)
                out[key + "_count"] = np.array((gt, pred) + tuple(ref.countAccuracyMetric(gt, pred)), dtype=np.float64)
                gts.append(gt)
                preds.append(pred)
            out[f"sc_{name}_{n}_ratio"] = _ratio_block(ref, gts[0], gts[1], preds[0], preds[1])
            if K == 4:
                out[f"sc_{name}_{n}_ratio3"] = _ratio3_block(gts, preds)
        out[f"sc_{name}_seconds"] = np.float64(time.perf_counter() - t0)
        print(name, masks.shape, "%.2f s" % out[f"sc_{name}_seconds"], flush=True)
    path = os.path.join(REPO, "tests", "golden", "multiclass_eval.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
