"""Writes tests/golden/density_peaks.npz: small density maps with SciPy's answers for the two halves of the peak rule of
umi/peaks.py.  Needs NumPy and SciPy only; scikit-image is not involved (umi/peaks.py says why).

Per case (a map kind, a size, a seed) and min_distance d in DISTANCES:
    map_<case>              the float32 map
    wmax_<case>_<d>         scipy.ndimage.maximum_filter(floored map, size=2d+1, mode='nearest')
    kept_<case>_<d>         int32 (K, 2) peaks as (x, y): the candidates sorted by descending value (stable, so raster order among
                            equal values), then a greedy walk over that list with scipy.spatial.cKDTree.query_ball_point under
                            the Chebyshev norm -- a peak throws out every later candidate closer than d.

    python tools/gen_golden_density.py
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "density_peaks.npz")
DISTANCES = (1, 3, 5)
FLOOR = 1e-3
KINDS = ("noise", "levels", "plateaus")
SIZES = ((8, 15), (13, 13), (24, 40), (33, 27))
CASES = [f"{k}_{h}x{w}" for k in KINDS for h, w in SIZES]


def make_map(kind, H, W, seed):
    """The three map kinds: continuous noise (no plateaus), noise quantised to four levels (plateaus everywhere), overlapping
    rectangular plateaus on a low background."""
    rng = np.random.default_rng(seed)
    if kind == "noise":
        m = rng.random((H, W))
    elif kind == "levels":
        m = np.floor(rng.random((H, W)) * 4) / 4
    elif kind == "plateaus":
        m = np.full((H, W), 0.0005)
        for _ in range(max(3, H * W // 40)):
            h, w = int(rng.integers(1, max(2, H // 3))), int(rng.integers(1, max(2, W // 3)))
            y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
            m[y:y + h, x:x + w] = np.maximum(m[y:y + h, x:x + w], rng.integers(1, 5) / 4)
    else:
        raise ValueError(kind)
    return m.astype(np.float32)


def case(name):
    kind, size = name.split("_")
    H, W = (int(v) for v in size.split("x"))
    return make_map(kind, H, W, seed=1000 + CASES.index(name))


def scipy_window_max(a, d):
    from scipy import ndimage
    return ndimage.maximum_filter(a, size=2 * d + 1, mode="nearest")


def scipy_candidates(x, d, floor=FLOOR):
    """(a, candidate mask) with the window maximum from SciPy."""
    a = np.where(x >= np.float32(floor), x, np.float32(0)).astype(np.float32)
    cand = (a == scipy_window_max(a, d)) & (a > a.min())
    cand[:d], cand[:, :d] = False, False
    cand[max(a.shape[0] - d, 0):], cand[:, max(a.shape[1] - d, 0):] = False, False
    return a, cand


def kdtree_greedy(a, cand, d):
    """int32 (K, 2) as (x, y): the greedy over the value-sorted candidate list described in the module docstring."""
    from scipy.spatial import cKDTree
    ys, xs = np.nonzero(cand)
    order = np.argsort(-a[ys, xs], kind="stable")
    pts = np.stack([ys[order], xs[order]], axis=1)
    if not len(pts):
        return np.zeros((0, 2), dtype=np.int32)
    tree = cKDTree(pts)
    out_of_play = np.zeros(len(pts), dtype=bool)
    kept = []
    for i in range(len(pts)):
        if out_of_play[i]:
            continue
        kept.append(i)
        for j in tree.query_ball_point(pts[i], r=d - 0.5, p=np.inf):        # integer offsets: Chebyshev distance <= d - 1
            if j != i:
                out_of_play[j] = True
    kept = pts[np.array(kept, dtype=np.int64)]
    return np.stack([kept[:, 1], kept[:, 0]], axis=1).astype(np.int32)


def main():
    data = {"case_names": np.array(CASES), "distances": np.array(DISTANCES), "floor": np.array(FLOOR)}
    total = 0
    for name in CASES:
        x = case(name)
        data[f"map_{name}"] = x
        for d in DISTANCES:
            a, cand = scipy_candidates(x, d)
            data[f"wmax_{name}_{d}"] = scipy_window_max(a, d)
            data[f"kept_{name}_{d}"] = kdtree_greedy(a, cand, d)
            total += len(data[f"kept_{name}_{d}"])
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT}: {len(CASES)} maps x {len(DISTANCES)} distances, {total} peaks, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    sys.exit(main())
