#!/usr/bin/env python3
"""Generate tests/golden/crowd_matching.npz: what the reference's own CrowdMatching.py returns on seeded cases.

The reference module is imported from the reference checkout (tools/gen_golden.REF) next to empty stand-in `cv2` and `skimage`
modules -- neither library is installed and none of the recorded functions calls into them with inputType='Coordinates'.  The
cases are built from fixed seeds by the functions below, which the tests import to rebuild the very same inputs; only RESULTS
are stored (plus the reference's wall time per case, as information):

  cm_<case>_prec / _recall / _f1   CrowdMatchingTest(g_dot, (x, y), SIGMAS, THRESHOLDS, inputType='Coordinates')
  dm_<case>_<k>                    CrowdMatchingTest2(g_dot, (x, y), DIST_THRESHOLDS[k]); NaNs where it raises ZeroDivisionError
  gmae_<case>                      (3, 3): GMAE(L, gt, pred) for L = 1, 2, 3

Run in the build container: python tools/gen_golden_crowd_matching.py
"""
import importlib.util
import os
import sys
import time
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIGMAS = [5, 20]
THRESHOLDS = list(np.arange(0.5, 1, 0.05))
DIST_THRESHOLDS = [10, 2.5, 1, 10.000001]


def _dot_map(shape, ys, xs):
    g = np.zeros(shape, dtype=np.float64)
    g[ys, xs] = 1
    return g


def _random_case(seed, shape, n_dots, jitter, n_spurious, drop=0):
    """Random dots; one centre per dot (but `drop` of them) moved by up to `jitter` pixels and clipped to the image, plus
    `n_spurious` uniform ones; the centre order is shuffled."""
    rng = np.random.default_rng(seed)
    H, W = shape
    flat = rng.choice(H * W, size=n_dots, replace=False)
    ys, xs = flat // W, flat % W
    keep = rng.permutation(n_dots)[:n_dots - drop]
    cx = np.clip(xs[keep] + rng.integers(-jitter, jitter + 1, keep.size), 0, W - 1)
    cy = np.clip(ys[keep] + rng.integers(-jitter, jitter + 1, keep.size), 0, H - 1)
    cx = np.concatenate([cx, rng.integers(0, W, n_spurious)])
    cy = np.concatenate([cy, rng.integers(0, H, n_spurious)])
    order = rng.permutation(cx.size)
    return _dot_map(shape, ys, xs), cx[order].astype(np.int64), cy[order].astype(np.int64)


def _lattice(shape, seed):
    """Dots on the 8-pixel grid, centres on the half grid: every centre is at the same distance from up to four dots."""
    H, W = shape
    gy, gx = np.meshgrid(np.arange(4, H, 8), np.arange(4, W, 8), indexing="ij")
    cy, cx = np.meshgrid(np.arange(8, H - 4, 8), np.arange(8, W - 4, 8), indexing="ij")
    cy, cx = cy.reshape(-1), cx.reshape(-1)
    if seed is not None:
        order = np.random.default_rng(seed).permutation(cy.size)
        cy, cx = cy[order], cx[order]
    return _dot_map(shape, gy.reshape(-1), gx.reshape(-1)), cx.astype(np.int64), cy.astype(np.int64)


def _border(shape):
    """Centres in the corners and within r = 20 / 80 pixels of every border, dots at and around them."""
    H, W = shape
    pts = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 3), (H // 2, 0), (H // 3, W - 1),
           (3, 5), (H - 4, W - 6), (17, W - 19), (H - 18, 16), (H // 2, W // 2)]
    cy, cx = np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
    rng = np.random.default_rng(77)
    dy, dx = rng.integers(-6, 7, (3, cy.size)), rng.integers(-6, 7, (3, cy.size))
    ys, xs = np.clip(cy[None] + dy, 0, H - 1).reshape(-1), np.clip(cx[None] + dx, 0, W - 1).reshape(-1)
    ys, xs = np.concatenate([ys, cy[:4]]), np.concatenate([xs, cx[:4]])
    return _dot_map(shape, ys, xs), cx.astype(np.int64), cy.astype(np.int64)


def _duplicates():
    g, cx, cy = _random_case(31, (64, 64), 30, 3, 2)
    return g, np.concatenate([cx, cx[:12], cx[:5]]), np.concatenate([cy, cy[:12], cy[:5]])


_NONE = np.zeros(0, dtype=np.int64)

CASES = {
    "lattice_64": lambda: _lattice((64, 64), None),
    "lattice_96x130_shuffled": lambda: _lattice((96, 130), 5),
    "lattice_64_shuffled": lambda: _lattice((64, 64), 6),
    "random_64": lambda: _random_case(11, (64, 64), 25, 4, 5),
    "random_96x130": lambda: _random_case(12, (96, 130), 60, 6, 10, drop=4),
    "random_512": lambda: _random_case(13, (512, 512), 100, 8, 10),
    "random_768": lambda: _random_case(14, (768, 768), 400, 10, 20),
    "border_64": lambda: _border((64, 64)),
    "border_96x130": lambda: _border((96, 130)),
    "duplicates": _duplicates,
    "empty_both": lambda: (np.zeros((64, 64)), _NONE, _NONE),
    "empty_dots": lambda: (np.zeros((64, 64)),) + _random_case(15, (64, 64), 5, 0, 3)[1:],
    "empty_centres": lambda: (_random_case(16, (64, 64), 9, 0, 0)[0], _NONE, _NONE),
    "more_centres": lambda: _random_case(17, (96, 130), 12, 5, 70),
    "more_dots": lambda: _random_case(18, (96, 130), 90, 5, 2, drop=70),
}


def case(name):
    """(g_dot float64 (H, W) of 0 / 1, centre x coordinates, centre y coordinates), both int64."""
    return CASES[name]()


GMAE_CASES = {"gmae_512": (21, (512, 512), 300, 280), "gmae_512_sparse": (22, (512, 512), 12, 30),
              "gmae_600x520": (23, (600, 520), 350, 350), "gmae_300x400": (24, (300, 400), 150, 140)}


def gmae_case(name):
    """(ground-truth dot map, predicted dot map), float64 0 / 1."""
    seed, shape, n_gt, n_pred = GMAE_CASES[name]
    rng = np.random.default_rng(seed)
    maps = []
    for n in (n_gt, n_pred):
        flat = rng.choice(shape[0] * shape[1], size=n, replace=False)
        maps.append(_dot_map(shape, flat // shape[1], flat % shape[1]))
    return maps[0], maps[1]


def _reference():
    from tools import gen_golden
    for name in ("cv2", "skimage", "skimage.feature"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["skimage.feature"].peak_local_max = None
    spec = importlib.util.spec_from_file_location("reference_CrowdMatching", os.path.join(gen_golden.REF, "CrowdMatching.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    sys.path[:0] = [REPO]
    ref = _reference()
    out = {"case_names": np.array(list(CASES)), "gmae_names": np.array(list(GMAE_CASES)),
           "sigmas": np.array(SIGMAS, dtype=np.float64), "thresholds": np.array(THRESHOLDS),
           "dist_thresholds": np.array(DIST_THRESHOLDS)}
    for name in CASES:
        g, x, y = case(name)
        t0 = time.perf_counter()
        p, r, f = ref.CrowdMatchingTest(g.copy(), (x.copy(), y.copy()), SIGMAS, THRESHOLDS, inputType='Coordinates')
        out[f"cm_{name}_seconds"] = np.float64(time.perf_counter() - t0)
        out[f"cm_{name}_prec"], out[f"cm_{name}_recall"], out[f"cm_{name}_f1"] = p, r, f
        out[f"cm_{name}_sizes"] = np.array([g.shape[0], g.shape[1], int(g.sum()), x.size])
        for k, th in enumerate(DIST_THRESHOLDS):
            try:
                res = np.array(ref.CrowdMatchingTest2(g.copy(), (x.copy(), y.copy()), th), dtype=np.float64)
            except ZeroDivisionError:
                res = np.full(3, np.nan)
            out[f"dm_{name}_{k}"] = res
        print(name, out[f"cm_{name}_sizes"].tolist(), "%.2f s" % out[f"cm_{name}_seconds"], flush=True)
    for name in GMAE_CASES:
        gt, pred = gmae_case(name)
        out[name] = np.array([ref.GMAE(L, gt, pred) for L in (1, 2, 3)], dtype=np.float64)
    path = os.path.join(REPO, "tests", "golden", "crowd_matching.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
