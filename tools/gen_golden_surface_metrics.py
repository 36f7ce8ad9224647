#!/usr/bin/env python3
"""Generate tests/golden/surface_metrics.npz from live SciPy / NumPy: for small binary mask pairs (A, G) the surface distances as
medpy and TransUNet's evaluation compute them for unit spacing,

    surface(M) = M ^ binary_erosion(M, generate_binary_structure(2, 1))
    d(A->G)    = distance_transform_edt(~surface(G))[surface(A)]            (and the other way round)
    hd = max(S), hd95 = np.percentile(S, 95), assd = (mean(d(A->G)) + mean(d(G->A))) / 2,   S = hstack of both

so that the tests need no SciPy.  Pairs with an empty side keep zeros and their state (1 both empty, 2 A empty, 3 G empty).

Stored: shapes [N, 2]; pred_bits / label_bits (np.packbits of the row-major masks, each case padded to whole bytes) with
offsets [N + 1]; hd, hd95, assd (float64 [N]); counts (int64 [N, 2]: surface pixels of A, of G); state (int64 [N]).

Usage:  python tools/gen_golden_surface_metrics.py
"""
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import scipy
import scipy.ndimage as ndi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")


def reference(a, g):
    st = ndi.generate_binary_structure(2, 1)
    na, ng = bool(a.any()), bool(g.any())
    if not (na and ng):
        sa = a ^ ndi.binary_erosion(a, st) if na else a
        sg = g ^ ndi.binary_erosion(g, st) if ng else g
        return 0.0, 0.0, 0.0, (int(sa.sum()), int(sg.sum())), (3 if na else (2 if ng else 1))
    sa, sg = a ^ ndi.binary_erosion(a, st), g ^ ndi.binary_erosion(g, st)
    dag, dga = ndi.distance_transform_edt(~sg)[sa], ndi.distance_transform_edt(~sa)[sg]
    S = np.hstack([dag, dga])
    return float(S.max()), float(np.percentile(S, 95)), float((dag.mean() + dga.mean()) / 2), (int(sa.sum()), int(sg.sum())), 0


def cases(rng):
    out = []
    for _ in range(48):                                   # random pairs, sizes 1..39, densities 0.02..1.0
        H, W = (int(v) for v in rng.integers(1, 40, 2))
        out.append((rng.random((H, W)) < rng.uniform(0.02, 1.0), rng.random((H, W)) < rng.uniform(0.02, 1.0)))
    yy, xx = np.mgrid[:37, :29]
    disc = (yy - 15) ** 2 + (xx - 12) ** 2 < 81
    out.append((disc, (yy - 20) ** 2 + (xx - 16) ** 2 < 64))                     # two overlapping discs
    out.append((disc, disc))                                                     # identical
    out.append((np.ones((9, 14), bool), np.ones((9, 14), bool)))                 # full: the surface is the frame
    a, g = np.zeros((23, 31), bool), np.zeros((23, 31), bool)
    a[0, 0], g[-1, -1] = True, True
    out.append((a, g))                                                           # opposite corners: the diagonal
    chk = (yy + xx) % 2 == 0
    out.append((chk, ~chk))                                                      # every pixel is surface
    z = np.zeros((11, 13), bool)
    out += [(z, z), (z, ~z), (~z, z)]                                            # states 1, 2, 3
    out += [(np.ones((1, 1), bool), np.ones((1, 1), bool)), (np.ones((1, 1), bool), np.zeros((1, 1), bool))]
    return out


def main():
    rng = np.random.default_rng(20261021)
    cs = cases(rng)
    shapes, pb, lb, off = [], [], [], [0]
    hd, hd95, assd, counts, state = [], [], [], [], []
    for a, g in cs:
        r = reference(a, g)
        shapes.append(a.shape)
        pb.append(np.packbits(a.ravel()))
        lb.append(np.packbits(g.ravel()))
        off.append(off[-1] + len(pb[-1]))
        hd.append(r[0]); hd95.append(r[1]); assd.append(r[2]); counts.append(r[3]); state.append(r[4])
    path = os.path.join(GOLD, "surface_metrics.npz")
    np.savez_compressed(path, shapes=np.array(shapes, np.int64), pred_bits=np.concatenate(pb), label_bits=np.concatenate(lb),
                        offsets=np.array(off, np.int64), hd=np.array(hd), hd95=np.array(hd95), assd=np.array(assd),
                        counts=np.array(counts, np.int64), state=np.array(state, np.int64),
                        numpy_version=np.__version__, scipy_version=scipy.__version__)
    print("wrote", path, os.path.getsize(path), "bytes;", len(cs), "cases; states", np.bincount(state, minlength=4).tolist())


if __name__ == "__main__":
    main()
