"""8-connected component labelling in NumPy: the CPU statement of what csrc/components.hip computes on the device.

`label_components_numpy(mask)` returns the same five outputs as `umi.infer.label_components`: label numbers in the raster
order of each component's first pixel (scipy.ndimage.label with a full 3x3 structure numbers them the same way;
tests/test_binary_infer.py compares the maps with `==`), counts, and per-label area and integer coordinate sums in rows of
`components_cap(H, W)` entries.  `loss.MRAccuracy` uses it for CPU tensors and the GPU tests use it as their live oracle.
`label_class_components_numpy(mask, n_classes)` is the same statement for class-valued masks (components of equal non-zero
value, numbered over all classes), the counterpart of `umi.infer.label_class_components`.

Run-based two-pass: the rows are cut into runs of foreground pixels, runs of adjacent rows that touch (8-connectivity: column
ranges overlapping after widening one of them by a pixel on each side) are linked, and the run graph is reduced to its
components by minimum-index hooking with pointer jumping, all as whole-array operations.  No SciPy, no OpenCV.
"""
import numpy as np


def components_cap(H, W):
    """Upper bound on the number of 8-connected components of an H x W mask: the four pixels of a 2 x 2 block are mutually
    adjacent, so a block meets at most one component."""
    return ((H + 1) // 2) * ((W + 1) // 2)


def _runs(m):
    """Row runs of a 2-D bool mask in raster order: row, first column, one-past-last column."""
    H, W = m.shape
    pad = np.zeros((H, W + 2), dtype=np.int8)
    pad[:, 1:-1] = m
    d = np.diff(pad, axis=1)
    ys, xs = np.nonzero(d == 1)
    _, xe = np.nonzero(d == -1)
    return ys, xs, xe


def _run_roots(ys, xs, xe, W):
    """For every run the smallest index of a run in its component."""
    n = ys.size
    lab = np.arange(n, dtype=np.int64)
    if n == 0:
        return lab
    # runs of the previous row touching run i: those with start <= end_i (exclusive end + 1 - 1) and end > start_i - 1, a
    # contiguous range of the raster-ordered run list; keys are row * (W + 2) + column
    K = W + 2
    key_start = ys * K + xs
    key_end = ys * K + xe                                   # exclusive
    lo = np.searchsorted(key_end, (ys - 1) * K + xs, side="left")        # first run above with end >= start_i (end > start_i - 1)
    hi = np.searchsorted(key_start, (ys - 1) * K + xe, side="right")     # first run above with start > end_i
    first_row = ys == 0
    cnt = np.where(first_row, 0, np.maximum(hi - lo, 0))
    tot = int(cnt.sum())
    if tot == 0:
        return lab
    a = np.repeat(np.arange(n, dtype=np.int64), cnt)
    offs = np.cumsum(cnt) - cnt
    b = np.repeat(lo, cnt) + (np.arange(tot, dtype=np.int64) - np.repeat(offs, cnt))
    while True:
        la, lb = lab[a], lab[b]
        differ = la != lb
        if not differ.any():
            return lab
        la, lb = la[differ], lb[differ]
        mn = np.minimum(la, lb)
        np.minimum.at(lab, la, mn)                           # hook the larger root under the smaller one
        np.minimum.at(lab, lb, mn)
        while True:                                          # pointer jumping until every run points at a root
            nxt = lab[lab]
            if np.array_equal(nxt, lab):
                break
            lab = nxt


def _label_one(m):
    H, W = m.shape
    cap = components_cap(H, W)
    ys, xs, xe = _runs(m)
    ys, xs, xe = ys.astype(np.int64), xs.astype(np.int64), xe.astype(np.int64)
    root = _run_roots(ys, xs, xe, W)
    is_root = root == np.arange(root.size)
    number = np.cumsum(is_root)                             # 1-based label of a root run, raster order of first pixels
    run_label = number[root] if root.size else root
    count = int(is_root.sum())
    flat = np.zeros(H * W + 1, dtype=np.int64)
    np.add.at(flat, ys * W + xs, run_label)
    np.add.at(flat, ys * W + xe, -run_label)                # xe == W lands on the next row's first pixel: its own run adds there
    labels = np.cumsum(flat)[:-1].reshape(H, W).astype(np.int32)
    ln = xe - xs
    area = np.zeros(cap, dtype=np.int64)
    sum_y = np.zeros(cap, dtype=np.int64)
    sum_x = np.zeros(cap, dtype=np.int64)
    if root.size:
        np.add.at(area, run_label - 1, ln)
        np.add.at(sum_y, run_label - 1, ln * ys)
        np.add.at(sum_x, run_label - 1, ln * xs + ln * (ln - 1) // 2)
    first = (ys * W + xs)[is_root]
    return labels, count, area.astype(np.int32), sum_y, sum_x, first


def label_components_numpy(mask, return_first=False):
    """mask: (N, H, W) or (H, W) array, foreground = non-zero.  Returns labels int32 (same shape; 0 = background, 1..n in the
    raster order of each component's first pixel), counts int32 (N,), area int32 (N, cap), sum_y and sum_x int64 (N, cap),
    cap = components_cap(H, W); rows beyond counts[n] are 0.  return_first=True appends a list with each image's vector of
    first-pixel flat indices (y * W + x), one per label."""
    mask = np.asarray(mask)
    if mask.ndim == 2:
        mask = mask[None]
        single = True
    elif mask.ndim == 3:
        single = False
    else:
        raise ValueError(f"expected an (N, H, W) or (H, W) mask, got {mask.shape}")
    N, H, W = mask.shape
    if H < 1 or W < 1:
        raise ValueError(f"empty mask {mask.shape}")
    cap = components_cap(H, W)
    labels = np.zeros((N, H, W), dtype=np.int32)
    counts = np.zeros(N, dtype=np.int32)
    area = np.zeros((N, cap), dtype=np.int32)
    sum_y = np.zeros((N, cap), dtype=np.int64)
    sum_x = np.zeros((N, cap), dtype=np.int64)
    firsts = []
    for n in range(N):
        labels[n], counts[n], area[n], sum_y[n], sum_x[n], f = _label_one(mask[n] != 0)
        firsts.append(f)
    if single:
        labels = labels[0]
    out = (labels, counts, area, sum_y, sum_x)
    return out + (firsts,) if return_first else out


MAX_CLASSES = 8                      # class values 0 .. 7 (csrc/components.hip CC_MAX_CLASSES)


def class_components_cap(H, W, n_classes):
    """Upper bound on the number of same-class 8-connected components of an H x W mask with values 0 .. n_classes - 1: the
    four pixels of a 2 x 2 block are mutually adjacent, so a block meets at most one component per class and at most four."""
    return min(min(n_classes - 1, 4) * components_cap(H, W), H * W)


def label_class_components_numpy(mask, n_classes, max_components=None, return_first=False):
    """Class-aware labelling of an (N, H, W) or (H, W) array of class values 0 .. n_classes - 1: two pixels are in one
    component iff they are 8-connected through pixels of the same non-zero value (scipy.ndimage.label(mask == c, ones((3, 3)))
    for every c).  A value >= n_classes is background.  Returns what umi.infer.label_class_components returns:
      labels int32 (the mask's shape; 0 = background, 1..n over ALL classes in the raster order of each component's first pixel),
      counts int32 (N,), class_counts int32 (N, n_classes) (column 0 is 0), label_class uint8 (N, cap), area int32 (N, cap),
      sum_y and sum_x int64 (N, cap); cap = max_components or class_components_cap(H, W, n_classes); rows beyond counts[n]
      are 0 and an image with more than cap components keeps exact counts and labels and the rows of its first cap labels.
    return_first=True appends a list with each image's vector of first-pixel flat indices, one per label."""
    mask = np.asarray(mask)
    if mask.ndim == 2:
        mask = mask[None]
        single = True
    elif mask.ndim == 3:
        single = False
    else:
        raise ValueError(f"expected an (N, H, W) or (H, W) mask, got {mask.shape}")
    if not 2 <= n_classes <= MAX_CLASSES:
        raise ValueError(f"n_classes must be in 2..{MAX_CLASSES}")
    N, H, W = mask.shape
    if H < 1 or W < 1:
        raise ValueError(f"empty mask {mask.shape}")
    cap = class_components_cap(H, W, n_classes) if max_components is None else int(max_components)
    if not 1 <= cap <= H * W:
        raise ValueError(f"max_components must be in 1..{H * W}")
    labels = np.zeros((N, H, W), dtype=np.int32)
    counts = np.zeros(N, dtype=np.int32)
    class_counts = np.zeros((N, n_classes), dtype=np.int32)
    label_class = np.zeros((N, cap), dtype=np.uint8)
    area = np.zeros((N, cap), dtype=np.int32)
    sum_y = np.zeros((N, cap), dtype=np.int64)
    sum_x = np.zeros((N, cap), dtype=np.int64)
    firsts = []
    for n in range(N):
        per = []
        for c in range(1, n_classes):
            lab, cnt, a, sy, sx, first = _label_one(mask[n] == c)
            class_counts[n, c] = cnt
            per.append((c, lab, a[:cnt], sy[:cnt], sx[:cnt], first))
        first = np.concatenate([p[5] for p in per])
        order = np.argsort(first, kind="stable")                # first pixels are distinct: the global raster order
        counts[n] = first.size
        k = min(first.size, cap)
        for name, j in ((area, 2), (sum_y, 3), (sum_x, 4)):
            name[n, :k] = np.concatenate([p[j] for p in per])[order][:k]
        label_class[n, :k] = np.concatenate([np.full(p[5].size, p[0], dtype=np.uint8) for p in per])[order][:k]
        number = np.empty(first.size, dtype=np.int32)
        number[order] = np.arange(1, first.size + 1, dtype=np.int32)
        at = 0
        for c, lab, *_rest, f in per:
            lut = np.concatenate([np.zeros(1, dtype=np.int32), number[at:at + f.size]])
            labels[n] += lut[lab]
            at += f.size
        firsts.append(first[order])
    if single:
        labels = labels[0]
    out = (labels, counts, class_counts, label_class, area, sum_y, sum_x)
    return out + (firsts,) if return_first else out


def count_components_numpy(mask):
    """Number of 8-connected components of one (H, W) mask."""
    m = np.asarray(mask) != 0
    ys, xs, xe = _runs(m)
    root = _run_roots(ys.astype(np.int64), xs.astype(np.int64), xe.astype(np.int64), m.shape[1])
    return int((root == np.arange(root.size)).sum())


def label_checksum(labels):
    """int64 checksum of one (H, W) label map: sum of label[p] * (p mod 65521 + 1) over flat indices p."""
    lab = np.asarray(labels).astype(np.int64).ravel()
    return int((lab * (np.arange(lab.size, dtype=np.int64) % 65521 + 1)).sum())
