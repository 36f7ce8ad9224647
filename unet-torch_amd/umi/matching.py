"""Localisation scoring: matching the centres of a predicted mask's components to a ground-truth dot map.

The reference's evaluation scripts (CrowdMatching.py) score a prediction three ways, each restated here on coordinate lists:

  crowd_match      `CrowdMatchingTest` (:108-189).  The reference pastes a (2r+1)^2 Gaussian (r = int(round(4 * sigma)), peak
                   scaled to 1) around a centre into a full-image map, multiplies it with the map of the dots not matched yet,
                   takes the maximum and the first pixel that reaches it.  Equivalently: among the remaining dots with
                   |dx|, |dy| <= r look table[dy + r][dx + r] up; the largest value wins, the first dot in raster order on
                   ties; a value below the threshold (0 without a dot in the window) is a false positive, otherwise the dot
                   is matched and removed.  The table is the reference's own expression evaluated on the host (`gauss_table`),
                   so the values compared with the thresholds are the reference's float64 values bit for bit.
  distance_match   the three-argument `CrowdMatchingTest2` (:270-296): the dots in raster order, each takes the nearest centre
                   that is still free (the first on ties) if it is closer than `thresh`.  Distances are compared as squared
                   integers against `d2_limit(thresh)`, the largest integer whose float64 square root is < thresh: sqrt is
                   monotone and distinct integers of this size have distinct float64 roots, so argmin and the test are the
                   reference's.
  grid_sums        the 8 x 8 grid of cell sums `GMAE` (:309-331) derives its three levels from.

`dot_lists` turns dot maps into raster-ordered coordinate lists and `component_centers` turns `label_components`' statistics
into centres.  For class-valued masks and dot maps (the reference's test_mc3serousv5.py) `split_classes` gives one 0/1 plane per
class, `class_center_lists` one centre list per (image, class), and `multiclass_scores` forms the script's per-class and ratio
metrics from the integers.  Coordinate pairs are (x, y) throughout, the order of the reference's `(e_coord_x, e_coord_y)`.

Device tensors run the HIP kernels of csrc/matching.hip (batched, no host synchronisation, safe to capture in a graph once
`match_tables` has been called for the sigma and threshold lists).  NumPy arrays run the `*_numpy` statements below, which
tests/test_crowd_matching.py pins to recorded results of the reference.

Centres are PIXEL centroids, round(sum / area) with Python's round (half to even).  The reference's `_findObjects` takes
cv2.moments of the cv2.findContours outline instead, which is a different number and drops components whose outline
encloses no area; OpenCV is not a dependency of this project, so that definition is neither restated nor claimed.
"""
import math

import numpy as np

MAX_DOTS = 8192                      # dots per image the kernels handle (== umi_match_max_dots(): 32 register bits x 256 threads)
MAX_SIGMAS = 8


# ---- host-side constants -------------------------------------------------------------------------------------------------
def gauss_radius(sigma):
    return int(round(4 * sigma))


def gauss_table(sigma):
    """(r, table): the (2r+1, 2r+1) float64 Gaussian the reference compares with its thresholds: exp(-(x^2 + y^2) / (2 sigma^2))
    on the integer offsets -r..r, entries below eps * max zeroed, divided by its sum (MATLAB's fspecial), then divided by its
    maximum.  Evaluated with the reference's operations in the reference's order, so every entry has the reference's bits."""
    r = gauss_radius(sigma)
    off = np.arange(-float(r), float(r) + 1.0)
    x, y = off[None, :], off[:, None]
    h = np.exp(-(x * x + y * y) / (2. * sigma * sigma))
    h[h < np.finfo(h.dtype).eps * h.max()] = 0
    total = h.sum()
    if total != 0:
        h /= total
    return r, h / h.max()


def d2_limit(thresh):
    """The largest integer d2 with float64 sqrt(d2) < thresh (-1 when there is none): `sqrt(d2) < thresh` <=> `d2 <= d2_limit`."""
    thresh = float(thresh)
    if not thresh > 0:
        return -1
    if thresh >= 2.0 ** 31:
        return 2 ** 62
    k = int(thresh * thresh)
    while k >= 0 and not math.sqrt(k) < thresh:
        k -= 1
    while math.sqrt(k + 1) < thresh:
        k += 1
    return k


def _check_lists(sigma_list, thresh_list):
    sigmas, thr = [float(s) for s in sigma_list], [float(t) for t in thresh_list]
    if not sigmas or not thr or len(sigmas) > MAX_SIGMAS:
        raise ValueError(f"crowd_match needs 1..{MAX_SIGMAS} sigmas and at least one threshold")
    if any(not s > 0 for s in sigmas):
        raise ValueError("sigmas must be positive")
    if any(not t > 0 for t in thr):
        # with a threshold <= 0 the reference 'matches' the first zero pixel of the image; that is not restated
        raise ValueError("thresholds must be positive")
    return sigmas, thr


# ---- NumPy statements ----------------------------------------------------------------------------------------------------
def _batched(a, nd):
    a = np.asarray(a)
    return (a[None], True) if a.ndim == nd - 1 else (a, False)


def dot_lists_numpy(dot_map, max_dots=MAX_DOTS):
    """(N,H,W) or (H,W) map -> dots int32 (N, max_dots, 2) as (x, y) in raster order (rows beyond the count are 0), g_count
    int32 (N,).  More than max_dots dots in an image raises."""
    m, single = _batched(dot_map, 3)
    if m.ndim != 3:
        raise ValueError(f"expected an (N,H,W) or (H,W) dot map, got {m.shape}")
    dots = np.zeros((m.shape[0], max_dots, 2), dtype=np.int32)
    cnt = np.zeros(m.shape[0], dtype=np.int32)
    for n in range(m.shape[0]):
        ys, xs = np.nonzero(m[n])
        if ys.size > max_dots:
            raise RuntimeError(f"dot_lists: image {n} has {ys.size} dots, more than max_dots = {max_dots}")
        cnt[n] = ys.size
        dots[n, :ys.size, 0] = xs
        dots[n, :ys.size, 1] = ys
    return dots, cnt


def round_div_half_even(s, a):
    """round(s / a) for integer arrays s >= 0, a > 0, ties to even, in integers."""
    s, a = np.asarray(s, dtype=np.int64), np.asarray(a, dtype=np.int64)
    q, r2 = s // a, 2 * (s % a)
    return q + ((r2 > a) | ((r2 == a) & (q % 2 == 1)))


def component_centers_numpy(counts, area, sum_y, sum_x):
    """label_components' statistics (rows of cap entries) -> centres int32 (N, cap, 2), (0, 0) beyond counts[n]."""
    counts, area = np.asarray(counts).reshape(-1), np.asarray(area)
    area = area.reshape(counts.size, -1)
    sum_y, sum_x = np.asarray(sum_y).reshape(area.shape), np.asarray(sum_x).reshape(area.shape)
    live = (np.arange(area.shape[1])[None, :] < counts[:, None]) & (area > 0)
    safe = np.where(live, area, 1)
    out = np.zeros(area.shape + (2,), dtype=np.int32)
    out[..., 0] = np.where(live, round_div_half_even(sum_x, safe), 0)
    out[..., 1] = np.where(live, round_div_half_even(sum_y, safe), 0)
    return out


def crowd_match_numpy(dots, g_count, centers, c_count, sigma_list, thresh_list):
    """int32 (N, S, T, 2) = (tp, fp) of the Gaussian matching; dots (N, max_dots, 2), centers (N, cap, 2), counts (N,)."""
    sigmas, thr = _check_lists(sigma_list, thresh_list)
    dots, centers = np.asarray(dots, dtype=np.int64), np.asarray(centers, dtype=np.int64)
    g_count, c_count = np.asarray(g_count).reshape(-1), np.asarray(c_count).reshape(-1)
    N = dots.shape[0]
    out = np.zeros((N, len(sigmas), len(thr), 2), dtype=np.int32)
    tables = [gauss_table(s) for s in sigmas]
    for n in range(N):
        ng, nc = min(max(int(g_count[n]), 0), dots.shape[1]), min(max(int(c_count[n]), 0), centers.shape[1])
        gx, gy = dots[n, :ng, 0], dots[n, :ng, 1]
        for si, (r, tab) in enumerate(tables):
            for ti, th in enumerate(thr):
                remaining = np.ones(ng, dtype=bool)
                tp = fp = 0
                for c in range(nc):
                    dx, dy = gx - centers[n, c, 0], gy - centers[n, c, 1]
                    idx = np.flatnonzero(remaining & (np.abs(dx) <= r) & (np.abs(dy) <= r))
                    best, hit = 0.0, -1
                    if idx.size:
                        vals = tab[dy[idx] + r, dx[idx] + r]
                        k = int(np.argmax(vals))                 # the first maximum: the lowest raster index
                        best, hit = vals[k], int(idx[k])
                    if best < th:
                        fp += 1
                    else:
                        tp += 1
                        remaining[hit] = False
                out[n, si, ti] = (tp, fp)
    return out


def distance_match_numpy(dots, g_count, centers, c_count, thresh):
    """int32 (N, 3) = (tp, centres, dots) of the nearest-centre matching within `thresh` pixels."""
    lim = d2_limit(thresh)
    dots, centers = np.asarray(dots, dtype=np.int64), np.asarray(centers, dtype=np.int64)
    g_count, c_count = np.asarray(g_count).reshape(-1), np.asarray(c_count).reshape(-1)
    out = np.zeros((dots.shape[0], 3), dtype=np.int32)
    for n in range(dots.shape[0]):
        ng, nc = min(max(int(g_count[n]), 0), dots.shape[1]), min(max(int(c_count[n]), 0), centers.shape[1])
        cx, cy = centers[n, :nc, 0], centers[n, :nc, 1]
        free = np.ones(nc, dtype=bool)
        big = np.iinfo(np.int64).max
        tp = 0
        for g in range(ng if nc else 0):
            d2 = np.where(free, (cx - dots[n, g, 0]) ** 2 + (cy - dots[n, g, 1]) ** 2, big)
            k = int(np.argmin(d2))
            if free[k] and d2[k] <= lim:
                tp += 1
                free[k] = False
        out[n] = (tp, nc, ng)
    return out


def grid_sums_numpy(maps, size=512):
    """(N,H,W) or (H,W) map -> (N, 8, 8) sums over the 8 x 8 grid of (size // 8)-pixel cells, clipped to the image: int64 for
    integer maps, float64 otherwise."""
    m, _ = _batched(maps, 3)
    if size <= 0 or size % 8:
        raise ValueError("size must be a positive multiple of 8")
    cs = size // 8
    acc = np.int64 if m.dtype.kind in "biu" else np.float64
    out = np.zeros((m.shape[0], 8, 8), dtype=acc)
    for i in range(8):
        for j in range(8):
            out[:, i, j] = m[:, i * cs:(i + 1) * cs, j * cs:(j + 1) * cs].sum(axis=(1, 2), dtype=acc)
    return out


def scatter_centers_numpy(centers, c_count, H, W):
    """uint8 (N, H, W): 1 at every centre c < c_count[n] inside the image (coinciding centres count once)."""
    centers, c_count = np.asarray(centers), np.asarray(c_count).reshape(-1)
    out = np.zeros((centers.shape[0], H, W), dtype=np.uint8)
    for n in range(centers.shape[0]):
        c = centers[n, :min(max(int(c_count[n]), 0), centers.shape[1])]
        ok = (c[:, 0] >= 0) & (c[:, 0] < W) & (c[:, 1] >= 0) & (c[:, 1] < H)
        out[n, c[ok, 1], c[ok, 0]] = 1
    return out


def level_sums(cells, L):
    """Level-L (L = 0..3) cell sums from the (..., 8, 8) level-3 sums: (..., 2^L, 2^L)."""
    if L not in (0, 1, 2, 3):
        raise ValueError("GAME levels 0..3 are derived from the 8 x 8 grid")
    k = 8 >> L
    c = np.asarray(cells)
    return c.reshape(c.shape[:-2] + (1 << L, k, 1 << L, k)).sum(axis=(-3, -1))


# ---- class-valued masks and dot maps (reference test_mc3serousv5.py Results2Class / Results3Class) -------------------------
def split_classes_numpy(class_map, n_classes):
    """(N,H,W) or (H,W) class-valued map -> uint8 (N, n_classes - 1, H, W): plane c - 1 is 1 where the map equals c."""
    m, _ = _batched(class_map, 3)
    return np.stack([(m == c).astype(np.uint8) for c in range(1, n_classes)], axis=1)


def class_center_lists_numpy(counts, label_class, area, sum_y, sum_x, n_classes):
    """label_class_components' statistics (rows of cap entries) -> centers int32 (N * (n_classes - 1), cap, 2) and c_count
    int32 (N * (n_classes - 1),): per (image, class) the centres of that class's labels in label order, (0, 0) beyond."""
    counts, label_class = np.asarray(counts).reshape(-1), np.asarray(label_class)
    N, cap = label_class.shape
    allc = component_centers_numpy(np.minimum(counts, cap), area, sum_y, sum_x)
    centers = np.zeros((N * (n_classes - 1), cap, 2), dtype=np.int32)
    c_count = np.zeros(N * (n_classes - 1), dtype=np.int32)
    for n in range(N):
        live = np.arange(cap) < counts[n]
        for c in range(1, n_classes):
            pick = np.flatnonzero(live & (label_class[n] == c))
            j = n * (n_classes - 1) + c - 1
            c_count[j] = pick.size
            centers[j, :pick.size] = allc[n, pick]
    return centers, c_count


def ratio_metrics(cell_gt, immune_gt, cell_pred, immune_pred):
    """The ratio block of the reference's Results2Class.compareImages (test_mc3serousv5.py:499-501, 518-523) on Python ints:
    immune / (cell + immune) of the ground truth and of the prediction and countAccuracyMetric of the two.  A prediction
    without a cell or immune object raises ZeroDivisionError as the reference does; a ground truth without either gives a
    ratio of nan (the reference's numpy.uint64 0 / 0), and the metrics derived from it are whatever the reference's
    expressions make of nan.  Counts given as Python floats (the float64 sums of density maps, umi/peaks.py) stay floats, as in
    the reference's regression scripts (test_mc3serousv5.py:1015-1017)."""
    import CrowdMatching as CM
    cell_gt, immune_gt, cell_pred, immune_pred = (v if isinstance(v, float) else int(v)
                                                  for v in (cell_gt, immune_gt, cell_pred, immune_pred))
    ratio_gt = immune_gt / (cell_gt + immune_gt) if cell_gt + immune_gt else float("nan")
    ratio_pred = immune_pred / (cell_pred + immune_pred)
    abs_diff, acc, rel, rel_pd = CM.countAccuracyMetric(ratio_gt, ratio_pred)
    return {"GT": ratio_gt, "Pred": ratio_pred, "AbsDiff": round(abs_diff, 4), "Accuracy": acc, "AccuracyRelative": rel,
            "AccuracyRelativePD": rel_pd}


def ratio3_metrics(gt, pred, smooth=1e-6):
    """The count accuracies and the two ratios of the reference's Results3Class.compareImages (test_mc3serousv5.py:226-228,
    242-252) on Python ints; gt / pred = (cell, immune, tumor) counts = classes (1, 2, 3)."""
    (cg, ig, tg), (cp, ip, tp) = (int(v) for v in gt), (int(v) for v in pred)
    r_immo_gt, r_immo_pred = ig / (ig + tg + cg + smooth), ip / (ip + tp + cp + smooth)
    r_it_gt, r_it_pred = ig / (ig + tg + smooth), ip / (ip + tp + smooth)
    return {"cellAccuracy": round(abs(cg - cp) / (cg + smooth), 4), "immuneAccuracy": round(abs(ig - ip) / (ig + smooth), 4),
            "tumorAccuracy": round(abs(tg - tp) / (tg + smooth), 4),
            "GTImmo": r_immo_gt, "PredImmo": r_immo_pred, "AccuracyImmo": round(abs(r_immo_gt - r_immo_pred), 4),
            "GTImmoTummor": r_it_gt, "PredImmoTummor": r_it_pred, "AccuracyImmoTummor": round(abs(r_it_gt - r_it_pred), 4)}


def multiclass_scores(class_counts, g_count, c_count, crowd, cells_gt, cells_pred, n_classes):
    """The host half of score_multiclass_masks: integers (class_counts (N, K), and per (image, class) row j = n * (K - 1) + c - 1
    the dot count g_count[j], the centre count c_count[j], the matching result crowd[j] (S, T, 2) and the two 8 x 8 cell sums)
    -> the list of N result dicts, every float formed by the reference's expressions on Python ints."""
    import CrowdMatching as CM
    K = int(n_classes)
    class_counts = np.asarray(class_counts).reshape(-1, K)
    out = []
    for n in range(class_counts.shape[0]):
        d = {}
        for c in range(1, K):
            j = n * (K - 1) + c - 1
            gt, pred = int(g_count[j]), int(class_counts[n, c])
            abs_diff, acc, rel, rel_pd = CM.countAccuracyMetric(gt, pred)
            arr_prec, arr_recall, arr_f1 = CM.precision_recall_f1(crowd[j], gt, int(c_count[j]))
            d[c] = {"GT": gt, "Pred": pred, "AbsDiff": abs_diff, "Accuracy": acc, "AccuracyRelative": rel,
                    "AccuracyRelativePD": rel_pd,
                    "G1": CM.game_from_cells(1, cells_gt[j], cells_pred[j]), "G2": CM.game_from_cells(2, cells_gt[j], cells_pred[j]),
                    "G3": CM.game_from_cells(3, cells_gt[j], cells_pred[j]),
                    "arr_prec": arr_prec, "arr_recall": arr_recall, "arr_f1": arr_f1}
        if K >= 3:
            d["ratio"] = ratio_metrics(d[1]["GT"], d[2]["GT"], d[1]["Pred"], d[2]["Pred"])
        if K == 4:
            d["ratio3"] = ratio3_metrics([d[c]["GT"] for c in (1, 2, 3)], [d[c]["Pred"] for c in (1, 2, 3)])
        out.append(d)
    return out


def score_multiclass_numpy(mask, gt_dots, n_classes, sigma_list, sigma_thresh_list, size=512, max_components=65536):
    """umi.infer.score_multiclass_masks on NumPy arrays, every step by the NumPy statements of this module and of
    umi/components.py: `mask` (N,H,W) class values, `gt_dots` (N,H,W) map whose value is the class of the dot."""
    from .components import label_class_components_numpy
    mask, gt_dots = np.asarray(mask), np.asarray(gt_dots)
    if mask.ndim != 3 or gt_dots.shape != mask.shape:
        raise ValueError(f"expected (N,H,W) masks and dot maps of one shape, got {mask.shape} {gt_dots.shape}")
    N, H, W = mask.shape
    K = int(n_classes)
    cap = min(int(max_components), H * W)
    _, counts, class_counts, label_class, area, sum_y, sum_x = label_class_components_numpy(mask, K, cap)
    if (counts > cap).any():
        raise RuntimeError(f"score_multiclass_masks: an image has more than max_components = {cap} components")
    centers, c_count = class_center_lists_numpy(counts, label_class, area, sum_y, sum_x, K)
    planes = split_classes_numpy(gt_dots, K).reshape(N * (K - 1), H, W)
    dots, g_count = dot_lists_numpy(planes)
    crowd = crowd_match_numpy(dots, g_count, centers, c_count, sigma_list, sigma_thresh_list)
    cells_gt = grid_sums_numpy(planes, size)
    cells_pred = grid_sums_numpy(scatter_centers_numpy(centers, c_count, H, W), size)
    return multiclass_scores(class_counts, g_count, c_count, crowd, cells_gt, cells_pred, K)


# ---- device entries ------------------------------------------------------------------------------------------------------
def _is_dev(x):
    import torch
    return isinstance(x, torch.Tensor) and x.is_cuda


def _to_np(x):
    import torch
    return x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _dev_modules():
    from . import lib, ops
    return lib, ops


def raise_on_dot_overflow(code, max_dots=MAX_DOTS):
    if int(code):
        raise RuntimeError(f"dot_lists: an image has more than max_dots = {max_dots} dots; its list was cut short")


def dot_lists(dot_map, max_dots=MAX_DOTS, check=False, _fault=False):
    """Dot coordinates of (N,H,W) or (H,W) uint8 / float32 maps (a dot = a non-zero pixel): dots int32 (N, max_dots, 2) as
    (x, y) in raster order and g_count int32 (N,), on the device without a host synchronisation.  An image with more than
    max_dots dots keeps its first max_dots and sets the kernels' fault word; check=True reads that word back (one
    synchronisation) and raises.  NumPy input runs dot_lists_numpy."""
    if not _is_dev(dot_map):
        return dot_lists_numpy(_to_np(dot_map), max_dots)
    import torch
    L, ops = _dev_modules()
    if dot_map.dim() not in (2, 3) or dot_map.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"dot_lists expects an (N,H,W) or (H,W) uint8 / float32 map, got {tuple(dot_map.shape)} {dot_map.dtype}")
    m = (dot_map.unsqueeze(0) if dot_map.dim() == 2 else dot_map).contiguous()
    N, H, W = m.shape
    if not 1 <= max_dots <= MAX_DOTS:
        raise ValueError(f"max_dots must be in 1..{MAX_DOTS}")
    nbytes = L.fn("umi_dot_lists_ws_bytes")(N, H, W) if min(N, H, W) >= 1 and max(N, H, W) < 2 ** 31 else 0
    if nbytes == 0:
        raise ValueError(f"dot_lists: unsupported map shape {tuple(dot_map.shape)} (H, W <= 65536, N * H * W < 2**31)")
    dots = torch.zeros((N, max_dots, 2), dtype=torch.int32, device=m.device)
    g_count = torch.empty(N, dtype=torch.int32, device=m.device)
    ws = ops.workspace(nbytes, m.device)
    L.call("umi_dot_lists", m.data_ptr(), 0 if m.dtype == torch.uint8 else 1, dots.data_ptr(), g_count.data_ptr(), N, H, W,
           max_dots, ws.data_ptr(), nbytes, ops._stream())
    fault = ops.fault_word(ws) if check or _fault else None
    if check:
        raise_on_dot_overflow(fault, max_dots)
    return (dots, g_count, fault) if _fault else (dots, g_count)


def component_centers(counts, area, sum_y, sum_x):
    """Centres int32 (N, cap, 2) = (round(sum_x / area), round(sum_y / area)) (half to even, integer arithmetic) of
    label_components' outputs; (0, 0) beyond counts[n].  These are pixel centroids, not the reference's contour moments
    (see the module docstring)."""
    if not _is_dev(area):
        return component_centers_numpy(_to_np(counts), _to_np(area), _to_np(sum_y), _to_np(sum_x))
    import torch
    L, ops = _dev_modules()
    if area.dim() != 2 or area.dtype != torch.int32 or counts.dtype != torch.int32 or sum_y.dtype != torch.int64 or \
            sum_x.dtype != torch.int64 or sum_y.shape != area.shape or sum_x.shape != area.shape or counts.numel() != area.shape[0]:
        raise ValueError("component_centers expects label_components' counts (N,), area (N,cap) int32 and sum_y, sum_x int64")
    N, cap = area.shape
    centers = torch.empty((N, cap, 2), dtype=torch.int32, device=area.device)
    L.call("umi_component_centers", counts.contiguous().data_ptr(), area.contiguous().data_ptr(), sum_y.contiguous().data_ptr(),
           sum_x.contiguous().data_ptr(), centers.data_ptr(), N, cap, ops._stream())
    return centers


_tables = {}


def match_tables(sigma_list, thresh_list, device):
    """The device copies of the Gaussian tables and thresholds for these lists (cached; call it once before capturing
    crowd_match in a graph, the upload is a host-to-device copy).  Returns (radii ctypes array, tables, thresholds)."""
    import ctypes

    import torch
    sigmas, thr = _check_lists(sigma_list, thresh_list)
    key = (tuple(sigmas), tuple(thr), str(device))
    hit = _tables.get(key)
    if hit is None:
        tabs = [gauss_table(s) for s in sigmas]
        radii = (ctypes.c_int * len(tabs))(*[r for r, _ in tabs])
        flat = torch.from_numpy(np.concatenate([t.reshape(-1) for _, t in tabs])).to(device)
        hit = _tables[key] = (radii, flat, torch.tensor(thr, dtype=torch.float64).to(device))
    return hit


def _lists_on_device(dots, g_count, centers, c_count):
    import torch
    for t, shape in ((dots, 3), (centers, 3), (g_count, 1), (c_count, 1)):
        if not _is_dev(t) or t.dtype != torch.int32 or t.dim() != shape or not t.is_contiguous():
            raise ValueError("expected contiguous int32 device tensors: dots (N,max_dots,2), g_count (N,), centers (N,cap,2), "
                             "c_count (N,)")
    N = dots.shape[0]
    if N < 1 or dots.shape[2] != 2 or centers.shape[2] != 2 or centers.shape[0] != N or g_count.numel() != N or \
            c_count.numel() != N or not 1 <= dots.shape[1] <= MAX_DOTS or centers.shape[1] < 1:
        raise ValueError(f"inconsistent list shapes {tuple(dots.shape)} {tuple(centers.shape)} (1 <= max_dots <= {MAX_DOTS}, cap >= 1)")
    return N, dots.shape[1], centers.shape[1]


def crowd_match(dots, g_count, centers, c_count, sigma_list, thresh_list):
    """Gaussian matching (the reference's CrowdMatchingTest on coordinates): int32 (N, S, T, 2) = (tp, fp) per image, sigma and
    threshold.  dots / g_count as dot_lists gives them, centers int32 (N, cap, 2) with their per-image number c_count int32 (N,),
    which the kernel reads on the device.  One workgroup per (image, sigma, threshold); no host synchronisation."""
    if not _is_dev(dots):
        return crowd_match_numpy(_to_np(dots), _to_np(g_count), _to_np(centers), _to_np(c_count), sigma_list, thresh_list)
    import torch
    L, ops = _dev_modules()
    N, max_dots, cap = _lists_on_device(dots, g_count, centers, c_count)
    radii, tables, thr = match_tables(sigma_list, thresh_list, dots.device)
    out = torch.empty((N, len(radii), thr.numel(), 2), dtype=torch.int32, device=dots.device)
    L.call("umi_crowd_match", dots.data_ptr(), g_count.data_ptr(), max_dots, centers.data_ptr(), c_count.data_ptr(), cap,
           tables.data_ptr(), tables.numel(), radii, len(radii), thr.data_ptr(), thr.numel(),
           out.data_ptr(), N, ops._stream())
    return out


def distance_match(dots, g_count, centers, c_count, thresh):
    """Distance matching (the reference's three-argument CrowdMatchingTest2): int32 (N, 3) = (tp, centres, dots) per image."""
    if not _is_dev(dots):
        return distance_match_numpy(_to_np(dots), _to_np(g_count), _to_np(centers), _to_np(c_count), thresh)
    import torch
    L, ops = _dev_modules()
    N, max_dots, cap = _lists_on_device(dots, g_count, centers, c_count)
    out = torch.empty((N, 3), dtype=torch.int32, device=dots.device)
    nbytes = L.fn("umi_distance_match_ws_bytes")(N, cap)
    ws = ops.workspace(nbytes, dots.device)
    L.call("umi_distance_match", dots.data_ptr(), g_count.data_ptr(), max_dots, centers.data_ptr(), c_count.data_ptr(), cap,
           d2_limit(thresh), out.data_ptr(), N, ws.data_ptr(), nbytes, ops._stream())
    return out


def grid_sums(maps, size=512):
    """(N, 8, 8) sums over the 8 x 8 grid of (size // 8)-pixel cells of (N,H,W) or (H,W) maps, clipped to the image: int64 for
    uint8 maps, float64 (fixed summation order) for float32 maps.  GAME levels 1 and 2 are sums of these cells (level_sums)."""
    if not _is_dev(maps):
        return grid_sums_numpy(_to_np(maps), size)
    import torch
    L, ops = _dev_modules()
    if maps.dim() not in (2, 3) or maps.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"grid_sums expects an (N,H,W) or (H,W) uint8 / float32 map, got {tuple(maps.shape)} {maps.dtype}")
    if size <= 0 or size % 8:
        raise ValueError("size must be a positive multiple of 8")
    m = (maps.unsqueeze(0) if maps.dim() == 2 else maps).contiguous()
    N, H, W = m.shape
    if min(N, H, W) < 1 or N * H * W >= 2 ** 31 or N > 65535:
        raise ValueError(f"grid_sums: unsupported map shape {tuple(maps.shape)}")
    out = torch.empty((N, 8, 8), dtype=torch.int64 if m.dtype == torch.uint8 else torch.float64, device=m.device)
    L.call("umi_grid_sums", m.data_ptr(), 0 if m.dtype == torch.uint8 else 1, out.data_ptr(), N, H, W, int(size),
           ops._stream())
    return out


def scatter_centers(centers, c_count, H, W):
    """uint8 (N, H, W) map with 1 at every centre c < c_count[n] inside the image: the reference's `e_dot[cy, cx] = 1`
    (test.py:242-245), so coinciding centres count once."""
    if not _is_dev(centers):
        return scatter_centers_numpy(_to_np(centers), _to_np(c_count), H, W)
    import torch
    L, ops = _dev_modules()
    if centers.dim() != 3 or centers.shape[2] != 2 or centers.dtype != torch.int32 or c_count.dtype != torch.int32 or \
            c_count.numel() != centers.shape[0] or centers.shape[1] < 1 or not centers.is_contiguous():
        raise ValueError("scatter_centers expects centers int32 (N,cap,2) and c_count int32 (N,)")
    N, cap = centers.shape[:2]
    out = torch.empty((N, H, W), dtype=torch.uint8, device=centers.device)
    L.call("umi_scatter_centers", centers.data_ptr(), c_count.contiguous().data_ptr(), cap, out.data_ptr(), N, H, W,
           ops._stream())
    return out


def split_classes(class_map, n_classes):
    """uint8 (N, n_classes - 1, H, W) 0/1 planes of a class-valued uint8 (N,H,W) or (H,W) map, plane c - 1 = (map == c): the
    reference's `gt_dot_other[gt_dot == 1] = 1`, `gt_dot_immune[gt_dot == 2] = 1` (test_mc3serousv5.py:482-485).  dot_lists and
    grid_sums take the (N * (n_classes - 1), H, W) view."""
    if not _is_dev(class_map):
        return split_classes_numpy(_to_np(class_map), n_classes)
    import torch
    L, ops = _dev_modules()
    if class_map.dim() not in (2, 3) or class_map.dtype != torch.uint8:
        raise ValueError(f"split_classes expects a uint8 (N,H,W) or (H,W) map, got {tuple(class_map.shape)} {class_map.dtype}")
    m = (class_map.unsqueeze(0) if class_map.dim() == 2 else class_map).contiguous()
    N, H, W = m.shape
    K = int(n_classes)
    if not 2 <= K <= 256 or min(N, H, W) < 1 or N * (K - 1) * H * W >= 2 ** 31 or N > 65535:
        raise ValueError(f"split_classes: unsupported shape {tuple(class_map.shape)} for {K} classes")
    planes = torch.empty((N, K - 1, H, W), dtype=torch.uint8, device=m.device)
    L.call("umi_split_classes", m.data_ptr(), planes.data_ptr(), N, H, W, K, ops._stream())
    return planes


def class_center_lists(counts, label_class, area, sum_y, sum_x, n_classes):
    """Per (image, class 1 .. n_classes - 1) the centres of that class's components, from label_class_components' outputs:
    centers int32 (N * (n_classes - 1), cap, 2) in label order (the raster order of first pixels within the class), (0, 0)
    beyond the count, and c_count int32 (N * (n_classes - 1),) -- the layout crowd_match, distance_match and scatter_centers
    take.  Centres are the pixel centroids of component_centers.  A fixed-order compaction: two runs give the same lists."""
    if not _is_dev(area):
        return class_center_lists_numpy(_to_np(counts), _to_np(label_class), _to_np(area), _to_np(sum_y), _to_np(sum_x), n_classes)
    import torch
    L, ops = _dev_modules()
    if area.dim() != 2 or area.dtype != torch.int32 or counts.dtype != torch.int32 or label_class.dtype != torch.uint8 or \
            sum_y.dtype != torch.int64 or sum_x.dtype != torch.int64 or sum_y.shape != area.shape or sum_x.shape != area.shape or \
            label_class.shape != area.shape or counts.numel() != area.shape[0]:
        raise ValueError("class_center_lists expects label_class_components' counts (N,), label_class uint8 (N,cap), area int32 "
                         "(N,cap) and sum_y, sum_x int64 (N,cap)")
    N, cap = area.shape
    K = int(n_classes)
    if not 2 <= K <= 256 or N * (K - 1) * cap >= 2 ** 30:
        raise ValueError(f"class_center_lists: unsupported size N = {N}, cap = {cap}, {K} classes")
    centers = torch.empty((N * (K - 1), cap, 2), dtype=torch.int32, device=area.device)
    c_count = torch.empty(N * (K - 1), dtype=torch.int32, device=area.device)
    L.call("umi_class_center_lists", counts.contiguous().data_ptr(), label_class.contiguous().data_ptr(),
           area.contiguous().data_ptr(), sum_y.contiguous().data_ptr(), sum_x.contiguous().data_ptr(),
           centers.data_ptr(), c_count.data_ptr(), N, cap, K, ops._stream())
    return centers, c_count
