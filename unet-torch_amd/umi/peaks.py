"""Density-map (regression) evaluation: count maps, their local maxima and the scores the reference records for them.

The reference's regression scripts (test_mc3serousv5.py `test_single_reg`, test_reg3serousv5mt.py `test_multiple_reg`) take the
rectified head output, zoom it back to the image (order 0), divide it by 200, sum it (the predicted count), compute GAME at
levels 1-3 on it and match its local maxima, `skimage.feature.peak_local_max(estimation, min_distance=3)` after
`estimation[estimation < 0.001] = 0`, to the ground-truth dots (`CrowdMatchingTest(..., inputType='Regression')`).

scikit-image is not a dependency of this project and nothing could be recorded from it.  THE RULE below is this project's own
restatement of what scikit-image's source does for those arguments (a (2d+1)^2 footprint, threshold_abs = image.min(), no
relative threshold, exclude_border = min_distance, ensure_spacing with p_norm = inf); tests/test_peaks.py pins it to SciPy
(`scipy.ndimage.maximum_filter`, `scipy.spatial.cKDTree`).  Agreement with any scikit-image release is unmeasured.

    THE RULE, per image, d = min_distance (1..8):
      1. floor       a = x if x >= floor else 0, in float32 (NaN -> 0).  The input is not modified.
      2. candidates  m = max of a over the (2d+1) x (2d+1) window clipped to the image
                     (== scipy.ndimage.maximum_filter(a, size=2d+1, mode='nearest')).  A pixel is a candidate when a == m,
                     a > min(a) over the whole image, d <= y < H - d and d <= x < W - d.  A constant image has none, nor has one
                     with H <= 2d or W <= 2d.
      3. spacing     the candidates in raster order; one is kept unless an already kept one lies at Chebyshev distance <= d - 1.
                     (scikit-image walks them by descending value, stable.  Two candidates closer than d are each the maximum of
                     a window that holds the other, so they are equal, and among equal values the stable order is raster order:
                     both walks keep the same set.)
      4. order       value descending, raster ascending among equal values -- part of the result, the Gaussian matching is
                     greedy over the centres in list order.
      5. overflow    more than max_peaks peaks: the fault flag, the first max_peaks in output order, p_count = max_peaks.

`peak_lists_numpy`, `density_maps_numpy` and `score_density_numpy` are the statements; `peak_lists` and `density_maps` run
csrc/peaks.hip on device tensors (no host synchronisation, safe to capture), bit for bit the statements.  Pairs are (x, y).
"""
import numpy as np

MAX_PEAKS = 8192                     # == umi_peaks_max(): the centre count the matching kernels accept
MAX_DISTANCE = 8
FAULT_OVERFLOW, FAULT_CONTESTED = 1, 2


def _check_rule(min_distance, floor, max_peaks):
    d = int(min_distance)
    if d != min_distance or not 1 <= d <= MAX_DISTANCE:
        raise ValueError(f"min_distance must be an integer in 1..{MAX_DISTANCE}, got {min_distance}")
    if not 0 <= float(floor) < float("inf"):
        raise ValueError(f"floor must be finite and >= 0, got {floor}")
    if not 1 <= int(max_peaks) <= MAX_PEAKS:
        raise ValueError(f"max_peaks must be in 1..{MAX_PEAKS}")
    return d, np.float32(floor), int(max_peaks)


def _maps3(maps):
    m = np.asarray(maps)
    if m.ndim == 2:
        m = m[None]
    if m.ndim != 3 or m.dtype != np.float32 or min(m.shape) < 1:
        raise ValueError(f"expected non-empty float32 maps (N,H,W) or (H,W), got {m.shape} {m.dtype}")
    return m


def floor_map(x, floor=1e-3):
    """Step 1 on one float32 image: a new array, x where x >= floor, else 0 (NaN -> 0)."""
    with np.errstate(invalid="ignore"):
        return np.where(x >= np.float32(floor), x, np.float32(0)).astype(np.float32)


def window_max(a, d):
    """Maximum of the float32 image `a` over the (2d+1) x (2d+1) window clipped to the image: rows first, then columns."""
    H, W = a.shape
    p = np.full((H, W + 2 * d), -np.inf, dtype=np.float32)
    p[:, d:d + W] = a
    r = p[:, :W].copy()
    for k in range(1, 2 * d + 1):
        np.maximum(r, p[:, k:k + W], out=r)
    p = np.full((H + 2 * d, W), -np.inf, dtype=np.float32)
    p[d:d + H] = r
    m = p[:H].copy()
    for k in range(1, 2 * d + 1):
        np.maximum(m, p[k:k + H], out=m)
    return m


def candidates_numpy(x, min_distance=3, floor=1e-3):
    """Steps 1 and 2 on one image: (a, boolean candidate mask)."""
    d = int(min_distance)
    a = floor_map(x, floor)
    H, W = a.shape
    cand = (a == window_max(a, d)) & (a > a.min())
    inside = np.zeros((H, W), dtype=bool)
    if H > 2 * d and W > 2 * d:
        inside[d:H - d, d:W - d] = True
    return a, cand & inside


def spacing_numpy(cand, min_distance=3):
    """Step 3: the raster walk over a boolean candidate mask -> boolean kept mask."""
    h = int(min_distance) - 1
    kept = np.zeros(cand.shape, dtype=bool)
    ys, xs = np.nonzero(cand)
    for y, x in zip(ys.tolist(), xs.tolist()):
        if not kept[max(y - h, 0):y + h + 1, max(x - h, 0):x + h + 1].any():
            kept[y, x] = True
    return kept


def peak_lists_numpy(maps, min_distance=3, floor=1e-3, max_peaks=MAX_PEAKS):
    """THE RULE on float32 maps (N,H,W) or (H,W): peaks int32 (N, max_peaks, 2) as (x, y) in output order ((0, 0) beyond the
    count), p_count int32 (N,) and the fault flag (0, or FAULT_OVERFLOW when an image's list was cut at max_peaks)."""
    d, floor, max_peaks = _check_rule(min_distance, floor, max_peaks)
    m = _maps3(maps)
    peaks = np.zeros((m.shape[0], max_peaks, 2), dtype=np.int32)
    p_count = np.zeros(m.shape[0], dtype=np.int32)
    fault = 0
    for n in range(m.shape[0]):
        a, cand = candidates_numpy(m[n], d, floor)
        ys, xs = np.nonzero(spacing_numpy(cand, d))                 # raster order
        order = np.argsort(-a[ys, xs], kind="stable")               # value descending, raster ascending among equals
        if order.size > max_peaks:
            fault |= FAULT_OVERFLOW
            order = order[:max_peaks]
        p_count[n] = order.size
        peaks[n, :order.size, 0] = xs[order]
        peaks[n, :order.size, 1] = ys[order]
    return peaks, p_count, fault


def density_maps_numpy(out, scale=200.0):
    """(pred, counts): pred = max(out, 0) / scale in float32 (NaN stays NaN), counts float64 (N,) = the float64 sum per image."""
    x = _maps3(out)
    if not 0 < float(scale) < float("inf"):
        raise ValueError(f"scale must be positive and finite, got {scale}")
    pred = (np.maximum(x, np.float32(0)).astype(np.float32) / np.float32(scale)).astype(np.float32)
    return pred, pred.sum(axis=(1, 2), dtype=np.float64)


def density_scores(g_count, counts, p_count, crowd, cells_gt, cells_pred):
    """The host half of score_density_maps: per image the dot count, the float64 sum of the map, the peak count, the matching
    result (S, T, 2) and the two 8 x 8 cell sums -> the list of result dicts, every float by the reference's expressions."""
    import CrowdMatching as CM
    out = []
    for n in range(len(g_count)):
        gt, pred, npk = int(g_count[n]), float(counts[n]), int(p_count[n])
        abs_diff, acc, rel, rel_pd = CM.countAccuracyMetric(gt, pred)
        arr_prec, arr_recall, arr_f1 = CM.precision_recall_f1(crowd[n], gt, npk)
        out.append({"GT": gt, "Pred": pred, "AbsDiff": abs_diff, "Accuracy": acc, "AccuracyRelative": rel,
                    "AccuracyRelativePD": rel_pd,
                    "G1": CM.game_from_cells(1, cells_gt[n], cells_pred[n]), "G2": CM.game_from_cells(2, cells_gt[n], cells_pred[n]),
                    "G3": CM.game_from_cells(3, cells_gt[n], cells_pred[n]),
                    "peaks": npk, "arr_prec": arr_prec, "arr_recall": arr_recall, "arr_f1": arr_f1})
    return out


def pair_scores(first, second):
    """Two heads' lists of dicts -> per image {0: first, 1: second, 'ratio': ...}.  The reference reads a two-headed regression
    model's outputs as (immune, other) (test_reg3serousv5mt.py), so the ratio is head 0 / (head 0 + head 1) of the ground-truth
    dot counts and of the predicted float64 sums, through umi.matching.ratio_metrics."""
    from . import matching as M
    return [{0: a, 1: b, "ratio": M.ratio_metrics(b["GT"], a["GT"], b["Pred"], a["Pred"])} for a, b in zip(first, second)]


def _heads(pred, gt_dots):
    pair = isinstance(pred, (tuple, list))
    if pair != isinstance(gt_dots, (tuple, list)) or (pair and (len(pred) != 2 or len(gt_dots) != 2)):
        raise ValueError("a pair of heads needs a pair of dot maps: (pred_0, pred_1), (gt_0, gt_1)")
    return pair


def score_density_numpy(pred, gt_dots, sigma_list, sigma_thresh_list, size=512, min_distance=3, floor=1e-3):
    """umi.infer.score_density_maps on NumPy arrays, every step by the statements of this module and of umi/matching.py."""
    from . import matching as M
    if _heads(pred, gt_dots):
        return pair_scores(*(score_density_numpy(p, g, sigma_list, sigma_thresh_list, size, min_distance, floor)
                             for p, g in zip(pred, gt_dots)))
    p, g = _maps3(pred), np.asarray(gt_dots)
    if g.shape != p.shape:
        raise ValueError(f"expected (N,H,W) maps and dot maps of one shape, got {p.shape} {g.shape}")
    peaks, p_count, fault = peak_lists_numpy(p, min_distance, floor)
    raise_on_peak_fault(fault)
    dots, g_count = M.dot_lists_numpy(g)
    crowd = M.crowd_match_numpy(dots, g_count, peaks, p_count, sigma_list, sigma_thresh_list)
    cells_gt = M.grid_sums_numpy(g != 0, size)
    cells_pred = M.grid_sums_numpy(p, size)
    return density_scores(g_count, p.sum(axis=(1, 2), dtype=np.float64), p_count, crowd, cells_gt, cells_pred)


# ---- device entries ------------------------------------------------------------------------------------------------------
def raise_on_peak_fault(code, max_peaks=MAX_PEAKS):
    code = int(code)
    if code & FAULT_CONTESTED:
        raise RuntimeError("peak_lists: an image has more candidates within min_distance - 1 of one another than the kernel's "
                           "contested list holds; its list is invalid")
    if code & FAULT_OVERFLOW:
        raise RuntimeError(f"peak_lists: an image has more than max_peaks = {max_peaks} peaks; its list was cut short")


def _device_maps(maps, what):
    import torch
    if maps.dim() not in (2, 3) or maps.dtype != torch.float32:
        raise ValueError(f"{what} expects float32 maps (N,H,W) or (H,W), got {tuple(maps.shape)} {maps.dtype}")
    return (maps.unsqueeze(0) if maps.dim() == 2 else maps).contiguous()      # a strided view is copied


def peak_lists(maps, min_distance=3, floor=1e-3, max_peaks=MAX_PEAKS, check=False, _fault=False, vmin=None):
    """THE RULE on float32 device maps (N,H,W) or (H,W) (a non-contiguous view is copied): peaks int32 (N, max_peaks, 2) as
    (x, y) in output order, (0, 0) beyond the count, and p_count int32 (N,), on the device without a host synchronisation --
    the `centers`, `c_count` that umi.matching.crowd_match takes.  An image with more than max_peaks peaks keeps its first
    max_peaks and sets the kernels' fault word; check=True reads that word back (one synchronisation) and raises.  `vmin`:
    density_maps' per-image minimum of the same maps (saves the kernels' own pass over them).  NumPy input runs
    peak_lists_numpy (and raises on overflow when check=True)."""
    from .matching import _dev_modules, _is_dev, _to_np
    if not _is_dev(maps):
        peaks, p_count, fault = peak_lists_numpy(_to_np(maps), min_distance, floor, max_peaks)
        if check:
            raise_on_peak_fault(fault, max_peaks)
        return (peaks, p_count, fault) if _fault else (peaks, p_count)
    import torch
    L, ops = _dev_modules()
    d, fl, max_peaks = _check_rule(min_distance, floor, max_peaks)
    m = _device_maps(maps, "peak_lists")
    N, H, W = m.shape
    nbytes = L.fn("umi_peak_lists_ws_bytes")(N, H, W) if min(N, H, W) >= 1 and max(N, H, W) < 2 ** 31 else 0
    if nbytes == 0:
        raise ValueError(f"peak_lists: unsupported map shape {tuple(maps.shape)} (H, W <= 4096, N <= 65535, N * H * W < 2**31)")
    if vmin is not None and (not _is_dev(vmin) or vmin.dtype != torch.float32 or vmin.numel() != N or not vmin.is_contiguous()):
        raise ValueError("vmin must be density_maps' contiguous float32 (N,) device tensor")
    peaks = torch.empty((N, max_peaks, 2), dtype=torch.int32, device=m.device)
    p_count = torch.empty(N, dtype=torch.int32, device=m.device)
    ws = ops.workspace(nbytes, m.device)
    L.call("umi_peak_lists", m.data_ptr(), None if vmin is None else vmin.data_ptr(), peaks.data_ptr(), p_count.data_ptr(),
           N, H, W, d, float(fl), max_peaks, ws.data_ptr(), nbytes, ops._stream())
    fault = ops.fault_word(ws) if check or _fault else None
    if check:
        raise_on_peak_fault(fault, max_peaks)
    return (peaks, p_count, fault) if _fault else (peaks, p_count)


def _density(x, scale, with_map):
    import torch
    from .matching import _dev_modules
    L, ops = _dev_modules()
    m = _device_maps(x, "density_maps")
    N, H, W = m.shape
    nbytes = L.fn("umi_density_maps_ws_bytes")(N, H, W) if min(N, H, W) >= 1 and max(N, H, W) < 2 ** 31 else 0
    if nbytes == 0:
        raise ValueError(f"density_maps: unsupported map shape {tuple(x.shape)} (H, W <= 4096, N <= 65535, N * H * W < 2**31)")
    if not 0 < float(scale) < float("inf"):
        raise ValueError(f"scale must be positive and finite, got {scale}")
    pred = torch.empty_like(m) if with_map else None
    counts = torch.empty(N, dtype=torch.float64, device=m.device)
    vmin = torch.empty(N, dtype=torch.float32, device=m.device)
    ws = ops.workspace(nbytes, m.device)
    L.call("umi_density_maps", m.data_ptr(), pred.data_ptr() if with_map else None, counts.data_ptr(), vmin.data_ptr(), N, H, W,
           float(scale), ws.data_ptr(), nbytes, ops._stream())
    return pred, counts, vmin


def density_maps(out, scale=200.0, _vmin=False):
    """Head output float32 (N,H,W) or (H,W) -> (pred, counts): pred = relu(out) / scale in float32 (a true division; NaN stays
    NaN), counts float64 (N,) = the sum of pred per image in a fixed order.  Device tensors run umi_density_maps (no host
    synchronisation); NumPy arrays run density_maps_numpy."""
    from .matching import _is_dev, _to_np
    if not _is_dev(out):
        return density_maps_numpy(_to_np(out), scale)
    pred, counts, vmin = _density(out, scale, True)
    pred = pred[0] if out.dim() == 2 else pred
    return (pred, counts, vmin) if _vmin else (pred, counts)


def map_sums(maps):
    """(counts float64 (N,), vmin float32 (N,)) of float32 device maps as they are: the fixed-order float64 sum per image and the
    minimum with a NaN counted as 0 (what peak_lists takes as `vmin`)."""
    return _density(maps, 1.0, False)[1:]
