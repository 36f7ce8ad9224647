"""Localisation metrics with the reference module's names and signatures (reference CrowdMatching.py), on the MI355X.

    arr_prec, arr_recall, arr_f1 = CrowdMatchingTest(g_dot, (x, y), sigma_list, sigma_thresh_list, inputType='Coordinates')
    prec, recall, f1 = CrowdMatchingTest2(gt_dot, (x, y), 10)
    gmae, gmae_rel, gmae_rel_pd = GMAE(L, gtImg, predImg)          # size=512; the regression script's copy uses 768

NumPy inputs run the NumPy statements of umi/matching.py.  Device tensors (the dot map and the two coordinate tensors on the
GPU) run the kernels of csrc/matching.hip and read the integers (tp, fp, counts, cell sums) back ONCE per call; the floats are
then formed on the host with the reference's expressions, so both paths return what the reference returns, bit for bit:
no dots and no centres give all ones; no dots but some centres give recall one and zeros; `fn` is clamped at 0;
CrowdMatchingTest2 gives (0, 0, 0) without centres and raises ZeroDivisionError for centres without dots.

Not restated: inputType='Segmentation' (centres from cv2.findContours / cv2.moments) and 'Regression'
(skimage.feature.peak_local_max) -- neither library is a dependency of this project; pass coordinates, e.g. from
umi.infer.label_components + umi.matching.component_centers (pixel centroids, see umi/matching.py).  For density maps,
CrowdMatchingTestPeaks(g_dot, estimation, sigma_list, sigma_thresh_list) below takes the centres from the project's own
restatement of the local-maximum rule (umi/peaks.py, pinned to SciPy; its agreement with scikit-image itself is unmeasured),
which is why it has a name of its own and inputType='Regression' keeps raising.  Dot maps must hold only 0
and 1, thresholds must be positive, and on the NumPy path centres must lie inside the image (ValueError otherwise: the
reference's slicing does something of its own there).
"""
import numpy as np

from umi import matching as M


def _on_device(*xs):
    import torch
    dev = [isinstance(x, torch.Tensor) and x.is_cuda for x in xs]
    if any(dev) and not all(dev):
        raise ValueError("the dot map and the coordinates must all be device tensors or all be host arrays")
    return all(dev)


def _coordinates(estimation, inputType):
    if inputType == 'Segmentation':
        raise NotImplementedError("inputType='Segmentation' takes the centres from cv2.findContours / cv2.moments; OpenCV (cv2) is "
                                  "not a dependency of this project: pass inputType='Coordinates'")
    if inputType == 'Regression':
        raise NotImplementedError("inputType='Regression' takes the centres from skimage.feature.peak_local_max; scikit-image "
                                  "(skimage) is not a dependency of this project: pass inputType='Coordinates'")
    if inputType != 'Coordinates':
        raise ValueError(f"inputType {inputType!r}: expected 'Coordinates'")
    e_coord_x, e_coord_y = estimation
    if len(e_coord_x) != len(e_coord_y):
        raise ValueError("the x and y coordinate lists differ in length")
    return e_coord_x, e_coord_y


def _host_lists(g_dot, e_coord_x, e_coord_y, inside):
    """NumPy map and coordinates -> (dots, g_count, centers, c_count) of one image."""
    g = np.asarray(g_dot.numpy() if hasattr(g_dot, "numpy") else g_dot)
    if g.ndim != 2:
        raise ValueError(f"expected an (H, W) dot map, got {g.shape}")
    if not np.all((g == 0) | (g == 1)):
        raise ValueError("the dot map must hold only 0 and 1")
    x = np.asarray(e_coord_x.numpy() if hasattr(e_coord_x, "numpy") else e_coord_x).astype(np.int64).reshape(-1)
    y = np.asarray(e_coord_y.numpy() if hasattr(e_coord_y, "numpy") else e_coord_y).astype(np.int64).reshape(-1)
    if inside and x.size and (x.min() < 0 or y.min() < 0 or x.max() >= g.shape[1] or y.max() >= g.shape[0]):
        raise ValueError("centres must lie inside the image")
    ng = int(np.count_nonzero(g))
    dots, g_count = M.dot_lists_numpy(g, max_dots=max(ng, 1))
    centers = np.zeros((1, max(x.size, 1), 2), dtype=np.int64)
    centers[0, :x.size, 0], centers[0, :x.size, 1] = x, y
    return dots, g_count, centers, np.array([x.size], dtype=np.int32)


def _device_lists(g_dot, e_coord_x, e_coord_y):
    import torch
    if g_dot.dim() != 2:
        raise ValueError(f"expected an (H, W) dot map, got {tuple(g_dot.shape)}")
    dots, g_count, fault = M.dot_lists(g_dot, _fault=True)
    n = len(e_coord_x)
    centers = torch.zeros((1, max(n, 1), 2), dtype=torch.int32, device=g_dot.device)
    if n:
        centers[0, :, 0] = e_coord_x.reshape(-1)
        centers[0, :, 1] = e_coord_y.reshape(-1)
    c_count = torch.full((1,), n, dtype=torch.int32, device=g_dot.device)
    return dots, g_count, fault, centers, c_count


def precision_recall_f1(tp_fp, g_count, n_centers):
    """The reference's three (S, T) float64 arrays from the integer (S, T, 2) matching result of one image."""
    tp_fp = np.asarray(tp_fp)
    S, T = tp_fp.shape[:2]
    arr_prec, arr_recall, arr_f1 = np.zeros((S, T)), np.zeros((S, T)), np.zeros((S, T))
    if g_count == 0:
        arr_recall.fill(1)
        if n_centers == 0:
            arr_prec.fill(1)
            arr_f1.fill(1)
        return arr_prec, arr_recall, arr_f1
    for s in range(S):
        for t in range(T):
            tp, fp = int(tp_fp[s, t, 0]), int(tp_fp[s, t, 1])
            fn = max(float(g_count) - tp, 0)
            prec = tp / (tp + fp + 1e-7)
            recall = tp / (tp + fn)
            arr_prec[s, t] = prec
            arr_recall[s, t] = recall
            arr_f1[s, t] = 2 * prec * recall / (prec + recall + 1e-7)
    return arr_prec, arr_recall, arr_f1


def CrowdMatchingTest(g_dot, estimation, sigma_list, sigma_thresh_list, inputType='Segmentation'):
    """Precision, recall and F1, each (len(sigma_list), len(sigma_thresh_list)) float64, of the Gaussian matching of the centres
    `estimation` = (x coordinates, y coordinates) to the dots of the 0/1 map `g_dot` (H, W)."""
    e_coord_x, e_coord_y = _coordinates(estimation, inputType)
    if _on_device(g_dot, e_coord_x, e_coord_y):
        from umi import ops
        dots, g_count, fault, centers, c_count = _device_lists(g_dot, e_coord_x, e_coord_y)
        res = M.crowd_match(dots, g_count, centers, c_count, sigma_list, sigma_thresh_list)
        code, g_h, res_h = ops.read_back(fault, g_count, res)
        M.raise_on_dot_overflow(code[0])
        return precision_recall_f1(res_h[0], int(g_h[0]), len(e_coord_x))
    dots, g_count, centers, c_count = _host_lists(g_dot, e_coord_x, e_coord_y, inside=True)
    res = M.crowd_match_numpy(dots, g_count, centers, c_count, sigma_list, sigma_thresh_list)
    return precision_recall_f1(res[0], int(g_count[0]), int(c_count[0]))


def CrowdMatchingTestPeaks(g_dot, estimation, sigma_list, sigma_thresh_list, min_distance=3, floor=0.001):
    """CrowdMatchingTest on the local maxima of the float32 density map `estimation` (H, W): the reference's
    inputType='Regression' with the peaks taken by umi.peaks' rule (the restatement of peak_local_max(estimation, min_distance)
    after estimation[estimation < floor] = 0; `estimation` itself is left unmodified).  NumPy inputs run the statements; device
    tensors run the kernels (peak lists, dot lists, matching) and read the integers back once."""
    from umi import peaks as P
    if _on_device(g_dot, estimation):
        from umi import ops
        if g_dot.dim() != 2 or estimation.shape != g_dot.shape:
            raise ValueError(f"expected an (H, W) dot map and density map, got {tuple(g_dot.shape)} {tuple(estimation.shape)}")
        peaks, p_count, peak_fault = P.peak_lists(estimation, min_distance, floor, _fault=True)
        dots, g_count, dot_fault = M.dot_lists(g_dot, _fault=True)
        res = M.crowd_match(dots, g_count, peaks, p_count, sigma_list, sigma_thresh_list)
        peak_code, dot_code, g_h, p_h, res_h = ops.read_back(peak_fault, dot_fault, g_count, p_count, res)
        P.raise_on_peak_fault(peak_code[0])
        M.raise_on_dot_overflow(dot_code[0])
        return precision_recall_f1(res_h[0], int(g_h[0]), int(p_h[0]))
    est = np.asarray(estimation.numpy() if hasattr(estimation, "numpy") else estimation)
    if est.ndim != 2:
        raise ValueError(f"expected an (H, W) density map, got {est.shape}")
    peaks, p_count, fault = P.peak_lists_numpy(est, min_distance, floor)
    P.raise_on_peak_fault(fault)
    n = int(p_count[0])
    return CrowdMatchingTest(g_dot, (peaks[0, :n, 0], peaks[0, :n, 1]), sigma_list, sigma_thresh_list, inputType='Coordinates')


def _prf_distance(tp, n_centers, n_dots):
    prec = tp / n_centers
    recall = tp / n_dots
    return prec, recall, 2 * prec * recall / (prec + recall + 1e-7)


def CrowdMatchingTest2(gt_dot, predLocalization, thresh):
    """(precision, recall, F1) of the nearest-centre matching: every dot of `gt_dot` (non-zero pixels, raster order) takes the
    nearest centre not taken yet if it is closer than `thresh` pixels.  (0, 0, 0) without centres; ZeroDivisionError for
    centres without dots, as in the reference."""
    e_coord_x, e_coord_y = predLocalization
    if len(e_coord_x) == 0:
        return 0, 0, 0
    if _on_device(gt_dot, e_coord_x, e_coord_y):
        from umi import ops
        dots, g_count, fault, centers, c_count = _device_lists(gt_dot, e_coord_x, e_coord_y)
        res = M.distance_match(dots, g_count, centers, c_count, thresh)
        code, res_h = ops.read_back(fault, res)
        M.raise_on_dot_overflow(code[0])
        return _prf_distance(*res_h[0].tolist())
    g = np.asarray(gt_dot.numpy() if hasattr(gt_dot, "numpy") else gt_dot)
    dots, g_count, centers, c_count = _host_lists(g != 0, e_coord_x, e_coord_y, inside=False)
    tp, nc, ng = (int(v) for v in M.distance_match_numpy(dots, g_count, centers, c_count, thresh)[0])
    return _prf_distance(tp, nc, ng)


def countAccuracyMetric(countGT, countPred):
    """(absolute difference, difference / ground truth, difference / larger count, difference / mean count), the three ratios
    rounded to four places."""
    abs_diff = abs(countGT - countPred)
    return (abs_diff, round(abs_diff / (countGT + 1e-6), 4), round(abs_diff / (max(countGT, countPred) + 1e-6), 4),
            round((2 * abs_diff) / (countGT + countPred + 1e-6), 4))


def game_from_cells(L, gt_cells, pred_cells):
    """[sum of absolute cell count differences, sum of the relative ones, sum of the symmetric relative ones] at grid level L
    from the two (8, 8) level-3 cell sums, cells in raster order as the reference sums them."""
    gt, pred = M.level_sums(gt_cells, L), M.level_sums(pred_cells, L)
    total = [0, 0, 0]
    for i in range(gt.shape[0]):
        for j in range(gt.shape[1]):
            d, _, rel, rel_pd = countAccuracyMetric(int(gt[i, j]), int(pred[i, j]))
            total[0] += d
            total[1] += rel
            total[2] += rel_pd
    return total


def GMAE(L, gtImg, predImg, size=512):
    """Grid mean absolute error at level L (4^L cells of size // 2^L pixels over the top-left size x size pixels) of two count
    maps (H, W); L = 0..3.  Device tensors: uint8 or float32 maps, one read-back."""
    if _on_device(gtImg, predImg):
        from umi import ops
        cells = [c[0] for c in ops.read_back(M.grid_sums(gtImg, size), M.grid_sums(predImg, size))]
    else:
        cells = [M.grid_sums_numpy(np.asarray(m.numpy() if hasattr(m, "numpy") else m), size)[0] for m in (gtImg, predImg)]
    return game_from_cells(L, cells[0], cells[1])
