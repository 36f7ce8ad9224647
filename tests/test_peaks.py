"""CPU: the NumPy statement of the density-map peak rule (umi/peaks.py) against its SciPy formulations -- computed here and
recorded in tests/golden/density_peaks.npz by tools/gen_golden_density.py -- its edge cases, and the host functions built on it.
Every comparison is exact.  Nothing here is scikit-image's output: agreement with scikit-image itself is unmeasured."""
import os

import numpy as np
import pytest

from tools import gen_golden_density as G

THRESHOLDS = np.arange(0.5, 1, 0.05)
SIGMAS = [5, 20]


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "density_peaks.npz"))


def _list(peaks, p_count, n=0):
    return peaks[n, :p_count[n]]


def _single(H, W, *spikes, base=0.0):
    m = np.full((H, W), base, dtype=np.float32)
    for y, x, v in spikes:
        m[y, x] = v
    return m


# ---- 1. the SciPy pin ----------------------------------------------------------------------------------------------------------
def test_fixture_lists_the_generator_cases(fixture):
    assert list(fixture["case_names"]) == G.CASES and tuple(fixture["distances"]) == G.DISTANCES
    for name in G.CASES:
        assert np.array_equal(fixture[f"map_{name}"], G.case(name))


@pytest.mark.parametrize("d", G.DISTANCES)
@pytest.mark.parametrize("name", G.CASES)
def test_statement_equals_scipy(fixture, name, d):
    from umi import peaks as P
    x = G.case(name)
    a, cand = P.candidates_numpy(x, d, G.FLOOR)
    # the window maximum and the candidates are the maximum_filter formulation, computed now and as recorded
    wmax = G.scipy_window_max(a, d)
    assert np.array_equal(P.window_max(a, d), wmax) and np.array_equal(wmax, fixture[f"wmax_{name}_{d}"])
    a2, cand2 = G.scipy_candidates(x, d)
    assert np.array_equal(a, a2) and np.array_equal(cand, cand2)
    # the kept set AND the order are the cKDTree greedy over the value-sorted candidates, computed now and as recorded
    peaks, p_count, fault = P.peak_lists_numpy(x, d, G.FLOOR)
    want = G.kdtree_greedy(a, cand, d)
    assert fault == 0 and np.array_equal(_list(peaks, p_count), want) and np.array_equal(want, fixture[f"kept_{name}_{d}"])
    assert not peaks[0, p_count[0]:].any()
    # the two walk orders keep the same set
    ys, xs = np.nonzero(P.spacing_numpy(cand, d))
    assert sorted(zip(xs.tolist(), ys.tolist())) == sorted(map(tuple, want.tolist()))


def test_the_maps_exercise_the_spacing_step(fixture):
    """The pin above means something only if candidates are dropped by the spacing step somewhere."""
    from umi import peaks as P
    dropped = 0
    for name in G.CASES:
        for d in (3, 5):
            _, cand = P.candidates_numpy(G.case(name), d, G.FLOOR)
            dropped += int(cand.sum()) - len(fixture[f"kept_{name}_{d}"])
    assert dropped > 100


# ---- 2. edge cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", (1, 3, 8))
def test_constant_and_below_floor_images_have_no_peaks(d):
    from umi import peaks as P
    for m in (np.full((20, 21), 0.5, np.float32), np.full((20, 21), 0.0005, np.float32), np.zeros((20, 21), np.float32),
              np.random.default_rng(0).random((20, 21)).astype(np.float32) * 0.00099):
        peaks, p_count, fault = P.peak_lists_numpy(m, d)
        assert p_count.tolist() == [0] and fault == 0 and not peaks.any()


@pytest.mark.parametrize("shape,d", [((6, 30), 3), ((30, 6), 3), ((2, 2), 1), ((16, 40), 8), ((1, 9), 1)])
def test_images_no_larger_than_the_border_have_no_peaks(shape, d):
    from umi import peaks as P
    m = np.random.default_rng(1).random(shape).astype(np.float32)
    assert P.peak_lists_numpy(m, d)[1].tolist() == [0]


@pytest.mark.parametrize("d", (1, 3, 5))
def test_border_distance(d):
    from umi import peaks as P
    H, W = 4 * d + 5, 4 * d + 7
    for y, x, keep in ((d - 1, W // 2, False), (d, W // 2, True), (H // 2, d - 1, False), (H // 2, d, True),
                       (H - d, W // 2, False), (H - d - 1, W // 2, True), (H // 2, W - d, False), (H // 2, W - d - 1, True)):
        peaks, p_count, _ = P.peak_lists_numpy(_single(H, W, (y, x, 1.0)), d)
        assert _list(peaks, p_count).tolist() == ([[x, y]] if keep else []), (y, x)


@pytest.mark.parametrize("d", (2, 3, 5))
def test_two_equal_maxima(d):
    from umi import peaks as P
    H, W = 6 * d, 6 * d
    y, x = 2 * d, 2 * d
    for dy, dx in ((0, 1), (1, 0), (1, 1), (1, -1)):
        near = _single(H, W, (y, x, 1.0), (y + dy * (d - 1), x + dx * (d - 1), 1.0))
        peaks, p_count, _ = P.peak_lists_numpy(near, d)
        assert _list(peaks, p_count).tolist() == [[x, y]]                       # the later one in raster order is dropped
        far = _single(H, W, (y, x, 1.0), (y + dy * d, x + dx * d, 1.0))
        peaks, p_count, _ = P.peak_lists_numpy(far, d)
        assert _list(peaks, p_count).tolist() == [[x, y], [x + dx * d, y + dy * d]]


def test_order_is_value_descending_then_raster():
    from umi import peaks as P
    m = _single(30, 30, (5, 20, 0.5), (12, 4, 0.75), (12, 14, 0.5), (20, 9, 2.0), (25, 25, 0.5))
    peaks, p_count, _ = P.peak_lists_numpy(m, 3)
    assert _list(peaks, p_count).tolist() == [[9, 20], [4, 12], [20, 5], [14, 12], [25, 25]]


def test_nan_and_inf_pixels():
    from umi import peaks as P
    m = _single(20, 20, (5, 5, np.nan), (10, 10, np.inf), (15, 5, 0.5))
    keep = m.copy()
    peaks, p_count, fault = P.peak_lists_numpy(m, 3)
    assert _list(peaks, p_count).tolist() == [[10, 10], [5, 15]] and fault == 0       # NaN -> 0: no peak; +inf first
    assert np.array_equal(m, keep, equal_nan=True)
    allnan = np.full((12, 12), np.nan, dtype=np.float32)
    assert P.peak_lists_numpy(allnan, 3)[1].tolist() == [0]


def test_overflow_keeps_the_first_in_output_order():
    from umi import peaks as P
    m = _single(30, 30, (5, 20, 0.5), (12, 4, 0.75), (12, 14, 0.5), (20, 9, 2.0), (25, 25, 0.5), (25, 5, 0.25))
    peaks, p_count, fault = P.peak_lists_numpy(np.stack([m, np.zeros_like(m)]), 3, max_peaks=4)
    assert fault == P.FAULT_OVERFLOW and p_count.tolist() == [4, 0] and peaks.shape == (2, 4, 2)
    assert peaks[0].tolist() == [[9, 20], [4, 12], [20, 5], [14, 12]]
    with pytest.raises(RuntimeError, match="max_peaks = 4"):
        P.peak_lists(m, 3, max_peaks=4, check=True)
    assert P.peak_lists(m, 3, max_peaks=6, check=True)[1].tolist() == [6]


def test_the_input_is_left_unmodified_and_arguments_are_checked():
    from umi import peaks as P
    m = G.make_map("noise", 16, 16, 3) * np.float32(0.002)
    keep = m.copy()
    P.peak_lists_numpy(m, 3)
    assert np.array_equal(m, keep) and (m < 1e-3).any()
    for bad in (dict(min_distance=0), dict(min_distance=9), dict(min_distance=2.5), dict(floor=-1.0), dict(floor=np.nan),
                dict(max_peaks=0), dict(max_peaks=P.MAX_PEAKS + 1)):
        with pytest.raises(ValueError):
            P.peak_lists_numpy(m, **bad)
    with pytest.raises(ValueError):
        P.peak_lists_numpy(m.astype(np.float64))


def test_density_maps_numpy():
    from umi import peaks as P
    x = np.array([[[-1.0, 0.0, 100.0], [np.nan, 300.0, 50.0]]], dtype=np.float32)
    pred, counts = P.density_maps(x)
    assert pred.dtype == np.float32 and counts.dtype == np.float64
    assert np.array_equal(pred[0], np.array([[0, 0, 0.5], [np.nan, 1.5, 0.25]], dtype=np.float32), equal_nan=True)
    assert np.isnan(counts[0])
    pred, counts = P.density_maps_numpy(np.nan_to_num(x))
    assert counts.tolist() == [2.25]
    # a division, not a multiplication by the reciprocal: the two differ in the last bit for many values
    v = np.arange(1, 4097, dtype=np.float32)
    assert np.array_equal(P.density_maps_numpy(v[None, None])[0][0, 0], v / np.float32(200))
    assert (v / np.float32(200) != v * (np.float32(1) / np.float32(200))).any()


# ---- 3. the drop-in function and the scoring dictionary ----------------------------------------------------------------------------
def _bumps(H, W, centres, sigma=1.5, amp=0.2):
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    m = np.zeros((H, W))
    for cy, cx in centres:
        m += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sigma * sigma))
    return m.astype(np.float32)


def test_crowd_matching_test_peaks_equals_coordinates():
    import CrowdMatching as CM
    from umi import peaks as P
    rng = np.random.default_rng(7)
    centres = [(int(rng.integers(6, 58)), int(rng.integers(6, 58))) for _ in range(14)]
    est = _bumps(64, 64, centres)
    g = np.zeros((64, 64), dtype=np.uint8)
    for cy, cx in centres[:11]:
        g[min(cy + int(rng.integers(-2, 3)), 63), cx] = 1
    keep = est.copy()
    got = CM.CrowdMatchingTestPeaks(g, est, SIGMAS, THRESHOLDS)
    peaks, p_count, _ = P.peak_lists_numpy(est)
    assert 5 <= p_count[0] <= 14 and np.array_equal(est, keep)
    want = CM.CrowdMatchingTest(g, (peaks[0, :p_count[0], 0], peaks[0, :p_count[0], 1]), SIGMAS, THRESHOLDS, inputType='Coordinates')
    for a, b in zip(got, want):
        assert a.dtype == np.float64 and np.array_equal(a, b)
    assert 0 < got[0][0, 0] <= 1


def test_regression_input_type_still_raises():
    import CrowdMatching as CM
    g = np.zeros((8, 8), dtype=np.uint8)
    with pytest.raises(NotImplementedError, match="skimage"):
        CM.CrowdMatchingTest(g, np.zeros((8, 8), np.float32), SIGMAS, THRESHOLDS, inputType='Regression')


def _by_eye():
    """64 x 64, size 64 (8-pixel cells): three unit-mass-ish spikes whose numbers can be checked by eye.
    map: 0.5 at (y 10, x 10), 0.25 at (y 10, x 40), 1.0 at (y 50, x 20); dots at (10, 10), (11, 40) and (30, 30)."""
    pred = _single(64, 64, (10, 10, 0.5), (10, 40, 0.25), (50, 20, 1.0))
    g = np.zeros((64, 64), dtype=np.uint8)
    g[10, 10] = g[11, 40] = g[30, 30] = 1
    return pred, g


def test_score_density_numpy_by_eye():
    from umi import peaks as P
    pred, g = _by_eye()
    (d,) = P.score_density_numpy(pred[None], g[None], [1], [0.5, 0.7], size=64)
    assert d["GT"] == 3 and d["Pred"] == 1.75 and d["peaks"] == 3
    assert d["AbsDiff"] == 1.25 and d["Accuracy"] == round(1.25 / (3 + 1e-6), 4) and d["AccuracyRelative"] == round(1.25 / (3 + 1e-6), 4)
    assert d["AccuracyRelativePD"] == round(2.5 / (4.75 + 1e-6), 4)
    # peaks in order: (20, 50) 1.0, (10, 10) 0.5, (40, 10) 0.25.  sigma 1: the peak on its dot scores 1, the one a pixel off
    # exp(-1/2) = 0.61 (a match at 0.5, not at 0.7), the third has no dot in reach
    assert d["arr_prec"].shape == (1, 2)
    assert np.allclose(d["arr_prec"][0], [2 / 3, 1 / 3]) and np.allclose(d["arr_recall"][0], [2 / 3, 1 / 3])
    # GAME: int() of every cell sum of the map is 0 except the cell of the 1.0 spike (lower left at every level); the dots sit
    # in three cells at levels 3 and 2 and as 2 + 1 in the two upper cells at level 1: 1 + 1 + 1 + 1, then 2 + 1 + 1
    assert d["G3"][0] == 4 and d["G2"][0] == 4 and d["G1"][0] == 4
    assert len(d["G1"]) == 3
    # a pair of heads: the ratio block on the float sums, head 0 read as 'immune'
    (p,) = P.score_density_numpy((pred[None], 2 * pred[None]), (g[None], g[None]), [1], [0.5], size=64)
    assert p[0]["Pred"] == 1.75 and p[1]["Pred"] == 3.5
    assert p["ratio"]["GT"] == 0.5 and p["ratio"]["Pred"] == 1.75 / 5.25 and p["ratio"]["AbsDiff"] == round(0.5 - 1.75 / 5.25, 4)


def test_cabi_symbols_exist():
    from umi import lib
    for name in ("umi_peaks_max", "umi_density_maps_ws_bytes", "umi_density_maps", "umi_peak_lists_ws_bytes", "umi_peak_lists"):
        assert name in lib.SIGNATURES and hasattr(lib.lib, name)
    from umi import peaks as P
    assert lib.fn("umi_peaks_max")() == P.MAX_PEAKS == lib.fn("umi_match_max_dots")()
    assert lib.ENUMS["UMI_PEAKS_FAULT_OVERFLOW"] == P.FAULT_OVERFLOW and lib.ENUMS["UMI_PEAKS_FAULT_CONTESTED"] == P.FAULT_CONTESTED
    # bad arguments are a status before any launch (no GPU touched)
    f = lib.fn("umi_peak_lists")
    assert f(None, None, None, None, 1, 8, 8, 3, 1e-3, 16, None, 0, None) == lib.UMI_ERR_BADARG
    assert f(1, None, 1, 1, 1, 8, 8, 0, 1e-3, 16, 1, 1 << 30, None) == lib.UMI_ERR_BADARG
    assert f(1, None, 1, 1, 1, 8, 8, 3, -1.0, 16, 1, 1 << 30, None) == lib.UMI_ERR_BADARG
    assert f(1, None, 1, 1, 1, 8, 8, 9, 1e-3, 16, 1, 1 << 30, None) == lib.UMI_ERR_UNSUPPORTED
    assert f(1, None, 1, 1, 1, 8, 8, 3, 1e-3, 8193, 1, 1 << 30, None) == lib.UMI_ERR_UNSUPPORTED
    assert f(1, None, 1, 1, 1, 4097, 8, 3, 1e-3, 16, 1, 1 << 30, None) == lib.UMI_ERR_UNSUPPORTED
    assert f(1, None, 1, 1, 1, 8, 8, 3, 1e-3, 16, None, 0, None) == lib.UMI_ERR_WORKSPACE
    assert lib.fn("umi_peak_lists_ws_bytes")(1, 4097, 8) == 0 and lib.fn("umi_peak_lists_ws_bytes")(1, 64, 64) > 64 * 64
    g = lib.fn("umi_density_maps")
    assert g(None, None, None, None, 1, 8, 8, 200.0, None, 0, None) == lib.UMI_ERR_BADARG
    assert g(1, 1, 1, None, 1, 8, 8, 0.0, 1, 1 << 30, None) == lib.UMI_ERR_BADARG
    assert g(1, 1, 1, None, 1, 8, 8, 200.0, None, 0, None) == lib.UMI_ERR_WORKSPACE
