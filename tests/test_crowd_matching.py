"""CPU: the NumPy statements of the localisation scoring (umi/matching.py) and the drop-in functions (CrowdMatching.py)
against what the reference's own CrowdMatching.py returned on the seeded cases of tools/gen_golden_crowd_matching.py
(tests/golden/crowd_matching.npz).  Every comparison is exact: float64 arrays with np.array_equal, tuples with ==."""
import math
import os

import numpy as np
import pytest

from tools import gen_golden_crowd_matching as G

CASES = list(G.CASES)


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "crowd_matching.npz"))


def test_fixture_lists_the_generator_cases(fixture):
    assert list(fixture["case_names"]) == CASES and list(fixture["gmae_names"]) == list(G.GMAE_CASES)
    assert np.array_equal(fixture["thresholds"], np.array(G.THRESHOLDS)) and fixture["sigmas"].tolist() == G.SIGMAS
    assert fixture["dist_thresholds"].tolist() == G.DIST_THRESHOLDS
    for name in CASES:
        g, x, y = G.case(name)
        assert fixture[f"cm_{name}_sizes"].tolist() == [g.shape[0], g.shape[1], int(g.sum()), x.size]


# ---- 1. the reference's recorded results -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_crowd_matching_equals_the_reference(fixture, name):
    import CrowdMatching as CM
    from umi import matching as M
    g, x, y = G.case(name)
    want = tuple(fixture[f"cm_{name}_{k}"] for k in ("prec", "recall", "f1"))
    got = CM.CrowdMatchingTest(g, (x, y), G.SIGMAS, G.THRESHOLDS, inputType='Coordinates')
    for a, b in zip(got, want):
        assert a.dtype == np.float64 and np.array_equal(a, b)
    # the batched statement on the lists, through the generic entry
    dots, g_count = M.dot_lists(g)
    centers = np.zeros((1, max(x.size, 1), 2), dtype=np.int32)
    centers[0, :x.size, 0], centers[0, :x.size, 1] = x, y
    res = M.crowd_match(dots, g_count, centers, np.array([x.size], dtype=np.int32), G.SIGMAS, G.THRESHOLDS)
    assert res.shape == (1, 2, 10, 2) and res.dtype == np.int32
    for a, b in zip(CM.precision_recall_f1(res[0], int(g_count[0]), x.size), want):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", CASES)
def test_distance_matching_equals_the_reference(fixture, name):
    import CrowdMatching as CM
    g, x, y = G.case(name)
    for k, th in enumerate(G.DIST_THRESHOLDS):
        want = fixture[f"dm_{name}_{k}"]
        if np.isnan(want).all():
            with pytest.raises(ZeroDivisionError):
                CM.CrowdMatchingTest2(g, (x, y), th)
            continue
        got = CM.CrowdMatchingTest2(g, (x, y), th)
        assert got == tuple(want.tolist()), (name, th)


@pytest.mark.parametrize("name", list(G.GMAE_CASES))
def test_gmae_equals_the_reference(fixture, name):
    import CrowdMatching as CM
    gt, pred = G.gmae_case(name)
    for row, L in zip(fixture[name], (1, 2, 3)):
        got = CM.GMAE(L, gt, pred)
        assert isinstance(got, list) and got == row.tolist()
        assert CM.GMAE(L, gt.astype(np.uint8), pred.astype(np.float32)) == row.tolist()


def test_gmae_size_keyword_and_levels():
    import CrowdMatching as CM
    from umi import matching as M
    gt, pred = G.gmae_case("gmae_600x520")
    for L in (0, 1, 2, 3):
        cs = 768 // 2 ** L
        want = [0, 0, 0]
        for i in range(0, 768, cs):
            for j in range(0, 768, cs):
                d = CM.countAccuracyMetric(int(gt[i:i + cs, j:j + cs].sum()), int(pred[i:i + cs, j:j + cs].sum()))
                want = [want[0] + d[0], want[1] + d[2], want[2] + d[3]]
        assert CM.GMAE(L, gt, pred, size=768) == want
    with pytest.raises(ValueError):
        CM.GMAE(4, gt, pred)
    cells = M.grid_sums(gt.astype(np.uint8), 512)
    assert cells.dtype == np.int64 and cells.shape == (1, 8, 8) and cells.sum() == gt[:512, :512].sum()
    assert np.array_equal(M.level_sums(cells, 1)[0], [[gt[:256, :256].sum(), gt[:256, 256:512].sum()],
                                                      [gt[256:512, :256].sum(), gt[256:512, 256:512].sum()]])


def test_count_accuracy_metric():
    import CrowdMatching as CM
    assert CM.countAccuracyMetric(10, 7) == (3, round(3 / (10 + 1e-6), 4), round(3 / (10 + 1e-6), 4), round(6 / (17 + 1e-6), 4))
    assert CM.countAccuracyMetric(0, 0) == (0, 0.0, 0.0, 0.0)
    assert CM.countAccuracyMetric(0, 2) == (2, round(2 / 1e-6, 4), round(2 / (2 + 1e-6), 4), round(4 / (2 + 1e-6), 4))


# ---- 2. corner cases ---------------------------------------------------------------------------------------------------------
def test_corner_cases():
    import CrowdMatching as CM
    none = np.zeros(0, dtype=np.int64)
    empty, one = np.zeros((32, 32)), np.zeros((32, 32))
    one[5, 7] = 1
    S, T = [5, 20], [0.5, 0.9]
    p, r, f = CM.CrowdMatchingTest(empty, (none, none), S, T, inputType='Coordinates')
    assert all(np.array_equal(a, np.ones((2, 2))) for a in (p, r, f))
    p, r, f = CM.CrowdMatchingTest(empty, (np.array([3]), np.array([4])), S, T, inputType='Coordinates')
    assert np.array_equal(r, np.ones((2, 2))) and np.array_equal(p, np.zeros((2, 2))) and np.array_equal(f, np.zeros((2, 2)))
    # three centres on one dot: one match, fn = 1 - 1 = 0; a fourth far away
    p, r, f = CM.CrowdMatchingTest(one, (np.array([7, 7, 7, 30]), np.array([5, 5, 5, 30])), [1], [0.5], inputType='Coordinates')
    assert p[0, 0] == 1 / (1 + 3 + 1e-7) and r[0, 0] == 1.0
    # fn is clamped at 0 (cannot go negative here, but the expression is the reference's)
    p, r, f = CM.precision_recall_f1(np.array([[[3, 0]]]), 2, 3)
    assert r[0, 0] == 1.0 and p[0, 0] == 3 / (3 + 1e-7)
    assert CM.CrowdMatchingTest2(one, (none, none), 10) == (0, 0, 0)
    assert CM.CrowdMatchingTest2(empty, (none, none), 10) == (0, 0, 0)
    with pytest.raises(ZeroDivisionError):
        CM.CrowdMatchingTest2(empty, (np.array([3]), np.array([4])), 10)
    with pytest.raises(NotImplementedError, match="cv2"):
        CM.CrowdMatchingTest(one, one.astype(np.uint8), S, T)                       # the reference's default inputType
    with pytest.raises(NotImplementedError, match="cv2"):
        CM.CrowdMatchingTest(one, one.astype(np.uint8), S, T, inputType='Segmentation')
    with pytest.raises(NotImplementedError, match="skimage"):
        CM.CrowdMatchingTest(one, one, S, T, inputType='Regression')
    with pytest.raises(ValueError):
        CM.CrowdMatchingTest(one * 2, (none, none), S, T, inputType='Coordinates')   # not 0 / 1 valued
    with pytest.raises(ValueError):
        CM.CrowdMatchingTest(one, (np.array([32]), np.array([0])), S, T, inputType='Coordinates')   # outside the image
    with pytest.raises(ValueError):
        CM.CrowdMatchingTest(one, (np.array([0]), np.array([-1])), S, T, inputType='Coordinates')
    with pytest.raises(ValueError):
        CM.CrowdMatchingTest(one, (none, none), S, [0.0], inputType='Coordinates')


# ---- 3. the host table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", [5, 20])
def test_gauss_table_is_the_direct_evaluation(sigma):
    from umi import matching as M
    r, tab = M.gauss_table(sigma)
    assert r == 4 * sigma and tab.shape == (2 * r + 1, 2 * r + 1) and tab.dtype == np.float64
    h = np.empty_like(tab)
    for i in range(2 * r + 1):
        for j in range(2 * r + 1):
            x, y = float(j - r), float(i - r)
            h[i, j] = np.exp(-(x * x + y * y) / (2. * sigma * sigma))
    eps = np.finfo(np.float64).eps
    zeroed = h < eps * h.max()
    h[zeroed] = 0
    h /= h.sum()
    assert np.array_equal(tab, h / h.max())
    assert tab[r, r] == 1.0 and tab.max() == 1.0
    assert np.array_equal(tab == 0, zeroed) and np.array_equal(tab, tab.T) and np.array_equal(tab, tab[::-1, ::-1])


def test_gauss_table_zeroes_its_tail():
    from umi import matching as M
    # With r = int(round(4 * sigma)) the corner term is about exp(-16), far above eps, so sigma 5 and 20 zero nothing.  A radius
    # that was rounded UP reaches further: sigma = 0.13 -> r = 1, edge exp(-1 / 0.0338) = 1.4e-13 stays, corner
    # exp(-2 / 0.0338) = 2e-26 < eps * max is zeroed.
    r, tab = M.gauss_table(0.13)
    assert r == 1 and tab[1, 1] == 1.0 and 0 < tab[0, 1] < 1e-12
    assert tab[0, 0] == 0 and tab[0, 2] == 0 and tab[2, 0] == 0 and tab[2, 2] == 0 and np.count_nonzero(tab) == 5
    r, tab = M.gauss_table(0.62)          # r = 2: corner exp(-8 / 0.7688) = 3e-5
    assert r == 2 and np.count_nonzero(tab) == 25
    r, tab = M.gauss_table(0.1249)        # int(round(0.4996)) = 0: the 1 x 1 table
    assert r == 0 and tab.tolist() == [[1.0]]


# ---- 4. the squared-distance limit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thresh", [1, 2.5, 10, 10.000001])
def test_d2_limit_against_a_scan(thresh):
    from umi import matching as M
    below = [d2 for d2 in range(0, 2000) if np.sqrt(np.float64(d2)) < thresh]
    assert M.d2_limit(thresh) == max(below) and below == list(range(len(below)))
    assert {1: 0, 2.5: 6, 10: 99, 10.000001: 100}[thresh] == M.d2_limit(thresh)


def test_d2_limit_edges():
    from umi import matching as M
    assert M.d2_limit(0) == -1 and M.d2_limit(-3) == -1 and M.d2_limit(1e-9) == 0
    assert M.d2_limit(float("inf")) == 2 ** 62
    for t in (3.0, 1e3, 12345.678, 2.0 ** 20):
        k = M.d2_limit(t)
        assert math.sqrt(k) < t <= math.sqrt(k + 1)


# ---- 5. centre rounding ------------------------------------------------------------------------------------------------------
def test_center_rounding_is_pythons_round_exhaustively():
    from umi import matching as M
    for area in range(1, 65):
        s = np.arange(0, 64 * 767 + 1, dtype=np.int64)
        got = M.round_div_half_even(s, area)
        want = np.array([round(int(v) / area) for v in s], dtype=np.int64)
        assert np.array_equal(got, want), area


def test_component_centers_numpy_on_label_statistics():
    from umi import components as C
    from umi import matching as M
    rng = np.random.default_rng(3)
    m = (rng.random((2, 40, 56)) < 0.3).astype(np.uint8)
    m[1] = 0
    stats = [C.label_components_numpy(m[n]) for n in range(2)]
    counts = np.array([int(np.asarray(s[1]).reshape(-1)[0]) for s in stats], dtype=np.int32)
    area = np.stack([np.asarray(s[2]).reshape(-1) for s in stats])
    sum_y = np.stack([np.asarray(s[3]).reshape(-1) for s in stats])
    sum_x = np.stack([np.asarray(s[4]).reshape(-1) for s in stats])
    cen = M.component_centers(counts, area, sum_y, sum_x)
    assert cen.shape == (2, area.shape[1], 2) and cen.dtype == np.int32 and counts[0] > 3 and counts[1] == 0
    for c in range(counts[0]):
        assert cen[0, c].tolist() == [round(int(sum_x[0, c]) / int(area[0, c])), round(int(sum_y[0, c]) / int(area[0, c]))]
    assert not cen[0, counts[0]:].any() and not cen[1].any()


# ---- the lists themselves ----------------------------------------------------------------------------------------------------
def test_dot_lists_numpy_raster_order_and_overflow():
    from umi import matching as M
    g, _, _ = G.case("random_96x130")
    dots, cnt = M.dot_lists(np.stack([g, np.zeros_like(g)]).astype(np.float32))
    ys, xs = np.nonzero(g)
    assert dots.shape == (2, M.MAX_DOTS, 2) and cnt.tolist() == [ys.size, 0]
    assert np.array_equal(dots[0, :ys.size, 0], xs) and np.array_equal(dots[0, :ys.size, 1], ys) and not dots[0, ys.size:].any()
    with pytest.raises(RuntimeError, match="max_dots"):
        M.dot_lists_numpy(g, max_dots=ys.size - 1)


def test_scatter_counts_coinciding_centres_once():
    from umi import matching as M
    cen = np.array([[[3, 4], [3, 4], [9, 0], [50, 1], [1, -1], [7, 7]]], dtype=np.int32)
    m = M.scatter_centers(cen, np.array([5], dtype=np.int32), 8, 10)
    assert m.dtype == np.uint8 and m.sum() == 2 and m[0, 4, 3] == 1 and m[0, 0, 9] == 1


def test_max_dots_is_the_librarys():
    from umi import lib
    from umi import matching as M
    assert lib.fn("umi_match_max_dots")() == M.MAX_DOTS
    # argument checks happen before any launch
    assert lib.fn("umi_dot_lists")(None, 0, None, None, 1, 8, 8, 16, None, 0, None) == -1
    assert lib.fn("umi_crowd_match")(None, None, 1, None, None, 1, None, 0, None, 1, None, 1, None, 1, None) == -1
    assert lib.fn("umi_distance_match")(None, None, 1, None, None, 1, 0, None, 1, None, 0, None) == -1
    assert lib.fn("umi_grid_sums")(None, 0, None, 1, 8, 8, 512, None) == -1
    assert lib.fn("umi_component_centers")(None, None, None, None, None, 1, 1, None) == -1
    assert lib.fn("umi_scatter_centers")(None, None, 1, None, 1, 8, 8, None) == -1
