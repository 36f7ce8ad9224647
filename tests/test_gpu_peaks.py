"""GPU: density-map evaluation on the MI355X (csrc/peaks.hip) -- umi.peaks.peak_lists / density_maps, CrowdMatchingTestPeaks on
device tensors, umi.infer.score_density_maps and predict_density -- against the NumPy statements that tests/test_peaks.py pins to
SciPy.  Lists, counts, padding and fault words compare with ==; the only floats with a bound are the float64 sums."""
import numpy as np
import pytest
import torch

from oracle import recipe
from tests import poison
from tools import gen_golden_binary_infer as GB
from tools import gen_golden_density as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE_H, TILE_W = 16, 64              # PK_TH, PK_TW of csrc/peaks.hip: the candidate and contested passes work on 64 x 16 pixel tiles
SHAPES = [(7, 7), (8, 15), (13, 13), (33, 70), (64, 64), (97, 131), (2 * TILE_H + 1, 2 * TILE_W + 1)]
DISTANCES = (1, 3, 5, 8)
THRESHOLDS = np.arange(0.5, 1, 0.05)
SIGMAS = [5, 20]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: torch.cuda.is_available() is False")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check(maps, d, max_peaks=None, floor=1e-3, want_fault=None, vmin=False):
    """Device lists, counts, (0, 0) padding and the fault word == the statement, on output buffers preset to 0xFF."""
    from umi import peaks as P
    max_peaks = max_peaks or P.MAX_PEAKS
    want_p, want_c, want_f = P.peak_lists_numpy(maps, d, floor, max_peaks)
    x = _dev(maps)
    with poison.poisoned(0xFF):
        kw = {"vmin": P.map_sums(x)[1]} if vmin else {}
        peaks, p_count, fault = P.peak_lists(x, d, floor, max_peaks, _fault=True, **kw)
    assert peaks.dtype == torch.int32 and tuple(peaks.shape) == want_p.shape and p_count.dtype == torch.int32
    assert fault.item() == want_f and want_fault in (None, want_f)
    assert np.array_equal(p_count.cpu().numpy(), want_c), (p_count.cpu().numpy(), want_c)
    assert np.array_equal(peaks.cpu().numpy(), want_p)
    return want_c


def _contents(H, W, seed):
    """Three images of one shape with different content: continuous noise, four-level noise, overlapping plateaus."""
    return np.stack([G.make_map(k, H, W, seed + i) for i, k in enumerate(G.KINDS)])


# ---- 1. peak lists -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DISTANCES)
@pytest.mark.parametrize("shape", SHAPES)
def test_peak_lists_equal_the_statement(shape, d):
    _need_gpu()
    maps = _contents(*shape, seed=100 * shape[0] + shape[1])
    counts = _check(maps, d)                                   # N = 3
    for n in range(3):                                         # N = 1, each kind on its own, once with the caller's minimum
        _check(maps[n], d, vmin=(n == 1))
    if shape[0] > 2 * d and shape[1] > 2 * d and shape[0] * shape[1] > 400:
        assert counts.min() > 0


def _tile_plateaus(H, W):
    """Rectangular plateaus across the tile edges (x = 64, y = 16, 32) and over the tile corner (16, 64) of a 64 x 16 tiling,
    equal heights where they touch so that candidates of one plateau lie in two and in four tiles."""
    m = np.full((H, W), 0.0005, dtype=np.float32)
    m[TILE_H - 3:TILE_H + 4, TILE_W - 5:TILE_W + 6] = 0.5           # over the corner (16, 64): four tiles
    m[2 * TILE_H - 2:2 * TILE_H + 1, 10:40] = 0.75                  # across the row edge y = 32
    m[4:12, TILE_W - 2:TILE_W + 2] = 0.75                           # across the column edge x = 64, inside one tile row
    m[TILE_H - 1:TILE_H + 1, 20:23] = 0.25                          # two rows, one either side of y = 16
    if W > 2 * TILE_W:
        m[20:30, 2 * TILE_W - 1:] = 1.0                             # across x = 128 to the image edge
    return m


@pytest.mark.parametrize("d", DISTANCES)
def test_plateaus_across_tile_edges_and_corners(d):
    _need_gpu()
    for H, W in ((33, 70), (97, 131), (2 * TILE_H + 1, 2 * TILE_W + 1)):
        m = _tile_plateaus(H, W)
        c = _check(np.stack([m, np.flipud(m).copy(), np.flipud(np.fliplr(m)).copy()]), d)
        assert c[0] >= (3 if d <= 3 else 1)
        _check(m, d)


@pytest.mark.parametrize("d", DISTANCES)
def test_longest_dependence_chains(d):
    """A full-width row plateau and a full-image plateau with one lower pixel: every interior pixel is a candidate that waits
    for its raster predecessors, the deepest fixed point the kernel meets (about W + d * H rounds)."""
    _need_gpu()
    for H, W in ((33, 70), (97, 131)):
        row = np.full((H, W), 0.01, dtype=np.float32)
        row[H // 2] = 0.5
        full = np.full((H, W), 0.5, dtype=np.float32)
        full[0, 0] = 0.25
        low_inside = np.full((H, W), 0.5, dtype=np.float32)
        low_inside[H // 2, W // 3] = 0.0
        c = _check(np.stack([row, full, low_inside]), d)
        per_row, rows = len(range(d, W - d, d)), len(range(d, H - d, d))         # (d = 1 at 97 x 131 overflows: also compared)
        assert c[0] == per_row and c[1] == min(rows * per_row, 8192)
    # more contested candidates than one round decides, many times over
    _check(np.full((1, 64, 64), 0.5, dtype=np.float32) - np.eye(64, dtype=np.float32)[None] * 0.25, d)


@pytest.mark.parametrize("d", (1, 3, 5))
def test_edge_cases(d):
    _need_gpu()
    H, W = 4 * d + 5, 4 * d + 7

    def single(*spikes, base=0.0, shape=(H, W)):
        m = np.full(shape, base, dtype=np.float32)
        for y, x, v in spikes:
            m[y, x] = v
        return m
    batch = [np.full((H, W), 0.5, np.float32), np.full((H, W), 0.0005, np.float32),                  # constant, below the floor
             single((d - 1, W // 2, 1.0)), single((d, W // 2, 1.0)), single((H // 2, W - d, 1.0)), single((H - d - 1, W // 2, 1.0)),
             single((2 * d, 2 * d, 1.0), (2 * d, 3 * d - 1, 1.0)), single((2 * d, 2 * d, 1.0), (2 * d, 3 * d, 1.0)),
             single((2 * d, 2 * d, 1.0), (3 * d - 1, d + 1, 1.0)), single((2 * d, 2 * d, 1.0), (3 * d, d, 1.0)),
             single((d, d + 2, np.nan), (2 * d, 2 * d, np.inf), (3 * d + 1, 3 * d + 2, 0.5)), np.full((H, W), np.nan, np.float32),
             single((2 * d, 2 * d, 1e-3), (3 * d + 1, 3 * d + 2, np.nextafter(np.float32(1e-3), np.float32(0)))),   # at the floor, just below
             single((2 * d, 2 * d, 3.0), base=2.0)]                                                  # nothing below the floor
    c = _check(np.stack(batch), d)
    assert c.tolist()[:6] == [0, 0, 0, 1, 0, 1] and c[10] == 2 and c[11] == 0 and c[12] == 1 and c[13] == 1
    for shape in ((2 * d, 30), (30, 2 * d), (2 * d + 1, 2 * d + 1)):                                 # H or W <= 2d: nothing
        m = np.random.default_rng(d).random(shape).astype(np.float32)
        m[d, d] = 2.0                                                                                # the only pixel inside, if any
        assert _check(m, d).tolist() == [0 if min(shape) <= 2 * d else 1]
    _check(np.stack(batch), d, floor=0.0)                                                            # -0 / 0 at a zero floor
    neg = np.random.default_rng(5).standard_normal((2, 40, 41)).astype(np.float32)                   # negative values
    neg[1, 3, 4] = -0.0
    _check(neg, d)
    _check(neg, d, floor=0.0, vmin=True)


def test_overflow_at_four_and_at_the_kernel_limit():
    _need_gpu()
    from umi import peaks as P
    rng = np.random.default_rng(9)
    m = rng.random((3, 40, 50)).astype(np.float32)
    m[2] = 0
    assert _check(m, 3, max_peaks=4, want_fault=P.FAULT_OVERFLOW).tolist() == [4, 4, 0]
    lv = np.stack([G.make_map("levels", 40, 50, 3), G.make_map("plateaus", 40, 50, 4)])              # cut inside runs of equal values
    _check(lv, 1, max_peaks=4, want_fault=P.FAULT_OVERFLOW)
    _check(lv, 1, max_peaks=37, want_fault=P.FAULT_OVERFLOW)
    for d, side in ((3, 300), (1, 200)):                        # a lattice of unit spikes of spacing d: 9604 and 19602 peaks
        lat = np.zeros((2, side, side), dtype=np.float32)
        lat[0, d:side - d:d, d:side - d:max(d, 2)] = 1.0
        lat[1, 50, 50] = 1.0
        want = len(range(d, side - d, d)) * len(range(d, side - d, max(d, 2)))
        assert want > P.MAX_PEAKS
        assert _check(lat, d, want_fault=P.FAULT_OVERFLOW).tolist() == [P.MAX_PEAKS, 1]
        with pytest.raises(RuntimeError, match="max_peaks"):
            P.peak_lists(_dev(lat), d, check=True)
    exact = np.zeros((1, 300, 300), dtype=np.float32)           # exactly 8192 peaks: no fault
    ys, xs = np.divmod(np.arange(P.MAX_PEAKS), 98)
    exact[0, 3 + 3 * ys, 3 + 3 * xs] = 1.0
    assert _check(exact, 3).tolist() == [P.MAX_PEAKS]


def test_non_contiguous_input_and_bad_arguments():
    _need_gpu()
    from umi import peaks as P
    base = np.random.default_rng(2).random((2, 60, 90)).astype(np.float32)
    x = _dev(base)
    for view, want in ((x[:, ::2, 1::2], base[:, ::2, 1::2]), (x.transpose(1, 2), base.transpose(0, 2, 1)), (x[1, 5:50, 7:], base[1, 5:50, 7:])):
        assert not view.is_contiguous()
        peaks, p_count = P.peak_lists(view, 3, check=True)
        wp, wc, _ = P.peak_lists_numpy(np.ascontiguousarray(want), 3)
        assert np.array_equal(peaks.cpu().numpy(), wp) and np.array_equal(p_count.cpu().numpy(), wc)
    for bad in (dict(min_distance=0), dict(min_distance=9), dict(floor=-1.0), dict(max_peaks=0), dict(max_peaks=P.MAX_PEAKS + 1)):
        with pytest.raises(ValueError):
            P.peak_lists(x, **bad)
    with pytest.raises(ValueError):
        P.peak_lists(x.double())
    with pytest.raises(ValueError):
        P.peak_lists(x, vmin=torch.zeros(5, device=DEV))


def test_two_runs_give_the_same_lists():
    _need_gpu()
    from umi import peaks as P
    x = _dev(np.stack([G.make_map("levels", 97, 131, s) for s in range(4)]))
    a = [t.clone() for t in P.peak_lists(x, 3)]
    for _ in range(3):
        b = P.peak_lists(x, 3)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 2. density maps -----------------------------------------------------------------------------------------------------------
def _sum_bound(pred):
    """n * 2^-53 * sum|x| per image: the project's bar for a fixed-order float64 sum against np.sum(dtype=float64)."""
    p = pred.reshape(pred.shape[0], -1).astype(np.float64)
    return p.shape[1] * 2.0 ** -53 * np.abs(p).sum(axis=1)


def test_density_maps_values_and_counts():
    _need_gpu()
    from umi import peaks as P
    rng = np.random.default_rng(11)
    for shape in ((1, 7, 7), (3, 33, 70), (2, 97, 131), (2, 64, 64), (1, 130, 4097 // 17)):
        x = (rng.standard_normal(shape) * 50).astype(np.float32)
        x[0, 1, 2], x[-1, 3, 3], x[0, 0, 0] = np.nan, np.inf, -0.0
        with poison.poisoned(0xFF):
            pred, counts, vmin = P.density_maps(_dev(x), _vmin=True)
        want = np.maximum(x, 0).astype(np.float32) / np.float32(200)
        got = pred.cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).sum() == 1
        assert np.array_equal(np.nan_to_num(got, nan=-1.0), np.nan_to_num(want, nan=-1.0))       # values; the sign of zero is not pinned
        assert np.isnan(counts[0].item()) and (shape[0] == 1 or counts[-1].item() == np.inf)
        assert vmin.cpu().tolist() == [0.0] * shape[0]
        # the same maps without the NaN / inf pixels: the sum within the bound, the statement's pair as the wrapper returns it
        x = np.nan_to_num(x, nan=1.0, posinf=2.0)
        pred, counts = P.density_maps(_dev(x))
        want_pred, want_counts = P.density_maps_numpy(x)
        assert np.array_equal(pred.cpu().numpy(), want_pred)
        err = np.abs(counts.cpu().numpy() - want_counts)
        print("density counts", shape, "err", err, "bound", _sum_bound(want_pred))
        assert (err <= _sum_bound(want_pred)).all()
    # values that are multiples of 2^-10 below 1: every partial sum is exact, so the fixed order must give == (see the bound on the
    # bits: pred < 2^-7 with ulp >= 2^-41, at most 2^13 of them)
    x = (rng.integers(0, 1024, size=(3, 61, 130)) / 1024).astype(np.float32)
    x[1] = -x[1]
    pred, counts = P.density_maps(_dev(x))
    want_pred, want_counts = P.density_maps_numpy(x)
    assert np.array_equal(pred.cpu().numpy(), want_pred) and np.array_equal(counts.cpu().numpy(), want_counts) and want_counts[1] == 0
    # other scales divide, too; a 2-D map gives a 2-D map
    for scale in (1.0, 3.0, 768.0):
        pred, counts = P.density_maps(_dev(x[0]), scale)
        assert tuple(pred.shape) == (61, 130) and np.array_equal(pred.cpu().numpy(), P.density_maps_numpy(x[0], scale)[0][0])
    with pytest.raises(ValueError):
        P.density_maps(_dev(x), 0.0)


# ---- 3. scoring ------------------------------------------------------------------------------------------------------------------
def _scene(seed, H=96, W=128, n=40):
    """A density map of Gaussian bumps (sigma 2) and a dot map with most of the bumps' centres, some a pixel or two off."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:H, :W].astype(np.float64)
    m = np.zeros((H, W))
    g = np.zeros((H, W), dtype=np.uint8)
    for k in range(n):
        cy, cx = float(rng.uniform(4, H - 4)), float(rng.uniform(4, W - 4))
        m += rng.uniform(0.6, 1.4) / (2 * np.pi * 4) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / 8)
        if k % 5:
            g[int(np.clip(round(cy) + rng.integers(-2, 3), 0, H - 1)), int(np.clip(round(cx) + rng.integers(-2, 3), 0, W - 1))] = 1
    return m.astype(np.float32), g


def _cells_clear_of_integers(pred, size):
    """The host statement alone: no level-1..3 cell sum of these maps lies within the summation bound of a non-zero integer, so
    int() in GMAE gives the same integer for any float64 sum within the bound (int() truncates toward zero, so nothing flips
    around 0)."""
    from umi import matching as M
    cells = M.grid_sums_numpy(pred, size)
    bound = _sum_bound(pred).max()
    for L in (1, 2, 3):
        s = M.level_sums(cells, L)
        if not ((np.abs(s - np.round(s)) > 4 * bound) | (np.round(s) == 0)).all():
            return False
    return True


def _compare_scores(got, want, pred_bound):
    import CrowdMatching as CM
    assert got.keys() == want.keys()
    for k in ("GT", "peaks", "G1", "G2", "G3"):
        assert got[k] == want[k], k
    for k in ("arr_prec", "arr_recall", "arr_f1"):
        assert got[k].dtype == np.float64 and np.array_equal(got[k], want[k]), k
    assert abs(got["Pred"] - want["Pred"]) <= pred_bound
    # carried through countAccuracyMetric: the metrics are those of the device's own sum, bit for bit
    assert (got["AbsDiff"], got["Accuracy"], got["AccuracyRelative"], got["AccuracyRelativePD"]) == CM.countAccuracyMetric(got["GT"], got["Pred"])
    assert abs(got["AbsDiff"] - want["AbsDiff"]) <= pred_bound
    for k in ("Accuracy", "AccuracyRelative", "AccuracyRelativePD"):
        assert abs(got[k] - want[k]) <= 1e-4 + 1e-12, k                 # rounded to four places: at most one step apart


@pytest.mark.parametrize("gt_dtype", [np.uint8, np.float32])
def test_score_density_maps_equals_the_statement(gt_dtype):
    _need_gpu()
    from umi import infer
    from umi import peaks as P
    scenes = [_scene(s) for s in (1, 2, 3)]
    pred = np.stack([s[0] for s in scenes])
    gt = np.stack([s[1] for s in scenes]).astype(gt_dtype)
    pred[2] *= 0                                                      # an image without peaks, with dots
    size = 128
    assert _cells_clear_of_integers(pred, size)
    want = P.score_density_numpy(pred, gt, SIGMAS, THRESHOLDS, size=size)
    got = infer.score_density_maps(_dev(pred), _dev(gt), SIGMAS, THRESHOLDS, size=size)
    assert len(got) == 3 and 20 < want[0]["peaks"] <= 40 and want[2]["peaks"] == 0 and 0 < want[0]["arr_f1"][0, 0] < 1
    bounds = _sum_bound(pred)
    for n in range(3):
        print("score", n, "Pred", got[n]["Pred"], want[n]["Pred"], "bound", bounds[n])
        _compare_scores(got[n], want[n], bounds[n])
    # a pair of heads
    pw = P.score_density_numpy((pred[:2], pred[1:]), (gt[:2], gt[1:]), SIGMAS, THRESHOLDS, size=size)
    pg = infer.score_density_maps((_dev(pred[:2]), _dev(pred[1:])), (_dev(gt[:2]), _dev(gt[1:])), SIGMAS, THRESHOLDS, size=size)
    for n in range(2):
        for h in (0, 1):
            _compare_scores(pg[n][h], pw[n][h], bounds[n + h])
        assert pg[n]["ratio"].keys() == pw[n]["ratio"].keys() and pg[n]["ratio"]["GT"] == pw[n]["ratio"]["GT"]
        assert abs(pg[n]["ratio"]["Pred"] - pw[n]["ratio"]["Pred"]) <= 1e-12
    # the drop-in function on device tensors: the same integers, so the same floats
    import CrowdMatching as CM
    for a, b in zip(CM.CrowdMatchingTestPeaks(_dev(gt[0]), _dev(pred[0]), SIGMAS, THRESHOLDS), (want[0]["arr_prec"], want[0]["arr_recall"], want[0]["arr_f1"])):
        assert np.array_equal(a, b)


def test_score_density_maps_raises_on_a_fault_word():
    _need_gpu()
    from umi import infer
    lat = np.zeros((1, 300, 300), dtype=np.float32)
    lat[0, 3:297:3, 3:297:3] = 1.0
    g = np.zeros((1, 300, 300), dtype=np.uint8)
    with pytest.raises(RuntimeError, match="max_peaks"):
        infer.score_density_maps(_dev(lat), _dev(g), SIGMAS, THRESHOLDS)


# ---- 4. predict_density ------------------------------------------------------------------------------------------------------------
def _model(two_heads, seed):
    import Model
    m = (Model.UNet_multitask if two_heads else Model.UNet)(1, 1, 8, False, compute_dtype="fp32")
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=seed))
    return m.to(DEV)


def _want_density(out, out_hw):
    r = torch.relu(out.cpu())[:, 0].numpy()
    if out_hw is not None:
        r = GB.zoom_nearest_numpy(r, out_hw)
    return r.astype(np.float32) / np.float32(200)


@pytest.mark.parametrize("two_heads", [False, True])
def test_predict_density_equals_relu_zoom_and_division(two_heads):
    _need_gpu()
    from umi import infer
    m = _model(two_heads, 41 + two_heads)
    m.train()
    x = torch.randn((2, 1, 32, 32), generator=torch.Generator().manual_seed(3)).to(DEV)
    got = infer.predict_density(m, x)
    assert m.training
    m.eval()
    with torch.no_grad():
        outs = m(x)
    outs = outs if two_heads else (outs,)
    assert isinstance(got, tuple) == two_heads
    for g, o in zip(got if two_heads else (got,), outs):
        want = _want_density(o, None)
        assert 0 < (want > 0).mean() < 1, "degenerate test: the rectified output is constant"
        assert g.dtype == torch.float32 and tuple(g.shape) == (2, 32, 32) and np.array_equal(g.cpu().numpy(), want)
    got = infer.predict_density(m, x, out_hw=(48, 40))
    for g, o in zip(got if two_heads else (got,), outs):
        assert tuple(g.shape) == (2, 48, 40) and np.array_equal(g.cpu().numpy(), _want_density(o, (48, 40)))
    # a callable composes: here the eval-mode model behind a lambda
    got = infer.predict_density(lambda v: m(v), x, out_hw=(48, 40), scale=100.0)
    for g, o in zip(got if two_heads else (got,), outs):
        assert np.array_equal(g.cpu().numpy(), _want_density(o, (48, 40)) * np.float32(2))
    # replayed from a HIP graph
    predict = infer.GraphedPredictor(m, x, density=True, out_hw=(48, 40))
    for xs in (x, torch.randn((2, 1, 32, 32), generator=torch.Generator().manual_seed(4)).to(DEV)):
        with torch.no_grad():
            outs = m(xs)
        outs = outs if two_heads else (outs,)
        got = predict(xs)
        for g, o in zip(got if two_heads else (got,), outs):
            assert np.array_equal(g.cpu().numpy(), _want_density(o, (48, 40)))
