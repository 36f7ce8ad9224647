"""GPU: the localisation scoring kernels (csrc/matching.hip) on the MI355X -- umi.matching.dot_lists / component_centers /
crowd_match / distance_match / grid_sums / scatter_centers, the drop-in CrowdMatching functions on device tensors and
umi.infer.score_binary_masks -- against the NumPy statements the CPU suite pins to the reference and against the reference's
recorded results (tests/golden/crowd_matching.npz).  Every comparison is exact."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tools import gen_golden_binary_infer as GB
from tools import gen_golden_crowd_matching as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = list(G.CASES)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: torch.cuda.is_available() is False")


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "crowd_matching.npz"))


def _batch_lists(names, cap=None):
    """All cases' lists in one batch: unequal dot and centre counts per image."""
    from umi import matching as M
    cases = [G.case(n) for n in names]
    cap = cap or max(1, max(c[1].size for c in cases))
    dots = np.zeros((len(names), M.MAX_DOTS, 2), dtype=np.int32)
    centers = np.zeros((len(names), cap, 2), dtype=np.int32)
    g_count, c_count = np.zeros(len(names), dtype=np.int32), np.zeros(len(names), dtype=np.int32)
    for n, (g, x, y) in enumerate(cases):
        d, k = M.dot_lists_numpy(g)
        dots[n], g_count[n], c_count[n] = d[0], k[0], x.size
        centers[n, :x.size, 0], centers[n, :x.size, 1] = x, y
    return dots, g_count, centers, c_count


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


# ---- 1. dot compaction -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_dot_lists_equal_nonzero_order(dtype):
    _need_gpu()
    from umi import matching as M
    rng = np.random.default_rng(1)
    for shape, density in (((3, 64, 64), 0.05), ((2, 96, 130), 0.02), ((4, 512, 512), 0.002), ((1, 768, 768), 0.004), ((2, 7, 5), 0.4)):
        m = (rng.random(shape) < density).astype(dtype)
        if dtype == np.float32:
            m *= rng.choice(np.array([1.0, 0.25, -3.0, 1e-30], dtype=np.float32), size=shape)      # any non-zero value is a dot
        if shape[0] > 1:
            m[-1] = 0                                                                               # an empty image in the batch
        dots, cnt = M.dot_lists(torch.from_numpy(m).to(DEV), check=True)
        want_d, want_c = M.dot_lists_numpy(m)
        assert dots.dtype == torch.int32 and tuple(dots.shape) == (shape[0], M.MAX_DOTS, 2)
        assert np.array_equal(cnt.cpu().numpy(), want_c) and want_c[0] > 0 and (shape[0] == 1 or want_c[-1] == 0)
        assert np.array_equal(dots.cpu().numpy(), want_d), shape
    full = np.ones((64, 64), dtype=dtype)                                                            # 4096 dots, a 2-D map
    dots, cnt = M.dot_lists(torch.from_numpy(full).to(DEV), check=True)
    ys, xs = np.nonzero(full)
    assert cnt.tolist() == [4096] and np.array_equal(dots[0, :4096].cpu().numpy(), np.stack([xs, ys], 1))


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_dot_lists_overflow_sets_the_fault_word_and_stays_in_bounds(dtype):
    _need_gpu()
    from umi import lib as L
    from umi import matching as M
    max_dots, N, H, W, guard = 16, 3, 40, 33, 64
    rng = np.random.default_rng(2)
    m = np.zeros((N, H * W), dtype=dtype)
    m[0, rng.choice(H * W, max_dots + 1, replace=False)] = 1            # one too many
    m[1, rng.choice(H * W, max_dots, replace=False)] = 1                # exactly full
    m[2, rng.choice(H * W, 400, replace=False)] = 1                     # far too many
    m = m.reshape(N, H, W)
    md = torch.from_numpy(m).to(DEV)
    sentinel = -123456789
    buf = torch.full((N * max_dots * 2 + guard,), sentinel, dtype=torch.int32, device=DEV)
    cnt = torch.full((N + guard,), sentinel, dtype=torch.int32, device=DEV)
    nbytes = L.fn("umi_dot_lists_ws_bytes")(N, H, W)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    st = L.fn("umi_dot_lists")(md.data_ptr(), 0 if dtype == np.uint8 else 1, buf.data_ptr(), cnt.data_ptr(), N, H, W, max_dots,
                               ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    assert ws[:4].view(torch.int32).item() == 1
    assert cnt[:N].tolist() == [max_dots] * 3 and (cnt[N:] == sentinel).all()
    assert (buf[N * max_dots * 2:] == sentinel).all()                   # nothing past the buffer
    got = buf[:N * max_dots * 2].view(N, max_dots, 2).cpu().numpy()
    for n in range(N):                                                  # each row: the image's FIRST max_dots dots, nothing of a neighbour
        ys, xs = np.nonzero(m[n])
        assert np.array_equal(got[n], np.stack([xs, ys], 1)[:max_dots]), n
    with pytest.raises(RuntimeError, match="max_dots"):
        M.dot_lists(md, max_dots=max_dots, check=True)
    dots, g_count, fault = M.dot_lists(md[1:2], max_dots=max_dots, _fault=True)       # exactly full is no fault
    assert fault.item() == 0 and g_count.tolist() == [max_dots]
    assert L.fn("umi_dot_lists")(md.data_ptr(), 0, buf.data_ptr(), cnt.data_ptr(), N, H, W, M.MAX_DOTS + 1, ws.data_ptr(), nbytes,
                                 None) == -2
    assert L.fn("umi_dot_lists")(md.data_ptr(), 0, buf.data_ptr(), cnt.data_ptr(), N, H, W, max_dots, ws.data_ptr(), nbytes - 1,
                                 None) == -3


# ---- 2. Gaussian matching ----------------------------------------------------------------------------------------------------
def test_crowd_match_equals_the_numpy_statement_on_every_case_in_one_batch():
    _need_gpu()
    from umi import matching as M
    host = _batch_lists(CASES)
    got = M.crowd_match(*_dev(*host), G.SIGMAS, G.THRESHOLDS)
    want = M.crowd_match_numpy(*host, G.SIGMAS, G.THRESHOLDS)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(CASES), 2, 10, 2)
    assert np.array_equal(got.cpu().numpy(), want)
    assert len(set(host[1].tolist())) > 5 and len(set(host[3].tolist())) > 5 and want[..., 0].max() > 300


@pytest.mark.parametrize("name", CASES)
def test_crowd_matching_test_on_device_tensors_equals_the_reference(fixture, name):
    _need_gpu()
    import CrowdMatching as CM
    g, x, y = G.case(name)
    for gd in (torch.from_numpy(g.astype(np.float32)).to(DEV), torch.from_numpy(g.astype(np.uint8)).to(DEV)):
        got = CM.CrowdMatchingTest(gd, tuple(_dev(x, y)), G.SIGMAS, G.THRESHOLDS, inputType='Coordinates')
        for a, k in zip(got, ("prec", "recall", "f1")):
            assert isinstance(a, np.ndarray) and a.dtype == np.float64 and np.array_equal(a, fixture[f"cm_{name}_{k}"]), k


def test_crowd_match_with_centres_far_outside_the_image_and_many_dots():
    _need_gpu()
    from umi import matching as M
    rng = np.random.default_rng(5)
    g = (rng.random((2, 200, 300)) < 0.128).astype(np.uint8)            # ~7700 dots per image: 31 of a thread's 32 bits in use
    dots, cnt = M.dot_lists_numpy(g)
    assert 7424 < cnt.min() and cnt.max() <= M.MAX_DOTS
    centers = np.stack([rng.integers(-50, 350, (2, 900)), rng.integers(-50, 250, (2, 900))], axis=2).astype(np.int32)
    centers[0, :6] = [[-2 ** 31, 5], [2 ** 31 - 1, 2 ** 31 - 1], [5, -2 ** 31], [-1, -1], [300, 200], [65536 + 3, 4]]
    c_count = np.array([900, 333], dtype=np.int32)
    got = M.crowd_match(*_dev(dots, cnt, centers, c_count), [1.5, 5], [0.3, 0.9])
    assert np.array_equal(got.cpu().numpy(), M.crowd_match_numpy(dots, cnt, centers, c_count, [1.5, 5], [0.3, 0.9]))


# ---- 3. distance matching and grid sums --------------------------------------------------------------------------------------
@pytest.mark.parametrize("thresh", G.DIST_THRESHOLDS)
def test_distance_match_equals_the_numpy_statement_on_every_case_in_one_batch(thresh):
    _need_gpu()
    from umi import matching as M
    host = _batch_lists(CASES)
    got = M.distance_match(*_dev(*host), thresh)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), M.distance_match_numpy(*host, thresh))


@pytest.mark.parametrize("name", CASES)
def test_crowd_matching_test2_on_device_tensors_equals_the_reference(fixture, name):
    _need_gpu()
    import CrowdMatching as CM
    g, x, y = G.case(name)
    gd, xy = torch.from_numpy(g.astype(np.float32)).to(DEV), tuple(_dev(x, y))
    for k, th in enumerate(G.DIST_THRESHOLDS):
        want = fixture[f"dm_{name}_{k}"]
        if np.isnan(want).all():
            with pytest.raises(ZeroDivisionError):
                CM.CrowdMatchingTest2(gd, xy, th)
        else:
            assert CM.CrowdMatchingTest2(gd, xy, th) == tuple(want.tolist()), th


def test_distance_match_beyond_the_lds_and_register_resident_centres():
    _need_gpu()
    from umi import matching as M
    rng = np.random.default_rng(6)
    g = (rng.random((3, 300, 400)) < 0.004).astype(np.uint8)
    dots, cnt = M.dot_lists_numpy(g)
    cap = 9500                                                           # > 4096 (LDS) and > 8192 (register flags)
    centers = np.stack([rng.integers(0, 400, (3, cap)), rng.integers(0, 300, (3, cap))], axis=2).astype(np.int32)
    # the centres closest to the dots sit at the END of the list, so the matches land beyond 8192
    ys, xs = np.nonzero(g[0])
    centers[0, cap - ys.size:, 0], centers[0, cap - ys.size:, 1] = xs, ys
    centers[0, :cap - ys.size] += 1000
    c_count = np.array([cap, 5000, 0], dtype=np.int32)
    for th in (1, 3.5):
        got = M.distance_match(*_dev(dots, cnt, centers, c_count), th).cpu().numpy()
        assert np.array_equal(got, M.distance_match_numpy(dots, cnt, centers, c_count, th)), th
    assert got[0, 0] == ys.size and got[2].tolist() == [0, 0, int(cnt[2])]


@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_grid_sums_equal_the_numpy_statement(dtype):
    _need_gpu()
    from umi import matching as M
    rng = np.random.default_rng(7)
    for shape, size in (((2, 512, 512), 512), ((1, 768, 768), 768), ((2, 600, 520), 512), ((3, 300, 400), 512), ((1, 768, 768), 512),
                        ((2, 31, 17), 64)):
        m = rng.integers(0, 4, shape).astype(dtype)                      # integer valued: float64 sums are exact in any order
        got = M.grid_sums(torch.from_numpy(m).to(DEV), size)
        want = M.grid_sums_numpy(m, size)
        assert got.dtype == (torch.int64 if dtype == np.uint8 else torch.float64) and tuple(got.shape) == (shape[0], 8, 8)
        assert np.array_equal(got.cpu().numpy(), want), (shape, size)
    if dtype == np.float32:                                              # fixed order: two runs, the same bits
        x = torch.from_numpy(rng.standard_normal((2, 512, 512)).astype(np.float32)).to(DEV)
        a, b = M.grid_sums(x), M.grid_sums(x)
        assert torch.equal(a.view(torch.int64), b.view(torch.int64))


@pytest.mark.parametrize("name", list(G.GMAE_CASES))
def test_gmae_on_device_tensors_equals_the_reference(fixture, name):
    _need_gpu()
    import CrowdMatching as CM
    gt, pred = G.gmae_case(name)
    for a, b in ((np.float32, np.float32), (np.uint8, np.float32), (np.uint8, np.uint8)):
        gd, pd = torch.from_numpy(gt.astype(a)).to(DEV), torch.from_numpy(pred.astype(b)).to(DEV)
        for row, L in zip(fixture[name], (1, 2, 3)):
            assert CM.GMAE(L, gd, pd) == row.tolist()


def test_scatter_centers_writes_one_per_place():
    _need_gpu()
    from umi import matching as M
    rng = np.random.default_rng(8)
    centers = np.stack([rng.integers(-3, 70, (3, 500)), rng.integers(-3, 50, (3, 500))], axis=2).astype(np.int32)
    centers[1, 100:200] = centers[1, :100]                               # coinciding centres
    c_count = np.array([500, 200, 0], dtype=np.int32)
    got = M.scatter_centers(*_dev(centers, c_count), 48, 64)
    want = M.scatter_centers_numpy(centers, c_count, 48, 64)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want) and want.max() == 1 and want[2].sum() == 0


# ---- 4. component centres ----------------------------------------------------------------------------------------------------
def test_component_centers_on_the_fixture_masks(golden_dir):
    _need_gpu()
    from umi import infer
    from umi import matching as M
    g = np.load(os.path.join(golden_dir, "binary_infer.npz"))
    for name in GB.masks():
        shape = tuple(g[f"mask_{name}_shape"])
        m = np.unpackbits(g[f"mask_{name}_bits"])[:shape[0] * shape[1]].reshape(shape)
        _, counts, area, sum_y, sum_x = infer.label_components(torch.from_numpy(m).to(DEV).unsqueeze(0), check=True)
        cen = M.component_centers(counts, area, sum_y, sum_x).cpu().numpy()
        n = int(g[f"mask_{name}_count"])
        a, sy, sx = (g[f"mask_{name}_{k}"].astype(np.int64) for k in ("area", "sum_y", "sum_x"))
        want = np.zeros((1, area.shape[1], 2), dtype=np.int32)
        for s, col in ((sx, 0), (sy, 1)):
            q, r2 = s // a, 2 * (s % a)
            want[0, :n, col] = q + ((r2 > a) | ((r2 == a) & (q % 2 == 1)))
        assert counts.item() == n and np.array_equal(cen, want), name
        if 0 < n <= 2000:
            assert cen[0, :n].tolist() == [[round(int(x) / int(k)), round(int(y) / int(k))] for x, y, k in zip(sx, sy, a)], name


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------
def _blob_batch():
    rng = np.random.default_rng(9)
    N, H, W = 4, 512, 512
    mask = np.zeros((N, H, W), dtype=np.uint8)
    dots = np.zeros((N, H, W), dtype=np.float32)
    yy, xx = np.mgrid[:H, :W]
    for n, k in enumerate((120, 40, 0, 7)):
        cy, cx, rad = rng.integers(8, H - 8, k), rng.integers(8, W - 8, k), rng.integers(2, 7, k)
        for y, x, r in zip(cy, cx, rad):
            mask[n][(yy - y) ** 2 + (xx - x) ** 2 <= r * r] = 1
        keep = rng.random(k) < 0.85
        dots[n, np.clip(cy[keep] + rng.integers(-3, 4, keep.sum()), 0, H - 1), np.clip(cx[keep] + rng.integers(-3, 4, keep.sum()), 0, W - 1)] = 1
        extra = rng.integers(0, H * W, 5)
        dots[n].reshape(-1)[extra] = 1
    dots[2] = 0                                                          # no components and no dots
    return mask, dots


def _score_numpy(mask, dots, dist_thresh):
    import CrowdMatching as CM
    from umi import components as C
    from umi import matching as M
    out = []
    for n in range(mask.shape[0]):
        _, counts, area, sum_y, sum_x = C.label_components_numpy(mask[n])
        counts = np.asarray(counts).reshape(-1)
        area, sum_y, sum_x = (np.asarray(a).reshape(1, -1) for a in (area, sum_y, sum_x))
        cen = M.component_centers_numpy(counts, area, sum_y, sum_x)
        k = int(counts[0])
        x, y = cen[0, :k, 0].astype(np.int64), cen[0, :k, 1].astype(np.int64)
        gt = int(np.sum(dots[n]))
        e_dot = np.zeros_like(dots[n])
        e_dot[y, x] = 1
        abs_diff, rel, _, _ = CM.countAccuracyMetric(gt, k)
        p, r, f = CM.CrowdMatchingTest(dots[n], (x, y), G.SIGMAS, G.THRESHOLDS, inputType='Coordinates')
        p2, r2, f2 = CM.CrowdMatchingTest2(dots[n], (x, y), dist_thresh)
        out.append({"GT": gt, "Pred": k, "AbsDiff": abs_diff, "RelativeAccuracy": rel,
                    "G1": CM.GMAE(1, dots[n], e_dot)[0], "G2": CM.GMAE(2, dots[n], e_dot)[0], "G3": CM.GMAE(3, dots[n], e_dot)[0],
                    "arr_prec": p, "arr_recall": r, "arr_f1": f, "precision": p2, "recall": r2, "f1": f2})
    return out


def test_score_binary_masks_end_to_end_with_one_device_to_host_copy(monkeypatch):
    _need_gpu()
    from umi import infer
    mask, dots = _blob_batch()
    md, dd = torch.from_numpy(mask).to(DEV), torch.from_numpy(dots).to(DEV)
    infer.score_binary_masks(md, dd, G.SIGMAS, G.THRESHOLDS)             # warm-up: tables uploaded, workspace grown
    copies = []
    for meth in ("cpu", "item", "tolist", "numpy", "to", "__bool__", "__int__", "__float__", "__index__"):
        orig = getattr(torch.Tensor, meth)

        def counted(self, *a, _orig=orig, _meth=meth, **kw):
            to_host = _meth != "to" or any(str(v) == "cpu" or (isinstance(v, torch.device) and v.type == "cpu")
                                           for v in list(a) + list(kw.values()))
            if self.is_cuda and to_host:
                copies.append(_meth)
            return _orig(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, meth, counted)
    got = infer.score_binary_masks(md, dd, G.SIGMAS, G.THRESHOLDS, dist_thresh=10)
    monkeypatch.undo()
    assert copies == ["cpu"], copies
    want = _score_numpy(mask, dots, 10)
    assert len(got) == len(want) == 4 and want[0]["Pred"] > 50 and want[2]["Pred"] == 0 and want[2]["GT"] == 0
    for a, b in zip(got, want):
        assert a.keys() == b.keys()
        for k in a:
            if isinstance(b[k], np.ndarray):
                assert a[k].dtype == np.float64 and np.array_equal(a[k], b[k]), k
            else:
                assert a[k] == b[k] and type(a[k]) is type(b[k]), (k, a[k], b[k])
    # components without dots: the reference's CrowdMatchingTest2 divides by zero
    with pytest.raises(ZeroDivisionError):
        infer.score_binary_masks(md[:1], torch.zeros_like(dd[:1]), G.SIGMAS, G.THRESHOLDS)


# ---- 6. graph replay ---------------------------------------------------------------------------------------------------------
def test_matching_replays_from_a_graph_on_new_contents():
    _need_gpu()
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_matching_graph.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "MATCHING_GRAPH_OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
