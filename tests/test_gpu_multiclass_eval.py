"""GPU: the multi-class evaluation on the MI355X -- umi.infer.label_class_components / count_class_objects /
score_multiclass_masks and umi.matching.split_classes / class_center_lists on device tensors -- against the NumPy statements
(umi.components.label_class_components_numpy, umi.matching.score_multiclass_numpy), which the CPU suite pins to SciPy and to the
reference's recorded results (tests/golden/multiclass_eval.npz), against that fixture directly, and against the merged binary
kernels (umi.infer.label_components).  Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from oracle import recipe
from tools import gen_golden_multiclass_eval as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
LABEL_CASES = list(G.label_cases())
FAULT_CLASS, FAULT_CAP = 5, 6


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: torch.cuda.is_available() is False")


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "multiclass_eval.npz"))


def _label(m, K, **kw):
    from umi import infer
    return infer.label_class_components(torch.from_numpy(np.ascontiguousarray(m)).to(DEV), K, **kw)


def _assert_equal_to_numpy(m, K, outs, max_components=None):
    from umi.components import label_class_components_numpy
    want = label_class_components_numpy(m, K, max_components)
    assert len(outs) == len(want) == 7
    for name, a, b in zip(("labels", "counts", "class_counts", "label_class", "area", "sum_y", "sum_x"), outs, want):
        a = a.cpu().numpy()
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert np.array_equal(a, b), name
    return want


# ---- labelling ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LABEL_CASES)
def test_labelling_equals_numpy_and_the_scipy_fixture(fixture, name):
    _need_gpu()
    from umi import infer
    from umi.components import label_checksum
    m, K = G.label_cases()[name]
    outs = _label(m, K, check=True)
    _assert_equal_to_numpy(m, K, outs)
    labels, counts, class_counts, label_class, area, sum_y, sum_x = (t.cpu().numpy() for t in outs)
    want_cc = fixture[f"lab_{name}_count"]
    assert class_counts[0].tolist() == want_cc.tolist() and counts[0] == want_cc.sum()
    assert label_checksum(labels) == int(fixture[f"lab_{name}_checksum"])
    n = int(counts[0])
    for c in range(1, K):
        pick = np.flatnonzero(label_class[0, :n] == c)
        assert area[0, pick].tolist() == fixture[f"lab_{name}_c{c}_area"].tolist()
        assert sum_y[0, pick].tolist() == fixture[f"lab_{name}_c{c}_sum_y"].tolist()
        assert sum_x[0, pick].tolist() == fixture[f"lab_{name}_c{c}_sum_x"].tolist()
        assert labels.reshape(-1)[fixture[f"lab_{name}_c{c}_first"]].tolist() == (pick + 1).tolist()
    md = torch.from_numpy(m).to(DEV)
    assert torch.equal(infer.count_class_objects(md, K, check=True), outs[2])


@pytest.mark.parametrize("K", [2, 3, 4, 8])
@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (63, 64), (64, 65), (33, 200), (257, 385), (300, 17)])
def test_random_classes_match_numpy(K, hw):
    _need_gpu()
    for i, d in enumerate((0.05, 0.3, 0.6, 1.0)):
        m = np.stack([G.random_classes(hw[0] * 31 + hw[1] + 100 * K + 10 * i + j, hw, K, d) for j in range(3)])
        _assert_equal_to_numpy(m, K, _label(m, K, check=True))


def test_tiling_gives_one_component_per_pixel_with_cap_hw():
    _need_gpu()
    for h, w in ((6, 6), (64, 70), (130, 129)):
        m = G.tiling_2x2(h, w)[None]
        outs = _label(m, 5, max_components=h * w, check=True)
        _assert_equal_to_numpy(m, 5, outs, h * w)
        assert outs[1].item() == h * w and outs[4].shape == (1, h * w)
        assert torch.equal(outs[0].cpu().reshape(-1), torch.arange(1, h * w + 1, dtype=torch.int32))
        assert outs[4].cpu().eq(1).all()


def test_two_class_checkerboard_has_two_components():
    _need_gpu()
    for h, w in ((65, 67), (256, 192)):
        m = G.checkerboard(h, w)[None]
        outs = _label(m, 3, check=True)
        _assert_equal_to_numpy(m, 3, outs)
        assert outs[1].item() == 2 and outs[2].cpu().tolist() == [[0, 1, 1]]


@pytest.mark.parametrize("K,width", [(3, 1), (3, 5), (4, 1), (8, 2)])
def test_concentric_rings(K, width):
    _need_gpu()
    m = G.rings(321, K, width)[None]
    _assert_equal_to_numpy(m, K, _label(m, K, check=True))


@pytest.mark.parametrize("vertical", [False, True])
@pytest.mark.parametrize("width", [1, 64])
def test_stripes_cross_every_seam(width, vertical):
    _need_gpu()
    for K in (3, 4):
        m = G.stripes(200, 330, K, width, vertical)[None]
        outs = _label(m, K, check=True)
        _assert_equal_to_numpy(m, K, outs)
        assert outs[1].item() == -(-(330 if vertical else 200) // width)


def test_serpentine_with_the_gaps_filled():
    _need_gpu()
    for h, w in ((130, 131), (257, 64), (512, 512)):
        m = G.serpentine(h, w)[None]
        outs = _label(m, 3, check=True)
        _assert_equal_to_numpy(m, 3, outs)
        assert outs[2][0, 1].item() == 1


def test_768_batch_16():
    _need_gpu()
    from umi import infer
    for K in (3, 4):
        m = np.stack([G.random_classes(7000 + 16 * K + j, (768, 768), K, (0.2, 0.5, 0.8, 1.0)[j % 4]) for j in range(16)])
        m[3, 300:330] = 1                                           # a band across every vertical seam
        m[5, :, 500:520] = 2
        md = torch.from_numpy(m).to(DEV)
        outs = infer.label_class_components(md, K, check=True)
        _assert_equal_to_numpy(m, K, outs)
        assert torch.equal(infer.count_class_objects(md, K, check=True), outs[2])


def test_one_2048_image():
    _need_gpu()
    from umi import infer
    m = G.random_classes(2048, (2048, 2048), 4, 0.7)[None]
    m[0, 1000:1040] = 3
    md = torch.from_numpy(m).to(DEV)
    outs = infer.label_class_components(md, 4, check=True)
    _assert_equal_to_numpy(m, 4, outs)
    assert torch.equal(infer.count_class_objects(md, 4, check=True), outs[2])


def test_batch_of_different_images():
    _need_gpu()
    hw = (150, 190)
    m = np.stack([G.random_classes(1, hw, 4, 0.1), np.zeros(hw, np.uint8), G.stripes(hw[0], hw[1], 4, 64, True),
                  G.random_classes(2, hw, 4, 0.9), G.checkerboard(*hw), np.full(hw, 3, np.uint8), G.serpentine(*hw)])
    outs = _label(m, 4, check=True)
    _assert_equal_to_numpy(m, 4, outs)
    for n in range(m.shape[0]):                                     # and each image on its own
        one = _label(m[n], 4, check=True)
        assert one[0].shape == hw and torch.equal(one[0], outs[0][n])
        for a, b in zip(one[1:], outs[1:]):
            assert torch.equal(a[0], b[n])


def test_two_runs_give_the_same_bits():
    _need_gpu()
    m = np.stack([G.random_classes(50 + j, (257, 385), 4, 0.6) for j in range(4)])
    a, b = _label(m, 4), _label(m, 4)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---- against the binary kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(1, 1), (33, 65), (257, 385), (512, 512)])
def test_two_classes_equal_label_components_bit_for_bit(hw):
    _need_gpu()
    from umi import infer
    rng = np.random.default_rng(hw[0] + hw[1])
    for d in (0.1, 0.45, 0.7, 1.0):
        md = torch.from_numpy((rng.random((3,) + hw) < d).astype(np.uint8)).to(DEV)
        labels, counts, class_counts, label_class, area, sum_y, sum_x = infer.label_class_components(md, 2, check=True)
        want = infer.label_components(md, check=True)
        for a, b in zip((labels, counts, area, sum_y, sum_x), want):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
        assert torch.equal(class_counts[:, 1], counts) and not class_counts[:, 0].any()
        assert torch.equal(label_class != 0, area != 0)
        assert torch.equal(infer.count_class_objects(md, 2)[:, 1], infer.count_objects(md))


@pytest.mark.parametrize("K", [3, 4, 8])
def test_per_class_results_equal_binary_calls_on_each_class(K):
    _need_gpu()
    from umi import infer
    m = np.stack([G.random_classes(900 + K, (257, 385), K, 0.6), G.blob_classes(901 + K, (257, 385), K, 150)[0],
                  G.rings(385, K, 2)[:257]])
    md = torch.from_numpy(m).to(DEV)
    labels, counts, class_counts, label_class, area, sum_y, sum_x = infer.label_class_components(md, K, check=True)
    total = torch.zeros_like(counts)
    for c in range(1, K):
        b_labels, b_counts, b_area, b_sy, b_sx = infer.label_components((md == c).to(torch.uint8), check=True)
        assert torch.equal(class_counts[:, c], b_counts)
        total += b_counts
        for n in range(m.shape[0]):
            nc, k = int(b_counts[n]), int(counts[n])
            pick = (label_class[n, :k] == c).nonzero().reshape(-1)          # global numbers - 1 of this class, ascending
            assert pick.numel() == nc
            assert torch.equal(area[n, pick], b_area[n, :nc]) and torch.equal(sum_y[n, pick], b_sy[n, :nc])
            assert torch.equal(sum_x[n, pick], b_sx[n, :nc])
            # the binary label map, renumbered through `pick`, is this class's part of the global map
            lut = torch.cat([torch.zeros(1, dtype=torch.int32, device=DEV), (pick + 1).to(torch.int32)])
            assert torch.equal(lut[b_labels[n].long()], torch.where(md[n] == c, labels[n], torch.zeros_like(labels[n])))
    assert torch.equal(total, counts)


# ---- cap and foreign values -----------------------------------------------------------------------------------------------------
def test_cap_smaller_than_the_count():
    _need_gpu()
    from umi import infer, lib as L, ops
    from umi.components import label_class_components_numpy
    K, cap, guard = 4, 100, 64
    for N in (1, 2):
        m = np.stack([G.random_classes(400 + j, (70, 130), K, 0.5) for j in range(N)])
        full = label_class_components_numpy(m, K)
        assert full[1].min() > cap
        md = torch.from_numpy(m).to(DEV)
        labels = torch.empty(m.shape, dtype=torch.int32, device=DEV)
        counts = torch.empty(N, dtype=torch.int32, device=DEV)
        class_counts = torch.empty((N, K), dtype=torch.int32, device=DEV)
        label_class = torch.full((N * cap + guard,), 0xAB, dtype=torch.uint8, device=DEV)
        area = torch.full((N * cap + guard,), -7, dtype=torch.int32, device=DEV)
        sum_y = torch.full((N * cap + guard,), -7, dtype=torch.int64, device=DEV)
        sum_x = torch.full((N * cap + guard,), -7, dtype=torch.int64, device=DEV)
        nbytes = L.fn("umi_class_components_ws_bytes")(N, 70, 130, K)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        L.check(L.fn("umi_label_class_components")(md.data_ptr(), labels.data_ptr(), counts.data_ptr(), class_counts.data_ptr(),
                                                   label_class.data_ptr(), area.data_ptr(), sum_y.data_ptr(), sum_x.data_ptr(), N, 70,
                                                   130, K, cap, ws.data_ptr(), nbytes, ops._stream()), "umi_label_class_components")
        assert ws[:4].view(torch.int32).item() == FAULT_CAP
        assert np.array_equal(counts.cpu().numpy(), full[1]) and np.array_equal(class_counts.cpu().numpy(), full[2])
        assert np.array_equal(labels.cpu().numpy(), full[0])
        for got, want, sentinel in ((label_class, full[3], 0xAB), (area, full[4], -7), (sum_y, full[5], -7), (sum_x, full[6], -7)):
            got = got.cpu().numpy()
            assert np.array_equal(got[:N * cap].reshape(N, cap), want[:, :cap])
            assert (got[N * cap:] == sentinel).all()                     # nothing written past the rows
        outs = infer.label_class_components(md, K, max_components=cap)
        _assert_equal_to_numpy(m, K, outs, cap)
        with pytest.raises(RuntimeError, match="max_components"):
            infer.label_class_components(md, K, max_components=cap, check=True)
    with pytest.raises(ValueError):
        infer.label_class_components(md, K, max_components=70 * 130 + 1)
    with pytest.raises(ValueError):
        infer.label_class_components(md, 9)


def test_value_above_n_classes_is_background_and_reported():
    _need_gpu()
    from umi import infer
    m = np.stack([G.random_classes(500 + j, (130, 200), 6, 0.7) for j in range(2)])
    m[1, 5, 5] = 255
    md = torch.from_numpy(m).to(DEV)
    outs, fault = infer._label_class_components(md, 3, None)
    assert fault.item() == FAULT_CLASS
    _assert_equal_to_numpy(np.where(m >= 3, 0, m).astype(np.uint8), 3, outs)
    with pytest.raises(RuntimeError, match="n_classes"):
        infer.label_class_components(md, 3, check=True)
    # a foreign value and an overflow of the rows in one call: the tile pass's code, stored first, stays
    assert infer._label_class_components(md, 3, 10)[1].item() == FAULT_CLASS
    with pytest.raises(RuntimeError, match="n_classes"):
        infer.count_class_objects(md, 3, check=True)
    assert torch.equal(infer.count_class_objects(md, 3), outs[2])
    # the same mask is clean for six classes
    _assert_equal_to_numpy(np.where(m == 255, 0, m).astype(np.uint8), 6,
                           infer.label_class_components(torch.from_numpy(np.where(m == 255, 0, m).astype(np.uint8)).to(DEV), 6,
                                                        check=True))


# ---- lists ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 3, 4, 8])
def test_split_classes_and_center_lists_match_numpy(K):
    _need_gpu()
    from umi import infer, matching as M
    m = np.stack([G.blob_classes(600 + K + j, (200, 333), K, 120)[0] for j in range(3)])
    md = torch.from_numpy(m).to(DEV)
    planes = M.split_classes(md, K)
    assert planes.dtype == torch.uint8 and np.array_equal(planes.cpu().numpy(), M.split_classes_numpy(m, K))
    _, counts, class_counts, label_class, area, sum_y, sum_x = infer.label_class_components(md, K, check=True)
    centers, c_count = M.class_center_lists(counts, label_class, area, sum_y, sum_x, K)
    want_c, want_n = M.class_center_lists_numpy(*(t.cpu().numpy() for t in (counts, label_class, area, sum_y, sum_x)), K)
    assert centers.dtype == torch.int32 and c_count.dtype == torch.int32
    assert np.array_equal(c_count.cpu().numpy(), want_n) and np.array_equal(centers.cpu().numpy(), want_c)
    assert torch.equal(c_count.view(3, K - 1), class_counts[:, 1:])


# ---- scoring --------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
    return type(a) is type(b) and (a == b or (a != a and b != b))


@pytest.mark.parametrize("name", [n for n in G.SCORE_CASES if n != "k3_no_pred_12"])
def test_scores_equal_numpy_and_the_reference_fixture(fixture, name):
    _need_gpu()
    from umi import infer, matching as M
    mask, dots, K = G.score_case(name)
    got = infer.score_multiclass_masks(torch.from_numpy(mask).to(DEV), torch.from_numpy(dots).to(DEV), K, G.SIGMAS, G.THRESHOLDS)
    assert _same(got, M.score_multiclass_numpy(mask, dots, K, G.SIGMAS, G.THRESHOLDS))
    for n, d in enumerate(got):
        for c in range(1, K):
            key, r = f"sc_{name}_{n}_c{c}", d[c]
            assert [r["GT"], r["Pred"], r["AbsDiff"], r["Accuracy"], r["AccuracyRelative"], r["AccuracyRelativePD"]] == \
                fixture[key + "_count"].tolist()
            for k in ("prec", "recall", "f1"):
                assert np.array_equal(r["arr_" + k], fixture[f"{key}_{k}"])
            assert [r["G1"], r["G2"], r["G3"]] == fixture[key + "_gmae"].tolist()
        want = fixture[f"sc_{name}_{n}_ratio"]
        assert np.array_equal(np.array([d["ratio"][k] for k in ("GT", "Pred", "AbsDiff", "Accuracy", "AccuracyRelative",
                                                                 "AccuracyRelativePD")]), want, equal_nan=True)
        if K == 4:
            keys = ("cellAccuracy", "immuneAccuracy", "tumorAccuracy", "GTImmo", "PredImmo", "AccuracyImmo", "GTImmoTummor",
                    "PredImmoTummor", "AccuracyImmoTummor")
            assert np.array_equal(np.array([d["ratio3"][k] for k in keys]), fixture[f"sc_{name}_{n}_ratio3"])


def test_scores_undefined_cases():
    _need_gpu()
    from umi import infer
    mask, dots, K = G.score_case("k3_no_pred_12")
    with pytest.raises(ZeroDivisionError):
        infer.score_multiclass_masks(torch.from_numpy(mask).to(DEV), torch.from_numpy(dots).to(DEV), K, G.SIGMAS, G.THRESHOLDS)
    mask, dots, K = G.score_case("k3_256")
    with pytest.raises(RuntimeError, match="max_components"):
        infer.score_multiclass_masks(torch.from_numpy(mask).to(DEV), torch.from_numpy(dots).to(DEV), K, G.SIGMAS, G.THRESHOLDS,
                                     max_components=10)
    with pytest.raises(ValueError):
        infer.score_multiclass_masks(torch.from_numpy(mask).to(DEV), torch.from_numpy(dots[:, :8]).to(DEV), K, G.SIGMAS, G.THRESHOLDS)


def test_two_class_scores_match_numpy():
    _need_gpu()
    from umi import infer, matching as M
    mask, dots, _ = G.score_case("k3_96x130")
    mask, dots = (mask != 0).astype(np.uint8), (dots != 0).astype(np.uint8)
    got = infer.score_multiclass_masks(torch.from_numpy(mask).to(DEV), torch.from_numpy(dots).to(DEV), 2, G.SIGMAS, G.THRESHOLDS)
    assert _same(got, M.score_multiclass_numpy(mask, dots, 2, G.SIGMAS, G.THRESHOLDS)) and list(got[0]) == [1]


def test_end_to_end_unet_3_3_8():
    _need_gpu()
    import Model
    from umi import infer, matching as M
    model = Model.UNet(3, 3, 8, False, compute_dtype="fp32")
    model.load_state_dict(recipe.fill_state_dict(model.state_dict(), seed=41))
    model.to(DEV)
    x = torch.randn((2, 3, 128, 128), generator=torch.Generator().manual_seed(9)).to(DEV)
    mask = infer.predict_mask(model, x)
    assert mask.dtype == torch.uint8 and mask.shape == (2, 128, 128)
    mh = mask.cpu().numpy()
    assert mh.max() <= 2
    rng = np.random.default_rng(10)
    dots = np.where(rng.random(mh.shape) < 0.004, rng.integers(1, 3, mh.shape), 0).astype(np.uint8)
    if not ((mh == 1) | (mh == 2)).reshape(2, -1).any(axis=1).all():
        pytest.fail("the seeded model predicts no object in an image; pick another seed")
    got = infer.score_multiclass_masks(mask, torch.from_numpy(dots).to(DEV), 3, G.SIGMAS, G.THRESHOLDS)
    assert _same(got, M.score_multiclass_numpy(mh, dots, 3, G.SIGMAS, G.THRESHOLDS))
    _assert_equal_to_numpy(mh, 3, infer.label_class_components(mask, 3, check=True))
