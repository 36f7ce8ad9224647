"""CPU: the NumPy statement of the component labelling (umi/components.py) against SciPy's recorded and live results,
loss.MRAccuracy on CPU tensors against the reference's recorded values (tests/golden/binary_infer.npz,
tools/gen_golden_binary_infer.py), the fp32 sigmoid threshold constant, and the new C-ABI entry points' argument checks."""
import os

import numpy as np
import pytest
import torch

from tools import gen_golden_binary_infer as G

_NAMES = list(G.masks())


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "binary_infer.npz"))


def _mask(g, name):
    shape = tuple(g[f"mask_{name}_shape"])
    return np.unpackbits(g[f"mask_{name}_bits"])[:shape[0] * shape[1]].reshape(shape)


def test_fixture_masks_are_the_generators(fixture):
    assert list(fixture["mask_names"]) == _NAMES
    for name, m in G.masks().items():
        np.testing.assert_array_equal(_mask(fixture, name), m, err_msg=name)


@pytest.mark.parametrize("name", _NAMES)
def test_label_components_numpy_matches_scipy_fixture(fixture, name):
    from umi import components as C
    m = _mask(fixture, name)
    labels, counts, area, sum_y, sum_x, firsts = C.label_components_numpy(m, return_first=True)
    n = int(fixture[f"mask_{name}_count"])
    assert labels.shape == m.shape and labels.dtype == np.int32
    assert counts.shape == (1,) and counts.dtype == np.int32 and int(counts[0]) == n
    cap = C.components_cap(*m.shape)
    assert area.shape == sum_y.shape == sum_x.shape == (1, cap) and n <= cap
    assert area.dtype == np.int32 and sum_y.dtype == np.int64 and sum_x.dtype == np.int64
    np.testing.assert_array_equal(area[0, :n], fixture[f"mask_{name}_area"])
    np.testing.assert_array_equal(sum_y[0, :n], fixture[f"mask_{name}_sum_y"])
    np.testing.assert_array_equal(sum_x[0, :n], fixture[f"mask_{name}_sum_x"])
    np.testing.assert_array_equal(firsts[0], fixture[f"mask_{name}_first"])
    assert not area[0, n:].any() and not sum_y[0, n:].any() and not sum_x[0, n:].any()
    assert C.label_checksum(labels) == int(fixture[f"mask_{name}_checksum"])
    assert C.count_components_numpy(m) == n
    np.testing.assert_array_equal(labels != 0, m != 0)


def test_isolated_pixels_reach_the_cap(fixture):
    from umi import components as C
    for name in ("isolated_512x512", "isolated_257x385"):
        shape = tuple(fixture[f"mask_{name}_shape"])
        assert int(fixture[f"mask_{name}_count"]) == C.components_cap(*shape)


def test_label_components_numpy_matches_live_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    from umi import components as C
    rng = np.random.default_rng(77)
    for shape in ((1, 1), (1, 7), (7, 1), (2, 2), (33, 65), (63, 64), (65, 129), (200, 311)):
        for d in (0.0, 0.05, 0.3, 0.45, 0.5, 0.6, 0.9, 1.0):
            m = (rng.random((3,) + shape) < d).astype(np.uint8) * 255
            labels, counts, area, sum_y, sum_x = C.label_components_numpy(m)
            yy, xx = np.mgrid[:shape[0], :shape[1]]
            for b in range(3):
                want, n = ndimage.label(m[b], structure=np.ones((3, 3)))
                assert counts[b] == n and np.array_equal(labels[b], want), (shape, d)
                idx = np.arange(1, n + 1)
                if n:
                    np.testing.assert_array_equal(area[b, :n], ndimage.sum(m[b] != 0, want, idx).astype(np.int64))
                    np.testing.assert_array_equal(sum_y[b, :n], ndimage.sum(yy, want, idx).astype(np.int64))
                    np.testing.assert_array_equal(sum_x[b, :n], ndimage.sum(xx, want, idx).astype(np.int64))
                assert not area[b, n:].any()


def test_label_components_numpy_shapes():
    from umi import components as C
    labels, counts, area, _, _ = C.label_components_numpy(np.ones((4, 6), dtype=np.uint8))
    assert labels.shape == (4, 6) and counts.tolist() == [1] and area.shape == (1, 6) and area[0, 0] == 24
    with pytest.raises(ValueError):
        C.label_components_numpy(np.ones((2, 1, 4, 6), dtype=np.uint8))


def test_zoom_rule_matches_scipy_fixture(fixture):
    """The NumPy statement of SciPy's order-0 rule that the GPU test holds the kernel to reproduces SciPy's recorded outputs."""
    for i, (seed, shape, ohw, dtype) in enumerate(G.ZOOM_CASES):
        got = G.zoom_nearest_numpy(G.zoom_input(seed, shape, dtype), ohw)
        assert got.shape == tuple(fixture[f"zoom{i}_shape"]) and got.dtype == np.dtype(dtype)
        if f"zoom{i}_checksum" in fixture:
            assert G.checksum(got) == int(fixture[f"zoom{i}_checksum"]) and got.sum() == int(fixture[f"zoom{i}_sum"])
        elif dtype == "uint8":
            np.testing.assert_array_equal(np.packbits(got), fixture[f"zoom{i}_bits"])
        else:
            np.testing.assert_array_equal(got, fixture[f"zoom{i}"])
    last = G.zoom_nearest_numpy(np.ones((512, 512), dtype=np.uint8), (224, 224))
    assert not last[-1].any() and not last[:, -1].any() and last[:-1, :-1].all()


@pytest.mark.parametrize("name", G.MR_CASES)
def test_mraccuracy_cpu_matches_reference(fixture, name):
    import loss as L
    pred, target = G.mr_case(name)
    got = L.MRAccuracy(torch.from_numpy(pred), torch.from_numpy(target))
    assert isinstance(got, float)
    assert got == float(fixture[f"mr_{name}"])


def test_mraccuracy_cases_cover_the_branches():
    pred, target = G.mr_case("both_empty")
    assert target[0].sum() == 0 and (pred[0] < 0).all() and target[2].sum() == 0 and (pred[2] >= 0).any()
    pred, target = G.mr_case("threshold")
    cut = np.float32(G.CUTOFF)
    assert (pred == cut).any() and (pred == np.nextafter(cut, np.float32(-1))).any()


def test_mraccuracy_wrong_shapes_fail():
    import loss as L
    t = torch.zeros(2, 8, 8)
    with pytest.raises(ValueError):                     # squeeze(1) leaves (B, 2, H, W): connectedComponents gets a 3-D image
        L.MRAccuracy(torch.zeros(2, 2, 8, 8), t)
    with pytest.raises(IndexError):                     # pred_bin[batch] beyond pred's batch
        L.MRAccuracy(torch.zeros(1, 1, 8, 8), t)
    with pytest.raises(ZeroDivisionError):              # mre /= 0
        L.MRAccuracy(torch.zeros(0, 1, 8, 8), torch.zeros(0, 8, 8))


def _sigmoid_ge_half(bits):
    x = torch.from_numpy(np.array([bits], dtype=np.uint32).view(np.float32))
    return bool(torch.sigmoid(x) >= 0.5)


def test_sigmoid_half_cutoff_is_where_torch_sigmoid_reaches_half():
    """Bisection over the bit patterns of the negative floats (a larger pattern is a more negative value) against torch.sigmoid
    of this torch build: the last pattern with sigmoid >= 0.5 is the exported constant, and the decision is monotone around it."""
    from umi import infer
    assert _sigmoid_ge_half(0x80000000) and _sigmoid_ge_half(0) and not _sigmoid_ge_half(0xBF800000)
    lo, hi = 0x80000000, 0xBF800000
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if _sigmoid_ge_half(mid):
            lo = mid
        else:
            hi = mid
    assert lo == infer.SIGMOID_HALF_CUTOFF_BITS == 0xB43FFFFE, hex(lo)
    assert infer.SIGMOID_HALF_CUTOFF == -1.7881390590446244e-07 == G.CUTOFF
    band = np.arange(lo - 5000, lo + 5001, dtype=np.uint32)
    ge = (torch.sigmoid(torch.from_numpy(band.view(np.float32))) >= 0.5).numpy()
    np.testing.assert_array_equal(ge, band <= lo)
    pos = torch.from_numpy(np.array([0, 1, 0x00800000, 0x3F800000, 0x7F800000], dtype=np.uint32).view(np.float32))
    assert bool((torch.sigmoid(pos) >= 0.5).all())


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    from umi import lib
    assert lib.fn("umi_binary_mask")(None, None, 16, None) == -1
    assert lib.fn("umi_binary_mask")(16, 16, 0, None) == -1
    assert lib.fn("umi_zoom_nearest")(None, 0, None, 1, 4, 4, 8, 8, None) == -1
    assert lib.fn("umi_zoom_nearest")(16, 0, 16, 1, 4, 0, 8, 8, None) == -1
    assert lib.fn("umi_zoom_nearest")(16, 2, 16, 1, 4, 4, 8, 8, None) == -1
    assert lib.fn("umi_sum_trunc")(None, None, 1, 16, None, 0, None) == -1
    assert lib.fn("umi_sum_trunc")(16, 16, 0, 16, 16, 1 << 20, None) == -1
    assert lib.fn("umi_sum_trunc")(16, 16, 2, 16, 16, 8, None) == -3
    assert lib.fn("umi_sum_trunc_ws_bytes")(16) == 16 * 64 * 8 and lib.fn("umi_sum_trunc_ws_bytes")(0) == 0
    assert lib.fn("umi_count_components")(None, None, 1, 8, 8, None, 0, None) == -1
    assert lib.fn("umi_count_components")(16, 16, 1, 0, 8, 16, 1 << 20, None) == -1
    assert lib.fn("umi_label_components")(None, None, None, None, None, None, 1, 8, 8, None, 0, None) == -1
    assert lib.fn("umi_label_components")(16, 16, 16, 16, 16, 16, -1, 8, 8, 16, 1 << 20, None) == -1
    assert lib.fn("umi_components_cap")(0, 8) == -1
    assert lib.fn("umi_components_cap")(5, 8) == 12 and lib.fn("umi_components_cap")(512, 512) == 65536
    # sizes: the fault word's slot, the int32 parent map and the block counts; unsupported sizes answer 0 / UMI_ERR_UNSUPPORTED
    assert lib.fn("umi_components_ws_bytes")(16, 512, 512) >= 16 * 512 * 512 * 4
    assert lib.fn("umi_components_ws_bytes")(0, 8, 8) == 0
    assert lib.fn("umi_components_ws_bytes")(4, 32768, 32768) == 0
    assert lib.fn("umi_count_components")(16, 16, 4, 32768, 32768, 16, 1 << 20, None) == -2
    assert lib.fn("umi_count_components")(16, 16, 1, 8, 8, 16, 8, None) == -3          # workspace too small
