"""CPU: the NumPy statements of the multi-class evaluation (umi.components.label_class_components_numpy,
umi.matching.score_multiclass_numpy) against tests/golden/multiclass_eval.npz: SciPy's per-class labelling of the seeded masks
of tools/gen_golden_multiclass_eval.py and the reference's own CrowdMatching.py results on its seeded scoring cases.  The inputs
are rebuilt from the seeds here.  Every comparison is exact."""
import math
import os

import numpy as np
import pytest

from tools import gen_golden_multiclass_eval as G

LABEL_CASES = list(G.label_cases())
SCORE_CASES = list(G.SCORE_CASES)
RAISES = ("k3_no_pred_12",)


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "multiclass_eval.npz"))


def same(a, b):
    """Exact equality of two floats / arrays, nan equal to nan."""
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def check_labelling(fixture, name, got, m, K):
    """`got` = the seven outputs of a labelling of the (H, W) mask m (+ the first-pixel list or None) against the fixture."""
    from umi.components import label_checksum
    labels, counts, class_counts, label_class, area, sum_y, sum_x, first = got
    want_cc = fixture[f"lab_{name}_count"]
    assert class_counts.reshape(-1).tolist() == want_cc.tolist() and class_counts.reshape(-1)[0] == 0
    n = int(want_cc.sum())
    assert int(np.asarray(counts).reshape(-1)[0]) == n
    assert label_checksum(labels) == int(fixture[f"lab_{name}_checksum"])
    label_class, area = np.asarray(label_class).reshape(-1), np.asarray(area).reshape(-1)
    sum_y, sum_x = np.asarray(sum_y).reshape(-1), np.asarray(sum_x).reshape(-1)
    assert n <= area.size
    assert not label_class[n:].any() and not area[n:].any() and not sum_y[n:].any() and not sum_x[n:].any()
    lab = np.asarray(labels).reshape(m.shape)
    for c in range(1, K):
        pick = np.flatnonzero(label_class[:n] == c)
        assert area[pick].tolist() == fixture[f"lab_{name}_c{c}_area"].tolist()
        assert sum_y[pick].tolist() == fixture[f"lab_{name}_c{c}_sum_y"].tolist()
        assert sum_x[pick].tolist() == fixture[f"lab_{name}_c{c}_sum_x"].tolist()
        want_first = fixture[f"lab_{name}_c{c}_first"]
        if first is not None:
            assert np.asarray(first)[pick].tolist() == want_first.tolist()
        # the label at a class's first pixels: that class's labels, ascending
        assert lab.reshape(-1)[want_first].tolist() == (pick + 1).tolist()
        assert np.all((lab > 0)[m == c]) and np.all(np.isin(lab[m == c], pick + 1))
    assert not lab[(m == 0) | (m >= K)].any()


def test_fixture_lists_the_generator_cases(fixture):
    assert list(fixture["label_names"]) == LABEL_CASES and list(fixture["score_names"]) == SCORE_CASES
    assert fixture["sigmas"].tolist() == G.SIGMAS and np.array_equal(fixture["thresholds"], np.array(G.THRESHOLDS))
    for name, (m, K) in G.label_cases().items():
        assert fixture[f"lab_{name}_shape"].tolist() == list(m.shape) + [K]


@pytest.mark.parametrize("name", LABEL_CASES)
def test_numpy_labelling_equals_scipy(fixture, name):
    from umi.components import class_components_cap, label_class_components_numpy
    m, K = G.label_cases()[name]
    *out, first = label_class_components_numpy(m, K, return_first=True)
    assert out[0].dtype == np.int32 and out[3].dtype == np.uint8 and out[4].dtype == np.int32 and out[5].dtype == np.int64
    assert out[4].shape == (1, class_components_cap(m.shape[0], m.shape[1], K))
    check_labelling(fixture, name, tuple(out) + (first[0],), m, K)


def test_tiling_has_one_component_per_pixel(fixture):
    from umi.components import class_components_cap, label_class_components_numpy
    m, K = G.label_cases()["tiling_6x6"]
    labels, counts, class_counts, *_ = label_class_components_numpy(m, K)
    assert counts[0] == 36 == class_components_cap(6, 6, K) and class_counts[0].tolist() == [0, 9, 9, 9, 9]
    assert np.array_equal(labels, np.arange(1, 37).reshape(6, 6))


def test_two_classes_equal_the_binary_statement():
    from umi.components import label_class_components_numpy, label_components_numpy
    m = (np.random.default_rng(5).random((3, 70, 90)) < 0.45).astype(np.uint8)
    labels, counts, class_counts, label_class, area, sum_y, sum_x = label_class_components_numpy(m, 2)
    for a, b in zip((labels, counts, area, sum_y, sum_x), label_components_numpy(m)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert np.array_equal(class_counts[:, 1], counts) and np.array_equal(label_class != 0, area != 0)


def test_numpy_cap_and_foreign_values():
    from umi.components import label_class_components_numpy
    m, K = G.label_cases()["random_k4_d0.5_33x65"]
    full = label_class_components_numpy(m, K)
    cut = label_class_components_numpy(m, K, max_components=50)
    assert cut[1][0] == full[1][0] > 50 and np.array_equal(cut[0], full[0]) and np.array_equal(cut[2], full[2])
    for a, b in zip(cut[3:], full[3:]):
        assert a.shape == (1, 50) and np.array_equal(a[0], b[0, :50])
    # a value >= n_classes is background
    a = label_class_components_numpy(m, 3)
    b = label_class_components_numpy(np.where(m >= 3, 0, m), 3)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        label_class_components_numpy(m, 9)


def check_scores(fixture, name, got, K):
    """The list of dicts of one scoring case against the reference's recorded results."""
    for n, d in enumerate(got):
        for c in range(1, K):
            key = f"sc_{name}_{n}_c{c}"
            r = d[c]
            assert type(r["GT"]) is int and type(r["Pred"]) is int
            want = fixture[key + "_count"].tolist()
            assert [r["GT"], r["Pred"], r["AbsDiff"], r["Accuracy"], r["AccuracyRelative"], r["AccuracyRelativePD"]] == want
            for k in ("prec", "recall", "f1"):
                assert r["arr_" + k].dtype == np.float64 and np.array_equal(r["arr_" + k], fixture[f"{key}_{k}"]), (key, k)
            assert [r["G1"], r["G2"], r["G3"]] == fixture[key + "_gmae"].tolist(), key
        rt = d["ratio"]
        assert same([rt[k] for k in ("GT", "Pred", "AbsDiff", "Accuracy", "AccuracyRelative", "AccuracyRelativePD")],
                    fixture[f"sc_{name}_{n}_ratio"])
        if K == 4:
            keys = ("cellAccuracy", "immuneAccuracy", "tumorAccuracy", "GTImmo", "PredImmo", "AccuracyImmo", "GTImmoTummor",
                    "PredImmoTummor", "AccuracyImmoTummor")
            assert same([d["ratio3"][k] for k in keys], fixture[f"sc_{name}_{n}_ratio3"])
        else:
            assert "ratio3" not in d


@pytest.mark.parametrize("name", [n for n in SCORE_CASES if n not in RAISES])
def test_numpy_scoring_equals_the_reference(fixture, name):
    from umi import matching as M
    mask, dots, K = G.score_case(name)
    got = M.score_multiclass_numpy(mask, dots, K, G.SIGMAS, G.THRESHOLDS)
    assert len(got) == mask.shape[0]
    check_scores(fixture, name, got, K)


def test_prediction_without_class_1_or_2_raises(fixture):
    from umi import matching as M
    mask, dots, K = G.score_case("k3_no_pred_12")
    assert np.isnan(fixture["sc_k3_no_pred_12_0_ratio"]).all()             # the generator met ZeroDivisionError too
    with pytest.raises(ZeroDivisionError):
        M.score_multiclass_numpy(mask, dots, K, G.SIGMAS, G.THRESHOLDS)
    with pytest.raises(ZeroDivisionError):
        M.ratio_metrics(3, 4, 0, 0)


def test_empty_ground_truth_ratio_is_nan_and_differences_do_not_wrap(fixture):
    from umi import matching as M
    mask, dots, K = G.score_case("k3_no_gt_12")
    d = M.score_multiclass_numpy(mask, dots, K, G.SIGMAS, G.THRESHOLDS)[0]
    assert math.isnan(d["ratio"]["GT"]) and not math.isnan(d["ratio"]["Pred"])
    assert d[1]["GT"] == 0 and d[1]["Pred"] > 0 and d[1]["AbsDiff"] == d[1]["Pred"]          # an int, not 2**64 - Pred
    mask, dots, K = G.score_case("k3_more_pred")
    d = M.score_multiclass_numpy(mask, dots, K, G.SIGMAS, G.THRESHOLDS)[0]
    for c in (1, 2):
        assert 0 < d[c]["GT"] < d[c]["Pred"] and d[c]["AbsDiff"] == d[c]["Pred"] - d[c]["GT"]


def test_split_and_center_lists_numpy():
    from umi import matching as M
    from umi.components import label_class_components_numpy
    mask, dots, K = G.score_case("k4_64")
    planes = M.split_classes(dots, K)
    assert planes.shape == (2, 3, 64, 64) and planes.dtype == np.uint8
    for c in (1, 2, 3):
        assert np.array_equal(planes[:, c - 1], (dots == c).astype(np.uint8))
    _, counts, class_counts, label_class, area, sum_y, sum_x = label_class_components_numpy(mask, K)
    centers, c_count = M.class_center_lists(counts, label_class, area, sum_y, sum_x, K)
    assert c_count.tolist() == class_counts[:, 1:].reshape(-1).tolist()
    allc = M.component_centers_numpy(counts, area, sum_y, sum_x)
    for n in range(2):
        for c in (1, 2, 3):
            j = n * 3 + c - 1
            assert np.array_equal(centers[j, :c_count[j]], allc[n, np.flatnonzero(label_class[n] == c)])
            assert not centers[j, c_count[j]:].any()
