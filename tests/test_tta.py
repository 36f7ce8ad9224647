"""CPU: the NumPy statement of test-time augmentation (umi/tta.py) -- the eight views against explicit np.rot90 / np.flip
compositions, their inverses, the index form the kernels restate, merging, masks, entropy, argument validation, and the status
codes of the three entry points of csrc/tta.hip for arguments they refuse before any launch."""
import ctypes

import numpy as np
import pytest

from umi import tta as T

SHAPES = [(1, 1), (3, 5), (4, 4)]


def _x(shape, lead=(2, 3), seed=0):
    return np.random.default_rng(seed).standard_normal(lead + shape).astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES)
def test_unview_inverts_view(shape):
    x = _x(shape)
    for e in range(8):
        v = T.view_numpy(x, e)
        assert v.shape == x.shape[:2] + T.view_shape(e, *shape) and v.flags["C_CONTIGUOUS"]
        assert np.array_equal(T.unview_numpy(v, e), x), e
        assert np.array_equal(T.view_numpy(T.unview_numpy(x.reshape(x.shape[:2] + T.view_shape(e, *shape)), e), e).ravel(),
                              x.ravel()), e


def test_the_eight_views_are_the_explicit_compositions():
    x = _x((3, 5))
    r = lambda k: np.rot90(x, k, axes=(2, 3))                      # noqa: E731
    want = [x, r(1), r(2), r(3), x[..., ::-1], np.flip(r(1), 3), np.flip(r(2), 3), np.flip(r(3), 3)]
    for e in range(8):
        assert np.array_equal(T.view_numpy(x, e), want[e]), e
    # what the four even elements are: identity, rot180, the mirror image left-right, the mirror image up-down
    assert np.array_equal(T.view_numpy(x, 2), x[..., ::-1, ::-1])
    assert np.array_equal(T.view_numpy(x, 6), x[..., ::-1, :])
    # all eight differ on a generic image, and a square image's eight views are its eight symmetries
    sq = _x((4, 4), lead=())
    assert len({T.view_numpy(sq, e).tobytes() for e in range(8)}) == 8
    assert {T.view_numpy(sq, e).tobytes() for e in range(8)} == \
        {np.rot90(m, k).tobytes() for m in (sq, sq.T) for k in range(4)}


@pytest.mark.parametrize("shape", SHAPES + [(2, 7)])
def test_the_index_form_is_the_view(shape):
    x = _x(shape, lead=())
    for e in range(8):
        ys, xs = T.view_source(e, *shape)
        assert ys.shape == T.view_shape(e, *shape)
        assert np.array_equal(x[ys, xs], T.view_numpy(x, e)), e


def test_view_sets_and_shapes():
    assert T.view_set("none") == (0,) and T.view_set("flips") == (0, 2, 4, 6) and T.view_set("d4") == tuple(range(8))
    assert T.view_set([3, 3, np.int64(1)]) == (3, 3, 1)
    x = _x((3, 5))
    for e in T.view_set("flips"):
        assert T.view_numpy(x, e).shape == x.shape and not T.transposes(e)
    for e in (1, 3, 5, 7):
        assert T.view_numpy(x, e).shape == (2, 3, 5, 3) and T.transposes(e)
    assert T.shape_classes("d4", 3, 5) == {(3, 5): [0, 2, 4, 6], (5, 3): [1, 3, 5, 7]}
    assert T.shape_classes("d4", 4, 4) == {(4, 4): list(range(8))}
    assert T.shape_classes((1, 0, 0, 3), 3, 5) == {(5, 3): [0, 3], (3, 5): [1, 2]}
    assert T.pack_elements((7, 0, 3)) == 7 + (3 << 8) and T.pack_elements((5,) * 16) == 0x5555555555555555


def test_argument_validation():
    for bad in ("D4", "all", (), (8,), (-1,), (0.0,), (True,), 3, None, ("0",)):
        with pytest.raises(ValueError):
            T.view_set(bad)
    with pytest.raises(ValueError):
        T.check_mode("softmax")
    with pytest.raises(ValueError):
        T.pack_elements((0,) * 17)
    y = _x((4, 4))
    with pytest.raises(ValueError):
        T.merge_numpy([y], (0, 1))
    with pytest.raises(ValueError):
        T.merge_numpy([y.astype(np.float64)], (0,))
    with pytest.raises(ValueError):
        T.merge_numpy([y[0]], (0,))
    with pytest.raises(ValueError):
        T.merge_numpy([_x((3, 5)), _x((3, 5))], (0, 1))             # the second one maps back to (5, 3)


def _pointwise(v):
    return (v * np.float32(3) - np.float32(0.5)).astype(np.float32)


@pytest.mark.parametrize("views", ["none", "flips", "d4", (1, 1, 6), (7,)])
@pytest.mark.parametrize("shape", [(3, 5), (4, 4)])
def test_merging_a_pointwise_function_returns_it_exactly(shape, views):
    """An equivariant network: every view's output maps back to the same array.  The values are multiples of 1/8 below 2^8, so
    every partial sum of up to 8 copies is exact in float32 and so is its division by the count: the mean is the value itself."""
    x = (np.random.default_rng(1).integers(-64, 65, size=(2, 3) + shape) / 8).astype(np.float32)
    els = T.view_set(views)
    outs = [_pointwise(T.view_numpy(x, e)) for e in els]
    got = T.merge_numpy(outs, els, "logit")
    assert got.dtype == np.float32 and got.shape == x.shape
    assert np.array_equal(got, _pointwise(x))
    relu = T.merge_numpy(outs, els, "relu")
    assert relu.dtype == np.float32 and np.array_equal(relu, np.maximum(_pointwise(x), 0))
    prob = T.merge_numpy([np.concatenate([o, -o], axis=1) for o in outs], els, "prob")
    assert prob.dtype == np.float64 and np.allclose(prob.sum(axis=1), 1.0, atol=1e-12)


def test_merge_is_the_ordered_float32_sum_and_repeats_count():
    rng = np.random.default_rng(3)
    els = (0, 5, 5, 2, 3)
    outs = [rng.standard_normal((1, 2) + T.view_shape(e, 3, 5)).astype(np.float32) * np.float32(10.0 ** i) for i, e in enumerate(els)]
    acc = np.zeros((1, 2, 3, 5), dtype=np.float32)
    for o, e in zip(outs, els):
        acc = (acc + T.unview_numpy(o, e)).astype(np.float32)
    assert np.array_equal(T.merge_numpy(outs, els), acc / np.float32(5))
    again = T.merge_numpy(outs[::-1], els[::-1])
    assert not np.array_equal(again, acc / np.float32(5))           # the order is part of the statement
    # a repeated element counts twice
    a, b = outs[1], outs[2]
    assert np.array_equal(T.merge_numpy([a, a], (5, 5)), T.unview_numpy(a, 5))
    assert not np.array_equal(T.merge_numpy([a, b], (5, 5)), T.unview_numpy(a, 5))


def test_relu_prob_mask_and_entropy_rules():
    y = np.array([-1.0, -0.0, 0.0, 2.0, np.nan, -np.inf, np.inf], dtype=np.float32).reshape(1, 1, 1, 7)
    r = T.merge_numpy([y], (0,), "relu")[0, 0, 0]
    assert r[0] == 0 and np.signbit(r[1]) == np.signbit(np.float32(-0.0) + np.float32(0)) and r[3] == 2 and np.isnan(r[4])
    assert r[5] == 0 and r[6] == np.inf
    p = T.merge_numpy([y], (0,), "prob")[0, 0, 0]
    assert p[2] == 0.5 and p[5] == 0 and p[6] == 1 and np.isnan(p[4]) and abs(p[3] - 1 / (1 + np.exp(-2.0))) < 1e-15
    assert T.mask_numpy(np.array([0.5, 0.49, np.nan]).reshape(1, 1, 1, 3), "prob").ravel().tolist() == [1, 0, 0]
    cut = T.BINARY_CUTOFF
    assert cut < 0 and cut.view(np.uint32) == 0xB43FFFFE
    lg = np.array([cut, np.nextafter(cut, np.float32(-1)), 0.0, np.nan], dtype=np.float32).reshape(1, 1, 1, 4)
    assert T.mask_numpy(lg, "logit").ravel().tolist() == [1, 0, 1, 0]
    # K >= 2: the first strict maximum wins, a NaN never wins, a NaN in channel 0 stays
    m = np.array([[1, 1, 0], [2, 2, 1], [np.nan, 5, 1], [0, np.nan, 3], [np.nan, np.nan, np.nan]], dtype=np.float32).T
    assert T.mask_numpy(m.reshape(1, 3, 1, 5), "logit").ravel().tolist() == [0, 0, 0, 2, 0]
    # entropy: uniform = log K, one-hot = 0 (0 log 0 = 0), K = 1 the binary entropy
    u = np.full((1, 4, 1, 1), 0.25)
    assert abs(T.entropy_numpy(u)[0, 0, 0] - np.log(4)) < 1e-15
    assert T.entropy_numpy(np.array([1.0, 0, 0]).reshape(1, 3, 1, 1))[0, 0, 0] == 0
    b = T.entropy_numpy(np.array([0.5, 0.0, 1.0, 0.25]).reshape(1, 1, 1, 4))[0, 0]
    assert abs(b[0] - np.log(2)) < 1e-15 and b[1] == 0 and b[2] == 0
    assert abs(b[3] + 0.25 * np.log(0.25) + 0.75 * np.log(0.75)) < 1e-15
    assert T.top_two_margin(np.array([0.2, 0.7, 0.1]).reshape(1, 3, 1, 1))[0, 0, 0] == pytest.approx(0.5)
    assert T.top_two_margin(np.array([0.2]).reshape(1, 1, 1, 1))[0, 0, 0] == pytest.approx(0.3)


def test_the_bounds_are_small_and_grow_with_their_arguments():
    b = T.prob_bound(9, 16, 40.0)
    assert 2.0 ** -24 * 90 < b < 1e-4 and T.prob_bound(9, 16, 41.0) > b and T.prob_bound(10, 16, 40.0) > b \
        and T.prob_bound(9, 17, 40.0) > b
    assert b < T.entropy_bound(9, b) < 2e-3


def test_the_statement_inputs_of_the_gpu_tests_meet_the_margin_cap():
    """tests/test_gpu_tta.py compares 'prob' masks where the statement's top-two margin exceeds twice the bound and demands that at
    most 1 % of the pixels are excluded: with its 4 x standard-normal logits (the very arrays, by seed) the statement alone meets
    that, for every shape, K and view set of its grid."""
    from tests import test_gpu_tta as G
    worst = 0.0
    for shape in G.SHAPES:
        N, _, H, W = shape
        for K in G.KS:
            for si, views in enumerate(G.SETS):
                els = T.view_set(views)
                outs = G._outputs(els, N, K, H, W, 2000 + 10 * K + si)
                bound = T.prob_bound(K, len(els), G._spread(outs, K))
                assert bound < 1e-5
                share = float((T.top_two_margin(T.merge_numpy(outs, els, "prob"), "prob") <= 2 * bound).mean())
                worst = max(worst, share)
                assert share <= 0.01, (shape, K, views, share)
    print(f"largest undecided share over the grid: {worst:.5f}")


# ---- the C ABI refuses before any launch (no GPU needed) -----------------------------------------------------------------------------
def test_entry_points_return_status_codes_with_nothing_launched():
    from umi import lib
    buf = (ctypes.c_float * 8)()                                     # a real, 16-byte-or-better aligned host address: never read
    p = ctypes.addressof(buf) & ~15
    views, acc, fin = lib.fn("umi_tta_views"), lib.fn("umi_tta_accumulate"), lib.fn("umi_tta_finish")
    BAD, UNS = lib.UMI_ERR_BADARG, lib.UMI_ERR_UNSUPPORTED
    e8 = T.pack_elements("d4")
    # null pointers
    assert views(None, 1, 1, 4, 4, p, e8, 8, None) == BAD and views(p, 1, 1, 4, 4, None, e8, 8, None) == BAD
    assert acc(None, 1, 2, 4, 4, p, e8, 8, 0, None) == BAD and acc(p, 1, 2, 4, 4, None, e8, 8, 0, None) == BAD
    assert fin(None, 1, 2, 4, 4, 8, 0, None, None, None) == BAD
    # K = 0, other non-positive sizes and counts, a misaligned pointer
    assert acc(p, 1, 0, 4, 4, p, e8, 8, 0, None) == BAD and fin(p, 1, 0, 4, 4, 8, 0, None, None, None) == BAD
    assert views(p, 1, 0, 4, 4, p, e8, 8, None) == BAD and views(p, 0, 1, 4, 4, p, e8, 8, None) == BAD
    assert fin(p, 1, 2, 4, 4, 0, 0, None, None, None) == BAD and views(p + 2, 1, 1, 4, 4, p, e8, 8, None) == BAD
    # element lists: V out of range, an element above 7, bits above the list, two shapes in one call
    assert views(p, 1, 1, 4, 4, p, e8, 0, None) == BAD and views(p, 1, 1, 4, 4, p, e8, 17, None) == BAD
    assert views(p, 1, 1, 4, 4, p, 8, 1, None) == BAD and views(p, 1, 1, 4, 4, p, e8, 7, None) == BAD
    assert views(p, 1, 1, 3, 5, p, e8, 8, None) == BAD and acc(p, 1, 2, 3, 5, p, T.pack_elements((0, 1)), 2, 0, None) == BAD
    # modes, entropy outside 'prob'
    assert acc(p, 1, 2, 4, 4, p, e8, 8, 3, None) == BAD and fin(p, 1, 2, 4, 4, 8, -1, None, None, None) == BAD
    assert fin(p, 1, 2, 4, 4, 8, 0, None, p, None) == BAD
    # oversize: K above 32, 2^31 elements, too many planes
    assert acc(p, 1, 33, 4, 4, p, e8, 8, 2, None) == UNS and fin(p, 1, 33, 4, 4, 8, 2, None, None, None) == UNS
    assert fin(p, 1, 2, 32768, 32768, 8, 0, None, None, None) == UNS
    assert acc(p, 1, 2, 16384, 16384, p, T.pack_elements((0, 2, 4, 6)), 4, 0, None) == UNS
    assert views(p, 1, 1, 65536, 32768, p, 0, 1, None) == UNS and views(p, 256, 256, 4, 4, p, 0, 1, None) == UNS
    assert acc(p, 65536, 1, 4, 4, p, 0, 1, 0, None) == UNS


def test_wrappers_refuse_host_tensors_and_bad_lists():
    import torch
    x = torch.zeros(1, 1, 4, 4)
    with pytest.raises(RuntimeError):
        T.views(x, "d4")
    with pytest.raises(ValueError):
        T.views(x, (9,))
    with pytest.raises(ValueError):
        T.finish(x, 8, "nope")
