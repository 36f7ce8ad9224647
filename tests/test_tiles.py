"""CPU: the tile plans of umi.tiles, the reflect rule against numpy.pad, and the NumPy statement of the three tile kernels
(gather / blend / finish): chunk invariance, overlap-tile exactness with poisoned halos, the float64 rounding bound; and the
argument checks of the C entry points, which answer before any launch."""
import ctypes

import numpy as np
import pytest

from umi import tiles as T
from umi.tiles import TilePlan


# ---- plans ------------------------------------------------------------------------------------------------------------------------
def test_sliding_origins_examples():
    assert TilePlan.sliding(70, 70, 32, 8).oy.tolist() == [0, 24, 38]
    assert TilePlan.sliding(10, 10, 16, 0).oy.tolist() == [-3]
    assert TilePlan.sliding(64, 64, 32, 16).oy.tolist() == [0, 16, 32]
    p = TilePlan.sliding(70, 10, 32, 8)
    assert p.oy.tolist() == [0, 24, 38] and p.ox.tolist() == [-11] and (p.ny, p.nx, p.n_tiles) == (3, 1, 3)
    assert TilePlan.sliding(32, 33, 32, 31).ox.tolist() == [0, 1]
    assert TilePlan.sliding(32, 32, 32, 5).oy.tolist() == [0]


def test_overlap_tile_origins_and_cores_partition_the_canvas():
    p = TilePlan.overlap_tile(70, 90, 32, 4)
    assert p.oy.tolist() == [-4, 20, 44] and p.ox.tolist() == [-4, 20, 44, 68]
    assert TilePlan.overlap_tile(64, 96, 32, 0).oy.tolist() == [0, 32] and TilePlan.overlap_tile(64, 96, 32, 0).ox.tolist() == [0, 32, 64]
    for H, tile, halo in ((70, 32, 4), (70, 32, 0), (70, 32, 8), (1, 5, 2), (37, 16, 7), (33, 32, 15)):
        p = TilePlan.overlap_tile(H, H + 3, tile, halo)
        for o, n, w, s in ((p.oy, p.H, p.wy, p.sy), (p.ox, p.W, p.wx, p.sx)):
            cover = np.zeros(n, dtype=np.int64)
            for a in o:
                core = np.arange(a + halo, a + tile - halo)
                core = core[(core >= 0) & (core < n)]
                cover[core] += 1
            assert (cover == 1).all()                                   # the cores partition the axis
            assert s.dtype == np.float32 and (s == 1).all()             # so every window sum is exactly 1
            assert w.tolist() == [0.0] * halo + [1.0] * (tile - 2 * halo) + [0.0] * halo


def test_window_tables_and_sums():
    p = TilePlan.sliding(70, 50, 32, 8)
    i = np.arange(32, dtype=np.float64)
    want = np.exp(-0.5 * ((i - 15.5) / (0.125 * 32)) ** 2)
    assert p.wy.dtype == np.float32 and np.array_equal(p.wy, want.astype(np.float32))
    s = np.zeros(70)
    for o in (0, 24, 38):
        s[o:o + 32] += p.wy.astype(np.float64)
    assert np.array_equal(p.sy, s.astype(np.float32))
    flat = TilePlan.sliding(70, 50, 32, 8, window="flat")
    assert (flat.wy == 1).all() and flat.sy[:24].tolist() == [1.0] * 24 and flat.sy[24:32].tolist() == [2.0] * 8
    assert flat.sy[38:56].tolist() == [2.0] * 18
    assert TilePlan.sliding(70, 50, 32, 8).chunks(8).tolist() == [[0, 1, 2, 3, 4, 5, -1, -1]]
    assert TilePlan.sliding(70, 50, 32, 8).chunks(3).tolist() == [[0, 1, 2], [3, 4, 5]]


def test_plan_refusals():
    with pytest.raises(ValueError):
        TilePlan.overlap_tile(70, 70, 32, 16)                            # T - 2 halo < 1
    with pytest.raises(ValueError):
        TilePlan.overlap_tile(70, 70, 32, -1)
    with pytest.raises(ValueError):
        TilePlan.sliding(70, 70, 32, 32)
    with pytest.raises(ValueError):
        TilePlan.sliding(70, 70, 32, -1)
    with pytest.raises(ValueError):
        TilePlan.sliding(70, 70, 32, 8, window="hann")
    with pytest.raises(ValueError):
        TilePlan.sliding(70, 70, 32, 8, pad="edge")
    one = np.ones(8)
    for bad in (np.nan, np.inf, -1.0):
        w = one.copy()
        w[3] = bad
        with pytest.raises(ValueError):
            TilePlan(16, 16, 8, [0, 8], [0, 8], w, one)
        with pytest.raises(ValueError):
            TilePlan(16, 16, 8, [0, 8], [0, 8], one, w)
    with pytest.raises(ValueError):
        TilePlan(17, 16, 8, [0, 8], [0, 8], one, one)                    # row 16 is in no tile: sy[16] = 0
    with pytest.raises(ValueError):
        w = one.copy()
        w[0] = 0.0
        TilePlan(16, 16, 8, [0, 8], [0, 8], one, w)                      # column 0 only meets a zero weight
    with pytest.raises(ValueError):
        TilePlan.sliding(64, 64, 32, 0, sigma_scale=1e-3)                # the window underflows to 0 at the tile edges
    with pytest.raises(ValueError):
        TilePlan.overlap_tile(5000, 5000, 4097, 0)                       # tile > 4096
    with pytest.raises(ValueError):
        TilePlan.overlap_tile(2000, 2000, 1, 0)                          # 2000 > 1024 tiles per axis
    with pytest.raises(ValueError):
        TilePlan.overlap_tile(46341, 46341, 4096, 0)                     # H * W >= 2^31
    with pytest.raises(ValueError):
        TilePlan(16, 16, 8, [0, 8], [0, 8], np.ones(7), one)
    with pytest.raises(ValueError):
        TilePlan.sliding(64, 64, 32, 0).chunks(65)


# ---- reflect rule -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 10, 37])
def test_reflect_index_is_numpy_pad_reflect(n):
    a = np.arange(n)
    for pad in (0, 1, 4, 9, 80):
        want = np.pad(a, (pad, pad), mode="reflect")
        got = [T.reflect_index(i, n) for i in range(-pad, n + pad)]
        assert got == want.tolist(), (n, pad)


# ---- gather -----------------------------------------------------------------------------------------------------------------------
def _plans(H, W, tile, **kw):
    """overlap_tile halo 0 (and 4), sliding overlap 0, T - 1 (and 8); `tile` = T or (th, tw)."""
    t = tile if np.isscalar(tile) else min(tile)
    out = [TilePlan.overlap_tile(H, W, tile, 0, **kw), TilePlan.sliding(H, W, tile, 0, **kw), TilePlan.sliding(H, W, tile, t - 1, **kw)]
    if t > 8:
        out += [TilePlan.overlap_tile(H, W, tile, 4, **kw), TilePlan.sliding(H, W, tile, 8, **kw)]
    return out


@pytest.mark.parametrize("pad", ["reflect", "constant"])
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 37, 53), (2, 10, 70)])
def test_gather_numpy_is_numpy_pad_and_slicing(shape, pad):
    C, H, W = shape
    x = np.random.default_rng(1).standard_normal(shape).astype(np.float32)
    for th, tw in ((16, 24), (5, 7)):
        for plan in _plans(H, W, (th, tw), pad=pad, pad_value=255.0):
            P = 2 * max(th, tw) + max(H, W)
            if pad == "reflect":
                big = np.pad(x, ((0, 0), (P, P), (P, P)), mode="reflect")
            else:
                big = np.pad(x, ((0, 0), (P, P), (P, P)), mode="constant", constant_values=255.0)
            ids = [plan.n_tiles - 1, -1] + list(range(plan.n_tiles))
            got = T.gather_numpy(x, plan, ids)
            assert got.dtype == np.float32 and got.shape == (len(ids), C, th, tw)
            for s, t in enumerate(ids):
                if t < 0:
                    assert not got[s].any()
                    continue
                oy, ox = plan.origin(t)
                assert np.array_equal(got[s], big[:, P + oy:P + oy + th, P + ox:P + ox + tw]), (th, tw, t)


# ---- blend + finish ---------------------------------------------------------------------------------------------------------------
def _logits(plan, K, seed):
    return np.random.default_rng(seed).standard_normal((plan.n_tiles, K, plan.th, plan.tw)).astype(np.float32)


@pytest.mark.parametrize("K", [1, 3])
def test_stitch_does_not_depend_on_the_chunking(K):
    for plan in _plans(37, 53, (16, 24)) + _plans(10, 70, (5, 7)) + [TilePlan.sliding(70, 90, 32, 16)]:
        lg = _logits(plan, K, 2)
        whole = T.stitch_numpy(lg, plan)
        assert whole.dtype == np.float32 and whole.shape == (K, plan.H, plan.W) and np.isfinite(whole).all()
        for chunk in (1, 3, 8):
            assert np.array_equal(T.stitch_numpy(lg, plan, chunk).view(np.uint32), whole.view(np.uint32)), chunk
        # empty slots between the ids change nothing
        acc = np.zeros((K, plan.H, plan.W), dtype=np.float32)
        ids = []
        for t in range(plan.n_tiles):
            ids += [t, -1]
        T.blend_numpy(acc, lg[np.maximum(ids, 0)], plan, ids)
        assert np.array_equal(T.finish_numpy(acc, plan).view(np.uint32), whole.view(np.uint32))


@pytest.mark.parametrize("halo", [0, 4, 8])
def test_overlap_tile_returns_the_tiles_own_values_and_no_halo_poison(halo):
    H, W, tile, K = 70, 90, 32, 2
    plan = TilePlan.overlap_tile(H, W, tile, halo)
    src = np.random.default_rng(3).standard_normal((K, H, W)).astype(np.float32)
    lg = T.gather_numpy(src, plan, list(range(plan.n_tiles)))
    poison = [np.inf, -np.inf, np.nan]
    for t in range(plan.n_tiles):                                        # every discarded halo pixel of every tile
        halo_px = np.ones((tile, tile), dtype=bool)
        halo_px[halo:tile - halo, halo:tile - halo] = False
        lg[t][:, halo_px] = poison[t % 3]
    for chunk in (1, 8, None):
        got = T.stitch_numpy(lg, plan, chunk)
        assert np.array_equal(got, src)                                 # as numbers (only the sign of a zero may differ)
        assert np.isfinite(got).all()


def test_sliding_gauss_within_the_rounding_bound_of_float64():
    """|fp32 statement - float64 sum(w l) / sum(w)| <= (n + 6) 2^-24 max|l|, n = tiles with w > 0 at the pixel: one rounding per
    weight product, per w * l and per add (n each, the first add to 0 is exact), against the exact weights; the denominator
    sy * sx carries one rounding per table entry and one for the product; one for the division."""
    for H, W, tile, ov in ((70, 90, 32, 16), (37, 53, 16, 15), (64, 64, 32, 8)):
        plan = TilePlan.sliding(H, W, tile, ov, window="gauss")
        lg = _logits(plan, 2, 4) * 8.0
        got = T.stitch_numpy(lg, plan, 3).astype(np.float64)
        ref, cover = T.stitch_float64(lg, plan)
        assert cover.min() >= 1
        bound = (cover + 6) * 2.0 ** -24 * np.abs(lg).max()
        err = np.abs(got - ref)
        print(f"sliding {H}x{W} tile {tile} overlap {ov}: max err {err.max():.3e}, min bound {bound.min():.3e}, "
              f"max err / bound {np.max(err / bound[None]):.3f}, cover up to {cover.max()}")
        assert (err <= bound[None]).all()


# ---- C ABI ------------------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_without_a_launch():
    from umi import lib
    buf = (ctypes.c_float * 16)()                                        # any non-null, 4-byte aligned address: nothing is launched
    p = ctypes.addressof(buf)
    BAD, UNS = lib.UMI_ERR_BADARG, lib.UMI_ERR_UNSUPPORTED
    gather, blend, finish = lib.fn("umi_tile_gather"), lib.fn("umi_tile_blend"), lib.fn("umi_tile_finish")

    def g(x=p, C=1, H=8, W=8, tiles=p, th=4, tw=4, oy=p, ox=p, ny=2, nx=2, ids=p, n=4, mode=0):
        return gather(x, C, H, W, tiles, th, tw, oy, ox, ny, nx, ids, n, mode, 0.0, None)

    def b(lg=p, K=1, th=4, tw=4, acc=p, H=8, W=8, oy=p, ox=p, ny=2, nx=2, wy=p, wx=p, ids=p, n=4):
        return blend(lg, K, th, tw, acc, H, W, oy, ox, ny, nx, wy, wx, ids, n, None)

    def f(acc=p, K=1, H=8, W=8, sy=p, sx=p, mask=None):
        return finish(acc, K, H, W, sy, sx, mask, None)

    for kw in ({"x": None}, {"tiles": None}, {"oy": None}, {"ox": None}, {"ids": None}, {"C": 0}, {"H": 0}, {"W": -1}, {"th": 0},
               {"tw": 0}, {"ny": 0}, {"nx": 0}, {"n": 0}, {"mode": 2}, {"x": p + 1}):
        assert g(**kw) == BAD, kw
    for kw in ({"lg": None}, {"acc": None}, {"oy": None}, {"ox": None}, {"wy": None}, {"wx": None}, {"ids": None}, {"K": 0}, {"H": 0},
               {"W": 0}, {"th": -1}, {"tw": 0}, {"ny": 0}, {"nx": 0}, {"n": 0}, {"acc": p + 2}):
        assert b(**kw) == BAD, kw
    for kw in ({"acc": None}, {"sy": None}, {"sx": None}, {"K": 0}, {"H": 0}, {"W": 0}):
        assert f(**kw) == BAD, kw
    big = {"th": 4097}, {"tw": 4097}, {"ny": 1025}, {"nx": 1025}, {"n": 65}
    for kw in big + ({"C": 2, "H": 32768, "W": 32768}, {"C": 128, "th": 4096, "tw": 4096, "n": 1}, {"C": 1024, "n": 64}):
        assert g(**kw) == UNS, kw
    for kw in big + ({"K": 2, "H": 32768, "W": 32768}, {"K": 128, "th": 4096, "tw": 4096, "n": 1}):
        assert b(**kw) == UNS, kw
    assert f(K=2, H=32768, W=32768) == UNS and f(K=257) == UNS
