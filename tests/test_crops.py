"""CPU: the statement side of the crop datasets (umi.augment CropPool / CropTransform / CropBatches) against the reference's
arithmetic recorded in tests/golden/crop_batches.npz (tools/gen_golden_crops.py: SciPy's rotate, np.pad, NumPy's mean / std), the
reference's order of random draws, the pad-value rule, the bound of the exact uint8 statistics, the loader, and the refusals."""
import math
import os
import random

import numpy as np
import pytest
import torch

from oracle import recipe, ref_unet
from tools import gen_golden_crops as G
from umi import augment as A

CROP = G.CROP


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "crop_batches.npz"))


@pytest.fixture(scope="module")
def pools():
    return {name: G.pool(name) for name in G.POOLS}


# ---- the statements against the recorded reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.POOLS))
def test_crop_statement_equals_the_recorded_training_samples(golden, pools, name):
    """Bit for bit, the image included: the statement takes the float64 np.mean / np.std of the very array the reference takes
    them of (a float32 pool's images enter the recorded reference widened to float64, see tools/gen_golden_crops.py)."""
    images, labels, dots = pools[name]
    crops, params = golden[f"train_{name}_crops"], golden[f"train_{name}_params"]
    assert set(params[:, 0]) == {0, 1, 2}
    for s, row in enumerate(crops):
        i = row[0]
        x, (lab,), d = A.crop_transform_numpy(images[i], [labels[i]], row, params[s], CROP, dots=dots[i])
        want = golden[f"train_{name}_x_{s}"]
        assert x.dtype == np.float32 and x.shape == want.shape == ((3 if images[i].ndim == 3 else 1), CROP, CROP)
        assert lab.dtype == np.int64 and d.dtype == np.uint8
        np.testing.assert_array_equal(lab, golden[f"train_{name}_label_{s}"], err_msg=f"{name} {s}")
        np.testing.assert_array_equal(d, golden[f"train_{name}_dots_{s}"], err_msg=f"{name} {s}")
        np.testing.assert_array_equal(x, want, err_msg=f"{name} {s}")


@pytest.mark.parametrize("name", list(G.POOLS))
def test_grid_statement_equals_the_recorded_validation_items(golden, pools, name):
    """Labels and dots exactly; the image within 2e-6, the bar tests/test_gpu_augment.py derives for this formula.  It is not
    bit-equal by construction: the statement forms mean and std from exact integer sums (uint8) or from the source's sums plus a
    closed-form pad term (float32), as the kernels do, and NumPy's pairwise float64 sums over the padded array round differently
    in the last float64 bits, which can move a float32 result by one ulp."""
    images, labels, dots = pools[name]
    for (top, left), i in zip(golden[f"val_{name}_pads"], G.VAL_IMAGES[name]):
        x, (lab,), d = A.grid_transform_numpy(images[i], [labels[i]], top, left, CROP, CROP, dots=dots[i])
        want = golden[f"val_{name}_{i}_x"]
        assert x.dtype == np.float32 and x.shape == want.shape and lab.dtype == np.int64 and d.dtype == np.uint8
        np.testing.assert_array_equal(lab, golden[f"val_{name}_{i}_label"])
        np.testing.assert_array_equal(d, golden[f"val_{name}_{i}_dots"])
        np.testing.assert_allclose(x, want, rtol=0, atol=2e-6, err_msg=f"{name} {i}")
        # preprocessCrop: centred, 255 whatever the rank, the whole padded image as one tile
        want = golden[f"center_{name}_{i}_x"]
        Hp, Wp = want.shape[2:]
        x, _, _ = A.grid_transform_numpy(images[i], [], *A.center_pad(*images[i].shape[:2], CROP), Hp, Wp, pad_value=255)
        assert x.shape == want.shape
        np.testing.assert_allclose(x, want, rtol=0, atol=2e-6, err_msg=f"{name} {i} center")


@pytest.mark.parametrize("name", list(G.POOLS))
def test_draws_are_the_references_in_order_and_leave_the_generators_where_it_does(golden, pools, name):
    images = pools[name][0]
    sizes = [im.shape[:2] for im in images]
    random.seed(G.SEEDS[name][0])
    np.random.seed(G.SEEDS[name][1])
    crops, params = A.draw_crop_params(sizes, CROP, True, indices=G.TRAIN_INDICES[name])
    assert crops.dtype == np.int32 and crops.shape == (len(G.TRAIN_INDICES[name]), 3) and params.dtype == np.int32
    np.testing.assert_array_equal(crops, golden[f"train_{name}_crops"])
    np.testing.assert_array_equal(params, golden[f"train_{name}_params"])
    assert [random.random(), np.random.random()] == golden[f"train_{name}_next"].tolist()
    pads = [A.draw_pad(*sizes[i], CROP) for i in G.VAL_IMAGES[name]]
    np.testing.assert_array_equal(np.array(pads), golden[f"val_{name}_pads"])
    assert random.random() == golden[f"val_{name}_next"][0]


def test_draws_with_a_crop_equal_to_the_image_and_without_augmentation():
    """H == crop: randint(0, 0) is still drawn (one generator step each), and so are the pads of an image that needs none."""
    a, b = random.Random(5), random.Random(5)
    crops, params = A.draw_crop_params([(16, 16), (16, 40)], 16, False, a, None)
    assert crops[:, 1].tolist() == [0, 0] and crops[0, 2] == 0 and not params.any()
    want = [b.randint(0, 0), b.randint(0, 0), b.randint(0, 0), b.randint(0, 24)]
    assert crops[1, 2] == want[3] and a.random() == b.random()
    assert A.draw_pad(32, 48, 16, a) == (0, 0) and (b.randint(0, 0), b.randint(0, 0)) == (0, 0) and a.random() == b.random()
    assert A.center_pad(70, 41, 32) == (13, 11) and A.center_pad(64, 64, 32) == (0, 0)
    # the whole pool in order when no indices are given, each generator of one's own
    c1, p1 = A.draw_crop_params([(30, 30), (40, 20)], 16, True, random.Random(1), np.random.RandomState(2))
    c2, p2 = A.draw_crop_params([(30, 30), (40, 20)], 16, True, random.Random(1), np.random.RandomState(2))
    assert c1[:, 0].tolist() == [0, 1] and (c1 == c2).all() and (p1 == p2).all()


def test_pad_value_rule_255_for_hwc_and_0_for_hw():
    rng = np.random.default_rng(3)
    hwc = (rng.random((20, 27, 3)) * 200).astype(np.uint8)
    hw = hwc[..., 0].copy()
    for img, rule, other in ((hwc, 255, 0), (hw, 0, 255)):
        x, _, _ = A.grid_transform_numpy(img, [], 5, 2, 16, 16)
        same, _, _ = A.grid_transform_numpy(img, [], 5, 2, 16, 16, pad_value=rule)
        diff, _, _ = A.grid_transform_numpy(img, [], 5, 2, 16, 16, pad_value=other)
        np.testing.assert_array_equal(x, same)
        assert not np.array_equal(x, diff)
        # tile 0's corner pixel is padding: the normalised pad value
        mean, std = A.padded_statistics(img, 32 * 32 - 20 * 27, rule)
        np.testing.assert_allclose(x[0, :, 0, 0], ((rule - mean) / std)[::-1], rtol=0, atol=2e-6)
    # labels and dots are padded with 0 whatever the image
    lab = np.full((20, 27), 2, np.uint8)
    _, (l,), d = A.grid_transform_numpy(hwc, [lab], 5, 2, 16, 16, dots=lab)
    assert l[0, 0, 0] == 0 and d[0, 0, 0] == 0 and l[0, 5, 2] == 2 and d[0, 5, 2] == 2 and l.sum() == 2 * 20 * 27


def test_exact_uint8_statistics_up_to_their_bound_and_refusal_beyond_it():
    """(255 n)^2 < 2^64 up to n = 16,843,009: an all-255 image of 4096^2 has n * S2 - S1^2 == 0 exactly (mean 255, std 0), and with
    the 65,793 pad pixels of value 0 that reach the bound, n * S2 - S1^2 = 255^2 * m * npad, still exact in 64 bits."""
    assert A.U8_STAT_PIXELS == 16843009 and (255 * A.U8_STAT_PIXELS) ** 2 < 2 ** 64 <= (255 * (A.U8_STAT_PIXELS + 1)) ** 2
    img = np.full((4096, 4096), 255, np.uint8)
    mean, std = A.padded_statistics(img, 0, 255)
    assert mean.tolist() == [255.0] and std.tolist() == [0.0]
    m, npad = 4096 * 4096, A.U8_STAT_PIXELS - 4096 * 4096
    n = m + npad
    mean, std = A.padded_statistics(img, npad, 0)
    assert n * 255 * 255 * m < 2 ** 64
    assert mean.tolist() == [255 * m / n] and std.tolist() == [math.sqrt(255 * 255 * m * npad) / n]
    with pytest.raises(ValueError, match="16843009"):
        A.padded_statistics(img, npad + 1, 0)
    with pytest.raises(ValueError, match="16843009"):
        A.grid_transform_numpy(np.zeros((4105, 4105), np.uint8), [], 0, 0, 4105, 4105)
    # the C ABI refuses the same sizes before any launch: UMI_ERR_UNSUPPORTED
    from umi import lib
    p = 4096
    assert lib.fn("umi_grid_znorm")(p, 0, 4105, 4105, 1, 0, 0, 0, 4105, 4105, 4105, 4105, p, 0, p, 1 << 20, None) == -2
    assert lib.fn("umi_crop_znorm")(p, 0, p, p, 1, 1 << 40, 1, p, p, p, 1, 4105, p, 0, p, 1 << 20, None) == -2


# ---- the pool and the loader -------------------------------------------------------------------------------------------------------
def _pool(name, pools, dots=True):
    images, labels, dts = pools[name]
    return A.CropPool(images, labels, dts if dots else None)


def test_pool_packs_images_of_different_sizes(pools):
    pool = _pool("rgb", pools)
    images, labels, dots = pools["rgb"]
    assert len(pool) == 3 and pool.sizes.dtype == np.int32 and pool.sizes.tolist() == [[26, 35], [21, 21], [38, 27]]
    assert pool.C == 3 and pool.hwc and pool.images.dtype == torch.uint8 and pool.images.dim() == 1 and not pool.is_cuda
    assert pool.offsets.tolist() == [0, 26 * 35 * 3, (26 * 35 + 21 * 21) * 3] and pool.map_offsets.tolist() == [0, 910, 1351]
    for i in range(3):
        np.testing.assert_array_equal(pool.image(i).numpy(), images[i])
        np.testing.assert_array_equal(pool.label(i).numpy(), labels[i])
        np.testing.assert_array_equal(pool.dot(i).numpy(), dots[i])
    gray = A.CropPool([torch.from_numpy(a) for a in pools["gray"][0]], pools["gray"][1])
    assert gray.C == 1 and not gray.hwc and gray.dots is None and gray.dot(0) is None
    assert _pool("f32", pools).images.dtype == torch.float32
    assert pool.to("cpu").images.data_ptr() == pool.images.data_ptr()


def test_crop_transform_on_a_cpu_pool_runs_the_statement(golden, pools):
    pool = _pool("rgb", pools)
    tf = A.CropTransform(CROP, True)
    x, lab, dots = tf(pool, golden["train_rgb_crops"], golden["train_rgb_params"])
    assert x.shape == (8, 3, CROP, CROP) and x.dtype == torch.float32 and lab.dtype == torch.int64 and dots.dtype == torch.uint8
    for s in range(8):
        np.testing.assert_array_equal(x[s].numpy(), golden[f"train_rgb_x_{s}"])
        np.testing.assert_array_equal(lab[s].numpy(), golden[f"train_rgb_label_{s}"])
        np.testing.assert_array_equal(dots[s].numpy(), golden[f"train_rgb_dots_{s}"])
    # crops=None draws for `indices` from the global generators, like the reference
    random.seed(G.SEEDS["rgb"][0])
    np.random.seed(G.SEEDS["rgb"][1])
    x2, lab2, _ = tf(pool, indices=G.TRAIN_INDICES["rgb"])
    assert torch.equal(x2, x) and torch.equal(lab2, lab)
    top, left = golden["val_rgb_pads"][1]
    gx, gl, gd = tf.grid(pool, 2, (top, left))
    np.testing.assert_array_equal(gl.numpy(), golden["val_rgb_2_label"])
    np.testing.assert_array_equal(gd.numpy(), golden["val_rgb_2_dots"])
    np.testing.assert_allclose(gx.numpy(), golden["val_rgb_2_x"], rtol=0, atol=2e-6)
    cx, _, _ = tf.grid(pool, 2, "center")
    want, _, _ = A.grid_transform_numpy(pools["rgb"][0][2], [], *A.center_pad(38, 27, CROP), CROP, CROP)
    np.testing.assert_array_equal(cx.numpy(), want)
    # the regression datasets' labels
    xr, lr = A.CropTransform(CROP, False, label_scale=200.0, label_dtype=torch.float32)(_pool("gray", pools, dots=False),
                                                                                         [[0, 3, 4], [2, 22, 11]])
    assert lr.dtype == torch.float32 and float(lr.max()) == 400.0 and xr.shape == (2, 1, CROP, CROP)


def test_crop_batches_lengths_shapes_and_dtypes(pools):
    pool = _pool("rgb", pools)
    train = A.CropBatches(pool, CROP, 2, True, train=True)
    assert len(train) == 2
    items = list(train)
    assert [tuple(x.shape) for x, _ in items] == [(2, 3, CROP, CROP), (1, 3, CROP, CROP)]             # drop_last=False
    assert all(x.dtype == torch.float32 and y.dtype == torch.int64 and tuple(y.shape) == (x.shape[0], CROP, CROP) for x, y in items)
    val = A.CropBatches(pool, CROP, 2, True, train=False)
    assert len(val) == 3 and val.transform.augmentation is False
    assert [tuple(x.shape) for x, _ in val] == [(6, 3, CROP, CROP), (4, 3, CROP, CROP), (6, 3, CROP, CROP)]
    assert all(tuple(y.shape) == (x.shape[0], CROP, CROP) and y.dtype == torch.int64 for x, y in val)
    dots = list(A.CropBatches(pool, CROP, 3, False, train=True, with_dots=True))
    assert len(dots) == 1 and len(dots[0]) == 3 and dots[0][2].dtype == torch.uint8 and tuple(dots[0][2].shape) == (3, CROP, CROP)
    vd = list(A.CropBatches(pool, CROP, 3, False, train=False, with_dots=True, indices=[1]))
    assert len(vd) == 1 and tuple(vd[0][2].shape) == (4, CROP, CROP) and vd[0][2].dtype == torch.uint8
    # a shard, and a seeded shuffle that permutes the images
    shard = A.CropBatches(pool, CROP, 4, False, train=True, indices=[2, 0])
    assert len(shard) == 1 and tuple(next(iter(shard))[0].shape) == (2, 3, CROP, CROP)
    seen = []

    class Spy(A.CropTransform):
        def __call__(self, pool, crops=None, params=None, geom=None, indices=None):
            seen.extend(int(i) for i in indices)
            return super().__call__(pool, crops, params, geom, indices)

    sh = A.CropBatches(pool, CROP, 2, False, train=True, shuffle=True, generator=torch.Generator().manual_seed(1))
    sh.transform = Spy(CROP, False)
    list(sh)
    assert seen == torch.randperm(3, generator=torch.Generator().manual_seed(1)).tolist()


class _Epochs:
    """A plain list of batches per epoch, handed out epoch after epoch."""

    def __init__(self, per_epoch):
        self.per_epoch, self.k = per_epoch, 0

    def __len__(self):
        return len(self.per_epoch[0])

    def __iter__(self):
        self.k += 1
        return iter(self.per_epoch[self.k - 1])


def _tiny_run(tmp_path, name, loaders, **kw):
    import loss as L
    from Trainer import Trainer
    torch.manual_seed(0)
    L.CLASS_NUMBER = 3
    m = ref_unet.RefUNet(3, 3, 4, False)
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=3))
    opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9)
    tr = Trainer(m, "single", torch.FloatTensor, "cpu", str(tmp_path / name), loaders, 2, opt, 25, 2, "dice_bce_mc", "dice_bce_mc",
                 **kw)
    tr.train()
    return tr


def test_trainer_on_crop_batches_equals_the_statements_batches(tmp_path, pools):
    """Two epochs of Trainer on CropBatches of a CPU pool (train: random crops with augmentation; val: the tile stacks under
    drawn pads) == two epochs on plain lists of the statement's batches made from the same draws in the same order."""
    images, labels, _ = pools["rgb"]
    pool = _pool("rgb", pools, dots=False)
    random.seed(11)
    np.random.seed(12)
    got = _tiny_run(tmp_path, "loader", {"train": A.CropBatches(pool, CROP, 2, True, train=True, indices=[0, 1, 2, 1]),
                                         "val": A.CropBatches(pool, CROP, 2, True, train=False, indices=[1, 2])})
    random.seed(11)
    np.random.seed(12)
    train, val = [], []
    for _ in range(2):                                            # an epoch: the train batches' draws, then the val pads
        batches = []
        for chunk in ([0, 1], [2, 1]):
            crops, params = A.draw_crop_params(pool.sizes, CROP, True, indices=chunk)
            out = [A.crop_transform_numpy(images[r[0]], [labels[r[0]]], r, p, CROP) for r, p in zip(crops, params)]
            batches.append((torch.from_numpy(np.stack([o[0] for o in out])), torch.from_numpy(np.stack([o[1][0] for o in out]))))
        train.append(batches)
        items = []
        for i in (1, 2):
            top, left = A.draw_pad(*pool.sizes[i], CROP)
            x, (lab,), _ = A.grid_transform_numpy(images[i], [labels[i]], top, left, CROP, CROP)
            items.append((torch.from_numpy(x), torch.from_numpy(lab)))
        val.append(items)
    want = _tiny_run(tmp_path, "lists", {"train": _Epochs(train), "val": _Epochs(val)})
    assert len(got.train_loss_list) == 2 and np.isfinite(got.train_loss_list).all() and np.isfinite(got.val_loss_list).all()
    assert got.train_loss_list == want.train_loss_list
    assert got.val_loss_list == want.val_loss_list
    assert got.val_score_list == want.val_score_list
    assert got.train_loss_list[0] != got.train_loss_list[1]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_bad_tables_raise_value_error(pools):
    pool = _pool("rgb", pools)
    tf = A.CropTransform(CROP, False)
    for rows in ([[3, 0, 0]], [[-1, 0, 0]], [[0, 11, 0]], [[0, 0, 20]], [[1, -1, 0]], [[2, 22, 12]], [[0, 0]]):
        with pytest.raises(ValueError):
            tf(pool, np.array(rows, np.int32))
    tf(pool, np.array([[0, 10, 19], [2, 22, 11]], np.int32))                                       # the last windows that fit
    with pytest.raises(ValueError, match="parameters"):
        tf(pool, np.array([[0, 0, 0]], np.int32), np.zeros((2, 4), np.int32))
    with pytest.raises(ValueError, match="smaller than the crop"):
        A.draw_crop_params(pool.sizes, 24, False)
    with pytest.raises(ValueError, match="outside the pool"):
        A.draw_crop_params(pool.sizes, CROP, False, indices=[3])
    with pytest.raises(ValueError):
        A.CropBatches(pool, 24, 2, False, train=True)
    with pytest.raises(ValueError):
        A.CropBatches(_pool("rgb", pools, dots=False), CROP, 2, False, train=True, with_dots=True)
    # 38x27 -> 48x32: pad_top 0 .. 10; 26x35 -> 32x48: pad_left 0 .. 13
    for index, pad in ((2, (11, 0)), (0, (0, 14)), (1, (-1, 0)), (1, "middle")):
        with pytest.raises(ValueError):
            tf.grid(pool, index, pad)
    tf.grid(pool, 2, (10, 5))
    tf.grid(pool, 0, (6, 13))
    with pytest.raises(ValueError):
        tf.grid(pool, 3)
    # pools: one channel count and dtype, maps of the images' sizes, tables inside the buffers
    images, labels, dots = pools["rgb"]
    with pytest.raises(ValueError, match="one channel count"):
        A.CropPool([images[0], pools["gray"][0][0]], labels[:2])
    with pytest.raises(ValueError, match="its map"):
        A.CropPool(images[:2], [labels[0], labels[0]])
    with pytest.raises(ValueError):
        A.CropPool(images, labels[:2])
    with pytest.raises(ValueError, match="dot map"):
        A.CropPool(images, labels, [d.astype(np.float32) for d in dots])
    buf, maps = torch.zeros(3000, dtype=torch.uint8), torch.zeros(1000, dtype=torch.uint8)
    A.CropPool.from_buffers(buf, [0], [(25, 40)], 3, True, maps, [0])
    for off, sizes, moff in (([1], [(25, 40)], [0]), ([0], [(25, 41)], [0]), ([0], [(25, 40)], [1]), ([-1], [(20, 20)], [0]),
                             ([0, 0], [(25, 40)], [0]), ([0], [(0, 40)], [0])):
        with pytest.raises(ValueError):
            A.CropPool.from_buffers(buf, off, sizes, 3, True, maps, moff)
    with pytest.raises(ValueError, match="channels"):
        A.CropPool.from_buffers(buf, [0], [(10, 10)], 5, True, maps, [0])


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """Null pointers, sizes <= 0, C > 4, a pad outside the frame and tiles that do not divide it return UMI_ERR_BADARG (-1)
    without touching a GPU; a missing workspace UMI_ERR_WORKSPACE (-3)."""
    from umi import lib
    cz, cl = lib.fn("umi_crop_znorm"), lib.fn("umi_crop_labels")
    gz, gl = lib.fn("umi_grid_znorm"), lib.fn("umi_grid_labels")
    p = 4096                                                    # any non-null address: rejected before it is used
    ok = [p, 0, p, p, 3, 10000, 3, p, p, p, 2, 16, p, 1, p, 1 << 20, None]
    for pos in (0, 2, 3, 7, 8, 9, 12):                          # pool, offsets, sizes, crops, params, geom, out
        assert cz(*[None if i == pos else a for i, a in enumerate(ok)]) == -1, pos
    for pos, bad in ((1, 2), (4, 0), (5, 0), (6, 5), (6, 0), (10, 0), (11, 0)):
        assert cz(*[bad if i == pos else a for i, a in enumerate(ok)]) == -1, pos
    assert cz(*[None if i == 14 else 0 if i == 15 else a for i, a in enumerate(ok)]) == -3
    assert cz(*[8 if i == 15 else a for i, a in enumerate(ok)]) == -3
    okl = [p, 0, p, p, 3, 10000, p, p, p, 2, 16, p, 1, 1.0, None]
    for pos in (0, 2, 3, 6, 7, 8, 11):
        assert cl(*[None if i == pos else a for i, a in enumerate(okl)]) == -1, pos
    assert cl(*[3 if i == 12 else a for i, a in enumerate(okl)]) == -1                       # dst_dtype
    assert cl(*[1 if i == 1 else 2 if i == 12 else a for i, a in enumerate(okl)]) == -1      # float32 pool -> uint8
    okg = [p, 0, 70, 41, 3, 13, 11, 255, 96, 64, 32, 32, p, 1, p, 1 << 20, None]
    for pos in (0, 12):
        assert gz(*[None if i == pos else a for i, a in enumerate(okg)]) == -1, pos
    for pos, bad in ((1, 2), (2, 0), (4, 5), (5, 27), (5, -1), (6, 24), (7, 256), (8, 64), (10, 40), (11, 0)):
        assert gz(*[bad if i == pos else a for i, a in enumerate(okg)]) == -1, (pos, bad)
    assert gz(*[None if i == 14 else a for i, a in enumerate(okg)]) == -3
    okgl = [p, 0, 70, 41, 13, 11, 96, 64, 32, 32, p, 1, 1.0, None]
    for pos in (0, 10):
        assert gl(*[None if i == pos else a for i, a in enumerate(okgl)]) == -1, pos
    for pos, bad in ((4, 27), (7, 63), (8, 36), (11, 3)):
        assert gl(*[bad if i == pos else a for i, a in enumerate(okgl)]) == -1, (pos, bad)
    assert lib.fn("umi_crop_znorm_ws_bytes")(0) == 0 and lib.fn("umi_crop_znorm_ws_bytes")(2) > 0
    assert lib.fn("umi_grid_znorm_ws_bytes")() > 0
