"""GPU: the kernels of csrc/crops.hip (umi.augment CropPool / CropTransform / CropBatches, umi.infer.preprocess_crop) against
the NumPy statements of umi.augment, which tests/test_crops.py pins to the recorded reference on the CPU.  Labels, dots and
zero-fill are exact; the normalised image is within 2e-6 of the float64 statement, the bar tests/test_gpu_augment.py derives for
this formula (one float32 rounding of an fp64 value of magnitude <= ~10 is 5e-7, the rest is the summation order of the
statistics), with NaNs in the same places."""
import random

import numpy as np
import pytest
import torch

from oracle import recipe
from umi import augment as A

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATOL = 2e-6

# every geometry mode: identity, all eight (k, axis), the angles -20, -7, 3, 19
MODES = [(0, 0, 0, 0)] + [(1, k, axis, 0) for k in range(4) for axis in range(2)] + [(2, 0, 0, a) for a in (-20, -7, 3, 19)]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: torch.cuda.is_available() is False")


def _arrays(shapes, dtype, seed):
    """(images, class maps 0 .. 3, dot maps) of the given shapes, seeded."""
    rng = np.random.default_rng(seed)
    images, labels, dots = [], [], []
    for shape in shapes:
        img = rng.random(shape) * 255
        images.append(img.astype(np.uint8) if dtype == "uint8" else (img / 255 - 0.3).astype(np.float32))
        labels.append(rng.integers(0, 4, shape[:2]).astype(np.uint8))
        dots.append(((rng.random(shape[:2]) < 0.05) * 255).astype(np.uint8))
    return images, labels, dots


def _shapes(crop, hwc):
    """Widths that are no multiple of 4 or 64, one image equal to the crop, and the largest image last."""
    c = (3,) if hwc else ()
    return [(40, 52) + c, (33, 33) + c, (crop, crop) + c, (70, 41) + c]


def _rows(shapes, crop):
    """One crop row per geometry mode: the four corners of image 0, the whole of image 2, the corners of the last image (two
    crops of one image in a batch, more than once), an inner window of image 1."""
    H0, W0 = shapes[0][:2]
    H3, W3 = shapes[3][:2]
    places = [(0, 0, 0), (0, 0, W0 - crop), (0, H0 - crop, 0), (0, H0 - crop, W0 - crop), (2, 0, 0), (3, H3 - crop, W3 - crop),
              (3, 0, W3 - crop), (3, H3 - crop, 0), (1, 5, 7), (3, 11, 3), (0, 3, 9), (1, 33 - crop, 33 - crop), (3, 0, 0)]
    assert len(places) == len(MODES)
    return np.array(places, np.int32), np.array(MODES, np.int32)


def _statement(arrays, crops, params, crop, scale=1.0, ldt=np.int64):
    images, labels, dots = arrays
    out = [A.crop_transform_numpy(images[r[0]], [labels[r[0]]], r, p, crop, label_scale=scale, label_dtype=ldt, dots=dots[r[0]])
           for r, p in zip(crops, params)]
    return np.stack([o[0] for o in out]), np.stack([o[1][0] for o in out]), np.stack([o[2] for o in out])


def _close(got, want, msg=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == np.float32 and got.shape == want.shape, (got.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=msg)
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL, err_msg=msg)


def _exact(got, want, msg=""):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    np.testing.assert_array_equal(got, want, err_msg=msg)


# ---- training crops ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("crop", [24, 16])
@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("hwc", [True, False])
def test_crops_of_a_pool_equal_the_statement(hwc, dtype, crop):
    """Every geometry mode on crops at all four corners, a crop equal to its image, the last image of the pool and repeated
    images, from images of different sizes; the HW pool with the regression labels (x 200, float32)."""
    _need_gpu()
    shapes = _shapes(crop, hwc)
    arrays = _arrays(shapes, dtype, seed=crop + 2 * hwc)
    crops, params = _rows(shapes, crop)
    scale, ldt = (1.0, torch.int64) if hwc else (200.0, torch.float32)
    pool = A.CropPool(*arrays).to(DEV)
    assert pool.is_cuda and pool.sizes.tolist() == [list(s[:2]) for s in shapes]
    x, lab, dots = A.CropTransform(crop, True, scale, ldt)(pool, crops, params)
    wx, wl, wd = _statement(arrays, crops, params, crop, scale, np.int64 if hwc else np.float32)
    assert tuple(x.shape) == (len(MODES), 3 if hwc else 1, crop, crop)
    _exact(lab, wl)
    _exact(dots, wd)
    _close(x, wx)
    rot = params[:, 0] == 2                                      # the rotation brings in 0 from outside the crop, not the image
    assert (wl[rot][:, 0, 0] == 0).all() and (wd[rot][:, 0, 0] == 0).all() and wl[~rot][:, 0, 0].any()
    # SciPy's own geometry handed in on the device gives the same as the geometry formed from the angle
    geom = A.batch_geometry(params, crop, crop)
    dev = [torch.from_numpy(a).to(DEV) for a in (crops, params, geom)]
    x2, lab2, dots2 = A.CropTransform(crop, True, scale, ldt)(pool, *dev)
    assert torch.equal(x2.view(torch.int32), x.view(torch.int32)) and torch.equal(lab2, lab) and torch.equal(dots2, dots)


def test_second_call_reuses_the_workspace_with_other_crops():
    _need_gpu()
    shapes = _shapes(24, True)
    arrays = _arrays(shapes, "uint8", seed=5)
    pool = A.CropPool(*arrays).to(DEV)
    tf = A.CropTransform(24, True)
    crops, params = _rows(shapes, 24)
    first = tf(pool, crops, params)
    order = np.array([7, 2, 12, 5, 9])                           # a shorter batch of other rows and modes: stale partials beyond it
    crops2, params2 = crops[order], params[order[::-1]]
    second = tf(pool, crops2, params2)
    third = tf(pool, crops, params)
    for got, want in zip(second, _statement(arrays, crops2, params2, 24)):
        (_close if got.dtype == torch.float32 else _exact)(got, want)
    for a, b in zip(first, third):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_pool_whose_last_image_starts_beyond_2_to_31_elements():
    """Element offsets are 64-bit: only the two small images are written and read, the 2 GiB between them stay untouched."""
    _need_gpu()
    arrays = _arrays([(30, 37, 3), (40, 52, 3)], "uint8", seed=6)
    images, labels, dots = arrays
    far = 2 ** 31 + 1235
    buf = torch.empty(2 ** 31 + 8192, dtype=torch.uint8, device=DEV)
    assert far + images[1].size <= buf.numel()
    buf[:images[0].size] = torch.from_numpy(images[0].reshape(-1)).to(DEV)
    buf[far:far + images[1].size] = torch.from_numpy(images[1].reshape(-1)).to(DEV)
    small = A.CropPool(*arrays).to(DEV)
    pool = A.CropPool.from_buffers(buf, [0, far], small.sizes, 3, True, small.labels, small.map_offsets, small.dots)
    crops = np.array([[1, 16, 28], [0, 6, 13], [1, 0, 0], [1, 3, 5]], np.int32)
    params = np.array([MODES[0], MODES[4], MODES[9], MODES[12]], np.int32)
    x, lab, d = A.CropTransform(24, True)(pool, crops, params)
    wx, wl, wd = _statement(arrays, crops, params, 24)
    _exact(lab, wl)
    _exact(d, wd)
    _close(x, wx)
    del buf, pool


# ---- tables on the device: safety, capture -----------------------------------------------------------------------------------------
def _raw_crop_calls(pool, c, p, g, crop, x, lab, dots):
    """The three C calls on output tensors of the caller's (views inside canary buffers)."""
    from umi import lib as L
    from umi import ops
    N = c.shape[0]
    off, moff, sizes = pool._tables
    nbytes = L.fn("umi_crop_znorm_ws_bytes")(N)
    ws = ops.workspace(nbytes, pool.device)
    L.call("umi_crop_znorm", pool.images.data_ptr(), 0, off.data_ptr(), sizes.data_ptr(), len(pool), pool.images.numel(), pool.C,
           c.data_ptr(), p.data_ptr(), g.data_ptr(), N, crop, x.data_ptr(), 1, ws.data_ptr(), nbytes, ops._stream())
    L.call("umi_crop_labels", pool.labels.data_ptr(), 0, moff.data_ptr(), sizes.data_ptr(), len(pool), pool.labels.numel(),
           c.data_ptr(), p.data_ptr(), g.data_ptr(), N, crop, lab.data_ptr(), 1, 1.0, ops._stream())
    L.call("umi_crop_labels", pool.dots.data_ptr(), 0, moff.data_ptr(), sizes.data_ptr(), len(pool), pool.dots.numel(),
           c.data_ptr(), p.data_ptr(), g.data_ptr(), N, crop, dots.data_ptr(), 2, 1.0, ops._stream())


def test_out_of_range_rows_in_a_device_table_come_out_zero_and_touch_nothing_else():
    """Device tables are not read back, so the ValueError of the host path cannot happen: a row whose index or window is out of
    range gives an all-zero sample, its neighbours are right, and nothing outside the outputs is written."""
    _need_gpu()
    crop = 24
    shapes = _shapes(crop, True)
    arrays = _arrays(shapes, "uint8", seed=7)
    pool = A.CropPool(*arrays).to(DEV)
    good = np.array([[0, 16, 28], [3, 46, 17], [1, 4, 4]], np.int32)
    bad = np.array([[4, 0, 0], [-1, 0, 0], [0, 17, 0], [0, 0, 29], [1, -1, 0], [3, 0, -5], [2 ** 31 - 1, 0, 0], [0, 2 ** 30, 2 ** 30],
                    [3, 2 ** 31 - 1, 0], [1, 0, -2 ** 31]], np.int64).astype(np.int32)
    for row in bad:
        with pytest.raises(ValueError):
            A.CropTransform(crop, True)(pool, row[None])
    crops = np.concatenate([good[:1], bad[:5], good[1:2], bad[5:], good[2:]])
    is_good = np.array([1] + [0] * 5 + [1] + [0] * 5 + [1], bool)
    N = len(crops)
    params = np.array([MODES[(3 * i) % len(MODES)] for i in range(N)], np.int32)
    geom = A.batch_geometry(params, crop, crop)
    c, p, g = (torch.from_numpy(a).to(DEV) for a in (crops, params, geom))
    pad = 4096
    bx = torch.full((pad + N * 3 * crop * crop + pad,), 12345.0, dtype=torch.float32, device=DEV)
    bl = torch.full((pad + N * crop * crop + pad,), -77, dtype=torch.int64, device=DEV)
    bd = torch.full((pad + N * crop * crop + pad,), 99, dtype=torch.uint8, device=DEV)
    x, lab, d = bx[pad:-pad].view(N, 3, crop, crop), bl[pad:-pad].view(N, crop, crop), bd[pad:-pad].view(N, crop, crop)
    _raw_crop_calls(pool, c, p, g, crop, x, lab, d)
    torch.cuda.synchronize()
    for buf, v in ((bx, 12345.0), (bl, -77), (bd, 99)):
        assert (buf[:pad] == v).all() and (buf[-pad:] == v).all()
    keep, zero = torch.from_numpy(is_good).to(DEV), torch.from_numpy(~is_good).to(DEV)
    assert not x[zero].any() and not lab[zero].any() and not d[zero].any()
    wx, wl, wd = _statement(arrays, crops[is_good], params[is_good], crop)
    _exact(lab[keep], wl)
    _exact(d[keep], wd)
    _close(x[keep], wx)
    # the public path takes device tables as they are
    x2, lab2, d2 = A.CropTransform(crop, True)(pool, c, p, g)
    assert torch.equal(x2.view(torch.int32), x.view(torch.int32)) and torch.equal(lab2, lab) and torch.equal(d2, d)
    with pytest.raises(ValueError, match="on the device as well"):
        A.CropTransform(crop, True)(pool, c, params)


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_constant_crop_gives_the_statements_nans(dtype):
    """std 0 is not guarded, as in NumPy: a constant channel of a crop is 0 / 0 = NaN under the identity and rot90 / flip, and
    finite again once a rotation brings zeros in; the other channels stay finite."""
    _need_gpu()
    images, labels, dots = _arrays([(40, 52, 3), (33, 33, 3)], dtype, seed=8)
    images[0][8:32, 20:44, 1] = 7 if dtype == "uint8" else 0.5
    images[1][..., 2] = 9 if dtype == "uint8" else 0.25
    crops = np.array([[0, 8, 20], [0, 8, 20], [0, 8, 20], [1, 9, 9], [0, 9, 20]], np.int32)
    params = np.array([MODES[0], MODES[6], MODES[10], MODES[3], MODES[0]], np.int32)
    with np.errstate(invalid="ignore", divide="ignore"):
        wx, _, _ = _statement((images, labels, dots), crops, params, 24)
    nan = np.isnan(wx).all(axis=(2, 3))
    assert nan.tolist() == [[0, 1, 0], [0, 1, 0], [0, 0, 0], [1, 0, 0], [0, 0, 0]]                  # channels come out reversed
    x, _, _ = A.CropTransform(24, True)(A.CropPool(images, labels, dots).to(DEV), crops, params)
    _close(x, wx)


def test_two_runs_are_bit_identical_and_a_captured_call_follows_its_tables():
    _need_gpu()
    crop = 24
    shapes = _shapes(crop, True)
    crops, params = _rows(shapes, crop)
    geom = A.batch_geometry(params, crop, crop)
    for dtype in ("uint8", "float32"):
        arrays = _arrays(shapes, dtype, seed=9)
        pool = A.CropPool(*arrays).to(DEV)
        tf = A.CropTransform(crop, True)
        c, p, g = (torch.from_numpy(a).to(DEV) for a in (crops, params, geom))
        first = tf(pool, c, p, g)
        again = tf(pool, c, p, g)
        for a, b in zip(first, again):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = tf(pool, c, p, g)
        perm = np.roll(np.arange(len(crops)), 5)
        c.copy_(torch.from_numpy(crops[perm]))                   # the tables rewritten in place: the replay reads them anew
        p.copy_(torch.from_numpy(params[::-1].copy()))
        g.copy_(torch.from_numpy(geom[::-1].copy()))
        graph.replay()
        torch.cuda.synchronize()
        eager = tf(pool, c, p, g)
        for a, b, old in zip(out, eager, first):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)) and not torch.equal(a, old)
        wx, wl, wd = _statement(arrays, crops[perm], params[::-1], crop)
        _exact(out[1], wl)
        _exact(out[2], wd)
        _close(out[0], wx)
        # the grid: deterministic too, and capturable (its arguments are scalars)
        img = pool.image(3)
        a, b = A.grid_image(img, 13, 11, 32, 32), A.grid_image(img, 13, 11, 32, 32)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            t = A.grid_image(img, 13, 11, 32, 32)
        img.copy_(pool.image(3).flip(0))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(t.view(torch.int32), A.grid_image(img, 13, 11, 32, 32).view(torch.int32)) and not torch.equal(t, a)


# ---- the validation grid ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("hwc", [True, False])
def test_tile_grid_equals_the_statement(hwc, dtype):
    """70x41 with crop 32 (padded 96x64, six tiles) at no pad offset, the maximal one and the centred one; 64x32 needs no
    padding; 255 around an HWC image and 0 around an HW one; labels and dots are padded with 0."""
    _need_gpu()
    c = (3,) if hwc else ()
    arrays = _arrays([(70, 41) + c, (64, 32) + c], dtype, seed=10 + hwc)
    images, labels, dots = arrays
    pool = A.CropPool(*arrays).to(DEV)
    tf = A.CropTransform(32, False)
    assert A.center_pad(70, 41, 32) == (13, 11)
    for index, pad, want_pad in ((0, (0, 0), (0, 0)), (0, (26, 23), (26, 23)), (0, "center", (13, 11)), (1, None, (0, 0))):
        x, lab, d = tf.grid(pool, index, pad)
        wx, (wl,), wd = A.grid_transform_numpy(images[index], [labels[index]], *want_pad, 32, 32, dots=dots[index])
        assert tuple(x.shape) == ((6 if index == 0 else 2), len(c) * 2 + 1, 32, 32)
        _exact(lab, wl, f"{index} {pad}")
        _exact(d, wd, f"{index} {pad}")
        _close(x, wx, f"{index} {pad}")
    # the rule's values, seen in a pad pixel: tile 0's corner under the maximal pad
    x, _, _ = tf.grid(pool, 0, (26, 23))
    mean, std = A.padded_statistics(images[0], 96 * 64 - 70 * 41, 255 if hwc else 0)
    np.testing.assert_allclose(x[0, :, 0, 0].cpu().numpy(), (((255 if hwc else 0) - mean) / std)[::-1], rtol=0, atol=ATOL)
    # regression labels, and a pad value of one's own
    got = A.grid_maps(pool.label(0), 13, 11, 32, 32, None, 200.0, torch.float32)
    _, (wl,), _ = A.grid_transform_numpy(images[0], [labels[0]], 13, 11, 32, 32, label_scale=200.0, label_dtype=np.float32)
    _exact(got, wl)
    wx, _, _ = A.grid_transform_numpy(images[0], [], 5, 7, 32, 32, pad_value=100)
    _close(A.grid_image(pool.image(0), 5, 7, 32, 32, pad_value=100), wx)


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("hwc", [True, False])
def test_preprocess_crop_is_the_whole_padded_image_as_one_tile(hwc, dtype):
    _need_gpu()
    from umi import infer
    c = (3,) if hwc else ()
    (img,), _, _ = _arrays([(70, 41) + c], dtype, seed=12)
    wx, _, _ = A.grid_transform_numpy(img, [], 13, 11, 96, 64, pad_value=255)
    assert wx.shape == (1, len(c) * 2 + 1, 96, 64)
    for source in (img, torch.from_numpy(img), torch.from_numpy(img).to(DEV)):
        _close(infer.preprocess_crop(source, 32), wx)
    # th, tw = Hp, Wp of the grid call is the same thing, and its 32-pixel tiles are cuts of it
    whole = A.grid_image(torch.from_numpy(img).to(DEV), 13, 11, 96, 64, pad_value=255)
    assert torch.equal(whole.view(torch.int32), infer.preprocess_crop(img, 32).view(torch.int32))
    tiles = A.grid_image(torch.from_numpy(img).to(DEV), 13, 11, 32, 32, pad_value=255)
    assert torch.equal(tiles[3], whole[0, :, 32:64, 32:64])
    _close(infer.preprocess_crop(img[:64, :32], 32), A.grid_transform_numpy(img[:64, :32], [], 0, 0, 64, 32, pad_value=255)[0])


def test_preprocess_crop_feeds_the_tiled_prediction_of_a_small_unet():
    _need_gpu()
    import Model
    from umi import infer
    m = Model.UNet(3, 1, 8, False, compute_dtype="fp32")
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=13))
    m = m.to(DEV).eval()
    (img,), _, _ = _arrays([(70, 41, 3)], "uint8", seed=14)
    x = infer.preprocess_crop(img, 32)
    mask = infer.predict_binary_mask_tiled(m, x, 32)
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (96, 64)
    with torch.no_grad():
        want = (torch.sigmoid(m(x[:, :, 32:64, 32:64].contiguous())) >= 0.5).to(torch.uint8)[0, 0]
    assert torch.equal(mask[32:64, 32:64], want) and 0 < mask.float().mean() < 1


# ---- through the layers ------------------------------------------------------------------------------------------------------------------
class _Epochs:
    """A plain list of batches per epoch, handed out epoch after epoch."""

    def __init__(self, per_epoch):
        self.per_epoch, self.k = per_epoch, 0

    def __len__(self):
        return len(self.per_epoch[0])

    def __iter__(self):
        self.k += 1
        return iter(self.per_epoch[self.k - 1])


def test_trainer_on_crop_batches_of_a_device_pool_equals_the_eager_run_on_the_same_draws(tmp_path):
    """CropBatches as dataloaders['train' | 'val'] of Trainer (small U-Net, dice_bce_mc, val_batch=2) for two epochs == the same
    Trainer fed lists of the batches that the transform gives, called by hand with the same draws in the same order: the kernels
    are deterministic, so both runs see the same bits and differ by the step's own run-to-run order only."""
    _need_gpu()
    import Model
    import loss as L
    from Trainer import Trainer
    L.CLASS_NUMBER = 4
    crop = 32
    arrays = _arrays([(40, 52, 3), (33, 33, 3), (70, 41, 3)], "uint8", seed=15)
    pool = A.CropPool(arrays[0], arrays[1]).to(DEV)

    def run(name, loaders):
        m = Model.UNet(3, 4, 8, False, compute_dtype="fp32")
        m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=16))
        m.to(DEV).train()
        opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9)
        tr = Trainer(m, "single", torch.cuda.FloatTensor, DEV, str(tmp_path / name), loaders, 2, opt, 25, 2, "dice_bce_mc",
                     "dice_bce_mc", val_batch=2)
        tr.train()
        return tr

    random.seed(17)
    np.random.seed(18)
    train = A.CropBatches(pool, crop, 2, True, train=True, indices=[0, 1, 2, 1])
    val = A.CropBatches(pool, crop, 2, True, train=False)        # tiles 4, 4, 6: one group of two images, one of one
    assert len(train) == 2 and len(val) == 3
    got = run("loader", {"train": train, "val": val})
    random.seed(17)
    np.random.seed(18)
    tf = A.CropTransform(crop, True)
    per_train, per_val = [], []
    for _ in range(2):
        per_train.append([tf(pool, indices=chunk) for chunk in ([0, 1], [2, 1])])
        per_val.append([tf.grid(pool, i) for i in range(3)])
    x, y = per_train[0][0]
    assert x.is_cuda and tuple(x.shape) == (2, 3, crop, crop) and y.dtype == torch.int64
    assert [t[0].shape[0] for t in per_val[0]] == [4, 4, 6]
    want = run("lists", {"train": _Epochs(per_train), "val": _Epochs(per_val)})
    assert len(got.train_loss_list) == 2 and np.isfinite(got.train_loss_list).all() and np.isfinite(got.val_loss_list).all()
    np.testing.assert_allclose(got.train_loss_list, want.train_loss_list, rtol=1e-5)
    np.testing.assert_allclose(got.val_loss_list, want.val_loss_list, rtol=1e-5)
    np.testing.assert_allclose(got.val_score_list, want.val_score_list, rtol=1e-5)
    for pa, pb in zip(got.model.parameters(), want.model.parameters()):
        np.testing.assert_allclose(pa.detach().cpu().numpy(), pb.detach().cpu().numpy(), rtol=1e-4, atol=1e-6)


# ---- the existing kernels after their helpers moved into a header ----------------------------------------------------------------
def test_existing_augment_kernels_give_the_statements_bytes():
    """umi_augment_geometry and umi_augment_labels are index maps: the statement's bytes.  umi_augment_znorm on uint8 forms
    mean = S1 / n and std = sqrt(n * S2 - S1^2) / n from exact integers and (v - mean) / std in float64 with one rounding to
    float32: restated here with Python integers, that is the kernel's result to the bit."""
    _need_gpu()
    rng = np.random.default_rng(19)
    img = (rng.random((len(MODES), 33, 33, 3)) * 255).astype(np.uint8)
    lab = rng.integers(0, 4, (len(MODES), 33, 33)).astype(np.uint8)
    params = np.array(MODES, np.int32)
    geom = A.batch_geometry(params, 33, 33)
    x, l = torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV)
    aug = np.stack([A.apply_geometry_numpy(img[n], params[n]) for n in range(len(MODES))])
    _exact(A.apply_geometry(x, params), aug)
    want_l = np.stack([A.apply_geometry_numpy(lab[n], params[n]) for n in range(len(MODES))])
    _exact(A.transform_labels(l, params, geom, (33, 33)), want_l.astype(np.int64))
    _exact(A.transform_labels(l, params, geom, (33, 33), 200.0, torch.float32), want_l.astype(np.float32) * np.float32(200))
    want = np.empty((len(MODES), 3, 33, 33), np.float32)
    for n in range(len(MODES)):
        mean, std = A.padded_statistics(aug[n], 0, 0)
        want[n] = ((aug[n].astype(np.float64) - mean) / std).transpose((2, 0, 1))[::-1].astype(np.float32)
    got = A.transform_image(x, params).cpu().numpy()
    np.testing.assert_array_equal(got.view(np.int32), want.view(np.int32))
