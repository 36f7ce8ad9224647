"""CPU: the statement side of the training-batch transform (umi.augment) against SciPy's recorded outputs
(tests/golden/augment.npz, tools/gen_golden_augment.py), the reference's order of random draws, the refusals, and the
Trainer's batch_transform hook."""
import os
import random

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from oracle import recipe, ref_unet
from tools import gen_golden_augment as G
from umi import augment as A


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "augment.npz"))


def test_cos_sin_table_is_scipys(golden):
    got = np.array([A.cos_sin_dg(a) for a in G.ANGLES])
    np.testing.assert_array_equal(got, golden["cos_sin"])
    with pytest.raises(ValueError):
        A.cos_sin_dg(21)
    with pytest.raises(ValueError):
        A.cos_sin_dg(2.5)


def test_rotation_statement_equals_every_recorded_scipy_output(golden):
    """Fed SciPy's own matrix and offset, the sampling rule reproduces scipy.ndimage.rotate(order=0, reshape=False) bit for bit;
    rotate_geometry forms the same matrix and offset from the table."""
    n = 0
    for name, seed, shape, dtype, angles in G.ROTATE_CASES:
        x = G.make(seed, shape, dtype)
        for a in angles:
            mat, off = golden[f"mat_{name}_{a}"], golden[f"off_{name}_{a}"]
            got = A.apply_geometry_numpy(x, (A.MODE_ROTATE, 0, 0, a), A.pack_geometry(mat, off))
            want = golden[f"rot_{name}_{a}"]
            assert got.dtype == want.dtype
            np.testing.assert_array_equal(got, want, err_msg=f"{name} {a}")
            m, o = A.rotate_geometry(a, *shape[:2])
            np.testing.assert_array_equal(m, mat, err_msg=f"{name} {a}")
            np.testing.assert_array_equal(o, off, err_msg=f"{name} {a}")
            n += 1
    assert n == sum(len(c[4]) for c in G.ROTATE_CASES) >= 80 + 11


def test_rot_flip_statement_equals_the_recorded_outputs(golden):
    for name, seed, shape, dtype in G.ROT_FLIP_CASES:
        x = G.make(seed, shape, dtype)
        for k, axis in G.ROT_FLIP:
            np.testing.assert_array_equal(A.apply_geometry_numpy(x, (A.MODE_ROT_FLIP, k, axis, 0)), golden[f"rf_{name}_{k}_{axis}"])
    np.testing.assert_array_equal(A.apply_geometry_numpy(x, (A.MODE_NONE, 3, 1, 7)), x)


def test_live_rotate_geometry_equals_live_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(77)
    for x in ((rng.random((29, 37, 3)) * 255).astype(np.uint8), rng.standard_normal((41, 23)).astype(np.float32)):
        for a in G.ANGLES:
            got = A.apply_geometry_numpy(x, (A.MODE_ROTATE, 0, 0, a))
            np.testing.assert_array_equal(got, ndimage.rotate(x, a, order=0, reshape=False), err_msg=f"{x.shape} {a}")


@pytest.mark.parametrize("case", range(len(G.TRANSFORM_CASES)))
def test_train_transform_statement_equals_the_recorded_transform(golden, case):
    name, seed, shape, dtype, size, kind, scale, ldt = G.TRANSFORM_CASES[case]
    img, lab = G.make(seed, shape, dtype), G.make_label(seed, shape, kind)
    for i, p in enumerate(G.TRANSFORM_PARAMS):
        x, (label,) = A.train_transform_numpy(img, [lab], p, size, label_scale=scale, label_dtype=ldt)
        want_x, want_l = golden[f"tf_{name}_{i}_x"], golden[f"tf_{name}_{i}_label"]
        assert x.dtype == np.float32 and x.shape == want_x.shape and label.dtype == want_l.dtype
        np.testing.assert_array_equal(label, want_l, err_msg=f"{name} {p}")
        np.testing.assert_allclose(x, want_x, rtol=0, atol=2e-6, err_msg=f"{name} {p}")
    if name == "bin48":                  # 48 -> 24: the last sample coordinate lies above 47, SciPy's last row and column are 0
        assert not want_l[-1].any() and not want_l[:, -1].any() and want_l[:-1, :-1].any()


def test_draw_params_makes_the_references_draws_in_order():
    random.seed(1234)
    np.random.seed(4321)
    want = []
    for _ in range(64):                                   # DataLoader.py:638-644 with :103-105 and :115 written out
        if random.random() > 0.5:
            k = np.random.randint(0, 4)
            axis = np.random.randint(0, 2)
            want.append((1, k, axis, 0))
        elif random.random() > 0.5:
            want.append((2, 0, 0, np.random.randint(-20, 20)))
        else:
            want.append((0, 0, 0, 0))
    random.seed(1234)
    np.random.seed(4321)
    got = A.draw_params(64)
    assert got.dtype == np.int32 and got.shape == (64, 4)
    np.testing.assert_array_equal(got, np.array(want))
    assert set(got[:, 0]) == {0, 1, 2}
    assert not A.no_augmentation(5).any() and A.no_augmentation(5).shape == (5, 4)
    # generators of one's own: same rule
    a = A.draw_params(16, random.Random(3), np.random.RandomState(4))
    b = A.draw_params(16, random.Random(3), np.random.RandomState(4))
    np.testing.assert_array_equal(a, b)


def test_refusals():
    tf = A.TrainTransform((24, 24), augmentation=True)
    rng = np.random.default_rng(0)
    img = (rng.random((2, 24, 24, 3)) * 255).astype(np.uint8)
    lab = np.zeros((2, 24, 24), np.uint8)
    with pytest.raises(ValueError, match="one size"):     # a batch whose images differ in size
        tf([img[0], img[1][:20]], lab, A.no_augmentation(2))
    wide = A.TrainTransform((24, 32), augmentation=True)
    with pytest.raises(ValueError, match="odd k"):        # H != W with an odd k
        wide(np.zeros((2, 24, 32), np.uint8), np.zeros((2, 24, 32), np.uint8), np.array([[1, 2, 0, 0], [1, 3, 1, 0]], np.int32))
    x, _ = wide(np.arange(2 * 24 * 32, dtype=np.float32).reshape(2, 24, 32), np.zeros((2, 24, 32), np.uint8),
                np.array([[1, 2, 0, 0], [2, 0, 0, 5]], np.int32))                   # even k and a rotation are fine
    assert x.shape == (2, 1, 24, 32)
    # a resize whose result, by the reference's swapped factors (width / x on axis 0), is not input_size: 48x64 -> (24, 32)
    # gives round(48 * 32 / 64) x round(64 * 24 / 48) = 24 x 32 (fine), 40x64 -> (24, 32) gives 20 x 38
    assert A.resized_shape(48, 64, (24, 32)) == (24, 32)
    with pytest.raises(ValueError, match="20x38"):
        wide(np.zeros((1, 40, 64), np.uint8), np.zeros((1, 40, 64), np.uint8), A.no_augmentation(1))
    with pytest.raises(ValueError):
        A.TrainTransform((24, 24), True, label_dtype=torch.int32)


def test_train_transform_on_host_batches_and_several_label_maps():
    """Host arrays and host tensors run the statement per sample; a list of label batches comes back as a list."""
    rng = np.random.default_rng(5)
    img = (rng.random((3, 24, 24, 3)) * 255).astype(np.uint8)
    l1 = rng.integers(0, 3, (3, 24, 24)).astype(np.uint8)
    l2 = rng.random((3, 24, 24)).astype(np.float32)
    p = np.array([[0, 0, 0, 0], [1, 3, 1, 0], [2, 0, 0, -9]], np.int32)
    tf = A.TrainTransform((24, 24), True, label_scale=200.0, label_dtype=torch.float32)
    x, labels = tf(torch.from_numpy(img), [torch.from_numpy(l1), l2], p)
    assert isinstance(labels, list) and x.shape == (3, 3, 24, 24) and x.dtype == torch.float32
    for n in range(3):
        wx, wl = A.train_transform_numpy(img[n], [l1[n], l2[n]], p[n], (24, 24), label_scale=200.0, label_dtype=np.float32)
        np.testing.assert_array_equal(x[n].numpy(), wx)
        np.testing.assert_array_equal(labels[0][n].numpy(), wl[0])
        np.testing.assert_array_equal(labels[1][n].numpy(), wl[1])
    assert labels[0].dtype == torch.float32 and float(labels[0].max()) == 400.0


def _tiny_run(tmp_path, name, loaders, **kw):
    import loss as L
    from Trainer import Trainer
    torch.manual_seed(0)
    L.CLASS_NUMBER = 2
    m = ref_unet.RefUNet(3, 2, 4, False)
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=3))
    opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9)
    tr = Trainer(m, "single", torch.FloatTensor, "cpu", str(tmp_path / name), loaders, 2, opt, 25, 2, "dice_bce_mc", "dice_bce_mc",
                 **kw)
    tr.train()
    return tr


def test_trainer_batch_transform_equals_pretransformed_batches(tmp_path):
    """Two epochs on raw uint8 batches through batch_transform (no augmentation) == two epochs on the same batches transformed
    beforehand by the statement: the hook changes where the transform runs, not the step."""
    rng = np.random.default_rng(9)
    img = torch.from_numpy((rng.random((6, 16, 16, 3)) * 255).astype(np.uint8))
    lab = torch.from_numpy((rng.random((6, 16, 16)) < 0.4).astype(np.uint8))
    tf = A.TrainTransform((16, 16), augmentation=False)

    def loaders(a, b):
        return {"train": DataLoader(TensorDataset(a[:4], b[:4]), batch_size=2, shuffle=False),
                "val": DataLoader(TensorDataset(a[4:], b[4:]), batch_size=1)}

    hooked = _tiny_run(tmp_path, "hooked", loaders(img, lab), batch_transform=tf)
    x, y = tf(img, lab, A.no_augmentation(6))
    assert x.shape == (6, 3, 16, 16) and y.dtype == torch.int64
    plain = _tiny_run(tmp_path, "plain", loaders(x, y))
    assert len(hooked.train_loss_list) == 2 and np.isfinite(hooked.train_loss_list).all()
    assert hooked.train_loss_list == plain.train_loss_list
    assert hooked.val_loss_list == plain.val_loss_list
    assert hooked.val_score_list == plain.val_score_list


def test_trainer_draws_in_the_train_phase_only(tmp_path):
    """With augmentation the hook draws fresh parameters for every train batch and none in the validation phase."""
    seen = []

    class Spy(A.TrainTransform):
        def __call__(self, images, label_maps, params=None, geom=None):
            seen.append(None if params is None else np.asarray(params).copy())
            return super().__call__(images, label_maps, params, geom)

    rng = np.random.default_rng(10)
    img = torch.from_numpy((rng.random((3, 16, 16, 3)) * 255).astype(np.uint8))
    lab = torch.from_numpy((rng.random((3, 16, 16)) < 0.4).astype(np.uint8))
    loaders = {"train": DataLoader(TensorDataset(img[:2], lab[:2]), batch_size=2), "val": DataLoader(TensorDataset(img[2:], lab[2:]))}
    _tiny_run(tmp_path, "spy", loaders, batch_transform=Spy((16, 16), augmentation=True))
    assert len(seen) == 4 and seen[0] is None and seen[2] is None                   # train, val, train, val
    assert seen[1].shape == (1, 4) and not seen[1].any() and not seen[3].any()


def test_c_abi_rejects_bad_arguments_before_any_launch():
    """Null pointers, sizes <= 0 and C > 4 return UMI_ERR_BADARG (-1) without touching a GPU, like the rest of the ABI."""
    from umi import lib
    geo, lab, zn = lib.fn("umi_augment_geometry"), lib.fn("umi_augment_labels"), lib.fn("umi_augment_znorm")
    p = 4096                                                    # any non-null address: rejected before it is used
    assert geo(None, 0, p, p, p, 1, 8, 8, 3, None) == -1 and geo(p, 0, p, None, p, 1, 8, 8, 3, None) == -1
    assert geo(p, 0, p, p, p, 1, 8, 8, 5, None) == -1 and geo(p, 0, p, p, p, 0, 8, 8, 3, None) == -1
    assert geo(p, 2, p, p, p, 1, 8, 8, 3, None) == -1 and geo(p, 0, p, p, p, 1, 8, 0, 3, None) == -1
    assert lab(p, 0, None, 1, 1.0, p, p, 1, 8, 8, 8, 8, None) == -1 and lab(p, 0, p, 1, 1.0, p, p, 1, 8, 8, 0, 8, None) == -1
    assert lab(p, 0, p, 2, 1.0, p, p, 1, 8, 8, 8, 8, None) == -1
    assert zn(p, 0, None, p, p, 1, 8, 8, 3, 1, p, 1 << 20, None) == -1 and zn(p, 0, p, p, p, 1, 8, 8, 5, 1, p, 1 << 20, None) == -1
    assert zn(p, 0, p, p, p, 1, 8, 8, 3, 1, None, 0, None) == -3                  # UMI_ERR_WORKSPACE
    assert lib.fn("umi_augment_znorm_ws_bytes")(0) == 0 and lib.fn("umi_augment_znorm_ws_bytes")(2) > 0
