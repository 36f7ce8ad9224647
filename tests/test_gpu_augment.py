"""GPU: the kernels of csrc/augment.hip (umi.augment.apply_geometry / transform_labels / transform_image / TrainTransform)
against the NumPy statement of umi.augment, which tests/test_augment.py pins to SciPy's recorded outputs on the CPU.  Geometry and
labels are exact; the normalised image is within 2e-6 of the float64 statement (the bar of tests/test_gpu_infer.py for the same
formula: one float32 rounding of an fp64 value of magnitude <= ~10 is 5e-7, the rest is the summation order of the statistics)."""
import os
import random

import numpy as np
import pytest
import torch

from oracle import recipe, ref_resize
from tools import gen_golden_augment as G
from umi import augment as A

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: torch.cuda.is_available() is False")


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "augment.npz"))


def _params(n, square, seed):
    """n rows cycling through modes 0, 1, 2 with seeded k / axis / angle; k is even when the samples are not square."""
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 4), np.int32)
    for i in range(n):
        if i % 3 == 1:
            p[i] = (1, rng.integers(0, 4) if square else 2 * rng.integers(0, 2), rng.integers(0, 2), 0)
        elif i % 3 == 2:
            p[i] = (2, 0, 0, rng.integers(-20, 20))
    return p


def _image(rng, shape, dtype):
    x = rng.random(shape) * 255
    return x.astype(np.uint8) if dtype == "uint8" else (x / 255 - 0.3).astype(np.float32)


def _statement(img, maps, p, size, scale=1.0, ldt=np.int64):
    out = [A.train_transform_numpy(img[n], [m[n] for m in maps], p[n], size, label_scale=scale, label_dtype=ldt)
           for n in range(img.shape[0])]
    return np.stack([o[0] for o in out]), [np.stack([o[1][j] for o in out]) for j in range(len(maps))]


# ---- geometry -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(G.ROTATE_CASES)))
def test_rotation_on_device_equals_statement_and_scipy(golden, case):
    """Every recorded angle of a case as one batch, fed SciPy's own matrix and offset."""
    _need_gpu()
    name, seed, shape, dtype, angles = G.ROTATE_CASES[case]
    x = G.make(seed, shape, dtype)
    p = np.array([(2, 0, 0, a) for a in angles], np.int32)
    geom = np.stack([A.pack_geometry(golden[f"mat_{name}_{a}"], golden[f"off_{name}_{a}"]) for a in angles])
    xb = torch.from_numpy(np.stack([x] * len(angles))).to(DEV)
    got = A.apply_geometry(xb, torch.from_numpy(p).to(DEV), torch.from_numpy(geom).to(DEV)).cpu().numpy()
    assert got.dtype == x.dtype and got.shape == xb.shape
    for n, a in enumerate(angles):
        np.testing.assert_array_equal(got[n], A.apply_geometry_numpy(x, p[n], geom[n]), err_msg=f"{name} {a}")
        np.testing.assert_array_equal(got[n], golden[f"rot_{name}_{a}"], err_msg=f"{name} {a}")
    np.testing.assert_array_equal(A.apply_geometry(xb, p).cpu().numpy(), got)          # host parameters: geometry formed here


def test_rot_flip_on_device_equals_the_recorded_outputs(golden):
    _need_gpu()
    for name, seed, shape, dtype in G.ROT_FLIP_CASES:
        x = G.make(seed, shape, dtype)
        p = np.array([(1, k, axis, 0) for k, axis in G.ROT_FLIP], np.int32)
        got = A.apply_geometry(torch.from_numpy(np.stack([x] * 8)).to(DEV), p).cpu().numpy()
        for n, (k, axis) in enumerate(G.ROT_FLIP):
            np.testing.assert_array_equal(got[n], golden[f"rf_{name}_{k}_{axis}"], err_msg=f"{name} {k} {axis}")


@pytest.mark.parametrize("dtype,shape", [("uint8", (5, 24, 24, 3)), ("float32", (5, 33, 33, 4)), ("uint8", (5, 96, 96, 1)),
                                         ("uint8", (5, 130, 70)), ("float32", (5, 31, 40)), ("float32", (5, 70, 130, 3))])
def test_mixed_modes_in_one_launch(dtype, shape):
    _need_gpu()
    x = _image(np.random.default_rng(21), shape, dtype)
    p = _params(shape[0], shape[1] == shape[2], seed=22)
    assert set(p[:, 0]) == {0, 1, 2}
    got = A.apply_geometry(torch.from_numpy(x).to(DEV), p).cpu().numpy()
    for n in range(shape[0]):
        np.testing.assert_array_equal(got[n], A.apply_geometry_numpy(x[n], p[n]), err_msg=f"{n} {p[n]}")


def test_odd_k_on_a_non_square_sample_with_device_parameters_comes_out_zero():
    """Device parameters are not read back, so the refusal of the host path cannot happen; the kernel stays inside the sample."""
    _need_gpu()
    x = torch.from_numpy(_image(np.random.default_rng(23), (2, 20, 36), "uint8")).to(DEV)
    p = np.array([[1, 1, 0, 0], [1, 2, 1, 0]], np.int32)
    with pytest.raises(ValueError, match="odd k"):
        A.apply_geometry(x, p)
    got = A.apply_geometry(x, torch.from_numpy(p).to(DEV), torch.zeros((2, 6), dtype=torch.float64, device=DEV)).cpu().numpy()
    assert not got[0].any()
    np.testing.assert_array_equal(got[1], A.apply_geometry_numpy(x[1].cpu().numpy(), p[1]))


# ---- label maps: order-0 zoom and geometry as one gather ------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(40, 40), (48, 48), (24, 24)])      # 48 -> 24: the zoom zeroes the last row and column; 24: no resize
@pytest.mark.parametrize("kind,scale,ldt", [("class", 1.0, "int64"), ("density", 200.0, "float32")])
def test_composed_label_gather_is_exact(hw, kind, scale, ldt):
    _need_gpu()
    N = 6
    lab = np.stack([G.make_label(30 + n, hw, kind) for n in range(N)])
    p = _params(N, True, seed=31)
    img = np.zeros((N,) + hw, np.uint8)
    img[:, ::3] = 9                                                  # any image with a non-zero std; only the labels matter here
    _, (want,) = _statement(img, [lab], p, (24, 24), scale, ldt)
    geom = A.batch_geometry(p, *hw)
    got = A.transform_labels(torch.from_numpy(lab).to(DEV), p, geom, (24, 24), scale, getattr(torch, ldt))
    assert got.dtype == getattr(torch, ldt) and tuple(got.shape) == (N, 24, 24)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    if hw == (48, 48):
        assert not want[:, -1].any() and not want[:, :, -1].any() and want.any()


def test_recorded_transform_labels_and_images(golden):
    """The whole transform on the device against SciPy's recorded results, resize cases included."""
    _need_gpu()
    for name, seed, shape, dtype, size, kind, scale, ldt in G.TRANSFORM_CASES:
        img, lab = G.make(seed, shape, dtype), G.make_label(seed, shape, kind)
        n = len(G.TRANSFORM_PARAMS)
        tf = A.TrainTransform(size, True, label_scale=scale, label_dtype=getattr(torch, ldt))
        x, label = tf(torch.from_numpy(np.stack([img] * n)).to(DEV), torch.from_numpy(np.stack([lab] * n)).to(DEV),
                      np.array(G.TRANSFORM_PARAMS, np.int32))
        for i in range(n):
            np.testing.assert_array_equal(label[i].cpu().numpy(), golden[f"tf_{name}_{i}_label"], err_msg=f"{name} {i}")
            np.testing.assert_allclose(x[i].cpu().numpy(), golden[f"tf_{name}_{i}_x"], rtol=0, atol=2e-6, err_msg=f"{name} {i}")


# ---- image path without a resize ----------------------------------------------------------------------------------------------
_IMAGES = {
    "u8_24x24": lambda r: _image(r, (4, 24, 24), "uint8"),
    "u8_33x33x3": lambda r: _image(r, (4, 33, 33, 3), "uint8"),
    "u8_96x96x3": lambda r: _image(r, (4, 96, 96, 3), "uint8"),
    "u8_130x70x4": lambda r: _image(r, (4, 130, 70, 4), "uint8"),
    # |mean| >> std: an fp32 accumulation, or a one-pass E[x^2] - E[x]^2 variance even in fp64, is visibly off here
    "f32_mean1e4": lambda r: (1e4 + r.standard_normal((4, 40, 56, 3))).astype(np.float32),
    "f32_mean1e6": lambda r: (1e6 + r.standard_normal((4, 64, 64))).astype(np.float32),
}


@pytest.mark.parametrize("name", list(_IMAGES))
def test_image_path_without_resize_matches_float64_statement(name):
    _need_gpu()
    img = _IMAGES[name](np.random.default_rng(41))
    H, W = img.shape[1:3]
    p = _params(img.shape[0], H == W, seed=42)
    want, _ = _statement(img, [], p, (H, W))
    x = torch.from_numpy(img).to(DEV)
    got = A.transform_image(x, p)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=2e-6)
    again = A.transform_image(x, p)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))                 # fixed summation order: identical bits


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_image_path_constant_channel_is_nan(dtype):
    """A constant channel has std 0: the reference divides 0 by 0 and gets NaN in every pixel of it; so do the kernels (modes 0
    and 1 keep a channel constant; a rotation brings zeros in)."""
    _need_gpu()
    img = (np.random.default_rng(43).random((2, 48, 48, 3)) * 255).astype(np.uint8).astype(dtype)
    img[..., 1] = 7 if dtype == "uint8" else 0.5              # exact in fp64 sums: the mean is exactly the value
    p = np.array([[0, 0, 0, 0], [1, 3, 0, 0]], np.int32)
    with np.errstate(invalid="ignore"):
        want, _ = _statement(img, [], p, (48, 48))
    assert np.isnan(want[:, 1]).all() and not np.isnan(want[:, [0, 2]]).any()         # reversed channels: 1 stays the middle
    got = A.transform_image(torch.from_numpy(img).to(DEV), p).cpu().numpy()
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-6)


# ---- image path with a resize -----------------------------------------------------------------------------------------------
def test_image_path_with_resize_matches_statement():
    _need_gpu()
    img = _image(np.random.default_rng(51), (3, 40, 40, 3), "uint8")
    lab = np.stack([G.make_label(52 + n, (40, 40), "class") for n in range(3)])
    p = np.array([[0, 0, 0, 0], [1, 1, 1, 0], [2, 0, 0, 13]], np.int32)
    for n in range(3):          # the device rounds the resized bytes from its own spline sums: no half-way value may decide a byte
        assert not ref_resize.halfway(A.apply_geometry_numpy(img[n], p[n]), (24, 24)).any()
    want_x, (want_l,) = _statement(img, [lab], p, (24, 24))
    x, label = A.TrainTransform((24, 24), True)(torch.from_numpy(img).to(DEV), torch.from_numpy(lab).to(DEV), p)
    assert tuple(x.shape) == (3, 3, 24, 24) and label.dtype == torch.int64
    np.testing.assert_array_equal(label.cpu().numpy(), want_l)
    np.testing.assert_allclose(x.cpu().numpy(), want_x, rtol=0, atol=2e-6)


# ---- TrainTransform and the Trainer hook --------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(24, 24), (40, 40)])
def test_train_transform_device_equals_host(hw):
    _need_gpu()
    rng = np.random.default_rng(61)
    img = _image(rng, (6,) + hw + (3,), "uint8")
    l1 = np.stack([G.make_label(62 + n, hw, "class") for n in range(6)])
    l2 = np.stack([G.make_label(72 + n, hw, "density") for n in range(6)])
    tf = A.TrainTransform((24, 24), True, label_scale=200.0, label_dtype=torch.float32)
    p = _params(6, True, seed=63)
    hx, hl = tf(img, [l1, l2], p)
    dx, dl = tf(torch.from_numpy(img).to(DEV), [torch.from_numpy(l1).to(DEV), torch.from_numpy(l2).to(DEV)], p)
    assert dx.is_cuda and isinstance(dl, list) and len(dl) == 2
    for h, d in zip(hl, dl):
        assert d.dtype == h.dtype
        np.testing.assert_array_equal(d.cpu().numpy(), h.numpy())
    np.testing.assert_allclose(dx.cpu().numpy(), hx.numpy(), rtol=0, atol=2e-6)
    # params=None: drawn on the host in the reference's order, the same rows on either path under the same seeds
    outs = []
    for im, a, b in ((img, l1, l2), (torch.from_numpy(img).to(DEV), torch.from_numpy(l1).to(DEV), torch.from_numpy(l2).to(DEV))):
        random.seed(7)
        np.random.seed(8)
        outs.append(tf(im, [a, b]))
    np.testing.assert_array_equal(outs[1][1][0].cpu().numpy(), outs[0][1][0].numpy())
    np.testing.assert_allclose(outs[1][0].cpu().numpy(), outs[0][0].numpy(), rtol=0, atol=2e-6)


def test_trainer_step_with_batch_transform_on_hip_model(tmp_path):
    """Trainer(batch_transform=...) on raw uint8 batches == the same Trainer fed the batch transformed beforehand with the same
    draws: the transform is deterministic, so both steps see the same bits and differ by the step's own run-to-run order only."""
    _need_gpu()
    import Model
    import loss as L
    from Trainer import Trainer
    L.CLASS_NUMBER = 2
    rng = np.random.default_rng(81)
    img = torch.from_numpy(_image(rng, (2, 32, 32, 3), "uint8"))
    lab = torch.from_numpy((rng.random((2, 32, 32)) < 0.4).astype(np.uint8))
    tf = A.TrainTransform((32, 32), augmentation=True)

    def trainer(name, **kw):
        m = Model.UNet(3, 2, 8, False, compute_dtype="fp32")
        m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=82))
        m.to(DEV).train()
        opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9)
        return Trainer(m, "single", torch.cuda.FloatTensor, DEV, str(tmp_path / name), {"train": [0], "val": [0]}, 2, opt, 25, 1,
                       "dice_bce_mc", "dice_bce_mc", **kw)

    random.seed(3)
    np.random.seed(4)
    hooked = trainer("hooked", batch_transform=tf)
    loss_a = hooked.train_step(img, lab)
    val_a = hooked.eval_step(img, lab)[0]
    random.seed(3)
    np.random.seed(4)
    x, y = tf(img.to(DEV), lab.to(DEV))
    assert x.dtype == torch.float32 and y.dtype == torch.int64
    plain = trainer("plain")
    loss_b = plain.train_step(x, y)
    val_b = plain.eval_step(*tf(img.to(DEV), lab.to(DEV), A.no_augmentation(2)))[0]
    assert torch.isfinite(loss_a) and torch.isfinite(val_a)
    np.testing.assert_allclose(loss_a.item(), loss_b.item(), rtol=1e-5)
    np.testing.assert_allclose(val_a.item(), val_b.item(), rtol=1e-5)
    for pa, pb in zip(hooked.model.parameters(), plain.model.parameters()):
        np.testing.assert_allclose(pa.detach().cpu().numpy(), pb.detach().cpu().numpy(), rtol=1e-4, atol=1e-6)
