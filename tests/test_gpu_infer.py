"""GPU: the on-device cubic resize of `umi.infer.preprocess` (reference test_mc3serousv5.py:100-127) against SciPy's outputs
(fixtures) and the whole preprocess against the reference's formula on the oracle's resize."""
import os

import numpy as np
import pytest
import torch

from oracle import ref_resize
from tools import gen_golden_resize as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("i", range(len(G.CASES)))
def test_zoom_cubic_on_device_matches_scipy(golden_dir, i):
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from umi import infer
    g = np.load(os.path.join(golden_dir, "zoom_cubic.npz"))
    seed, shape, ohw, dtype = G.CASES[i]
    img = G.make(seed, shape, dtype)
    got = infer.zoom_cubic(img, ohw).cpu().numpy()
    want = g[f"case{i}"]
    assert got.shape == want.shape and got.dtype == want.dtype
    if dtype == "uint8":
        np.testing.assert_array_equal(got, want)          # bit-exact for byte images (what cv2.imread gives the reference)
    else:
        np.testing.assert_allclose(got, want, rtol=0, atol=2e-6)


@pytest.mark.parametrize("shape", [(100, 80, 3), (70, 90)])
def test_preprocess_with_resize_matches_reference_formula(shape):
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from umi import infer
    rng = np.random.default_rng(5)
    img = (rng.random(shape) * 255).astype(np.uint8)
    size = (64, 96)
    x = infer.preprocess(img, input_size=size).cpu().numpy()
    z = ref_resize.zoom_cubic(img, size)                     # == scipy.ndimage.zoom(order=3) (tests/test_oracle_resize.py)
    z = (z - np.mean(z, axis=(0, 1))) / np.std(z, axis=(0, 1))
    want = z.astype(np.float32)[None, None] if len(shape) == 2 else z.transpose((2, 0, 1))[::-1].astype(np.float32)[None]
    assert x.shape == want.shape
    np.testing.assert_allclose(x, want, rtol=0, atol=2e-6)


def _assert_matches_oracle(got, img, ohw):
    """uint8: exact (within 1 only at exact half-way values, ref_resize.halfway); float32: one float32 ulp of the oracle plus
    1e-9 (the device pow may differ from the host's in the last float64 bit); out-of-range samples (mode 'constant'): exactly 0."""
    want = ref_resize.zoom_cubic(img, ohw)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape)
    if img.dtype == np.uint8:
        tie = ref_resize.halfway(img, ohw)
        np.testing.assert_array_equal(got[~tie], want[~tie], err_msg=f"{img.shape} -> {ohw}")
        assert np.all(np.abs(got[tie].astype(int) - want[tie]) <= 1)
    else:
        err = np.abs(got.astype(np.float64) - want)
        assert np.all(err <= np.spacing(np.abs(want)) + 1e-9), (img.shape, ohw, err.max())
    _, _, zy = ref_resize._axis_plan(img.shape[0], ohw[0])
    _, _, zx = ref_resize._axis_plan(img.shape[1], ohw[1])
    assert np.all(got[zy] == 0) and np.all(got[:, zx] == 0), (img.shape, ohw)


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_zoom_cubic_on_device_matches_oracle_sweep(dtype):
    """Every size class of gen_golden_resize.SWEEP (one-axis strips up and down, both axes, n_in == n_out, 1-, 2- and 3-pixel
    axes, C = 1 / 3 / 4, affected 224-sizes, evaluation sizes to 224 and 512) against the oracle, which the CPU suite pins to
    SciPy on the same inputs."""
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from umi import infer
    for i, (shape, ohw) in enumerate(G.SWEEP):
        img = G.make(100 + i, shape, dtype)
        _assert_matches_oracle(infer.zoom_cubic(img, ohw).cpu().numpy(), img, ohw)


def test_zoom_cubic_on_device_zeroes_out_of_range_samples():
    """All input heights 2..4099 to 224 (222 of them have their last sample coordinate above n_in - 1): a constant strip comes
    out 100 inside and 0 exactly at the samples SciPy's mode 'constant' zeroes."""
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from umi import infer
    affected = 0
    for n_in in range(2, 4100):
        got = infer.zoom_cubic(np.full((n_in, 2), 100, np.uint8), (224, 2)).cpu().numpy()
        _, _, out_of_range = ref_resize._axis_plan(n_in, 224)
        want = np.where(out_of_range, 0, 100).astype(np.uint8)[:, None].repeat(2, axis=1)
        np.testing.assert_array_equal(got, want, err_msg=f"{n_in} -> 224")
        affected += bool(out_of_range.any())
    assert affected == 222


def _reference_preprocess(img):
    """The reference's formula (test_mc3serousv5.py:115-125) in float64: per-channel z-normalisation over H, W; every HWC input
    has its channels reversed."""
    z = img.astype(np.float64)
    z = (z - np.mean(z, axis=(0, 1))) / np.std(z, axis=(0, 1))
    return z.astype(np.float32)[None, None] if img.ndim == 2 else z.transpose((2, 0, 1))[::-1].astype(np.float32)[None]


@pytest.mark.parametrize("shape,size", [((512, 512, 3), (224, 224)), ((1080, 1920, 3), (512, 512)), ((1000, 1000), (224, 224))])
def test_preprocess_with_resize_at_evaluation_sizes(shape, size):
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from umi import infer
    img = (np.random.default_rng(7).random(shape) * 255).astype(np.uint8)
    x = infer.preprocess(img, input_size=size).cpu().numpy()
    want = _reference_preprocess(ref_resize.zoom_cubic(img, size))
    assert x.shape == want.shape
    np.testing.assert_allclose(x, want, rtol=0, atol=2e-6)


@pytest.mark.parametrize("shape", [(224, 224, 3), (96, 80)])
def test_preprocess_without_resize_when_the_size_matches(shape):
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from umi import infer
    img = (np.random.default_rng(8).random(shape) * 255).astype(np.uint8)
    x = infer.preprocess(img, input_size=shape[:2]).cpu().numpy()
    np.testing.assert_allclose(x, _reference_preprocess(img), rtol=0, atol=2e-6)
    np.testing.assert_array_equal(x, infer.preprocess(img).cpu().numpy())


_ZNORM_IMAGES = {  # name: image from a seeded generator, made in the test rather than at collection
    # 4M pixels: the 512-workgroup reductions take 32 grid strides
    "u8_2048x2048x3": lambda r: (r.random((2048, 2048, 3)) * 255).astype(np.uint8),
    # |mean| >> std: an fp32 accumulation, or a one-pass E[x^2] - E[x]^2 variance even in fp64, is visibly off here
    "f32_mean1e4": lambda r: (1e4 + r.standard_normal((300, 400, 3))).astype(np.float32),
    "f32_mean1e6": lambda r: (1e6 + r.standard_normal((512, 512))).astype(np.float32),
    # C = 1, 2, 4: the reference reverses the channels of every HWC input
    "u8_c1": lambda r: (r.random((64, 80, 1)) * 255).astype(np.uint8),
    "u8_c2": lambda r: (r.random((130, 70, 2)) * 255).astype(np.uint8),
    "u8_c4": lambda r: (r.random((257, 129, 4)) * 255).astype(np.uint8),
    "f32_c4": lambda r: (r.standard_normal((33, 65, 4)) * [1.0, 1e-3, 50.0, 1e3] + [0.0, 7.0, -3.0, 1e5]).astype(np.float32),
}


@pytest.mark.parametrize("name", list(_ZNORM_IMAGES))
def test_preprocess_znorm_matches_float64(name):
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from umi import infer
    img = _ZNORM_IMAGES[name](np.random.default_rng(9))
    x = infer.preprocess(img).cpu().numpy()
    want = _reference_preprocess(img)
    assert x.shape == want.shape
    np.testing.assert_allclose(x, want, rtol=0, atol=2e-6)


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_preprocess_znorm_constant_channel_is_nan(dtype):
    """A constant channel has std 0: the reference divides 0 by 0 and gets NaN in every pixel of it; so does the kernel."""
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from umi import infer
    rng = np.random.default_rng(10)
    img = (rng.random((48, 40, 3)) * 255).astype(np.uint8).astype(dtype)
    img[..., 1] = 7 if dtype == "uint8" else 0.5              # exact in fp64 sums: the mean is exactly the value
    x = infer.preprocess(img).cpu().numpy()
    with np.errstate(invalid="ignore"):
        want = _reference_preprocess(img)
    assert np.isnan(want[0, 1]).all() and not np.isnan(want[0, [0, 2]]).any()
    np.testing.assert_array_equal(np.isnan(x), np.isnan(want))
    np.testing.assert_allclose(x, want, rtol=0, atol=2e-6)     # equal_nan: the other channels to 2e-6
