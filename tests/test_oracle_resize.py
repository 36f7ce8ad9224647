"""CPU: the resize oracle (oracle/ref_resize.py, SciPy's cubic-spline zoom restated) against outputs of SciPy itself
(tests/golden/zoom_cubic.npz, tools/gen_golden_resize.py) and, where SciPy is importable, against SciPy directly."""
import os

import numpy as np
import pytest

from oracle import ref_resize
from tools import gen_golden_resize as G


@pytest.mark.parametrize("i", range(len(G.CASES)))
def test_zoom_oracle_matches_scipy_fixture(golden_dir, i):
    g = np.load(os.path.join(golden_dir, "zoom_cubic.npz"))
    seed, shape, ohw, dtype = G.CASES[i]
    img = G.make(seed, shape, dtype)
    got = ref_resize.zoom_cubic(img, ohw)
    want = g[f"case{i}"]
    assert got.shape == want.shape and got.dtype == want.dtype
    if dtype == "uint8":
        np.testing.assert_array_equal(got, want)
    else:
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-6)


def test_zoom_oracle_matches_scipy_live():
    zoom = pytest.importorskip("scipy.ndimage").zoom
    rng = np.random.default_rng(11)
    img = (rng.random((45, 61, 3)) * 255).astype(np.uint8)
    np.testing.assert_array_equal(ref_resize.zoom_cubic(img, (96, 32)), zoom(img, (96 / 45, 32 / 61, 1), order=3))


def _scipy_zoom(img, ohw):
    zoom = pytest.importorskip("scipy.ndimage").zoom
    return zoom(img, (ohw[0] / img.shape[0], ohw[1] / img.shape[1]) + ((1,) if img.ndim == 3 else ()), order=3)


@pytest.mark.parametrize("n_out", [224, 256, 512])
def test_zoom_oracle_zeroes_out_of_range_samples_like_scipy(n_out):
    """mode='constant': SciPy writes cval = 0 where the sample coordinate x = i * ((n_in - 1) / (n_out - 1)) is > n_in - 1.
    A constant strip is 100 inside and 0 there, so its zeros are exactly SciPy's out-of-range samples."""
    pytest.importorskip("scipy.ndimage")
    affected = 0
    for n_in in range(2, 4100):
        strip = np.full((n_in, 2), 100, np.uint8)
        want = _scipy_zoom(strip, (n_out, 2))
        _, _, out_of_range = ref_resize._axis_plan(n_in, n_out)
        np.testing.assert_array_equal(out_of_range, want[:, 0] == 0, err_msg=f"{n_in} -> {n_out}")
        affected += bool(out_of_range.any())
        # the whole resize where the rule bites, and at every small size (the oracle's prefilter is a Python loop over n_in)
        if out_of_range.any() or n_in <= 300:
            np.testing.assert_array_equal(ref_resize.zoom_cubic(strip, (n_out, 2)), want, err_msg=f"{n_in} -> {n_out}")
    if n_out == 224:
        assert affected == 222          # 32, 58, ..., 512, 1000, 1920, 2048, ...: the rule is exercised, not vacuous


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("i", range(len(G.SWEEP)))
def test_zoom_oracle_matches_scipy_sweep(i, dtype):
    shape, ohw = G.SWEEP[i]
    img = G.make(100 + i, shape, dtype)
    want = _scipy_zoom(img, ohw)
    got = ref_resize.zoom_cubic(img, ohw)
    assert got.shape == want.shape and got.dtype == want.dtype
    if dtype == "uint8":
        tie = ref_resize.halfway(img, ohw)
        np.testing.assert_array_equal(got[~tie], want[~tie])
        assert np.all(np.abs(got[tie].astype(int) - want[tie]) <= 1)
    else:
        # within one float32 ulp of SciPy's value (SciPy rounds a float64 that differs from ours in the last bits)
        err = np.abs(got.astype(np.float64) - want)
        assert np.all(err <= np.spacing(np.abs(want)) + 1e-9), err.max()
