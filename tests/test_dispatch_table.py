"""The host-side dispatch of libunetmi (csrc/kernels.h: umi_conv_fwd_path, umi_conv_wgrad_path and the workspace bounds) answers
every query of tests/dispatch_grid.py as the commit before the selectors were introduced did (tests/golden/dispatch_table.npz,
recorded from that commit's library by tools/gen_dispatch_table.py), and the predicates carry the refusals that used to surface
only in the launchers.  No GPU needed: these functions launch nothing."""
import ctypes
import os

import numpy as np
import pytest

from tests import dispatch_grid

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dispatch_table.npz")
F16 = dispatch_grid.F16
UPSAMPLE2 = 1
LIMIT_31 = 0x7FFFFFF0


@pytest.fixture(scope="module")
def current():
    from umi import lib
    return dispatch_grid.tables(lib.fn)


def test_grid_is_the_recorded_one():
    g = np.load(GOLDEN)
    n_ch, n_geo, n_shape = len(dispatch_grid.CHANNELS) ** 2, len(dispatch_grid.GEOMETRIES), len(dispatch_grid.SHAPES)
    assert g["plan"].shape == (493920, 3)
    assert g["wgrad_ws"].shape == (n_ch * n_geo * n_shape, 4) and g["wgrad_ws"].size == 21952
    assert g["gather_rows"].shape == (n_ch * n_geo * n_shape, 2)
    assert g["head_rows"].shape == (n_ch * n_shape, 6) and g["head_ws"].shape == (n_ch * n_shape,)
    # the recorded commit's own figures: the table is not degenerate
    assert int((g["plan"][:, 0] == -2).sum()) == 95888 and int((g["plan"][:, 1] == 1).sum()) == 9232
    assert (g["gather_rows"] > 0).any() and (g["head_rows"] > 0).any() and (g["wgrad_ws"] > 0).all()


@pytest.mark.parametrize("name", ["plan", "wgrad_ws", "gather_rows", "head_rows", "head_ws"])
def test_table_is_identical(current, name):
    want = np.load(GOLDEN)[name]
    got = current[name]
    assert got.shape == want.shape and got.dtype == want.dtype
    bad = np.flatnonzero((got != want).reshape(len(want), -1).any(axis=1))
    assert bad.size == 0, f"{name}: {bad.size} rows differ, first {bad[:5]}: got {got[bad[:5]]}, recorded {want[bad[:5]]}"


def _plan(H, W, ldx, flags):
    from umi import lib
    lay, rows = ctypes.c_int(-7), ctypes.c_int(-7)
    st = lib.fn("umi_conv_fwd_plan")(1, H, W, 64, 64, 2, 2, 2, 0, ldx, 64, F16, F16, flags, 0, ctypes.byref(lay), ctypes.byref(rows))
    return st, lay.value, rows.value


@pytest.mark.parametrize("flags", [0, UPSAMPLE2])
def test_source_image_limit_is_in_the_predicate(flags):
    """The tap-gather / transposed-conv kernel addresses two source images with 31-bit byte offsets.  2 * H * W * ldx * 2 at or
    above 0x7FFFFFF0 used to be refused by the launcher only, after the plan had said layout 1."""
    from umi import lib
    H = W = 2048
    assert 2 * H * W * 128 * 2 == 2 ** 31 >= LIMIT_31 and 2 * H * W * 120 * 2 == 2013265920 < LIMIT_31
    st, lay, rows = _plan(H, W, 128, flags)
    assert (st, lay) == (0, 0) and rows > 0
    st, lay, rows = _plan(H, W, 120, flags)
    assert (st, lay) == (0, 1) and rows > 0
    if flags == 0:
        gather = lib.fn("umi_conv_gather_bnred_rows")
        assert gather(1, H, W, 64, 64, 2, 2, 2, 0, H // 2, W // 2, 128, 64, F16, 0) == 0
        assert gather(1, H, W, 64, 64, 2, 2, 2, 0, H // 2, W // 2, 120, 64, F16, 0) > 0
