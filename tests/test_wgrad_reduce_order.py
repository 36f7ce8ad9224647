"""The NumPy statement of the split-K reduction order (tests/wgrad_reduce_order.py) against float64, on the CPU.

tests/test_gpu_wgrad_reduce.py demands that the device kernels reproduce these two functions bit for bit; here the functions
themselves are held to the arithmetic they claim: exact on integers, inside the a-priori bound of recursive summation on
normal data, and the documented ORDER on inputs built so that another order rounds differently."""
import numpy as np
import pytest

from tests.wgrad_reduce_order import error_bound, reduce_one_chain, reduce_two_chains, reference_f64

SPLITS = [1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 33, 64]
FORMS = [reduce_one_chain, reduce_two_chains]
SHAPE = (3, 5, 37)          # [tap][ci][co]: the reduction is element-wise, any shape serves


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f.__name__)
@pytest.mark.parametrize("splits", SPLITS)
def test_integer_slabs_reduce_exactly(form, splits):
    rng = np.random.default_rng(100 + splits)
    part = rng.integers(-64, 65, (splits,) + SHAPE).astype(np.float32)
    for scale in (0.5, 4.0, 2.0 ** -10):
        got = form(part, scale)
        assert got.dtype == np.float32 and got.shape == SHAPE
        assert np.array_equal(got.astype(np.float64), reference_f64(part, scale))


@pytest.mark.parametrize("form", FORMS, ids=lambda f: f.__name__)
@pytest.mark.parametrize("splits", SPLITS)
def test_normal_slabs_stay_inside_the_summation_bound(form, splits):
    rng = np.random.default_rng(200 + splits)
    part = rng.standard_normal((splits,) + SHAPE).astype(np.float32)
    got = form(part, 0.37)
    err = np.abs(got.astype(np.float64) - reference_f64(part, 0.37))
    bound = error_bound(part, 0.37)
    print("splits", splits, form.__name__, "worst err / bound", float((err / bound).max()))
    assert (err <= bound).all()


B = 2.0 ** 24               # fp32 spacing is 2 from here on: B + 1 rounds back to B, B + 3 to B + 4


def _col(*vals):
    return np.array(vals, np.float32).reshape(-1, 1)


def test_lane_sums_are_added_in_lane_order():
    """8 splits = one term per lane.  Big term first: every later + 1 is rounded away.  Big term last: 1 + ... + 1 = 7 is exact,
    then 7 + 2^24 lies midway between 2^24 + 6 and 2^24 + 8 and rounds to the even mantissa, 2^24 + 8."""
    for form in FORMS:
        assert form(_col(B, 1, 1, 1, 1, 1, 1, 1), 1.0)[0] == B
        assert form(_col(1, 1, 1, 1, 1, 1, 1, B), 1.0)[0] == B + 8


def test_one_chain_and_two_chains_differ_where_documented():
    """Lane 0 of 17 splits owns z = 0, 8, 16 = (1, 2^24, 1); the other lanes are zero.
    One chain: (1 + 2^24) + 1 = 2^24 + 1 -> 2^24, both times.  Two chains: a = 1 + 1 (z = 0 and the trailing z = 16),
    b = 2^24, a + b = 2^24 + 2 exactly."""
    part = np.zeros((17, 1), np.float32)
    part[0], part[8], part[16] = 1.0, B, 1.0
    assert reduce_one_chain(part, 1.0)[0] == B
    assert reduce_two_chains(part, 1.0)[0] == B + 2
    # with 25 splits lane 0 owns z = 0, 8, 16, 24: the loop takes the pairs (0, 8) and (16, 24), nothing trails:
    # a = part[0] + part[16], b = part[8] + part[24]
    part = np.zeros((25, 1), np.float32)
    part[0], part[8], part[16], part[24] = 1.0, B, 1.0, 2.0
    assert reduce_two_chains(part, 1.0)[0] == B + 4         # (1 + 1) + (2^24 + 2), exact
    assert reduce_one_chain(part, 1.0)[0] == B + 2          # ((1 + 2^24) + 1) + 2: the ones are lost
    # 24 splits: lane 0 owns z = 0, 8, 16 like above; lane 7 owns z = 7, 15, 23 with the trailing term at z = 23
    part = np.zeros((24, 1), np.float32)
    part[7], part[15], part[23] = 1.0, B, 1.0
    assert reduce_two_chains(part, 1.0)[0] == B + 2
    assert reduce_one_chain(part, 1.0)[0] == B


def test_scale_is_applied_once_after_the_sum():
    """(1 + 2^24) * 3 with the scale applied last is 2^24 * 3; applied per term it would be 3 + 3 * 2^24, which rounds up to
    3 * 2^24 + 4 (a power-of-two scale commutes with rounding and could not tell the two apart)."""
    for form in FORMS:
        assert form(_col(1, B), 3.0)[0] == 3 * B
