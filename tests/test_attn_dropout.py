"""Attention-probability dropout, the parts that need no device: the float64 restatement against the decomposition the kernels
implement, the preconditions of the GPU read-out tests, and the C ABI's argument checks (tests/attn_dropout_cases.py)."""
import ctypes

import pytest
import torch

from tests import attn_dropout_cases as cases


def test_autograd_of_the_restatement_equals_the_decomposition():
    """delta = rowsum(dO o O), dS = P o (Z o dP - delta), dV = (P o Z)^T dO against float64 autograd of O = (P o Z) V, with the
    stream's mask under a seed >= 2^31 and a device counter."""
    shape, D, p = (2, 70, 3), 64, 0.25
    assert cases.SEED >= 2 ** 31
    x = cases.inputs(shape, D)
    m = cases.keep(shape, p, cases.SEED, cases.COUNTER)
    assert 0.70 < m.double().mean().item() < 0.80                 # 29,400 draws at 1 - p = 0.75: 4 sigma is 0.01
    auto, hand = cases.evaluate(x, m, p, shape, D), cases.decomposition(x, m, p, shape, D)
    for n in cases.OUTS:
        err, top = cases.error(hand[n], auto[n])
        print(f"{n}: {err:.3e} of {top:.3e}")
        assert err <= 1e-12 * max(top, 1.0), (n, err, top)
    # and the counter matters: another counter is another mask
    assert not torch.equal(m, cases.keep(shape, p, cases.SEED, cases.COUNTER + 1))


READOUTS = sorted({(shape, f["D"]) for f in cases.FAMILIES.values() for shape in f["readout"]})


@pytest.mark.parametrize("shape,D", READOUTS)
def test_readout_preconditions_in_float64(shape, D):
    """What the GPU read-out tests rely on, in exact-enough arithmetic: the zero pattern of O is the mask, the sign of dQ is the
    mask, and |dQ| over a window spans less than a factor 5 (so no element is near a rounding's reach of zero)."""
    p = cases.READOUT_P
    m = cases.keep(shape, p, cases.SEED, cases.COUNTER)
    worst = 1.0
    for r0 in cases.windows(shape[1], D):
        ref = cases.decomposition(cases.readout("o", shape, D, r0), m, p, shape, D)
        assert torch.equal(cases.shown("o", ref, shape, D, r0), cases.window_of_mask("o", m, shape, D, r0)), r0
        ref = cases.decomposition(cases.readout("dv", shape, D, r0), m, p, shape, D)
        assert torch.equal(cases.shown("dv", ref, shape, D, r0), cases.window_of_mask("dv", m, shape, D, r0)), r0
        ref = cases.decomposition(cases.readout("dq", shape, D, r0), m, p, shape, D)
        assert torch.equal(cases.shown("dq", ref, shape, D, r0), cases.window_of_mask("dq", m, shape, D, r0)), r0
        w = cases.window_of_output(ref["dq"], shape, D, r0).abs()
        worst = min(worst, (w.min() / w.max()).item())
    print(f"{shape} D={D}: min |dQ| / max |dQ| over a window = {worst:.3f}")
    assert worst >= 0.2


def test_c_abi_checks_p_before_anything_else():
    from umi import lib
    assert "umi_attn_fwd_dropout" in lib.SIGNATURES and "umi_attn_bwd_dropout" in lib.SIGNATURES
    fwd, bwd = lib.fn("umi_attn_fwd_dropout"), lib.fn("umi_attn_bwd_dropout")
    for p in (-0.1, 1.5, float("nan")):                           # null pointers: nothing is launched, no device is touched
        assert fwd(None, None, None, 64, None, 64, None, 1, 8, 1, 64, lib.UMI_F32, 0, p, 0, None, None) == lib.UMI_ERR_BADARG
        assert bwd(None, None, None, 64, None, None, 64, None, None, None, None, 64, None, 1, 8, 1, 64, lib.UMI_F32, 0,
                   p, 0, None, None) == lib.UMI_ERR_BADARG
    # a head dimension no kernel knows is refused before a launch too (host addresses stand in for the tensors: never read)
    buf = (ctypes.c_float * 1024)()
    a = ctypes.addressof(buf)
    for dt in (lib.UMI_F32, lib.UMI_F16):
        for p in (0.0, 0.5, 1.0):
            assert fwd(a, a, a, 48, a, 48, a, 1, 4, 1, 48, dt, 0, p, 0, None, None) == lib.UMI_ERR_UNSUPPORTED
            assert bwd(a, a, a, 48, a, a, 48, a, a, a, a, 48, a, 1, 4, 1, 48, dt, 0, p, 0, None, None) == lib.UMI_ERR_UNSUPPORTED
            assert bwd(a, a, a, 48, a, a, 48, a, a, a, a, 48, a, 1, 4, 1, 48, dt, lib.UMI_ATTN_F32_MFMA, p, 0, None, None) \
                == lib.UMI_ERR_UNSUPPORTED
