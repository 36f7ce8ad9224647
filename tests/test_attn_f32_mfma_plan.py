"""Host-side contract of the opt-in fp32 matrix-core attention (UMI_ATTN_F32_MFMA = 1, compute_dtype "fp32_mfma_attn"): where
umi_attn_plan names it (kernel 2), and that the flag is IGNORED -- the answer is the flag-less one -- wherever the new kernels do
not apply.  Pure host code of libunetmi: no GPU is touched, the pointers handed to the plan are plain integers."""
import ctypes
import itertools

import pytest

from tests import attn_f32_cases as cases

F32, F16 = 0, 1
FLAG = 1
BADARG = -1
BASE = 0x7F0000001000          # a 16-byte aligned "address"; the plan only looks at alignment


def _plan(N=196, heads=12, D=64, ld=768, ldo=768, ldd=0, dtype=F32, flags=FLAG, q=BASE, k=BASE + 256, v=BASE + 512, o=BASE + 1024):
    from umi import lib
    kernel = ctypes.c_int(-7)
    status = lib.fn("umi_attn_plan")(N, heads, D, ld, ldo, ldd, dtype, flags, q, k, v, o, ctypes.byref(kernel))
    return status, kernel.value


def test_names_and_constants():
    import torch
    import Model
    from umi import lib
    assert lib.UMI_ATTN_F32_MFMA == FLAG == 1
    assert Model._resolve_dtype("fp32_mfma_attn") is torch.float32
    with pytest.raises(ValueError, match="fp32_mfma_attn"):
        Model._resolve_dtype("fp33")
    assert Model._resolve_conv_flags("fp32_mfma_attn") == Model._resolve_conv_flags("fp32_mfma_gemm") == (16, 32)
    assert Model._resolve_attn_flags("fp32_mfma_attn") == FLAG
    for name in ("fp16", "fp32", "fp32_mfma", "fp32_mfma_gemm"):
        assert Model._resolve_attn_flags(name) == 0, name


def test_the_mode_comes_from_the_environment_too(monkeypatch):
    import torch
    import Model
    monkeypatch.setenv("UMI_COMPUTE_DTYPE", "fp32_mfma_attn")
    assert Model._resolve_dtype(None) is torch.float32
    assert Model._resolve_conv_flags(None) == (16, 32) and Model._resolve_attn_flags(None) == FLAG
    monkeypatch.setenv("UMI_COMPUTE_DTYPE", "fp32_mfma_gemm")
    assert Model._resolve_attn_flags(None) == 0


def test_plan_names_the_fp32_matrix_core_kernel():
    for N, heads, ld, ldo, ldd in itertools.product((1, 17, 196, 1024), (1, 12), (768, 2304), (768, 772), (0, 768, 2304)):
        assert _plan(N=N, heads=heads, ld=ld, ldo=ldo, ldd=ldd) == (0, 2), (N, heads, ld, ldo, ldd)
    # null pointers: "not given, assume fine"
    assert _plan(q=None, k=None, v=None, o=None) == (0, 2)


def test_without_the_flag_every_fp32_plan_is_the_valu_kernel():
    for N, ld, ldd, D in itertools.product((1, 196, 1024), (768, 2304), (0, 2304), (16, 32, 64)):
        assert _plan(N=N, ld=ld, ldd=ldd, D=D, flags=0) == (0, 0), (N, ld, ldd, D)


def test_flag_is_ignored_where_the_kernel_does_not_apply():
    for D in (16, 32):
        assert _plan(D=D, ld=12 * D, ldo=12 * D) == _plan(D=D, ld=12 * D, ldo=12 * D, flags=0) == (0, 0)
    for ld in (769, 770, 771, 2305):
        assert _plan(ld=ld) == _plan(ld=ld, flags=0) == (0, 0), ld
    assert _plan(ldo=770) == (0, 0) and _plan(ldd=770) == (0, 0) and _plan(ldo=769, ldd=2304) == (0, 0)
    for which in ("q", "k", "v", "o"):                        # 4-byte but not 16-byte aligned
        for off in (4, 8, 12):
            assert _plan(**{which: BASE + off}) == _plan(flags=0, **{which: BASE + off}) == (0, 0), (which, off)


def test_fp16_takes_its_own_kernel_with_and_without_the_flag():
    for flags, N, ldd in itertools.product((0, FLAG), (196, 1024), (0, 768, 2304)):
        assert _plan(dtype=F16, flags=flags, N=N, ldd=ldd) == (0, 1), (flags, N, ldd)
    # and its own refusals stay what they were: a stride that is no multiple of 8 halves, head dimension 32
    for flags in (0, FLAG):
        assert _plan(dtype=F16, flags=flags, ld=772) == (0, 0)
        assert _plan(dtype=F16, flags=flags, D=32, ld=384, ldo=384) == (0, 0)


def test_bad_arguments():
    from umi import lib
    assert _plan(N=0)[0] == BADARG and _plan(N=-3)[0] == BADARG and _plan(heads=0)[0] == BADARG
    assert _plan(dtype=7)[0] == BADARG
    assert lib.fn("umi_attn_plan")(196, 12, 64, 768, 768, 0, F32, FLAG, BASE, BASE, BASE, BASE, None) == BADARG


def test_the_tape_passes_its_flag_on(monkeypatch):
    import torch
    from umi import graph, graph_tu, ops_tu
    seen = []

    def attn_fwd(q, k, v, o, heads, flags=0):
        seen.append(("fwd", flags))
        return torch.zeros(q.shape[0] * heads * q.shape[2])

    def attn_bwd(q, k, v, o, dO, lse, dq, dk, dv, heads, flags=0):
        seen.append(("bwd", flags))

    monkeypatch.setattr(ops_tu, "attn_fwd", attn_fwd)
    monkeypatch.setattr(ops_tu, "attn_bwd", attn_bwd)
    for flags in (0, FLAG):
        t = graph_tu.TUTape(torch.float32, training=True, record=True)
        assert t.attn_flags == 0                              # no mode set: no flag
        t.attn_flags = flags
        q, k, v = (graph.Act(torch.zeros(1, 1, 5, 128)) for _ in range(3))
        o = t.attention(q, k, v, 2)
        o.grad = torch.zeros_like(o.raw)
        t.steps[-1]()
        assert seen == [("fwd", flags), ("bwd", flags)]
        seen.clear()


@pytest.mark.parametrize("shape", cases.SHAPES)
def test_a_float32_evaluation_of_the_formula_stays_inside_the_bars_of_the_gpu_test(shape):
    """The bars tests/test_gpu_attn_f32_mfma.py holds the kernels to are attainable in fp32: torch's own float32 evaluation of
    softmax(QK^T/8)V and its autograd, on the CPU, stays inside them against float64 at every shape of that test."""
    import torch
    x, ref = cases.case(shape)
    cases.assert_inside_bars(cases.evaluate(x["q"], x["k"], x["v"], x["dO"], *shape, torch.float32), ref, f"float32 torch {shape}")
