"""umi_patch_rows (csrc/patch_embed.hip): the P x P patches of an NCHW image as the token-major rows of the patch convolution's
GEMM, against `F.unfold(x, P, stride=P).transpose(1, 2)` cast to the output type.  Pure data movement plus at most one rounding
(fp32 -> fp16, to nearest even, which is torch's cast too): the bar is equality.  Every output lives in a larger NaN-filled
allocation -- a row stride of K + 8, guard rows before and after -- whose other elements must keep their bits."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, F16 = torch.float32, torch.float16
GUARD, PAD = 3, 8

# (B, C, H, W, P), input type, output type, variant
CASES = {
    "vector_f32_f16": ((2, 3, 32, 32, 16), F32, F16, None),
    "vector_f32_f32": ((2, 3, 32, 32, 16), F32, F32, None),
    "vector_f16_f16": ((2, 3, 32, 32, 16), F16, F16, None),
    "p32_grid_2x3": ((1, 3, 64, 96, 32), F32, F16, None),
    "remainder_rows_and_columns_nan": ((1, 3, 40, 52, 16), F32, F16, "nan_remainder"),
    "w_not_multiple_of_4": ((1, 3, 40, 50, 16), F32, F16, None),
    "base_off_by_one_float": ((2, 3, 32, 32, 16), F32, F16, "offset"),
    "p_not_multiple_of_4": ((1, 3, 28, 28, 14), F32, F16, None),
    "one_channel_tiny_patch": ((1, 1, 6, 10, 2), F32, F16, None),
    "past_the_block_cap": ((2, 3, 512, 512, 16), F32, F16, None),          # 2,048 tokens: 1,536 blocks of work, 2,048-block cap
    "past_the_block_cap_elementwise": ((1, 3, 512, 514, 16), F32, F16, None),   # W % 4 != 0: 786,432 elements, 3,072 blocks
}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: torch.cuda.is_available() is False")


def _input(shape, dtype, variant):
    B, C, H, W, P = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, C, H, W, generator=g).to(dtype)
    if variant == "nan_remainder":                      # what a stride-P convolution ignores must never reach the output
        x[:, :, H // P * P:, :] = float("nan")
        x[:, :, :, W // P * P:] = float("nan")
    if variant == "offset":
        buf = torch.empty(x.numel() + 1, dtype=dtype, device=DEV)
        xd = buf[1:].view(B, C, H, W)
        xd.copy_(x)
        assert xd.data_ptr() % 16 == 4 and xd.is_contiguous()
        return x, xd
    return x, x.to(DEV)


def _guarded(M, K, dtype):
    """([GUARD + M + GUARD, K + PAD] NaN-filled allocation, its [M, K] window)."""
    full = torch.full((M + 2 * GUARD, K + PAD), float("nan"), dtype=dtype, device=DEV)
    return full, full[GUARD:GUARD + M, :K]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == F16 else torch.int32)


@pytest.mark.parametrize("name", list(CASES))
def test_patch_rows_equals_unfold(name):
    _need_gpu()
    from umi import ops_tu
    shape, dt_in, dt_out, variant = CASES[name]
    B, C, H, W, P = shape
    x, xd = _input(shape, dt_in, variant)
    M, K = B * (H // P) * (W // P), C * P * P
    want = F.unfold(x[:, :, :H // P * P, :W // P * P].float(), P, stride=P).transpose(1, 2).reshape(M, K).to(dt_out)
    full, rows = _guarded(M, K, dt_out)
    before = _bits(full).clone()
    ops_tu.patch_rows(xd, P, rows)
    full2, rows2 = _guarded(M, K, dt_out)
    ops_tu.patch_rows(xd, P, rows2)
    torch.cuda.synchronize()
    got = rows.cpu()
    assert torch.isfinite(got).all()
    assert torch.equal(got, want)
    assert torch.equal(_bits(rows), _bits(rows2))                          # two calls, identical bits
    # nothing outside rows[0:M, 0:K] was written: the guard rows and the 8 extra columns still hold their NaN bits
    after = _bits(full)
    outside = torch.ones_like(after, dtype=torch.bool)
    outside[GUARD:GUARD + M, :K] = False
    assert torch.equal(after[outside], before[outside])


def test_patch_rows_wrapper_refuses_what_the_kernel_cannot_address():
    _need_gpu()
    from umi import ops_tu
    x = torch.zeros(1, 3, 32, 32, device=DEV)
    with pytest.raises(ValueError, match="contiguous NCHW"):
        ops_tu.patch_rows(x.permute(0, 1, 3, 2), 16, torch.empty(4, 768, device=DEV))
    with pytest.raises(ValueError, match=r"rows \[4, 768\]"):
        ops_tu.patch_rows(x, 16, torch.empty(4, 767, device=DEV))
    with pytest.raises(ValueError, match="contiguous columns"):
        ops_tu.patch_rows(x, 16, torch.empty(768, 4, device=DEV).t())
