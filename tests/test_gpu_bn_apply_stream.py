"""The streaming BatchNorm-backward apply pass (elementwise_f16.hip bn_bwd_apply_v8: constants once per workgroup, a
contiguous row range per workgroup, four row pairs in flight per lane) against the generic fp16 kernel, bit for bit.

Both run through umi_bn_bwd_apply.  The vector kernel takes 16-B aligned bases; the same values in a buffer whose `da` base
sits one element (2 B) off alignment fall to bn_bwd_apply_kernel<half_t>.  Every case also checks that nothing outside the
target is written: guard rows in front of and behind it, and the other channels of a wider (sliced) buffer, hold a sentinel
that is compared afterwards."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 3                      # guard rows on either side of the target
SENTINEL = -1234.0             # exact in fp16; no input or output value is drawn near it


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from umi import lib, ops
    return lib, ops


def _rows_per_workgroup(C):
    """Rows a workgroup of the streaming kernel owns on a SMALL tensor (the floor of its grid rule: 8 rows per lane, 256
    lanes spread over min(C/8, 64) channel groups)."""
    return 8 * (256 // min(C // 8, 64))


def _bits(t):
    return t.contiguous().view(torch.int16)


def _constants(M, C, lo, g):
    t = torch.empty(C, 4)
    t[:, 0] = 0.1 * torch.randn(C, generator=g)                                                 # batch mean
    t[:, 1] = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.25, -1.0, 1.0)   # gamma*rstd
    t[:, 2] = 0.2 * torch.randn(C, generator=g)
    t[:, 3] = lo
    rstd = 0.5 + torch.rand(C, generator=g)
    sums = torch.randn(2, C, generator=g) * 0.05 * M                                            # c1, c2 of order 0.05
    return t.to(DEV).contiguous(), rstd.to(DEV), sums.to(DEV)


def _framed(vals, ld, col, misalign):
    """[GUARD + M + GUARD, ld] fp16 buffer of sentinels with `vals` ([M, C]) at rows GUARD.., columns col..col+C.  misalign:
    the whole buffer starts one element into a larger allocation (its base is then 2 B off 16-B alignment)."""
    M, C = vals.shape
    n = (M + 2 * GUARD) * ld
    raw = torch.full((n + 8,), SENTINEL, dtype=torch.float16, device=DEV)
    buf = raw[1:1 + n] if misalign else raw[:n]
    buf = buf.view(M + 2 * GUARD, ld)
    buf[GUARD:GUARD + M, col:col + C] = vals
    assert (buf.data_ptr() % 16 != 0) == bool(misalign)
    return buf


def _apply(lib, buf, ld, col, ybuf, ldy, ycol, td, rstd, sums, M, C):
    da_ptr = buf.data_ptr() + 2 * (GUARD * ld + col)
    y_ptr = ybuf.data_ptr() + 2 * (GUARD * ldy + ycol)
    lib.check(lib.fn("umi_bn_bwd_apply")(da_ptr, ld, y_ptr, ldy, td.data_ptr(), rstd.data_ptr(), sums[0].data_ptr(),
                                         sums[1].data_ptr(), M, C, lib.UMI_F16, torch.cuda.current_stream().cuda_stream),
              "umi_bn_bwd_apply")


def _check_frame(buf, before, M, C, col):
    """Everything but the target still holds what it held (the sentinel)."""
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[GUARD:GUARD + M, col:col + C] = False
    assert torch.equal(_bits(buf[mask]), _bits(before[mask]))
    assert bool((buf[mask] == SENTINEL).all())


def _run(M, C, lo, ldda=None, col=0, ldy=None, ycol=0, seed=0):
    lib, _ = _gpu()
    ldda = ldda or C
    ldy = ldy or C
    g = torch.Generator().manual_seed(1000 * seed + C + M % 997)
    td, rstd, sums = _constants(M, C, lo, g)
    gd = torch.Generator(device=DEV).manual_seed(seed + C)
    y = torch.randn(M, C, device=DEV, generator=gd).half()
    da = (0.1 * torch.randn(M, C, device=DEV, generator=gd)).half()
    ybuf = _framed(y, ldy, ycol, False)
    y_before = ybuf.clone()
    vec, gen = _framed(da, ldda, col, False), _framed(da, ldda, col, True)
    vec_before = vec.clone()
    gen_before = gen.clone()
    _apply(lib, vec, ldda, col, ybuf, ldy, ycol, td, rstd, sums, M, C)
    _apply(lib, gen, ldda, col, ybuf, ldy, ycol, td, rstd, sums, M, C)
    torch.cuda.synchronize()
    out_vec, out_gen = vec[GUARD:GUARD + M, col:col + C], gen[GUARD:GUARD + M, col:col + C]
    assert torch.equal(_bits(out_vec), _bits(out_gen))
    assert not torch.equal(_bits(out_vec), _bits(da))                 # the pass did run
    assert bool(torch.isfinite(out_vec).all())
    _check_frame(vec, vec_before, M, C, col)
    _check_frame(gen, gen_before, M, C, col)
    assert torch.equal(_bits(ybuf), _bits(y_before))
    # a second launch on identical inputs: identical bits
    again = _framed(da, ldda, col, False)
    _apply(lib, again, ldda, col, ybuf, ldy, ycol, td, rstd, sums, M, C)
    torch.cuda.synchronize()
    assert torch.equal(_bits(again), _bits(vec))


LO = [0.0, float("-inf")]

# the five (M, C) of the benchmark's U-Net levels at N = 2, and the two deepest at the benchmark's batch of 16
LEVELS = [(2 * 512 * 512, 64), (2 * 256 * 256, 128), (2 * 128 * 128, 256), (2 * 64 * 64, 512), (2 * 32 * 32, 1024),
          (16 * 32 * 32, 1024), (16 * 64 * 64, 512)]


@pytest.mark.parametrize("lo", LO)
@pytest.mark.parametrize("M,C", LEVELS)
def test_stream_apply_matches_generic_on_unet_levels(M, C, lo):
    _run(M, C, lo, seed=1)


@pytest.mark.parametrize("lo", LO)
@pytest.mark.parametrize("C", [8, 64, 2048])
def test_stream_apply_matches_generic_channel_extremes(C, lo):
    _run(2 * 12 * 20, C, lo, seed=2)


def _ragged_rows():
    out = [(1 * 37 * 53, C) for C in (16, 64, 512, 1024)] + [(1, 64), (3, 1024), (5, 8)]
    for C in (8, 64, 256, 512, 1024, 2048):
        r = _rows_per_workgroup(C)
        out += [(r - 1, C), (r + 1, C), (3 * r - 1, C), (3 * r + 1, C)]
    return out


@pytest.mark.parametrize("lo", LO)
@pytest.mark.parametrize("M,C", _ragged_rows())
def test_stream_apply_matches_generic_ragged_rows(M, C, lo):
    _run(M, C, lo, seed=3)


# (M, C, ldda, first da channel, ldy, first y channel): the upper half of a concat buffer, y inside a wider tensor
SLICES = [(1 * 37 * 53, 64, 128, 64, 64, 0), (2 * 24 * 24, 128, 256, 128, 136, 8), (2 * 16 * 16, 512, 1024, 512, 512, 0),
          (1 * 19 * 23, 1024, 2048, 1024, 1040, 16), (2 * 64 * 64, 256, 512, 256, 264, 0), (1 * 9 * 11, 8, 16, 8, 24, 16),
          (2 * 12 * 20, 2048, 4096, 2048, 2048, 0), (1 * 37 * 53, 64, 128, 0, 72, 8)]


@pytest.mark.parametrize("lo", LO)
@pytest.mark.parametrize("case", SLICES)
def test_stream_apply_matches_generic_in_channel_slices(case, lo):
    M, C, ldda, col, ldy, ycol = case
    _run(M, C, lo, ldda=ldda, col=col, ldy=ldy, ycol=ycol, seed=4)
