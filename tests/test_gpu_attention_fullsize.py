"""The attention U-Net's gate kernels at the production shapes and calling conventions of UNet_attention(1, 2, 64), B = 16 at
512 x 512, element by element against float64 references.

A gate (reference Model.py:265-305) runs, on top of the kernels the plain U-Net shares:
  * umi_gate_fwd / _bwd   y = tx_x(x) * A, A = sigmoid(tx_p(p));  dx = dy * A;  dp = A (1 - A) sum_c dy tx_x(x)
                          (gate_kernels.hip: 16-byte `*_v8` kernels for fp16 with C/8 a power of two <= 64 and 16-byte-aligned
                          rows, the scalar kernels otherwise);
  * umi_add2_relu_fwd / _bwd   E = relu(tx_q(q1) + tx_x(x1)) of the two hidden-width branches;
  * the psi branch: a 1x1 conv C_hidden -> 1 with its statistics epilogue, bn_finalize and the BatchNorm backward with C = 1;
  * the W_q / W_x branches: the pointwise matrix-core conv without statistics, then bn_stats (the two-pass form).
The gate writes into the decoder's concat buffer (cat[..., :C], ld = 2C) and takes its dy from the same slice of the concat
gradient, so the tables below run those strides; output buffers and the unused columns of strided ones are prefilled with
NaN.  Exact cases use small integers with A in {0, 1/2, 1}, so every output is representable and must be equal bit for bit;
random cases use |y - ref| <= (a |ref| + b s) u + f (see tests/test_gpu_tu_fullsize.py::_check), each b with its measured
worst case.

`test_model_calls_are_covered` records every configuration the model passes to these kernels and requires each to appear in
the tables, batch aside."""
import pytest
import torch

from tests.test_gpu_exact import _int_tx, _ints
from tests.test_gpu_tu_fullsize import SUB16, U16, U32, _check, _kernels, _nan

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, F32 = torch.float16, torch.float32
SUB32 = 2.0 ** -120                  # absolute floor of the fp32 outputs: sigmoid(z) under-/overflows to 0 below z ~ -88


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from umi import ops
    return ops


# (N, H, W, C_x, C_hidden, C_q) of the four gates of UNet_attention(1, 2, 64) at B = 16, 512 x 512: attenion1 .. attenion4
GATES = [(16, 512, 512, 64, 32, 128), (16, 256, 256, 128, 64, 256), (16, 128, 128, 256, 128, 512),
         (16, 64, 64, 512, 256, 1024)]
# gate kernel cases (N, H, W, C, width, off, dtype): the output / dy view is buf[..., off:off + C] of an [N, H, W, width] buffer
GATE_CASES = [(N, H, W, C, 2 * C, 0, F16) for N, H, W, C, _, _ in GATES] + [
    (16, 512, 512, 32, 64, 0, F16),          # UNet_attention(.., 32).attenion1: G = 4
    (2, 64, 64, 1024, 2048, 0, F16),         # G = 128: scalar kernel
    (16, 256, 256, 24, 48, 0, F16),          # C % 8 != 0: scalar kernel, capped grid (M > 16,384 x 16 pixels)
    (4, 128, 128, 64, 129, 0, F16),          # odd ld
    (4, 128, 128, 64, 128, 1, F16),          # base one element off 16-byte alignment
    (4, 128, 128, 64, 128, 0, F32),          # fp32
]
# add2_relu cases (N, H, W, C, width, off, dtype): hidden widths; y / dy views as above
ADD_CASES = [(N, H, W, Ch, Ch, 0, F16) for N, H, W, _, Ch, _ in GATES] + [
    (16, 512, 512, 16, 16, 0, F16),          # UNet_attention(.., 32).attenion1: G = 2
    (16, 128, 128, 24, 24, 0, F16),          # C % 8 != 0
    (4, 128, 128, 32, 33, 0, F16),           # odd ld
    (4, 128, 128, 32, 64, 1, F16),           # misaligned base
    (4, 128, 128, 32, 32, 0, F32),           # fp32
]


def _vec(C, width, off, dtype):
    """gate_vec_ok: the path the case must take (dense operands from the allocator are 16-byte aligned)."""
    G = C // 8
    return dtype == F16 and C % 8 == 0 and G <= 64 and (G & (G - 1)) == 0 and width % 8 == 0 and off % 8 == 0


def _cid(c):
    N, H, W, C, width, off, dt = c
    return f"{N}x{H}x{W}x{C}-ld{width}-off{off}-{'f16' if dt == F16 else 'f32'}"


def _slice_buf(N, H, W, C, width, off, dt):
    buf = _nan(N, H, W, width, dtype=dt)
    return buf, buf[..., off:off + C]


def _untouched(buf, off, C):
    return bool(torch.isnan(buf[..., :off]).all()) and bool(torch.isnan(buf[..., off + C:]).all())


def _dev_tx(t):
    return t.to(DEV).contiguous()


def _tx64(v, t):
    """float64 consumer transform max(v * scale + shift, lo) with fp32 rows t [C, 4] (None: identity)."""
    if t is None:
        return v
    t = t.double()
    return torch.maximum(v * t[:, 1] + t[:, 2], t[:, 3])


def _gate_ref(x, txx, p, txp, dy):
    """float64 gate forward / backward of one image (x, dy [.., C], p [.., 1]); returns y, dx, dp, z, S, sum |dy tx(x)|."""
    xt = _tx64(x.double(), txx)
    z = _tx64(p.double(), txp)
    A = torch.sigmoid(z)
    g = dy.double()
    S = (g * xt).sum(-1, keepdim=True)
    return xt * A, g * A, A * (1 - A) * S, z, A, S, (g * xt).abs().sum(-1, keepdim=True)


def _run_gate(ops, case, x, txx, p, txp, dyv, check_path=True):
    N, H, W, C, width, off, dt = case
    ybuf, y = _slice_buf(N, H, W, C, width, off, dt)
    dx, dp = _nan(N, H, W, C, dtype=dt), _nan(N, H, W, 1, dtype=dt)
    if check_path:
        vec = _vec(C, width, off, dt)
        kf = _kernels(lambda: ops.gate(x, txx, p, txp, y))
        kb = _kernels(lambda: ops.gate_bwd(dyv, x, txx, p, txp, dx, dp))
        assert ("gate_fwd_v8" in kf) == vec and ("gate_fwd_kernel" in kf) != vec, kf
        assert ("gate_bwd_v8" in kb) == vec and ("gate_bwd_kernel" in kb) != vec, kb
    else:
        ops.gate(x, txx, p, txp, y)
        ops.gate_bwd(dyv, x, txx, p, txp, dx, dp)
    torch.cuda.synchronize()
    assert _untouched(ybuf, off, C), "gate wrote outside its channel slice"
    return y, dx, dp


# ========================================================================================================================
# a. gate, exact: small-integer x / dy, integer transform rows, z in {-200, 0, 200} per pixel -> A in {0, 1/2, 1} exactly
#    (expf(200) overflows: A = 1 / (1 + inf) = 0; float64's sigmoid(-200) = 1.4e-87 rounds to 0 in fp16 and fp32 alike)
# ========================================================================================================================
@pytest.mark.parametrize("tx", ["both", "none"])
@pytest.mark.parametrize("case", GATE_CASES, ids=_cid)
def test_gate_exact(case, tx):
    ops = _gpu()
    N, H, W, C, width, off, dt = case
    g = torch.Generator(device=DEV).manual_seed(N * H + C + width + off)
    gc = torch.Generator().manual_seed(C)
    x = torch.randint(-3, 4, (N, H, W, C), generator=g, device=DEV).to(dt)
    dybuf, dyv = _slice_buf(N, H, W, C, width, off, dt)
    dyv.copy_(torch.randint(-2, 3, (N, H, W, C), generator=g, device=DEV))
    code = torch.randint(0, 3, (N, H, W, 1), generator=g, device=DEV)        # 0, 1, 2 -> A = 0, 1/2, 1
    if tx == "both":
        txx = _dev_tx(_int_tx(C, gc))                                         # scale +-1 / 2, integer shift, ReLU (lo = 0)
        txp = torch.tensor([[0.0, 200.0, -200.0, float("-inf")]], device=DEV)  # psi's BatchNorm: no ReLU
        p = code.to(dt)
    else:
        txx = txp = None
        p = ((code - 1) * 200).to(dt)
    y, dx, dp = _run_gate(ops, case, x, txx, p, txp, dyv)
    for n in range(N):
        ry, rdx, rdp, z, A, S, _ = _gate_ref(x[n], txx, p[n], txp, dyv[n])
        assert torch.equal(torch.unique(z), torch.tensor([-200.0, 0.0, 200.0], device=DEV, dtype=torch.float64))
        assert S.abs().max().item() < 2048                                     # A(1-A) S = S/4 is an fp16 number
        assert torch.equal(y[n].double(), ry.to(dt).double()), n
        assert torch.equal(dx[n].double(), rdx.to(dt).double()), n
        assert torch.equal(dp[n].double(), rdp.to(dt).double()), n


# ========================================================================================================================
# b. gate, random, against float64.  Rounding model (fp32 arithmetic, one rounding per step):
#    z = fma(p, s, t): relative U32, which moves A by A (1 - A) |z| U32;  expf and the division: a few U32 of A;  tx_x(x)
#    one U32;  the products one U32 each.  y, dx: s = |ref| (4 + (1 - A)|z|) in U32.  dp: the fp32 dot product over C
#    channels, s = A (1 - A) (C sum_c |dy tx(x)| + (6 + |z|) |S|) + A |S| in U32 (the last term: 1 - A of an A rounded to
#    fp32 near 1 loses all its digits, e.g. z = 20).  The fp16 store is a = 1 at u = U16; s is scaled to U16 units there.
# ========================================================================================================================
def _bound_gate(name, got, ref, s32, dt):
    if dt == F16:
        _check(name, got, ref, s32 * (U32 / U16), 1.0, 2.0, U16, SUB16)
    else:
        _check(name, got, ref, s32, 1.0, 2.0, U32, SUB32)


@pytest.mark.parametrize("case", GATE_CASES, ids=_cid)
def test_gate_random_against_float64(case):
    ops = _gpu()
    N, H, W, C, width, off, dt = case
    g = torch.Generator(device=DEV).manual_seed(7 * C + width + off + N)
    x = (torch.randn(N, H, W, C, generator=g, device=DEV) * 2).to(dt)
    dybuf, dyv = _slice_buf(N, H, W, C, width, off, dt)
    dyv.copy_(torch.randn(N, H, W, C, generator=g, device=DEV))
    p = torch.randn(N, H, W, 1, generator=g, device=DEV) * 3
    sat = torch.rand(N, H, W, 1, generator=g, device=DEV) < 0.02         # saturating z: |z| up to 1e4
    big = torch.exp(torch.rand(N, H, W, 1, generator=g, device=DEV) * 6.2 + 3.0) * torch.sign(p)
    p = torch.where(sat, big, p).to(dt)
    txx = torch.zeros(C, 4, device=DEV)
    txx[:, 1] = (torch.rand(C, generator=g, device=DEV) + 0.5) * torch.sign(torch.randn(C, generator=g, device=DEV))
    txx[:, 2] = torch.randn(C, generator=g, device=DEV)
    txp = torch.tensor([[0.0, 0.93, 0.37, float("-inf")]], device=DEV)
    y, dx, dp = _run_gate(ops, case, x, txx, p, txp, dyv, check_path=False)
    zmax = 0.0
    # measured worst b (fp16 cases / fp32 case, one run): y 0 / 0.90, dx 0 / 0.90, dp 1.18 / 1.39 (bound 2)
    for n in range(N):                                                         # one image at a time: bounded memory
        ry, rdx, rdp, z, A, S, absdot = _gate_ref(x[n], txx, p[n], txp, dyv[n])
        zmax = max(zmax, z.abs().max().item())
        cond = 4 + (1 - A) * z.abs()
        _bound_gate(f"y[{n}]", y[n], ry, ry.abs() * cond, dt)
        _bound_gate(f"dx[{n}]", dx[n], rdx, rdx.abs() * cond, dt)
        _bound_gate(f"dp[{n}]", dp[n], rdp, A * (1 - A) * (C * absdot + (6 + z.abs()) * S.abs()) + A * S.abs(), dt)
    assert zmax > 5e3                                                          # premise: the saturating pixels are there


# ========================================================================================================================
# c. add2_relu forward / backward, exact: integer a, b and transform rows without ReLU (the W_q / W_x BatchNorms), so that
#    many pre-activations are exactly 0; there relu's gradient is 0 (torch's relu backward) in both outputs
# ========================================================================================================================
@pytest.mark.parametrize("case", ADD_CASES, ids=_cid)
def test_add2_relu_exact_at_production_sizes(case):
    ops = _gpu()
    N, H, W, C, width, off, dt = case
    g = torch.Generator(device=DEV).manual_seed(3 * C + width + off + N)
    gc = torch.Generator().manual_seed(C + 1)
    a = torch.randint(-3, 4, (N, H, W, C), generator=g, device=DEV).to(dt)
    b = torch.randint(-3, 4, (N, H, W, C), generator=g, device=DEV).to(dt)
    txa, txb = _int_tx(C, gc), _int_tx(C, gc)
    txa[:, 3] = txb[:, 3] = float("-inf")
    txa, txb = _dev_tx(txa), _dev_tx(txb)
    ybuf, y = _slice_buf(N, H, W, C, width, off, dt)
    dybuf, dy = _slice_buf(N, H, W, C, width, off, dt)
    dy.copy_(torch.randint(1, 3, (N, H, W, C), generator=g, device=DEV) *
             (torch.randint(0, 2, (N, H, W, C), generator=g, device=DEV) * 2 - 1))       # nonzero: every mask bit shows
    da, db = _nan(N, H, W, C, dtype=dt), _nan(N, H, W, C, dtype=dt)
    vec = _vec(C, width, off, dt)
    kf = _kernels(lambda: ops.add2_relu(a, txa, b, txb, y))
    kb = _kernels(lambda: ops.add2_relu_bwd(dy, y, da, db))
    assert ("add2_relu_fwd_v8" in kf) == vec and ("add2_relu_bwd_v8" in kb) == vec, (kf, kb)
    torch.cuda.synchronize()
    assert _untouched(ybuf, off, C)
    zeros = 0
    for n in range(N):
        z = (_tx64(a[n].double(), txa) + _tx64(b[n].double(), txb)).requires_grad_(True)
        r = torch.relu(z)
        r.backward(dy[n].double())
        zeros += int((z == 0).sum())
        assert torch.equal(y[n].double(), r.detach()), n
        assert torch.equal(da[n].double(), z.grad) and torch.equal(db[n].double(), z.grad), n
    assert zeros > 0.02 * N * H * W * C                                      # premise: exact zeros of the pre-activation


# ========================================================================================================================
# d. the psi branch (C_hidden -> 1) and the hidden BatchNorms at production M
# ========================================================================================================================
def _stats_check(name, part, C, ref_y):
    """Statistics partial rows [rows][2][C] (fp32 sums of partial pixel ranges) against float64 sums of the stored values:
    |sum - ref| <= 8 U32 sum |terms| (measured 0 at every table entry, one run: on these integer data every partial row
    stays below 2^24 and is exact)."""
    tot = part.view(-1, 2, C).double().sum(0)
    y = ref_y.reshape(-1, C)
    ref = torch.stack([y.sum(0), (y * y).sum(0)])
    s = torch.stack([y.abs().sum(0), (y * y).sum(0)])
    _check(name, tot, ref, s, 0.0, 8.0, U32)
    return ref


def _finalize_check(ops, part, C, M, ref_sums, g):
    """bn_finalize against float64 from the exact statistics, bounds of test_bn_finalize_row_reduction_forms."""
    gamma, beta = torch.randn(C, generator=g, device=DEV), torch.randn(C, generator=g, device=DEV)
    rm0, rv0 = torch.randn(C, generator=g, device=DEV), torch.rand(C, generator=g, device=DEV) + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    tx, rs = ops.bn_finalize(part, C, M, gamma, beta, 1e-5, 0.1, rm, rv)
    mean = ref_sums[0] / M
    var = (ref_sums[1] / M - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    scale = gamma.double() * rstd
    tx, rs = tx.double(), rs.double()
    assert (tx[:, 0] - mean).abs().max().item() < 1e-6 * max(1.0, mean.abs().max().item())
    assert (tx[:, 1] - scale).abs().max().item() < 2e-6 * scale.abs().max().item()
    assert (tx[:, 2] - (beta.double() - mean * scale)).abs().max().item() < 1e-5
    assert (rs - rstd).abs().max().item() < 2e-6 * rstd.abs().max().item()
    assert (rm.double() - (0.9 * rm0.double() + 0.1 * mean)).abs().max().item() < 1e-6 * max(1.0, mean.abs().max().item())
    assert (rv.double() - (0.9 * rv0.double() + 0.1 * var * M / (M - 1))).abs().max().item() < 1e-5 * max(1.0, var.max().item())


def _bn_bwd_check(ops, y, C, g, kernel):
    """bn_bwd (reduce + apply) of a BatchNorm without ReLU (the gate branches) on a gradient of small integers and dyadic
    mean / scale / rstd rows: every term dz * xhat is a multiple of 1/16 far below 2^20, so both sums are exact in any order
    and the float64 sums, rounded once to fp32, must match bit for bit.  The apply pass against float64 from the kernel's
    own sums: one fp16 rounding (a = 1) plus fp32 steps on |scale| (|dz| + |c1| + |xhat c2|) (s in U32, scaled to U16; b
    measured 0 at every table entry, one run)."""
    shape = tuple(y.shape)
    M = shape[0] * shape[1] * shape[2]
    da0 = torch.randint(-3, 4, shape, generator=g, device=DEV).half()
    tx = torch.zeros(C, 4, device=DEV)
    tx[:, 0] = torch.randint(-4, 5, (C,), generator=g, device=DEV) * 0.5
    tx[:, 1] = torch.randint(1, 5, (C,), generator=g, device=DEV) * 0.25
    tx[:, 2] = torch.randint(-4, 5, (C,), generator=g, device=DEV) * 0.125
    tx[:, 3] = float("-inf")
    rstd = torch.randint(1, 5, (C,), generator=g, device=DEV) * 0.125
    da = da0.clone()
    names = _kernels(lambda: ops.bn_bwd(da, y, tx, rstd))
    assert kernel in names, names
    da.copy_(da0)
    s0, s1 = ops.bn_bwd(da, y, tx, rstd)
    torch.cuda.synchronize()
    y64, g64 = y.reshape(-1, C).double(), da0.reshape(-1, C).double()
    xh = (y64 - tx[:, 0].double()) * rstd.double()
    r0, r1 = g64.sum(0), (g64 * xh).sum(0)
    assert torch.equal(s0, r0.float()) and torch.equal(s1, r1.float()), ((s0 - r0).abs().max(), (s1 - r1).abs().max())
    c1, c2 = s0.double() / M, s1.double() / M
    ref = tx[:, 1].double() * (g64 - c1 - xh * c2)
    s = tx[:, 1].double().abs() * (g64.abs() + c1.abs() + (xh * c2).abs()) * 4
    _check("bn_bwd apply", da.reshape(-1, C), ref, s * (U32 / U16), 1.0, 2.0, U16, SUB16)


def _gid(gt):
    return f"{gt[0]}x{gt[1]}x{gt[2]}-Cx{gt[3]}-Ch{gt[4]}"


@pytest.mark.parametrize("gate", GATES, ids=_gid)
def test_psi_conv_stats_finalize_and_bn_bwd_c1(gate):
    """psi = Conv2d(C_hidden, 1, 1) on E (stored activated: non-negative integers here), the narrow-output kernel with its
    statistics epilogue (rows exact), bn_finalize with C = 1 and the one-channel BatchNorm backward (scalar kernels)."""
    ops = _gpu()
    N, H, W, _, Ch, _ = gate
    M = N * H * W
    g = torch.Generator(device=DEV).manual_seed(Ch)
    e = torch.randint(0, 3, (N, H, W, Ch), generator=g, device=DEV).half()
    w = _ints((1, Ch, 1, 1), -1, 1, torch.Generator().manual_seed(Ch)).to(DEV)
    p = _nan(N, H, W, 1)
    part = []
    names = _kernels(lambda: part.append(ops.conv_fwd(e, None, lambda lay: ops.pack_conv_fwd(w, F16, k8=bool(lay)), None, p,
                                                      1, 1, 1, 0, want_stats=True)))
    assert "head1x1_fwd_kernel" in names, names                               # the narrow-output kernel ran
    part = part[0]
    ref = torch.cat([(e[n].reshape(-1, Ch).double() @ w.view(Ch, 1).double()) for n in range(N)]).view(N, H, W, 1)
    assert ref.abs().max().item() < 2048
    assert torch.equal(p.double(), ref)
    sums = _stats_check("psi statistics", part, 1, ref)
    _finalize_check(ops, part, 1, M, sums, g)
    _bn_bwd_check(ops, p, 1, g, "bn_bwd_reduce1_kernel")


@pytest.mark.parametrize("N,H,W", [(2, 8, 8), (2, 16, 16), (2, 32, 32), (2, 64, 64)])
def test_bn_bwd_c1_at_small_sizes(N, H, W):
    """The one-channel BatchNorm backward at the psi sizes of UNet_attention(1, 2, 8) at B = 2, 64 x 64 (M = 128 ... 8,192:
    one to 32 stage-1 workgroups, the last one partial at M = 128)."""
    ops = _gpu()
    g = torch.Generator(device=DEV).manual_seed(N * H * W)
    y = torch.randint(-40, 41, (N, H, W, 1), generator=g, device=DEV).half()
    _bn_bwd_check(ops, y, 1, g, "bn_bwd_reduce1_kernel")


@pytest.mark.parametrize("branch", ["W_x", "W_q"])
@pytest.mark.parametrize("gate", GATES, ids=_gid)
def test_hidden_branch_two_pass_stats_finalize_and_bn_bwd(gate, branch):
    """W_x (input: the skip, raw with its BatchNorm + ReLU applied on load) and W_q (input: the upsampled query, stored with
    its bias, no transform): the pointwise matrix-core conv without statistics (rows exact on integer data), then bn_stats,
    bn_finalize and the BatchNorm backward at C_hidden."""
    ops = _gpu()
    from umi import lib as L
    N, H, W, Cx, Ch, Cq = gate
    Ci = Cx if branch == "W_x" else Cq
    M = N * H * W
    g = torch.Generator(device=DEV).manual_seed(Ci + Ch)
    gc = torch.Generator().manual_seed(Ci)
    x = torch.randint(-1, 2, (N, H, W, Ci), generator=g, device=DEV).half()
    tx = _int_tx(Ci, gc) if branch == "W_x" else None
    w = _ints((Ch, Ci, 1, 1), -1, 1, gc).to(DEV)
    out = _nan(N, H, W, Ch)
    assert ops.conv_plan(x, out, 1, 1, 1, 0, 0, False)[0] == 1                  # the pointwise MFMA kernel
    ops.conv_fwd(x, None if tx is None else tx.to(DEV), lambda lay: ops.pack_conv_fwd(w, F16, k8=bool(lay)), None, out,
                 1, 1, 1, 0, want_stats=False)
    part = ops.bn_stats(out)
    assert part is not None
    wt = w.view(Ch, Ci).t().double()
    ref = torch.empty(N, H, W, Ch, dtype=torch.float64, device=DEV)
    for n in range(N):
        a = _tx64(x[n].reshape(-1, Ci).double(), None if tx is None else tx.to(DEV))
        ref[n] = (a @ wt).view(H, W, Ch)
    assert ref.abs().max().item() < 2048
    assert torch.equal(out.double(), ref)
    sums = _stats_check(f"{branch} statistics", part, Ch, ref)
    _finalize_check(ops, part, Ch, M, sums, g)
    _bn_bwd_check(ops, out, Ch, g, "bn_bwd_reduce1_v8")


# ========================================================================================================================
# e. the tables above cover every configuration the model passes to these kernels inside its gates (batch aside)
# ========================================================================================================================
def _ld(t):
    from umi.ops import _nhwc
    return _nhwc(t)[4]


def test_model_calls_are_covered(monkeypatch):
    ops = _gpu()
    import Model
    import loss as L
    from umi import graph
    from oracle import recipe
    seen, in_gate = set(), [False]

    def wrap(name, key, gate_only=False):
        orig = getattr(ops, name)

        def f(*a, **k):
            if in_gate[0] or not gate_only:
                seen.add(key(*a, **k))
            return orig(*a, **k)
        monkeypatch.setattr(ops, name, f)

    def flagged(fn):
        def run(*a, **k):
            in_gate[0] = True
            try:
                return fn(*a, **k)
            finally:
                in_gate[0] = False
        return run

    orig_conv_bn = graph.Tape.conv_bn

    def conv_bn(self, *a, **k):
        if k.get("relu", True):                  # relu=False: only the gates' W_q / W_x / psi branches
            return orig_conv_bn(self, *a, **k)
        n = len(self.steps)
        o = flagged(orig_conv_bn)(self, *a, **k)
        if self.record:
            assert len(self.steps) == n + 1
            self.steps[-1] = flagged(self.steps[-1])
        return o
    monkeypatch.setattr(graph.Tape, "conv_bn", conv_bn)

    def hwc(t):
        return tuple(t.shape[1:])

    wrap("gate", lambda x, txx, p, txp, y: ("gate",) + hwc(x) + (_ld(x), _ld(y), x.dtype, txx is not None, txp is not None))
    wrap("gate_bwd", lambda dy, x, txx, p, txp, dx, dp: ("gate_bwd",) + hwc(x) + (_ld(dy), _ld(x), _ld(dx), x.dtype,
                                                                                 txx is not None, txp is not None))
    wrap("add2_relu", lambda a, txa, b, txb, y: ("add2_relu",) + hwc(a) + (_ld(a), _ld(b), _ld(y), a.dtype, txa is not None,
                                                                           txb is not None))
    wrap("add2_relu_bwd", lambda dy, y, da, db: ("add2_relu_bwd",) + hwc(y) + (_ld(dy), _ld(y), _ld(da), _ld(db), y.dtype))
    wrap("bn_stats", lambda y: ("bn_stats",) + hwc(y) + (_ld(y), y.dtype), gate_only=True)
    wrap("bn_bwd", lambda da, y, tx, rstd, partials=None, apply=True: ("bn_bwd",) + hwc(y) + (
        _ld(da), _ld(y), y.dtype, partials is None, apply, bool(torch.isinf(tx[:, 3]).all())), gate_only=True)
    wrap("bn_finalize", lambda part, C, *a: ("bn_finalize", C), gate_only=True)
    L.CLASS_NUMBER = 2
    torch.manual_seed(0)
    m = Model.UNet_attention(1, 2, 64, False, compute_dtype="fp16").to(DEV).train()
    x, lab = recipe.synthetic_batch(1, 1, 512, 512, 2, seed=1)
    L.calc_loss(m(x.to(DEV)), lab.to(DEV), loss_type="dice_bce_mc").backward()
    torch.cuda.synchronize()

    allowed = set()
    for N, H, W, C, width, off, dt in GATE_CASES:
        if dt == F16 and off == 0:
            allowed.add(("gate", H, W, C, C, width, dt, True, True))
            allowed.add(("gate_bwd", H, W, C, width, C, C, dt, True, True))
    for N, H, W, C, width, off, dt in ADD_CASES:
        if dt == F16 and off == 0 and width == C:
            allowed.add(("add2_relu", H, W, C, C, C, C, dt, True, True))
            allowed.add(("add2_relu_bwd", H, W, C, C, C, C, C, dt))
    for N, H, W, Cx, Ch, Cq in GATES:         # test_hidden_branch_two_pass_... and test_psi_conv_...
        allowed |= {("bn_stats", H, W, Ch, Ch, F16), ("bn_bwd", H, W, Ch, Ch, Ch, F16, True, True, True),
                    ("bn_bwd", H, W, 1, 1, 1, F16, True, True, True), ("bn_finalize", Ch), ("bn_finalize", 1)}
    assert {k[0] for k in seen} == {"gate", "gate_bwd", "add2_relu", "add2_relu_bwd", "bn_stats", "bn_bwd",
                                    "bn_finalize"}, sorted(seen)
    missing = sorted(k for k in seen if k not in allowed)
    assert not missing, f"configurations the model uses that the tables do not pin: {missing}"
