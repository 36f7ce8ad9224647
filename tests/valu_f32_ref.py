"""Float64 statement of the operations the fp32 VALU kernels of csrc/generic_kernels.hip compute, in their calling convention.

Everything here runs on the CPU in torch float64 and is written from the kernels' contract (include/unetmi.h, umi/ops.py), not
from torch's operators: tests/test_valu_f32_ref.py pins it against F.conv2d / F.conv_transpose2d / F.max_pool2d / autograd, and
tests/test_gpu_valu_f32.py then holds the kernels to it.

Conventions
  * activations are NHWC tensors `[N, H, W, C]` of any float dtype, possibly channel slices of wider buffers (plain views);
  * `tx` is the per-channel consumer transform `[C, 4]` = (mean, scale, shift, floor), applied as max(v * scale + shift, floor)
    to every IN-BOUNDS value (the zero padding of a convolution is padded after the transform); `None` = consumed as stored;
  * weights arrive PACKED, as ops.pack_conv_* lay them out (the `pack_*` functions below state those layouts);
  * every contraction returns `(value, mag)`: `mag` is the sum of the absolute values of the terms that were added up, with
    |tx(v)| bounded by |v| * |scale| + |shift| -- the magnitude sum the rounding bound gamma_n * mag needs (Higham, Accuracy and
    Stability of Numerical Algorithms, 3.1 / 3.4).

fp32 and fp16 inputs are exact in float64, and so is the product of two of them; a sum of products carries float64 roundings
only (2^-53 relative), which is what makes this a reference for fp32 arithmetic."""
import torch

F64 = torch.float64
U = 2.0 ** -24


def gamma(n):
    """gamma_n = n u / (1 - n u), u = 2^-24: the relative error bound of n fp32 roundings in any order."""
    return n * U / (1.0 - n * U)


# ---- consumer transform ----------------------------------------------------------------------------------------------------
def tx_pre(x, tx):
    """z = v * scale + shift (what umi_tx_pre rounds once to fp32), float64."""
    t = tx.to(F64)
    return x.to(F64) * t[:, 1] + t[:, 2]


def apply_tx(x, tx):
    """(max(v * scale + shift, floor), |v| * |scale| + |shift|); tx None: (v, |v|)."""
    x = x.to(F64)
    if tx is None:
        return x, x.abs()
    t = tx.to(F64)
    return torch.maximum(tx_pre(x, tx), t[:, 3]), x.abs() * t[:, 1].abs() + t[:, 2].abs()


# ---- weight layouts (ops.pack_conv_*): [taps][K][N], N fastest ---------------------------------------------------------------
def pack_conv_fwd(w):
    """OIHW -> [R*S][Ci][Co]."""
    Co, Ci, R, S = w.shape
    return w.permute(2, 3, 1, 0).reshape(R * S, Ci, Co).contiguous()


def pack_conv_dgrad(w):
    """OIHW -> [R*S][Co][Ci] with the taps rotated by 180 degrees: the stride-1 data gradient is then a forward convolution."""
    Co, Ci, R, S = w.shape
    return w.flip(2, 3).permute(2, 3, 0, 1).reshape(R * S, Co, Ci).contiguous()


def pack_conv_dgrad_strided(w):
    """OIHW -> [R*S][Co][Ci], taps as they are (UMI_CONV_DGRAD_STRIDED)."""
    Co, Ci, R, S = w.shape
    return w.permute(2, 3, 0, 1).reshape(R * S, Co, Ci).contiguous()


def pack_convT_fwd(w):
    """ConvTranspose2d [Cin][Cout][2][2] -> [4][Cin][Cout]."""
    Cin, Cout = w.shape[:2]
    return w.permute(2, 3, 0, 1).reshape(4, Cin, Cout).contiguous()


def pack_convT_dgrad(w):
    """ConvTranspose2d [Cin][Cout][2][2] -> [4][Cout][Cin]."""
    Cin, Cout = w.shape[:2]
    return w.permute(2, 3, 1, 0).reshape(4, Cout, Cin).contiguous()


# ---- convolutions ----------------------------------------------------------------------------------------------------------
def _padded(a, pad, Hp, Wp):
    N, H, W, C = a.shape
    out = torch.zeros(N, Hp, Wp, C, dtype=F64)
    out[:, pad:pad + H, pad:pad + W] = a
    return out


def conv_fwd(x, tx, wp, bias, R, S, stride, pad, Co):
    """y[n, ho, wo, co] = sum_{r, s, ci} tx(x)[n, ho * stride - pad + r, wo * stride - pad + s, ci] * wp[r * S + s][ci][co]
    (+ bias[co]); out-of-range pixels contribute zero.  Returns (y, mag), both [N, Ho, Wo, Co]."""
    N, H, W, Ci = x.shape
    Ho, Wo = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    a, am = apply_tx(x, tx)
    Hp, Wp = max(H + 2 * pad, stride * (Ho - 1) + R), max(W + 2 * pad, stride * (Wo - 1) + S)
    a, am = _padded(a, pad, Hp, Wp), _padded(am, pad, Hp, Wp)
    w = wp.to(F64).reshape(R * S, Ci, Co)
    y = torch.zeros(N, Ho, Wo, Co, dtype=F64)
    mag = torch.zeros_like(y)
    for r in range(R):
        for s in range(S):
            rows, cols = slice(r, r + stride * (Ho - 1) + 1, stride), slice(s, s + stride * (Wo - 1) + 1, stride)
            y += a[:, rows, cols] @ w[r * S + s]
            mag += am[:, rows, cols] @ w[r * S + s].abs()
    if bias is not None:
        y += bias.to(F64)
        mag += bias.to(F64).abs()
    return y, mag


def conv_stats(y):
    """The statistics epilogue's column totals of a stored output: (sum y, sum y^2) per channel; both are their own magnitude
    sums when taken of |y| (returned third: sum |y|)."""
    y = y.to(F64).reshape(-1, y.shape[-1])
    return y.sum(0), (y * y).sum(0), y.abs().sum(0)


def convT_fwd(x, tx, wp, bias, up_offset, out_hw, Co):
    """ConvTranspose2d(2, 2) scattered into an [N, out_H, out_W, Co] destination:
    y[n, 2h + dy + off_h, 2w + dx + off_w, co] = sum_ci tx(x)[n, h, w, ci] * wp[dy * 2 + dx][ci][co] + bias[co]; positions that
    fall outside the destination are dropped.  Returns (y, mag, written): `written` marks the pixels the scatter reaches (the rest
    of y and mag is zero: the kernel leaves those bytes alone)."""
    N, H, W, Ci = x.shape
    oH, oW = out_hw
    a, am = apply_tx(x, tx)
    w = wp.to(F64).reshape(4, Ci, Co)
    y = torch.zeros(N, oH, oW, Co, dtype=F64)
    mag = torch.zeros_like(y)
    written = torch.zeros(N, oH, oW, dtype=torch.bool)
    b = bias.to(F64) if bias is not None else torch.zeros(Co, dtype=F64)
    for dy in range(2):
        for dx in range(2):
            v, m = a @ w[dy * 2 + dx] + b, am @ w[dy * 2 + dx].abs() + b.abs()
            for h in range(H):
                ho = 2 * h + dy + up_offset[0]
                if ho < 0 or ho >= oH:
                    continue
                for wi in range(W):
                    wo = 2 * wi + dx + up_offset[1]
                    if wo < 0 or wo >= oW:
                        continue
                    y[:, ho, wo], mag[:, ho, wo], written[:, ho, wo] = v[:, h, wi], m[:, h, wi], True
    return y, mag, written


def conv_dgrad_strided(dy, wpd, R, S, stride, pad, in_hw, Ci):
    """Data gradient of a strided convolution (UMI_CONV_DGRAD_STRIDED), wpd = [R*S][Co][Ci] unflipped:
    dx[n, h, w, ci] = sum over taps (r, s) with (h + pad - r, w + pad - s) = stride * (ho, wo) in range, and co, of
    dy[n, ho, wo, co] * wpd[r * S + s][co][ci].  Returns (dx, mag), both [N, in_H, in_W, Ci]."""
    N, Ho, Wo, Co = dy.shape
    H, W = in_hw
    g = dy.to(F64)
    w = wpd.to(F64).reshape(R * S, Co, Ci)
    dx = torch.zeros(N, H, W, Ci, dtype=F64)
    mag = torch.zeros_like(dx)
    for r in range(R):
        for s in range(S):
            v, m = g @ w[r * S + s], g.abs() @ w[r * S + s].abs()
            for ho in range(Ho):
                h = ho * stride - pad + r
                if h < 0 or h >= H:
                    continue
                for wo in range(Wo):
                    wi = wo * stride - pad + s
                    if wi < 0 or wi >= W:
                        continue
                    dx[:, h, wi] += v[:, ho, wo]
                    mag[:, h, wi] += m[:, ho, wo]
    return dx, mag


def conv_wgrad(x, txa, dy, txb, R, S, stride, pad, numel, s_co, s_ci, s_t, out_scale, fill=0.0):
    """Weight gradient written through the destination strides:
    dW[co * s_co + ci * s_ci + t * s_t] = out_scale * sum_{n, ho, wo} txa(x)[n, ho * stride - pad + r, wo * stride - pad + s, ci]
                                                                     * txb(dy)[n, ho, wo, co],   t = r * S + s.
    Returns (dW, mag) as flat float64 vectors of `numel` elements; elements no (co, ci, t) maps to hold `fill` / zero."""
    N, H, W, Ci = x.shape
    _, Ho, Wo, Co = dy.shape
    a, am = apply_tx(x, txa)
    g, gm = apply_tx(dy, txb)
    Hp, Wp = max(H + 2 * pad, stride * (Ho - 1) + R), max(W + 2 * pad, stride * (Wo - 1) + S)
    a, am = _padded(a, pad, Hp, Wp), _padded(am, pad, Hp, Wp)
    g, gm = g.reshape(-1, Co), gm.reshape(-1, Co)
    dW = torch.full((numel,), fill, dtype=F64)
    mag = torch.zeros(numel, dtype=F64)
    idx = (torch.arange(Ci)[:, None] * s_ci + torch.arange(Co)[None, :] * s_co)
    for r in range(R):
        for s in range(S):
            rows, cols = slice(r, r + stride * (Ho - 1) + 1, stride), slice(s, s + stride * (Wo - 1) + 1, stride)
            t = r * S + s
            dW[idx + t * s_t] = out_scale * (a[:, rows, cols].reshape(-1, Ci).t() @ g)
            mag[idx + t * s_t] = abs(out_scale) * (am[:, rows, cols].reshape(-1, Ci).t() @ gm)
    return dW, mag


# ---- MaxPool2d(2) ------------------------------------------------------------------------------------------------------------
def _pool_select(x, tx):
    """(max, index of the FIRST maximum in window order (0,0), (0,1), (1,0), (1,1)) of the transformed tensor's 2x2 windows."""
    N, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    a, _ = apply_tx(x, tx)
    m, best = None, None
    for d in range(4):
        v = a[:, (d >> 1):2 * Ho:2, (d & 1):2 * Wo:2]
        if d == 0:
            m, best = v.clone(), torch.zeros(N, Ho, Wo, C, dtype=torch.long)
        else:
            up = v > m
            m, best = torch.where(up, v, m), torch.where(up, torch.full_like(best, d), best)
    return m, best


def pool2_fwd(x, tx):
    """y[n, ho, wo, c] = max of tx(x) over the window rows 2ho, 2ho + 1 and columns 2wo, 2wo + 1; an odd last row / column is dropped."""
    return _pool_select(x, tx)[0]


def pool2_bwd(dpool, x, tx, da, accumulate):
    """The gradient of each pooled value goes to the first maximum of its window, every other position of the H x W input
    (the odd tail included) gets zero; accumulate: added to `da`, else `da` is overwritten."""
    N, H, W, C = x.shape
    Ho, Wo = H // 2, W // 2
    _, best = _pool_select(x, tx)
    g = dpool.to(F64)
    out = torch.zeros(N, H, W, C, dtype=F64)
    for d in range(4):
        out[:, (d >> 1):2 * Ho:2, (d & 1):2 * Wo:2] = torch.where(best == d, g, torch.zeros_like(g))
    return out + da.to(F64) if accumulate else out


# ---- BatchNorm + ReLU backward -------------------------------------------------------------------------------------------------
def bn_bwd_terms(da, y, tx, rstd):
    """(dz, xhat) per element: z = y * scale + shift, dz = da where z > floor else 0, xhat = (y - mean) * rstd."""
    t = tx.to(F64)
    z = tx_pre(y, tx)
    dz = torch.where(z > t[:, 3], da.to(F64), torch.zeros((), dtype=F64))
    return dz, (y.to(F64) - t[:, 0]) * rstd.to(F64)


def bn_bwd_reduce(da, y, tx, rstd):
    """(sum dz, sum dz * xhat, sum |dz|, sum |dz * xhat|) per channel over all pixels."""
    dz, xh = bn_bwd_terms(da, y, tx, rstd)
    C = dz.shape[-1]
    dz, p = dz.reshape(-1, C), (dz * xh).reshape(-1, C)
    return dz.sum(0), p.sum(0), dz.abs().sum(0), p.abs().sum(0)


def bn_bwd_apply(da, y, tx, rstd, sum_dz, sum_dzx, count):
    """d(raw conv output) = scale * (dz - sum_dz / count - xhat * sum_dzx / count), and the sum of its terms' magnitudes
    |scale| * (|dz| + |sum_dz / count| + |xhat * sum_dzx / count|)."""
    dz, xh = bn_bwd_terms(da, y, tx, rstd)
    sc = tx.to(F64)[:, 1]
    c1, c2 = sum_dz.to(F64) / count, sum_dzx.to(F64) / count
    return sc * (dz - c1 - xh * c2), sc.abs() * (dz.abs() + c1.abs() + (xh * c2).abs())


# ---- column sums, layout change ----------------------------------------------------------------------------------------------
def colsum(x, out_scale):
    """(out_scale * sum over pixels, |out_scale| * sum of magnitudes) per channel."""
    v = x.to(F64).reshape(-1, x.shape[-1])
    return out_scale * v.sum(0), abs(out_scale) * v.abs().sum(0)


def materialize_nchw(x, tx):
    """NHWC storage + consumer transform -> NCHW."""
    return apply_tx(x, tx)[0].permute(0, 3, 1, 2).contiguous()
