"""Attention-probability dropout (umi_attn_fwd_dropout / umi_attn_bwd_dropout), shared by tests/test_attn_dropout.py (CPU) and
tests/test_gpu_attn_dropout.py: the float64 restatement with the NumPy mask of tests/dropout_stream.py, the hand decomposition
the kernels implement, the four kernel families with their shapes and bars, and the read-out inputs.

  S = Q K^T / sqrt(D),  P = softmax(S),  M = the keep mask of the dense [B * heads * N, N] tensor of probabilities,
  Z = M / (1 - p) (0 where p = 1),  O = (P o Z) V,  lse = logsumexp(S) (undropped).

Read-out inputs turn one window of D keys (or queries) of the mask into an output whose ZERO PATTERN or SIGN is the mask, so a
kernel's mask is compared bit for bit, in fp16 as well (a value comparison could not: one flipped bit moves dq by about 1 % of
its maximum, below the fp16 backward bar).  q is scaled by 0.25 so that P stays near 1 / N, inside fp16's normal range.
A reference is computed once per case and never modified."""
import math

import numpy as np
import torch

from tests import dropout_stream as stream

SEED = 0xC0FFEE11            # >= 2^31: the seed is an unsigned word
COUNTER = 5
NEG_COUNTER = -3             # the device scalar is int32; the kernels read it as unsigned
OUTS = ("o", "lse", "dq", "dk", "dv")

# max-abs error over max |reference|: the project's attention bars (tests/attn_f32_cases.BARS; fp16:
# tests/test_gpu_kernels_tu.py::test_attention_fwd_bwd, 3e-3 forward and 5 x 3e-3 backward).  They carry over to p > 0: dropout
# zeroes terms and multiplies the kept ones by a constant, signal and rounding error of a row both grow as sqrt(N / (1 - p)).
BARS_F32 = {"o": 2e-5, "lse": 2e-5, "dq": 1e-4, "dk": 1e-4, "dv": 1e-4}
BARS_F16 = {"o": 3e-3, "lse": 3e-3, "dq": 1.5e-2, "dk": 1.5e-2, "dv": 1.5e-2}

SHAPES_D64 = [(2, 17, 1), (2, 33, 2), (1, 63, 1), (1, 65, 2), (2, 196, 3), (1, 257, 2), (1, 1024, 2)]
# name -> head dimension, dtype, flags of the calls (1 = UMI_ATTN_F32_MFMA), the kernel umi_attn_plan must name, bars, value shapes,
# read-out shapes
FAMILIES = {
    "valu_f32_d16": dict(D=16, dtype=torch.float32, flags=0, kernel=0, bars=BARS_F32, shapes=[(2, 50, 4)],
                         readout=[(2, 17, 1), (2, 50, 4)]),
    "valu_f16_d32": dict(D=32, dtype=torch.float16, flags=0, kernel=0, bars=BARS_F16, shapes=[(2, 40, 2)],
                         readout=[(2, 17, 1), (2, 40, 2)]),
    # (1, 129, 1) and (1, 225, 2): one past the 128-key and 224-key staging chunks of csrc/attention_mfma.hip
    "mfma_f16": dict(D=64, dtype=torch.float16, flags=0, kernel=1, bars=BARS_F16, shapes=SHAPES_D64 + [(1, 129, 1), (1, 225, 2)],
                     readout=[(2, 17, 1), (1, 65, 2), (2, 196, 3), (1, 1024, 2)]),
    "mfma_f32": dict(D=64, dtype=torch.float32, flags=1, kernel=2, bars=BARS_F32, shapes=SHAPES_D64,
                     readout=[(2, 17, 1), (1, 65, 2), (2, 196, 3), (1, 1024, 2)]),
}
READOUT_P = 0.5

_cache = {}


def keep(shape, p, seed, counter=None):
    """The keep mask as a bool tensor [B, heads, N, N]: the project's stream on the dense [B * heads * N, N] tensor."""
    B, N, heads = shape
    return torch.from_numpy(stream.keep_mask(B * heads * N, N, p, seed, counter).astype(bool)).view(B, heads, N, N)


def heads_of(t, shape, D):
    B, N, heads = shape
    return t.reshape(B, N, heads, D).permute(0, 2, 1, 3)


def tokens_of(t, shape, D):
    B, N, heads = shape
    return t.permute(0, 2, 1, 3).reshape(B, 1, N, heads * D)


def zmask(m, p, dtype=torch.float64):
    """Z = M / (1 - p); p = 1 keeps nothing and the infinite scale is selected away."""
    return m.to(dtype) * (1.0 / (1.0 - p) if p < 1 else 0.0)


def forward(q, k, v, m, p, shape, D):
    """(o [B,1,N,C], lse [B*heads*N], P, Z) of token tensors [B,1,N,C] in their own dtype."""
    s = heads_of(q, shape, D) @ heads_of(k, shape, D).transpose(-1, -2) / math.sqrt(D)
    P, Z = torch.softmax(s, -1), zmask(m, p, q.dtype)
    return tokens_of((P * Z) @ heads_of(v, shape, D), shape, D), torch.logsumexp(s, -1).reshape(-1), P, Z


def evaluate(x, m, p, shape, D):
    """o, lse, dq, dk, dv of the restatement and its autograd in float64 on the CPU."""
    qr, kr, vr = (x[n].double().clone().requires_grad_(True) for n in ("q", "k", "v"))
    o, lse, _, _ = forward(qr, kr, vr, m, p, shape, D)
    o.backward(x["dO"].double())
    return {"o": o.detach(), "lse": lse.detach(), "dq": qr.grad, "dk": kr.grad, "dv": vr.grad}


def decomposition(x, m, p, shape, D):
    """The kernels' formulas in float64, no autograd: delta = rowsum(dO o O), dS = P o (Z o dP - delta), dV = (P o Z)^T dO."""
    q, k, v, dO = (x[n].double() for n in ("q", "k", "v", "dO"))
    o, lse, P, Z = forward(q, k, v, m, p, shape, D)
    qh, kh, vh, doh, oh = (heads_of(t, shape, D) for t in (q, k, v, dO, o))
    scale = 1.0 / math.sqrt(D)
    delta = (doh * oh).sum(-1, keepdim=True)
    dS = P * (Z * (doh @ vh.transpose(-1, -2)) - delta)
    return {"o": o, "lse": lse, "dq": tokens_of(scale * dS @ kh, shape, D), "dk": tokens_of(scale * dS.transpose(-1, -2) @ qh, shape, D),
            "dv": tokens_of((P * Z).transpose(-1, -2) @ doh, shape, D)}


def inputs(shape, D, dtype=torch.float32):
    """{q, k, v, dO} [B,1,N,C] standard normal, rounded to `dtype` (the reference is evaluated on the rounded values)."""
    key = ("in", shape, D, dtype)
    if key not in _cache:
        B, N, heads = shape
        g = torch.Generator().manual_seed(1000 * B + 10 * N + heads + 7 * D)
        _cache[key] = {n: torch.randn(B, 1, N, heads * D, generator=g).to(dtype) for n in ("q", "k", "v", "dO")}
    return _cache[key]


def case(shape, D, dtype, p, seed=SEED, counter=COUNTER):
    """(inputs, float64 reference {o, lse, dq, dk, dv}) under the mask of (p, seed, counter)."""
    key = ("case", shape, D, dtype, p, seed, counter)
    if key not in _cache:
        x = inputs(shape, D, dtype)
        _cache[key] = (x, evaluate(x, keep(shape, p, seed, counter), p, shape, D))
    return _cache[key]


def error(got, ref):
    return (got.detach().double().cpu().reshape(ref.shape) - ref).abs().max().item(), ref.abs().max().item()


def assert_inside_bars(got, ref, bars, what, names=OUTS):
    for n in names:
        err, top = error(got[n], ref[n])
        print(f"{what} {n}: max-abs error {err:.3e} = {err / top if top else 0.0:.3e} of max |ref| {top:.3e} (bar {bars[n]:.0e})")
        assert err <= bars[n] * top, (what, n, err, top)


# ---- read-out inputs -----------------------------------------------------------------------------------------------------------------
def windows(N, D):
    """Starts of the windows of D keys / queries: every one for N <= 257, the first, a middle and the last one above."""
    every = list(range(0, N, D))
    return every if N <= 257 else [every[0], every[len(every) // 2], every[-1]]


def _one_hot_rows(shape, D, r0):
    """[B,1,N,C] with row r of every head = e_{r - r0} for r0 <= r < r0 + D, zero rows elsewhere."""
    B, N, heads = shape
    t = torch.zeros(B, 1, N, heads, D)
    for c in range(min(D, N - r0)):
        t[:, :, r0 + c, :, c] = 1.0
    return t.view(B, 1, N, heads * D)


def _e0_rows(shape, D):
    B, N, heads = shape
    t = torch.zeros(B, 1, N, heads, D)
    t[..., 0] = 1.0
    return t.view(B, 1, N, heads * D)


def readout(kind, shape, D, r0, dtype=torch.float32):
    """Inputs whose output shows the mask window starting at r0 (kind "o": keys, "dv": queries, "dq": keys)."""
    x = {n: t.clone() for n, t in inputs(shape, D, torch.float32).items()}
    x["q"] = x["q"] * 0.25
    if kind == "o":              # V[j] = e_{j - j0}: O[i, c] = (P o Z)[i, j0 + c]
        x["v"] = _one_hot_rows(shape, D, r0)
    elif kind == "dv":           # dO[i] = e_{i - i0}: dV[j, c] = (P o Z)[i0 + c, j]
        x["dO"] = _one_hot_rows(shape, D, r0)
    elif kind == "dq":           # V, dO rows = e_0, K[j] = e_{j - j0}: dQ[i, c] = scale P_ij (Z_ij - s_i), s_i = sum_j P_ij Z_ij in (0, 2)
        x["v"], x["dO"], x["k"] = _e0_rows(shape, D), _e0_rows(shape, D), _one_hot_rows(shape, D, r0)
    else:
        raise ValueError(kind)
    return {n: t.to(dtype) for n, t in x.items()}


def window_of_mask(kind, m, shape, D, r0):
    """The slice of the mask [B, heads, N, N] the read-out shows, laid out like the output's window: bool [B, N, heads, w]."""
    w = min(D, shape[1] - r0)
    if kind == "dv":             # dV[j, c] <-> M[i0 + c, j]
        return m[:, :, r0:r0 + w, :].permute(0, 3, 1, 2)
    return m[:, :, :, r0:r0 + w].permute(0, 2, 1, 3)


def window_of_output(t, shape, D, r0):
    """The first min(D, N - r0) channels of every head of a [B,1,N,C] output: [B, N, heads, w]."""
    B, N, heads = shape
    return t.reshape(B, N, heads, D)[..., :min(D, N - r0)]


def shown(kind, out, shape, D, r0):
    """The bool pattern a read-out output shows: nonzero for "o" / "dv", positive for "dq"."""
    w = window_of_output(out[kind], shape, D, r0)
    return w > 0 if kind == "dq" else w != 0
