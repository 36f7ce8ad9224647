"""Shapes, inputs, float64 reference and bars shared by tests/test_attn_f32_mfma_plan.py (CPU) and tests/test_gpu_attn_f32_mfma.py:
softmax(Q K^T / 8) V at head dimension 64 and its autograd, from fp32 standard-normal inputs.  A reference is computed once per
shape and never modified."""
import math

import torch

D = 64
KEY_CHUNK = 64          # keys per staged chunk of csrc/attention_mfma_f32.hip: its neighbours 63 and 65 are in SHAPES
# (B, N, heads)
SHAPES = [(1, 1, 1), (2, 17, 1), (1, 32, 3), (2, 33, 2), (2, 50, 4), (1, 63, 1), (1, 65, 2), (2, 196, 3), (1, 257, 2), (1, 1024, 2)]
# the project's fp32 attention bars (tests/test_gpu_kernels_tu.py::test_attention_fwd_bwd): max-abs error / max |reference|
TOL_FWD, TOL_BWD = 2e-5, 1e-4
BARS = {"o": TOL_FWD, "lse": TOL_FWD, "dq": TOL_BWD, "dk": TOL_BWD, "dv": TOL_BWD}

_cache = {}


def heads_of(t, B, N, heads):
    return t.view(B, N, heads, D).permute(0, 2, 1, 3)


def attention(q, k, v, B, N, heads):
    """(o [B,1,N,C], lse [B*heads*N]) of token tensors [B,1,N,C] in their own dtype."""
    s = heads_of(q, B, N, heads) @ heads_of(k, B, N, heads).transpose(-1, -2) / math.sqrt(D)
    o = (torch.softmax(s, -1) @ heads_of(v, B, N, heads)).permute(0, 2, 1, 3).reshape(B, 1, N, heads * D)
    return o, torch.logsumexp(s, -1).reshape(-1)


def evaluate(q, k, v, dO, B, N, heads, dtype):
    """o, lse, dq, dk, dv of the formula and its autograd evaluated by torch in `dtype` on the CPU."""
    qr, kr, vr = (t.to(dtype).clone().requires_grad_(True) for t in (q, k, v))
    o, lse = attention(qr, kr, vr, B, N, heads)
    o.backward(dO.to(dtype))
    return {"o": o.detach(), "lse": lse.detach(), "dq": qr.grad, "dk": kr.grad, "dv": vr.grad}


def case(shape):
    """({q, k, v, dO} fp32 [B,1,N,C], float64 reference {o, lse, dq, dk, dv})."""
    if shape not in _cache:
        B, N, heads = shape
        g = torch.Generator().manual_seed(1000 * B + 10 * N + heads)
        x = {n: torch.randn(B, 1, N, heads * D, generator=g) for n in ("q", "k", "v", "dO")}
        _cache[shape] = (x, evaluate(x["q"], x["k"], x["v"], x["dO"], B, N, heads, torch.float64))
    return _cache[shape]


def error(got, ref):
    """(max-abs error, max |reference|) against the float64 reference."""
    return (got.detach().double().cpu().reshape(ref.shape) - ref).abs().max().item(), ref.abs().max().item()


def assert_inside_bars(got, ref, what, names=tuple(BARS)):
    for n in names:
        err, top = error(got[n], ref[n])
        print(f"{what} {n}: max-abs error {err:.3e} = {err / top if top else 0.0:.3e} of max |ref| {top:.3e} (bar {BARS[n]:.0e})")
        assert err <= BARS[n] * top, (what, n, err, top)
