"""The TransUNet fp16 kernels at the R50-ViT-B/16 production shapes and calling conventions, element by element against
float64 references (BASELINE configs[3]: B = 24 at 224 x 224, 196 tokens; configs[4]: B = 12 at 512 x 512, 1,024 tokens).

Every reference is plain torch in float64 on the exact fp16 (or fp32) inputs, cast up.  Every comparison is elementwise:
|y - ref| <= (a |ref| + b s) u + f, with u the unit roundoff of the kernel's arithmetic (U16 = 2^-11 or U32 = 2^-24), s an
elementwise scale that the kernel's rounding model names (e.g. P|V| for a product P V whose P is rounded to fp16 before its
MFMA, or 1/rstd-sized terms of a normalisation), and f half the fp16 subnormal spacing where the output is fp16.  a = 1 is
the output's own rounding; b is the budget for the rounding inside the kernel, and each one states its measured worst case.
Output buffers, and the unused columns of strided ones, are prefilled with NaN.

`test_model_calls_are_covered` keeps the case tables honest: it records every configuration the model itself passes to
these kernels and requires each to appear in the tables, batch aside."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U16, U32 = 2.0 ** -11, 2.0 ** -24
SUB16 = 2.0 ** -25                   # half the fp16 subnormal spacing: the absolute floor of rounding to fp16
HEADS, D, C_VIT = 12, 64, 768


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from umi import lib, ops, ops_tu
    return lib, ops, ops_tu


def _nan(*shape, dtype=torch.float16):
    return torch.full(shape, float("nan"), dtype=dtype, device=DEV)


def _check(name, y, ref, s, a, b, u, floor=0.0):
    """|y - ref| <= (a |ref| + b s) u + floor, elementwise.  Prints the measured b: max over elements of
    (|y - ref| - a |ref| u - floor) / (s u), so that a bound's comment can record its worst case."""
    y = y.double()
    assert torch.isfinite(y).all(), f"{name}: non-finite (unwritten?) elements"
    err = (y - ref).abs()
    lim = (a * ref.abs() + b * s) * u + floor
    bad = err > lim
    used = ((err - a * ref.abs() * u - floor).clamp_min(0) / (s * u).clamp_min(1e-300)).max().item()
    print(f"[bound] {name}: b measured {used:.3g}, bound {b}")
    if bad.any():
        i = bad.nonzero()[0].tolist()
        pytest.fail(f"{name}: {int(bad.sum())} elements out of bound; first at {i}: got {y[tuple(i)].item()!r}, "
                    f"ref {ref[tuple(i)].item()!r}, s {s[tuple(i)].item() if s.dim() else s.item()!r}; measured b {used:.3g}")


def _kernels(fn):
    """Names of the device kernels `fn` launches (the premise checks: which path ran)."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return " ".join(e.name for e in prof.events())


# ========================================================================================================================
# 1. MFMA attention: q/k/v are channel slices of one [B,1,N,3C] buffer (ld = 2304), o has ldo = 768, and dq/dk/dv are
#    channel slices of one [B,1,N,3C] gradient buffer (ldd = 2304), exactly as TUTape.qkv_attention calls it.
# ========================================================================================================================
A_CODE = 12.0                        # key codes are +-A: logits (q.k)/8 = 18 (64 - 2 hamming), the lead per bit is 36
# (B, N) at 12 heads: production, then N straddling the forward's 224-key chunk, the dQ kernel's 128-key chunk, the
# 128-query / 128-key blocks and the 32-row tiles
ATTN_SHAPES = [(24, 196), (12, 1024), (2, 223), (2, 224), (2, 225), (3, 257), (1, 1025)]
ATTN_ODD = (5, 257, 3)               # (B, N, heads): B * heads = 15 is not a multiple of 4 (12 heads always are)


def _attn_buffers(B, N, dtype=torch.float16, C=C_VIT):
    qkv = _nan(B, 1, N, 3 * C, dtype=dtype)
    o = _nan(B, 1, N, C, dtype=dtype)
    dqkv = _nan(B, 1, N, 3 * C, dtype=dtype)
    return qkv, o, dqkv


def _codes(g, B, N, heads):
    """[B, heads, N, 64] distinct +-1 codes (independent random bits per head: every channel is used, differently per head)."""
    return torch.randint(0, 2, (B, heads, N, D), generator=g, device=DEV, dtype=torch.int8).double() * 2 - 1


def _onehot_case(g, B, N, heads):
    """Keys: distinct +-A codes.  Query i gets the code of key sel[i] (one-hot softmax, lead >= 36 over every other key) or,
    for the two-hot queries 16..23, a code at hamming distance 1 from each of two keys that differ in exactly two bits
    (P = 1/2 each).  Returns q, k (float64 [B,h,N,64]) and the exact P ([B,h,N,N])."""
    kc = _codes(g, B, N, heads)
    decoys = []
    if N > 224:
        # decoy d of chunk 0 = the code of a later-chunk key j with one bit flipped; queries 3..10 select j, so the running
        # maximum of chunk 0 (the decoy, 36 below) must be rescaled by corr = exp(-36) when j arrives
        for t in range(8):
            j, d_ = 224 + (t * 37) % (N - 224), 5 + 11 * t
            kc[:, :, d_] = kc[:, :, j]
            kc[:, :, d_, (7 * t) % D] *= -1
            decoys.append((3 + t, j))
    pairs = []
    for t in range(8):                                   # keys 100..107 / 120..141 (all N here are > 141)
        j1, j2, ba, bb = 100 + t, 120 + 3 * t, (5 * t) % D, (5 * t + 3) % D
        kc[:, :, j2] = kc[:, :, j1]
        kc[:, :, j2, ba] *= -1
        kc[:, :, j2, bb] *= -1
        pairs.append((16 + t, j1, j2, ba))
    sel = torch.randint(0, N, (B, heads, N), generator=g, device=DEV)     # birthday collisions: some keys picked by many
    last0 = (N - 1) // 224 * 224                                         # queries, others by none
    sel[..., 0], sel[..., 1], sel[..., 2] = N - 1, 0, last0 + (N - 1 - last0) // 2
    for qi, j in decoys:
        sel[..., qi] = j
    qc = kc.gather(2, sel[..., None].expand(-1, -1, -1, D)).clone()
    P = torch.zeros(B, heads, N, N, dtype=torch.float64, device=DEV)
    P.scatter_(-1, sel[..., None], 1.0)
    for qi, j1, j2, ba in pairs:
        qc[:, :, qi] = kc[:, :, j1]
        qc[:, :, qi, ba] *= -1
        P[:, :, qi] = 0
        P[:, :, qi, j1] = P[:, :, qi, j2] = 0.5
    # premise: distinct keys; one-hot rows lead by >= 36, two-hot rows tie their pair and lead the rest by >= 36
    for b in range(B):
        kk = kc[b] @ kc[b].transpose(-1, -2)
        assert (kk - 64 * torch.eye(N, device=DEV, dtype=torch.float64)).max() < 64, "distinct codes"
        s = (qc[b] @ kc[b].transpose(-1, -2)) * (A_CODE * A_CODE / 8)
        top = s.topk(3, dim=-1).values
        one = (P[b] == 1).any(-1)
        assert (top[..., 0] - top[..., 1])[one].min() >= 36 and (s.argmax(-1) == P[b].argmax(-1))[one].all()
        assert (top[..., 0] == top[..., 1])[~one].all() and (top[..., 1] - top[..., 2])[~one].min() >= 36
        assert int((~one).sum()) == heads * len(pairs)
    return qc * A_CODE, kc * A_CODE, P


def _to_tokens(t):
    """[B, h, N, 64] float64 -> [B, 1, N, h*64] fp16-valued."""
    B, h, N, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, 1, N, h * D)


def _heads(t):
    B, _, N, C = t.shape
    return t.double().reshape(B, N, C // D, D).permute(0, 2, 1, 3)


def _attn_run(T, q, k, v, dO, heads, dtype=torch.float16):
    """Runs attn_fwd / attn_bwd in the tape's layout on fp16-exact values ([B,1,N,C] float64 or fp16) -> device outputs."""
    B, _, N, C = q.shape
    qkv, o, dqkv = _attn_buffers(B, N, dtype, C)
    for i, t in enumerate((q, k, v)):
        qkv[..., i * C:(i + 1) * C] = t.to(dtype)
    qs, ks, vs = (qkv[..., i * C:(i + 1) * C] for i in range(3))
    lse = T.attn_fwd(qs, ks, vs, o, heads)
    dOd = dO.to(dtype).contiguous()
    dq, dk, dv = (dqkv[..., i * C:(i + 1) * C] for i in range(3))
    T.attn_bwd(qs, ks, vs, o, dOd, lse, dq, dk, dv, heads)
    torch.cuda.synchronize()
    return qkv, o, lse.view(B, heads, N), dq, dk, dv


def _attn_ref_check(tag, qkv, o, lse, dq, dk, dv, dO, heads, u, b_o, b_lse, b_dv, b_dqk, bsz=1):
    """float64 forward from q/k/v; float64 backward from the backward's own inputs (q/k/v, o, dO and the saved lse):
    P = exp(S/8 - lse), delta = rowsum(dO o), dS = P (dP - delta), dQ = dS K / 8, dK = dS^T Q / 8, dV = P^T dO.
    Scales, with c = u32 / u and A = |Q||K|^T / 8 (the fp32 logits carry an absolute error ~u32 A, so P a relative one):
    (P (1 + c A)) |V| for O (P rounded to fp16 before its MFMA), its transpose against |dO| for dV, and
    (|dS| (1 + c A) + 64 c P (|dO||V|^T + |dO||o|)) |K| / 8 for dQ and dK (dS rounded before its MFMA; dP - delta formed
    in fp32 from 64-term products)."""
    B, _, N, C3 = qkv.shape
    C = C3 // 3
    floor = SUB16 if o.dtype == torch.float16 else 0.0
    c = U32 / u
    for b0 in range(0, B, bsz):
        sl = slice(b0, b0 + bsz)
        Q, K, V = (_heads(qkv[sl, ..., i * C:(i + 1) * C]) for i in range(3))
        G, Ok = _heads(dO[sl]), _heads(o[sl])
        S = Q @ K.transpose(-1, -2) * 0.125
        A = 1 + c * (Q.abs() @ K.abs().transpose(-1, -2) * 0.125)
        lse_ref = torch.logsumexp(S, -1)
        P = torch.exp(S - lse_ref[..., None])
        _check(f"{tag} O b{b0}", Ok, P @ V, (P * A) @ V.abs(), 1, b_o, u, floor)
        _check(f"{tag} lse b{b0}", lse[sl].double(), lse_ref, lse_ref.abs() + 1, 0, b_lse, U32)
        del P
        Pk = torch.exp(S - lse[sl].double()[..., None])
        del S
        dP = G @ V.transpose(-1, -2)
        delta = (G * Ok).sum(-1, keepdim=True)
        dS = Pk * (dP - delta)
        mag = dS.abs() * A + 64 * c * Pk * (G.abs() @ V.abs().transpose(-1, -2) + (G.abs() * Ok.abs()).sum(-1, keepdim=True))
        del dP
        _check(f"{tag} dV b{b0}", _heads(dv[sl]), Pk.transpose(-1, -2) @ G, (Pk * A).transpose(-1, -2) @ G.abs(), 1, b_dv, u,
               floor)
        _check(f"{tag} dQ b{b0}", _heads(dq[sl]), dS @ K * 0.125, mag @ K.abs() * 0.125, 1, b_dqk, u, floor)
        _check(f"{tag} dK b{b0}", _heads(dk[sl]), dS.transpose(-1, -2) @ Q * 0.125, mag.transpose(-1, -2) @ Q.abs() * 0.125,
               1, b_dqk, u, floor)
        del Pk, dS, mag


@pytest.mark.parametrize("B,N,heads", [(B, N, HEADS) for B, N in ATTN_SHAPES] + [ATTN_ODD])
def test_attention_one_and_two_hot_exact(B, N, heads):
    """Constructed softmax whose answer is exact: O = P V, dV = P^T dO, dQ = dK = 0 bit for bit on one-hot queries (exp(0)
    = 1, exp(-36) vanishes in fp16 and against 1 in fp32), LSE = the known maximum; the two-hot ties (P = 1/2) give non-zero
    dQ / dK that are checked against float64 with the elementwise bound."""
    lib, ops, T = _gpu()
    g = torch.Generator(device=DEV).manual_seed(1000 + N)
    C = heads * D
    q, k, P = _onehot_case(g, B, N, heads)
    v = torch.randint(-4, 5, (B, heads, N, D), generator=g, device=DEV).double()
    dO = torch.randint(-2, 3, (B, heads, N, D), generator=g, device=DEV).double()
    run = lambda: _attn_run(T, _to_tokens(q), _to_tokens(k), _to_tokens(v), _to_tokens(dO), heads)
    names = _kernels(run)
    assert "attn_q_side_kernel" in names and "attn_kv_side_kernel" in names, "premise: the MFMA path runs"
    qkv, o, lse, dq, dk, dv = run()
    O_exp = P @ v                                            # one-hot rows: V[sel]; two-hot rows: (V1 + V2) / 2, exact
    assert torch.equal(_heads(o), O_exp)
    onehot = (P == 1).any(-1)                                # [B, h, N]
    top = (q @ k.transpose(-1, -2) * 0.125).amax(-1)
    lse_exp = top + (~onehot).double() * math.log(2.0)
    # LSE = max + log(1) exactly on one-hot rows; the fp32 rounding of max + __logf(2) on the two-hot rows
    assert torch.equal(lse.double()[onehot], lse_exp[onehot])
    assert ((lse.double() - lse_exp).abs() <= 2 * U32 * lse_exp.abs()).all()
    G = dO
    dV_exp = P.transpose(-1, -2) @ G                         # scatter-sum of dO (small integers: exact)
    assert torch.equal(_heads(dv), dV_exp)
    assert torch.equal(_heads(dq)[onehot], torch.zeros_like(_heads(dq)[onehot]))
    twohot_keys = (P == 0.5).any(-2)                          # [B, h, N]: keys of a tied pair
    assert torch.equal(_heads(dk)[~twohot_keys], torch.zeros_like(_heads(dk)[~twohot_keys]))
    assert _heads(dq)[~onehot].abs().max() > 0 and _heads(dk)[twohot_keys].abs().max() > 0
    # the rest against float64, elementwise: O, dQ, dK measured b 0 (exact), dV 0.03 (P = exp(S - lse) of the tied rows
    # carries the fp32 rounding of lse = 1116 + log 2), bound 1 for each; lse measured 0.48 u32, bound 2
    _attn_ref_check(f"hot {B}x{N}", qkv, o, lse, dq, dk, dv, _to_tokens(dO), heads, U16, 1, 2, 1, 1, bsz=4)


@pytest.mark.parametrize("B,N,heads", [(B, N, HEADS) for B, N in ATTN_SHAPES] + [ATTN_ODD])
def test_attention_equal_logits_counts_exactly_n_keys(B, N, heads):
    """q = 0: every logit is 0, so O is the mean of exactly N rows of V and lse = log N.  A padded key that is counted
    (the one-hot case cannot see it: a padded key scores 0 there and its weight underflows) changes both."""
    lib, ops, T = _gpu()
    g = torch.Generator(device=DEV).manual_seed(2000 + N)
    C = heads * D
    k = torch.randn(B, 1, N, C, generator=g, device=DEV).half()
    v = torch.randint(-8, 9, (B, 1, N, C), generator=g, device=DEV).half()
    dO = torch.randn(B, 1, N, C, generator=g, device=DEV).half()
    qkv, o, lse, dq, dk, dv = _attn_run(T, torch.zeros_like(k), k, v, dO, heads)
    mean = _heads(v).mean(-2, keepdim=True).expand(-1, -1, N, -1)
    # O = fp16(acc * fp32(1 / N)), acc an exact integer sum: measured b 0 (a = 1), bound 0.01 (the fp32 reciprocal)
    _check(f"mean {B}x{N}", _heads(o), mean, _heads(v).abs().mean(-2, keepdim=True).expand(-1, -1, N, -1), 1, 0.01, U16,
           SUB16)
    # lse = 0 + __logf(N): measured 1.6 u32 of log N, bound 4
    _check(f"lse {B}x{N}", lse.double(), torch.full_like(lse, math.log(N), dtype=torch.float64),
           torch.full_like(lse, math.log(N), dtype=torch.float64), 0, 4, U32)
    # backward of the uniform softmax: dV measured b 0.13, dQ 0.2, dK 0, bound 1; lse measured 1.4 u32, bound 4
    _attn_ref_check(f"eq {B}x{N}", qkv, o, lse, dq, dk, dv, dO, heads, U16, 1, 4, 1, 1, bsz=4)


@pytest.mark.parametrize("B,N,heads", [(B, N, HEADS) for B, N in ATTN_SHAPES] + [ATTN_ODD])
def test_attention_random_against_float64(B, N, heads):
    """General case, logits with std ~3.5 (a peaked, not near-uniform, softmax; rescales across the forward's chunks)."""
    lib, ops, T = _gpu()
    g = torch.Generator(device=DEV).manual_seed(3000 + N)
    C = heads * D
    q, k = ((torch.randn(B, 1, N, C, generator=g, device=DEV) * 1.9).half() for _ in range(2))
    v, dO = (torch.randn(B, 1, N, C, generator=g, device=DEV).half() for _ in range(2))
    qkv, o, lse, dq, dk, dv = _attn_run(T, q, k, v, dO, heads)
    lg = (_heads(q)[:1] @ _heads(k)[:1].transpose(-1, -2) * 0.125).std().item()
    assert 2.5 < lg < 5, lg
    # O: P rounded to fp16 (u16 relative) and the output rounding: measured b 0.64, bound 1.  dV: fp16(P): measured b 0.8,
    # bound 1.  dQ / dK: fp16(dS) and the fp32 dP - delta: measured b 0.76, bound 1.  lse: measured 3 u32 of |lse| + 1,
    # bound 8 (__expf / __logf and the fp32 running sums)
    _attn_ref_check(f"rand {B}x{N}", qkv, o, lse, dq, dk, dv, dO, heads, U16, 1, 8, 1, 1, bsz=2)


def test_attention_fp32_scalar_kernels_strided():
    """fp32 compute mode (attn_*_kernel<float, 64>) once at (2, 1025) in the same strided layout."""
    lib, ops, T = _gpu()
    g = torch.Generator(device=DEV).manual_seed(4)
    B, N = 2, 1025
    q, k = ((torch.randn(B, 1, N, C_VIT, generator=g, device=DEV) * 1.9) for _ in range(2))
    v, dO = (torch.randn(B, 1, N, C_VIT, generator=g, device=DEV) for _ in range(2))
    run = lambda: _attn_run(T, q, k, v, dO, HEADS, torch.float32)
    names = _kernels(run)
    assert "attn_q_side_kernel" not in names, "premise: fp32 takes the scalar kernels"
    qkv, o, lse, dq, dk, dv = run()
    # fp32 throughout (u32 units): O / dV measured b 6.3 / 4.3, bound 16 (1,025-term fp32 sums); dQ / dK 0.29, bound 2;
    # lse 9.3, bound 32
    _attn_ref_check("fp32", qkv, o, lse, dq, dk, dv, dO, HEADS, U32, 16, 32, 16, 2, bsz=1)


# ========================================================================================================================
# 2. LayerNorm fp16 (C = 768): ln_fwd_kernel<half> and ln_bwd_v4_kernel, the production path of the ViT's 25 LayerNorms
# ========================================================================================================================
LN_ROWS = [24 * 196, 12 * 1024, 16 * 77 + 5]      # the last: not a multiple of LNV_ROWS = 16


def _ln_inputs(g, M, C=C_VIT):
    drift = torch.randn(M, 1, generator=g, device=DEV) * 24          # row means large against their spread
    spread = torch.rand(M, 1, generator=g, device=DEV) * 1.5 + 0.25
    x = (drift + spread * torch.randn(M, C, generator=g, device=DEV)).half()
    gamma = 1 + 0.5 * torch.randn(C, generator=g, device=DEV)
    beta = 0.2 * torch.randn(C, generator=g, device=DEV)
    dy = torch.randn(M, C, generator=g, device=DEV).half()
    return x, gamma, beta, dy


@pytest.mark.parametrize("M", LN_ROWS)
def test_layer_norm_fp16_fwd_bwd_and_deferred_param_grads(M):
    lib, ops, T = _gpu()
    g = torch.Generator(device=DEV).manual_seed(M)
    C = C_VIT
    x, gamma, beta, dy = _ln_inputs(g, M)
    as4 = lambda t: t.view(1, 1, M, -1)
    y = _nan(M, C)
    mean, rstd = T.ln_fwd(as4(x), gamma, beta, 1e-6, as4(y))
    x64 = x.double()
    m_ref = x64.mean(1, keepdim=True)
    var = x64.var(1, unbiased=False, keepdim=True)
    r_ref = 1 / torch.sqrt(var + 1e-6)
    xh = (x64 - m_ref) * r_ref
    # mean: fp32 sums of 768 values ~24: measured b 1.4, bound 4 (u32 of |mean| + 1/rstd)
    _check(f"ln mean {M}", mean.double()[:, None], m_ref, m_ref.abs() + 1 / r_ref, 0, 4, U32)
    # rstd: two-pass variance around the fp32 mean, rsqrtf: measured b 2.7, bound 8 (u32 relative)
    _check(f"ln rstd {M}", rstd.double()[:, None], r_ref, r_ref, 0, 8, U32)
    # y: fp16 output rounding (a = 1) + the fp32 mean's error times rstd: measured b 1e-4, bound 0.01 of
    # |gamma| (1 + |xhat| + |mean| rstd) u16
    s = gamma.double().abs() * (1 + xh.abs() + m_ref.abs() * r_ref)
    _check(f"ln y {M}", y, xh * gamma.double() + beta.double(), s, 1, 0.01, U16, SUB16)
    # backward against float64 on its own inputs (dy, x, gamma, mean, rstd as stored)
    mk, rk = mean.double()[:, None], rstd.double()[:, None]
    xk = (x64 - mk) * rk
    gd = dy.double() * gamma.double()
    dx_ref = rk * (gd - gd.mean(1, keepdim=True) - xk * (gd * xk).mean(1, keepdim=True))
    rms = gd.pow(2).mean(1, keepdim=True).sqrt()
    dx = _nan(M, C)
    names = _kernels(lambda: T.ln_bwd(as4(dy), as4(x), gamma, mean, rstd, as4(dx), 0.25))
    assert "ln_bwd_v4_kernel" in names, "premise: the fp16 vector path"
    dx.fill_(float("nan"))
    dg, db = T.ln_bwd(as4(dy), as4(x), gamma, mean, rstd, as4(dx), 0.25)
    # dx: fp16 output rounding + fp32 row sums (768 terms): measured b 1e-5, bound 0.01 of rstd rms(dy gamma) (1 + |xhat|)
    _check(f"ln dx {M}", dx, dx_ref, rk * rms * (1 + xk.abs()), 1, 0.01, U16, SUB16)
    dg_ref = 0.25 * (dy.double() * xk).sum(0)
    db_ref = 0.25 * dy.double().sum(0)
    # dgamma / dbeta: fp32 sums of 16 rows per workgroup, summed in double: measured b 0.16 / 0.07, bound 2 (u32 of
    # 0.25 sum|terms|)
    _check(f"ln dgamma {M}", dg, dg_ref, 0.25 * (dy.double() * xk).abs().sum(0), 0, 2, U32)
    _check(f"ln dbeta {M}", db, db_ref, 0.25 * dy.double().abs().sum(0), 0, 2, U32)
    # keep_part: one partial row per LNV_ROWS = 16 rows, reduced later by gn_param_grads_group
    dx2 = _nan(M, C)
    part, rows = T.ln_bwd(as4(dy), as4(x), gamma, mean, rstd, as4(dx2), 0.25, keep_part=True)
    assert rows == (M + 15) // 16
    assert torch.equal(dx2, dx)
    dg2, db2 = torch.full_like(dg, float("nan")), torch.full_like(db, float("nan"))
    T.gn_param_grads_group([part[:rows * 2 * C]], rows, [dg2], [db2], 0.25)
    _check(f"ln dgamma deferred {M}", dg2, dg_ref, 0.25 * (dy.double() * xk).abs().sum(0), 0, 2, U32)
    _check(f"ln dbeta deferred {M}", db2, db_ref, 0.25 * dy.double().abs().sum(0), 0, 2, U32)


def test_layer_norm_fp16_generic_path_same_reference():
    """A view with ld % 4 != 0 takes the scalar backward: the same data, the same float64 reference and bound."""
    lib, ops, T = _gpu()
    g = torch.Generator(device=DEV).manual_seed(9)
    M, C = 16 * 77 + 5, C_VIT
    x, gamma, beta, dy = _ln_inputs(g, M)
    wide = _nan(M, C + 2)
    wide[:, :C] = dy
    dyv = wide[:, :C].unsqueeze(0).unsqueeze(0)
    as4 = lambda t: t.view(1, 1, M, -1)
    y = _nan(M, C)
    mean, rstd = T.ln_fwd(as4(x), gamma, beta, 1e-6, as4(y))
    dx = _nan(M, C)
    names = _kernels(lambda: T.ln_bwd(dyv, as4(x), gamma, mean, rstd, as4(dx), 1.0))
    assert "ln_bwd_v4_kernel" not in names, "premise: ld % 4 != 0 takes the generic kernel"
    dx.fill_(float("nan"))
    dg, db = T.ln_bwd(dyv, as4(x), gamma, mean, rstd, as4(dx), 1.0)
    mk, rk = mean.double()[:, None], rstd.double()[:, None]
    xk = (x.double() - mk) * rk
    gd = dy.double() * gamma.double()
    dx_ref = rk * (gd - gd.mean(1, keepdim=True) - xk * (gd * xk).mean(1, keepdim=True))
    rms = gd.pow(2).mean(1, keepdim=True).sqrt()
    # the scalar kernel's partial rows cover 64 rows each: dgamma measured b 0.23, bound 2
    _check("ln dx generic", dx, dx_ref, rk * rms * (1 + xk.abs()), 1, 0.01, U16, SUB16)
    _check("ln dgamma generic", dg, (dy.double() * xk).sum(0), (dy.double() * xk).abs().sum(0), 0, 2, U32)
    assert torch.isnan(wide[:, C:]).all()


# ========================================================================================================================
# 3. GroupNorm fp16 vector path (groupnorm_f16.hip) at every distinct GroupNorm of the R50 hybrid, production batch
#    (H, W, C, G, relu, residual, eps) per image size; B = 24 at 224, 12 at 512.
# ========================================================================================================================
GN_224 = [(112, 112, 64, 32, True, False, 1e-6),                      # root
          (55, 55, 256, 256, False, False, 1e-5), (55, 55, 64, 32, True, False, 1e-6), (55, 55, 256, 32, True, True, 1e-6),
          (55, 55, 128, 32, True, False, 1e-6), (28, 28, 128, 32, True, False, 1e-6), (28, 28, 512, 32, True, True, 1e-6),
          (28, 28, 512, 512, False, False, 1e-5), (28, 28, 256, 32, True, False, 1e-6), (14, 14, 256, 32, True, False, 1e-6),
          (14, 14, 1024, 32, True, True, 1e-6), (14, 14, 1024, 1024, False, False, 1e-5)]
GN_512 = [(256, 256, 64, 32, True, False, 1e-6),
          (127, 127, 256, 256, False, False, 1e-5), (127, 127, 64, 32, True, False, 1e-6),
          (127, 127, 256, 32, True, True, 1e-6), (127, 127, 128, 32, True, False, 1e-6), (64, 64, 128, 32, True, False, 1e-6),
          (64, 64, 512, 32, True, True, 1e-6), (64, 64, 512, 512, False, False, 1e-5), (64, 64, 256, 32, True, False, 1e-6),
          (32, 32, 256, 32, True, False, 1e-6), (32, 32, 1024, 32, True, True, 1e-6), (32, 32, 1024, 1024, False, False, 1e-5)]
GN_CASES = [(24,) + c for c in GN_224] + [(12,) + c for c in GN_512]
# the row-block plan gn_rows() / umi_gn_splits() must produce at each (N, H*W): S row blocks (ragged last one where
# H*W % rows != 0; the 512 root hits the 1,024-row cap)
GN_SPLITS = {(24, 112 * 112): 22, (12, 256 * 256): 64}


def _gn_splits(lib, N, HW, C):
    return lib.fn("umi_gn_fwd_ws_bytes")(N, HW, C) // (N * 2 * C * 4)


def _gn_ref_stats(x64, G, eps):
    N, H, W, C = x64.shape
    xg = x64.reshape(N, H * W, G, C // G)
    m = xg.mean((1, 3))
    var = xg.var((1, 3), unbiased=False)
    return m, 1 / torch.sqrt(var + eps)                 # [N, G]


def _per_channel(t, C, G):
    """[N, G] -> [N, 1, 1, C]"""
    return t.repeat_interleave(C // G, 1)[:, None, None, :]


def _gn_case(T, N, H, W, C, G, relu, resid, eps, xv=None, tag=""):
    g = torch.Generator(device=DEV).manual_seed(N * 7 + H * 13 + C + G)
    mu = torch.randn(N, 1, 1, C, generator=g, device=DEV) * 12       # channel means large against their spread
    sd = torch.rand(N, 1, 1, C, generator=g, device=DEV) + 0.5
    x = mu + sd * torch.randn(N, H, W, C, generator=g, device=DEV)
    x[:, 0, 0, :] = mu[:, 0, 0, :] + 6 * sd[:, 0, 0, :]               # the first pixel (gn_rowsum_v8's shift): an outlier
    x = x.half()
    res = torch.randn(N, H, W, C, generator=g, device=DEV).half() if resid else None
    gamma = 1 + 0.5 * torch.randn(C, generator=g, device=DEV)
    beta = 0.3 * torch.randn(C, generator=g, device=DEV)
    dy = torch.randn(N, H, W, C, generator=g, device=DEV).half()
    if xv is not None:
        x = xv(x)
    y = _nan(N, H, W, C)
    mean, rstd = T.gn_fwd(x, gamma, beta, G, eps, relu, res, y)
    x64 = x.double()
    m_ref, r_ref = _gn_ref_stats(x64, G, eps)
    # the shift's distance from the mean in units of the spread: the fp32 sums of (x - shift)^2 lose that factor squared
    sh = ((x64[:, 0, 0, :] - _per_channel(m_ref, C, G)[:, 0, 0]).abs() * _per_channel(r_ref, C, G)[:, 0, 0])
    shg = sh.reshape(N, G, C // G).amax(-1)
    # mean: measured b 5.4, bound 16 (u32 of |mean| + (1 + shift distance) / rstd)
    _check(f"gn mean {tag}", mean.double().view(N, G), m_ref, m_ref.abs() + (1 + shg) / r_ref, 0, 16, U32)
    # rstd: double finish of fp32 partial sums of (x - shift)^2, which lose the shift's distance squared: measured b 11,
    # bound 16 (u32 relative, times 1 + shift distance^2)
    _check(f"gn rstd {tag}", rstd.double().view(N, G), r_ref, r_ref * (1 + shg ** 2), 0, 16, U32)
    mC, rC = _per_channel(m_ref, C, G), _per_channel(r_ref, C, G)
    xh = (x64 - mC) * rC
    pre = xh * gamma.double() + beta.double() + (res.double() if resid else 0)
    ref = pre.clamp_min(0) if relu else pre
    # y: output rounding + fp32 mean / rstd: measured b 5e-4, bound 0.01 of |gamma| (1 + |xhat|) (1 + shift distance^2)
    s = gamma.double().abs() * (1 + xh.abs()) * (1 + _per_channel(shg, C, G) ** 2)
    _check(f"gn y {tag}", y, ref, s, 1, 0.01, U16, SUB16)
    # backward on its own inputs (dy, y, x, mean / rstd as stored)
    mk, rk = _per_channel(mean.double().view(N, G), C, G), _per_channel(rstd.double().view(N, G), C, G)
    xk = (x64 - mk) * rk
    dz = torch.where(y.double() > 0, dy.double(), 0.0) if relu else dy.double()
    gz = dz * gamma.double()
    grp = lambda t: _per_channel(t.reshape(N, H * W, G, C // G).mean((1, 3)), C, G)
    dx_ref = rk * (gz - grp(gz) - xk * grp(gz * xk))
    dx, dres = _nan(N, H, W, C), (_nan(N, H, W, C) if resid else None)
    dg, db = T.gn_bwd(dy, y, x, mean, rstd, gamma, G, relu, dx, dres, 0.5)
    # dx: output rounding + fp32 per-channel sums finished in fp32: measured b 2e-5, bound 0.01 of
    # rstd (|dz gamma| + mean_g|dz gamma| (1 + |xhat|))
    _check(f"gn dx {tag}", dx, dx_ref, rk * (gz.abs() + grp(gz.abs()) * (1 + xk.abs())), 1, 0.01, U16, SUB16)
    if resid:
        assert torch.equal(dres.double(), dz), "dres = dz exactly"
    dg_ref, db_ref = 0.5 * (dz * xk).sum((0, 1, 2)), 0.5 * dz.sum((0, 1, 2))
    sg, sb = 0.5 * (dz * xk).abs().sum((0, 1, 2)), 0.5 * dz.abs().sum((0, 1, 2))
    # dgamma / dbeta: fp32 sums of row blocks, finished in fp32 over S and in double over N: measured b 0.52 / 0.11,
    # bound 4 (u32 of 0.5 sum|terms|)
    _check(f"gn dgamma {tag}", dg, dg_ref, sg, 0, 4, U32)
    _check(f"gn dbeta {tag}", db, db_ref, sb, 0, 4, U32)
    dx2 = _nan(N, H, W, C)
    part = T.gn_bwd(dy, y, x, mean, rstd, gamma, G, relu, dx2, None, 0.5, keep_part=True)
    assert torch.equal(dx2, dx)
    dg2, db2 = torch.full_like(dg, float("nan")), torch.full_like(db, float("nan"))
    T.gn_param_grads_group([part], N, [dg2], [db2], 0.5)
    _check(f"gn dgamma deferred {tag}", dg2, dg_ref, sg, 0, 4, U32)
    _check(f"gn dbeta deferred {tag}", db2, db_ref, sb, 0, 4, U32)


@pytest.mark.parametrize("N,H,W,C,G,relu,resid,eps", GN_CASES)
def test_group_norm_fp16_r50_shapes(N, H, W, C, G, relu, resid, eps):
    lib, ops, T = _gpu()
    HW = H * W
    rows = max(16, min(1024, ((N * HW + 511) // 512 + 7) // 8 * 8))
    S = _gn_splits(lib, N, HW, C)
    assert S == (HW + rows - 1) // rows and S == GN_SPLITS.get((N, HW), S)
    assert S > 1, "premise: several row blocks per sample"
    x0 = torch.zeros(N, H, W, C, device=DEV, dtype=torch.float16)
    y0 = torch.empty_like(x0)
    g1 = torch.ones(C, device=DEV)
    names = _kernels(lambda: T.gn_fwd(x0, g1, g1, G, eps, relu, None, y0))
    assert "gn_rowsum_v8" in names and "gn_apply_fin_kernel" in names, "premise: the fp16 vector path"
    _gn_case(T, N, H, W, C, G, relu, resid, eps, tag=f"{N}x{H}x{W}x{C}/{G}")


def test_group_norm_fp16_generic_path_same_reference():
    """The same data through a view with ld % 8 != 0 takes the generic kernels: same reference, same bounds."""
    lib, ops, T = _gpu()
    N, H, W, C, G = 24, 28, 28, 512, 512

    def strided(x):
        wide = _nan(N, H, W, C + 4)
        wide[..., :C] = x
        return wide[..., :C]
    xs = strided(torch.zeros(N, H, W, C, device=DEV, dtype=torch.float16))
    y0 = _nan(N, H, W, C)
    g1 = torch.ones(C, device=DEV)
    names = _kernels(lambda: T.gn_fwd(xs, g1, g1, G, 1e-5, False, None, y0))
    assert "gn_rowsum_v8" not in names, "premise: the generic kernels"
    _gn_case(T, N, H, W, C, G, False, False, 1e-5, xv=strided, tag="generic")


# ========================================================================================================================
# 4. Weight standardisation, GELU, bilinear x2
# ========================================================================================================================
WSTD_SHAPES = [(64, 147), (64, 576), (128, 1152), (256, 2304), (256, 64), (64, 256), (128, 256), (512, 256), (128, 512),
               (1024, 512), (256, 1024), (1024, 256), (512, 1024)]          # (Co, K): 7x7 root, 3x3 convs, 1x1 convs


@pytest.mark.parametrize("Co,K", WSTD_SHAPES)
def test_wstd_fwd_bwd(Co, K):
    lib, ops, T = _gpu()
    g = torch.Generator(device=DEV).manual_seed(Co + K)
    w = (0.05 * torch.randn(Co, K, generator=g, device=DEV) + 0.02 * torch.randn(Co, 1, generator=g, device=DEV))
    ws, rstd = T.wstd_fwd(w, 1e-5)
    w64 = w.double()
    m = w64.mean(1, keepdim=True)
    r = 1 / torch.sqrt(w64.var(1, unbiased=False, keepdim=True) + 1e-5)
    # one-pass fp32 variance (q / K - mean^2): relative error ~ u32 (1 + mean^2 rstd^2): measured b 2.5, bound 8
    _check(f"wstd rstd {Co}x{K}", rstd.double()[:, None], r, r * (1 + (m * r) ** 2), 0, 8, U32)
    # ws = (w - mean) rstd: the fp32 mean's error scales with mean|w|: measured b 1.9, bound 8
    _check(f"wstd ws {Co}x{K}", ws, (w64 - m) * r, ((w64 - m).abs() + w64.abs().mean(1, keepdim=True)) * r * (1 + (m * r) ** 2),
           1, 8, U32)
    gr = torch.randn(Co, K, generator=g, device=DEV)
    dw = T.wstd_bwd(ws, rstd, gr)
    wk, rk, g64 = ws.double(), rstd.double()[:, None], gr.double()
    ref = rk * (g64 - g64.mean(1, keepdim=True) - wk * (g64 * wk).mean(1, keepdim=True))
    # fp32 block sums of K terms: measured b 1.2, bound 4 (u32 of rstd (|g| + mean|g| (1 + |what|)))
    _check(f"wstd dw {Co}x{K}", dw, ref, rk * (g64.abs() + g64.abs().mean(1, keepdim=True) * (1 + wk.abs())), 1, 4, U32)


def test_gelu_fp16_fwd_bwd_ew8():
    """umi_elementwise modes 0 / 1 on the ew8 path at the MLP's 4704 x 3072, |u| up to 10."""
    lib, ops, T = _gpu()
    g = torch.Generator(device=DEV).manual_seed(5)
    M, C = 24 * 196, 3072
    u = torch.randn(M, C, generator=g, device=DEV) * 2.5
    u[::7] = torch.rand(len(u[::7]), C, generator=g, device=DEV) * 20 - 10
    u = u.half().view(1, 1, M, C)
    gg = torch.randn(1, 1, M, C, generator=g, device=DEV).half()
    y = _nan(1, 1, M, C)
    names = _kernels(lambda: T.gelu_fwd(u, y))
    assert "ew8_kernel" in names, "premise: the fp16 vector path"
    y.fill_(float("nan"))
    T.gelu_fwd(u, y)
    u64 = u.double()
    phi = 0.5 * (1 + torch.erf(u64 / math.sqrt(2)))
    # 0.5 u (1 + erff(u / sqrt 2)) in fp32: 1 + erf cancels for u << 0, an absolute error of ~u32 |u|: measured b 0.24,
    # bound 8 (u32 of |u|)
    _check("gelu fwd", y, u64 * phi, u64.abs(), U16 / U32, 1, U32, SUB16)
    dx = _nan(1, 1, M, C)
    T.gelu_bwd(u, gg, dx)
    dref = gg.double() * (phi + u64 * torch.exp(-0.5 * u64 * u64) / math.sqrt(2 * math.pi))
    # g (Phi(u) + u phi(u)): the same cancellation plus __expf of an argument up to 50: measured b 0.04, bound 1 (u32 of
    # |g| (1 + |u|))
    _check("gelu bwd", dx, dref, gg.double().abs() * (1 + u64.abs()), U16 / U32, 1, U32, SUB16)


# (N, H, W, C, Cskip): the decoder's four x2 upsamplings into the channel slice [..., :C] of the concat buffer
BIL_CASES = [(24, 14, 14, 512, 512), (24, 28, 28, 256, 256), (24, 56, 56, 128, 64), (24, 112, 112, 64, 0),
             (12, 32, 32, 512, 512), (12, 64, 64, 256, 256), (12, 128, 128, 128, 64), (12, 256, 256, 64, 0)]


def _bilinear_ref(x64):
    """UpsamplingBilinear2d(x2, align_corners=True) in float64, NHWC."""
    import torch.nn.functional as F
    return F.interpolate(x64.permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)


@pytest.mark.parametrize("N,H,W,C,Cs", BIL_CASES)
def test_bilinear2x_fp16_fwd_adjoint_decoder_shapes(N, H, W, C, Cs):
    lib, ops, T = _gpu()
    g = torch.Generator(device=DEV).manual_seed(H + C)
    x = (torch.randn(N, H, W, C, generator=g, device=DEV) * 3 + 1).half()
    # consumer transform rows (BatchNorm + ReLU folded): max(v * scale + shift, floor)
    tx = torch.stack([torch.zeros(C, device=DEV), 0.5 + torch.rand(C, generator=g, device=DEV),
                      torch.randn(C, generator=g, device=DEV), torch.zeros(C, device=DEV)], 1).contiguous()
    cat = _nan(N, 2 * H, 2 * W, C + Cs)
    dest = cat[..., :C]
    names = _kernels(lambda: T.bilinear2x(x, dest, False, tx))
    assert "bilinear2x_fwd8_kernel" in names, "premise: the fp16 vector path"
    cat.fill_(float("nan"))
    T.bilinear2x(x, dest, False, tx)
    t64 = tx.double()
    xa = torch.maximum(x.double() * t64[:, 1] + t64[:, 2], t64[:, 3])
    ref = _bilinear_ref(xa)
    # the kernel's fractional offsets ly / lx come from fp32 ho * sy with sy = fp32((H-1) / (2H-1)): off by ~u32 H, which
    # moves the result by ~u32 H times the taps' spread.  Scale: sum w |v| + (u32 / u16) 2 H max|tap|.  Measured b 0.4,
    # bound 1 (u16)
    ti = lambda n: (lambda i0: (i0, (i0 + 1).clamp_max(n - 1)))(
        torch.div(torch.arange(2 * n, device=DEV) * (n - 1), 2 * n - 1, rounding_mode="floor"))
    (y0, y1), (x0, x1) = ti(H), ti(W)
    xa_abs = xa.abs()
    tap = torch.maximum(torch.maximum(xa_abs[:, y0][:, :, x0], xa_abs[:, y0][:, :, x1]),
                        torch.maximum(xa_abs[:, y1][:, :, x0], xa_abs[:, y1][:, :, x1]))
    _check(f"bil fwd {H}x{C}", dest, ref, _bilinear_ref(xa_abs) + (U32 / U16) * 2 * max(H, W) * tap, 1, 1, U16, SUB16)
    del tap
    assert torch.isnan(cat[..., C:]).all(), "the skip's columns are not the kernel's"
    gwide = torch.randn(N, 2 * H, 2 * W, C + Cs, generator=g, device=DEV).half()
    dyv = gwide[..., :C]
    dx = _nan(N, H, W, C)
    T.bilinear2x(dyv, dx, True)
    xr = torch.zeros(N, H, W, C, dtype=torch.float64, device=DEV, requires_grad=True)
    _bilinear_ref(xr).backward(dyv.double())
    xr2 = torch.zeros_like(xr, requires_grad=True)
    _bilinear_ref(xr2).backward(dyv.double().abs())
    # adjoint: fp32 sums of up to 9 taps whose weights come from the same fp32 ly / lx (off by ~u32 H = 0.03 u16 at
    # H = 256): measured b 0.025, bound 0.1 (u16 of sum w |dy|)
    _check(f"bil adj {H}x{C}", dx, xr.grad, xr2.grad, 1, 0.1, U16, SUB16)


# ========================================================================================================================
# 5. The tables above cover every configuration the model passes to these kernels (batch aside)
# ========================================================================================================================
def _ld(t):
    from umi.ops import _nhwc
    return _nhwc(t)[4]


@pytest.mark.parametrize("img", [224, 512])
def test_model_calls_are_covered(img, monkeypatch):
    lib, ops, T = _gpu()
    import loss as L
    from oracle import recipe, ref_transunet
    from TransUnet.vit_seg_modeling import VisionTransformer
    from tests.test_gpu_transunet import product_config
    seen = set()

    def wrap(name, key):
        orig = getattr(T, name)

        def f(*a, **k):
            seen.add(key(*a, **k))
            return orig(*a, **k)
        monkeypatch.setattr(T, name, f)

    wrap("gn_fwd", lambda x, gm, bt, G, eps, relu, res, y: ("gn",) + tuple(x.shape[1:]) + (G, bool(relu), res is not None,
                                                                                            eps, _ld(x), _ld(y)))
    wrap("gn_bwd", lambda dy, y, x, m, r, gm, G, relu, dx, dres, sc, keep_part=False:
         ("gnb",) + tuple(x.shape[1:]) + (G, bool(relu), dres is not None, _ld(dy), _ld(x), _ld(dx)))
    wrap("ln_fwd", lambda x, gm, bt, eps, y: ("ln", x.shape[2] * x.shape[1], x.shape[3], eps, _ld(x), _ld(y)))
    wrap("ln_bwd", lambda dy, x, gm, m, r, dx, sc, keep_part=False: ("lnb", x.shape[2] * x.shape[1], x.shape[3], _ld(dy),
                                                                      _ld(x), _ld(dx)))
    wrap("attn_fwd", lambda q, k, v, o, h: ("attn", q.shape[2], q.shape[3], h, _ld(q), _ld(o)))
    wrap("attn_bwd", lambda q, k, v, o, dO, lse, dq, dk, dv, h: ("attnb", q.shape[2], q.shape[3], h, _ld(q), _ld(o),
                                                                 _ld(dO), _ld(dq)))
    wrap("bilinear2x", lambda x, y, backward=False, tx=None:
         ("bil", bool(backward)) + (tuple(y.shape[1:]) + (_ld(y), _ld(x)) if backward else
                                    tuple(x.shape[1:]) + (_ld(x), _ld(y), tx is not None)))
    cfg = ref_transunet.r50_vit_b16_config(2, 3, dropout_rate=0.0)
    L.CLASS_NUMBER = 2
    torch.manual_seed(0)
    m = VisionTransformer(product_config(cfg, img), img_size=img, num_classes=2, compute_dtype="fp16").to(DEV).train()
    x, lab = recipe.synthetic_batch(1, 1, img, img, 2, seed=1)
    L.calc_loss(m(x.to(DEV)), lab.to(DEV), loss_type="dice_bce_mc").backward()
    torch.cuda.synchronize()

    gn = GN_224 if img == 224 else GN_512
    ntok = (img // 16) ** 2
    allowed = set()
    for H, W, C, G, relu, resid, eps in gn:
        allowed.add(("gn", H, W, C, G, relu, resid, eps, C, C))
        allowed.add(("gnb", H, W, C, G, relu, resid, C, C, C))
    allowed |= {("ln", ntok, C_VIT, 1e-6, C_VIT, C_VIT), ("lnb", ntok, C_VIT, C_VIT, C_VIT, C_VIT),
                ("attn", ntok, C_VIT, HEADS, 3 * C_VIT, C_VIT),
                ("attnb", ntok, C_VIT, HEADS, 3 * C_VIT, C_VIT, C_VIT, 3 * C_VIT)}
    for N, H, W, C, Cs in BIL_CASES:
        if (N == 24) == (img == 224):
            allowed.add(("bil", False, H, W, C, C, C + Cs, True))
            allowed.add(("bil", True, H, W, C, C, C + Cs))
            allowed.add(("bil", True, H, W, C, C, C))
    assert any(k[0] == "attn" for k in seen) and any(k[0] == "gnb" for k in seen), sorted(seen)
    missing = sorted(k for k in seen if k not in allowed)
    assert not missing, f"configurations the model uses that the tables do not pin: {missing}"
