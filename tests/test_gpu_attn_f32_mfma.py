"""The opt-in fp32 matrix-core attention (csrc/attention_mfma_f32.hip, UMI_ATTN_F32_MFMA, compute_dtype "fp32_mfma_attn").

Every case first asserts through umi_attn_plan that the fp32 matrix-core kernel (2) is the one taken.
Rounding: against softmax(QK^T/8)V and its autograd in float64 on the CPU, from the same fp32 standard-normal inputs, inside the
project's fp32 attention bars (tests/test_gpu_kernels_tu.py::test_attention_fwd_bwd): max-abs error <= 2e-5 max|ref| for O and the
log-sum-exp, <= 1e-4 max|ref| for dQ, dK and dV.  tests/test_attn_f32_mfma_plan.py shows on the CPU that torch's float32
evaluation of the same formula stays inside them at every shape used here (tests/attn_f32_cases.py).
Exact cases at zero tolerance, masking against NaN rows and sentinels, silent refusals, the log-sum-exp shared with the VALU
kernels, and the whole R50-ViT-B/16 network with the bars of its "fp32_mfma_gemm" test."""
import os

import numpy as np
import pytest
import torch

from oracle import recipe, ref_transunet
from tests import attn_f32_cases as cases
from tests.test_gpu_transunet import product_config
from tests.test_oracle_golden import sig

pytestmark = pytest.mark.gpu
DEV = "cuda"
D = cases.D
SENTINEL = -777.25
TAIL = 64               # rows of NaN behind the inputs / of sentinel behind the outputs
OUTS = ("o", "lse", "dq", "dk", "dv")


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from umi import lib, ops_tu
    return lib, ops_tu


def _rows(B, N, width, fill):
    """A [(B N + TAIL), width] buffer filled with `fill` and its [B,1,N,width] view of the first B N rows."""
    buf = torch.full((B * N + TAIL, width), fill, device=DEV)
    return buf, buf[:B * N].view(B, 1, N, width)


class _Call:
    """One forward + backward on the device.  Inputs are views of buffers whose last TAIL rows hold NaN, outputs views of buffers
    pre-filled with SENTINEL.  fused_in: q / k / v are channel slices of one [.., 3C] buffer, o (and dO, which shares its stride)
    slices of [.., C + 8] buffers.  fused_grads: dq / dk / dv are slices of one [.., 3C] buffer."""

    def __init__(self, x, shape, fused_in=False, fused_grads=False):
        B, N, heads = shape
        C = heads * D
        self.shape, self.C = shape, C
        nan = float("nan")
        if fused_in:
            _, qkv = _rows(B, N, 3 * C, nan)
            self.q, self.k, self.v = (qkv[..., i * C:(i + 1) * C] for i in range(3))
            self.obuf, ow = _rows(B, N, C + 8, SENTINEL)
            _, dow = _rows(B, N, C + 8, nan)
            self.o, self.dO = ow[..., 4:4 + C], dow[..., 4:4 + C]
            self.o_cols = slice(4, 4 + C)
        else:
            self.q, self.k, self.v, self.dO = (_rows(B, N, C, nan)[1] for _ in range(4))
            self.obuf, self.o = _rows(B, N, C, SENTINEL)
            self.o_cols = slice(0, C)
        for n in ("q", "k", "v", "dO"):
            getattr(self, n).copy_(x[n].to(DEV))
        if fused_grads:
            self.gbuf, g = _rows(B, N, 3 * C, SENTINEL)
            self.dq, self.dk, self.dv = (g[..., i * C:(i + 1) * C] for i in range(3))
        else:
            self.gbuf = None
            self.gbufs, gs = zip(*(_rows(B, N, C, SENTINEL) for _ in range(3)))
            self.dq, self.dk, self.dv = gs

    def plan(self, T, flags, bwd=False):
        return T.attn_plan(self.q, self.k, self.v, self.o, self.shape[2], flags, dq=self.dq if bwd else None)

    def run(self, T, flags, bwd_flags=None):
        heads = self.shape[2]
        self.lse = T.attn_fwd(self.q, self.k, self.v, self.o, heads, flags=flags)
        T.attn_bwd(self.q, self.k, self.v, self.o, self.dO, self.lse, self.dq, self.dk, self.dv, heads,
                   flags=flags if bwd_flags is None else bwd_flags)
        torch.cuda.synchronize()
        return {n: getattr(self, n).detach().cpu().clone() for n in OUTS}

    def assert_nothing_else_was_written(self):
        rows = self.shape[0] * self.shape[1]
        keep = torch.ones_like(self.obuf, dtype=torch.bool)
        keep[:rows, self.o_cols] = False
        assert (self.obuf[keep].view(torch.int32) == torch.tensor(SENTINEL).view(torch.int32).item()).all().item()
        for buf in ([self.gbuf] if self.gbuf is not None else self.gbufs):
            assert (buf[rows:].view(torch.int32) == torch.tensor(SENTINEL).view(torch.int32).item()).all().item()
            assert not (buf[:rows] == SENTINEL).any().item()          # and every element of the slices was written


def _taken(lib, T, call, fwd=True, bwd=True):
    """The fp32 matrix-core kernel is the one the flagged calls take."""
    assert (not fwd or call.plan(T, lib.UMI_ATTN_F32_MFMA) == 2) and (not bwd or call.plan(T, lib.UMI_ATTN_F32_MFMA, bwd=True) == 2)


LAYOUTS = {"contiguous": {}, "fused_qkv": {"fused_in": True}, "fused_grads": {"fused_grads": True}}


# ---- 1 + 3. rounding against float64, on every layout; NaN rows behind the inputs, sentinels around the outputs ---------------------
@pytest.mark.parametrize("shape", cases.SHAPES)
def test_forward_and_backward_against_float64(shape):
    lib, T = _gpu()
    x, ref = cases.case(shape)
    call = _Call(x, shape)
    _taken(lib, T, call)
    cases.assert_inside_bars(call.run(T, lib.UMI_ATTN_F32_MFMA), ref, f"{shape}")
    call.assert_nothing_else_was_written()


@pytest.mark.parametrize("shape", [(2, 33, 2), (2, 50, 4), (2, 196, 3)])
@pytest.mark.parametrize("layout", ["fused_qkv", "fused_grads"])
def test_channel_slices_of_wider_buffers(shape, layout):
    """q / k / v as slices of one [B, N, 3C] buffer (ld = 3C) with o in a slice of a wider one; dq / dk / dv into slices of one
    [B, N, 3C] buffer (ldd = 3C).  The other columns and the rows past B N keep their sentinel bit for bit."""
    lib, T = _gpu()
    x, ref = cases.case(shape)
    call = _Call(x, shape, **LAYOUTS[layout])
    _taken(lib, T, call)
    got = call.run(T, lib.UMI_ATTN_F32_MFMA)
    cases.assert_inside_bars(got, ref, f"{shape} {layout}")
    call.assert_nothing_else_was_written()
    # the layout changes addresses only: the same bits as the contiguous call
    plain = _Call(x, shape).run(T, lib.UMI_ATTN_F32_MFMA)
    for n in OUTS:
        assert torch.equal(got[n], plain[n]), n


# ---- 2. exact cases ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [32, 64, 256])
def test_zero_queries_give_the_mean_of_v_bit_for_bit(N):
    """Q = 0: every score is 0, exp(0) = 1, the sum is N and 1 / N a power of two, V small integers: O is the per-head mean of V."""
    lib, T = _gpu()
    B, heads = 2, 2
    g = torch.Generator().manual_seed(N)
    x = {"q": torch.zeros(B, 1, N, heads * D), "k": torch.randn(B, 1, N, heads * D, generator=g),
         "v": torch.randint(-8, 9, (B, 1, N, heads * D), generator=g).float(), "dO": torch.zeros(B, 1, N, heads * D)}
    assert x["v"].abs().sum(2).max().item() < 2 ** 24         # the integer sums are exact in any order
    ref = (x["v"].sum(2, keepdim=True) / N).expand(B, 1, N, heads * D)
    call = _Call(x, (B, N, heads))
    _taken(lib, T, call)
    got = call.run(T, lib.UMI_ATTN_F32_MFMA)
    assert torch.equal(got["o"], ref)
    assert (got["lse"].double() - np.log(N)).abs().max().item() <= cases.TOL_FWD * np.log(N)     # max = 0, sum = N


def test_samples_and_heads_are_independent_bit_for_bit():
    lib, T = _gpu()
    shape = B, N, heads = 3, 50, 3
    x, _ = cases.case(shape)
    whole = _Call(x, shape)
    _taken(lib, T, whole)
    got = whole.run(T, lib.UMI_ATTN_F32_MFMA)
    lse = got["lse"].view(B, heads, N)
    for b in range(B):                                          # sample b of the B = 3 call == a B = 1 call on that sample
        one = _Call({n: t[b:b + 1] for n, t in x.items()}, (1, N, heads))
        _taken(lib, T, one)
        alone = one.run(T, lib.UMI_ATTN_F32_MFMA)
        for n in ("o", "dq", "dk", "dv"):
            assert torch.equal(got[n][b:b + 1], alone[n]), (b, n)
        assert torch.equal(lse[b].reshape(-1), alone["lse"]), b
    for h in range(heads):                                      # head h == a 1-head call on that channel slice, same strides
        sl = slice(h * D, (h + 1) * D)
        c = _Call(x, shape)
        for n in ("q", "k", "v", "dO", "o", "dq", "dk", "dv"):
            setattr(c, n, getattr(c, n)[..., sl])
        c.shape = (B, N, 1)
        _taken(lib, T, c)
        alone = c.run(T, lib.UMI_ATTN_F32_MFMA)
        for n in ("o", "dq", "dk", "dv"):
            assert torch.equal(got[n][..., sl], alone[n]), (h, n)
        assert torch.equal(lse[:, h].reshape(-1), alone["lse"]), h


@pytest.mark.parametrize("shape", [(2, 50, 4), (2, 196, 3)])
def test_two_calls_give_identical_bits(shape):
    lib, T = _gpu()
    x, _ = cases.case(shape)
    outs = []
    for _ in range(2):
        call = _Call(x, shape, fused_in=True, fused_grads=True)
        _taken(lib, T, call)
        outs.append(call.run(T, lib.UMI_ATTN_F32_MFMA))
    for n in OUTS:
        assert torch.equal(outs[0][n], outs[1][n]), n


# ---- 4. refusals are silent and exact ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,kernel", [("d32", 0), ("fp16", 1), ("ld", 0)])
def test_flag_is_ignored_on_the_device(what, kernel):
    """Head dimension 32 in fp32, fp16 at head dimension 64 and a row stride that is no multiple of 4: the plan names the kernel
    the flag-less call takes, and every output equals the flag-less call's bit for bit."""
    lib, T = _gpu()
    B, N, heads = 2, 50, 2
    g = torch.Generator().manual_seed(7)
    d = 32 if what == "d32" else 64
    C, dt = heads * d, torch.float16 if what == "fp16" else torch.float32
    wide = C + 2 if what == "ld" else C
    src = [torch.randn(B, 1, N, C, generator=g).to(dt) for _ in range(4)]
    outs = []
    for flags in (0, lib.UMI_ATTN_F32_MFMA):
        q, k, v, dO = (torch.zeros(B, 1, N, wide, device=DEV, dtype=dt)[..., :C].copy_(t.to(DEV)) for t in src)
        o, dq, dk, dv = (torch.zeros(B, 1, N, wide, device=DEV, dtype=dt)[..., :C] for _ in range(4))
        assert T.attn_plan(q, k, v, o, heads, flags) == T.attn_plan(q, k, v, o, heads, flags, dq=dq) == kernel
        lse = T.attn_fwd(q, k, v, o, heads, flags=flags)
        T.attn_bwd(q, k, v, o, dO, lse, dq, dk, dv, heads, flags=flags)
        outs.append([t.cpu().clone() for t in (o, lse, dq, dk, dv)])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert all(torch.isfinite(t.float()).all().item() for t in outs[0])


# ---- 5. the log-sum-exp is the VALU kernels' ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 50, 4), (2, 196, 3)])
@pytest.mark.parametrize("fwd_flag,bwd_flag", [(1, 0), (0, 1)])
def test_forward_of_one_kernel_feeds_the_backward_of_the_other(shape, fwd_flag, bwd_flag):
    lib, T = _gpu()
    assert lib.UMI_ATTN_F32_MFMA == 1
    x, ref = cases.case(shape)
    call = _Call(x, shape)
    _taken(lib, T, call, fwd=bool(fwd_flag), bwd=bool(bwd_flag))
    assert call.plan(T, 0) == call.plan(T, 0, bwd=True) == 0        # and the other half is the VALU kernels'
    cases.assert_inside_bars(call.run(T, fwd_flag, bwd_flags=bwd_flag), ref, f"{shape} fwd flag {fwd_flag} bwd flag {bwd_flag}")


# ---- 6. whole networks ---------------------------------------------------------------------------------------------------------------
class _Spy:
    """Records (kind, flags, the kernel umi_attn_plan names) of every attention call of the tape."""

    def __init__(self, monkeypatch):
        from umi import ops_tu
        self.calls = []
        fwd, bwd = ops_tu.attn_fwd, ops_tu.attn_bwd

        def attn_fwd(q, k, v, o, heads, flags=0):
            self.calls.append(("fwd", flags, ops_tu.attn_plan(q, k, v, o, heads, flags)))
            return fwd(q, k, v, o, heads, flags=flags)

        def attn_bwd(q, k, v, o, dO, lse, dq, dk, dv, heads, flags=0):
            self.calls.append(("bwd", flags, ops_tu.attn_plan(q, k, v, o, heads, flags, dq=dq)))
            return bwd(q, k, v, o, dO, lse, dq, dk, dv, heads, flags=flags)

        monkeypatch.setattr(ops_tu, "attn_fwd", attn_fwd)
        monkeypatch.setattr(ops_tu, "attn_bwd", attn_bwd)


def test_transunet_r50_vit_b16_224_fp32_mfma_attn(golden_dir, monkeypatch):
    """tests/test_gpu_gemm_f32_mfma.py::test_transunet_r50_vit_b16_224_fp32_mfma_gemm under "fp32_mfma_attn", same bars; all 12
    attention forwards and backwards take the fp32 matrix-core kernels."""
    lib, _ = _gpu()
    import loss as L
    from TransUnet.vit_seg_modeling import VisionTransformer
    spy = _Spy(monkeypatch)
    g = np.load(os.path.join(golden_dir, "transunet_r50_b16_224.npz"))
    cfg = ref_transunet.r50_vit_b16_config(2, 3, dropout_rate=0.0)
    L.CLASS_NUMBER = 2
    m = VisionTransformer(product_config(cfg, 224), img_size=224, num_classes=2, compute_dtype="fp32_mfma_attn")
    assert len(m.state_dict()) == 409
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=int(g["seed"]), negative_gamma=False))
    m.to(DEV).train()
    x, lab = recipe.synthetic_batch(1, 1, 224, 224, 2, seed=int(g["seed"]))
    logits = m(x.to(DEV))
    loss = L.calc_loss(logits, lab.to(DEV), loss_type="dice_bce_mc")
    loss.backward()
    assert spy.calls == [("fwd", lib.UMI_ATTN_F32_MFMA, 2)] * 12 + [("bwd", lib.UMI_ATTN_F32_MFMA, 2)] * 12, spy.calls
    s = sig(logits.cpu())
    np.testing.assert_allclose(s[[0, 2]], g["logits_sig"][[0, 2]], rtol=2e-4)
    np.testing.assert_allclose(s[3:], g["logits_sig"][3:], rtol=1e-3, atol=1e-3 * s[0] / 300)
    assert abs(loss.item() - float(g["loss0"])) < 2e-5
    bad = []
    for k, p in m.named_parameters():
        ref_norm = float(g["grad_sig." + k][0])
        assert torch.isfinite(p.grad).all(), k
        if ref_norm < 1e-7:                                    # e.g. key biases: mathematically zero gradient
            continue
        if abs(p.grad.double().norm().item() - ref_norm) > 1e-2 * ref_norm:
            bad.append((k, p.grad.double().norm().item(), ref_norm))
    assert not bad, bad[:5]


def test_standalone_attention_module_takes_the_mode_from_the_environment(monkeypatch):
    """`Attention.forward` on its own builds a tape of its own: under UMI_COMPUTE_DTYPE="fp32_mfma_attn" that tape passes the flag and
    the fp32 matrix-core kernels run, under "fp32_mfma_gemm" neither.  The two runs share every other kernel and each attention is
    inside its bar against float64, so they differ by at most the sum of the two bars."""
    lib, _ = _gpu()
    from TransUnet.vit_seg_modeling import CONFIGS, Attention
    spy = _Spy(monkeypatch)
    torch.manual_seed(0)
    m = Attention(CONFIGS["R50-ViT-B_16"], False).to(DEV).train()
    x, gy = torch.randn(2, 50, 768, device=DEV), torch.randn(2, 50, 768, device=DEV)
    runs = {}
    for mode, want in (("fp32_mfma_gemm", (0, 0)), ("fp32_mfma_attn", (lib.UMI_ATTN_F32_MFMA, 2))):
        monkeypatch.setenv("UMI_COMPUTE_DTYPE", mode)
        spy.calls.clear()
        xr = x.clone().requires_grad_(True)
        y, _none = m(xr)
        y.backward(gy)
        assert spy.calls == [("fwd",) + want, ("bwd",) + want], (mode, spy.calls)
        runs[mode] = (y.detach().cpu(), xr.grad.cpu())
    for (a, b), tol in zip(zip(*runs.values()), (2 * cases.TOL_FWD, 2 * cases.TOL_BWD)):
        assert torch.isfinite(b).all() and (a - b).abs().max().item() <= tol * a.abs().max().item()


def test_transunet_small_ignores_the_flag_bit_for_bit(golden_dir, monkeypatch):
    """The small TransUNet fixture has head dimension 16: under "fp32_mfma_attn" the tape passes the flag, the plan names the VALU
    kernels and logits, loss and every gradient equal the "fp32_mfma_gemm" run's bit for bit.  "fp32_mfma_gemm" itself passes no
    flag."""
    lib, _ = _gpu()
    import loss as L
    from TransUnet.vit_seg_modeling import VisionTransformer
    spy = _Spy(monkeypatch)
    g = np.load(os.path.join(golden_dir, "transunet_small.npz"))
    cfg = ref_transunet.small_config(2)
    img, B, cin, seed = int(g["img"]), int(g["B"]), int(g["cin"]), int(g["seed"])
    ref = ref_transunet.RefTransUNet(cfg, img)
    state = recipe.fill_state_dict(ref.state_dict(), seed=seed, negative_gamma=False)
    x, lab = recipe.synthetic_batch(B, cin, img, img, 2, seed=seed)
    L.CLASS_NUMBER = 2
    runs = {}
    for mode in ("fp32_mfma_gemm", "fp32_mfma_attn"):
        spy.calls.clear()
        m = VisionTransformer(product_config(cfg, img), img_size=img, num_classes=2, compute_dtype=mode)
        m.load_state_dict(state)
        m.to(DEV).train()
        logits = m(x.to(DEV))
        loss = L.calc_loss(logits, lab.to(DEV), loss_type="dice_bce_mc")
        loss.backward()
        flag = lib.UMI_ATTN_F32_MFMA if mode == "fp32_mfma_attn" else 0
        assert spy.calls and {c[1:] for c in spy.calls} == {(flag, 0)}, spy.calls
        assert {c[0] for c in spy.calls} == {"fwd", "bwd"}
        runs[mode] = [logits.detach().cpu(), loss.detach().cpu()] + [p.grad.cpu() for p in m.parameters()]
    for a, b in zip(*runs.values()):
        assert torch.equal(a, b)
