"""Attention-probability dropout on the MI355X: umi_attn_fwd_dropout / umi_attn_bwd_dropout in the four kernel families
(VALU fp32 at D = 16, VALU fp16 at D = 32, the fp16 and the fp32 matrix-core kernels at D = 64) and the TransUNet models on top.

A. values of o, lse, dq, dk, dv against the float64 restatement with the NumPy mask, inside the project's attention bars
B. the masks of the forward, the dQ and the dK/dV kernels bit for bit, through read-out inputs (tests/attn_dropout_cases.py)
C. p = 0 is the call without dropout bit for bit; p = 1 gives zeros and nothing non-finite; lse never sees the mask
D. the stream: repeatable, (seed, counter) == (seed + counter * 0x9E3779B9, no counter), counters differ
E. q / k / v and dq / dk / dv as channel slices of [B, N, 3C] buffers, bit for bit the contiguous call
F. the models: a standalone Attention, VisionTransformer (training, eval, reproducibility, distinct seeds), the snapshot of the
   device counter, head dimension 64 under "fp16" and "fp32_mfma_attn", and graph capture (child process)."""
import os
import subprocess
import sys

import pytest
import torch

from oracle import ref_transunet
from tests import attn_dropout_cases as cases
from tests import dropout_stream as stream
from tests.test_gpu_transunet import product_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUTS = cases.OUTS
FAMS = list(cases.FAMILIES)


def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from umi import lib, ops_tu
    return lib, ops_tu


def _counter(c):
    return None if c is None else torch.tensor([c], dtype=torch.int32, device=DEV)


class _Call:
    """One forward + backward on the device.  fused: q / k / v are the three slices of one [B,1,N,3C] buffer and dq / dk / dv go
    into the slices of another one filled with NaN (ld = ldd = 3C, as TUTape.qkv_attention calls the kernels)."""

    def __init__(self, x, shape, fam, fused=False):
        B, N, heads = shape
        self.shape, self.fam, C, dt = shape, fam, heads * fam["D"], fam["dtype"]
        if fused:
            qkv = torch.empty(B, 1, N, 3 * C, device=DEV, dtype=dt)
            g = torch.full((B, 1, N, 3 * C), float("nan"), device=DEV, dtype=dt)
            self.q, self.k, self.v = (qkv[..., i * C:(i + 1) * C] for i in range(3))
            self.dq, self.dk, self.dv = (g[..., i * C:(i + 1) * C] for i in range(3))
        else:
            self.q, self.k, self.v = (torch.empty(B, 1, N, C, device=DEV, dtype=dt) for _ in range(3))
            self.dq, self.dk, self.dv = (torch.full((B, 1, N, C), float("nan"), device=DEV, dtype=dt) for _ in range(3))
        self.o = torch.full((B, 1, N, C), float("nan"), device=DEV, dtype=dt)
        self.dO = torch.empty(B, 1, N, C, device=DEV, dtype=dt)
        for n in ("q", "k", "v", "dO"):
            getattr(self, n).copy_(x[n].to(DEV))

    def taken(self, T):
        """Dropout never changes the selection: the plan names the family's kernel, forward and backward."""
        heads, fl = self.shape[2], self.fam["flags"]
        assert T.attn_plan(self.q, self.k, self.v, self.o, heads, fl) == self.fam["kernel"]
        assert T.attn_plan(self.q, self.k, self.v, self.o, heads, fl, dq=self.dq) == self.fam["kernel"]

    def run(self, T, p=0.0, seed=0, counter=None, direct=False, bwd=True):
        """Through umi.ops_tu (p = 0: the existing entry points), or `direct`: the new C entry points whatever p is."""
        from umi import lib as L
        from umi.ops import _dt, _nhwc, _ptr, _stream
        self.taken(T)
        B, N, heads = self.shape
        D, fl, sd = self.fam["D"], self.fam["flags"], _counter(counter)
        if direct:
            ld, ldo, ldd = _nhwc(self.q)[4], _nhwc(self.o)[4], _nhwc(self.dq)[4]
            self.lse = torch.empty(B * heads * N, dtype=torch.float32, device=DEV)
            delta = torch.empty_like(self.lse)
            L.call("umi_attn_fwd_dropout", self.q.data_ptr(), self.k.data_ptr(), self.v.data_ptr(), ld, self.o.data_ptr(), ldo,
                   self.lse.data_ptr(), B, N, heads, D, _dt(self.q), fl, p, seed & 0xFFFFFFFF, _ptr(sd), _stream())
            if bwd:
                L.call("umi_attn_bwd_dropout", self.q.data_ptr(), self.k.data_ptr(), self.v.data_ptr(), ld, self.o.data_ptr(),
                       self.dO.data_ptr(), ldo, self.lse.data_ptr(), self.dq.data_ptr(), self.dk.data_ptr(), self.dv.data_ptr(),
                       ldd, delta.data_ptr(), B, N, heads, D, _dt(self.q), fl, p, seed & 0xFFFFFFFF, _ptr(sd), _stream())
        else:
            kw = dict(flags=fl, p=p, seed=seed, seed_dev=sd) if p > 0 else dict(flags=fl)
            self.lse = T.attn_fwd(self.q, self.k, self.v, self.o, heads, **kw)
            if bwd:
                T.attn_bwd(self.q, self.k, self.v, self.o, self.dO, self.lse, self.dq, self.dk, self.dv, heads, **kw)
        torch.cuda.synchronize()
        return {n: getattr(self, n).detach().cpu().clone() for n in (OUTS if bwd else ("o", "lse"))}


def _same(a, b, names=OUTS):
    for n in names:
        assert torch.equal(a[n], b[n]), n


# ---- A. values ---------------------------------------------------------------------------------------------------------------------------
VALUE_CASES = [(f, s, p) for f in FAMS for s in cases.FAMILIES[f]["shapes"] for p in (0.1, 0.5)]


@pytest.mark.parametrize("family,shape,p", VALUE_CASES)
def test_values_against_float64(family, shape, p):
    _, T = _gpu()
    fam = cases.FAMILIES[family]
    x, ref = cases.case(shape, fam["D"], fam["dtype"], p)
    got = _Call(x, shape, fam).run(T, p, cases.SEED, cases.COUNTER)
    cases.assert_inside_bars(got, ref, fam["bars"], f"{family} {shape} p={p}")


@pytest.mark.parametrize("family", FAMS)
def test_values_with_a_negative_counter(family):
    """The device scalar is an int32; -3 enters the stream as 2^32 - 3."""
    _, T = _gpu()
    fam = cases.FAMILIES[family]
    shape = fam["shapes"][0]
    x, ref = cases.case(shape, fam["D"], fam["dtype"], 0.5, cases.SEED, cases.NEG_COUNTER)
    got = _Call(x, shape, fam).run(T, 0.5, cases.SEED, cases.NEG_COUNTER)
    cases.assert_inside_bars(got, ref, fam["bars"], f"{family} {shape} counter {cases.NEG_COUNTER}")


# ---- B. masks, per kernel ------------------------------------------------------------------------------------------------------------------
READOUT_CASES = [(f, s) for f in FAMS for s in cases.FAMILIES[f]["readout"]]


@pytest.mark.parametrize("family,shape", READOUT_CASES)
def test_masks_bit_for_bit(family, shape):
    """Forward: O != 0 is the mask.  K/V side: dV != 0 is the mask.  dQ: dQ > 0 is the mask.  Every window of D keys / queries
    (the first, a middle and the last one at N = 1,024); tests/test_attn_dropout.py checks the preconditions in float64."""
    _, T = _gpu()
    fam = cases.FAMILIES[family]
    D, p = fam["D"], cases.READOUT_P
    m = cases.keep(shape, p, cases.SEED, cases.COUNTER)
    for r0 in cases.windows(shape[1], D):
        for kind in ("o", "dv", "dq"):
            x = cases.readout(kind, shape, D, r0, fam["dtype"])
            got = _Call(x, shape, fam).run(T, p, cases.SEED, cases.COUNTER, bwd=kind != "o")
            want = cases.window_of_mask(kind, m, shape, D, r0)
            diff = (cases.shown(kind, got, shape, D, r0) != want).sum().item()
            assert diff == 0, f"{family} {shape} {kind} window {r0}: {diff} of {want.numel()} mask bits differ"


# ---- C. edges ------------------------------------------------------------------------------------------------------------------------------
def _edge_shape(fam):
    return (2, 196, 3) if fam["D"] == 64 else fam["shapes"][0]


@pytest.mark.parametrize("family", FAMS)
def test_p_zero_is_the_call_without_dropout(family):
    _, T = _gpu()
    fam = cases.FAMILIES[family]
    shape = _edge_shape(fam)
    x = cases.inputs(shape, fam["D"], fam["dtype"])
    _same(_Call(x, shape, fam).run(T, 0.0, cases.SEED, cases.COUNTER, direct=True), _Call(x, shape, fam).run(T))


@pytest.mark.parametrize("family", FAMS)
def test_p_one_keeps_nothing_and_lse_never_sees_the_mask(family):
    _, T = _gpu()
    fam = cases.FAMILIES[family]
    shape = _edge_shape(fam)
    x = cases.inputs(shape, fam["D"], fam["dtype"])
    plain = _Call(x, shape, fam).run(T)
    one = _Call(x, shape, fam).run(T, 1.0, cases.SEED, cases.COUNTER)
    for n in ("o", "dq", "dk", "dv"):
        assert (one[n] == 0).all().item(), n                      # (NaN != 0: also "everything finite")
    assert torch.equal(one["lse"], plain["lse"])
    half = _Call(x, shape, fam).run(T, 0.5, cases.SEED, cases.COUNTER)
    assert torch.equal(half["lse"], plain["lse"])
    assert all(torch.isfinite(t.float()).all().item() for t in half.values())


# ---- D. the stream -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMS)
def test_stream_facts(family):
    _, T = _gpu()
    fam = cases.FAMILIES[family]
    shape = _edge_shape(fam)
    x = cases.inputs(shape, fam["D"], fam["dtype"])
    a = _Call(x, shape, fam).run(T, 0.5, cases.SEED, cases.COUNTER)
    _same(a, _Call(x, shape, fam).run(T, 0.5, cases.SEED, cases.COUNTER))                      # the same call twice
    folded = stream.effective_seed(cases.SEED, cases.COUNTER)
    assert folded == (cases.SEED + cases.COUNTER * 0x9E3779B9) % 2 ** 32
    _same(a, _Call(x, shape, fam).run(T, 0.5, folded, None))                                    # the counter folded into the seed
    other = _Call(x, shape, fam).run(T, 0.5, cases.SEED, cases.COUNTER + 1)
    for n in ("o", "dq", "dk", "dv"):
        assert not torch.equal(a[n], other[n]), n


# ---- E. strided views ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMS)
def test_slices_of_fused_buffers_equal_the_contiguous_call(family):
    _, T = _gpu()
    fam = cases.FAMILIES[family]
    shape = _edge_shape(fam)
    x = cases.inputs(shape, fam["D"], fam["dtype"])
    _same(_Call(x, shape, fam, fused=True).run(T, 0.1, cases.SEED, cases.COUNTER),
          _Call(x, shape, fam).run(T, 0.1, cases.SEED, cases.COUNTER))


# ---- F. models -----------------------------------------------------------------------------------------------------------------------------
class _Spy:
    """Records the attention calls of a tape (arguments, tensors and the kernel umi_attn_plan names) and the seed of every
    dropout site that ran."""

    def __init__(self, monkeypatch):
        from umi import ops_tu
        self.fwd, self.bwd, self.seeds = [], [], []
        real = {n: getattr(ops_tu, n) for n in ("attn_fwd", "attn_bwd", "dropout", "dropout_fused", "linear_fused")}

        def attn_fwd(q, k, v, o, heads, **kw):
            lse = real["attn_fwd"](q, k, v, o, heads, **kw)
            self.fwd.append(dict(kw, heads=heads, kernel=ops_tu.attn_plan(q, k, v, o, heads, kw.get("flags", 0)),
                                 counter=None if kw.get("seed_dev") is None else int(kw["seed_dev"].item()),
                                 q=q.detach().clone(), k=k.detach().clone(), v=v.detach().clone(), o=o.detach().clone(), lse=lse.clone()))
            if kw.get("p", 0.0) > 0:
                self.seeds.append(kw["seed"] & 0xFFFFFFFF)
            return lse

        def attn_bwd(q, k, v, o, dO, lse, dq, dk, dv, heads, **kw):
            real["attn_bwd"](q, k, v, o, dO, lse, dq, dk, dv, heads, **kw)
            self.bwd.append(dict(kw, counter=None if kw.get("seed_dev") is None else int(kw["seed_dev"].item()),
                                 kernel=ops_tu.attn_plan(q, k, v, o, heads, kw.get("flags", 0), dq=dq),
                                 dO=dO.detach().clone(), dq=dq.detach().clone(), dk=dk.detach().clone(), dv=dv.detach().clone()))

        def dropout(x, y, mask, backward, p, seed, *a, **kw):
            if not backward:
                self.seeds.append(seed & 0xFFFFFFFF)
            return real["dropout"](x, y, mask, backward, p, seed, *a, **kw)

        def dropout_fused(x, y, mask, backward, p, seed, *a, **kw):
            ran = real["dropout_fused"](x, y, mask, backward, p, seed, *a, **kw)
            if ran and not backward:
                self.seeds.append(seed & 0xFFFFFFFF)
            return ran

        def linear_fused(x, wp8, bias, y, epi, p, seed, *a, **kw):
            ran = real["linear_fused"](x, wp8, bias, y, epi, p, seed, *a, **kw)
            if ran:
                self.seeds.append(seed & 0xFFFFFFFF)
            return ran

        for n, f in (("attn_fwd", attn_fwd), ("attn_bwd", attn_bwd), ("dropout", dropout), ("dropout_fused", dropout_fused),
                     ("linear_fused", linear_fused)):
            monkeypatch.setattr(ops_tu, n, f)


def _small(rate, **over):
    """The small TransUNet fixture config (head dimension 16) with dropout."""
    return dict(ref_transunet.small_config(2), attention_dropout_rate=rate, dropout_rate=0.1 if rate else 0.0, **over)


def _hd64(rate):
    """The same miniature with hidden 128 and 2 heads: head dimension 64, 16 tokens at 64 x 64."""
    return _small(rate, hidden_size=128, num_heads=2, mlp_dim=256)


def _model(cfg, mode="fp32", seed=0):
    from TransUnet.vit_seg_modeling import VisionTransformer
    torch.manual_seed(seed)
    return VisionTransformer(product_config(cfg, 64), img_size=64, num_classes=2, compute_dtype=mode).to(DEV)


def _batch(seed=1, B=2):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, 1, 64, 64, generator=g).to(DEV), torch.randint(0, 2, (B, 64, 64), generator=g).float().to(DEV)


def _loss(m, x, lab):
    import loss as L
    L.CLASS_NUMBER = 2
    return L.calc_loss(m(x), lab, loss_type="dice_bce_mc")


def test_standalone_attention_module(monkeypatch):
    """Attention(rate 0.3) on a tape of its own: the forward and the backward call get the same (p, seed, snapshot), and with the
    mask of exactly those the attention lies inside the fp32 bars against the float64 restatement."""
    _gpu()
    from TransUnet.vit_seg_modeling import Attention
    monkeypatch.setenv("UMI_COMPUTE_DTYPE", "fp32")
    spy = _Spy(monkeypatch)
    torch.manual_seed(0)
    m = Attention(product_config(_hd64(0.3), 64), False).to(DEV).train()
    B, N, heads, D = 2, 50, 2, 64
    x = torch.randn(B, N, heads * D, device=DEV, requires_grad=True)
    y, _none = m(x)
    y.backward(torch.randn_like(y))
    assert len(spy.fwd) == len(spy.bwd) == 1
    f, b = spy.fwd[0], spy.bwd[0]
    assert abs(f["p"] - 0.3) < 1e-12 and f["counter"] is not None
    assert (b["p"], b["seed"], b["counter"]) == (f["p"], f["seed"], f["counter"])
    assert len(set(spy.seeds)) == len(spy.seeds) == 2                                           # the mask and the projection dropout
    shape = (B, N, heads)
    rec = {"q": f["q"], "k": f["k"], "v": f["v"], "dO": b["dO"]}
    ref = cases.evaluate({n: t.cpu() for n, t in rec.items()}, cases.keep(shape, f["p"], f["seed"], f["counter"]), f["p"], shape, D)
    got = {"o": f["o"], "lse": f["lse"], "dq": b["dq"], "dk": b["dk"], "dv": b["dv"]}
    cases.assert_inside_bars(got, ref, cases.BARS_F32, "Attention(0.3)")
    assert torch.isfinite(x.grad).all().item()


def test_vision_transformer_trains_and_eval_ignores_the_rate(monkeypatch):
    _gpu()
    spy = _Spy(monkeypatch)
    m = _model(_small(0.1)).train()
    x, lab = _batch()
    opt = torch.optim.SGD(m.parameters(), lr=0.01)
    for step in range(2):
        spy.seeds.clear()
        opt.zero_grad(set_to_none=True)
        loss = _loss(m, x, lab)
        loss.backward()
        assert torch.isfinite(loss).item()
        assert all(p.grad is not None and torch.isfinite(p.grad).all().item() for p in m.parameters())
        # embeddings + per layer (attention mask, projection, fc1, fc2): nine sites, nine seeds
        assert len(spy.seeds) == 9 and len(set(spy.seeds)) == 9, spy.seeds
        opt.step()
    assert [c["p"] for c in spy.fwd] == [0.1] * 4 and [c["p"] for c in spy.bwd] == [0.1] * 4
    # every layer of one forward reads one snapshot, and the backward reads the same one
    assert [c["counter"] for c in spy.fwd] == [1, 1, 2, 2] and [c["counter"] for c in spy.bwd] == [1, 1, 2, 2]
    plain = _model(_small(0.0))
    plain.load_state_dict(m.state_dict())
    with torch.no_grad():
        assert torch.equal(m.eval()(x), plain.eval()(x))


def test_the_same_manual_seed_gives_the_same_run():
    _gpu()
    x, lab = _batch()
    runs = []
    for _ in range(2):
        m = _model(_small(0.1), seed=11).train()
        out = []
        for _step in range(2):
            m.zero_grad(set_to_none=True)
            loss = _loss(m, x, lab)
            loss.backward()
            out += [loss.detach().cpu()] + [p.grad.cpu().clone() for p in m.parameters()]
        runs.append(out)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_counter_snapshot_survives_an_interleaved_forward():
    """forward A, forward B, backward A, backward B == the two steps one after the other from the same counter values: A's
    backward rebuilds A's mask although B's forward has advanced the device counter in between."""
    _gpu()
    m = _model(_small(0.1)).train()
    (xa, la), (xb, lb) = _batch(1), _batch(2)
    params = list(m.parameters())
    _loss(m, xa, la)                                              # creates the model's seed and counter
    m._drop_step.fill_(10)
    fa, fb = _loss(m, xa, la), _loss(m, xb, lb)
    ga, gb = torch.autograd.grad(fa, params), torch.autograd.grad(fb, params)
    m._drop_step.fill_(10)
    fa2 = _loss(m, xa, la)
    ga2 = torch.autograd.grad(fa2, params)
    fb2 = _loss(m, xb, lb)
    gb2 = torch.autograd.grad(fb2, params)
    assert torch.equal(fa, fa2) and torch.equal(fb, fb2)
    for a, b in zip(ga + gb, ga2 + gb2):
        assert torch.equal(a, b)


@pytest.mark.parametrize("mode,kernel", [("fp16", 1), ("fp32_mfma_attn", 2)])
def test_head_dimension_64_model_takes_the_matrix_core_kernels(monkeypatch, mode, kernel):
    _gpu()
    spy = _Spy(monkeypatch)
    m = _model(_hd64(0.1), mode).train()
    x, lab = _batch()
    loss = _loss(m, x, lab)
    loss.backward()
    assert torch.isfinite(loss).item() and all(torch.isfinite(p.grad).all().item() for p in m.parameters())
    assert [(c["kernel"], c["p"]) for c in spy.fwd] == [(kernel, 0.1)] * 2, spy.fwd
    assert [(c["kernel"], c["p"]) for c in spy.bwd] == [(kernel, 0.1)] * 2


def test_graph_capture_follows_eager_and_draws_fresh_masks():
    """Child process (stream capture is sensitive to what ran before it): tools/check_attn_dropout_graph.py."""
    _gpu()
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_attn_dropout_graph.py")], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "ATTN_DROPOUT_GRAPH_OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
