"""Pure-ViT TransUNet (patch gather -> patch GEMM -> ViT encoder -> CUP decoder without skips) on the HIP path against the
reference's fixtures (tools/gen_golden_vit.py) and, for full gradients and post-step parameters, against a float64 run of the
tests' plain restatement (tests/vit_plain.py, itself pinned to the same fixtures in tests/test_vit_pure.py).

Bars are those of the hybrid's tests (tests/test_gpu_transunet.py), restated where they are used.  The HIP-graph and the
UMI_TRACE_GENERIC cases run this file as a child process, like tests/test_gpu_poisoned_step.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

if __name__ == "__main__":
    _REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_REPO, os.path.join(_REPO, "unet-torch_amd")]

from oracle import recipe
from tests import vit_plain
from tests.test_oracle_golden import sig
from tests.test_vit_pure import _named, logits_close, plain_case
from tools.gen_golden_vit import small_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SGD = dict(lr=0.01, momentum=0.9, weight_decay=1e-4)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: torch.cuda.is_available() is False")


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@functools.lru_cache(maxsize=None)
def _plain64(name):
    """One float64 training step of the plain restatement on the fixture's weights and batch: computed once per fixture, read only."""
    g, cfg, m, x, labs, outputs = plain_case(GOLDEN, name)
    names = [k for k, _ in m.named_parameters()]
    return vit_plain.train_step(m.state_dict(), names, x, [l.double() for l in labs], cfg["n_classes"], cfg["num_heads"],
                                cfg["patch"], outputs, dtype=torch.float64, **SGD)


def _loss(out, labs):
    import loss as L
    outs = out if isinstance(out, (tuple, list)) else (out,)
    return outs, sum(L.calc_loss(o, l, loss_type="dice_bce_mc") for o, l in zip(outs, labs))


@pytest.mark.parametrize("dtype", ["fp32", "fp32_mfma_attn"])
@pytest.mark.parametrize("name", ["vit_small_p16", "vit_small_p32_rgb", "vit_small_multitask"])
def test_vit_small_fp32_parity(name, dtype):
    _need_gpu()
    import loss as L
    from umi import optim as uo
    g, cfg, m, x, labs, _ = plain_case(GOLDEN, name)
    ref = _plain64(name)
    L.CLASS_NUMBER = cfg["n_classes"]
    m._compute_dtype = dtype
    m.to(DEV).train()
    opt = uo.SGD(m.parameters(), **SGD)
    outs, loss = _loss(m(x.to(DEV)), [l.to(DEV) for l in labs])
    opt.zero_grad(set_to_none=True)
    loss.backward()
    tags = ["logits"] if len(outs) == 1 else [f"logits{i + 1}" for i in range(len(outs))]
    for o, t in zip(outs, tags):
        assert tuple(o.shape) == g[t].shape                       # P = 32: half-size logits, as the reference's
        logits_close(o, g[t])
    print(name, dtype, "loss", loss.item(), "fixture", float(g["loss0"]))
    assert abs(loss.item() - float(g["loss0"])) < 1e-4
    w = m.transformer.embeddings.patch_embeddings.weight
    assert w.grad.shape == w.shape and w.dim() == 4 and w.grad.is_contiguous()
    worst, worst_sig = ("", 0.0), ("", 0.0)
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        rg = ref["grads"][k]
        # key biases have a mathematically zero gradient (softmax is shift invariant): absolute floor 1e-6
        e = (p.grad.detach().double().cpu() - rg).norm().item() / (rg.norm().item() + 1e-6 / 3e-3)
        worst = max(worst, (k, e), key=lambda t: t[1])
        rn = float(g["grad_sig." + k][0])
        worst_sig = max(worst_sig, (k, abs(p.grad.double().norm().item() - rn) / (rn + 1e-6 / 3e-3)), key=lambda t: t[1])
    print(name, dtype, "worst gradient vs plain float64", worst, "worst gradient norm vs fixture", worst_sig)
    assert worst[1] < 3e-3, worst
    assert worst_sig[1] < 3e-3, worst_sig
    opt.step()
    worst = max(((k, rel_err(v, ref["after"][k])) for k, v in m.state_dict().items() if v.is_floating_point()), key=lambda t: t[1])
    print(name, dtype, "worst state entry after one SGD step", worst)
    assert worst[1] < 1e-4, worst
    for k, v in m.state_dict().items():
        np.testing.assert_allclose(sig(v.float().cpu())[[0, 2]], g["after1." + k][[0, 2]], rtol=1e-4, err_msg=k)
    m.eval()
    with torch.no_grad():
        ev = m(x.to(DEV))
    for o, t in zip(ev if isinstance(ev, tuple) else (ev,), tags):
        logits_close(o, g["eval_" + t])


@pytest.mark.parametrize("dtype", ["fp32_mfma", "fp32_mfma_gemm", "fp32_mfma_convt"])
def test_vit_small_other_fp32_modes(dtype):
    """The three remaining compute_dtype names on vit_small_p16, at the fp32 bars: training logits, loss, gradients against the
    plain float64 step ("fp16", "fp32" and "fp32_mfma_attn" have their own tests)."""
    _need_gpu()
    import loss as L
    g, cfg, m, x, labs, _ = plain_case(GOLDEN, "vit_small_p16")
    ref = _plain64("vit_small_p16")
    L.CLASS_NUMBER = 2
    m._compute_dtype = dtype
    m.to(DEV).train()
    outs, loss = _loss(m(x.to(DEV)), [l.to(DEV) for l in labs])
    loss.backward()
    logits_close(outs[0], g["logits"])
    assert abs(loss.item() - float(g["loss0"])) < 1e-4
    worst = max(((p.grad.double().cpu() - ref["grads"][k]).norm().item() / (ref["grads"][k].norm().item() + 1e-6 / 3e-3), k)
                for k, p in m.named_parameters())
    print(dtype, "worst gradient vs plain float64", worst)
    assert worst[0] < 3e-3, worst


def test_standalone_embeddings_and_transformer_return_no_features():
    """`Embeddings.forward` / `Transformer.forward` of a pure-ViT model called on their own, as the reference's can be: tokens
    against the plain restatement (fp32: rtol 1e-4 of scale), `features` None, no attention maps."""
    _need_gpu()
    g, cfg, m, x, labs, _ = plain_case(GOLDEN, "vit_small_p16")
    sd = vit_plain.leaves(m.state_dict(), torch.float64)
    m.to(DEV).eval()
    for mod in m.modules():
        mod._compute_dtype = "fp32"
    with torch.no_grad():
        tok, feats = m.transformer.embeddings(x.to(DEV))
        enc, attn, feats2 = m.transformer(x.to(DEV))
    assert feats is None and feats2 is None and attn == []
    e = "transformer.embeddings."
    xx = x.double().repeat(1, 3, 1, 1)
    want = torch.nn.functional.conv2d(xx, sd[e + "patch_embeddings.weight"], sd[e + "patch_embeddings.bias"], stride=16)
    want = want.flatten(2).transpose(1, 2) + sd[e + "position_embeddings"]
    assert tuple(tok.shape) == (2, 16, 64)
    assert (tok.cpu().double() - want).abs().max().item() < 1e-4 * want.abs().max().item()
    want_enc = vit_plain.encode(sd, x.double(), cfg["num_heads"], 16)
    assert (enc.cpu().double() - want_enc).abs().max().item() < 1e-4 * want_enc.abs().max().item()


# ViT-L_16, eval logits after one SGD step, fp32.  No seed of this model can be screened: at each of 29 seeds (62 .. 90) the
# reference's OWN float32 run flips ReLU masks against its float64 run (largest gradient gap 9e-4 .. 1e-2; ViT-B_16 is clean at
# one seed in three, and its fixture uses such a seed).  The step turns a flip into a weight difference that the eval forward
# amplifies, so the reference's float32 eval logits lie this far from its float64 ones (tools/gen_golden_vit.py --eval-gap
# --model ViT-L_16, signature metric: norm, abs-sum, largest sample error over the sampled scale), over the 29 seeds:
#   median 4.3e-5 / 5.8e-5 / 3.4e-4, 90th percentile 2.0e-4 / 2.4e-4 / 1.1e-3, largest 3.39e-4 / 3.21e-4 / 2.12e-3.
# The hybrid's bars (2e-4, 1e-3) are therefore ones the reference itself misses against float64 at 3 of 29 seeds.  The bar here is
# the largest gap the reference showed, doubled, because fixture (the reference's float32 run) and device are two independent
# evaluation orders each that far from the exact value.  (Four times the median, 1.7e-4 / 2.3e-4, is a bar the reference's own
# float32 run misses at 7 of the 29 seeds.)  A wrong gradient moves these figures by 1e-2 and more.  DESIGN.md section 3.
VIT_L_EVAL_FP32_BAR = dict(norm=2 * 3.39e-4, abs_sum=2 * 3.21e-4, samples=2 * 2.12e-3)


def _sig_bars(s, gs, dtype, what, fp32_bar=None):
    """The signature bars of test_transunet_r50_vit_b16_224: fp32 norm and abs-sum rtol 2e-4, samples rtol 1e-3 (floor
    1e-3 |t| / 300); fp16 norm and abs-sum rtol 2e-2, samples within 6e-2 of the sampled scale.  fp32_bar: VIT_L_EVAL_FP32_BAR."""
    scale = np.abs(gs[3:]).max()
    print(what, dtype, "norm, abs-sum rel", np.abs(s[[0, 2]] / gs[[0, 2]] - 1), "samples max abs / sampled scale",
          np.abs(s[3:] - gs[3:]).max() / scale)
    if dtype == "fp32" and fp32_bar is not None:
        assert abs(s[0] / gs[0] - 1) < fp32_bar["norm"] and abs(s[2] / gs[2] - 1) < fp32_bar["abs_sum"], what
        assert np.abs(s[3:] - gs[3:]).max() < fp32_bar["samples"] * scale, what
    elif dtype == "fp32":
        np.testing.assert_allclose(s[[0, 2]], gs[[0, 2]], rtol=2e-4, err_msg=what)
        np.testing.assert_allclose(s[3:], gs[3:], rtol=1e-3, atol=1e-3 * s[0] / 300, err_msg=what)
    else:
        np.testing.assert_allclose(s[[0, 2]], gs[[0, 2]], rtol=2e-2, err_msg=what)
        assert np.abs(s[3:] - gs[3:]).max() < 6e-2 * max(scale, s[0] / 300), what


@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
@pytest.mark.parametrize("name,fixture", [("ViT-B_16", "vit_b16_224"), ("ViT-L_16", "vit_l16_224")])
def test_vit_named_224(name, fixture, dtype):
    """`CONFIGS[name]` with n_skip = 0, dropout 0.0, at 224 x 224, B = 1 (196 tokens at head dimension 64: the matrix-core
    attention in fp16) against the reference's signatures, at the bars of test_transunet_r50_vit_b16_224: logits and eval logits
    (_sig_bars; the eval logits after one SGD step, as the fixture takes it, at the same bars for ViT-B_16, whose fixture seed is screened on
    the CPU for ReLU inputs within rounding of zero, so the reference's float32 figures are the exact ones to 1e-6; ViT-L_16 has
    no such seed and takes VIT_L_EVAL_FP32_BAR), loss within 2e-5 (fp16: 5e-3), every gradient
    finite, gradient norms within 1 % (fp16: 25 %, large tensors)."""
    _need_gpu()
    import loss as L
    from TransUnet.vit_seg_modeling import VisionTransformer
    from umi import optim as uo
    g = np.load(os.path.join(GOLDEN, fixture + ".npz"))
    cfg = _named(name)
    cfg.transformer.dropout_rate = 0.0
    L.CLASS_NUMBER = 2
    m = VisionTransformer(cfg, img_size=224, num_classes=2, compute_dtype=dtype)
    assert len(m.state_dict()) == int(g["n_keys"])
    seed, cin = int(g["seed"]), int(g["cin"])
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=seed, negative_gamma=False))
    m.to(DEV).train()
    x, lab = recipe.synthetic_batch(1, cin, 224, 224, 2, seed=seed)
    opt = uo.SGD(m.parameters(), **SGD)
    logits = m(x.to(DEV))
    loss = L.calc_loss(logits, lab.to(DEV), loss_type="dice_bce_mc")
    opt.zero_grad(set_to_none=True)
    loss.backward()
    assert tuple(logits.shape) == (1, 2, 224, 224)
    print(name, dtype, "loss", loss.item(), "fixture", float(g["loss0"]))
    _sig_bars(sig(logits.cpu()), g["logits_sig"], dtype, "logits")
    assert abs(loss.item() - float(g["loss0"])) < (2e-5 if dtype == "fp32" else 5e-3)
    bad, worst = [], ("", 0.0)
    for k, p in m.named_parameters():
        ref_norm = float(g["grad_sig." + k][0])
        assert torch.isfinite(p.grad).all(), k
        if ref_norm < 1e-7 or (dtype == "fp16" and p.numel() < 4096):   # e.g. key biases: mathematically zero gradient
            continue
        e = abs(p.grad.double().norm().item() - ref_norm) / ref_norm
        worst = max(worst, (k, e), key=lambda t: t[1])
        if e > (1e-2 if dtype == "fp32" else 0.25):
            bad.append((k, p.grad.double().norm().item(), ref_norm))
    print(name, dtype, "worst gradient norm", worst)
    assert not bad, bad[:5]
    opt.step()                                                   # the fixture's eval logits follow its one SGD step
    m.eval()
    with torch.no_grad():
        ev = m(x.to(DEV))
    _sig_bars(sig(ev.cpu()), g["eval_logits_sig"], dtype, "eval logits", VIT_L_EVAL_FP32_BAR if name == "ViT-L_16" else None)


def test_vit_small_fp16_runs_close():
    """fp16 storage: logits within 3e-2 of the logit scale of the fp32 reference, finite gradients, cosine > 0.9 on the large
    tensors (the bars of test_transunet_small_fp16_runs_close)."""
    _need_gpu()
    import loss as L
    g, cfg, m, x, labs, _ = plain_case(GOLDEN, "vit_small_p16")
    ref = _plain64("vit_small_p16")
    L.CLASS_NUMBER = 2
    m._compute_dtype = "fp16"
    m.to(DEV).train()
    outs, loss = _loss(m(x.to(DEV)), [l.to(DEV) for l in labs])
    loss.backward()
    gl = torch.from_numpy(g["logits"])
    e = ((outs[0].detach().cpu() - gl).abs().max() / gl.abs().max()).item()
    print("fp16 logits error over scale", e)
    assert e < 3e-2
    for k, p in m.named_parameters():
        assert torch.isfinite(p.grad).all(), k
        rg = ref["grads"][k]
        if rg.numel() >= 4096 and rg.norm() > 1e-8:
            c = (p.grad.cpu().flatten().double() @ rg.flatten() / (p.grad.double().norm().cpu() * rg.norm())).item()
            assert c > 0.9, (k, c)


def _small(dtype, dropout=0.0, seed=7):
    from TransUnet.vit_seg_modeling import VisionTransformer
    cfg = small_config(2, 16)
    cfg["dropout_rate"] = dropout
    torch.manual_seed(seed)                                      # initial weights, and the model's dropout seed at its first forward
    m = VisionTransformer(vit_plain.product_config(cfg), img_size=64, num_classes=2, compute_dtype=dtype)
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=seed, negative_gamma=False))
    x, lab = recipe.synthetic_batch(2, 1, 64, 64, 2, seed=seed)
    return m.to(DEV).train(), x.to(DEV), lab.to(DEV)


def _step_tensors(m, x, lab, opt=None):
    import loss as L
    L.CLASS_NUMBER = 2
    logits = m(x)
    loss = L.calc_loss(logits, lab, loss_type="dice_bce_mc")
    (opt.zero_grad if opt is not None else m.zero_grad)(set_to_none=True)
    loss.backward()
    out = {"logits": logits.detach().clone(), "loss": loss.detach().clone()}
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        out["grad." + k] = p.grad.detach().clone()
    if opt is not None:
        opt.step()
        out.update({"param." + k: p.detach().clone() for k, p in m.named_parameters()})
    return out


def _same_bits(a, b, what):
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), f"{what}: {k} differs ({(a[k] != b[k]).sum().item()} of {a[k].numel()} elements)"


@pytest.mark.parametrize("dtype", ["fp16", "fp32"])
def test_grad_reducer_sink_equals_plain_step(dtype):
    """The training step under a GradReducer sink (gradients written into bucket slots, the patch weight's through the grouped
    launches) equals the step without it bit for bit, as the hybrid's does (test_grad_reducer_sink_path_matches_plain_backward_
    transunet), and .grad is the slot.  One exception, which the hybrid shares (its encoder is the same code): under a sink the
    query / key / value bias gradients are three column sums over the slices of the fused gradient, without one they are one
    column sum 3 C wide, and the two launches add the M = B * tokens = 32 rows in different orders.  Those three may differ by the
    rounding of a 32-term fp32 sum: 2 M * 2^-24 of the largest of the layer's three bias gradients (measured: one ulp, 5e-8 of
    it, in about one bias per model and seed; the hybrid with seeded weights shows the same at one seed of eight)."""
    _need_gpu()
    from umi import ddp
    m, x, lab = _small(dtype)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    plain = _step_tensors(m, x, lab)
    m.zero_grad(set_to_none=True)
    m.load_state_dict(sd)
    red = ddp.GradReducer(m, world_size=1, bucket_mb=0.05)
    assert len(red.buckets) > 1
    import loss as L
    loss = L.calc_loss(m(x), lab, loss_type="dice_bce_mc")
    loss.backward()
    red.sync()
    assert torch.equal(loss.detach(), plain["loss"])
    grads = dict(m.named_parameters())
    rows = x.shape[0] * m.transformer.embeddings.position_embeddings.shape[1]
    for k, p in grads.items():
        assert p.grad.data_ptr() == red.buffer_for(p).data_ptr(), k
        assert p.grad.shape == p.shape, k
        if k.endswith(("attn.query.bias", "attn.key.bias", "attn.value.bias")):
            layer = k.rsplit(".", 2)[0]
            scale = max(plain[f"grad.{layer}.{n}.bias"].abs().max().item() for n in ("query", "key", "value"))
            assert (p.grad - plain["grad." + k]).abs().max().item() <= 2 * rows * 2.0 ** -24 * scale, k
        else:
            assert torch.equal(p.grad, plain["grad." + k]), k


def test_default_dropout_training_step_is_finite_and_reproducible():
    """Dropout 0.1 (the configs' default), training mode, fp16 (the fused linear + dropout epilogues): finite, and two models
    built from the same seed give identical bits."""
    _need_gpu()
    from umi import optim as uo
    runs = []
    for _ in range(2):
        m, x, lab = _small("fp16", dropout=0.1, seed=11)
        assert m.transformer.embeddings.dropout.p == 0.1
        runs.append(_step_tensors(m, x, lab, uo.SGD(m.parameters(), **SGD)))
    _same_bits(runs[0], runs[1], "two models from one seed")
    assert all(torch.isfinite(t).all() for t in runs[0].values())
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(x), m(x))                           # dropout is off in eval mode


def test_wrong_input_size_raises_and_launches_nothing(monkeypatch):
    _need_gpu()
    from umi import lib
    m, x, _ = _small("fp16")
    calls = []
    real = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    with pytest.raises(ValueError, match=r"96x96 input has 36 patches of 16x16.*16 tokens"):
        m(torch.zeros(2, 1, 96, 96, device=DEV))
    with pytest.raises(ValueError, match=r"8 patches"):
        m.transformer(torch.zeros(2, 3, 64, 32, device=DEV))
    assert calls == []
    m(x)
    assert "umi_patch_rows" in calls                             # (the counter does see the launches of a good call)


# ---- child-process cases ------------------------------------------------------------------------------------------------------
def _child_graph():
    """vit_small_p16's weights, fp16: (a) forward + loss + backward captured by umi.graphs.GraphedStep and replayed twice equals
    the eager step bit for bit, and the two replays equal each other; (b) the whole training step (with the fused SGD) through
    GraphedStep(warmup=1) + 2 replays follows three eager steps bit for bit."""
    import copy
    import loss as L
    from umi import optim as uo
    from umi.graphs import GraphedStep
    L.CLASS_NUMBER = 2
    master, x, lab = _small("fp16")
    # (a)
    m_e, m_g = copy.deepcopy(master), copy.deepcopy(master)
    eager = _step_tensors(m_e, x, lab)

    def fwd_bwd(xx, ll):
        loss = L.calc_loss(m_g(xx), ll, loss_type="dice_bce_mc")
        m_g.zero_grad(set_to_none=True)
        loss.backward()
        return loss.detach()
    gs = GraphedStep(fwd_bwd, [x, lab], warmup=1)
    reps = []
    for _ in range(2):
        loss = gs(x, lab).clone()
        reps.append(dict({"loss": loss}, **{"grad." + k: p.grad.detach().clone() for k, p in m_g.named_parameters()}))
    _same_bits(reps[0], reps[1], "two replays")
    _same_bits({k: eager[k] for k in reps[0]}, reps[0], "eager against replay")
    # (b)
    m_e, m_g = copy.deepcopy(master), copy.deepcopy(master)
    opt_e, opt_g = uo.SGD(m_e.parameters(), **SGD), uo.SGD(m_g.parameters(), **SGD)

    def step(xx, ll):
        loss = L.calc_loss(m_g(xx), ll, loss_type="dice_bce_mc")
        opt_g.zero_grad(set_to_none=True)
        loss.backward()
        opt_g.step()
        return loss.detach()
    gs = GraphedStep(step, [x, lab], warmup=1)
    _step_tensors(m_e, x, lab, opt_e)
    for i in range(2):
        lg = gs(x, lab).clone()
        le = _step_tensors(m_e, x, lab, opt_e)["loss"]
        assert torch.equal(lg, le), (i, float(lg), float(le))
    for (k, pg), pe in zip(m_g.named_parameters(), m_e.parameters()):
        assert torch.equal(pg, pe) and torch.isfinite(pg).all(), k
    print("VIT_GRAPH_OK", float(lg))


def _child_trace():
    """One ViT-B_16 fp16 training step at 224 x 224, B = 1; the parent reads the library's UMI_TRACE_GENERIC lines from stderr."""
    import loss as L
    from TransUnet.vit_seg_modeling import VisionTransformer
    L.CLASS_NUMBER = 2
    torch.manual_seed(5)
    m = VisionTransformer(_named("ViT-B_16"), img_size=224, num_classes=2, compute_dtype="fp16").to(DEV).train()
    x, lab = recipe.synthetic_batch(1, 3, 224, 224, 2, seed=5)
    loss = L.calc_loss(m(x.to(DEV)), lab.to(DEV), loss_type="dice_bce_mc")
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in m.parameters())
    print("VIT_TRACE_OK", float(loss))


def _run_child(mode, env=None):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), mode], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, **(env or {})))
    return r


def test_graphed_step_equals_eager_and_replays_agree():
    _need_gpu()
    r = _run_child("graph")
    assert r.returncode == 0 and "VIT_GRAPH_OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])


def test_patch_gemm_runs_on_the_matrix_cores_in_fp16():
    """Under UMI_TRACE_GENERIC=1 a ViT-B_16 fp16 step reports no pointwise call with 768 input channels on the generic kernels:
    the patch GEMM (K = 3 * 16 * 16 = 768 -> 768, 196 rows), its weight gradient, and with them every linear of the encoder."""
    _need_gpu()
    r = _run_child("trace", {"UMI_TRACE_GENERIC": "1"})
    assert r.returncode == 0 and "VIT_TRACE_OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    lines = [l for l in r.stderr.splitlines() if "[umi generic" in l]
    print("\n".join(sorted(set(lines))))
    patch = [l for l in lines if " R=1 " in l and (" Ci=768 " in l or " Co=768 " in l)]
    assert not patch, patch[:8]


if __name__ == "__main__":
    {"graph": _child_graph, "trace": _child_trace}[sys.argv[1]]()
