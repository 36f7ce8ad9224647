"""A training step's results do not depend on what its memory held before.

The tapes (umi/graph.py, umi/graph_tu.py) allocate every activation, gradient, mask and partial-sum tensor with torch.empty,
share one scratch buffer (ops.workspace) between all layers and, under a GradReducer, write into long-lived bucket slots.  A
whole-model test normally runs on whatever the caching allocator hands back -- very often last step's correct values of the
same role -- so a read of something nobody wrote this step (a pad row of a concat buffer, the odd tail of a pooled gradient,
a partial row past `rows`, a gradient slot no launch filled, an accumulate target never seeded) passes and is "deterministic".

Here every case is built three times from one state_dict and one torch.manual_seed (a fresh model per run: BatchNorm
statistics, dropout seed and device counter start equal) and runs the same steps on the same batch with every such byte
preset (tests/poison.py): runs A0 and A1 to 0x00, run B to 0xFF (NaN in fp16 / fp32, 255 in masks, -1 in integers).
  * A0 == A1 bit for bit (otherwise the step is not deterministic -- a different bug);
  * A0 == B bit for bit (otherwise something read memory nobody wrote this step);
  * everything in B is finite.
No tolerance anywhere.  Compared: logits and loss of every step, every parameter gradient of every step, every parameter,
momentum buffer and module buffer at the end.  Outside the reach of the method: the library's static reduction scratch
(`g_red_scratch`), which Python cannot fill."""
import contextlib
import copy
import os
import subprocess
import sys

import pytest
import torch

if __name__ == "__main__":                                   # the HIP-graph case runs this file as a child process
    _REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_REPO, os.path.join(_REPO, "unet-torch_amd")]

from oracle import recipe, ref_transunet
from tests import poison

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 70

# model: (class, constructor arguments); dropout = the U-Net family's fifth constructor argument
#   mode "train": `steps` x (forward, loss, backward, optimizer step); "eval": `steps` eval-mode forwards under no_grad
#   reducer: GradReducer(world_size=1, **reducer) whose buckets are poisoned before every backward
CASES = {
    # all MFMA tile forms and every fused backward (premise asserted below)
    "unet64_fp16_64x64": dict(model=("UNet", 1, 2, 64), dtype="fp16", shape=(2, 1, 64, 64),
                              nonnull=("conv_dgrad_bnred", "pool2_bwd_bnred", "conv_gather_bnred", "head_dgrad_bnred",
                                       "convT_wgrad_bias")),
    # odd pools 35x45, 17x22; a pad at three decoder levels
    "unet64_fp16_70x90": dict(model=("UNet", 1, 2, 64), dtype="fp16", shape=(2, 1, 70, 90),
                              nonnull=("pool2_bwd_bnred",), null=("pool2_bwd_bnred",)),
    # batch 1, stem cin = 3, dropout masks, odd 11x18 -> 5x9
    "unet64_rgb_dropout_fp16_44x72": dict(model=("UNet", 3, 4, 64), dropout=True, dtype="fp16", shape=(1, 3, 44, 72)),
    # every bucket slot must be rewritten by the step
    "unet64_fp16_70x90_reducer": dict(model=("UNet", 1, 2, 64), dtype="fp16", shape=(2, 1, 70, 90),
                                      reducer=dict(bucket_mb=0.5)),
    # copy_into, two decoders on one skip
    "multitask64_fp16_70x90": dict(model=("UNet_multitask", 1, 2, 64), dtype="fp16", shape=(2, 1, 70, 90)),
    # gates, CONV_ACCUMULATE into an existing gradient, bias_cancelled
    "attention64_fp16_64x64": dict(model=("UNet_attention", 1, 2, 64), dtype="fp16", shape=(2, 1, 64, 64)),
    # the generic kernels incl. the odd-tail pool
    "unet8_rgb_fp32_33x47": dict(model=("UNet", 3, 4, 8), dtype="fp32", shape=(3, 3, 33, 47)),
    # the fp32 matrix-core trio
    "unet64_fp32_mfma_32x48": dict(model=("UNet", 1, 2, 64), dtype="fp32_mfma", shape=(2, 1, 32, 48)),
    # the pointwise fp32 path
    "attention32_fp32_mfma_gemm_32x32": dict(model=("UNet_attention", 1, 2, 32), dtype="fp32_mfma_gemm", shape=(2, 1, 32, 32)),
    # TUTape: grouped end-of-backward launches, GroupNorm / LayerNorm partial rows, weight standardisation
    "transunet_small_fp16": dict(model=("TransUNet", "small", 64), dtype="fp16", shape=(2, 1, 64, 64)),
    "transunet_small_fp32": dict(model=("TransUNet", "small", 64), dtype="fp32", shape=(2, 1, 64, 64)),
    # the slots of the grouped launches
    "transunet_small_fp16_reducer": dict(model=("TransUNet", "small", 64), dtype="fp16", shape=(2, 1, 64, 64), reducer={}),
    # MFMA attention, the 55 -> 56 skip pad, the fp32 attention kernels: one step, no optimizer
    "transunet_r50_b16_224_fp16": dict(model=("TransUNet", "r50", 224), dtype="fp16", shape=(1, 1, 224, 224), steps=1,
                                       optimizer=False),
    "transunet_r50_b16_224_fp32_mfma_attn": dict(model=("TransUNet", "r50", 224), dtype="fp32_mfma_attn",
                                                 shape=(1, 1, 224, 224), steps=1, optimizer=False),
    # the inference tape (BatchNorm fold, activated stores)
    "unet64_fp16_70x90_eval": dict(model=("UNet", 1, 2, 64), dtype="fp16", shape=(2, 1, 70, 90), mode="eval"),
}
GRAPH_CASE = dict(model=("UNet", 1, 2, 64), dtype="fp16", shape=(2, 1, 64, 64))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: torch.cuda.is_available() is False")


def _ncls(case):
    return 2 if case["model"][0] == "TransUNet" else case["model"][2]


def _master(case):
    """The case's network on the CPU with seeded weights; never run, every run deep-copies it."""
    kind = case["model"][0]
    torch.manual_seed(SEED)
    if kind == "TransUNet":
        from tests.test_gpu_transunet import product_config
        from TransUnet.vit_seg_modeling import VisionTransformer
        _, size, img = case["model"]
        cfg = ref_transunet.small_config(2) if size == "small" else ref_transunet.r50_vit_b16_config(2, 3, dropout_rate=0.0)
        m = VisionTransformer(product_config(cfg, img), img_size=img, num_classes=2, compute_dtype=case["dtype"])
        m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=SEED, negative_gamma=False))
    else:
        import Model
        _, cin, ncls, feat = case["model"]
        m = getattr(Model, kind)(cin, ncls, feat, False, case.get("dropout", False), compute_dtype=case["dtype"])
        m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=SEED))
    return m


def _batch(case):
    B, C, H, W = case["shape"]
    x, lab = recipe.synthetic_batch(B, C, H, W, _ncls(case), seed=SEED)
    labs = [lab]
    if case["model"][0] == "UNet_multitask":
        labs.append(recipe.synthetic_batch(B, C, H, W, _ncls(case), seed=SEED + 100)[1])
    return x.to(DEV), [l.to(DEV) for l in labs]


def _loss(out, labs):
    """dice_bce_mc as each variant's parity test forms it: summed over both heads for the multitask network."""
    import loss as L
    outs = out if isinstance(out, (tuple, list)) else (out,)
    total = None
    for o, lab in zip(outs, labs):
        l = L.calc_loss(o, lab, loss_type="dice_bce_mc")
        total = l if total is None else total + l
    return outs, total


@contextlib.contextmanager
def _counting(names):
    """Wrap umi.ops functions and record what they return (the tape calls them as ops.NAME)."""
    from umi import ops
    seen = {n: [] for n in names}
    real = {n: getattr(ops, n) for n in names}

    def wrap(n):
        def f(*a, **k):
            r = real[n](*a, **k)
            seen[n].append(r is not None and r is not False)
            return r
        return f
    try:
        for n in names:
            setattr(ops, n, wrap(n))
        yield seen
    finally:
        for n in names:
            setattr(ops, n, real[n])


def _snap(out, prefix, named):
    for k, t in named:
        out[prefix + k] = t.detach().clone()


def _end_state(out, m, opt):
    _snap(out, "param.", m.named_parameters())
    _snap(out, "buffer.", m.named_buffers())
    if opt is not None:
        for k, p in m.named_parameters():
            buf = opt.state.get(p, {}).get("momentum_buffer")
            assert buf is not None, k
            out["momentum." + k] = buf.detach().clone()


def _run(case, master, x, labs, byte, steps=None):
    """One run of the case under poisoned(byte) on a fresh copy of `master`: name -> tensor, in a fixed order."""
    import loss as L
    from umi import ddp, optim as uo
    L.CLASS_NUMBER = _ncls(case)
    steps = steps or case.get("steps", 2)
    out = {}
    torch.manual_seed(SEED)                                  # the model's dropout seed is drawn from this stream
    with poison.poisoned(byte):
        m = copy.deepcopy(master).to(DEV)
        if case.get("mode") == "eval":
            m.eval()
            with torch.no_grad():
                for s in range(steps):
                    outs = m(x)
                    _snap(out, f"step{s}.logits", _heads(outs))
            _end_state(out, m, None)
            torch.cuda.synchronize()
            return out
        m.train()
        red = ddp.GradReducer(m, world_size=1, **case["reducer"]) if "reducer" in case else None
        if red is not None and "bucket_mb" in case["reducer"]:
            assert len(red.buckets) > 1
        opt = uo.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4) if case.get("optimizer", True) else None
        for s in range(steps):
            outs, loss = _loss(m(x), labs)
            if opt is not None:
                opt.zero_grad(set_to_none=True)
            if red is not None:
                poison.poison_buckets(red, byte)
            loss.backward()
            if red is not None:
                red.sync()
                assert all(p.grad.data_ptr() == red.buffer_for(p).data_ptr() for p in m.parameters())
            _snap(out, f"step{s}.logits", _heads(outs))
            out[f"step{s}.loss"] = loss.detach().clone()
            for k, p in m.named_parameters():
                assert p.grad is not None, k
                out[f"step{s}.grad.{k}"] = p.grad.detach().clone()
            if opt is not None:
                opt.step()
        _end_state(out, m, opt)
    torch.cuda.synchronize()
    return out


def _heads(outs):
    outs = outs if isinstance(outs, (tuple, list)) else (outs,)
    return [(str(i), o) for i, o in enumerate(outs)]


def _bits(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def _first_difference(a, b):
    """None when the two runs are bit-identical, else a description of the first differing tensor and its first index."""
    assert list(a) == list(b), "the two runs collected different tensors"
    for k in a:
        ta, tb = a[k], b[k]
        if ta.shape != tb.shape or ta.dtype != tb.dtype:
            return f"{k}: {tuple(ta.shape)} {ta.dtype} against {tuple(tb.shape)} {tb.dtype}"
        ne = _bits(ta) != _bits(tb)
        if bool(ne.any()):
            flat = int(ne.nonzero()[0]) // ta.element_size()
            idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ta.shape)) if ta.dim() else ()
            n = int((ta.reshape(-1) != tb.reshape(-1)).sum())
            return (f"{k}{list(idx)}: {ta.reshape(-1)[flat].item()!r} against {tb.reshape(-1)[flat].item()!r} "
                    f"({n} of {ta.numel()} elements differ)")
    return None


def _assert_finite(run):
    bad = [k for k, t in run.items() if t.is_floating_point() and not bool(torch.isfinite(t).all())]
    assert not bad, f"non-finite values under poisoned(0xFF) in {bad[:6]} ({len(bad)} tensors)"


def _check_invariance(a0, a1, b):
    d = _first_difference(a0, a1)
    assert d is None, "not deterministic: two runs on zero-filled memory differ at " + d
    d = _first_difference(a0, b)
    assert d is None, "reads memory nobody wrote this step: zero-filled against 0xFF-filled runs differ at " + d
    _assert_finite(b)


@pytest.mark.parametrize("name", list(CASES))
def test_step_is_invariant_to_prior_memory_contents(name):
    _need_gpu()
    case = CASES[name]
    master = _master(case)
    x, labs = _batch(case)
    watch = tuple(dict.fromkeys(case.get("nonnull", ()) + case.get("null", ())))
    with _counting(watch) as seen:
        a0 = _run(case, master, x, labs, 0x00)
    # premise: the paths the case is there for really ran (counted by what the ops functions returned, not by kernel names)
    for n in case.get("nonnull", ()):
        assert any(seen[n]), f"ops.{n} never took the fused path in this case: {seen[n]}"
    for n in case.get("null", ()):
        assert not all(seen[n]), f"ops.{n} never declined in this case: {seen[n]}"
    assert len(a0) > 4 and all(t.is_cuda for t in a0.values())
    a1 = _run(case, master, x, labs, 0x00)
    b = _run(case, master, x, labs, 0xFF)
    _check_invariance(a0, a1, b)


def _graphed_run(case, master, x, labs, byte, replays):
    """GraphedStep(forward + loss + backward + optimizer step, warmup=1) captured and replayed under poisoned(byte): the fill
    kernels are captured with the step, so every replay starts from poisoned memory again."""
    import loss as L
    from umi import optim as uo
    from umi.graphs import GraphedStep
    L.CLASS_NUMBER = _ncls(case)
    out = {}
    torch.manual_seed(SEED)
    with poison.poisoned(byte):
        m = copy.deepcopy(master).to(DEV).train()
        opt = uo.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)

        def step(xx, *ll):
            outs, loss = _loss(m(xx), ll)
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            return outs[0].detach(), loss.detach()
        gs = GraphedStep(step, [x] + labs, warmup=1)
        for s in range(1, 1 + replays):
            logits, loss = gs(x, *labs)
            out[f"step{s}.logits0"] = logits.clone()
            out[f"step{s}.loss"] = loss.clone()
            _snap(out, f"step{s}.grad.", ((k, p.grad) for k, p in m.named_parameters()))
        _end_state(out, m, opt)
    torch.cuda.synchronize()
    return out


def _graph_child():
    """Child-process body of test_graphed_step_is_invariant_to_prior_memory_contents (stream capture is sensitive to what ran
    before it in the process).  The eager run A0 does three steps: the GraphedStep's warm-up step and its two replays."""
    case = GRAPH_CASE
    master = _master(case)
    x, labs = _batch(case)
    a0 = _run(case, master, x, labs, 0x00, steps=3)
    b = _graphed_run(case, master, x, labs, 0xFF, replays=2)
    assert [k for k in b if k.startswith("step1")] and "step2.loss" in b
    a0 = {k: a0[k] for k in b}                               # (the warm-up step's own tensors are not visible from outside)
    d = _first_difference(a0, b)
    assert d is None, "graph replays on 0xFF-filled memory differ from the eager run on zero-filled memory at " + d
    _assert_finite(b)
    print("POISONED_GRAPH_OK", len(b), float(b["step2.loss"]))


def test_graphed_step_is_invariant_to_prior_memory_contents():
    """UNet(1,2,64) fp16 through umi.graphs.GraphedStep, captured and replayed twice on 0xFF-filled memory, against the eager
    run of the same steps on zero-filled memory: logits, loss and gradients of both replays, parameters, momentum and
    BatchNorm buffers at the end, bit for bit and finite."""
    _need_gpu()
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "POISONED_GRAPH_OK" in r.stdout, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])


if __name__ == "__main__":
    _graph_child()
