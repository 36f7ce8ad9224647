"""TransUNet (R50-ViT hybrid) on the HIP path vs fixtures of the reference itself and vs the CPU oracle.

Config objects: product `TransUnet.vit_seg_configs.ConfigDict` built from the oracle's plain dict, so both sides
describe the same network.  Dropout is 0.0 in the parity configs."""
import os

import numpy as np
import pytest
import torch

from oracle import recipe, ref_transunet, ref_unet
from tests.test_oracle_golden import _sig_close, sig

DEV = "cuda"


def product_config(cfg, img):
    from TransUnet.vit_seg_configs import ConfigDict
    g = img // 16
    return ConfigDict(patches={"size": (16, 16), "grid": (g, g)}, hidden_size=cfg["hidden_size"],
                      transformer=dict(mlp_dim=cfg["mlp_dim"], num_heads=cfg["num_heads"], num_layers=cfg["num_layers"],
                                       attention_dropout_rate=cfg["attention_dropout_rate"], dropout_rate=cfg["dropout_rate"]),
                      classifier="seg", representation_size=None, decoder_channels=tuple(cfg["decoder_channels"]),
                      n_classes=cfg["n_classes"], activation="softmax",
                      resnet=dict(num_layers=tuple(cfg["resnet_layers"]), width_factor=cfg["width_factor"]),
                      skip_channels=list(cfg["skip_channels"]), n_skip=cfg["n_skip"])


def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


@pytest.mark.parametrize("tag,old_grid", [("zoom", 3), ("drop_cls", 4)])
def test_load_from_matches_reference(golden_dir, tag, old_grid):
    """CPU (host logic): `VisionTransformer.load_from` -> `Block.load_from` -> `PreActBottleneck.load_from` (reference
    vit_seg_modeling.py:189-224,394-441, vit_seg_modeling_resnet_skip.py:76-110) on a synthetic JAX-keyed checkpoint
    (oracle/recipe.py: HWIO kernels, [hidden, heads, head_dim] attention kernels, class-token position embedding) against
    the state_dict the REFERENCE's load_from produces from the same arrays (fixture), for both position-embedding paths
    (3 x 3 grid resized to 4 x 4 with ndimage.zoom; 4 x 4 grid with the class token dropped)."""
    from TransUnet.vit_seg_modeling import VisionTransformer
    g = np.load(os.path.join(golden_dir, "transunet_small_load_from.npz"))
    cfg = ref_transunet.small_config(2)
    torch.manual_seed(0)
    m = VisionTransformer(product_config(cfg, 64), img_size=64, num_classes=2)
    w = recipe.synthetic_jax_checkpoint(m, cfg["hidden_size"], cfg["num_heads"], old_grid, seed=77)
    assert len(w) == int(g[tag + ".n_ckpt_keys"])
    before = {k: v.clone() for k, v in m.state_dict().items()}
    m.load_from(w)
    changed = [k for k, v in m.state_dict().items() if not torch.equal(v, before[k])]
    assert changed == g[tag + ".changed"].tolist()              # exactly the tensors the reference overwrites
    for k, v in m.state_dict().items():
        np.testing.assert_allclose(sig(v.float()), g[f"{tag}.sig." + k], rtol=1e-6, atol=1e-7, err_msg=k)


def test_product_transunet_surface_and_init(golden_dir):
    """CPU: constructor, key set/order and init RNG stream equal the reference's (fixture `keys`, `init_sig.*`)."""
    from TransUnet.vit_seg_modeling import CONFIGS, VisionTransformer
    g = np.load(os.path.join(golden_dir, "transunet_small.npz"))
    cfg = ref_transunet.small_config(2)
    torch.manual_seed(0)
    m = VisionTransformer(product_config(cfg, 64), img_size=64, num_classes=2)
    assert list(m.state_dict().keys()) == g["keys"].tolist()
    if "init_sig." + g["keys"][0] in g:
        for k, v in m.state_dict().items():
            _sig_close(sig(v.float()), g["init_sig." + k], rtol=1e-6)
    assert CONFIGS["R50-ViT-B_16"].n_skip == 3 and CONFIGS["R50-ViT-B_16"].patches.grid == (16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 1, 64, 64))


@pytest.mark.gpu
@pytest.mark.parametrize("name,ncls", [("transunet_small", 2), ("transunet_small_rgb4", 4), ("transunet_small_neg_gamma", 2)])
def test_transunet_small_fp32_parity(golden_dir, name, ncls):
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    import loss as L
    from TransUnet.vit_seg_modeling import VisionTransformer
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    cfg = ref_transunet.small_config(ncls)
    img, B, cin, seed = int(g["img"]), int(g["B"]), int(g["cin"]), int(g["seed"])
    ref = ref_transunet.RefTransUNet(cfg, img)
    neg = bool(int(g["neg_gamma"])) if "neg_gamma" in g else False      # every 7th norm scale negative (oracle/recipe.py)
    ref.load_state_dict(recipe.fill_state_dict(ref.state_dict(), seed=seed, negative_gamma=neg))
    x, lab = recipe.synthetic_batch(B, cin, img, img, ncls, seed=seed)
    L.CLASS_NUMBER = ncls
    m = VisionTransformer(product_config(cfg, img), img_size=img, num_classes=ncls, compute_dtype="fp32")
    m.load_state_dict(ref.state_dict())
    m.to(DEV).train()
    logits = m(x.to(DEV))
    loss = L.calc_loss(logits, lab.to(DEV), loss_type="dice_bce_mc")
    loss.backward()
    gl = g["logits"]
    np.testing.assert_allclose(logits.detach().cpu().numpy(), gl, rtol=1e-4, atol=1e-4 * float(np.abs(gl).max()))
    assert abs(loss.item() - float(g["loss0"])) < 2e-5
    ref.train()
    rl = ref_unet.dice_bce_mc(ref(x), lab, ncls)
    rl.backward()
    worst = ("", 0.0)
    for (k, p), (_, rp) in zip(m.named_parameters(), ref.named_parameters()):
        assert p.grad is not None, k
        # key biases have a mathematically zero gradient (softmax is shift invariant): absolute floor 1e-6
        e = (p.grad.detach().double().cpu() - rp.grad.double()).norm().item() / (rp.grad.double().norm().item() + 1e-6 / 3e-3)
        worst = max(worst, (k, e), key=lambda t: t[1])
    assert worst[1] < 3e-3, worst
    # BatchNorm running stats after one step, eval-mode forward
    for k, v in m.state_dict().items():
        if "running" in k:
            assert rel_err(v, ref.state_dict()[k]) < 1e-4, k
    m.eval()
    ref.eval()
    with torch.no_grad():
        ev, rev = m(x.to(DEV)), ref(x)
    assert ((ev.cpu() - rev).abs().max() / rev.abs().max()).item() < 2e-4


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_transunet_r50_vit_b16_224(golden_dir, dtype):
    """Full R50-ViT-B/16 @224 (BASELINE configs[3] shape, B=1: 196 tokens, the 55 -> 56 skip pad): logits signature, loss and
    per-parameter grad norms vs the reference.  fp16 storage (the matrix-core kernels): sampled logits within 6e-2 of scale
    (3e-2 at 512 x 512), loss within 5e-3, gradient norms of the large tensors within 25 %."""
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    import loss as L
    from TransUnet.vit_seg_modeling import VisionTransformer
    g = np.load(os.path.join(golden_dir, "transunet_r50_b16_224.npz"))
    cfg = ref_transunet.r50_vit_b16_config(2, 3, dropout_rate=0.0)
    L.CLASS_NUMBER = 2
    m = VisionTransformer(product_config(cfg, 224), img_size=224, num_classes=2, compute_dtype=dtype)
    assert len(m.state_dict()) == 409
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=int(g["seed"]), negative_gamma=False))
    m.to(DEV).train()
    x, lab = recipe.synthetic_batch(1, 1, 224, 224, 2, seed=int(g["seed"]))
    logits = m(x.to(DEV))
    loss = L.calc_loss(logits, lab.to(DEV), loss_type="dice_bce_mc")
    loss.backward()
    s = sig(logits.cpu())
    if dtype == "fp32":
        np.testing.assert_allclose(s[[0, 2]], g["logits_sig"][[0, 2]], rtol=2e-4)
        np.testing.assert_allclose(s[3:], g["logits_sig"][3:], rtol=1e-3, atol=1e-3 * s[0] / 300)
        assert abs(loss.item() - float(g["loss0"])) < 2e-5
    else:
        scale = np.abs(g["logits_sig"][3:]).max()
        np.testing.assert_allclose(s[[0, 2]], g["logits_sig"][[0, 2]], rtol=2e-2)
        # 16 sampled logits: measured 4.6e-2 of the sampled scale here against < 3e-2 at 512 x 512 (B = 1: the decoder's
        # BatchNorm statistics and the 14 x 14 token grid average fp16 rounding over ~5x fewer values than at 512 x 512)
        assert np.abs(s[3:] - g["logits_sig"][3:]).max() < 6e-2 * max(scale, s[0] / 300)
        assert abs(loss.item() - float(g["loss0"])) < 5e-3
    bad = []
    for k, p in m.named_parameters():
        ref_norm = float(g["grad_sig." + k][0])
        assert torch.isfinite(p.grad).all(), k
        if ref_norm < 1e-7 or (dtype == "fp16" and p.numel() < 4096):   # e.g. key biases: mathematically zero gradient
            continue
        tol = 1e-2 if dtype == "fp32" else 0.25
        if abs(p.grad.double().norm().item() - ref_norm) > tol * ref_norm:
            bad.append((k, p.grad.double().norm().item(), ref_norm))
    assert not bad, bad[:5]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["fp32", "fp16"])
def test_transunet_r50_vit_b16_512(golden_dir, dtype):
    """BASELINE configs[4] shape: R50-ViT-B/16 at 512 x 512, B = 1 -- 1,024 tokens through the MFMA attention (fp16) and the
    ResNet's odd-size skip (127 x 127 zero-padded to 128 x 128, reference vit_seg_modeling_resnet_skip.py:142-160) --
    against the reference's own outputs (fixture: logits signature, loss, per-parameter gradient norms).
    fp32: the bars of the 224 case.  fp16 storage: logits within 3e-2 of scale, loss within 5e-3, gradient norms of the
    large tensors within 25 % (masks flip under fp16 rounding; cosine is checked on the miniature config)."""
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    import loss as L
    from TransUnet.vit_seg_modeling import VisionTransformer
    g = np.load(os.path.join(golden_dir, "transunet_r50_b16_512.npz"))
    cfg = ref_transunet.r50_vit_b16_config(2, 3, dropout_rate=0.0)
    L.CLASS_NUMBER = 2
    m = VisionTransformer(product_config(cfg, 512), img_size=512, num_classes=2, compute_dtype=dtype)
    assert len(m.state_dict()) == 409 and m.state_dict()["transformer.embeddings.position_embeddings"].shape[1] == 1024
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=int(g["seed"]), negative_gamma=False))
    m.to(DEV).train()
    x, lab = recipe.synthetic_batch(1, 1, 512, 512, 2, seed=int(g["seed"]))
    logits = m(x.to(DEV))
    loss = L.calc_loss(logits, lab.to(DEV), loss_type="dice_bce_mc")
    loss.backward()
    assert tuple(logits.shape) == (1, 2, 512, 512)
    s = sig(logits.cpu())
    if dtype == "fp32":
        np.testing.assert_allclose(s[[0, 2]], g["logits_sig"][[0, 2]], rtol=2e-4)
        np.testing.assert_allclose(s[3:], g["logits_sig"][3:], rtol=1e-3, atol=1e-3 * s[0] / 300)
        assert abs(loss.item() - float(g["loss0"])) < 2e-5
    else:
        scale = np.abs(g["logits_sig"][3:]).max()
        np.testing.assert_allclose(s[[0, 2]], g["logits_sig"][[0, 2]], rtol=2e-2)
        assert np.abs(s[3:] - g["logits_sig"][3:]).max() < 3e-2 * max(scale, s[0] / 700)
        assert abs(loss.item() - float(g["loss0"])) < 5e-3
    bad = []
    for k, p in m.named_parameters():
        ref_norm = float(g["grad_sig." + k][0])
        assert torch.isfinite(p.grad).all(), k
        if ref_norm < 1e-7 or (dtype == "fp16" and p.numel() < 4096):
            continue
        tol = 1e-2 if dtype == "fp32" else 0.25
        if abs(p.grad.double().norm().item() - ref_norm) > tol * ref_norm:
            bad.append((k, p.grad.double().norm().item(), ref_norm))
    assert not bad, bad[:5]


@pytest.mark.gpu
def test_transunet_small_fp16_runs_close(golden_dir):
    """fp16 storage: logits within 3e-2 of logit scale of the fp32 reference, finite grads, cosine > 0.9 on big tensors."""
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    import loss as L
    from TransUnet.vit_seg_modeling import VisionTransformer
    g = np.load(os.path.join(golden_dir, "transunet_small.npz"))
    cfg = ref_transunet.small_config(2)
    ref = ref_transunet.RefTransUNet(cfg, 64)
    ref.load_state_dict(recipe.fill_state_dict(ref.state_dict(), seed=int(g["seed"]), negative_gamma=False))
    x, lab = recipe.synthetic_batch(2, 1, 64, 64, 2, seed=int(g["seed"]))
    L.CLASS_NUMBER = 2
    m = VisionTransformer(product_config(cfg, 64), img_size=64, num_classes=2, compute_dtype="fp16")
    m.load_state_dict(ref.state_dict())
    m.to(DEV).train()
    logits = m(x.to(DEV))
    L.calc_loss(logits, lab.to(DEV), loss_type="dice_bce_mc").backward()
    gl = torch.from_numpy(g["logits"])
    assert ((logits.detach().cpu() - gl).abs().max() / gl.abs().max()).item() < 3e-2
    ref.train()
    ref_unet.dice_bce_mc(ref(x), lab, 2).backward()
    for (k, p), (_, rp) in zip(m.named_parameters(), ref.named_parameters()):
        assert torch.isfinite(p.grad).all(), k
        if rp.numel() >= 4096 and rp.grad.norm() > 1e-8:
            c = (p.grad.cpu().flatten().double() @ rp.grad.flatten().double() / (p.grad.norm().cpu().double() * rp.grad.norm().double())).item()
            assert c > 0.9, (k, c)


@pytest.mark.gpu
@pytest.mark.parametrize("name,pcls,rcls", [
    ("transunet_small_multitask", "VisionTransformerMultitask", "RefTransUNetMultitask"),
    ("transunet_small_multitask_em", "VisionTransformerMultitaskEM", "RefTransUNetMultitaskEM")])
def test_transunet_multitask_fp32_parity(golden_dir, name, pcls, rcls):
    """the multitask TransUNets (one encoder, 2 / 6 decoders on one tape) against the REFERENCE's logits
    of every head (fixture) and the oracle's gradients (encoder gradients = sum over the decoders)."""
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    import loss as L
    from TransUnet import vit_seg_modeling as vsm
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    cfg = ref_transunet.small_config(2)
    img, B, cin, seed = int(g["img"]), int(g["B"]), int(g["cin"]), int(g["seed"])
    ref = getattr(ref_transunet, rcls)(cfg, img)
    ref.load_state_dict(recipe.fill_state_dict(ref.state_dict(), seed=seed, negative_gamma=False))
    x, _ = recipe.synthetic_batch(B, cin, img, img, 2, seed=seed)
    L.CLASS_NUMBER = 2
    m = getattr(vsm, pcls)(product_config(cfg, img), img_size=img, num_classes=2, compute_dtype="fp32")
    assert list(m.state_dict().keys()) == g["keys"].tolist()
    m.load_state_dict(ref.state_dict())
    m.to(DEV).train()
    outs = m(x.to(DEV))
    assert isinstance(outs, tuple) and len(outs) == len(ref.HEADS)
    labs = [recipe.synthetic_batch(B, cin, img, img, 2, seed=seed + 100 * i)[1] for i in range(len(outs))]
    loss = sum(L.calc_loss(o, l.to(DEV), loss_type="dice_bce_mc") for o, l in zip(outs, labs))
    loss.backward()
    for i, o in enumerate(outs):
        gl = g[f"logits{i + 1}"]
        np.testing.assert_allclose(o.detach().cpu().numpy(), gl, rtol=1e-4, atol=1e-4 * float(np.abs(gl).max()))
    assert abs(loss.item() - float(g["loss0"])) < 1e-4
    ref.train()
    sum(ref_unet.dice_bce_mc(o, l, 2) for o, l in zip(ref(x), labs)).backward()
    worst = ("", 0.0)
    for (k, p), (_, rp) in zip(m.named_parameters(), ref.named_parameters()):
        assert p.grad is not None, k
        e = (p.grad.detach().double().cpu() - rp.grad.double()).norm().item() / (rp.grad.double().norm().item() + 1e-6 / 3e-3)
        worst = max(worst, (k, e), key=lambda t: t[1])
    assert worst[1] < 3e-3, worst


@pytest.mark.gpu
def test_transunet_submodules_run_standalone():
    """The sub-modules of the TransUNet can be called on their own like the reference's (vit_seg_modeling.py:73-94,113-119,
    154-165,177-187,237-244,309-315,355-367; vit_seg_modeling_resnet_skip.py:20-25,60-74,142-160): each builds a small HIP
    tape.  fp32 path against a plain-PyTorch restatement with the module's own parameters, forward and input gradient."""
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    import torch.nn.functional as F
    from TransUnet import vit_seg_modeling as vsm
    from TransUnet import vit_seg_modeling_resnet_skip as rs
    cfg = product_config(ref_transunet.small_config(2), 64)
    torch.manual_seed(3)
    g = torch.Generator().manual_seed(4)
    hid, heads = cfg.hidden_size, cfg.transformer["num_heads"]

    def close(a, b, tol=2e-4):
        a, b = a.detach().float().cpu(), b.detach().float().cpu()
        assert a.shape == b.shape, (a.shape, b.shape)
        assert (a - b).abs().max().item() <= tol * max(b.abs().max().item(), 1e-3), (a - b).abs().max().item()

    def with_grad(mod, x, ref_fn, tol=2e-4):
        import copy
        mod_cpu = copy.deepcopy(mod).train()
        mod.to(DEV).train()
        mod._compute_dtype = "fp32"
        xd = x.to(DEV).requires_grad_(True)
        out = mod(xd)
        out = out[0] if isinstance(out, tuple) else out
        xr = x.clone().requires_grad_(True)
        want = ref_fn(mod_cpu, xr)
        close(out, want, tol)
        gy = torch.randn(want.shape, generator=g)
        out.backward(gy.to(DEV))
        want.backward(gy)
        close(xd.grad, xr.grad, 5 * tol)
        for (k, p), (_, rp) in zip(mod.named_parameters(), mod_cpu.named_parameters()):
            if rp.grad is not None and rp.grad.abs().max() > 1e-6:
                close(p.grad, rp.grad, 10 * tol)

    def ref_attn(m, x):
        B, N, C = x.shape
        sp = lambda t: t.view(B, N, heads, C // heads).permute(0, 2, 1, 3)
        p = torch.softmax(sp(m.query(x)) @ sp(m.key(x)).transpose(-1, -2) / (C // heads) ** 0.5, -1)
        return m.out((p @ sp(m.value(x))).permute(0, 2, 1, 3).reshape(B, N, C))

    def ref_mlp(m, x):
        return m.fc2(F.gelu(m.fc1(x)))

    def ref_block(m, x):
        h = x + ref_attn(m.attn, F.layer_norm(x, (hid,), m.attention_norm.weight, m.attention_norm.bias, 1e-6))
        return h + ref_mlp(m.ffn, F.layer_norm(h, (hid,), m.ffn_norm.weight, m.ffn_norm.bias, 1e-6))

    def ref_encoder(m, x):
        for blk in m.layer:
            x = ref_block(blk, x)
        return F.layer_norm(x, (hid,), m.encoder_norm.weight, m.encoder_norm.bias, 1e-6)

    def ref_decoder_block(m, x):
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
        for c in (m.conv1, m.conv2):
            x = F.relu(F.batch_norm(F.conv2d(x, c[0].weight, None, 1, 1), None, None, c[1].weight, c[1].bias, True, 0.1, 1e-5))
        return x

    def ref_stdconv(m, x):
        w = m.weight
        v, mu = torch.var_mean(w, dim=[1, 2, 3], keepdim=True, unbiased=False)
        return F.conv2d(x, (w - mu) / torch.sqrt(v + 1e-5), None, m.stride, m.padding)

    tok = torch.randn(2, 16, hid, generator=g)
    with_grad(vsm.Attention(cfg, False), tok, ref_attn)
    with_grad(vsm.Mlp(cfg), tok, ref_mlp)
    with_grad(vsm.Block(cfg, False), tok, ref_block)
    with_grad(vsm.Encoder(cfg, False), tok, ref_encoder, tol=5e-4)
    with_grad(vsm.DecoderBlock(32, 16), torch.randn(2, 32, 6, 5, generator=g), ref_decoder_block, tol=5e-4)
    with_grad(rs.StdConv2d(8, 16, kernel_size=3, stride=2, padding=1, bias=False), torch.randn(2, 8, 11, 9, generator=g), ref_stdconv)

    # shape-level: the multi-output modules return what the reference returns
    emb = vsm.Embeddings(cfg, img_size=64).to(DEV).train()
    toks, feats = emb(torch.randn(2, 1, 64, 64, generator=g).to(DEV))
    assert tuple(toks.shape) == (2, 16, hid) and [tuple(f.shape[2:]) for f in feats] == [(8, 8), (16, 16), (32, 32)]
    tr = vsm.Transformer(cfg, 64, False).to(DEV).train()
    enc, attn_w, feats = tr(torch.randn(2, 3, 64, 64, generator=g).to(DEV))
    assert tuple(enc.shape) == (2, 16, hid) and attn_w == [] and len(feats) == 3
    dec = vsm.DecoderCup(cfg).to(DEV).train()
    y = dec(enc.detach(), [f.detach() for f in feats])
    assert tuple(y.shape) == (2, cfg.decoder_channels[-1], 64, 64)
    y.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in dec.parameters())


@pytest.mark.gpu
def test_block_applied_twice_in_one_tape_accumulates_both_gradients():
    """A ViT Block (LayerNorm, Q/K/V/out/fc1/fc2 linears with biases) applied twice in ONE fp16 tape: the grouped
    end-of-backward launches (umi_conv_wgrad_group, umi_colsum_group, umi_gn_param_grads_group) WRITE their outputs, so the
    second use of every parameter has to be added after them.  Reference: torch autograd, CPU fp32."""
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    import copy
    import torch.nn.functional as F
    from Model import _run_tape
    from umi.graph_tu import TUTape
    from TransUnet import vit_seg_modeling as vsm
    cfg = product_config(ref_transunet.small_config(2), 64)
    cfg.transformer["dropout_rate"] = 0.0
    hid, heads = cfg.hidden_size, cfg.transformer["num_heads"]
    torch.manual_seed(7)
    blk = vsm.Block(cfg, False)
    for p in blk.parameters():                     # biases / LayerNorm weights away from their trivial initial values
        if p.dim() == 1:
            p.data += 0.1 * torch.randn_like(p)
    ref = copy.deepcopy(blk).train()

    def ref_block(m, x):
        def attn(a, v):
            B, N, C = v.shape
            sp = lambda t: t.view(B, N, heads, C // heads).permute(0, 2, 1, 3)
            p = torch.softmax(sp(a.query(v)) @ sp(a.key(v)).transpose(-1, -2) / (C // heads) ** 0.5, -1)
            return a.out((p @ sp(a.value(v))).permute(0, 2, 1, 3).reshape(B, N, C))
        h = x + attn(m.attn, F.layer_norm(x, (hid,), m.attention_norm.weight, m.attention_norm.bias, 1e-6))
        return h + m.ffn.fc2(F.gelu(m.ffn.fc1(F.layer_norm(h, (hid,), m.ffn_norm.weight, m.ffn_norm.bias, 1e-6))))

    class Twice(torch.nn.Module):
        def __init__(self, b):
            super().__init__()
            self.b = b
            self._compute_dtype = "fp16"

        def forward(self, x):
            build = lambda t, a: vsm._build_block(t, vsm._build_block(t, a, self.b), self.b)
            return vsm._tok_out(_run_tape(self, [vsm._tok_in(x)], build, tape_cls=TUTape, dtype=torch.float16))

    x = torch.randn(2, 16, hid)
    gy = torch.randn(2, 16, hid)
    m = Twice(blk.to(DEV)).train()
    y = m(x.to(DEV))
    y.backward(gy.to(DEV))
    yr = ref_block(ref, ref_block(ref, x))
    yr.backward(gy)
    rel = lambda a, b: ((a.detach().float().cpu() - b).norm() / (b.norm() + 1e-12)).item()
    assert rel(y, yr.detach()) < 2e-2
    for (k, p), (_, rp) in zip(blk.named_parameters(), ref.named_parameters()):
        assert p.grad is not None, k
        if k == "attn.key.bias":                   # softmax is invariant to a shift of the keys: this gradient is rounding noise
            continue
        assert rel(p.grad, rp.grad) < 6e-2, (k, rel(p.grad, rp.grad))      # a dropped second contribution is off by ~0.5-1


# Bar of test_bottleneck_applied_twice_in_one_tape_accumulates_both_gradients: three times the worst per-tensor relative L2
# error of this very test, measured on one MI355X at the commit before the tape's deferred fills moved into umi/deferred.py
# (4.52e-2, conv2.weight; fp16 storage rounding, the same figures after the move, which is bit-identical): the margin only
# absorbs a change of seed.  A dropped second contribution moves every tensor by >= 0.62 (checked in the test: >= 4 bars).
_TWICE_BOTTLENECK_BAR = 3 * 4.52e-2


def _twice_bottleneck_reference(seed):
    """CPU fp32 autograd side of the test below: the unit, the input, the seed gradient, the reference output of two
    applications, every parameter's reference gradient, and the same with the second use's contribution cut off."""
    import copy
    import torch.nn.functional as F
    from TransUnet import vit_seg_modeling_resnet_skip as rs
    torch.manual_seed(seed)
    unit = rs.PreActBottleneck(cin=64, cout=64, cmid=32)          # stride 1, no downsample branch: output width = input width
    for p in unit.parameters():                    # GroupNorm weights / biases away from their trivial initial values
        if p.dim() == 1:
            p.data += 0.1 * torch.randn_like(p)
    ref = copy.deepcopy(unit).train()

    def ref_unit(x):
        def std_conv(c, v):
            var, mu = torch.var_mean(c.weight, dim=[1, 2, 3], keepdim=True, unbiased=False)
            return F.conv2d(v, (c.weight - mu) / torch.sqrt(var + 1e-5), None, c.stride, c.padding)
        y = F.relu(F.group_norm(std_conv(ref.conv1, x), 32, ref.gn1.weight, ref.gn1.bias, 1e-6))
        y = F.relu(F.group_norm(std_conv(ref.conv2, y), 32, ref.gn2.weight, ref.gn2.bias, 1e-6))
        return F.relu(x + F.group_norm(std_conv(ref.conv3, y), 32, ref.gn3.weight, ref.gn3.bias, 1e-6))

    x, gy = torch.randn(2, 64, 8, 8), torch.randn(2, 64, 8, 8)
    grads = []
    for cut in (False, True):
        ref.zero_grad()
        h = ref_unit(x)
        yr = ref_unit(h.detach() if cut else h)
        yr.backward(gy)
        grads.append({k: p.grad.clone() for k, p in ref.named_parameters()})
    return unit, x, gy, yr.detach(), grads[0], grads[1]


@pytest.mark.gpu
def test_bottleneck_applied_twice_in_one_tape_accumulates_both_gradients():
    """A stride-1 PreActBottleneck (three StdConv2d, three GroupNorm(32, .)) applied twice in ONE fp16 tape with a pack cache: the
    use the backward pass meets first takes the deferred slots (umi_wstd_bwd_multi, umi_gn_param_grads_group, which WRITE their
    outputs at the flush); the other use gets no slot, runs its standardisation backward / row sums at once and has to be added
    after the flush.  Reference: torch autograd, CPU fp32."""
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    from Model import _run_tape
    from umi.graph_tu import TUTape
    from TransUnet import vit_seg_modeling_resnet_skip as rs
    BAR = _TWICE_BOTTLENECK_BAR
    unit, x, gy, yr, g_full, g_cut = _twice_bottleneck_reference(seed=7)
    rel = lambda a, b: ((a.detach().float().cpu() - b).norm() / (b.norm() + 1e-12)).item()
    # the test must tell a dropped contribution from rounding: without the second use every reference gradient moves by at
    # least four bars (no tensor had to be left out)
    for k in g_full:
        assert rel(g_cut[k], g_full[k]) >= 4 * BAR, (k, rel(g_cut[k], g_full[k]))

    class Twice(torch.nn.Module):
        def __init__(self, u):
            super().__init__()
            self.u = u
            self._compute_dtype = "fp16"

        def forward(self, v):
            build = lambda t, a: rs.build_unit(t, rs.build_unit(t, a, self.u), self.u)
            return _run_tape(self, [v], build, tape_cls=TUTape, dtype=torch.float16)

    m = Twice(unit.to(DEV)).train()
    y = m(x.to(DEV))
    y.backward(gy.to(DEV))
    assert rel(y, yr) < 2e-2
    errs = {k: rel(p.grad, g_full[k]) for k, p in unit.named_parameters()}
    print("worst per-tensor gradient error", max(errs.items(), key=lambda kv: kv[1]))
    for k, e in errs.items():
        assert e < BAR, (k, e)


@pytest.mark.gpu
def test_fused_linear_epilogues_leave_the_dropout_training_step_unchanged(monkeypatch):
    """TransUNet with dropout 0.1 in train mode, fp16: the step with the ViT linears' GELU / dropout / residual tails in the GEMM
    epilogues (umi_linear_fused) equals the step with the separate kernels (UMI_NO_LINEAR_FUSION=1) bit for bit -- logits and
    every parameter gradient (same counter-based random stream)."""
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    import loss as L
    from TransUnet.vit_seg_modeling import VisionTransformer
    cfg = ref_transunet.small_config(2)
    cfg["dropout_rate"] = 0.1
    L.CLASS_NUMBER = 2
    x, lab = recipe.synthetic_batch(2, 1, 64, 64, 2, seed=9)
    outs = []
    for off in ("1", "0"):
        monkeypatch.setenv("UMI_NO_LINEAR_FUSION", off)
        torch.manual_seed(11)
        m = VisionTransformer(product_config(cfg, 64), img_size=64, num_classes=2, compute_dtype="fp16")
        m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=9, negative_gamma=False))
        m.to(DEV).train()
        torch.manual_seed(12)                      # the model draws its dropout base seed from torch's generator
        logits = m(x.to(DEV))
        L.calc_loss(logits, lab.to(DEV), loss_type="dice_bce_mc").backward()
        outs.append((logits.detach().clone(), [p.grad.detach().clone() for p in m.parameters()]))
    assert torch.equal(outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1], outs[1][1]):
        assert torch.equal(a, b)
