"""Pure-ViT TransUNet (`ViT-B_16`, `ViT-B_32`, `ViT-L_16`, `ViT-L_32` with `n_skip = 0`) on the CPU: the public surface against the
reference's fixtures (tools/gen_golden_vit.py), `load_from` of a checkpoint without ResNet keys, the tests' plain restatement
(tests/vit_plain.py) against the same fixtures, the refusals that stay, and the patch gather's argument checks."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import recipe
from tests import vit_plain
from tests.test_oracle_golden import _sig_close, sig
from tools.gen_golden_vit import small_config, synthetic_vit_checkpoint


def _named(name):
    from TransUnet.vit_seg_modeling import CONFIGS
    c = copy.deepcopy(CONFIGS[name])
    c.n_skip = 0
    c.n_classes = 2
    return c


@pytest.mark.parametrize("name", ["ViT-B_16", "ViT-B_32", "ViT-L_16", "ViT-L_32"])
def test_named_configs_construct(golden_dir, name):
    from TransUnet.vit_seg_modeling import VisionTransformer
    cfg = _named(name)
    P = cfg.patches["size"][0]
    m = VisionTransformer(cfg, img_size=224, num_classes=2)
    sd = m.state_dict()
    assert not any("hybrid_model" in k for k in sd)
    emb = m.transformer.embeddings
    assert emb.hybrid is False and not hasattr(emb, "hybrid_model")
    assert tuple(emb.patch_embeddings.weight.shape) == (cfg.hidden_size, 3, P, P) and emb.patch_embeddings.stride == (P, P)
    assert tuple(emb.position_embeddings.shape) == (1, (224 // P) ** 2, cfg.hidden_size)
    assert list(sd)[:3] == ["transformer.embeddings.position_embeddings", "transformer.embeddings.patch_embeddings.weight",
                            "transformer.embeddings.patch_embeddings.bias"]
    fixture = {"ViT-B_16": "vit_b16_224.npz", "ViT-L_16": "vit_l16_224.npz"}.get(name)
    if fixture:
        g = np.load(os.path.join(golden_dir, fixture))
        assert list(sd.keys()) == g["keys"].tolist()
        assert [",".join(map(str, v.shape)) for v in sd.values()] == g["shapes"].tolist()


def test_small_surface_and_init(golden_dir):
    """Key set, order, shapes and the init random stream under torch.manual_seed(0) equal the reference's."""
    from TransUnet.vit_seg_modeling import CONFIGS, VisionTransformer
    g = np.load(os.path.join(golden_dir, "vit_small_p16.npz"))
    torch.manual_seed(0)
    m = VisionTransformer(vit_plain.product_config(small_config(2, 16)), img_size=64, num_classes=2)
    sd = m.state_dict()
    assert list(sd.keys()) == g["keys"].tolist()
    assert [",".join(map(str, v.shape)) for v in sd.values()] == g["shapes"].tolist()
    for k, v in sd.items():
        _sig_close(sig(v.float()), g["init_sig." + k], rtol=1e-6)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(1, 1, 64, 64))
    # the hybrid still builds as before
    h = VisionTransformer(copy.deepcopy(CONFIGS["R50-ViT-B_16"]), img_size=256, num_classes=2)     # grid (16, 16): patch 1 x 1
    assert h.transformer.embeddings.hybrid is True and len(h.state_dict()) == 409
    assert h.transformer.embeddings.patch_embeddings.kernel_size == (1, 1)


@pytest.mark.parametrize("tag,old_grid", [("zoom", 3), ("drop_cls", 4)])
def test_load_from_matches_reference(golden_dir, tag, old_grid):
    from TransUnet.vit_seg_modeling import VisionTransformer
    g = np.load(os.path.join(golden_dir, "vit_small_load_from.npz"))
    cfg = small_config(2, 16)
    torch.manual_seed(0)
    m = VisionTransformer(vit_plain.product_config(cfg), img_size=64, num_classes=2)
    w = synthetic_vit_checkpoint(m, cfg["hidden_size"], cfg["num_heads"], old_grid, seed=77)
    assert len(w) == int(g[tag + ".n_ckpt_keys"]) and not any(k.startswith(("conv_root", "gn_root", "block")) for k in w)
    assert w["embedding/kernel"].shape == (16, 16, 3, 64)                      # HWIO
    before = {k: v.clone() for k, v in m.state_dict().items()}
    m.load_from(w)
    changed = [k for k, v in m.state_dict().items() if not torch.equal(v, before[k])]
    assert changed == g[tag + ".changed"].tolist()
    for k, v in m.state_dict().items():
        np.testing.assert_allclose(sig(v.float()), g[f"{tag}.sig." + k], rtol=1e-6, atol=1e-7, err_msg=k)


def plain_case(golden_dir, name):
    """(fixture, config dict, product model with the fixture's weights, x, labels, outputs) of a small fixture."""
    from TransUnet.vit_seg_modeling import VisionTransformer, VisionTransformerMultitask
    g = np.load(os.path.join(golden_dir, name + ".npz"))
    multi = "multitask" in name
    cfg = small_config(int(g["n_classes"]), int(g["patch"]))
    img, B, cin, seed = int(g["img"]), int(g["B"]), int(g["cin"]), int(g["seed"])
    m = (VisionTransformerMultitask if multi else VisionTransformer)(vit_plain.product_config(cfg), img_size=img,
                                                                      num_classes=cfg["n_classes"], compute_dtype="fp32")
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=seed, negative_gamma=False))
    out_hw = img // cfg["patch"] * 16
    x, _ = recipe.synthetic_batch(B, cin, img, img, cfg["n_classes"], seed=seed)
    labs = [recipe.synthetic_batch(B, cin, out_hw, out_hw, cfg["n_classes"], seed=seed + 100 * i)[1] for i in range(2 if multi else 1)]
    return g, cfg, m, x, labs, vit_plain.MULTITASK if multi else (("decoder", "segmentation_head"),)


def logits_close(got, want):
    np.testing.assert_allclose(got.detach().cpu().numpy(), want, rtol=1e-4, atol=1e-4 * float(np.abs(want).max()))


@pytest.mark.parametrize("name", ["vit_small_p16", "vit_small_p32_rgb", "vit_small_multitask"])
def test_plain_restatement_reproduces_the_fixtures(golden_dir, name):
    g, cfg, m, x, labs, outputs = plain_case(golden_dir, name)
    r = vit_plain.train_step(m.state_dict(), [k for k, _ in m.named_parameters()], x, labs, cfg["n_classes"], cfg["num_heads"],
                             cfg["patch"], outputs)
    outs = r["logits"] if isinstance(r["logits"], tuple) else (r["logits"],)
    for i, o in enumerate(outs):
        logits_close(o, g[f"logits{i + 1}" if len(outs) > 1 else "logits"])
    assert tuple(outs[0].shape[2:]) == (int(g["img"]) // cfg["patch"] * 16,) * 2          # P = 32: half-size logits
    assert abs(r["loss"].item() - float(g["loss0"])) < 1e-4
    for k in r["grads"]:
        if g["grad_sig." + k][0] > 1e-7:                          # (key biases: a mathematically zero gradient, rounding only)
            _sig_close(sig(r["grads"][k]), g["grad_sig." + k], rtol=2e-3)
    for k, v in r["after"].items():
        _sig_close(sig(v.float()), g["after1." + k], rtol=1e-4)
    ev = vit_plain.forward(vit_plain.leaves(r["after"]), x, cfg["num_heads"], cfg["patch"], False, outputs)
    for i, o in enumerate(ev if isinstance(ev, tuple) else (ev,)):
        logits_close(o, g[f"eval_logits{i + 1}" if len(outs) > 1 else "eval_logits"])


def test_multitask_classes_inherit_the_variant():
    from TransUnet.vit_seg_modeling import VisionTransformerMultitask, VisionTransformerMultitaskEM
    cfg = vit_plain.product_config(small_config(2, 16))
    m2 = VisionTransformerMultitask(cfg, img_size=64, num_classes=2)
    m6 = VisionTransformerMultitaskEM(cfg, img_size=64, num_classes=2)
    for m, n in ((m2, 2), (m6, 6)):
        keys = list(m.state_dict())
        assert not any("hybrid_model" in k for k in keys)
        assert sum(k.endswith("conv_more.0.weight") for k in keys) == n
        assert all(f"segmentation_head{i}.0.weight" in keys for i in range(1, n + 1))
        assert m.transformer.embeddings.hybrid is False


def test_refusals_that_stay():
    from TransUnet.vit_seg_modeling import CONFIGS, VisionTransformer
    from TransUnet.vit_seg_configs import get_b16_config
    with pytest.raises(AttributeError):                           # like the reference: the caller sets n_skip
        VisionTransformer(get_b16_config(), img_size=224, num_classes=2)
    with pytest.raises(NotImplementedError, match="vis=True"):
        VisionTransformer(_named("ViT-B_16"), img_size=224, num_classes=2, vis=True)
    with pytest.raises(NotImplementedError, match="patch size"):
        VisionTransformer(copy.deepcopy(CONFIGS["R50-ViT-B_16"]), img_size=512, num_classes=2)
    with pytest.raises((AttributeError, KeyError)):               # classifier 'token': no decoder fields
        VisionTransformer(copy.deepcopy(CONFIGS["testing"]), img_size=224, num_classes=2)


def test_wrong_input_size_raises_before_the_device_is_touched():
    """The token-count check is host arithmetic and comes first: a CPU tensor of the wrong size meets it, not the
    'no CPU fallback' error of the first device call."""
    from TransUnet.vit_seg_modeling import VisionTransformer
    m = VisionTransformer(vit_plain.product_config(small_config(2, 16)), img_size=64, num_classes=2)
    with pytest.raises(ValueError, match=r"36 patches.*16 tokens"):
        m(torch.zeros(1, 1, 96, 96))
    with pytest.raises(ValueError, match=r"16 patches.*not a square number|8 patches.*16 tokens"):
        m(torch.zeros(1, 3, 64, 32))
    m2 = VisionTransformer(vit_plain.product_config(small_config(2, 16)), img_size=(64, 32), num_classes=2)
    with pytest.raises(ValueError, match=r"8 is not a square number"):
        m2(torch.zeros(1, 3, 64, 32))


def test_patch_rows_bad_arguments_return_status():
    from umi import lib
    f = lib.fn("umi_patch_rows")
    ok = dict(x=1 << 20, it=lib.UMI_F32, rows=1 << 21, ld=768, ot=lib.UMI_F16, B=1, C=3, H=32, W=32, P=16)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a["x"], a["it"], a["rows"], a["ld"], a["ot"], a["B"], a["C"], a["H"], a["W"], a["P"], None)
    bad = lib.UMI_ERR_BADARG
    assert call(x=None) == bad and call(rows=None) == bad
    for k in ("B", "C", "H", "W", "P"):
        assert call(**{k: 0}) == bad and call(**{k: -1}) == bad, k
    assert call(P=64) == bad                                     # no whole patch
    assert call(ld=767) == bad                                   # rows would overlap
    assert call(it=2) == bad and call(ot=-1) == bad
    assert call(C=1 << 15, P=512, H=512, W=512, ld=1 << 40) == lib.UMI_ERR_UNSUPPORTED
