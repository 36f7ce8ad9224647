#!/usr/bin/env python3
"""Pure-ViT TransUNet fixtures (tests/golden/vit_*.npz) from the REFERENCE itself (build container only).

The reference's `TransUnet.vit_seg_modeling.VisionTransformer` / `VisionTransformerMultitask` built from a config without
`patches.grid` (the non-hybrid branch of its `Embeddings`, vit_seg_modeling.py:137-140: a P x P / stride-P patch convolution on
the image, no ResNet, `n_skip = 0`), weights from oracle/recipe.fill_state_dict, inputs from oracle/recipe.synthetic_batch,
forward + `dice_bce_mc` + backward (+ one SGD step), numeric outputs only.  Dropout is 0.0 in every config (CPU and device
random streams cannot match).  The reference is imported through tools/gen_golden.py's stubs.

Seeds: a seed is taken only if two float32 evaluations -- the reference's own and the tests' plain restatement, which orders its
operations differently -- both give gradients within `TIE_BAR` (relative L2, every parameter) of a float64 run of the reference
with the same weights, i.e. no ReLU input sits within rounding of zero (gen_golden.gen_unet_multitask has the story); the first
such seed from the case's starting seed on is used and recorded with the gap it measured.
The device's fp32 kernels are two more evaluation orders ("fp32": the VALU kernels, "fp32_mfma_*": the matrix-core ones), and each
order has its own unlucky seeds: of the multitask case's CPU-clean seeds 59, 64, 65, 67, 76 and 81, the VALU kernels flip a mask
at 59, 64, 65 and 81 (gradient gaps 4e-4 .. 2e-3 against the float64 step; one flipped pixel of a 32 x 32 map moves a BatchNorm
bias gradient that far) and the matrix-core kernels at 65 and 67; 76 is clean in all four orders (worst gap 9e-5, a key bias's
rounding residue), so the multitask case starts there.  Seed 52 of the two single-head cases is clean in all four as it came.
The full-size fixtures go through the same screen: `ViT-B_16` is clean at seed 63 (61 and 62 flip: gradient gaps 2.5e-3, 2.1e-3)
and uses it.  `ViT-L_16` has no clean seed: at every one of 62 .. 90 the reference's float32 run flips masks against its float64
run (`--eval-gap --model ViT-L_16 --ref-only 63 .. 90`: largest gradient gap 9e-4 .. 1e-2), so `_case` gives up after
`BIG_TRIES` seeds and keeps the first; tests/test_gpu_vit_pure.py derives that model's eval-logit bar from the measured gaps.

Usage:  python tools/gen_golden_vit.py [--only small|big|load_from]
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

TIE_BAR = 1e-4
BIG_TRIES = {"ViT-B_16": 12, "ViT-L_16": 29}      # seeds screened from the case's first one on before giving up
SMALL = dict(hidden_size=64, mlp_dim=128, num_heads=4, num_layers=2, decoder_channels=(64, 32, 32, 16))


def small_config(n_classes, patch):
    """The miniature pure-ViT configuration of the fixtures as a plain dict (the tests build the product's ConfigDict from it)."""
    return dict(SMALL, n_classes=n_classes, patch=patch, n_skip=0, dropout_rate=0.0, attention_dropout_rate=0.0)


def synthetic_vit_checkpoint(model, hidden, heads, old_grid, seed=77):
    """A seeded stand-in for the JAX `ViT-*.npz` checkpoints `load_from` consumes (reference vit_seg_modeling.py:189-224,394-430):
    their key names and layouts -- HWIO [P, P, 3, hidden] `embedding/kernel`, [hidden, heads, head_dim] attention kernels,
    [1, 1 + grid^2, hidden] position embedding with a class token -- and no ResNet keys.  Walks the MODEL's module tree, which
    the reference and the product share, so both sides draw identical arrays."""
    g = np.random.default_rng(seed)
    w = {}

    def r(*shape):
        return (g.standard_normal(shape) * 0.1).astype(np.float32)
    emb = model.transformer.embeddings
    O, I, kh, kw = emb.patch_embeddings.weight.shape
    w["embedding/kernel"], w["embedding/bias"] = r(kh, kw, I, O), r(O)
    w["Transformer/encoder_norm/scale"], w["Transformer/encoder_norm/bias"] = r(hidden), r(hidden)
    w["Transformer/posembed_input/pos_embedding"] = r(1, 1 + old_grid * old_grid, hidden)
    hd = hidden // heads
    for i, blk in enumerate(model.transformer.encoder.layer):
        root = f"Transformer/encoderblock_{i}"
        for n in ("query", "key", "value"):
            w[f"{root}/MultiHeadDotProductAttention_1/{n}/kernel"] = r(hidden, heads, hd)
            w[f"{root}/MultiHeadDotProductAttention_1/{n}/bias"] = r(heads, hd)
        w[f"{root}/MultiHeadDotProductAttention_1/out/kernel"] = r(heads, hd, hidden)
        w[f"{root}/MultiHeadDotProductAttention_1/out/bias"] = r(hidden)
        mlp = blk.ffn.fc1.weight.shape[0]
        w[f"{root}/MlpBlock_3/Dense_0/kernel"], w[f"{root}/MlpBlock_3/Dense_0/bias"] = r(hidden, mlp), r(mlp)
        w[f"{root}/MlpBlock_3/Dense_1/kernel"], w[f"{root}/MlpBlock_3/Dense_1/bias"] = r(mlp, hidden), r(hidden)
        for ln in ("LayerNorm_0", "LayerNorm_2"):
            w[f"{root}/{ln}/scale"], w[f"{root}/{ln}/bias"] = r(hidden), r(hidden)
    return w


def _ref_config(cfg):
    import ml_collections
    C = ml_collections.ConfigDict
    p = cfg["patch"]
    return C(dict(patches=C({"size": (p, p)}), hidden_size=cfg["hidden_size"],
                  transformer=C(dict(mlp_dim=cfg["mlp_dim"], num_heads=cfg["num_heads"], num_layers=cfg["num_layers"],
                                     attention_dropout_rate=cfg["attention_dropout_rate"], dropout_rate=cfg["dropout_rate"])),
                  classifier="seg", representation_size=None, resnet_pretrained_path=None, pretrained_path=None, patch_size=p,
                  decoder_channels=tuple(cfg["decoder_channels"]), n_classes=cfg["n_classes"], activation="softmax",
                  n_skip=cfg["n_skip"]))


def _named_config(vsm, name):
    c = vsm.CONFIGS[name]                 # (the gen_golden stub of ml_collections.ConfigDict cannot be deep-copied: edited in place)
    c.n_skip = 0
    c.n_classes = 2
    c.transformer.dropout_rate = 0.0
    return c


def _batch(recipe, cfg, img, B, cin, seed, heads=1):
    """x at the image size; one label map per head at the LOGITS' size (img for P = 16, img / 2 for P = 32: four x2 blocks)."""
    out_hw = img // cfg["patch"] * 16
    x, _ = recipe.synthetic_batch(B, cin, img, img, cfg["n_classes"], seed=seed)
    labs = [recipe.synthetic_batch(B, cin, out_hw, out_hw, cfg["n_classes"], seed=seed + 100 * i)[1] for i in range(heads)]
    return x, labs


def _loss(loss_mod, logits, labs):
    outs = logits if isinstance(logits, (tuple, list)) else (logits,)
    return sum(loss_mod.calc_loss(o, l, loss_type="dice_bce_mc") for o, l in zip(outs, labs))


def _tie_gap(loss_mod, make, m, x, labs, cfg):
    """max over the parameters of |g32 - g64| / |g64| (relative L2) for two float32 evaluations against the reference's float64
    run of the same weights: the reference's own, and the tests' plain restatement (tests/vit_plain.py), whose operations come in
    another order -- as the device's do.  A ReLU input within rounding of zero shows in either as a gap of 1e-4 .. 1e-2."""
    from tests import vit_plain
    m64 = make()                                  # (a model holds its config: the stub ConfigDict cannot be deep-copied)
    m64.load_state_dict(m.state_dict())
    m64.double()
    gs = []
    for mod, xx, ll in ((m, x, labs), (m64, x.double(), [l.double() for l in labs])):
        mod.train()
        mod.zero_grad()
        _loss(loss_mod, mod(xx), ll).backward()
        gs.append([p.grad.double().clone() for p in mod.parameters()])
        mod.zero_grad()
    names = [k for k, _ in m.named_parameters()]
    outputs = vit_plain.MULTITASK if len(labs) > 1 else (("decoder", "segmentation_head"),)
    plain = vit_plain.train_step(m.state_dict(), names, x, labs, cfg["n_classes"], cfg["num_heads"], cfg["patch"], outputs)
    gs.append([plain["grads"][k].double() for k in names])
    # (the key biases' gradient is mathematically zero, softmax is shift invariant: ~1e-17 in float64, left out)
    gaps = [max(((a - b).norm() / b.norm()).item() for a in (a0, a1)) if b.norm() > 1e-12 else 0.0
            for a0, b, a1 in zip(*gs)]
    return max(gaps)


def _pick_seed(recipe, loss_mod, make, cfg, img, B, cin, seed0, heads=1, tries=12, scan=False, allow_unscreened=False):
    """The first seed from seed0 on that passes the screen (scan: prints the gap of all `tries` seeds, returns the clean ones)."""
    clean, first = [], None
    for seed in range(seed0, seed0 + tries):
        torch.manual_seed(0)
        m = make()
        m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=seed, negative_gamma=False))
        x, labs = _batch(recipe, cfg, img, B, cin, seed, heads)
        gap = _tie_gap(loss_mod, make, m, x, labs, cfg)
        print(f"  seed {seed}: float32 vs float64 gradient gap {gap:.2e}")
        if gap < TIE_BAR and not scan:
            return seed, gap
        if gap < TIE_BAR:
            clean.append(seed)
        first = first if seed > seed0 else (seed, gap)
    if scan:
        return clean
    if allow_unscreened:
        print(f"  no clean seed in {seed0}..{seed0 + tries - 1}: keeping {first[0]} (gap {first[1]:.2e})")
        return first
    raise RuntimeError(f"no seed in {seed0}..{seed0 + tries - 1} is free of ReLU near-ties")


def _case(vsm, loss_mod, recipe, sig, meta, GOLD, name, cfg, rcfg, img, B, cin, seed0, full, cls_name="VisionTransformer",
          tries=12, allow_unscreened=False):
    heads = 2 if cls_name == "VisionTransformerMultitask" else 1
    loss_mod.CLASS_NUMBER = cfg["n_classes"]

    def make():
        return getattr(vsm, cls_name)(rcfg, img_size=img, num_classes=cfg["n_classes"])
    seed, gap = _pick_seed(recipe, loss_mod, make, cfg, img, B, cin, seed0, heads, tries, allow_unscreened=allow_unscreened)
    torch.manual_seed(0)
    m = make()
    out = dict(img=img, B=B, cin=cin, seed=seed, tie_gap=gap, n_keys=len(m.state_dict()), patch=cfg["patch"],
               n_classes=cfg["n_classes"])
    out["keys"] = np.array(list(m.state_dict().keys()))
    out["shapes"] = np.array([",".join(map(str, v.shape)) for v in m.state_dict().values()])
    if full:
        for k, v in m.state_dict().items():                # the reference's own init under torch.manual_seed(0)
            out["init_sig." + k] = sig(v.float())
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=seed, negative_gamma=False))
    x, labs = _batch(recipe, cfg, img, B, cin, seed, heads)
    opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    m.train()
    logits = m(x)
    loss = _loss(loss_mod, logits, labs)
    opt.zero_grad()
    loss.backward()
    outs = logits if heads > 1 else (logits,)
    out["loss0"] = loss.item()
    for i, o in enumerate(outs):
        tag = f"logits{i + 1}" if heads > 1 else "logits"
        out[tag + "_sig"] = sig(o)
        if full:
            out[tag] = o.detach().numpy()
    for k, p in m.named_parameters():
        out["grad_sig." + k] = sig(p.grad)
    opt.step()
    for k, v in m.state_dict().items():
        if "running" in k or "num_batches" in k or full:
            out["after1." + k] = sig(v.float())
    m.eval()
    with torch.no_grad():
        ev = m(x)
    for i, o in enumerate(ev if heads > 1 else (ev,)):
        tag = f"eval_logits{i + 1}" if heads > 1 else "eval_logits"
        out[tag + "_sig"] = sig(o)
        if full:
            out[tag] = o.numpy()
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out, **meta())
    print(f"wrote {name}.npz keys={out['n_keys']} seed={seed} loss0={out['loss0']:.6f}")


def _case_load_from(vsm, sig, meta, GOLD):
    """state_dict signatures and the changed keys after the REFERENCE's `load_from` of the synthetic pure-ViT checkpoint, for the
    two position-embedding paths a 4 x 4-token model can take: a 3 x 3 grid + class token (`ndimage.zoom`) and a 4 x 4 grid +
    class token (class token dropped)."""
    cfg = small_config(2, 16)
    out = {}
    for tag, old_grid in (("zoom", 3), ("drop_cls", 4)):
        torch.manual_seed(0)
        m = vsm.VisionTransformer(_ref_config(cfg), img_size=64, num_classes=2)
        w = synthetic_vit_checkpoint(m, cfg["hidden_size"], cfg["num_heads"], old_grid, seed=77)
        before = {k: v.clone() for k, v in m.state_dict().items()}
        m.load_from(w)
        out[tag + ".n_ckpt_keys"] = len(w)
        changed = []
        for k, v in m.state_dict().items():
            out[f"{tag}.sig." + k] = sig(v.float())
            if not torch.equal(v, before[k]):
                changed.append(k)
        out[tag + ".changed"] = np.array(changed)
    np.savez_compressed(os.path.join(GOLD, "vit_small_load_from.npz"), **out, **meta())
    print("wrote vit_small_load_from.npz", out["zoom.n_ckpt_keys"], len(out["zoom.changed"]))


def _eval_gap(vsm, loss_mod, recipe, sig, key, seed, orders=("ref32", "plain32")):
    """How far two float32 evaluations -- the reference's OWN and the tests' plain restatement, which orders its operations
    differently -- lie from the reference's float64 run of the same weights, in the signature metric of the tests (relative error
    of norm and abs-sum, largest sample error over the sampled scale), for the training logits and for the eval logits after one
    SGD step; and the largest per-parameter gradient gap (the near-tie screen of the small fixtures).  The yardstick for a
    device bar where the hybrid's bars do not carry over."""
    from tests import vit_plain
    rcfg = _named_config(vsm, key)
    loss_mod.CLASS_NUMBER = 2
    cfg = dict(n_classes=2, patch=16)
    x, labs = _batch(recipe, cfg, 224, 1, 3, seed)
    runs = {}
    for tag, dt in (("ref32", torch.float32), ("ref64", torch.float64)):
        torch.manual_seed(0)
        m = vsm.VisionTransformer(rcfg, img_size=224, num_classes=2)
        m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=seed, negative_gamma=False))
        if tag == "ref32":
            sd0, names, heads = {k: v.clone() for k, v in m.state_dict().items()}, [k for k, _ in m.named_parameters()], \
                rcfg.transformer["num_heads"]
        m.to(dt).train()
        opt = torch.optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        logits = m(x.to(dt))
        opt.zero_grad()
        _loss(loss_mod, logits, [l.to(dt) for l in labs]).backward()
        grads = [p.grad.double().clone() for p in m.parameters()]
        opt.step()
        m.eval()
        with torch.no_grad():
            runs[tag] = (sig(logits), sig(m(x.to(dt))), grads)
        del m, opt
    if "plain32" in orders:
        plain = vit_plain.train_step(sd0, names, x, labs, 2, heads, 16)
        with torch.no_grad():
            ev = vit_plain.forward(vit_plain.leaves(plain["after"]), x, heads, 16, False)
        runs["plain32"] = (sig(plain["logits"]), sig(ev), [plain["grads"][k].double() for k in names])
    out = {}
    b = runs["ref64"]
    for tag in orders:
        a = runs[tag]
        ggap = max(((ga - gb).norm() / gb.norm()).item() for ga, gb in zip(a[2], b[2]) if gb.norm() > 1e-12)
        for what, sa, sb in (("train", a[0], b[0]), ("eval", a[1], b[1])):
            out[tag, what] = (abs(sa[0] / sb[0] - 1), abs(sa[2] / sb[2] - 1), np.abs(sa[3:] - sb[3:]).max() / np.abs(sb[3:]).max())
            print(f"{key} seed {seed} {tag} {what} logits: norm {out[tag, what][0]:.2e} abs-sum {out[tag, what][1]:.2e} "
                  f"samples {out[tag, what][2]:.2e} of the sampled scale", flush=True)
        print(f"{key} seed {seed} {tag} worst gradient gap {ggap:.2e}", flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["small", "big", "load_from"])
    ap.add_argument("--scan", nargs=2, type=int, metavar=("SEED0", "N"),
                    help="write nothing: screen N seeds from SEED0 on for the multitask case and list the clean ones")
    ap.add_argument("--eval-gap", nargs="*", type=int, metavar="SEED", default=None,
                    help="write nothing: two float32 evaluations against the reference's float64 run of ViT-B_16 / ViT-L_16 at "
                         "224, for the fixtures' seeds and any further SEEDs; --model picks one")
    ap.add_argument("--model", choices=["ViT-B_16", "ViT-L_16"])
    ap.add_argument("--ref-only", action="store_true", help="--eval-gap: the reference's own float32 run only (the plain "
                    "restatement's float32 run gives the same figures at these sizes)")
    args = ap.parse_args()
    from oracle import recipe
    from tools.gen_golden import GOLD, import_reference, meta, sig
    _, loss_mod, _ = import_reference()
    from TransUnet import vit_seg_modeling as vsm
    torch.set_num_threads(min(8, torch.get_num_threads()))
    a = (vsm, loss_mod, recipe, sig, meta, GOLD)
    if args.eval_gap is not None:
        for key, seed in (("ViT-B_16", 61), ("ViT-L_16", 62)):
            if args.model in (None, key):
                orders = ("ref32",) if args.ref_only else ("ref32", "plain32")
                gaps = [_eval_gap(vsm, loss_mod, recipe, sig, key, sd, orders) for sd in [seed] + [e for e in args.eval_gap if e != seed]]
                worst = [max(g[t, "eval"][i] for g in gaps for t in orders) for i in range(3)]
                print(f"{key}: largest eval-logit gap over {len(gaps)} seeds x {len(orders)} float32 orders: norm {worst[0]:.2e} "
                      f"abs-sum {worst[1]:.2e} samples {worst[2]:.2e}", flush=True)
        return
    if args.scan:
        c16 = small_config(2, 16)
        loss_mod.CLASS_NUMBER = 2
        print("clean:", _pick_seed(recipe, loss_mod, lambda: vsm.VisionTransformerMultitask(_ref_config(c16), img_size=64, num_classes=2),
                                   c16, 64, 2, 1, args.scan[0], 2, args.scan[1], scan=True))
        return
    if args.only in (None, "small"):
        c16, c32 = small_config(2, 16), small_config(4, 32)
        _case(*a, "vit_small_p16", c16, _ref_config(c16), 64, 2, 1, 51, True)
        _case(*a, "vit_small_p32_rgb", c32, _ref_config(c32), 96, 1, 3, 52, True)
        _case(*a, "vit_small_multitask", c16, _ref_config(c16), 64, 2, 1, 76, True, cls_name="VisionTransformerMultitask")
    if args.only in (None, "load_from"):
        _case_load_from(vsm, sig, meta, GOLD)
    if args.only in (None, "big"):
        for name, key, seed in (("vit_b16_224", "ViT-B_16", 61), ("vit_l16_224", "ViT-L_16", 62)):
            if args.model not in (None, key):
                continue
            rcfg = _named_config(vsm, key)
            cfg = dict(n_classes=2, patch=16, num_heads=rcfg.transformer["num_heads"])
            _case(*a, name, cfg, rcfg, 224, 1, 3, seed, False, tries=BIG_TRIES[key], allow_unscreened=key == "ViT-L_16")


if __name__ == "__main__":
    main()
