"""A plain functional restatement of the pure-ViT TransUNet (ViT encoder + CUP decoder, no skips) for the tests.

`oracle/` states the hybrid only.  This module states the patch-embedding variant in torch.nn.functional calls over a PRODUCT
`state_dict` (same keys), so the device tests have full per-tensor gradients and post-step parameters to compare against; it is
itself pinned to the reference's fixtures on the CPU (tests/test_vit_pure.py).

    tokens  = conv2d(x, patch weight, stride P) flattened to [B, n, hidden] + position embedding
    block   : h += attn(LN(h)); h += fc2(gelu(fc1(LN(h))))      LN eps 1e-6, softmax(q k^T / sqrt(d)) v, exact GELU
    decoder : tokens -> [B, hidden, g, g]; conv3x3 + BN + ReLU to 512; four times (bilinear x2, align_corners, two conv3x3 + BN +
              ReLU); conv3x3 head with bias
BatchNorm: batch statistics and a running-statistics update (momentum 0.1, unbiased variance) when training, the running ones
otherwise.  Dropout is not stated: the parity configs set it to 0.
"""
import math

import torch
import torch.nn.functional as F


def product_config(cfg):
    """The product's ConfigDict from the fixtures' plain dict (tools/gen_golden_vit.small_config)."""
    from TransUnet.vit_seg_configs import ConfigDict
    p = cfg["patch"]
    return ConfigDict(patches={"size": (p, p)}, hidden_size=cfg["hidden_size"],
                      transformer=dict(mlp_dim=cfg["mlp_dim"], num_heads=cfg["num_heads"], num_layers=cfg["num_layers"],
                                       attention_dropout_rate=cfg["attention_dropout_rate"], dropout_rate=cfg["dropout_rate"]),
                      classifier="seg", representation_size=None, decoder_channels=tuple(cfg["decoder_channels"]),
                      n_classes=cfg["n_classes"], activation="softmax", n_skip=cfg["n_skip"])


def leaves(state_dict, dtype=torch.float32):
    """A working copy of a state_dict: floating entries as fresh tensors of `dtype`, the counters as they are."""
    return {k: v.detach().clone().to(dtype) if v.is_floating_point() else v.detach().clone() for k, v in state_dict.items()}


def _conv_bn_relu(sd, pre, x, training):
    x = F.conv2d(x, sd[pre + ".0.weight"], None, padding=1)
    rm, rv = sd[pre + ".1.running_mean"], sd[pre + ".1.running_var"]
    x = F.batch_norm(x, rm, rv, sd[pre + ".1.weight"], sd[pre + ".1.bias"], training, 0.1, 1e-5)
    if training:
        sd[pre + ".1.num_batches_tracked"] += 1
    return F.relu(x)


def _block(sd, pre, h, heads):
    B, n, C = h.shape
    d = C // heads
    y = F.layer_norm(h, (C,), sd[pre + ".attention_norm.weight"], sd[pre + ".attention_norm.bias"], 1e-6)
    q, k, v = (F.linear(y, sd[f"{pre}.attn.{t}.weight"], sd[f"{pre}.attn.{t}.bias"]).view(B, n, heads, d).transpose(1, 2)
               for t in ("query", "key", "value"))
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d), dim=-1)
    ctx = (p @ v).transpose(1, 2).reshape(B, n, C)
    h = h + F.linear(ctx, sd[pre + ".attn.out.weight"], sd[pre + ".attn.out.bias"])
    y = F.layer_norm(h, (C,), sd[pre + ".ffn_norm.weight"], sd[pre + ".ffn_norm.bias"], 1e-6)
    y = F.gelu(F.linear(y, sd[pre + ".ffn.fc1.weight"], sd[pre + ".ffn.fc1.bias"]))
    return h + F.linear(y, sd[pre + ".ffn.fc2.weight"], sd[pre + ".ffn.fc2.bias"])


def encode(sd, x, heads, patch):
    if x.shape[1] == 1:
        x = x.repeat(1, 3, 1, 1)
    e = "transformer.embeddings."
    h = F.conv2d(x, sd[e + "patch_embeddings.weight"], sd[e + "patch_embeddings.bias"], stride=patch)
    h = h.flatten(2).transpose(1, 2) + sd[e + "position_embeddings"]
    i = 0
    while f"transformer.encoder.layer.{i}.ffn.fc1.weight" in sd:
        h = _block(sd, f"transformer.encoder.layer.{i}", h, heads)
        i += 1
    C = h.shape[-1]
    return F.layer_norm(h, (C,), sd["transformer.encoder.encoder_norm.weight"], sd["transformer.encoder.encoder_norm.bias"], 1e-6)


def decode(sd, h, training, decoder="decoder", head="segmentation_head"):
    B, n, C = h.shape
    g = int(math.isqrt(n))
    x = h.transpose(1, 2).reshape(B, C, g, g)
    x = _conv_bn_relu(sd, decoder + ".conv_more", x, training)
    j = 0
    while f"{decoder}.blocks.{j}.conv1.0.weight" in sd:
        x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True)
        x = _conv_bn_relu(sd, f"{decoder}.blocks.{j}.conv1", x, training)
        x = _conv_bn_relu(sd, f"{decoder}.blocks.{j}.conv2", x, training)
        j += 1
    return F.conv2d(x, sd[head + ".0.weight"], sd[head + ".0.bias"], padding=1)


def forward(sd, x, heads, patch, training=True, outputs=(("decoder", "segmentation_head"),)):
    """Logits (one tensor, or a tuple for several (decoder, head) pairs over the one encoder).  `sd` is updated in place
    where BatchNorm's running statistics are."""
    h = encode(sd, x, heads, patch)
    outs = tuple(decode(sd, h, training, d, s) for d, s in outputs)
    return outs[0] if len(outs) == 1 else outs


MULTITASK = (("decoder1", "segmentation_head1"), ("decoder2", "segmentation_head2"))


def train_step(state_dict, param_names, x, labels, n_classes, heads, patch, outputs=(("decoder", "segmentation_head"),),
               lr=0.01, momentum=0.9, weight_decay=1e-4, dtype=torch.float32):
    """One training step as the fixtures take it: forward, the sum of the heads' dice_bce_mc losses, backward, the FIRST step of
    SGD with momentum and weight decay (buf = g + wd p; p -= lr buf).  -> dict(logits, loss, grads {name: tensor},
    after {name: tensor}: every state_dict entry after the step)."""
    from oracle import ref_unet
    sd = leaves(state_dict, dtype)
    for k in param_names:
        sd[k].requires_grad_(True)
    logits = forward(sd, x.to(dtype), heads, patch, True, outputs)
    outs = logits if isinstance(logits, tuple) else (logits,)
    labels = labels if isinstance(labels, (list, tuple)) else [labels]
    loss = sum(ref_unet.dice_bce_mc(o, l, n_classes) for o, l in zip(outs, labels))
    loss.backward()
    grads = {k: sd[k].grad.detach().clone() for k in param_names}
    after = {k: v.detach().clone() for k, v in sd.items()}
    for k in param_names:
        after[k] = after[k] - lr * (grads[k] + weight_decay * after[k])
    return dict(logits=logits, loss=loss.detach(), grads=grads, after=after)
