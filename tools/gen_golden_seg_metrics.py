#!/usr/bin/env python3
"""Generate tests/golden/seg_metrics.npz by running the REFERENCE's own `DiceLoss(K)` (loss.py:215-251) on the CPU on the one-hot
argmax mask of a handful of small cases:  DiceLoss(K)(one_hot(argmax(pred)), target, softmax=False).

The argmax is torch.argmax on logits without ties or NaN (the generator asserts a clear margin), so the mask does not depend on a
tie rule.  Each case keeps every per-class count below 2^24 (asserted), so the reference's float32 sums of 0/1 products are exact
integers; what is left of its float32 arithmetic is fewer than ten roundings of values <= 2 at 6e-8 each, and the generator
asserts that the float64 statement (umi.metrics.scores_numpy on confusion_numpy) is within 1e-6 of the reference's value.

Stored: `cases`, <case>_pred (float32 logits), <case>_target, <case>_dice (the reference's float32 value).

Usage:  python tools/gen_golden_seg_metrics.py
"""
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "unet-torch_amd"))
from tools.gen_golden import GOLD, import_reference, meta  # noqa: E402

BAR = 1e-6
MARGIN = 1e-3


def cases(rng):
    def logits(shape, scale=2.0):
        while True:
            x = (rng.standard_normal(shape) * scale).astype(np.float32)
            top = np.sort(x, axis=1)
            if (top[:, -1] - top[:, -2]).min() > MARGIN:
                return x

    out = {}
    out["c2_b2_17x23_int64"] = (logits((2, 2, 17, 23)), rng.integers(0, 2, (2, 17, 23)).astype(np.int64))
    out["c3_b1_9x31_float"] = (logits((1, 3, 9, 31)), rng.integers(0, 3, (1, 9, 31)).astype(np.float32))
    out["c4_b3_16x16_uint8"] = (logits((3, 4, 16, 16)), rng.integers(0, 4, (3, 16, 16)).astype(np.uint8))
    out["c5_b2_7x5_int32"] = (logits((2, 5, 7, 5)), rng.integers(0, 5, (2, 7, 5)).astype(np.int32))
    # a class that is never predicted and one that is never labelled: the smooth term alone decides those quotients
    x = logits((2, 3, 12, 20))
    x[:, 2] = -50.0
    out["c3_class_never_predicted"] = (x, rng.integers(0, 3, (2, 12, 20)).astype(np.int64))
    out["c3_class_never_labelled"] = (logits((2, 3, 12, 20)), rng.integers(0, 2, (2, 12, 20)).astype(np.int64))
    # labels outside 0..K-1 and a half-integer float label: matched to no class by the reference's one-hot encoder
    t = rng.integers(-1, 4, (2, 11, 13)).astype(np.int64)
    out["c3_out_of_range_labels"] = (logits((2, 3, 11, 13)), t)
    t = rng.integers(0, 2, (1, 10, 10)).astype(np.float32)
    t[0, ::3, ::2] = 0.5
    out["c2_half_labels"] = (logits((1, 2, 10, 10)), t)
    # mostly background predicted as background
    x = logits((1, 2, 32, 32), 0.5)
    x[:, 0] += 4.0
    t = np.zeros((1, 32, 32), np.int64)
    t[0, 10:14, 8:20] = 1
    x[0, 1, 11:15, 9:21] += 8.0
    out["c2_mostly_background"] = (x, t)
    return out


def main():
    _, R, _ = import_reference()
    from umi import metrics
    rng = np.random.default_rng(20261020)
    store, names = {}, []
    for name, (x, t) in cases(rng).items():
        K = x.shape[1]
        pred = torch.from_numpy(x)
        mask = torch.argmax(pred, dim=1)
        onehot = F.one_hot(mask, K).movedim(-1, 1).float()
        ref = R.DiceLoss(K)(onehot, torch.from_numpy(t), softmax=False)
        ref = np.float32(float(ref))
        counts = metrics.confusion_numpy(x, t)
        assert counts.sum() == t.size and counts.max() < (1 << 24), (name, counts.max())
        assert np.array_equal(counts[0].sum(axis=0)[:K], np.bincount(mask.numpy().ravel(), minlength=K)), name
        mine = metrics.scores_numpy(counts, 0)[0]
        assert abs(float(mine) - float(ref)) <= BAR, (name, mine, ref)
        store[f"{name}_pred"], store[f"{name}_target"], store[f"{name}_dice"] = x, t, ref
        names.append(name)
        print(f"{name:28s} {tuple(x.shape)} {t.dtype} reference={ref:.8f} statement={mine:.8f} diff={float(mine) - float(ref):+.2e}")
    path = os.path.join(GOLD, "seg_metrics.npz")
    np.savez_compressed(path, cases=np.array(names), **store, **meta())
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
