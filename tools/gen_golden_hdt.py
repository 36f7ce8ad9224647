#!/usr/bin/env python3
"""Generate tests/golden/hausdorff_dt.npz by running the REFERENCE's HausdorffDTLoss (loss.py:146-212) on the CPU.

The fields come from the reference's own `HausdorffDTLoss.distance_field` (scipy's distance_transform_edt).  Its
`forward` moves the distance to "cuda:0" (loss.py:189), so the three lines after the fields are restated here on the
CPU, with the reference's own alpha; loss and d loss / d pred come from autograd.  Logits keep |x| >= 1e-3, so the
foreground mask sigmoid(x) > 0.5 does not depend on how a platform rounds exp near 0.

Each case <name> stores <name>_pred, <name>_target (B, 1, H, W), <name>_pred_dt, <name>_target_dt (the fields),
<name>_loss and <name>_grad; `cases` lists the names.

Usage:  python tools/gen_golden_hdt.py
"""
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools.gen_golden import GOLD, import_reference, meta  # noqa: E402


def _logits(rng, shape, scale=3.0, shift=0.0):
    x = (rng.standard_normal(shape) * scale + shift).astype(np.float32)
    return np.where(np.abs(x) < 1e-3, np.float32(1e-3), x).astype(np.float32)


def _blobs(rng, B, H, W, density):
    """Smooth random shapes: box-blurred noise thresholded at the `density` quantile."""
    n = rng.standard_normal((B, 1, H + 8, W + 8))
    for ax in (2, 3):
        n = sum(np.roll(n, s, axis=ax) for s in range(-4, 5))
    n = n[:, :, 4:4 + H, 4:4 + W]
    return (n > np.quantile(n, 1 - density)).astype(np.float32)


def cases(rng):
    out = {}

    def rand_mask(B, H, W, density):
        return (rng.random((B, 1, H, W)) < density).astype(np.float32)

    out["dense_48"] = (_logits(rng, (2, 1, 48, 48)), rand_mask(2, 48, 48, 0.5))
    out["sparse_64"] = (_logits(rng, (2, 1, 64, 64), shift=-4.0), rand_mask(2, 64, 64, 0.03))
    t = np.concatenate([rand_mask(1, 37, 53, d) for d in (0.1, 0.5, 0.9)])
    out["odd_37x53"] = (_logits(rng, (3, 1, 37, 53)), t)
    out["wide_64x200"] = (_logits(rng, (2, 1, 64, 200)), _blobs(rng, 2, 64, 200, 0.3))
    out["tall_200x17"] = (_logits(rng, (1, 1, 200, 17)), rand_mask(1, 200, 17, 0.2))
    x = np.full((1, 1, 32, 32), -2.0, np.float32)
    x[0, 0, 5, 27] = 2.0
    t = np.zeros((1, 1, 32, 32), np.float32)
    t[0, 0, 20, 3] = 1.0
    out["single_pixel"] = (x, t)
    out["pred_all_fg"] = (np.abs(_logits(rng, (2, 1, 40, 24))), rand_mask(2, 40, 24, 0.4))
    out["pred_all_bg"] = (-np.abs(_logits(rng, (2, 1, 40, 24))), rand_mask(2, 40, 24, 0.4))
    t = rand_mask(2, 33, 33, 0.3)
    t[1] = 0.0
    out["target_empty_one"] = (_logits(rng, (2, 1, 33, 33)), t)
    t = rand_mask(2, 20, 30, 0.3)
    t[0] = 1.0
    out["target_all_fg_one"] = (_logits(rng, (2, 1, 20, 30)), t)
    out["one_by_one"] = (np.array([[[[0.7]]], [[[-0.7]]]], np.float32), np.array([[[[1.0]]], [[[1.0]]]], np.float32))
    out["blobs_224"] = (_logits(rng, (1, 1, 224, 224), 4.0), _blobs(rng, 1, 224, 224, 0.2))
    return out


def main():
    _, R, _ = import_reference()
    ref = R.HausdorffDTLoss()
    rng = np.random.default_rng(20261015)
    store = {}
    for name, (x, t) in cases(rng).items():
        pred = torch.from_numpy(x).requires_grad_(True)
        target = torch.from_numpy(t)
        s = torch.sigmoid(pred)
        pred_dt = torch.from_numpy(ref.distance_field(s.detach().cpu().numpy())).float()
        target_dt = torch.from_numpy(ref.distance_field(target.detach().cpu().numpy())).float()
        # reference loss.py:186-190 without the device move
        pred_error = (s - target) ** 2
        distance = pred_dt ** ref.alpha + target_dt ** ref.alpha
        loss = (pred_error * distance).mean()
        loss.backward()
        store.update({f"{name}_pred": x, f"{name}_target": t, f"{name}_pred_dt": pred_dt.numpy(),
                      f"{name}_target_dt": target_dt.numpy(), f"{name}_loss": np.float32(loss.item()),
                      f"{name}_grad": pred.grad.numpy()})
        print(f"{name:18s} {tuple(x.shape)} loss={loss.item():.6f}")
    path = os.path.join(GOLD, "hausdorff_dt.npz")
    np.savez_compressed(path, cases=np.array(sorted({k.rsplit('_', 1)[0] for k in store if k.endswith('_loss')})),
                        alpha=np.float32(ref.alpha), **store, **meta())
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
