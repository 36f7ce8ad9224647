#!/usr/bin/env python3
"""Generate tests/golden/binary_losses.npz by running the REFERENCE's own `calc_loss` (loss.py:442-516) on the CPU for the
losses 'dice_bce', 'Tversky', 'TopK' and 'BCE_HEM'; loss and d loss / d pred come from the reference's autograd.

Binary cases are (B, 1, H, W) fp32 logits with (B, H, W) fp32 targets and run all four losses ('BCE_HEM' only where
N = B*H*W >= 500: below that the reference's torch.topk raises).  Multi-class cases are (B, C, H, W) logits with (B, H, W)
labels and run 'Tversky'.  For the selection losses the generator redraws a case until the k-th and (k+1)-th keys of the
reference (true-class probability for TopK, per-pixel BCE for BCE_HEM) are clearly apart, so the selected set does not
depend on how a platform rounds the last bits of the key.

Stored: `entries` ("<case>:<loss>"), `cases`, <case>_pred, <case>_target, <case>:<loss>_loss, <case>:<loss>_grad.

Usage:  python tools/gen_golden_binary_losses.py
"""
import os
import sys

sys.dont_write_bytecode = True

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tools.gen_golden import GOLD, import_reference, meta  # noqa: E402

BINARY = ("dice_bce", "Tversky", "TopK", "BCE_HEM")
REL_GAP = 1e-5


def selection_keys(x, t, loss_type):
    """The reference's own selection keys (float32, CPU), k, and whether the k largest are taken."""
    p = torch.from_numpy(x).reshape(-1)
    tt = torch.from_numpy(t).reshape(-1)
    if loss_type == "TopK":
        fg = torch.sigmoid(p)
        key = torch.where(tt.long() == 1, fg, 1 - fg)
        return key.numpy(), len(tt) // 2, False
    return F.binary_cross_entropy_with_logits(p, tt, reduction="none").numpy(), 500, True


def clear_gap(x, t):
    for lt in ("TopK", "BCE_HEM"):
        key, k, largest = selection_keys(x, t, lt)
        if k >= len(key):
            continue
        s = np.sort(key.astype(np.float64))
        if largest:
            s = s[::-1]
        a, b = s[k - 1], s[k]
        if abs(a - b) <= REL_GAP * max(abs(a), abs(b)) + 1e-30:
            return False
    return True


def binary_cases(rng):
    def logits(shape, scale=3.0):
        return (rng.standard_normal(shape) * scale).astype(np.float32)

    def mask(shape, density):
        return (rng.random(shape) < density).astype(np.float32)

    def saturated(shape):
        # 30 % confidently right, 20 % confidently wrong (|x| in 30..50), the rest moderate: the TopK and BCE_HEM thresholds
        # fall inside the non-saturated part
        t = mask(shape, 0.5)[:, 0]
        sign = np.where(t > 0, 1.0, -1.0)
        u = rng.random(t.shape)
        mag = rng.uniform(30.0, 50.0, t.shape)
        x = np.where(u < 0.3, sign * mag, np.where(u < 0.5, -sign * mag, rng.standard_normal(t.shape) * 2.0))[:, None]
        return x.astype(np.float32), t

    makers = {
        "odd_b3_37x53": lambda: (logits((3, 1, 37, 53)), mask((3, 37, 53), 0.4)),              # N = 5883, odd
        "odd_b1_25x41": lambda: (logits((1, 1, 25, 41)), mask((1, 25, 41), 0.3)),              # N = 1025, odd
        "b2_48x64": lambda: (logits((2, 1, 48, 64), 2.0), mask((2, 48, 64), 0.2)),
        "target_all_zero": lambda: (logits((2, 1, 24, 40)), np.zeros((2, 24, 40), np.float32)),
        "target_all_one": lambda: (logits((2, 1, 24, 40)), np.ones((2, 24, 40), np.float32)),
        "soft_targets": lambda: (logits((2, 1, 32, 33)), rng.uniform(0.0, 0.999, (2, 32, 33)).astype(np.float32)),
        "saturated": lambda: saturated((2, 1, 40, 40)),
        "near_zero_logits": lambda: (logits((1, 1, 9, 13), 0.05), mask((1, 9, 13), 0.5)),     # N = 117 < 500
        "hem_exactly_500": lambda: (logits((2, 1, 10, 25)), mask((2, 10, 25), 0.5)),          # BCE_HEM takes all 500
    }
    out = {}
    for name, make in makers.items():
        for _ in range(100):
            x, t = make()
            if clear_gap(x, t):
                break
        else:
            raise RuntimeError(f"{name}: no draw with a clear selection gap")
        out[name] = (x, t)
    return out


def multiclass_cases(rng):
    out = {}
    x = (rng.standard_normal((2, 3, 20, 30)) * 2.0).astype(np.float32)
    out["mc3_float_labels"] = (x, rng.integers(0, 3, (2, 20, 30)).astype(np.float32))
    x = (rng.standard_normal((3, 5, 17, 11)) * 2.0).astype(np.float32)
    out["mc5_int64_labels"] = (x, rng.integers(0, 5, (3, 17, 11)).astype(np.int64))
    return out


def main():
    _, R, _ = import_reference()
    rng = np.random.default_rng(20261016)
    store, entries = {}, []

    def run(name, x, t, loss_type):
        pred = torch.from_numpy(x).requires_grad_(True)
        loss = R.calc_loss(pred, torch.from_numpy(t), loss_type=loss_type)
        loss.backward()
        key = f"{name}:{loss_type}"
        entries.append(key)
        store[f"{key}_loss"] = np.float32(loss.item())
        store[f"{key}_grad"] = pred.grad.numpy().copy()
        print(f"{key:32s} {tuple(x.shape)} loss={loss.item():.7f}")

    for name, (x, t) in binary_cases(rng).items():
        store[f"{name}_pred"], store[f"{name}_target"] = x, t
        for lt in BINARY:
            if lt == "BCE_HEM" and x.size < 500:
                continue
            run(name, x, t, lt)
    for name, (x, t) in multiclass_cases(rng).items():
        store[f"{name}_pred"], store[f"{name}_target"] = x, t
        run(name, x, t, "Tversky")
    path = os.path.join(GOLD, "binary_losses.npz")
    cases = sorted({e.split(":")[0] for e in entries})
    np.savez_compressed(path, entries=np.array(entries), cases=np.array(cases), **store, **meta())
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
