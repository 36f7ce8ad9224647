"""Float64 statements of the single-channel training losses (csrc/binary_losses.hip, csrc/hausdorff_dt.hip), written from
the reference's formulas in plain torch / NumPy / SciPy with no project imports, for the tests that pin the kernels.

Each loss statement takes the fp32 inputs as given, works in float64 and returns a `Ref`: the loss, its gradient by float64
autograd of the statement itself, and the scales that the tests' bounds are written in:
    S      sum of the magnitudes of the terms that enter the loss, before any cancellation
    scale  elementwise, the same for the gradient at an upstream gradient of 1 (multiply by |g| for another one)
`Ref.coef` holds the float64 coefficients the gradient scale is built from; tests/test_loss_f64_ref.py checks that they
reproduce the autograd gradient, so that the scales describe the statement and not a second derivation."""
from collections import namedtuple

import numpy as np
import torch

Ref = namedtuple("Ref", "loss grad S scale coef")


def _leaf(x):
    return x.detach().double().clone().requires_grad_(True)


def bce_terms(x, t):
    """BCEWithLogits per element in float64: (1 - t) x - log_sigmoid(x), written as log(1 + e^x) - t x so that its autograd
    gradient is sigmoid(x) - t itself: no 1 - 1 where the sigmoid underflows, no kink of min / |.| at x = 0."""
    x, t = x.double(), t.double()
    return torch.logaddexp(x, torch.zeros_like(x)) - t * x


def dice_bce(x, t):
    """0.5 BCEWithLogits + 0.5 mean_b (1 - (2 sum_b s t + 1) / (sum_b |s| + sum_b |t| + 1)); x (B, 1, H, W), t (B, H, W)."""
    B = x.shape[0]
    xd, td = _leaf(x), t.double().reshape(B, -1)
    bce = bce_terms(xd.reshape(B, -1), td)
    s = torch.sigmoid(xd).reshape(B, -1)
    num = 2.0 * (s * td).sum(1) + 1.0
    den = (s.abs() + td.abs()).sum(1) + 1.0
    loss = 0.5 * bce.mean() + 0.5 * (1.0 - num / den).mean()
    loss.backward()
    with torch.no_grad():
        S = 0.5 * bce.abs().mean() + 0.5 * ((2.0 * (s * td).abs().sum(1) + 1.0 + den) / den).mean()
        cb = torch.full((B, 1), 0.5 / xd.numel(), dtype=torch.float64)
        c1 = (-0.5 / B * 2.0 / den)[:, None]
        c2 = (0.5 / B * num / (den * den))[:, None]
        scale = cb.abs() * (s + td.abs()) + ((c1 * td).abs() + c2.abs()) * s
    return Ref(loss.detach(), xd.grad, S, scale.reshape(x.shape), (cb, c1, c2))


def tversky_bin(x, t, a, b):
    """1 - (TP + 1) / (TP + a FP + b FN + 1) over the whole batch, TP = sum s t, FP = sum (1 - t) s, FN = sum t (1 - s)."""
    xd, td = _leaf(x), t.double().reshape(-1)
    s = torch.sigmoid(xd).reshape(-1)
    tp, fp, fn = (s * td).sum(), ((1.0 - td) * s).sum(), (td * (1.0 - s)).sum()
    n, d = tp + 1.0, tp + a * fp + b * fn + 1.0
    loss = 1.0 - n / d
    loss.backward()
    with torch.no_grad():
        atp = (s * td).abs().sum()
        S = (atp + 1.0 + abs(1.0 - a - b) * atp + a * s.sum() + b * td.abs().sum() + 1.0) / d.abs()
        one = torch.ones(1, 1, dtype=torch.float64)
        cb, c1, c2 = 0.0 * one, (-1.0 / d + n * (1.0 - a - b) / (d * d)) * one, (a * n / (d * d)) * one
        scale = ((c1 * td).abs() + c2.abs()) * s
    return Ref(loss.detach(), xd.grad, S, scale.reshape(x.shape), (cb, c1, c2))


def tversky_mc(x, labels, a, b):
    """Mean over classes of the Tversky loss of softmax(x)[:, c] against [labels == c]; x (B, C, H, W), labels (B, H, W) of
    any dtype, compared exactly: a label that equals no class counts nowhere."""
    C = x.shape[1]
    xd = _leaf(x)
    p = torch.softmax(xd, dim=1)
    onehot = torch.stack([(labels == c) for c in range(C)], dim=1).double()
    tp, ps, ts = (p * onehot).sum((0, 2, 3)), p.sum((0, 2, 3)), onehot.sum((0, 2, 3))
    n, d = tp + 1.0, tp + a * (ps - tp) + b * (ts - tp) + 1.0
    loss = (1.0 - n / d).mean()
    loss.backward()
    with torch.no_grad():
        S = ((tp + 1.0 + abs(1.0 - a - b) * tp + a * ps + b * ts + 1.0) / d.abs()).mean()
        c1 = ((-1.0 / d + n * (1.0 - a - b) / (d * d)) / C).view(1, C, 1, 1)
        c2 = (a * n / (d * d) / C).view(1, C, 1, 1)
        h = c1 * onehot + c2                             # d loss / d p_c; d loss / d x_c = p_c (h_c - sum_k h_k p_k)
        scale = p * (h.abs() + (h.abs() * p).sum(1, keepdim=True))
    return Ref(loss.detach(), xd.grad, S, scale, (c1, c2))


def selection_keys(x, t, mode):
    """Float64 rank keys of the selection, smaller = taken first.  mode 0 ('TopK'): the true-class probability, sigmoid(x)
    where trunc(t) == 1 and 1 - sigmoid(x) otherwise.  mode 1 ('BCE_HEM'): minus the BCE term."""
    x, t = x.double().reshape(-1), t.double().reshape(-1)
    if mode == 0:
        p = torch.sigmoid(x)
        return torch.where(torch.trunc(t) == 1.0, p, torch.sigmoid(-x))
    return -bce_terms(x, t)


def selected_mean(x, t, idx):
    """Mean BCE over the flat indices `idx` (the loss of TopK / BCE_HEM once the set is known) and its gradient."""
    xd, td = _leaf(x), t.double().reshape(-1)
    k = len(idx)
    idx = torch.as_tensor(np.asarray(idx), dtype=torch.long)
    terms = bce_terms(xd.reshape(-1), td)[idx]
    loss = terms.mean()
    loss.backward()
    with torch.no_grad():
        inside = torch.zeros(td.numel(), dtype=torch.float64)
        inside[idx] = 1.0
        scale = inside * (torch.sigmoid(xd).reshape(-1) + td.abs()) / k
    return Ref(loss.detach(), xd.grad, terms.detach().abs().mean(), scale.reshape(x.shape), None)


def edt_fields(mask):
    """The reference's `distance_field` on (B, 1, H, W): per image edt(fg) + edt(~fg) of the (1, H, W) slice fg = img > 0.5,
    by scipy.ndimage.distance_transform_edt; an image without foreground stays 0.  (An all-foreground slice is measured by
    SciPy from a virtual zero at index -1 of the size-1 axis: sqrt(1 + h^2 + w^2).)  float32, as the reference's field is."""
    from scipy.ndimage import distance_transform_edt as edt
    img = np.asarray(mask)
    field = np.zeros(img.shape, dtype=np.float32)
    for b in range(len(img)):
        fg = img[b] > 0.5
        if fg.any():
            field[b] = edt(fg) + edt(~fg)
    return field


def hdt(x, t, alpha, pred_field, target_field):
    """mean((sigmoid(x) - t)^2 D), D = pred_field^alpha + target_field^alpha with the given fp32 fields as constants."""
    xd, td = _leaf(x), t.double()
    D = torch.as_tensor(pred_field).double() ** alpha + torch.as_tensor(target_field).double() ** alpha
    s = torch.sigmoid(xd)
    loss = ((s - td) ** 2 * D).mean()
    loss.backward()
    with torch.no_grad():
        S = ((s + td.abs()) ** 2 * D).mean()
        scale = D * 2.0 * (s + td.abs()) * s / xd.numel()
    return Ref(loss.detach(), xd.grad, S, scale, D)
