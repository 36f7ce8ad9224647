"""Hard-mask segmentation metrics: an exact integer confusion matrix per item, and Dice / IoU / pixel error from it.

The rule.  A prediction is a class per pixel: of logits [N, C, ...] with C >= 2 the argmax over the channels as
`umi_argmax_mask` takes it (the first strict maximum wins; a NaN never wins, so a NaN in channel 0 stays), K = C classes; of
one-logit maps [N, 1, ...] the threshold of `umi_binary_mask` (1 where x >= SIGMOID_HALF_CUTOFF, i.e. where torch's fp32 sigmoid
is >= 0.5; NaN gives 0), K = 2; or a ready uint8 mask with K given, whose values >= K are "not a class".  A label is a class when
it is an integer in 0..K-1 or a float exactly equal to one of 0.0 .. K-1, else "not a class": the reference's one-hot encoder
(`input_tensor == i`, loss.py:220-226) matches such a pixel to no class, while its prediction still counts.

The layout.  counts[item] is [K+1, K+1] int64: row = the label's class, column = the predicted class, index K = "not a class"
(column K is 0 from logits).  With I_c = counts[c, c], Z_c = the column sum and Y_c = the row sum over all K+1 entries, in
float64, in this order, rounded once to float32:

    kind 0 / 'dice'   1 - (sum_{c = c0..K-1} (2 I_c + 1e-5) / (Z_c + Y_c + 1e-5)) / (K - c0), classes added in class order
    kind 1 / 'iou'    the same with (I_c + 1e-5) / (Z_c + Y_c - I_c + 1e-5)
    kind 2 / 'pixel'  1 - (sum_c I_c + 1e-5) / (sum_{rows < K} Y_c + 1e-5)

With c0 = 0 kind 0 is the reference's DiceLoss(K)(one_hot(argmax), target, softmax=False) (loss.py:228-251; score * score ==
score on a hard mask).  All three are errors: lower is better.

`confusion_numpy` / `scores_numpy` are the statement.  `confusion` / `scores` run the HIP kernels (csrc/seg_metrics.hip: one
streaming pass and one finalize, no global atomics, no host synchronisation, capturable) on the inputs they take -- contiguous fp32
device logits or a contiguous uint8 device mask with a contiguous device label map of one of the four label dtypes -- and raise on
anything else; `confusion_composite` (torch.bincount; integer scatter-adds on the device) serves CPU tensors and every other input with the same integers, and
`scores_composite` is the same float64 formula in torch, bit for bit `scores_numpy`."""
import numpy as np
import torch

SIGMOID_HALF_CUTOFF = float(np.array(0xB43FFFFE, dtype=np.uint32).view(np.float32))      # -0x1.7ffffcp-23, as umi.infer
EPS = 1e-5
KINDS = {"dice": 0, "iou": 1, "pixel": 2}
MAX_K = 8
_TARGET_DTYPES = {torch.int64: 0, torch.float32: 1, torch.uint8: 2, torch.int32: 3}


def _kind(kind):
    k = KINDS.get(kind, kind)
    if k not in (0, 1, 2) or isinstance(k, bool):
        raise ValueError(f"kind takes 0 / 'dice', 1 / 'iou' or 2 / 'pixel', not {kind!r}")
    return k


# ---- the statement (NumPy) ---------------------------------------------------------------------------------------------------

def predict_numpy(pred, K=None):
    """The predicted class per pixel and K: pred float [N, C, ...] logits, or a uint8 [N, ...] mask with K given."""
    pred = np.asarray(pred)
    if pred.dtype == np.uint8:
        if K is None:
            raise ValueError("a uint8 mask needs K")
        return np.minimum(pred, K).astype(np.int64), int(K)
    if pred.shape[1] == 1:
        with np.errstate(invalid="ignore"):
            return (pred[:, 0] >= np.float32(SIGMOID_HALF_CUTOFF)).astype(np.int64), 2
    best, cls = pred[:, 0].copy(), np.zeros(pred[:, 0].shape, np.int64)
    for c in range(1, pred.shape[1]):
        with np.errstate(invalid="ignore"):
            win = pred[:, c] > best                            # strict: the first maximum stays; a NaN on either side is False
        best[win], cls[win] = pred[:, c][win], c
    return cls, pred.shape[1]


def rows_numpy(target, K):
    """The row of every label: its class, K where it is not a class."""
    t = np.asarray(target)
    row = np.full(t.shape, K, np.int64)
    for c in range(K):
        row[t == c] = c
    return row


def confusion_numpy(pred, target, items=1, K=None):
    """[items, K+1, K+1] int64; pred and target hold `items` consecutive groups of equally many images."""
    cls, K = predict_numpy(pred, K)
    target = np.asarray(target)
    if target.ndim == cls.ndim + 1 and target.shape[1] == 1:           # binary labels [B, 1, H, W]
        target = target[:, 0]
    if target.shape != cls.shape:
        raise ValueError(f"prediction {cls.shape} and labels {target.shape} do not match")
    if items < 1 or cls.shape[0] % items:
        raise ValueError(f"{cls.shape[0]} images do not split into {items} equal groups")
    key = (rows_numpy(target, K) * (K + 1) + cls).reshape(items, -1)
    return np.stack([np.bincount(k, minlength=(K + 1) ** 2).reshape(K + 1, K + 1) for k in key]).astype(np.int64)


def scores_numpy(counts, kind, c0=0):
    """float32 [items] from int64 [items, K+1, K+1] (or one [K+1, K+1] matrix -> a float32 scalar)."""
    kind = _kind(kind)
    m = np.asarray(counts, dtype=np.int64)
    single = m.ndim == 2
    m = m[None] if single else m
    K = m.shape[-1] - 1
    if not 0 <= c0 < K:
        raise ValueError(f"c0 = {c0} outside 0..{K - 1}")
    I = np.diagonal(m, axis1=1, axis2=2).astype(np.float64)
    Z, Y = m.sum(axis=1).astype(np.float64), m.sum(axis=2).astype(np.float64)
    if kind == 2:
        inter = np.diagonal(m, axis1=1, axis2=2)[:, :K].sum(axis=1).astype(np.float64)
        labelled = m[:, :K].sum(axis=(1, 2)).astype(np.float64)
        out = 1.0 - (inter + EPS) / (labelled + EPS)
    else:
        total = np.zeros(len(m), np.float64)
        for c in range(c0, K):
            if kind == 0:
                total = total + (2.0 * I[:, c] + EPS) / (Z[:, c] + Y[:, c] + EPS)
            else:
                total = total + (I[:, c] + EPS) / (Z[:, c] + Y[:, c] - I[:, c] + EPS)
        out = 1.0 - total / float(K - c0)
    out = out.astype(np.float32)
    return out[0] if single else out


def class_scores_numpy(matrix):
    """Per-class Dice, IoU, precision and recall of one [K+1, K+1] matrix (float64 [K] each; the smoothed quotients above, and
    I / Z, I / Y with 0 / 0 = nan)."""
    m = np.asarray(matrix, dtype=np.int64)
    K = m.shape[-1] - 1
    I = np.diagonal(m)[:K].astype(np.float64)
    Z, Y = m.sum(axis=0)[:K].astype(np.float64), m.sum(axis=1)[:K].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"dice": (2.0 * I + EPS) / (Z + Y + EPS), "iou": (I + EPS) / (Z + Y - I + EPS), "precision": I / Z, "recall": I / Y}


# ---- torch composite ------------------------------------------------------------------------------------------------------------

def _squeeze_target(pred_shape, target):
    if target.dim() == len(pred_shape) + 1 and target.shape[1] == 1:
        target = target[:, 0]
    if tuple(target.shape) != tuple(pred_shape):
        raise ValueError(f"prediction {tuple(pred_shape)} and labels {tuple(target.shape)} do not match")
    return target


def predict_composite(pred, K=None):
    if pred.dtype == torch.uint8:
        if K is None:
            raise ValueError("a uint8 mask needs K")
        return pred.long().clamp(max=K), int(K)
    if pred.shape[1] == 1:
        return (pred[:, 0].float() >= SIGMOID_HALF_CUTOFF).long(), 2
    best, cls = pred[:, 0].clone(), torch.zeros(pred[:, 0].shape, dtype=torch.long, device=pred.device)
    for c in range(1, pred.shape[1]):
        win = pred[:, c] > best
        best, cls = torch.where(win, pred[:, c], best), torch.where(win, torch.full_like(cls, c), cls)
    return cls, pred.shape[1]


def confusion_composite(pred, target, items=1, K=None):
    """The same integers from torch ops (torch.bincount; on the device a scatter_add_ of ones, which -- unlike bincount -- reads
    nothing back, so the composite too can sit in a captured validation group): CPU tensors and whatever the kernel does not
    take."""
    cls, K = predict_composite(pred.detach(), K)
    target = _squeeze_target(cls.shape, target.detach())
    if items < 1 or cls.shape[0] % items:
        raise ValueError(f"{cls.shape[0]} images do not split into {items} equal groups")
    row = torch.full(cls.shape, K, dtype=torch.long, device=cls.device)
    for c in range(K):
        row = torch.where(target == c, torch.full_like(row, c), row)
    key = (row * (K + 1) + cls).reshape(items, -1)
    key = key + torch.arange(items, device=key.device).unsqueeze(1) * (K + 1) ** 2
    key, size = key.reshape(-1), items * (K + 1) ** 2
    if key.is_cuda:                     # torch.bincount reads its maximum back, which a graph capture forbids: integer adds instead
        flat = torch.zeros(size, dtype=torch.long, device=key.device).scatter_add_(0, key, torch.ones_like(key))
    else:
        flat = torch.bincount(key, minlength=size)
    return flat.reshape(items, K + 1, K + 1)


def scores_composite(counts, kind, c0=0):
    """scores_numpy in torch float64 (IEEE adds, products and quotients in the same order: the same bits)."""
    kind = _kind(kind)
    m = counts.long()
    K = m.shape[-1] - 1
    if m.dim() != 3 or m.shape[-2] != K + 1 or not 0 <= c0 < K:
        raise ValueError(f"counts {tuple(m.shape)} / c0 {c0}")
    I = torch.diagonal(m, dim1=1, dim2=2).double()
    Z, Y = m.sum(dim=1).double(), m.sum(dim=2).double()
    if kind == 2:
        inter = torch.diagonal(m, dim1=1, dim2=2)[:, :K].sum(dim=1).double()
        labelled = m[:, :K].sum(dim=(1, 2)).double()
        out = 1.0 - (inter + EPS) / (labelled + EPS)
    else:
        total = torch.zeros(m.shape[0], dtype=torch.float64, device=m.device)
        for c in range(c0, K):
            if kind == 0:
                total = total + (2.0 * I[:, c] + EPS) / (Z[:, c] + Y[:, c] + EPS)
            else:
                total = total + (I[:, c] + EPS) / (Z[:, c] + Y[:, c] - I[:, c] + EPS)
        out = 1.0 - total / float(K - c0)
    return out.float()


# ---- the kernels ------------------------------------------------------------------------------------------------------------------

def kernel_ok(pred, target, items=1, K=None):
    """Whether `confusion` takes these inputs (the same conditions as loss._fused_ok, plus the uint8-mask form)."""
    if not (torch.is_tensor(pred) and torch.is_tensor(target) and pred.is_cuda and target.is_cuda and pred.device == target.device
            and pred.is_contiguous() and target.is_contiguous() and target.dtype in _TARGET_DTYPES):
        return False
    if pred.dtype == torch.uint8:
        shape, ok = tuple(pred.shape), K is not None and 2 <= K <= MAX_K and pred.dim() >= 2
    else:
        ok = pred.dtype == torch.float32 and pred.dim() >= 3 and 1 <= pred.shape[1] <= MAX_K
        shape = (pred.shape[0],) + tuple(pred.shape[2:])
    tshape = tuple(target.shape)
    if len(tshape) == len(shape) + 1 and tshape[1] == 1:
        tshape = tshape[:1] + tshape[2:]
    if not ok or tshape != shape or items < 1 or items > 65535 or shape[0] % items or pred.numel() == 0:
        return False
    return (shape[0] // items) * int(np.prod(shape[1:])) < (1 << 31)


def confusion(pred, target, items=1, K=None):
    """Device int64 [items, K+1, K+1] of fp32 logits [items*n, C, ...] (K from C) or a uint8 mask [items*n, ...] (K given) against
    labels [items*n, ...] ([items*n, 1, ...] too): two launches, nothing read back.  Raises on inputs the kernels do not take
    (use confusion_composite for those)."""
    from . import lib as L, ops
    if not kernel_ok(pred, target, items, K):
        raise ValueError("umi.metrics.confusion takes contiguous fp32 device logits [N, C <= 8, ...] or a contiguous uint8 device mask "
                         "with K in 2..8, and contiguous device labels (int64 / float32 / uint8 / int32) of the matching shape; got "
                         f"{tuple(pred.shape)} {pred.dtype} on {pred.device} and {tuple(target.shape)} {target.dtype} on "
                         f"{target.device}")
    mask = pred.dtype == torch.uint8
    n = pred.shape[0] // items
    HW = pred[0].numel() if mask else pred[0, 0].numel()
    C = None if mask else pred.shape[1]
    K = int(K) if mask else (2 if C == 1 else C)
    counts = torch.empty((items, K + 1, K + 1), dtype=torch.int64, device=pred.device)
    ws = ops.workspace(L.fn("umi_confusion_ws_bytes")(items, n, K, HW), pred.device)
    L.call("umi_confusion_masks" if mask else "umi_confusion_logits", pred.data_ptr(), target.data_ptr(),
           _TARGET_DTYPES[target.dtype], items, n, K if mask else C, HW, counts.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
    return counts


def scores(counts, kind, c0=0):
    """float32 [items] of int64 [items, K+1, K+1]: the kernel for contiguous device counts, the torch composite otherwise."""
    kind = _kind(kind)
    if not (counts.is_cuda and counts.dtype == torch.int64 and counts.is_contiguous() and counts.dim() == 3
            and counts.shape[1] == counts.shape[2] and 3 <= counts.shape[1] <= MAX_K + 1 and counts.shape[0] > 0):
        return scores_composite(counts, kind, c0)
    from . import lib as L, ops
    out = torch.empty(counts.shape[0], dtype=torch.float32, device=counts.device)
    L.call("umi_confusion_scores", counts.data_ptr(), counts.shape[0], counts.shape[1] - 1, kind, int(c0), out.data_ptr(),
           ops._stream())
    return out


class ConfusionMeter:
    """Accumulates confusion matrices on the device: `update(pred, target)` adds the matrix of a batch (kernel or composite),
    `add(counts)` adds ready [items, K+1, K+1] or [K+1, K+1] matrices; neither synchronises.  `read()` copies the sum to the host
    once and returns {'matrix': int64 [K+1, K+1], 'dice', 'iou', 'precision', 'recall': float64 [K]}."""

    def __init__(self, K=None):
        self.K, self.total = K, None

    def add(self, counts):
        c = counts.reshape(-1, counts.shape[-2], counts.shape[-1]).sum(dim=0)
        if self.total is None:
            self.total = c.clone()
        else:
            self.total.add_(c.to(self.total.device))
        return self

    def update(self, pred, target, K=None):
        K = self.K if K is None else K
        return self.add(confusion(pred, target, 1, K) if kernel_ok(pred, target, 1, K) else confusion_composite(pred, target, 1, K))

    def reset(self):
        if self.total is not None:
            self.total.zero_()

    def read(self):
        if self.total is None:
            raise RuntimeError("ConfusionMeter.read() before the first update")
        m = self.total.cpu().numpy()
        return dict(matrix=m, **class_scores_numpy(m))
