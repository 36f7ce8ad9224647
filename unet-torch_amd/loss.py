"""Losses of the hot path: drop-in for the reference `loss.py` entry point `calc_loss`.

`calc_loss(pred, target, bce_weight=0.5, loss_type='mse')` keeps the reference signature
(loss.py:442) and the module-level `CLASS_NUMBER` that `train.py:163` sets.  The branch on
the training hot path is 'dice_bce_mc' (loss.py:488-500): 0.5*CrossEntropy + 0.5*Dice of
the softmax (DiceLoss, loss.py:215-251: per-class `1 - (2*sum(p*t)+1e-5)/(sum(p*p)+sum(t*t)+1e-5)`
over the whole batch, mean over classes).  It runs as fp32 device ops on the logits the HIP
network returns; unlike the reference it does not `.item()`-sync once per class.

'HausdorffDTLoss' (loss.py:146-212, dispatched at :508) runs on the device as HIP kernels
(csrc/hausdorff_dt.hip): the exact distance fields, D and the loss without a host round trip, so
it stays inside a captured graph.  CPU tensors use a NumPy restatement of the same separable exact
transform, bit-identical to the reference's scipy fields.

The binary-segmentation losses 'dice_bce' (loss.py:484-487), 'Tversky' (:514-515), 'TopK' (:445-446) and 'BCE_HEM'
(:447-467) run on the device as HIP kernels (csrc/binary_losses.hip) for contiguous fp32 logits of the shapes the kernels
cover: streaming statistics with fp64 fixed-order sums for dice_bce and Tversky, and an exact device radix select of the
k-th key for TopK and BCE_HEM (ties go to the lowest flat index), so no value travels to the host and a step with any of
them can be captured in a graph.  Every other input (CPU tensors, other dtypes or shapes) runs a torch composite that
restates the reference branch and raises where it raises.

`multi_task_ratio_loss(o1, o2, l1, l2, ratio_weighted)` is the step loss of the reference's count-ratio-weighted multi-task
loop (Trainer.py:1225-1249, used by Trainer.multi_task_trainRatio): per-task MSE of the ReLU'd heads, the mean absolute
error r of the per-image immune : (immune + other) count ratio, and (L1 + L2) * (1 + 10 r) when `ratio_weighted` (epoch > 5).
Contiguous fp32 device heads (B, 1, H, W) with labels (B, H, W) run two HIP kernels forward and one backward
(csrc/multitask_ratio.hip, fp64 fixed-order sums, nothing read back, so the step can be captured); every other input runs a
torch composite that restates the reference lines.

`MRAccuracy(pred, target)` is the reference's cell-count error of a batch (loss.py:422-440): threshold the one-logit map at
fp32 sigmoid >= 0.5, count the 8-connected components of every image and compare with the number of ground-truth dots.  Device
tensors run the threshold, the labelling (csrc/components.hip, a union-find in separate launches) and the dot sums as HIP kernels
and read 2 B integers (and the labelling's fault word) back once; CPU tensors run a NumPy restatement (umi/components.py).  The
component count is cv2.connectedComponents' / scipy.ndimage.label's with a full 3x3 structure; the same Python expression on the
same integers gives the reference's float.

Under `umi.ddp.GradReducer(model, world, global_batch=True)` 'dice_bce_mc' is the loss of the data-parallel group's WHOLE batch on
every rank: the float64 sums of the fused kernels (`umi_dice_ce_sums`) or of a torch composite (CPU tensors) are all-reduced with
the pixel count before the quotients are formed, and the backward is world x the gradient of that loss w.r.t. this rank's logits,
so that the averaged parameter gradients are those of the global loss.  Shards must be equal; 'Tversky', 'TopK' and 'BCE_HEM',
which couple the batch in ways this does not cover, raise NotImplementedError while the switch is on.

`calc_loss_items(pred, target, items, loss_type)` is the validation phase's form (Trainer(val_batch=k)): pred and target hold
`items` consecutive groups of n images, and element i of the [items] result is `calc_loss` of the i-th group -- by default that
very loop over contiguous slices, so every name behaves as in `calc_loss`; 'dice_bce_mc' on the fused kernels' inputs takes one
`umi_dice_ce_fwd_items` pass whose stats rows are bit for bit those of `umi_dice_ce_fwd` on the slices (values only, no backward).
It raises under an active global-batch switch.

The hard-mask metrics 'dice_err_mc', 'iou_err_mc', 'pixel_err_mc' (logits with C >= 2 channels, the argmax mask, all classes),
'dice_err', 'iou_err' (one logit, the fp32 sigmoid >= 0.5 mask, the foreground class alone) and 'pixel_err' (one logit, both
classes) are values for `accuracy_metric`, not losses: 1 - Dice / 1 - IoU / 1 - pixel accuracy of the hard mask from an exact
integer confusion matrix (umi/metrics.py states the rule), lower is better, returned without a graph.  Contiguous fp32 device
logits with contiguous device labels run two HIP kernels and a scoring kernel (csrc/seg_metrics.hip; `calc_loss_items` counts all
items in one pass), everything else a torch.bincount composite with the same integers and the same float64 formula.
`METRICS_KERNEL = False` sends every input to the composite (the A/B switch of tools/bench_seg_metrics.py).  Under a
global-batch switch they stay per replica, like the pointwise losses.

The surface-distance metrics 'hd_mc', 'hd95_mc', 'assd_mc' (logits with C >= 2 channels, the argmax mask, K = C) and 'hd',
'hd95', 'assd' (one logit, the fp32 sigmoid >= 0.5 mask, K = 2) are values for `accuracy_metric` too: the Hausdorff distance, its
95th percentile and the average symmetric surface distance between the boundaries of the predicted and the true mask, in pixels,
per image and FOREGROUND class (c0 = 1, as TransUNet's evaluation averages them), averaged over the item's images and classes
(umi/surface.py states the rule; it is medpy's / scipy's for unit spacing).  Lower is better; returned without a graph, fp32.
Logits must be 4-D; binary labels may be (B, H, W) or (B, 1, H, W).  An (image, class) with one empty mask scores by the
module-level `SURFACE_EMPTY`: 'diagonal' (default: the image diagonal, so an empty prediction is never the best model), 'zero'
(TransUNet's script) or 'nan'.  Contiguous fp32 device logits with contiguous device labels run `umi_argmax_mask` /
`umi_binary_mask` and the HIP kernels of csrc/surface_metrics.hip (one call for all items of `calc_loss_items`, capturable);
everything else -- logits with MORE THAN 8 CHANNELS (the 9-class Synapse TransUNet among them), other dtypes, non-contiguous tensors,
H or W > 4096, and every input under `METRICS_KERNEL = False` -- runs the NumPy statement on host copies: about 65 ms per 512 x 512
image and class instead of microseconds, synchronising and therefore not capturable; on device logits it warns once
(RuntimeWarning), `surface_host_calls()` counts it, and the Trainer keeps such validation groups eager.
Under a global-batch switch they stay per replica.

The remaining names raise NotImplementedError: 'dice', 'dice_score', 'dice_score_mc' and 'log_cosh_dice_loss' call
DiceLoss() without n_classes, 'FL' names an undefined BinaryFocalLoss, HausdorffERLoss has no gradient and
ActiveContourLoss hard-codes 512x512 tensors on cuda:0 in the reference itself.
"""
import warnings

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

CLASS_NUMBER = 2      # overwritten by the caller, as train.py:163 does for the reference


class DiceLoss(nn.Module):
    """Multi-class soft Dice on probabilities (reference loss.py:215-251)."""

    def __init__(self, n_classes):
        super().__init__()
        self.n_classes = n_classes

    def forward(self, inputs, target, weight=None, softmax=False):
        if softmax:
            inputs = torch.softmax(inputs, dim=1)
        if weight is None:
            weight = [1] * self.n_classes
        if inputs.shape[1] != self.n_classes or inputs.shape[0] != target.shape[0] \
                or inputs.shape[2:] != target.shape[1:]:
            raise AssertionError(f"predict {tuple(inputs.shape)} & target {tuple(target.shape)} shape do not match")
        total = 0.0
        for c in range(self.n_classes):
            t = (target == c).float()
            p = inputs[:, c]
            dice = (2 * torch.sum(p * t) + 1e-5) / (torch.sum(p * p) + torch.sum(t * t) + 1e-5)
            total = total + (1 - dice) * weight[c]
        return total / self.n_classes


_OUT_OF_SCOPE = {"FL", "dice", "dice_score", "log_cosh_dice_loss", "dice_score_mc", "HausdorffERLoss", "ActiveContourLoss"}


_TARGET_DTYPES = {torch.int64: 0, torch.float32: 1, torch.uint8: 2, torch.int32: 3}


class _FusedDiceCE(torch.autograd.Function):
    """'dice_bce_mc' on device logits as two streaming libunetmi kernels per direction (csrc/loss_kernels.hip) instead of
    ~25 elementwise / reduction launches; same arithmetic as the composite below (fp64 final sums, deterministic)."""

    @staticmethod
    def forward(ctx, pred, target):
        from umi import lib as L, ops
        N, C = pred.shape[0], pred.shape[1]
        HW = pred[0, 0].numel()
        stats = torch.empty(3 * C + 2, dtype=torch.float32, device=pred.device)
        ws = ops.workspace(L.fn("umi_dice_ce_ws_bytes")(N, C, HW), pred.device)
        L.call("umi_dice_ce_fwd", pred.data_ptr(), target.data_ptr(), _TARGET_DTYPES[target.dtype], N, C, HW,
               stats.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
        ctx.save_for_backward(pred, target, stats)
        return stats[3 * C + 1].clone()

    @staticmethod
    def backward(ctx, gout):
        from umi import lib as L, ops
        pred, target, stats = ctx.saved_tensors
        N, C = pred.shape[0], pred.shape[1]
        HW = pred[0, 0].numel()
        g = gout.detach().to(torch.float32).contiguous()
        dl = torch.empty_like(pred)
        L.call("umi_dice_ce_bwd", pred.data_ptr(), target.data_ptr(), _TARGET_DTYPES[target.dtype], stats.data_ptr(),
               g.data_ptr(), N, C, HW, dl.data_ptr(), ops._stream())
        return dl, None


class _FusedDiceCEGlobal(torch.autograd.Function):
    """'dice_bce_mc' of a data-parallel group's whole batch (umi.ddp.GradReducer(global_batch=True)): this rank's float64 sums,
    one all-reduce of [sums | pixel count], the loss from the global sums; the backward is world x the gradient of that loss
    w.r.t. this rank's logits, so that the averaged parameter gradients are those of the global loss."""

    @staticmethod
    def forward(ctx, pred, target, sync):
        from umi import lib as L, ops
        N, C = pred.shape[0], pred.shape[1]
        HW = pred[0, 0].numel()
        sums = torch.full((3 * C + 2,), float(N * HW), dtype=torch.float64, device=pred.device)     # [A | B | T | CE sum | count]
        stats = torch.empty(3 * C + 2, dtype=torch.float32, device=pred.device)
        ws = ops.workspace(L.fn("umi_dice_ce_ws_bytes")(N, C, HW), pred.device)
        L.call("umi_dice_ce_sums", pred.data_ptr(), target.data_ptr(), _TARGET_DTYPES[target.dtype], N, C, HW,
               sums.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
        ctx.count = sync.reduce_counted(sums, N * HW)
        ctx.world = sync.world
        L.call("umi_dice_ce_finalize", sums.data_ptr(), C, float(ctx.count), stats.data_ptr(), ops._stream())
        ctx.save_for_backward(pred, target, stats)
        return stats[3 * C + 1].clone()

    @staticmethod
    def backward(ctx, gout):
        from umi import lib as L, ops
        pred, target, stats = ctx.saved_tensors
        N, C = pred.shape[0], pred.shape[1]
        HW = pred[0, 0].numel()
        g = gout.detach().to(torch.float32).contiguous()
        dl = torch.empty_like(pred)
        L.call("umi_dice_ce_bwd_global", pred.data_ptr(), target.data_ptr(), _TARGET_DTYPES[target.dtype], stats.data_ptr(),
               g.data_ptr(), float(ctx.world), float(ctx.count), N, C, HW, dl.data_ptr(), ops._stream())
        return dl, None, None


def dice_bce_mc_global_composite(pred, target, sync):
    """The same loss as torch ops (CPU tensors, any float dtype): the sums of `DiceLoss` and of the cross entropy are added over
    the group before the quotients are formed.  Value: the global loss.  Gradient: world x d(global loss) / d(local logits)."""
    C = CLASS_NUMBER
    if pred.shape[1] != C or pred.shape[0] != target.shape[0] or pred.shape[2:] != target.shape[1:]:
        raise AssertionError(f"predict {tuple(pred.shape)} & target {tuple(target.shape)} shape do not match")
    t = target.long()
    p = torch.softmax(pred, dim=1)
    onehot = F.one_hot(t, C).movedim(-1, 1).to(pred.dtype)
    dims = [0] + list(range(2, pred.dim()))
    count = t.numel()
    local = torch.cat([(p * onehot).sum(dims), (p * p).sum(dims), onehot.sum(dims),
                       F.cross_entropy(pred, t, reduction="sum").reshape(1), pred.new_full((1,), float(count))])
    total = sync.all_reduce(local.detach().clone())
    count = sync.check_count(total[-1], count)
    # value = the all-reduced sums; derivative = world x d/d(local sums): every rank's sums enter the global ones with weight 1
    S = total + sync.world * (local - local.detach())
    A, B, T, ce = S[:C], S[C:2 * C], S[2 * C:3 * C], S[3 * C]
    dice = (1 - (2 * A + 1e-5) / (B + T + 1e-5)).sum() / C
    return 0.5 * ce / count + 0.5 * dice


def _batch_sync():
    from umi import ddp
    return ddp.active_batch_sync()


_BATCH_COUPLED = {"Tversky", "TopK", "BCE_HEM"}


def _fused_ok(pred, target):
    return (pred.is_cuda and pred.dtype == torch.float32 and pred.dim() >= 3 and pred.is_contiguous() and pred.shape[1] <= 8
            and pred.shape[1] == CLASS_NUMBER and target.is_cuda and target.is_contiguous() and target.dtype in _TARGET_DTYPES
            and target.shape[0] == pred.shape[0] and tuple(target.shape[1:]) == tuple(pred.shape[2:]))


# ---------------------------------------------------------------------------------------------------------------------
# HausdorffDTLoss (reference loss.py:146-212)

_BIG = 1 << 20         # row-index sentinel of "no pixel of that class in this column" (H <= 4096 << _BIG)
_INF = 1 << 40         # squared-distance infinity


def _col_sq(mask):
    """Squared distance of every pixel of `mask` (H, W) to the nearest True pixel of its own column, _INF if none."""
    H = mask.shape[0]
    r = np.arange(H, dtype=np.int64)[:, None]
    above = np.maximum.accumulate(np.where(mask, r, -_BIG), axis=0)
    below = np.minimum.accumulate(np.where(mask, r, _BIG)[::-1], axis=0)[::-1]
    d = np.minimum(r - above, below - r)
    return np.where(d > H, _INF, d * d)


def _row_min(g2):
    """Exact min over w' of g2[h, w'] + (w - w')^2 per row, searched outward: a column k away adds k^2, so the search
    stops once k^2 reaches the largest current minimum (the kernel's hdt_row_d2, vectorised over the image)."""
    best = g2.copy()
    W = g2.shape[1]
    for k in range(1, W):
        kk = k * k
        if kk >= best.max():
            break
        np.minimum(best[:, k:], g2[:, :-k] + kk, out=best[:, k:])
        np.minimum(best[:, :-k], g2[:, k:] + kk, out=best[:, :-k])
    return best


def _distance_field(img):
    """The reference's `HausdorffDTLoss.distance_field` on (B, 1, H, W) float32: per image, the Euclidean distance of
    every pixel to the nearest pixel of the other class of img > 0.5 -- edt(fg) + edt(~fg) -- zero if the image has no
    foreground, sqrt(1 + h^2 + w^2) if it has no background (scipy's edt of an all-ones (1, H, W) slice).  Squared
    distances are exact integers; the float64 root cast to float32 is scipy's value bit for bit."""
    field = np.zeros(img.shape, dtype=np.float32)
    for b in range(len(img)):
        fg = img[b, 0] > 0.5
        if not fg.any():
            continue
        if fg.all():
            h, w = np.mgrid[0:fg.shape[0], 0:fg.shape[1]]
            d2 = 1 + h.astype(np.int64) ** 2 + w.astype(np.int64) ** 2
        else:
            d2 = np.where(fg, _row_min(_col_sq(~fg)), _row_min(_col_sq(fg)))
        field[b, 0] = np.sqrt(d2.astype(np.float64)).astype(np.float32)
    return field


def _hdt_check(pred, target):
    if pred.dim() != 4 or tuple(pred.shape) != tuple(target.shape) or pred.shape[1] != 1:
        raise NotImplementedError(f"HausdorffDTLoss supports pred and target of one shape (B, 1, H, W); got pred "
                                  f"{tuple(pred.shape)} and target {tuple(target.shape)}")


class _HausdorffDT(torch.autograd.Function):
    """HausdorffDTLoss on device tensors: csrc/hausdorff_dt.hip computes the fields, D and the loss (forward) and
    d loss / d pred (backward); D is kept for the backward, the fields only when asked for (debug)."""

    @staticmethod
    def forward(ctx, pred, target, alpha, fields):
        from umi import lib as L, ops
        B, C, H, W = pred.shape
        D = torch.empty_like(pred)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        ws = ops.workspace(L.fn("umi_hdt_ws_bytes")(B, H, W), pred.device)
        L.call("umi_hdt_fwd", pred.data_ptr(), target.data_ptr(), B, C, H, W, alpha, D.data_ptr(),
               None if fields is None else fields.data_ptr(), loss.data_ptr(), ws.data_ptr(),
               ws.numel(), ops._stream())
        ctx.save_for_backward(pred, target, D)
        ctx.mark_non_differentiable(D)
        return loss, D

    @staticmethod
    def backward(ctx, gout, _gD):
        from umi import lib as L, ops
        pred, target, D = ctx.saved_tensors
        B, C, H, W = pred.shape
        g = gout.detach().to(torch.float32).contiguous()
        dpred = torch.empty_like(pred)
        L.call("umi_hdt_bwd", pred.data_ptr(), target.data_ptr(), D.data_ptr(), g.data_ptr(), B, C, H, W,
               dpred.data_ptr(), ops._stream())
        return dpred, None, None, None


class HausdorffDTLoss(nn.Module):
    """Binary Hausdorff loss based on distance transform (reference loss.py:146-212): loss = mean((s - t)^2 * D),
    s = sigmoid(pred), D = field(s)^alpha + field(target)^alpha.  pred, target: (B, 1, H, W).  The target is a label and
    gets no gradient."""

    def __init__(self, alpha=0.2, **kwargs):
        super().__init__()
        self.alpha = alpha

    @torch.no_grad()
    def distance_field(self, img: np.ndarray) -> np.ndarray:
        return _distance_field(img)

    def forward(self, pred, target, debug=False):
        _hdt_check(pred, target)
        if pred.is_cuda:
            if pred.dtype != torch.float32:
                raise NotImplementedError(f"HausdorffDTLoss on the device takes fp32 logits, got {pred.dtype}")
            pred = pred.contiguous()
            target = target.to(device=pred.device, dtype=torch.float32).contiguous()
            fields = torch.empty((2,) + tuple(pred.shape), dtype=torch.float32, device=pred.device) if debug else None
            loss, distance = _HausdorffDT.apply(pred, target, float(self.alpha), fields)
            if not debug:
                return loss
            s = torch.sigmoid(pred)
            pred_error = (s - target) ** 2
            pred_dt, target_dt = fields[0], fields[1]
        else:
            s = torch.sigmoid(pred)
            pred_dt = torch.from_numpy(self.distance_field(s.detach().cpu().numpy())).float()
            target_dt = torch.from_numpy(self.distance_field(target.detach().cpu().float().numpy())).float()
            pred_error = (s - target) ** 2
            distance = pred_dt ** self.alpha + target_dt ** self.alpha
            loss = (pred_error * distance).mean()
            if not debug:
                return loss
        dt_field = pred_error * distance
        return (loss.detach().cpu().numpy(),
                (dt_field.detach().cpu().numpy()[0, 0], pred_error.detach().cpu().numpy()[0, 0],
                 distance.cpu().numpy()[0, 0], pred_dt.cpu().numpy()[0, 0], target_dt.cpu().numpy()[0, 0]))


# ---------------------------------------------------------------------------------------------------------------------
# dice_bce, Tversky, TopK, BCE_HEM (reference loss.py:254-307, 344-420, 442-516)

TVERSKY_ALPHA, TVERSKY_BETA = 0.4, 0.6     # calc_loss's FocalTverskyLoss(alpha=0.4, beta=0.6), gamma 1, smooth 1
BCE_HEM_K = 500
_TOPK, _BCE_HEM = 0, 1


def _flatten(pred, target):
    """The reference's `flatten` (loss.py:344-352): (B, C, H, W) -> (B*H*W, C), target -> (B*H*W,)."""
    return pred.permute(0, 2, 3, 1).contiguous().view(-1, pred.size(1)), target.view(-1)


def _binary_dice(pred, target):
    """BinaryDiceLoss() (loss.py:254-307) on logits: per-image 1 - (2 sum(s t) + 1) / (sum(|s| + |t|) + 1), mean."""
    s = torch.sigmoid(pred)
    s = s.contiguous().view(s.shape[0], -1)
    t = target.contiguous().view(target.shape[0], -1).float()
    num = 2 * torch.sum(torch.mul(s, t), dim=1) + 1
    den = torch.sum(s.abs() + t.abs(), dim=1) + 1
    return (1 - num / den).mean()


def dice_bce_composite(pred, target):
    p = pred.squeeze(1)
    return 0.5 * F.binary_cross_entropy_with_logits(p, target) + 0.5 * _binary_dice(p, target)


def tversky_composite(pred, target, alpha=TVERSKY_ALPHA, beta=TVERSKY_BETA, smooth=1.0):
    pred, target = _flatten(pred, target)
    if pred.size(1) == 1:
        p = torch.sigmoid(pred[:, 0])
        t_p = (p * target).sum()
        f_p = ((1 - target) * p).sum()
        f_n = (target * (1 - p)).sum()
        return 1 - (t_p + smooth) / (t_p + alpha * f_p + beta * f_n + smooth)
    p = F.softmax(pred, dim=1)
    losses = []
    for c in range(pred.size(1)):
        t_c = (target == c).float()
        p_c = p[:, c]
        t_p = (p_c * t_c).sum()
        f_p = ((1 - t_c) * p_c).sum()
        f_n = (t_c * (1 - p_c)).sum()
        losses.append(1 - (t_p + smooth) / (t_p + alpha * f_p + beta * f_n + smooth))
    return torch.stack(losses).mean()


def topk_composite(pred, target):
    pred, target = _flatten(pred, target)
    p = pred[:, 0]
    fg = torch.sigmoid(p)
    prob = torch.gather(torch.stack((1 - fg, fg), dim=1), 1, target.unsqueeze(1).long())[:, 0]
    _, idx = torch.topk(prob, len(target) // 2, largest=False)
    ce = F.binary_cross_entropy_with_logits(p, target, reduction='none')
    mask = torch.zeros_like(ce)
    mask[idx] = 1
    return ce[mask > 0].mean()


def bce_hem_composite(pred, target):
    loss_f = F.binary_cross_entropy_with_logits(pred.squeeze(1), target, reduction='none').flatten()
    _, idx = torch.topk(loss_f, BCE_HEM_K)
    mask = torch.zeros_like(loss_f)
    mask[idx] = 1
    return (loss_f * mask).sum() / mask.sum()


class _DiceBCE(torch.autograd.Function):
    """'dice_bce' on (B, 1, H, W) fp32 device logits: umi_dice_bce_fwd / _bwd; the fp64 per-image stats are saved."""

    @staticmethod
    def forward(ctx, pred, target):
        from umi import lib as L, ops
        B, HW = pred.shape[0], pred[0, 0].numel()
        stats = torch.empty(5 * B, dtype=torch.float64, device=pred.device)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        ws = ops.workspace(L.fn("umi_binloss_ws_bytes")(B, 1, HW), pred.device)
        L.call("umi_dice_bce_fwd", pred.data_ptr(), target.data_ptr(), B, HW, stats.data_ptr(), loss.data_ptr(),
               ws.data_ptr(), ws.numel(), ops._stream())
        ctx.save_for_backward(pred, target, stats)
        return loss

    @staticmethod
    def backward(ctx, gout):
        from umi import lib as L, ops
        pred, target, stats = ctx.saved_tensors
        g = gout.detach().to(torch.float32).contiguous()
        dpred = torch.empty_like(pred)
        L.call("umi_dice_bce_bwd", pred.data_ptr(), target.data_ptr(), stats.data_ptr(), g.data_ptr(), pred.shape[0],
               pred[0, 0].numel(), dpred.data_ptr(), ops._stream())
        return dpred, None


class _Tversky(torch.autograd.Function):
    """'Tversky' on (B, C, H, W) fp32 device logits, C <= 8: umi_tversky_fwd / _bwd; the fp64 stats are saved."""

    @staticmethod
    def forward(ctx, pred, target, alpha, beta):
        from umi import lib as L, ops
        B, C, HW = pred.shape[0], pred.shape[1], pred[0, 0].numel()
        stats = torch.empty(5 * B if C == 1 else 3 * C, dtype=torch.float64, device=pred.device)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        ws = ops.workspace(L.fn("umi_binloss_ws_bytes")(B, C, HW), pred.device)
        L.call("umi_tversky_fwd", pred.data_ptr(), target.data_ptr(), _TARGET_DTYPES[target.dtype], B, C, HW, alpha,
               beta, stats.data_ptr(), loss.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
        ctx.save_for_backward(pred, target, stats)
        ctx.ab = (alpha, beta)
        return loss

    @staticmethod
    def backward(ctx, gout):
        from umi import lib as L, ops
        pred, target, stats = ctx.saved_tensors
        B, C, HW = pred.shape[0], pred.shape[1], pred[0, 0].numel()
        g = gout.detach().to(torch.float32).contiguous()
        dpred = torch.empty_like(pred)
        L.call("umi_tversky_bwd", pred.data_ptr(), target.data_ptr(), _TARGET_DTYPES[target.dtype], stats.data_ptr(),
               g.data_ptr(), B, C, HW, ctx.ab[0], ctx.ab[1], dpred.data_ptr(), ops._stream())
        return dpred, None, None, None


class _TopKBCE(torch.autograd.Function):
    """'TopK' (mode 0) and 'BCE_HEM' (mode 1) on (B, 1, H, W) fp32 device logits: umi_topk_loss_fwd selects the k pixels
    on the device and writes their mask, which is saved for umi_topk_loss_bwd."""

    @staticmethod
    def forward(ctx, pred, target, k, mode):
        from umi import lib as L, ops
        N = pred.numel()
        mask = torch.empty(N, dtype=torch.uint8, device=pred.device)
        loss = torch.empty((), dtype=torch.float32, device=pred.device)
        ws = ops.workspace(L.fn("umi_topk_loss_ws_bytes")(N), pred.device)
        L.call("umi_topk_loss_fwd", pred.data_ptr(), target.data_ptr(), N, k, mode, mask.data_ptr(), loss.data_ptr(),
               ws.data_ptr(), ws.numel(), ops._stream())
        ctx.save_for_backward(pred, target, mask)
        ctx.k = k
        return loss

    @staticmethod
    def backward(ctx, gout):
        from umi import lib as L, ops
        pred, target, mask = ctx.saved_tensors
        g = gout.detach().to(torch.float32).contiguous()
        dpred = torch.empty_like(pred)
        L.call("umi_topk_loss_bwd", pred.data_ptr(), target.data_ptr(), mask.data_ptr(), g.data_ptr(), pred.numel(),
               ctx.k, dpred.data_ptr(), ops._stream())
        return dpred, None, None, None


def _device_logits(pred, max_c):
    return (pred.is_cuda and pred.dtype == torch.float32 and pred.dim() == 4 and pred.is_contiguous()
            and 1 <= pred.shape[1] <= max_c and 0 < pred.numel() < (1 << 31))


def _binary_target_ok(pred, target, exact_shape):
    """fp32 contiguous device target of B*H*W elements; `exact_shape`: (B, H, W), as BCEWithLogits(pred.squeeze(1), t) needs."""
    if not (_device_logits(pred, 1) and target.is_cuda and target.dtype == torch.float32 and target.is_contiguous()):
        return False
    B, _, H, W = pred.shape
    return tuple(target.shape) == (B, H, W) if exact_shape else target.numel() == B * H * W


def _mc_target_ok(pred, target):
    B, C, H, W = pred.shape
    return (C >= 2 and target.is_cuda and target.dtype in _TARGET_DTYPES and target.is_contiguous()
            and tuple(target.shape) == (B, H, W))


def dice_bce_loss(pred, target):
    if _binary_target_ok(pred, target, exact_shape=True):
        return _DiceBCE.apply(pred, target)
    return dice_bce_composite(pred, target)


def tversky_loss(pred, target):
    if _device_logits(pred, 8) and (_binary_target_ok(pred, target, exact_shape=False) if pred.shape[1] == 1
                                    else _mc_target_ok(pred, target)):
        return _Tversky.apply(pred, target, TVERSKY_ALPHA, TVERSKY_BETA)
    return tversky_composite(pred, target)


def topk_loss(pred, target):
    if _binary_target_ok(pred, target, exact_shape=False) and pred.numel() >= 2:
        return _TopKBCE.apply(pred, target, pred.numel() // 2, _TOPK)
    return topk_composite(pred, target)


def bce_hem_loss(pred, target):
    if _binary_target_ok(pred, target, exact_shape=True) and pred.numel() >= BCE_HEM_K:
        return _TopKBCE.apply(pred, target, BCE_HEM_K, _BCE_HEM)
    return bce_hem_composite(pred, target)


def MRAccuracy(pred, target):
    """Mean relative cell-count error of a batch (reference loss.py:422-440), a Python float: per image the number n of
    8-connected components of `sigmoid(pred.squeeze(1)) >= 0.5` against count_gt = int(sum(target[b])):
    |count_gt - n| / count_gt, or 1 where count_gt == 0 and n != 0, averaged over target.shape[0].
    pred (B, 1, H, W) logits, target (B, H, W) dot maps.  Device logits: HIP kernels, one read-back of 2 B + 1 integers
    (count_gt is the fixed-order float64 sum of the fp32 map truncated toward zero: exact for 0/1 dot maps).  CPU logits: NumPy."""
    batch_size = target.shape[0]
    pred = pred.detach().squeeze(1)
    if pred.dim() != 3:
        raise ValueError(f"MRAccuracy: pred.squeeze(1) must be (B, H, W) (connectedComponents takes one 2-D image), got "
                         f"{tuple(pred.shape)}")
    if pred.shape[0] < batch_size:
        raise IndexError(f"MRAccuracy: target has {batch_size} images, pred {pred.shape[0]}")
    if batch_size == 0:
        raise ZeroDivisionError("MRAccuracy of an empty batch")
    if pred.is_cuda:
        from umi import infer, ops
        pred = pred[:batch_size]
        if pred.dtype == torch.float32:
            mask = infer.binary_mask(pred.unsqueeze(1))
        else:
            mask = (torch.sigmoid(pred) >= 0.5).to(torch.uint8).contiguous()
        gts = infer.sum_trunc(target.detach().reshape(batch_size, -1).float()) if target.is_cuda else None
        counts, fault = infer.count_objects(mask, _fault=True)
        if gts is not None:
            n_pred, n_gt, (code,) = (h.tolist() for h in ops.read_back(counts, gts, fault))
        else:
            n_pred, (code,) = (h.tolist() for h in ops.read_back(counts, fault))
            tnp = target.detach().numpy()
            n_gt = [int(np.sum(tnp[b])) for b in range(batch_size)]
        if code:
            raise RuntimeError(f"MRAccuracy: the component labelling reported fault {code}; the counts are invalid")
    else:
        from umi import components
        tnp = target.detach().cpu().numpy()
        pred_bin = torch.sigmoid(pred).numpy()
        pred_bin = (pred_bin >= 0.5).astype(np.uint8)             # NaN compares false: 0
        n_pred = [components.count_components_numpy(pred_bin[b]) for b in range(batch_size)]
        n_gt = [int(np.sum(tnp[b])) for b in range(batch_size)]
    mre = 0
    for count_pred, count_gt in zip(n_pred, n_gt):
        if count_gt != 0:
            mre += abs(count_gt - count_pred) / (count_gt)
        elif count_pred != 0:
            mre += 1
    mre /= batch_size
    return mre


# ---------------------------------------------------------------------------------------------------------------------
# hard-mask metrics (umi/metrics.py, csrc/seg_metrics.hip)

# name -> (kind of umi.metrics.scores, first class c0, multi-class)
SEG_METRICS = {'dice_err_mc': (0, 0, True), 'iou_err_mc': (1, 0, True), 'pixel_err_mc': (2, 0, True),
               'dice_err': (0, 1, False), 'iou_err': (1, 1, False), 'pixel_err': (2, 0, False)}

# False: the hard-mask metrics run the torch composite on every input (the A/B switch of tools/bench_seg_metrics.py)
METRICS_KERNEL = True


def seg_confusion_items(pred, target, items=1, multiclass=None):
    """The confusion matrices [items, K+1, K+1] (int64, where pred lives) of `items` consecutive groups of logits: the argmax
    mask of C >= 2 channels (`multiclass`; K = C) or the threshold mask of one logit (K = 2; labels (B, H, W) or (B, 1, H, W)).
    `multiclass` None: by the channel count.  One pass of the items-native kernel on its inputs, else the composite."""
    from umi import metrics
    if pred.dim() < 3:
        raise ValueError(f"hard-mask metrics take logits (B, C, ...), got {tuple(pred.shape)}")
    if multiclass is None:
        multiclass = pred.shape[1] != 1
    if multiclass and pred.shape[1] < 2:
        raise ValueError(f"the multi-class metrics ('*_mc') take logits with C >= 2 channels, got {tuple(pred.shape)}")
    if not multiclass and pred.shape[1] != 1:
        raise ValueError(f"the binary metrics take one-logit maps (B, 1, ...), got {tuple(pred.shape)}; use the '*_mc' names")
    pred = pred.detach()
    if METRICS_KERNEL and metrics.kernel_ok(pred, target, items):
        return metrics.confusion(pred, target, items)
    return metrics.confusion_composite(pred, target, items)


def seg_scores(counts, loss_type):
    """[items] fp32 values of a hard-mask metric name from its confusion matrices."""
    from umi import metrics
    kind, c0, _ = SEG_METRICS[loss_type]
    return (metrics.scores if METRICS_KERNEL else metrics.scores_composite)(counts, kind, c0)


def _seg_metric_items(pred, target, items, loss_type):
    return seg_scores(seg_confusion_items(pred, target, items, SEG_METRICS[loss_type][2]), loss_type)


# ---------------------------------------------------------------------------------------------------------------------
# surface-distance metrics (umi/surface.py, csrc/surface_metrics.hip)

# name -> (kind of umi.surface.surface_scores, multi-class); all of them score the foreground classes c0 = 1 .. K-1
SURFACE_METRICS = {'hd_mc': (0, True), 'hd95_mc': (1, True), 'assd_mc': (2, True),
                   'hd': (0, False), 'hd95': (1, False), 'assd': (2, False)}

# what an (image, class) with exactly one empty mask scores: 'diagonal' (sqrt((H-1)^2 + (W-1)^2)), 'zero' or 'nan'
SURFACE_EMPTY = 'diagonal'


def surface_stats_items(pred, target, multiclass=None):
    """(stats [B, K, 4] float64, counts [B, K, 2] int64, where pred lives) of 4-D logits against labels: the surface distances of the
    argmax mask of C >= 2 channels (`multiclass`; K = C) or of the threshold mask of one logit (K = 2; labels (B, H, W) or
    (B, 1, H, W)), foreground classes.  `multiclass` None: by the channel count.  The mask and distance kernels on their inputs,
    else the host composite."""
    from umi import metrics, surface
    if pred.dim() != 4:
        raise ValueError(f"surface-distance metrics take logits (B, C, H, W), got {tuple(pred.shape)}")
    if multiclass is None:
        multiclass = pred.shape[1] != 1
    if multiclass and pred.shape[1] < 2:
        raise ValueError(f"the multi-class metrics ('*_mc') take logits with C >= 2 channels, got {tuple(pred.shape)}")
    if not multiclass and pred.shape[1] != 1:
        raise ValueError(f"the binary metrics take one-logit maps (B, 1, ...), got {tuple(pred.shape)}; use the '*_mc' names")
    pred = pred.detach()
    K = pred.shape[1] if multiclass else 2
    if target.dim() == 4 and target.shape[1] == 1:
        target = target[:, 0]
    if tuple(target.shape) != (pred.shape[0],) + tuple(pred.shape[2:]):
        raise ValueError(f"logits {tuple(pred.shape)} and labels {tuple(target.shape)} do not match")
    if (METRICS_KERNEL and pred.is_cuda and pred.dtype == torch.float32 and pred.is_contiguous() and K <= 8 and pred.numel()
            and target.is_cuda and target.device == pred.device and target.is_contiguous() and target.dtype in _TARGET_DTYPES):
        from umi import infer
        mask = infer.argmax_mask(pred) if multiclass else infer.binary_mask(pred)
        if surface.surface_kernel_ok(mask, target, K):
            return surface.surface(mask, target, K, 1)
    else:
        mask = metrics.predict_composite(pred)[0].to(torch.uint8)
    _SURFACE_HOST_CALLS[0] += 1
    if pred.is_cuda and METRICS_KERNEL:
        warnings.warn(f"surface-distance metric on device logits {tuple(pred.shape)} {pred.dtype} with labels {target.dtype} runs the "
                      "NumPy statement on host copies (the kernels take contiguous fp32 logits with at most 8 channels, contiguous "
                      "int64 / float32 / uint8 / int32 labels and H, W <= 4096): thousands of times slower, and not capturable",
                      RuntimeWarning, stacklevel=3)
    return surface.surface_composite(mask, target, K, 1)


_SURFACE_HOST_CALLS = [0]


def surface_host_calls():
    """How often a surface-distance metric has taken the host composite so far.  A caller that wants to capture a step compares
    the figure before and after an eager run of it: the composite copies to the host, which a graph capture forbids."""
    return _SURFACE_HOST_CALLS[0]


def _surface_metric_items(pred, target, items, loss_type):
    from umi import surface
    kind, multiclass = SURFACE_METRICS[loss_type]
    stats, _ = surface_stats_items(pred, target, multiclass)
    score = surface.surface_scores if METRICS_KERNEL else surface.surface_scores_composite
    return score(stats, items, kind, 1, SURFACE_EMPTY, tuple(pred.shape[2:]))


def calc_loss(pred, target, bce_weight=0.5, loss_type='mse'):
    sync = _batch_sync()              # umi.ddp.GradReducer(global_batch=True): losses are those of the group's whole batch
    if sync is not None and loss_type in _BATCH_COUPLED:
        raise NotImplementedError(f"loss_type {loss_type!r} couples the batch in a way global_batch does not cover; it would "
                                  "silently stay per-replica")
    if loss_type == 'dice_bce_mc' and sync is not None:
        if _fused_ok(pred, target):
            return _FusedDiceCEGlobal.apply(pred, target, sync)
        return dice_bce_mc_global_composite(pred, target, sync)
    if loss_type == 'dice_bce_mc':
        if _fused_ok(pred, target):
            return _FusedDiceCE.apply(pred, target)
        loss_ce = F.cross_entropy(pred, target.long())
        loss_dice = DiceLoss(CLASS_NUMBER)(pred, target, softmax=True)
        return 0.5 * loss_ce + 0.5 * loss_dice
    if loss_type == 'CE':
        return F.cross_entropy(pred, target.long())
    if loss_type == 'BCE':
        return F.binary_cross_entropy_with_logits(pred.squeeze(1), target)
    if loss_type == 'mse':
        return F.mse_loss(pred.squeeze(1), target)
    if loss_type == 'mseMC':
        return F.mse_loss(pred, target)
    if loss_type == 'rmse':
        return torch.sqrt(F.mse_loss(pred, target))
    if loss_type == 'l1loss':
        return F.l1_loss(pred, target)
    if loss_type == 'HausdorffDTLoss':
        return HausdorffDTLoss()(pred, target, debug=False)
    if loss_type == 'dice_bce':
        return dice_bce_loss(pred, target)
    if loss_type == 'Tversky':
        return tversky_loss(pred, target)
    if loss_type == 'TopK':
        return topk_loss(pred, target)
    if loss_type == 'BCE_HEM':
        return bce_hem_loss(pred, target)
    if loss_type in SEG_METRICS:
        return _seg_metric_items(pred, target, 1, loss_type)[0]
    if loss_type in SURFACE_METRICS:
        return _surface_metric_items(pred, target, 1, loss_type)[0]
    if loss_type in _OUT_OF_SCOPE:
        raise NotImplementedError(f"loss_type {loss_type!r} is outside the MI355X hot-path scope")
    raise ValueError(f"unknown loss_type {loss_type!r}")


def _dice_ce_items(pred, target, items):
    """'dice_bce_mc' of `items` consecutive groups in one pass: umi_dice_ce_fwd_items, whose stats row i holds the bits
    umi_dice_ce_fwd leaves on the i-th slice.  Forward only."""
    from umi import lib as L, ops
    n, C = pred.shape[0] // items, pred.shape[1]
    HW = pred[0, 0].numel()
    stats = torch.empty((items, 3 * C + 2), dtype=torch.float32, device=pred.device)
    ws = ops.workspace(L.fn("umi_dice_ce_items_ws_bytes")(items, n, C, HW), pred.device)
    L.call("umi_dice_ce_fwd_items", pred.data_ptr(), target.data_ptr(), _TARGET_DTYPES[target.dtype], items, n, C, HW,
           stats.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
    return stats[:, 3 * C + 1].clone()


# False: calc_loss_items runs the per-slice loop for 'dice_bce_mc' too (the A/B switch of tools/bench_validation.py)
ITEMS_KERNEL = True


def calc_loss_items(pred, target, items, loss_type='mse'):
    """The losses of `items` consecutive groups of n images each: pred [items*n, C, H, W] and target [items*n, ...] ->
    a [items] tensor whose element i is calc_loss(pred[i*n:(i+1)*n], target[i*n:(i+1)*n], loss_type=loss_type).  By default
    literally that loop over contiguous slices, so every loss name behaves as in calc_loss (the names that raise included);
    'dice_bce_mc' on inputs of the fused kernels, the hard-mask metrics and the surface-distance metrics take one pass for all items
    (same bits).  Values only: made for the
    validation phase (Trainer(val_batch=k)), where nothing is differentiated.  Raises under an active global-batch switch
    (umi.ddp), where a loss is that of the data-parallel group's whole batch and a per-item value has no meaning."""
    items = int(items)
    if items < 1 or pred.shape[0] % items or target.shape[0] != pred.shape[0]:
        raise ValueError(f"calc_loss_items: {pred.shape[0]} predictions and {target.shape[0]} targets do not split into {items} "
                         "equal groups")
    if _batch_sync() is not None:
        raise NotImplementedError("calc_loss_items under global_batch: losses are those of the group's whole batch there")
    n = pred.shape[0] // items
    if (loss_type == 'dice_bce_mc' and ITEMS_KERNEL and items <= 65535 and not (torch.is_grad_enabled() and pred.requires_grad)
            and _fused_ok(pred, target)):
        return _dice_ce_items(pred, target, items)
    if loss_type in SEG_METRICS and METRICS_KERNEL:      # one counting pass over all items (the composite when not eligible)
        return _seg_metric_items(pred, target, items, loss_type)
    if loss_type in SURFACE_METRICS:                     # one call for all items (the host composite when not eligible)
        return _surface_metric_items(pred, target, items, loss_type)
    vals = [calc_loss(pred[i * n:(i + 1) * n], target[i * n:(i + 1) * n], loss_type=loss_type) for i in range(items)]
    return torch.stack([v if torch.is_tensor(v) else torch.as_tensor(v) for v in vals])


# ---------------------------------------------------------------------------------------------------------------------
# count-ratio-weighted multi-task loss (reference Trainer.py:1225-1249)

def multi_task_ratio_composite(output1, output2, label1, label2, ratio_weighted):
    """The reference lines, restated: returns (loss, loss1, loss2, ratioAccuracy)."""
    output1 = F.relu(output1)
    output2 = F.relu(output2)
    loss1 = calc_loss(output1, label1, loss_type='mse')
    loss2 = calc_loss(output2, label2, loss_type='mse')
    cellCountGt_immune = torch.sum(label1, axis=(1, 2))
    cellCountPred_immune = torch.sum(output1.squeeze(1), axis=(1, 2))
    cellCountGt_other = torch.sum(label2, axis=(1, 2))
    cellCountPred_other = torch.sum(output2.squeeze(1), axis=(1, 2))
    ratioGT = cellCountGt_immune / (cellCountGt_other + cellCountGt_immune)
    ratioPred = cellCountPred_immune / (cellCountPred_other + cellCountPred_immune)
    ratioAccuracy = torch.mean(abs(ratioGT - ratioPred))
    if ratio_weighted:
        loss = (loss1 + loss2) * (1 + (10 * ratioAccuracy))
    else:
        loss = loss1 + loss2
    return loss, loss1, loss2, ratioAccuracy


class _MultiTaskRatio(torch.autograd.Function):
    """multi_task_ratio_loss on (B, 1, H, W) fp32 device heads: umi_mt_ratio_fwd / _bwd; the fp64 stats are saved.  The gate
    (a bool, or a device tensor the kernel reads, so that a captured graph follows it) is kept in the stats for the backward."""

    @staticmethod
    def forward(ctx, o1, o2, l1, l2, gate):
        from umi import lib as L, ops
        B, HW = o1.shape[0], o1[0, 0].numel()
        dev = o1.device
        stats = torch.empty(L.fn("umi_mt_ratio_stats_len")(B), dtype=torch.float64, device=dev)
        outs = [torch.empty((), dtype=torch.float32, device=dev) for _ in range(4)]
        ws = ops.workspace(L.fn("umi_mt_ratio_ws_bytes")(B, HW), dev)
        flag = torch.is_tensor(gate)
        L.call("umi_mt_ratio_fwd", o1.data_ptr(), o2.data_ptr(), l1.data_ptr(), l2.data_ptr(), B, HW,
               0 if flag else int(bool(gate)), gate.data_ptr() if flag else None, stats.data_ptr(), *[t.data_ptr() for t in outs], ws.data_ptr(), ws.numel(),
               ops._stream())
        ctx.save_for_backward(o1, o2, l1, l2, stats)
        return tuple(outs)

    @staticmethod
    def backward(ctx, gL, g1, g2, gr):
        from umi import lib as L, ops
        o1, o2, l1, l2, stats = ctx.saved_tensors
        zero = torch.zeros((), dtype=torch.float32, device=o1.device)
        g = torch.stack([zero if v is None else v.detach().to(torch.float32) for v in (gL, g1, g2, gr)])
        d1, d2 = torch.empty_like(o1), torch.empty_like(o2)
        L.call("umi_mt_ratio_bwd", o1.data_ptr(), o2.data_ptr(), l1.data_ptr(), l2.data_ptr(), stats.data_ptr(),
               g.data_ptr(), o1.shape[0], o1[0, 0].numel(), d1.data_ptr(), d2.data_ptr(),
               ops._stream())
        return d1, d2, None, None, None


def _mt_ratio_device_ok(o1, o2, l1, l2):
    if not all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in (o1, o2, l1, l2)):
        return False
    if l1.requires_grad or l2.requires_grad:            # the kernels give the labels no gradient
        return False
    if o1.dim() != 4 or o1.shape[1] != 1 or tuple(o2.shape) != tuple(o1.shape):
        return False
    B, _, H, W = o1.shape
    return (tuple(l1.shape) == (B, H, W) and tuple(l2.shape) == (B, H, W) and 0 < o1.numel() < (1 << 31)
            and B <= 65535 and len({o1.device, o2.device, l1.device, l2.device}) == 1)


def multi_task_ratio_loss(o1, o2, l1, l2, ratio_weighted):
    """Step loss of the reference's multi_task_trainRatio (Trainer.py:1225-1249) on the RAW head outputs o1, o2 (the ReLU is
    part of it) and the label maps l1, l2: returns (loss, loss1, loss2, ratioAccuracy), all differentiable.  ratio_weighted:
    the reference's `epoch > 5` gate, loss = (loss1 + loss2) * (1 + 10 * ratioAccuracy); else loss = loss1 + loss2.  It may
    be a one-element fp32 device tensor (nonzero = on), which the device kernels read at run time (graph replay); with the
    composite it is read on the host."""
    if torch.is_tensor(ratio_weighted):
        if _mt_ratio_device_ok(o1, o2, l1, l2) and ratio_weighted.is_cuda and ratio_weighted.dtype == torch.float32 \
                and ratio_weighted.numel() == 1 and ratio_weighted.device == o1.device:
            return _MultiTaskRatio.apply(o1, o2, l1, l2, ratio_weighted.detach())
        ratio_weighted = bool(ratio_weighted)
    if _mt_ratio_device_ok(o1, o2, l1, l2):
        return _MultiTaskRatio.apply(o1, o2, l1, l2, bool(ratio_weighted))
    return multi_task_ratio_composite(o1, o2, l1, l2, ratio_weighted)
