"""Surface-distance metrics of hard masks: Hausdorff distance ('hd'), its 95th percentile ('hd95') and the average symmetric
surface distance ('assd') per (image, class), the common (medpy / TransUNet evaluation) definition for unit pixel spacing, 2-D.

The rule.  For one image and one class c: A = (pred_mask == c), G = (label is class c) by `umi.metrics.rows_numpy`'s label rule (an
integer in 0..K-1 or a float exactly equal to one is a class, anything else belongs to no class).  The surface of a mask M is
M & ~erode(M) with a 4-connected erosion and pixels outside the image counting as 0: a pixel of M on the image edge or with a
4-neighbour outside M (scipy: M ^ binary_erosion(M, generate_binary_structure(2, 1))).  Every surface pixel of A gets d2, the exact
integer squared Euclidean distance to the nearest surface pixel of G, and the other way round; the distance is sqrt((double)d2).
With S = hstack(d(A->G), d(G->A)), n = len(S), sorted ascending:

    hd    max(S)
    hd95  np.percentile(S, 95): v = (n-1) * 0.95, lo = floor(v), t = v - lo, a = S[lo], b = S[min(lo+1, n-1)];
          a + (b-a) * t if t < 0.5 else b - (b-a) * (1-t), without contraction
    assd  (mean(d(A->G)) + mean(d(G->A))) / 2

State per (image, class): 0 both masks non-empty, 1 both empty, 2 prediction empty only, 3 label empty only; hd, hd95 and assd are
0.0 unless the state is 0.  stats[B, K, 4] = (hd, hd95, assd, state) in float64, counts[B, K, 2] = the surface pixels of A and of G
(int64); classes below c0 are zeros.

The score of an item (a group of n images) is the float64 mean over its images and the classes c0..K-1, added in (image, class)
order and rounded once to fp32, of the value in state 0, of 0.0 in state 1, and in states 2 and 3 of the empty rule: 'diagonal' =
sqrt((H-1)^2 + (W-1)^2), the largest value the field can hold (an empty prediction is never the best model), 'zero' (what
TransUNet's evaluation script does) or 'nan'.

`surface_numpy` / `surface_scores_numpy` are the statement (a separable exact integer transform, no SciPy).  `surface` /
`surface_scores` run the HIP kernels (csrc/surface_metrics.hip: four launches and one, integer atomics only, nothing read back,
capturable) on contiguous device masks and labels and raise on anything else; `surface_composite` / `surface_scores_composite`
serve every other input by running the statement on host copies.  Out of scope: anisotropic spacing, 3-D volumes."""
import numpy as np
import torch

from .metrics import MAX_K, _TARGET_DTYPES, rows_numpy

KINDS = {"hd": 0, "hd95": 1, "assd": 2}
EMPTY_RULES = {"diagonal": 0, "zero": 1, "nan": 2}
MAX_HW = 4096
_BIG = 1 << 20
_INF = 1 << 40


def _kind(kind):
    k = KINDS.get(kind, kind)
    if k not in (0, 1, 2) or isinstance(k, bool):
        raise ValueError(f"kind takes 0 / 'hd', 1 / 'hd95' or 2 / 'assd', not {kind!r}")
    return k


def _rule(rule):
    r = EMPTY_RULES.get(rule, rule)
    if r not in (0, 1, 2) or isinstance(r, bool):
        raise ValueError(f"the empty rule takes 'diagonal', 'zero' or 'nan', not {rule!r}")
    return r


# ---- the statement (NumPy) ---------------------------------------------------------------------------------------------------

def surface_mask(m):
    """M & ~erode4(M) of a 2-D bool mask, pixels outside the image counting as 0."""
    p = np.pad(m, 1)
    return m & ~(p[:-2, 1:-1] & p[2:, 1:-1] & p[1:-1, :-2] & p[1:-1, 2:])


def _col_sq(mask):
    """Squared distance of every pixel to the nearest True pixel of its own column, _INF if the column has none."""
    H = mask.shape[0]
    r = np.arange(H, dtype=np.int64)[:, None]
    above = np.maximum.accumulate(np.where(mask, r, -_BIG), axis=0)
    below = np.minimum.accumulate(np.where(mask, r, _BIG)[::-1], axis=0)[::-1]
    d = np.minimum(r - above, below - r)
    return np.where(d > H, _INF, d * d)


def directed_d2(src, dst):
    """int64 d2 of every True pixel of `src` (row-major order) to the nearest True pixel of `dst` (not empty): the separable exact
    transform; the outward row search stops once k^2 reaches the largest current minimum among the source pixels."""
    best = _col_sq(dst)
    g2 = best.copy()
    W = g2.shape[1]
    for k in range(1, W):
        kk = k * k
        if kk >= best[src].max():
            break
        np.minimum(best[:, k:], g2[:, :-k] + kk, out=best[:, k:])
        np.minimum(best[:, :-k], g2[:, k:] + kk, out=best[:, :-k])
    return best[src]


def percentile95(S):
    """np.percentile(S, 95) of a non-empty float64 vector, spelled out."""
    S = np.sort(np.asarray(S, dtype=np.float64))
    n = len(S)
    v = np.float64(n - 1) * np.float64(0.95)
    lo = int(np.floor(v))
    t = v - np.float64(lo)
    a, b = S[lo], S[min(lo + 1, n - 1)]
    diff = b - a
    return a + diff * t if t < 0.5 else b - diff * (np.float64(1.0) - t)


def _squeeze_np(shape, target):
    target = np.asarray(target)
    if target.ndim == len(shape) + 1 and target.shape[1] == 1:
        target = target[:, 0]
    if tuple(target.shape) != tuple(shape):
        raise ValueError(f"mask {tuple(shape)} and labels {tuple(target.shape)} do not match")
    return target


def surface_numpy(pred_mask, target, K, c0=1):
    """(stats float64 [B, K, 4], counts int64 [B, K, 2]) of a uint8 mask [B, H, W] against labels [B, H, W] ([B, 1, H, W] too)."""
    pred = np.asarray(pred_mask)
    if pred.ndim != 3 or pred.dtype != np.uint8:
        raise ValueError(f"surface metrics take a uint8 mask [B, H, W], got {pred.shape} {pred.dtype}")
    K, c0 = int(K), int(c0)
    if K < 2 or not 0 <= c0 < K:
        raise ValueError(f"K = {K} / c0 = {c0}")
    row = rows_numpy(_squeeze_np(pred.shape, target), K)
    B = pred.shape[0]
    stats, counts = np.zeros((B, K, 4), np.float64), np.zeros((B, K, 2), np.int64)
    for b in range(B):
        for c in range(c0, K):
            sa, sg = surface_mask(pred[b] == c), surface_mask(row[b] == c)
            na, ng = int(sa.sum()), int(sg.sum())
            counts[b, c] = na, ng
            state = (0 if ng else 3) if na else (2 if ng else 1)
            stats[b, c, 3] = state
            if state:
                continue
            dag = np.sqrt(directed_d2(sa, sg).astype(np.float64))
            dga = np.sqrt(directed_d2(sg, sa).astype(np.float64))
            S = np.hstack([dag, dga])
            stats[b, c, 0] = S.max()
            stats[b, c, 1] = percentile95(S)
            stats[b, c, 2] = (dag.sum() / np.float64(na) + dga.sum() / np.float64(ng)) / np.float64(2.0)
    return stats, counts


def surface_scores_numpy(stats, items, kind, c0=1, empty="diagonal", hw=None):
    """float32 [items] from stats [items*n, K, 4]; hw = (H, W) of the images (the 'diagonal' rule needs it)."""
    kind, rule = _kind(kind), _rule(empty)
    st = np.asarray(stats, dtype=np.float64)
    items = int(items)
    if st.ndim != 3 or st.shape[2] != 4 or items < 1 or st.shape[0] % items or not 0 <= c0 < st.shape[1]:
        raise ValueError(f"stats {st.shape} / items {items} / c0 {c0}")
    n, K = st.shape[0] // items, st.shape[1]
    if rule == 0:
        if hw is None:
            raise ValueError("the 'diagonal' rule needs hw = (H, W)")
        fill = np.sqrt(np.float64((int(hw[0]) - 1) ** 2 + (int(hw[1]) - 1) ** 2))
    else:
        fill = np.float64(0.0) if rule == 1 else np.float64(np.nan)
    state = st[..., 3]
    val = np.where(state == 0, st[..., kind], np.where(state == 1, 0.0, fill)).reshape(items, n, K)
    total = np.zeros(items, np.float64)
    for i in range(n):
        for c in range(c0, K):
            total = total + val[:, i, c]
    return (total / np.float64(n * (K - c0))).astype(np.float32)


# ---- composite: the statement on host copies ------------------------------------------------------------------------------------

def surface_composite(pred_mask, target, K, c0=1):
    """The statement on host copies of the tensors, results where pred_mask lives: CPU tensors, non-contiguous views, sizes the
    kernels refuse.  It synchronises (device inputs are copied to the host), so it is NOT capturable."""
    stats, counts = surface_numpy(pred_mask.detach().cpu().numpy(), target.detach().cpu().numpy(), K, c0)
    return torch.from_numpy(stats).to(pred_mask.device), torch.from_numpy(counts).to(pred_mask.device)


def surface_scores_composite(stats, items, kind, c0=1, empty="diagonal", hw=None):
    """surface_scores_numpy on a host copy (not capturable)."""
    return torch.from_numpy(surface_scores_numpy(stats.detach().cpu().numpy(), items, kind, c0, empty, hw)).to(stats.device)


# ---- the kernels ------------------------------------------------------------------------------------------------------------------

def _squeeze_target(shape, target):
    if target.dim() == len(shape) + 1 and target.shape[1] == 1:
        target = target[:, 0]
    return target


def surface_kernel_ok(pred_mask, target, K):
    """Whether `surface` takes these inputs."""
    if not (torch.is_tensor(pred_mask) and torch.is_tensor(target) and pred_mask.is_cuda and target.is_cuda
            and pred_mask.device == target.device and pred_mask.dtype == torch.uint8 and pred_mask.dim() == 3
            and pred_mask.is_contiguous() and target.is_contiguous() and target.dtype in _TARGET_DTYPES):
        return False
    B, H, W = pred_mask.shape
    if tuple(_squeeze_target(pred_mask.shape, target).shape) != (B, H, W) or K is None or not 2 <= K <= MAX_K:
        return False
    return 0 < H <= MAX_HW and 0 < W <= MAX_HW and B > 0 and B * K <= 65535 and B * K * H * W < (1 << 31)


def surface(pred_mask, target, K, c0=1):
    """Device (stats float64 [B, K, 4], counts int64 [B, K, 2]) of a contiguous uint8 device mask [B, H, W] against contiguous device
    labels [B, H, W] ([B, 1, H, W] too): four launches, nothing read back.  Raises on inputs the kernels do not take (use
    surface_composite for those)."""
    from . import lib as L, ops
    if not surface_kernel_ok(pred_mask, target, K) or not 0 <= int(c0) < K:
        raise ValueError("umi.surface.surface takes a contiguous uint8 device mask [B, H <= 4096, W <= 4096] with K in 2..8, c0 in "
                         "0..K-1 and contiguous device labels (int64 / float32 / uint8 / int32) of the matching shape; got "
                         f"{tuple(pred_mask.shape)} {pred_mask.dtype} on {pred_mask.device}, {tuple(target.shape)} {target.dtype} on "
                         f"{target.device}, K = {K}, c0 = {c0}")
    B, H, W = pred_mask.shape
    stats = torch.empty((B, K, 4), dtype=torch.float64, device=pred_mask.device)
    counts = torch.empty((B, K, 2), dtype=torch.int64, device=pred_mask.device)
    ws = ops.workspace(L.fn("umi_surface_ws_bytes")(B, int(K), int(c0), H, W), pred_mask.device)
    L.call("umi_surface_distances", pred_mask.data_ptr(), target.data_ptr(), _TARGET_DTYPES[target.dtype], B, int(K), int(c0), H, W,
           stats.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream())
    return stats, counts


def surface_scores(stats, items, kind, c0=1, empty="diagonal", hw=None):
    """float32 [items] of stats [items*n, K, 4]: the kernel for contiguous float64 device stats, the host composite otherwise."""
    kind, rule = _kind(kind), _rule(empty)
    items = int(items)
    if hw is None:
        if rule == 0:
            raise ValueError("the 'diagonal' rule needs hw = (H, W)")
        hw = (1, 1)
    H, W = int(hw[0]), int(hw[1])
    if not (stats.is_cuda and stats.dtype == torch.float64 and stats.is_contiguous() and stats.dim() == 3 and stats.shape[2] == 4
            and 2 <= stats.shape[1] <= MAX_K and items >= 1 and stats.shape[0] > 0 and stats.shape[0] % items == 0
            and 0 <= c0 < stats.shape[1] and 0 < H <= MAX_HW and 0 < W <= MAX_HW):
        return surface_scores_composite(stats, items, kind, c0, rule, hw)
    from . import lib as L, ops
    out = torch.empty(items, dtype=torch.float32, device=stats.device)
    L.call("umi_surface_scores", stats.data_ptr(), items, stats.shape[0] // items, stats.shape[1], int(c0), kind, rule, H, W,
           out.data_ptr(), ops._stream())
    return out


class SurfaceMeter:
    """Accumulates surface distances over an evaluation loop: `add(pred_mask, label)` takes the uint8 [B, H, W] masks of
    `umi.infer.predict_mask` / `predict_binary_mask` (K = the class count, 2 for a binary model) and the labels; the kernels where
    they apply (no synchronisation), the host composite otherwise.  `read()` copies the sums to the host once and returns
    {'hd', 'hd95', 'assd': float64 [K], the mean over the (image, class) cases in state 0 (nan where there is none);
    'states': int64 [K, 4], the number of cases in each state per class}.  Classes below c0 are not scored: nan and zeros."""

    def __init__(self, K, c0=1):
        self.K, self.c0 = int(K), int(c0)
        self.sums = self.states = None

    def add(self, pred_mask, label):
        if surface_kernel_ok(pred_mask, label, self.K):
            stats, _ = surface(pred_mask, label, self.K, self.c0)
        else:
            stats, _ = surface_composite(pred_mask, label, self.K, self.c0)
        state = stats[..., 3].long()
        scored = torch.zeros_like(state, dtype=torch.bool)
        scored[:, self.c0:] = True
        sums = (stats[..., :3] * ((state == 0) & scored).unsqueeze(-1)).sum(dim=0)
        states = torch.stack([((state == s) & scored).sum(dim=0) for s in range(4)], dim=1)
        if self.sums is None:
            self.sums, self.states = sums, states
        else:
            self.sums.add_(sums.to(self.sums.device))
            self.states.add_(states.to(self.states.device))
        return self

    def reset(self):
        if self.sums is not None:
            self.sums.zero_()
            self.states.zero_()

    def read(self):
        if self.sums is None:
            raise RuntimeError("SurfaceMeter.read() before the first add")
        sums, states = self.sums.cpu().numpy(), self.states.cpu().numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = sums / states[:, :1].astype(np.float64)
        return {"hd": mean[:, 0], "hd95": mean[:, 1], "assd": mean[:, 2], "states": states}
