"""Test-time augmentation over the symmetries of the square, and model ensembles: the NumPy statement of the rule and thin
device wrappers over the three kernels of csrc/tta.hip (umi_tta_views, umi_tta_accumulate, umi_tta_finish).

    merged = umi.infer.predict_logits_tta(model, x, views='d4', mode='prob')      # fp32 (N,K,H,W) on the device
    mask = umi.infer.predict_mask_tta(model, x, views='flips', mode='logit')      # uint8 (N,H,W)

The reference trains under `random_rot_flip` (DataLoader.py:103-111: np.rot90 by k, then one np.flip); a model trained over
those views is evaluated by averaging over them.

Elements.  e in 0..7, k = e & 3, f = e >> 2:
    view_e(x)   = flip(rot90(x, k, axes=(-2, -1)), axis=-1) if f else rot90(x, k, axes=(-2, -1))
    unview_e(y) = the inverse, applied to the network's output.
Odd k turns (H, W) into (W, H).  In index form, with (H', W') the view's shape and j' = W' - 1 - j if f else j, view pixel
(i, j) shows the image pixel
    k = 0: (i, j')      k = 1: (j', W - 1 - i)      k = 2: (H - 1 - i, W - 1 - j')      k = 3: (H - 1 - j', i)
(`view_source`; the kernels restate these four lines and their inverses).

View sets.  'none' = (0,), 'flips' = (0, 2, 4, 6) (identity, rot180 and the two mirror images: the views that keep (H, W)),
'd4' = (0, .., 7); any tuple of elements, repeats allowed.

Modes.  y_v = fp32 output of view v mapped back by unview:
    'logit'  mean of y_v                              any K
    'relu'   mean of (0 where y_v < 0 else y_v)       the regression heads (test_mc3serousv5.py:961 applies ReLU first); a NaN
                                                      and -0.0 pass through
    'prob'   mean of softmax(y_v) over the K channels; K = 1: mean of sigmoid(y_v)
Accumulation: acc = 0; acc = fp32(acc + t(y_v)) in the order of the `views` tuple, then model after model for an ensemble; one
IEEE division by float32(count) finishes it.  The result therefore does not depend on how the views are cut into forwards.

Mask.  'logit' and 'relu': umi_argmax_mask's rule on the mean (the first strict maximum wins, a NaN never wins), for K = 1
umi_binary_mask's (mean >= -0x1.7ffffcp-23).  'prob': the same argmax of the mean probabilities, for K = 1 mean >= 0.5.
Entropy ('prob' only): -sum_c p_c log p_c of the mean probabilities, 0 log 0 = 0; K = 1: the binary entropy of p and 1 - p.

'logit' and 'relu' are stated in float32 and the device matches them bit for bit.  'prob' and the entropy are stated in
float64; `prob_bound` / `entropy_bound` bound the device's fp32 evaluation (derivation in DESIGN.md section 3)."""
import numpy as np

VIEW_SETS = {"none": (0,), "flips": (0, 2, 4, 6), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}
MODES = {"logit": 0, "relu": 1, "prob": 2}
# the kernels' limits (csrc/tta.hip refuses the same with UMI_ERR_UNSUPPORTED)
MAX_K = 32
MAX_CALL_VIEWS = 16                 # elements per call: 4 bits each in one 64-bit integer
MAX_PLANES = 65535                  # N * C (views), N (accumulate, finish): a grid dimension
BINARY_CUTOFF = np.frombuffer(np.uint32(0xB43FFFFE).tobytes(), dtype=np.float32)[0]      # umi_binary_mask's cut-off

# Largest error of the device expf / logf against float64, in units in the last place, measured on the MI355X over the ranges the
# kernels and the tests use and rounded up to a whole ulp (tools/bench_tta.py -> profiles/tta.json "math_ulp": expf 0.85 on
# [-60, 20], logf 2.15 on (0, 1]; ROCm ships no accuracy table on the machine).
EXPF_ULP = 1.0
LOGF_ULP = 3.0
_U = 2.0 ** -24                     # fp32 unit roundoff


def view_set(views):
    """'none' / 'flips' / 'd4' or any sequence of elements 0..7 -> tuple of ints (repeats kept, order kept)."""
    if isinstance(views, str):
        if views not in VIEW_SETS:
            raise ValueError(f"views must be one of {sorted(VIEW_SETS)} or a tuple of elements 0..7, got {views!r}")
        return VIEW_SETS[views]
    try:
        out = tuple(views)
    except TypeError:
        raise ValueError(f"views must be a name or a tuple of elements 0..7, got {views!r}") from None
    if not out:
        raise ValueError("views must name at least one element")
    for e in out:
        if isinstance(e, bool) or not isinstance(e, (int, np.integer)) or not 0 <= int(e) <= 7:
            raise ValueError(f"a view element must be an int in 0..7, got {e!r}")
    return tuple(int(e) for e in out)


def check_mode(mode):
    if mode not in MODES:
        raise ValueError(f"mode must be one of {sorted(MODES)}, got {mode!r}")
    return MODES[mode]


def transposes(e):
    """Whether element e turns (H, W) into (W, H)."""
    return bool(e & 1)


def view_shape(e, H, W):
    return (W, H) if e & 1 else (H, W)


def view_numpy(x, e):
    """view_e of an array (..., H, W)."""
    (e,) = view_set((e,))
    r = np.rot90(x, e & 3, axes=(-2, -1))
    return np.ascontiguousarray(np.flip(r, axis=-1) if e >> 2 else r)


def unview_numpy(y, e):
    """The inverse of view_numpy(., e): undo the flip, then turn back."""
    (e,) = view_set((e,))
    r = np.flip(y, axis=-1) if e >> 2 else y
    return np.ascontiguousarray(np.rot90(r, -(e & 3), axes=(-2, -1)))


def view_source(e, H, W):
    """(ys, xs): int arrays of the view's shape, the image pixel that view pixel (i, j) of element e shows -- the four lines of the
    module docstring, which csrc/tta.hip restates."""
    (e,) = view_set((e,))
    k, f = e & 3, e >> 2
    Hv, Wv = view_shape(e, H, W)
    i, j = np.meshgrid(np.arange(Hv), np.arange(Wv), indexing="ij")
    jp = Wv - 1 - j if f else j
    return ((i, jp), (jp, W - 1 - i), (H - 1 - i, W - 1 - jp), (H - 1 - jp, i))[k]


def shape_classes(elements, H, W):
    """The elements' positions in the tuple grouped by the shape of their views: {(H', W'): [positions]}, one class for a square
    image, two (the even and the odd turns) otherwise."""
    out = {}
    for pos, e in enumerate(view_set(elements)):
        out.setdefault(view_shape(e, H, W), []).append(pos)
    return out


def pack_elements(elements):
    """<= 16 elements as one integer, 4 bits each, the first in the lowest bits: how a list travels to the kernels by value."""
    elements = view_set(elements)
    if len(elements) > MAX_CALL_VIEWS:
        raise ValueError(f"at most {MAX_CALL_VIEWS} elements per call, got {len(elements)}")
    return sum(e << (4 * s) for s, e in enumerate(elements))


def _transform(y, mode):
    """Per-view transform of 'relu' (float32) and 'prob' (float64) on (N, K, h, w)."""
    if mode == "relu":
        return np.where(y < 0, np.float32(0), y)
    y = y.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        if y.shape[1] == 1:
            return 1.0 / (1.0 + np.exp(-y))
        ex = np.exp(y - y.max(axis=1, keepdims=True))
        return ex / ex.sum(axis=1, keepdims=True)


def merge_numpy(outputs, elements, mode="logit"):
    """outputs: one array (N, K, H', W') per entry of `elements`, the network's output for that view (an ensemble passes its
    models' lists one after the other, with `elements` repeated) -> the mean in the image's frame, (N, K, H, W): float32 for 'logit'
    and 'relu', each addition rounded, one division by float32(count); float64 for 'prob'."""
    elements = view_set(elements)
    check_mode(mode)
    if len(outputs) != len(elements):
        raise ValueError(f"{len(outputs)} outputs for {len(elements)} elements")
    acc = None
    with np.errstate(invalid="ignore", over="ignore"):
        for y, e in zip(outputs, elements):
            y = np.asarray(y)
            if y.ndim != 4 or y.dtype != np.float32:
                raise ValueError(f"an output must be float32 (N, K, H', W'), got {y.shape} {y.dtype}")
            t = unview_numpy(y if mode == "logit" else _transform(y, mode), e)
            if acc is None:
                acc = np.zeros(t.shape, dtype=t.dtype)
            if t.shape != acc.shape:
                raise ValueError(f"the outputs map back to different shapes: {t.shape} after {acc.shape}")
            acc = acc + t
        if mode == "prob":
            return acc / float(len(elements))
        assert acc.dtype == np.float32
        return acc / np.float32(len(elements))


def mask_numpy(mean, mode="logit"):
    """uint8 (N, H, W) of a merged (N, K, H, W): the first strict maximum over K (a NaN never wins); K = 1: mean >= the cut-off of
    umi_binary_mask ('logit', 'relu') or >= 0.5 ('prob'), a NaN gives 0."""
    check_mode(mode)
    mean = np.asarray(mean)
    if mean.shape[1] == 1:
        with np.errstate(invalid="ignore"):
            return (mean[:, 0] >= (0.5 if mode == "prob" else BINARY_CUTOFF)).astype(np.uint8)
    best, idx = mean[:, 0].copy(), np.zeros(mean[:, 0].shape, dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        for k in range(1, mean.shape[1]):
            win = mean[:, k] > best
            best, idx = np.where(win, mean[:, k], best), np.where(win, np.uint8(k), idx)
    return idx


def entropy_numpy(mean):
    """float64 (N, H, W): -sum_c p_c log p_c of mean probabilities (N, K, H, W), 0 log 0 = 0; K = 1: of (p, 1 - p)."""
    p = np.asarray(mean, dtype=np.float64)
    if p.shape[1] == 1:
        p = np.concatenate([p, 1.0 - p], axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return -np.where(p > 0, p * np.log(np.where(p > 0, p, 1.0)), 0.0).sum(axis=1)


def top_two_margin(mean, mode="prob"):
    """float64 (N, H, W): how far the statement's decision is from flipping -- largest minus second-largest channel, for K = 1 the
    distance of the mean from the threshold."""
    mean = np.asarray(mean, dtype=np.float64)
    if mean.shape[1] == 1:
        return np.abs(mean[:, 0] - (0.5 if mode == "prob" else float(BINARY_CUTOFF)))
    s = np.sort(mean, axis=1)
    return s[:, -1] - s[:, -2]


def prob_bound(K, count, spread):
    """Bound on |device mean probability - float64 statement| for `count` accumulated views of K channels whose logits lie within
    `spread` of the pixel's maximum (K = 1: |logit| <= spread).  u = 2^-24; per view, relative to p <= 1:
      d = fp32(y - max): |d| u, which exp turns into a relative |d| u <= spread u;  expf: 2 EXPF_ULP u;
      both once more through the sum in the denominator, whose K - 1 additions add (K - 1) u;  the division: u.
      (K = 1: -y is exact, expf, 1 + e, 1 / s: 2 EXPF_ULP u + 2 u, inside the same expression.)
    The fp32 accumulation of `count` values in [0, 1]: the i-th partial sum is <= i, so the additions err by at most
    u (1 + 2 + ... + count), which the division by count turns into u (count + 1) / 2; the division itself: u."""
    per_view = 2.0 * (spread + 2.0 * EXPF_ULP) + (K - 1) + 1.0
    return _U * (per_view + (count + 1) / 2.0 + 1.0) * 1.01


def entropy_bound(K, eps):
    """Bound on |device entropy - float64 statement| given mean probabilities within `eps` (prob_bound) of the statement's, over
    max(K, 2) terms t(p) = -p log p:  |t(p) - t(q)| <= -|p - q| log |p - q| for |p - q| <= 1/2 (the modulus of continuity of
    x log x), here eps plus u for fp32(1 - p) when K = 1;  logf and the product: (2 LOGF_ULP + 1) u relative to t <= 1 / e;
    the fp32 sum of the terms, each partial sum <= log max(K, 2): (terms - 1) u log(terms)."""
    n = max(K, 2)
    d = eps + _U
    return (n * (-d * np.log(d) + (2.0 * LOGF_ULP + 1.0) * _U / np.e) + (n - 1) * _U * np.log(n)) * 1.01


# ---- device wrappers --------------------------------------------------------------------------------------------------------------
def _nchw(t, what):
    import torch
    from . import ops
    ops._need_cuda(t)
    if t.dim() != 4 or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() == 0:
        raise ValueError(f"{what} must be a contiguous non-empty fp32 device tensor (N, C, H, W), got {tuple(t.shape)} {t.dtype}")
    return tuple(t.shape)


def _one_shape(elements, H, W):
    if H != W and len({e & 1 for e in elements}) > 1:
        raise ValueError(f"the views {elements} of a {H}x{W} image have two shapes; pass each shape class on its own")


def views(x, elements, out=None):
    """x fp32 (N, C, H, W) -> fp32 (V * N, C, H', W'), view-major: view_numpy(x, e) for every e of `elements`, which must share one
    output shape (any mix for H == W, otherwise all even or all odd turns)."""
    import torch
    from . import lib as L, ops
    elements = view_set(elements)
    N, C, H, W = _nchw(x, "x")
    _one_shape(elements, H, W)
    Hv, Wv = view_shape(elements[0], H, W)
    shape = (len(elements) * N, C, Hv, Wv)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise ValueError(f"views: `out` must be a contiguous fp32 device tensor {shape}, got {tuple(out.shape)} {out.dtype}")
    for a in range(0, len(elements), MAX_CALL_VIEWS):
        part = elements[a:a + MAX_CALL_VIEWS]
        if not L.supported("umi_tta_views", x.data_ptr(), N, C, H, W, out[a * N:].data_ptr(), pack_elements(part), len(part),
                           ops._stream()):
            raise ValueError(f"views: unsupported size {(N, C, H, W)} (N * C <= {MAX_PLANES}, V * N * C * H * W < 2**31)")
    return out


def accumulate(acc, outputs, elements, mode="logit"):
    """acc fp32 (N, K, H, W) += the outputs fp32 (V * N, K, H', W') of the views `elements` (view-major, one output shape) mapped
    back and transformed by `mode`, in place, view after view in the order given."""
    from . import lib as L, ops
    elements = view_set(elements)
    m = check_mode(mode)
    N, K, H, W = _nchw(acc, "acc")
    shape = _nchw(outputs, "outputs")
    _one_shape(elements, H, W)
    want =(len(elements) * N, K) + view_shape(elements[0], H, W)
    if shape != want:
        raise ValueError(f"accumulate: outputs of the views {elements} into {(N, K, H, W)} must be {want}, got {shape}")
    if K > MAX_K:
        raise ValueError(f"accumulate: K = {K} beyond the kernels' limit of {MAX_K}")
    for a in range(0, len(elements), MAX_CALL_VIEWS):
        part = elements[a:a + MAX_CALL_VIEWS]
        if not L.supported("umi_tta_accumulate", acc.data_ptr(), N, K, H, W, outputs[a * N:].data_ptr(), pack_elements(part),
                           len(part), m, ops._stream()):
            raise ValueError(f"accumulate: unsupported size {(N, K, H, W)} (K <= {MAX_K}, N <= {MAX_PLANES}, "
                             "V * N * K * H * W < 2**31)")
    return acc


def finish(acc, count, mode="logit", mask=False, entropy=False):
    """acc / float32(count) in place; returns acc, then the uint8 (N, H, W) mask if `mask`, then the fp32 (N, H, W) entropy of the
    mean probabilities if `entropy` ('prob' only)."""
    import torch
    from . import lib as L, ops
    m = check_mode(mode)
    N, K, H, W = _nchw(acc, "acc")
    count = int(count)
    if count < 1:
        raise ValueError(f"count must be >= 1, got {count}")
    if entropy and mode != "prob":
        raise ValueError("the entropy map exists in 'prob' mode only")
    mk = torch.empty((N, H, W), dtype=torch.uint8, device=acc.device) if mask else None
    en = torch.empty((N, H, W), dtype=torch.float32, device=acc.device) if entropy else None
    if not L.supported("umi_tta_finish", acc.data_ptr(), N, K, H, W, count, m, mk.data_ptr() if mask else None,
                       en.data_ptr() if entropy else None, ops._stream()):
        raise ValueError(f"finish: unsupported size {(N, K, H, W)} (K <= {MAX_K}, N * K * H * W < 2**31)")
    res = (acc,) + ((mk,) if mask else ()) + ((en,) if entropy else ())
    return res if len(res) > 1 else acc
