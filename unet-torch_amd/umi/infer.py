"""Inference entry on the MI355X: the steps either side of the network in the reference's evaluation scripts
(test_mc3serousv5.py:100-127 `preprocess`, :877-887 forward -> softmax -> argmax -> uint8 mask), SURVEY 8(f) rank 4.

    x = infer.preprocess(img)                 # HWC uint8 / float image (numpy or tensor) -> [1,C,H,W] fp32 on the device
    mask = infer.predict_mask(model, x)       # eval-mode forward (BatchNorm from running statistics) + argmax, uint8 [N,H,W]

    x = infer.preprocess(img, input_size=(512, 512))   # + the reference's cubic scipy.ndimage.zoom resize, on the device
    predict = infer.GraphedPredictor(model, x)         # the same call replayed from a HIP graph for inputs of x's shape

Binary (one-logit) models, the reference's test.py:391-455 and loss.py:422-440:

    mask = infer.predict_binary_mask(model, x, out_hw=(h, w))      # sigmoid >= 0.5, nearest resize to the image's own size
    mask = infer.predict_binary_mask_tiled(model, x, crop_size)    # the same over crop_size tiles of a padded image
    labels, counts, area, sum_y, sum_x = infer.label_components(mask)   # 8-connected components, all on the device
    counts = infer.count_objects(mask)

    scores = infer.score_binary_masks(mask, gt_dots, [5, 20], np.arange(0.5, 1, 0.05))   # localisation metrics per image

Images larger than the network input, any model (umi/tiles.py: overlap-tile or windowed sliding average, stitched on the device):

    plan = tiles.TilePlan.overlap_tile(H, W, 512, halo=64)
    logits = infer.predict_logits_tiled(model, x, plan, batch=8)   # fp32 (K,H,W); predict_mask_tiled: the uint8 (H,W) mask
    predict = infer.TiledPredictor(model, plan, channels)          # the chunk replayed from a HIP graph

Test-time augmentation over the rot90 / flip views the models are trained under, and model ensembles (umi/tta.py):

    probs = infer.predict_logits_tta(model, x, views='d4', mode='prob')      # fp32 (N,K,H,W): mean softmax over the eight views
    mask = infer.predict_mask_tta([model_a, model_b], x, 'flips', 'logit')   # uint8 (N,H,W); a list of models is an ensemble
    predict = infer.TTAPredictor(model, x, 'd4', 'prob')                     # views -> forwards -> accumulate from a HIP graph

Multi-class models, the rest of test_mc3serousv5.py (Results2Class / Results3Class) after predict_mask:

    labels, counts, class_counts, label_class, area, sum_y, sum_x = infer.label_class_components(mask, n_classes)
    class_counts = infer.count_class_objects(mask, n_classes)
    scores = infer.score_multiclass_masks(mask, gt_dots, n_classes, [10, 20], np.arange(0.5, 1, 0.05))

Regression (density-map) models, the reference's test_single_reg / test_multiple_reg (umi/peaks.py: the peak rule is the
project's restatement of skimage.feature.peak_local_max, pinned to SciPy; agreement with scikit-image itself is unmeasured):

    pred = infer.predict_density(model, x, out_hw=(h, w))           # relu -> order-0 zoom -> / 200, fp32 (N,H,W) per head
    peaks, p_count = peaks.peak_lists(pred, min_distance=3)          # local maxima as (x, y), value descending
    scores = infer.score_density_maps(pred, gt_dots, [5, 20], np.arange(0.5, 1, 0.05))   # counts, GAME, matching per image

No CPU path: the arithmetic is libunetmi kernels (the resize restates SciPy's spline algorithm, oracle/ref_resize.py).
"""
import contextlib
import struct

import numpy as np
import torch

from . import lib as L
from . import ops


def _modules(models):
    return [m for m in (models if isinstance(models, (list, tuple)) else [models]) if isinstance(m, torch.nn.Module)]


@contextlib.contextmanager
def _eval_mode(models):
    """`models` (a module, a callable, or a list of either): the modules in eval mode for the duration, every training flag
    restored on exit, also on error; anything that is no module is left alone."""
    flags = [(m, m.training) for m in _modules(models)]
    for m, _ in flags:
        m.eval()
    try:
        yield
    finally:
        for m, was_training in flags:
            m.train(was_training)


def _capture(fn, example_inputs, models):
    """`fn` run eagerly once (allocations, pack entries, the shared workspace) and then captured, both under no_grad with
    `models` in eval mode: the umi.graphs.GraphedEval of `fn` that holds the modules' weight-pack caches."""
    from . import graph as G
    from .graphs import GraphedEval
    with _eval_mode(models), torch.no_grad():
        fn(*example_inputs)
        return GraphedEval(fn, example_inputs, pack_cache=[G.pack_cache_of(m) for m in _modules(models)])


def zoom_cubic(img, input_size):
    """scipy.ndimage.zoom(img, (input_size[0] / H, input_size[1] / W[, 1]), order=3) of one HWC / HW image on the device
    (reference test_mc3serousv5.py:100-113); uint8 or float32 in, same type out.  `img`: numpy array or tensor.
    Like SciPy's default mode='constant', an output whose sample coordinate i * ((in - 1) / (out - 1)) (float64) lies above
    in - 1 on either axis is 0: the whole last row / column for some sizes, e.g. 32, 512, 1000, 2048 -> 224.  uint8 outputs are
    SciPy's except at exact half-way values k + 0.5 (2- and 3-pixel axes), which may round the other way; float32 outputs are
    within one float32 ulp of SciPy's (oracle/ref_resize.py, tests/test_oracle_resize.py)."""
    if isinstance(img, np.ndarray):
        img = torch.from_numpy(np.ascontiguousarray(img))
    hw = img.dim() == 2
    if hw:
        img = img.unsqueeze(-1)
    if img.dim() != 3 or img.shape[2] > 4:
        raise ValueError(f"expected an HW or HWC image with at most 4 channels, got {tuple(img.shape)}")
    if img.dtype not in (torch.uint8, torch.float32):
        img = img.float()
    img = img.contiguous().to("cuda", non_blocking=True)
    H, W, C = img.shape
    oh, ow = int(round(H * (input_size[0] / H))), int(round(W * (input_size[1] / W)))
    out = torch.empty((oh, ow, C), dtype=img.dtype, device=img.device)
    nbytes = L.fn("umi_zoom_cubic_ws_bytes")(H, W, C)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=img.device)
    L.call("umi_zoom_cubic_hwc", img.data_ptr(), 0 if img.dtype == torch.uint8 else 1, out.data_ptr(), H, W, C, oh, ow,
           ws.data_ptr(), nbytes, ops._stream())
    return out[..., 0] if hw else out


def preprocess(img, reverse_channels=None, input_size=None):
    """Per-channel z-normalisation of one image, HWC (or HW) -> [1,C,H,W] fp32 (reference `preprocess`: mean / np.std over
    H,W in fp64).  The reference reverses the channel order of EVERY 3-D (HWC) input (`transpose((2, 0, 1))[::-1]`,
    test_mc3serousv5.py:124: BGR -> RGB for cv2 images, but 2- and 4-channel inputs are reversed as well) and leaves 2-D
    (HW) inputs alone; `reverse_channels=None` follows that rule, True / False override it.
    `input_size` = (H, W) of the network input: an image of another size is first resized like the reference does, with the
    cubic `scipy.ndimage.zoom` (zoom_cubic above, on the device: SciPy's values, zeroed last row / column included, up to the
    half-way and ulp caveats there)."""
    if input_size is not None:
        shp = img.shape
        if shp[0] != input_size[0] or shp[1] != input_size[1]:
            was_2d = len(shp) == 2
            img = zoom_cubic(img, input_size)
            if reverse_channels is None:
                reverse_channels = not was_2d
    if isinstance(img, np.ndarray):
        img = torch.from_numpy(np.ascontiguousarray(img))
    was_hwc = img.dim() == 3
    if img.dim() == 2:
        img = img.unsqueeze(-1)
    if img.dim() != 3 or img.shape[2] > 4:
        raise ValueError(f"expected an HW or HWC image with at most 4 channels, got {tuple(img.shape)}")
    if img.dtype not in (torch.uint8, torch.float32):
        img = img.float()
    img = img.contiguous().to("cuda", non_blocking=True)
    H, W, C = img.shape
    if reverse_channels is None:
        reverse_channels = was_hwc
    out = torch.empty((1, C, H, W), dtype=torch.float32, device=img.device)
    nbytes = L.fn("umi_znorm_ws_bytes")()
    ws = ops.workspace(nbytes, img.device)
    L.call("umi_znorm_hwc", img.data_ptr(), 0 if img.dtype == torch.uint8 else 1, out.data_ptr(), H * W, C,
           int(bool(reverse_channels)), ws.data_ptr(), nbytes, ops._stream())
    return out


def preprocess_crop(img, crop_size):
    """Reference `preprocessCrop` (test.py:91-128) for the image: HW / HWC (C <= 4) -> [1,C,Hp,Wp] fp32 with Hp, Wp the next
    multiples of crop_size, the image centred (pad_top = padding_h // 2, pad_left = padding_w // 2) in a frame of 255,
    z-normalised with the statistics of the whole padded image and channel-reversed like `preprocess`.  The padded image is
    not materialised (umi.augment.grid_image); the result feeds predict_binary_mask_tiled / predict_logits_tiled."""
    from . import augment
    if isinstance(img, np.ndarray):
        img = torch.from_numpy(np.ascontiguousarray(img))
    if img.dtype not in (torch.uint8, torch.float32):
        img = img.float()
    img = img.to("cuda", non_blocking=True)
    H, W = img.shape[:2]
    crop_size = int(crop_size)
    if crop_size < 1:
        raise ValueError(f"crop_size {crop_size}")
    Hp, Wp = H + (-H) % crop_size, W + (-W) % crop_size
    top, left = augment.center_pad(H, W, crop_size)
    return augment.grid_image(img, top, left, Hp, Wp, pad_value=255, padded=(Hp, Wp))


def argmax_mask(logits):
    """[N,C,H,W] fp32 logits -> uint8 [N,H,W] class mask (== softmax(dim=1).argmax(dim=1), first maximum wins)."""
    ops._need_cuda(logits)
    if logits.dim() != 4 or logits.dtype != torch.float32:
        raise ValueError("argmax_mask expects fp32 logits [N,C,H,W]")
    logits = logits.contiguous()
    N, C, H, W = logits.shape
    mask = torch.empty((N, H, W), dtype=torch.uint8, device=logits.device)
    L.call("umi_argmax_mask", logits.data_ptr(), mask.data_ptr(), N, C, H * W, ops._stream())
    return mask


@torch.no_grad()
def predict_mask(model, x):
    """Reference evaluation step (test_mc3serousv5.py:879-885): eval-mode forward, softmax, argmax -> uint8 mask.  The
    model's kernel-layout weight copies are cached between calls (ops.PackCache), so a loop over images packs once."""
    with _eval_mode(model):
        out = model(x.to("cuda"))
        if isinstance(out, tuple):
            return tuple(argmax_mask(o) for o in out)
        return argmax_mask(out)


# fp32 sigmoid(x) >= 0.5 as torch evaluates it (1 / (1 + exp(-x))) holds exactly for x >= this value, not for x >= 0: 1 + exp(-x)
# rounds to 2 for every x down to -0x1.7ffffcp-23.  Found by bisection over fp32 bit patterns against torch.sigmoid on the CPU;
# tests/test_binary_infer.py repeats the bisection on the torch build it runs on.
SIGMOID_HALF_CUTOFF_BITS = 0xB43FFFFE
SIGMOID_HALF_CUTOFF = struct.unpack("<f", struct.pack("<I", SIGMOID_HALF_CUTOFF_BITS))[0]      # -1.7881390590446244e-07


def binary_mask(logits):
    """[N,1,H,W] fp32 device logits -> uint8 [N,H,W], 1 where fp32 sigmoid(x) >= 0.5 (reference test.py:395-399,
    loss.py:425-428).  The kernel compares x with SIGMOID_HALF_CUTOFF, which is where torch's sigmoid reaches exactly 0.5; it
    evaluates no exp.  A NaN logit gives 0 (the reference's np.uint8(nan) is undefined)."""
    ops._need_cuda(logits)
    if logits.dim() != 4 or logits.shape[1] != 1 or logits.dtype != torch.float32:
        raise ValueError(f"binary_mask expects fp32 logits [N,1,H,W], got {tuple(logits.shape)} {logits.dtype}")
    logits = logits.contiguous()
    N, _, H, W = logits.shape
    mask = torch.empty((N, H, W), dtype=torch.uint8, device=logits.device)
    if mask.numel():
        L.call("umi_binary_mask", logits.data_ptr(), mask.data_ptr(), mask.numel(), ops._stream())
    return mask


def zoom_nearest(mask, out_hw):
    """scipy.ndimage.zoom(mask, (out_hw[0] / H, out_hw[1] / W), order=0) of an (H,W) or (N,H,W) uint8 / float32 device mask
    (reference test.py:400-401), same dtype out.  SciPy's rule: output size round(in * zoom); sample coordinate
    i * ((in - 1) / (out - 1)) in float64 (0 when out == 1); source index floor(x + 0.5); like the cubic resize, an output
    whose coordinate exceeds in - 1 on either axis is 0 (the whole last row and column for 512 -> 224)."""
    ops._need_cuda(mask)
    if mask.dim() not in (2, 3) or mask.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"zoom_nearest expects an (H,W) or (N,H,W) uint8 / float32 mask, got {tuple(mask.shape)} {mask.dtype}")
    single = mask.dim() == 2
    m = (mask.unsqueeze(0) if single else mask).contiguous()
    N, H, W = m.shape
    if N < 1 or H < 1 or W < 1:
        raise ValueError(f"empty mask {tuple(mask.shape)}")
    oh, ow = int(round(H * (out_hw[0] / H))), int(round(W * (out_hw[1] / W)))
    if oh < 1 or ow < 1:
        raise ValueError(f"output size {(oh, ow)}")
    out = torch.empty((N, oh, ow), dtype=m.dtype, device=m.device)
    if not L.supported("umi_zoom_nearest", m.data_ptr(), 0 if m.dtype == torch.uint8 else 1, out.data_ptr(), N, H, W, oh, ow,
                       ops._stream()):
        raise ValueError(f"zoom_nearest: unsupported size {tuple(m.shape)} -> {(oh, ow)}")
    return out[0] if single else out


def _component_mask(mask):
    ops._need_cuda(mask)
    if mask.dim() not in (2, 3) or mask.dtype != torch.uint8:
        raise ValueError(f"expected a uint8 (N,H,W) or (H,W) mask, got {tuple(mask.shape)} {mask.dtype}")
    if not mask.is_contiguous():
        raise ValueError("the mask must be contiguous")
    m = mask.unsqueeze(0) if mask.dim() == 2 else mask
    N, H, W = m.shape
    nbytes = L.fn("umi_components_ws_bytes")(N, H, W) if min(N, H, W) >= 1 and max(N, H, W) < 2 ** 31 else 0
    if nbytes == 0:
        raise ValueError(f"label_components: unsupported mask shape {tuple(mask.shape)} (N, H, W >= 1, N * H * W < 2**31)")
    return m, N, H, W, nbytes


def _raise_on_fault(code, what):
    code = int(code)
    if code:
        raise RuntimeError(f"{what}: the union-find reported fault {code} (iteration cap reached or parent chain corrupted); "
                           "the results are invalid")


def label_components(mask, check=False, _fault=False):
    """8-connected components (cv2.connectedComponents(connectivity=8), reference loss.py:432) of a uint8 (N,H,W) or (H,W)
    device mask, foreground = non-zero.  Returns, all on the device and without a host synchronisation:
      labels int32, the mask's shape: 0 = background, 1..n numbered in the raster order of each component's first pixel
             (scipy.ndimage.label's numbering with a full 3x3 structure);
      counts int32 (N,);  area int32 (N,cap);  sum_y, sum_x int64 (N,cap): pixel count and integer coordinate sums per label
             (pixel centroid = sum / area), cap = ceil(H/2) * ceil(W/2), rows beyond counts[n] are 0.
    check=True reads the kernels' fault word back (one synchronisation) and raises if a find / union loop gave up."""
    m, N, H, W, nbytes = _component_mask(mask)
    cap = L.fn("umi_components_cap")(H, W)
    dev = m.device
    labels = torch.empty((N, H, W), dtype=torch.int32, device=dev)
    counts = torch.empty(N, dtype=torch.int32, device=dev)
    area = torch.empty((N, cap), dtype=torch.int32, device=dev)
    sum_y = torch.empty((N, cap), dtype=torch.int64, device=dev)
    sum_x = torch.empty((N, cap), dtype=torch.int64, device=dev)
    ws = ops.workspace(nbytes, dev)
    L.call("umi_label_components", m.data_ptr(), labels.data_ptr(), counts.data_ptr(), area.data_ptr(), sum_y.data_ptr(),
           sum_x.data_ptr(), N, H, W, ws.data_ptr(), nbytes, ops._stream())
    fault = ops.fault_word(ws) if check or _fault else None
    if check:
        _raise_on_fault(fault, "label_components")
    outs = (labels[0] if mask.dim() == 2 else labels), counts, area, sum_y, sum_x
    return outs + (fault,) if _fault else outs


def count_objects(mask, check=False, _fault=False):
    """Number of 8-connected components per image, int32 (N,) on the device: label_components' `counts` without the relabel
    and statistics passes."""
    m, N, H, W, nbytes = _component_mask(mask)
    counts = torch.empty(N, dtype=torch.int32, device=m.device)
    ws = ops.workspace(nbytes, m.device)
    L.call("umi_count_components", m.data_ptr(), counts.data_ptr(), N, H, W, ws.data_ptr(), nbytes, ops._stream())
    fault = ops.fault_word(ws) if check or _fault else None
    if check:
        _raise_on_fault(fault, "count_objects")
    return (counts, fault) if _fault else counts


def sum_trunc(x):
    """int32 (N,): per image of a contiguous fp32 device tensor (N, ...) the float64 sum in a fixed order, truncated toward
    zero: int(np.sum(dot_map[n])), exact for 0/1 maps."""
    ops._need_cuda(x)
    if x.dtype != torch.float32 or x.dim() < 2 or x.numel() == 0:
        raise ValueError(f"sum_trunc expects a non-empty fp32 tensor (N, ...), got {tuple(x.shape)} {x.dtype}")
    x = x.contiguous()
    out = torch.empty(x.shape[0], dtype=torch.int32, device=x.device)
    nbytes = L.fn("umi_sum_trunc_ws_bytes")(x.shape[0])
    ws = ops.workspace(nbytes, x.device)
    L.call("umi_sum_trunc", x.data_ptr(), out.data_ptr(), x.shape[0], x[0].numel(), ws.data_ptr(), nbytes, ops._stream())
    return out


def _binary_head(out, out_hw):
    m = binary_mask(out)
    if out_hw is not None and (int(out_hw[0]) != m.shape[1] or int(out_hw[1]) != m.shape[2]):
        m = zoom_nearest(m, out_hw)
    return m


@torch.no_grad()
def predict_binary_mask(model, x, out_hw=None):
    """Reference evaluation step of a one-logit model (test.py:391-404): eval-mode forward, sigmoid >= 0.5 -> uint8 [N,H,W]
    mask, and the nearest (order-0) resize to `out_hw` = the image's own (height, width) when that differs from the network
    size.  Two-headed models give a tuple of masks, as predict_mask does."""
    with _eval_mode(model):
        out = model(x.to("cuda"))
        if isinstance(out, tuple):
            return tuple(_binary_head(o, out_hw) for o in out)
        return _binary_head(out, out_hw)


def _density_head(out, out_hw, scale):
    from . import peaks as P
    if out.dim() != 4 or out.dtype != torch.float32 or not out.is_cuda:
        raise ValueError(f"predict_density expects fp32 device outputs (N,K,H,W), got {tuple(out.shape)} {out.dtype}")
    N, K, H, W = out.shape
    m = out.contiguous().view(N * K, H, W)
    if out_hw is not None and (int(out_hw[0]) != H or int(out_hw[1]) != W):
        m = zoom_nearest(m, out_hw)               # a gather (0 past the last sample): relu and the division commute with it
    pred, _ = P.density_maps(m, scale)
    return pred if K == 1 else pred.view(N, K, pred.shape[1], pred.shape[2])


@torch.no_grad()
def predict_density(model, x, out_hw=None, scale=200.0):
    """Reference evaluation step of a regression (density-map) model (test_mc3serousv5.py:959-974): eval-mode forward, relu, the
    order-0 zoom to `out_hw` = the image's own (height, width) when that differs from the network size, and the division by
    `scale` (an IEEE division, umi_density_maps) -> fp32 (N,H,W) count map per head ((N,K,H,W) for a head with K > 1 channels).
    A two-headed model gives a tuple in the model's own order; the reference reads it as (immune, other).  `model` may be any
    callable returning fp32 device outputs (n,K,h,w), e.g. `lambda v: predict_logits_tiled(m, v, plan)[None]` or
    `lambda v: predict_logits_tta(m, v, mode='relu')`.  Nothing returns to the host; a module's training flag is restored."""
    with _eval_mode(model):
        out = model(x.to("cuda"))
        if isinstance(out, tuple):
            return tuple(_density_head(o, out_hw, scale) for o in out)
        return _density_head(out, out_hw, scale)


class GraphedPredictor:
    """predict_mask (predict_binary_mask for a one-logit model) replayed from a HIP graph for inputs of one shape:

        predict = infer.GraphedPredictor(model, example_x)
        mask = predict(x)                         # uint8 [N,H,W], or a tuple of them for a two-headed model

    With density=True it replays predict_density(model, x, out_hw, scale) instead and returns fp32 count maps.

    The constructor runs the eval-mode forward once eagerly and captures it, with the mask kernels behind it, in a
    umi.graphs.GraphedEval that holds the model's weight-pack cache: a call copies x into the static input, brings the weight
    copies up to date if a parameter changed since (optimizer step, load_state_dict), replays and returns CLONES of the static
    masks.  Inputs of another shape go through predict_mask / predict_binary_mask.  The model's training flag is left as it was."""

    def __init__(self, model, example_x, density=False, out_hw=None, scale=200.0):
        self.model = model
        self.density, self.out_hw, self.scale = bool(density), out_hw, scale
        x = example_x.to("cuda")
        self.shape, self.dtype = tuple(x.shape), x.dtype

        def fwd(xs):
            out = model(xs)
            self._tuple = isinstance(out, tuple)
            outs = out if self._tuple else (out,)
            self.binary = outs[0].shape[1] == 1
            if self.density:
                return tuple(_density_head(o, out_hw, scale) for o in outs)
            return tuple((binary_mask if o.shape[1] == 1 else argmax_mask)(o) for o in outs)

        self._ge = _capture(fwd, [x], model)

    @torch.no_grad()
    def __call__(self, x):
        x = x.to("cuda")
        if tuple(x.shape) != self.shape or x.dtype != self.dtype:
            if self.density:
                return predict_density(self.model, x, self.out_hw, self.scale)
            return (predict_binary_mask if self.binary else predict_mask)(self.model, x)
        masks = tuple(m.clone() for m in self._ge(x))
        return masks if self._tuple else masks[0]


@torch.no_grad()
def predict_binary_mask_tiled(model, x, crop_size):
    """Reference test_single_crop (test.py:437-448): x (1,C,Hp,Wp) with Hp and Wp multiples of crop_size (`preprocess_crop`
    above pads the image with 255 and normalises it, test.py:91-119); every crop_size tile goes through the network on its
    own, one tile per forward as the reference does, and its thresholded mask is placed into a uint8 (Hp,Wp) mask on the
    device.  Two-headed models give a tuple of masks."""
    crop_size = int(crop_size)
    if x.dim() != 4 or x.shape[0] != 1:
        raise ValueError(f"predict_binary_mask_tiled expects x (1,C,Hp,Wp), got {tuple(x.shape)}")
    Hp, Wp = x.shape[2], x.shape[3]
    if crop_size < 1 or Hp % crop_size or Wp % crop_size or Hp == 0 or Wp == 0:
        raise ValueError(f"the padded image {Hp}x{Wp} is not a whole number of {crop_size}-pixel tiles")
    x = x.to("cuda")
    with _eval_mode(model):
        pred = None
        for i in range(0, Hp, crop_size):
            for j in range(0, Wp, crop_size):
                out = model(x[:, :, i:i + crop_size, j:j + crop_size].contiguous())
                outs = out if isinstance(out, tuple) else (out,)
                if pred is None:
                    pred = [torch.zeros((Hp, Wp), dtype=torch.uint8, device=x.device) for _ in outs]
                for p, o in zip(pred, outs):
                    p[i:i + crop_size, j:j + crop_size] = binary_mask(o)[0]
        return tuple(pred) if isinstance(out, tuple) else pred[0]


# ---- overlap-tile / sliding-window inference over an image larger than the network input (umi/tiles.py, csrc/tiles.hip) -------------
def tile_gather(x, plan, ids, out=None):
    """x fp32 (C,H,W) on the device, ids int32 (n,) DEVICE tile ids (< 0: empty slot) -> fp32 (n,C,th,tw): tiles.gather_numpy."""
    from .tiles import PAD_MODES
    ops._need_cuda(x, ids)
    if x.dim() != 3 or x.dtype != torch.float32 or tuple(x.shape[1:]) != (plan.H, plan.W) or not x.is_contiguous():
        raise ValueError(f"tile_gather expects a contiguous fp32 (C,{plan.H},{plan.W}) image, got {tuple(x.shape)} {x.dtype}")
    if ids.dim() != 1 or ids.dtype != torch.int32 or not ids.is_contiguous() or ids.numel() < 1:
        raise ValueError(f"tile_gather expects contiguous int32 (n,) ids, got {tuple(ids.shape)} {ids.dtype}")
    C, n = x.shape[0], ids.numel()
    if out is None:
        out = torch.empty((n, C, plan.th, plan.tw), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (n, C, plan.th, plan.tw) or out.dtype != torch.float32 or not out.is_cuda or not out.is_contiguous():
        raise ValueError(f"tile_gather: `out` must be a contiguous fp32 device tensor ({n},{C},{plan.th},{plan.tw}), got "
                         f"{tuple(out.shape)} {out.dtype}")
    oy, ox = plan.device_tables(x.device)[:2]
    L.call("umi_tile_gather", x.data_ptr(), C, plan.H, plan.W, out.data_ptr(), plan.th, plan.tw, oy.data_ptr(), ox.data_ptr(),
           plan.ny, plan.nx, ids.data_ptr(), n, PAD_MODES[plan.pad], plan.pad_value, ops._stream())
    return out


def tile_blend(acc, logits, plan, ids):
    """acc fp32 (K,H,W) += the chunk's windowed logits fp32 (n,K,th,tw), in place: tiles.blend_numpy, bit for bit."""
    ops._need_cuda(acc, logits, ids)
    n = ids.numel()
    if logits.dtype != torch.float32 or logits.dim() != 4 or tuple(logits.shape[2:]) != (plan.th, plan.tw) or logits.shape[0] != n:
        raise ValueError(f"tile_blend expects fp32 logits ({n},K,{plan.th},{plan.tw}), got {tuple(logits.shape)} {logits.dtype}")
    K = logits.shape[1]
    if acc.dtype != torch.float32 or tuple(acc.shape) != (K, plan.H, plan.W) or not acc.is_contiguous():
        raise ValueError(f"tile_blend expects a contiguous fp32 canvas ({K},{plan.H},{plan.W}), got {tuple(acc.shape)} {acc.dtype}")
    if ids.dtype != torch.int32 or ids.dim() != 1 or not ids.is_contiguous():
        raise ValueError(f"tile_blend expects contiguous int32 (n,) ids, got {tuple(ids.shape)} {ids.dtype}")
    logits = logits.contiguous()
    oy, ox, wy, wx = plan.device_tables(acc.device)[:4]
    L.call("umi_tile_blend", logits.data_ptr(), K, plan.th, plan.tw, acc.data_ptr(), plan.H, plan.W, oy.data_ptr(), ox.data_ptr(),
           plan.ny, plan.nx, wy.data_ptr(), wx.data_ptr(), ids.data_ptr(), n, ops._stream())
    return acc


def tile_finish(acc, plan, mask=False):
    """The canvas of window-weighted sums -> stitched logits, in place (tiles.finish_numpy); mask=True also returns the uint8 (H,W)
    mask of the stitched logits: binary_mask's rule for one logit, argmax_mask's otherwise."""
    ops._need_cuda(acc)
    if acc.dtype != torch.float32 or acc.dim() != 3 or tuple(acc.shape[1:]) != (plan.H, plan.W) or not acc.is_contiguous():
        raise ValueError(f"tile_finish expects a contiguous fp32 canvas (K,{plan.H},{plan.W}), got {tuple(acc.shape)} {acc.dtype}")
    sy, sx = plan.device_tables(acc.device)[4:]
    m = torch.empty((plan.H, plan.W), dtype=torch.uint8, device=acc.device) if mask else None
    L.call("umi_tile_finish", acc.data_ptr(), acc.shape[0], plan.H, plan.W, sy.data_ptr(), sx.data_ptr(),
           m.data_ptr() if mask else None, ops._stream())
    return (acc, m) if mask else acc


def _tiled_image(x, plan):
    if x.dim() != 4 or x.shape[0] != 1 or tuple(x.shape[2:]) != (plan.H, plan.W):
        raise ValueError(f"expected x (1,C,{plan.H},{plan.W}) for this plan, got {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise ValueError(f"expected an fp32 image, got {x.dtype}")
    return x.to("cuda")[0].contiguous()


def _chunk_ids(plan, batch, device):
    return torch.from_numpy(plan.chunks(batch)).to(device)


def _tiled_chunk(model, x3, plan, ids, canvases, tiles=None):
    """One chunk: gather -> eval forward -> blend into `canvases` (a list filled with zeroed canvases on the first chunk).
    Returns whether the model is two-headed."""
    out = model(tile_gather(x3, plan, ids, tiles))
    outs = out if isinstance(out, tuple) else (out,)
    if not canvases:
        canvases.extend(torch.zeros((o.shape[1], plan.H, plan.W), dtype=torch.float32, device=x3.device) for o in outs)
    for acc, o in zip(canvases, outs):
        tile_blend(acc, o, plan, ids)
    return isinstance(out, tuple)


@torch.no_grad()
def _predict_tiled(model, x, plan, batch, mask):
    x3 = _tiled_image(x, plan)
    ids = _chunk_ids(plan, batch, x3.device)
    with _eval_mode(model):
        canvases, two = [], False
        for c in range(ids.shape[0]):
            two = _tiled_chunk(model, x3, plan, ids[c], canvases)
        res = tuple(tile_finish(acc, plan, mask) for acc in canvases)
        if mask:
            res = tuple(m for _, m in res)
        return res if two else res[0]


def predict_logits_tiled(model, x, plan, batch=8):
    """Whole-image logits of a model whose input is one tile of `plan` (umi.tiles.TilePlan over x's H x W): x (1,C,H,W) fp32 ->
    fp32 (K,H,W) stitched logits on the device, a tuple of them for a two-headed model.  Eval-mode forwards over chunks of `batch`
    tiles in ascending id order (the last chunk padded with empty slots, which go through the network as zero tiles and are not
    blended): umi_tile_gather -> model -> umi_tile_blend per chunk, then umi_tile_finish; nothing returns to the host.  The
    stitching is umi.tiles' NumPy statement bit for bit and does not depend on `batch`; the model's training flag is restored."""
    return _predict_tiled(model, x, plan, batch, False)


def predict_mask_tiled(model, x, plan, batch=8):
    """predict_logits_tiled, returning the uint8 (H,W) mask of the stitched logits instead (a tuple for a two-headed model): the
    threshold of binary_mask for a one-logit model, argmax_mask's first maximum otherwise, written by the finish kernel.  With
    TilePlan.overlap_tile(H, W, crop_size, 0) on a padded image this is predict_binary_mask_tiled with `batch` tiles per forward."""
    return _predict_tiled(model, x, plan, batch, True)


class TiledPredictor:
    """predict_logits_tiled / predict_mask_tiled with the chunk replayed from a HIP graph:

        predict = infer.TiledPredictor(model, plan, channels, batch=8)
        logits = predict(x)                       # fp32 (K,H,W), or a tuple for a two-headed model
        mask = predict.predict_mask(x)            # uint8 (H,W)

    The constructor runs one chunk eagerly and captures it (gather -> eval forward -> blend into static canvases) in a
    umi.graphs.GraphedEval holding the model's weight-pack cache.  A call copies the image into the static input once, zeroes the
    canvases, replays the graph once per chunk with that chunk's ids copied into the static id buffer, runs the finish kernel behind
    the last replay and returns CLONES.  A replay after an optimizer step or load_state_dict reads the current weights, as
    GraphedPredictor does.  The model's training flag is left as it was."""

    def __init__(self, model, plan, channels, batch=8):
        self.model, self.plan = model, plan
        dev = torch.device("cuda", torch.cuda.current_device())
        self._ids = _chunk_ids(plan, batch, dev)
        x3 = torch.zeros((int(channels), plan.H, plan.W), dtype=torch.float32, device=dev)
        self._tiles = torch.empty((self._ids.shape[1], int(channels), plan.th, plan.tw), dtype=torch.float32, device=dev)
        self._canvases = []

        def chunk(xs, ids):
            self._tuple = _tiled_chunk(model, xs, plan, ids, self._canvases, self._tiles)
            return ()

        self._ge = _capture(chunk, [x3, self._ids[0]], model)

    @torch.no_grad()
    def _run(self, x, mask):
        x3 = _tiled_image(x, self.plan)
        xs = self._ge.static_inputs[0]
        if tuple(x3.shape) != tuple(xs.shape):
            raise ValueError(f"this TiledPredictor was built for {xs.shape[0]} channels, got {x3.shape[0]}")
        xs.copy_(x3, non_blocking=True)
        for acc in self._canvases:
            acc.zero_()
        for c in range(self._ids.shape[0]):
            self._ge(xs, self._ids[c])            # xs is the static input itself: only the ids are copied
        res = tuple(tile_finish(acc, self.plan, mask) for acc in self._canvases)
        res = tuple(m for _, m in res) if mask else tuple(acc.clone() for acc in res)
        return res if self._tuple else res[0]

    def __call__(self, x):
        return self._run(x, False)

    def predict_mask(self, x):
        return self._run(x, True)


# ---- test-time augmentation over the rot90 / flip views, and model ensembles (umi/tta.py, csrc/tta.hip) ------------------------------
def _tta_models(model):
    models = list(model) if isinstance(model, (list, tuple)) else [model]
    if not models:
        raise ValueError("an empty list of models")
    return models


def _tta_input(x):
    if x.dim() != 4 or x.dtype != torch.float32 or x.numel() == 0:
        raise ValueError(f"expected a non-empty fp32 batch (N,C,H,W), got {tuple(x.shape)} {x.dtype}")
    return x.to("cuda").contiguous()


def _tta_forward(model, v, batch):
    """model over the rows of v in chunks of at most `batch` -> a list (one entry per head) of fp32 (rows,K,h,w) and whether the
    model is two-headed."""
    rows = v.shape[0]
    step = rows if batch is None else int(batch)
    heads, two = None, False
    for a in range(0, rows, step):
        out = model(v[a:a + step])
        two = isinstance(out, tuple)
        outs = out if two else (out,)
        for o in outs:
            if o.dim() != 4 or o.dtype != torch.float32 or not o.is_cuda or o.shape[0] != min(step, rows - a):
                raise ValueError(f"a model under TTA must return fp32 device logits (n,K,h,w) for n view-images, got "
                                 f"{tuple(o.shape)} {o.dtype}")
        if heads is None:
            if step >= rows:
                return [o.contiguous() for o in outs], two
            heads = [torch.empty((rows,) + tuple(o.shape[1:]), dtype=torch.float32, device=v.device) for o in outs]
        for h, o in zip(heads, outs):
            h[a:a + step] = o
    return heads, two


def _tta_accumulate(models, x, elements, mode, batch, accs):
    """Every model's outputs over every view of x, accumulated into `accs` (a list filled with zeroed (N,K,H,W) sums on first use)
    model after model and, per pixel, in the order of `elements`.  The views of one shape go through a model together (in chunks of
    `batch` view-images) and their outputs are kept; the accumulate calls then walk the tuple in runs of one shape, so the order
    of the sum is the tuple's whatever the shapes and the chunks.  Returns whether the models are two-headed."""
    from . import tta as T
    N, _, H, W = x.shape
    classes = T.shape_classes(elements, H, W)
    vx = {shape: T.views(x, [elements[p] for p in pos]) for shape, pos in classes.items()}
    slot = {p: (shape, s) for shape, pos in classes.items() for s, p in enumerate(pos)}
    two = False
    for model in models:
        outs = {}
        for shape in classes:
            outs[shape], two = _tta_forward(model, vx[shape], batch)
        if not accs:
            accs.extend(torch.zeros((N, o.shape[1], H, W), dtype=torch.float32, device=x.device) for o in next(iter(outs.values())))
        a = 0
        while a < len(elements):
            shape, s0 = slot[a]
            b = a + 1
            while b < len(elements) and b - a < T.MAX_CALL_VIEWS and slot[b] == (shape, s0 + b - a):
                b += 1
            for acc, o in zip(accs, outs[shape]):
                T.accumulate(acc, o[s0 * N:(s0 + b - a) * N], elements[a:b], mode)
            a = b
    return two


def _tta_finish(accs, count, mode, mask, entropy, two, clone=False):
    from . import tta as T
    res = []
    for acc in accs:
        r = T.finish(acc, count, mode, mask=mask, entropy=entropy)
        r = list(r) if isinstance(r, tuple) else [r]
        mean = r.pop(0)
        head = r.pop(0) if mask else (mean.clone() if clone else mean)
        res.append((head, r[0]) if entropy else head)
    return tuple(res) if two else res[0]


@torch.no_grad()
def _predict_tta(model, x, views, mode, batch, entropy, mask):
    from . import tta as T
    elements = T.view_set(views)
    T.check_mode(mode)
    if entropy and mode != "prob":
        raise ValueError("the entropy map exists in 'prob' mode only")
    if batch is not None and int(batch) < 1:
        raise ValueError(f"batch must be >= 1 or None, got {batch}")
    x = _tta_input(x)
    models = _tta_models(model)
    with _eval_mode(models):
        accs = []
        two = _tta_accumulate(models, x, elements, mode, batch, accs)
        return _tta_finish(accs, len(elements) * len(models), mode, mask, entropy, two)


def predict_logits_tta(model, x, views="d4", mode="prob", batch=None, entropy=False):
    """Test-time augmentation (umi/tta.py): the model's outputs over the rot90 / flip views of x (N,C,H,W) fp32, mapped back and
    averaged on the device -> fp32 (N,K,H,W): the mean logits ('logit'), the mean of the rectified outputs ('relu') or the mean
    softmax / sigmoid probabilities ('prob').  views: 'none', 'flips', 'd4' or a tuple of elements 0..7.  entropy=True ('prob')
    returns (mean, entropy) with the fp32 (N,H,W) predictive entropy of the mean probabilities.  A two-headed model gives a tuple.

    Eval-mode forwards over chunks of at most `batch` view-images (None: all views of one shape at once); with H != W the odd
    turns form a second batch of shape (W,H).  The sum runs per pixel in the order of `views` whatever the chunks: 'logit' and
    'relu' are tta.merge_numpy bit for bit, 'prob' within tta.prob_bound.  Nothing returns to the host; the training flags are
    restored.  `model` may also be a callable returning fp32 device logits (n,K,h,w) for n view-images, e.g.
    `lambda v: predict_logits_tiled(m, v, plan)[None]` with batch=1, or a list of models or callables: the per-seed ensemble of
    train.py, accumulated model after model and divided by len(views) * len(models)."""
    return _predict_tta(model, x, views, mode, batch, entropy, False)


def predict_mask_tta(model, x, views="d4", mode="prob", batch=None, entropy=False):
    """predict_logits_tta, returning the uint8 (N,H,W) mask of the mean instead, written by the finish kernel: argmax_mask's rule
    (K >= 2); for one logit binary_mask's rule on the mean logit, or mean probability >= 0.5 in 'prob' mode.  entropy=True:
    (mask, entropy)."""
    return _predict_tta(model, x, views, mode, batch, entropy, True)


class TTAPredictor:
    """predict_logits_tta / predict_mask_tta replayed from a HIP graph for inputs of one shape:

        predict = infer.TTAPredictor(model, example_x, views='d4', mode='prob')
        mean = predict(x)                         # fp32 (N,K,H,W); predict(x, entropy=True): (mean, entropy)
        mask = predict.predict_mask(x)            # uint8 (N,H,W)

    The constructor runs views -> forward(s) -> accumulate once eagerly and captures it in a umi.graphs.GraphedEval holding the
    models' weight-pack caches; a call copies x into the static input, replays (the sums are zeroed inside the graph), runs the
    finish kernel behind the replay and returns CLONES.  As GraphedPredictor: a replay after an optimizer step or load_state_dict
    reads the current weights, inputs of another shape go through the eager functions, the training flags are left as they were.
    `model` may be a list of models (an ensemble)."""

    def __init__(self, model, example_x, views="d4", mode="prob", batch=None):
        from . import tta as T
        self.model, self.views, self.mode, self.batch = model, T.view_set(views), mode, batch
        T.check_mode(mode)
        models = _tta_models(model)
        x = _tta_input(example_x)
        self.shape = tuple(x.shape)
        self._accs = []

        def fwd(xs):
            for acc in self._accs:
                acc.zero_()
            self._tuple = _tta_accumulate(models, xs, self.views, mode, batch, self._accs)
            return ()

        self._count = len(self.views) * len(models)
        self._ge = _capture(fwd, [x], models)

    @torch.no_grad()
    def _run(self, x, entropy, mask):
        if tuple(x.shape) != self.shape or x.dtype != torch.float32:
            return _predict_tta(self.model, x, self.views, self.mode, self.batch, entropy, mask)
        if entropy and self.mode != "prob":
            raise ValueError("the entropy map exists in 'prob' mode only")
        self._ge(x.to("cuda"))
        return _tta_finish(self._accs, self._count, self.mode, mask, entropy, self._tuple, clone=True)

    def __call__(self, x, entropy=False):
        return self._run(x, entropy, False)

    def predict_mask(self, x, entropy=False):
        return self._run(x, entropy, True)


def score_binary_masks(mask, gt_dots, sigma_list, sigma_thresh_list, dist_thresh=10, size=512):
    """What the reference's `ResultsCC.compareImages` (test.py:227-271) appends for each image of a batch, computed on the
    device with ONE device-to-host copy: `mask` uint8 (N,H,W) predicted masks, `gt_dots` uint8 / float32 (N,H,W) 0/1 dot maps.
    label_components -> centres -> Gaussian matching (CrowdMatchingTest) and distance matching (CrowdMatchingTest2) against the
    dot lists -> grid sums of the dot map and of the map with a 1 at every centre (GMAE at levels 1-3 over `size` pixels).

    Returns a list of N dicts: 'GT', 'Pred' (dot and component counts), 'AbsDiff', 'RelativeAccuracy', 'G1', 'G2', 'G3',
    'arr_prec', 'arr_recall', 'arr_f1' ((S, T) float64 arrays), 'precision', 'recall', 'f1'.  An image with components but no
    dots raises ZeroDivisionError, as the reference's CrowdMatchingTest2 does.

    The centres are PIXEL centroids, round(sum / area) half to even (umi.matching.component_centers).  The reference's
    `_findObjects` uses cv2.moments of the cv2.findContours outline, a different number that also drops components whose
    outline encloses no area (while still counting them); OpenCV is not available to this project, so that definition is not
    reproduced and 'Pred' here is the number of 8-connected components."""
    import CrowdMatching as CM
    from . import matching as M
    if gt_dots.shape != mask.shape or mask.dim() != 3:
        raise ValueError(f"score_binary_masks expects (N,H,W) masks and dot maps of one shape, got {tuple(mask.shape)} "
                         f"{tuple(gt_dots.shape)}")
    ops._need_cuda(mask, gt_dots)
    N, H, W = mask.shape
    _, counts, area, sum_y, sum_x, cc_fault = label_components(mask, _fault=True)
    centers = M.component_centers(counts, area, sum_y, sum_x)
    dots, g_count, dot_fault = M.dot_lists(gt_dots, _fault=True)
    crowd = M.crowd_match(dots, g_count, centers, counts, sigma_list, sigma_thresh_list)
    dist = M.distance_match(dots, g_count, centers, counts, dist_thresh)
    cells_gt = M.grid_sums(gt_dots, size).to(torch.int64)           # sums of a 0/1 map: exact in either type
    cells_pred = M.grid_sums(M.scatter_centers(centers, counts, H, W), size)
    cc_code, dot_code, counts_h, g_h, crowd_h, dist_h, cg, cp = ops.read_back(cc_fault, dot_fault, counts, g_count, crowd, dist,
                                                                              cells_gt, cells_pred)
    if cc_code[0]:
        raise RuntimeError(f"score_binary_masks: the union-find reported fault {cc_code[0]}; the results are invalid")
    M.raise_on_dot_overflow(dot_code[0])
    out = []
    for n in range(N):
        gt, pred = int(g_h[n]), int(counts_h[n])
        abs_diff, rel, _, _ = CM.countAccuracyMetric(gt, pred)
        arr_prec, arr_recall, arr_f1 = CM.precision_recall_f1(crowd_h[n], gt, pred)
        tp, nc, ng = (int(v) for v in dist_h[n])
        prec, recall, f1 = (0, 0, 0) if nc == 0 else CM._prf_distance(tp, nc, ng)
        out.append({"GT": gt, "Pred": pred, "AbsDiff": abs_diff, "RelativeAccuracy": rel,
                    "G1": CM.game_from_cells(1, cg[n], cp[n])[0], "G2": CM.game_from_cells(2, cg[n], cp[n])[0],
                    "G3": CM.game_from_cells(3, cg[n], cp[n])[0],
                    "arr_prec": arr_prec, "arr_recall": arr_recall, "arr_f1": arr_f1,
                    "precision": prec, "recall": recall, "f1": f1})
    return out


# ---- class-valued masks ----------------------------------------------------------------------------------------------------------
_CLASS_FAULTS = {5: "the mask holds a value >= n_classes (taken as background)",
                 6: "an image has more components than max_components; counts and labels are exact, the statistics rows hold "
                    "the first max_components labels only"}


def _raise_on_class_fault(code, what):
    code = int(code)
    if code:
        raise RuntimeError(f"{what}: " + _CLASS_FAULTS.get(code, f"the union-find reported fault {code} (iteration cap reached or "
                                                                 "parent chain corrupted); the results are invalid"))


def _class_component_mask(mask, n_classes):
    from .components import MAX_CLASSES
    K = int(n_classes)
    if not 2 <= K <= MAX_CLASSES:
        raise ValueError(f"n_classes must be in 2..{MAX_CLASSES}, got {n_classes}")
    m, N, H, W, _ = _component_mask(mask)
    nbytes = L.fn("umi_class_components_ws_bytes")(N, H, W, K)
    if nbytes == 0:
        raise ValueError(f"label_class_components: unsupported mask shape {tuple(mask.shape)}")
    return m, N, H, W, K, nbytes


def _label_class_components(mask, n_classes, max_components, _fault=True):
    """label_class_components' seven outputs and the kernels' fault word (ops.fault_word: a tensor of its own; None without _fault)."""
    from .components import class_components_cap
    m, N, H, W, K, nbytes = _class_component_mask(mask, n_classes)
    cap = class_components_cap(H, W, K) if max_components is None else int(max_components)
    if not 1 <= cap <= H * W:
        raise ValueError(f"max_components must be in 1..{H * W}, got {max_components}")
    dev = m.device
    labels = torch.empty((N, H, W), dtype=torch.int32, device=dev)
    counts = torch.empty(N, dtype=torch.int32, device=dev)
    class_counts = torch.empty((N, K), dtype=torch.int32, device=dev)
    label_class = torch.empty((N, cap), dtype=torch.uint8, device=dev)
    area = torch.empty((N, cap), dtype=torch.int32, device=dev)
    sum_y = torch.empty((N, cap), dtype=torch.int64, device=dev)
    sum_x = torch.empty((N, cap), dtype=torch.int64, device=dev)
    ws = ops.workspace(nbytes, dev)
    L.call("umi_label_class_components", m.data_ptr(), labels.data_ptr(), counts.data_ptr(), class_counts.data_ptr(),
           label_class.data_ptr(), area.data_ptr(), sum_y.data_ptr(), sum_x.data_ptr(), N, H, W, K,
           cap, ws.data_ptr(), nbytes, ops._stream())
    return ((labels[0] if mask.dim() == 2 else labels), counts, class_counts, label_class, area, sum_y, sum_x), \
        (ops.fault_word(ws) if _fault else None)


def label_class_components(mask, n_classes, max_components=None, check=False):
    """Class-aware 8-connected components of a uint8 (N,H,W) or (H,W) device mask of class values 0 .. n_classes - 1
    (2 <= n_classes <= 8), e.g. predict_mask's output: two pixels belong to one component iff they are 8-connected through
    pixels of the same non-zero value -- scipy.ndimage.label(mask == c, ones((3, 3))) for every c, all classes in one set of
    launches (reference test_mc3serousv5.py:410-443 `_findObjects` loops over the classes on the host).  Returns, all on the
    device and without a host synchronisation:
      labels int32, the mask's shape: 0 = background, 1..n over ALL classes in the raster order of each component's first pixel;
      counts int32 (N,);  class_counts int32 (N, n_classes), column 0 is 0;  label_class uint8 (N, cap): the class of label i + 1;
      area int32 (N, cap);  sum_y, sum_x int64 (N, cap);  rows beyond counts[n] are 0.
    cap = max_components (1 .. H * W), by default min(n_classes - 1, 4) * ceil(H/2) * ceil(W/2) (at most H * W), which no mask
    exceeds: a 2 x 2 block meets one component per class.  With a smaller max_components an image that has more components
    keeps exact counts, class_counts and labels, gets the rows of its first cap labels, and sets a fault code; a mask value
    >= n_classes is taken as background and sets another (the first of the two stays; a union-find fault overrides both).  check=True reads the fault word back (one synchronisation) and
    raises on either, and on a union-find fault.  With n_classes = 2 and the default cap, labels, counts, area and the sums
    are label_components' bit for bit on a 0/1 mask."""
    outs, fault = _label_class_components(mask, n_classes, max_components, _fault=check)
    if check:
        _raise_on_class_fault(fault, "label_class_components")
    return outs


def count_class_objects(mask, n_classes, check=False, _fault=False):
    """Number of components per image and class, int32 (N, n_classes) on the device (column 0 is 0): label_class_components'
    `class_counts` without the flatten, rank, relabel and statistics passes."""
    m, N, H, W, K, nbytes = _class_component_mask(mask, n_classes)
    class_counts = torch.empty((N, K), dtype=torch.int32, device=m.device)
    ws = ops.workspace(nbytes, m.device)
    L.call("umi_count_class_components", m.data_ptr(), class_counts.data_ptr(), N, H, W, K, ws.data_ptr(), nbytes,
           ops._stream())
    fault = ops.fault_word(ws) if check or _fault else None
    if check:
        _raise_on_class_fault(fault, "count_class_objects")
    return (class_counts, fault) if _fault else class_counts


def score_multiclass_masks(mask, gt_dots, n_classes, sigma_list, sigma_thresh_list, size=512, max_components=65536):
    """What the reference's multi-class evaluation (test_mc3serousv5.py `Results2Class.compareImages` :481-566, and for four
    classes the counts and ratios of `Results3Class.compareImages` :218-255) records for each image of a batch, computed on
    the device with ONE device-to-host copy.  `mask` uint8 (N,H,W) class values 0 .. n_classes - 1 (predict_mask's output, after
    zoom_nearest if the sizes differ), `gt_dots` uint8 (N,H,W) whose value is the class of the dot.
    label_class_components -> per-class centre lists; split_classes(gt_dots) -> per-class dot lists; Gaussian matching
    (CrowdMatchingTest, inputType='Coordinates') and the 8 x 8 grid sums of the dot planes and of the maps with a 1 at every
    centre (GMAE levels 1-3 over `size` pixels), each per (image, class).

    Returns a list of N dicts.  d[c] for c in 1 .. n_classes - 1: 'GT' (dots of value c), 'Pred' (components of class c),
    'AbsDiff', 'Accuracy', 'AccuracyRelative', 'AccuracyRelativePD' (CrowdMatching.countAccuracyMetric), 'G1', 'G2', 'G3'
    (each [gmae, relative, relativePD], CrowdMatching.game_from_cells), 'arr_prec', 'arr_recall', 'arr_f1' ((S, T) float64).
    For n_classes >= 3, d['ratio']: class 2 / (class 1 + class 2) of the ground truth and the prediction with the four metrics
    (umi.matching.ratio_metrics, :499-501).  For n_classes == 4, d['ratio3']: Results3Class's three count accuracies and two
    ratios with their 1e-6 smoothing (umi.matching.ratio3_metrics); the ground-truth counts there are the dot counts.

    Every float is the reference's expression on Python ints.  Where the reference is undefined: a prediction without a
    component of class 1 or 2 raises ZeroDivisionError, as the reference's ratio does; the reference's ground-truth counts are
    numpy.uint64, so its abs(gt - pred) wraps to ~1.8e19 when the prediction is larger -- that is NOT reproduced, the
    differences are those of ints; a ground truth without a dot of class 1 or 2 gives d['ratio']['GT'] = nan (the reference's
    uint64 0 / 0).  More than max_components components in an image raises RuntimeError.

    As on the binary path: 'Pred' is the number of 8-connected components (the reference's len(cv2.findContours(RETR_EXTERNAL))
    may leave out a component inside a hole of another; OpenCV is not available, so that is not claimed); centres are pixel
    centroids, not contour moments; Results3Class's cv2.minEnclosingCircle matching (:257-289) is not restated."""
    from . import matching as M
    if gt_dots.shape != mask.shape or mask.dim() != 3:
        raise ValueError(f"score_multiclass_masks expects (N,H,W) masks and dot maps of one shape, got {tuple(mask.shape)} "
                         f"{tuple(gt_dots.shape)}")
    ops._need_cuda(mask, gt_dots)
    N, H, W = mask.shape
    K = int(n_classes)
    cap = min(int(max_components), H * W)
    (_, counts, class_counts, label_class, area, sum_y, sum_x), cc_fault = _label_class_components(mask, K, cap)
    centers, c_count = M.class_center_lists(counts, label_class, area, sum_y, sum_x, K)
    planes = M.split_classes(gt_dots, K).view(N * (K - 1), H, W)
    dots, g_count, dot_fault = M.dot_lists(planes, _fault=True)
    crowd = M.crowd_match(dots, g_count, centers, c_count, sigma_list, sigma_thresh_list)
    cells_gt = M.grid_sums(planes, size)
    cells_pred = M.grid_sums(M.scatter_centers(centers, c_count, H, W), size)
    cc_code, dot_code, *host = ops.read_back(cc_fault, dot_fault, class_counts, g_count, c_count, crowd, cells_gt, cells_pred)
    _raise_on_class_fault(cc_code[0], "score_multiclass_masks")
    M.raise_on_dot_overflow(dot_code[0])
    return M.multiclass_scores(*host, K)


# ---- density maps ----------------------------------------------------------------------------------------------------------------
def score_density_maps(pred, gt_dots, sigma_list, sigma_thresh_list, size=512, min_distance=3, floor=1e-3):
    """What the reference's regression evaluation (test_mc3serousv5.py `test_single_reg` :973-1024 and the localisation block
    behind it, test_reg3serousv5mt.py `test_multiple_reg`) records for each image and head, computed on the device with ONE
    device-to-host copy.  `pred` fp32 (N,H,W) count maps (predict_density's output), `gt_dots` uint8 / float32 (N,H,W) 0/1 dot
    maps.  The fixed-order float64 sum of the map -> peak_lists (umi/peaks.py: the project's restatement of
    skimage.feature.peak_local_max(pred, min_distance) after pred[pred < floor] = 0) -> Gaussian matching of the peaks against
    the dot list (CrowdMatchingTest) -> the 8 x 8 grid sums of the dot map and of the count map (GMAE at levels 1-3 over `size`
    pixels; CrowdMatching.game_from_cells truncates the cell sums with int() as the reference's GMAE does).

    Returns a list of N dicts: 'GT' (dot count), 'Pred' (the float64 sum; the reference's np.sum of a float32 array is a float32
    pairwise sum, a different rounding of the same number), 'AbsDiff', 'Accuracy', 'AccuracyRelative', 'AccuracyRelativePD'
    (CrowdMatching.countAccuracyMetric), 'G1', 'G2', 'G3' (each [gmae, relative, relativePD]), 'peaks' (their number),
    'arr_prec', 'arr_recall', 'arr_f1' ((S, T) float64).  For a pair of heads pass `pred` = (head 0, head 1) and `gt_dots` likewise:
    every image then gives {0: ..., 1: ..., 'ratio': ...} with the reference's immune / (other + immune) block through
    umi.matching.ratio_metrics, the heads read as (immune, other); still one copy.  Raises on either fault word (more than
    umi.peaks.MAX_PEAKS peaks or umi.matching.MAX_DOTS dots in an image).  umi.peaks.score_density_numpy is the host statement."""
    from . import matching as M
    from . import peaks as P
    pair = P._heads(pred, gt_dots)
    if pair:
        n_first = pred[0].shape[0]
        pred, gt_dots = torch.cat([p.contiguous() for p in pred]), torch.cat([g.contiguous() for g in gt_dots])
    if pred.dim() != 3 or gt_dots.shape != pred.shape or pred.dtype != torch.float32:
        raise ValueError(f"score_density_maps expects fp32 (N,H,W) maps and dot maps of one shape, got {tuple(pred.shape)} "
                         f"{pred.dtype} {tuple(gt_dots.shape)}")
    ops._need_cuda(pred, gt_dots)
    pred = pred.contiguous()
    N = pred.shape[0]
    counts, vmin = P.map_sums(pred)
    peaks, p_count, peak_fault = P.peak_lists(pred, min_distance, floor, _fault=True, vmin=vmin)
    dots, g_count, dot_fault = M.dot_lists(gt_dots, _fault=True)
    crowd = M.crowd_match(dots, g_count, peaks, p_count, sigma_list, sigma_thresh_list)
    cells_gt = M.grid_sums(gt_dots, size).to(torch.int64)           # sums of a 0/1 map: exact in either type
    cells_pred = M.grid_sums(pred, size)
    peak_code, dot_code, g_h, p_h, crowd_h, cg, cnt_h, cp = ops.read_back(peak_fault, dot_fault, g_count, p_count, crowd, cells_gt,
                                                                          counts, cells_pred)
    P.raise_on_peak_fault(peak_code[0])
    M.raise_on_dot_overflow(dot_code[0])
    res = P.density_scores(g_h, cnt_h, p_h, crowd_h, cg, cp)
    return P.pair_scores(res[:n_first], res[n_first:]) if pair else res
