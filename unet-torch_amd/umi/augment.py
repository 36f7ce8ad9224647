"""Training-batch transform: the arithmetic of the reference's `Dataset.transform` (DataLoader.py `Data_Binary` :636-680,
`Data_Reg` :275-373, `Data_Reg_Binary` :132-174) for a whole batch, on the device.

    tf = augment.TrainTransform((512, 512), augmentation=True)                     # Data_Binary: int64 labels
    x, (label,) = tf(images_u8_nhwc_on_device, [label_maps_on_device])             # [N,C,h,w] fp32, [N,h,w] int64
    tf = augment.TrainTransform((512, 512), True, label_scale=200.0, label_dtype=torch.float32)   # the regression datasets

Per sample the reference does, in NumPy / SciPy on the host:
  1. with `augmentation`: u = random.random(); u > 0.5 -> np.rot90(k) + np.flip(axis) with k = np.random.randint(0, 4),
     axis = np.random.randint(0, 2) (mode 1); else a second random.random() > 0.5 -> scipy.ndimage.rotate(angle, order=0,
     reshape=False) with angle = np.random.randint(-20, 20) (mode 2); else nothing (mode 0) -- on the image and every label map;
  2. when the size differs from the network's: zoom(image, (width / x, height / y[, 1]), order=3) and zoom(label, same, order=0)
     (the factor order is the reference's: axis 0 gets width / x);
  3. float64 per-channel mean and np.std over H, W; (image - mean) / std;
  4. float32 CHW with REVERSED channels for an HWC image, unsqueeze(0) for an HW one; labels to float32, times 200 in the
     regression datasets, `.long()` in Data_Binary.

`draw_params` draws step 1's random numbers in the reference's order; `train_transform_numpy` is the statement of steps 1-4
for one sample; `apply_geometry` and `TrainTransform` run them for a batch with the kernels of csrc/augment.hip.

The rotation (mode 2) is SciPy's mode='constant', cval=0, order=0 rule, pinned against SciPy by tests/golden/augment.npz:
  matrix M = [[c, s], [-s, c]] with c, s = scipy.special.cosdg / sindg(angle) (the float64 table below; math.cos(a * pi / 180)
  differs from it in the last bit at several angles), offset = (shape - 1) / 2 - M @ ((shape - 1) / 2) with NumPy's `@`.
  `M @ centre` is NOT the two-rounding expression c * cy + s * cx (the BLAS behind `@` fuses), so the offset is always formed
  on the host, here, and handed to the kernels; nothing recomputes it on the device.
  Output pixel (r, q) samples y = (off0 + r * M00) + q * M01, x = (off1 + r * M10) + q * M11, float64, each product and sum
  rounded on its own; it is 0 unless 0 <= y <= H - 1 and 0 <= x <= W - 1, else src[floor(y + 0.5), floor(x + 0.5)], the same
  source pixel for every channel.

Random crops of large images (reference `DataRandomCrop`, DataLoader.py:928-1069, `pad_image` :27-47; test.py `preprocessCrop`
:91-128) are the second half of this module: `CropPool` holds the images on the device, `CropTransform` cuts training batches
and padded validation tile grids out of them with the kernels of csrc/crops.hip, `CropBatches` is the loader for `Trainer`;
`draw_crop_params` / `draw_pad` make the reference's draws, `crop_transform_numpy` / `grid_transform_numpy` are the statements.

Out of scope: file reading, the imgaug / torchio / ColorJitter pipelines, stain normalisation, random draws on the device (the
draws stay on the host in the reference's order, one upload per batch), augmentation of the validation grid.
"""
import math
import random

import numpy as np
import torch

MODE_NONE, MODE_ROT_FLIP, MODE_ROTATE = 0, 1, 2

# (scipy.special.cosdg(a), scipy.special.sindg(a)) for a = 0 .. 20, recorded from SciPy 1.15.3; cosdg is even and sindg odd in
# SciPy for every angle -20 .. 19 (tests/golden/augment.npz holds the 40 pairs as SciPy gave them).  SciPy is not needed at run time.
_COS_SIN_DG = (
    (1.0, 0.0),
    (0.9998476951563913, 0.01745240643728351),
    (0.9993908270190958, 0.03489949670250097),
    (0.9986295347545738, 0.052335956242943835),
    (0.9975640502598242, 0.0697564737441253),
    (0.9961946980917455, 0.08715574274765817),
    (0.9945218953682733, 0.10452846326765347),
    (0.992546151641322, 0.12186934340514748),
    (0.9902680687415704, 0.13917310096006544),
    (0.9876883405951378, 0.15643446504023087),
    (0.984807753012208, 0.17364817766693033),
    (0.981627183447664, 0.1908089953765448),
    (0.9781476007338057, 0.20791169081775934),
    (0.9743700647852352, 0.224951054343865),
    (0.9702957262759965, 0.24192189559966773),
    (0.9659258262890683, 0.25881904510252074),
    (0.9612616959383189, 0.27563735581699916),
    (0.9563047559630354, 0.29237170472273677),
    (0.9510565162951535, 0.3090169943749474),
    (0.9455185755993168, 0.3255681544571567),
    (0.9396926207859084, 0.3420201433256687),
)


def cos_sin_dg(angle):
    """(cosdg, sindg) of an integer angle in -20 .. 20 degrees from the recorded table."""
    a = int(angle)
    if a != angle or not -20 <= a <= 20:
        raise ValueError(f"the rotation table covers the integer angles -20 .. 20, got {angle!r}")
    c, s = _COS_SIN_DG[abs(a)]
    return c, (-s if a < 0 else s)


def draw_params(n, py_rng=random, np_rng=np.random):
    """int32 (n, 4) rows [mode, k, axis, angle]: the reference's draws in the reference's order, sample after sample
    (DataLoader.py:103-120, :638-644).  Fields a mode does not use are 0."""
    p = np.zeros((n, 4), dtype=np.int32)
    for i in range(n):
        if py_rng.random() > 0.5:
            k = np_rng.randint(0, 4)
            axis = np_rng.randint(0, 2)
            p[i] = (MODE_ROT_FLIP, k, axis, 0)
        elif py_rng.random() > 0.5:
            p[i] = (MODE_ROTATE, 0, 0, np_rng.randint(-20, 20))
    return p


def no_augmentation(n):
    """All-zero parameter rows: the validation phase, and augmentation=False."""
    return np.zeros((n, 4), dtype=np.int32)


def rotate_geometry(angle, H, W):
    """(matrix 2x2, offset 2), float64, as scipy.ndimage.rotate(angle, reshape=False) forms them for an (H, W[, C]) input."""
    c, s = cos_sin_dg(angle)
    matrix = np.array([[c, s], [-s, c]], dtype=np.float64)
    center = (np.array([H, W]) - 1) / 2
    return matrix, center - matrix @ center


def pack_geometry(matrix, offset):
    """The six float64 the kernels and the statement take: [M00, M01, M10, M11, off0, off1]."""
    return np.concatenate([np.asarray(matrix, dtype=np.float64).reshape(4), np.asarray(offset, dtype=np.float64).reshape(2)])


def batch_geometry(params, H, W):
    """float64 (n, 6): pack_geometry(rotate_geometry(angle, H, W)) for the rows of mode 2, zeros elsewhere."""
    params = np.asarray(params)
    geom = np.zeros((params.shape[0], 6), dtype=np.float64)
    for i, (mode, _, _, angle) in enumerate(params):
        if mode == MODE_ROTATE:
            geom[i] = pack_geometry(*rotate_geometry(int(angle), H, W))
    return geom


def _check_rot_flip(params, H, W):
    params = np.asarray(params)
    if H != W and np.any((params[:, 0] == MODE_ROT_FLIP) & (params[:, 1] % 2 == 1)):
        raise ValueError(f"rot90 by an odd k turns a {H}x{W} sample into {W}x{H}: a batch of one size needs H == W")


def apply_geometry_numpy(x, p, geom=None):
    """Step 1 for one HW / HWC array `x`: p = [mode, k, axis, angle]; geom = the six float64 of pack_geometry (mode 2 only;
    None: formed from the angle).  Mode 1 is np.flip(np.rot90(x, k), axis); mode 2 the sampling rule of the module docstring."""
    x = np.asarray(x)
    mode, k, axis, angle = (int(v) for v in p)
    if mode == MODE_ROT_FLIP:
        return np.flip(np.rot90(x, k), axis=axis).copy()
    if mode != MODE_ROTATE:
        return x.copy()
    H, W = x.shape[:2]
    g = pack_geometry(*rotate_geometry(angle, H, W)) if geom is None else np.asarray(geom, dtype=np.float64).reshape(6)
    r = np.arange(H, dtype=np.float64)[:, None]
    q = np.arange(W, dtype=np.float64)[None, :]
    y = (g[4] + r * g[0]) + q * g[1]
    xx = (g[5] + r * g[2]) + q * g[3]
    inside = (y >= 0) & (y <= H - 1) & (xx >= 0) & (xx <= W - 1)
    iy = np.where(inside, np.floor(y + 0.5), 0).astype(np.int64)
    ix = np.where(inside, np.floor(xx + 0.5), 0).astype(np.int64)
    out = x[iy, ix]
    out[~inside] = 0
    return out


def resized_shape(H, W, input_size):
    """Shape of zoom(a, (width / W, height / H)) of an (H, W) array, the reference's (swapped) factors; ValueError unless it
    is input_size = (height, width), which the network needs."""
    height, width = int(input_size[0]), int(input_size[1])
    oh, ow = int(round(H * (width / W))), int(round(W * (height / H)))
    if (oh, ow) != (height, width):
        raise ValueError(f"the reference's zoom factors (width / x, height / y) turn a {H}x{W} sample into {oh}x{ow}, "
                         f"not the network size {height}x{width}")
    return oh, ow


def _host_zooms():
    """The project's restatements of scipy.ndimage.zoom order 3 and order 0, each pinned against SciPy by its own tests.  Only
    the NumPy statement uses them (a resize on host arrays); they live with the test oracle and the fixture tools at the
    repository root, which then has to be on sys.path."""
    try:
        from oracle.ref_resize import zoom_cubic
        from tools.gen_golden_binary_infer import zoom_nearest_numpy
    except ImportError as e:
        raise RuntimeError("the NumPy statement of the resize needs oracle/ref_resize.py and tools/gen_golden_binary_infer.py "
                           "(repository root on sys.path); device tensors are resized by the kernels instead") from e
    return zoom_cubic, zoom_nearest_numpy


def _np_label_dtype(label_dtype):
    if label_dtype in (torch.int64, np.int64, "int64"):
        return np.int64
    if label_dtype in (torch.float32, np.float32, "float32"):
        return np.float32
    raise ValueError(f"label_dtype must be int64 or float32, got {label_dtype!r}")


def train_transform_numpy(image, label_maps, p, input_size, geom=None, label_scale=1.0, label_dtype=np.int64):
    """The whole `transform` of one sample in NumPy: image HW / HWC (uint8 or float32), label_maps a list of HW arrays,
    p = [mode, k, axis, angle].  Returns (float32 [C, h, w], [label [h, w] of label_dtype, ...])."""
    image = apply_geometry_numpy(image, p, geom)
    labels = [apply_geometry_numpy(m, p, geom) for m in label_maps]
    H, W = image.shape[:2]
    if (H, W) != (int(input_size[0]), int(input_size[1])):
        ohw = resized_shape(H, W, input_size)
        zoom_cubic, zoom_nearest = _host_zooms()
        image = zoom_cubic(image, ohw)
        labels = [zoom_nearest(m, ohw) for m in labels]
    z = image.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = (z - np.mean(z, axis=(0, 1))) / np.std(z, axis=(0, 1))
    x = z.astype(np.float32)[None] if z.ndim == 2 else np.ascontiguousarray(z.transpose((2, 0, 1))[::-1]).astype(np.float32)
    dt = _np_label_dtype(label_dtype)
    scale = np.float32(label_scale)
    return x, [(m.astype(np.float32) * scale).astype(dt) for m in labels]


# ---- device entry points ------------------------------------------------------------------------------------------------------
def _dev_params(params, geom, N, H, W, device):
    """int32 (N, 4) and float64 (N, 6) device tensors.  Host parameters are checked (odd k needs H == W) and uploaded with ONE
    copy; device parameters are taken as they are, without a read-back (the kernels write 0 for an odd k on H != W)."""
    if isinstance(params, torch.Tensor) and params.is_cuda:
        if geom is None or not (isinstance(geom, torch.Tensor) and geom.is_cuda):
            raise ValueError("device parameters need their (N, 6) float64 geometry on the device as well (batch_geometry)")
        p, g = params, geom
    else:
        ph = np.ascontiguousarray(params.numpy() if isinstance(params, torch.Tensor) else params, dtype=np.int32)
        if ph.shape != (N, 4):
            raise ValueError(f"expected ({N}, 4) parameters, got {ph.shape}")
        _check_rot_flip(ph, H, W)
        gh = batch_geometry(ph, H, W) if geom is None else np.ascontiguousarray(
            geom.numpy() if isinstance(geom, torch.Tensor) else geom, dtype=np.float64)
        if gh.shape != (N, 6):
            raise ValueError(f"expected ({N}, 6) geometry, got {gh.shape}")
        blob = torch.from_numpy(np.concatenate([gh.view(np.uint8).reshape(-1), ph.view(np.uint8).reshape(-1)]))
        blob = blob.to(device, non_blocking=True)                   # geometry first: the float64 view stays 8-byte aligned
        g = blob[:N * 48].view(torch.float64).view(N, 6)
        p = blob[N * 48:].view(torch.int32).view(N, 4)
    if p.dtype != torch.int32 or tuple(p.shape) != (N, 4) or g.dtype != torch.float64 or tuple(g.shape) != (N, 6):
        raise ValueError(f"expected int32 ({N}, 4) parameters and float64 ({N}, 6) geometry, got {p.dtype} {tuple(p.shape)}, "
                         f"{g.dtype} {tuple(g.shape)}")
    return p.contiguous(), g.contiguous()


def _batch_dims(x, what):
    if x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[3] > 4) or x.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"{what}: expected (N,H,W) or (N,H,W,C <= 4) uint8 / float32, got {tuple(x.shape)} {x.dtype}")
    N, H, W = x.shape[:3]
    C = x.shape[3] if x.dim() == 4 else 1
    if min(N, H, W, C) < 1:
        raise ValueError(f"{what}: empty batch {tuple(x.shape)}")
    return N, H, W, C


def _status(st, what, shape):
    from . import lib as L
    if st == L.UMI_ERR_UNSUPPORTED:
        raise ValueError(f"{what}: unsupported size {tuple(shape)}")
    L.check(st, what)


def apply_geometry(x, params, geom=None):
    """Step 1 for a device batch `x` (N,H,W) or (N,H,W,C <= 4), uint8 or float32, one launch for every sample and mode.
    params int32 (N, 4), geom float64 (N, 6) (batch_geometry): device tensors are used as they are -- no read-back, so the
    call may be captured in a graph; host arrays are checked and uploaded."""
    from . import lib as L
    from . import ops
    ops._need_cuda(x)
    N, H, W, C = _batch_dims(x, "apply_geometry")
    x = x.contiguous()
    p, g = _dev_params(params, geom, N, H, W, x.device)
    out = torch.empty_like(x)
    _status(L.fn("umi_augment_geometry")(x.data_ptr(), 0 if x.dtype == torch.uint8 else 1, out.data_ptr(), p.data_ptr(),
                                         g.data_ptr(), N, H, W, C, ops._stream()), "umi_augment_geometry", x.shape)
    return out


def transform_labels(label_map, params, geom, out_hw, label_scale=1.0, label_dtype=torch.int64):
    """Steps 1, 2 and 4 for a device batch of label maps (N,H,W), uint8 or float32, as ONE gather: output pixel -> source index
    of the order-0 zoom (umi.infer.zoom_nearest's rule) -> source index of the geometry; the float32 scale and the cast happen
    on the store.  Returns (N, out_h, out_w) of label_dtype (int64 or float32)."""
    from . import lib as L
    from . import ops
    ops._need_cuda(label_map)
    if label_map.dim() != 3:
        raise ValueError(f"transform_labels: expected (N,H,W) label maps, got {tuple(label_map.shape)}")
    N, H, W, _ = _batch_dims(label_map, "transform_labels")
    dt = _np_label_dtype(label_dtype)
    m = label_map.contiguous()
    p, g = _dev_params(params, geom, N, H, W, m.device)
    oh, ow = int(out_hw[0]), int(out_hw[1])
    out = torch.empty((N, oh, ow), dtype=torch.int64 if dt is np.int64 else torch.float32, device=m.device)
    _status(L.fn("umi_augment_labels")(m.data_ptr(), 0 if m.dtype == torch.uint8 else 1, out.data_ptr(),
                                       1 if dt is np.int64 else 0, float(label_scale), p.data_ptr(), g.data_ptr(), N, H, W, oh, ow,
                                       ops._stream()), "umi_augment_labels", m.shape)
    return out


def transform_image(x, params, geom=None, reverse_channels=None):
    """Steps 1, 3 and 4 for a device batch of images that need no resize: float64 statistics of the augmented image per (sample,
    channel), then one pass that gathers, normalises and writes [N,C,H,W] float32 (channels reversed for (N,H,W,C) input, like
    the reference).  The augmented image is never written out.  The sums run in a fixed order (two runs give the same bits):
    exact integer sums for uint8, two passes (mean, then squared deviations) in float64 for float32."""
    from . import lib as L
    from . import ops
    ops._need_cuda(x)
    N, H, W, C = _batch_dims(x, "transform_image")
    if reverse_channels is None:
        reverse_channels = x.dim() == 4
    x = x.contiguous()
    p, g = _dev_params(params, geom, N, H, W, x.device)
    out = torch.empty((N, C, H, W), dtype=torch.float32, device=x.device)
    nbytes = L.fn("umi_augment_znorm_ws_bytes")(N)
    ws = ops.workspace(nbytes, x.device)
    _status(L.fn("umi_augment_znorm")(x.data_ptr(), 0 if x.dtype == torch.uint8 else 1, out.data_ptr(), p.data_ptr(), g.data_ptr(),
                                      N, H, W, C, int(bool(reverse_channels)), ws.data_ptr(), nbytes, ops._stream()),
            "umi_augment_znorm", x.shape)
    return out


def _as_batch(a):
    """A batch as ONE array / tensor: a list of equally sized samples is stacked; samples of different sizes are refused."""
    if isinstance(a, (list, tuple)):
        shapes = {tuple(s.shape) for s in a}
        if len(shapes) != 1:
            raise ValueError(f"the samples of a batch must have one size, got {sorted(shapes)}")
        return torch.stack(list(a)) if isinstance(a[0], torch.Tensor) else np.stack([np.asarray(s) for s in a])
    return a


class TrainTransform:
    """`transform` of the reference's datasets for a whole batch.  input_size = (height, width) of the network;
    label_scale = 200 and label_dtype = torch.float32 for the regression datasets, the defaults for Data_Binary.

        x, labels = tf(images, label_maps, params=None, geom=None)

    images (N,H,W) / (N,H,W,C <= 4) uint8 or float32 (or a list of such samples), label_maps one (N,H,W) batch or a list /
    tuple of such batches (labels then comes back as a list).  params: int32 (N, 4) rows of draw_params / no_augmentation;
    None draws them on the host (draw_params when `augmentation`, else no_augmentation).  Host parameters are checked and
    uploaded with one copy; device parameters come with their device `geom` (batch_geometry) and are not read back.
    Device images run the kernels of csrc/augment.hip; host tensors and arrays run train_transform_numpy and return host
    tensors."""

    def __init__(self, input_size, augmentation, label_scale=1.0, label_dtype=torch.int64):
        self.input_size = (int(input_size[0]), int(input_size[1]))
        self.augmentation = bool(augmentation)
        self.label_scale = float(label_scale)
        _np_label_dtype(label_dtype)
        self.label_dtype = label_dtype

    def draw(self, n):
        return draw_params(n) if self.augmentation else no_augmentation(n)

    def __call__(self, images, label_maps, params=None, geom=None):
        images = _as_batch(images)
        single = not isinstance(label_maps, (list, tuple))
        maps = [label_maps] if single else [_as_batch(m) for m in label_maps]
        N, H, W = images.shape[:3]
        if images.ndim not in (3, 4):
            raise ValueError(f"expected (N,H,W) or (N,H,W,C) images, got {tuple(images.shape)}")
        for m in maps:
            if tuple(m.shape) != (N, H, W):
                raise ValueError(f"label maps must be ({N}, {H}, {W}) like the images, got {tuple(m.shape)}")
        if params is None:
            params = self.draw(N)
        resize = (H, W) != self.input_size
        if resize:
            resized_shape(H, W, self.input_size)
        on_device = isinstance(images, torch.Tensor) and images.is_cuda
        x, labels = (self._device if on_device else self._host)(images, maps, params, geom, resize)
        return x, (labels[0] if single else labels)

    def _host(self, images, maps, params, geom, resize):
        params = np.asarray(params.cpu() if isinstance(params, torch.Tensor) else params)
        _check_rot_flip(params, *images.shape[1:3])
        images = images.numpy() if isinstance(images, torch.Tensor) else np.asarray(images)
        maps = [m.cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m) for m in maps]
        xs, ls = [], [[] for _ in maps]
        for n in range(images.shape[0]):
            x, lab = train_transform_numpy(images[n], [m[n] for m in maps], params[n], self.input_size,
                                           geom=None if geom is None else np.asarray(geom)[n], label_scale=self.label_scale, label_dtype=self.label_dtype)
            xs.append(x)
            for acc, l in zip(ls, lab):
                acc.append(l)
        return torch.from_numpy(np.stack(xs)), [torch.from_numpy(np.stack(l)) for l in ls]

    def _device(self, images, maps, params, geom, resize):
        from . import infer
        N, H, W = images.shape[:3]
        if images.dtype not in (torch.uint8, torch.float32):
            images = images.float()
        p, g = _dev_params(params, geom, N, H, W, images.device)
        labels = []
        for m in maps:
            m = m.to(images.device)
            if m.dtype not in (torch.uint8, torch.float32):
                m = m.float()
            labels.append(transform_labels(m, p, g, self.input_size, self.label_scale, self.label_dtype))
        if not resize:
            return transform_image(images, p, g), labels
        # the rare path (datasets are stored at the network size): the augmented image is written out once for the whole batch,
        # then the existing single-image cubic resize and z-normalisation run per sample, N launches of each
        aug = apply_geometry(images, p, g)
        x = torch.cat([infer.preprocess(aug[n], input_size=self.input_size) for n in range(N)])
        return x, labels


# ---- random crops and padded tile grids of large images: the reference's DataRandomCrop ------------------------------------------
# Train: r0 = random.randint(0, H - crop), c0 = random.randint(0, W - crop), the three arrays cut to the window, then steps 1, 3, 4
# above ON THE CROP (a rotation brings in 0, not the pixels next to the window); the dot map goes through step 1 and comes back
# as it is (uint8).  Validation: the image constant-padded to multiples of `crop` (255 for an HWC image, 0 for an HW one and for
# the maps), steps 3 and 4 over the whole padded image, then its row-major crop x crop tiles.
#
# uint8 statistics are exact integers, as the kernels compute them: S1 = sum v, S2 = sum v^2, mean = S1 / n and
# std = sqrt(n * S2 - S1^2) / n.  n * S2 - S1^2 fits unsigned 64 bits while (255 n)^2 < 2^64:
U8_STAT_PIXELS = 16843009            # the largest pixel count n of a uint8 crop or padded image; 4096 x 4096 fits


def draw_crop_params(sizes, crop, augmentation, py_rng=random, np_rng=np.random, indices=None):
    """(int32 (N, 3) rows [index, r0, c0], int32 (N, 4) rows of draw_params) for the images `indices` (None: every image of
    `sizes`, an (n, 2) table of (H, W), in order).  The draws run in the reference's order, sample after sample: r0, c0
    (DataLoader.py:1061-1062, both ends inclusive), then that sample's augmentation draws."""
    sizes = np.asarray(sizes).reshape(-1, 2)
    crop = int(crop)
    idx = np.arange(len(sizes)) if indices is None else np.asarray(indices, dtype=np.int64).reshape(-1)
    crops = np.zeros((len(idx), 3), dtype=np.int32)
    params = np.zeros((len(idx), 4), dtype=np.int32)
    for n, i in enumerate(idx):
        if not 0 <= i < len(sizes):
            raise ValueError(f"image index {int(i)} outside the pool of {len(sizes)} images")
        H, W = int(sizes[i][0]), int(sizes[i][1])
        if crop < 1 or H < crop or W < crop:
            raise ValueError(f"image {int(i)} is {H}x{W}, smaller than the crop {crop}")
        r0 = py_rng.randint(0, H - crop)
        c0 = py_rng.randint(0, W - crop)
        crops[n] = (i, r0, c0)
        if augmentation:
            params[n] = draw_params(1, py_rng, np_rng)[0]
    return crops, params


def _padding(size, crop):
    return (-int(size)) % int(crop)


def draw_pad(H, W, crop, py_rng=random):
    """(pad_top, pad_left) as `pad_image` draws them: pad_left = randint(0, padding_w) FIRST, then pad_top; both are drawn even
    when the padding is 0."""
    pad_left = py_rng.randint(0, _padding(W, crop))
    pad_top = py_rng.randint(0, _padding(H, crop))
    return pad_top, pad_left


def center_pad(H, W, crop):
    """(pad_top, pad_left) of test.py `preprocessCrop`: half the padding, rounded down."""
    return _padding(H, crop) // 2, _padding(W, crop) // 2


def _check_crops(crops, sizes, crop):
    crops, sizes = np.asarray(crops), np.asarray(sizes)
    if crops.ndim != 2 or crops.shape[1] != 3 or crops.shape[0] < 1:
        raise ValueError(f"expected (N, 3) crop rows [index, r0, c0], got {crops.shape}")
    i = crops[:, 0].astype(np.int64)
    if np.any((i < 0) | (i >= len(sizes))):
        raise ValueError(f"crop rows name images outside the pool of {len(sizes)}")
    hw = sizes[i].astype(np.int64)
    rc = crops[:, 1:].astype(np.int64)
    if np.any(rc < 0) or np.any(rc + int(crop) > hw):
        bad = int(np.argmax(np.any((rc < 0) | (rc + int(crop) > hw), axis=1)))
        raise ValueError(f"crop row {bad} {crops[bad].tolist()}: a {crop}-pixel window leaves the {hw[bad].tolist()} image")


def crop_transform_numpy(image, maps, crop_row, p, crop, geom=None, label_scale=1.0, label_dtype=np.int64, dots=None):
    """One training sample of DataRandomCrop: `image` HW / HWC and the HW `maps` / `dots` are whole source arrays, crop_row =
    [index, r0, c0] (the index is the caller's), p = [mode, k, axis, angle].  The window, then train_transform_numpy on it (no
    resize: the crop is the network size).  Returns (float32 [C, crop, crop], [label, ...], dots uint8 or None).  The reference's
    `crop` indexes `img[..., :]` and so takes HWC images only; HW images are taken here."""
    crop = int(crop)
    r0, c0 = int(crop_row[-2]), int(crop_row[-1])
    H, W = np.asarray(image).shape[:2]
    if r0 < 0 or c0 < 0 or r0 + crop > H or c0 + crop > W:
        raise ValueError(f"a {crop}-pixel window at ({r0}, {c0}) leaves the {H}x{W} image")

    def win(a):
        return np.asarray(a)[r0:r0 + crop, c0:c0 + crop]

    x, labels = train_transform_numpy(win(image), [win(m) for m in maps], p, (crop, crop), geom, label_scale, label_dtype)
    return x, labels, None if dots is None else apply_geometry_numpy(win(dots), p, geom)


def padded_statistics(image, npad, pad_value):
    """float64 (mean, std) per channel of an HW / HWC image with `npad` further pixels of `pad_value`, as the grid kernels form
    them.  uint8: Python integers (see U8_STAT_PIXELS; ValueError beyond it).  float32: two float64 passes, the pad term added
    last in each."""
    image = np.asarray(image)
    a = image.reshape(image.shape[0] * image.shape[1], -1)
    n, v = a.shape[0] + int(npad), int(pad_value)
    mean, std = np.zeros(a.shape[1]), np.zeros(a.shape[1])
    if image.dtype == np.uint8:
        if n > U8_STAT_PIXELS:
            raise ValueError(f"{n} pixels: the exact uint8 statistics hold up to {U8_STAT_PIXELS}")
        for c in range(a.shape[1]):
            hist = np.bincount(a[:, c], minlength=256).tolist()
            S1 = sum(k * h for k, h in enumerate(hist)) + npad * v
            S2 = sum(k * k * h for k, h in enumerate(hist)) + npad * v * v
            mean[c] = S1 / n
            std[c] = math.sqrt(n * S2 - S1 * S1) / n
        return mean, std
    a = a.astype(np.float64)
    mean = (a.sum(axis=0) + npad * float(v)) / n
    d = a - mean
    std = np.sqrt(((d * d).sum(axis=0) + npad * ((v - mean) * (v - mean))) / n)
    return mean, std


def _grid_dims(H, W, pad_top, pad_left, th, tw, padded):
    th, tw = int(th), int(tw)
    if th < 1 or tw < 1:
        raise ValueError(f"tile size {th}x{tw}")
    Hp, Wp = (H + _padding(H, th), W + _padding(W, tw)) if padded is None else (int(padded[0]), int(padded[1]))
    if Hp % th or Wp % tw or not 0 <= pad_top <= Hp - H or not 0 <= pad_left <= Wp - W:
        raise ValueError(f"a {H}x{W} image at ({pad_top}, {pad_left}) of a {Hp}x{Wp} padded image does not split into {th}x{tw} tiles")
    return Hp, Wp, th, tw


def _tiles(a, th, tw):
    """(..., Hp, Wp) -> (T, ..., th, tw), tiles in row-major order."""
    lead = a.shape[:-2]
    a = a.reshape(lead + (a.shape[-2] // th, th, a.shape[-1] // tw, tw))
    k = len(lead)
    return np.ascontiguousarray(a.transpose((k, k + 2) + tuple(range(k)) + (k + 1, k + 3))).reshape((-1,) + lead + (th, tw))


def grid_transform_numpy(image, maps, pad_top, pad_left, th, tw, pad_value=None, padded=None, label_scale=1.0,
                         label_dtype=np.int64, dots=None):
    """One validation item of DataRandomCrop: `image` padded with the constant pad_value to `padded` = (Hp, Wp) (None: the next
    multiples of th, tw) with the source at (pad_top, pad_left), z-normalised with the statistics of the WHOLE padded image (pad
    pixels count), cut into th x tw tiles.  pad_value=None is the reference's rule: 255 for an HWC image, 0 for an HW one; maps
    and dots are padded with 0.  Returns (float32 (T, C, th, tw), [label (T, th, tw), ...], dots (T, th, tw) uint8 or None).
    th, tw = Hp, Wp is test.py's `preprocessCrop`."""
    image = np.asarray(image)
    hwc = image.ndim == 3
    H, W = image.shape[:2]
    pad_top, pad_left = int(pad_top), int(pad_left)
    Hp, Wp, th, tw = _grid_dims(H, W, pad_top, pad_left, th, tw, padded)
    v = (255 if hwc else 0) if pad_value is None else int(pad_value)
    if not 0 <= v <= 255:
        raise ValueError(f"pad_value {v} outside 0 .. 255")
    mean, std = padded_statistics(image, Hp * Wp - H * W, v)

    def pad(a, value):
        out = np.full((Hp, Wp) + a.shape[2:], value, dtype=a.dtype)
        out[pad_top:pad_top + H, pad_left:pad_left + W] = a
        return out

    z = pad(image.reshape(H, W, -1), v).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = (z - mean) / std
    z = z.transpose((2, 0, 1))[::-1] if hwc else z.transpose((2, 0, 1))
    x = _tiles(np.ascontiguousarray(z).astype(np.float32), th, tw)
    dt = _np_label_dtype(label_dtype)
    scale = np.float32(label_scale)
    labels = [_tiles((pad(np.asarray(m), 0).astype(np.float32) * scale).astype(dt), th, tw) for m in maps]
    return x, labels, None if dots is None else _tiles(pad(np.asarray(dots), 0), th, tw)


def _pool_tensor(a, what, dtypes=(torch.uint8, torch.float32)):
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype not in dtypes:
        if torch.float32 not in dtypes:
            raise ValueError(f"{what}: expected {dtypes[0]}, got {t.dtype}")
        t = t.float()
    return t.contiguous()


class CropPool:
    """Images of any sizes, with their label maps (and dot maps), packed ONCE into one flat buffer each: `images` (all HW or all
    HWC with one channel count <= 4, uint8 or float32), `labels` (uint8 or float32) and `dots` (uint8 or None), with the host
    tables `offsets` / `map_offsets` (int64 element offsets) and `sizes` (int32 (n, 2) rows (H, W)).  `.to(device)` moves the
    buffers and uploads the tables; a CPU pool runs the NumPy statements."""

    def __init__(self, images, label_maps, dot_maps=None, device=None):
        if not len(images) or len(label_maps) != len(images) or (dot_maps is not None and len(dot_maps) != len(images)):
            raise ValueError("a pool needs at least one image, and one label map (and dot map) per image")
        imgs = [_pool_tensor(a, "image") for a in images]
        labs = [_pool_tensor(a, "label map") for a in label_maps]
        dots = None if dot_maps is None else [_pool_tensor(a, "dot map", (torch.uint8,)) for a in dot_maps]
        first = imgs[0]
        if first.dim() not in (2, 3):
            raise ValueError(f"expected HW or HWC images, got {tuple(first.shape)}")
        for i, t in enumerate(imgs):
            if t.dim() != first.dim() or t.shape[2:] != first.shape[2:] or t.dtype != first.dtype:
                raise ValueError(f"image {i}: {tuple(t.shape)} {t.dtype}; a pool holds one channel count and dtype "
                                 f"({tuple(first.shape)} {first.dtype})")
            for m in (labs[i],) + (() if dots is None else (dots[i],)):
                if tuple(m.shape) != tuple(t.shape[:2]):
                    raise ValueError(f"image {i} is {tuple(t.shape[:2])}, its map {tuple(m.shape)}")
            if labs[i].dtype != labs[0].dtype:
                raise ValueError("the label maps of a pool have one dtype")
        sizes = np.array([t.shape[:2] for t in imgs], dtype=np.int32)
        C = first.shape[2] if first.dim() == 3 else 1
        px = np.concatenate([[0], np.cumsum(sizes[:, 0].astype(np.int64) * sizes[:, 1])[:-1]])

        def flat(ts):
            return torch.cat([t.reshape(-1).cpu() for t in ts])

        self._init(flat(imgs), px * C, sizes, C, first.dim() == 3, flat(labs), px, None if dots is None else flat(dots))
        if device is not None:
            self._move(torch.device(device))

    @classmethod
    def from_buffers(cls, images, offsets, sizes, channels, hwc, labels, map_offsets, dots=None):
        """A pool over buffers that are packed already (1-D tensors on one device) and their tables; the tables are checked."""
        self = cls.__new__(cls)
        self._init(images, offsets, sizes, channels, hwc, labels, map_offsets, dots)
        if images.is_cuda:
            self._upload()
        return self

    def _init(self, images, offsets, sizes, C, hwc, labels, map_offsets, dots):
        sizes = np.ascontiguousarray(sizes, dtype=np.int32)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        map_offsets = np.ascontiguousarray(map_offsets, dtype=np.int64)
        n = sizes.shape[0]
        if sizes.ndim != 2 or sizes.shape[1] != 2 or n < 1 or offsets.shape != (n,) or map_offsets.shape != (n,):
            raise ValueError(f"expected (n, 2) sizes and (n,) offsets, got {sizes.shape}, {offsets.shape}, {map_offsets.shape}")
        C = int(C)
        if not 1 <= C <= 4 or (not hwc and C != 1):
            raise ValueError(f"{C} channels: a pool holds HW images or HWC images of up to 4 channels")
        if images.dtype not in (torch.uint8, torch.float32) or labels.dtype not in (torch.uint8, torch.float32) or \
                (dots is not None and dots.dtype != torch.uint8):
            raise ValueError("pool buffers are uint8 or float32 (dot maps: uint8)")
        px = sizes[:, 0].astype(np.int64) * sizes[:, 1]
        if np.any(sizes < 1):
            raise ValueError("an image of the size table is empty")
        for name, buf, off, per in (("images", images, offsets, C), ("labels", labels, map_offsets, 1), ("dots", dots, map_offsets, 1)):
            if buf is None:
                continue
            if buf.dim() != 1 or not buf.is_contiguous() or buf.device != images.device:
                raise ValueError(f"{name}: expected a contiguous 1-D buffer on {images.device}")
            if np.any(off < 0) or np.any(off + px * per > buf.numel()):
                raise ValueError(f"{name}: an offset table entry leaves the buffer of {buf.numel()} elements")
        self.images, self.labels, self.dots = images, labels, dots
        self.offsets, self.map_offsets, self.sizes = offsets, map_offsets, sizes
        self.C, self.hwc = C, bool(hwc)
        self._tables = None

    def _upload(self):
        n = len(self)
        blob = np.concatenate([self.offsets.view(np.uint8), self.map_offsets.view(np.uint8), self.sizes.view(np.uint8).reshape(-1)])
        blob = torch.from_numpy(blob).to(self.device)               # the int64 tables first: they stay 8-byte aligned
        self._tables = (blob[:8 * n].view(torch.int64), blob[8 * n:16 * n].view(torch.int64), blob[16 * n:].view(torch.int32))

    def _move(self, device):
        self.images, self.labels = self.images.to(device), self.labels.to(device)
        self.dots = None if self.dots is None else self.dots.to(device)
        self._tables = None
        if self.images.is_cuda:
            self._upload()

    def to(self, device):
        """This pool on `device` (a new CropPool; the buffers are copied unless they are there already)."""
        other = CropPool.__new__(CropPool)
        other.__dict__.update(self.__dict__)
        other._move(torch.device(device))
        return other

    def __len__(self):
        return self.sizes.shape[0]

    @property
    def device(self):
        return self.images.device

    @property
    def is_cuda(self):
        return self.images.is_cuda

    def image(self, i):
        """Image i as an (H, W) / (H, W, C) view of the buffer."""
        H, W = (int(v) for v in self.sizes[i])
        o = int(self.offsets[i])
        return self.images[o:o + H * W * self.C].view((H, W, self.C) if self.hwc else (H, W))

    def _map(self, buf, i):
        H, W = (int(v) for v in self.sizes[i])
        o = int(self.map_offsets[i])
        return buf[o:o + H * W].view(H, W)

    def label(self, i):
        return self._map(self.labels, i)

    def dot(self, i):
        return None if self.dots is None else self._map(self.dots, i)


_LABEL_CODE = {np.float32: 0, np.int64: 1, np.uint8: 2}
_LABEL_TORCH = {np.float32: torch.float32, np.int64: torch.int64, np.uint8: torch.uint8}


def _dev_crop_tables(pool, crops, params, geom, crop):
    """int32 (N, 3), int32 (N, 4) and float64 (N, 6) device tensors.  Host tables are checked against the pool (ValueError) and
    uploaded with ONE copy; device tables are taken as they are, without a read-back (the kernels write 0 for a row that leaves
    its image)."""
    dev = [isinstance(t, torch.Tensor) and t.is_cuda for t in (crops, params, geom)]
    if any(dev):
        if not all(dev):
            raise ValueError("device crop rows need their (N, 4) parameters and (N, 6) float64 geometry on the device as well")
        c, p, g = crops, params, geom
    else:
        ch = np.ascontiguousarray(crops.numpy() if isinstance(crops, torch.Tensor) else crops, dtype=np.int32)
        _check_crops(ch, pool.sizes, crop)
        N = ch.shape[0]
        ph = np.ascontiguousarray(params.numpy() if isinstance(params, torch.Tensor) else params, dtype=np.int32)
        if ph.shape != (N, 4):
            raise ValueError(f"expected ({N}, 4) parameters, got {ph.shape}")
        gh = batch_geometry(ph, crop, crop) if geom is None else np.ascontiguousarray(
            geom.numpy() if isinstance(geom, torch.Tensor) else geom, dtype=np.float64)
        if gh.shape != (N, 6):
            raise ValueError(f"expected ({N}, 6) geometry, got {gh.shape}")
        blob = torch.from_numpy(np.concatenate([gh.view(np.uint8).reshape(-1), ph.view(np.uint8).reshape(-1),
                                                ch.view(np.uint8).reshape(-1)])).to(pool.device, non_blocking=True)
        g = blob[:N * 48].view(torch.float64).view(N, 6)
        p = blob[N * 48:N * 64].view(torch.int32).view(N, 4)
        c = blob[N * 64:].view(torch.int32).view(N, 3)
    N = c.shape[0]
    if c.dtype != torch.int32 or tuple(c.shape) != (N, 3) or p.dtype != torch.int32 or tuple(p.shape) != (N, 4) or \
            g.dtype != torch.float64 or tuple(g.shape) != (N, 6):
        raise ValueError(f"expected int32 (N, 3) crop rows, int32 (N, 4) parameters and float64 (N, 6) geometry, got "
                         f"{c.dtype} {tuple(c.shape)}, {p.dtype} {tuple(p.shape)}, {g.dtype} {tuple(g.shape)}")
    return c.contiguous(), p.contiguous(), g.contiguous()


def crop_image(pool, crops, params, geom, crop):
    """N crops of a device pool -> [N, C, crop, crop] float32 (umi_crop_znorm): window, geometry, float64 statistics of the
    augmented crop and the normalising store; channels reversed for an HWC pool.  Three launches for uint8 (five for float32),
    whatever N; device tables are not read back, so the call may be captured in a graph."""
    from . import lib as L
    from . import ops
    ops._need_cuda(pool.images)
    crop = int(crop)
    c, p, g = _dev_crop_tables(pool, crops, params, geom, crop)
    N = c.shape[0]
    off, _, sizes = pool._tables
    out = torch.empty((N, pool.C, crop, crop), dtype=torch.float32, device=pool.device)
    nbytes = L.fn("umi_crop_znorm_ws_bytes")(N)
    ws = ops.workspace(nbytes, pool.device)
    _status(L.fn("umi_crop_znorm")(pool.images.data_ptr(), 0 if pool.images.dtype == torch.uint8 else 1, off.data_ptr(),
                                   sizes.data_ptr(), len(pool), pool.images.numel(), pool.C, c.data_ptr(), p.data_ptr(),
                                   g.data_ptr(), N, crop, out.data_ptr(), int(pool.hwc), ws.data_ptr(), nbytes, ops._stream()),
            "umi_crop_znorm", (N, crop, crop))
    return out


def crop_maps(pool, buf, crops, params, geom, crop, label_scale=1.0, label_dtype=torch.int64):
    """The same gather for `buf` = pool.labels or pool.dots -> [N, crop, crop] of label_dtype: int64 / float32 ((float)v * scale)
    or uint8 (the value as it is)."""
    from . import lib as L
    from . import ops
    ops._need_cuda(buf)
    crop = int(crop)
    dt = np.uint8 if label_dtype in (torch.uint8, np.uint8, "uint8") else _np_label_dtype(label_dtype)
    c, p, g = _dev_crop_tables(pool, crops, params, geom, crop)
    N = c.shape[0]
    _, off, sizes = pool._tables
    out = torch.empty((N, crop, crop), dtype=_LABEL_TORCH[dt], device=buf.device)
    _status(L.fn("umi_crop_labels")(buf.data_ptr(), 0 if buf.dtype == torch.uint8 else 1, off.data_ptr(), sizes.data_ptr(), len(pool),
                                    buf.numel(), c.data_ptr(), p.data_ptr(), g.data_ptr(), N, crop, out.data_ptr(), _LABEL_CODE[dt],
                                    float(label_scale), ops._stream()), "umi_crop_labels", (N, crop, crop))
    return out


def grid_image(img, pad_top, pad_left, th, tw, pad_value=None, padded=None):
    """One device image HW / HWC -> its (T, C, th, tw) float32 tile stack (umi_grid_znorm); arguments as grid_transform_numpy.
    The padded image is never written: its statistics are the source's sums plus the pad terms."""
    from . import lib as L
    from . import ops
    ops._need_cuda(img)
    if img.dim() not in (2, 3) or (img.dim() == 3 and img.shape[2] > 4) or img.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"grid_image: expected an HW / HWC (C <= 4) uint8 or float32 image, got {tuple(img.shape)} {img.dtype}")
    hwc = img.dim() == 3
    H, W = img.shape[:2]
    C = img.shape[2] if hwc else 1
    pad_top, pad_left = int(pad_top), int(pad_left)
    Hp, Wp, th, tw = _grid_dims(H, W, pad_top, pad_left, th, tw, padded)
    v = (255 if hwc else 0) if pad_value is None else int(pad_value)
    if not 0 <= v <= 255:
        raise ValueError(f"pad_value {v} outside 0 .. 255")
    if img.dtype == torch.uint8 and Hp * Wp > U8_STAT_PIXELS:
        raise ValueError(f"{Hp * Wp} pixels: the exact uint8 statistics hold up to {U8_STAT_PIXELS}")
    img = img.contiguous()
    out = torch.empty(((Hp // th) * (Wp // tw), C, th, tw), dtype=torch.float32, device=img.device)
    nbytes = L.fn("umi_grid_znorm_ws_bytes")()
    ws = ops.workspace(nbytes, img.device)
    _status(L.fn("umi_grid_znorm")(img.data_ptr(), 0 if img.dtype == torch.uint8 else 1, H, W, C, pad_top, pad_left, v, Hp, Wp, th, tw,
                                   out.data_ptr(), int(hwc), ws.data_ptr(), nbytes, ops._stream()), "umi_grid_znorm", (Hp, Wp))
    return out


def grid_maps(m, pad_top, pad_left, th, tw, padded=None, label_scale=1.0, label_dtype=torch.int64):
    """One device map HW, padded with 0 -> its (T, th, tw) tile stack of label_dtype (umi_grid_labels)."""
    from . import lib as L
    from . import ops
    ops._need_cuda(m)
    if m.dim() != 2 or m.dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"grid_maps: expected an HW uint8 or float32 map, got {tuple(m.shape)} {m.dtype}")
    dt = np.uint8 if label_dtype in (torch.uint8, np.uint8, "uint8") else _np_label_dtype(label_dtype)
    H, W = m.shape
    pad_top, pad_left = int(pad_top), int(pad_left)
    Hp, Wp, th, tw = _grid_dims(H, W, pad_top, pad_left, th, tw, padded)
    m = m.contiguous()
    out = torch.empty(((Hp // th) * (Wp // tw), th, tw), dtype=_LABEL_TORCH[dt], device=m.device)
    _status(L.fn("umi_grid_labels")(m.data_ptr(), 0 if m.dtype == torch.uint8 else 1, H, W, pad_top, pad_left, Hp, Wp, th, tw,
                                    out.data_ptr(), _LABEL_CODE[dt], float(label_scale), ops._stream()), "umi_grid_labels", (Hp, Wp))
    return out


class CropTransform:
    """DataRandomCrop's two paths over a CropPool.  crop = the network size; label_scale / label_dtype as TrainTransform.

        x, label[, dots] = tf(pool, crops=None, params=None, geom=None, indices=None)     # a training batch
        x, label[, dots] = tf.grid(pool, index, pad=None)                                 # one validation image's tiles

    crops: int32 (N, 3) rows [index, r0, c0]; None draws them, and the parameters, for the images `indices` (None: the whole
    pool) with draw_crop_params from py_rng / np_rng.  Host tables are checked against the pool and uploaded with one copy;
    device tables come with device `params` and `geom` and are not read back.  dots come back when the pool has dot maps.  A
    device pool runs the kernels of csrc/crops.hip, a CPU pool the NumPy statements."""

    def __init__(self, crop, augmentation, label_scale=1.0, label_dtype=torch.int64, py_rng=random, np_rng=np.random):
        self.crop = int(crop)
        if self.crop < 1:
            raise ValueError(f"crop size {crop}")
        self.augmentation = bool(augmentation)
        self.label_scale = float(label_scale)
        _np_label_dtype(label_dtype)
        self.label_dtype = label_dtype
        self.py_rng, self.np_rng = py_rng, np_rng

    def draw(self, pool, indices=None):
        return draw_crop_params(pool.sizes, self.crop, self.augmentation, self.py_rng, self.np_rng, indices)

    def __call__(self, pool, crops=None, params=None, geom=None, indices=None):
        if crops is None:
            crops, drawn = self.draw(pool, indices)
            params = drawn if params is None else params
        elif params is None:
            params = draw_params(len(crops), self.py_rng, self.np_rng) if self.augmentation else no_augmentation(len(crops))
        if pool.is_cuda:
            c, p, g = _dev_crop_tables(pool, crops, params, geom, self.crop)
            out = (crop_image(pool, c, p, g, self.crop),
                   crop_maps(pool, pool.labels, c, p, g, self.crop, self.label_scale, self.label_dtype))
            return out if pool.dots is None else out + (crop_maps(pool, pool.dots, c, p, g, self.crop, 1.0, torch.uint8),)
        crops = np.asarray(crops.cpu() if isinstance(crops, torch.Tensor) else crops)
        params = np.asarray(params.cpu() if isinstance(params, torch.Tensor) else params)
        _check_crops(crops, pool.sizes, self.crop)
        if params.shape != (crops.shape[0], 4):
            raise ValueError(f"expected ({crops.shape[0]}, 4) parameters, got {params.shape}")
        xs, ls, ds = [], [], []
        for n, row in enumerate(crops):
            i = int(row[0])
            x, (lab,), d = crop_transform_numpy(pool.image(i).numpy(), [pool.label(i).numpy()], row, params[n], self.crop,
                                                None if geom is None else np.asarray(geom)[n], self.label_scale, self.label_dtype,
                                                None if pool.dots is None else pool.dot(i).numpy())
            xs.append(x)
            ls.append(lab)
            ds.append(d)
        out = (torch.from_numpy(np.stack(xs)), torch.from_numpy(np.stack(ls)))
        return out if pool.dots is None else out + (torch.from_numpy(np.stack(ds)),)

    def grid(self, pool, index, pad=None):
        """The (T, C, crop, crop) tile stack of image `index`, its (T, crop, crop) labels (and dots).  pad: None draws
        (pad_top, pad_left) as the reference's `pad_image` does, 'center' is test.py's rule, or the pair itself."""
        index = int(index)
        if not 0 <= index < len(pool):
            raise ValueError(f"image index {index} outside the pool of {len(pool)} images")
        H, W = (int(v) for v in pool.sizes[index])
        if pad is None:
            pad = draw_pad(H, W, self.crop, self.py_rng)
        elif isinstance(pad, str):
            if pad != "center":
                raise ValueError(f"pad takes None, 'center' or (pad_top, pad_left), got {pad!r}")
            pad = center_pad(H, W, self.crop)
        top, left = int(pad[0]), int(pad[1])
        t = self.crop
        _grid_dims(H, W, top, left, t, t, None)
        if pool.is_cuda:
            out = (grid_image(pool.image(index), top, left, t, t),
                   grid_maps(pool.label(index), top, left, t, t, None, self.label_scale, self.label_dtype))
            return out if pool.dots is None else out + (grid_maps(pool.dot(index), top, left, t, t, None, 1.0, torch.uint8),)
        x, (lab,), d = grid_transform_numpy(pool.image(index).numpy(), [pool.label(index).numpy()], top, left, t, t,
                                            label_scale=self.label_scale, label_dtype=self.label_dtype,
                                            dots=None if pool.dots is None else pool.dot(index).numpy())
        out = (torch.from_numpy(x), torch.from_numpy(lab))
        return out if pool.dots is None else out + (torch.from_numpy(d),)


class CropBatches:
    """The loader of the crop datasets for `Trainer` (dataloaders['train' | 'val'], batch_transform=None): an iterable with
    __len__ over the images `indices` of a CropPool (None: all; a data-parallel caller passes its rank's shard -- equal lengths
    over ranks stay the caller's business).

    train=True: batches (x (B, C, crop, crop), label (B, crop, crop)) of one fresh random crop per image, batch_size images per
    batch, the last one shorter (drop_last=False); shuffle=True permutes the images with torch.randperm(generator) every epoch.
    train=False: one item (x (T, C, crop, crop), label (T, crop, crop)) per image: all tiles of the padded image, what the
    reference's validation loop feeds after its squeeze(0); Trainer's val_batch groups images with equal T.  The validation
    grid is not augmented.  with_dots=True appends the dot maps to every item (loss.MRAccuracy loops)."""

    def __init__(self, pool, crop, batch_size, augmentation, train, indices=None, shuffle=False, generator=None, with_dots=False):
        self.pool, self.train = pool, bool(train)
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError(f"batch_size {batch_size}")
        self.indices = np.arange(len(pool)) if indices is None else np.asarray(indices, dtype=np.int64).reshape(-1)
        if np.any((self.indices < 0) | (self.indices >= len(pool))):
            raise ValueError(f"indices outside the pool of {len(pool)} images")
        if with_dots and pool.dots is None:
            raise ValueError("with_dots=True needs a pool with dot maps")
        if np.any(pool.sizes[self.indices] < int(crop)):
            raise ValueError(f"an image of the pool is smaller than the crop {crop}")
        self.shuffle, self.generator, self.with_dots = bool(shuffle), generator, bool(with_dots)
        self.transform = CropTransform(crop, augmentation and self.train)

    def __len__(self):
        n = len(self.indices)
        return (n + self.batch_size - 1) // self.batch_size if self.train else n

    def _item(self, out):
        return out if self.with_dots else out[:2]

    def __iter__(self):
        if not self.train:
            for i in self.indices:
                yield self._item(self.transform.grid(self.pool, i))
            return
        order = self.indices
        if self.shuffle:
            order = order[torch.randperm(len(order), generator=self.generator).numpy()]
        for b in range(0, len(order), self.batch_size):
            yield self._item(self.transform(self.pool, indices=order[b:b + self.batch_size]))
