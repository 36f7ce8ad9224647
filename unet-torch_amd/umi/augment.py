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

Out of scope: file reading, the imgaug / torchio / ColorJitter pipelines, stain normalisation, the crop datasets.
"""
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
