"""Fixtures for the crop datasets (umi.augment CropPool / CropTransform) -> tests/golden/crop_batches.npz.  Runs on the CPU,
needs SciPy.

The reference's `DataRandomCrop` (DataLoader.py:928-1069, `pad_image` :27-47) and test.py's `preprocessCrop` (:91-128) written out
with SciPy's own `ndimage.rotate`, `np.pad` and NumPy's `mean` / `std`, drawing from the seeded global `random` / `np.random` in
the reference's order:

  train_<pool>_{x,label,dots}_<s>   sample s of TRAIN_INDICES[pool]: crop window, augmentation, z-normalisation, CHW reversed
  train_<pool>_crops / _params      the draws made on the way: rows [index, r0, c0] and [mode, k, axis, angle]
  train_<pool>_next                 [random.random(), np.random.random()] drawn AFTER the last sample: the generators' state
  val_<pool>_<i>_{x,label,dots}     the tile stack of image i of VAL_IMAGES[pool], pads drawn as `pad_image` draws them
  val_<pool>_pads / _next           the (pad_top, pad_left) drawn, and the generator's state after them
  center_<pool>_<i>_x               `preprocessCrop` of image i: centred, value 255, the whole padded image

The pools are regenerated from the seeds by the tests (pool() below); only the outputs and the draws are stored.  The
reference's own real-valued images (the haematoxylin channel of rgb2hed) are float64 arrays, so a float32 pool's images enter
the reference arithmetic widened to float64 (as_reference below): NumPy would otherwise keep mean, std and quotient in float32.
"""
import os
import random

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CROP = 16
POOLS = {  # name: (dtype, [image shapes]); one image with H == W == CROP: randint(0, 0), and no padding
    "rgb": ("uint8", [(26, 35, 3), (21, 21, 3), (38, 27, 3)]),
    "gray": ("uint8", [(26, 35), (16, 16), (38, 27)]),
    "f32": ("float32", [(26, 35, 3), (21, 21, 3)]),
}
SEEDS = {"rgb": (101, 102), "gray": (201, 202), "f32": (301, 302)}            # random.seed, np.random.seed
TRAIN_INDICES = {"rgb": [0, 1, 2, 2, 1, 0, 2, 0], "gray": [0, 1, 2, 1, 2, 0, 0, 2], "f32": [0, 1, 1, 0]}
VAL_IMAGES = {"rgb": [0, 2], "gray": [1, 2], "f32": [1]}


def pool(name):
    """(images, label maps, dot maps) of a pool, from seeds."""
    dtype, shapes = POOLS[name]
    base = sum(ord(c) for c in name)
    images, labels, dots = [], [], []
    for i, shape in enumerate(shapes):
        rng = np.random.default_rng(base * 10 + i)
        img = rng.random(shape) * 255.0
        images.append(img.astype(np.uint8) if dtype == "uint8" else (img / 255.0 - 0.3).astype(np.float32))
        cells = rng.integers(0, 3, size=((shape[0] + 3) // 4, (shape[1] + 3) // 4)).astype(np.uint8)
        labels.append(np.kron(cells, np.ones((4, 4), dtype=np.uint8))[:shape[0], :shape[1]].copy())
        dots.append(((rng.random(shape[:2]) < 0.03) * 255).astype(np.uint8))
    return images, labels, dots


def as_reference(image):
    return image.astype(np.float64) if image.dtype == np.float32 else image


def normalise(image, label):
    """The tail of the reference's `transform`: float64 z-normalisation, CHW with reversed channels, label .long()."""
    z = (image - np.mean(image, axis=(0, 1))) / np.std(image, axis=(0, 1))
    z = z[None] if z.ndim == 2 else z.transpose((2, 0, 1))[::-1]
    return np.ascontiguousarray(z.astype(np.float32)), label.astype(np.float32).astype(np.int64)


def reference_train_sample(image, label, dot, crop, augmentation):
    """One training sample, drawing from the global generators.  Returns (x, label, dots, crop row tail, parameter row)."""
    from scipy import ndimage
    r0 = random.randint(0, image.shape[0] - crop)
    c0 = random.randint(0, image.shape[1] - crop)
    arrays = [a[r0:r0 + crop, c0:c0 + crop] for a in (image, label, dot)]
    p = (0, 0, 0, 0)
    if augmentation:
        if random.random() > 0.5:
            k = np.random.randint(0, 4)
            axis = np.random.randint(0, 2)
            arrays = [np.flip(np.rot90(a, k), axis=axis).copy() for a in arrays]
            p = (1, k, axis, 0)
        elif random.random() > 0.5:
            angle = np.random.randint(-20, 20)
            arrays = [ndimage.rotate(a, angle, order=0, reshape=False) for a in arrays]
            p = (2, 0, 0, angle)
    x, lab = normalise(arrays[0], arrays[1])
    return x, lab, arrays[2], (r0, c0), p


def pad_to(arrays, pad_top, pad_left, padding_h, padding_w, image_value):
    out = []
    for a in arrays:
        widths = ((pad_top, padding_h - pad_top), (pad_left, padding_w - pad_left))
        if a.ndim == 3:
            out.append(np.pad(a, widths + ((0, 0),), mode="constant", constant_values=image_value))
        else:
            out.append(np.pad(a, widths, mode="constant", constant_values=0 if image_value is None else image_value))
    return out


def reference_val_item(image, label, dot, crop):
    """One validation item: pads drawn from the global `random` (left first), 255 for an HWC image and 0 for an HW one."""
    padding_h, padding_w = (-image.shape[0]) % crop, (-image.shape[1]) % crop
    pad_left = random.randint(0, padding_w)
    pad_top = random.randint(0, padding_h)
    img = pad_to([image], pad_top, pad_left, padding_h, padding_w, 255 if image.ndim == 3 else 0)[0]
    lab, dt = pad_to([label, dot], pad_top, pad_left, padding_h, padding_w, None)
    x, lab = normalise(img, lab)
    xs, ls, ds = [], [], []
    for i in range(0, x.shape[1], crop):
        for j in range(0, x.shape[2], crop):
            xs.append(x[:, i:i + crop, j:j + crop])
            ls.append(lab[i:i + crop, j:j + crop])
            ds.append(dt[i:i + crop, j:j + crop])
    return np.stack(xs), np.stack(ls), np.stack(ds), (pad_top, pad_left)


def reference_center(image, crop):
    """test.py's preprocessCrop for the image: centred, value 255 whatever the image's rank, no tiling."""
    padding_h, padding_w = (-image.shape[0]) % crop, (-image.shape[1]) % crop
    img = pad_to([image], padding_h // 2, padding_w // 2, padding_h, padding_w, 255)[0]
    return normalise(img, np.zeros(img.shape[:2], np.uint8))[0][None]


if __name__ == "__main__":
    import scipy
    out = {"scipy_version": np.array(scipy.__version__)}
    for name in POOLS:
        images, labels, dots = pool(name)
        random.seed(SEEDS[name][0])
        np.random.seed(SEEDS[name][1])
        crops, params = [], []
        for s, i in enumerate(TRAIN_INDICES[name]):
            x, lab, dt, rc, p = reference_train_sample(as_reference(images[i]), labels[i], dots[i], CROP, True)
            out[f"train_{name}_x_{s}"], out[f"train_{name}_label_{s}"], out[f"train_{name}_dots_{s}"] = x, lab, dt
            crops.append((i,) + rc)
            params.append(p)
        out[f"train_{name}_crops"] = np.array(crops, dtype=np.int32)
        out[f"train_{name}_params"] = np.array(params, dtype=np.int32)
        out[f"train_{name}_next"] = np.array([random.random(), np.random.random()])
        pads = []
        for i in VAL_IMAGES[name]:
            x, lab, dt, pad = reference_val_item(as_reference(images[i]), labels[i], dots[i], CROP)
            out[f"val_{name}_{i}_x"], out[f"val_{name}_{i}_label"], out[f"val_{name}_{i}_dots"] = x, lab, dt
            pads.append(pad)
            out[f"center_{name}_{i}_x"] = reference_center(as_reference(images[i]), CROP)
        out[f"val_{name}_pads"] = np.array(pads, dtype=np.int32)
        out[f"val_{name}_next"] = np.array([random.random()])
    path = os.path.join(REPO, "tests", "golden", "crop_batches.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes,", len(out), "arrays")
    for name in POOLS:
        print(name, "modes", sorted(set(out[f"train_{name}_params"][:, 0].tolist())), "pads", out[f"val_{name}_pads"].tolist())
