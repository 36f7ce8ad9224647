"""GPU: the binary-model inference path on the MI355X -- umi.infer.binary_mask / zoom_nearest / label_components /
count_objects / predict_binary_mask(_tiled) and loss.MRAccuracy on device tensors -- against torch.sigmoid on the CPU, SciPy's
recorded results (tests/golden/binary_infer.npz) and the NumPy statements the CPU suite pins to SciPy
(umi.components.label_components_numpy, tools.gen_golden_binary_infer.zoom_nearest_numpy).  Every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from oracle import recipe
from tools import gen_golden_binary_infer as G
from tools import gen_golden_resize as GR

pytestmark = pytest.mark.gpu
DEV = "cuda"
_NAMES = list(G.masks())


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: torch.cuda.is_available() is False")


@pytest.fixture(scope="module")
def fixture(golden_dir):
    return np.load(os.path.join(golden_dir, "binary_infer.npz"))


def _mask(g, name):
    shape = tuple(g[f"mask_{name}_shape"])
    return np.unpackbits(g[f"mask_{name}_bits"])[:shape[0] * shape[1]].reshape(shape)


# ---- threshold ------------------------------------------------------------------------------------------------------------------
def _check_binary_mask(x_dev):
    from umi import infer
    got = infer.binary_mask(x_dev).cpu()
    want = (torch.sigmoid(x_dev.cpu()) >= 0.5).to(torch.uint8)[:, 0]
    assert got.dtype == torch.uint8 and got.shape == want.shape
    assert torch.equal(got, want)
    return got


def test_binary_mask_special_values():
    _need_gpu()
    from umi import infer
    cut = infer.SIGMOID_HALF_CUTOFF_BITS
    bits = np.concatenate([
        np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x80800000,
                  0x7F800000, 0xFF800000], dtype=np.uint32),                        # +-0, denormals, smallest normals, +-inf
        np.arange(cut - 1000, cut + 1001, dtype=np.uint32)])                       # the cut-off and its +-1000 neighbours
    vals = np.concatenate([bits.view(np.float32), np.array([1e-8, -1e-8, 1e-6, -1e-6], dtype=np.float32)])
    x = torch.from_numpy(vals).reshape(1, 1, 1, -1).to(DEV)
    got = _check_binary_mask(x)
    k = 10 + 1000
    assert got[0, 0, k] == 1 and got[0, 0, k + 1] == 0 and got[0, 0, k - 1] == 1    # at, just below, just above the cut-off
    nan = torch.tensor([float("nan"), -float("nan"), 1.0, -1.0], device=DEV).reshape(1, 1, 2, 2)
    assert infer.binary_mask(nan).cpu().flatten().tolist() == [0, 0, 1, 0]


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 1, 33, 65), (16, 1, 512, 512)])
def test_binary_mask_random_logits(shape):
    _need_gpu()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(shape, generator=g)
    x.view(-1)[::7] *= 1e-7                             # many logits around the cut-off
    _check_binary_mask(x.to(DEV))


def test_binary_mask_on_a_view_one_float_into_its_storage():
    _need_gpu()
    g = torch.Generator().manual_seed(4)
    t = torch.randn(3, 1, 33, 65, generator=g) * 1e-6
    buf = torch.empty(t.numel() + 1, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    _check_binary_mask(v)


def test_binary_mask_rejects_other_inputs():
    _need_gpu()
    from umi import infer
    with pytest.raises(ValueError):
        infer.binary_mask(torch.zeros(2, 2, 4, 4, device=DEV))
    with pytest.raises(ValueError):
        infer.binary_mask(torch.zeros(2, 1, 4, 4, device=DEV, dtype=torch.float16))
    with pytest.raises(RuntimeError):
        infer.binary_mask(torch.zeros(2, 1, 4, 4))


# ---- nearest resize -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(G.ZOOM_CASES)))
def test_zoom_nearest_matches_scipy_fixture(fixture, i):
    _need_gpu()
    from umi import infer
    seed, shape, ohw, dtype = G.ZOOM_CASES[i]
    a = G.zoom_input(seed, shape, dtype)
    got = infer.zoom_nearest(torch.from_numpy(a).to(DEV), ohw).cpu().numpy()
    assert got.shape == tuple(fixture[f"zoom{i}_shape"]) and got.dtype == a.dtype
    if f"zoom{i}_checksum" in fixture:
        assert G.checksum(got) == int(fixture[f"zoom{i}_checksum"]) and got.sum() == int(fixture[f"zoom{i}_sum"])
    elif dtype == "uint8":
        np.testing.assert_array_equal(np.packbits(got), fixture[f"zoom{i}_bits"])
    else:
        np.testing.assert_array_equal(got, fixture[f"zoom{i}"])
    np.testing.assert_array_equal(got, G.zoom_nearest_numpy(a, ohw))


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_zoom_nearest_matches_rule_on_the_resize_sweep(dtype):
    """Every size class of gen_golden_resize.SWEEP (strips up and down, both axes, equal sizes, 1- to 3-pixel axes, sizes whose
    last sample lies above in - 1, evaluation sizes), its channel count used as the batch."""
    _need_gpu()
    from umi import infer
    for k, (shape, ohw) in enumerate(GR.SWEEP):
        a = GR.make(200 + k, shape, dtype)
        a = a[None] if a.ndim == 2 else np.ascontiguousarray(a.transpose(2, 0, 1))
        got = infer.zoom_nearest(torch.from_numpy(a).to(DEV), ohw).cpu().numpy()
        np.testing.assert_array_equal(got, G.zoom_nearest_numpy(a, ohw), err_msg=f"{shape} -> {ohw}")
    one = infer.zoom_nearest(torch.ones(512, 512, dtype=torch.uint8, device=DEV), (224, 224)).cpu().numpy()
    assert one.shape == (224, 224) and not one[-1].any() and not one[:, -1].any() and one[:-1, :-1].all()


# ---- labelling ------------------------------------------------------------------------------------------------------------------
def _first_pixels(labels, n):
    """Flat index of the first pixel of labels 1..n of one (H, W) map."""
    flat = labels.ravel()
    idx = np.nonzero(flat)[0]
    first = np.full(n + 1, flat.size, dtype=np.int64)
    np.minimum.at(first, flat[idx], idx)
    return first[1:]


def _assert_equal_to_numpy(m_np, outs):
    from umi import components as C
    want = C.label_components_numpy(m_np)
    for got, w, what in zip(outs, want, ("labels", "counts", "area", "sum_y", "sum_x")):
        assert got.dtype == torch.from_numpy(w).dtype and tuple(got.shape) == w.shape, what
        assert torch.equal(got.cpu(), torch.from_numpy(w)), what
    return want


@pytest.mark.parametrize("name", _NAMES)
def test_label_components_matches_scipy_fixture(fixture, name):
    _need_gpu()
    from umi import components as C, infer
    m = _mask(fixture, name)
    md = torch.from_numpy(m).to(DEV)
    outs = infer.label_components(md, check=True)
    labels, counts, area, sum_y, sum_x = (t.cpu().numpy() for t in outs)
    n = int(fixture[f"mask_{name}_count"])
    assert labels.shape == m.shape and counts.tolist() == [n]
    np.testing.assert_array_equal(area[0, :n], fixture[f"mask_{name}_area"])
    np.testing.assert_array_equal(sum_y[0, :n], fixture[f"mask_{name}_sum_y"])
    np.testing.assert_array_equal(sum_x[0, :n], fixture[f"mask_{name}_sum_x"])
    np.testing.assert_array_equal(_first_pixels(labels, n), fixture[f"mask_{name}_first"])
    assert C.label_checksum(labels) == int(fixture[f"mask_{name}_checksum"])
    assert not area[0, n:].any() and not sum_y[0, n:].any() and not sum_x[0, n:].any()
    _assert_equal_to_numpy(m, outs)
    assert infer.count_objects(md, check=True).cpu().tolist() == [n]
    assert infer.count_objects((md * 255).contiguous(), check=True).cpu().tolist() == [n]      # foreground = non-zero


@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (33, 65), (63, 64), (65, 129), (512, 512)])
@pytest.mark.parametrize("N", [1, 3, 16])
def test_label_components_random_batches(N, hw):
    _need_gpu()
    from umi import infer
    rng = np.random.default_rng(N * 1000 + hw[0] + hw[1])
    dens = rng.choice([0.05, 0.3, 0.45, 0.5, 0.6], size=N)
    m = (rng.random((N,) + hw) < dens[:, None, None]).astype(np.uint8)
    md = torch.from_numpy(m).to(DEV)
    outs = infer.label_components(md, check=True)
    want = _assert_equal_to_numpy(m, outs)
    counts = infer.count_objects(md, check=True)
    assert counts.dtype == torch.int32 and torch.equal(counts, outs[1])
    for b in range(N):                                     # rows beyond counts are 0
        n = int(want[1][b])
        assert not outs[2][b, n:].any() and not outs[3][b, n:].any() and not outs[4][b, n:].any()
    again = infer.label_components(md, check=True)          # two runs: identical bits
    for a, b in zip(outs, again):
        assert torch.equal(a, b)


@pytest.mark.parametrize("hw", [(90, 37), (70, 63), (5, 200), (129, 64), (3, 2)])
def test_label_components_narrow_and_odd_widths(hw):
    """Widths under 64 pixels take the statistics pass's per-run path (a 64-pixel chunk then spans several rows); widths that
    are no multiple of 64 put row ends inside chunks."""
    _need_gpu()
    from umi import infer
    rng = np.random.default_rng(hw[0] * 7 + hw[1])
    for d in (0.1, 0.5, 0.7, 1.0):
        m = (rng.random((5,) + hw) < d).astype(np.uint8)
        _assert_equal_to_numpy(m, infer.label_components(torch.from_numpy(m).to(DEV), check=True))


def test_label_components_2048():
    _need_gpu()
    from umi import infer
    rng = np.random.default_rng(2048)
    m = (rng.random((1, 2048, 2048)) < 0.45).astype(np.uint8)
    m[0, 1000:1040] = 1                                     # and one band across every vertical seam
    md = torch.from_numpy(m).to(DEV)
    outs = infer.label_components(md, check=True)
    _assert_equal_to_numpy(m, outs)
    assert torch.equal(infer.count_objects(md, check=True), outs[1])


def test_label_components_after_other_sizes_reuses_the_workspace():
    """The workspace is shared and re-initialised by every call: a small mask after a large one, then the large one again."""
    _need_gpu()
    from umi import infer
    rng = np.random.default_rng(5)
    big = (rng.random((2, 300, 200)) < 0.5).astype(np.uint8)
    small = (rng.random((40, 50)) < 0.5).astype(np.uint8)
    for m in (big, small, big):
        _assert_equal_to_numpy(m, infer.label_components(torch.from_numpy(m).to(DEV), check=True))


def test_label_components_rejects_other_inputs():
    _need_gpu()
    from umi import infer
    m = torch.ones(4, 8, 8, dtype=torch.uint8, device=DEV)
    for f in (infer.label_components, infer.count_objects):
        with pytest.raises(ValueError):
            f(m[:, :, ::2])                                 # non-contiguous
        with pytest.raises(ValueError):
            f(m.float())
        with pytest.raises(ValueError):
            f(m[None])
        with pytest.raises(ValueError):
            f(m[:0])
        with pytest.raises(RuntimeError):
            f(m.cpu())


# ---- MRAccuracy -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.MR_CASES)
def test_mraccuracy_device_matches_reference(fixture, name):
    _need_gpu()
    import loss as L
    pred, target = G.mr_case(name)
    got = L.MRAccuracy(torch.from_numpy(pred).to(DEV), torch.from_numpy(target).to(DEV))
    assert isinstance(got, float) and got == float(fixture[f"mr_{name}"])
    assert L.MRAccuracy(torch.from_numpy(pred).to(DEV), torch.from_numpy(target)) == got       # dot maps left on the host


def test_mraccuracy_device_matches_cpu_path_at_full_size():
    _need_gpu()
    import loss as L
    rng = np.random.default_rng(16)
    B, H, W = 16, 512, 512
    low = rng.standard_normal((B, H // 16, W // 16))
    pred = (np.kron(low, np.ones((16, 16))) + 0.5 * rng.standard_normal((B, H, W)) - 0.7).astype(np.float32)[:, None]
    pred.reshape(-1)[::11] *= 1e-7
    target = (rng.random((B, H, W)) < 0.002).astype(np.float32)
    target[3] = 0
    pred[5] = -1.0
    target[5] = 0
    p, t = torch.from_numpy(pred), torch.from_numpy(target)
    got = L.MRAccuracy(p.to(DEV), t.to(DEV))
    assert got == L.MRAccuracy(p, t)
    with pytest.raises(ValueError):
        L.MRAccuracy(torch.zeros(2, 2, 8, 8, device=DEV), torch.zeros(2, 8, 8, device=DEV))


# ---- model entry points ---------------------------------------------------------------------------------------------------------
def _unet(seed=31):
    import Model
    m = Model.UNet(1, 1, 8, False, compute_dtype="fp32")
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=seed))
    return m.to(DEV)


def _cpu_threshold(logits):
    return (torch.sigmoid(logits.cpu()) >= 0.5).to(torch.uint8)[:, 0].numpy()


def _input(shape, seed):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed))
    return x.to(DEV)


def test_predict_binary_mask_equals_threshold_and_resize_of_the_models_logits():
    _need_gpu()
    from umi import infer
    m = _unet()
    m.train()
    x = _input((2, 1, 64, 96), 1)
    got = infer.predict_binary_mask(m, x)
    assert m.training                                       # the mode is restored
    m.eval()
    with torch.no_grad():
        logits = m(x)
    want = _cpu_threshold(logits)
    assert 0 < want.mean() < 1, "degenerate test: the model's mask is constant"
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 64, 96)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    np.testing.assert_array_equal(infer.predict_binary_mask(m, x, out_hw=(64, 96)).cpu().numpy(), want)
    for ohw in ((100, 83), (224, 224), (31, 200)):
        got = infer.predict_binary_mask(m, x, out_hw=ohw).cpu().numpy()
        np.testing.assert_array_equal(got, G.zoom_nearest_numpy(want, ohw), err_msg=str(ohw))


def test_predict_binary_mask_returns_a_tuple_for_two_heads():
    _need_gpu()
    import Model
    from umi import infer
    m = Model.UNet_multitask(1, 1, 8, False, compute_dtype="fp32")
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=22))
    m.to(DEV).eval()
    x = _input((1, 1, 64, 64), 2)
    got = infer.predict_binary_mask(m, x, out_hw=(90, 70))
    with torch.no_grad():
        outs = m(x)
    assert isinstance(got, tuple) and len(got) == len(outs) == 2
    for g, o in zip(got, outs):
        np.testing.assert_array_equal(g.cpu().numpy(), G.zoom_nearest_numpy(_cpu_threshold(o), (90, 70)))


def test_predict_binary_mask_tiled_equals_one_tile_forwards_placed_by_hand():
    _need_gpu()
    from umi import infer
    m = _unet(seed=32).eval()
    c = 64
    x = _input((1, 1, 2 * c, 3 * c), 3)
    got = infer.predict_binary_mask_tiled(m, x, c)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (2 * c, 3 * c) and got.is_cuda
    want = np.zeros((2 * c, 3 * c), dtype=np.uint8)
    with torch.no_grad():
        for i in range(0, 2 * c, c):
            for j in range(0, 3 * c, c):
                want[i:i + c, j:j + c] = _cpu_threshold(m(x[:, :, i:i + c, j:j + c].contiguous()))[0]
    assert 0 < want.mean() < 1
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    with pytest.raises(ValueError):
        infer.predict_binary_mask_tiled(m, x, 48)
    with pytest.raises(ValueError):
        infer.predict_binary_mask_tiled(m, torch.cat([x, x]), c)
