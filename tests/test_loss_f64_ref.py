"""Pins tests/loss_f64_ref.py, the float64 statements that tests/test_gpu_loss_edges.py holds the loss kernels to, where no
GPU is needed: every statement reproduces the reference's recorded outputs (tests/golden/binary_losses.npz,
tests/golden/hausdorff_dt.npz) at the tolerances the GPU tests use for the same fixtures, the coefficients behind the
gradient scales reproduce the autograd gradient, the SciPy fields equal loss._distance_field bit for bit on the edge shapes,
and every premise the GPU tests assert on the reference alone holds on the same seeded inputs."""
import os

import numpy as np
import pytest
import torch

from tests import loss_f64_ref as R
from tests import test_gpu_loss_edges as E


@pytest.fixture(scope="module")
def binary_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "binary_losses.npz"))


@pytest.fixture(scope="module")
def hdt_golden(golden_dir):
    return np.load(os.path.join(golden_dir, "hausdorff_dt.npz"))


def _close(ref, loss_want, grad_want, loss_tol, name):
    assert abs(ref.loss.item() - loss_want) <= loss_tol * abs(loss_want), (name, ref.loss.item(), loss_want)
    assert np.abs(ref.grad.numpy() - grad_want).max() <= 1e-5 * np.abs(grad_want).max(), name


def test_statements_reproduce_the_binary_loss_fixtures(binary_golden):
    g = binary_golden
    seen = set()
    for e in (str(s) for s in g["entries"]):
        c, lt = e.split(":")
        x, t = torch.from_numpy(g[f"{c}_pred"]), torch.from_numpy(g[f"{c}_target"])
        want, gw = float(g[f"{e}_loss"]), g[f"{e}_grad"]
        if lt == "dice_bce":
            ref = R.dice_bce(x, t)
        elif lt == "Tversky":
            ref = R.tversky_bin(x, t, E.ALPHA, E.BETA) if x.shape[1] == 1 else R.tversky_mc(x, t, E.ALPHA, E.BETA)
        else:
            # the reference's selected set must be one the float64 keys allow: nothing outside ranks before anything inside
            mode = 0 if lt == "TopK" else 1
            idx = np.flatnonzero(gw.reshape(-1))
            assert idx.size == (x.numel() // 2 if lt == "TopK" else 500), e
            key = R.selection_keys(x, t, mode).numpy()
            outside = np.setdiff1d(np.arange(key.size), idx)
            if outside.size:
                assert key[idx].max() <= key[outside].min() + 1e-6 * abs(key[outside].min()), e
            ref = R.selected_mean(x, t, idx)
        _close(ref, want, gw, 2e-6, e)
        seen.add(lt)
    assert seen == {"dice_bce", "Tversky", "TopK", "BCE_HEM"}


def test_statements_reproduce_the_hausdorff_fixtures(hdt_golden):
    g = hdt_golden
    alpha = float(g["alpha"])
    for c in (str(n) for n in g["cases"]):
        x, t = torch.from_numpy(g[f"{c}_pred"]), torch.from_numpy(g[f"{c}_target"])
        fp, ft = R.edt_fields(torch.sigmoid(x).numpy()), R.edt_fields(t.numpy())
        assert fp.dtype == np.float32 and np.array_equal(fp.view(np.int32), g[f"{c}_pred_dt"].view(np.int32)), c
        assert np.array_equal(ft.view(np.int32), g[f"{c}_target_dt"].view(np.int32)), c
        _close(R.hdt(x, t, alpha, fp, ft), float(g[f"{c}_loss"]), g[f"{c}_grad"], 1e-6, c)


def test_bce_terms_are_torchs_float64_bce(binary_golden):
    import torch.nn.functional as F
    x = torch.from_numpy(binary_golden["saturated_pred"])[:, 0]
    t = torch.from_numpy(binary_golden["soft_targets_target"])[:, :x.shape[1], :x.shape[2]]
    x = x[:, :t.shape[1], :t.shape[2]]
    want = F.binary_cross_entropy_with_logits(x.double(), t.double(), reduction="none")
    assert torch.allclose(R.bce_terms(x, t), want, rtol=1e-12, atol=0)
    # its autograd gradient is sigmoid(x) - t to float64 accuracy, at the kink of |x| and where the sigmoid underflows too
    xe = torch.tensor([0.0, -0.0, 100.0, -100.0, 30.0, -30.0, 0.25] * 2, dtype=torch.float64, requires_grad=True)
    te = torch.tensor([0.0] * 7 + [1.0] * 7, dtype=torch.float64)
    R.bce_terms(xe, te).sum().backward()
    s = torch.sigmoid(xe.detach())
    assert bool(((xe.grad - (s - te)).abs() <= 1e-15 * (s + te)).all())
    x0, t0 = E.sel_tie_inputs(64)
    ref = R.selected_mean(x0, t0, np.arange(16))
    assert torch.equal(ref.grad[:16], (0.5 - t0[:16].double()) / 16) and bool((ref.grad[16:] == 0).all())


@pytest.mark.parametrize("lt", ["dice_bce", "Tversky"])
@pytest.mark.parametrize("content", E.BIN_CONTENTS)
def test_binary_coefficients_reproduce_the_autograd_gradient(lt, content):
    """grad = cb (s - t) + (c1 t + c2) s (1 - s): the scale |cb| (s + |t|) + (|c1 t| + |c2|) s bounds these terms."""
    for B, H, W in sorted({c[:3] for c in E.BIN_CASES}):
        x, t = E.bin_inputs(B, H, W, content)
        ref = E.bin_ref(lt, B, H, W, content)
        cb, c1, c2 = ref.coef
        s, td = torch.sigmoid(x.double()).reshape(B, -1), t.double().reshape(B, -1)
        want = cb * (s - td) + (c1 * td + c2) * (s * (1 - s))
        err = (ref.grad.reshape(B, -1) - want).abs()
        assert bool((err <= 1e-12 * ref.scale.reshape(B, -1) + 1e-300).all()), (lt, content, (B, H, W))
        assert torch.isfinite(ref.S) and ref.S >= ref.loss.abs() * (1 - 1e-12)


def test_binary_premises():
    for B, H, W in sorted({c[:3] for c in E.BIN_CASES}):
        x, t = E.bin_inputs(B, H, W, "negative")
        assert float(t.min()) < -0.25 and float((t.abs() - t).sum()) > 0.5
        x, t = E.bin_inputs(B, H, W, "edges")
        assert bool((t[B - 1] == 1).all()) and (B == 1 or bool((t[0] == 0).all()))
        assert set(x[B // 2].unique().tolist()) <= {-100.0, -30.0, 30.0, 100.0}
        x, t = E.bin_inputs(B, H, W, "soft")
        assert 0.0 <= float(t.min()) and float(t.max()) <= 1.0
    assert 300 * 5 > 1024 and (2, 64, 65, 0, 0) in E.BIN_CASES


@pytest.mark.parametrize("C", [2, 3, 8])
def test_multiclass_coefficients_and_off_class_labels(C):
    """grad_c = p_c (h_c - sum_k h_k p_k), h = c1 [label == c] + c2; labels that equal no class enter no T_c and no TP_c."""
    for dtype in [None] + list(E.MC_DTYPES):
        x, labels = E.mc_inputs(C, E.MC_SMALL, dtype)
        ref = E.mc_ref(C, E.MC_SMALL, dtype)
        c1, c2 = ref.coef
        p = torch.softmax(x.double(), dim=1)
        onehot = torch.stack([labels == c for c in range(C)], dim=1).double()
        h = c1 * onehot + c2
        want = p * (h - (h * p).sum(1, keepdim=True))
        assert bool(((ref.grad - want).abs() <= 1e-12 * ref.scale + 1e-300).all()), (C, dtype)
        if dtype is not None:
            present = set(labels.double().unique().tolist())
            assert set(float(v) for v in E.MC_OFF_CLASS[dtype](C)) <= present and labels.dtype == dtype
            in_class = sum(int((labels == c).sum()) for c in range(C))
            assert 0 < in_class < labels.numel() and int(onehot.sum()) == in_class
            # the same labels clamped into range give another loss: the off-class pixels do matter
            moved = R.tversky_mc(x, labels.double().clamp(0, C - 1).round().long(), E.ALPHA, E.BETA)
            assert abs(moved.loss.item() - ref.loss.item()) > 1e-5        # a hundred times the loss bound


@pytest.mark.parametrize("mode", list(E.SEL_MODES), ids=E.SEL_MODES.get)
def test_selection_premises(mode):
    for N in E.SEL_N:
        x, t = E.sel_inputs(N, E.SEL_N.index(N) % 2)
        E.assert_keys_separated(x, t, mode)
        assert set(t.unique().tolist()) <= {0.0, 1.0} and float(x.abs().max()) <= 3.0 and float(x.abs().min()) > 0
        assert len(torch.unique(x.abs())) == len(torch.unique(x))            # no logit has its mirror image in the grid
        assert E.sel_ks(N)[0] == 1 and E.sel_ks(N)[-1] == N
    x, t = E.sel_inputs(32 * 33, 0)
    E.assert_keys_separated(x, t, mode)
    x, t = E.sel_tie_inputs(E.SEL_TIES_N)
    assert len(np.unique(R.selection_keys(x, t, mode).numpy())) == 1 and 0 < t.sum() < t.numel()
    assert E.SEL_TIES_N == 2 * 16384 + 5 and E.SEL_TIES_K == (16384, 16387, E.SEL_TIES_N - 1)


def test_selection_key_premise_rejects_mirrored_pairs():
    """(x, 1) and (-x, 0) have one float64 key from two different (x, t): the premise must refuse them."""
    x, t = torch.tensor([0.5, -0.5, 1.0]), torch.tensor([1.0, 0.0, 1.0])
    with pytest.raises(AssertionError):
        E.assert_keys_separated(x, t, 0)
    with pytest.raises(AssertionError):
        E.assert_keys_separated(torch.tensor([1.0, 1.0 + 2.0 ** -14]), torch.tensor([0.0, 0.0]), 1)


def test_last_digit_keys_share_their_leading_digits():
    """With torch's CPU arithmetic in place of the device's: the fp32 keys of logits j 2^-e share the leading radix digits."""
    import torch.nn.functional as F
    for mode, e, shared in E.SEL_DIGIT_CASES:
        x, t = E.sel_digit_inputs(32773, e)
        key = torch.sigmoid(x) if mode == 0 else -F.binary_cross_entropy_with_logits(x, t, reduction="none")
        assert E.shared_key_digits(key.numpy()) >= shared and len(np.unique(key.numpy())) >= 128, (mode, e)
    one = np.float32(1.0)
    assert E.shared_key_digits(np.array([one, np.nextafter(one, np.float32(2))])) == 3
    assert E.shared_key_digits(np.array([one, -one])) == 0 and E.shared_key_digits(np.array([one, one])) == 4


@pytest.mark.parametrize("shape", E.HDT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_scipy_fields_equal_the_cpu_path_on_the_edge_shapes(shape):
    import loss as L
    H, W = shape
    masks = E.hdt_masks(H, W)
    assert len(masks) == (6 if H > 1024 else 4) and masks[1].sum() == 1 and masks[2].sum() == H * W - 1
    if H > 1024:
        assert not masks[4][:1024].any() and masks[4][1024:].all() and np.array_equal(masks[5], ~masks[4])
    for x, t, fp, ft in E.hdt_field_batches(H, W):
        assert float(x.abs().min()) >= 0.25                                  # the mask is sign(x) in any arithmetic
        s = torch.sigmoid(x).numpy()
        kinds = {("none" if not (m > 0.5).any() else "all" if (m > 0.5).all() else "mixed") for m in s}
        assert kinds == {"none", "all", "mixed"}
        assert np.array_equal(fp.view(np.int32), L._distance_field(s).view(np.int32))
        assert np.array_equal(ft.view(np.int32), L._distance_field(t.numpy()).view(np.int32))
        assert fp.dtype == np.float32 and fp.shape == tuple(x.shape)
    if shape == (4096, 2):
        assert max(float(b[2].max()) for b in E.hdt_field_batches(H, W)) == np.float32(np.sqrt(4095.0 ** 2 + 1))


@pytest.mark.parametrize("case", E.HDT_BWD_CASES, ids=lambda c: "x".join(map(str, c[:3])))
def test_scipy_fields_equal_the_cpu_path_on_the_gradient_cases(case):
    import loss as L
    B, H, W, _ = case
    x, t, fp, ft = E.hdt_bwd_inputs(B, H, W)
    assert float(x.abs().min()) >= 1e-3 and x.numel() == B * H * W
    assert np.array_equal(fp.view(np.int32), L._distance_field(torch.sigmoid(x).numpy()).view(np.int32))
    assert np.array_equal(ft.view(np.int32), L._distance_field(t.numpy()).view(np.int32))
    if case == E.HDT_BWD_CASES[-1]:
        assert x.numel() > 2048 * 1024 and x.numel() % 4 == 1


def test_hdt_scale_bounds_the_gradient_terms():
    x, t, fp, ft = E.hdt_bwd_inputs(1, 5, 7)
    for alpha in E.HDT_ALPHAS:
        ref = R.hdt(x, t, alpha, fp, ft)
        s, td = torch.sigmoid(x.double()), t.double()
        want = ref.coef * 2 * (s - td) * s * (1 - s) / x.numel()
        assert torch.allclose(ref.grad, want, rtol=1e-12, atol=0) and bool((ref.grad.abs() <= ref.scale).all())
        assert torch.equal(ref.coef, torch.from_numpy(fp).double() ** alpha + torch.from_numpy(ft).double() ** alpha)
