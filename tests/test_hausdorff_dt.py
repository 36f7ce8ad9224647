"""HausdorffDTLoss on the CPU: the NumPy exact distance transform and the loss against the reference's own numbers
(tests/golden/hausdorff_dt.npz, written by tools/gen_golden_hdt.py from the reference's scipy fields)."""
import os

import numpy as np
import pytest
import torch


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "hausdorff_dt.npz"))
    return g, [str(c) for c in g["cases"]]


def test_fixture_covers_the_degenerate_cases(golden_dir):
    g, names = _golden(golden_dir)
    assert len(names) >= 10
    fg = lambda c: g[f"{c}_pred"] > 0                           # noqa: E731  (|logits| >= 1e-3 in the fixture)
    assert any(fg(c).reshape(len(fg(c)), -1).all(1).any() for c in names)          # an all-foreground prediction
    assert any((~fg(c)).reshape(len(fg(c)), -1).all(1).any() for c in names)       # an all-background prediction
    assert any((g[f"{c}_target"].reshape(len(g[f"{c}_target"]), -1) == 0).all(1).any() for c in names)


def test_numpy_fields_are_the_reference_fields_bit_for_bit(golden_dir):
    import loss as L
    g, names = _golden(golden_dir)
    for c in names:
        s = torch.sigmoid(torch.from_numpy(g[f"{c}_pred"])).numpy()
        for got, want in ((L._distance_field(s), g[f"{c}_pred_dt"]), (L._distance_field(g[f"{c}_target"]), g[f"{c}_target_dt"])):
            assert got.dtype == np.float32 and got.shape == want.shape, c
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (c, np.abs(got - want).max())


def test_all_foreground_field_measures_from_the_virtual_zero():
    import loss as L
    f = L._distance_field(np.ones((1, 1, 3, 4), np.float32))
    h, w = np.mgrid[0:3, 0:4]
    assert np.array_equal(f[0, 0], np.sqrt(1.0 + h ** 2 + w ** 2).astype(np.float32))
    assert not L._distance_field(np.zeros((1, 1, 3, 4), np.float32)).any()


def test_loss_and_gradient_match_the_reference(golden_dir):
    import loss as L
    g, names = _golden(golden_dir)
    for c in names:
        x = torch.from_numpy(g[f"{c}_pred"]).requires_grad_(True)
        t = torch.from_numpy(g[f"{c}_target"])
        loss = L.HausdorffDTLoss()(x, t)
        loss.backward()
        want = float(g[f"{c}_loss"])
        assert abs(loss.item() - want) <= 1e-6 * abs(want), (c, loss.item(), want)
        gw = g[f"{c}_grad"]
        assert np.abs(x.grad.numpy() - gw).max() <= 1e-5 * np.abs(gw).max(), c


def test_calc_loss_dispatches_hausdorff_dt(golden_dir):
    import loss as L
    g, _ = _golden(golden_dir)
    x, t = torch.from_numpy(g["odd_37x53_pred"]), torch.from_numpy(g["odd_37x53_target"])
    v = L.calc_loss(x, t, loss_type="HausdorffDTLoss")
    assert abs(v.item() - float(g["odd_37x53_loss"])) <= 1e-6 * float(g["odd_37x53_loss"])
    assert "HausdorffDTLoss" not in L._OUT_OF_SCOPE


def test_debug_tuple_has_the_reference_layout(golden_dir):
    import loss as L
    g, _ = _golden(golden_dir)
    x, t = torch.from_numpy(g["dense_48_pred"]), torch.from_numpy(g["dense_48_target"])
    loss, (dt_field, pred_error, distance, pred_dt, target_dt) = L.HausdorffDTLoss()(x, t, debug=True)
    assert abs(float(loss) - float(g["dense_48_loss"])) <= 1e-6 * float(g["dense_48_loss"])
    assert dt_field.shape == pred_error.shape == distance.shape == (48, 48)
    assert np.array_equal(pred_dt, g["dense_48_pred_dt"][0, 0]) and np.array_equal(target_dt, g["dense_48_target_dt"][0, 0])
    assert np.allclose(dt_field, pred_error * distance)


@pytest.mark.parametrize("shapes", [((2, 2, 8, 8), (2, 8, 8)), ((2, 1, 8, 8), (2, 8, 8)), ((2, 3, 8, 8), (2, 3, 8, 8)),
                                    ((1, 1, 4, 8, 8), (1, 1, 4, 8, 8)), ((2, 1, 8, 8), (2, 1, 8, 9)), ((8, 8), (8, 8))])
def test_out_of_domain_shapes_raise(shapes):
    import loss as L
    x, t = torch.zeros(shapes[0]), torch.zeros(shapes[1])
    with pytest.raises(NotImplementedError, match=r"\(B, 1, H, W\)"):
        L.calc_loss(x, t, loss_type="HausdorffDTLoss")
