"""'dice_bce', 'Tversky', 'TopK' and 'BCE_HEM' on the CPU: the torch composites of loss.py against the reference's own
numbers (tests/golden/binary_losses.npz, written by tools/gen_golden_binary_losses.py from the reference's calc_loss)."""
import os

import numpy as np
import pytest
import torch


def _golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "binary_losses.npz"))
    return g, [str(e) for e in g["entries"]]


def test_fixture_covers_the_edge_cases(golden_dir):
    g, entries = _golden(golden_dir)
    cases = {e.split(":")[0] for e in entries}
    n = {c: g[f"{c}_pred"].size for c in cases}
    binary = [c for c in cases if g[f"{c}_pred"].shape[1] == 1]
    assert {"dice_bce", "Tversky", "TopK", "BCE_HEM"} <= {e.split(":")[1] for e in entries}
    assert {g[f"{c}_pred"].shape[0] for c in binary} >= {1, 2, 3}
    assert any(n[c] % 2 for c in binary if f"{c}:TopK" in entries)                     # TopK's floor
    assert any(not g[f"{c}_target"].any() for c in binary)                             # all-zero targets
    assert any((g[f"{c}_target"] == 1).all() for c in binary)                          # all-one targets
    soft = [c for c in binary if ((g[f"{c}_target"] > 0) & (g[f"{c}_target"] < 1)).any()]
    assert any(f"{c}:{lt}" in entries for c in soft for lt in ("dice_bce", "BCE_HEM", "TopK"))
    assert any((np.abs(g[f"{c}_pred"]) > 30).any() for c in binary)                    # saturated logits
    assert any((np.abs(g[f"{c}_pred"]) < 0.05).mean() > 0.5 for c in binary)           # logits near 0
    assert {g[f"{c}_pred"].shape[1] for c in cases if f"{c}:Tversky" in entries} >= {1, 3, 5}
    assert any(n[c] == 500 for c in binary if f"{c}:BCE_HEM" in entries)               # BCE_HEM takes every pixel


@pytest.mark.parametrize("loss_type", ["dice_bce", "Tversky", "TopK", "BCE_HEM"])
def test_composite_matches_the_reference(golden_dir, loss_type):
    import loss as L
    g, entries = _golden(golden_dir)
    mine = [e for e in entries if e.endswith(":" + loss_type)]
    assert mine
    for e in mine:
        c = e.split(":")[0]
        x = torch.from_numpy(g[f"{c}_pred"]).requires_grad_(True)
        t = torch.from_numpy(g[f"{c}_target"])
        v = L.calc_loss(x, t, loss_type=loss_type)
        v.backward()
        want = float(g[f"{e}_loss"])
        assert abs(v.item() - want) <= 2e-6 * abs(want), (e, v.item(), want)
        gw = g[f"{e}_grad"]
        assert np.abs(x.grad.numpy() - gw).max() <= 1e-5 * np.abs(gw).max(), e


def test_selection_gradients_are_nonzero_exactly_on_k_pixels(golden_dir):
    g, entries = _golden(golden_dir)
    for e in entries:
        c, lt = e.split(":")
        if lt in ("TopK", "BCE_HEM"):
            k = g[f"{c}_pred"].size // 2 if lt == "TopK" else 500
            assert np.count_nonzero(g[f"{e}_grad"]) <= k, e


def test_bce_hem_below_500_pixels_raises_as_the_reference():
    import loss as L
    with pytest.raises(RuntimeError):
        L.calc_loss(torch.zeros(1, 1, 9, 13), torch.zeros(1, 9, 13), loss_type="BCE_HEM")


def test_dice_bce_target_shape_is_checked_as_the_reference():
    import loss as L
    with pytest.raises(ValueError):
        L.calc_loss(torch.zeros(2, 1, 8, 8), torch.zeros(2, 1, 8, 8), loss_type="dice_bce")


@pytest.mark.parametrize("loss_type", ["HausdorffERLoss", "FL", "dice", "ActiveContourLoss", "dice_score", "dice_score_mc",
                                       "log_cosh_dice_loss"])
def test_broken_reference_losses_still_raise(loss_type):
    import loss as L
    with pytest.raises(NotImplementedError):
        L.calc_loss(torch.zeros(2, 1, 8, 8), torch.zeros(2, 8, 8), loss_type=loss_type)


def test_the_four_losses_left_the_out_of_scope_set():
    import loss as L
    assert not {"dice_bce", "Tversky", "TopK", "BCE_HEM"} & L._OUT_OF_SCOPE
