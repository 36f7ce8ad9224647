"""CPU tests of batched validation: Trainer(val_batch=k) driving the CPU oracle models against the item-by-item loop of the
same run, and loss.calc_loss_items against the loop over calc_loss.

Bar: atol 5e-6 on the epoch figures, the project's bar for Trainer losses (tests/test_host_logic.py).  On the CPU a batch-1
forward and the slice of a batched forward differ by rounding only (measured for RefUNet(1, 2, 8) at 32x32: 6.0e-8 per item,
6.8e-8 on the epoch mean)."""
import os
import re

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from oracle import recipe, ref_unet

ATOL = 5e-6
PICK = lambda s: re.findall(r"(Epoch \d+/\d+|LR [0-9.e-]+|saving best model|Early stopping)", s)


class _Items(torch.utils.data.Dataset):
    """A list of ready (inputs, labels) loader items (so that items may differ in size)."""

    def __init__(self, items):
        self.items = items

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def _loader(items):
    return DataLoader(_Items(items), batch_size=None, shuffle=False)


def _single_data(n_val=7, per_item=1, odd_at=None, classes=2, float_labels=False):
    """4 training images in batches of 2 and n_val validation items of per_item images at 32x32 (item `odd_at`: 48x32)."""
    xs, ls = recipe.synthetic_batch(4 + n_val * per_item, 1, 32, 32, classes, seed=21)
    if float_labels:
        ls = ls.float()
    val = []
    for i in range(n_val):
        a = 4 + i * per_item
        x, l = xs[a:a + per_item], ls[a:a + per_item]
        if i == odd_at:
            x, l = torch.cat([x, x[:, :, :16]], dim=2), torch.cat([l, l[:, :16]], dim=1)
        val.append((x, l))
    return {"train": DataLoader(TensorDataset(xs[:4], ls[:4]), batch_size=2, shuffle=False), "val": _loader(val)}


def _run(tmp, loaders, val_batch, model_type="single", loss="dice_bce_mc", metric=None, model=None, epochs=3):
    import loss as L
    from Trainer import Trainer
    torch.manual_seed(0)
    L.CLASS_NUMBER = 2
    m = model() if model else ref_unet.RefUNet(1, 2, 8, False)
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=21))
    opt = torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    os.makedirs(tmp, exist_ok=True)
    tr = Trainer(m, model_type, torch.FloatTensor, "cpu", str(tmp), loaders, 2, opt, 25, epochs, loss, metric or loss,
                 lr_scheduler=True, val_batch=val_batch)
    tr.train()
    return tr


def _same_run(a, b, da, db, per_task=False):
    assert len(a.val_loss_list) == len(b.val_loss_list) == 3
    np.testing.assert_allclose(a.val_loss_list, b.val_loss_list, rtol=0, atol=ATOL)
    np.testing.assert_allclose(a.val_score_list, b.val_score_list, rtol=0, atol=ATOL)
    np.testing.assert_allclose(a.train_loss_list, b.train_loss_list, rtol=0, atol=0)      # training is untouched
    if per_task:
        assert len(a.val_loss_list_1) == len(a.val_loss_list_2) == 3
        np.testing.assert_allclose(a.val_loss_list_1, b.val_loss_list_1, rtol=0, atol=ATOL)
        np.testing.assert_allclose(a.val_loss_list_2, b.val_loss_list_2, rtol=0, atol=ATOL)
    assert abs(a.best_val_score - b.best_val_score) <= ATOL and abs(a.best_loss - b.best_loss) <= ATOL
    assert sorted(os.listdir(os.path.join(da, "models"))) == sorted(os.listdir(os.path.join(db, "models")))
    la, lb = (open(os.path.join(d, "logs.txt")).read() for d in (da, db))
    assert PICK(la) == PICK(lb) and "saving best model" in la
    for x, y in zip(a.best_model.values(), b.best_model.values()):
        assert torch.equal(x, y)                                                          # the same best epoch's weights


def _groups(monkeypatch):
    """Spy on Validation.run_group: the sizes of the groups the validation phases formed."""
    from umi.val_batch import Validation
    sizes, orig = [], Validation.run_group

    def spy(self, group):
        sizes.append(len(group))
        return orig(self, group)
    monkeypatch.setattr(Validation, "run_group", spy)
    return sizes


def test_groups_of_3_3_1_match_the_item_loop(tmp_path, monkeypatch):
    sizes = _groups(monkeypatch)
    a = _run(tmp_path / "a", _single_data(), 3)
    assert sizes == [3, 3, 1] * 3
    b = _run(tmp_path / "b", _single_data(), None)
    assert sizes == [3, 3, 1] * 3                     # val_batch=None never comes here
    _same_run(a, b, tmp_path / "a", tmp_path / "b")
    assert a._graphs == {} and a._validation().graphs == {}   # no device, no graphs


def test_items_of_two_images(tmp_path, monkeypatch):
    sizes = _groups(monkeypatch)
    a = _run(tmp_path / "a", _single_data(n_val=5, per_item=2), 2)
    assert sizes == [2, 2, 1] * 3
    b = _run(tmp_path / "b", _single_data(n_val=5, per_item=2), None)
    _same_run(a, b, tmp_path / "a", tmp_path / "b")


def test_shape_change_closes_the_group(tmp_path, monkeypatch):
    sizes = _groups(monkeypatch)
    a = _run(tmp_path / "a", _single_data(odd_at=3), 3)
    assert sizes == [3, 1, 3] * 3                     # items 0-2 | item 3 (48x32) | items 4-6
    b = _run(tmp_path / "b", _single_data(odd_at=3), None)
    _same_run(a, b, tmp_path / "a", tmp_path / "b")


def test_k_1_and_k_larger_than_the_loader(tmp_path):
    b = _run(tmp_path / "b", _single_data(), None)
    for k in (1, 16):
        a = _run(tmp_path / f"a{k}", _single_data(), k)
        _same_run(a, b, tmp_path / f"a{k}", tmp_path / "b")


def test_multi_task(tmp_path):
    from tools.gen_golden import PairLabels, multitask_trainer_data

    def data():
        xs, l1, l2 = multitask_trainer_data()
        xs, l1, l2 = (torch.cat([t, t.flip(1), t.flip(2)])[:11] for t in (xs, l1, l2))
        val = [(xs[i:i + 1], (l1[i:i + 1], l2[i:i + 1])) for i in range(4, 11)]
        return {"train": DataLoader(PairLabels(xs[:4], l1[:4], l2[:4]), batch_size=2, shuffle=False), "val": _loader(val)}
    mk = lambda: ref_unet.RefUNetMultitask(1, 1, 8, False)
    a = _run(tmp_path / "a", data(), 3, model_type="multi_task", loss="mse", model=mk)
    b = _run(tmp_path / "b", data(), None, model_type="multi_task", loss="mse", model=mk)
    _same_run(a, b, tmp_path / "a", tmp_path / "b", per_task=True)
    assert a.val_score_list == [0.0] * 3


def test_regression(tmp_path):
    mk = lambda: ref_unet.RefUNet(1, 1, 8, False)
    a = _run(tmp_path / "a", _single_data(float_labels=True), 3, model_type="regression", loss="mse", model=mk)
    b = _run(tmp_path / "b", _single_data(float_labels=True), None, model_type="regression", loss="mse", model=mk)
    _same_run(a, b, tmp_path / "a", tmp_path / "b")


def test_loss_and_metric_differ(tmp_path):
    a = _run(tmp_path / "a", _single_data(), 3, loss="dice_bce_mc", metric="CE")
    b = _run(tmp_path / "b", _single_data(), None, loss="dice_bce_mc", metric="CE")
    _same_run(a, b, tmp_path / "a", tmp_path / "b")
    assert a.val_loss_list != a.val_score_list


# ---- calc_loss_items ----------------------------------------------------------------------------------------------------------

def _loss_inputs(name, B=6, H=24, W=40):
    g = torch.Generator().manual_seed(7)
    if name in ("dice_bce_mc", "CE", "Tversky"):
        return torch.randn(B, 2, H, W, generator=g), torch.randint(0, 2, (B, H, W), generator=g).float()
    if name == "mseMC":
        return torch.randn(B, 2, H, W, generator=g), torch.randn(B, 2, H, W, generator=g)
    if name in ("rmse", "l1loss", "HausdorffDTLoss"):
        return torch.randn(B, 1, H, W, generator=g), torch.randint(0, 2, (B, 1, H, W), generator=g).float()
    return torch.randn(B, 1, H, W, generator=g), torch.randint(0, 2, (B, H, W), generator=g).float()


SUPPORTED = ["dice_bce_mc", "CE", "BCE", "mse", "mseMC", "rmse", "l1loss", "HausdorffDTLoss", "dice_bce", "Tversky", "TopK",
             "BCE_HEM"]


@pytest.mark.parametrize("name", SUPPORTED)
def test_calc_loss_items_is_the_loop(name):
    import loss as L
    L.CLASS_NUMBER = 2
    pred, target = _loss_inputs(name)
    for items in (1, 2, 3, 6):
        n = 6 // items
        got = L.calc_loss_items(pred, target, items, loss_type=name)
        want = torch.stack([L.calc_loss(pred[i * n:(i + 1) * n], target[i * n:(i + 1) * n], loss_type=name) for i in range(items)])
        assert got.shape == (items,) and torch.equal(got, want), (name, items)


def test_calc_loss_items_raises_where_calc_loss_raises():
    import loss as L
    from umi import ddp
    L.CLASS_NUMBER = 2
    pred, target = _loss_inputs("dice_bce_mc")
    for name in sorted(L._OUT_OF_SCOPE):
        with pytest.raises(NotImplementedError):
            L.calc_loss_items(pred, target, 3, loss_type=name)
    with pytest.raises(ValueError):
        L.calc_loss_items(pred, target, 3, loss_type="nope")
    for items in (0, 4, -1):                                    # 6 images do not split into 4 groups
        with pytest.raises(ValueError):
            L.calc_loss_items(pred, target, items, loss_type="CE")
    with pytest.raises(ValueError):
        L.calc_loss_items(pred, target[:5], 3, loss_type="CE")
    ddp.set_active_batch_sync(object())                         # any active switch: refused before it is used
    try:
        with pytest.raises(NotImplementedError):
            L.calc_loss_items(pred, target, 3, loss_type="dice_bce_mc")
        with pytest.raises(NotImplementedError):
            L.calc_loss_items(pred, target, 3, loss_type="mse")
    finally:
        ddp.set_active_batch_sync(None)


# ---- refusals -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", [0, -2, 2.0, "3", True, (3,)])
def test_bad_val_batch(tmp_path, bad):
    from Trainer import Trainer
    m = torch.nn.Linear(1, 1)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    with pytest.raises(ValueError, match="val_batch"):
        Trainer(m, "single", torch.FloatTensor, "cpu", str(tmp_path), {"train": [0], "val": [0]}, 1, opt, 1, 1, "mse", "mse",
                val_batch=bad)


def test_ratio_loop_refuses_val_batch(tmp_path):
    from Trainer import Trainer

    class Never:
        def __len__(self):
            return 1

        def __iter__(self):
            raise AssertionError("the refusal comes before the first step")
    m = torch.nn.Linear(1, 1)
    opt = torch.optim.SGD(m.parameters(), lr=0.1)
    tr = Trainer(m, "multi_task", torch.FloatTensor, "cpu", str(tmp_path), {"train": Never(), "val": Never()}, 1, opt, 1, 1,
                 "multi_task_loss_ratio", "multi_task_loss_ratio", val_batch=2)
    with pytest.raises(NotImplementedError, match="val_batch"):
        tr.train()
    Trainer(m, "multi_task", torch.FloatTensor, "cpu", str(tmp_path), {"train": Never(), "val": Never()}, 1, opt, 1, 1,
            "multi_task_loss_ratio", "multi_task_loss_ratio", val_batch=None)          # today's constructor still takes it
