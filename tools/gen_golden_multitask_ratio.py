#!/usr/bin/env python3
"""Generate tests/golden/trainer_multitask_ratio.npz by running the REFERENCE's own Trainer.multi_task_trainRatio
(Trainer.py:1174-1366) on the CPU: reference UNet_multitask(1, 1, 8), model type 'multi_task_reg', the data of
tools/gen_golden.py's `multitask_trainer_data` (32x32, 4 training images at batch 2, 2 validation images at batch 1), SGD at
0.01, 8 epochs, so the ratio gate switches on at epoch 6.

Runs (prefix in the file):
  none_    lr_scheduler=None;
  plateau_ lr_scheduler=ReduceLROnPlateau(patience=0): the reference steps it with val_score = 0.0 after every validation from
           epoch 6 on, so the LR is cut from epoch 7 on (the poly rule then overwrites it after the next step);
  stop_    lr_scheduler=None, lr 0.05 and patience 0: the validation loss rises, and the early-stop path is taken.

Per run: the per-epoch lists (_1 / _2 included), alpha of every epoch, iter_num, the final LR, best_val_score, the checkpoint
file names, whether the run stopped early and how it ended, and signatures of the weights at the point where the reference
stopped, one row per state_dict entry in the order of `keys`: `last` = the weights after the last step
(models/last_epoch.pt), `final` = the model's weights when the reference returned or raised (the best model after an early
stop -- it is loaded before the plot -- else the last-step weights, because the reference dies in plot_loss_functions before
it reloads the best model).

Usage:  python tools/gen_golden_multitask_ratio.py
"""
import os
import sys
import tempfile

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import recipe  # noqa: E402
from tools.gen_golden import GOLD, PairLabels, import_reference, meta, multitask_trainer_data, sig  # noqa: E402

EPOCHS = 8
RUNS = {"none": dict(lr=0.01, patience=25, sched=False), "plateau": dict(lr=0.01, patience=25, sched=True),
        "stop": dict(lr=0.05, patience=0, sched=False)}


def loaders():
    from torch.utils.data import DataLoader
    xs, l1, l2 = multitask_trainer_data()
    return {"train": DataLoader(PairLabels(xs[:4], l1[:4], l2[:4]), batch_size=2, shuffle=False),
            "val": DataLoader(PairLabels(xs[4:], l1[4:], l2[4:]), batch_size=1)}


def run(Model, Trainer, lr, patience, sched):
    class Recording(Trainer.Trainer):
        """Records every value the reference assigns to self.alpha (one per training phase)."""

        def __setattr__(self, k, v):
            if k == "alpha" and "alpha_list" in self.__dict__:
                self.alpha_list.append(float(v))
            object.__setattr__(self, k, v)

    torch.manual_seed(0)
    m = Model.UNet_multitask(1, 1, 8, False)
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=22))
    opt = torch.optim.SGD(m.parameters(), lr=lr, momentum=0.9, weight_decay=1e-4)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, patience=0) if sched else None
    with tempfile.TemporaryDirectory() as d:
        cwd = os.getcwd()
        os.chdir(d)
        tr = Recording(m, "multi_task_reg", torch.FloatTensor, "cpu", d, loaders(), 2, opt, patience, EPOCHS,
                       "multi_task_loss_ratio", "mse", lr_scheduler=scheduler)
        tr.alpha_list = []
        ending = "returned"
        try:
            tr.train()
        except ValueError as e:
            # plot_loss_functions (Trainer.py:69): val_score_list is never filled by this loop, so matplotlib gets x and y
            # of different lengths; everything recorded below was produced before that point
            if "same first dimension" not in str(e):
                raise
            ending = "plot ValueError"
        os.chdir(cwd)
        files = sorted(os.listdir(os.path.join(d, "models")))
        last = torch.load(os.path.join(d, "models", "last_epoch.pt"))
    out = dict(train_loss=np.array(tr.train_loss_list), val_loss=np.array(tr.val_loss_list),
               train_loss_1=np.array(tr.train_loss_list_1), train_loss_2=np.array(tr.train_loss_list_2),
               val_loss_1=np.array(tr.val_loss_list_1), val_loss_2=np.array(tr.val_loss_list_2),
               alpha=np.array(tr.alpha_list), iter_num=tr.iter_num, final_lr=opt.param_groups[0]["lr"], files=np.array(files),
               best_val_score=float(tr.best_val_score), early_stop=tr.early_stop_counter > tr.patience,
               ending=np.array(ending), lr=lr, patience=patience, scheduler=sched, epochs=EPOCHS)
    state = m.state_dict()
    out["keys"] = np.array(list(state))
    out["final"] = np.stack([sig(v.float()) for v in state.values()])
    out["last"] = np.stack([sig(last[k].float()) for k in state])
    return out


def main():
    Model, _, Trainer = import_reference()
    res = {}
    for name, cfg in RUNS.items():
        out = run(Model, Trainer, **cfg)
        print(name, "train", np.round(out["train_loss"], 4), "val", np.round(out["val_loss"], 4), "alpha",
              np.round(out["alpha"], 4), "files", list(out["files"]), "early_stop", out["early_stop"], out["ending"])
        res.update({f"{name}_{k}": v for k, v in out.items()})
    np.savez_compressed(os.path.join(GOLD, "trainer_multitask_ratio.npz"), runs=np.array(list(RUNS)), **res, **meta())
    print("wrote trainer_multitask_ratio.npz")


if __name__ == "__main__":
    main()
