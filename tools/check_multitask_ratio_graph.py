"""Child-process body of tests/test_gpu_multitask_ratio.py::test_trainer_ratio_graph_mode_replays_the_eager_run.

The product Trainer's multi_task_trainRatio ('multi_task_reg', loss 'multi_task_loss_ratio') on UNet_multitask(1, 1, 8, fp32)
+ umi.optim.SGD over 7 epochs, 5 training images at batch 2 (a ragged last batch of 1), once eagerly and once with graph=True,
each without a scheduler and with a ReduceLROnPlateau object (its LR cut after the epoch-6 and epoch-7 validations reaches the
device LR block of the captured step).  Every per-step loss and the final weights agree bit for bit across the epoch-5 -> 6
switch of the gate (a device flag the captured kernel reads); the graph path took one capture per batch shape, and every step
ran the device kernels.
"""
import collections
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import torch  # noqa: E402
from torch.utils.data import DataLoader  # noqa: E402

import Model  # noqa: E402
import loss as L  # noqa: E402
from oracle import recipe  # noqa: E402
from tools.gen_golden import PairLabels, multitask_trainer_data  # noqa: E402
from Trainer import Trainer  # noqa: E402
from umi import optim as uo  # noqa: E402

DEV = "cuda"
EPOCHS = 7
CALLS = collections.Counter()


def count_device_forwards():
    base = L._MultiTaskRatio

    def forward(ctx, *args):
        CALLS["fwd"] += 1
        return base.forward(ctx, *args)
    L._MultiTaskRatio = type("_MultiTaskRatio", (base,), {"forward": staticmethod(forward)})


class Recording(Trainer):
    def train_step(self, inputs, labels):
        loss = super().train_step(inputs, labels)
        self.step_losses.append(torch.stack([loss] + [t.detach() for t in self._task_losses] + [self._ratio.detach()]))
        return loss


def run(graph, scheduler):
    torch.manual_seed(0)
    m = Model.UNet_multitask(1, 1, 8, False, compute_dtype="fp32")
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=22))
    m.to(DEV)
    xs, l1, l2 = multitask_trainer_data()
    loaders = {"train": DataLoader(PairLabels(xs[:5], l1[:5], l2[:5]), batch_size=2, shuffle=False),    # batches 2, 2, 1
               "val": DataLoader(PairLabels(xs[5:], l1[5:], l2[5:]), batch_size=1)}
    opt = uo.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, patience=0) if scheduler else None
    with tempfile.TemporaryDirectory() as td:
        tr = Recording(m, "multi_task_reg", torch.cuda.FloatTensor, DEV, td, loaders, 2, opt, 25, EPOCHS,
                       "multi_task_loss_ratio", "mse", lr_scheduler=sched, graph=graph)
        tr.step_losses = []
        before = CALLS["fwd"]
        tr.train()
        # eager: 3 training steps and 1 validation step per epoch.  graph: a replay runs no Python, so the Function's forward
        # runs for the validation steps, the first eager step and the capture of each batch shape (epochs 1 and 2) only
        want = EPOCHS * 4 if not graph else EPOCHS + 4
        assert CALLS["fwd"] - before == want, ("the device kernels were not taken", CALLS["fwd"] - before, want)
    if graph:
        assert len(tr._graphs) == 2, ("expected one graph per batch shape (full, ragged)", list(tr._graphs))
        opt.sync_host()
    losses = torch.stack(tr.step_losses).cpu()
    w = torch.cat([p.detach().flatten() for p in m.parameters()]).cpu()
    return dict(losses=losses, w=w, lr=opt.param_groups[0]["lr"], it=tr.iter_num, train=list(tr.train_loss_list),
                val=list(tr.val_loss_list), alpha=list(tr.alpha_list))


def main():
    count_device_forwards()
    for scheduler in (False, True):
        a, b = run(False, scheduler), run(True, scheduler)
        print("scheduler", scheduler, "train", a["train"], "val", a["val"], "alpha", a["alpha"], "lr", a["lr"], b["lr"])
        assert a["losses"].shape == (EPOCHS * 3, 4), a["losses"].shape
        diff = (a["losses"] - b["losses"]).abs().max().item()
        assert torch.equal(a["losses"].view(torch.int32), b["losses"].view(torch.int32)), ("per-step losses differ", diff)
        assert torch.equal(a["w"].view(torch.int32), b["w"].view(torch.int32)), \
            ("final weights differ", (a["w"] - b["w"]).abs().max().item())
        # the LR is a double: the host's and the device's pow() of the poly rule may differ in the last bit (the fp32 LR the
        # update kernel reads, and so every weight, is identical -- checked above)
        assert a["it"] == b["it"] == EPOCHS * 3 and abs(a["lr"] - b["lr"]) <= 1e-12 * a["lr"], (a["it"], b["it"], a["lr"], b["lr"])
        assert a["train"][5] > 2 * a["train"][4], a["train"]                   # the gate switched on at epoch 6
        assert len(a["val"]) == EPOCHS - 5
        if scheduler:
            assert a["lr"] < 1e-3, a["lr"]                                      # the plateau cut after epoch 7's validation
    print("MT_RATIO_GRAPH_OK")


if __name__ == "__main__":
    main()
