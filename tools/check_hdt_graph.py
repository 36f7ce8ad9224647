"""Child-process body of tests/test_gpu_hausdorff_dt.py::test_trainer_graph_mode_replays_the_eager_losses.

Three Trainer steps of UNet(1, 1, 8, fp32) + umi.optim.SGD with loss 'HausdorffDTLoss', once eagerly and once with
graph=True (step 1 eager, steps 2-3 replayed from the captured HIP graph): the per-step losses agree bit for bit, and the
first step's loss equals the CPU path's loss on the same logits.
"""
import os
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import Model  # noqa: E402
import loss as L  # noqa: E402
from oracle import recipe  # noqa: E402
from Trainer import Trainer  # noqa: E402
from umi import optim as uo  # noqa: E402

DEV = "cuda"


def run(graph, x, y, state):
    m = Model.UNet(1, 1, 8, False, compute_dtype="fp32")
    m.load_state_dict(state)
    m.to(DEV)
    opt = uo.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    with tempfile.TemporaryDirectory() as td:
        tr = Trainer(m, "single", torch.cuda.FloatTensor, DEV, td, {"train": [], "val": []}, 2, opt, 25, 1,
                     "HausdorffDTLoss", "HausdorffDTLoss", graph=graph)
        losses = [tr.train_step(x, y) for _ in range(3)]
    torch.cuda.synchronize()
    if graph:
        assert len(tr._graphs) == 1, "the graph path was not taken"
    return [v.cpu() for v in losses]


def main():
    torch.manual_seed(0)
    m = Model.UNet(1, 1, 8, False, compute_dtype="fp32")
    state = recipe.fill_state_dict(m.state_dict(), seed=31)
    gen = torch.Generator().manual_seed(31)
    x = torch.randn(2, 1, 48, 48, generator=gen)
    y = (F.avg_pool2d(torch.randn(2, 1, 56, 56, generator=gen), 9, stride=1) > 0.1).float()

    # the first step's logits: the same model state in train mode, on the same input, through the training forward
    m.load_state_dict(state)
    m.to(DEV).train()
    logits = m(x.to(DEV)).detach().float().cpu()
    cpu_loss = L.HausdorffDTLoss()(logits, y).item()

    eager = run(False, x, y, state)
    graphed = run(True, x, y, state)
    print("eager", [v.item() for v in eager], "graphed", [v.item() for v in graphed], "cpu step 1", cpu_loss)
    for a, b in zip(eager, graphed):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (a.item(), b.item())
    assert abs(eager[0].item() - cpu_loss) <= 1e-6 * cpu_loss, (eager[0].item(), cpu_loss)
    assert eager[2].item() != eager[0].item(), "the steps did not train"
    print("HDT_GRAPH_OK")


if __name__ == "__main__":
    main()
