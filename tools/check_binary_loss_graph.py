"""Child-process body of tests/test_gpu_binary_losses.py::test_trainer_graph_mode_replays_the_eager_losses.

For each of 'dice_bce', 'Tversky', 'TopK' and 'BCE_HEM': three Trainer steps of UNet(1, 1, 8, fp32) + umi.optim.SGD, once
eagerly and once with graph=True (step 1 eager, steps 2-3 replayed from the captured HIP graph): the per-step losses agree
bit for bit, the graph path and the device kernels were taken, and the first step's loss agrees with the CPU composite on
the same logits.
"""
import collections
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
LOSSES = {"dice_bce": "_DiceBCE", "Tversky": "_Tversky", "TopK": "_TopKBCE", "BCE_HEM": "_TopKBCE"}
CALLS = collections.Counter()


def count_device_forwards():
    """Route loss.py's device autograd Functions through subclasses that count their forwards."""
    for name in set(LOSSES.values()):
        base = getattr(L, name)

        def forward(ctx, *args, _base=base, _name=name):
            CALLS[_name] += 1
            return _base.forward(ctx, *args)
        setattr(L, name, type(name, (base,), {"forward": staticmethod(forward)}))


def run(loss_type, graph, x, y, state):
    m = Model.UNet(1, 1, 8, False, compute_dtype="fp32")
    m.load_state_dict(state)
    m.to(DEV)
    opt = uo.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    with tempfile.TemporaryDirectory() as td:
        tr = Trainer(m, "single", torch.cuda.FloatTensor, DEV, td, {"train": [], "val": []}, 2, opt, 25, 1,
                     loss_type, loss_type, graph=graph)
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
    y = (F.avg_pool2d(torch.randn(2, 1, 56, 56, generator=gen), 9, stride=1) > 0.1).float()[:, 0]

    m.load_state_dict(state)
    m.to(DEV).train()
    logits = m(x.to(DEV)).detach().float().cpu()
    count_device_forwards()
    for lt, fn in LOSSES.items():
        cpu_loss = L.calc_loss(logits, y, loss_type=lt).item()
        before = CALLS[fn]
        eager = run(lt, False, x, y, state)
        assert CALLS[fn] == before + 3, f"{lt}: the eager steps did not run the device kernels"
        graphed = run(lt, True, x, y, state)
        print(lt, "eager", [v.item() for v in eager], "graphed", [v.item() for v in graphed], "cpu step 1", cpu_loss)
        for a, b in zip(eager, graphed):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (lt, a.item(), b.item())
        assert abs(eager[0].item() - cpu_loss) <= 1e-5 * abs(cpu_loss), (lt, eager[0].item(), cpu_loss)
        assert eager[2].item() != eager[0].item(), f"{lt}: the steps did not train"
    print("BINARY_LOSS_GRAPH_OK")


if __name__ == "__main__":
    main()
