"""Child-process body of tests/test_gpu_unet.py::test_graphed_step_matches_eager_trajectory (the defaults) and of
tests/test_gpu_exact_fullsize.py::test_graphed_step_matches_eager_at_bench_scale (--features 64 --size 512 --batch 16).
usage: python tools/check_graphed_step.py [torch] [--features 8] [--size 64] [--batch 2]"""
import argparse, copy, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import torch
import Model
import loss as L
from umi.graphs import GraphedStep

ap = argparse.ArgumentParser()
ap.add_argument("opt", nargs="?", choices=["umi", "torch"], default="umi")
ap.add_argument("--features", type=int, default=8)
ap.add_argument("--size", type=int, default=64)
ap.add_argument("--batch", type=int, default=2)
a = ap.parse_args()
DEV = "cuda"
L.CLASS_NUMBER = 2
torch.manual_seed(21)
base = Model.UNet(1, 2, a.features, compute_dtype="fp16").to(DEV).train()
x = torch.randn(a.batch, 1, a.size, a.size, device=DEV)
lab = torch.randint(0, 2, (a.batch, a.size, a.size), device=DEV).float()


def make(model):
    # the fused optimizer (one launch per step; its descriptor table is uploaded from pinned memory, also under capture)
    # unless "torch" is passed on the command line
    from umi import optim as umi_optim
    cls = torch.optim.SGD if a.opt == "torch" else umi_optim.SGD
    opt = cls(model.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)

    def step(xx, yy):
        loss = L.calc_loss(model(xx), yy, loss_type="dice_bce_mc")
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss
    return step


m_g, m_e = copy.deepcopy(base), copy.deepcopy(base)
gs = GraphedStep(make(m_g), [x, lab], warmup=2)             # 2 warm-up steps have run on m_g (capturing executes nothing)
step_e = make(m_e)
for _ in range(2):
    le = step_e(x, lab)
for i in range(4):
    lg = gs(x, lab).clone()
    le = step_e(x, lab)
    assert torch.equal(lg, le.detach()), (i, float(lg), float(le))
for pg, pe in zip(m_g.parameters(), m_e.parameters()):
    assert torch.equal(pg, pe)
    assert torch.isfinite(pg).all()
assert torch.isfinite(lg).all()
print("GRAPHED_STEP_OK", float(lg))
