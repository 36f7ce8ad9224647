"""Child-process body of tests/test_gpu_attn_dropout.py::test_graph_capture_follows_eager_and_draws_fresh_masks: a TransUNet with
attention-probability dropout captured in a HIP graph.
  1. GraphedStep (forward + loss + backward + optimizer step) over 3 replays equals the eager run bit for bit: every loss and
     every weight.  Both models share the host seed and start from the same device counter, so replay i and eager step i draw the
     same masks -- the attention kernels read the tape's snapshot of the counter, which the captured copy refreshes each replay.
  2. A captured forward + backward WITHOUT an optimizer, replayed twice on the same input with the same weights, gives different
     logits: the masks are fresh.
Run for the small fixture config in fp32 (head dimension 16: the VALU kernels) and for the head-dimension-64 miniature in fp16 (the
matrix-core kernels).
usage: python tools/check_attn_dropout_graph.py"""
import copy, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import torch
import loss as L
from oracle import ref_transunet
from TransUnet.vit_seg_configs import ConfigDict
from TransUnet.vit_seg_modeling import VisionTransformer
from umi import optim as umi_optim
from umi.graphs import GraphedStep

DEV = "cuda"
L.CLASS_NUMBER = 2
IMG, RATE = 64, 0.1


def config(**over):
    cfg = dict(ref_transunet.small_config(2), attention_dropout_rate=RATE, dropout_rate=0.1, **over)
    g = IMG // 16
    return ConfigDict(patches={"size": (16, 16), "grid": (g, g)}, hidden_size=cfg["hidden_size"],
                      transformer=dict(mlp_dim=cfg["mlp_dim"], num_heads=cfg["num_heads"], num_layers=cfg["num_layers"],
                                       attention_dropout_rate=cfg["attention_dropout_rate"], dropout_rate=cfg["dropout_rate"]),
                      classifier="seg", representation_size=None, decoder_channels=tuple(cfg["decoder_channels"]),
                      n_classes=cfg["n_classes"], activation="softmax",
                      resnet=dict(num_layers=tuple(cfg["resnet_layers"]), width_factor=cfg["width_factor"]),
                      skip_channels=list(cfg["skip_channels"]), n_skip=cfg["n_skip"])


def train_step(model):
    opt = umi_optim.SGD(model.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4)

    def step(xx, yy):
        loss = L.calc_loss(model(xx), yy, loss_type="dice_bce_mc")
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss
    return step


def grad_step(model):
    def step(xx, yy):
        logits = model(xx)
        model.zero_grad(set_to_none=True)
        L.calc_loss(logits, yy, loss_type="dice_bce_mc").backward()
        return logits.detach()
    return step


for mode, over in (("fp32", {}), ("fp16", dict(hidden_size=128, num_heads=2, mlp_dim=256))):
    torch.manual_seed(31)
    base = VisionTransformer(config(**over), img_size=IMG, num_classes=2, compute_dtype=mode).to(DEV).train()
    x = torch.randn(2, 1, IMG, IMG, device=DEV)
    lab = torch.randint(0, 2, (2, IMG, IMG), device=DEV).float()
    with torch.no_grad():
        base(x)                                  # the first training forward draws the host seed and creates the device counter
    assert base._drop_base is not None and int(base._drop_step.item()) == 1

    # 1. the whole step: graph == eager, bit for bit
    m_g, m_e = copy.deepcopy(base), copy.deepcopy(base)
    assert m_g._drop_base == m_e._drop_base and m_g._drop_step.data_ptr() != m_e._drop_step.data_ptr()
    gs = GraphedStep(train_step(m_g), [x, lab], warmup=2)   # 2 warm-up steps have run on m_g (capturing executes nothing)
    step_e = train_step(m_e)
    for _ in range(2):
        step_e(x, lab)
    losses = []
    for i in range(3):
        lg = gs(x, lab).clone()
        le = step_e(x, lab).detach()
        assert torch.equal(lg, le), (mode, i, float(lg), float(le))
        losses.append(float(lg))
    del le
    assert int(m_g._drop_step.item()) == int(m_e._drop_step.item()) == 6
    for pg, pe in zip(m_g.parameters(), m_e.parameters()):
        assert torch.equal(pg, pe) and torch.isfinite(pg).all()
    assert len(set(losses)) == 3, losses

    # 2. fresh masks on every replay: same input, same weights, different logits; and the first replay is the eager forward
    m_f, m_r = copy.deepcopy(base), copy.deepcopy(base)
    gf = GraphedStep(grad_step(m_f), [x, lab], warmup=1)
    grad_step(m_r)(x, lab)
    first = gf(x, lab).clone()
    second = gf(x, lab).clone()
    assert torch.equal(first, grad_step(m_r)(x, lab)), mode
    assert torch.isfinite(first).all() and torch.isfinite(second).all() and not torch.equal(first, second), mode
    for pf, pb in zip(m_f.parameters(), base.parameters()):
        assert torch.equal(pf, pb)                            # nothing updated the weights: only the masks changed
    print(mode, "losses", losses)
print("ATTN_DROPOUT_GRAPH_OK")
