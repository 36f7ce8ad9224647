"""CPU tests of the warm-up + decay learning-rate rule and of what goes with umi.optim.AdamW on the host: `schedule_lr` against
torch's LambdaLR, the refusals of `device_schedule(schedule=...)` and `Trainer(lr_schedule=...)`, `decay_groups`, the Trainer's
host path with a torch optimizer against a hand-written loop, and the layout of the device hyper block."""
import ctypes
import math
import os

import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

from oracle import recipe, ref_unet

KINDS = ("cosine", "poly", "constant")


def _factor(kind, warmup, mx, power, final_ratio):
    """The rule as include/unetmi.h states it, written out for LambdaLR (which multiplies the group's initial LR by it)."""
    def f(k):
        w = min(1.0, (k + 1) / warmup) if warmup > 0 else 1.0
        x = min(k, mx) / mx
        s = {"poly": lambda: (1.0 - x) ** power, "cosine": lambda: 0.5 * (1.0 + math.cos(math.pi * x)),
             "constant": lambda: 1.0}[kind]()
        return w * (final_ratio + (1.0 - final_ratio) * s)
    return f


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("warmup", [0, 1, 5])
@pytest.mark.parametrize("mx", [1, 20])
@pytest.mark.parametrize("final_ratio", [0.0, 0.01])
def test_schedule_lr_equals_lambda_lr(kind, warmup, mx, final_ratio):
    from umi.optim import schedule_lr
    base = [3e-4, 1e-3]
    p = [torch.nn.Parameter(torch.zeros(2)) for _ in base]
    opt = torch.optim.AdamW([dict(params=[q], lr=b) for q, b in zip(p, base)], weight_decay=0.01)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, _factor(kind, warmup, mx, 0.9, final_ratio))
    for k in range(mx + 3):                                            # 0 .. max + 2: past the end
        for group, b in zip(opt.param_groups, base):
            mine = schedule_lr(k, b, kind, mx, warmup=warmup, power=0.9, final_ratio=final_ratio)
            assert isinstance(mine, float) and mine == group["lr"], (k, mine, group["lr"])
        opt.step()
        sched.step()
    # the ends of the rule, as numbers
    assert abs(schedule_lr(0, 1.0, kind, mx, warmup, 0.9, final_ratio) - (1.0 / warmup if warmup > 1 else 1.0)) < 1e-15
    if kind != "constant":
        assert schedule_lr(mx + 2, 1.0, kind, mx, 0, 0.9, final_ratio) == schedule_lr(mx, 1.0, kind, mx, 0, 0.9, final_ratio)
        assert abs(schedule_lr(mx, 1.0, kind, mx, 0, 0.9, final_ratio) - final_ratio) < 1e-16


def test_schedule_lr_refuses_an_unknown_kind():
    from umi.optim import schedule_lr
    with pytest.raises(ValueError, match="kind"):
        schedule_lr(0, 1.0, "linear", 10)


# ---- refusals -----------------------------------------------------------------------------------------------------------------

BAD = [dict(kind="linear", max_iterations=10), dict(max_iterations=10), dict(kind="cosine", max_iterations=10, warmup=-1),
       dict(kind="cosine", max_iterations=10, final_ratio=1.5), dict(kind="cosine", max_iterations=10, final_ratio=-0.1),
       dict(kind="poly", max_iterations=10, power=0.0), dict(kind="poly", max_iterations=10, power=-1.0),
       dict(kind="cosine", max_iterations=0), dict(kind="cosine", max_iterations=-3)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_device_schedule_refuses_bad_schedules(bad):
    from umi import optim as uo
    for cls in (uo.AdamW, uo.Adam, uo.SGD):
        opt = cls([torch.nn.Parameter(torch.zeros(3))], lr=1e-3)
        with pytest.raises(ValueError, match=r"device_schedule\(schedule="):
            opt.device_schedule(schedule=bad)
        assert opt.device_hyper is None


def test_device_schedule_refuses_a_missing_max_iterations_and_poly_with_schedule():
    from umi import optim as uo
    opt = uo.AdamW([torch.nn.Parameter(torch.zeros(3))], lr=1e-3)
    with pytest.raises(ValueError, match="max_iterations"):
        opt.device_schedule(schedule=dict(kind="cosine"))
    with pytest.raises(ValueError, match="not both"):
        opt.device_schedule(poly=dict(base_lr=1e-3, max_iterations=10), schedule=dict(kind="cosine", max_iterations=10))
    assert opt.device_hyper is None


def _tiny_trainer(tmp_path, **kw):
    from Trainer import Trainer
    m = torch.nn.Linear(1, 1)
    opt = torch.optim.AdamW(m.parameters(), lr=0.1)
    return Trainer(m, "single", torch.FloatTensor, "cpu", str(tmp_path), {"train": [0, 1], "val": [0]}, 1, opt, 1, 3, "mse", "mse",
                   **kw)


@pytest.mark.parametrize("bad", BAD + [dict(warmup=3), dict(kind="cosine", iter_num=2), dict(kind="cosine", decay=0.1), "cosine",
                                       True], ids=repr)
def test_trainer_refuses_bad_schedules(tmp_path, bad):
    with pytest.raises(ValueError, match="lr_schedule"):
        _tiny_trainer(tmp_path, lr_schedule=bad)


def test_trainer_refuses_lr_schedule_with_lr_scheduler_and_fills_max_iterations(tmp_path):
    with pytest.raises(ValueError, match="lr_scheduler"):
        _tiny_trainer(tmp_path, lr_schedule=dict(kind="cosine", warmup=3), lr_scheduler=True)
    tr = _tiny_trainer(tmp_path, lr_schedule=dict(kind="cosine", warmup=3), lr_scheduler=None)
    assert tr._lr_schedule == dict(kind="cosine", max_iterations=6, warmup=3, power=0.9, final_ratio=0.0)   # 3 epochs x 2 batches
    assert _tiny_trainer(tmp_path, lr_schedule=dict(kind="poly", max_iterations=40))._lr_schedule["max_iterations"] == 40
    assert _tiny_trainer(tmp_path)._lr_schedule is None


# ---- decay_groups -------------------------------------------------------------------------------------------------------------

def _models():
    import Model
    from oracle import ref_transunet
    from tests.test_gpu_transunet import product_config
    from TransUnet.vit_seg_modeling import VisionTransformer
    yield "unet", Model.UNet(1, 2, 8)
    yield "transunet", VisionTransformer(product_config(ref_transunet.small_config(2), 64), img_size=64, num_classes=2)


def test_decay_groups_split_every_trainable_parameter_once():
    from umi.optim import decay_groups
    for name, model in _models():
        frozen = next(p for p in model.parameters() if p.ndim == 4)   # a convolution weight
        frozen.requires_grad_(False)                                  # not trainable: in neither group
        groups = decay_groups(model, 0.05)
        assert [g["weight_decay"] for g in groups] == [0.05, 0.0] and len(groups) == 2
        decayed, rest = ({id(p) for p in g["params"]} for g in groups)
        assert len(decayed) == len(groups[0]["params"]) and len(rest) == len(groups[1]["params"])
        assert not decayed & rest
        assert decayed | rest == {id(p) for p in model.parameters() if p.requires_grad}
        assert id(frozen) not in decayed | rest
        names = {id(p): n for n, p in model.named_parameters()}
        assert all(p.ndim > 1 and not names[id(p)].endswith("position_embeddings") for p in groups[0]["params"]), name
        for mod_name, mod in model.named_modules():
            if isinstance(mod, (torch.nn.Conv2d, torch.nn.ConvTranspose2d, torch.nn.Linear)) and mod.weight.requires_grad:
                assert id(mod.weight) in decayed, (name, mod_name)
                assert mod.bias is None or id(mod.bias) in rest, (name, mod_name)
            if isinstance(mod, (torch.nn.BatchNorm2d, torch.nn.GroupNorm, torch.nn.LayerNorm)) and mod.weight is not None:
                assert id(mod.weight) in rest and id(mod.bias) in rest, (name, mod_name)
        if name == "transunet":
            pos = [p for n, p in model.named_parameters() if n.endswith("position_embeddings")]
            assert pos and all(p.ndim > 1 and id(p) in rest for p in pos)
            # another suffix list: the position embeddings are decayed again
            assert all(id(p) in {id(q) for q in decay_groups(model, 0.05, no_decay_names=())[0]["params"]} for p in pos)
        torch.optim.AdamW(groups, lr=1e-3)                            # the groups are what an optimizer takes


# ---- Trainer on the CPU with a torch optimizer: the host path -------------------------------------------------------------------

def test_trainer_host_path_equals_a_loop_with_lambda_lr(tmp_path):
    import loss as L
    from Trainer import Trainer
    EPOCHS, WARMUP = 3, 3
    xs, ls = recipe.synthetic_batch(6, 1, 32, 32, 2, seed=21)

    def fresh():
        torch.manual_seed(0)
        L.CLASS_NUMBER = 2
        m = ref_unet.RefUNet(1, 2, 8, False)
        m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=21))
        decay = [p for p in m.parameters() if p.ndim > 1]
        rest = [p for p in m.parameters() if p.ndim <= 1]
        opt = torch.optim.AdamW([dict(params=decay, lr=2e-3, weight_decay=0.05), dict(params=rest, lr=1e-3, weight_decay=0.0)])
        return m, opt

    loaders = {"train": DataLoader(TensorDataset(xs[:4], ls[:4]), batch_size=2, shuffle=False),
               "val": DataLoader(TensorDataset(xs[4:], ls[4:]), batch_size=1)}
    steps = EPOCHS * len(loaders["train"])

    # the hand-written loop: LambdaLR over the same optimizer class, stepped after every optimizer step
    m0, o0 = fresh()
    sched = torch.optim.lr_scheduler.LambdaLR(o0, _factor("cosine", WARMUP, steps, 0.9, 0.0))
    want_lrs = []
    m0.train()
    for _ in range(EPOCHS):
        for x, lab in loaders["train"]:
            want_lrs.append([g["lr"] for g in o0.param_groups])
            loss = L.calc_loss(m0(x.float()), lab.float(), loss_type="dice_bce_mc")
            o0.zero_grad()
            loss.backward()
            o0.step()
            sched.step()

    m1, o1 = fresh()
    got_lrs, step = [], o1.step

    def spy(*a, **k):
        got_lrs.append([g["lr"] for g in o1.param_groups])
        return step(*a, **k)
    o1.step = spy
    os.makedirs(tmp_path, exist_ok=True)
    tr = Trainer(m1, "single", torch.FloatTensor, "cpu", str(tmp_path), loaders, 2, o1, 25, EPOCHS, "dice_bce_mc", "dice_bce_mc",
                 lr_schedule=dict(kind="cosine", warmup=WARMUP))
    tr.train()
    assert tr.iter_num == steps == len(got_lrs) == 6
    assert got_lrs == want_lrs                                        # every step, both groups, as Python floats
    assert got_lrs[0] == [2e-3 * (1.0 / 3), 1e-3 * (1.0 / 3)] and got_lrs[3][0] == 2e-3 * (0.5 * (1.0 + math.cos(math.pi * 0.5)))
    # train() loads the best epoch's weights at its end; the last epoch's are in last_epoch.pt
    last = torch.load(os.path.join(tmp_path, "models", "last_epoch.pt"))
    assert list(last) == list(m0.state_dict())
    for k, v in m0.state_dict().items():
        assert torch.equal(last[k], v), k
    # the per-epoch LR lines show the LR of the step that follows
    lines = [l for l in open(os.path.join(tmp_path, "logs.txt")).read().split("\n") if l.startswith("LR ")]
    assert lines == [f"LR {lr}" for e in range(EPOCHS) for lr in want_lrs[2 * e]]


# ---- layout ---------------------------------------------------------------------------------------------------------------------

def test_hyper_block_layout_keeps_every_old_offset():
    from umi import lib
    from umi.optim import SCHEDULE_KINDS, _HYPER
    cls = lib.STRUCTS["umi_optim_hyper"]
    assert ctypes.sizeof(cls) == 96 == _HYPER.itemsize
    off = {n: (getattr(cls, n).offset, getattr(cls, n).size) for n, _ in cls._fields_}
    old = dict(lr=(0, 8), base_lr=(8, 8), iter=(16, 8), max_iter=(24, 8), power=(32, 8), adam_t=(40, 8), beta1=(48, 8),
               beta2=(56, 8), lr_f=(64, 4), step_size_f=(68, 4), bc2_sqrt_f=(72, 4))
    assert {k: off[k] for k in old} == old
    assert {k: off[k] for k in off if k not in old} == dict(kind=(76, 4), warmup=(80, 8), final_ratio=(88, 8))   # the old padding
    assert SCHEDULE_KINDS == dict(poly=1, cosine=2, constant=3) and lib.ENUMS["UMI_SCHED_NONE"] == 0
    for name in ("umi_optim_adamw_multi", "umi_optim_adamw_multi_dev", "umi_optim_adamw_multi_guarded", "umi_optim_hyper_schedule"):
        assert name in lib.SIGNATURES
    # same argument checks and status codes as the Adam siblings: refused before any launch
    assert lib.fn("umi_optim_adamw_multi")(None, 0, 0, 1e-3, 1e-3, 0.9, 0.999, 1.0, 1e-8, 0.01, None) == lib.UMI_ERR_BADARG
    assert lib.fn("umi_optim_adamw_multi_dev")(None, 0, 0, None, 0.9, 0.999, 1e-8, 0.01, None) == lib.UMI_ERR_BADARG
    assert lib.fn("umi_optim_adamw_multi_guarded")(None, 0, 0, None, 1e-3, 1e-3, 0.9, 0.999, 1.0, 1e-8, 0.01, None, None) == \
        lib.UMI_ERR_BADARG
    assert lib.fn("umi_optim_hyper_schedule")(None, None) == lib.UMI_ERR_BADARG


def test_adamw_is_torch_s_adamw_on_the_host():
    from umi import optim as uo
    p = torch.nn.Parameter(torch.zeros(3))
    opt = uo.AdamW([p], lr=1e-3, weight_decay=0.1)
    assert isinstance(opt, torch.optim.AdamW) and opt.param_groups[0]["decoupled_weight_decay"] is True
    ref = torch.optim.AdamW([p], lr=1e-3, weight_decay=0.1)
    assert opt.state_dict() == ref.state_dict()
    opt.load_state_dict(ref.state_dict())
    ref.load_state_dict(opt.state_dict())
    assert uo.Adam([p], lr=1e-3, decoupled_weight_decay=True).param_groups[0]["decoupled_weight_decay"] is True
    assert uo.AdamW.step is not torch.optim.AdamW.step
    p.grad = torch.ones(3)
    for kw in (dict(lr=1e-3, amsgrad=True), dict(lr=1e-3, maximize=True), dict(lr=1e-3, capturable=True),
               dict(lr=torch.tensor(1e-3))):
        with pytest.raises(NotImplementedError, match="umi.optim.AdamW"):
            uo.AdamW([p], **kw).step()
