"""umi.ema without a GPU: the NumPy statements of the state machine and of the update, the statement against
torch.optim.swa_utils.AveragedModel, the header's enum and the entry points' argument checks, and Trainer(ema=...) on the CPU
oracle: what is validated is what is saved, validate=False changes no file, a cut run resumes bit for bit, and the refusals."""
import os
import random

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

EPOCHS = 3


# ---- the state machine -----------------------------------------------------------------------------------------------------

def _state(decay, warmup, t=0.0):
    from umi.ema import EMA, EMA_LEN
    st = np.zeros(EMA_LEN)
    st[EMA["DECAY"]], st[EMA["WARMUP"]], st[EMA["UPDATES"]] = decay, float(warmup), t
    st[EMA["SPARE0"]], st[EMA["SPARE1"]] = 0.25, -3.0              # must survive untouched
    return st


@pytest.mark.parametrize("warmup", [True, False])
@pytest.mark.parametrize("t", [0, 1, 8, 9, 10, 10 ** 6])
def test_state_machine(warmup, t):
    from umi.ema import EMA, ema_state_update_numpy
    d = 0.999
    st = _state(d, warmup, float(t))
    out = ema_state_update_numpy(st, False)
    want = min(d, (1.0 + t) / (10.0 + t)) if warmup else d
    assert out[EMA["LAST"]] == want and out[EMA["UPDATES"]] == t + 1 and out[EMA["ACTIVE"]] == 1.0
    assert out[EMA["DECAY"]] == d and out[EMA["WARMUP"]] == float(warmup)
    assert out[EMA["SPARE0"]] == 0.25 and out[EMA["SPARE1"]] == -3.0
    w = out[EMA["WEIGHT"]]
    assert w == float(np.float32(w)) and w == float(np.float32(1.0 - want))        # exactly a float32 value
    if warmup and t < 9:
        assert out[EMA["LAST"]] < d                                                # the warm-up is what bounds it
    if t == 0 and warmup:
        assert out[EMA["LAST"]] == 0.1
    # the input is not modified, and a skip changes ACTIVE alone
    assert st[EMA["UPDATES"]] == t
    sk = ema_state_update_numpy(out, True)
    assert sk[EMA["ACTIVE"]] == 0.0
    keep = [i for i in range(len(out)) if i != EMA["ACTIVE"]]
    assert np.array_equal(sk[keep], out[keep])
    again = ema_state_update_numpy(sk, False)                                       # the un-advanced t is used
    assert again[EMA["UPDATES"]] == t + 2 and again[EMA["ACTIVE"]] == 1.0


def test_update_statement_is_three_float32_roundings():
    from umi.ema import ema_update_numpy
    g = np.random.default_rng(0)
    e, p = g.standard_normal(1000).astype(np.float32), g.standard_normal(1000).astype(np.float32)
    w = np.float32(0.1)
    out = ema_update_numpy(e, p, 0.1)                                                # the weight is rounded to float32 first
    d = (p - e).astype(np.float32)
    assert out.dtype == np.float32 and np.array_equal(out, e + (w * d).astype(np.float32))
    assert np.array_equal(ema_update_numpy(e, p, 0.0), e) and np.array_equal(ema_update_numpy(e, e, 0.3), e)


@pytest.mark.parametrize("decay", [0.9, 0.999])
def test_statement_against_averaged_model(decay):
    """One update from an identical averaged state, against AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay)).

    Bound, per element, with M = max(|e|, |p|) and w = float32(1 - decay) <= 0.1 (both sides use that w: torch rounds its
    Python scalar to the tensors' dtype).  The exact value v = e + w (p - e) lies between e and p, so |v| <= M.  The statement
    rounds three times: p - e (|p - e| <= 2 M, error <= ulp(2 M) / 2 = ulp(M), scaled by w), the product (|.| <= 2 w M, error
    <= ulp(2 w M) / 2 <= w ulp(M)) and the sum (|.| <= M up to rounding, error <= ulp(M) / 2): (2 w + 1/2) ulp(M) <= 0.7
    ulp(M).  torch's lerp rounds the difference and then either fuses or does not fuse the multiply-add: at most the same three
    roundings, <= 0.7 ulp(M).  Two values within 0.7 ulp(M) of v differ by at most 1.4 ulp(M) < 2 ulp(M)."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    from umi.ema import ema_update_numpy
    torch.manual_seed(3)
    m = torch.nn.Sequential(torch.nn.Linear(37, 53), torch.nn.Linear(53, 11))
    avg = AveragedModel(m, multi_avg_fn=get_ema_multi_avg_fn(decay))
    avg.update_parameters(m)                                                       # the first call copies
    e = [p.detach().numpy().copy() for p in avg.module.parameters()]
    with torch.no_grad():
        for p in m.parameters():
            p.add_(torch.randn_like(p) * 0.3)
    avg.update_parameters(m)
    w = np.float32(1.0 - decay)
    for e0, p, got in zip(e, m.parameters(), avg.module.parameters()):
        p = p.detach().numpy()
        want = ema_update_numpy(e0, p, w)
        bound = 2.0 * np.spacing(np.maximum(np.abs(e0), np.abs(p)))
        assert np.all(np.abs(want.astype(np.float64) - got.detach().numpy().astype(np.float64)) <= bound)
        assert not np.array_equal(want, e0)


# ---- the header and the entry points ---------------------------------------------------------------------------------------

def test_enum_comes_from_the_header_and_null_arguments_are_refused():
    from umi import ema, lib
    assert lib.UMI_EMA_LEN == 8 == ema.EMA_LEN
    assert ema.EMA == dict(DECAY=0, WARMUP=1, UPDATES=2, LAST=3, WEIGHT=4, ACTIVE=5, SPARE0=6, SPARE1=7)
    assert all(lib.ENUMS["UMI_EMA_" + k] == v for k, v in ema.EMA.items())
    for name in ("umi_ema_pre", "umi_ema_multi", "umi_ema_swap_multi"):
        assert name in lib.SIGNATURES
    # nothing below reaches a launch: no GPU is touched
    assert lib.fn("umi_ema_pre")(None, None, None) == lib.UMI_ERR_BADARG
    assert lib.fn("umi_ema_multi")(None, 1, 1, None, None) == lib.UMI_ERR_BADARG
    assert lib.fn("umi_ema_multi")(None, 0, 0, None, None) == lib.UMI_ERR_BADARG          # no state block
    assert lib.fn("umi_ema_swap_multi")(None, 1, 1, None) == lib.UMI_ERR_BADARG
    assert lib.fn("umi_ema_swap_multi")(None, -1, 0, None) == lib.UMI_ERR_BADARG
    assert lib.fn("umi_ema_swap_multi")(None, 0, -1, None) == lib.UMI_ERR_BADARG
    assert lib.fn("umi_ema_swap_multi")(None, 0, 1, None) == lib.UMI_ERR_BADARG
    assert lib.fn("umi_ema_swap_multi")(None, 0, 0, None) == lib.UMI_OK                    # an empty table: nothing to launch


# ---- ModelEMA on the CPU ---------------------------------------------------------------------------------------------------

def test_model_ema_cpu_follows_the_statements():
    from umi.ema import EMA, ModelEMA, ema_state_update_numpy, ema_update_numpy
    torch.manual_seed(1)
    m = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.BatchNorm1d(7), torch.nn.Linear(7, 3))
    m[2].bias.requires_grad_(False)
    ema = ModelEMA(m, decay=0.99, warmup=True)
    assert ema.names == [n for n, p in m.named_parameters() if p.requires_grad] and "2.bias" not in ema.names
    assert list(ema.tensors()) == ["shadow." + n for n in ema.names] + ["state"]
    e = [s.numpy().copy() for s in ema.shadows]
    st = ema.state.numpy().copy()
    for step in range(12):
        with torch.no_grad():
            for p in m.parameters():
                p.add_(torch.randn_like(p) * 0.1)
        ema.update()
        st = ema_state_update_numpy(st, False)
        e = [ema_update_numpy(a, p.detach().numpy(), st[EMA["WEIGHT"]]) for a, p in zip(e, ema.params)]
        assert np.array_equal(ema.state.numpy(), st)
        assert all(np.array_equal(a, s.numpy()) for a, s in zip(e, ema.shadows))
    assert ema.sync_host() == dict(decay=0.99, warmup=True, updates=12, last=12.0 / 21.0, weight=float(np.float32(1 - 12.0 / 21.0)),     # t = 11
                                   active=True)
    live = [p.detach().clone() for p in ema.params]
    versions = [p._version for p in ema.params]
    ema.swap()
    assert ema.swapped and all(np.array_equal(a, p.detach().numpy()) for a, p in zip(e, ema.params))
    assert all(torch.equal(a, s) for a, s in zip(live, ema.shadows)) and all(p._version > v for p, v in zip(ema.params, versions))
    with pytest.raises(RuntimeError, match="swapped"):
        ema.update()
    sd = ema.state_dict()                                          # the average, whichever side holds it
    assert all(np.array_equal(a, sd[n].numpy()) for a, n in zip(e, ema.names))
    ema.swap()
    assert not ema.swapped and all(torch.equal(a, p) for a, p in zip(live, ema.params))
    twin = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.BatchNorm1d(7), torch.nn.Linear(7, 3))
    twin[2].bias.requires_grad_(False)
    ema.copy_to(twin)
    assert all(np.array_equal(a, dict(twin.named_parameters())[n].detach().numpy()) for a, n in zip(e, ema.names))
    other = ModelEMA(twin, decay=0.5, warmup=False)
    other.load_state_dict(sd)
    assert torch.equal(other.state, ema.state) and all(torch.equal(a, b) for a, b in zip(other.shadows, ema.shadows))
    with pytest.raises(ValueError):
        other.load_state_dict({k: v for k, v in sd.items() if k != "0.bias"})
    with pytest.raises(ValueError):
        ModelEMA(m, decay=1.0)


# ---- Trainer(ema=...) on the CPU oracle ------------------------------------------------------------------------------------

class Cut(Exception):
    pass


class CutLoader:
    """A loader that raises Cut when its `at`-th epoch is about to start (None: never)."""

    def __init__(self, loader, at=None):
        self.loader, self.at, self.epochs, self.generator = loader, at, 0, loader.generator

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        self.epochs += 1
        if self.at is not None and self.epochs == self.at:
            raise Cut()
        return iter(self.loader)


def _trainer(out_dir, cut_at=None, **kw):
    """RefUNet(1, 2, 4) at 16 x 16, four training images at batch 2 (shuffled by the loader's own generator), two validation
    images, torch.optim.SGD with momentum and the poly rule."""
    import loss as L
    from Trainer import Trainer
    from oracle import ref_unet
    L.CLASS_NUMBER = 2
    torch.manual_seed(100)
    m = ref_unet.RefUNet(1, 2, 4, False)
    g = torch.Generator().manual_seed(7)
    x, lab = torch.randn(6, 1, 16, 16, generator=g), torch.randint(0, 2, (6, 16, 16), generator=g).float()
    train = DataLoader(TensorDataset(x[:4], lab[:4]), batch_size=2, shuffle=True, generator=torch.Generator().manual_seed(3))
    loaders = {"train": CutLoader(train, cut_at), "val": DataLoader(TensorDataset(x[4:], lab[4:]), batch_size=2)}
    opt = torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    tr = Trainer(m, "single", torch.FloatTensor, "cpu", str(out_dir), loaders, 2, opt, 25, EPOCHS, "dice_bce_mc", "dice_bce_mc",
                 lr_scheduler=True, **kw)
    return tr, m, opt


def _seed_everything():
    torch.manual_seed(5)
    random.seed(5)
    np.random.seed(5)


def _files(out):
    d = os.path.join(out, "models")
    return {n: torch.load(os.path.join(d, n), weights_only=True) for n in sorted(os.listdir(d))}


def _same_files(a, b):
    assert list(a) == list(b)
    for n in a:
        assert list(a[n]) == list(b[n])
        assert all(torch.equal(a[n][k], b[n][k]) for k in a[n]), n


EMA_KW = dict(decay=0.9, warmup=True)


@pytest.fixture(scope="module")
def whole(tmp_path_factory):
    """The uncut run with ema validating, its parameters recorded after every optimizer step: the reference of this module."""
    out = tmp_path_factory.mktemp("whole")
    _seed_everything()
    tr, m, opt = _trainer(out, ema=dict(EMA_KW))
    names = [n for n, _ in m.named_parameters()]
    first = [p.detach().numpy().copy() for p in m.parameters()]
    steps = []
    opt.register_step_post_hook(lambda *a: steps.append([p.detach().numpy().copy() for p in m.parameters()]))
    tr.train()
    return dict(tr=tr, m=m, out=out, names=names, first=first, steps=steps, files=_files(out),
                lists=[list(getattr(tr, n)) for n in tr._LISTS], log=open(os.path.join(out, "logs.txt")).read())


def test_trainer_validates_and_saves_the_averaged_weights(whole):
    from umi.ema import EMA, EMA_LEN, ema_state_update_numpy, ema_update_numpy
    tr, names, steps = whole["tr"], whole["names"], whole["steps"]
    assert len(steps) == 2 * EPOCHS and tr.ema is not None and not tr.ema.swapped
    st = np.zeros(EMA_LEN)
    st[EMA["DECAY"]], st[EMA["WARMUP"]] = 0.9, 1.0
    e, at_epoch = whole["first"], {}
    for i, params in enumerate(steps):
        st = ema_state_update_numpy(st, False)
        e = [ema_update_numpy(a, p, st[EMA["WEIGHT"]]) for a, p in zip(e, params)]
        if i % 2 == 1:
            at_epoch[i // 2 + 1] = e
    # the state block and the shadows after the run are the statement's
    assert np.array_equal(tr.ema.state.numpy(), st)
    assert all(np.array_equal(a, s.numpy()) for a, s in zip(e, tr.ema.shadows))
    files = whole["files"]
    saved = sorted(int(n[5:-3]) for n in files if n.startswith("epoch"))
    assert saved and "best.pt" in files and "last_epoch.pt" in files
    best = saved[-1]
    for n, a in zip(names, at_epoch[best]):                          # what was validated is what was saved
        assert np.array_equal(files["best.pt"][n].numpy(), a), n
        assert np.array_equal(files[f"epoch{best}.pt"][n].numpy(), a), n
        assert np.array_equal(tr.best_model[n].numpy(), a), n
    for ep in saved:
        assert all(np.array_equal(files[f"epoch{ep}.pt"][n].numpy(), a) for n, a in zip(names, at_epoch[ep]))
    for n, a in zip(names, steps[-1]):                               # last_epoch.pt keeps the live weights
        assert np.array_equal(files["last_epoch.pt"][n].numpy(), a), n
    assert any(not np.array_equal(a, b) for a, b in zip(steps[-1], at_epoch[EPOCHS]))
    for n, p in whole["m"].named_parameters():                       # train() returns the best averaged weights
        assert torch.equal(p.detach(), files["best.pt"][n])
    for ep in range(1, EPOCHS + 1):
        d = min(0.9, (1.0 + (2 * ep - 1)) / (10.0 + (2 * ep - 1)))
        assert "EMA on epoch %i: decay %g, updates %i\n" % (ep, d, 2 * ep) in whole["log"]


def test_validate_false_changes_no_file(whole, tmp_path):
    _seed_everything()
    tr0, m0, _ = _trainer(tmp_path / "off")
    tr0.train()
    _seed_everything()
    tr1, m1, _ = _trainer(tmp_path / "kept", ema=dict(validate=False, **EMA_KW))
    tr1.train()
    _same_files(_files(tmp_path / "off"), _files(tmp_path / "kept"))
    assert [list(getattr(tr0, n)) for n in tr0._LISTS] == [list(getattr(tr1, n)) for n in tr1._LISTS]
    assert tr0.ema is None and "EMA on epoch" not in open(tmp_path / "off" / "logs.txt").read()
    # ... and the average was maintained all the same: the one of the validating run, whose training steps are the same
    assert tr1.ema.sync_host()["updates"] == 2 * EPOCHS
    assert all(torch.equal(a, b) for a, b in zip(tr1.ema.shadows, whole["tr"].ema.shadows))
    assert whole["lists"][0] == tr0.train_loss_list and whole["lists"][1] != tr0.val_loss_list


def test_cut_and_resumed_run_equals_the_whole_run(whole, tmp_path):
    _seed_everything()
    tr, m, opt = _trainer(tmp_path, cut_at=2, resume=True, ema=dict(EMA_KW))
    with pytest.raises(Cut):
        tr.train()
    assert len(tr.train_loss_list) == 1
    pl = torch.load(tmp_path / "run_state.pt", weights_only=True)
    assert list(pl["ema"]) == ["shadow." + n for n in whole["names"]] + ["state"] and pl["epoch"] == 1
    torch.manual_seed(999)
    random.seed(999)
    np.random.seed(999)
    tr, m, opt = _trainer(tmp_path, resume=True, ema=dict(EMA_KW))              # new objects: everything comes from the file
    tr.train()
    assert [list(getattr(tr, n)) for n in tr._LISTS] == whole["lists"]
    _same_files(_files(tmp_path), whole["files"])
    assert torch.equal(tr.ema.state, whole["tr"].ema.state)
    assert all(torch.equal(a, b) for a, b in zip(tr.ema.shadows, whole["tr"].ema.shadows))
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), whole["m"].parameters()))


@pytest.mark.parametrize("written_with", [True, False])
def test_run_state_and_ema_must_agree(tmp_path, written_with):
    on, off = dict(ema=dict(EMA_KW)), {}
    _seed_everything()
    tr, m, opt = _trainer(tmp_path, cut_at=2, resume=True, **(on if written_with else off))
    with pytest.raises(Cut):
        tr.train()
    tr, m, opt = _trainer(tmp_path, resume=True, **(off if written_with else on))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with pytest.raises(ValueError, match="ema"):
        tr.train()
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())      # nothing was modified
    assert tr.iter_num == 0 and tr.train_loss_list == [] and not opt.state


def test_trainer_refusals(tmp_path):
    from Trainer import Trainer
    from oracle import ref_unet

    class Never:
        generator = None

        def __len__(self):
            return 1

        def __iter__(self):
            raise AssertionError("a step ran")

    m = ref_unet.RefUNet(1, 2, 4, False)
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    loaders = {"train": Never(), "val": Never()}
    tr = Trainer(m, "multi_task", torch.FloatTensor, "cpu", str(tmp_path), loaders, 1, opt, 1, 1, "multi_task_loss_ratio", "mse",
                 ema=True)
    with pytest.raises(NotImplementedError, match="multi_task_loss_ratio"):
        tr.train()
    for bad in ("yes", 1, 1.5, [0.9], dict(decay=0.9, momentum=1), dict(validate="no"), object()):
        with pytest.raises(ValueError, match="ema"):
            Trainer(m, "single", torch.FloatTensor, "cpu", str(tmp_path), loaders, 1, opt, 1, 1, "dice_bce_mc", "dice_bce_mc", ema=bad)
    for ok in (None, False, True, 0.99, dict(decay=0.5, warmup=False, validate=False)):
        tr = Trainer(m, "single", torch.FloatTensor, "cpu", str(tmp_path), loaders, 1, opt, 1, 1, "dice_bce_mc", "dice_bce_mc", ema=ok)
        assert tr.ema is None                                         # built at the first step
    with pytest.raises(TypeError):                                    # keyword-only: the positionals stay the reference's
        Trainer(m, "single", torch.FloatTensor, "cpu", str(tmp_path), loaders, 1, opt, 1, 1, "dice_bce_mc", "dice_bce_mc", None, 1,
                True)
