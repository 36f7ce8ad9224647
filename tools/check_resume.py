"""The runs of tests/test_gpu_snapshot.py's Trainer cases, and the child process that resumes one of them.

    python tools/check_resume.py <case> <out_dir> <summary.pt>

resumes the run whose state lies in <out_dir>/run_state.pt -- in THIS fresh process: new model, optimizer and Trainer, no
captured graph, generators seeded differently -- trains it to its end and writes its summary() to <summary.pt>.  The test
compares that summary with the run that was never cut.

A case is small: UNet(1, 2, 8) or UNet_multitask(1, 1, 8) at 32 x 32, four training images at batch 2 shuffled by the loader's
own generator, two validation images, 4 epochs, the poly rule on.  `build(case, out_dir, cut_at=None, **flags)` makes its
Trainer; `cut_at=k` makes the training loader raise Cut when epoch k is about to start.
"""
import os
import struct
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (REPO, os.path.join(REPO, "unet-torch_amd")) if p not in sys.path]
import torch                                          # noqa: E402
from torch.utils.data import DataLoader, Dataset      # noqa: E402

DEV = "cuda:0"
EPOCHS = 4
CASES = {
    # name: (compute mode, graph, optimizer, model / Trainer extras)
    "fp32_eager_sgd": ("fp32", False, "sgd", {}),
    "fp16_graph_sgd": ("fp16", True, "sgd", {}),
    "fp32_graph_adam": ("fp32", True, "adam", {}),
    "fp16_eager_adam": ("fp16", False, "adam", {}),
    "dropout": ("fp32", True, "sgd", dict(dropout=True)),
    # one batch of epoch 2 carries an inf: a skipped step, the dynamic scale backs off before the cut
    "guard": ("fp16", True, "sgd", dict(grad_guard=dict(max_norm=1.0, dynamic_scale=True), inf_at=2)),
    "multitask": ("fp32", True, "sgd", dict(multitask=True)),
}


class Cut(Exception):
    pass


class Items(Dataset):
    """(image, label) or (image, (label 1, label 2))."""

    def __init__(self, x, *labels):
        self.x, self.labels = x, labels

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], (self.labels[0][i] if len(self.labels) == 1 else tuple(l[i] for l in self.labels))


class CutLoader:
    """The training loader: raises Cut when its `at`-th epoch is about to start (None: never), and writes an inf into the first
    pixel of batch number `inf_at` (counted over the run's lifetime in this process, from 0; None: never)."""

    def __init__(self, loader, at=None, inf_at=None):
        self.loader, self.at, self.inf_at, self.epochs, self.batches, self.generator = loader, at, inf_at, 0, 0, loader.generator

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        self.epochs += 1
        if self.at is not None and self.epochs == self.at:
            raise Cut()
        for x, y in self.loader:
            if self.batches == self.inf_at:
                x = x.clone()
                x[0, 0, 0, 0] = float("inf")
            self.batches += 1
            yield x, y


def build(case, out_dir, cut_at=None, past_cut=False, **flags):
    """(Trainer, model, optimizer) of `case`, from fixed seeds: model 100, data 7, loader 3.  `past_cut`: the run continues
    behind the cut, so a batch the case poisons before the cut is not poisoned again."""
    import Model
    import loss as L
    from Trainer import Trainer
    from umi import optim as uo
    mode, graph, kind, extra = CASES[case]
    extra = dict(extra)
    multi, inf_at = extra.pop("multitask", False), extra.pop("inf_at", None)
    dropout = extra.pop("dropout", False)
    L.CLASS_NUMBER = 2
    torch.manual_seed(100)
    if multi:
        m = Model.UNet_multitask(1, 1, 8, False, compute_dtype=mode).to(DEV)
    else:
        m = Model.UNet(1, 2, 8, False, dropout=dropout, compute_dtype=mode).to(DEV)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(6, 1, 32, 32, generator=g)
    if multi:
        labels = [torch.rand(6, 32, 32, generator=g) for _ in range(2)]
    else:
        labels = [torch.randint(0, 2, (6, 32, 32), generator=g).float()]
    train = DataLoader(Items(x[:4], *[l[:4] for l in labels]), batch_size=2, shuffle=True,
                       generator=torch.Generator().manual_seed(3))
    loaders = {"train": CutLoader(train, cut_at, None if past_cut else inf_at), "val": DataLoader(Items(x[4:], *[l[4:] for l in labels]), batch_size=2)}
    if kind == "sgd":
        opt = uo.SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    else:
        opt = uo.Adam(m.parameters(), lr=1e-3, weight_decay=1e-4)
    loss = "mse" if multi else "dice_bce_mc"
    tr = Trainer(m, "multi_task" if multi else "single", torch.cuda.FloatTensor, DEV, str(out_dir), loaders, 2, opt, 25, EPOCHS,
                 loss, loss, lr_scheduler=True, graph=graph, **extra, **flags)
    return tr, m, opt


def _bits(values):
    return [struct.pack("<d", float(v)) for v in values]              # (a skipped step's loss may be NaN: compare the bits)


def summary(tr, m, opt, out_dir):
    """Everything the cut-and-resumed run must share with the whole run, on the host."""
    torch.cuda.synchronize()
    osd = opt.state_dict()                                            # (sync_host: LR, iteration and Adam's step from the device)
    state = {i: {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in st.items()} for i, st in osd["state"].items()}
    hyper = [dev.cpu().clone() for dev, _ in (opt.device_hyper or [])]
    guard = None if tr._guard is None or tr._guard.state is None else tr._guard.state.cpu().clone()
    drops = {n: (mod._drop_base, mod._drop_step.cpu().clone()) for n, mod in m.named_modules()
             if getattr(mod, "_drop_step", None) is not None}
    return dict(lists={n: _bits(getattr(tr, n)) for n in tr._LISTS}, iters=tr.iter_num,
                best=_bits([tr.best_val_score, tr.best_loss, tr.early_stop_counter]),
                lr=_bits(g["lr"] for g in opt.param_groups), files=sorted(os.listdir(os.path.join(out_dir, "models"))),
                weights={k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, optimizer=state, hyper=hyper,
                guard=guard, drops=drops, best_model={k: v.detach().cpu().clone() for k, v in dict(tr.best_model or {}).items()},
                graphs=len(tr._graphs))


def _eq(u, v):
    """The same bits (torch.equal calls two NaNs different; a poisoned batch leaves NaNs in the BatchNorm statistics)."""
    return u.dtype == v.dtype and u.shape == v.shape and torch.equal(u.contiguous().reshape(-1).view(torch.uint8),
                                                                     v.contiguous().reshape(-1).view(torch.uint8))


def same(a, b):
    """None, or the first difference between two summaries (`graphs` is not compared: it is a count of this process)."""
    for key in ("lists", "iters", "best", "lr", "files"):
        if a[key] != b[key]:
            return f"{key}: {a[key]!r} != {b[key]!r}"
    for key in ("weights", "best_model"):
        if list(a[key]) != list(b[key]):
            return f"{key}: other names"
        for k in a[key]:
            if not _eq(a[key][k], b[key][k]):
                return f"{key}[{k}] differs"
    if sorted(a["optimizer"]) != sorted(b["optimizer"]):
        return "optimizer: other parameters have state"
    for i in a["optimizer"]:
        for k, v in a["optimizer"][i].items():
            w = b["optimizer"][i].get(k)
            if not (torch.is_tensor(w) and _eq(v, w) if torch.is_tensor(v) else v == w):
                return f"optimizer state {i}.{k} differs"
    if len(a["hyper"]) != len(b["hyper"]) or not all(_eq(u, v) for u, v in zip(a["hyper"], b["hyper"])):
        return "the device hyper blocks differ"
    if (a["guard"] is None) != (b["guard"] is None) or (a["guard"] is not None and
                                                        a["guard"].view(torch.int64).tolist() != b["guard"].view(torch.int64).tolist()):
        return f"the guard blocks differ: {a['guard']} / {b['guard']}"
    if sorted(a["drops"]) != sorted(b["drops"]) or any(a["drops"][n][0] != b["drops"][n][0] or
                                                      not torch.equal(a["drops"][n][1], b["drops"][n][1]) for n in a["drops"]):
        return "the dropout bases or counters differ"
    return None


def main(case, out_dir, summary_path):
    import random
    import numpy as np
    assert os.path.exists(os.path.join(out_dir, "run_state.pt")), "nothing to resume"
    tr, m, opt = build(case, out_dir, past_cut=True, resume=True)
    torch.manual_seed(999)                            # the generators of this process: the file's states must replace them
    random.seed(999)
    np.random.seed(999)
    tr.train()
    torch.save(summary(tr, m, opt, out_dir), summary_path)
    print("resumed", case, "iterations", tr.iter_num)


if __name__ == "__main__":
    main(*sys.argv[1:4])
