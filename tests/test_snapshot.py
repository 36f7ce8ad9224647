"""Snapshots and resumption without a GPU: the NumPy statement of the arena (umi.snapshot.layout / snapshot_numpy), the C ABI's
refusals, the CPU path of Snapshot and CheckpointWriter, and Trainer(resume=...) on the CPU oracle: a run cut after epoch 2 and
resumed with new objects against the run that was never cut, bit for bit."""
import os
import random

import numpy as np
import pytest
import torch
from torch.utils.data import DataLoader, TensorDataset

EPOCHS = 4


# ---- the arena ---------------------------------------------------------------------------------------------------------------

def test_layout_and_snapshot_numpy_by_hand():
    from umi import ddp, snapshot as S
    assert S.layout([]) == ([], 0)
    assert S.layout([5, 0, 0, 1, 4, 8193]) == ([0, 8, 8, 8, 12, 16], 16 + 8196)
    with pytest.raises(ValueError):
        S.layout([3, -1])
    arrays = [np.array([1.0, -0.0, 0.0, 2.5, 3.0], dtype=np.float32), np.zeros(0, dtype=np.float32),
              np.array([7, -1], dtype=np.int64), np.array([[1, 2, 3, 4]], dtype=np.uint8)]
    arena, word = S.snapshot_numpy(arrays)
    f32 = lambda v: int(np.array([v], dtype=np.float32).view(np.uint32)[0])      # noqa: E731
    assert arena.dtype == np.uint32 and arena.tolist() == [
        f32(1.0), 0x80000000, 0, f32(2.5), f32(3.0), 0, 0, 0,           # 5 words, 3 pad words
        7, 0, 0xFFFFFFFF, 0xFFFFFFFF,                                   # the empty tensor has no slot; two int64 = 4 words
        0x04030201, 0, 0, 0]                                            # 4 bytes = one word, 3 pad words
    assert word == ddp.fingerprint_numpy(arrays)
    with pytest.raises(ValueError, match="32-bit words"):
        S.snapshot_numpy([np.zeros(3, dtype=np.uint8)])


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    import ctypes
    from umi import build, lib
    cdll = ctypes.CDLL(build.LIB)
    for n in ("umi_snapshot_multi", "umi_restore_multi", "umi_snapshot_ws_bytes"):
        assert n in lib.SIGNATURES and hasattr(cdll, n), n
    assert lib.fn("umi_snapshot_ws_bytes")(0) == 0 and lib.fn("umi_snapshot_ws_bytes")(-2) == 0
    assert lib.fn("umi_snapshot_ws_bytes")(3) == 24
    f = lib.fn("umi_snapshot_multi")
    word = (ctypes.c_ulonglong * 2)()
    out, ws, descs = ctypes.addressof(word), ctypes.addressof((ctypes.c_ulonglong * 4)()), ctypes.addressof((ctypes.c_char * 96)())
    assert f(descs, 1, 1, ws, 8, None, None) == lib.UMI_ERR_BADARG                  # no result word
    assert f(descs, 1, 1, ws, 8, out + 4, None) == lib.UMI_ERR_BADARG               # misaligned result word
    assert f(descs, -1, 0, ws, 8, out, None) == lib.UMI_ERR_BADARG
    assert f(descs, 1, -1, ws, 8, out, None) == lib.UMI_ERR_BADARG
    assert f(None, 1, 1, ws, 8, out, None) == lib.UMI_ERR_BADARG                    # no table
    assert f(descs, 1, 1, None, 8, out, None) == lib.UMI_ERR_BADARG                 # no workspace
    assert f(descs, 1, 1, ws + 4, 8, out, None) == lib.UMI_ERR_BADARG               # misaligned workspace
    assert f(descs, 0, 1, ws, 8, out, None) == lib.UMI_ERR_BADARG                   # blocks without tensors
    assert f(descs, 2, 2, ws, 8, out, None) == lib.UMI_ERR_WORKSPACE                # 16 bytes needed
    g = lib.fn("umi_restore_multi")
    assert g(descs, -1, 0, None) == lib.UMI_ERR_BADARG
    assert g(descs, 1, -1, None) == lib.UMI_ERR_BADARG
    assert g(None, 1, 1, None) == lib.UMI_ERR_BADARG
    assert g(descs, 0, 1, None) == lib.UMI_ERR_BADARG
    assert g(None, 0, 0, None) == lib.UMI_OK                                        # nothing to copy: no launch


def test_cpu_snapshot_views_restore_and_writer(tmp_path):
    from umi import snapshot as S
    g = torch.Generator().manual_seed(1)
    st = {"w": torch.randn(3, 5, generator=g), "n": torch.tensor(7), "e": torch.zeros(0), "b": torch.arange(8, dtype=torch.uint8),
          "shifted": torch.randn(9, generator=g)[1:6]}
    keep = {k: v.clone() for k, v in st.items()}
    snap = S.Snapshot(st).take()
    arena, word = S.snapshot_numpy([v.numpy() for v in st.values()])
    assert snap.word() == word and (snap.arena.numpy().view(np.uint32) == arena).all() and snap.verify()
    views = snap.views()
    assert list(views) == list(st) and all(torch.equal(views[k], keep[k]) and views[k].dtype == keep[k].dtype for k in st)
    for v in st.values():
        v.zero_()
    snap.restore()
    assert all(torch.equal(st[k], keep[k]) for k in st)
    # the way to a file: every tensor in its own storage, the file written atomically
    w = S.CheckpointWriter()
    path = str(tmp_path / "ck.pt")
    for _ in range(2):                                                   # the second job waits for the first on the same path
        w.submit(snap.to_host_async(), snap.host_views(), path, snap.hold_host())
    w.join()
    got = torch.load(path, weights_only=True)
    assert list(got) == list(st) and all(torch.equal(got[k], keep[k]) for k in st)
    assert os.listdir(tmp_path) == ["ck.pt"]
    assert os.path.getsize(path) < 4096                                  # not the arena once per tensor
    # an error of the thread is raised by join(), once
    w.submit(snap.to_host_async(), snap.host_views(), str(tmp_path / "no_such_dir" / "ck.pt"), snap.hold_host())
    with pytest.raises((OSError, RuntimeError), match="no_such_dir"):
        w.join()
    w.join()                                                             # raised once
    w.close()
    with pytest.raises(RuntimeError, match="after close"):
        w.submit(None, {}, path)
    # a flipped bit: restore() raises and writes nothing
    for v in st.values():
        v.zero_()
    snap.arena[5] ^= 4
    with pytest.raises(RuntimeError, match="nothing was restored"):
        snap.restore()
    assert not any(bool(v.any()) for v in st.values())
    with pytest.raises(ValueError, match="tensor 1"):
        S.Snapshot([torch.zeros(2), torch.zeros(3, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="tensor 0 is not contiguous"):
        S.Snapshot([torch.zeros(3, 3).t()])


# ---- Trainer(resume=...) on the CPU oracle -------------------------------------------------------------------------------------

class Cut(Exception):
    pass


class CutLoader:
    """A loader that raises Cut when its `at`-th epoch is about to start (None: never): how the tests stop a run."""

    def __init__(self, loader, at=None):
        self.loader, self.at, self.epochs, self.generator = loader, at, 0, loader.generator

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        self.epochs += 1
        if self.at is not None and self.epochs == self.at:
            raise Cut()
        return iter(self.loader)


def _trainer(out_dir, cut_at=None, feat=8, epochs=EPOCHS, **kw):
    """RefUNet(1, 2, feat) at 32 x 32, four training images at batch 2 (shuffled by the loader's own generator), two validation
    images, SGD with momentum and the poly rule.  Model seed 100, data seed 7, loader seed 3."""
    import loss as L
    from Trainer import Trainer
    from oracle import ref_unet
    L.CLASS_NUMBER = 2
    torch.manual_seed(100)
    m = ref_unet.RefUNet(1, 2, feat, False)
    g = torch.Generator().manual_seed(7)
    x, lab = torch.randn(6, 1, 32, 32, generator=g), torch.randint(0, 2, (6, 32, 32), generator=g).float()
    train = DataLoader(TensorDataset(x[:4], lab[:4]), batch_size=2, shuffle=True, generator=torch.Generator().manual_seed(3))
    loaders = {"train": CutLoader(train, cut_at), "val": DataLoader(TensorDataset(x[4:], lab[4:]), batch_size=2)}
    opt = torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9, weight_decay=1e-4)
    tr = Trainer(m, "single", torch.FloatTensor, "cpu", str(out_dir), loaders, 2, opt, 25, epochs, "dice_bce_mc", "dice_bce_mc",
                 lr_scheduler=True, **kw)
    return tr, m, opt


def _summary(tr, m, opt, out_dir):
    return dict(lists=[list(getattr(tr, n)) for n in tr._LISTS], best=(tr.best_val_score, tr.best_loss, tr.early_stop_counter),
                iters=tr.iter_num, lr=[g["lr"] for g in opt.param_groups], files=sorted(os.listdir(os.path.join(out_dir, "models"))),
                weights={k: v.clone() for k, v in m.state_dict().items()},
                momentum=[opt.state[p]["momentum_buffer"].clone() for p in m.parameters()],
                best_model={k: v.clone() for k, v in tr.best_model.items()})


def _same(a, b):
    assert a["lists"] == b["lists"] and a["best"] == b["best"] and a["iters"] == b["iters"] and a["lr"] == b["lr"]
    assert a["files"] == b["files"]
    for name in ("weights", "best_model"):
        assert list(a[name]) == list(b[name])
        for k in a[name]:
            assert torch.equal(a[name][k], b[name][k]), (name, k)
    assert len(a["momentum"]) == len(b["momentum"]) and all(torch.equal(x, y) for x, y in zip(a["momentum"], b["momentum"]))


def _seed_everything():
    torch.manual_seed(5)
    random.seed(5)
    np.random.seed(5)


@pytest.fixture(scope="module")
def whole(tmp_path_factory):
    """The run that is never cut and never asked to resume: the reference of this module, computed once."""
    out = tmp_path_factory.mktemp("whole")
    _seed_everything()
    tr, m, opt = _trainer(out)
    tr.train()
    assert sorted(os.listdir(out)) == ["logs.txt", "models", "total.png"]          # both flags off: the files of before
    assert len(tr.train_loss_list) == EPOCHS and tr.iter_num == 2 * EPOCHS
    return _summary(tr, m, opt, out)


def _cut_run(out):
    """A run with resume=True cut at the start of epoch 3.  Returns the path of its run state."""
    _seed_everything()
    tr, m, opt = _trainer(out, cut_at=3, resume=True)
    with pytest.raises(Cut):
        tr.train()
    assert len(tr.train_loss_list) == 2
    path = os.path.join(out, "run_state.pt")
    assert os.path.exists(path) and not os.path.exists(path + ".tmp")
    return path


def test_resume_flag_perturbs_nothing(whole, tmp_path):
    _seed_everything()
    tr, m, opt = _trainer(tmp_path, resume=True)
    tr.train()
    _same(_summary(tr, m, opt, tmp_path), whole)
    assert sorted(os.listdir(tmp_path)) == ["logs.txt", "models", "run_state.pt", "total.png"]


def test_cut_and_resumed_run_equals_the_whole_run(whole, tmp_path):
    path = _cut_run(tmp_path)
    pl = torch.load(path, weights_only=True)                                       # one dict that weights_only accepts
    assert pl["format"] == 1 and pl["epoch"] == 2 and pl["over"] is False
    assert pl["host"]["iter_num"] == 4 and len(pl["host"]["lists"]["val_loss_list"]) == 2
    assert set(pl["host"]["rng"]) == {"torch_cpu", "torch_cuda", "python", "numpy", "loaders"}
    assert list(pl["host"]["rng"]["loaders"]) == ["train"]
    # new model, optimizer and Trainer objects, other generator states than the first run's: everything comes from the file
    torch.manual_seed(999)
    random.seed(999)
    np.random.seed(999)
    tr, m, opt = _trainer(tmp_path, resume=True)
    tr.train()
    _same(_summary(tr, m, opt, tmp_path), whole)
    # ... and the finished run's state says "over": another train() returns at once, with the best model loaded
    tr2, m2, opt2 = _trainer(tmp_path, cut_at=1, resume=True)                      # (any training epoch would raise Cut)
    tr2.train()
    assert tr2.train_loss_list == whole["lists"][0] and tr2.iter_num == whole["iters"]
    for k, v in m2.state_dict().items():
        assert torch.equal(v, whole["best_model"][k]) and torch.equal(v, m.state_dict()[k])


def _bits(m):
    return {k: v.clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("damage", ["truncated", "flipped_byte", "num_epochs", "width"])
def test_a_state_that_does_not_fit_raises_and_touches_nothing(tmp_path, damage):
    path = _cut_run(tmp_path)
    kw = {}
    if damage == "truncated":
        raw = open(path, "rb").read()
        open(path, "wb").write(raw[:len(raw) // 2])
    elif damage == "flipped_byte":
        raw = bytearray(open(path, "rb").read())
        w = torch.load(path, weights_only=True)["model"]["inc.double_conv.0.weight"].numpy().tobytes()
        at = bytes(raw).index(w)                                                   # inside the first weight tensor's bytes
        raw[at + len(w) // 2] ^= 0x10
        open(path, "wb").write(bytes(raw))
    elif damage == "num_epochs":
        kw["epochs"] = EPOCHS + 1
    else:
        kw["feat"] = 16
    tr, m, opt = _trainer(tmp_path, resume=True, **kw)
    before = _bits(m)
    with pytest.raises((ValueError, RuntimeError)):
        tr.train()
    assert all(torch.equal(v, before[k]) for k, v in m.state_dict().items())
    assert tr.iter_num == 0 and tr.train_loss_list == [] and not opt.state


def test_resume_refusals_come_before_the_first_step(tmp_path):
    from Trainer import Trainer

    class Never:
        generator = None

        def __len__(self):
            return 1

        def __iter__(self):
            raise AssertionError("a step ran")

    from oracle import ref_unet
    m = ref_unet.RefUNet(1, 2, 8, False)
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    loaders = {"train": Never(), "val": Never()}
    tr = Trainer(m, "multi_task", torch.FloatTensor, "cpu", str(tmp_path), loaders, 1, opt, 1, 1, "multi_task_loss_ratio", "mse",
                 resume=True)
    with pytest.raises(NotImplementedError, match="multi_task_loss_ratio"):
        tr.train()
    tr = Trainer(m, "single", torch.FloatTensor, "cpu", str(tmp_path), loaders, 1, opt, 1, 1, "dice_bce_mc", "dice_bce_mc",
                 resume=str(tmp_path / "elsewhere.pt"), data_parallel=dict(world_size=2))
    with pytest.raises(NotImplementedError, match="more than one rank"):
        tr.train()
    assert tr._run.resume_path == str(tmp_path / "elsewhere.pt")


def test_roll_back_in_memory_on_the_cpu(tmp_path):
    """snapshot_run_state() / restore_run_state() between steps: the same steps after the roll-back give the same bits."""
    _seed_everything()
    tr, m, opt = _trainer(tmp_path)
    g = torch.Generator().manual_seed(7)
    x, lab = torch.randn(6, 1, 32, 32, generator=g), torch.randint(0, 2, (6, 32, 32), generator=g).float()
    m.train()
    for i in range(2):
        tr.train_step(x[2 * i:2 * i + 2], lab[2 * i:2 * i + 2])
    tr.snapshot_run_state()
    ptrs = [p.data_ptr() for p in m.parameters()]

    def more():
        losses = [float(tr.train_step(x[2 * i:2 * i + 2], lab[2 * i:2 * i + 2])) for i in range(2)]
        return losses, _bits(m), [opt.state[p]["momentum_buffer"].clone() for p in m.parameters()], tr.iter_num, \
            [g_["lr"] for g_ in opt.param_groups], torch.rand(1).item()
    a = more()
    tr.restore_run_state()
    assert tr.iter_num == 2 and [p.data_ptr() for p in m.parameters()] == ptrs
    b = more()
    assert a[0] == b[0] and a[3:] == b[3:]
    assert all(torch.equal(a[1][k], b[1][k]) for k in a[1]) and all(torch.equal(u, v) for u, v in zip(a[2], b[2]))


# ---- the run-state file across changes of the Trainer -------------------------------------------------------------------------

def _tensor_specs(obj, at=""):
    """[(where, dtype, shape)] of every tensor in a nest of dicts, lists and tuples, in order."""
    if torch.is_tensor(obj):
        return [(at, obj.dtype, tuple(obj.shape))]
    if isinstance(obj, dict):
        return [s for k, v in obj.items() for s in _tensor_specs(v, f"{at}/{k}")]
    if isinstance(obj, (list, tuple)):
        return [s for i, v in enumerate(obj) for s in _tensor_specs(v, f"{at}/{i}")]
    return []


def test_a_run_state_file_of_format_1_still_resumes(tmp_path, golden_dir):
    """tests/golden/run_state_v1.pt was written by tools/gen_golden_run_state.py (the setting of _cut_run at feat=2) before the
    Trainer was split into umi/run_state.py, umi/val_batch.py and umi/dp_run.py.  No number of it is compared with a fresh run:
    CPU arithmetic may differ between torch builds, and total_time is wall clock."""
    import shutil
    from umi import ddp, run_state as R
    gold = torch.load(os.path.join(golden_dir, "run_state_v1.pt"), weights_only=True)
    assert gold["format"] == 1 and gold["epoch"] == 2 and gold["over"] is False
    # (a) both words, recomputed from the file's contents: the section order and host_word
    assert ddp.fingerprint(list(R.payload_tensors(gold).values())) == gold["word"]
    assert R.host_word(gold["host"]) == gold["host_word"]
    # (b) a new Trainer resumes from a copy of it and trains to the end
    path = str(tmp_path / "copy_of_v1.pt")
    shutil.copyfile(os.path.join(golden_dir, "run_state_v1.pt"), path)
    tr, m, opt = _trainer(tmp_path / "resumed", feat=2, resume=path)
    tr.train()
    assert tr.iter_num == 2 * EPOCHS and len(tr.train_loss_list) == len(tr.val_loss_list) == len(tr.val_score_list) == EPOCHS
    for n in tr._LISTS:
        was = gold["host"]["lists"][n]
        assert len(getattr(tr, n)) == (EPOCHS if was else 0) and getattr(tr, n)[:2] == was, n
    # (c) the file this code writes at the same cut has the fixture's layout
    _seed_everything()
    tr, m, opt = _trainer(tmp_path / "cut", cut_at=3, resume=True, feat=2)
    with pytest.raises(Cut):
        tr.train()
    new = torch.load(str(tmp_path / "cut" / "run_state.pt"), weights_only=True)
    assert list(new) == list(gold) and list(new["host"]) == list(gold["host"])
    assert list(R.payload_tensors(new)) == list(R.payload_tensors(gold))
    assert _tensor_specs(new) == _tensor_specs(gold) and len(_tensor_specs(R.payload_tensors(gold))) == len(R.payload_tensors(gold))
