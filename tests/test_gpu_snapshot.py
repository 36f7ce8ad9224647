"""umi_snapshot_multi / umi_restore_multi and umi.snapshot.Snapshot on the MI355X against the NumPy statement
(umi.snapshot.snapshot_numpy, umi.ddp.fingerprint_numpy), bit for bit: block and vector edges, aligned and misaligned sources
and destinations, empty neighbours, zero pads, canaries around everything that is written.  Then the Trainer on top of them:
a run cut after epoch 2 and resumed (new objects; one case in a fresh process) against the run that was never cut, the in-place
roll-back under graph=True, and asynchronous checkpoints against the synchronous files.  The runs are tools/check_resume.py's."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COUNTS = (0, 1, 3, 4, 5, 4095, 4096, 4097, 8193)         # 32-bit words: the vector (4) and block (4,096) edges
DTYPES = (torch.float32, torch.int64, torch.int32, torch.uint8, torch.float64)
GUARD = 8                                                # words kept around every source, destination and the arena
MASK = (1 << 64) - 1


def _source(rng, words, dtype, shifted):
    """A device tensor of `words` 32-bit words of random bits with dtype `dtype`, cut out of a larger random buffer `shifted`
    floats (0, 1 or 2) past a 16-byte boundary.  Returns (tensor, its words on the host)."""
    host = rng.integers(0, 2 ** 32, size=words + 2 * GUARD, dtype=np.uint64).astype(np.uint32)
    buf = torch.from_numpy(host.view(np.int32)).cuda()
    at = GUARD + shifted
    t = buf[at:at + words].view(dtype)
    assert (not words or t.data_ptr() % 16 == 4 * shifted) and t.numel() * t.element_size() == 4 * words     # (empty: no pointer)
    return t, host[at:at + words]


def _table(rows):
    """Device umi_optim_desc table of rows (p, s0, n); returns (table, total_blocks)."""
    from umi import lib as L, ops
    blk = L.fn("umi_optim_block_elems")()
    arr = np.zeros(len(rows), dtype=ops.OPTIM_DESC)
    b0 = 0
    for i, (p, s0, n) in enumerate(rows):
        arr[i] = (p, 0, s0, 0, n, b0, 0)
        b0 += (n + blk - 1) // blk
    return torch.from_numpy(arr.view(np.uint8).reshape(-1).copy()).cuda(), b0


def _draw(seed):
    """[(words, dtype, shifted)] of one random table of one to twelve tensors."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(int(rng.integers(1, 13))):
        words = int(rng.choice(COUNTS))
        ok = [d for d in DTYPES if (4 * words) % torch.empty(0, dtype=d).element_size() == 0]
        dtype = ok[int(rng.integers(0, len(ok)))]
        # one float past a 16-byte boundary; two for the 8-byte dtypes (torch wants a tensor aligned to its element)
        out.append((words, dtype, int(rng.integers(0, 2)) * max(1, torch.empty(0, dtype=dtype).element_size() // 4)))
    return out


TABLES = {
    # two neighbouring empty tensors between non-empty ones (equal blk0: the last of them owns the block), an empty one first
    # and last, every count once, 8-byte dtypes, shifted and unshifted sources
    "edges": [(0, torch.float32, 0), (4097, torch.float32, 1), (0, torch.int32, 0), (0, torch.float64, 0), (5, torch.int32, 1),
              (4096, torch.float64, 0), (4095, torch.uint8, 1), (8193, torch.float32, 0), (1, torch.int32, 1), (3, torch.uint8, 0),
              (4, torch.int64, 0), (0, torch.float32, 1)],
    "one_word": [(1, torch.float32, 1)],
    "only_empty": [(0, torch.float32, 0), (0, torch.float32, 0)],
}
TABLES.update({f"single_{w}_{s}": [(w, torch.float32, s)] for w in COUNTS[1:] for s in (0, 1)})
TABLES.update({f"random_{s}": _draw(s) for s in range(4)})


@pytest.mark.parametrize("name", sorted(TABLES))
def test_snapshot_and_restore_against_numpy(name):
    from umi import ddp, lib as L, ops, snapshot as S
    spec = TABLES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    srcs = [_source(rng, w, d, s) for w, d, s in spec]
    host = [h for _, h in srcs]
    offsets, total = S.layout([h.size for h in host])
    want_arena, want_word = S.snapshot_numpy(host)
    assert want_word == ddp.fingerprint_numpy(host)

    # the arena between two canaries, everything preset to 0xFF: the pads must come out 0, the canaries stay
    buf = torch.full((total + 2 * GUARD,), -1, dtype=torch.int32, device="cuda")
    arena = buf[GUARD:GUARD + total]
    base = arena.data_ptr() if total else buf.data_ptr() + 4 * GUARD
    assert base % 16 == 0
    table, blocks = _table([(t.data_ptr(), base + 4 * off, h.size) for (t, h), off in zip(srcs, offsets)])
    ws = torch.empty(max(blocks, 1), dtype=torch.int64, device="cuda")
    out = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    assert L.fn("umi_snapshot_ws_bytes")(blocks) == 8 * blocks
    L.call("umi_snapshot_multi", table.data_ptr(), len(srcs), blocks, ws.data_ptr(), ws.numel() * 8, out.data_ptr(), ops._stream())
    L.call("umi_fingerprint_multi", table.data_ptr(), len(srcs), blocks, ws.data_ptr(), ws.numel() * 8, out.data_ptr() + 8,
           ops._stream())
    got = buf.cpu().numpy().view(np.uint32)
    assert (got[:GUARD] == 0xFFFFFFFF).all() and (got[GUARD + total:] == 0xFFFFFFFF).all()
    assert (got[GUARD:GUARD + total] == want_arena).all()
    words = [int(v) & MASK for v in out.tolist()]
    assert words[0] == want_word and words[1] == want_word
    for (t, h) in srcs:                                   # the sources were only read
        assert (t.reshape(-1).view(torch.int32).cpu().numpy().view(np.uint32) == h).all()

    # restore into fresh destinations, aligned and one float past alignment, each inside a patterned buffer
    for shifted in (0, 1):
        dbufs = [torch.full((h.size + 2 * GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for h in host]
        rows = [(d.data_ptr() + 4 * (GUARD + shifted), base + 4 * off, h.size) for d, h, off in zip(dbufs, host, offsets)]
        assert all(r[0] % 16 == 4 * shifted for r in rows)
        rtable, rblocks = _table(rows)
        assert rblocks == blocks
        L.call("umi_restore_multi", rtable.data_ptr(), len(rows), rblocks, ops._stream())
        for d, h in zip(dbufs, host):
            g = d.cpu().numpy().view(np.uint32)
            at = GUARD + shifted
            assert (g[at:at + h.size] == h).all()
            assert (g[:at] == 0x5A5A5A5A).all() and (g[at + h.size:] == 0x5A5A5A5A).all()     # nothing before, nothing past
    assert (buf.cpu().numpy().view(np.uint32)[GUARD:GUARD + total] == want_arena).all()       # restore only reads the arena


def test_empty_table_writes_zero_and_restores_nothing():
    from umi import lib as L, ops
    out = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    L.call("umi_snapshot_multi", None, 0, 0, None, 0, out.data_ptr(), ops._stream())
    assert int(out.item()) == 0
    L.call("umi_restore_multi", None, 0, 0, ops._stream())


def _state(seed=3):
    g = torch.Generator().manual_seed(seed)
    return {"w": torch.randn(3, 4097, generator=g).cuda(), "steps": torch.arange(3).cuda(), "empty": torch.zeros(0).cuda(),
            "mask": torch.randint(0, 255, (8,), generator=g, dtype=torch.uint8).cuda(),
            "shifted": torch.randn(4102, generator=g).cuda()[1:4098], "d": torch.randn(5, generator=g, dtype=torch.float64).cuda()}


def test_snapshot_class_views_verify_restore():
    from umi import ddp, snapshot as S
    st = _state()
    keep = {k: v.clone() for k, v in st.items()}
    snap = S.Snapshot(st).take()
    arena, word = S.snapshot_numpy([v.cpu().numpy() for v in st.values()])
    assert snap.word() == word == ddp.fingerprint(list(st.values()))
    assert (snap.arena.cpu().numpy().view(np.uint32) == arena).all()
    views = snap.views()
    assert list(views) == list(st)
    for k, v in views.items():
        assert v.dtype == st[k].dtype and v.shape == st[k].shape and torch.equal(v, keep[k])
    assert snap.verify()
    ptrs = [v.data_ptr() for v in st.values()]
    for v in st.values():
        v.zero_()
    versions = [v._version for v in st.values()]
    snap.restore()
    assert [v.data_ptr() for v in st.values()] == ptrs
    assert all(v._version > v0 for v, v0 in zip(st.values(), versions))           # the restore bumps: PackCache re-packs
    for k, v in st.items():
        assert torch.equal(v, keep[k])
    # one flipped bit of the arena: restore() raises and writes nothing
    for v in st.values():
        v.zero_()
    snap.arena.view(torch.int32)[4100] ^= 1 << 7
    assert not snap.verify()
    with pytest.raises(RuntimeError, match="nothing was restored"):
        snap.restore()
    assert all(not bool(v.any()) for v in st.values())
    with pytest.raises(ValueError, match="tensor 1"):
        S.Snapshot([torch.zeros(4).cuda(), torch.zeros(6, dtype=torch.uint8).cuda()])
    with pytest.raises(ValueError, match="tensor 0 is not contiguous"):
        S.Snapshot([torch.zeros(4, 4).cuda().t()])


def test_second_take_waits_for_the_copy_in_flight():
    """take(), to_host_async(), change the tensors, take() again at once: the host copy must hold the FIRST state whole (the
    second take's stream waited for the copy), the arena the second."""
    from umi import snapshot as S
    g = torch.Generator().manual_seed(9)
    big = torch.randn(1 << 22, generator=g).cuda()                      # 16 MiB: a copy that is not over at once
    st = {"big": big, "small": torch.arange(5, dtype=torch.float32).cuda()}
    first = {k: v.clone() for k, v in st.items()}
    snap = S.Snapshot(st).take()
    word1 = snap.word()
    ev = snap.to_host_async()
    big.mul_(-3.0)
    st["small"].add_(1.0)
    snap.take()
    ev.synchronize()
    host = snap.host_views()
    assert all(torch.equal(host[k], first[k].cpu()) for k in st)
    assert snap.word() != word1 and snap.verify()
    assert all(torch.equal(snap.views()[k], st[k]) for k in st)


# ---- Trainer: cut and resumed against never cut --------------------------------------------------------------------------------

CHILD_CASE = "fp16_graph_sgd"                    # resumed in a fresh process; the others with new objects in this one


def _seed_everything(seed=5):
    import random
    torch.manual_seed(seed)
    random.seed(seed)
    np.random.seed(seed)


def _whole(case, out, **flags):
    from tools import check_resume as C
    _seed_everything()
    tr, m, opt = C.build(case, out, **flags)
    tr.train()
    assert len(tr.train_loss_list) == C.EPOCHS and tr.iter_num == 2 * C.EPOCHS
    return C.summary(tr, m, opt, out)


def _cut(case, out, **flags):
    from tools import check_resume as C
    _seed_everything()
    tr, m, opt = C.build(case, out, cut_at=3, resume=True, **flags)
    with pytest.raises(C.Cut):
        tr.train()
    assert len(tr.train_loss_list) == 2 and os.path.exists(os.path.join(out, "run_state.pt"))
    assert not [f for f in os.listdir(out) + os.listdir(os.path.join(out, "models")) if f.endswith(".tmp")]
    return tr


@pytest.mark.parametrize("case", ["fp32_eager_sgd", "fp16_graph_sgd", "fp32_graph_adam", "fp16_eager_adam", "dropout", "guard",
                                  "multitask"])
def test_cut_and_resumed_run_equals_the_whole_run(tmp_path, case):
    from tools import check_resume as C
    whole = _whole(case, tmp_path / "whole")                          # both flags off
    graph = C.CASES[case][1]
    assert whole["graphs"] == (1 if graph else 0)
    if case == "guard":                                               # the scale moved before the cut: one skipped step
        from umi.optim import GUARD
        assert whole["guard"][GUARD["SKIPPED"]] == 1 and whole["guard"][GUARD["SCALE"]] == 0.5
    if case == "dropout":
        assert whole["drops"] and all(int(step) == 2 * C.EPOCHS for _, step in whole["drops"].values())
    out = tmp_path / "cut"
    cut = _cut(case, out)
    pl = torch.load(out / "run_state.pt", weights_only=True)
    assert pl["epoch"] == 2 and pl["over"] is False and pl["host"]["iter_num"] == 4
    assert (pl["hyper"] is not None) == bool(cut.optimizer.device_hyper) and (pl["guard"] is not None) == (case == "guard")
    if case == CHILD_CASE:
        del cut
        done = subprocess.run([sys.executable, os.path.join(REPO, "tools", "check_resume.py"), case, str(out),
                               str(tmp_path / "summary.pt")], capture_output=True, text=True, timeout=240)
        assert done.returncode == 0, done.stdout[-2000:] + done.stderr[-4000:]        # (nothing more runs here if it failed)
        resumed = torch.load(tmp_path / "summary.pt", weights_only=False)
    else:
        _seed_everything(999)                                         # the file's generator states must replace these
        tr, m, opt = C.build(case, out, past_cut=True, resume=True)
        tr.train()
        resumed = C.summary(tr, m, opt, out)
    assert resumed["graphs"] == whole["graphs"]
    assert C.same(whole, resumed) is None, C.same(whole, resumed)
    assert torch.load(out / "run_state.pt", weights_only=True)["over"] is True


# ---- Trainer: roll-back in place under graph=True ------------------------------------------------------------------------------

def test_roll_back_in_place_keeps_the_graphs_and_repacks_the_weights(tmp_path):
    import Model
    from tools import check_resume as C
    _seed_everything()
    tr, m, opt = C.build("fp16_graph_sgd", tmp_path)
    g = torch.Generator().manual_seed(7)
    x, lab = torch.randn(6, 1, 32, 32, generator=g), torch.randint(0, 2, (6, 32, 32), generator=g).float()
    batches = [(x[0:2], lab[0:2]), (x[2:4], lab[2:4])]

    def epoch():
        m.train()
        return [float(tr.train_step(*b)) for b in batches]

    epoch(), epoch()
    snap = tr.snapshot_run_state()
    graphs, ptrs = dict(tr._graphs), [p.data_ptr() for p in m.parameters()]
    assert len(graphs) == 1
    kept = {k: v.clone() for k, v in snap.views().items() if k.startswith("model.")}
    first = (epoch(), {k: v.clone() for k, v in m.state_dict().items()}, tr.iter_num, opt.state_dict()["param_groups"][0]["lr"])
    tr.restore_run_state()
    assert tr.iter_num == 4 and [p.data_ptr() for p in m.parameters()] == ptrs
    # a forward right after the restore runs on re-packed weights: the output of a fresh model loaded from the snapshot
    m.eval()
    fresh = Model.UNet(1, 2, 8, False, compute_dtype="fp16").to(C.DEV).eval()
    fresh.load_state_dict({k[len("model."):]: v for k, v in kept.items()})
    with torch.no_grad():
        assert torch.equal(m(x[4:].to(C.DEV)), fresh(x[4:].to(C.DEV)))
    second = (epoch(), {k: v.clone() for k, v in m.state_dict().items()}, tr.iter_num, opt.state_dict()["param_groups"][0]["lr"])
    assert first[0] == second[0] and first[2:] == second[2:]
    assert all(torch.equal(first[1][k], second[1][k]) for k in first[1])
    assert tr._graphs == graphs and all(tr._graphs[k] is graphs[k] for k in graphs)          # none captured again
    assert not torch.equal(first[1]["inc.double_conv.0.weight"], kept["model.inc.double_conv.0.weight"])   # (the epoch did train)


# ---- Trainer: asynchronous checkpoints -----------------------------------------------------------------------------------------

def test_async_checkpoints_write_the_files_of_the_synchronous_path(tmp_path):
    from tools import check_resume as C
    sync = _whole("fp32_graph_adam", tmp_path / "sync")
    both = _whole("fp32_graph_adam", tmp_path / "async", async_checkpoints=True, resume=True)
    assert C.same(sync, both) is None, C.same(sync, both)
    assert sorted(sync["files"]) == sorted(both["files"]) and {"best.pt", "last_epoch.pt"} <= set(sync["files"])
    for name in sync["files"]:
        a_path, b_path = tmp_path / "sync" / "models" / name, tmp_path / "async" / "models" / name
        a = torch.load(a_path, map_location="cpu", weights_only=True)
        b = torch.load(b_path, map_location="cpu", weights_only=True)
        assert list(a) == list(b), name
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(a[k], b[k]), (name, k)
        sa, sb = os.path.getsize(a_path), os.path.getsize(b_path)
        assert abs(sa - sb) <= 0.01 * sa, (name, sa, sb)               # no tensor drags the arena's storage into the file
    left = [f for d in ("", "models") for f in os.listdir(tmp_path / "async" / d) if f.endswith(".tmp")]
    assert not left                                                    # train() joined the writer


def test_async_checkpoint_that_cannot_be_written_raises_from_train(tmp_path):
    from tools import check_resume as C
    _seed_everything()
    tr, m, opt = C.build("fp32_eager_sgd", tmp_path, async_checkpoints=True)
    os.rmdir(tmp_path / "models")
    (tmp_path / "models").write_text("not a directory")               # every file under models/ is unwritable now
    with pytest.raises((OSError, RuntimeError), match="models"):
        tr.train()
    assert tr._run.writer is None                                          # joined and closed all the same
