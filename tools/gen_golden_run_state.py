#!/usr/bin/env python3
"""Generate tests/golden/run_state_v1.pt: the run-state file (format 1) that `Trainer(resume=True)` writes on the CPU in the
setting of tests/test_snapshot.py's `_cut_run` -- RefUNet(1, 2, FEAT) at 32 x 32, SGD with momentum and the poly rule, every
generator seeded with 5, the run cut when epoch 3 is about to start, so the file holds the state after epoch 2 of 4.  The
setting itself is read from tests/test_snapshot.py (`_trainer`, `_seed_everything`, `Cut`), so it is written once.

The file pins the format across changes of the Trainer: tests/test_snapshot.py recomputes its two fingerprint words, resumes
from a copy of it and compares the layout of a freshly written file with it.  Regenerate it only when RUN_STATE_FORMAT
changes (then under a new name, the old file stays readable or is refused by its format number).

FEAT = 2 gives 486 KB (weights, momentum buffers and the best model: three copies of the state); FEAT = 4 gives 1.6 MB, over the limit for a committed file.

Usage:  python tools/gen_golden_run_state.py
"""
import importlib.util
import os
import shutil
import sys
import tempfile

sys.dont_write_bytecode = True
os.environ.setdefault("MPLBACKEND", "Agg")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "unet-torch_amd")):
    sys.path.insert(0, p)
GOLD = os.path.join(REPO, "tests", "golden")
FEAT = 2


def setting():
    spec = importlib.util.spec_from_file_location("test_snapshot", os.path.join(REPO, "tests", "test_snapshot.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import torch
    T = setting()
    with tempfile.TemporaryDirectory() as d:
        T._seed_everything()
        tr, m, opt = T._trainer(d, cut_at=3, resume=True, feat=FEAT)
        try:
            tr.train()
            raise SystemExit("the run was not cut")
        except T.Cut:
            pass
        path = os.path.join(d, "run_state.pt")
        pl = torch.load(path, weights_only=True)
        assert pl["format"] == 1 and pl["epoch"] == 2 and pl["over"] is False
        shutil.copyfile(path, os.path.join(GOLD, "run_state_v1.pt"))
        print("wrote run_state_v1.pt:", os.path.getsize(path), "bytes, epoch", pl["epoch"], "word", hex(pl["word"]),
              "host_word", hex(pl["host_word"]), "train", pl["host"]["lists"]["train_loss_list"])


if __name__ == "__main__":
    main()
