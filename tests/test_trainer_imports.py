"""What `import Trainer` and a Trainer with every keyword at its default load: no `umi.*` module and no matplotlib at import,
and after a one-epoch CPU run no `umi.*` module beyond those the same run loaded before the Trainer was split into
umi/run_state.py, umi/val_batch.py and umi/dp_run.py (the 'dice_bce_mc' loss asks umi.ddp for the active batch sync)."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# measured at the commit before the split, with the script below
LOADED_BEFORE_THE_SPLIT = {"umi", "umi.ddp"}

SCRIPT = r"""
import json, os, sys, tempfile
repo = sys.argv[1]
sys.path[:0] = [repo, os.path.join(repo, "unet-torch_amd")]
os.environ.setdefault("MPLBACKEND", "Agg")
umi = lambda: sorted(k for k in sys.modules if k == "umi" or k.startswith("umi."))
import Trainer
at_import = umi() + sorted(k for k in sys.modules if k.split(".")[0] == "matplotlib")
import torch
import loss as L
from oracle import ref_unet
from torch.utils.data import DataLoader, TensorDataset
L.CLASS_NUMBER = 2
torch.manual_seed(0)
m = ref_unet.RefUNet(1, 2, 2, False)
x, lab = torch.randn(4, 1, 32, 32), torch.randint(0, 2, (4, 32, 32)).float()
loaders = {"train": DataLoader(TensorDataset(x[:2], lab[:2]), batch_size=2), "val": DataLoader(TensorDataset(x[2:], lab[2:]), batch_size=2)}
opt = torch.optim.SGD(m.parameters(), lr=0.05, momentum=0.9)
with tempfile.TemporaryDirectory() as d:
    tr = Trainer.Trainer(m, "single", torch.FloatTensor, "cpu", d, loaders, 2, opt, 25, 1, "dice_bce_mc", "dice_bce_mc")
    tr.train()
    assert len(tr.val_loss_list) == 1
print("RESULT " + json.dumps(dict(at_import=at_import, after_run=umi())))
"""


def test_import_and_default_run_load_no_new_module():
    r = subprocess.run([sys.executable, "-c", SCRIPT, REPO], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    assert got["at_import"] == []
    assert set(got["after_run"]) <= LOADED_BEFORE_THE_SPLIT, got["after_run"]
