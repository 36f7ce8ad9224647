"""Records the host-side dispatch answers of libunetmi over tests/dispatch_grid.py -> tests/golden/dispatch_table.npz.

The fixture pins the answers of the commit BEFORE a change to the dispatch code, so point UMI_LIB_OVERRIDE at a library built
from that commit:

    UMI_LIB_OVERRIDE=/path/to/parent/libunetmi.so python tools/gen_dispatch_table.py

Runs on the CPU (plan and bounds functions launch nothing)."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "unet-torch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from tests import dispatch_grid  # noqa: E402
from umi import lib  # noqa: E402

if __name__ == "__main__":
    t = dispatch_grid.tables(lib.fn)
    out = os.path.join(REPO, "tests", "golden", "dispatch_table.npz")
    np.savez_compressed(out, **t)
    plan = t["plan"]
    print("library:", os.environ.get("UMI_LIB_OVERRIDE", "(in-tree)"))
    print("plan queries", len(plan), "UMI_ERR_UNSUPPORTED", int((plan[:, 0] == -2).sum()), "layout 1", int((plan[:, 1] == 1).sum()))
    print("wgrad_ws queries", t["wgrad_ws"].size, "distinct", len(np.unique(t["wgrad_ws"])))
    print("wrote", out, os.path.getsize(out), "bytes")
