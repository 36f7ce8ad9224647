"""A census of the benchmark's training step: every C-ABI call that UNet(1,2,64) and UNet(3,4,64) make in one fp16 step at
2 x 512 x 512 must be a call that a pinning test makes, argument for argument.

The step: forward, calc_loss(..., "dice_bce_mc"), backward, umi.optim.SGD(lr 0.01, momentum 0.9, weight decay 1e-4).step(), and a
second forward (the weight re-pack), train mode, default environment.  umi.lib.call / supported / fn are wrapped (tests/abi_calls.py),
so every call through the binding is seen; the device kernel names of the same step (torch.profiler) are then mapped back to entry
points: a library kernel that ran without a recorded entry point that launches it fails the test.

A call's key (abi_calls.key) is the entry point, every integer and float scalar by name and the set of null addresses, batch aside
(N dropped, rows per image).  Keyed are the entry points that take a stream, i.e. that launch work; the others (umi_conv_fwd_plan,
umi_*_rows, umi_*_ws_bytes, umi_*_block_elems) are host functions of integers that size the buffers of a keyed call, and the pinning
tests call them with the same integers to size theirs.  The pinned keys come from the case tables of the pinning tests:
tests/test_gpu_unet_step_exact.py (each of its tests asserts that it made the calls its case lists), SHAPES of
tests/test_gpu_exact_fullsize.py and LEVELS of tests/test_gpu_bn_apply_stream.py.  Entry points whose arguments are a descriptor
table are exempt from keying: EXEMPT names the test that covers each."""
import collections
import glob
import importlib
import os
import re
import subprocess
import sys

import pytest
import torch

from tests import abi_calls as A
from tests import test_gpu_unet_step_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH, SIZE = 2, 512
CONFIGS = [(1, 2), (3, 4)]

# entry point -> the test that covers it (its arguments are a table of descriptors, not a geometry)
EXEMPT = {
    "umi_optim_sgd_multi": "tests.test_gpu_kernels::test_optim_sgd_matches_torch",
    "umi_pack_kn_multi": "tests.test_gpu_kernels::test_pack_cache_multi_repack_is_bit_identical_to_single_packs",
    "umi_table_upload": "tests.test_gpu_kernels::test_pack_cache_multi_repack_is_bit_identical_to_single_packs",
    "umi_wgrad_reduce_group": "tests.test_gpu_wgrad_reduce::test_grouped_reduction_on_synthetic_slabs",
}

# library kernel -> the entry points of this step that launch it
KERNEL_ENTRIES = {
    "stem3x3_fwd_kernel": ("umi_conv_fwd",),
    "head1x1_fwd_kernel": ("umi_conv_fwd",),
    "conv3x3_mfma_kernel": ("umi_conv_fwd", "umi_conv_dgrad_bnred"),
    "conv1x1_mfma_kernel": ("umi_conv_fwd", "umi_conv_gather_bnred"),
    "bn_finalize_kernel": ("umi_bn_finalize",),
    "bn_finalize2d_kernel": ("umi_bn_finalize",),
    "pool2_fwd_v8": ("umi_pool2_fwd",),
    "pool2_bwd_v8": ("umi_pool2_bwd_bnred",),
    "dice_ce_stats_kernel": ("umi_dice_ce_fwd",),
    "dice_ce_finalize_kernel": ("umi_dice_ce_fwd",),
    "dice_ce_bwd_kernel": ("umi_dice_ce_bwd",),
    "smallk1x1_bnred_kernel": ("umi_head_bwd_fused",),
    "head_wpart_reduce_kernel": ("umi_head_bwd_fused",),
    "colsum_v8": ("umi_colsum",),
    "fold_cols_kernel": ("umi_colsum",),
    "reduce_rows2_kernel": ("umi_bn_bwd_from_partials",),
    "reduce_rows2_2d_kernel": ("umi_bn_bwd_from_partials",),
    "reduce_rows2_wide_kernel": ("umi_bn_bwd_from_partials",),
    "bn_bwd_apply_v8": ("umi_bn_bwd_apply",),
    "wgrad3x3_ws_kernel": ("umi_conv_wgrad_deferred", "umi_conv_wgrad_bnapply"),
    "wgrad3x3_mfma_kernel": ("umi_conv_wgrad_deferred", "umi_conv_wgrad_bnapply"),
    "stem3x3_wgrad_kernel": ("umi_conv_wgrad_bnapply",),
    "wgrad_reduce_kernel": ("umi_conv_wgrad_bnapply",),
    "wgrad_reduce_v4_kernel": ("umi_conv_wgrad_bnapply",),
    "wgradT2x2_mfma_kernel": ("umi_conv_wgrad_bias",),
    "wgrad_reduce_group_kernel": ("umi_wgrad_reduce_group",),
    "pack_kn_kernel": ("umi_pack_kn", "umi_pack_kn8"),
    "pack_multi_kernel": ("umi_pack_kn_multi",),
    "table_upload_kernel": ("umi_table_upload",),
    "optim_multi_kernel": ("umi_optim_sgd_multi",),
}


def _library_kernels():
    """Names of the __global__ functions of csrc/."""
    names = set()
    pat = re.compile(r"__global__\s+(?:__launch_bounds__\s*\((?:[^()]|\([^()]*\))*\)\s*)?(?:static\s+)?void\s+(\w+)\s*\(", re.S)
    n_global = 0
    for path in glob.glob(os.path.join(REPO, "unet-torch_amd", "csrc", "*.hip")) + glob.glob(
            os.path.join(REPO, "unet-torch_amd", "csrc", "*.h")):
        with open(path) as f:
            text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", f.read(), flags=re.S)
        n_global += len(re.findall(r"__global__", text))
        names.update(pat.findall(text))
    assert len(names) > 100 and n_global < 1.5 * len(names) + 20, (len(names), n_global)      # the pattern reads the sources
    return names


def _kernel_of(event_name, kernels):
    """The library kernel an event of the profile is, or None (a torch kernel, a runtime call); a name in the library's
    anonymous namespace that csrc/ does not define raises."""
    for k in kernels:
        if f"{len(k)}{k}" in event_name or re.search(rf"(?<!\w){re.escape(k)}[(<]", event_name):
            return k
    if event_name.startswith(("_ZN12_GLOBAL__N_1", "(anonymous namespace)::", "void (anonymous namespace)::")):
        raise AssertionError(f"a kernel of an anonymous namespace that csrc/ does not define: {event_name[:160]}")
    return None


def _existing_specs():
    """The calls that the tables of the earlier bench-size tests pin with the step's own arguments."""
    from tests import test_gpu_bn_apply_stream as S
    from tests import test_gpu_exact_fullsize as E
    out = []
    for n, H, W, Ci, Co in E.SHAPES:
        if n != BATCH or H != W:
            continue
        # test_conv3x3_forward_and_stat_rows_exact_at_bench_size: dense tensors, a transform on load unless 128 -> 128
        out += [X.spec_conv_fwd(H, Ci, Co, Ci, Co, (Ci, Co) != (128, 128), True), X.spec_pack("conv_fwd", (Co, Ci, 3, 3), True),
                X.spec_finalize(X._conv_rows(H, Co), Co, H * W)]
        # test_conv3x3_dgrad_and_fused_bn_rows_exact_at_bench_size: the plain data gradient Co -> Ci it also runs
        out += [X.spec_conv_fwd(H, Co, Ci, Co, Ci, False, False), X.spec_pack("conv_dgrad", (Co, Ci, 3, 3), True)]
    for M, C in S.LEVELS:                                  # test_stream_apply_matches_generic_on_unet_levels: dense, M = 2 H W
        out.append(X._spec("umi_bn_bwd_apply", ldda=C, ldy=C, M=M // BATCH, C=C, dtype=X.F16))
    return out


def _pinned_keys():
    return {X.key_of(s) for s in X.all_specs() + _existing_specs()}


def _make_step(cin, ncls):
    import Model
    import loss as L
    from oracle import recipe
    from umi import optim
    L.CLASS_NUMBER = ncls
    torch.manual_seed(0)
    m = Model.UNet(cin, ncls, 64, compute_dtype="fp16").to(DEV).train()
    opt = optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    x, lab = recipe.synthetic_batch(BATCH, cin, SIZE, SIZE, ncls, seed=1)
    x, lab = x.to(DEV), lab.to(DEV)

    state = {}

    def forward_and_loss():
        state["loss"] = L.calc_loss(m(x), lab, loss_type="dice_bce_mc")

    def backward():
        state["loss"].backward()

    def update_and_forward():
        opt.step()
        m(x)

    def run():
        for part in run.parts:
            part()
        torch.cuda.synchronize()
        return state["loss"].item()
    run.parts = (forward_and_loss, backward, update_and_forward)
    return run


def test_exempt_entry_points_name_existing_tests():
    assert len(EXEMPT) <= 10
    for entry, test in EXEMPT.items():
        mod, name = test.split("::")
        assert callable(getattr(importlib.import_module(mod), name)), (entry, test)


def test_loss_scale_of_the_pinned_weight_gradients():
    from umi import graph as G
    assert 1.0 / G.default_loss_scale(torch.float16, BATCH * SIZE * SIZE) == X.OUT_SCALE


@pytest.mark.parametrize("cin,ncls", CONFIGS)
def test_every_call_of_the_step_is_pinned(cin, ncls, monkeypatch):
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    knobs = sorted(k for k in os.environ if k.startswith("UMI_"))
    assert not knobs, f"the census describes the default step; unset {knobs}"
    pinned = _pinned_keys()
    run = _make_step(cin, ncls)
    rec = A.Recorder(monkeypatch)
    assert run() > 0.0                                     # (a first step: individual weight packs, first_step = 1)
    calls = list(rec.calls)

    # ---- every launching call is pinned ------------------------------------------------------------------------------
    launching = [(e, v, st) for e, v, st in calls if "stream" in dict(A.params(e))]
    refused = [e for e, v, st in launching if st != 0]
    assert not refused, f"calls of the default step that the library refused (a fusion not taken): {refused}"
    seen = collections.Counter(A.key(e, v, BATCH) for e, v, st in launching if e not in EXEMPT)
    print(f"[census] UNet({cin},{ncls},64): {len(launching)} launching calls, {len(seen)} distinct keys, {len(pinned)} pinned keys")
    missing = sorted(A.show(k) for k in seen if k not in pinned)
    assert not missing, (f"{len(missing)} of {len(seen)} kernel calls of UNet({cin},{ncls},64)'s step are not pinned by any case "
                         "table:\n  " + "\n  ".join(missing))
    assert len(seen) > 100, len(seen)
    for e in EXEMPT:
        assert any(c[0] == e for c in calls), f"exempt entry point {e} is no longer called: drop it from EXEMPT"

    # ---- the fusions the tape is written to take ---------------------------------------------------------------------
    by = collections.defaultdict(list)
    for e, v, st in launching:
        by[e].append(v)
    assert len(by["umi_conv_dgrad_bnred"]) == 9 and len(by["umi_conv_gather_bnred"]) == 4 and len(by["umi_conv_wgrad_bias"]) == 4
    assert len(by["umi_head_bwd_fused"]) == 1 and not by["umi_head_dgrad_bnred"]
    assert len(by["umi_pool2_bwd_bnred"]) == 4
    assert all(v["accumulate"] == 1 and v["ldda"] == 2 * v["C"] == v["ldx"] for v in by["umi_pool2_bwd_bnred"])
    assert len(by["umi_conv_wgrad_bnapply"]) == 4 and sum(not v["dz"] for v in by["umi_conv_wgrad_bnapply"]) == 1
    assert [v["Ci"] for v in by["umi_conv_wgrad_bnapply"] if not v["dz"]] == [cin]            # the stem
    for e in ("umi_bn_bwd_reduce", "umi_pool2_bwd", "umi_conv_wgrad", "umi_bn_stats"):
        assert not by[e], f"{e}: the separate pass of a fusion the default step takes"

    # ---- the wrapping sees every launch: kernel names of the next step against its recorded entry points -------------------
    from torch.profiler import ProfilerActivity, profile
    del rec.calls[:]
    kernels = _library_kernels()
    ran = collections.Counter()
    for part in run.parts:                                 # one short trace per part of the step: a long one drops events here
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            part()
            torch.cuda.synchronize()
        ran.update(k for k in (_kernel_of(ev.name, kernels) for ev in prof.events()) if k)
    entries = {e for e, v, st in rec.calls}
    # (the trace may still be incomplete: the check is that no kernel it does show lacks an entry point, not that it shows all)
    assert len(ran) >= 5, sorted(ran)                      # the profile did see the library's kernels
    unknown = sorted(k for k in ran if k not in KERNEL_ENTRIES)
    assert not unknown, f"library kernels of the step that KERNEL_ENTRIES does not attribute to an entry point: {unknown}"
    orphan = sorted(k for k in ran if not entries & set(KERNEL_ENTRIES[k]))
    assert not orphan, f"library kernels that ran without a recorded entry point: {orphan}"


def test_default_step_runs_no_generic_conv_kernel():
    """UMI_TRACE_GENERIC=1 is read once per process: a child runs the step of both configurations."""
    if not torch.cuda.is_available():
        pytest.fail("needs an MI355X")
    code = ("import sys; sys.path[:0] = [%r, %r]\n"
            "from tests.test_gpu_unet_step_calls import CONFIGS, _make_step\n"
            "for c in CONFIGS:\n    print('STEP_LOSS', _make_step(*c)())\n") % (REPO, os.path.join(REPO, "unet-torch_amd"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, UMI_TRACE_GENERIC="1"), cwd=REPO)
    assert r.returncode == 0 and r.stdout.count("STEP_LOSS") == len(CONFIGS), (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    lines = [l for l in r.stderr.splitlines() if "[umi generic" in l]
    assert not lines, lines[:8]
