"""GPU: the evaluation path's fault words and read-backs do not depend on what the shared workspace holds between calls.

A labelling, dot-list or peak-list call leaves a status word (list overflow, a mask value >= n_classes, a union-find that gave
up: data conditions, not GPU faults) in the first 4 bytes of `ops.workspace`, the scratch buffer every op shares.  The rule
(binary inference): the function that launched the kernel clones the word right after its own call
(`ops.fault_word`), nothing returns a view of the workspace and nothing reads it across calls.  So
  1. a word taken with `_fault=True` keeps its value when the whole workspace is overwritten afterwards;
  2. every scoring chain gives the same result under tests/poison.py's 0x00 and 0xFF, and that result is the host statement's;
  3. every chain still does exactly one device-to-host copy;
  4. the graphed predictors leave the training flag alone (also when the first eager run raises) and replay the eager call.
All inputs are tiny: two 70 x 130 masks (the labelling's 64-pixel tiles have seams both ways), the smallest fixture cases."""
import os

import numpy as np
import pytest
import torch

from oracle import recipe
from tests import poison
from tests.test_gpu_crowd_matching import _score_numpy
from tests.test_gpu_peaks import _cells_clear_of_integers, _compare_scores, _scene, _sum_bound
from tools import gen_golden_binary_infer as GB
from tools import gen_golden_crowd_matching as GC
from tools import gen_golden_multiclass_eval as GM

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W = 70, 130
SIZE = 128                                        # GAME grid: 16-pixel cells, clipped to the 70 x 130 image


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: torch.cuda.is_available() is False")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _blobs():
    """Two 70 x 130 images: 0/1 discs, the discs' classes (1, 2) and a float32 dot map with a dot near most discs."""
    masks, classes, dots = [], [], []
    for seed in (71, 72):
        m, cy, cx, _ = GM.blob_classes(seed, (H, W), 3, 14)
        g = np.zeros((H, W), dtype=np.float32)
        g[np.clip(cy[2:] + 1, 0, H - 1), np.clip(cx[2:] - 1, 0, W - 1)] = 1
        masks.append((m != 0).astype(np.uint8))
        classes.append(m)
        dots.append(g)
    return np.stack(masks), np.stack(classes), np.stack(dots)


def _same(a, b):
    """Equal values of equal types, through dicts, lists and tuples; arrays by dtype and content (NaN == NaN)."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
    return type(a) is type(b) and (a == b or (a != a and b != b))


# ---- 1. the word survives foreign use of the workspace ---------------------------------------------------------------------------
def _fault_cases():
    from umi import infer, matching as M, peaks as P
    from umi.components import label_class_components_numpy
    mask, classes, dots = _blobs()
    n_comp = int(label_class_components_numpy(classes, 3)[1].min())
    foreign = classes.copy()
    foreign[1, 5, 5] = 255
    n_dots = int(np.count_nonzero(dots[0]))
    maps = np.stack([_scene(s, H, W, 20)[0] for s in (1, 2)])
    n_peaks = int(P.peak_lists_numpy(maps)[1].max())
    md, cd, fd, dd, pd = _dev(mask), _dev(classes), _dev(foreign), _dev(dots[:1]), _dev(maps)
    assert n_dots > 4 and n_peaks > 4 and n_comp > 2
    return md.device, {
        "label_components_clean": (lambda: infer.label_components(md, _fault=True)[-1], 0),
        "count_objects_clean": (lambda: infer.count_objects(md, _fault=True)[1], 0),
        "class_labelling_foreign_value": (lambda: infer._label_class_components(fd, 3, None)[1], 5),
        "class_labelling_cap_below_count": (lambda: infer._label_class_components(cd, 3, 2)[1], 6),
        "class_labelling_clean": (lambda: infer._label_class_components(cd, 3, None)[1], 0),
        "count_class_objects_foreign_value": (lambda: infer.count_class_objects(fd, 3, _fault=True)[1], 5),
        "count_class_objects_clean": (lambda: infer.count_class_objects(cd, 3, _fault=True)[1], 0),
        "dot_lists_overflow": (lambda: M.dot_lists(dd, max_dots=n_dots - 1, _fault=True)[2], 1),
        "dot_lists_exactly_full": (lambda: M.dot_lists(dd, max_dots=n_dots, _fault=True)[2], 0),
        "peak_lists_overflow": (lambda: P.peak_lists(pd, max_peaks=n_peaks - 1, _fault=True)[2], P.FAULT_OVERFLOW),
        "peak_lists_clean": (lambda: P.peak_lists(pd, _fault=True)[2], 0),
    }


FAULT_NAMES = ["label_components_clean", "count_objects_clean", "class_labelling_foreign_value", "class_labelling_cap_below_count",
               "class_labelling_clean", "count_class_objects_foreign_value", "count_class_objects_clean", "dot_lists_overflow",
               "dot_lists_exactly_full", "peak_lists_overflow", "peak_lists_clean"]


@pytest.fixture(scope="module")
def fault_cases():
    _need_gpu()
    return _fault_cases()


@pytest.mark.parametrize("name", FAULT_NAMES)
def test_fault_word_survives_an_overwritten_workspace(fault_cases, name):
    from umi import ops
    device, cases = fault_cases
    assert sorted(cases) == sorted(FAULT_NAMES)
    produce, want = cases[name]
    fault = produce()
    assert fault.dtype == torch.int32 and fault.numel() == 1
    ws = ops.workspace(1, device)
    assert fault.untyped_storage().data_ptr() != ws.untyped_storage().data_ptr()
    poison.fill_bytes(ws, 0xFF)                                        # what any later op may do to the shared buffer
    assert ws[:4].view(torch.int32).item() == -1
    assert fault.item() == want


# ---- 2, 3. the scoring chains on poisoned memory, one copy each -------------------------------------------------------------------
@pytest.fixture(scope="module")
def chains(golden_dir):
    """name -> (the call on device inputs, a check of its result against the host statement); inputs and statements made once."""
    _need_gpu()
    import CrowdMatching as CM
    import loss as L
    from umi import infer, matching as M, peaks as P
    out = {}

    mask, _, dots = _blobs()
    md, dd = _dev(mask), _dev(dots)
    want_bin = _score_numpy(mask, dots, 10)
    assert min(w["Pred"] for w in want_bin) > 3 and min(w["GT"] for w in want_bin) > 3
    out["score_binary_masks"] = (lambda: infer.score_binary_masks(md, dd, GC.SIGMAS, GC.THRESHOLDS, dist_thresh=10),
                                 lambda got: _same(got, want_bin))

    cmask, cdots, K = GM.score_case("k3_64")
    cmd, cdd = _dev(cmask), _dev(cdots)
    want_mc = M.score_multiclass_numpy(cmask, cdots, K, GM.SIGMAS, GM.THRESHOLDS)
    out["score_multiclass_masks"] = (lambda: infer.score_multiclass_masks(cmd, cdd, K, GM.SIGMAS, GM.THRESHOLDS),
                                     lambda got: _same(got, want_mc))

    scenes = [_scene(s, H, W, 20) for s in (1, 2)]
    pred, gt = np.stack([s[0] for s in scenes]), np.stack([s[1] for s in scenes])
    assert _cells_clear_of_integers(pred, SIZE)
    pdv, gdv = _dev(pred), _dev(gt)
    bounds = _sum_bound(pred)
    want_d = P.score_density_numpy(pred, gt, GC.SIGMAS, GC.THRESHOLDS, size=SIZE)
    want_p = P.score_density_numpy((pred[:1], pred[1:]), (gt[:1], gt[1:]), GC.SIGMAS, GC.THRESHOLDS, size=SIZE)
    assert min(w["peaks"] for w in want_d) > 5

    def check_density(got):
        for n in range(2):
            _compare_scores(got[n], want_d[n], bounds[n])
        return len(got) == 2

    def check_pair(got):
        for h in (0, 1):
            _compare_scores(got[0][h], want_p[0][h], bounds[h])
        r, w = got[0]["ratio"], want_p[0]["ratio"]
        return len(got) == 1 and r.keys() == w.keys() and r["GT"] == w["GT"] and abs(r["Pred"] - w["Pred"]) <= 1e-12

    out["score_density_maps"] = (lambda: infer.score_density_maps(pdv, gdv, GC.SIGMAS, GC.THRESHOLDS, size=SIZE), check_density)
    out["score_density_maps_pair"] = (lambda: infer.score_density_maps((pdv[:1], pdv[1:]), (gdv[:1], gdv[1:]), GC.SIGMAS,
                                                                       GC.THRESHOLDS, size=SIZE), check_pair)
    want_peaks = (want_d[0]["arr_prec"], want_d[0]["arr_recall"], want_d[0]["arr_f1"])
    out["CrowdMatchingTestPeaks"] = (lambda: CM.CrowdMatchingTestPeaks(gdv[0], pdv[0], GC.SIGMAS, GC.THRESHOLDS),
                                     lambda got: _same(got, want_peaks))

    logits, target = GB.mr_case("plain")
    want_mr = float(np.load(os.path.join(golden_dir, "binary_infer.npz"))["mr_plain"])
    ld, td, th = _dev(logits), _dev(target), torch.from_numpy(target)
    out["MRAccuracy_device_target"] = (lambda: L.MRAccuracy(ld, td), lambda got: _same(got, want_mr))
    out["MRAccuracy_cpu_target"] = (lambda: L.MRAccuracy(ld, th), lambda got: _same(got, want_mr))

    g, x, y = GC.case("random_64")
    fx = np.load(os.path.join(golden_dir, "crowd_matching.npz"))
    want_cm = tuple(fx[f"cm_random_64_{k}"] for k in ("prec", "recall", "f1"))
    gd, xy = _dev(g.astype(np.uint8)), (_dev(x), _dev(y))
    out["CrowdMatchingTest"] = (lambda: CM.CrowdMatchingTest(gd, xy, GC.SIGMAS, GC.THRESHOLDS, inputType='Coordinates'),
                                lambda got: _same(got, want_cm))
    return out


CHAINS = ["score_binary_masks", "score_multiclass_masks", "score_density_maps", "score_density_maps_pair", "CrowdMatchingTestPeaks",
          "MRAccuracy_device_target", "MRAccuracy_cpu_target", "CrowdMatchingTest"]


@pytest.mark.parametrize("name", CHAINS)
def test_chain_on_poisoned_memory_equals_the_host_statement(chains, name):
    assert sorted(chains) == sorted(CHAINS)
    call, check = chains[name]
    with poison.poisoned(0x00):
        clean = call()
    with poison.poisoned(0xFF):
        dirty = call()
    assert _same(clean, dirty), "the result depends on what unwritten memory or the shared workspace held"
    assert check(clean)


@pytest.mark.parametrize("name", CHAINS)
def test_chain_does_one_device_to_host_copy(chains, name, monkeypatch):
    call, check = chains[name]
    call()                                                             # warm-up: tables uploaded, workspace grown
    copies = []
    for meth in ("cpu", "item", "tolist", "numpy", "to", "__bool__", "__int__", "__float__", "__index__"):
        orig = getattr(torch.Tensor, meth)

        def counted(self, *a, _orig=orig, _meth=meth, **kw):
            to_host = _meth != "to" or any(str(v) == "cpu" or (isinstance(v, torch.device) and v.type == "cpu")
                                           for v in list(a) + list(kw.values()))
            if self.is_cuda and to_host:
                copies.append(_meth)
            return _orig(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, meth, counted)
    got = call()
    monkeypatch.undo()
    assert copies == ["cpu"], copies
    assert check(got)


# ---- 4. the graphed predictors ----------------------------------------------------------------------------------------------------
class _Raises(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x):
        raise FloatingPointError("the first eager run")


def _unet():
    import Model
    m = Model.UNet(1, 2, 8, False, compute_dtype="fp32")
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=41))
    return m.to(DEV).train()


def _bits_equal(a, b):
    a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
    return len(a) == len(b) and all(p.dtype == q.dtype and p.shape == q.shape and
                                    torch.equal(p.contiguous().view(torch.uint8), q.contiguous().view(torch.uint8)) for p, q in zip(a, b))


def _predictor(kind, m):
    """(constructor, eager function, two inputs) of one predictor kind around the model `m`."""
    from umi import infer
    from umi.tiles import TilePlan
    g = torch.Generator().manual_seed(5)
    if kind == "graphed":
        xs = [torch.randn((2, 1, 32, 32), generator=g).to(DEV) for _ in range(2)]
        return (lambda: infer.GraphedPredictor(m, xs[0])), (lambda x: infer.predict_mask(m, x)), xs
    if kind == "tiled":
        plan = TilePlan.overlap_tile(48, 70, 32, 8)
        xs = [torch.randn((1, 1, 48, 70), generator=g).to(DEV) for _ in range(2)]
        return (lambda: infer.TiledPredictor(m, plan, 1, batch=4)), (lambda x: infer.predict_logits_tiled(m, x, plan, batch=4)), xs
    xs = [torch.randn((2, 1, 48, 32), generator=g).to(DEV) for _ in range(2)]
    return (lambda: infer.TTAPredictor(m, xs[0], "d4", "prob")), (lambda x: infer.predict_logits_tta(m, x, "d4", "prob")), xs


@pytest.mark.parametrize("kind", ["graphed", "tiled", "tta"])
def test_predictor_keeps_the_training_flag_and_replays_the_eager_call(kind):
    _need_gpu()
    m = _unet()
    build, eager, xs = _predictor(kind, m)
    predict = build()
    assert m.training
    for x in xs:
        got = predict(x)
        assert m.training
        want = eager(x)
        assert _bits_equal(got, want)
    assert not _bits_equal(eager(xs[0]), eager(xs[1])), "degenerate test: both inputs give one result"
    assert m.training
    for training in (True, False):
        bad = _Raises(m).train(training)
        with pytest.raises(FloatingPointError):
            _predictor(kind, bad)[0]()
        assert bad.training == training and m.training == training
    m.train()
