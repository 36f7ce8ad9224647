"""GPU: test-time augmentation on the MI355X -- the kernels umi_tta_views / umi_tta_accumulate / umi_tta_finish against the NumPy
statement of umi.tta, and umi.infer.predict_logits_tta / predict_mask_tta / TTAPredictor on callables, U-Nets and the small TransUNet.

Views, and the 'logit' and 'relu' merges with their masks, are compared bit for bit.  'prob' is compared with the float64 statement
inside umi.tta.prob_bound(K, count, spread) = 2^-24 * (2 * (spread + 2 * EXPF_ULP) + K + (count + 1) / 2 + 1) * 1.01, the fp32
arithmetic of one softmax over K (argument rounding |v - max| u, expf, the sum, the division), `count` additions of values in
[0, 1] and one division; the entropy inside umi.tta.entropy_bound(K, that).  EXPF_ULP = 1, LOGF_ULP = 3: ROCm ships no accuracy
table on the machine, so tools/bench_tta.py measured the device expf on [-60, 20] and logf on (0, 1] against float64 (0.85 and 2.15
ulp, profiles/tta.json "math_ulp"), rounded up here.  'prob' masks are compared wherever the statement's top-two margin exceeds twice the bound; at most 1 % of the pixels
may be excluded (tests/test_tta.py checks that the statement alone meets the cap for these inputs)."""
import numpy as np
import pytest
import torch

from oracle import recipe
from tests import poison
from umi import tta as T

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(1, 1, 1, 1), (2, 3, 33, 47), (1, 2, 64, 64), (3, 1, 10, 70), (2, 4, 65, 31)]
KS = [1, 2, 3, 9]
SETS = [(e,) for e in range(8)] + ["flips", "d4", (5, 0, 3, 3, 6, 1)]
CHUNKS = [1, 3, None]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: torch.cuda.is_available() is False")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _runs(els, H, W, chunk):
    """The tuple cut into runs of one view shape of at most `chunk` elements, in order: [(start, stop)]."""
    out, a = [], 0
    while a < len(els):
        b = a + 1
        while b < len(els) and (chunk is None or b - a < chunk) and T.view_shape(els[b], H, W) == T.view_shape(els[a], H, W):
            b += 1
        out.append((a, b))
        a = b
    return out


def _offset(t):
    """A copy of t whose base address is one float past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    assert flat.data_ptr() % 16 == 0
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


# ---- views ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_views_are_the_statement(shape):
    _need_gpu()
    N, C, H, W = shape
    x = np.random.default_rng(3).standard_normal(shape).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    for views in SETS:
        els = T.view_set(views)
        for a, b in _runs(els, H, W, None):
            want = np.concatenate([T.view_numpy(x, e) for e in els[a:b]])
            got = {}
            for byte in (0x00, 0xFF):
                with poison.poisoned(byte):
                    got[byte] = T.views(xd, els[a:b]).cpu().numpy()
            assert got[0x00].shape == want.shape
            assert np.array_equal(_bits(got[0x00]), _bits(got[0xFF])), (views, a, b)       # every element written
            assert np.array_equal(_bits(got[0x00]), _bits(want)), (views, a, b)


def test_views_on_a_base_pointer_offset_by_one_float():
    _need_gpu()
    x = np.random.default_rng(4).standard_normal((1, 2, 64, 64)).astype(np.float32)
    xd = _offset(torch.from_numpy(x).to(DEV))
    for views in ("flips", "d4"):
        els = T.view_set(views)
        want = np.concatenate([T.view_numpy(x, e) for e in els])
        out = _offset(torch.full(want.shape, float("nan"), device=DEV))
        T.views(xd, els, out=out)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)), views
    with pytest.raises(ValueError):
        T.views(torch.zeros(1, 1, 3, 5, device=DEV), "d4")           # two shapes in one call


# ---- accumulate and finish --------------------------------------------------------------------------------------------------------
def _outputs(els, N, K, H, W, seed, scale=4.0):
    rng = np.random.default_rng(seed)
    return [(scale * rng.standard_normal((N, K) + T.view_shape(e, H, W))).astype(np.float32) for e in els]


def _device_merge(outs_d, els, N, K, H, W, mode, chunk, mask=True, entropy=False, offset=False):
    """zero -> accumulate in runs of at most `chunk` views -> finish; returns numpy (mean, mask[, entropy])."""
    acc = torch.zeros((N, K, H, W), dtype=torch.float32, device=DEV)
    if offset:
        acc = _offset(acc)
    for a, b in _runs(els, H, W, chunk):
        y = torch.cat(outs_d[a:b])
        T.accumulate(acc, _offset(y) if offset else y, els[a:b], mode)
    res = T.finish(acc, len(els), mode, mask=mask, entropy=entropy)
    res = res if isinstance(res, tuple) else (res,)
    assert res[0].data_ptr() == acc.data_ptr()
    return tuple(r.cpu().numpy() for r in res)


def _spread(outs, K):
    return max(float(np.abs(o).max()) if K == 1 else float((o.max(axis=1) - o.min(axis=1)).max()) for o in outs)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", SHAPES)
def test_logit_and_relu_merges_are_the_statement_bit_for_bit(shape, K):
    _need_gpu()
    N, _, H, W = shape
    for si, views in enumerate(SETS):
        els = T.view_set(views)
        outs = _outputs(els, N, K, H, W, 1000 + 10 * K + si)
        outs[0].reshape(-1)[::7] *= np.float32(1e-8)                   # values around the binary cut-off, zeros of both signs
        outs[-1].reshape(-1)[::5] = np.float32(-0.0)
        outs_d = [torch.from_numpy(o).to(DEV) for o in outs]
        for mode in ("logit", "relu"):
            want = T.merge_numpy(outs, els, mode)
            want_mask = T.mask_numpy(want, mode)
            for chunk in CHUNKS:
                got = {}
                for byte in (0x00, 0xFF):
                    with poison.poisoned(byte):
                        got[byte] = _device_merge(outs_d, els, N, K, H, W, mode, chunk)
                for g0, g1 in zip(got[0x00], got[0xFF]):
                    assert np.array_equal(_bits(g0), _bits(g1)), (views, mode, chunk)
                mean, mask = got[0x00]
                assert np.array_equal(_bits(mean), _bits(want)), (views, mode, chunk)
                assert mask.dtype == np.uint8 and np.array_equal(mask, want_mask), (views, mode, chunk)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", SHAPES)
def test_prob_merge_entropy_and_mask_are_inside_the_bound(shape, K):
    _need_gpu()
    N, _, H, W = shape
    worst = [0.0, 0.0, 0.0]
    for si, views in enumerate(SETS):
        els = T.view_set(views)
        outs = _outputs(els, N, K, H, W, 2000 + 10 * K + si)
        outs_d = [torch.from_numpy(o).to(DEV) for o in outs]
        want = T.merge_numpy(outs, els, "prob")
        want_ent, want_mask = T.entropy_numpy(want), T.mask_numpy(want, "prob")
        bound = T.prob_bound(K, len(els), _spread(outs, K))
        ebound = T.entropy_bound(K, bound)
        decided = T.top_two_margin(want, "prob") > 2 * bound
        first = None
        for chunk in CHUNKS:
            got = {}
            for byte in (0x00, 0xFF):
                with poison.poisoned(byte):
                    got[byte] = _device_merge(outs_d, els, N, K, H, W, "prob", chunk, entropy=True)
            for g0, g1 in zip(got[0x00], got[0xFF]):
                assert np.array_equal(_bits(g0), _bits(g1)), (views, chunk)
            mean, mask, ent = got[0x00]
            if first is None:
                first = got[0x00]
            for g0, g1 in zip(first, got[0x00]):                       # the chunking does not change a bit
                assert np.array_equal(_bits(g0), _bits(g1)), (views, chunk)
            err, eerr = float(np.abs(mean - want).max()), float(np.abs(ent - want_ent).max())
            worst = [max(worst[0], err / bound), max(worst[1], eerr / ebound), max(worst[2], 1.0 - decided.mean())]
            assert err <= bound, (views, chunk, err, bound)
            assert eerr <= ebound, (views, chunk, eerr, ebound)
            assert (~decided).mean() <= 0.01, (views, (~decided).mean())
            assert np.array_equal(mask[decided], want_mask[decided]), (views, chunk)
    print(f"{shape} K={K}: worst |mean - statement| / bound = {worst[0]:.3f}, entropy / bound = {worst[1]:.3f}, "
          f"undecided share = {worst[2]:.4f}")


@pytest.mark.parametrize("mode", ["logit", "relu", "prob"])
def test_merge_on_base_pointers_offset_by_one_float(mode):
    _need_gpu()
    N, K, H, W = 1, 2, 64, 64
    for views in ("flips", "d4"):
        els = T.view_set(views)
        outs_d = [torch.from_numpy(o).to(DEV) for o in _outputs(els, N, K, H, W, 77)]
        aligned = _device_merge(outs_d, els, N, K, H, W, mode, None, entropy=mode == "prob")
        shifted = _device_merge(outs_d, els, N, K, H, W, mode, None, entropy=mode == "prob", offset=True)
        for a, s in zip(aligned, shifted):
            assert np.array_equal(_bits(a), _bits(s)), (views, mode)


@pytest.mark.parametrize("mode", ["logit", "relu", "prob"])
def test_a_non_finite_logit_reaches_its_own_pixel_only(mode):
    _need_gpu()
    N, K, H, W = 2, 3, 33, 47
    els = T.view_set("d4")
    outs = _outputs(els, N, K, H, W, 5)
    clean = _device_merge([torch.from_numpy(o).to(DEV) for o in outs], els, N, K, H, W, mode, 3, entropy=mode == "prob")
    for v, (value, n, k, i, j) in enumerate([(np.nan, 1, 2, 5, 7), (np.inf, 0, 0, 46, 0), (-np.inf, 1, 1, 0, 32),
                                             (np.nan, 0, 1, 46, 32), (np.inf, 1, 0, 32, 46), (np.nan, 0, 2, 0, 0)]):
        e = els[v]
        Hv, Wv = T.view_shape(e, H, W)
        i, j = min(i, Hv - 1), min(j, Wv - 1)
        bad = [o.copy() for o in outs]
        bad[v][n, k, i, j] = value
        ys, xs = T.view_source(e, H, W)
        y, x = int(ys[i, j]), int(xs[i, j])
        got = _device_merge([torch.from_numpy(o).to(DEV) for o in bad], els, N, K, H, W, mode, 3, entropy=mode == "prob")
        for g, c in zip(got, clean):
            same = _bits(g) == _bits(c)
            if g.ndim == 4:
                same[n, :, y, x] = True
            else:
                same[n, y, x] = True
            assert same.all(), (mode, v, np.argwhere(~same)[:4])
        if mode == "logit":
            assert not np.isfinite(got[0][n, k, y, x])
        if np.isnan(value):                                            # a NaN passes through every mode's transform
            assert np.isnan(got[0][n, k, y, x]), (mode, v)


def test_wrappers_reject_other_inputs():
    _need_gpu()
    acc = torch.zeros(1, 2, 3, 5, device=DEV)
    with pytest.raises(ValueError):
        T.accumulate(acc, torch.zeros(2, 2, 3, 5, device=DEV), (0, 1))                    # two shapes
    with pytest.raises(ValueError):
        T.accumulate(acc, torch.zeros(1, 2, 3, 5, device=DEV), (1,))                      # (5, 3) expected
    with pytest.raises(ValueError):
        T.accumulate(torch.zeros(1, 33, 4, 4, device=DEV), torch.zeros(1, 33, 4, 4, device=DEV), (0,))
    with pytest.raises(ValueError):
        T.finish(acc, 0)
    with pytest.raises(ValueError):
        T.finish(acc, 1, "logit", entropy=True)
    with pytest.raises(ValueError):
        T.finish(acc.double(), 1)
    with pytest.raises(RuntimeError):
        T.finish(acc.cpu(), 1)


# ---- callables --------------------------------------------------------------------------------------------------------------------
def _pointwise(v):
    return torch.cat([v * 3.0 - 0.5, v.flip(1) * -2.0], dim=1)


def test_a_callable_gives_the_same_bits_for_every_batch():
    _need_gpu()
    from umi import infer
    x = torch.randn((3, 2, 10, 70), generator=torch.Generator().manual_seed(2)).to(DEV)
    for mode in ("logit", "prob"):
        for views in ("d4", (1, 1, 6)):
            ref = infer.predict_logits_tta(_pointwise, x, views, mode, batch=None, entropy=mode == "prob")
            ref = ref if isinstance(ref, tuple) else (ref,)
            assert tuple(ref[0].shape) == (3, 4, 10, 70) and ref[0].is_cuda
            for batch in (1, 3, 5):
                got = infer.predict_logits_tta(_pointwise, x, views, mode, batch=batch, entropy=mode == "prob")
                got = got if isinstance(got, tuple) else (got,)
                assert all(torch.equal(a, b) for a, b in zip(ref, got)), (mode, views, batch)
            if mode == "logit":                                        # an equivariant function: the mean is the function of x
                assert torch.allclose(ref[0], _pointwise(x), rtol=1e-6, atol=1e-6)
    with pytest.raises(ValueError):
        infer.predict_logits_tta(_pointwise, x, "d4", "logit", entropy=True)
    with pytest.raises(ValueError):
        infer.predict_logits_tta(_pointwise, x.half(), "d4")
    with pytest.raises(ValueError):
        infer.predict_logits_tta(lambda v: _pointwise(v).half(), x, "d4")


# ---- models -----------------------------------------------------------------------------------------------------------------------
class _Recorder(torch.nn.Module):
    """Keeps the logits of the very forwards that ran."""

    def __init__(self, model):
        super().__init__()
        self.model, self.seen = model, []

    def forward(self, v):
        out = self.model(v)
        self.seen.append((tuple(v.shape), tuple(o.cpu().numpy() for o in (out if isinstance(out, tuple) else (out,)))))
        return out


def _model(kind, seed=41):
    import Model
    if kind == "unet2":
        m = Model.UNet(1, 2, 8, False, compute_dtype="fp16")
    elif kind == "unet1":
        m = Model.UNet(1, 1, 8, False, compute_dtype="fp16")
    elif kind == "multitask":
        m = Model.UNet_multitask(1, 2, 8, False, compute_dtype="fp32")
    else:
        from oracle import ref_transunet
        from tests.test_gpu_transunet import product_config
        from TransUnet.vit_seg_modeling import VisionTransformer
        m = VisionTransformer(product_config(ref_transunet.small_config(2), 64), img_size=64, num_classes=2, compute_dtype="fp16")
        m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=seed, negative_gamma=False))
        return m.to(DEV).eval()
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=seed))
    return m.to(DEV).eval()


def _image(hw, n=2, seed=7):
    return torch.randn((n, 1) + hw, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _recorded_outputs(seen, els, N, H, W, head):
    """The recorded forwards (one per shape class per model, all views of the class at once) -> one output per element, model-major."""
    classes = T.shape_classes(els, H, W)
    per_model = len(classes)
    assert len(seen) % per_model == 0
    outs = []
    for m in range(len(seen) // per_model):
        by_pos = {}
        for (shape, pos), (in_shape, heads) in zip(classes.items(), seen[m * per_model:(m + 1) * per_model]):
            assert in_shape[0] == len(pos) * N and in_shape[2:] == shape
            for s, p in enumerate(pos):
                by_pos[p] = heads[head][s * N:(s + 1) * N]
        outs += [by_pos[p] for p in range(len(els))]
    return outs


def _check_against_statement(outs, els, mode, mean, mask, tag):
    want = T.merge_numpy(outs, els, mode)
    K = want.shape[1]
    if mode == "logit":
        assert np.array_equal(_bits(mean), _bits(want)), tag
        assert np.array_equal(mask, T.mask_numpy(want, mode)), tag
        return
    bound = T.prob_bound(K, len(els), _spread(outs, K))
    err = float(np.abs(mean - want).max())
    decided = T.top_two_margin(want, "prob") > 2 * bound
    print(f"{tag}: |mean - statement| = {err:.3e}, bound {bound:.3e}, undecided share {1 - decided.mean():.4f}")
    assert err <= bound, (tag, err, bound)
    assert np.array_equal(mask[decided], T.mask_numpy(want, "prob")[decided]), tag


@pytest.mark.parametrize("kind,hw", [("unet2", (32, 32)), ("unet2", (48, 32)), ("unet1", (32, 32)), ("multitask", (32, 32)),
                                     ("transunet", (64, 64))])
def test_model_tta_is_the_statement_over_the_forwards_that_ran(kind, hw):
    _need_gpu()
    from umi import infer
    rec = _Recorder(_model(kind)).train()
    x, els = _image(hw), T.view_set("d4")
    N, (H, W) = x.shape[0], hw
    for mode in ("logit", "prob"):
        rec.seen = []
        mean = infer.predict_logits_tta(rec, x, "d4", mode)
        seen = list(rec.seen)
        mask = infer.predict_mask_tta(rec, x, "d4", mode)
        assert rec.training and rec.model.training                    # the flag is restored
        two = isinstance(mean, tuple)
        assert two == (kind == "multitask") and isinstance(mask, tuple) == two
        assert len(seen) == (1 if H == W else 2)
        for head, (mn, mk) in enumerate(zip(mean if two else (mean,), mask if two else (mask,))):
            assert mn.dtype == torch.float32 and mn.is_cuda and tuple(mn.shape[2:]) == hw and tuple(mk.shape) == (N,) + hw
            outs = _recorded_outputs(seen, els, N, H, W, head)
            assert all(np.isfinite(o).all() for o in outs) and outs[0].std() > 0
            _check_against_statement(outs, els, mode, mn.cpu().numpy(), mk.cpu().numpy(), (kind, hw, mode, head))
    ent = infer.predict_mask_tta(rec, x, "flips", "prob", entropy=True)
    ent = ent[0] if isinstance(ent[0], tuple) else ent
    assert ent[0].dtype == torch.uint8 and ent[1].dtype == torch.float32 and tuple(ent[1].shape) == (N,) + hw
    assert float(ent[1].min()) >= 0 and float(ent[1].max()) <= np.log(max(2, mean[0].shape[1] if two else mean.shape[1])) + 1e-5


def test_a_list_of_two_models_is_the_statement_over_all_their_outputs():
    _need_gpu()
    from umi import infer
    recs = [_Recorder(_model("unet2", seed=41)), _Recorder(_model("unet2", seed=43))]
    x, els = _image((48, 32)), T.view_set("d4")
    for mode in ("logit", "prob"):
        for r in recs:
            r.seen = []
        mean = infer.predict_logits_tta(recs, x, "d4", mode, batch=3)
        # batch = 3 cuts the forwards; glue the recorded chunks back per shape class
        outs = []
        for r in recs:
            glued, rows = [], {}
            for in_shape, heads in r.seen:
                rows.setdefault(in_shape[2:], []).append(heads[0])
            for shape in T.shape_classes(els, 48, 32):
                cat = np.concatenate(rows[shape])
                glued.append(((cat.shape[0], 1) + shape, (cat,)))
            outs += _recorded_outputs(glued, els, 2, 48, 32, 0)
        assert len(outs) == 16
        mask = infer.predict_mask_tta(recs, x, "d4", mode, batch=3)
        _check_against_statement(outs, els * 2, mode, mean.cpu().numpy(), mask.cpu().numpy(), ("ensemble", mode))
    single = infer.predict_logits_tta(recs[0], x, "d4", "logit")
    assert not torch.equal(single, infer.predict_logits_tta(recs, x, "d4", "logit"))


@pytest.mark.parametrize("kind", ["unet2", "multitask"])
def test_tta_predictor_replays_the_eager_call_and_follows_the_weights(kind):
    _need_gpu()
    from umi import infer
    m = _model(kind).train()
    x = _image((48, 32))
    predict = infer.TTAPredictor(m, x, "d4", "prob")
    assert m.training

    def same(a, b):
        a, b = (a if isinstance(a, tuple) else (a,)), (b if isinstance(b, tuple) else (b,))
        return len(a) == len(b) and all(same(p, q) if isinstance(p, tuple) else torch.equal(p, q) for p, q in zip(a, b))

    for xx in (x, _image((48, 32), seed=8)):
        assert same(predict(xx), infer.predict_logits_tta(m, xx, "d4", "prob"))
        assert same(predict(xx, entropy=True), infer.predict_logits_tta(m, xx, "d4", "prob", entropy=True))
        assert same(predict.predict_mask(xx), infer.predict_mask_tta(m, xx, "d4", "prob"))
    first = predict(x)
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    g = torch.Generator().manual_seed(3)
    for p in m.parameters():
        p.grad = (0.1 * torch.randn(p.shape, generator=g)).to(DEV)
    opt.step()
    want = infer.predict_logits_tta(m, x, "d4", "prob")
    assert not same(want, first)
    got = predict(x)
    assert same(got, want)
    again = predict(x)
    assert same(again, got)
    assert (got[0] if isinstance(got, tuple) else got).data_ptr() != (again[0] if isinstance(again, tuple) else again).data_ptr()
    other = _image((32, 32))                                           # another shape: the eager path
    assert same(predict(other), infer.predict_logits_tta(m, other, "d4", "prob"))
    logit = infer.TTAPredictor(m, x, "flips", "logit", batch=3)
    assert same(logit(x), infer.predict_logits_tta(m, x, "flips", "logit", batch=3))
    assert same(logit.predict_mask(x), infer.predict_mask_tta(m, x, "flips", "logit", batch=3))


def test_tta_composes_with_the_tiled_path():
    _need_gpu()
    from umi import infer
    from umi.tiles import TilePlan
    m = _model("unet2")
    plan = TilePlan.overlap_tile(70, 90, 32, 8)
    x = _image((70, 90), n=1)
    seen = []

    def tiled(v):
        out = infer.predict_logits_tiled(m, v, plan)[None]
        seen.append(out.cpu().numpy())
        return out

    els = T.view_set("flips")
    mean = infer.predict_logits_tta(tiled, x, "flips", "logit", batch=1)
    assert tuple(mean.shape) == (1, 2, 70, 90) and len(seen) == 4
    assert np.array_equal(_bits(mean.cpu().numpy()), _bits(T.merge_numpy(seen, els, "logit")))
    mask = infer.predict_mask_tta(tiled, x, "flips", "logit", batch=1)
    assert torch.equal(mask, infer.argmax_mask(mean)) and 0 < mask.float().mean() < 1
