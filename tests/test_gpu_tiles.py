"""GPU: overlap-tile / sliding-window inference on the MI355X -- the kernels umi_tile_gather / umi_tile_blend / umi_tile_finish
against the NumPy statement of umi.tiles, bit for bit, and umi.infer.predict_logits_tiled / predict_mask_tiled / TiledPredictor
on an identity model and on small U-Nets.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from oracle import recipe
from tests import poison
from umi import tiles as T
from umi.tiles import TilePlan

pytestmark = pytest.mark.gpu
DEV = "cuda"

IMAGES = [(1, 1, 1), (3, 37, 53), (2, 10, 70), (4, 64, 64)]
TILES = [(16, 24), (5, 7), (32, 32)]
CHUNKS = [1, 3, 8, 64]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: torch.cuda.is_available() is False")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _plans(H, W, tile, **kw):
    """overlap_tile with halo 0 and 4, sliding (gauss) with overlap 0, 8 and T - 1; halo 4 / overlap 8 where the tile allows."""
    t = min(tile)
    out = [TilePlan.overlap_tile(H, W, tile, 0, **kw), TilePlan.sliding(H, W, tile, 0, **kw), TilePlan.sliding(H, W, tile, t - 1, **kw)]
    if t - 8 >= 1:
        out.append(TilePlan.overlap_tile(H, W, tile, 4, **kw))
    if t > 8:
        out.append(TilePlan.sliding(H, W, tile, 8, **kw))
    return out


def _chunked_ids(n_tiles, c):
    """The ids 0 .. n_tiles - 1 ascending in chunks of c slots: from 3 slots on, slot 1 of every chunk is empty (a hole in the
    middle); the last chunk is padded with empty slots; one wholly empty chunk at the end."""
    real = c - 1 if c >= 3 else c
    rows = []
    for a in range(0, n_tiles, real):
        ids = list(range(a, min(n_tiles, a + real)))
        if c >= 3:
            ids.insert(1, -1)
        rows.append(ids + [-1] * (c - len(ids)))
    rows.append([-1] * c)
    return np.array(rows, dtype=np.int32)


# ---- kernels ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("shape", IMAGES)
def test_gather_is_the_statement(shape, tile):
    _need_gpu()
    from umi import infer
    C, H, W = shape
    x = np.random.default_rng(11).standard_normal(shape).astype(np.float32)
    xd = torch.from_numpy(x).to(DEV)
    for pad in ("reflect", "constant"):
        for plan in _plans(H, W, tile, pad=pad, pad_value=255.0):
            want = T.gather_numpy(x, plan, list(range(plan.n_tiles)))
            for c in CHUNKS:
                rows = _chunked_ids(plan.n_tiles, c)
                ids = torch.from_numpy(rows).to(DEV)
                got = {}
                for byte in (0x00, 0xFF):
                    with poison.poisoned(byte):
                        got[byte] = torch.stack([infer.tile_gather(xd, plan, ids[r]) for r in range(len(rows))]).cpu().numpy()
                assert np.array_equal(_bits(got[0x00]), _bits(got[0xFF])), (pad, c)       # no slot element left unwritten
                flat, slots = got[0x00].reshape((-1,) + want.shape[1:]), rows.reshape(-1)
                assert not flat[slots < 0].any(), (pad, c)                                # empty slots are zeros
                assert np.array_equal(_bits(flat[slots >= 0]), _bits(want)), (pad, c, plan.oy.tolist(), plan.ox.tolist())


def _poisoned_logits(plan, K, seed):
    """Random logits for every tile, scaled per tile; +-inf and NaN wherever the tile's weight is 0 (a discarded halo)."""
    rng = np.random.default_rng(seed)
    lg = rng.standard_normal((plan.n_tiles, K, plan.th, plan.tw)).astype(np.float32)
    lg.reshape(-1)[::13] *= np.float32(1e-7)                                              # values around the mask's cut-off
    dead = (plan.wy[:, None] * plan.wx[None, :]) == 0
    for t in range(plan.n_tiles):
        lg[t][:, dead] = (np.inf, -np.inf, np.nan)[t % 3]
    return lg


@pytest.mark.parametrize("tile", TILES)
@pytest.mark.parametrize("shape", IMAGES)
def test_blend_and_finish_are_the_statement(shape, tile):
    _need_gpu()
    from umi import infer
    _, H, W = shape
    for plan in _plans(H, W, tile):
        for K in (1, 2, 3, 5):
            lg = _poisoned_logits(plan, K, 100 + K)
            want = T.stitch_numpy(lg, plan)
            assert np.isfinite(want).all()
            lgd = torch.from_numpy(lg).to(DEV)
            for c in CHUNKS:
                rows = _chunked_ids(plan.n_tiles, c)
                ids = torch.from_numpy(rows).to(DEV)
                got = {}
                for byte in (0x00, 0xFF):
                    with poison.poisoned(byte):
                        acc = torch.zeros((K, H, W), dtype=torch.float32, device=DEV)
                        chunks = torch.empty((len(rows), c, K, plan.th, plan.tw), dtype=torch.float32, device=DEV)
                        chunks[ids >= 0] = lgd[ids[ids >= 0].long()]                       # empty slots keep the preset (NaN for 0xFF)
                        for r in range(len(rows)):
                            infer.tile_blend(acc, chunks[r], plan, ids[r])
                        out, mask = infer.tile_finish(acc, plan, mask=True)
                        ref_mask = (infer.binary_mask if K == 1 else infer.argmax_mask)(out[None])[0]
                        assert mask.dtype == torch.uint8 and torch.equal(mask, ref_mask), (K, c)
                        got[byte] = out.cpu().numpy()
                assert np.array_equal(_bits(got[0x00]), _bits(got[0xFF])), (K, c)
                assert np.array_equal(_bits(got[0x00]), _bits(want)), (K, c, plan.oy.tolist(), plan.ox.tolist())


def test_entry_points_reject_other_inputs():
    _need_gpu()
    from umi import infer
    plan = TilePlan.overlap_tile(37, 53, 16, 4)
    x = torch.zeros(3, 37, 53, device=DEV)
    ids = torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        infer.tile_gather(x[:, :, :50], plan, ids)
    with pytest.raises(ValueError):
        infer.tile_gather(x, plan, ids.long())
    with pytest.raises(RuntimeError):
        infer.tile_gather(x.cpu(), plan, ids)
    with pytest.raises(ValueError):
        infer.tile_blend(torch.zeros(2, 37, 53, device=DEV), torch.zeros(4, 3, 16, 16, device=DEV), plan, ids)
    with pytest.raises(ValueError):
        infer.tile_finish(torch.zeros(2, 37, 50, device=DEV), plan)
    with pytest.raises(ValueError):
        infer.predict_logits_tiled(torch.nn.Identity(), torch.zeros(1, 3, 37, 50, device=DEV), plan)
    with pytest.raises(ValueError):
        infer.predict_logits_tiled(torch.nn.Identity(), torch.zeros(2, 3, 37, 53, device=DEV), plan)


# ---- identity model ---------------------------------------------------------------------------------------------------------------
class _Identity(torch.nn.Module):
    def forward(self, x):
        return x


@pytest.mark.parametrize("pad", ["reflect", "constant"])
@pytest.mark.parametrize("halo", [0, 4, 8])
def test_identity_model_under_overlap_tile_returns_the_image(halo, pad):
    _need_gpu()
    from umi import infer
    x = torch.randn((1, 3, 70, 90), generator=torch.Generator().manual_seed(halo)).to(DEV)
    plan = TilePlan.overlap_tile(70, 90, 32, halo, pad=pad, pad_value=255.0)
    m = _Identity().train()
    for batch in (1, 3, 8):
        got = infer.predict_logits_tiled(m, x, plan, batch=batch)
        assert got.dtype == torch.float32 and tuple(got.shape) == (3, 70, 90) and got.is_cuda
        assert torch.equal(got, x[0]), (halo, pad, batch)
    assert m.training                                                     # the flag is restored


# ---- U-Nets -----------------------------------------------------------------------------------------------------------------------
H_IMG, W_IMG, TILE = 70, 90, 32
_cache = {}


def _unet(cout, mode, seed=41):
    import Model
    m = Model.UNet(1, cout, 8, False, compute_dtype=mode)
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=seed))
    return m.to(DEV).eval()


def _image(seed=7, hw=(H_IMG, W_IMG)):
    return torch.randn((1, 1) + hw, generator=torch.Generator().manual_seed(seed)).to(DEV)


def _plan(kind):
    if kind == "overlap_tile":
        plan = TilePlan.overlap_tile(H_IMG, W_IMG, TILE, 8)
        assert (plan.ny, plan.nx) == (5, 6)
        return plan
    return TilePlan.sliding(H_IMG, W_IMG, TILE, 16, window="gauss")


def _one_per_forward(cout, mode, kind):
    """(model, image, plan, the statement applied to the logits of the plan's tiles sent through the model one per forward)."""
    key = (cout, mode, kind)
    if key not in _cache:
        from umi import infer
        m, x, plan = _unet(cout, mode), _image(), _plan(kind)
        ids = torch.arange(plan.n_tiles, dtype=torch.int32, device=DEV)
        tiles = torch.cat([infer.tile_gather(x[0], plan, ids[a:a + 32]) for a in range(0, plan.n_tiles, 32)])
        with torch.no_grad():
            lg = torch.cat([m(tiles[t:t + 1]) for t in range(plan.n_tiles)]).cpu().numpy()
        assert lg.dtype == np.float32 and lg.shape == (plan.n_tiles, cout, TILE, TILE) and np.isfinite(lg).all()
        _cache[key] = (m, x, plan, T.stitch_numpy(lg, plan))
    return _cache[key]


@pytest.mark.parametrize("kind", ["overlap_tile", "sliding"])
@pytest.mark.parametrize("mode", ["fp32", "fp16"])
@pytest.mark.parametrize("cout", [2, 1])
def test_unet_stitched_logits_are_the_statement_for_every_batch(cout, mode, kind):
    _need_gpu()
    from umi import infer
    m, x, plan, want = _one_per_forward(cout, mode, kind)
    assert want.std() > 0
    for batch in (1, 3, 8):
        got = infer.predict_logits_tiled(m, x, plan, batch=batch)
        assert tuple(got.shape) == (cout, H_IMG, W_IMG)
        diff = np.abs(got.cpu().numpy() - want).max()
        print(f"UNet(1,{cout},8) {mode} {kind} batch {batch}: max |stitched - statement| = {diff:.3e}")
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want)), (batch, diff)


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
def test_halo_0_mask_equals_the_one_tile_per_forward_loop(mode):
    _need_gpu()
    from umi import infer
    m, x = _unet(1, mode), _image(9, (64, 96))
    plan = TilePlan.overlap_tile(64, 96, 32, 0)
    want = infer.predict_binary_mask_tiled(m, x, 32)
    assert 0 < want.float().mean() < 1, "degenerate test: the model's mask is constant"
    for batch in (1, 8):
        got = infer.predict_mask_tiled(m, x, plan, batch=batch)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (64, 96)
        assert torch.equal(got, want), batch


@pytest.mark.parametrize("mode", ["fp32", "fp16"])
@pytest.mark.parametrize("cout", [2, 1])
def test_tiled_predictor_replays_the_eager_call_and_follows_the_weights(cout, mode):
    _need_gpu()
    from umi import infer
    m, x, plan = _unet(cout, mode), _image(), _plan("overlap_tile")
    m.train()
    predict = infer.TiledPredictor(m, plan, 1, batch=8)
    assert m.training
    for xx in (x, _image(8)):
        assert torch.equal(predict(xx), infer.predict_logits_tiled(m, xx, plan, batch=8))
        assert torch.equal(predict.predict_mask(xx), infer.predict_mask_tiled(m, xx, plan, batch=8))
    first = predict(x)
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=43))
    want = infer.predict_logits_tiled(m, x, plan, batch=8)
    assert not torch.equal(want, first)
    got = predict(x)
    assert torch.equal(got, want)
    assert torch.equal(predict(x), got) and got.data_ptr() != predict(x).data_ptr()        # clones
    sliding = _plan("sliding")
    predict = infer.TiledPredictor(m, sliding, 1, batch=3)
    assert torch.equal(predict(x), infer.predict_logits_tiled(m, x, sliding, batch=3))


def test_two_headed_model_returns_a_tuple():
    _need_gpu()
    import Model
    from umi import infer
    m = Model.UNet_multitask(1, 2, 8, False, compute_dtype="fp32")
    m.load_state_dict(recipe.fill_state_dict(m.state_dict(), seed=22))
    m.to(DEV).eval()
    x, plan = _image(), _plan("overlap_tile")
    logits = infer.predict_logits_tiled(m, x, plan)
    masks = infer.predict_mask_tiled(m, x, plan)
    assert isinstance(logits, tuple) and isinstance(masks, tuple) and len(logits) == len(masks) == 2
    for lg, mk in zip(logits, masks):
        assert tuple(lg.shape[1:]) == (H_IMG, W_IMG) and tuple(mk.shape) == (H_IMG, W_IMG)
        assert torch.equal(mk, (infer.binary_mask if lg.shape[0] == 1 else infer.argmax_mask)(lg[None])[0])
    replay = infer.TiledPredictor(m, plan, 1)(x)
    assert isinstance(replay, tuple) and all(torch.equal(a, b) for a, b in zip(replay, logits))


def test_stitched_outputs_feed_the_counters_and_metrics_on_the_device():
    _need_gpu()
    import loss as L
    from umi import components as C, infer
    m, x, plan = _unet(2, "fp32"), _image(), _plan("overlap_tile")
    logits = infer.predict_logits_tiled(m, x, plan)
    mask = infer.predict_mask_tiled(m, x, plan)
    assert torch.equal(mask, infer.argmax_mask(logits[None])[0]) and 0 < mask.float().mean() < 1
    counts = infer.count_objects(mask, check=True)
    assert counts.is_cuda and counts.tolist() == C.label_components_numpy(mask.cpu().numpy()[None])[1].tolist()
    labels = (torch.rand((1, H_IMG, W_IMG), generator=torch.Generator().manual_seed(1)) < 0.4).long().to(DEV)
    L.CLASS_NUMBER = 2
    err = L.calc_loss(logits[None], labels, loss_type="dice_err_mc")
    assert err.is_cuda and 0.0 < float(err) < 1.0
    perfect = L.calc_loss(logits[None], mask[None].long(), loss_type="dice_err_mc")
    assert abs(float(perfect)) < 1e-6
