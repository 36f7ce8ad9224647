"""Overlap-tile and sliding-window inference over an image larger than the network input: the host plan and the NumPy
statement of the three device kernels of csrc/tiles.hip (umi_tile_gather, umi_tile_blend, umi_tile_finish).

    plan = TilePlan.overlap_tile(H, W, 512, halo=64)                 # U-Net paper: mirrored context, only the tile's core kept
    plan = TilePlan.sliding(H, W, 512, overlap=128, window='gauss')  # windowed average of overlapping tiles
    logits = umi.infer.predict_logits_tiled(model, x, plan)          # fp32 (K, H, W) on the device

A plan is a grid of ny x nx equal th x tw tiles, tile id = iy * nx + ix, described by integers and small fp32 tables:
  oy[ny], ox[nx]   tile origins in image coordinates; they may be negative or run past H - th (the tile then hangs over the edge);
  wy[th], wx[tw]   the tile window per axis, evaluated in float64 and rounded once; the weight of tile pixel (i, j) is
                   fp32(wy[i] * wx[j]);
  sy[H], sx[W]     the window sums per axis, sy[y] = fp32(sum over the tiles, ascending, of wy[y - oy]) with the sum in float64;
                   the weights of all tiles at (y, x) add up to sy[y] * sx[x] up to rounding, which is what the finish divides by.

The statement is NumPy on np.float32 values only, every operation rounded on its own (NumPy has no fused multiply-add), and the
kernels match it bit for bit:
  gather   tile t, channel c, pixel (i, j) = x[c, r(oy + i), r(ox + j)] (pad 'reflect') or the constant where the sample lies
           outside the image (pad 'constant'); a slot with id < 0 is all zeros;
  blend    acc[k, p] = fp32(acc[k, p] + fp32(w * logit[t, k, i, j])) for the tiles of the chunk in the order given that contain p
           with w > 0.  A tile whose weight at p is 0 is skipped, not multiplied: what the network writes into a discarded halo,
           an inf or NaN included, never reaches the canvas;
  finish   out[k, y, x] = fp32(acc[k, y, x] / fp32(sy[y] * sx[x])).
Each canvas pixel sees its tiles in ascending id order however the id list is cut into chunks, so the result does not depend on
the chunk size.  Under overlap_tile every pixel lies in one core with weight 1 and sy = sx = 1: the stitched value is 0 + 1 * l, then
/ 1, the tile's logit itself."""
import numpy as np

# the kernels' limits (csrc/tiles.hip refuses the same with UMI_ERR_UNSUPPORTED)
MAX_TILE = 4096
MAX_GRID = 1024
MAX_CHUNK = 64
PAD_MODES = {"reflect": 0, "constant": 1}


def reflect_index(i, n):
    """numpy.pad(mode='reflect')'s source index of sample i of an axis of n, for every i (repeated reflection included)."""
    if n == 1:
        return 0
    p = 2 * (n - 1)
    m = i % p                                   # Python: non-negative
    return m if m < n else p - m


def _window(T, kind, sigma_scale):
    i = np.arange(T, dtype=np.float64)
    if kind == "flat":
        return np.ones(T, dtype=np.float64)
    if kind == "gauss":
        return np.exp(-0.5 * ((i - (T - 1) / 2.0) / (float(sigma_scale) * T)) ** 2)
    raise ValueError(f"window must be 'gauss' or 'flat', got {kind!r}")


def _sliding_origins(n, T, s):
    if n <= T:
        return [-((T - n) // 2)]
    return list(range(0, n - T, s)) + [n - T]


def _pair(tile):
    """tile = T or (th, tw)."""
    return (int(tile), int(tile)) if np.isscalar(tile) else (int(tile[0]), int(tile[1]))


class TilePlan:
    def __init__(self, H, W, tile, oy, ox, wy, wx, pad="reflect", pad_value=0.0):
        th, tw = _pair(tile)
        H, W = int(H), int(W)
        if H < 1 or W < 1 or th < 1 or tw < 1:
            raise ValueError(f"image {H}x{W} and tile {th}x{tw} must be positive")
        if pad not in PAD_MODES:
            raise ValueError(f"pad must be 'reflect' or 'constant', got {pad!r}")
        self.H, self.W, self.th, self.tw = H, W, th, tw
        self.pad, self.pad_value = pad, float(np.float32(pad_value))
        self.oy, self.ox = np.asarray(oy, dtype=np.int64).reshape(-1), np.asarray(ox, dtype=np.int64).reshape(-1)
        self.ny, self.nx = len(self.oy), len(self.ox)
        wy64, wx64 = np.asarray(wy, dtype=np.float64).reshape(-1), np.asarray(wx, dtype=np.float64).reshape(-1)
        if len(wy64) != th or len(wx64) != tw:
            raise ValueError(f"window tables of {len(wy64)} and {len(wx64)} entries for a {th}x{tw} tile")
        if self.ny < 1 or self.nx < 1:
            raise ValueError("a plan needs at least one tile per axis")
        if th > MAX_TILE or tw > MAX_TILE or self.ny > MAX_GRID or self.nx > MAX_GRID:
            raise ValueError(f"tile {th}x{tw} (at most {MAX_TILE}) or grid {self.ny}x{self.nx} (at most {MAX_GRID}) beyond the "
                             "kernels' limits")
        if H * W >= 2 ** 31 or th * tw >= 2 ** 31:
            raise ValueError(f"image {H}x{W} beyond the kernels' limits (H * W < 2**31)")
        for o, t, n in ((self.oy, th, H), (self.ox, tw, W)):
            if (o <= -2 ** 30).any() or (o >= 2 ** 30).any():
                raise ValueError("tile origin out of range")
        self.wy, self.wx = wy64.astype(np.float32), wx64.astype(np.float32)       # rounded once
        for w in (self.wy, self.wx):
            if not np.isfinite(w).all() or (w < 0).any():
                raise ValueError("a window table has a non-finite or negative entry")
        self.sy = self._sums(self.oy, self.wy, H)
        self.sx = self._sums(self.ox, self.wx, W)
        for s in (self.sy, self.sx):
            if not (s > 0).all() or not np.isfinite(s).all():
                raise ValueError("the tiles' windows leave a pixel of the image without weight (a window sum is not > 0)")
        self._dev = {}

    @staticmethod
    def _sums(origins, w, n):
        s = np.zeros(n, dtype=np.float64)
        for o in origins:                               # ascending tile order, float64
            lo, hi = max(0, int(o)), min(n, int(o) + len(w))
            if hi > lo:
                s[lo:hi] += w[lo - int(o):hi - int(o)].astype(np.float64)
        return s.astype(np.float32)

    @property
    def n_tiles(self):
        return self.ny * self.nx

    def origin(self, tile_id):
        return int(self.oy[tile_id // self.nx]), int(self.ox[tile_id % self.nx])

    @classmethod
    def overlap_tile(cls, H, W, tile, halo, pad="reflect", pad_value=0.0):
        """The U-Net paper's rule: tiles of `tile` pixels whose cores of tile - 2 * halo pixels partition the canvas; each tile
        sees `halo` pixels of context on every side, extrapolated by `pad` outside the image.  halo = 0 is the reference's
        non-overlapping tiling (test.py:437-448) for any image size."""
        (th, tw), halo = _pair(tile), int(halo)
        if halo < 0 or min(th, tw) - 2 * halo < 1:
            raise ValueError(f"tile {th}x{tw} with halo {halo} leaves no core (tile - 2 * halo must be >= 1)")

        def axis(n, T):
            w = np.zeros(T, dtype=np.float64)
            w[halo:T - halo] = 1.0
            return [-halo + k * (T - 2 * halo) for k in range(-(-int(n) // (T - 2 * halo)))], w

        (oy, wy), (ox, wx) = axis(H, th), axis(W, tw)
        return cls(H, W, (th, tw), oy, ox, wy, wx, pad, pad_value)

    @classmethod
    def sliding(cls, H, W, tile, overlap, window="gauss", sigma_scale=0.125, pad="reflect", pad_value=0.0):
        """The windowed sliding-window average: stride tile - overlap, the last tile pulled back to end at the image edge, a
        single centred tile on an axis no longer than the tile.  'gauss': w[i] = exp(-((i - (T-1)/2) / (sigma_scale * T))^2 / 2)."""
        (th, tw), overlap = _pair(tile), int(overlap)
        if not 0 <= overlap < min(th, tw):
            raise ValueError(f"overlap must be in 0..{min(th, tw) - 1}, got {overlap}")
        return cls(H, W, (th, tw), _sliding_origins(int(H), th, th - overlap), _sliding_origins(int(W), tw, tw - overlap),
                   _window(th, window, sigma_scale), _window(tw, window, sigma_scale), pad, pad_value)

    def chunks(self, batch):
        """The tile ids 0 .. n_tiles - 1 in ascending order as an int32 (n_chunks, batch) array, the last row padded with -1."""
        batch = int(batch)
        if not 1 <= batch <= MAX_CHUNK:
            raise ValueError(f"batch must be in 1..{MAX_CHUNK}, got {batch}")
        n = self.n_tiles
        ids = np.full(-(-n // batch) * batch, -1, dtype=np.int32)
        ids[:n] = np.arange(n, dtype=np.int32)
        return ids.reshape(-1, batch)

    def device_tables(self, device):
        """(oy, ox int32; wy, wx, sy, sx fp32) on `device`, uploaded once per device."""
        import torch
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in (
                self.oy.astype(np.int32), self.ox.astype(np.int32), self.wy, self.wx, self.sy, self.sx))
        return self._dev[key]


# ---- the statement ---------------------------------------------------------------------------------------------------------------
def _axis_source(o, t, n, pad):
    """Source index per tile sample of one axis, -1 where pad 'constant' applies."""
    idx = np.arange(o, o + t)
    if pad == "reflect":
        return np.array([reflect_index(int(i), n) for i in idx], dtype=np.int64)
    return np.where((idx >= 0) & (idx < n), idx, -1)


def gather_numpy(x, plan, ids):
    """x fp32 (C, H, W) -> fp32 (len(ids), C, th, tw)."""
    x = np.asarray(x, dtype=np.float32)
    C = x.shape[0]
    assert x.shape == (C, plan.H, plan.W)
    out = np.zeros((len(ids), C, plan.th, plan.tw), dtype=np.float32)
    for s, t in enumerate(ids):
        if t < 0:
            continue
        oy, ox = plan.origin(int(t))
        iy, ix = _axis_source(oy, plan.th, plan.H, plan.pad), _axis_source(ox, plan.tw, plan.W, plan.pad)
        tile = x[:, np.maximum(iy, 0)][:, :, np.maximum(ix, 0)]
        outside = (iy < 0)[:, None] | (ix < 0)[None, :]
        out[s] = np.where(outside[None], np.float32(plan.pad_value), tile)
    return out


def blend_numpy(acc, logits, plan, ids):
    """acc fp32 (K, H, W), updated in place and returned; logits fp32 (len(ids), K, th, tw)."""
    assert acc.dtype == np.float32 and logits.dtype == np.float32
    w = plan.wy[:, None] * plan.wx[None, :]                      # fp32 * fp32, rounded once
    assert w.dtype == np.float32
    for s, t in enumerate(ids):
        if t < 0:
            continue
        oy, ox = plan.origin(int(t))
        y0, y1, x0, x1 = max(0, oy), min(plan.H, oy + plan.th), max(0, ox), min(plan.W, ox + plan.tw)
        if y1 <= y0 or x1 <= x0:
            continue
        ws = w[y0 - oy:y1 - oy, x0 - ox:x1 - ox]
        take = ws > 0
        lt = logits[s][:, y0 - oy:y1 - oy, x0 - ox:x1 - ox]
        with np.errstate(invalid="ignore", over="ignore"):
            prod = ws[None] * lt                                  # rounded product ...
            view = acc[:, y0:y1, x0:x1]
            view[:, take] = (view + prod)[:, take]                # ... then a rounded add, only where the weight is > 0
    return acc


def finish_numpy(acc, plan):
    d = plan.sy[:, None] * plan.sx[None, :]
    assert d.dtype == np.float32 and acc.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        return acc / d[None]


def stitch_numpy(logits, plan, chunk=None):
    """All tiles' logits fp32 (n_tiles, K, th, tw) -> stitched fp32 (K, H, W), blended in chunks of `chunk` ids."""
    n = plan.n_tiles
    chunk = n if chunk is None else int(chunk)
    acc = np.zeros((logits.shape[1], plan.H, plan.W), dtype=np.float32)
    for a in range(0, n, chunk):
        ids = list(range(a, min(n, a + chunk)))
        blend_numpy(acc, logits[ids], plan, ids)
    return finish_numpy(acc, plan)


def stitch_float64(logits, plan):
    """sum w l / sum w in float64 from the fp32 tables (the yardstick of the rounding bound) and the number of tiles with
    w > 0 per pixel."""
    K = logits.shape[1]
    num, den = np.zeros((K, plan.H, plan.W)), np.zeros((plan.H, plan.W))
    cover = np.zeros((plan.H, plan.W), dtype=np.int64)
    w = plan.wy.astype(np.float64)[:, None] * plan.wx.astype(np.float64)[None, :]
    for t in range(plan.n_tiles):
        oy, ox = plan.origin(t)
        y0, y1, x0, x1 = max(0, oy), min(plan.H, oy + plan.th), max(0, ox), min(plan.W, ox + plan.tw)
        if y1 <= y0 or x1 <= x0:
            continue
        ws = w[y0 - oy:y1 - oy, x0 - ox:x1 - ox]
        lt = logits[t][:, y0 - oy:y1 - oy, x0 - ox:x1 - ox].astype(np.float64)
        num[:, y0:y1, x0:x1] += np.where(ws > 0, ws * lt, 0.0)
        den[y0:y1, x0:x1] += ws
        cover[y0:y1, x0:x1] += ws > 0
    return num / den[None], cover
