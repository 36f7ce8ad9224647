"""What overlap-tile inference costs on one MI355X: the three stitch kernels against a copy of the bytes they move, and whole-image
prediction against the existing one-tile-per-forward loop.

    python tools/bench_tiles.py [--out profiles/tiled_inference.json] [--rounds 9] [--only kernel|predict]

kernel   umi_tile_gather (C = 3), umi_tile_blend and umi_tile_finish (K = 2, with the mask) over one 2048 x 2048 image, tile 512, in
         chunks of 8 tiles, under TilePlan.overlap_tile(halo 64) (6 x 6 tiles) and TilePlan.sliding(overlap 128, gauss) (5 x 5).
         Each against a device-to-device copy that moves the same number of bytes (a copy of B / 2 bytes reads and writes B):
           gather  reads and writes n * C * T^2 floats;
           blend   reads n * K * T^2 logits, reads and writes the canvas pixels the tiles cover with a weight > 0 (once per chunk
                   that touches them), K planes;
           finish  reads and writes K * H * W floats, writes H * W mask bytes.
         Every variant walks a ring of input copies larger than the 256 MiB Infinity Cache; one process, the variants take turns,
         device events around each whole-image pass, medians over `--rounds` turns after a warm-up turn; `*_again` is the A/A spread.
predict  UNet(1, 1, 64) fp16 on a 1 x 1 x 2048 x 2048 image, tile 512: infer.predict_binary_mask_tiled (the existing loop, one tile
         per forward), infer.predict_mask_tiled with overlap_tile halo 0, batch 8, eager, the same through infer.TiledPredictor,
         and both at halo 64 (36 tiles instead of 16).  Acceptance: at halo 0 neither new path is slower than the existing loop by
         more than the A/A spread (the loop measured twice).  The stitch kernels' share: their three times on the same shapes
         (C = K = 1), measured alone, over the eager total."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

S, TILE, BATCH = 2048, 512, 8
CACHE = 320 << 20


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3                                       # us


def _turns(variants, rounds, inner=1):
    """variants {name: fn(call_index)} take turns; median per turn of `inner` calls, medians over the turns after a warm-up."""
    turns = {v: [] for v in variants}
    calls = 0
    for r in range(rounds + 1):
        for v, fn in variants.items():
            per = []
            for _ in range(inner):
                i = calls
                calls += 1
                per.append(_timed(lambda: fn(i)))
            if r:
                turns[v].append(statistics.median(per))
    return {v: statistics.median(t) for v, t in turns.items()}, {v: min(t) for v, t in turns.items()}


def _covered(plan, chunks):
    """Canvas pixels a chunked blend reads and writes: per chunk, the pixels some tile of the chunk covers with a weight > 0."""
    w = (plan.wy[:, None] * plan.wx[None, :]) > 0
    total = 0
    for row in chunks:
        m = np.zeros((plan.H, plan.W), dtype=bool)
        for t in row[row >= 0]:
            oy, ox = plan.origin(int(t))
            y0, y1, x0, x1 = max(0, oy), min(plan.H, oy + plan.th), max(0, ox), min(plan.W, ox + plan.tw)
            m[y0:y1, x0:x1] |= w[y0 - oy:y1 - oy, x0 - ox:x1 - ox]
        total += int(m.sum())
    return total


def _ring(nbytes, make):
    return [make() for _ in range(max(3, CACHE // nbytes + 1))]


def time_kernels(rounds, C=3, K=2):
    from umi import infer
    from umi.tiles import TilePlan
    rows = {}
    for name, plan in (("overlap_tile halo 64", TilePlan.overlap_tile(S, S, TILE, 64)),
                       ("sliding overlap 128 gauss", TilePlan.sliding(S, S, TILE, 128))):
        chunks = plan.chunks(BATCH)
        ids = torch.from_numpy(chunks).to("cuda")
        n, nc = plan.n_tiles, len(chunks)
        tile_f = TILE * TILE
        moved = {"gather": 2 * n * C * tile_f * 4,
                 "blend": n * K * tile_f * 4 + 2 * K * _covered(plan, chunks) * 4,
                 "finish": 2 * K * S * S * 4 + S * S}
        g = torch.Generator(device="cuda").manual_seed(1)
        images = _ring(C * S * S * 4, lambda: torch.randn(C, S, S, device="cuda", generator=g))
        tiles = torch.empty((nc, BATCH, C, TILE, TILE), device="cuda")
        logits = _ring(nc * BATCH * K * tile_f * 4, lambda: torch.randn(nc, BATCH, K, TILE, TILE, device="cuda", generator=g))
        canvases = _ring(K * S * S * 4, lambda: torch.randn(K, S, S, device="cuda", generator=g))
        copies = {k: (_ring(b // 2, lambda b=b: torch.empty(b // 8, device="cuda").normal_(generator=g)), torch.empty(b // 8, device="cuda"))
                  for k, b in moved.items()}

        def gather(i):
            x = images[i % len(images)]
            for c in range(nc):
                infer.tile_gather(x, plan, ids[c], tiles[c])

        def blend(i):
            lg, acc = logits[i % len(logits)], canvases[i % len(canvases)]
            for c in range(nc):
                infer.tile_blend(acc, lg[c], plan, ids[c])

        def finish(i):
            infer.tile_finish(canvases[i % len(canvases)], plan, mask=True)

        def copy_of(k):
            ring, dst = copies[k]
            return lambda i: dst.copy_(ring[i % len(ring)])
        variants = {"gather": gather, "gather_copy": copy_of("gather"), "blend": blend, "blend_copy": copy_of("blend"),
                    "finish": finish, "finish_copy": copy_of("finish"), "gather_again": gather, "blend_again": blend,
                    "finish_again": finish}
        med, fastest = _turns(variants, rounds, inner=5)
        row = {"image": f"{C}x{S}x{S} (K={K})", "tile": TILE, "tiles": n, "chunks": nc, "chunk_slots": BATCH, "rounds": rounds,
               "launches": {"gather": nc, "blend": nc, "finish": 1}, "bytes_moved": moved,
               "us": {v: round(t, 2) for v, t in med.items()}, "us_fastest": {v: round(t, 2) for v, t in fastest.items()}}
        for k in moved:
            mine = 0.5 * (med[k] + med[f"{k}_again"])
            row[k] = {"aa_spread_us": round(abs(med[k] - med[f"{k}_again"]), 2), "GBps": round(moved[k] / (mine * 1e-6) / 1e9, 1),
                      "copy_GBps": round(moved[k] / (med[f"{k}_copy"] * 1e-6) / 1e9, 1), "over_copy": round(mine / med[f"{k}_copy"], 3)}
        rows[name] = row
        print(json.dumps({name: row}), flush=True)
        del images, tiles, logits, canvases, copies
        torch.cuda.empty_cache()
    return rows


def time_predict(rounds):
    import Model
    from umi import infer
    from umi.tiles import TilePlan
    torch.manual_seed(0)
    m = Model.UNet(1, 1, 64, compute_dtype="fp16").cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn(1, 1, S, S, device="cuda", generator=g)
    plans = {0: TilePlan.overlap_tile(S, S, TILE, 0), 64: TilePlan.overlap_tile(S, S, TILE, 64)}
    replay = {h: infer.TiledPredictor(m, p, 1, batch=BATCH) for h, p in plans.items()}
    want = infer.predict_binary_mask_tiled(m, x, TILE)
    same = {"eager": bool(torch.equal(infer.predict_mask_tiled(m, x, plans[0], batch=BATCH), want)),
            "replayed": bool(torch.equal(replay[0].predict_mask(x), want))}
    variants = {"existing loop": lambda i: infer.predict_binary_mask_tiled(m, x, TILE)}
    for h, p in plans.items():
        variants[f"halo {h} eager"] = lambda i, p=p: infer.predict_mask_tiled(m, x, p, batch=BATCH)
        variants[f"halo {h} replayed"] = lambda i, h=h: replay[h].predict_mask(x)
    variants["existing loop again"] = variants["existing loop"]
    med, fastest = _turns(variants, rounds)
    spread = abs(med["existing loop"] - med["existing loop again"])
    base = 0.5 * (med["existing loop"] + med["existing loop again"])
    stitch = {}
    for h, p in plans.items():                                          # the stitch kernels alone, on the shapes of the prediction
        ids = torch.from_numpy(p.chunks(BATCH)).to("cuda")
        tiles = torch.empty((BATCH, 1, TILE, TILE), device="cuda")
        lg = torch.randn(BATCH, 1, TILE, TILE, device="cuda", generator=g)
        acc = torch.zeros(1, S, S, device="cuda")

        def run(i):
            acc.zero_()
            for c in range(ids.shape[0]):
                infer.tile_gather(x[0], p, ids[c], tiles)
                infer.tile_blend(acc, lg, p, ids[c])
            infer.tile_finish(acc, p, mask=True)
        stitch[h] = _turns({"stitch": run}, rounds, inner=3)[0]["stitch"]
    row = {"workload": f"UNet(1,1,64) fp16, 1x1x{S}x{S}, tile {TILE}, batch {BATCH}", "rounds": rounds,
           "tiles": {f"halo {h}": p.n_tiles for h, p in plans.items()},
           "ms": {v: round(t / 1e3, 3) for v, t in med.items()}, "ms_fastest": {v: round(t / 1e3, 3) for v, t in fastest.items()},
           "aa_spread_ms": round(spread / 1e3, 3), "mask_equals_existing_loop": same,
           "halo_0_over_existing": {k: round(med[f"halo 0 {k}"] / base, 4) for k in ("eager", "replayed")},
           "halo_0_slower_than_existing_by_more_than_the_spread": {k: bool(med[f"halo 0 {k}"] - base > spread)
                                                                   for k in ("eager", "replayed")},
           "halo_64_over_halo_0": {k: round(med[f"halo 64 {k}"] / med[f"halo 0 {k}"], 4) for k in ("eager", "replayed")},
           "stitch_kernels_ms": {f"halo {h}": round(t / 1e3, 3) for h, t in stitch.items()},
           "stitch_share_of_eager": {f"halo {h}": round(stitch[h] / med[f"halo {h} eager"], 4) for h in plans},
           "multi_gpu": "unmeasured"}
    print(json.dumps({"predict": row}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tiled_inference.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--only", choices=["kernel", "predict"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_tiles.py needs an MI355X")
    result = {"device": torch.cuda.get_device_name(0)}
    if os.path.exists(a.out):
        with open(a.out) as f:
            result = {**json.load(f), **result}
    if a.only in (None, "kernel"):
        result["kernels"] = time_kernels(a.rounds)
    if a.only in (None, "predict"):
        result["whole_image"] = time_predict(a.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
