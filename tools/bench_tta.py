"""What test-time augmentation costs on one MI355X, and the accuracy of the device expf / logf its 'prob' bound rests on.

    python tools/bench_tta.py [--out profiles/tta.json] [--rounds 7] [--only math|kernel|predict]

math     builds tools/tta_math_ulp.hip with the library's flags and runs it: the largest error of the device expf on [-60, 20] and
         logf on (0, 1] against float64, in units in the last place ("math_ulp"; umi.tta.EXPF_ULP / LOGF_ULP state the result).
kernel   umi_tta_views (C = 3), umi_tta_accumulate and umi_tta_finish (K = 2, 'prob', with mask and entropy) over a 4 x . x 512 x 512
         batch with all views in one call -- 'd4' (V = 8, even and odd turns: the tile kernels with LDS staging) and 'flips' (V = 4,
         even turns: the row kernels with 16-byte accesses) -- each against a one-launch device-to-device copy that moves the same
         number of bytes (a copy of B / 2 bytes reads and writes B).  Device events around one call: the wrapper's host time counts.
           views       reads V and writes V * N * C * H * W floats (the image is read once per view);
           accumulate  reads V * N * K * H * W outputs, reads and writes N * K * H * W sums;
           finish      reads and writes N * K * H * W floats, writes N * H * W mask bytes and N * H * W entropy floats.
         Every variant walks a ring of inputs larger than the 256 MiB Infinity Cache.
predict  UNet(1, 2, 64) fp16 on a 1 x 1 x 512 x 512 image: infer.predict_mask_tta with 'd4' ('prob'), eager and through
         infer.TTAPredictor, against eight plain infer.predict_mask calls (the forwards alone, one image each) and against the torch
         composite over the same batched forward (rot90 / flip / cat -> model -> softmax -> rot90 / flip back -> stack -> mean ->
         argmax).
One process, the variants take turns, device events around each call, medians over `--rounds` turns after a warm-up turn; `*_again` is
the A/A spread.  There is no gate: the ratios are recorded."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import torch  # noqa: E402

S, N, C, K = 512, 4, 3, 2
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


def _ring(nbytes, make):
    return [make() for _ in range(max(3, CACHE // nbytes + 1))]


def measure_math():
    from umi import build
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "tta_math_ulp")
        subprocess.check_call([build.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", os.path.join(REPO, "tools", "tta_math_ulp.hip"),
                               "-o", exe])
        row = json.loads(subprocess.check_output([exe], text=True, timeout=300))
    print(json.dumps({"math_ulp": row}), flush=True)
    return row


def time_kernels(rounds):
    """'d4' mixes even and odd turns: the 32 x 32 tile kernels with LDS staging; 'flips' has even turns only: the row kernels with
    16-byte accesses."""
    rows = {}
    for views in ("d4", "flips"):
        rows[views] = _time_kernels(rounds, views)
        torch.cuda.empty_cache()
    return rows


def _time_kernels(rounds, views):
    from umi import tta as T
    els = T.view_set(views)
    V = len(els)
    img, out = N * C * S * S, N * K * S * S
    moved = {"views": 2 * V * img * 4, "accumulate": (V + 2) * out * 4, "finish": 2 * out * 4 + N * S * S * 5}
    g = torch.Generator(device="cuda").manual_seed(1)
    images = _ring(img * 4, lambda: torch.randn(N, C, S, S, device="cuda", generator=g))
    viewed = torch.empty((V * N, C, S, S), device="cuda")
    outputs = _ring(V * out * 4, lambda: torch.randn(V * N, K, S, S, device="cuda", generator=g))
    sums = _ring(out * 4, lambda: torch.rand(N, K, S, S, device="cuda", generator=g))
    copies = {k: (_ring(b // 2, lambda b=b: torch.empty(b // 8, device="cuda").normal_(generator=g)), torch.empty(b // 8, device="cuda"))
              for k, b in moved.items()}

    def copy_of(k):
        ring, dst = copies[k]
        return lambda i: dst.copy_(ring[i % len(ring)])
    variants = {"views": lambda i: T.views(images[i % len(images)], els, out=viewed),
                "accumulate": lambda i: T.accumulate(sums[i % len(sums)], outputs[i % len(outputs)], els, "prob"),
                "finish": lambda i: T.finish(sums[i % len(sums)], V, "prob", mask=True, entropy=True)}
    variants.update({f"{k}_copy": copy_of(k) for k in moved})
    variants.update({f"{k}_again": variants[k] for k in moved})
    med, fastest = _turns(variants, rounds, inner=5)
    row = {"batch": f"{N}x.x{S}x{S} (C={C}, K={K}), views {views} in one call, mode prob", "rounds": rounds, "bytes_moved": moved,
           "us": {v: round(t, 2) for v, t in med.items()}, "us_fastest": {v: round(t, 2) for v, t in fastest.items()}}
    for k in moved:
        mine = 0.5 * (med[k] + med[f"{k}_again"])
        row[k] = {"aa_spread_us": round(abs(med[k] - med[f"{k}_again"]), 2), "GBps": round(moved[k] / (mine * 1e-6) / 1e9, 1),
                  "copy_GBps": round(moved[k] / (med[f"{k}_copy"] * 1e-6) / 1e9, 1), "over_copy": round(mine / med[f"{k}_copy"], 3)}
    print(json.dumps({"kernels": {views: row}}), flush=True)
    return row


def _composite(m, x, els):
    """The torch composite over one batched forward: what a user writes by hand today."""
    def view(t, e):
        r = torch.rot90(t, e & 3, dims=(-2, -1))
        return torch.flip(r, dims=(-1,)) if e >> 2 else r

    def unview(t, e):
        r = torch.flip(t, dims=(-1,)) if e >> 2 else t
        return torch.rot90(r, -(e & 3), dims=(-2, -1))
    n = x.shape[0]
    out = m(torch.cat([view(x, e) for e in els]).contiguous())
    probs = torch.softmax(out, dim=1)
    mean = torch.stack([unview(probs[s * n:(s + 1) * n], e) for s, e in enumerate(els)]).mean(dim=0)
    return mean.argmax(dim=1).to(torch.uint8)


def time_predict(rounds):
    import Model
    from umi import infer
    from umi import tta as T
    torch.manual_seed(0)
    m = Model.UNet(1, 2, 64, compute_dtype="fp16").cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.randn(1, 1, S, S, device="cuda", generator=g)
    els = T.view_set("d4")
    replay = infer.TTAPredictor(m, x, "d4", "prob")
    with torch.no_grad():
        want = infer.predict_mask_tta(m, x, "d4", "prob")
        agree = {"replayed_equals_eager": bool(torch.equal(replay.predict_mask(x), want)),
                 "composite_mask_agreement": float((_composite(m, x, els) == want).float().mean())}

        def plain(i):
            for _ in els:
                infer.predict_mask(m, x)
        variants = {"eight predict_mask": plain, "tta eager": lambda i: infer.predict_mask_tta(m, x, "d4", "prob"),
                    "tta replayed": lambda i: replay.predict_mask(x), "torch composite": lambda i: _composite(m, x, els),
                    "eight predict_mask again": plain}
        med, fastest = _turns(variants, rounds)
    spread = abs(med["eight predict_mask"] - med["eight predict_mask again"])
    base = 0.5 * (med["eight predict_mask"] + med["eight predict_mask again"])
    row = {"workload": f"UNet(1,2,64) fp16, 1x1x{S}x{S}, views d4, mode prob", "rounds": rounds,
           "ms": {v: round(t / 1e3, 3) for v, t in med.items()}, "ms_fastest": {v: round(t / 1e3, 3) for v, t in fastest.items()},
           "aa_spread_ms": round(spread / 1e3, 3), **agree,
           "over_eight_predict_mask": {k: round(med[k] / base, 4) for k in ("tta eager", "tta replayed", "torch composite")},
           "tta_over_torch_composite": {k: round(med[f"tta {k}"] / med["torch composite"], 4) for k in ("eager", "replayed")},
           "tta_beats_composite_by_more_than_the_spread": {k: bool(med["torch composite"] - med[f"tta {k}"] > spread)
                                                           for k in ("eager", "replayed")},
           "multi_gpu": "unmeasured"}
    print(json.dumps({"predict": row}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "tta.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", choices=["math", "kernel", "predict"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_tta.py needs an MI355X")
    result = {"device": torch.cuda.get_device_name(0)}
    if os.path.exists(a.out):
        with open(a.out) as f:
            result = {**json.load(f), **result}
    if a.only in (None, "math"):
        result["math_ulp"] = measure_math()
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
