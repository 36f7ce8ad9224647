"""What the surface-distance metrics cost on one MI355X: the kernels against the in-tree distance transform on the same masks and
against the host route, and the validation phase with 'hd95_mc' as the score.

    python tools/bench_surface_metrics.py [--out profiles/surface_metrics.json] [--rounds 9] [--items 64] [--k 16] [--only kernel|phase]

kernel  16 items of 1 x C x 512 x 512 fp32 logits with int64 labels, C = 2 and 4, blob-shaped masks (smooth random fields; the label
        field is the logits' field plus a perturbation, so the two boundaries run near each other as a prediction's do):
          surface      umi_argmax_mask + umi_surface_distances + umi_surface_scores ('hd95_mc', C - 1 foreground classes)
          hdt_fwd      umi_hdt_fwd on the class-1 masks of the same inputs: the in-tree yardstick for the field passes (one call
                       does two tensors' full fields; one class of `surface` does two surfaces' fields plus the select)
          host         the route a user has without the kernels: masks to the host and the NumPy statement, timed on 2 items
          surface_again  the A/A measure of spread
        Every device variant walks a ring of input copies larger than the 256 MiB Infinity Cache; one process, the variants take
        turns, device events around each call, medians over `--rounds` turns after a warm-up turn.  `kernels_us` lists the device
        kernels of one `surface` call with their durations (torch.profiler, where it can see the device).
phase   the validation phase (tools/bench_validation.py `_phase`) of UNet(1,2,64) fp16 on `--items` items of 1 x 1 x 512 x 512 with
        blob-shaped labels, val_batch = k, eager-batched and replayed, with accuracy_metric = 'hd95_mc' against 'dice_err_mc' in the
        same process ('dice_err_mc' twice: the A/A pair).  The untrained network's masks are noise-like, so nearly every predicted
        pixel is a surface pixel: the select's and the histograms' worst case, recorded with the surface counts."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def _smooth(g, n, C, S, cells=12):
    low = torch.randn(n, C, cells, cells, device="cuda", generator=g)
    return low, F.interpolate(low, size=(S, S), mode="bicubic", align_corners=False)


def _inputs(C, items, S, copies, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ring = []
    for _ in range(copies):
        low, x = _smooth(g, items, C, S)
        x[:, 0] += 0.5                                                  # some more background
        lab = F.interpolate(low + 0.35 * torch.randn(low.shape, device="cuda", generator=g), size=(S, S), mode="bicubic",
                            align_corners=False)
        lab[:, 0] += 0.5
        ring.append((x.contiguous(), lab.argmax(dim=1).contiguous()))
    return ring


def _kernel_times(fn):
    """{kernel name: us} of the device kernels one call launches, or None where the profiler cannot see the device."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        out = {}
        for e in prof.events():
            if str(getattr(e, "device_type", "")).endswith("CUDA"):
                name = e.name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0]
                out[name] = round(out.get(name, 0.0) + float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0)), 2)
        return out or None
    except Exception:                                                   # noqa: BLE001 -- a figure we then do not report
        return None


def time_kernels(rounds, items=16, S=512):
    import loss as L
    from umi import infer, lib, surface as SF
    rows = {}
    for C in (2, 4):
        nbytes = items * S * S * (4 * C + 8)
        copies = max(3, (320 << 20) // nbytes + 1)
        ring = _inputs(C, items, S, copies)
        hdt_ring = [((x[:, 1:2] - x[:, 0:1]).contiguous(), (t == 1).float().unsqueeze(1).contiguous()) for x, t in ring]
        hdt = L.HausdorffDTLoss()

        def surface(i):
            x, t = ring[i]
            return L.calc_loss_items(x, t, items, loss_type="hd95_mc")

        def hdt_fwd(i):
            return hdt(*hdt_ring[i])
        variants = {"surface": surface, "hdt_fwd": hdt_fwd, "surface_again": surface}
        turns = {v: [] for v in variants}
        calls = 0
        with torch.no_grad():
            for r in range(rounds + 1):
                for v, fn in variants.items():
                    per = []
                    for _ in range(copies):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        fn(calls % copies)
                        b.record()
                        b.synchronize()
                        calls += 1
                        per.append(a.elapsed_time(b) * 1e3)
                    if r:
                        turns[v].append(statistics.median(per))
            kernels = _kernel_times(lambda: surface(0))
            stats, counts = SF.surface(infer.argmax_mask(ring[0][0]), ring[0][1], C, 1)
        x, t = ring[0]
        mask = infer.argmax_mask(x[:2])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_stats, _ = SF.surface_numpy(mask.cpu().numpy(), t[:2].cpu().numpy(), C, 1)
        SF.surface_scores_numpy(host_stats, 2, "hd95", 1, "diagonal", (S, S))
        host_us = (time.perf_counter() - t0) * 1e6 * items / 2           # 2 items timed, scaled to all
        med = {v: statistics.median(t) for v, t in turns.items()}
        spread = abs(med["surface"] - med["surface_again"])
        mine = 0.5 * (med["surface"] + med["surface_again"])
        key = f"C={C} blobs"
        rows[key] = {"items": items, "shape": f"1x{C}x{S}x{S}", "labels": "int64", "foreground_classes": C - 1, "ring_copies": copies,
                     "rounds": rounds, "us": {v: round(t, 2) for v, t in med.items()},
                     "us_fastest": {v: round(min(t), 2) for v, t in turns.items()}, "aa_spread_us": round(spread, 2),
                     "host_us_scaled_from_2_items": round(host_us, 0),
                     "surface_over_hdt_fwd": round(mine / med["hdt_fwd"], 3),
                     "surface_per_class_over_hdt_fwd": round(mine / (C - 1) / med["hdt_fwd"], 3),
                     "host_over_surface": round(host_us / mine, 1), "kernels_us": kernels,
                     "surface_pixels_per_image_and_class": round(float(counts[:, 1:].sum()) / (items * (C - 1)), 1),
                     "states": torch.bincount(stats[:, 1:, 3].long().reshape(-1), minlength=4).tolist(),
                     "ws_bytes": lib.fn("umi_surface_ws_bytes")(items, C, 1, S, S)}
        print(json.dumps({key: rows[key]}), flush=True)
        del ring, hdt_ring
        torch.cuda.empty_cache()
    return rows


def _val_items(n, S, seed=1234):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, 1, S, S, device="cuda", generator=g)
    lab = _smooth(g, n, 2, S)[1].argmax(dim=1).float()
    return [(x[i:i + 1], lab[i:i + 1].contiguous()) for i in range(n)]


def time_phase(rounds, items, k):
    import loss as L
    import Model
    from Trainer import Trainer
    from tools.bench_validation import _phase
    from umi import infer, optim as uo, surface as SF
    L.CLASS_NUMBER = 2
    tmp = tempfile.mkdtemp(prefix="bench_surface_metrics_")
    torch.manual_seed(0)
    m = Model.UNet(1, 2, 64, compute_dtype="fp16").cuda()
    loaders = {"train": [0], "val": _val_items(items, 512)}
    variants = {}
    for graph in (False, True):
        tag = "replayed" if graph else "eager"
        variants[f"dice_err_mc {tag}"] = ("dice_err_mc", graph)
        variants[f"hd95_mc {tag}"] = ("hd95_mc", graph)
        variants[f"dice_err_mc {tag} again"] = ("dice_err_mc", graph)
    trainers = {}
    for v, (metric, graph) in variants.items():
        opt = uo.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        trainers[v] = Trainer(m, "single", torch.cuda.FloatTensor, "cuda", os.path.join(tmp, v.replace(" ", "_")), loaders, 16, opt,
                              10 ** 6, 1, "dice_bce_mc", metric, lr_scheduler=None, val_batch=k, graph=graph)
    turns = {v: [] for v in variants}
    for r in range(rounds + 1):                                         # round 0 warms up: allocations, packs, the captures
        for v, tr in trainers.items():
            ms, _ = _phase(tr)
            if r:
                turns[v].append(ms)
    med = {v: statistics.median(t) for v, t in turns.items()}
    spread = {tag: abs(med[f"dice_err_mc {tag}"] - med[f"dice_err_mc {tag} again"]) for tag in ("eager", "replayed")}
    x, lab = torch.cat([i[0] for i in loaders["val"][:k]]), torch.cat([i[1] for i in loaders["val"][:k]])
    m.eval()
    with torch.no_grad():
        out = m(x)
        kernels = _kernel_times(lambda: L.calc_loss_items(out, lab, k, loss_type="hd95_mc"))
        _, counts = SF.surface(infer.argmax_mask(out), lab, 2, 1)
    row = {"workload": f"validation phase, UNet(1,2,64) fp16 (untrained: noise-like masks), {items} items of 1x1x512x512 with blob "
                       f"labels, val_batch={k}", "rounds": rounds,
           "phase_ms": {v: round(t, 3) for v, t in med.items()}, "phase_ms_fastest": {v: round(min(t), 3) for v, t in turns.items()},
           "aa_spread_ms": {t: round(s, 3) for t, s in spread.items()},
           "hd95_cost_ms": {tag: round(med[f"hd95_mc {tag}"] - 0.5 * (med[f"dice_err_mc {tag}"] + med[f"dice_err_mc {tag} again"]), 3)
                            for tag in ("eager", "replayed")},
           "hd95_over_dice_err": {tag: round(med[f"hd95_mc {tag}"] / (0.5 * (med[f"dice_err_mc {tag}"] + med[f"dice_err_mc {tag} again"])), 4)
                                  for tag in ("eager", "replayed")},
           "score_kernels_us_per_group": kernels,
           "surface_pixels_per_image": {"prediction": round(float(counts[:, 1, 0].sum()) / k, 1), "label": round(float(counts[:, 1, 1].sum()) / k, 1)},
           "multi_gpu": "unmeasured"}
    print(json.dumps({"phase": row}), flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "surface_metrics.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--only", choices=["kernel", "phase"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_surface_metrics.py needs an MI355X")
    result = {"device": torch.cuda.get_device_name(0)}
    if os.path.exists(a.out):
        with open(a.out) as f:
            result = {**json.load(f), **result}
    if a.only in (None, "kernel"):
        result["kernels"] = time_kernels(a.rounds)
    if a.only in (None, "phase"):
        result["validation_phase"] = time_phase(max(3, a.rounds // 2), a.items, a.k)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
