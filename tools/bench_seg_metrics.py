"""What the hard-mask metrics cost on one MI355X: the counting pass against a copy and against the fused loss on the same bytes,
and the validation phase with the score as a hard-mask metric.

    python tools/bench_seg_metrics.py [--out profiles/seg_metrics.json] [--rounds 9] [--items 64] [--k 16] [--only kernel|phase]

kernel  umi_confusion_logits + umi_confusion_scores on 16 items of 1 x C x 512 x 512 fp32 logits with int64 labels, C = 2 and 4,
        under two label / prediction distributions: `one_bin` (every pixel background predicted as background) and `uniform` (labels
        and predictions uniform over the classes).  Against, on the same inputs: a device-to-device copy of the same bytes
        (logits + labels; it also WRITES them) and umi_dice_ce_fwd_items, which reads the same bytes and does strictly more
        arithmetic per byte.  Every variant walks a ring of input copies larger than the 256 MiB Infinity Cache, so no call finds
        its inputs cached; one process, the variants take turns, device events around each call, medians over `--rounds` turns
        after a warm-up turn; `confusion_again` is the A/A measure of spread.
phase   the validation phase (tools/bench_validation.py `_phase`) of UNet(1,2,64) fp16 on `--items` items of 1 x 1 x 512 x 512,
        val_batch = k, eager-batched and replayed, with accuracy_metric = 'dice_bce_mc' (the score is the loss: free),
        'dice_err_mc' on the kernels and 'dice_err_mc' on the composite (loss.METRICS_KERNEL = False); device-kernel launches of
        one group's score (torch.profiler, when it can see the device) beside them."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import torch  # noqa: E402


def _inputs(C, dist, items, S, copies, seed=1):
    g = torch.Generator(device="cuda").manual_seed(seed)
    ring = []
    for _ in range(copies):
        if dist == "one_bin":
            x = torch.randn(items, C, S, S, device="cuda", generator=g) * 0.1
            x[:, 0] += 4.0
            t = torch.zeros(items, S, S, dtype=torch.int64, device="cuda")
        else:
            x = torch.randn(items, C, S, S, device="cuda", generator=g)
            t = torch.randint(0, C, (items, S, S), device="cuda", generator=g)
        ring.append((x, t))
    return ring


def time_kernels(rounds, items=16, S=512):
    import loss as L
    from umi import lib, metrics as M, ops
    rows = {}
    for C in (2, 4):
        for dist in ("one_bin", "uniform"):
            nbytes = items * S * S * (4 * C + 8)
            copies = max(3, (320 << 20) // nbytes + 1)
            ring = _inputs(C, dist, items, S, copies)
            dst = (torch.empty_like(ring[0][0]), torch.empty_like(ring[0][1]))
            L.CLASS_NUMBER = C

            def confusion(x, t):
                return M.scores(M.confusion(x, t, items), 0)

            def dice_ce(x, t):
                return L._dice_ce_items(x, t, items)

            def copy(x, t):
                dst[0].copy_(x)
                dst[1].copy_(t)
            variants = {"confusion": confusion, "dice_ce_fwd_items": dice_ce, "d2d_copy": copy, "confusion_again": confusion}
            turns = {v: [] for v in variants}
            calls = 0
            for r in range(rounds + 1):
                for v, fn in variants.items():
                    per = []
                    for _ in range(copies):
                        x, t = ring[calls % copies]
                        calls += 1
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        fn(x, t)
                        b.record()
                        b.synchronize()
                        per.append(a.elapsed_time(b) * 1e3)
                    if r:
                        turns[v].append(statistics.median(per))
            med = {v: statistics.median(t) for v, t in turns.items()}
            spread = abs(med["confusion"] - med["confusion_again"])
            mine = 0.5 * (med["confusion"] + med["confusion_again"])
            key = f"C={C} {dist}"
            rows[key] = {"items": items, "shape": f"1x{C}x{S}x{S}", "labels": "int64", "bytes_read": nbytes, "ring_copies": copies,
                         "rounds": rounds, "us": {v: round(t, 2) for v, t in med.items()},
                         "us_fastest": {v: round(min(t), 2) for v, t in turns.items()}, "aa_spread_us": round(spread, 2),
                         "read_GBps": {v: round(nbytes / (t * 1e-6) / 1e9, 1) for v, t in med.items()},
                         "confusion_over_dice_ce": round(mine / med["dice_ce_fwd_items"], 4),
                         "confusion_slower_than_dice_ce_by_more_than_the_spread": bool(mine - med["dice_ce_fwd_items"] > spread),
                         "ws_bytes": lib.fn("umi_confusion_ws_bytes")(items, 1, C, S * S)}
            print(json.dumps({key: rows[key]}), flush=True)
            del ring, dst
            torch.cuda.empty_cache()
    return rows


def _launches(fn):
    """Device kernels one call launches, or None where the profiler cannot see the device."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return n or None
    except Exception:                                                   # noqa: BLE001 -- a figure we then do not report
        return None


def time_phase(rounds, items, k):
    import loss as L
    import Model
    from Trainer import Trainer
    from tools.bench_validation import _phase, _val_items
    from umi import optim as uo
    L.CLASS_NUMBER = 2
    tmp = tempfile.mkdtemp(prefix="bench_seg_metrics_")
    torch.manual_seed(0)
    m = Model.UNet(1, 2, 64, compute_dtype="fp16").cuda()
    loaders = {"train": [0], "val": _val_items(items, 512)}
    variants = {}
    for graph in (False, True):
        tag = "replayed" if graph else "eager"
        variants[f"dice_bce_mc {tag}"] = ("dice_bce_mc", True, graph)
        variants[f"dice_err_mc kernel {tag}"] = ("dice_err_mc", True, graph)
        variants[f"dice_err_mc composite {tag}"] = ("dice_err_mc", False, graph)
        variants[f"dice_bce_mc {tag} again"] = ("dice_bce_mc", True, graph)
    trainers = {}
    for v, (metric, _, graph) in variants.items():
        opt = uo.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        trainers[v] = Trainer(m, "single", torch.cuda.FloatTensor, "cuda", os.path.join(tmp, v.replace(" ", "_")), loaders, 16, opt,
                              10 ** 6, 1, "dice_bce_mc", metric, lr_scheduler=None, val_batch=k, graph=graph)
    turns = {v: [] for v in variants}
    try:
        for r in range(rounds + 1):                                     # round 0 warms up: allocations, packs, the captures
            for v, tr in trainers.items():
                L.METRICS_KERNEL = variants[v][1]
                ms, _ = _phase(tr)
                if r:
                    turns[v].append(ms)
    finally:
        L.METRICS_KERNEL = True
    med = {v: statistics.median(t) for v, t in turns.items()}
    spread = {tag: abs(med[f"dice_bce_mc {tag}"] - med[f"dice_bce_mc {tag} again"]) for tag in ("eager", "replayed")}
    x, lab = torch.cat([i[0] for i in loaders["val"][:k]]), torch.cat([i[1] for i in loaders["val"][:k]])
    m.eval()
    with torch.no_grad():
        out = m(x)
    launches = {"dice_err_mc kernel": _launches(lambda: L.calc_loss_items(out, lab, k, loss_type="dice_err_mc"))}
    L.METRICS_KERNEL = False
    try:
        launches["dice_err_mc composite"] = _launches(lambda: L.calc_loss_items(out, lab, k, loss_type="dice_err_mc"))
    finally:
        L.METRICS_KERNEL = True
    row = {"workload": f"validation phase, UNet(1,2,64) fp16, {items} items of 1x1x512x512, val_batch={k}", "rounds": rounds,
           "phase_ms": {v: round(t, 3) for v, t in med.items()}, "phase_ms_fastest": {v: round(min(t), 3) for v, t in turns.items()},
           "aa_spread_ms": {t: round(s, 3) for t, s in spread.items()},
           "metric_cost_ms": {f"{how} {tag}": round(med[f"dice_err_mc {how} {tag}"] - med[f"dice_bce_mc {tag}"], 3)
                              for how in ("kernel", "composite") for tag in ("eager", "replayed")},
           "score_launches_per_group": launches, "multi_gpu": "unmeasured"}
    print(json.dumps({"phase": row}), flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "seg_metrics.json"))
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--only", choices=["kernel", "phase"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_seg_metrics.py needs an MI355X")
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
