"""What batching and graph-replaying the Trainer's validation phase buys on one MI355X.

    python tools/bench_validation.py [--out profiles/validation_batched.json] [--rounds 7] [--items 64] [--k 16]
                                     [--only phase|epoch|split]

phase   the validation phase alone (model.eval(), the loop over the loader, the running sums, one read-back at the end) of
        UNet(1,2,64) fp16 on `--items` items of 1 x 1 x 512 x 512 and of TransUNet R50-ViT-B/16 fp16 on items of 1 x 1 x 224 x 224:
          items            today's path: eval_step item by item (val_batch=None)
          batched_eager    val_batch=k, graph=False
          batched_replay   val_batch=k, graph=True (the first full group eager, the second captured: both in the warm-up round)
          replay_slices    the same with the per-slice loss loop in place of umi_dice_ce_fwd_items (loss.ITEMS_KERNEL = False)
          items_again      today's path again: the A/A measure of spread
        One process, one model per workload, the variants take turns; medians over `--rounds` turns after a warm-up turn.
        Also recorded: that all variants gave the same loss sum (bits), under "same_sums".
epoch   one Trainer epoch of UNet(1,2,64) fp16, graph=True: 30 training steps at 16 x 512 x 512 plus `--items` validation items
        of one image, checkpoint writes included, with val_batch=None, val_batch=k and None again.
split   the epoch of profiles/trainer_data_parallel.json (30 graph-replayed steps at 16 x 512 x 512, 2 validation steps of 16
        images, checkpoint writes) divided into training steps, validation and checkpoint writes: host clocks around each part,
        each ending in a device synchronise."""
import argparse
import copy
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
from tqdm import tqdm  # noqa: E402


def _models():
    import Model
    from TransUnet.vit_seg_modeling import CONFIGS, VisionTransformer
    cfg = copy.deepcopy(CONFIGS["R50-ViT-B_16"])
    cfg.n_classes, cfg.n_skip, cfg.patches.grid = 2, 3, (224 // 16, 224 // 16)
    return {"UNet(1,2,64) fp16, 1x512x512": ("single", 512, lambda: Model.UNet(1, 2, 64, compute_dtype="fp16")),
            "TransUNet R50-ViT-B/16 fp16, 1x224x224": ("TransUnet", 224, lambda: VisionTransformer(
                cfg, img_size=224, num_classes=2, compute_dtype="fp16"))}


def _val_items(n, S, seed=1234):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(n, 1, S, S, device="cuda", generator=g)
    lab = torch.randint(0, 2, (n, S, S), device="cuda", generator=g).float()
    return [(x[i:i + 1], lab[i:i + 1]) for i in range(n)]


def _trainer(m, model_type, out, loaders, **kw):
    from Trainer import Trainer
    from umi import optim as uo
    opt = uo.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    return Trainer(m, model_type, torch.cuda.FloatTensor, "cuda", out, loaders, 16, opt, 10 ** 6, 1, "dice_bce_mc", "dice_bce_mc",
                   lr_scheduler=None, **kw)


def _phase(tr):
    """The validation phase of Trainer.singe_train for one epoch; returns (ms, loss sum)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tr.model.eval()
    with tqdm(tr.dataloader["val"], disable=True) as bar:
        if tr.val_batch is not None:
            loss_sum, score_sum, steps, _ = tr._validation().validate(bar, 1, True, "")
        else:
            loss_sum, score_sum, steps = None, None, 0
            for inputs, labels in bar:
                steps += 1
                loss, score = tr.eval_step(inputs, labels)
                score_sum = score if score_sum is None else score_sum + score
                loss_sum = loss if loss_sum is None else loss_sum + loss
    total = float(loss_sum) + 0.0 * float(score_sum)                 # the read-back that ends the phase
    return (time.perf_counter() - t0) * 1e3, total


def time_phase(rounds, items, k):
    import loss as L
    L.CLASS_NUMBER = 2
    tmp = tempfile.mkdtemp(prefix="bench_validation_")
    rows = {}
    for name, (model_type, S, make) in _models().items():
        torch.manual_seed(0)
        m = make().cuda()
        loaders = {"train": [0], "val": _val_items(items, S)}
        variants = {"items": dict(val_batch=None, graph=False), "batched_eager": dict(val_batch=k, graph=False),
                    "batched_replay": dict(val_batch=k, graph=True), "replay_slices": dict(val_batch=k, graph=True),
                    "items_again": dict(val_batch=None, graph=False)}
        trainers = {v: _trainer(m, model_type, os.path.join(tmp, v), loaders, **kw) for v, kw in variants.items()}
        turns, sums = {v: [] for v in variants}, {}
        for r in range(rounds + 1):                                    # round 0 warms up: allocations, packs, the captures
            for v, tr in trainers.items():
                L.ITEMS_KERNEL = v != "replay_slices"
                ms, total = _phase(tr)
                L.ITEMS_KERNEL = True
                sums.setdefault(v, total)
                assert sums[v] == total, (v, sums[v], total)           # a replay gives what the first turn gave
                if r:
                    turns[v].append(ms)
        assert all(len(trainers[v]._validation().graphs) == 1 for v in ("batched_replay", "replay_slices"))
        med = {v: statistics.median(t) for v, t in turns.items()}
        spread = abs(med["items"] - med["items_again"])
        base = 0.5 * (med["items"] + med["items_again"])
        kernel_gain = med["replay_slices"] - med["batched_replay"]
        rows[name] = {
            "items": items, "val_batch": k, "rounds": rounds,
            "phase_ms": {v: round(t, 3) for v, t in med.items()},
            "phase_ms_fastest": {v: round(min(t), 3) for v, t in turns.items()},
            "phase_ms_turns": {v: [round(x, 3) for x in t] for v, t in turns.items()},
            "aa_spread_ms": round(spread, 3),
            "per_item_ms": {v: round(t / items, 4) for v, t in med.items()},
            "replay_over_items": round(med["batched_replay"] / base, 4),
            "replay_beats_items_by_more_than_the_spread": bool(base - med["batched_replay"] > spread),
            "items_kernel_minus_slice_loop_ms": round(-kernel_gain, 3),
            "items_kernel_beats_slice_loop_by_more_than_the_spread": bool(kernel_gain > spread),
            "same_sums": len({repr(s) for s in sums.values()}) == 1, "loss_sums": sums}
        print(json.dumps({name: {a: b for a, b in rows[name].items() if a != "phase_ms_turns"}}), flush=True)
        del trainers, m
        torch.cuda.empty_cache()
    shutil.rmtree(tmp, ignore_errors=True)
    return rows


def _train_data(steps, B=16, S=512):
    g = torch.Generator(device="cuda").manual_seed(1234)
    x = torch.randn(B, 1, S, S, device="cuda", generator=g)
    lab = torch.randint(0, 2, (B, S, S), device="cuda", generator=g).float()
    return x, lab, [(x, lab)] * steps


def time_epoch(rounds, items, k, steps=30):
    import loss as L
    import Model
    L.CLASS_NUMBER = 2
    _, _, train = _train_data(steps)
    loaders = {"train": train, "val": _val_items(items, 512)}
    tmp = tempfile.mkdtemp(prefix="bench_validation_")
    trainers = {}
    for name, vb in (("none_a", None), ("val_batch", k), ("none_b", None)):
        torch.manual_seed(0)
        m = Model.UNet(1, 2, 64, compute_dtype="fp16").cuda()
        trainers[name] = _trainer(m, "single", os.path.join(tmp, name), loaders, graph=True, val_batch=vb)
    turns = {v: [] for v in trainers}
    for r in range(rounds + 1):
        for v, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.train()
            torch.cuda.synchronize()
            if r:
                turns[v].append((time.perf_counter() - t0) * 1e3)
    med = {v: statistics.median(t) for v, t in turns.items()}
    base = statistics.median(turns["none_a"] + turns["none_b"])
    row = {"workload": f"Trainer epoch, UNet(1,2,64) fp16, graph=True, {steps} training steps at 16x512x512 + {items} validation "
                       "items of one image, checkpoint writes included",
           "val_batch": k, "rounds": rounds, "epoch_ms": {v: round(t, 2) for v, t in med.items()},
           "epoch_ms_turns": {v: [round(x, 2) for x in t] for v, t in turns.items()},
           "aa_spread_ms": round(abs(med["none_a"] - med["none_b"]), 2),
           "val_batch_minus_none_ms": round(med["val_batch"] - base, 2), "val_batch_over_none": round(med["val_batch"] / base, 4),
           "eval_graphs": {v: len(tr._validation().graphs) for v, tr in trainers.items()},
           "val_loss_equal": len({repr(tr.val_loss_list) for tr in trainers.values()}) == 1}
    print(json.dumps({"epoch": row}), flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
    return row


def time_split(rounds, steps=30):
    """The epoch of profiles/trainer_data_parallel.json (data_parallel=None) with a clock on validation steps and checkpoint
    writes; training = the rest."""
    import loss as L
    import Model
    from Trainer import Trainer
    L.CLASS_NUMBER = 2
    x, lab, train = _train_data(steps)
    tmp = tempfile.mkdtemp(prefix="bench_validation_")
    torch.manual_seed(0)
    m = Model.UNet(1, 2, 64, compute_dtype="fp16").cuda()
    tr = _trainer(m, "single", tmp, {"train": train, "val": [(x, lab)] * 2}, graph=True)
    clock = {"val": 0.0, "save": 0.0}

    def timed(fn, key):
        def run(*a, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn(*a, **kw)
            torch.cuda.synchronize()
            clock[key] += (time.perf_counter() - t0) * 1e3
            return out
        return run
    real_save, real_eval = torch.save, Trainer.eval_step
    torch.save, Trainer.eval_step = timed(real_save, "save"), timed(real_eval, "val")
    rows = []
    try:
        for r in range(rounds + 1):
            clock["val"] = clock["save"] = 0.0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.train()
            torch.cuda.synchronize()
            total = (time.perf_counter() - t0) * 1e3
            if r:
                rows.append((total, clock["val"], clock["save"]))
    finally:
        torch.save, Trainer.eval_step = real_save, real_eval
    total, val, save = (statistics.median(c) for c in zip(*rows))
    row = {"workload": f"Trainer epoch, UNet(1,2,64) 16x512x512 fp16, graph=True, {steps} training + 2 validation steps of 16 images, "
                       "checkpoint writes (last_epoch.pt; epochN.pt and best.pt when the score improves)",
           "rounds": rounds, "epoch_ms": round(total, 2), "validation_ms": round(val, 2), "checkpoint_writes_ms": round(save, 2),
           "training_and_rest_ms": round(total - val - save, 2),
           "turns_ms_total_val_save": [[round(v, 2) for v in r_] for r_ in rows],
           "note": "the clocks add a device synchronise around each validation step and each torch.save"}
    print(json.dumps({"split": row}), flush=True)
    shutil.rmtree(tmp, ignore_errors=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "validation_batched.json"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--only", choices=["phase", "epoch", "split"])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_validation.py needs an MI355X")
    result = {"device": torch.cuda.get_device_name(0)}
    if os.path.exists(a.out):                                         # keep the parts this call does not measure (e.g. `drift`)
        with open(a.out) as f:
            result = {**json.load(f), **result}
    if a.only in (None, "phase"):
        result["validation_phase"] = time_phase(a.rounds, a.items, a.k)
    if a.only in (None, "epoch"):
        result["trainer_epoch"] = time_epoch(max(3, a.rounds // 2), a.items, a.k)
    if a.only in (None, "split"):
        result["epoch_split"] = time_split(max(3, a.rounds // 2))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
