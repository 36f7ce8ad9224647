"""Whole-network parity of the BENCHMARKED path: UNet(cin, ncls, 64) in fp16 storage (every MFMA tile configuration of the
bench workload is live at these channel widths) against the CPU oracle, fp32 and with the same fp16 rounding points.

Runs as a child of tests/test_gpu_unet.py::test_unet_fp16_feat64_benchmark_widths with UMI_TRACE_GENERIC=1 (the library then
reports every convolution / weight gradient that falls back to the generic VALU kernels on stderr; the test asserts there
is none) and prints ONE JSON line with the measurements; `--out FILE` also writes it (profiles/r02_fp16_feat64_parity.json is
such a run).  --height / --width (default: --size) give a ragged input: floor in every pool, zero-filled pad + offset scatter in
the transposed convs, the odd-tail pool backward.  --model multitask: UNet_multitask against RefUNetMultitask, the loss summed
over both heads (labels of seeds S and S + 100), logits and argmax masks compared per head (the worst head is reported, the
pixel counts are totals).
usage: python tools/check_fp16_feat64.py CIN NCLS [--size 64] [--height H] [--width W] [--model unet|multitask] [--batch 2] [--out FILE]"""
import argparse, json, os, sys
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "unet-torch_amd")]
import numpy as np
import torch
import Model
import loss as L
from oracle import recipe, ref_unet

ap = argparse.ArgumentParser()
ap.add_argument("cin", type=int)
ap.add_argument("ncls", type=int)
ap.add_argument("--size", type=int, default=64)
ap.add_argument("--height", type=int)
ap.add_argument("--width", type=int)
ap.add_argument("--model", choices=["unet", "multitask"], default="unet")
ap.add_argument("--batch", type=int, default=2)
ap.add_argument("--seed", type=int, default=64)
ap.add_argument("--out")
a = ap.parse_args()
DEV, F = "cuda", 64
H, W = a.height or a.size, a.width or a.size
MT = a.model == "multitask"
RefNet = ref_unet.RefUNetMultitask if MT else ref_unet.RefUNet
L.CLASS_NUMBER = a.ncls
torch.set_num_threads(min(16, os.cpu_count() or 1))


def rel(x, y):
    x, y = x.detach().double().cpu(), y.detach().double().cpu()
    return ((x - y).norm() / (y.norm() + 1e-30)).item()


def cos(x, y):
    x, y = x.detach().double().cpu().flatten(), y.detach().double().cpu().flatten()
    return (x @ y / (x.norm() * y.norm() + 1e-30)).item()


def heads(out):
    return list(out) if MT else [out]


def total_loss(outs, fn):
    """dice_bce_mc summed over the heads, head i against labs[i]."""
    return sum(fn(o, l) for o, l in zip(outs, labs))


ref = RefNet(a.cin, a.ncls, F, False)
ref.load_state_dict(recipe.fill_state_dict(ref.state_dict(), seed=a.seed))
x, lab = recipe.synthetic_batch(a.batch, a.cin, H, W, a.ncls, seed=a.seed)
labs = [lab] + ([recipe.synthetic_batch(a.batch, a.cin, H, W, a.ncls, seed=a.seed + 100)[1]] if MT else [])

m = (Model.UNet_multitask if MT else Model.UNet)(a.cin, a.ncls, F, False, compute_dtype="fp16")
m.load_state_dict(ref.state_dict())
m.to(DEV).train()
logits = heads(m(x.to(DEV)))
loss = total_loss(logits, lambda o, l: L.calc_loss(o, l.to(DEV), loss_type="dice_bce_mc"))
loss.backward()
torch.cuda.synchronize()
logits = [o.detach().float().cpu() for o in logits]

ref.train()
rl = heads(ref(x))
rloss = total_loss(rl, lambda o, l: ref_unet.dice_bce_mc(o, l, a.ncls))
rloss.backward()
rl = [o.detach() for o in rl]


def quant_run(noise):
    q = RefNet(a.cin, a.ncls, F, False, quant="fp16")
    q.load_state_dict(ref.state_dict())
    q.train()
    q.noise = noise
    ql = heads(q(x))
    qloss = total_loss(ql, lambda o, l: ref_unet.dice_bce_mc(o, l, a.ncls))
    qloss.backward()
    return q, [o.detach() for o in ql], qloss.item()


q, ql, qloss = quant_run(0.0)
qn, _, _ = quant_run(1e-7)            # the quantised oracle against itself under summation-order-sized noise: the chaos floor

e32 = max((o - r).abs().max().item() / r.abs().max().item() for o, r in zip(logits, rl))
eq = max((o - r).abs().max().item() / r.abs().max().item() for o, r in zip(logits, ql))
# argmax masks away from near-ties of the fp32 oracle: a pixel counts when its top-2 logit margin exceeds 4x the measured
# worst logit error (a pixel below that margin can legitimately flip under fp16 storage)
pixels = n_clear = mism_clear = mism_all = 0
for o, r in zip(logits, rl):
    top2 = r.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 4.0 * (o - r).abs().max().item()
    am, ar = o.argmax(1), r.argmax(1)
    pixels, n_clear = pixels + int(am.numel()), n_clear + int(clear.sum())
    mism_clear, mism_all = mism_clear + int(((am != ar) & clear).sum()), mism_all + int((am != ar).sum())
names = [k for k, _ in m.named_parameters()]
g_q = {k: rel(p.grad, qp.grad) for (k, p), (_, qp) in zip(m.named_parameters(), q.named_parameters())}
g_cos = {k: cos(p.grad, rp.grad) for (k, p), (_, rp) in zip(m.named_parameters(), ref.named_parameters())}
g_32 = {k: rel(p.grad, rp.grad) for (k, p), (_, rp) in zip(m.named_parameters(), ref.named_parameters())}
floor = {k: rel(p.grad, qp.grad) for (k, p), (_, qp) in zip(qn.named_parameters(), q.named_parameters())}
worst = max(g_q, key=g_q.get)
out = {
    "model": f"{'UNet_multitask' if MT else 'UNet'}({a.cin},{a.ncls},64) fp16 storage, {a.batch}x{a.cin}x{H}x{W}, seed {a.seed}",
    "logits_max_err_over_scale_vs_fp32_oracle": e32, "logits_max_err_over_scale_vs_fp16_oracle": eq,
    "loss": float(loss.detach()), "loss_fp32_oracle": float(rloss.detach()), "loss_fp16_oracle": qloss,
    "pixels": pixels, "pixels_clear_of_near_ties": n_clear, "argmax_mismatch_clear": mism_clear,
    "argmax_mismatch_all": mism_all,
    "grad_rel_l2_vs_fp16_oracle": {"median": float(np.median(list(g_q.values()))), "worst": g_q[worst], "worst_tensor": worst},
    "grad_rel_l2_fp16_oracle_self_noise_floor": {"median": float(np.median(list(floor.values()))), "worst": max(floor.values())},
    "grad_rel_l2_vs_fp32_oracle": {"median": float(np.median(list(g_32.values()))), "worst": max(g_32.values())},
    "grad_cosine_vs_fp32_oracle": {"median": float(np.median(list(g_cos.values()))), "worst": min(g_cos.values()),
                                   "worst_tensor": min(g_cos, key=g_cos.get)},
    "grads_finite": bool(all(torch.isfinite(p.grad).all() for p in m.parameters())),
}
line = json.dumps(out)
print("FP16_FEAT64 " + line, flush=True)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
