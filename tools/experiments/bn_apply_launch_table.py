"""Per-launch table of bn_bwd_apply / pool2 kernels from two step timelines (tools/step_timeline.py --all output)."""
import re, sys

par, new = sys.argv[1:3]
B = 16
# timeline order of the 14 apply launches: (layer, side, C)
APPLY = [("dec3.c1", 512, 64), ("dec2.c2", 256, 128), ("dec2.c1", 256, 128), ("dec1.c2", 128, 256), ("dec1.c1", 128, 256),
         ("dec0.c2", 64, 512), ("dec0.c1", 64, 512), ("enc4.c2", 32, 1024), ("enc4.c1", 32, 1024), ("enc3.c2", 64, 512),
         ("enc3.c1", 64, 512), ("enc2.c2", 128, 256), ("enc2.c1", 128, 256), ("enc1.c2", 256, 128)]
POOLF = [("pool1", 512, 64), ("pool2", 256, 128), ("pool3", 128, 256), ("pool4", 64, 512)]      # input side, C
POOLB = [("pool4", 64, 512), ("pool3", 128, 256), ("pool2", 256, 128), ("pool1", 512, 64)]


def durs(path, key):
    out = []
    for ln in open(path):
        m = re.match(r"\s*[\d.]+ us\s+gap\s+[-\d.]+\s+dur\s+([\d.]+)\s+(\S+)", ln)
        if m and key in m.group(2):
            out.append(float(m.group(1)))
    return out


def floor(path):
    return min(float(m.group(1)) for ln in open(path) for m in [re.match(r"\s*[\d.]+ us\s+gap\s+[-\d.]+\s+dur\s+([\d.]+)", ln)] if m)


def summary(path):
    for ln in open(path):
        if ln.startswith("step:"):
            return ln.strip()


pa, na = durs(par, "bn_bwd_apply"), durs(new, "bn_bwd_apply")
assert len(pa) == len(na) == 14, (len(pa), len(na))
fl = floor(par)
bytes0 = 3 * B * 512 * 512 * 64 * 2
bw_ref = bytes0 / pa[0] / 1e6          # TB/s
print(f"parent: {summary(par)}")
print(f"new:    {summary(new)}")
print(f"BW_ref (parent, 512^2 x 64 launch) = {bw_ref:.2f} TB/s, floor (shortest launch of the parent trace) = {fl:.1f} us\n")
print("| launch | M x C | MB | parent us | parent TB/s | new us | new TB/s | bound 1.10 x (bytes / BW_ref + floor) us | within |")
print("|---|---|---|---|---|---|---|---|---|")
ok = True
for (name, s, c), p, n in zip(APPLY, pa, na):
    by = 3 * B * s * s * c * 2
    bound = 1.10 * (by / bw_ref / 1e6 + fl)
    good = n <= bound
    ok &= good
    print(f"| bn_bwd_apply {name} | {B * s * s} x {c} | {by / 1e6:.0f} | {p:.1f} | {by / p / 1e6:.2f} | {n:.1f} | {by / n / 1e6:.2f} | {bound:.1f} | {'yes' if good else 'NO'} |")
print(f"| bn_bwd_apply, 14 launches | | | {sum(pa):.1f} | | {sum(na):.1f} | | | {'all' if ok else 'NOT all'} |")
for key, tab, fac, label in (("pool2_fwd", POOLF, 1.25, "pool2_fwd"), ("pool2_bwd", POOLB, 3.25, "pool2_bwd+bnred")):
    pp, nn = durs(par, key), durs(new, key)
    assert len(pp) == len(nn) == 4
    for (name, s, c), p, n in zip(tab, pp, nn):
        by = fac * B * s * s * c * 2
        bound = 1.10 * (by / bw_ref / 1e6 + fl)
        print(f"| {label} {name} (unchanged code) | {B * s * s} x {c} in | {by / 1e6:.0f} | {p:.1f} | {by / p / 1e6:.2f} | {n:.1f} | {by / n / 1e6:.2f} | {bound:.1f} | {'yes' if n <= bound else 'NO'} |")
