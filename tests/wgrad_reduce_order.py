"""NumPy float32 statement of the fixed split-K reduction order of the weight gradients (csrc/generic_kernels.hip:
wgrad_reduce_kernel, wgrad_reduce_v4_kernel, wgrad_reduce_group_kernel, wg_reduce_tiles), shared by
tests/test_wgrad_reduce_order.py (CPU) and tests/test_gpu_wgrad_reduce.py (GPU).

  part[z] = split z's slab, z = 0 .. splits - 1; every output element is reduced on its own.
  * 8 lanes; lane l owns the splits l, l + 8, l + 16, ...
  * scalar form: one chain per lane, s = 0; s += part[l]; s += part[l + 8]; ...
  * float4 and tile forms: two chains per lane.  a = b = 0; while z + 8 < splits: a += part[z]; b += part[z + 8]; z += 16.
    A trailing odd term goes to a.  The lane's sum is a + b.
  * the 8 lane sums are added in lane order (scalar form: onto 0; the other two: onto lane 0's sum)
  * the result is multiplied by `scale` (fp32).
Every operation is an fp32 add or multiply of arrays: NumPy rounds each one to nearest-even like the device does."""
import numpy as np

LANES = 8
F32 = np.float32


def _slabs(part):
    part = np.asarray(part)
    assert part.dtype == np.float32 and part.ndim >= 1
    return part, part.shape[0], np.zeros(part.shape[1:], F32)


def reduce_one_chain(part, scale):
    """The scalar form (wgrad_reduce_kernel; the grouped kernel where Co % 4 != 0 or the slabs are not 16-byte aligned)."""
    part, splits, zero = _slabs(part)
    total = zero.copy()
    for lane in range(LANES):
        s = zero.copy()
        for z in range(lane, splits, LANES):
            s = s + part[z]
        total = total + s
    return total * F32(scale)


def reduce_two_chains(part, scale):
    """The float4 and the tile forms (wgrad_reduce_v4_kernel, the grouped kernel's vector branch, wg_reduce_tiles)."""
    part, splits, zero = _slabs(part)
    total = None
    for lane in range(LANES):
        a, b = zero.copy(), zero.copy()
        z = lane
        while z + LANES < splits:
            a = a + part[z]
            b = b + part[z + LANES]
            z += 2 * LANES
        if z < splits:
            a = a + part[z]
        s = a + b
        total = s if total is None else total + s
    return total * F32(scale)


def reference_f64(part, scale):
    """scale (the fp32 value the kernel multiplies by) times the sum over splits, in float64."""
    return np.asarray(part, np.float64).sum(0) * np.float64(F32(scale))


def error_bound(part, scale):
    """A-priori bound of recursive fp32 summation of `splits` terms plus one multiply, per element:
    (splits + 1) * u * scale * sum_z |part_z| with u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4:
    any order of n - 1 adds is within (n - 1) u + O(u^2); the multiply adds one u; one more u covers the O(u^2) terms and the
    zero-initialised accumulators, which add exactly)."""
    part = np.asarray(part, np.float64)
    return (part.shape[0] + 1) * 2.0 ** -24 * np.float64(F32(scale)) * np.abs(part).sum(0)
