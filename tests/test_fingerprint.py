"""The replica fingerprint (include/unetmi.h, umi_fingerprint_multi) as NumPy states it: the pinned words, the vectorised
statement against a plain loop, and the changes it must see.  No GPU."""
import numpy as np
import pytest

MASK = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
f32 = np.float32


def mix(z):
    z &= MASK
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & MASK
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & MASK
    return z ^ (z >> 31)


def loop_fingerprint(arrays):
    """The definition, word by word on Python integers."""
    F = 0
    for t, a in enumerate(arrays):
        H = 0
        for i, w in enumerate(np.ascontiguousarray(a).reshape(-1).view(np.uint32).tolist()):
            H = (H + mix(w + G * (i + 1))) & MASK
        F = (F + mix(H + G * (t + 1))) & MASK
    return F


PINNED = [
    ([np.array([1.0, -0.0, 0.0], f32), np.array([3.5], f32)], 0x665791ee769a408b),
    ([np.array([1.0, 0.0, -0.0], f32), np.array([3.5], f32)], 0xf16f7461918fc54b),      # the two zeros swapped
    ([np.array([3.5], f32), np.array([1.0, -0.0, 0.0], f32)], 0xb2f97be71456b16d),      # the two tensors swapped
    ([], 0),
    ([np.zeros(0, f32)], 0xe220a8397b1dcdaf),
]


@pytest.mark.parametrize("case", range(len(PINNED)))
def test_pinned_words(case):
    from umi import ddp
    arrays, want = PINNED[case]
    assert ddp.fingerprint_numpy(arrays) == want
    assert loop_fingerprint(arrays) == want


def test_cpu_tensors_go_through_the_numpy_statement():
    import torch
    from umi import ddp
    arrays, want = PINNED[0]
    assert ddp.fingerprint([torch.from_numpy(a) for a in arrays]) == want
    assert ddp.fingerprint([]) == 0


@pytest.mark.parametrize("n", [1, 7, 1000, 4097])
def test_vectorised_statement_is_the_loop(n):
    from umi import ddp
    rng = np.random.default_rng(n)
    arrays = [rng.standard_normal(n).astype(f32), rng.integers(0, 1 << 32, size=3, dtype=np.uint32)]
    want = loop_fingerprint(arrays)
    assert ddp.fingerprint_numpy(arrays) == want
    assert ddp.fingerprint_numpy(arrays, chunk=5) == want              # chunk edges inside a tensor change nothing


def test_sees_a_bit_flip_a_signed_zero_and_a_swap_of_tensors():
    from umi import ddp
    rng = np.random.default_rng(0)
    a, b = rng.standard_normal(1000).astype(f32), rng.standard_normal(7).astype(f32)
    base = ddp.fingerprint_numpy([a, b])
    flipped = a.copy()
    flipped.view(np.uint32)[-1] ^= 1                                   # one bit of the last word
    assert ddp.fingerprint_numpy([flipped, b]) != base
    z = a.copy()
    z[3] = 0.0
    nz = z.copy()
    nz[3] = -0.0
    assert z[3] == nz[3] and ddp.fingerprint_numpy([z, b]) != ddp.fingerprint_numpy([nz, b])
    assert ddp.fingerprint_numpy([b, a]) != base


def test_entry_point_is_declared_exported_and_rejects_bad_arguments():
    """No GPU is touched: every refusal comes before a launch."""
    import ctypes
    from umi import build, lib
    cdll = ctypes.CDLL(build.LIB)
    for n in ("umi_fingerprint_multi", "umi_fingerprint_ws_bytes"):
        assert n in lib.SIGNATURES and hasattr(cdll, n), n
    assert lib.fn("umi_fingerprint_ws_bytes")(0) == 0 and lib.fn("umi_fingerprint_ws_bytes")(3) == 24
    buf = ctypes.create_string_buffer(256)
    p = (ctypes.addressof(buf) + 15) & ~15                             # an aligned address that is never dereferenced
    f = lib.fn("umi_fingerprint_multi")
    assert f(p, 1, 1, p, 8, None, None) == lib.UMI_ERR_BADARG           # no result word
    assert f(p, 1, 1, p, 8, p + 4, None) == lib.UMI_ERR_BADARG          # a misaligned one
    assert f(None, 1, 1, p, 8, p, None) == lib.UMI_ERR_BADARG           # rows but no table
    assert f(p, 1, 1, None, 8, p, None) == lib.UMI_ERR_BADARG           # blocks but no scratch
    assert f(p, -1, 0, p, 8, p, None) == lib.UMI_ERR_BADARG
    assert f(p, 1, 2, p, 8, p, None) == lib.UMI_ERR_WORKSPACE
