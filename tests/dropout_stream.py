"""NumPy uint32 statement of the dropout kernels' random stream (csrc/transformer_kernels.hip: dropout_kernel;
csrc/elementwise_tu_f16.hip: dropout8_kernel, dropout8_fused_kernel; csrc/conv1x1_mfma.hip: the epi 1 / epi 2 epilogue), shared
by tests/test_dropout_stream.py (CPU) and tests/test_gpu_dropout.py (GPU).

  e      = row * C + col, the element's index in the dense [M, C] tensor (no leading dimension enters), e_lo / e_hi its low and
           high 32-bit words
  seed'  = seed + counter * 0x9E3779B9 (mod 2^32) where a device step counter is given, else seed
  x      = e_lo * 0x9E3779B1 ^ ((seed' ^ e_hi) + 0x7F4A7C15)                        (uint32, wrapping)
  x     ^= x >> 16;  x *= 0x85EBCA6B;  x ^= x >> 13;  x *= 0xC2B2AE35;  x ^= x >> 16    (the fmix32 finaliser)
  u      = (x >> 8) * 2^-24 as float32 (exact: 24 bits)
  keep   = u >= float32(p); the kept values are scaled by 1 / (1 - p), the others are 0.
Every step is a uint32 array operation; nothing here is derived from the kernels' output."""
import numpy as np

K_INDEX = 0x9E3779B1          # multiplies the low word of the element index
K_OFFSET = 0x7F4A7C15         # added to the seed word
K_COUNTER = 0x9E3779B9        # stride of the device step counter in seed space
_CHUNK = 1 << 20


def effective_seed(seed, counter=None):
    """seed + counter * 0x9E3779B9 (mod 2^32); `counter` is the int32 device scalar read as uint32."""
    seed = int(seed) & 0xFFFFFFFF
    if counter is None:
        return seed
    return (seed + (int(counter) & 0xFFFFFFFF) * K_COUNTER) & 0xFFFFFFFF


def _mix(lo, hi, seed):
    """x of the index words `lo`, `hi` (uint32 arrays; `lo` is overwritten)."""
    lo *= np.uint32(K_INDEX)                                                   # uint32 arrays wrap
    lo ^= (np.uint32(seed) ^ hi) + np.uint32(K_OFFSET)
    lo ^= lo >> np.uint32(16)
    lo *= np.uint32(0x85EBCA6B)
    lo ^= lo >> np.uint32(13)
    lo *= np.uint32(0xC2B2AE35)
    lo ^= lo >> np.uint32(16)
    return lo


def hash32(e, seed):
    """The 32-bit hash of the element indices `e` (any integers < 2^64) under the effective seed `seed`."""
    e = np.atleast_1d(np.asarray(e, dtype=np.uint64))
    return _mix((e & np.uint64(0xFFFFFFFF)).astype(np.uint32), (e >> np.uint64(32)).astype(np.uint32), seed)


def _to_unit(x):
    return (x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def uniform_at(e, seed, counter=None):
    """float32 u in [0, 1) of the element indices `e`."""
    return _to_unit(hash32(e, effective_seed(seed, counter)))


def uniform(n, seed, counter=None):
    """u of the elements 0 .. n - 1 (float32 [n]); one hash serves every p."""
    assert 0 <= n <= 1 << 32, "larger index ranges: uniform_at"
    seed = effective_seed(seed, counter)
    out = np.empty(n, np.float32)
    zero = np.zeros(1, np.uint32)                                               # the high word of every index below 2^32
    for s in range(0, n, _CHUNK):
        t = min(n, s + _CHUNK)
        out[s:t] = _to_unit(_mix(np.arange(s, t, dtype=np.uint32), zero, seed))
    return out


def keep_of(u, p):
    return (u >= np.float32(p)).astype(np.uint8)


def keep_at(e, p, seed, counter=None):
    return keep_of(uniform_at(e, seed, counter), p)


def keep_mask(M, C, p, seed, counter=None):
    """The mask bytes of a dense [M, C] dropout: uint8 [M * C], 1 = kept."""
    return keep_of(uniform(int(M) * int(C), seed, counter), p)
