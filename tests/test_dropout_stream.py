"""CPU tests of the NumPy statement of the dropout stream (tests/dropout_stream.py), which tests/test_gpu_dropout.py holds the
device kernels to bit for bit.  Every test is a fixed, deterministic computation; the statistical ones assert |z| <= 5 under
the binomial null hypothesis (a two-sided tail of 6e-7 per figure; the worst figures observed on exactly these inputs are
stated next to each bound).

Element counts of 2^32 and more are pinned HERE ONLY (the high word of the index, `test_high_word_of_the_index`): a device
tensor of that size is 8 GB in fp16 and is outside the GPU suite."""
import math

import numpy as np
import pytest

from tests import dropout_stream as D

PS = (0.1, 0.25, 0.5)
Z_MAX = 5.0


def _python_hash(e, seed):
    """The documented rule once more in plain Python integers (no NumPy wrapping involved)."""
    m = 0xFFFFFFFF
    x = (((e & m) * 0x9E3779B1) & m) ^ (((seed ^ (e >> 32)) + 0x7F4A7C15) & m)
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & m
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & m
    x ^= x >> 16
    return x


def test_statement_matches_plain_integer_arithmetic():
    es = [0, 1, 7, 8, 4095, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 1]
    for seed in (0, 1, 0x7FFFFFF5, 0xFFFFFFFF):
        got = D.hash32(es, seed)
        assert got.dtype == np.uint32
        assert got.tolist() == [_python_hash(e, seed) for e in es]
    # one hand-computed element: e = 5, seed 1 -> x = 1292754274, u = (x >> 8) / 2^24
    assert _python_hash(5, 1) == 1292754274
    u = D.uniform_at(5, 1)
    assert u.dtype == np.float32 and float(u[0]) == (1292754274 >> 8) / 2.0 ** 24
    assert D.keep_mask(3, 5, 0.25, 9).shape == (15,) and D.keep_mask(3, 5, 0.25, 9).dtype == np.uint8


def test_keep_rate_of_the_stream_and_of_each_vector_lane():
    """n = 2^22 elements; seed = base + site, counter 0..2, p = 0.1, 0.25, 0.5; the whole stream and each class e mod 8 (the
    eight lanes of the vector kernels).  Worst |z| 3.47 (p = 0.1), 3.30, 3.06."""
    n = 1 << 22
    worst = dict.fromkeys(PS, 0.0)
    for base in (0, 1, 12345 * 7919, 0x7FFFFFF0):
        for site in range(1, 6):
            for counter in range(3):
                u = D.uniform(n, base + site, counter)                 # one hash serves the three p
                for p in PS:
                    q = 1 - p
                    k = D.keep_of(u, p)
                    assert np.array_equal(k[:4096], D.keep_mask(64, 64, p, base + site, counter))
                    z = (int(k.sum(dtype=np.int64)) - n * q) / math.sqrt(n * p * q)
                    lanes = k.reshape(-1, 8).sum(0, dtype=np.int64)
                    zl = (lanes - (n // 8) * q) / math.sqrt((n // 8) * p * q)
                    w = max(abs(z), float(np.abs(zl).max()))
                    worst[p] = max(worst[p], w)
                    assert w <= Z_MAX, (p, base, site, counter, z, zl.tolist())
    print("[stream] keep rate: worst |z|", {p: round(w, 3) for p, w in worst.items()})


@pytest.mark.parametrize("p", PS)
def test_serial_correlation(p):
    """Seed 1, counter 0, n = 2^22: z = sum (k_i - q)(k_{i+l} - q) / (p q sqrt(n - l)) at the lags of the kernels' strides
    (neighbours, vector lanes, rows of 768 / 1024 / 3072 / 4096 channels, 65536).  Worst |z| over the three p: 3.43."""
    n, q = 1 << 22, 1 - p
    d = D.keep_mask(n, 1, p, 1, 0).astype(np.float64) - q
    worst = 0.0
    for lag in list(range(1, 65)) + [128, 768, 1024, 3072, 4096, 65536]:
        z = float(d[:-lag] @ d[lag:]) / (p * q * math.sqrt(n - lag))
        worst = max(worst, abs(z))
        assert abs(z) <= Z_MAX, (lag, z)
    print(f"[stream] serial correlation p={p}: worst |z| {worst:.3g}")


def _site_step_streams():
    out = []
    for base in (0, 1, 12345, 2 ** 31 - 1):
        for site in range(1, 6):
            for counter in range(3):
                out.append(((base * 7919 + site) % 2 ** 32, counter))
    return out


@pytest.mark.parametrize("p", PS)
def test_sites_and_steps_are_independent(p):
    """The streams of the tapes' seeds ((base * 7919 + site) mod 2^32, device counter 0..2): all 1,770 pairs of the 60 streams,
    stream a at element i against stream b at element i + shift for shifts 0, 1 and 8; the number of agreeing elements against
    its expectation m (q^2 + p^2) over the m = n - shift compared elements.  Worst |z| 3.48 (p = 0.1), 4.04, 4.37."""
    n, q = 1 << 20, 1 - p
    streams = _site_step_streams()
    eff = [D.effective_seed(s, c) for s, c in streams]
    assert len(set(eff)) == len(eff) == 60, "premise: no two streams share an effective seed"
    # +-1 coding: agreements = (m + <s_a, s_b>) / 2; the inner products are integers below 2^24, exact in float32
    S = np.stack([D.keep_mask(n, 1, p, s, c) for s, c in streams]).astype(np.float32) * 2 - 1
    a = q * q + p * p
    iu = np.triu_indices(len(streams), 1)
    worst = 0.0
    for shift in (0, 1, 8):
        m = n - shift
        agree = (m + (S[:, :m] @ S[:, shift:].T).astype(np.float64)) / 2
        z = (agree - m * a) / math.sqrt(m * a * (1 - a))
        zp = np.abs(z[iu])
        assert zp.size == 1770
        worst = max(worst, float(zp.max()))
        j = int(zp.argmax())
        assert zp.max() <= Z_MAX, (shift, streams[iu[0][j]], streams[iu[1][j]], float(zp.max()))
    print(f"[stream] independence p={p}: worst |z| {worst:.3g}")


def test_p_zero_keeps_everything_and_p_below_one_keeps_only_u_at_least_p():
    n = 1 << 16
    assert D.keep_mask(n, 1, 0.0, 77, 2).all()
    p = np.nextafter(np.float32(1), np.float32(0))                    # 1 - 2^-24, the largest float32 below 1
    u = D.uniform(1 << 22, 3)
    k = D.keep_of(u, p)
    assert float(u.max()) <= float(p), "u has 24 bits: its largest value is 1 - 2^-24"
    assert not k[u < p].any() and k[u >= p].all()
    assert int(k.sum()) == int((u == p).sum())                        # only an all-ones draw survives
    assert not D.keep_of(u, 1.0).any()                                # p = 1 keeps nothing: u >= 1 never holds


def test_counter_is_a_seed_offset():
    n = 4096
    for seed in (0, 5, 0x7FFFFFF0, 0xFFFFFFFF):
        for counter in (0, 1, 2, 7, -2147483643, 2 ** 31 + 5):
            eff = (seed + (counter % 2 ** 32) * 0x9E3779B9) % 2 ** 32
            assert D.effective_seed(seed, counter) == eff
            for p in PS:
                assert np.array_equal(D.keep_mask(n, 1, p, seed, counter), D.keep_mask(n, 1, p, eff))
    assert D.effective_seed(9, None) == 9
    assert np.array_equal(D.keep_mask(64, 64, 0.5, 9, 0), D.keep_mask(64, 64, 0.5, 9))
    assert not np.array_equal(D.keep_mask(64, 64, 0.5, 9, 1), D.keep_mask(64, 64, 0.5, 9))


def test_mask_is_keyed_by_the_dense_index():
    """e = row * C + col: the mask of [M, C] is the first M * C elements of one stream, whatever the split into rows."""
    full = D.keep_mask(1, 77 * 64, 0.25, 4242, 1)
    assert np.array_equal(D.keep_mask(77, 64, 0.25, 4242, 1), full)
    assert np.array_equal(D.keep_mask(7, 64, 0.25, 4242, 1), full[:7 * 64])


def test_high_word_of_the_index():
    """Indices of 2^32 and more: the high word is xor-ed into the seed word.  Hand-computed: e = 2^32 + 5 under seed 1 is
    e_lo = 5 under seed word 1 ^ 1 = 0, x = 1840164237; e = 3 * 2^32 + (2^32 - 1) under seed 0xFFFFFFF0 gives 2255515891."""
    e1, e2 = (1 << 32) + 5, (3 << 32) + 0xFFFFFFFF
    assert D.hash32(e1, 1).tolist() == [1840164237] == [_python_hash(5, 0)]
    assert D.hash32(e2, 0xFFFFFFF0).tolist() == [2255515891] == [_python_hash(0xFFFFFFFF, 0xFFFFFFF0 ^ 3)]
    assert D.hash32(e1, 1).tolist() != D.hash32(5, 1).tolist()
    for e, seed, x in ((e1, 1, 1840164237), (e2, 0xFFFFFFF0, 2255515891)):
        u = (x >> 8) / 2.0 ** 24
        assert float(D.uniform_at(e, seed)[0]) == u
        for p in PS:
            assert int(D.keep_at(e, p, seed)[0]) == int(u >= float(np.float32(p)))
