"""umi_fingerprint_multi on the MI355X against umi.ddp.fingerprint_numpy, bit for bit: block edges, a long table, a pointer
that is 4- but not 16-byte aligned, tensors cut out of one random buffer (a read past an end would change the word)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool():
    """One random device buffer and its host copy; every tensor of the tests is a slice of it."""
    from umi import lib
    E = lib.fn("umi_optim_block_elems")()
    g = torch.Generator().manual_seed(11)
    host = torch.randint(-2 ** 31, 2 ** 31 - 1, (8 * E + 64,), generator=g, dtype=torch.int64).to(torch.int32)
    return E, host.cuda().view(torch.float32), host.numpy().view(np.float32)


def _both(pool, cuts):
    from umi import ddp
    _, dev, host = pool
    got = ddp.fingerprint([dev[a:b] for a, b in cuts])
    assert got == ddp.fingerprint_numpy([host[a:b] for a, b in cuts]), cuts
    return got


def test_block_edges(pool):
    E = pool[0]
    words = {_both(pool, [(0, n)]) for n in (1, E - 1, E, E + 1, 2 * E + 3)}
    assert len(words) == 5
    _both(pool, [(4, 4 + n) for n in (1, E - 1, E, E + 1, 2 * E + 3)])           # overlapping slices, as one table


def test_table_of_118_small_tensors(pool):
    rng = np.random.default_rng(5)
    cuts, at = [], 0
    for n in rng.integers(0, 67, size=118):                                       # some empty, none a multiple of the tile
        cuts.append((at, at + int(n)))
        at += int(n) + int(rng.integers(0, 3)) * 4
    _both(pool, cuts)


def test_pointer_that_is_four_but_not_sixteen_byte_aligned(pool):
    E, dev, _ = pool
    for off in (1, 2, 3):
        assert dev[off:].data_ptr() % 16 == 4 * off
        _both(pool, [(off, off + E + 5), (off + E + 5, off + 3 * E)])


def test_neighbours_do_not_leak_in(pool):
    """Adjacent slices of the random buffer: the word of a slice depends on that slice alone."""
    from umi import ddp
    E, dev, _ = pool
    a = _both(pool, [(E + 1, 2 * E + 4)])
    moved = dev.clone()
    assert ddp.fingerprint([moved[E + 1:2 * E + 4]]) == a
    moved[E] += 1.0
    moved[2 * E + 4] += 1.0                                                       # the words just outside either end
    assert ddp.fingerprint([moved[E + 1:2 * E + 4]]) == a
    moved.view(torch.int32)[2 * E + 3] ^= 1                                      # the last word inside
    assert ddp.fingerprint([moved[E + 1:2 * E + 4]]) != a


def test_empty_table_writes_zero():
    from umi import lib as L, ops
    out = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    L.call("umi_fingerprint_multi", None, 0, 0, None, 0, out.data_ptr(), ops._stream())
    assert int(out.item()) == 0


def test_pinned_words_and_repeatability():
    from umi import ddp
    f = lambda *v: torch.tensor(v, dtype=torch.float32, device="cuda")            # noqa: E731
    assert ddp.fingerprint([f(1.0, -0.0, 0.0), f(3.5)]) == 0x665791ee769a408b
    assert ddp.fingerprint([f(1.0, 0.0, -0.0), f(3.5)]) == 0xf16f7461918fc54b
    assert ddp.fingerprint([f(3.5), f(1.0, -0.0, 0.0)]) == 0xb2f97be71456b16d
    assert ddp.fingerprint([torch.empty(0, device="cuda")]) == 0xe220a8397b1dcdaf
    ts = [torch.randn(5000, device="cuda"), torch.arange(7, device="cuda")]     # int64: two words per element
    assert ddp.fingerprint(ts) == ddp.fingerprint(ts) == ddp.fingerprint_numpy([t.cpu().numpy() for t in ts])
