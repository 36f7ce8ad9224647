"""The poison helper itself (tests/poison.py), on the CPU: byte patterns per dtype, what is left alone, restoration."""
import math

import pytest
import torch

from tests import poison

SHAPES = [(), (0,), (1,), (3, 5), (2, 0, 4)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8, torch.bool])
def test_fill_patterns_per_dtype(dtype):
    """0xFF: NaN in every float format, -1 in signed integers, 255 in uint8, True in bool; 0x00: zero everywhere; any other
    byte: that byte in every position.  0-dim and empty tensors included."""
    for shape in SHAPES:
        with poison.poisoned(0xFF, cpu_too=True):
            ts = [torch.empty(shape, dtype=dtype), torch.empty_like(torch.zeros(shape, dtype=dtype)),
                  torch.empty_strided(shape, torch.zeros(shape).stride(), dtype=dtype)]
        for t in ts:
            assert t.shape == torch.Size(shape) and t.dtype == dtype
            if dtype.is_floating_point:
                assert torch.isnan(t).all()
            elif dtype == torch.bool:
                assert t.all()
            else:
                assert (t == (255 if dtype == torch.uint8 else -1)).all()
        with poison.poisoned(0x00, cpu_too=True):
            assert (torch.empty(shape, dtype=dtype) == 0).all()
        with poison.poisoned(0x5A, cpu_too=True):
            t = torch.empty(shape, dtype=dtype)
        if dtype != torch.bool and t.numel():
            assert (t.contiguous().view(-1).view(torch.uint8) == 0x5A).all()


def test_strided_result_is_filled_gaps_included():
    with poison.poisoned(0xFF, cpu_too=True):
        t = torch.empty_strided((2, 3), (8, 2))
    assert torch.isnan(t).all() and t.stride() == (8, 2)
    assert (poison.fill_bytes(torch.zeros(4, 6)[:, ::2], 0xFF).untyped_storage().tolist() == [255] * (4 * 6 * 4))


def test_cpu_tensors_are_left_alone_when_only_the_device_is_meant(monkeypatch):
    """The default fills CUDA results only: for a CPU result the wrappers never reach the fill."""
    def no_fill(*a, **k):
        raise AssertionError("a CPU tensor was filled")
    monkeypatch.setattr(poison, "fill_bytes", no_fill)
    with poison.poisoned(0xFF):
        assert torch.empty.__wrapped__ is not None
        assert torch.empty(3, 5).shape == (3, 5)
        assert torch.empty_like(torch.zeros(7, dtype=torch.int64)).dtype == torch.int64
        assert torch.empty_strided((2, 3), (3, 1)).stride() == (3, 1)
        assert torch.empty(4, device="meta").device.type == "meta"
    with pytest.raises(AssertionError, match="was filled"):
        with poison.poisoned(0xFF, cpu_too=True):
            torch.empty(3)


def test_everything_is_restored_on_exit_and_on_error():
    from umi import ops, ops_tu
    real = (torch.empty, torch.empty_like, torch.empty_strided, ops.workspace)
    assert ops_tu.workspace is ops.workspace
    with poison.poisoned(0xFF):
        assert torch.empty is not real[0] and torch.empty_like is not real[1] and torch.empty_strided is not real[2]
        assert ops.workspace is not real[3] and ops_tu.workspace is ops.workspace       # the by-name import follows
        with poison.poisoned(0x00, cpu_too=True):                                       # nests: innermost wins, unwinds in order
            assert (torch.empty(4) == 0).all()
    assert (torch.empty, torch.empty_like, torch.empty_strided, ops.workspace) == real and ops_tu.workspace is real[3]
    with pytest.raises(ZeroDivisionError):
        with poison.poisoned(0xFF, cpu_too=True):
            assert math.isnan(torch.empty(()).item())
            1 / 0
    assert (torch.empty, torch.empty_like, torch.empty_strided, ops.workspace) == real and ops_tu.workspace is real[3]


def test_poison_buckets_fills_every_flat_buffer():
    from umi import ddp
    m = torch.nn.Sequential(torch.nn.Linear(40, 40), torch.nn.Linear(40, 3))
    red = ddp.GradReducer(m, world_size=1, bucket_mb=0.005)
    assert len(red.buckets) > 1
    poison.poison_buckets(red, 0xFF)
    for p in m.parameters():
        assert torch.isnan(red.buffer_for(p)).all()
    poison.poison_buckets(red, 0x00)
    assert all((b.flat == 0).all() for b in red.buckets)
