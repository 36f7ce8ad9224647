"""CPU: the two helpers the evaluation path shares -- umi.ops.read_back (several tensors to the host through one copy, shapes,
dtypes and bits kept) and umi.infer._eval_mode (modules in eval mode for a block, every training flag restored)."""
import numpy as np
import pytest
import torch


def test_read_back_round_trips_mixed_tensors_bit_for_bit():
    from umi import ops
    f64 = np.array([0x7FF8000000000ABC, 0xFFF0000000000123, 0x8000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF,
                    0x3FF0000000000000], dtype=np.uint64).view(np.float64)        # NaNs with payloads, -0.0, subnormals, 1.0
    assert np.isnan(f64[:2]).all() and np.signbit(f64[2]) and f64[2] == 0 and 0 < f64[3] < np.finfo(np.float64).tiny
    want = [np.array([[-1, 2 ** 31 - 1, -2 ** 31], [0, 7, -123456789]], dtype=np.int32),
            np.array([-2 ** 63, 2 ** 63 - 1, -1, 5], dtype=np.int64),
            np.array([0, 1, 128, 255, 77], dtype=np.uint8),                       # an odd byte count ahead of wider elements
            f64.reshape(3, 2),
            np.zeros((0, 3), dtype=np.int64),
            np.array(-0.0, dtype=np.float64),
            np.array(-9, dtype=np.int32)]
    got = ops.read_back(*(torch.from_numpy(a) for a in want))
    assert isinstance(got, list) and len(got) == len(want)
    for g, w in zip(got, want):
        assert isinstance(g, np.ndarray) and g.dtype == w.dtype and g.shape == w.shape
        assert g.tobytes() == w.tobytes()
    assert ops.read_back(torch.from_numpy(want[0]).t())[0].tolist() == want[0].T.tolist()      # a strided view


def test_read_back_does_one_copy_and_rejects_other_dtypes(monkeypatch):
    from umi import ops
    calls = []
    orig = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (calls.append(tuple(self.shape)), orig(self, *a, **k))[1])
    ops.read_back(torch.zeros(3, dtype=torch.int32), torch.zeros((2, 2), dtype=torch.float64), torch.zeros(5, dtype=torch.uint8))
    monkeypatch.undo()
    assert calls == [(3 * 4 + 4 * 8 + 5,)]
    for dtype in (torch.float32, torch.float16, torch.int16, torch.bool):
        with pytest.raises(TypeError):
            ops.read_back(torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=dtype))


def _modules():
    a, b, c = torch.nn.Linear(2, 2), torch.nn.Sequential(torch.nn.Linear(2, 2), torch.nn.Dropout()), torch.nn.BatchNorm1d(2)
    a.train()
    b.eval()
    c.train()
    return a, b, c


def test_eval_mode_restores_every_flag():
    from umi.infer import _eval_mode
    a, b, c = _modules()
    with _eval_mode([a, b, c]):
        assert not a.training and not b.training and not c.training
    assert a.training and not b.training and c.training
    with _eval_mode(a):                               # a single module
        assert not a.training
    assert a.training
    with _eval_mode((c, b)):                          # a tuple
        assert not c.training
    assert c.training and not b.training


def test_eval_mode_restores_the_flags_when_the_body_raises():
    from umi.infer import _eval_mode
    a, b, c = _modules()
    with pytest.raises(KeyError):
        with _eval_mode([a, b, c]):
            assert not a.training
            raise KeyError("body")
    assert a.training and not b.training and c.training


def test_eval_mode_leaves_callables_alone():
    from umi.infer import _eval_mode
    seen = []

    def fn(v):
        seen.append(v)
        return v

    a = torch.nn.Linear(2, 2).train()
    with _eval_mode(fn):
        assert fn(1) == 1
    with _eval_mode([fn, a, len]):
        assert not a.training and fn(2) == 2
    assert a.training and seen == [1, 2] and not hasattr(fn, "training")
