"""umi_dice_ce_fwd_items: every stats row is bit-identical to umi_dice_ce_fwd on that item's slice.

The per-item kernel runs the whole-batch kernel's block decomposition once per item (grid = items x that call's grid) and one
finalize block per item, so the comparison is `==` on the bit patterns, for all four target dtypes.  The workspace and the
memory behind `stats` are preset to NaN bytes and must come back untouched outside what the call owns."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
TARGET_DTYPES = {0: torch.int64, 1: torch.float32, 2: torch.uint8, 3: torch.int32}
GUARD = 4096            # bytes behind the workspace and behind stats

GRID = [(items, n, C, HW) for items in (1, 3, 5) for n in (1, 2) for C in (2, 4, 8) for HW in (1, 63, 64 * 64 + 1)]
GRID.append((2, 1, 2, 512 * 512))            # the benchmark's image: 256 blocks per item


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X: torch.cuda.is_available() is False")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _nan_bytes(nbytes):
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("items,n,C,HW", GRID)
def test_rows_are_the_bits_of_the_whole_batch_call_on_the_slice(items, n, C, HW):
    _need_gpu()
    from umi import lib as L, ops
    g = torch.Generator().manual_seed(items * 1000 + n * 100 + C * 10 + HW % 7)
    logits = (3.0 * torch.randn(items * n, C, HW, generator=g)).to(DEV)
    classes = torch.randint(0, C, (items * n, HW), generator=g)
    K = 3 * C + 2
    need = L.fn("umi_dice_ce_items_ws_bytes")(items, n, C, HW)
    one = L.fn("umi_dice_ce_ws_bytes")(n, C, HW)
    assert need == items * one and one > 0
    for code, dt in TARGET_DTYPES.items():
        target = classes.to(dt).to(DEV)
        ws = _nan_bytes(need + GUARD)
        stats = _nan_bytes(items * K * 4 + GUARD)
        L.call("umi_dice_ce_fwd_items", logits.data_ptr(), target.data_ptr(), code, items, n, C, HW, stats.data_ptr(),
               ws.data_ptr(), need, ops._stream())
        rows = stats[:items * K * 4].view(torch.float32).view(items, K)
        ref_ws = torch.empty(one, dtype=torch.uint8, device=DEV)
        for i in range(items):
            ref = torch.empty(K, dtype=torch.float32, device=DEV)
            L.call("umi_dice_ce_fwd", logits[i * n:(i + 1) * n].data_ptr(), target[i * n:(i + 1) * n].data_ptr(), code, n, C, HW,
                   ref.data_ptr(), ref_ws.data_ptr(), one, ops._stream())
            assert torch.equal(_bits(rows[i]), _bits(ref)), (code, i, rows[i].tolist(), ref.tolist())
        assert torch.isfinite(rows).all()
        assert bool((ws[need:] == 0xFF).all()) and bool((stats[items * K * 4:] == 0xFF).all()), code
        # every workspace byte the call owns was written: items x rows x (3C + 1) floats, nothing left as preset
        assert not bool(torch.isnan(ws[:need].view(torch.float32)).any())


def test_calc_loss_items_takes_the_kernel_and_equals_the_loop():
    """loss.calc_loss_items on fused-kernel inputs: one umi_dice_ce_fwd_items call, the values of the calc_loss loop."""
    _need_gpu()
    import loss as Lm
    from umi import lib as L
    Lm.CLASS_NUMBER = 2
    g = torch.Generator().manual_seed(5)
    pred = torch.randn(6, 2, 33, 47, generator=g).to(DEV)
    target = torch.randint(0, 2, (6, 33, 47), generator=g).float().to(DEV)
    calls, real = [], L.call

    def spy(name, *a):
        calls.append(name)
        return real(name, *a)
    L.call = spy
    try:
        got = Lm.calc_loss_items(pred, target, 3, loss_type="dice_bce_mc")
        assert calls == ["umi_dice_ce_fwd_items"]
        del calls[:]
        want = torch.stack([Lm.calc_loss(pred[2 * i:2 * i + 2], target[2 * i:2 * i + 2], loss_type="dice_bce_mc") for i in range(3)])
        assert calls == ["umi_dice_ce_fwd"] * 3
        Lm.ITEMS_KERNEL = False
        loop = Lm.calc_loss_items(pred, target, 3, loss_type="dice_bce_mc")
    finally:
        L.call = real
        Lm.ITEMS_KERNEL = True
    assert got.shape == (3,) and torch.equal(_bits(got), _bits(want)) and torch.equal(_bits(loop), _bits(want))
    # a loss without an items kernel runs the loop on the device, value for value
    ce = Lm.calc_loss_items(pred, target, 3, loss_type="CE")
    assert torch.equal(ce, torch.stack([Lm.calc_loss(pred[2 * i:2 * i + 2], target[2 * i:2 * i + 2], loss_type="CE")
                                        for i in range(3)]))


def test_bad_arguments_return_status_before_any_launch():
    _need_gpu()
    from umi import lib as L
    f = L.fn("umi_dice_ce_fwd_items")
    items, n, C, HW = 3, 2, 2, 63
    logits = torch.zeros(items * n, C, HW, device=DEV)
    target = torch.zeros(items * n, HW, device=DEV)
    need = L.fn("umi_dice_ce_items_ws_bytes")(items, n, C, HW)
    ws, stats = _nan_bytes(need), _nan_bytes(items * (3 * C + 2) * 4)
    lp, tp, sp, wp = logits.data_ptr(), target.data_ptr(), stats.data_ptr(), ws.data_ptr()
    ok = (lp, tp, 1, items, n, C, HW, sp, wp, need, None)

    def with_(i, v):
        return ok[:i] + (v,) + ok[i + 1:]
    for bad in (with_(0, None), with_(1, None), with_(7, None), with_(8, None), with_(2, -1), with_(2, 4), with_(3, 0),
                with_(3, -3), with_(3, 65536), with_(4, 0), with_(6, 0), with_(6, -5)):
        assert f(*bad) == L.UMI_ERR_BADARG, bad
    assert f(*with_(5, 0)) == L.UMI_ERR_UNSUPPORTED and f(*with_(5, 9)) == L.UMI_ERR_UNSUPPORTED
    assert f(*with_(9, need - 1)) == L.UMI_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((ws == 0xFF).all()) and bool((stats == 0xFF).all())          # nothing ran
    assert f(*ok) == L.UMI_OK
    torch.cuda.synchronize()
    assert torch.isfinite(stats.view(torch.float32)).all()
