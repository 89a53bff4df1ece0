"""-m gpu: the conv epilogues that request their operands (aux / aux2 / aux3) before the K loop instead of at the point of use, and the
parity classes of a 3x3 / stride-2 / pad-1 data gradient.  Every case checks the output against torch-CPU fp32 fed the same rounded
operands (TOL of test_gpu_conv.py), the statistic sums within 5e-3 relative (the bound of the existing epilogue tests), and that a second
identical launch returns a bit-identical y: a request register that is stale, or read for a row it was not requested for, differs there.
Shapes: ragged last tiles in M, a single tile whose rows >= M are clamped, more tiles than statistic rows, class rasters of 1 x 1."""
import pytest
import torch
import torch.nn.functional as F

from gpu_util import err, from_nhwc, q, report, to_nhwc
from test_gpu_conv import TOL

pytestmark = pytest.mark.gpu

DT = torch.bfloat16
STAT_TOL = 5e-3


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _flags(name):
    from tinyfaces import _hip
    return {"mask_stats2": _hip.EPI_MASK | _hip.EPI_STATS2,
            "res_mask2_stats3": _hip.EPI_RES | _hip.EPI_MASK2 | _hip.EPI_STATS3,
            "mask2_stats3": _hip.EPI_MASK2 | _hip.EPI_STATS3}[name]


def _run_and_check(name, base, gy_nchw, wt, Cout, K, s, p, hw, flags, tile, g):
    """base: the plain data gradient (fp32, NCHW, torch-CPU).  Builds the operands of `flags`, the reference, launches twice, asserts."""
    from tinyfaces import ops
    shape = base.shape
    C = shape[1]
    kw = {}
    if flags == "mask_stats2":
        craw = torch.randn(shape, generator=g)
        ms, mh = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5
        ref = base * ((q(craw, DT) * ms.view(1, -1, 1, 1) + mh.view(1, -1, 1, 1)) > 0)
        second = q(craw, DT)
        kw = dict(aux=to_nhwc(craw, DT), mask=(ms.cuda(), mh.cuda()))
    else:
        yprev = torch.randn(shape, generator=g)
        c3 = torch.randn(shape, generator=g) * 1.5 + 0.3
        ref = base
        kw = dict(aux2=to_nhwc(yprev, DT), aux3=to_nhwc(c3, DT))
        if flags == "res_mask2_stats3":
            res = torch.randn(shape, generator=g)
            ref = ref + q(res, DT)
            kw["aux"] = to_nhwc(res, DT)
        ref = ref * (q(yprev, DT) > 0)
        second = q(c3, DT)
    x = to_nhwc(gy_nchw, DT)

    def launch():
        return ops.conv2d_nhwc(x, wt, Cout, K, K, s, p, mode=1, out_hw=hw, epi=_flags(flags), want_stats=True, tile=tile, **kw)

    y, st = launch()
    y_again, _ = launch()
    d = err(from_nhwc(y), ref)
    ssum = st.sum(0).cpu()
    d1 = err(ssum[0], ref.sum(dim=(0, 2, 3)))
    d2 = err(ssum[1], (ref * second).sum(dim=(0, 2, 3)))
    report(name, rel=d[2], s1=d1[2], s2=d2[2])
    print(f"{name}: rel {d[2]:.3e} s1 {d1[2]:.3e} s2 {d2[2]:.3e}")
    assert d[2] < TOL[DT]
    assert d1[2] < STAT_TOL and d2[2] < STAT_TOL
    assert torch.equal(y, y_again), "a second identical launch returned another y"


def _pointwise(nhw, Cin, Cout, flags, tile, seed):
    from tinyfaces import ops
    N, H, W = nhw
    g = _g(seed)
    gy = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cin, Cout, 1, 1, generator=g) / Cin ** 0.5        # the forward conv Cout -> Cin; its data gradient has Cout channels
    base = F.conv_transpose2d(q(gy, DT), q(w, DT))
    wt = ops.pack_weight(w.cuda(), DT, transpose=True)
    _run_and_check(f"epi_req_pw[{nhw},{Cin}->{Cout},{flags},t{tile}]", base, gy, wt, Cout, 1, 1, 0, (H, W), flags, tile, g)


@pytest.mark.parametrize("flags", ["mask_stats2", "res_mask2_stats3", "mask2_stats3"])
@pytest.mark.parametrize("nhw", [(2, 17, 15), (1, 2, 3)])
def test_conv_dma_64x128_pointwise_dgrad(nhw, flags):
    """64 x 128 / 32x32x16 tile, 2-deep ring (tile code 46): M = 510 (eight tiles, the last one ragged) and M = 6 (one tile, rows >= M clamped),
    64 -> 256 channels (two channel tiles, one K stage: the requests travel behind the only stage's DMAs)."""
    _pointwise(nhw, 64, 256, flags, 46, 5)


@pytest.mark.parametrize("flags", ["mask_stats2", "res_mask2_stats3"])
def test_conv_dma_64x64_two_deep_pointwise_dgrad(flags):
    """64 x 64 tile (code 13), 512 -> 128 channels: 8 K stages = the 2-deep ring (5..16 stages), two channel tiles, M = 510."""
    _pointwise((2, 17, 15), 512, 128, flags, 13, 6)


@pytest.mark.parametrize("case", [(2, 5, 33, 128, 128), (3, 30, 45, 128, 256), (1, 4, 32, 128, 128)])
def test_conv3x3h_dgrad_mask_stats2(case):
    """conv3x3h (tile code 50), MASK | STATS2 data gradient: one row and one column past a tile; 48 tiles (more than the statistic rows);
    exactly one tile."""
    from tinyfaces import ops
    N, H, W, Cin, Cout = case
    g = _g(7)
    gy = torch.randn(N, Cout, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    base = F.conv_transpose2d(q(gy, DT), q(w, DT), padding=1)
    wt = ops.pack_weight(w.cuda(), DT, transpose=True)
    _run_and_check(f"epi_req_c3h[{case}]", base, gy, wt, Cin, 3, 1, 1, (H, W), "mask_stats2", 50, g)


@pytest.mark.parametrize("tile", [46, 13])
@pytest.mark.parametrize("hw", [(14, 17), (15, 18), (2, 2)])
def test_stride2_3x3_dgrad_parity_classes(hw, tile):
    """3x3 / stride 2 / pad 1 data gradient with MASK | STATS2, N = 2, 64 -> 128 channels: even and odd rasters, 1 x 1 class rasters, class row
    counts that are no multiple of the tile (class boundaries inside the tile sequence)."""
    from tinyfaces import ops
    N, Cin, Cout = 2, 64, 128
    H, W = hw
    oh, ow = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = _g(9)
    gy = torch.randn(N, Cin, oh, ow, generator=g)
    w = torch.randn(Cin, Cout, 3, 3, generator=g) / (Cin * 9) ** 0.5    # the forward conv Cout -> Cin
    base = F.conv_transpose2d(q(gy, DT), q(w, DT), stride=2, padding=1, output_padding=(H - (2 * oh - 1), W - (2 * ow - 1)))
    assert base.shape[2:] == (H, W)
    wt = ops.pack_weight(w.cuda(), DT, transpose=True)
    _run_and_check(f"epi_req_parity[{hw},t{tile}]", base, gy, wt, Cout, 3, 2, 1, (H, W), "mask_stats2", tile, g)
