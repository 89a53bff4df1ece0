"""-m gpu: did the kernel write ONLY what its contract says?  Every tensor of a launch sits between 0xFF guard bands (tests/redzone.py): outputs start
as NaN / -1 and must be written exactly over the region include/tinyfaces_hip.h names, their guards must be untouched afterwards, and the
inputs' guards are NaN, so an operand read out of range shows in the parity check beside the guard check.  Parity is against a float64 CPU
reference of the same op fed the same rounded operands (q() of tests/gpu_util.py), held to the bars of tests/test_gpu_conv.py -- the reference
here is only more precise than the fp32 one those bars were set against.  Shapes are the edges, not the workload: M below any tile, M = 1
modulo 64 and 128, Cout below the channel tile, pad columns, both modes, strides 1 and 2."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from gpu_util import err, q, report
from redzone import assert_guards, assert_written, guarded, guarded_like, guarded_workspace, unwritten
from test_gpu_conv import MMA32_TILES, PWG_CASES, TOL, TOL_H

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DEV = "cuda"
DMA_TILES = [0, 11, 12, 13, 22, 23, 32]                    # the tile codes tests/test_gpu_conv.py names for the 16x16x32-fragment kernel


def _tol(dtype):
    return TOL_H[dtype] if dtype in TOL_H else TOL[dtype]


def _g(seed):
    return torch.Generator().manual_seed(seed)


def qd(t, dtype):
    """The operand value the kernel sees, in float64."""
    return q(t, dtype).double()


def gin(t, dtype=None):
    """An input on the device between NaN guards."""
    return guarded_like((t if dtype is None else t.to(dtype)).contiguous(), DEV)


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _sync_ok():
    torch.cuda.synchronize()


# =============================================================================================== a. the conv engine
# (K, stride, OH, OW, Cout, ldy): the OUTPUT raster (mode 0: of the conv; mode 1: of the data gradient) and its channels
CONV_SHAPES = [
    (1, 1, 3, 3, 64, 64),          # M = 9: smaller than any tile; Cout = 64 = ldy on the 128-wide channel tiles
    (3, 1, 5, 13, 125, 128),       # M = 65 = 1 mod 64; three pad columns
    (1, 1, 3, 43, 64, 64),         # M = 129 = 1 mod 128
    (3, 2, 5, 13, 64, 64),         # 3x3 / stride 2 (mode 1: the four parity-class launches)
    (1, 2, 3, 43, 125, 128),       # 1x1 / stride 2 (mode 1: the generic transposed gather, ldy != Cout)
    (1, 2, 5, 13, 64, 64),         # 1x1 / stride 2 with ldy == Cout (mode 1 with RES alone: raster initialised from aux, rows scattered over it)
]
EPI_SETS = ["stats", "mask_stats2", "handover", "eval"]    # STATS | MASK+STATS2 | RES+MASK2+STATS3 (a training step) | AFFINE+RES+RELU (evaluation)


def _conv_args(hip, dtype, mode, N, H, W, Cin, OH, OW, Cout, K, stride, pad, ldy, epi, tile):
    a = hip.ConvArgs()
    a.dtype, a.mode = hip.tf_dtype(dtype), mode
    a.N, a.H, a.W, a.Cin, a.OH, a.OW, a.Cout, a.KH, a.KW, a.stride, a.pad = N, H, W, Cin, OH, OW, Cout, K, K, stride, pad
    a.ldy, a.epi, a.tile = ldy, epi, tile
    return a


def _conv_problem(dtype, mode, K, stride, OH, OW, Cin, Cout, ldy, seed, N=1):
    """Operands of one launch and the float64 accumulator (N, OH, OW, ldy), pad columns zero, from the rounded operands."""
    from tinyfaces import ops
    g = _g(seed)
    pad = K // 2
    if mode == 0:
        H, W = (OH, OW) if stride == 1 else (2 * OH - 1, 2 * OW - 1)
        x = torch.randn(N, Cin, H, W, generator=g)
        w = torch.randn(Cout, Cin, K, K, generator=g) / (Cin * K * K) ** 0.5
        base = F.conv2d(qd(x, dtype), qd(w, dtype), stride=stride, padding=pad)
        wp = ops.pack_weight(w.cuda(), dtype)
    else:                                                   # x = the gradient of a conv Cout -> Cin with (stride, pad); y = its input gradient
        H, W = (OH, OW) if stride == 1 else ((OH + 1) // 2, (OW + 1) // 2)
        x = torch.randn(N, Cin, H, W, generator=g)
        w = torch.randn(Cin, Cout, K, K, generator=g) / (Cin * K * K) ** 0.5
        base = F.conv_transpose2d(qd(x, dtype), qd(w, dtype), stride=stride, padding=pad)
        wp = ops.pack_weight(w.cuda(), dtype, transpose=True)
    assert base.shape == (N, Cout, OH, OW), base.shape
    acc = torch.zeros(N, OH, OW, ldy, dtype=torch.float64)
    acc[..., :Cout] = nhwc(base)
    return g, gin(nhwc(x), dtype), guarded_like(wp, DEV), acc, (H, W, pad)


def _epilogue(name, hip, dtype, acc, g):
    """(flags, keyword operands of ops.conv2d_nhwc, float64 result over all ldy columns, float64 statistic sums (2, ldy) or None, the two
    bounds of tests/test_gpu_conv.py for the sums)."""
    shp, ldy = acc.shape, acc.shape[-1]
    rnd = lambda scale=1.0: torch.randn(shp, generator=g) * scale
    if name == "stats":
        return hip.EPI_STATS, {}, acc, torch.stack([acc.sum(dim=(0, 1, 2)), (acc ** 2).sum(dim=(0, 1, 2))]), "mean"
    if name == "mask_stats2":
        aux = rnd()
        ms, mh = torch.rand(ldy, generator=g) + 0.5, torch.randn(ldy, generator=g) * 0.5
        mask = (q(aux, dtype) * ms + mh) > 0               # the decision itself in fp32, as the kernel and the existing tests take it
        ref = acc * mask
        return (hip.EPI_MASK | hip.EPI_STATS2, dict(aux=gin(aux, dtype), mask=(gin(ms), gin(mh))), ref,
                torch.stack([ref.sum(dim=(0, 1, 2)), (ref * qd(aux, dtype)).sum(dim=(0, 1, 2))]), "rel")
    if name == "handover":
        res, yprev, c3 = rnd(), rnd(), rnd(1.5) + 0.3
        ref = (acc + qd(res, dtype)) * (q(yprev, dtype) > 0)
        return (hip.EPI_RES | hip.EPI_MASK2 | hip.EPI_STATS3, dict(aux=gin(res, dtype), aux2=gin(yprev, dtype), aux3=gin(c3, dtype)), ref,
                torch.stack([ref.sum(dim=(0, 1, 2)), (ref * qd(c3, dtype)).sum(dim=(0, 1, 2))]), "rel")
    if name == "res":                                       # (beside the issue's four: the only set the NOT-in-place scattered stride-2 form takes)
        res = rnd()
        return hip.EPI_RES, dict(aux=gin(res, dtype)), acc + qd(res, dtype), None, None
    assert name == "eval"
    sc, sh, res = torch.rand(ldy, generator=g) + 0.5, torch.randn(ldy, generator=g), rnd()
    ref = torch.relu(acc * sc.double() + sh.double() + qd(res, dtype))
    return hip.EPI_AFFINE | hip.EPI_RES | hip.EPI_RELU, dict(epi_scale=gin(sc), epi_shift=gin(sh), aux=gin(res, dtype)), ref, None, None


def _run_conv(hip, tag, dtype, tile, mode, K, stride, OH, OW, Cin, Cout, ldy, epi_name, seed, N=1):
    from tinyfaces import ops
    g, x, wp, acc, (H, W, pad) = _conv_problem(dtype, mode, K, stride, OH, OW, Cin, Cout, ldy, seed, N)
    epi, kw, ref, sums, bar = _epilogue(epi_name, hip, dtype, acc, g)
    y = guarded((N, OH, OW, ldy), dtype, DEV)
    stats = None
    if sums is not None:
        a = _conv_args(hip, dtype, mode, N, H, W, Cin, OH, OW, Cout, K, stride, pad, ldy, epi, tile)
        mt = hip.lib().tf_conv_mtiles(C.byref(a))
        assert mt >= 1, (tag, mt)
        stats = guarded((mt, 2, ldy), F32, DEV, body="keep").zero_()        # exactly tf_conv_mtiles() rows; the sums are accumulated into zeros
    ops.conv2d_nhwc(x, wp, Cout, K, K, stride, pad, mode=mode, out_hw=(OH, OW), ldy=ldy, epi=epi, want_stats=sums is not None, tile=tile, out=y,
                    stats_into=stats, **kw)
    _sync_ok()
    assert_guards(y, f"{tag}: y")
    assert_written(y, what=f"{tag}: y (rows [0, M), all ldy columns)")
    d = err(y.double().cpu(), ref)
    res = dict(rel=d[2])
    ok = d[2] < _tol(dtype)
    if stats is not None:
        assert_guards(stats, f"{tag}: stat_out")
        s = stats.sum(0).double().cpu()
        n = float(N * OH * OW)
        if bar == "mean":                                   # the bars of test_conv_forward_stats_no_prologue
            d1, d2 = err(s[0] / n, sums[0] / n), err(s[1] / n, sums[1] / n)
            res.update(mean_abs=d1[0], sq_rel=d2[2])
            ok = ok and d1[0] < 2e-3 and d2[2] < 2e-3
        else:                                               # ... of test_conv_dgrad_mask_stats2_and_join / test_conv_dgrad_res_mask2_stats3
            d1, d2 = err(s[0], sums[0]), err(s[1], sums[1])
            res.update(s1=d1[2], s2=d2[2])
            ok = ok and d1[2] < 5e-3 and d2[2] < 5e-3
    report(f"bounds_conv[{tag}]", **res)
    assert ok, (tag, res)


def _conv_cases(shapes):
    """(shape, mode, epilogue set) of every launch: both modes times the four sets; the NOT-in-place scattered stride-2 gradient takes RES alone too."""
    return [(shape, mode, epi_name) for shape in shapes for mode in (0, 1)
            for epi_name in EPI_SETS + (["res"] if (mode, shape[0], shape[1]) == (1, 1, 2) else [])]


def _conv_id(case):
    (K, stride, OH, OW, Cout, ldy), mode, epi_name = case
    return f"k{K}s{stride}-{OH}x{OW}-c{Cout}of{ldy}-m{mode}-{epi_name}"


def _conv_case(hip, dtype, tile, case, Cin=64):
    (K, stride, OH, OW, Cout, ldy), mode, epi_name = case
    tag = f"{dtype},t{tile},k{K}s{stride},{OH}x{OW},c{Cout}/{ldy},m{mode},{epi_name}"
    _run_conv(hip, tag, dtype, tile, mode, K, stride, OH, OW, Cin, Cout, ldy, epi_name, seed=100 * mode + (EPI_SETS + ["res"]).index(epi_name) + OH * OW)


@pytest.mark.parametrize("case", _conv_cases(CONV_SHAPES), ids=_conv_id)
@pytest.mark.parametrize("tile", DMA_TILES)
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_conv_dma_tiles_write_their_rows_and_nothing_else(hip, dtype, tile, case):
    _conv_case(hip, dtype, tile, case)


@pytest.mark.parametrize("case", _conv_cases(CONV_SHAPES), ids=_conv_id)
@pytest.mark.parametrize("tile", MMA32_TILES)
@pytest.mark.parametrize("dtype", [BF16, F16])
def test_conv_mma32_tiles_write_their_rows_and_nothing_else(hip, dtype, tile, case):
    _conv_case(hip, dtype, tile, case)


@pytest.mark.parametrize("case", _conv_cases([(3, 1, 3, 3, 128, 128), (3, 1, 5, 13, 128, 128), (3, 1, 3, 43, 128, 128)]), ids=_conv_id)
@pytest.mark.parametrize("dtype", [BF16, F16])
def test_conv3x3h_writes_its_rows_and_nothing_else(hip, dtype, case):
    """Tile code 50 (4 x 32 pixel tiles, 128 channels): rasters smaller than a tile, one column / one row past one."""
    _conv_case(hip, dtype, 50, case, Cin=128)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("hw", [(128, 128), (5, 3277)])
@pytest.mark.parametrize("dtype,epi_name", [(BF16, e) for e in EPI_SETS] + [(F16, "eval")])
def test_conv_pws_writes_its_rows_and_nothing_else(hip, dtype, hw, mode, epi_name):
    """Tile code 70 at the smallest M it takes (16 384) and one pixel more: 64 -> 64, ldy == Cout, the statistic buffer at exactly
    tf_conv_mtiles() = tf_get_stat_rows() rows.  fp16 is inference only: the evaluation set."""
    OH, OW = hw
    _run_conv(hip, f"{dtype},t70,{OH}x{OW},m{mode},{epi_name}", dtype, 70, mode, 1, 1, OH, OW, 64, 64, 64, epi_name, seed=7 + EPI_SETS.index(epi_name) + mode)


@pytest.mark.parametrize("dtype,tile,K,Cin,Cout,ldy", [(F32, 11, 1, 64, 125, 128), (F32, 13, 3, 64, 68, 68), (BF16, 12, 1, 64, 125, 128),
                                                       (BF16, 13, 3, 64, 100, 104), (BF16, 14, 1, 64, 125, 128), (F16, 46, 3, 64, 64, 64),
                                                       (BF16, 50, 3, 128, 128, 128)])
def test_shifted_statistics_read_and_publish_exactly_ldy_floats(hip, dtype, tile, K, Cin, Cout, ldy):
    """TF_EPI_STATS with tf_conv_args.stat_shift / stat_shift_out (what a training step launches; ops.conv2d_nhwc does not expose them, so
    through tf_conv_args): both vectors hold exactly ldy floats between guards.  stat_shift is read over [0, ldy) and no further (a read from
    its guard would put NaN into the sums), stat_shift_out[0, ldy) receives its bits and nothing beside it is written; the sums are those of
    (y - s) and (y - s)^2, held to the bars of test_conv_forward_stats_no_prologue."""
    OH, OW = 5, 13                                           # M = 65 = 1 mod 64
    g, x, wp, acc, (H, W, pad) = _conv_problem(dtype, 0, K, 1, OH, OW, Cin, Cout, ldy, seed=tile + ldy)
    shift = torch.randn(ldy, generator=g) * 0.3
    sh_d, sh_out = gin(shift), guarded((ldy,), F32, DEV)
    y = guarded((1, OH, OW, ldy), dtype, DEV)
    a = _conv_args(hip, dtype, 0, 1, H, W, Cin, OH, OW, Cout, K, 1, pad, ldy, hip.EPI_STATS, tile)
    mt = hip.lib().tf_conv_mtiles(C.byref(a))
    assert mt >= 1
    stats = guarded((mt, 2, ldy), F32, DEV, body="keep").zero_()
    a.x, a.w, a.y, a.stat_out, a.stat_shift, a.stat_shift_out = x.data_ptr(), wp.data_ptr(), y.data_ptr(), stats.data_ptr(), sh_d.data_ptr(), sh_out.data_ptr()
    assert hip.lib().tf_conv2d(C.byref(a), hip.stream()) == 0
    _sync_ok()
    for t, what in ((y, "y"), (stats, "stat_out"), (sh_out, "stat_shift_out"), (sh_d, "stat_shift")):
        assert_guards(t, what)
    assert_written(y, what="y")
    assert_written(sh_out, what="stat_shift_out [0, ldy)")
    assert torch.equal(sh_out.view(torch.int32), sh_d.view(torch.int32))
    n = float(OH * OW)
    cen = acc - shift.double()
    s = stats.sum(0).double().cpu()
    d, d1, d2 = err(y.double().cpu(), acc), err(s[0] / n, cen.sum(dim=(0, 1, 2)) / n), err(s[1] / n, (cen ** 2).sum(dim=(0, 1, 2)) / n)
    report(f"bounds_conv_stat_shift[{dtype},t{tile},k{K},c{Cout}/{ldy}]", rel=d[2], mean_abs=d1[0], sq_rel=d2[2])
    assert d[2] < _tol(dtype) and d1[0] < 2e-3 and d2[2] < 2e-3


@pytest.mark.parametrize("dtype,tile", [(F32, 0), (F32, 11), (F32, 12), (F32, 13), (BF16, 0), (BF16, 11), (BF16, 12), (BF16, 13), (BF16, 46)])
def test_scattered_stride2_gradient_in_place_touches_no_odd_pixel(hip, dtype, tile):
    """mode 1, 1x1, stride 2 with TF_EPI_RES and aux == y: the rows are ADDED to the even-even pixels of a raster that holds another launch's
    result; every other pixel keeps its bits (the header's promise), the guards theirs; MASK2 / STATS3 see the rows of this launch only."""
    from tinyfaces import ops
    N, h, w_, Cg, Cin = 1, 3, 7, 64, 64                     # gradient raster 3 x 7 -> input raster 5 x 13 = 65 pixels
    H, W = 2 * h - 1, 2 * w_ - 1
    g = _g(5)
    wt = torch.randn(Cg, Cin, 1, 1, generator=g) / Cg ** 0.5
    gy = torch.randn(N, Cg, h, w_, generator=g)
    yprev, x3 = torch.randn(N, H, W, Cin, generator=g), torch.randn(N, H, W, Cin, generator=g)
    mask = (q(yprev, dtype) > 0).double()
    g1 = qd(torch.randn(N, H, W, Cin, generator=g), dtype) * mask
    gds = nhwc(F.conv_transpose2d(qd(gy, dtype), qd(wt, dtype), stride=2))
    ref = (g1 + gds) * mask
    raster = guarded((N, H, W, Cin), dtype, DEV, body="keep")
    raster.copy_(g1)
    before = raster.clone()
    a = _conv_args(hip, dtype, 1, N, h, w_, Cg, H, W, Cin, 1, 2, 0, Cin, hip.EPI_RES | hip.EPI_MASK2 | hip.EPI_STATS3, tile)
    mt = hip.lib().tf_conv_mtiles(C.byref(a))
    assert mt >= 1
    stats = guarded((mt, 2, Cin), F32, DEV, body="keep").zero_()
    sums0 = torch.stack([g1.sum(dim=(0, 1, 2)), (g1 * qd(x3, dtype)).sum(dim=(0, 1, 2))])
    stats[0] = sums0.float().cuda()
    out, st = ops.conv2d_nhwc(gin(nhwc(gy), dtype), guarded_like(ops.pack_weight(wt.cuda(), dtype, transpose=True), DEV), Cin, 1, 1, 2, 0, mode=1,
                              out_hw=(H, W), epi=hip.EPI_RES | hip.EPI_MASK2 | hip.EPI_STATS3, aux=raster, aux2=gin(yprev, dtype), aux3=gin(x3, dtype),
                              want_stats=True, tile=tile, out=raster, stats_into=stats)
    _sync_ok()
    assert_guards(raster, "in-place raster")
    assert_guards(stats, "stat_out")
    odd = torch.ones(H, W, dtype=torch.bool)
    odd[0::2, 0::2] = False
    assert torch.equal(raster[:, odd].view(torch.uint8), before[:, odd].view(torch.uint8))      # bit-unchanged
    d = err(raster.double().cpu(), ref)
    tot = st.sum(0).double().cpu()
    want = torch.stack([ref.sum(dim=(0, 1, 2)), (ref * qd(x3, dtype)).sum(dim=(0, 1, 2))])
    d1, d2 = err(tot[0], want[0]), err(tot[1], want[1])
    report(f"bounds_scatter_inplace[{dtype},t{tile}]", rel=d[2], s1=d1[2], s2=d2[2])
    assert d[2] < _tol(dtype) and d1[2] < 5e-3 and d2[2] < 5e-3


# =============================================================================================== b. the leading-dimension contract
HALF_TILES = DMA_TILES + MMA32_TILES


def _affine_launch(hip, dtype, tile, Cout, ldy, OH=5, OW=13, out=None):
    """A 1x1 conv 64 -> Cout over 65 pixels with the AFFINE epilogue, every tensor guarded, per-channel vectors of exactly ldy elements."""
    from tinyfaces import ops
    g, x, wp, acc, _ = _conv_problem(dtype, 0, 1, 1, OH, OW, 64, Cout, ldy, seed=Cout + ldy)
    sc, sh = torch.rand(ldy, generator=g) + 0.5, torch.randn(ldy, generator=g)
    y = guarded((1, OH, OW, ldy), dtype, DEV) if out is None else out
    call = lambda ld: ops.conv2d_nhwc(x, wp, Cout, 1, 1, 1, 0, ldy=ld, epi=hip.EPI_AFFINE, epi_scale=gin(sc), epi_shift=gin(sh), tile=tile, out=y)
    return call, y, acc * sc.double() + sh.double()


@pytest.mark.parametrize("cout", [100, 68])
@pytest.mark.parametrize("tile", HALF_TILES)
@pytest.mark.parametrize("dtype", [BF16, F16])
def test_two_byte_ldy_that_is_no_multiple_of_8_is_refused_before_anything_is_launched(hip, dtype, tile, cout):
    """ldy = Cout = 100 / 68 (a multiple of 4, not of 8) with 2-byte types: the epilogue's last 16-byte chunk of a row would cover the first four
    channels of the next row (a race with their owner) and, on the last row, eight bytes behind y.  tf_conv2d and tf_conv_mtiles return
    TF_ERR_ARG; the NaN-filled output and its guards stay as they were."""
    call, y, _ = _affine_launch(hip, dtype, tile, cout, cout)
    with pytest.raises(RuntimeError, match="TF_ERR_ARG"):
        call(cout)
    a = _conv_args(hip, dtype, 0, 1, 5, 13, 64, 5, 13, cout, 1, 1, 0, cout, hip.EPI_AFFINE | hip.EPI_STATS, tile)
    assert hip.lib().tf_conv_mtiles(C.byref(a)) == -1        # TF_ERR_ARG: a caller cannot size a statistic buffer for it either
    _sync_ok()
    assert_guards(y, "refused launch: y")
    assert unwritten(y)[0] == y.numel()                      # nothing was written


@pytest.mark.parametrize("dtype,cout,ldy", [(BF16, 100, 104), (F16, 68, 72), (F32, 100, 100), (F32, 68, 68), (BF16, 125, 128)])
@pytest.mark.parametrize("tile", [0, 11, 13])
def test_default_ldy_is_the_smallest_the_header_allows_and_stays_inside_its_rows(hip, dtype, cout, ldy, tile):
    """ops.conv2d_nhwc's default leading dimension: Cout rounded up to 4 (fp32) / 8 (2-byte) elements -- one case per type at that smallest
    documented alignment, inside its guards, pad columns [Cout, ldy) written (0 * scale + shift)."""
    call, y, ref = _affine_launch(hip, dtype, tile, cout, ldy)
    out = call(None)                                         # ldy=None: the default
    assert out.data_ptr() == y.data_ptr()
    _sync_ok()
    assert_guards(y, "y")
    assert_written(y, what="y")
    d = err(y.double().cpu(), ref)
    report(f"bounds_ldy_default[{dtype},{cout}/{ldy},t{tile}]", rel=d[2])
    assert d[2] < _tol(dtype)


def test_in_lds_bn_prologue_and_its_side_output_are_refused_by_this_build(hip):
    """tf_conv_args.bnf / bnf_out (once a second [M][Cin] output of the ring-less tile) are reserved fields of a removed prologue: the
    library refuses the launch, y and bnf_out stay untouched."""
    lib = hip.lib()
    g, x, wp, _, _ = _conv_problem(BF16, 0, 1, 1, 5, 13, 64, 64, 64, seed=3)
    y, side = guarded((1, 5, 13, 64), BF16, DEV), guarded((1, 5, 13, 64), BF16, DEV)
    vec = [gin(torch.ones(64)) for _ in range(7)]
    rows = gin(torch.zeros(8, 2, 64))
    desc = hip.BnFwdDesc(rows.data_ptr(), *[v.data_ptr() for v in vec[:6]], None, None, None)
    a = _conv_args(hip, BF16, 0, 1, 5, 13, 64, 5, 13, 64, 1, 1, 0, 64, 0, 32)
    a.x, a.w, a.y = x.data_ptr(), wp.data_ptr(), y.data_ptr()
    a.bnf, a.bnf_out, a.bnf_rows, a.bnf_count, a.bnf_eps, a.bnf_momentum = C.addressof(desc), side.data_ptr(), 8, 65.0, 1e-5, 0.1
    assert lib.tf_conv2d(C.byref(a), hip.stream()) == -3     # TF_ERR_UNSUPPORTED
    _sync_ok()
    for t in (y, side):
        assert_guards(t, "refused launch")
        assert unwritten(t)[0] == t.numel()


# =============================================================================================== b. (audit) / c. weight gradients
def _pw_problem(dtype, M, Cin, Cout, ldx, lddy, seed):
    """A pointwise weight-gradient problem with garbage in the pad columns: (x (1,1,M,ldx), dy (1,1,M,lddy)) guarded, float64 dW (Cout, Cin)."""
    g = _g(seed)
    x, dy = torch.full((M, ldx), 7.0), torch.full((M, lddy), -3.0)
    x[:, :Cin] = torch.randn(M, Cin, generator=g)
    dy[:, :Cout] = torch.randn(M, Cout, generator=g)
    ref = qd(dy[:, :Cout], dtype).t() @ qd(x[:, :Cin], dtype)
    return gin(x.view(1, 1, M, ldx), dtype), gin(dy.view(1, 1, M, lddy), dtype), ref


WG_TOL = {F32: 5e-5, BF16: 2e-3}                           # test_wgrad's bars


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("prob", [(25, 40, 24, 40, 24), (143, 125, 512, 128, 512)])      # M, Cin, Cout, ldx, lddy: the (40, 24) and (125, 512) problems of PWG_CASES
@pytest.mark.parametrize("dtype,tile", [(F32, 0), (F32, 64), (F32, 128), (BF16, 0), (BF16, 1), (BF16, 64), (BF16, 128)])
def test_wgrad_pointwise_stays_inside_dw(hip, dtype, tile, prob, packed):
    """tf_conv2d_wgrad with channel counts below one tile side and dw_ld == Cin*KH*KW exactly: dW (zeroed by the caller, accumulated into)
    right, nothing outside it touched.  ldx = 40 / lddy = 24 are the smallest documented alignment of the 2-byte types' 16-byte slots."""
    from tinyfaces import ops
    assert any(p[:2] == (40, 24) for c in PWG_CASES for p in c[3]) and any(p[:2] == (125, 512) for c in PWG_CASES for p in c[3])
    M, Cin, Cout, ldx, lddy = prob
    x, dy, ref = _pw_problem(dtype, M, Cin, Cout, ldx, lddy, seed=M + tile)
    dw = guarded((Cout, Cin, 1, 1), F32, DEV, body="keep").zero_()
    ops.conv2d_wgrad(x, dy, Cin, Cout, 1, 1, 1, 0, tile=tile, out=dw, packed=packed)
    _sync_ok()
    assert_guards(dw, "dw")
    d = err(dw.double().cpu().reshape(Cout, Cin), ref)
    report(f"bounds_wgrad_pw[{dtype},t{tile},{prob},packed={packed}]", rel=d[2])
    assert d[2] < WG_TOL[dtype]


@pytest.mark.parametrize("dtype,Cin,Cout,ok", [(F32, 36, 20, True), (BF16, 40, 24, True), (BF16, 36, 24, False), (BF16, 40, 20, False)])
def test_wgrad_leading_dimensions_at_their_smallest_alignment(hip, dtype, Cin, Cout, ok):
    """ldx = Cin / lddy = Cout: multiples of 4 (fp32) / 8 (bf16) elements.  (36, 20) works in fp32 and (40, 24) in bf16, inside their guards; a
    bf16 ldx = 36 or lddy = 20 is TF_ERR_ARG from tf_conv2d_wgrad and tf_conv2d_wgrad_group, with dW untouched."""
    from tinyfaces import ops
    x, dy, ref = _pw_problem(dtype, 25, Cin, Cout, Cin, Cout, seed=Cin + Cout)
    if ok:
        dw = guarded((Cout, Cin, 1, 1), F32, DEV, body="keep").zero_()
        ops.conv2d_wgrad(x, dy, Cin, Cout, 1, 1, 1, 0, out=dw)
        _sync_ok()
        assert_guards(dw, "dw")
        d = err(dw.double().cpu().reshape(Cout, Cin), ref)
        report(f"bounds_wgrad_ld[{dtype},{Cin},{Cout}]", rel=d[2])
        assert d[2] < WG_TOL[dtype]
        return
    dw = guarded((Cout, Cin, 1, 1), F32, DEV)
    with pytest.raises(RuntimeError, match="TF_ERR_ARG"):
        ops.conv2d_wgrad(x, dy, Cin, Cout, 1, 1, 1, 0, out=dw)
    with pytest.raises(RuntimeError, match="TF_ERR_ARG"):
        ops.conv2d_wgrad_group([(x, dy, Cin, Cout)], 1, 0, out=[dw])
    _sync_ok()
    assert_guards(dw, "refused: dw")
    assert unwritten(dw)[0] == dw.numel()


@pytest.fixture
def exact_workspace(monkeypatch):
    """ops._workspace without its 25 % + 256 bytes of slack: every request gets exactly the bytes it asked for, between guards."""
    from tinyfaces import ops
    handed = []

    def ws(key, nbytes, device):
        t = guarded_workspace(nbytes, device)
        handed.append((key, int(nbytes), t))
        return t
    monkeypatch.setattr(ops, "_workspace", ws)
    return handed


def _check_workspaces(handed, expect_key=None):
    torch.cuda.synchronize()
    assert handed, "the op asked for no workspace"
    if expect_key is not None:
        assert any(k == expect_key and n > 0 for k, n, _ in handed), [(k, n) for k, n, _ in handed]
    for key, n, t in handed:
        assert_guards(t, f"workspace '{key}' of exactly {n} bytes")


@pytest.mark.parametrize("case", [(2, 5, 7, 64, 64), (1, 9, 11, 128, 192)])
@pytest.mark.parametrize("mode", ["atomics", "packed", "two_phase", "per_tap", "staged"])
def test_wgrad_3x3_stays_inside_dw_and_its_partial_workspace(hip, exact_workspace, case, mode):
    """The 3x3 weight gradients (all-taps kernel with fp32 atomics, its packed layout, its two-phase form through a partial-tile workspace of
    exactly tf_wgrad_workspace_bytes() bytes; the per-tap LDS-DMA kernel; the register-staged kernel) on frames smaller than a stage."""
    from tinyfaces import ops
    dtype = BF16
    N, H, W, Cin, Cout = case
    g = _g(sum(case))
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(N, Cout, H, W, generator=g)
    F.conv2d(qd(x, dtype), w, padding=1).backward(qd(gy, dtype))
    xd, gyd = gin(nhwc(x), dtype), gin(nhwc(gy), dtype)
    kw = dict(atomics=dict(tile=3), packed=dict(tile=3, packed=True), two_phase=dict(tile=3, splitk=3, two_phase=True), per_tap=dict(tile=1),
              staged=dict(tile=64))[mode]
    dw = guarded((Cout, 9, Cin) if mode == "packed" else (Cout, Cin, 3, 3), F32, DEV, body="keep").zero_()
    ops.conv2d_wgrad(xd, gyd, Cin, Cout, 3, 3, 1, 1, out=dw, **kw)
    _sync_ok()
    assert_guards(dw, "dw")
    if mode == "two_phase":
        _check_workspaces(exact_workspace, "wgrad3")
    got = dw.double().cpu()
    if mode == "packed":
        got = got.permute(0, 2, 1).reshape(Cout, Cin, 3, 3)
    d = err(got, w.grad)
    report(f"bounds_wgrad3x3[{case},{mode}]", rel=d[2])
    assert d[2] < 2e-3                                       # test_wgrad3x3_all_taps / test_wgrad


@pytest.mark.parametrize("ci", [1, 2])
def test_wgrad_group_pointwise_overwrites_exactly_dw(hip, ci):
    """tf_conv2d_wgrad_group on the PWG_CASES that hold the (40, 24) and the (125, 512) problems: every dW between guards, NaN before the
    launch (the group OVERWRITES: every element written, none beside)."""
    from tinyfaces import ops
    N, H, W, probs = PWG_CASES[ci]
    M = N * H * W
    ins, refs, outs = [], [], []
    for n, (Cin, Cout, ldx, lddy) in enumerate(probs):
        x, dy, ref = _pw_problem(BF16, M, Cin, Cout, ldx, lddy, seed=ci * 10 + n)
        ins.append((x.view(N, H, W, ldx), dy.view(N, H, W, lddy), Cin, Cout))
        refs.append(ref)
        outs.append(guarded((Cout, Cin, 1, 1), F32, DEV))
    ops.conv2d_wgrad_group(ins, 1, 0, out=outs)
    _sync_ok()
    for n, (dw, ref) in enumerate(zip(outs, refs)):
        assert_guards(dw, f"dw[{n}]")
        assert_written(dw, what=f"dw[{n}]")
        assert torch.isfinite(dw).all(), f"dw[{n}]: a NaN / Inf (an operand read from a guard)"
        e = err(dw.double().cpu().reshape(ref.shape), ref)[2]
        report(f"bounds_wgrad_group_pw[{ci},{n}]", rel=e)
        assert e < 1e-4, (n, e)                              # test_wgrad_group_pointwise; each problem on its own: max() would drop a NaN


def test_wgrad_group_3x3_overwrites_exactly_dw(hip):
    from tinyfaces import ops
    N, H, W, Cin, Cout, n = 2, 9, 11, 64, 64, 3
    g = _g(97)
    ins, refs, outs = [], [], []
    for _ in range(n):
        x, gy = torch.randn(N, Cin, H, W, generator=g), torch.randn(N, Cout, H, W, generator=g)
        w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
        F.conv2d(qd(x, BF16), w, padding=1).backward(qd(gy, BF16))
        refs.append(w.grad)
        ins.append((gin(nhwc(x), BF16), gin(nhwc(gy), BF16), Cin, Cout))
        outs.append(guarded((Cout, Cin, 3, 3), F32, DEV))
    ops.conv2d_wgrad_group(ins, 3, 1, out=outs)
    _sync_ok()
    for n, (dw, ref) in enumerate(zip(outs, refs)):
        assert_guards(dw, f"dw[{n}]")
        assert_written(dw, what=f"dw[{n}]")
        assert torch.isfinite(dw).all(), f"dw[{n}]: a NaN / Inf (an operand read from a guard)"
        e = err(dw.double().cpu(), ref)[2]
        report(f"bounds_wgrad_group_3x3[{n}]", rel=e)
        assert e < 2e-3, (n, e)                              # test_wgrad_group_3x3; each problem on its own: max() would drop a NaN


# =============================================================================================== d. the companions (odd M, C = 64)
def _bn_tols(dtype):
    """test_bn_fused_consumers_chain's bars: (activations, gradients)."""
    return (1e-5, 1e-4) if dtype == F32 else (1.5e-2, 2e-2)


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_maxpool_forward_backward_write_their_tensors_only(hip, dtype):
    """tf_maxpool_fwd (stem BN + ReLU fused in front) / tf_maxpool_bwd on a 19 x 23 raster (odd in both directions: ragged windows on every
    border), C = 64: y, the arg-max bytes and gz between guards, every element written."""
    lib, tfd = hip.lib(), hip.tf_dtype(dtype)
    g = _g(5)
    N, H, W, Cc = 1, 19, 23, 64
    a = torch.randn(N, Cc, H, W, generator=g)
    sc, sh = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3
    act = torch.relu(qd(a, dtype) * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)).requires_grad_(True)
    pref = F.max_pool2d(act, 3, 2, 1)
    PH, PW = pref.shape[2:]
    xin, scd, shd = gin(nhwc(a), dtype), gin(sc), gin(sh)
    y = guarded((N, PH, PW, Cc), dtype, DEV)
    idx = guarded((N * PH * PW * Cc,), torch.uint8, DEV, pitch_bytes=Cc)
    assert lib.tf_maxpool_fwd(tfd, xin.data_ptr(), N, H, W, Cc, scd.data_ptr(), shd.data_ptr(), y.data_ptr(), idx.data_ptr(), hip.stream()) == 0
    _sync_ok()
    for t, what in ((y, "y"), (idx, "argmax")):
        assert_guards(t, what)
        assert_written(t, what=what)                          # (arg-max bytes are window positions 0..8, never 0xFF)
    assert int(idx.max()) <= 8
    d = err(y.double().cpu(), qd(nhwc(pref.detach()).float(), dtype))
    gp = torch.randn(pref.shape, generator=g)
    pref.backward(qd(gp, dtype))
    gz = guarded((N, H, W, Cc), dtype, DEV)
    gpd = gin(nhwc(gp), dtype)
    assert lib.tf_maxpool_bwd(tfd, gpd.data_ptr(), idx.data_ptr(), xin.data_ptr(), scd.data_ptr(), shd.data_ptr(), N, H, W, Cc, gz.data_ptr(), hip.stream()) == 0
    _sync_ok()
    assert_guards(gz, "gz")
    assert_written(gz, what="gz")
    d2 = err(gz.double().cpu(), nhwc(act.grad * (act.detach() > 0)))
    report(f"bounds_maxpool[{dtype}]", pool_maxabs=d[0], pool_bwd_rel=d2[2])
    assert d[0] < (1e-6 if dtype == F32 else 1e-2) and d2[2] < (1e-6 if dtype == F32 else 8e-3)      # test_stem_im2col_and_maxpool


@pytest.mark.parametrize("ds", [False, True])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_bn_fused_consumers_write_their_tensors_only(hip, dtype, ds):
    """tf_bn_relu_fused, tf_bn_add_relu_fused (identity / second BatchNorm on the residual) and tf_bn_bwd_apply_fused at M = 11 * 13 = 143
    rows, C = 64: outputs and every published per-channel vector (exactly C floats each) between guards and fully written; the statistic
    rows hold what tf_colstats wrote into zeros (max(blocks, tf_get_stat_rows()) rows: the consumers read tf_get_stat_rows() of them)."""
    lib, tfd = hip.lib(), hip.tf_dtype(dtype)
    g = _g(100 + ds)
    N, H, W, Cc = 1, 11, 13, 64
    M = N * H * W
    R = lib.tf_get_stat_rows()
    nb = lib.tf_colstats_blocks(M, Cc, tfd)
    xr, idn = torch.randn(M, Cc, generator=g) * 1.3 + 0.2, torch.randn(M, Cc, generator=g) * 0.7 - 0.1
    gam = [torch.rand(Cc, generator=g) + 0.5 for _ in range(2)]
    bet = [torch.randn(Cc, generator=g) * 0.2 for _ in range(2)]
    xq, iq = qd(xr, dtype).requires_grad_(True), qd(idn, dtype).requires_grad_(True)
    gm = [t.double().requires_grad_(True) for t in gam]
    bt = [t.double().requires_grad_(True) for t in bet]

    def bn(v, k):
        mean, var = v.mean(0), v.var(0, unbiased=False)
        return (v - mean) / torch.sqrt(var + 1e-5) * gm[k] + bt[k], mean.detach(), var.detach()
    b1, mean1, var1 = bn(xq, 0)
    yref = torch.relu(b1 + (bn(iq, 1)[0] if ds else iq))
    r1ref = torch.relu(b1.detach())
    gy = torch.randn(M, Cc, generator=g)
    yref.backward(qd(gy, dtype))
    x_d, id_d, gy_d = gin(xr, dtype), gin(idn, dtype), gin(gy, dtype)

    def rows_of(nk, *operands):
        rows = guarded((max(nb, R), nk, Cc), F32, DEV, body="keep").zero_()
        assert lib.tf_colstats(tfd, *operands, M, Cc, Cc, rows.data_ptr(), hip.stream()) == 0
        _sync_ok()
        assert_guards(rows, "colstats rows")
        return rows
    rows1 = rows_of(2, x_d.data_ptr(), None, x_d.data_ptr(), None)
    rows2 = rows_of(2, id_d.data_ptr(), None, id_d.data_ptr(), None)
    vec = lambda: guarded((Cc,), F32, DEV)
    pub1, pub2, pub0 = [vec() for _ in range(4)], [vec() for _ in range(4)], [vec() for _ in range(4)]
    run1 = [gin(torch.zeros(Cc)), gin(torch.ones(Cc))]
    run2 = [gin(torch.zeros(Cc)), gin(torch.ones(Cc))]
    gd, bd = [gin(t) for t in gam], [gin(t) for t in bet]
    P = lambda ts: [t.data_ptr() for t in ts]
    d0 = hip.BnFwdDesc(rows1.data_ptr(), gd[0].data_ptr(), bd[0].data_ptr(), *P(pub0), None, None, None)
    d1 = hip.BnFwdDesc(rows1.data_ptr(), gd[0].data_ptr(), bd[0].data_ptr(), *P(pub1), *P(run1), None)
    d2 = hip.BnFwdDesc(rows2.data_ptr(), gd[1].data_ptr(), bd[1].data_ptr(), *P(pub2), *P(run2), None)
    r1 = guarded((M, Cc), dtype, DEV)
    assert lib.tf_bn_relu_fused(tfd, x_d.data_ptr(), d0, R, M, Cc, float(M), 1e-5, 0.1, r1.data_ptr(), hip.stream()) == 0
    y = guarded((M, Cc), dtype, DEV)
    assert lib.tf_bn_add_relu_fused(tfd, x_d.data_ptr(), d1, id_d.data_ptr(), d2 if ds else None, R, M, Cc, float(M), 1e-5, 0.1, y.data_ptr(), hip.stream()) == 0
    _sync_ok()
    written = [(r1, "bn_relu y"), (y, "bn_add_relu y")] + [(t, "published vector") for t in pub0 + pub1 + (pub2 if ds else [])]
    for t, what in written:
        assert_guards(t, what)
        assert_written(t, what=what)
    for t in run1 + run2 + (pub2 if not ds else []):
        assert_guards(t, "running statistics / unused vectors")
    if not ds:
        assert all(unwritten(t)[0] == Cc for t in pub2)      # identity residual: the second descriptor is not touched
    t_act, t_grad = _bn_tols(dtype)
    dr1, dy = err(r1.double().cpu(), r1ref), err(y.double().cpu(), yref.detach())
    unb = var1 * M / (M - 1)
    drm, drv = err(run1[0].double().cpu(), 0.1 * mean1), err(run1[1].double().cpu(), 0.9 + 0.1 * unb)
    # backward: sums of gz = gy * (y > 0) with x (k = 1) and the residual-branch input (k = 2, ds)
    nk = 3 if ds else 2
    brow = rows_of(nk, gy_d.data_ptr(), y.data_ptr(), x_d.data_ptr(), id_d.data_ptr() if ds else None)
    dga, dbe, gx = vec(), vec(), guarded((M, Cc), dtype, DEV)
    bdesc = hip.BnBwdDesc(brow.data_ptr(), gd[0].data_ptr(), pub1[2].data_ptr(), pub1[3].data_ptr(), dga.data_ptr(), dbe.data_ptr(), nk, 1)
    assert lib.tf_bn_bwd_apply_fused(tfd, gy_d.data_ptr(), y.data_ptr(), x_d.data_ptr(), bdesc, R, M, Cc, float(M), gx.data_ptr(), hip.stream()) == 0
    _sync_ok()
    for t, what in ((gx, "bn_bwd_apply out"), (dga, "dgamma"), (dbe, "dbeta")):
        assert_guards(t, what)
        assert_written(t, what=what)
    assert_guards(y, "y (read as the ReLU mask)")
    dgx, dgg, dgb = err(gx.double().cpu(), xq.grad), err(dga.double().cpu(), gm[0].grad), err(dbe.double().cpu(), bt[0].grad)
    report(f"bounds_bn_fused[{dtype},ds={ds}]", r1_rel=dr1[2], y_rel=dy[2], rm=drm[0], rv=drv[0], gx_rel=dgx[2], dgamma_rel=dgg[2], dbeta_rel=dgb[2])
    assert dr1[2] < t_act and dy[2] < t_act and dgx[2] < t_grad and dgg[2] < t_grad and dgb[2] < t_grad
    assert drm[0] < 1e-4 and drv[0] < 1e-3


@pytest.mark.parametrize("dtype,Cc,ldc", [(F32, 125, 128), (BF16, 125, 128), (F32, 9, 12), (BF16, 9, 16), (F16, 125, 136)])
def test_upsample_add_crop_forward_writes_out_only(hip, dtype, Cc, ldc):
    """tf_upsample_add_crop at 13 x 17 (odd: the crop cuts the upsampled 14 x 18), the head's 125 channels in 128 columns, and one case per
    type at the smallest ldc the header documents (a multiple of 4 fp32 / 8 two-byte elements, not of 16 or 32)."""
    from oracle.model import bilinear_kernel
    lib, tfd = hip.lib(), hip.tf_dtype(dtype)
    g = _g(ldc)
    B, H3, W3 = 2, 13, 17
    H4, W4 = (H3 + 1) // 2, (W3 + 1) // 2
    s3, s4 = torch.randn(B, H3, W3, ldc, generator=g), torch.randn(B, H4, W4, ldc, generator=g)
    wfull = torch.zeros(Cc, Cc, 4, 4, dtype=torch.float64)
    wfull[torch.arange(Cc), torch.arange(Cc)] = torch.from_numpy(bilinear_kernel(4)).double()
    up = F.conv_transpose2d(qd(s4[..., :Cc], dtype).permute(0, 3, 1, 2), wfull, stride=2, padding=1)[:, :, :H3, :W3]
    ref = qd(s3[..., :Cc], dtype).permute(0, 3, 1, 2) + up
    diag = gin(wfull[torch.arange(Cc), torch.arange(Cc)].reshape(Cc, 16).float())
    out = guarded((B, Cc, H3, W3), F32, DEV, pitch_bytes=W3 * 4 * H3)
    s3d, s4d = gin(s3, dtype), gin(s4, dtype)
    assert lib.tf_upsample_add_crop(tfd, s3d.data_ptr(), s4d.data_ptr(), diag.data_ptr(), B, Cc, ldc, H3, W3, H4, W4,
                                    out.data_ptr(), hip.stream()) == 0
    _sync_ok()
    assert_guards(out, "out_nchw")
    assert_written(out, what="out_nchw")
    d = err(out.double().cpu(), ref)
    report(f"bounds_upsample_fwd[{dtype},{Cc}/{ldc}]", fwd_maxabs=d[0])
    assert d[0] < 1e-5                                       # test_upsample_add_crop_fwd_bwd


@pytest.mark.parametrize("dtype,ldc,code", [(BF16, 12, -3), (F16, 132, -3), (F32, 126, -1)])
def test_upsample_add_crop_refuses_a_row_pitch_that_is_no_multiple_of_16_bytes(hip, dtype, ldc, code):
    """ldc no multiple of 4: TF_ERR_ARG (-1) for every type; a multiple of 4 and not of 8 in a two-byte type: TF_ERR_UNSUPPORTED (-3)."""
    lib, tfd = hip.lib(), hip.tf_dtype(dtype)
    B, Cc, H3, W3, H4, W4 = 1, 9, 5, 7, 3, 4
    s3, s4 = gin(torch.randn(B, H3, W3, ldc), dtype), gin(torch.randn(B, H4, W4, ldc), dtype)
    diag = gin(torch.ones(Cc, 16))
    out = guarded((B, Cc, H3, W3), F32, DEV)
    rc = lib.tf_upsample_add_crop(tfd, s3.data_ptr(), s4.data_ptr(), diag.data_ptr(), B, Cc, ldc, H3, W3, H4, W4, out.data_ptr(), hip.stream())
    _sync_ok()
    assert rc == code
    assert_guards(out, "refused: out")
    assert unwritten(out)[0] == out.numel()


@pytest.mark.parametrize("dtype", [F32, BF16])
def test_upsample_add_crop_backward_writes_all_columns_of_g3_and_g4(hip, dtype):
    from oracle.model import bilinear_kernel
    lib, tfd = hip.lib(), hip.tf_dtype(dtype)
    g = _g(13)
    B, Cc, ldc, H3, W3 = 2, 125, 128, 13, 17
    H4, W4 = (H3 + 1) // 2, (W3 + 1) // 2
    wfull = torch.zeros(Cc, Cc, 4, 4, dtype=torch.float64)
    wfull[torch.arange(Cc), torch.arange(Cc)] = torch.from_numpy(bilinear_kernel(4)).double()
    s4 = torch.zeros(B, Cc, H4, W4, dtype=torch.float64, requires_grad=True)
    go = torch.randn(B, Cc, H3, W3, generator=g)
    F.conv_transpose2d(s4, wfull, stride=2, padding=1)[:, :, :H3, :W3].backward(go.double())
    diag = gin(wfull[torch.arange(Cc), torch.arange(Cc)].reshape(Cc, 16).float())
    g3, g4 = guarded((B, H3, W3, ldc), dtype, DEV), guarded((B, H4, W4, ldc), dtype, DEV)
    god = gin(go)
    assert lib.tf_upsample_add_crop_bwd(tfd, god.data_ptr(), diag.data_ptr(), B, Cc, ldc, H3, W3, H4, W4, g3.data_ptr(), g4.data_ptr(), hip.stream()) == 0
    _sync_ok()
    for t, what in ((g3, "g3"), (g4, "g4")):
        assert_guards(t, what)
        assert_written(t, what=f"{what} (all ldc columns)")
        assert float(t[..., Cc:].float().abs().max()) == 0   # pad columns: zeros
    d3, d4 = err(g3.double().cpu()[..., :Cc], nhwc(go.double())), err(g4.double().cpu()[..., :Cc], nhwc(s4.grad))
    report(f"bounds_upsample_bwd[{dtype}]", g3=d3[2], g4=d4[2])
    assert d3[2] < TOL[dtype] and d4[2] < TOL[dtype]         # test_upsample_add_crop_fwd_bwd
    bad = guarded((B, H3, W3, 136), dtype, DEV)              # ldc = 136: a multiple of 8, not of the backward's 32-channel chunk
    assert lib.tf_upsample_add_crop_bwd(tfd, god.data_ptr(), diag.data_ptr(), B, Cc, 136, H3, W3, H4, W4, bad.data_ptr(), g4.data_ptr(), hip.stream()) == -1
    _sync_ok()
    assert_guards(bad, "refused: g3")
    assert unwritten(bad)[0] == bad.numel()


@pytest.mark.parametrize("dtype,ldc", [(F32, 152), (BF16, 152), (BF16, 192)])
def test_stem_im2col_writes_all_ldc_columns_of_its_rows(hip, dtype, ldc):
    """tf_stem_im2col on (1, 37, 45): ldc = 152 is the smallest the header allows (>= 147, a multiple of 8, not of 16); 148 is refused."""
    lib, tfd = hip.lib(), hip.tf_dtype(dtype)
    g = _g(ldc)
    N, H, W = 1, 37, 45
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = torch.randn(N, 3, H, W, generator=g)
    col = guarded((N * OH * OW, ldc), dtype, DEV)
    xd = gin(x)
    assert lib.tf_stem_im2col(xd.data_ptr(), N, H, W, tfd, col.data_ptr(), ldc, hip.stream()) == 0
    _sync_ok()
    assert_guards(col, "col")
    assert_written(col, what="col")
    ref = F.unfold(qd(x, dtype), 7, padding=3, stride=2).transpose(1, 2).reshape(-1, 147)
    assert err(col.double().cpu()[:, :147], ref)[0] == 0 and float(col[:, 147:].float().abs().max()) == 0      # test_stem_im2col_and_maxpool
    col2 = guarded((N * OH * OW, 148), dtype, DEV)
    assert lib.tf_stem_im2col(xd.data_ptr(), N, H, W, tfd, col2.data_ptr(), 148, hip.stream()) == -1
    _sync_ok()
    assert_guards(col2, "refused: col")
    assert unwritten(col2)[0] == col2.numel()


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_stem_conv_writes_its_rows_and_statistic_rows_only(hip, dtype):
    """tf_stem_conv on (1, 37, 45) -> 19 x 23 = 437 output pixels (partial tiles on every border): y [437][64] and the statistic rows
    [tf_get_stat_rows()][2][64] between guards, with the batch-statistic and the folded-BN + ReLU epilogue."""
    from tinyfaces import ops
    lib, tfd = hip.lib(), hip.tf_dtype(dtype)
    g = _g(31)
    N, H, W = 1, 37, 45
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x = torch.randn(N, 3, H, W, generator=g)
    w = torch.randn(64, 3, 7, 7, generator=g) / 147 ** 0.5
    ref = nhwc(F.conv2d(qd(x, dtype), qd(w, dtype), stride=2, padding=3))
    xd = gin(x)
    wp = guarded_like(ops.pack_weight(w.cuda().reshape(64, 147, 1, 1), dtype, cols_pad=192), DEV)
    y = guarded((N, OH, OW, 64), dtype, DEV)
    st = guarded((lib.tf_get_stat_rows(), 2, 64), F32, DEV, body="keep").zero_()
    rows = C.c_int(0)
    assert lib.tf_stem_conv(tfd, xd.data_ptr(), N, H, W, wp.data_ptr(), 192, y.data_ptr(), hip.EPI_STATS, None, None, st.data_ptr(), C.byref(rows), hip.stream()) == 0
    _sync_ok()
    assert_guards(y, "y"); assert_guards(st, "stat_out")
    assert_written(y, what="y")
    assert 1 <= rows.value <= st.shape[0]
    s = st[:rows.value].sum(0).double().cpu()
    d, d1, d2 = err(y.double().cpu(), ref), err(s[0], ref.sum(dim=(0, 1, 2))), err(s[1], (ref ** 2).sum(dim=(0, 1, 2)))
    sc, sh = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.2
    y2, scd, shd = guarded((N, OH, OW, 64), dtype, DEV), gin(sc), gin(sh)
    assert lib.tf_stem_conv(tfd, xd.data_ptr(), N, H, W, wp.data_ptr(), 192, y2.data_ptr(), hip.EPI_AFFINE | hip.EPI_RELU, scd.data_ptr(), shd.data_ptr(),
                            None, C.byref(rows), hip.stream()) == 0
    _sync_ok()
    assert_guards(y2, "y (eval)")
    assert_written(y2, what="y (eval)")
    d3 = err(y2.double().cpu(), torch.relu(ref * sc.double() + sh.double()))
    report(f"bounds_stem_conv[{dtype}]", rel=d[2], sum_rel=d1[2], sumsq_rel=d2[2], eval_rel=d3[2])
    assert d[2] < TOL_H[dtype] and d3[2] < TOL_H[dtype] and d1[2] < 1e-4 and d2[2] < 1e-4      # test_stem_conv_direct_equals_im2col_gemm_and_torch


# =============================================================================================== e. workspace sizes without slack
@pytest.mark.parametrize("n,seed", [(63, 1), (64, 2), (65, 3), (1025, 4), (2049, 5)])
def test_nms_in_exactly_its_workspace(exact_workspace, n, seed):
    """tf_nms_f64 with tf_nms_workspace_bytes(n) bytes and not one more (test_nms_random_vs_oracle's boxes: many exact score ties)."""
    from tinyfaces import ops
    from oracle.nms import nms as onms
    rng = np.random.RandomState(seed)
    cx, cy = rng.uniform(0, 1500, n), rng.uniform(0, 1000, n)
    w = np.exp(rng.uniform(np.log(8), np.log(150), n)); h = w * rng.uniform(1.0, 1.4, n)
    boxes = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    scores = np.round(rng.randn(n), 2)
    keep = ops.nms(torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), 0.3).cpu().numpy()
    _check_workspaces(exact_workspace, "nms")
    assert np.array_equal(keep, onms(boxes, scores, 0.3))


def test_batched_nms_with_an_empty_segment_in_exactly_its_workspace(exact_workspace):
    from tinyfaces import ops
    from oracle.nms import nms as onms
    rng = np.random.RandomState(11)
    sizes = [65, 0, 129, 1]
    n = sum(sizes)
    c, wh = rng.uniform(0, 400, (n, 2)), rng.uniform(10, 80, (n, 2))
    boxes, scores = np.concatenate([c - wh / 2, c + wh / 2], 1), np.round(rng.randn(n), 1)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    keeps = ops.nms_batched(torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda(), offs.tolist(), 0.3)
    _check_workspaces(exact_workspace, "nms")
    assert len(keeps) == len(sizes)
    for k, (sz, o) in enumerate(zip(sizes, offs)):
        want = onms(boxes[o:o + sz], scores[o:o + sz], 0.3) + o if sz else np.empty(0, np.int64)
        assert np.array_equal(keeps[k].cpu().numpy(), want), f"segment {k} (n={sz})"


def test_decode_golden_in_exactly_its_workspace(exact_workspace, golden):
    from tinyfaces.models.utils import get_bboxes
    from oracle.targets import RF
    g, t, tag = golden("decode"), golden("targets")["templates"], "d0"
    b, s = get_bboxes(g[f"{tag}_score_cls"], g[f"{tag}_score_reg"], g[f"{tag}_prob"].copy(), t, float(g[f"{tag}_thr"]), RF, float(g[f"{tag}_scale"]))
    _check_workspaces(exact_workspace, "decode")
    rb, rs = g[f"{tag}_boxes"], g[f"{tag}_scores"]
    assert b.shape[0] == rb.shape[0] and np.array_equal(s, rs)                    # test_decode_golden's asserts
    size = float(max((rb[:, 2] - rb[:, 0]).max(), (rb[:, 3] - rb[:, 1]).max()))
    assert np.abs(b - rb).max() <= 1.3e-7 * size


def test_criterion_golden_in_exactly_its_workspace_writes_every_gradient_element_once(exact_workspace, golden):
    """Criterion golden case 0 with a workspace of exactly tf_criterion_workspace_bytes() and a NaN-filled gradient between guards: the kernel
    promises to write every element of the gradient itself (no memset)."""
    from tinyfaces import ops
    from oracle import criterion as ocrit
    from test_gpu_small_ops import _keep_flags
    g, tag = golden("criterion"), "k0"
    out = torch.from_numpy(g[f"{tag}_output"])
    cm = torch.from_numpy(g[f"{tag}_class_map"].astype(np.float32))
    rm = torch.from_numpy(g[f"{tag}_reg_map"])
    np.random.seed(int(g[f"{tag}_seed"]))
    r = ocrit.criterion(out, cm, rm)
    B, _, H, W = out.shape
    pk, nk = _keep_flags(r["records"], B, 25 * H * W)
    cm_d = gin(cm)
    grad = guarded(out.shape, F32, DEV, pitch_bytes=W * 4)
    loss2, gout, labels = ops.criterion_fwd_bwd(gin(out), cm_d, gin(rm), pos_keep=pk, neg_keep=nk, want_labels=True, grad=grad)
    _check_workspaces(exact_workspace, "criterion")
    assert gout is grad
    assert_guards(grad, "grad")
    assert_guards(cm_d, "class_map (mined in place)")
    assert_written(grad, what="grad")
    ref = g[f"{tag}_loss"]
    assert int((labels.cpu() != r["class_map_final"]).sum()) == 0                # test_criterion_golden's asserts
    assert np.allclose(loss2.cpu().numpy(), [ref[1], ref[2]], rtol=1e-5)
    assert np.allclose(grad.cpu().numpy(), g[f"{tag}_grad"], rtol=1e-5, atol=1e-6)


def test_targets_golden_in_exactly_its_workspace(exact_workspace, golden):
    from tinyfaces import ops
    from oracle import targets as otgt
    from test_gpu_small_ops import _noise, _valid
    g, tag = golden("targets"), "c0"
    t, boxes = g["templates"], g[f"{tag}_boxes"]
    noise = _noise(g, tag, _valid(boxes).shape[0])
    cm, rm = ops.dense_overlap_targets([boxes], t, paste_boxes=[g[f"{tag}_paste"]], flips=[int(g[f"{tag}_flip"])], noise=[noise])
    _check_workspaces(exact_workspace, "targets")
    cm, rm = cm.cpu().numpy()[0].transpose(1, 2, 0), rm.cpu().numpy()[0].transpose(1, 2, 0)
    pad = otgt.get_padding(t, g[f"{tag}_paste"])
    if int(g[f"{tag}_flip"]):
        pad = np.fliplr(pad)
    _, orm, _ = otgt.get_heatmaps(boxes.copy(), t, pad, noise=noise)
    assert np.array_equal(cm.astype(np.int8), g[f"{tag}_class"])                 # test_targets_vs_reference_golden's asserts
    rm_ref = orm.astype(np.float32)
    assert int((rm != rm_ref).sum()) <= max(1, rm.size // 100000) and np.allclose(rm, rm_ref, rtol=2e-7, atol=0)


# =============================================================================================== f. the executor's workspace
_TRUNK_STATE = {}


def _trunk_model(name, dtype):
    from test_gpu_trunks import oracle_model, product_model
    if name not in _TRUNK_STATE:
        _TRUNK_STATE[name] = oracle_model(name).state_dict()
    m = product_model(name, None, dtype)
    m.load_state_dict(_TRUNK_STATE[name], strict=True)
    m.model.bn1.momentum = 0.0                               # the running means are the shift of the statistic sums: keep them fixed between the two passes
    return m


@pytest.mark.parametrize("name,dtype,mode", [("resnet50", d, k) for d in (BF16, F32) for k in ("eval", "train", "frozen")] + [("resnet101", BF16, "train")])
def test_executor_stays_inside_exactly_its_workspace(hip, name, dtype, mode):
    """DetectionModel with `_ws` pre-installed as a guarded view of exactly tf_detnet_trunk_workspace_bytes() bytes (0xFF-filled: nothing the
    executor reads may be left over from an earlier pass), golden-style (2, 3, 97, 131): the maps equal a pass through an ordinary
    workspace bit for bit (statistic rows unfolded: no atomics in the forward), and the bump-allocated tensors never leave the workspace
    (the guards hold 384 rows of the widest activation: 1024 fp32 channels).  The gradients are NOT asked bit for bit: the weight gradients
    are split over pixel slices that add into dW with fp32 atomics, whose order differs between two passes through the SAME workspace too.
    Each gradient is finite and within 1e-4 of its own largest element of the ordinary pass (the bar
    test_frozen_dual_stream_backward_equals_single_stream sets for the same effect); which ones came out bit-identical is reported."""
    from tinyfaces.models import model as mm
    lib = hip.lib()
    m = _trunk_model(name, dtype)
    m = m.eval() if mode == "eval" else m.train()
    m.freeze_batchnorm(mode == "frozen")
    g = _g(9)
    x = torch.randn(2, 3, 97, 131, generator=g).cuda()
    gy = None
    N, _, H, W = x.shape
    emode = {"eval": 0, "train": 1, "frozen": hip.TF_DETNET_FROZEN_BN}[mode]
    prev = lib.tf_get_stat_rows()

    def run(ws):
        nonlocal gy
        m._ws = ws
        m.zero_grad(set_to_none=True)
        if mode == "eval":
            with torch.no_grad():
                y = m(x)
            grads = {}
        else:
            y = m(x)
            if gy is None:
                gy = (torch.randn(y.shape, generator=g) * 0.1).cuda()
            y.backward(gy)
            grads = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
        torch.cuda.synchronize()
        return y.detach().clone(), grads
    try:
        lib.tf_set_stat_rows(0)
        m._sync_tables(x.device)
        y0, g0 = run(None)
        nbytes = lib.tf_detnet_trunk_workspace_bytes(mm._trunk_arg(m.trunk), m.compute_dtype, N, H, W, m.num_out, emode)
        assert m._ws.numel() == nbytes                       # what an ordinary pass allocates
        ws = guarded_workspace(nbytes, x.device, pitch_bytes=4096)
        y1, g1 = run(ws)
        assert m._ws is ws                                    # large enough: reused, not replaced
        assert_guards(ws, f"executor workspace of exactly {nbytes} bytes")
    finally:
        lib.tf_set_stat_rows(prev)
        m._ws = None
    assert torch.isfinite(y0).all() and torch.isfinite(y1).all()
    assert torch.equal(y1, y0)
    assert set(g1) == set(g0) and (mode == "eval" or len(g0) > 40)
    rels = {}
    for k in g0:                                              # each gradient on its own (max() over floats would drop a NaN)
        assert torch.isfinite(g0[k]).all() and torch.isfinite(g1[k]).all(), f"{k}: a NaN / Inf in a gradient"
        rels[k] = float((g1[k] - g0[k]).abs().max() / (g0[k].abs().max() + 1e-30))
    exact = [k for k in g0 if torch.equal(g1[k], g0[k])]
    report(f"bounds_executor[{name},{dtype},{mode}]", ws_bytes=nbytes, grads=len(g0), grad_worst_rel=max(rels.values(), default=0.0),
           grads_bit_identical=len(exact), differing=",".join(sorted(set(g0) - set(exact))[:6]))
    for k, r in rels.items():
        assert r < 1e-4, (k, r)
