"""-m gpu: the deterministic (slab) form of the weight gradients at operator level -- tf_conv2d_wgrad_det, tf_stem_wgrad_det.

Every case: dW starts NON-ZERO between guard bands (tests/redzone.py), the slab is sized exactly by the query, pre-filled with NaN (0xFF) and
sits between guard bands too; two calls must agree bit for bit, and the result minus the starting dW must meet the bar tests/test_gpu_conv.py
applies to the atomic form of the same kernel (torch autograd on the rounded operands: 5e-5 fp32, 2e-3 bf16, 3e-3 for the padded-head and
stem shapes).  The summation order is pinned bit for bit against tests/wgrad_det_ref.py on planted powers of two."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import wgrad_det_ref as ref
from gpu_util import err, q, report, to_nhwc
from redzone import assert_guards, guarded, guarded_workspace, unwritten
from test_gpu_conv import W3_CASES, WG_CASES

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DEV = "cuda"
TOL = {F32: 5e-5, BF16: 2e-3}
PAD_TOL = {F32: 5e-5, BF16: 3e-3}              # test_wgrad_with_prologue_and_padded_head's bar for the head and stem shapes

CASES = {
    # name: (N, H, W, Cin, Cout, K, stride, ldx, lddy, padded-shape bar)
    "below_one_stage": (1, 9, 7, 64, 64, 1, 1, 64, 64, False),              # M = 63 (WG_CASES[0])
    "ragged_last_stage": (2, 9, 7, 128, 128, 1, 1, 128, 128, False),        # M = 126 = 64 + 62 (fp32: 3 x 32 + 30)
    "head_125_of_128": (2, 12, 16, 512, 125, 1, 1, 512, 128, True),
    "stem_147_of_192": (2, 12, 16, 147, 64, 1, 1, 192, 64, True),
    "below_one_tile": (1, 5, 5, 40, 24, 1, 1, 40, 24, False),
    "3x3_stride2": (2, 21, 19, 128, 128, 3, 2, 128, 128, False),            # WG_CASES[3]
    "3x3_stride1": (2, 20, 22, 64, 64, 3, 1, 64, 64, False),                # WG_CASES[2], W3_CASES[2]
    "3x3_rect_192": (2, 30, 17, 128, 192, 3, 1, 128, 192, False),           # W3_CASES[6]
    "pointwise_16_tiles": (2, 16, 16, 1024, 256, 1, 1, 1024, 256, False),   # WG_CASES[6]
    "pointwise_stride2": (2, 31, 29, 512, 1024, 1, 2, 512, 1024, False),    # WG_CASES[5]
}
assert {CASES["below_one_stage"][:7], CASES["3x3_stride2"][:7], CASES["3x3_stride1"][:7], CASES["pointwise_16_tiles"][:7],
        CASES["pointwise_stride2"][:7]} <= set(WG_CASES) and CASES["3x3_rect_192"][:5] in W3_CASES


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _tiles_for(name, dtype):
    """The `tile` codes that reach a kernel for this case: 1 = per-tap DMA (bf16), 3 = all-taps (bf16, 3x3 / stride 1), 64 / 128 = register-staged."""
    K, s = CASES[name][5], CASES[name][6]
    if dtype == F32:
        return [0, 64, 128]
    return [0, 1, 64, 128] + ([3] if K == 3 and s == 1 else [])


@functools.lru_cache(maxsize=None)
def _problem(name, dtype):
    """(x NHWC on the device with ldx columns, dy NHWC with lddy columns, autograd's dW on the rounded operands, a non-zero starting dW)."""
    N, H, W, Cin, Cout, K, s, ldx, lddy, _ = CASES[name]
    g = _g(sum(map(ord, name)))
    x = torch.randn(N, Cin, H, W, generator=g)
    w = (torch.randn(Cout, Cin, K, K, generator=g) * 0.05).requires_grad_(True)
    y = F.conv2d(q(x, dtype), w, stride=s, padding=K // 2)
    gy = torch.randn(y.shape, generator=g)
    y.backward(q(gy, dtype))
    xp = torch.cat([x, torch.zeros(N, ldx - Cin, H, W)], 1) if ldx > Cin else x
    gyp = torch.cat([gy, torch.zeros(N, lddy - Cout, *gy.shape[2:])], 1) if lddy > Cout else gy
    base = torch.randn(Cout, Cin, K, K, generator=g)
    return to_nhwc(xp, dtype), to_nhwc(gyp, dtype), w.grad.detach().clone(), base


def _det(name, dtype, tile, splitk, packed=False, row_scale=None, pro=None, ws_bytes=None, xdy=None, base=None):
    """One deterministic call into a guarded non-zero dW through a guarded, NaN-filled slab sized exactly by the query (or ws_bytes)."""
    from tinyfaces import ops
    N, H, W, Cin, Cout, K, s = CASES[name][:7]
    xd, gyd = xdy if xdy is not None else _problem(name, dtype)[:2]
    base = _problem(name, dtype)[3] if base is None else base
    if packed:
        base = base.reshape(Cout, Cin, K * K).permute(0, 2, 1).contiguous().reshape(Cout, Cin, K, K)      # the same numbers as [Cout][tap][Cin]
    want = ops.wgrad_det_workspace_bytes(xd, gyd, Cin, Cout, K, K, s, K // 2, pro=pro, splitk=splitk, tile=tile)
    assert want > 0
    slab = guarded_workspace(want if ws_bytes is None else ws_bytes, DEV)
    dw = guarded((Cout, Cin, K, K), F32, DEV, body="keep")
    dw.copy_(base)
    out = ops.conv2d_wgrad(xd, gyd, Cin, Cout, K, K, s, K // 2, pro=pro, splitk=splitk, tile=tile, out=dw, packed=packed, row_scale=row_scale,
                           deterministic=True, slab=slab)
    torch.cuda.synchronize()
    assert out is dw
    assert_guards(slab, "slab")
    assert_guards(dw, "dw")
    got = dw.detach().cpu()
    if packed:
        got = got.reshape(Cout, K * K, Cin).permute(0, 2, 1).reshape(Cout, Cin, K, K)
    return got, want


def _cases_tiles():
    return [(n, d, t) for n in CASES for d in (F32, BF16) for t in _tiles_for(n, d)]


@pytest.mark.parametrize("splitk", [0, 1, 3, 7])
@pytest.mark.parametrize("name,dtype,tile", _cases_tiles())
def test_two_calls_agree_bit_for_bit_and_meet_the_atomic_forms_bar(name, dtype, tile, splitk):
    wgrad, base = _problem(name, dtype)[2:]
    a, _ = _det(name, dtype, tile, splitk)
    b, _ = _det(name, dtype, tile, splitk)
    d = err(a - base, wgrad)
    report(f"wgrad_det[{name},{dtype},t{tile},sk{splitk}]", rel=d[2])
    print(f"wgrad_det[{name},{dtype},t{tile},sk{splitk}] rel {d[2]:.3e}")
    assert torch.equal(a, b)
    assert d[2] < (PAD_TOL if CASES[name][9] else TOL)[dtype]


@pytest.mark.parametrize("name,dtype,tile,kernel", [("3x3_stride1", BF16, 3, "all_taps"), ("3x3_rect_192", BF16, 0, "all_taps"), ("3x3_stride2", BF16, 0, "dma"),
                                                    ("pointwise_16_tiles", BF16, 128, "reg128_bf16"), ("3x3_stride1", F32, 0, "reg64_f32")])
def test_a_slab_of_two_slices_caps_a_plan_of_seven(name, dtype, tile, kernel):
    """splitk = 7 asked (more than two slices in the restated plan), a slab of two slices and a bit handed in: the result repeats and meets the
    bar, nothing outside the slab is touched -- on every kernel, the all-taps one through its two-phase form included."""
    N, H, W, Cin, Cout, K, s = CASES[name][:7]
    wgrad, base = _problem(name, dtype)[2:]
    M = N * (H + 2) * (W + 2) if kernel == "all_taps" else N * ((H + 2 * (K // 2) - K) // s + 1) * ((W + 2 * (K // 2) - K) // s + 1)
    one = ref.slice_bytes(kernel, Cin, Cout, K * K)
    assert len(ref.plan(kernel, M, Cin, Cout, K * K, 7)) > 2
    a, want = _det(name, dtype, tile, 7, ws_bytes=2 * one + 112)
    b, _ = _det(name, dtype, tile, 7, ws_bytes=2 * one + 112)
    assert want == ref.preferred_bytes(kernel, M, Cin, Cout, K * K, 7)
    d = err(a - base, wgrad)
    report(f"wgrad_det_capped[{name},{dtype},t{tile}]", rel=d[2])
    assert torch.equal(a, b)
    assert d[2] < TOL[dtype]


@pytest.mark.parametrize("splitk", [0, 3])
@pytest.mark.parametrize("name,dtype,tile", [(n, d, t) for (n, d, t) in _cases_tiles() if n in ("below_one_tile", "3x3_stride2", "3x3_stride1", "head_125_of_128")])
def test_packed_output_is_the_oihw_result_bit_for_bit(name, dtype, tile, splitk):
    """[Cout][tap][Cin]: the same plan and the same order, another address -- the same bits, the same single writer."""
    wgrad, base = _problem(name, dtype)[2:]
    a, _ = _det(name, dtype, tile, splitk)
    p, _ = _det(name, dtype, tile, splitk, packed=True)
    p2, _ = _det(name, dtype, tile, splitk, packed=True)
    d = err(p - base, wgrad)
    report(f"wgrad_det_packed[{name},{dtype},t{tile},sk{splitk}]", rel=d[2])
    assert torch.equal(p, p2) and torch.equal(p, a)
    assert d[2] < (PAD_TOL if CASES[name][9] else TOL)[dtype]


@pytest.mark.parametrize("splitk", [0, 3])
@pytest.mark.parametrize("name,dtype,tile", [(n, d, t) for (n, d, t) in _cases_tiles() if n in ("ragged_last_stage", "head_125_of_128", "3x3_stride2") and t != 3])
def test_row_scale_is_applied_once_to_the_sum(name, dtype, tile, splitk):
    """dW = dW_in + row_scale[co] * total: bit-equal to the unscaled call's total scaled on the host (one rounded product, one rounded add)."""
    Cout = CASES[name][4]
    wgrad, base = _problem(name, dtype)[2:]
    rs = (torch.rand(Cout, generator=_g(5)) + 0.5)
    zero = torch.zeros_like(base)
    total, _ = _det(name, dtype, tile, splitk, base=zero)                                     # 0 + total = total exactly
    a, _ = _det(name, dtype, tile, splitk, row_scale=rs.to(DEV))
    b, _ = _det(name, dtype, tile, splitk, row_scale=rs.to(DEV))
    want = torch.from_numpy(ref.reduce_into(base.numpy(), total.numpy()[None], row_scale=rs.numpy()))
    d = err(a - base, wgrad * rs.view(-1, 1, 1, 1))
    report(f"wgrad_det_rs[{name},{dtype},t{tile},sk{splitk}]", rel=d[2])
    assert torch.equal(a, b) and torch.equal(a, want)
    assert d[2] < (PAD_TOL if CASES[name][9] else TOL)[dtype]


@pytest.mark.parametrize("splitk", [0, 3])
@pytest.mark.parametrize("tile", [0, 64, 128])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_prologue_takes_the_register_staged_kernel(dtype, tile, splitk):
    """pro=: the BatchNorm + ReLU prologue of test_wgrad_with_prologue_and_padded_head (3x3, 128 -> 256) in the slab form."""
    from tinyfaces import ops
    g = _g(77)
    N, H, W, Cin, Cout = 2, 12, 16, 128, 256
    raw = torch.randn(N, Cin, H, W, generator=g)
    ps, ph = torch.rand(Cin, generator=g) + 0.5, torch.randn(Cin, generator=g) * 0.3
    act = q(torch.relu(q(raw, dtype) * ps.view(1, -1, 1, 1) + ph.view(1, -1, 1, 1)), dtype)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * 0.05).requires_grad_(True)
    y = F.conv2d(act, w, padding=1)
    gy = torch.randn(y.shape, generator=g)
    y.backward(q(gy, dtype))
    base = torch.randn(Cout, Cin, 3, 3, generator=g)
    xd, gyd, pro = to_nhwc(raw, dtype), to_nhwc(gy, dtype), (ps.to(DEV), ph.to(DEV), True)
    outs = []
    for _ in range(2):
        slab = guarded_workspace(ops.wgrad_det_workspace_bytes(xd, gyd, Cin, Cout, 3, 3, 1, 1, pro=pro, splitk=splitk, tile=tile), DEV)
        dw = guarded((Cout, Cin, 3, 3), F32, DEV, body="keep")
        dw.copy_(base)
        ops.conv2d_wgrad(xd, gyd, Cin, Cout, 3, 3, 1, 1, pro=pro, splitk=splitk, tile=tile, out=dw, deterministic=True, slab=slab)
        torch.cuda.synchronize()
        assert_guards(slab, "slab")
        assert_guards(dw, "dw")
        outs.append(dw.cpu())
    d = err(outs[0] - base, w.grad)
    report(f"wgrad_det_pro[{dtype},t{tile},sk{splitk}]", rel=d[2])
    assert torch.equal(outs[0], outs[1])
    assert d[2] < PAD_TOL[dtype]


# ------------------------------------------------------------------ the order, pinned bit for bit
def _planted(kernel, dtype, tile, splitk, n_slices_of_pixels, slab_slices=None):
    """Pointwise 64 -> 64, x = 1, dy constant per slice of the restated plan and a power of two: every slice's partial tile is EXACT
    (pixels x value), so the total depends on the order alone.  The big slice is the first one for co < 32 and the last one for co >= 32."""
    from tinyfaces import ops
    pk = ref.KERNELS[kernel]["PK"]
    M = pk * n_slices_of_pixels
    one = ref.slice_bytes(kernel, 64, 64, 1)
    slab_bytes = None if slab_slices is None else slab_slices * one + 100          # (not a whole number of slices)
    sl = ref.plan(kernel, M, 64, 64, 1, splitk, slab_bytes)
    n = len(sl)
    dy = torch.zeros(M, 64)
    partial = np.zeros((n, 64, 64), np.float64)
    for s, (a, b) in enumerate(sl):
        v = torch.full((64,), 2.0 ** -6)
        v[:32] = 2.0 ** 18 if s == 0 else 2.0 ** -6
        v[32:] = 2.0 ** 18 if s == n - 1 else 2.0 ** -6
        dy[a:b] = v
        partial[s] = (float(b - a) * v.double().numpy())[:, None]
    assert np.array_equal(partial.astype(np.float32).astype(np.float64), partial)              # exact in fp32
    want = ref.reduce_into(np.zeros((64, 64), np.float32), partial.astype(np.float32))
    x = torch.ones(1, 1, M, 64, dtype=dtype, device=DEV)
    gyd = dy.view(1, 1, M, 64).to(dtype).to(DEV)
    assert torch.equal(gyd.float().cpu().view(M, 64), dy)                                      # the planted values survive the operand type
    pref = ops.wgrad_det_workspace_bytes(x, gyd, 64, 64, 1, 1, 1, 0, splitk=splitk, tile=tile)
    assert pref == len(ref.plan(kernel, M, 64, 64, 1, splitk)) * one
    slab = guarded_workspace(pref if slab_bytes is None else slab_bytes, DEV)
    dw = guarded((64, 64, 1, 1), F32, DEV, body="keep").zero_()
    ops.conv2d_wgrad(x, gyd, 64, 64, 1, 1, 1, 0, splitk=splitk, tile=tile, out=dw, deterministic=True, slab=slab)
    torch.cuda.synchronize()
    assert_guards(slab, "slab")
    assert_guards(dw, "dw")
    # the slab holds exactly the planned slices' tiles, [slice][co][ci], and not one byte more
    tiles = slab[:n * one].view(torch.float32).view(n, 64, 64).cpu().numpy()
    assert np.array_equal(tiles, partial.astype(np.float32))
    assert unwritten(slab[n * one:])[0] == slab.numel() - n * one
    return dw.cpu().numpy().reshape(64, 64), want, partial, n


@pytest.mark.parametrize("kernel,dtype,tile", [("dma", BF16, 0), ("reg64_f32", F32, 0), ("reg64_bf16", BF16, 64)])
@pytest.mark.parametrize("splitk,pixels,slab_slices", [(1, 5, None), (3, 7, None), (7, 7, None), (15, 15, None), (16, 16, None), (33, 33, None),
                                                        (130, 130, None), (0, 40, None), (7, 7, 3), (40, 40, 17), (0, 64, 2)])
def test_summation_order_is_the_restated_one(kernel, dtype, tile, splitk, pixels, slab_slices):
    got, want, partial, n = _planted(kernel, dtype, tile, splitk, pixels, slab_slices)
    if slab_slices is not None:
        assert n <= slab_slices
    if n >= 3:
        # the planted values do depend on the order: summed last-to-first they give other bits
        rev = ref.reduce_into(np.zeros((64, 64), np.float32), partial[::-1].astype(np.float32))
        assert not np.array_equal(rev, want)
    assert np.array_equal(got, want), f"{n} slices: co 0 got {got[0, 0]!r} want {want[0, 0]!r}; co 63 got {got[63, 0]!r} want {want[63, 0]!r}"


# ------------------------------------------------------------------ stem
@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("shape", [(2, 37, 45), (1, 130, 71), (3, 64, 64), (2, 250, 250)])
def test_stem_wgrad_det_repeats_and_meets_the_direct_kernels_bar(dtype, shape):
    """The shapes and bars of test_stem_wgrad_direct_equals_autograd, without and with the folded BN-backward apply; a capped slab (three
    tiles: three blocks walk all tiles) too."""
    from tinyfaces import ops
    from tinyfaces._hip import lib
    g = _g(37)
    N, H, W = shape
    x = torch.randn(N, 3, H, W, generator=g)
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gy = torch.randn(N, 64, OH, OW, generator=g)
    w = torch.zeros(64, 3, 7, 7, requires_grad=True)
    F.conv2d(q(x, dtype), w, stride=2, padding=3).backward(q(gy, dtype))
    xc = torch.randn(N, 64, OH, OW, generator=g)
    cA, cB, cD = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1, torch.randn(64, generator=g) * 0.05
    ga = q(cA.view(1, -1, 1, 1) * q(gy, dtype) + cB.view(1, -1, 1, 1) * q(xc, dtype) + cD.view(1, -1, 1, 1), dtype)
    w2 = torch.zeros(64, 3, 7, 7, requires_grad=True)
    F.conv2d(q(x, dtype), w2, stride=2, padding=3).backward(ga)
    base = torch.randn(64, 3, 7, 7, generator=g)
    want = lib().tf_stem_wgrad_det_workspace_bytes(N, H, W)
    assert want == min(384, N * ((OW + 31) // 32) * ((OH + 3) // 4)) * 64 * 147 * 4
    xd, gyd, xcd = x.to(DEV), to_nhwc(gy, dtype), to_nhwc(xc, dtype)

    def run(apply, nbytes):
        slab = guarded_workspace(nbytes, DEV)
        dw = guarded((64, 3, 7, 7), F32, DEV, body="keep")
        dw.copy_(base)
        extra = (xcd, cA.to(DEV), cB.to(DEV), cD.to(DEV)) if apply else ()
        ops.stem_wgrad(xd, gyd, *extra, deterministic=True, slab=slab, out=dw)
        torch.cuda.synchronize()
        assert_guards(slab, "slab")
        assert_guards(dw, "dw")
        if nbytes % (64 * 147 * 4) == 0:
            assert unwritten(slab.view(torch.float32))[0] == 0                     # every fp32 element of every tile of the grid is written
        return dw.cpu()

    a, a2 = run(False, want), run(False, want)
    b, b2 = run(True, want), run(True, want)
    c, c2 = run(False, 3 * 64 * 147 * 4 + 8), run(False, 3 * 64 * 147 * 4 + 8)
    d, d2, dc = err(a - base, w.grad), err(b - base, w2.grad), err(c - base, w.grad)
    report(f"stem_wgrad_det[{dtype},{shape}]", rel=d[2], applied_rel=d2[2], capped_rel=dc[2])
    print(f"stem_wgrad_det[{dtype},{shape}] rel {d[2]:.3e} applied {d2[2]:.3e} capped {dc[2]:.3e}")
    assert torch.equal(a, a2) and torch.equal(b, b2) and torch.equal(c, c2)
    assert d[2] < 2e-4 and d2[2] < 2e-3 and dc[2] < 2e-4


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("name,dtype,tile", [("below_one_stage", BF16, 0), ("below_one_stage", F32, 0), ("3x3_stride1", BF16, 0), ("3x3_stride2", BF16, 128)])
def test_no_slab_or_less_than_one_slice_is_refused_with_nothing_enqueued(name, dtype, tile):
    from tinyfaces import ops
    N, H, W, Cin, Cout, K, s = CASES[name][:7]
    xd, gyd = _problem(name, dtype)[:2]
    want = ops.wgrad_det_workspace_bytes(xd, gyd, Cin, Cout, K, K, s, K // 2, tile=tile, splitk=1)       # exactly one slice
    dw = guarded((Cout, Cin, K, K), F32, DEV)
    with pytest.raises(RuntimeError, match="TF_ERR_ARG"):
        ops.conv2d_wgrad(xd, gyd, Cin, Cout, K, K, s, K // 2, tile=tile, out=dw, deterministic=True, ws_bytes=0)
    slab = guarded_workspace(want - 16, DEV)
    with pytest.raises(RuntimeError, match="TF_ERR_ARG"):
        ops.conv2d_wgrad(xd, gyd, Cin, Cout, K, K, s, K // 2, tile=tile, out=dw, deterministic=True, slab=slab)
    torch.cuda.synchronize()
    assert_guards(dw, "refused: dw")
    assert_guards(slab, "refused: slab")
    assert unwritten(dw)[0] == dw.numel() and unwritten(slab)[0] == slab.numel()
    # ... and the stem
    x = torch.randn(1, 3, 37, 45, device=DEV)
    g = torch.randn(1, 19, 23, 64, device=DEV).to(BF16)
    sdw = guarded((64, 3, 7, 7), F32, DEV)
    with pytest.raises(RuntimeError, match="TF_ERR_ARG"):
        ops.stem_wgrad(x, g, deterministic=True, ws_bytes=0, out=sdw)
    sslab = guarded_workspace(64 * 147 * 4 - 16, DEV)
    with pytest.raises(RuntimeError, match="TF_ERR_ARG"):
        ops.stem_wgrad(x, g, deterministic=True, slab=sslab, out=sdw)
    torch.cuda.synchronize()
    assert unwritten(sdw)[0] == sdw.numel() and unwritten(sslab)[0] == sslab.numel()
