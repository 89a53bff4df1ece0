"""-m gpu: gradient-norm clipping and the non-finite-step guard (csrc/sgd.hip: grad_sqnorm_kernel, grad_norm_finalize_kernel, the clipped
forms of the two SGD kernels, scale_segments_kernel; ops.grad_clip_coef / clip_grad_norm_; TrainEngine(max_grad_norm=, skip_nonfinite=)).

Where the bars come from:
  sumsq   every square of an fp32 value is exact in fp64, so the kernel's only error is that of summing n non-negative doubles in SOME order:
          relative error <= n * 2^-53 for any order (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  The reference is the
          exactly rounded sum (math.fsum) of the same squares, not another floating-point order.
  norm    sqrt halves a relative error and rounds once: n * 2^-54 + 2^-53.
  coef    fp64 arithmetic on that norm, stored as fp32: one fp32 ulp around the float64 formula.
  updates the clipped SGD kernels against the EXISTING kernels called with the host-side product float32(grad_scale) * float32(coef): bit for bit.
  engine against trainer after one step: 2e-3 (tests/test_gpu_trainable_layers.py); two ranks against one process, first step: 1e-5 (same file).
Measured values go through gpu_util.report."""
import io
import math
import os
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from gpu_util import err, report
from redzone import assert_guards, guarded, guarded_like, guarded_workspace

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
N = 40000
# the five range tables of test_sgd_step_segments_equals_a_torch_reference_on_every_path (tests/test_gpu_frozen_bn.py)
TABLES = {
    "aligned": [(0, 64), (128, 4096), (8192, 8196), (20000, 39996)],
    "unaligned_empty_single": [(3, 10), (10, 10), (17, 18), (101, 4099), (9001, 9002), (20001, 39999)],
    "300_aligned": [(100 * i, 100 * i + 4 * (1 + i % 20)) for i in range(300)],               # three launches, 16-byte path
    "300_unaligned": [(100 * i + 1, 100 * i + 3 + i % 50) for i in range(300)],               # three launches, scalar path
    "whole": [(0, N)],
}
# more than one block and a ragged tail; and, since the capped grid (2048 blocks x 256 threads x 4 elements) takes 2^21 elements per trip,
# a buffer beyond that for the grid-stride loop itself, on the 16-byte and on the scalar path
BIG = (1 << 20) + 3
STRIDE = 3 * (1 << 20) + 3
LARGE = {
    "big_whole": (BIG, [(0, BIG)]),
    "big_aligned": (BIG, [(0, 1 << 19), ((1 << 19) + 64, 1 << 20)]),
    "stride_aligned": (STRIDE, [(0, STRIDE - 3)]),
    "stride_scalar": (STRIDE, [(1, STRIDE)]),
}
CASES = [(name, N, segs) for name, segs in TABLES.items()] + [(name, n, segs) for name, (n, segs) in LARGE.items()]

_DATA = {}


def _data(n):
    """One host gradient per size (values of order 1 with a few large and a few tiny ones), computed once and left unchanged."""
    if n not in _DATA:
        g = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000)).numpy().copy()
        g[::97] *= 1e3
        g[5::89] *= 1e-6
        _DATA[n] = g
    return _DATA[n]


def _mask(n, segs):
    mk = np.zeros(n, dtype=bool)
    for a, b in segs:
        mk[a:b] = True
    return mk


_REF = {}


def _reference(name, n, segs):
    """(exactly rounded sum of squares, its square root, element count) over the ranges, float64 on the host; shared between the tests."""
    if name not in _REF:
        x = _data(n)[_mask(n, segs)].astype(np.float64)
        sumsq = math.fsum((x * x).tolist())                      # the squares are exact; fsum rounds their true sum once
        _REF[name] = (sumsq, math.sqrt(sumsq), int(x.size))
    return _REF[name]


def _device_grad(n, segs, outside=float("nan")):
    """The gradient on the device with everything OUTSIDE the ranges replaced (NaN: a stray read cannot hide in a sum)."""
    g = _data(n).copy()
    g[~_mask(n, segs)] = outside
    return torch.from_numpy(g).cuda()


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def _coef64(max_norm, norm):
    """torch's definition in float64: min(1, max_norm / (norm + 1e-6)) with max_norm the fp32 value the entry point receives."""
    return min(1.0, float(np.float32(max_norm)) / (norm + 1e-6))


@pytest.mark.parametrize("name,n,segs", CASES, ids=[c[0] for c in CASES])
def test_norm_matches_float64_within_the_summation_bound_and_repeats_bit_for_bit(name, n, segs):
    from tinyfaces import ops
    sumsq, norm, count = _reference(name, n, segs)
    g = _device_grad(n, segs)
    keep = g.clone()
    runs = []
    for _ in range(2):
        st = ops.grad_clip_coef(g, segs, ops.ClipState("cuda"), grad_scale=1.0, max_norm=None).read()
        runs.append((st.sumsq, st.norm, st.coef, st.skip, st.skipped))
    torch.cuda.synchronize()
    assert runs[0] == runs[1], runs                                            # deterministic: no atomics, a fixed order
    got_sumsq, got_norm, coef, skip, skipped = runs[0]
    e_sumsq, e_norm = abs(got_sumsq - sumsq) / sumsq, abs(got_norm - norm) / norm
    report(f"grad_norm[{name}]", elements=count, ranges=len(segs), sumsq_rel=e_sumsq, sumsq_bound=count * U, norm_rel=e_norm, norm_bound=count * U / 2 + U)
    print(name, count, e_sumsq, count * U, e_norm)
    assert math.isfinite(got_sumsq) and math.isfinite(got_norm)               # nothing outside the ranges (all NaN) was read
    assert e_sumsq <= count * U, (e_sumsq, count * U)
    assert e_norm <= count * U / 2 + U, (e_norm, count * U / 2 + U)
    assert (coef, skip, skipped) == (1.0, 0, 0)                                # max_norm None: no clipping
    assert torch.equal(g.view(torch.int32), keep.view(torch.int32))           # the gradient is read only
    # grad_scale enters the norm as |grad_scale|, not the sum
    st = ops.grad_clip_coef(g, segs, ops.ClipState("cuda"), grad_scale=-0.5, max_norm=None).read()
    assert st.sumsq == got_sumsq and abs(st.norm - 0.5 * norm) / norm <= count * U / 2 + 2 * U


def test_empty_table_is_norm_zero_coef_one():
    from tinyfaces import ops
    g = torch.full((64,), float("nan")).cuda()
    for segs in ([], [(5, 5), (9, 9)]):
        st = ops.grad_clip_coef(g, segs, ops.ClipState("cuda"), max_norm=0.5, skip_nonfinite=True).read()
        assert (st.sumsq, st.norm, st.coef, st.skip, st.skipped) == (0.0, 0.0, 1.0, 0, 0), segs


@pytest.mark.parametrize("name", ["aligned", "300_unaligned", "big_whole"])
def test_coefficient_is_torchs_formula_within_one_ulp_and_tracks_torch_itself(name):
    from tinyfaces import _hip, ops
    n, segs = (N, TABLES[name]) if name in TABLES else LARGE[name]
    sumsq, norm, count = _reference(name, n, segs)
    g = _device_grad(n, segs)
    state = ops.ClipState("cuda")
    # below, at (the fp32 neighbours of the norm on either side) and above the norm; no clipping for None, 0, negative and +inf
    at = np.float32(norm)
    for c in (0.25 * norm, float(np.nextafter(at, np.float32(0))), float(at), float(np.nextafter(at, np.float32(np.inf))), 4.0 * norm):
        c = float(np.float32(c))
        st = ops.grad_clip_coef(g, segs, state, max_norm=c).read()
        want = np.float32(_coef64(c, norm))
        report(f"clip_coef[{name}]", max_norm=c, coef=st.coef, want=float(want), ulps=abs(st.coef - float(want)) / _ulp32(want))
        assert abs(st.coef - float(want)) <= _ulp32(want), (c, st.coef, want)
        assert st.coef <= 1.0 and st.skip == 0
    assert ops.grad_clip_coef(g, segs, state, max_norm=0.25 * norm).read().coef < 0.2500001
    assert ops.grad_clip_coef(g, segs, state, max_norm=4.0 * norm).read().coef == 1.0
    table = (_hip.i64 * (2 * len(segs)))(*[v for se in segs for v in se])
    ws = torch.empty(_hip.lib().tf_grad_norm_workspace_bytes(len(segs)), dtype=torch.uint8, device="cuda")
    for raw in (0.0, -1.0, float("inf"), float("nan")):
        _hip.check(_hip.lib().tf_grad_clip_coef(g.data_ptr(), table, len(segs), 1.0, raw, 0, ws.data_ptr(), ws.numel(), state.buf.data_ptr(),
                                                torch.cuda.current_stream().cuda_stream), "tf_grad_clip_coef")
        assert state.read().coef == 1.0, raw
    # torch.nn.utils.clip_grad_norm_ on CPU copies of the same ranges (fp32 norms of norms): the device value may differ from torch's by no
    # more than torch's own distance from float64 plus the device's bound (triangle inequality), for the norm and for the coefficient
    c = float(np.float32(0.25 * norm))
    host = _data(n)
    params = []
    for a, b in segs:
        if b > a:
            p = torch.nn.Parameter(torch.zeros(b - a))
            p.grad = torch.from_numpy(host[a:b].copy())
            params.append(p)
    t_norm = float(torch.nn.utils.clip_grad_norm_(params, c, foreach=False))
    t_coef = float(torch.clamp(torch.tensor(c, dtype=torch.float32) / (torch.tensor(t_norm, dtype=torch.float32) + 1e-6), max=1.0))
    st = ops.grad_clip_coef(g, segs, state, max_norm=c).read()
    bound = count * U / 2 + U
    d_norm, torch_norm = abs(st.norm - t_norm), abs(t_norm - norm)
    d_coef, torch_coef = abs(st.coef - t_coef), abs(t_coef - _coef64(c, norm))
    report(f"clip_vs_torch[{name}]", norm_dev_vs_torch=d_norm, norm_torch_vs_f64=torch_norm, coef_dev_vs_torch=d_coef, coef_torch_vs_f64=torch_coef)
    assert d_norm <= torch_norm + bound * norm
    assert d_coef <= torch_coef + bound * _coef64(c, norm) + _ulp32(t_coef)      # (+ the one fp32 rounding of the stored coefficient)
    # ... and the scaled gradients are torch's, element for element, up to that coefficient difference and one fp32 rounding
    ops.scale_segments(g, segs, state)
    torch.cuda.synchronize()
    o = 0
    got = g.cpu()
    for a, b in segs:
        if b > a:
            ref = params[o].grad
            o += 1
            raw = torch.from_numpy(host[a:b]).abs()                           # (torch scaled its copies in place: `ref` is already clipped)
            tol = raw * (d_coef + 2.0 ** -24 * (st.coef + t_coef))
            assert bool(((got[a:b] - ref).abs() <= tol).all()), (name, a, b)


def _clipped_state(g, segs, gs, frac=0.3):
    """A state whose coefficient is < 1: max_norm = frac x the scaled norm of g over segs (neither frac nor the scales the tests use are
    powers of two: a product taken in another order or precision would round differently)."""
    from tinyfaces import ops
    state = ops.ClipState("cuda")
    norm = ops.grad_clip_coef(g, segs, state, grad_scale=gs, max_norm=None).norm()
    coef = ops.grad_clip_coef(g, segs, state, grad_scale=gs, max_norm=float(np.float32(frac * norm))).coef()
    assert 0.0 < coef < 1.0
    return state, coef


def _skip_state(n=64):
    from tinyfaces import ops
    bad = torch.ones(n).cuda()
    bad[n // 2] = float("nan")
    state = ops.ClipState("cuda")
    st = ops.grad_clip_coef(bad, [(0, n)], state, max_norm=1.0, skip_nonfinite=True).read()
    assert (st.skip, st.coef, st.skipped) == (1, 0.0, 1) and math.isnan(st.norm)
    return state


@pytest.mark.parametrize("offset", [0, 1], ids=["float4", "scalar"])
def test_clipped_sgd_step_equals_the_plain_step_at_the_product_scale(offset):
    """tf_sgd_step_clipped against tf_sgd_step with grad_scale = float32(gs) * float32(coef), two steps (momentum), on the 16-byte path and
    (buffers one element off a 16-byte boundary) on the scalar path; with skip set nothing moves."""
    from tinyfaces import ops
    lr, mu, wd, gs = 0.05, 0.9, 5e-4, 0.37
    gen = torch.Generator().manual_seed(1)
    n = N + 3
    base = [torch.randn(n + 4, generator=gen).cuda() for _ in range(3)]
    p, g, m = [t[offset:offset + n] for t in base]
    m.zero_()
    state, coef = _clipped_state(g.clone(), [(0, n)], gs)
    prod = float(np.float32(gs) * np.float32(coef))
    p_start = p.clone()
    rp, rm = p.clone(), m.clone()
    if offset:
        rp, rm = [torch.cat([t.new_zeros(offset), t])[offset:] for t in (rp, rm)]       # the reference takes the same (scalar) path
    for step in range(2):
        ops.sgd_step(p, g, m, lr, mu, wd, gs, clip_state=state)
        ops.sgd_step(rp, g, rm, lr, mu, wd, prod)
        torch.cuda.synchronize()
        assert torch.equal(p, rp) and torch.equal(m, rm), step
    assert not torch.equal(p, p_start) and float(m.abs().max()) > 0.0
    skip = _skip_state()
    p0, m0 = p.clone(), m.clone()
    ops.sgd_step(p, g, m, lr, mu, wd, gs, clip_state=skip)
    torch.cuda.synchronize()
    assert torch.equal(p.view(torch.int32), p0.view(torch.int32)) and torch.equal(m.view(torch.int32), m0.view(torch.int32))
    assert skip.skipped() == 1                                               # the SGD forms only read the state
    report(f"sgd_clipped[{'scalar' if offset else 'float4'}]", coef=coef, product_scale=prod)


@pytest.mark.parametrize("name", list(TABLES))
def test_clipped_segment_step_equals_the_plain_segment_step_at_the_product_scale(name):
    from tinyfaces import ops
    segs = TABLES[name]
    lr, mu, wd, gs = 0.05, 0.9, 5e-4, 0.37
    gen = torch.Generator().manual_seed(2)
    p = torch.randn(N, generator=gen).cuda()
    g = _device_grad(N, segs, outside=0.0)
    m = torch.zeros(N).cuda()
    state, coef = _clipped_state(g, segs, gs)
    prod = float(np.float32(gs) * np.float32(coef))
    rp, rm = p.clone(), m.clone()
    p_start = p.clone()
    for step in range(2):
        ops.sgd_step_segments(p, g, m, segs, lr, mu, wd, gs, clip_state=state)
        ops.sgd_step_segments(rp, g, rm, segs, lr, mu, wd, prod)
        torch.cuda.synchronize()
        assert torch.equal(p, rp) and torch.equal(m, rm), (name, step)
    mk = torch.from_numpy(_mask(N, segs)).cuda()
    assert torch.equal(p[~mk], p_start[~mk]) and float(m[~mk].abs().sum()) == 0.0 and not torch.equal(p[mk], p_start[mk])
    skip = _skip_state()
    p0, m0 = p.clone(), m.clone()
    ops.sgd_step_segments(p, g, m, segs, lr, mu, wd, gs, clip_state=skip)
    ops.grad_clip_coef(torch.full((8,), float("inf")).cuda(), [(0, 8)], skip, max_norm=1.0, skip_nonfinite=True)      # a second skipped step
    ops.sgd_step_segments(p, g, m, segs, lr, mu, wd, gs, clip_state=skip)
    torch.cuda.synchronize()
    assert torch.equal(p.view(torch.int32), p0.view(torch.int32)) and torch.equal(m.view(torch.int32), m0.view(torch.int32))
    assert skip.skipped() == 2 and skip.skip() == 1
    ops.grad_clip_coef(torch.ones(8).cuda(), [(0, 8)], skip, max_norm=1.0, skip_nonfinite=True)                        # a clean one: trains again
    assert (skip.skip(), skip.skipped()) == (0, 2)
    ops.sgd_step_segments(p, g, m, segs, lr, mu, wd, gs, clip_state=skip)
    torch.cuda.synchronize()
    assert not torch.equal(p, p0)


@pytest.mark.parametrize("name", list(TABLES))
def test_scale_segments_is_an_exact_product_inside_and_touches_nothing_outside(name):
    from tinyfaces import ops
    segs = TABLES[name]
    g = _device_grad(N, segs)                                                  # NaN outside: compared as bit patterns
    g0 = g.clone()
    state, coef = _clipped_state(g, segs, 1.0)
    ops.scale_segments(g, segs, state)
    torch.cuda.synchronize()
    mk = torch.from_numpy(_mask(N, segs)).cuda()
    assert torch.equal(g[mk], g0[mk] * coef)                                   # one fp32 product per element
    assert torch.equal(g[~mk].view(torch.int32), g0[~mk].view(torch.int32))
    # a skipped step: the gradient an optimizer sees is zero (NaN * 0 would stay NaN), the outside still untouched
    g1 = g.clone()
    g1[segs[0][0]] = float("nan")
    ops.scale_segments(g1, segs, _skip_state())
    torch.cuda.synchronize()
    assert float(g1[mk].abs().max()) == 0.0
    assert torch.equal(g1[~mk].view(torch.int32), g0[~mk].view(torch.int32))


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")], ids=["nan", "inf", "-inf"])
@pytest.mark.parametrize("name", ["aligned", "300_unaligned"])
def test_one_nonfinite_element_flips_skip_with_the_flag_and_gives_torchs_coefficient_without(name, bad):
    from tinyfaces import ops
    segs = TABLES[name]
    a, b = segs[len(segs) // 2]
    g = _device_grad(N, segs)
    g[b - 1] = bad                                                             # the last element of a range in the middle of the table
    state = ops.ClipState("cuda")
    st = ops.grad_clip_coef(g, segs, state, max_norm=1.0, skip_nonfinite=True).read()
    assert (st.skip, st.coef, st.skipped) == (1, 0.0, 1) and not math.isfinite(st.norm)
    st = ops.grad_clip_coef(g, segs, state, max_norm=None, skip_nonfinite=True).read()          # the guard alone
    assert (st.skip, st.coef, st.skipped) == (1, 0.0, 2)
    st = ops.grad_clip_coef(g, segs, state, max_norm=1.0).read()               # error_if_nonfinite=False: whatever the formula yields
    t_norm = torch.tensor(float("nan") if math.isnan(bad) else float("inf"), dtype=torch.float32)
    t_coef = float(torch.clamp(torch.tensor(1.0) / (t_norm + 1e-6), max=1.0))
    assert st.skip == 0 and st.skipped == 2
    assert (math.isnan(st.coef) and math.isnan(t_coef)) or st.coef == t_coef == 0.0, (st.coef, t_coef)
    g[b - 1] = 1.0
    st = ops.grad_clip_coef(g, segs, state, max_norm=1.0, skip_nonfinite=True).read()
    assert st.skip == 0 and 0.0 < st.coef < 1.0 and st.skipped == 2 and math.isfinite(st.norm)
    # the same element just OUTSIDE a range is never read
    g[b] = bad if _mask(N, segs)[b] == 0 else g[b]
    assert ops.grad_clip_coef(g, segs, state, max_norm=1.0, skip_nonfinite=True).read().skip == 0


@pytest.mark.parametrize("name", ["unaligned_empty_single", "300_aligned", "300_unaligned", "whole"])
def test_every_entry_point_writes_inside_its_operands_only(hip, name):
    """tests/redzone.py: the gradient, a workspace of EXACTLY tf_grad_norm_workspace_bytes bytes, the 32-byte state and the two
    SGD operands between 0xFF guard bands; every guard intact after each of the five entries."""
    l = hip.lib()
    segs = [se for se in TABLES[name]]
    nseg = len(segs)
    table = (hip.i64 * (2 * nseg))(*[v for se in segs for v in se])
    host = torch.from_numpy(_data(N).copy())
    g = guarded_like(host, "cuda")
    p = guarded_like(torch.randn(N, generator=torch.Generator().manual_seed(4)), "cuda")
    m = guarded_like(torch.zeros(N), "cuda")
    need = l.tf_grad_norm_workspace_bytes(nseg)
    assert need == 8 * 2048 * -(-nseg // 128)
    ws = guarded_workspace(need, "cuda")
    state = guarded((32,), torch.uint8, "cuda", body="keep")
    state.zero_()
    s = torch.cuda.current_stream().cuda_stream
    sumsq, norm, _ = _reference(name, N, segs)

    def everything(what):
        torch.cuda.synchronize()
        for t, label in ((g, "gradient"), (p, "parameters"), (m, "momentum"), (ws, f"workspace of exactly {need} bytes"), (state, "state")):
            assert_guards(t, f"{what}: {label}")

    assert l.tf_grad_clip_coef(g.data_ptr(), table, nseg, 1.0, float(np.float32(0.25 * norm)), 1, ws.data_ptr(), need, state.data_ptr(), s) == 0
    everything("tf_grad_clip_coef")
    st = hip.ClipState.from_buffer_copy(state.cpu().numpy().tobytes())
    assert abs(st.norm - norm) <= norm * (N * U) and 0.0 < st.coef < 1.0 and st.skip == 0
    assert l.tf_grad_clip_coef(g.data_ptr(), table, nseg, 1.0, 1.0, 1, ws.data_ptr(), need - 8, state.data_ptr(), s) == -1     # one double short
    assert l.tf_sgd_step_segments_clipped(p.data_ptr(), g.data_ptr(), m.data_ptr(), table, nseg, 0.05, 0.9, 5e-4, 1.0, state.data_ptr(), s) == 0
    everything("tf_sgd_step_segments_clipped")
    assert l.tf_sgd_step_clipped(p.data_ptr(), g.data_ptr(), m.data_ptr(), N, 0.05, 0.9, 5e-4, 1.0, state.data_ptr(), s) == 0
    everything("tf_sgd_step_clipped")
    assert l.tf_sgd_step_clipped(p.data_ptr() + 4, g.data_ptr() + 4, m.data_ptr() + 4, N - 1, 0.05, 0.9, 5e-4, 1.0, state.data_ptr(), s) == 0   # scalar path
    everything("tf_sgd_step_clipped, scalar path")
    assert l.tf_scale_segments(g.data_ptr(), table, nseg, state.data_ptr(), s) == 0
    everything("tf_scale_segments")
    assert l.tf_grad_clip_coef(None, None, 0, 1.0, 1.0, 1, None, 0, state.data_ptr(), s) == 0                                    # finalize only
    everything("tf_grad_clip_coef, empty table")
    st = hip.ClipState.from_buffer_copy(state.cpu().numpy().tobytes())
    assert (st.sumsq, st.norm, st.coef, st.skip, st.skipped) == (0.0, 0.0, 1.0, 0, 0)
    assert torch.isfinite(p).all() and torch.isfinite(m).all()


def test_clip_grad_norm_drop_in_on_views_and_on_separate_tensors():
    """ops.clip_grad_norm_ against torch.nn.utils.clip_grad_norm_ on CPU copies: gradients that are views of one flat buffer (with gaps that
    hold NaN) and gradients allocated one by one; returns the norm as a device scalar."""
    from tinyfaces import ops
    gen = torch.Generator().manual_seed(7)
    shapes = [(64, 3, 7, 7), (64,), (125,), (256, 64, 1, 1), (1,), (33, 5)]

    def run(make):
        params, ref = [], []
        for i, shp in enumerate(shapes):
            val = torch.randn(shp, generator=gen) * (10.0 if i == 3 else 1.0)
            p = torch.nn.Parameter(torch.zeros(shp).cuda())
            p.grad = make(val)
            params.append(p)
            r = torch.nn.Parameter(torch.zeros(shp))
            r.grad = val.clone()
            ref.append(r)
        extra = torch.nn.Parameter(torch.zeros(3).cuda())                    # a parameter without a gradient is skipped, as torch does
        n64 = math.sqrt(math.fsum((torch.cat([r.grad.flatten() for r in ref]).double() ** 2).tolist()))
        c = float(np.float32(n64 / 3))
        t_norm = float(torch.nn.utils.clip_grad_norm_(ref, c, foreach=False))
        got = ops.clip_grad_norm_(params + [extra], c)
        assert got.is_cuda and got.dim() == 0 and got.dtype == torch.float64
        count = sum(r.numel() for r in ref)
        assert abs(float(got) - n64) <= n64 * (count * U / 2 + U)
        assert abs(float(got) - t_norm) <= abs(t_norm - n64) + n64 * (count * U / 2 + U)
        coef = ops._clip_states[got.device].coef()
        assert abs(coef - float(np.float32(_coef64(c, n64)))) <= _ulp32(coef) and coef < 0.34
        worst = 0.0
        for p, r in zip(params, ref):
            d = (p.grad.cpu() - r.grad).abs()
            worst = max(worst, float((d / (r.grad.abs() + 1e-30)).max()))
        report("clip_grad_norm_drop_in", norm=float(got), torch_norm=t_norm, worst_rel=worst)
        # the two coefficients differ by the two norms' distance and by their fp32 roundings (torch: sum, quotient; here: the stored value),
        # the products by one more rounding each: six fp32 half-ulps on top of the norms' distance covers them
        assert worst <= 6 * 2.0 ** -24 + abs(t_norm - n64) / n64
        return got

    flat = torch.full((sum((math.prod(s) + 3) // 4 * 4 + 8 for s in shapes),), float("nan")).cuda()
    offs = [0]

    def view(val):
        o = offs[0]
        offs[0] += (val.numel() + 3) // 4 * 4 + 8
        flat[o:o + val.numel()] = val.flatten().cuda()
        return flat[o:o + val.numel()].view(val.shape)

    run(view)
    assert int(torch.isnan(flat).sum()) == flat.numel() - sum(math.prod(s) for s in shapes)      # the gaps still hold their NaN
    run(lambda val: val.clone().cuda())
    g = torch.nn.Parameter(torch.zeros(4).cuda())
    g.grad = torch.tensor([1.0, float("nan"), 2.0, 3.0]).cuda()
    before = ops.clip_skipped_steps("cuda:0")
    assert math.isnan(float(ops.clip_grad_norm_(g, 1.0, skip_nonfinite=True)))
    assert float(g.grad.abs().max()) == 0.0 and ops.clip_skipped_steps("cuda:0") == before + 1


# ---------------------------------------------------------------------------------------------------------------- engine level
def _engine_inputs():
    g = torch.Generator().manual_seed(3)                                       # the batch of test_engine_leaves_the_frozen_stages_alone...
    x = torch.randn(2, 3, 256, 256, generator=g).cuda()
    cm = torch.where(torch.rand(2, 25, 32, 32, generator=g) < 0.02, 1.0, -1.0).cuda()
    rm = torch.randn(2, 100, 32, 32, generator=g).cuda()
    return x, cm, rm


def _host_norm(gflat, ranges):
    """float64 L2 norm of the flat gradient over `ranges`, on the host: exact squares, exactly rounded sum, one square root."""
    g = gflat.detach().cpu().numpy()
    x = np.concatenate([g[a:b] for a, b in ranges]).astype(np.float64)
    return math.sqrt(math.fsum((x * x).tolist()))


@pytest.mark.parametrize("frozen", [False, True], ids=["batch_stats", "frozen_bn_k2"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_engine_clips_on_the_device_and_skips_a_step_with_a_nan(dtype, frozen):
    """ResNet-50, 2 x 3 x 256 x 256.  A plain step gives the norm N0; at max_grad_norm = N0 / 4 the next step's coefficient is < 1, is the float64
    formula on the gradient that step left in the persistent flat buffer, and the parameters and momentum are bit for bit what the EXISTING SGD
    ops give on (p0, m0, that gradient) at the product scale; frozen slices and BN vectors do not move.  Then the guard: one NaN planted into
    a trained slice behind the real backward pass leaves parameters and momentum bit-identical and counts one skipped step; the next clean
    step trains again and stays finite."""
    from test_gpu_frozen_bn import _bn_snapshot, _oracle, _product
    from tinyfaces import ops
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.loss import DetectionCriterion
    m = _product(_oracle("resnet50", seed=6), "resnet50").set_compute_dtype(dtype)
    if frozen:
        m.freeze_batchnorm().set_trainable_layers(2)
    lr, mu, wd = 1e-3, 0.9, 5e-4
    eng = TrainEngine(m, DetectionCriterion(25), lr=lr, momentum=mu, weight_decay=wd, device="cuda")
    x, cm, rm = _engine_inputs()
    seg, gflat = m._segments, m._grad_flat_persistent
    trained_names = set(m.trainable_parameter_names())
    trained = sorted((seg[n][0], seg[n][0] + seg[n][1]) for n in trained_names)
    count = sum(b - a for a, b in trained)
    tag = f"engine_clip[{'bf16' if dtype == torch.bfloat16 else 'fp32'},{'frozen_k2' if frozen else 'batch_stats'}]"

    eng.step(x, cm.clone(), rm)                                               # plain: nothing of the feature runs
    torch.cuda.synchronize()
    assert eng._clip_state is None and eng.last_grad_norm is None
    n0 = _host_norm(gflat, trained)
    assert math.isfinite(n0) and n0 > 0.0
    c = float(np.float32(n0 / 4))
    eng.set_max_grad_norm(c)
    p0, m0 = eng.flat_p.clone(), eng.flat_m.clone()
    bn0 = _bn_snapshot(m) if frozen else None
    eng.step(x, cm.clone(), rm)
    norm_dev = eng.last_grad_norm
    assert norm_dev.is_cuda and norm_dev.dim() == 0
    torch.cuda.synchronize()
    st = eng._clip_state.read()
    n1 = _host_norm(gflat, trained)                                           # the gradient this step left behind
    want = np.float32(_coef64(c, n1))
    report(tag, n0=n0, n1=n1, norm_dev=st.norm, norm_rel=abs(st.norm - n1) / n1, norm_bound=count * U / 2 + U, coef=st.coef, coef_want=float(want),
           trained_elements=count, ranges=len(eng._norm_segments()))
    print(tag, n0, n1, st.norm, st.coef, float(want))
    assert st.coef < 1.0 and st.skip == 0 and eng.skipped_steps == 0          # not vacuous: the step WAS clipped
    assert abs(st.norm - n1) <= n1 * (count * U / 2 + U) and float(norm_dev) == st.norm
    assert abs(st.coef - float(want)) <= _ulp32(want)
    assert eng.last_clip_coef == st.coef
    prod = float(np.float32(1.0) * np.float32(st.coef))
    rp, rmom = p0.clone(), m0.clone()
    for a, b, mult in eng.groups:
        if mult == 0.0:
            continue
        if frozen:
            ops.sgd_step_segments(rp, gflat, rmom, [(max(s, a), min(e, b)) for s, e in trained if e > a and s < b], lr * mult, mu, wd, prod)
        else:
            ops.sgd_step(rp[a:b], gflat[a:b], rmom[a:b], lr * mult, mu, wd, prod)
    torch.cuda.synchronize()
    assert torch.equal(eng.flat_p, rp) and torch.equal(eng.flat_m, rmom)
    moved = 0
    for n, (o, num) in seg.items():
        if n in trained_names:
            moved += not torch.equal(eng.flat_p[o:o + num], p0[o:o + num])
        else:                                                                 # frozen stages, BN vectors (frozen) and the lr-0 upsample weight
            assert torch.equal(eng.flat_p[o:o + num], p0[o:o + num]) and torch.equal(eng.flat_m[o:o + num], m0[o:o + num]), n
    assert moved == len(trained_names)
    if frozen:
        bn1 = _bn_snapshot(m)
        assert all(torch.equal(bn0[k], bn1[k]) for k in bn0)

    # ---- the guard
    eng.skip_nonfinite = True
    victim = seg["model.layer3.1.conv2.weight"][0] + 5
    run_backward, plant = m._run_backward, [True]

    def planted(xx, grad, persistent=False):
        out = run_backward(xx, grad, persistent=persistent)
        if plant[0]:
            out[victim] = float("nan")                                        # behind the real backward pass, on the training stream
        return out

    m._run_backward = planted
    try:
        p1, m1 = eng.flat_p.clone(), eng.flat_m.clone()
        eng.step(x, cm.clone(), rm)
        torch.cuda.synchronize()
        assert torch.equal(eng.flat_p.view(torch.int32), p1.view(torch.int32)) and torch.equal(eng.flat_m.view(torch.int32), m1.view(torch.int32))
        st = eng._clip_state.read()
        assert eng.skipped_steps == 1 and st.skip == 1 and st.coef == 0.0 and math.isnan(st.norm) and math.isnan(float(eng.last_grad_norm))
        plant[0] = False
        eng.step(x, cm.clone(), rm)
        torch.cuda.synchronize()
    finally:
        m._run_backward = run_backward
    st = eng._clip_state.read()
    assert eng.skipped_steps == 1 and st.skip == 0 and 0.0 < st.coef <= 1.0 and math.isfinite(st.norm)
    assert not torch.equal(eng.flat_p, p1) and not torch.equal(eng.flat_m, m1)
    assert torch.isfinite(eng.flat_p).all() and torch.isfinite(eng.flat_m).all()
    eng.close()


def test_trainer_clips_like_torch_clip_grad_norm(golden):
    """fp32, ResNet-50, the first batch of tests/golden/trainer.npz, deterministic sampling: trainer.train(..., max_grad_norm=c) against the same
    step done by hand with torch.nn.utils.clip_grad_norm_ on copies of the .grads -- the one-step bar of the engine-vs-trainer tests, 2e-3."""
    from test_gpu_frozen_bn import _golden_batches, _keep, _oracle, _product
    from tinyfaces import ops, trainer
    from tinyfaces.models.loss import DetectionCriterion
    batch = _golden_batches(golden)[0]
    om = _oracle("resnet50", seed=9)
    dev = torch.device("cuda")

    def fresh():
        m = _product(om, "resnet50").set_compute_dtype(torch.float32).to(dev).train()
        c = DetectionCriterion(25)
        c.inject_sampling(_keep(), _keep())
        return m, c, torch.optim.SGD(m.learnable_parameters(1e-3), lr=1e-3, momentum=0.9, weight_decay=5e-4)

    # by hand
    m1, c1, opt1 = fresh()
    img, cmap, rmap = (t.float().to(dev) for t in batch)
    loss = c1(m1(img), cmap, rmap)
    opt1.zero_grad()
    loss.backward()
    with_grad = [p for p in m1.parameters() if p.grad is not None]
    for p in with_grad:
        p.grad = p.grad.clone()                                               # copies: separately allocated tensors
    n_hand = float(torch.nn.utils.clip_grad_norm_(with_grad, float("inf")))
    c = float(np.float32(n_hand / 4))
    assert math.isfinite(n_hand) and float(torch.nn.utils.clip_grad_norm_(with_grad, c)) == n_hand
    opt1.step()
    # the product
    m2, c2, opt2 = fresh()
    with redirect_stdout(io.StringIO()):
        trainer.train(m2, c2, opt2, [batch], 0, dev, max_grad_norm=c)
    torch.cuda.synchronize()
    st = ops._clip_states[torch.device("cuda", torch.cuda.current_device())].read()
    assert 0.2 < st.coef < 0.3 and st.skip == 0                               # it did clip, to a quarter
    s0, s1, s2 = om.state_dict(), m1.state_dict(), m2.state_dict()
    worst, wname, moved = 0.0, "", 0
    for n in s1:
        d = err(s2[n].cpu().numpy(), s1[n].cpu().numpy())[2]
        if d > worst:
            worst, wname = d, n
        moved += not torch.equal(s2[n].cpu(), s0[n])
    report("trainer_clip[resnet50,fp32]", norm_hand=n_hand, norm_dev=st.norm, coef=st.coef, worst_rel=worst, worst_tensor=wname)
    print("trainer_clip", n_hand, st.norm, st.coef, worst, wname)
    assert abs(st.norm - n_hand) <= 2e-3 * n_hand and moved > 100
    assert worst < 2e-3, (worst, wname)


def test_two_ranks_agree_on_norm_and_coefficient_and_skip_together(tmp_path):
    """2 gloo ranks sharing cuda:0 (tests/dist_worker_clip.py) against ONE process that sums the gradients of the same two micro-batches, takes
    the norm of their average and clips: same norm and coefficient on both ranks, parameters within the suite's first-step bar (1e-5); with a
    NaN planted on rank 1 alone both ranks skip the same step, and both train again afterwards."""
    from tinyfaces import ops
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dist_worker_clip
    golden = os.path.join(ROOT, "tests", "golden", "trainer.npz")
    # the single process first: it also decides the clip value (a quarter of the averaged gradient's norm)
    reps = []
    for r_ in range(2):
        m, c, batches = dist_worker_clip.build(golden)
        m = m.cuda().train()
        flat = m.flatten_parameters()
        reps.append(dict(m=m, c=c, flat=flat, batch=[t.cuda() for t in batches[r_]]))
    m0 = reps[0]["m"]
    seg, names, groups = m0._segments, m0.trainable_parameter_names(), m0.group_ranges()
    trained = sorted((seg[n][0], seg[n][0] + seg[n][1]) for n in names)
    grads = []
    for rp in reps:
        m, c = rp["m"], rp["c"]
        img, cm, rm = rp["batch"]
        m._sync_tables(img.device)
        o = m._run_forward(img, training=True)
        _, g, _ = ops.criterion_fwd_bwd(o, cm.clone(), rm, c.n_templates, c.reg_weight, c.ohem_thresh, c.max_pos, c.max_neg, c._pos_keep, c._neg_keep,
                                        c._next_seed())
        grads.append(m._run_backward(img, g, persistent=True).clone())
    gsum = grads[0] + grads[1]
    n_avg = 0.5 * _host_norm(gsum, trained)
    max_norm = float(np.float32(n_avg / 4))
    state = ops.grad_clip_coef(gsum, trained, ops.ClipState("cuda"), grad_scale=0.5, max_norm=max_norm)
    ref_p, ref_m = reps[0]["flat"].clone(), torch.zeros_like(reps[0]["flat"])
    first = ref_p.cpu().numpy().copy()
    for a, b, mult in groups:
        if mult != 0.0:
            ops.sgd_step_segments(ref_p, gsum, ref_m, [(max(s_, a), min(e_, b)) for s_, e_ in trained if e_ > a and s_ < b], 1e-4 * mult, 0.9, 5e-4, 0.5,
                                  clip_state=state)
    torch.cuda.synchronize()
    ref_state = state.read()
    assert 0.2 < ref_state.coef < 0.3
    ref = ref_p.cpu().numpy()

    out = str(tmp_path / "clip")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29581", os.path.join(ROOT, "tests", "dist_worker_clip.py"), golden, out, repr(max_norm)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = [np.load(f"{out}.rank{k}.npz") for k in range(2)]
    # step 0: clipped, the same on both ranks, and the single process's
    for key in ("state0", "norm0", "p0", "m0"):
        assert np.array_equal(got[0][key], got[1][key]), key
    sumsq, norm, coef, skip, skipped = got[0]["state0"]
    worst = float(np.abs(got[0]["p0"] - ref).max() / (np.abs(ref).max() + 1e-30))
    report("clip_dist_2_ranks_vs_single[resnet50,k=1]", norm=norm, ref_norm=ref_state.norm, coef=coef, ref_coef=ref_state.coef, worst_rel=worst)
    print("clip_dist", norm, ref_state.norm, coef, ref_state.coef, worst)
    assert (skip, skipped) == (0, 0) and coef < 1.0 and float(got[0]["norm0"]) == norm
    assert abs(norm - ref_state.norm) <= 1e-5 * ref_state.norm and abs(coef - ref_state.coef) <= 1e-5 * ref_state.coef
    assert worst < 1e-5, worst
    assert float(np.abs(got[0]["p0"] - first).max()) > 0.0
    # step 1: the NaN of rank 1 reaches both ranks through the sum; neither moves
    for k in range(2):
        st = got[k]["state1"]
        assert np.isnan(st[1]) and st[2] == 0.0 and (st[3], st[4]) == (1, 1) and int(got[k]["skipped1"]) == 1, (k, st)
        assert np.array_equal(got[k]["p1"], got[k]["p0"]) and np.array_equal(got[k]["m1"], got[k]["m0"]), k
    # step 2: clean again
    for k in range(2):
        st = got[k]["state2"]
        assert np.isfinite(st[1]) and 0.0 < st[2] <= 1.0 and (st[3], st[4]) == (0, 1), (k, st)
        assert not np.array_equal(got[k]["p2"], got[k]["p1"]) and np.isfinite(got[k]["p2"]).all() and np.isfinite(got[k]["m2"]).all()
    assert np.array_equal(got[0]["p2"], got[1]["p2"])
