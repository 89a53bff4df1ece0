"""-m gpu: the AdamW optimizer (csrc/adamw.hip: adamw_advance_kernel, adamw_kernel<CLIP, EMA>, adamw_segments_kernel<CLIP, EMA>;
ops.AdamState / adamw_advance / adamw_step / adamw_step_segments; TrainEngine(optimizer="adamw"); main.py --optimizer adamw --warmup-iters).

Every comparison is bit for bit against tests/adamw_ref.py, the numpy float32 restatement of the arithmetic the header defines, which
tests/test_adamw.py holds against torch.optim.AdamW on the CPU.  The step counter and the bias corrections read back from the device are
compared with the host's pow_int values with ==.  Three successive steps with a fresh gradient each, so that both moments are non-trivial.

The backward pass sums some weight gradients with fp32 atomics and differs from run to run in the last bits; where two engines have to take
the same step (the default-optimizer test, the checkpoint test) the second one is fed the first one's gradient behind its own backward pass,
the way the guard tests plant their NaN.  Measured values go through gpu_util.report."""
import io
import math
import os
import subprocess
import sys
from contextlib import contextmanager, redirect_stdout

import numpy as np
import pytest
import torch

import adamw_ref
from gpu_util import report
from redzone import assert_guards, guarded, guarded_like

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tiny-faces-pytorch_amd")
F = np.float32
LR, BETAS, EPS, WD, GS = 1e-3, (0.9, 0.999), 1e-8, 1e-2, 0.37
HYPER = (LR, BETAS, EPS, WD)
EMA_W = float(F(1e-3))


def _i32(t):
    return t.contiguous().view(torch.int32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _same(t, a):
    """A float32 device / host tensor and a float32 numpy array hold the same bits."""
    return np.array_equal(_bits(t.detach().cpu().numpy()), _bits(a))


def _randn(n, seed, scale=True):
    x = torch.randn(n, generator=torch.Generator().manual_seed(seed)).numpy().copy()
    if scale and n > 200:
        x[::97] *= 1e3
        x[5::89] *= 1e-6
    return x


def _mask(n, segs):
    mk = np.zeros(n, dtype=bool)
    for a, b in segs:
        mk[a:b] = True
    return mk


def _state_is(state, step):
    st = state.read()
    b1, b2 = adamw_ref.bias_corrections(BETAS, step) if step else (0.0, 0.0)
    assert (st.step, st.bias1, st.bias2) == (step, b1, b2), (st.step, st.bias1, st.bias2, step, b1, b2)
    assert state.step() == step and state.bias1() == b1 and state.bias2() == b2


# ---------------------------------------------------------------------------------------------------------------- 1: the flat entry point
@pytest.mark.parametrize("offset", [0, 1], ids=["float4", "scalar"])
@pytest.mark.parametrize("n", [1, 3, 4, 1027, 40000])
def test_flat_step_is_the_restatement_bit_for_bit(n, offset):
    from tinyfaces import ops
    base = [torch.zeros(n + 8).cuda() for _ in range(4)]
    p, g, m, v = [t[offset:offset + n] for t in base]
    assert (p.data_ptr() % 16 == 0) == (offset == 0)
    hp = _randn(n, 100 + n)
    p.copy_(torch.from_numpy(hp))
    hm, hv = np.zeros(n, F), np.zeros(n, F)
    state = ops.AdamState("cuda")
    _state_is(state, 0)
    for t in range(3):
        hg = _randn(n, 200 + 7 * n + t)
        g.copy_(torch.from_numpy(hg))
        ops.adamw_advance(state, BETAS)
        ops.adamw_step(p, g, m, v, state, *HYPER, GS)
        torch.cuda.synchronize()
        hp, hm, hv = adamw_ref.adamw_step(hp, hg, hm, hv, t + 1, *HYPER, grad_scale=GS)
        assert _same(p, hp) and _same(m, hm) and _same(v, hv), (n, offset, t)
        _state_is(state, t + 1)
    for t_, inner in zip(base, (p, g, m, v)):                                   # nothing outside [0, n)
        assert float(t_[:offset].abs().sum()) == 0.0 and float(t_[offset + n:].abs().sum()) == 0.0
    assert np.isfinite(hp).all() and float(np.abs(hm).max()) > 0.0 and float(hv.max()) > 0.0
    report(f"adamw_flat[n{n},{'scalar' if offset else 'float4'}]", steps=3)


# ---------------------------------------------------------------------------------------------------------------- 2: the segment entry point
def _segment_cases():
    from test_gpu_grad_clip import LARGE, N, TABLES
    cases = [(name, N, segs, 0) for name, segs in TABLES.items()]
    cases += [(name, n, segs, 0) for name, (n, segs) in LARGE.items()]
    cases += [("base_off_by_one", N, TABLES["aligned"], 1)]
    return cases


P_OUT, M_OUT, V_OUT = 123.25, -7.5, 3.0                                          # sentinels outside the ranges


@pytest.mark.parametrize("name,n,segs,offset", _segment_cases(), ids=[c[0] for c in _segment_cases()])
def test_segment_step_is_the_restatement_inside_and_touches_nothing_outside(name, n, segs, offset):
    from tinyfaces import ops
    mk = _mask(n, segs)
    idx = np.flatnonzero(mk)
    base = [torch.zeros(n + 4).cuda() for _ in range(4)]
    p, g, m, v = [t[offset:offset + n] for t in base]
    assert (p.data_ptr() % 16 == 0) == (offset == 0)
    hp = _randn(n, 31)
    hp[~mk] = P_OUT
    hm, hv = np.full(n, M_OUT, F), np.full(n, V_OUT, F)
    hm[mk], hv[mk] = 0.0, 0.0
    for dev, host in ((p, hp), (m, hm), (v, hv)):
        dev.copy_(torch.from_numpy(host))
    out0 = [hp[~mk].copy(), hm[~mk].copy(), hv[~mk].copy()]
    state = ops.AdamState("cuda")
    for t in range(3):
        hg = _randn(n, 40 + t)
        dg = hg.copy()
        dg[~mk] = np.nan                                                        # never read: a NaN could not hide in a moment
        g.copy_(torch.from_numpy(dg))
        ops.adamw_advance(state, BETAS)
        ops.adamw_step_segments(p, g, m, v, state, segs, *HYPER, GS)
        torch.cuda.synchronize()
        rp, rm, rv = adamw_ref.adamw_step(hp[idx], hg[idx], hm[idx], hv[idx], t + 1, *HYPER, grad_scale=GS)
        hp[idx], hm[idx], hv[idx] = rp, rm, rv
        gp, gm, gv = (x.cpu().numpy() for x in (p, m, v))
        assert np.array_equal(_bits(gp[mk]), _bits(rp)) and np.array_equal(_bits(gm[mk]), _bits(rm)) and np.array_equal(_bits(gv[mk]), _bits(rv)), (name, t)
        for got, want in zip((gp, gm, gv), out0):
            assert np.array_equal(_bits(got[~mk]), _bits(want)), (name, t)
        assert np.array_equal(_bits(g.cpu().numpy()), _bits(dg))                # the gradient is read only
    for t_ in base:
        assert float(t_[:offset].abs().sum()) == 0.0 and float(t_[offset + n:].abs().sum()) == 0.0
    _state_is(state, 3)
    report(f"adamw_segments[{name}]", elements=int(mk.sum()), ranges=len(segs))


# ---------------------------------------------------------------------------------------------------------------- 3: planted elements
@pytest.mark.parametrize("offset", [0, 1], ids=["float4", "scalar"])
def test_planted_elements_follow_the_restatement(offset):
    """g = 0 with v = 0; g = +-1e25, whose square overflows fp32; g = +-1e-30, whose square underflows; subnormal g; g = +-1e-20, whose square
    is a subnormal v (the square root of a subnormal); p = 0.  All bit for bit, three steps.  Parameters and exp_avg stay finite everywhere.
    exp_avg_sq is +inf at the two overflow elements -- (w2 * g) * g = 1e47 has no float32 value, in torch.optim.AdamW's float32 step as in
    this one -- and from there on those parameters only decay (m / inf = 0); everywhere else exp_avg_sq is finite too."""
    from tinyfaces import ops
    n = 4099
    plant = {8: 0.0, 9: 0.0, 16: 1e25, 17: -1e25, 24: 1e-30, 25: -1e-30, 32: 1e-40, 33: -3e-42, 40: 1e-20, 41: -1e-20, 4097: 1e25, 4098: 0.0}
    base = [torch.zeros(n + 8).cuda() for _ in range(4)]
    p, g, m, v = [t[offset:offset + n] for t in base]
    hp = _randn(n, 5)
    hp[[9, 48, 49, 4096]] = 0.0
    p.copy_(torch.from_numpy(hp))
    hm, hv = np.zeros(n, F), np.zeros(n, F)
    state = ops.AdamState("cuda")
    overflow = np.array([k for k, x in plant.items() if abs(x) > 1e20])
    for t in range(3):
        hg = _randn(n, 60 + t)
        for k, x in plant.items():
            hg[k] = x
        assert 0.0 < abs(float(hg[32])) < 1.2e-38 and 0.0 < abs(float(hg[33])) < 1.2e-38
        g.copy_(torch.from_numpy(hg))
        ops.adamw_advance(state, BETAS)
        ops.adamw_step(p, g, m, v, state, *HYPER, 1.0)
        torch.cuda.synchronize()
        hp, hm, hv = adamw_ref.adamw_step(hp, hg, hm, hv, t + 1, *HYPER, grad_scale=1.0)
        assert _same(p, hp) and _same(m, hm) and _same(v, hv), (offset, t)
        assert np.isfinite(hp).all() and np.isfinite(hm).all()
        fin = np.isfinite(hv)
        assert np.array_equal(np.flatnonzero(~fin), np.sort(overflow)) and (hv[overflow] == np.inf).all()
        assert hv[8] == 0.0 and hm[8] == 0.0 and hv[24] == 0.0 and 0.0 < hv[40] < 1.2e-38
    assert hp[9] == 0.0 and hp[48] != 0.0                                       # p = 0 with g = 0 stays 0; p = 0 with a gradient moves
    report(f"adamw_planted[{'scalar' if offset else 'float4'}]", planted=len(plant))


# ---------------------------------------------------------------------------------------------------------------- 4: the EMA, fused
@pytest.mark.parametrize("kind", ["flat_float4", "flat_scalar", "aligned", "300_unaligned"])
def test_fused_average_is_the_fmaf_on_the_updated_parameter(kind):
    from test_gpu_grad_clip import N, TABLES
    from tinyfaces import ops
    offset = 1 if kind == "flat_scalar" else 0
    segs = None if kind.startswith("flat") else TABLES[kind]
    n = N + 3
    mk = np.ones(n, dtype=bool) if segs is None else _mask(n, segs)

    def operands():
        base = [torch.from_numpy(_randn(n + 4, 70 + k)).cuda() for k in range(5)]
        p, g, m, v, e = [t[offset:offset + n] for t in base]
        m.zero_()
        v.zero_()
        return p, g, m, v, e

    p, g, m, v, e = operands()
    rp, _, rm, rv, _ = operands()
    sa, sb = ops.AdamState("cuda"), ops.AdamState("cuda")
    e_start = e.cpu().numpy()
    for t in range(3):
        g.copy_(torch.from_numpy(_randn(n, 80 + t)))
        e_before = e.cpu().numpy()
        ops.adamw_advance(sa, BETAS)
        ops.adamw_advance(sb, BETAS)
        if segs is None:
            ops.adamw_step(p, g, m, v, sa, *HYPER, GS, ema=e, ema_weight=EMA_W)
            ops.adamw_step(rp, g, rm, rv, sb, *HYPER, GS)
        else:
            ops.adamw_step_segments(p, g, m, v, sa, segs, *HYPER, GS, ema=e, ema_weight=EMA_W)
            ops.adamw_step_segments(rp, g, rm, rv, sb, segs, *HYPER, GS)
        torch.cuda.synchronize()
        assert torch.equal(_i32(p), _i32(rp)) and torch.equal(_i32(m), _i32(rm)) and torch.equal(_i32(v), _i32(rv)), (kind, t)
        got = e.cpu().numpy()
        want = adamw_ref.ema_step(e_before[mk], p.cpu().numpy()[mk], EMA_W)
        assert np.array_equal(_bits(got[mk]), _bits(want)), (kind, t)
        assert np.array_equal(_bits(got[~mk]), _bits(e_start[~mk])), (kind, t)
    assert not np.array_equal(e.cpu().numpy()[mk], e_start[mk])


# ---------------------------------------------------------------------------------------------------------------- 5: the clip state
@pytest.mark.parametrize("kind", ["flat_float4", "flat_scalar", "aligned", "300_unaligned"])
def test_clipped_step_is_the_plain_step_at_the_product_scale_and_a_skipped_one_is_a_no_op(kind):
    from test_gpu_grad_clip import N, TABLES, _clipped_state, _skip_state
    from tinyfaces import ops
    offset = 1 if kind == "flat_scalar" else 0
    segs = None if kind.startswith("flat") else TABLES[kind]
    n = N + 3
    table = [(0, n)] if segs is None else segs

    def operands():
        base = [torch.from_numpy(_randn(n + 4, 90 + k)).cuda() for k in range(5)]
        p, g, m, v, e = [t[offset:offset + n] for t in base]
        m.zero_()
        v.zero_()
        return p, g, m, v, e

    def launch(p, g, m, v, st, gs, **kw):
        if segs is None:
            ops.adamw_step(p, g, m, v, st, *HYPER, gs, **kw)
        else:
            ops.adamw_step_segments(p, g, m, v, st, segs, *HYPER, gs, **kw)

    p, g, m, v, e = operands()
    rp, _, rm, rv, _ = operands()
    clip, coef = _clipped_state(g.clone(), table, GS)
    prod = float(F(GS) * F(coef))
    sa, sb = ops.AdamState("cuda"), ops.AdamState("cuda")
    for t in range(2):
        ops.adamw_advance(sa, BETAS, clip)
        ops.adamw_advance(sb, BETAS)
        launch(p, g, m, v, sa, GS, clip_state=clip)
        launch(rp, g, rm, rv, sb, prod)
        torch.cuda.synchronize()
        assert torch.equal(_i32(p), _i32(rp)) and torch.equal(_i32(m), _i32(rm)) and torch.equal(_i32(v), _i32(rv)), (kind, t)
    _state_is(sa, 2)
    # skip = 1: parameters, both moments, the average and the 24-byte state keep their bits
    skip = _skip_state()
    p0, m0, v0, e0, s0 = p.clone(), m.clone(), v.clone(), e.clone(), sa.buf.clone()
    ops.adamw_advance(sa, BETAS, skip)
    launch(p, g, m, v, sa, GS, ema=e, ema_weight=EMA_W, clip_state=skip)
    torch.cuda.synchronize()
    assert torch.equal(_i32(p), _i32(p0)) and torch.equal(_i32(m), _i32(m0)) and torch.equal(_i32(v), _i32(v0)) and torch.equal(_i32(e), _i32(e0))
    assert torch.equal(sa.buf, s0) and skip.skipped() == 1                      # (the AdamW entries only read the clip state)
    # the step after a skipped one is step + 1, not step + 2
    ops.adamw_advance(sa, BETAS, clip)
    ops.adamw_advance(sb, BETAS)
    launch(p, g, m, v, sa, GS, clip_state=clip)
    launch(rp, g, rm, rv, sb, prod)
    torch.cuda.synchronize()
    _state_is(sa, 3)
    assert torch.equal(_i32(p), _i32(rp)) and torch.equal(_i32(m), _i32(rm)) and torch.equal(_i32(v), _i32(rv))
    assert not torch.equal(p, p0)
    report(f"adamw_clipped[{kind}]", coef=coef, product_scale=prod)


# ---------------------------------------------------------------------------------------------------------------- 6: argument errors
def test_argument_errors_and_empty_calls_launch_nothing(hip):
    from tinyfaces import ops
    l = hip.lib()
    n = 64
    p, g, m, v = [torch.from_numpy(_randn(n, 110 + k, scale=False)).cuda() for k in range(4)]
    keep = [t.clone() for t in (p, g, m, v)]
    state = ops.AdamState("cuda")
    ops.adamw_advance(state, BETAS)
    s0 = state.buf.clone()
    s = torch.cuda.current_stream().cuda_stream
    ok = (LR, BETAS[0], BETAS[1], EPS, WD, 1.0, 0.0)
    tab = (hip.i64 * 4)(0, 8, 16, 32)
    bad = (hip.i64 * 4)(16, 32, 0, 8)
    P, G, M, V, S = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), state.buf.data_ptr()
    ERR = -1
    assert l.tf_adamw_advance(None, 0.9, 0.999, None, s) == ERR and l.tf_adamw_advance(S, 0.9, 1.0, None, s) == ERR
    for args in ((None, G, M, V), (P, None, M, V), (P, G, None, V), (P, G, M, None)):
        assert l.tf_adamw_step(*args, None, n, *ok, S, None, s) == ERR
        assert l.tf_adamw_step_segments(*args, None, tab, 2, *ok, S, None, s) == ERR
    assert l.tf_adamw_step(P, G, M, V, None, n, *ok, None, None, s) == ERR
    assert l.tf_adamw_step_segments(P, G, M, V, None, None, 2, *ok, S, None, s) == ERR
    assert l.tf_adamw_step_segments(P, G, M, V, None, bad, 2, *ok, S, None, s) == ERR
    for eps in (0.0, -1e-8, float("nan")):
        assert l.tf_adamw_step(P, G, M, V, None, n, LR, 0.9, 0.999, eps, WD, 1.0, 0.0, S, None, s) == ERR
        assert l.tf_adamw_step_segments(P, G, M, V, None, tab, 2, LR, 0.9, 0.999, eps, WD, 1.0, 0.0, S, None, s) == ERR
    assert l.tf_adamw_step(P, G, M, V, None, -1, *ok, S, None, s) == ERR and l.tf_adamw_step_segments(P, G, M, V, None, tab, -1, *ok, S, None, s) == ERR
    assert l.tf_adamw_step(P, G, M, V, None, 0, *ok, S, None, s) == 0 and l.tf_adamw_step_segments(P, G, M, V, None, tab, 0, *ok, S, None, s) == 0
    ops.adamw_step_segments(p, g, m, v, state, [], *HYPER)
    ops.adamw_step_segments(p, g, m, v, state, [(5, 5)], *HYPER)
    with pytest.raises(ValueError):
        ops.adamw_step(p, g, m, v, state, LR, BETAS, 0.0, WD)
    with pytest.raises(ValueError):
        ops.adamw_step(p, g, m, v, state, LR, (0.9, 1.0), EPS, WD)
    with pytest.raises(ValueError):
        ops.adamw_step(p, g, m, v, state, *HYPER, ema=p.clone())
    with pytest.raises(ValueError):
        ops.adamw_step_segments(p, g, m, v, state, [(8, 16), (0, 4)], *HYPER)
    torch.cuda.synchronize()
    for t, t0 in zip((p, g, m, v), keep):
        assert torch.equal(_i32(t), _i32(t0))
    assert torch.equal(state.buf, s0)
    # set_step: the counter alone; the corrections follow at the next advance
    state.set_step(41)
    assert state.step() == 41
    ops.adamw_advance(state, BETAS)
    _state_is(state, 42)
    with pytest.raises(ValueError):
        state.set_step(-1)


# ---------------------------------------------------------------------------------------------------------------- 7: the write contract
@pytest.mark.parametrize("name", ["unaligned_empty_single", "300_aligned", "300_unaligned", "whole"])
def test_every_entry_point_writes_inside_its_operands_only(hip, name):
    """tests/redzone.py: parameters, gradient, both moments, the average and the 24-byte state between 0xFF guard bands; after each of the
    three entries (the flat one on its 16-byte and on its scalar path, with and without the average) every guard is intact, the gradient is
    unchanged and the table entry writes nothing outside its ranges."""
    from test_gpu_grad_clip import N, TABLES
    l = hip.lib()
    segs = TABLES[name]
    nseg = len(segs)
    table = (hip.i64 * (2 * nseg))(*[x for se in segs for x in se])
    mk = torch.from_numpy(_mask(N, segs)).cuda()
    host = [torch.from_numpy(_randn(N, 120 + k)) for k in range(5)]
    host[2].zero_()
    host[3].zero_()
    p, g, m, v, e = [guarded_like(t, "cuda") for t in host]
    state = guarded((24,), torch.uint8, "cuda", body="keep")
    state.zero_()
    g0 = g.clone()
    s = torch.cuda.current_stream().cuda_stream
    hy = (LR, BETAS[0], BETAS[1], EPS, WD, 1.0)

    def everything(what):
        torch.cuda.synchronize()
        for t, label in ((p, "parameters"), (g, "gradient"), (m, "exp_avg"), (v, "exp_avg_sq"), (e, "average"), (state, "state")):
            assert_guards(t, f"{what}: {label}")
        assert torch.equal(_i32(g), _i32(g0)), what

    assert l.tf_adamw_advance(state.data_ptr(), BETAS[0], BETAS[1], None, s) == 0
    everything("tf_adamw_advance")
    st = hip.AdamState.from_buffer_copy(state.cpu().numpy().tobytes())
    assert (st.step, st.bias1, st.bias2) == (1,) + adamw_ref.bias_corrections(BETAS, 1)
    before = [t.clone() for t in (p, m, v, e)]
    assert l.tf_adamw_step_segments(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr(), table, nseg, *hy, EMA_W, state.data_ptr(), None, s) == 0
    everything("tf_adamw_step_segments")
    for t, t0 in zip((p, m, v, e), before):
        assert torch.equal(_i32(t[~mk]), _i32(t0[~mk])) and not torch.equal(t[mk], t0[mk])
    assert l.tf_adamw_step_segments(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None, table, nseg, *hy, 0.0, state.data_ptr(), None, s) == 0
    everything("tf_adamw_step_segments without the average")
    assert l.tf_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), e.data_ptr(), N, *hy, EMA_W, state.data_ptr(), None, s) == 0
    everything("tf_adamw_step")
    assert l.tf_adamw_step(p.data_ptr() + 4, g.data_ptr() + 4, m.data_ptr() + 4, v.data_ptr() + 4, e.data_ptr() + 4, N - 1, *hy, EMA_W, state.data_ptr(), None, s) == 0
    everything("tf_adamw_step, scalar path")
    assert l.tf_adamw_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None, N, *hy, 0.0, state.data_ptr(), None, s) == 0
    everything("tf_adamw_step without the average")
    assert all(torch.isfinite(t).all() for t in (p, m, v, e))
    assert hip.AdamState.from_buffer_copy(state.cpu().numpy().tobytes()).step == 1      # the step entries only read the state


# ---------------------------------------------------------------------------------------------------------------- engine level
def _model(dtype=torch.float32, frozen=False, seed=6):
    from test_gpu_frozen_bn import _oracle, _product
    m = _product(_oracle("resnet50", seed=seed), "resnet50").set_compute_dtype(dtype)
    if frozen:
        m.freeze_batchnorm().set_trainable_layers(2)
    return m


def _trained(m):
    seg = m._segments
    return sorted((seg[k][0], seg[k][0] + seg[k][1]) for k in m.trainable_parameter_names())


def _update_index(eng):
    """[(element indices, lr multiplier)] per group the update touches: the whole group on batch statistics (pads and BatchNorm vectors
    included, as the flat launch walks them), its trained segments under frozen BatchNorm."""
    m = eng.model
    out = []
    for a, b, mult in eng.groups:
        if mult == 0.0:
            continue
        if m.batchnorm_frozen:
            idx = np.concatenate([np.arange(max(s, a), min(e, b)) for s, e in _trained(m) if e > a and s < b] or [np.zeros(0, np.int64)])
        else:
            idx = np.arange(a, b)
        out.append((idx, mult))
    return out


def _host_update(eng, before, gflat, step, coef, scale=1.0, ema_w=None):
    """The restatement applied on the host to the engine's buffers `before` = (p, m, v, e or None), group by group with the lr multipliers."""
    p, m, v, e = [None if t is None else t.copy() for t in before]
    g = gflat.detach().cpu().numpy()
    for idx, mult in _update_index(eng):
        rp, rm, rv = adamw_ref.adamw_step(p[idx], g[idx], m[idx], v[idx], step, eng.lr * mult, eng.betas, eng.eps, eng.weight_decay,
                                          grad_scale=scale, coef=coef)
        p[idx], m[idx], v[idx] = rp, rm, rv
        if e is not None:
            e[idx] = adamw_ref.ema_step(e[idx], rp, ema_w)
    return p, m, v, e


def _snapshot(eng):
    return tuple(None if t is None else t.detach().cpu().numpy().copy()
                 for t in (eng.flat_p, eng.flat_m, eng.flat_v, None if eng.ema is None else eng.ema.flat))


@contextmanager
def _planted_gradient(m, source):
    """Behind the real backward pass, on the training stream: source() returns the gradient to leave in the flat buffer (a tensor), a
    (index, value) pair to plant, or None."""
    run_backward = m._run_backward

    def planted(xx, grad, persistent=False):
        out = run_backward(xx, grad, persistent=persistent)
        what = source()
        if isinstance(what, tuple):
            out[what[0]] = what[1]
        elif what is not None:
            out.copy_(what)
        return out

    m._run_backward = planted
    try:
        yield
    finally:
        m._run_backward = run_backward


@pytest.mark.parametrize("frozen", [False, True], ids=["batch_stats", "frozen_bn_k2"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_engine_takes_the_restatements_step(dtype, frozen):
    """ResNet-50, 2 x 3 x 256 x 256, ema_decay 0.999, three steps: the first plain (it gives the norm), the next two with max_grad_norm at a
    quarter of that norm (coef < 1).  After each, flat_p, flat_m, flat_v and the average are bit for bit the restatement applied on the host
    to the gradient the step left in the persistent flat buffer, group by group with the lr multipliers; everything else -- frozen slices,
    the lr-0 group -- keeps its bits, and the device step counts the steps."""
    from test_gpu_grad_clip import _engine_inputs, _host_norm
    from tinyfaces.ema import ema_decay_at
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.loss import DetectionCriterion
    m = _model(dtype, frozen)
    eng = TrainEngine(m, DetectionCriterion(25), lr=1e-3, weight_decay=1e-2, device="cuda", ema_decay=0.999, optimizer="adamw", betas=BETAS, eps=EPS)
    assert eng.flat_v.shape == eng.flat_p.shape and float(eng.flat_v.abs().sum()) == 0.0 and eng.adam_state.step() == 0
    x, cm, rm = _engine_inputs()
    gflat = m._grad_flat_persistent
    tag = f"engine_adamw[{'bf16' if dtype == torch.bfloat16 else 'fp32'},{'frozen_k2' if frozen else 'batch_stats'}]"
    touched = np.zeros(eng.flat_p.numel(), dtype=bool)
    for idx, _ in _update_index(eng):
        touched[idx] = True
    init = _snapshot(eng)
    for t in range(3):
        before = _snapshot(eng)
        eng.step(x, cm.clone(), rm)
        torch.cuda.synchronize()
        coef = None
        if t > 0:
            st = eng._clip_state.read()
            coef = st.coef
            assert 0.0 < coef < 1.0 and st.skip == 0
        w = float(F(1.0 - ema_decay_at(0.999, t)))
        want = _host_update(eng, before, gflat, t + 1, coef, ema_w=w)
        got = _snapshot(eng)
        for name, a, b in zip(("flat_p", "flat_m", "flat_v", "ema"), got, want):
            assert np.array_equal(_bits(a), _bits(b)), (tag, t, name, int((_bits(a) != _bits(b)).sum()))
        for name, a, b in zip(("flat_p", "flat_m", "flat_v", "ema"), got, init):
            assert np.array_equal(_bits(a[~touched]), _bits(b[~touched])), (tag, t, name)
        assert not np.array_equal(got[0][touched], before[0][touched])
        _state_is(eng.adam_state, t + 1)
        if t == 0:
            assert eng._clip_state is None
            eng.set_max_grad_norm(float(F(_host_norm(gflat, _trained(m)) / 4)))
        report(tag, step=t, coef=1.0 if coef is None else coef, updated_elements=int(touched.sum()))
    assert all(np.isfinite(a).all() for a in got)
    if frozen:
        assert int((~touched).sum()) > 1000
    eng.close()


def test_engine_guard_leaves_a_skipped_step_untouched_and_accumulation_applies_the_sum():
    """skip_nonfinite: a NaN planted behind the backward pass moves nothing -- parameters, both moments, the average, the 24-byte state -- and the
    next clean step is step 2, not 3.  accum_steps = 2: the window's update is the restatement on the sum the accumulation left in the flat
    gradient buffer, which is the first micro-batch's gradient plus the second's, and the device step advances once per window."""
    from test_gpu_grad_clip import _engine_inputs
    from tinyfaces.ema import ema_decay_at
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.loss import DetectionCriterion
    m = _model(torch.bfloat16, frozen=True)
    eng = TrainEngine(m, DetectionCriterion(25), lr=1e-3, weight_decay=1e-2, device="cuda", ema_decay=0.999, optimizer="adamw", skip_nonfinite=True)
    x, cm, rm = _engine_inputs()
    gflat = m._grad_flat_persistent
    victim = m._segments["model.layer3.1.conv2.weight"][0] + 5
    plant = [None]
    with _planted_gradient(m, lambda: plant[0]):
        eng.step(x, cm.clone(), rm)
        torch.cuda.synchronize()
        _state_is(eng.adam_state, 1)
        before, s0 = _snapshot(eng), eng.adam_state.buf.clone()
        plant[0] = (victim, float("nan"))
        eng.step(x, cm.clone(), rm)
        torch.cuda.synchronize()
        assert eng.skipped_steps == 1 and torch.equal(eng.adam_state.buf, s0)
        for a, b in zip(_snapshot(eng), before):
            assert np.array_equal(_bits(a), _bits(b))
        plant[0] = None
        eng.step(x, cm.clone(), rm)
        torch.cuda.synchronize()
    _state_is(eng.adam_state, 2)
    w = float(F(1.0 - ema_decay_at(0.999, 2)))                                  # (ema.updates counts steps taken, skipped ones included)
    want = _host_update(eng, before, gflat, 2, eng._clip_state.read().coef, ema_w=w)
    for a, b in zip(_snapshot(eng), want):
        assert np.array_equal(_bits(a), _bits(b))
    assert eng.steps == 3 and eng.skipped_steps == 1
    eng.close()

    m = _model(torch.bfloat16, frozen=True)
    eng = TrainEngine(m, DetectionCriterion(25), lr=1e-3, weight_decay=1e-2, device="cuda", optimizer="adamw", accum_steps=2)
    gflat = m._grad_flat_persistent
    mk = _mask(eng.flat_p.numel(), _trained(m))
    before = _snapshot(eng)
    eng.step(x, cm.clone(), rm)
    torch.cuda.synchronize()
    g1 = gflat.cpu().numpy().copy()
    assert eng.steps == 0 and eng.adam_state.step() == 0
    for a, b in zip(_snapshot(eng), before):
        assert a is None or np.array_equal(_bits(a), _bits(b))                  # a micro-batch that is not applied updates nothing
    seen = []
    with _planted_gradient(m, lambda: seen.append(gflat.cpu().numpy().copy())):
        eng.step(x.flip(0), cm.flip(0).clone(), rm.flip(0))
    torch.cuda.synchronize()
    g2, gsum = seen[0], gflat.cpu().numpy()
    assert np.array_equal(_bits(gsum[mk]), _bits((g1 + g2)[mk])) and not np.array_equal(g1[mk], g2[mk])
    want = _host_update(eng, before, gflat, 1, None)
    for a, b in zip(_snapshot(eng), want):
        assert a is None or np.array_equal(_bits(a), _bits(b))
    _state_is(eng.adam_state, 1)
    assert eng.steps == 1 and eng.micro_steps == 2
    eng.close()


def test_default_optimizer_is_the_engine_of_before(monkeypatch):
    """optimizer="sgd" spelled out against an engine built without the new keywords, three steps on the same gradients (see the module
    docstring): parameters and momentum bit-identical, flat_v and the adam state do not exist, the SGD ops are called with positional
    arguments only as before, and no AdamW entry point is called."""
    from test_gpu_grad_clip import _engine_inputs
    from tinyfaces import _hip, ops
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.loss import DetectionCriterion
    a = TrainEngine(_model(torch.bfloat16), DetectionCriterion(25), lr=1e-3, device="cuda")
    b = TrainEngine(_model(torch.bfloat16), DetectionCriterion(25), lr=1e-3, device="cuda", optimizer="sgd", betas=(0.8, 0.99), eps=1e-6)
    for eng in (a, b):
        assert eng.optimizer == "sgd" and not hasattr(eng, "flat_v") and not hasattr(eng, "adam_state")
    seen, new_calls = [], []
    for name in ("sgd_step", "sgd_step_segments", "adamw_advance", "adamw_step", "adamw_step_segments"):
        def spy(*args, _f=getattr(ops, name), _n=name, **kw):
            seen.append((_n, len(args), sorted(kw)))
            return _f(*args, **kw)
        monkeypatch.setattr(ops, name, spy)
    l = _hip.lib()
    for name in ("tf_adamw_advance", "tf_adamw_step", "tf_adamw_step_segments"):
        def entry(*args, _f=getattr(l, name), _n=name):
            new_calls.append(_n)
            return _f(*args)
        monkeypatch.setattr(l, name, entry)
    x, cm, rm = _engine_inputs()
    ga = a.model._grad_flat_persistent
    assert torch.equal(_i32(a.flat_p), _i32(b.flat_p))
    with _planted_gradient(b.model, lambda: ga):
        for t in range(3):
            a.step(x, cm.clone(), rm)
            b.step(x, cm.clone(), rm)
            torch.cuda.synchronize()
            assert torch.equal(_i32(a.flat_p), _i32(b.flat_p)) and torch.equal(_i32(a.flat_m), _i32(b.flat_m)), t
    assert [c[0] for c in seen] == ["sgd_step"] * 18 and all(c[1] == 7 and c[2] == [] for c in seen)
    assert new_calls == [] and float(a.flat_m.abs().max()) > 0.0
    # ... and the spies do see the feature when it is on
    c = TrainEngine(_model(torch.bfloat16), DetectionCriterion(25), lr=1e-3, device="cuda", optimizer="adamw")
    del seen[:]
    c.step(x, cm.clone(), rm)
    torch.cuda.synchronize()
    assert [s[0] for s in seen] == ["adamw_advance"] + ["adamw_step"] * 3
    assert new_calls == ["tf_adamw_advance"] + ["tf_adamw_step"] * 3
    for eng in (a, b, c):
        eng.close()


def test_engine_refusals(monkeypatch):
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.loss import DetectionCriterion
    for kw in (dict(optimizer="adam"), dict(optimizer="adamw", betas=(0.9, 1.0)), dict(optimizer="adamw", betas=(-0.1, 0.9)),
               dict(optimizer="adamw", eps=0.0), dict(optimizer="adamw", eps=-1.0)):
        with pytest.raises(ValueError):
            TrainEngine(_model(torch.bfloat16), DetectionCriterion(25), device="cuda", **kw)
    monkeypatch.setenv("TINYFACES_SGD_PER_BUCKET", "1")
    with pytest.raises(ValueError, match="TINYFACES_SGD_PER_BUCKET"):
        TrainEngine(_model(torch.bfloat16), DetectionCriterion(25), device="cuda", optimizer="adamw")


# ---------------------------------------------------------------------------------------------------------------- 11: checkpoints
def test_checkpoint_is_torchs_adamw_format_and_resumes_bit_for_bit(capsys):
    from test_gpu_grad_clip import _engine_inputs
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as zoo
    from tinyfaces.models.loss import DetectionCriterion
    lr, wd = 1e-3, 1e-2
    m = _model(torch.float32, frozen=True)
    eng = TrainEngine(m, DetectionCriterion(25), lr=lr, weight_decay=wd, device="cuda", optimizer="adamw", betas=BETAS, eps=EPS)
    assert eng.optimizer_state_dict()["state"] == {}                            # never stepped: torch has no state either
    x, cm, rm = _engine_inputs()
    for _ in range(2):
        eng.step(x, cm.clone(), rm)
    torch.cuda.synchronize()
    sd = eng.optimizer_state_dict(base_lr=lr)
    seg, names = m._segments, set(m.trainable_parameter_names())

    # a real AdamW takes it
    opt = torch.optim.AdamW(m.learnable_parameters(lr), lr=lr, betas=BETAS, eps=EPS, weight_decay=wd)
    real = opt.state_dict()
    assert [set(g) | {"initial_lr"} for g in real["param_groups"]] == [set(g) for g in sd["param_groups"]]
    assert [g["params"] for g in real["param_groups"]] == [g["params"] for g in sd["param_groups"]]
    opt.load_state_dict(sd)
    name_of = {id(p): k for k, p in m.named_parameters()}
    with_state = 0
    for gi, group in enumerate(opt.param_groups):
        for p in group["params"]:
            k = name_of[id(p)]
            st = opt.state.get(p)
            if k in names and k in seg and gi != 3:
                o, n = seg[k]
                assert float(st["step"]) == 2.0
                assert torch.equal(_i32(st["exp_avg"].reshape(-1)), _i32(eng.flat_m[o:o + n])), k
                assert torch.equal(_i32(st["exp_avg_sq"].reshape(-1)), _i32(eng.flat_v[o:o + n])), k
                with_state += 1
            else:
                assert not st, k                                                # frozen tensors and the lr-0 group: no state
    assert with_state > 10
    for st in sd["state"].values():
        assert st["step"].dtype == torch.float32 and st["step"].dim() == 0 and not st["step"].is_cuda and not st["exp_avg"].is_cuda

    # an open accumulation window refuses the export, as under SGD
    eng._window = 1
    with pytest.raises(RuntimeError, match="accumulated"):
        eng.optimizer_state_dict()
    eng._window = 0

    # a fresh engine on the same weights continues bit for bit
    m2 = zoo.DetectionModel(base_model=zoo.resnet50, num_templates=25).set_compute_dtype(torch.float32)
    m2.load_state_dict(m.state_dict())
    m2.freeze_batchnorm().set_trainable_layers(2)
    eng2 = TrainEngine(m2, DetectionCriterion(25), lr=lr, weight_decay=0.5, device="cuda", optimizer="adamw", betas=(0.5, 0.5), eps=1.0)
    assert eng2.load_optimizer_state_dict(sd) is True
    assert (eng2.betas, eng2.eps, eng2.weight_decay) == (BETAS, EPS, wd) and eng2.adam_state.step() == 2
    assert torch.equal(_i32(eng2.flat_p), _i32(eng.flat_p)) and torch.equal(_i32(eng2.flat_m), _i32(eng.flat_m)) and torch.equal(_i32(eng2.flat_v), _i32(eng.flat_v))
    ga = m._grad_flat_persistent
    with _planted_gradient(m2, lambda: ga):
        eng.step(x, cm.clone(), rm)
        eng2.step(x, cm.clone(), rm)
        torch.cuda.synchronize()
    for name in ("flat_p", "flat_m", "flat_v"):
        assert torch.equal(_i32(getattr(eng, name)), _i32(getattr(eng2, name))), name
    _state_is(eng2.adam_state, 3)

    # the other optimizer's state: a warning that names both, moments from zero, no exception
    sgd = TrainEngine(_model(torch.float32, frozen=True), DetectionCriterion(25), lr=lr, device="cuda")
    sgd.step(x, cm.clone(), rm)
    torch.cuda.synchronize()
    capsys.readouterr()
    assert eng2.load_optimizer_state_dict(sgd.optimizer_state_dict()) is True
    text = capsys.readouterr().out
    assert "WARNING" in text and "sgd" in text and "adamw" in text
    assert float(eng2.flat_m.abs().sum()) == 0.0 and float(eng2.flat_v.abs().sum()) == 0.0 and eng2.adam_state.step() == 0
    assert sgd.load_optimizer_state_dict(sd) is True
    text = capsys.readouterr().out
    assert "WARNING" in text and "sgd" in text and "adamw" in text and float(sgd.flat_m.abs().sum()) == 0.0
    for e_ in (eng, eng2, sgd):
        e_.close()


# ---------------------------------------------------------------------------------------------------------------- 12: two ranks
def test_two_ranks_hold_the_same_parameters_moments_and_step(tmp_path):
    """2 gloo ranks sharing cuda:0 (tests/dist_worker_adamw.py), two clipped steps: both ranks hold the same parameter bits, the same moments
    and the same device step without a collective of the optimizer's own."""
    golden = os.path.join(ROOT, "tests", "golden", "trainer.npz")
    out = str(tmp_path / "adamw")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29587", os.path.join(ROOT, "tests", "dist_worker_adamw.py"), golden, out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = [np.load(f"{out}.rank{k}.npz") for k in range(2)]
    mk = got[0]["trained"]
    assert int(mk.sum()) > 0
    for key in ("trained", "p_init", "p0", "p1", "m0", "m1", "v0", "v1", "step", "bias"):
        assert np.array_equal(_bits(got[0][key]) if got[0][key].dtype == np.float32 else got[0][key], _bits(got[1][key]) if got[1][key].dtype == np.float32 else got[1][key]), key
    assert int(got[0]["step"]) == 2 and tuple(got[0]["bias"]) == adamw_ref.bias_corrections(BETAS, 2)
    assert not np.array_equal(got[0]["p1"][mk], got[0]["p0"][mk]) and not np.array_equal(got[0]["p0"][mk], got[0]["p_init"][mk])
    assert np.array_equal(_bits(got[0]["p1"][~mk]), _bits(got[0]["p_init"][~mk])) and float(np.abs(got[0]["v1"][~mk]).sum()) == 0.0
    assert float(got[0]["v1"][mk].max()) > 0.0 and np.isfinite(got[0]["p1"]).all()
    report("adamw_dist_2_ranks[resnet50,k=1]", trained_elements=int(mk.sum()))


# ---------------------------------------------------------------------------------------------------------------- 13: warm-up and the scripts
def test_fused_epoch_sets_the_closed_form_lr_once_per_optimizer_step():
    """main.run_fused_epoch with --warmup-iters 4 --warmup-factor 0.01 and accum_steps = 2 over five batches an epoch (S = 3), two epochs: the lr
    the engine holds at every micro-batch is lr_at * (F + (1 - F) * min(T, N) / N) with T = epoch * S + the optimizer steps taken so far."""
    import main
    from test_gpu_grad_clip import _engine_inputs
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.loss import DetectionCriterion
    base, N_, F_ = 1e-3, 4, 0.01
    crit = DetectionCriterion(25, lazy_meters=True)
    eng = TrainEngine(_model(torch.bfloat16, frozen=True), crit, lr=base, device="cuda", optimizer="adamw", accum_steps=2)
    batch = tuple(t.cpu() for t in _engine_inputs())
    seen, step = [], eng.step

    def spy(*a, **kw):
        seen.append(eng.lr)
        return step(*a, **kw)

    eng.step = spy
    with redirect_stdout(io.StringIO()):
        for epoch in range(2):
            main.run_fused_epoch(eng, crit, [batch] * 5, epoch, torch.device("cuda"), base, warmup=(N_, F_))
    torch.cuda.synchronize()
    T = [0, 0, 1, 1, 2, 3, 3, 4, 4, 5]
    assert seen == [base * (F_ + (1 - F_) * min(t, N_) / N_) for t in T]
    assert seen[0] == pytest.approx(base * F_) and seen[-1] == base and eng.steps == 6 and eng.adam_state.step() == 6
    # off: one set_lr per epoch, as before
    del seen[:]
    with redirect_stdout(io.StringIO()):
        main.run_fused_epoch(eng, crit, [batch] * 2, 20, torch.device("cuda"), base)
    assert seen == [main.lr_at(base, 20)] * 2
    eng.close()


def test_trainer_warms_up_torchs_adamw_and_puts_the_lr_back(golden):
    from test_gpu_frozen_bn import _golden_batches, _keep
    from tinyfaces import trainer
    from tinyfaces.models.loss import DetectionCriterion
    dev = torch.device("cuda")
    m = _model(torch.float32, seed=9).to(dev).train()
    c = DetectionCriterion(25)
    c.inject_sampling(_keep(), _keep())
    lr = 1e-3
    opt = torch.optim.AdamW(m.learnable_parameters(lr), lr=lr, weight_decay=1e-2)
    found = [g["lr"] for g in opt.param_groups]
    seen, step = [], opt.step

    def spy(*a, **kw):
        seen.append([g["lr"] for g in opt.param_groups])
        return step(*a, **kw)

    opt.step = spy
    batches = _golden_batches(golden)
    with redirect_stdout(io.StringIO()):
        trainer.train(m, c, opt, [batches[0], batches[1], batches[0]], 0, dev, warmup=(3, 1e-3, 1))
    want = [[f * trainer.warmup_factor(1 + k, 3, 1e-3) for f in found] for k in range(3)]
    assert seen == want and [g["lr"] for g in opt.param_groups] == found
    assert seen[0][0] == pytest.approx(lr * (1e-3 + 0.999 / 3)) and seen[2] == found
    del seen[:]
    with redirect_stdout(io.StringIO()):
        trainer.train(m, c, opt, [batches[0]], 1, dev)                          # no warm-up: the groups are not touched
    assert seen == [found]


def _run_main(tmp_path, args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(PKG, "main.py"), "synthetic", "synthetic", "--base-model", "resnet50", "--synthetic-len", "6",
                        "--batch_size", "2", "--save-every", "1", "--optimizer", "adamw", "--warmup-iters", "3", "--lr", "1e-4"] + args,
                       cwd=tmp_path, capture_output=True, text=True, timeout=400, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    return r.stdout


def _check_adamw_checkpoint(path, epochs):
    state = torch.load(path, map_location="cpu")
    groups, st = state["optimizer"]["param_groups"], state["optimizer"]["state"]
    real = torch.optim.AdamW([torch.zeros(1)]).state_dict()["param_groups"][0]
    assert state["epoch"] == epochs and len(groups) == 4 and all(set(real) <= set(g) for g in groups)
    assert groups[0]["betas"] == (0.9, 0.999) and groups[0]["eps"] == 1e-8
    assert groups[0]["lr"] == pytest.approx(1e-4) and groups[1]["lr"] == pytest.approx(1e-5)      # the StepLR closed form, not the warm-up's
    # (the lr-0 group: the fused engine skips it and exports no state for it, torch steps it with lr 0 and counts from when it first did)
    frozen_lr = set(groups[3]["params"])
    assert len(st) > 100 and all(float(s["step"]) == 3.0 * epochs for i, s in st.items() if i not in frozen_lr)
    assert all(float(s["step"]) in (3.0, 3.0 * epochs) for i, s in st.items() if i in frozen_lr)
    assert all(torch.isfinite(s["exp_avg"]).all() and torch.isfinite(s["exp_avg_sq"]).all() for s in st.values())
    assert all(torch.isfinite(v).all() for v in state["model"].values())
    return state


@pytest.mark.parametrize("first", ["fused", "autograd"])
def test_scripts_train_with_adamw_and_resume_on_the_other_path(tmp_path, first):
    """main.py --optimizer adamw --warmup-iters 3, one epoch of three steps on the synthetic dataset on one path, then --resume of its checkpoint
    for a second epoch on the OTHER path: both checkpoints hold torch.optim.AdamW's state, the step count goes 3 -> 6."""
    flags = {"fused": [], "autograd": ["--no-fused", "--dtype", "fp32"]}
    other = "autograd" if first == "fused" else "fused"
    a, b = tmp_path / "a", tmp_path / "b"
    _run_main(tmp_path, flags[first] + ["--epochs", "1", "--save-path", str(a)])
    one = _check_adamw_checkpoint(a / "checkpoint_1.pth", 1)
    out = _run_main(tmp_path, flags[other] + ["--epochs", "2", "--resume", str(a / "checkpoint_1.pth"), "--save-path", str(b)])
    assert "start from zero" not in out                                         # the moments were taken over, not dropped
    two = _check_adamw_checkpoint(b / "checkpoint_2.pth", 2)
    moved = sum(not torch.equal(one["model"][k], two["model"][k]) for k in one["model"] if k.endswith("conv2.weight"))
    report(f"adamw_scripts[{first}_then_{other}]", conv2_weights_moved=moved)
    assert moved > 0
