"""-m gpu: the model EMA (csrc/sgd.hip: the EMA instantiations of the two SGD kernels, ema_segments_kernel; ops.sgd_step(..., ema=, ema_weight=),
ops.ema_update_segments; tinyfaces.ema.ModelEma; TrainEngine(ema_decay=); trainer.train(..., ema=); main.py --model-ema, evaluate_model.py --ema).

Every comparison is bit for bit.  One update is e = fmaf(w, p - e, e) in fp32.  The host reference is
    (e.double() + (p - e).double() * float(w)).float()
The difference p - e is the same single fp32 rounding on both sides, its product with w is exact in fp64 (24 + 24 bits), so the fp64 sum s is
the exact value rounded once to 53 bits, and s.float() can differ from a true fmaf only where s sits exactly halfway between two fp32
neighbours (the low 29 bits of its mantissa are 2^28).  The kernel tests use fixed seeds for which no element is such a tie and assert that
on the host before they compare.  The engine tests cannot choose: their parameters come out of a backward pass whose fp32 sums are not
ordered, 10^7 elements a step.  There `_fmaf` settles a tie by the exact error of the fp64 sum (Knuth's TwoSum): error > 0 rounds up, < 0
rounds down, = 0 is a true tie and s.float() has already taken the even neighbour -- the exactly rounded fmaf in every case, nothing looser.
For w < 0.5 the reference must also equal torch.lerp on the CPU.  Measured values go through gpu_util.report."""
import io
import os
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from gpu_util import report
from redzone import assert_guards, guarded_like

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tiny-faces-pytorch_amd")
WEIGHTS = [float(np.float32(0.9)), float(np.float32(1e-3)), float(np.float32(1e-4))]


def _i32(t):
    return t.contiguous().view(torch.int32)


def _fmaf(e, p, w):
    """(fmaf(w, p - e, e) for fp32 CPU tensors e, p and the fp32 value w, how many elements were halfway cases of the fp64 sum)."""
    assert e.dtype == p.dtype == torch.float32 and not e.is_cuda and float(np.float32(w)) == w
    prod = (p - e).double() * float(w)
    ed = e.double()
    s = ed + prod
    r = s.float()
    tie = (s.view(torch.int64) & ((1 << 29) - 1)) == (1 << 28)
    tie &= torch.isfinite(s)
    ties = int(tie.sum())
    if ties:
        b = s - ed
        err = (ed - (s - b)) + (prod - b)                                      # exact: s + err is the true sum
        up = torch.nextafter(r, torch.full_like(r, float("inf")))
        down = torch.nextafter(r, torch.full_like(r, float("-inf")))
        other = torch.where(r.double() > s, down, up)                         # the fp32 neighbour of s on the other side
        hi, lo = torch.maximum(r, other), torch.minimum(r, other)
        r = torch.where(tie & (err > 0), hi, torch.where(tie & (err < 0), lo, r))
    if w < 0.5:
        assert torch.equal(_i32(r), _i32(torch.lerp(e, p, w))), "the reference is not torch.lerp"
    return r, ties


def _fmaf_no_ties(e, p, w):
    r, ties = _fmaf(e, p, w)
    assert ties == 0, f"{ties} halfway cases: choose another seed"
    return r


def _tables():
    from test_gpu_grad_clip import N, TABLES
    return N, TABLES


def _mask(n, segs):
    mk = torch.zeros(n, dtype=torch.bool)
    for a, b in segs:
        mk[a:b] = True
    return mk


_HOST = {}


def _host(n, seed):
    """(e0, p) on the host, computed once per size and left unchanged: values of order 1, a few large and a few tiny ones, p near e in places."""
    if (n, seed) not in _HOST:
        g = torch.Generator().manual_seed(seed)
        e = torch.randn(n, generator=g)
        p = torch.randn(n, generator=g)
        p[::7] = e[::7] + 1e-3 * torch.randn(e[::7].shape, generator=g)        # an average that has nearly caught up
        e[::97] *= 1e3
        p[5::89] *= 1e-6
        _HOST[(n, seed)] = (e, p)
    return _HOST[(n, seed)]


def _standalone_cases():
    N, TABLES = _tables()
    stride = 3 * (1 << 20) + 3                                                  # beyond one trip of the capped grid (2048 x 256 x 4 elements)
    cases = [(name, N, segs, 0) for name, segs in TABLES.items()]
    cases += [(f"n{n}", n, [(0, n)], 0) for n in (1, 3, 5)]
    cases += [("base_off_by_one", N, TABLES["aligned"], 1)]
    cases += [("stride_aligned", stride, [(0, stride - 3)], 0), ("stride_scalar", stride, [(1, stride)], 0)]
    return cases


@pytest.mark.parametrize("name,n,segs,offset", _standalone_cases(), ids=[c[0] for c in _standalone_cases()])
def test_standalone_kernel_is_fmaf_bit_for_bit_and_touches_nothing_outside(name, n, segs, offset):
    from tinyfaces import ops
    e0, p = _host(n, 39 if n > (1 << 20) else 11)                               # (seeds without a halfway case at these sizes: _fmaf_no_ties)
    mk = _mask(n, segs)
    p_dev_src = p.clone()
    p_dev_src[~mk] = float("nan")                                               # never read: a NaN could not hide in an average
    for w in WEIGHTS:
        want = _fmaf_no_ties(e0, p, w)
        eb, pb = torch.zeros(n + 4).cuda(), torch.zeros(n + 4).cuda()
        e, pd = eb[offset:offset + n], pb[offset:offset + n]
        e.copy_(e0)
        pd.copy_(p_dev_src)
        assert (e.data_ptr() % 16 == 0) == (offset == 0)
        ops.ema_update_segments(e, pd, segs, w)
        torch.cuda.synchronize()
        got = e.cpu()
        assert torch.equal(_i32(got[mk]), _i32(want[mk])), (name, w)
        assert torch.equal(_i32(got[~mk]), _i32(e0[~mk])), (name, w)            # outside the ranges: the bits of before
        assert torch.equal(_i32(pd.cpu()), _i32(p_dev_src))                     # the parameters are read only
        assert float(eb[:offset].abs().sum()) == 0.0 and float(eb[offset + n:].abs().sum()) == 0.0
        moved = int((_i32(got[mk]) != _i32(e0[mk])).sum())
        report(f"ema_standalone[{name}]", w=w, elements=int(mk.sum()), moved=moved)
        assert moved > 0.9 * int(mk.sum())


def test_standalone_kernel_obeys_the_skip_verdict_and_ignores_the_coefficient():
    from test_gpu_grad_clip import _clipped_state, _skip_state
    from tinyfaces import ops
    N, TABLES = _tables()
    for name in ("aligned", "300_unaligned"):
        segs = TABLES[name]
        e0, p = _host(N, 11)
        w = WEIGHTS[1]
        want = _fmaf_no_ties(e0, p, w)
        mk = _mask(N, segs)
        e, pd = e0.cuda(), p.cuda()
        ops.ema_update_segments(e, pd, segs, w, clip_state=_skip_state())
        torch.cuda.synchronize()
        assert torch.equal(_i32(e.cpu()), _i32(e0)), name                       # a skipped step: no-op
        state, coef = _clipped_state(pd.clone(), segs, 1.0)
        ops.ema_update_segments(e, pd, segs, w, clip_state=state)              # a clipped one: the average of the parameters, as always
        torch.cuda.synchronize()
        got = e.cpu()
        assert coef < 1.0 and torch.equal(_i32(got[mk]), _i32(want[mk])) and torch.equal(_i32(got[~mk]), _i32(e0[~mk])), name
    ops.ema_update_segments(e, pd, [], w)                                       # an empty table: nothing to launch
    ops.ema_update_segments(e, pd, [(5, 5)], w)
    torch.cuda.synchronize()
    assert torch.equal(_i32(e.cpu()), _i32(got))


LR, MU, WD, GS = 0.05, 0.9, 5e-4, 0.37


@pytest.mark.parametrize("offset", [0, 1], ids=["float4", "scalar"])
def test_fused_flat_step_is_the_plain_step_plus_the_average(offset):
    """tf_sgd_step_ema: p and m bit for bit those of tf_sgd_step / tf_sgd_step_clipped on copies of the same inputs (at the same alignment), e the
    reference on (e0, p after the step, w); two steps (momentum), a new weight each; with skip set nothing moves."""
    from test_gpu_grad_clip import _clipped_state, _skip_state
    from tinyfaces import ops
    N, _ = _tables()
    n = N + 3

    def operands():
        base = [torch.randn(n + 4, generator=torch.Generator().manual_seed(21 + k)).cuda() for k in range(4)]
        p, g, m, e = [t[offset:offset + n] for t in base]
        m.zero_()
        return p, g, m, e

    for clipped in (False, True):
        p, g, m, e = operands()
        rp, _, rm, _ = operands()
        assert torch.equal(p, rp) and p.data_ptr() % 16 == rp.data_ptr() % 16 == (4 * offset) % 16 == e.data_ptr() % 16
        kw = {}
        if clipped:
            state, coef = _clipped_state(g.clone(), [(0, n)], GS)
            kw = {"clip_state": state}
        p_start = p.clone()
        for step, w in enumerate(WEIGHTS[:2]):
            e_before = e.cpu()
            ops.sgd_step(p, g, m, LR, MU, WD, GS, ema=e, ema_weight=w, **kw)
            ops.sgd_step(rp, g, rm, LR, MU, WD, GS, **kw)
            torch.cuda.synchronize()
            assert torch.equal(_i32(p), _i32(rp)) and torch.equal(_i32(m), _i32(rm)), (clipped, step)
            assert torch.equal(_i32(e.cpu()), _i32(_fmaf_no_ties(e_before, p.cpu(), w))), (clipped, step)
        assert not torch.equal(p, p_start)
        p0, m0, e0 = p.clone(), m.clone(), e.clone()
        skip = _skip_state()
        ops.sgd_step(p, g, m, LR, MU, WD, GS, ema=e, ema_weight=WEIGHTS[0], clip_state=skip)
        torch.cuda.synchronize()
        assert torch.equal(_i32(p), _i32(p0)) and torch.equal(_i32(m), _i32(m0)) and torch.equal(_i32(e), _i32(e0)), clipped
        assert skip.skipped() == 1                                              # the fused forms only read the state
    report(f"ema_fused_flat[{'scalar' if offset else 'float4'}]", elements=n, clip_coef=coef)


def _table_names():
    return list(_tables()[1])


@pytest.mark.parametrize("name", _table_names())
def test_fused_segment_step_is_the_plain_segment_step_plus_the_average(name):
    from test_gpu_grad_clip import _clipped_state, _device_grad, _skip_state
    from tinyfaces import ops
    N, TABLES = _tables()
    segs = TABLES[name]
    mk = _mask(N, segs)
    for clipped in (False, True):
        p = torch.randn(N, generator=torch.Generator().manual_seed(31)).cuda()
        e = torch.randn(N, generator=torch.Generator().manual_seed(32)).cuda()
        g = _device_grad(N, segs, outside=0.0)
        m = torch.zeros(N).cuda()
        rp, rm = p.clone(), m.clone()
        p_start, e_start = p.cpu(), e.cpu()
        kw = {}
        if clipped:
            state, coef = _clipped_state(g, segs, GS)
            kw = {"clip_state": state}
        for step, w in enumerate(WEIGHTS[:2]):
            e_before = e.cpu()
            ops.sgd_step_segments(p, g, m, segs, LR, MU, WD, GS, ema=e, ema_weight=w, **kw)
            ops.sgd_step_segments(rp, g, rm, segs, LR, MU, WD, GS, **kw)
            torch.cuda.synchronize()
            assert torch.equal(_i32(p), _i32(rp)) and torch.equal(_i32(m), _i32(rm)), (name, clipped, step)
            got, want = e.cpu(), _fmaf_no_ties(e_before, p.cpu(), w)
            assert torch.equal(_i32(got[mk]), _i32(want[mk])), (name, clipped, step)
            assert torch.equal(_i32(got[~mk]), _i32(e_start[~mk])), (name, clipped, step)
        assert torch.equal(p.cpu()[~mk], p_start[~mk]) and not torch.equal(p.cpu()[mk], p_start[mk])
        p0, m0, e0 = p.clone(), m.clone(), e.clone()
        ops.sgd_step_segments(p, g, m, segs, LR, MU, WD, GS, ema=e, ema_weight=WEIGHTS[0], clip_state=_skip_state())
        torch.cuda.synchronize()
        assert torch.equal(_i32(p), _i32(p0)) and torch.equal(_i32(m), _i32(m0)) and torch.equal(_i32(e), _i32(e0)), (name, clipped)


@pytest.mark.parametrize("name", ["unaligned_empty_single", "300_aligned", "300_unaligned", "whole"])
def test_every_new_entry_point_writes_inside_its_operands_only(hip, name):
    """tests/redzone.py: parameters, gradient, momentum and average between 0xFF guard bands; after each of the three entries (the flat one on
    its 16-byte and on its scalar path) every guard is intact, the gradient is unchanged, the stand-alone entry leaves the parameters
    unchanged, and the table entries write nothing outside their ranges."""
    l = hip.lib()
    N, TABLES = _tables()
    segs = TABLES[name]
    nseg = len(segs)
    table = (hip.i64 * (2 * nseg))(*[v for se in segs for v in se])
    mk = _mask(N, segs).cuda()
    host = [torch.randn(N, generator=torch.Generator().manual_seed(40 + k)) for k in range(4)]
    p, g, m, e = [guarded_like(t, "cuda") for t in host]
    g0 = g.clone()
    s = torch.cuda.current_stream().cuda_stream
    w = WEIGHTS[1]

    def everything(what):
        torch.cuda.synchronize()
        for t, label in ((p, "parameters"), (g, "gradient"), (m, "momentum"), (e, "average")):
            assert_guards(t, f"{what}: {label}")
        assert torch.equal(_i32(g), _i32(g0)), what

    p0, m0, e0 = p.clone(), m.clone(), e.clone()
    assert l.tf_ema_update_segments(e.data_ptr(), p.data_ptr(), table, nseg, w, None, s) == 0
    everything("tf_ema_update_segments")
    assert torch.equal(_i32(p), _i32(p0)) and torch.equal(_i32(m), _i32(m0))
    assert torch.equal(_i32(e[~mk]), _i32(e0[~mk])) and not torch.equal(e[mk], e0[mk])
    e1 = e.clone()
    assert l.tf_sgd_step_segments_ema(p.data_ptr(), g.data_ptr(), m.data_ptr(), e.data_ptr(), table, nseg, 0.05, 0.9, 5e-4, 1.0, w, None, s) == 0
    everything("tf_sgd_step_segments_ema")
    for t, t0 in ((p, p0), (m, m0), (e, e1)):
        assert torch.equal(_i32(t[~mk]), _i32(t0[~mk])) and not torch.equal(t[mk], t0[mk])
    assert l.tf_sgd_step_ema(p.data_ptr(), g.data_ptr(), m.data_ptr(), e.data_ptr(), N, 0.05, 0.9, 5e-4, 1.0, w, None, s) == 0
    everything("tf_sgd_step_ema")
    assert l.tf_sgd_step_ema(p.data_ptr() + 4, g.data_ptr() + 4, m.data_ptr() + 4, e.data_ptr() + 4, N - 1, 0.05, 0.9, 5e-4, 1.0, w, None, s) == 0
    everything("tf_sgd_step_ema, scalar path")
    assert torch.isfinite(p).all() and torch.isfinite(m).all() and torch.isfinite(e).all()


def test_drop_in_against_torchs_averaged_model():
    """Five parameter vectors fed in turn to AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(0.999)) on the CPU and to the device kernel with the
    warm-up off; the clone ModelEma takes at construction is AveragedModel's first, copying call.  Equal bit for bit after every update."""
    from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn
    from tinyfaces import ops
    from tinyfaces.ema import ModelEma
    n = 40000
    gen = torch.Generator().manual_seed(51)
    vectors = [torch.randn(n, generator=gen) for _ in range(5)]
    net = torch.nn.Linear(n, 1, bias=False)
    avg = AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(0.999))
    sched = ModelEma.__new__(ModelEma)                                           # the schedule alone (no DetectionModel behind it)
    sched.decay, sched.warmup, sched.updates = 0.999, False, 0
    e = None
    for k, v in enumerate(vectors):
        with torch.no_grad():
            net.weight.copy_(v.view(1, n))
        avg.update_parameters(net)
        if k == 0:
            e = v.clone().cuda()
        else:
            before = e.cpu()
            w = sched.next_weight()
            ops.ema_update_segments(e, v.cuda(), [(0, n)], w)
            torch.cuda.synchronize()
            assert torch.equal(_i32(e.cpu()), _i32(_fmaf_no_ties(before, v, w))), k
        assert torch.equal(_i32(e.cpu()), _i32(avg.module.weight.detach().view(-1))), k
    assert sched.updates == 4 and int(avg.n_averaged) == 5
    report("ema_vs_averaged_model", updates=4, elements=n)


# ---------------------------------------------------------------------------------------------------------------- engine level
def _trained_mask(m):
    seg = m._segments
    names = set(m.trainable_parameter_names())
    mk = torch.zeros(m._flat_params.numel(), dtype=torch.bool)
    for k in names:
        mk[seg[k][0]:seg[k][0] + seg[k][1]] = True
    return mk, sorted((seg[k][0], seg[k][0] + seg[k][1]) for k in names)


@pytest.mark.parametrize("frozen", [False, True], ids=["batch_stats", "frozen_bn_k2"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_engine_averages_inside_its_sgd_launches(dtype, frozen):
    """ResNet-50, 2 x 3 x 256 x 256, ema_decay 0.999 with the warm-up, three steps: after each the average of the trained tensors is the reference
    on (the average before, flat_p after, w_t) and everything else still holds the initial parameters; flat_p and flat_m are what the EXISTING
    ops give on (p0, m0, the gradient left in the persistent buffer).  Then the guard: a NaN planted behind the backward pass leaves parameters,
    momentum and average bit-identical, and the next clean step moves all three."""
    from test_gpu_frozen_bn import _oracle, _product
    from test_gpu_grad_clip import _engine_inputs
    from tinyfaces import ops
    from tinyfaces.ema import ema_decay_at
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.loss import DetectionCriterion
    m = _product(_oracle("resnet50", seed=6), "resnet50").set_compute_dtype(dtype)
    if frozen:
        m.freeze_batchnorm().set_trainable_layers(2)
    lr, mu, wd = 1e-3, 0.9, 5e-4
    eng = TrainEngine(m, DetectionCriterion(25), lr=lr, momentum=mu, weight_decay=wd, device="cuda", ema_decay=0.999)
    ema = eng.ema
    x, cm, rm = _engine_inputs()
    gflat = m._grad_flat_persistent
    mk, trained = _trained_mask(m)
    p_init = eng.flat_p.cpu()
    assert ema.updates == 0 and ema.flat.data_ptr() != eng.flat_p.data_ptr() and torch.equal(_i32(ema.flat.cpu()), _i32(p_init))
    tag = f"engine_ema[{'bf16' if dtype == torch.bfloat16 else 'fp32'},{'frozen_k2' if frozen else 'batch_stats'}]"
    ties_seen = 0
    for t in range(3):
        p0, m0, e0 = eng.flat_p.clone(), eng.flat_m.clone(), ema.flat.cpu()
        eng.step(x, cm.clone(), rm)
        torch.cuda.synchronize()
        w = float(np.float32(1.0 - ema_decay_at(0.999, t)))
        rp, rmom = p0.clone(), m0.clone()
        for a, b, mult in eng.groups:
            if mult == 0.0:
                continue
            if frozen:
                ops.sgd_step_segments(rp, gflat, rmom, [(max(s, a), min(e, b)) for s, e in trained if e > a and s < b], lr * mult, mu, wd, 1.0)
            else:
                ops.sgd_step(rp[a:b], gflat[a:b], rmom[a:b], lr * mult, mu, wd, 1.0)
        torch.cuda.synchronize()
        assert torch.equal(_i32(eng.flat_p), _i32(rp)) and torch.equal(_i32(eng.flat_m), _i32(rmom)), t
        assert not torch.equal(eng.flat_p, p0)
        ref, ties = _fmaf(e0, eng.flat_p.cpu(), w)
        ties_seen += ties
        want = p_init.clone()
        want[mk] = ref[mk]
        got = ema.flat.cpu()
        assert torch.equal(_i32(got), _i32(want)), t
        moved = int((_i32(got[mk]) != _i32(e0[mk])).sum())
        report(tag, step=t, w=w, trained_elements=int(mk.sum()), moved=moved, halfway_cases=ties)
        assert moved > 0
    assert ema.updates == 3 and eng.steps == 3

    # ---- the guard
    eng.skip_nonfinite = True
    victim = m._segments["model.layer3.1.conv2.weight"][0] + 5
    run_backward, plant = m._run_backward, [True]

    def planted(xx, grad, persistent=False):
        out = run_backward(xx, grad, persistent=persistent)
        if plant[0]:
            out[victim] = float("nan")                                        # behind the real backward pass, on the training stream
        return out

    m._run_backward = planted
    try:
        p1, m1, e1 = eng.flat_p.clone(), eng.flat_m.clone(), ema.flat.clone()
        eng.step(x, cm.clone(), rm)
        torch.cuda.synchronize()
        assert eng.skipped_steps == 1
        assert torch.equal(_i32(eng.flat_p), _i32(p1)) and torch.equal(_i32(eng.flat_m), _i32(m1)) and torch.equal(_i32(ema.flat), _i32(e1))
        assert ema.updates == 4                                                 # indexed by steps taken: the host does not know
        plant[0] = False
        eng.step(x, cm.clone(), rm)
        torch.cuda.synchronize()
    finally:
        m._run_backward = run_backward
    assert eng.skipped_steps == 1 and ema.updates == 5
    assert not torch.equal(eng.flat_p, p1) and not torch.equal(eng.flat_m, m1) and not torch.equal(ema.flat, e1)
    w = float(np.float32(1.0 - ema_decay_at(0.999, 4)))
    ref, _ = _fmaf(e1.cpu(), eng.flat_p.cpu(), w)
    want = p_init.clone()
    want[mk] = ref[mk]
    assert torch.equal(_i32(ema.flat.cpu()), _i32(want))
    assert torch.isfinite(ema.flat).all()
    eng.close()


@pytest.mark.parametrize("frozen", [False, True], ids=["batch_stats", "frozen_bn"])
def test_default_engine_has_no_average_and_calls_nothing_new(monkeypatch, frozen):
    from test_gpu_frozen_bn import _oracle, _product
    from test_gpu_grad_clip import _engine_inputs
    from tinyfaces import _hip, ops
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.loss import DetectionCriterion
    m = _product(_oracle("resnet50", seed=6), "resnet50").set_compute_dtype(torch.bfloat16).freeze_batchnorm(frozen)
    eng = TrainEngine(m, DetectionCriterion(25), lr=1e-3, device="cuda")
    assert eng.ema is None
    seen, new_calls = [], []
    for name in ("sgd_step", "sgd_step_segments"):
        def spy(*a, _f=getattr(ops, name), _n=name, **kw):
            seen.append((_n, len(a), sorted(kw)))
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, spy)
    l = _hip.lib()
    for name in ("tf_sgd_step_ema", "tf_sgd_step_segments_ema", "tf_ema_update_segments"):
        def entry(*a, _f=getattr(l, name), _n=name):
            new_calls.append(_n)
            return _f(*a)
        monkeypatch.setattr(l, name, entry)
    x, cm, rm = _engine_inputs()
    p0 = eng.flat_p.clone()
    eng.step(x, cm.clone(), rm)
    torch.cuda.synchronize()
    assert [c[0] for c in seen] == ["sgd_step_segments" if frozen else "sgd_step"] * 3
    assert all(c[1] == (8 if frozen else 7) and c[2] == [] for c in seen)      # positional arguments only, as before
    assert new_calls == [] and not torch.equal(eng.flat_p, p0)
    # ... and the spies do see the feature when it is on
    eng2 = TrainEngine(_product(_oracle("resnet50", seed=6), "resnet50").set_compute_dtype(torch.bfloat16).freeze_batchnorm(frozen),
                       DetectionCriterion(25), lr=1e-3, device="cuda", ema_decay=0.999)
    del seen[:]
    eng2.step(x, cm.clone(), rm)
    torch.cuda.synchronize()
    assert all(c[2] == ["ema", "ema_weight"] for c in seen) and len(seen) == 3
    assert new_calls == ["tf_sgd_step_segments_ema" if frozen else "tf_sgd_step_ema"] * 3
    eng.close()
    eng2.close()


def test_state_dict_export_loads_into_a_fresh_model_and_evaluates():
    from test_gpu_frozen_bn import _oracle, _product
    from test_gpu_grad_clip import _engine_inputs
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as zoo
    from tinyfaces.models.loss import DetectionCriterion
    m = _product(_oracle("resnet50", seed=6), "resnet50").set_compute_dtype(torch.float32)
    eng = TrainEngine(m, DetectionCriterion(25), lr=1e-3, device="cuda", ema_decay=0.9, ema_warmup=False)
    x, cm, rm = _engine_inputs()
    for _ in range(2):
        eng.step(x, cm.clone(), rm)
    torch.cuda.synchronize()
    ema, seg = eng.ema, m._segments
    live, sd = m.state_dict(), ema.state_dict()
    assert list(sd) == list(live) and all(sd[k].shape == live[k].shape and sd[k].dtype == live[k].dtype for k in live)
    params = {k for k, _ in m.named_parameters()}
    differ = 0
    for k in live:
        if k in seg:
            o, n = seg[k]
            assert k in params and torch.equal(_i32(sd[k].reshape(-1)), _i32(ema.flat[o:o + n])), k
            assert sd[k].data_ptr() != ema.flat[o:o + n].data_ptr()
            differ += not torch.equal(sd[k], live[k])
        else:
            assert torch.equal(sd[k], live[k]), k                               # buffers (and anything the executor does not train): the live model's
    assert differ >= len(m.trainable_parameter_names()) - 1
    assert sum(k.endswith("running_mean") for k in sd) > 0 and any(int(sd[k]) == 2 for k in sd if k.endswith("num_batches_tracked"))

    img = torch.randn(1, 3, 128, 128, generator=torch.Generator().manual_seed(8)).cuda()

    def fresh():
        return zoo.DetectionModel(base_model=zoo.resnet50, num_templates=25).set_compute_dtype(torch.float32)

    a = fresh()
    a.load_state_dict(sd)
    b = fresh()
    b.load_state_dict(live)
    with torch.no_grad():
        for k, pm in b.named_parameters():
            if k in seg:
                o, n = seg[k]
                pm.copy_(ema.flat[o:o + n].view(pm.shape).cpu())                # the averaged parameters, copied by hand
    c = fresh()
    c.load_state_dict(live)
    ema.copy_to(c)
    outs = []
    with torch.no_grad():
        for net in (a, b, c, m):
            outs.append(net.cuda().eval()(img).float().cpu())
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(_i32(outs[0]), _i32(outs[1])) and torch.equal(_i32(outs[0]), _i32(outs[2]))
    assert not torch.equal(outs[0], outs[3])                                    # (the live weights give another map)
    report("ema_export", keys=len(sd), tensors_that_differ=differ, map_abs_max=float(outs[0].abs().max()))
    # round trip through load_state_dict
    m.train()
    keep = ema.flat.clone()
    ema.flat.zero_()
    ema.load_state_dict({k: v.cpu() for k, v in sd.items()}, 7)
    assert ema.updates == 7 and torch.equal(_i32(ema.flat), _i32(keep))
    eng.close()


def test_trainer_updates_the_average_behind_every_optimizer_step(golden):
    """fp32, ResNet-50, the two batches of tests/golden/trainer.npz through trainer.train(..., ema=ModelEma(...)) and torch.optim.SGD.  The
    optimizer is built BEFORE ModelEma flattens the model and still updates the same nn.Parameters; after each optimizer.step() the average
    is the reference on the parameters torch left."""
    from test_gpu_frozen_bn import _golden_batches, _keep, _oracle, _product
    from tinyfaces import trainer
    from tinyfaces.ema import ModelEma, ema_decay_at
    from tinyfaces.models.loss import DetectionCriterion
    dev = torch.device("cuda")
    m = _product(_oracle("resnet50", seed=9), "resnet50").set_compute_dtype(torch.float32).to(dev).train()
    c = DetectionCriterion(25)
    c.inject_sampling(_keep(), _keep())
    opt = torch.optim.SGD(m.learnable_parameters(1e-3), lr=1e-3, momentum=0.9, weight_decay=5e-4)
    held = [p for g in opt.param_groups for p in g["params"]]
    assert getattr(m, "_flat_params", None) is None
    ema = ModelEma(m, 0.999)
    flat = m._flat_params
    assert all(a is b for a, b in zip(held, [p for g in m.learnable_parameters(1e-3) for p in g["params"]]))      # identity kept
    assert torch.equal(_i32(ema.flat), _i32(flat)) and ema.flat.data_ptr() != flat.data_ptr()
    mk, _ = _trained_mask(m)
    init = flat.cpu()
    snaps, update = [], ema.update

    def spy():
        before, params = ema.flat.cpu(), flat.cpu()
        update()
        torch.cuda.synchronize()
        snaps.append((before, params, ema.flat.cpu()))

    ema.update = spy
    with redirect_stdout(io.StringIO()):
        trainer.train(m, c, opt, _golden_batches(golden), 0, dev, ema=ema)
    assert len(snaps) == 2 and ema.updates == 2 and m._flat_params is flat
    last = init
    for t, (before, params, after) in enumerate(snaps):
        w = float(np.float32(1.0 - ema_decay_at(0.999, t)))
        assert not torch.equal(params[mk], last[mk])                            # torch.optim.SGD moved the flat buffer through the held Parameters
        ref, ties = _fmaf(before, params, w)
        want = init.clone()
        want[mk] = ref[mk]
        assert torch.equal(_i32(after), _i32(want)), t
        report("ema_trainer[resnet50,fp32]", step=t, w=w, halfway_cases=ties, moved=int((_i32(after) != _i32(before)).sum()))
        last = params
    # a model whose parameters left the flat buffer is refused
    m.flatten_parameters()
    with pytest.raises(RuntimeError, match="no longer live"):
        update()


def test_two_ranks_hold_the_same_average(tmp_path):
    """2 gloo ranks sharing cuda:0 (tests/dist_worker_ema.py), two steps: both ranks' averages are bit-identical without a collective of their
    own, and each is the reference on that rank's own parameters."""
    from tinyfaces.ema import ema_decay_at
    golden = os.path.join(ROOT, "tests", "golden", "trainer.npz")
    out = str(tmp_path / "ema")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29583", os.path.join(ROOT, "tests", "dist_worker_ema.py"), golden, out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = [np.load(f"{out}.rank{k}.npz") for k in range(2)]
    mk = torch.from_numpy(got[0]["trained"])
    assert np.array_equal(got[0]["trained"], got[1]["trained"]) and int(mk.sum()) > 0
    for key in ("e_init", "e0", "e1", "p0", "p1"):
        assert np.array_equal(got[0][key].view(np.int32), got[1][key].view(np.int32)), key
    for k in range(2):
        init = torch.from_numpy(got[k]["e_init"])
        before = init
        for s in range(2):
            w = float(np.float32(1.0 - ema_decay_at(0.999, s)))
            p, e = torch.from_numpy(got[k][f"p{s}"]), torch.from_numpy(got[k][f"e{s}"])
            ref, ties = _fmaf(before, p, w)
            want = init.clone()
            want[mk] = ref[mk]
            assert torch.equal(_i32(e), _i32(want)), (k, s)
            assert not torch.equal(e[mk], before[mk])
            before = e
        assert int(got[k]["updates"]) == 2
    report("ema_dist_2_ranks[resnet50,k=1]", trained_elements=int(mk.sum()))


def test_scripts_store_the_average_and_evaluate_it(tmp_path):
    """main.py --model-ema for three steps in a fresh process, then evaluate_model.py --ema on its checkpoint.  The evaluation runs at
    --prob_thresh 0.9, as the other script tests raise theirs: three steps from random weights leave every score near 0.5, and at the
    default 0.03 all 2.36 M anchors of the pyramid are candidates, more than one NMS call takes (524 160).  What is checked is that the
    script finds the averaged weights in the checkpoint, runs them and writes its result file, whatever the count."""
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def run(args):
        r = subprocess.run([sys.executable] + args, cwd=tmp_path, capture_output=True, text=True, timeout=400, env=env)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        return r.stdout

    save = tmp_path / "ckpt"
    run([os.path.join(PKG, "main.py"), "synthetic", "synthetic", "--base-model", "resnet50", "--epochs", "1", "--synthetic-len", "6", "--batch_size", "2",
         "--save-every", "1", "--model-ema", "0.9", "--save-path", str(save)])
    state = torch.load(save / "checkpoint_1.pth", map_location="cpu")
    assert sorted(state) == ["batch_size", "ema", "epoch", "model", "model_ema", "optimizer"]
    assert state["ema"] == {"decay": 0.9, "warmup": True, "updates": 3}
    live, mean = state["model"], state["model_ema"]
    assert list(live) == list(mean) and all(live[k].shape == mean[k].shape for k in live)
    buffers = [k for k in live if k.rsplit(".", 1)[1] in ("running_mean", "running_var", "num_batches_tracked")]
    assert buffers and all(torch.equal(live[k], mean[k]) for k in buffers)
    from tinyfaces.models import model as zoo
    trained = zoo.DetectionModel(base_model=zoo.resnet50, num_templates=25).trainable_parameter_names()
    differ = sum(not torch.equal(live[k], mean[k]) for k in trained)
    report("ema_scripts", trained_tensors=len(trained), differ=differ)
    assert differ > 0.9 * len(trained)
    assert all(torch.isfinite(mean[k]).all() for k in trained)
    from tinyfaces.evaluation import get_model
    loaded = get_model(str(save / "checkpoint_1.pth"), 25, ema=True).state_dict()
    assert all(torch.equal(loaded[k], mean[k]) for k in mean)
    run([os.path.join(PKG, "evaluate_model.py"), "synthetic", "--ema", "--num-images", "1", "--checkpoint", str(save / "checkpoint_1.pth"),
         "--prob_thresh", "0.9"])
    lines = (tmp_path / "val_results" / "synthetic" / "img_0.txt").read_text().split("\n")
    assert lines[0] == "img_0.jpg" and int(lines[1]) == len([ln for ln in lines[2:] if ln.strip()])
