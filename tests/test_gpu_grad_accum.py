"""-m gpu: gradient accumulation (csrc/sgd.hip: grad_accumulate_kernel; ops.grad_accumulate; TrainEngine(accum_steps=, accum_average=) and
step(apply=); trainer.train(accum_steps=); tests/dist_worker_accum.py).

Where the bars come from:
  kernel   one fp32 add per element, acc on the left: bit for bit torch's own fp32 `a + b` on the host (IEEE round-to-nearest-even on both
           sides; no operand is a NaN inside the ranges, so no payload question arises).  The chain STORE, ADD, FINISH is ((g1 + g2) + g3).
           Every fifth element holds the triple (1, 2^-24, 2^-24): left to right both adds are ties that round to even, the sum is 1; g2 + g3
           first gives 1 + 2^-23, and so does a sum kept in higher precision.  The next one holds (1 + 2^-23, 2^-24, -2^-24): left to right the
           first tie rounds UP to 1 + 2^-22 and the sum ends at 1 + 2^-22; exact arithmetic gives 1 + 2^-23.
  engine   bit for bit: the accumulated gradient against torch's fp32 adds of the cloned micro-batch gradients in the same order, the
           parameters and the momentum against the EXISTING ops on that sum from the state before the window.
  window   a window of two micro-batches against the batch of their four images, frozen BatchNorm, fp32, every label kept: relative L2 error
           of the flat gradient <= 1e-3, the project's fp32 bar (a mean taken for a sum, or a dropped micro-batch, gives >= 0.3).
  ranks    the bounds of tests/test_gpu_trainable_layers.py's two-rank test: first window < 1e-5, last < 1e-2.
Measured values go through gpu_util.report."""
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
TRIP = 2048 * 256 * 4                                      # what one trip of the capped grid covers
LONG = TRIP + 1028                                         # ... so this range takes a second trip
PITCH = 256 * 4 * 4                                        # the bytes one block moves per trip: the guards hold 384 of them on either side


def _i32(t):
    return t.contiguous().view(torch.int32)


def _cases():
    """(name, buffer length, ranges, element offset of both bases).  The five tables of tests/test_gpu_grad_clip.py (an empty range, single
    unaligned elements, 300 ranges = three launches on the 16-byte and on the scalar path), one range of 300 elements aligned and not,
    bases one element off a 16-byte boundary, and the grid-stride loop's second trip on both paths."""
    from test_gpu_grad_clip import N, TABLES
    cases = [(name, N, segs, 0) for name, segs in TABLES.items()]
    cases += [("one_300_aligned", 512, [(0, 300)], 0), ("one_300_unaligned", 512, [(1, 301)], 0), ("single", 64, [(17, 18)], 0)]
    cases += [("base_off_by_one", N, TABLES["aligned"], 1), ("base_off_by_one_300", N, TABLES["300_aligned"], 1)]
    cases += [("second_trip_aligned", LONG + 8, [(0, LONG)], 0), ("second_trip_scalar", LONG + 8, [(3, LONG + 3)], 0)]
    return cases


CASES = _cases()
_HOST = {}


def _host(n):
    """(g1, g2, g3) on the host, computed once per size and left unchanged: values of order 1 with a few large and a few tiny ones, and the
    planted triples of the module docstring."""
    if n not in _HOST:
        gen = torch.Generator().manual_seed(n % 1000 + 7)
        g = [torch.randn(n, generator=gen) for _ in range(3)]
        g[0][::97] *= 1e3
        g[1][5::89] *= 1e-6
        tie = 2.0 ** -24
        for k, triple in ((0, (1.0, tie, tie)), (1, (1.0 + 2.0 ** -23, tie, -tie))):
            for t, v in zip(g, triple):
                t[k::5] = v
        assert float((g[0][0] + g[1][0]) + g[2][0]) == 1.0 and float(g[0][0] + (g[1][0] + g[2][0])) == 1.0 + 2.0 ** -23
        assert float((g[0][1] + g[1][1]) + g[2][1]) == 1.0 + 2.0 ** -22
        _HOST[n] = tuple(g)
    return _HOST[n]


def _mask(n, segs):
    mk = torch.zeros(n, dtype=torch.bool)
    for a, b in segs:
        mk[a:b] = True
    return mk


def _device_pair(n, offset):
    """(acc, grad) of n elements on the device, `offset` elements into their allocations."""
    return tuple(torch.zeros(n + 4).cuda()[offset:offset + n] for _ in range(2))


@pytest.mark.parametrize("name,n,segs,offset", CASES, ids=[c[0] for c in CASES])
def test_kernel_is_torchs_fp32_add_bit_for_bit_in_every_mode_and_touches_nothing_else(name, n, segs, offset):
    """STORE, ADD, FINISH in turn.  After each: the destination is the host's fp32 sum (for STORE: the gradient) inside the ranges, the other
    operand is unchanged everywhere, and outside the ranges both still hold the NaN pattern they were given, which neither a read nor a
    write has touched (a NaN read into a sum would show inside the ranges).  The accumulator is all NaN before STORE: none survives."""
    from tinyfaces import ops
    g1, g2, g3 = _host(n)
    mk = _mask(n, segs)
    nan = torch.full((n,), float("nan"))
    acc, grad = _device_pair(n, offset)
    assert (acc.data_ptr() % 16 == 0) == (offset == 0) and (grad.data_ptr() % 16 == 0) == (offset == 0)
    acc.copy_(nan)                                                              # whatever an earlier window left, a NaN included

    def load(g):
        src = torch.where(mk, g, nan)
        grad.copy_(src)
        return src

    def check(stage, want_acc, want_grad):
        torch.cuda.synchronize()
        got_acc, got_grad = acc.cpu(), grad.cpu()
        assert torch.equal(_i32(got_acc), _i32(torch.where(mk, want_acc, nan))), (name, stage, "acc")
        assert torch.equal(_i32(got_grad), _i32(torch.where(mk, want_grad, nan))), (name, stage, "grad")

    load(g1)
    ops.grad_accumulate(acc, grad, segs, ops.ACCUM_STORE)
    check("store", g1, g1)
    assert not torch.isnan(acc.cpu()[mk]).any()
    load(g2)
    ops.grad_accumulate(acc, grad, segs, ops.ACCUM_ADD)
    s12 = g1 + g2
    check("add", s12, g2)
    load(g3)
    ops.grad_accumulate(acc, grad, segs, ops.ACCUM_FINISH)
    s123 = s12 + g3
    check("finish", s12, s123)
    planted = int((_i32(s123) != _i32(g1 + (g2 + g3)))[mk].sum())
    report(f"grad_accumulate[{name}]", elements=int(mk.sum()), ranges=len(segs), order_sensitive=planted)
    assert planted > 0 or int(mk.sum()) < 8                                      # the data can tell another order apart


def test_empty_tables_launch_nothing():
    from tinyfaces import ops
    acc, grad = torch.full((64,), float("nan")).cuda(), torch.ones(64).cuda()
    for mode in (ops.ACCUM_STORE, ops.ACCUM_ADD, ops.ACCUM_FINISH):
        for segs in ([], [(5, 5), (9, 9)]):
            ops.grad_accumulate(acc, grad, segs, mode)
    torch.cuda.synchronize()
    assert torch.isnan(acc).all() and bool((grad == 1).all())
    with pytest.raises(ValueError, match="mode"):
        ops.grad_accumulate(acc, grad, [(0, 8)], 3)
    with pytest.raises(ValueError, match="out of order"):
        ops.grad_accumulate(acc, grad, [(8, 16), (0, 4)], ops.ACCUM_ADD)
    with pytest.raises(ValueError, match="outside"):
        ops.grad_accumulate(acc, grad, [(60, 68)], ops.ACCUM_ADD)


@pytest.mark.parametrize("name,n,segs,offset", CASES, ids=[c[0] for c in CASES])
def test_every_mode_writes_inside_its_operands_only(hip, name, n, segs, offset):
    """tests/redzone.py: accumulator and gradient between 0xFF guard bands, on the tables of the test above; after every mode both pairs of
    guards are intact.  `offset` moves both bases one element into their bodies (the scalar path), the table then spans one element less."""
    l = hip.lib()
    g1, g2, _ = _host(n)
    acc, grad = guarded_like(g1, "cuda", pitch_bytes=PITCH), guarded_like(g2, "cuda", pitch_bytes=PITCH)
    segs = [(a, min(b, n - offset)) for a, b in segs if a < n - offset]
    table = (hip.i64 * (2 * len(segs)))(*[v for se in segs for v in se])
    s = torch.cuda.current_stream().cuda_stream
    for mode in (hip.TF_ACCUM_STORE, hip.TF_ACCUM_ADD, hip.TF_ACCUM_FINISH):
        assert l.tf_grad_accumulate_segments(acc.data_ptr() + 4 * offset, grad.data_ptr() + 4 * offset, table, len(segs), mode, s) == 0
        torch.cuda.synchronize()
        assert_guards(acc, f"{name}, mode {mode}: accumulator")
        assert_guards(grad, f"{name}, mode {mode}: gradient")
    mk = _mask(n, [(a + offset, b + offset) for a, b in segs])
    want = torch.where(mk, (g2 + g2) + g2, g2)                                  # STORE g2, ADD g2, FINISH: (g2 + g2) + g2 inside, g2 outside
    assert torch.equal(_i32(grad.cpu()), _i32(want)), name
    assert torch.equal(_i32(acc.cpu()), _i32(torch.where(mk, g2 + g2, g1))), name


# ---------------------------------------------------------------------------------------------------------------- engine level
def _trained_mask(m):
    seg = m._segments
    names = set(m.trainable_parameter_names())
    mk = torch.zeros(m._flat_params.numel(), dtype=torch.bool)
    for k in names:
        mk[seg[k][0]:seg[k][0] + seg[k][1]] = True
    return mk, sorted((seg[k][0], seg[k][0] + seg[k][1]) for k in names)


def _recording(m):
    """Wrap m._run_backward as the EMA test's `planted` does: clone every micro-batch's gradient behind the real backward pass."""
    run_backward, seen = m._run_backward, []

    def recorded(xx, grad, persistent=False):
        out = run_backward(xx, grad, persistent=persistent)
        seen.append(out.clone() if persistent else [v.clone() for v in out])
        return out

    m._run_backward = recorded
    return seen, run_backward


def _reference_update(eng, p0, m0, gsum, trained, frozen, lr, mu, wd, scale):
    """What the EXISTING ops give on `gsum` from (p0, m0): the plain launches of TrainEngine._sgd."""
    from tinyfaces import ops
    rp, rmom = p0.clone(), m0.clone()
    for a, b, mult in eng.groups:
        if mult == 0.0:
            continue
        if frozen:
            ops.sgd_step_segments(rp, gsum, rmom, [(max(s, a), min(e, b)) for s, e in trained if e > a and s < b], lr * mult, mu, wd, scale)
        else:
            ops.sgd_step(rp[a:b], gsum[a:b], rmom[a:b], lr * mult, mu, wd, scale)
    torch.cuda.synchronize()
    return rp, rmom


@pytest.mark.parametrize("frozen", [False, True], ids=["batch_stats", "frozen_bn_k2"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_engine_applies_the_left_to_right_sum_once_per_window(dtype, frozen):
    """ResNet-50, 2 x 3 x 256 x 256, accum_steps = 3 with the model EMA on, two windows, then a window cut short by apply=True with
    accum_average."""
    from test_gpu_frozen_bn import _oracle, _product
    from test_gpu_grad_clip import _engine_inputs
    from test_gpu_model_ema import _fmaf
    from tinyfaces.ema import ema_decay_at
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.loss import DetectionCriterion
    m = _product(_oracle("resnet50", seed=6), "resnet50").set_compute_dtype(dtype)
    if frozen:
        m.freeze_batchnorm().set_trainable_layers(2)
    lr, mu, wd = 1e-3, 0.9, 5e-4
    eng = TrainEngine(m, DetectionCriterion(25), lr=lr, momentum=mu, weight_decay=wd, device="cuda", ema_decay=0.999, accum_steps=3)
    assert eng._accum is None and (eng.steps, eng.micro_steps, eng.pending_micro_batches) == (0, 0, 0)
    ema = eng.ema
    x, cm, rm = _engine_inputs()
    xs = [x, x.flip(3), x * 0.5]                                                # three different micro-batches
    gflat = m._grad_flat_persistent
    mk, trained = _trained_mask(m)
    mkd = mk.cuda()
    seen, run_backward = _recording(m)
    tag = f"engine_accum[{'bf16' if dtype == torch.bfloat16 else 'fp32'},{'frozen_k2' if frozen else 'batch_stats'}]"
    try:
        for window in range(2):
            p0, m0, e0 = eng.flat_p.clone(), eng.flat_m.clone(), ema.flat.clone()
            del seen[:]
            for k in range(2):
                eng.step(xs[k], cm.clone(), rm)
                torch.cuda.synchronize()
                assert torch.equal(_i32(eng.flat_p), _i32(p0)) and torch.equal(_i32(eng.flat_m), _i32(m0)) and torch.equal(_i32(ema.flat), _i32(e0))
                assert (eng.steps, eng.micro_steps, eng.pending_micro_batches, ema.updates) == (window, 3 * window + k + 1, k + 1, window)
            with pytest.raises(RuntimeError, match="micro-batches"):
                eng.optimizer_state_dict()
            eng.step(xs[2], cm.clone(), rm)
            torch.cuda.synchronize()
            g1, g2, g3 = seen
            gsum = (g1 + g2) + g3
            assert not torch.equal(g1[mkd], g2[mkd]) and not torch.equal(g2[mkd], g3[mkd])
            assert torch.equal(_i32(gflat[mkd]), _i32(gsum[mkd])), window
            rp, rmom = _reference_update(eng, p0, m0, gsum, trained, frozen, lr, mu, wd, 1.0)
            assert torch.equal(_i32(eng.flat_p), _i32(rp)) and torch.equal(_i32(eng.flat_m), _i32(rmom)), window
            assert not torch.equal(eng.flat_p, p0)
            assert (eng.steps, eng.micro_steps, eng.pending_micro_batches, ema.updates) == (window + 1, 3 * window + 3, 0, window + 1)
            ref, ties = _fmaf(e0.cpu(), eng.flat_p.cpu(), float(np.float32(1.0 - ema_decay_at(0.999, window))))
            assert torch.equal(_i32(ema.flat.cpu()[mk]), _i32(ref[mk])) and torch.equal(_i32(ema.flat.cpu()[~mk]), _i32(e0.cpu()[~mk])), window
            order = int((_i32(gsum[mkd]) != _i32(g1[mkd] + (g2[mkd] + g3[mkd]))).sum())
            report(tag, window=window, trained_elements=int(mk.sum()), elements_another_order_would_change=order, halfway_cases=ties)
        assert int(m.model.bn1.num_batches_tracked) == (0 if frozen else 6)                             # running statistics advance with every micro-batch
        assert len(eng.optimizer_state_dict()["state"]) > 0                     # no window is open

        # ---- the end of an epoch: two micro-batches of three, applied now, as their mean
        eng.accum_average = True
        p0, m0 = eng.flat_p.clone(), eng.flat_m.clone()
        del seen[:]
        eng.step(xs[0], cm.clone(), rm)
        eng.step(xs[1], cm.clone(), rm, apply=True)
        torch.cuda.synchronize()
        g1, g2 = seen
        gsum = g1 + g2
        assert torch.equal(_i32(gflat[mkd]), _i32(gsum[mkd]))
        rp, rmom = _reference_update(eng, p0, m0, gsum, trained, frozen, lr, mu, wd, float(np.float32(1.0 / 2)))
        assert torch.equal(_i32(eng.flat_p), _i32(rp)) and torch.equal(_i32(eng.flat_m), _i32(rmom))
        assert (eng.steps, eng.micro_steps, eng.pending_micro_batches, ema.updates) == (3, 8, 0, 3)
        eng.step(xs[0], cm.clone(), rm, apply=False)
        eng.step(xs[1], cm.clone(), rm, apply=False)
        with pytest.raises(ValueError, match="fills the window"):
            eng.step(xs[2], cm.clone(), rm, apply=False)
        assert eng.pending_micro_batches == 2 and eng.micro_steps == 10           # the refused call did no work
    finally:
        m._run_backward = run_backward
    eng.close()


def test_a_nan_in_any_micro_batch_skips_the_window_and_the_next_one_starts_clean():
    from test_gpu_frozen_bn import _oracle, _product
    from test_gpu_grad_clip import _engine_inputs
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.loss import DetectionCriterion
    m = _product(_oracle("resnet50", seed=6), "resnet50").set_compute_dtype(torch.bfloat16)
    eng = TrainEngine(m, DetectionCriterion(25), lr=1e-3, device="cuda", skip_nonfinite=True, ema_decay=0.999, accum_steps=2)
    x, cm, rm = _engine_inputs()
    victim = m._segments["model.layer3.1.conv2.weight"][0] + 5
    run_backward, calls = m._run_backward, [0]

    def planted(xx, grad, persistent=False):
        out = run_backward(xx, grad, persistent=persistent)
        calls[0] += 1
        if calls[0] == 1:
            out[victim] = float("nan")                                            # micro-batch 1 of the first window, behind the real backward pass
        return out

    m._run_backward = planted
    try:
        p0, m0, e0 = eng.flat_p.clone(), eng.flat_m.clone(), eng.ema.flat.clone()
        eng.step(x, cm.clone(), rm)
        eng.step(x.flip(3), cm.clone(), rm)
        torch.cuda.synchronize()
        assert torch.isfinite(m._grad_flat_persistent[victim - 5:victim]).all() and torch.isnan(m._grad_flat_persistent[victim])
        assert eng.skipped_steps == 1 and (eng.steps, eng.micro_steps) == (1, 2)
        assert torch.equal(_i32(eng.flat_p), _i32(p0)) and torch.equal(_i32(eng.flat_m), _i32(m0)) and torch.equal(_i32(eng.ema.flat), _i32(e0))
        eng.step(x, cm.clone(), rm)
        eng.step(x.flip(3), cm.clone(), rm)
        torch.cuda.synchronize()
    finally:
        m._run_backward = run_backward
    assert eng.skipped_steps == 1 and (eng.steps, eng.micro_steps) == (2, 4)
    assert not torch.equal(eng.flat_p, p0) and not torch.equal(eng.flat_m, m0) and not torch.equal(eng.ema.flat, e0)
    assert torch.isfinite(eng.flat_p).all() and torch.isfinite(eng.flat_m).all() and torch.isfinite(eng.ema.flat).all()
    assert torch.isfinite(m._grad_flat_persistent).all()                        # STORE left nothing of the first window behind
    eng.close()


def test_a_window_of_two_micro_batches_is_the_step_of_the_four_image_batch():
    """Frozen BatchNorm, fp32, ohem_thresh = 0, every label kept (sampling injected as tests/dist_worker_trunks.py does): the accumulated gradient
    of (b0, b1) against the gradient of ONE plain engine on [b0; b1].  <= 1e-3 relative L2 over the trained ranges."""
    import dist_worker_trunks
    from tinyfaces.engine import TrainEngine
    golden = os.path.join(ROOT, "tests", "golden", "trainer.npz")

    def engine(images, **kw):
        m, c, batches = dist_worker_trunks.build(golden)
        m.freeze_batchnorm()
        c.ohem_thresh = 0.0
        E = 25 * batches[0][1].shape[2] * batches[0][1].shape[3]
        keep = torch.ones(images, E, dtype=torch.uint8)
        c.inject_sampling(keep, keep)
        return TrainEngine(m, c, lr=1e-4, device="cuda", **kw), [[t.cuda() for t in b] for b in batches]

    acc, batches = engine(2, accum_steps=2)
    big, _ = engine(4)
    for img, cm, rm in batches:
        acc.step(img, cm.clone(), rm)
    img, cm, rm = [torch.cat([batches[0][k], batches[1][k]]) for k in range(3)]
    big.step(img, cm.clone(), rm)
    torch.cuda.synchronize()
    assert (acc.steps, acc.micro_steps, big.steps) == (1, 2, 1)
    mk, _ = _trained_mask(acc.model)
    mk = mk.cuda()
    ga, gb = acc.model._grad_flat_persistent[mk].double(), big.model._grad_flat_persistent[mk].double()
    rel = float((ga - gb).norm() / gb.norm())
    pa, pb = acc.flat_p[mk].double(), big.flat_p[mk].double()
    report("accum_window_vs_big_batch[resnet50,fp32,frozen]", grad_rel_l2=rel, param_max_abs=float((pa - pb).abs().max()),
           trained_elements=int(mk.sum()))
    print("accum window vs 4-image batch: grad rel L2", rel)
    assert float(gb.norm()) > 0.0 and rel <= 1e-3, rel
    acc.close()
    big.close()


@pytest.mark.parametrize("frozen", [False, True], ids=["batch_stats", "frozen_bn"])
def test_default_engine_allocates_no_accumulator_and_calls_nothing_new(monkeypatch, frozen):
    from test_gpu_frozen_bn import _oracle, _product
    from test_gpu_grad_clip import _engine_inputs
    from tinyfaces import _hip, ops
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.loss import DetectionCriterion

    def model():
        return _product(_oracle("resnet50", seed=6), "resnet50").set_compute_dtype(torch.bfloat16).freeze_batchnorm(frozen)

    eng = TrainEngine(model(), DetectionCriterion(25), lr=1e-3, device="cuda")
    seen, modes = [], []
    for name in ("sgd_step", "sgd_step_segments"):
        def spy(*a, _f=getattr(ops, name), _n=name, **kw):
            seen.append((_n, len(a), sorted(kw)))
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, spy)
    l = _hip.lib()

    def entry(*a, _f=l.tf_grad_accumulate_segments):
        modes.append(a[4])
        return _f(*a)

    monkeypatch.setattr(l, "tf_grad_accumulate_segments", entry)
    x, cm, rm = _engine_inputs()
    p0 = eng.flat_p.clone()
    eng.step(x, cm.clone(), rm)
    eng.step(x, cm.clone(), rm, apply=True)                                     # what main.py passes on an epoch's last batch
    torch.cuda.synchronize()
    assert [c[0] for c in seen] == ["sgd_step_segments" if frozen else "sgd_step"] * 6
    assert all(c[1] == (8 if frozen else 7) and c[2] == [] for c in seen)      # positional arguments only, as before
    assert modes == [] and eng._accum is None and not torch.equal(eng.flat_p, p0)
    assert (eng.steps, eng.micro_steps, eng.pending_micro_batches) == (2, 2, 0)
    # ... and the spy does see the feature when it is on
    eng2 = TrainEngine(model(), DetectionCriterion(25), lr=1e-3, device="cuda", accum_steps=2)
    del seen[:]
    eng2.step(x, cm.clone(), rm)
    assert seen == [] and modes == [_hip.TF_ACCUM_STORE]
    eng2.step(x, cm.clone(), rm)
    torch.cuda.synchronize()
    assert modes == [_hip.TF_ACCUM_STORE, _hip.TF_ACCUM_FINISH] and len(seen) == 3 and all(c[2] == [] for c in seen)
    assert eng2._accum is not None and eng2._accum.shape == eng2.flat_m.shape and eng2._accum.dtype == torch.float32
    eng.close()
    eng2.close()


def test_trainer_steps_once_per_window_on_the_sum_autograd_accumulates(golden):
    """fp32, ResNet-50, three batches of tests/golden/trainer.npz through trainer.train(accum_steps=2) and torch.optim.SGD: two optimizer
    steps, the first on g(b0) + g(b1), the second on the single gradient of the loader's last batch; ema.update() behind each."""
    from test_gpu_frozen_bn import _golden_batches, _keep, _oracle, _product
    from tinyfaces import trainer
    from tinyfaces.ema import ModelEma
    from tinyfaces.models.loss import DetectionCriterion
    dev = torch.device("cuda")
    m = _product(_oracle("resnet50", seed=9), "resnet50").set_compute_dtype(torch.float32).to(dev).train()
    c = DetectionCriterion(25)
    c.inject_sampling(_keep(), _keep())
    opt = torch.optim.SGD(m.learnable_parameters(1e-3), lr=1e-3, momentum=0.9, weight_decay=5e-4)
    ema = ModelEma(m, 0.999)
    batches = _golden_batches(golden)
    seen, run_backward = _recording(m)
    params = dict(m.named_parameters())
    at_step, step, zeroed, zero_grad = [], opt.step, [], opt.zero_grad

    def stepping(*a, **kw):
        at_step.append((len(seen), {k: p.grad.clone() for k, p in params.items() if p.grad is not None}))
        return step(*a, **kw)

    def zeroing(*a, **kw):
        zeroed.append(len(seen))
        return zero_grad(*a, **kw)

    opt.step, opt.zero_grad = stepping, zeroing
    updates, update = [], ema.update

    def updating():
        updates.append(len(at_step))
        return update()

    ema.update = updating
    try:
        with redirect_stdout(io.StringIO()):
            trainer.train(m, c, opt, [batches[0], batches[1], batches[0]], 0, dev, ema=ema, accum_steps=2)
    finally:
        m._run_backward = run_backward
    torch.cuda.synchronize()
    assert len(seen) == 3 and [n for n, _ in at_step] == [2, 3] and zeroed == [0, 2] and updates == [1, 2] and ema.updates == 2
    changed, names = 0, list(m._grad_names)
    for k, name in enumerate(names):
        assert torch.equal(_i32(at_step[0][1][name]), _i32(seen[0][k] + seen[1][k])), name
        assert torch.equal(_i32(at_step[1][1][name]), _i32(seen[2][k])), name
        changed += not torch.equal(seen[0][k], seen[1][k])
    report("accum_trainer[resnet50,fp32]", tensors=len(names), tensors_whose_micro_batches_differ=changed)
    assert changed > 0.9 * len(names)
    # accum_average: the mean of the window, scaled before the step (k = 2: a product with 0.5 is exact)
    del seen[:], at_step[:]
    seen2, _ = _recording(m)
    try:
        with redirect_stdout(io.StringIO()):
            trainer.train(m, c, opt, [batches[1], batches[0]], 1, dev, accum_steps=2, accum_average=True)
    finally:
        m._run_backward = run_backward
    torch.cuda.synchronize()
    assert len(seen2) == 2 and len(at_step) == 1
    for k, name in enumerate(names):
        assert torch.equal(_i32(at_step[0][1][name]), _i32((seen2[0][k] + seen2[1][k]) * 0.5)), name


def test_two_ranks_exchange_once_per_window_and_match_a_single_process(tmp_path):
    """2 gloo ranks sharing cuda:0 (tests/dist_worker_accum.py), accum_steps = 2, two windows, rank r on (b[r % 2], b[(r + 1) % 2]): both ranks
    end every window with bit-identical parameters; rank 0 agrees with ONE process that sums the gradients and takes the segment-aware step
    (bounds of tests/test_gpu_trainable_layers.py); no collective before a window's last micro-batch (asserted by the worker, checked here)."""
    from tinyfaces import ops
    import dist_worker_accum
    golden = os.path.join(ROOT, "tests", "golden", "trainer.npz")
    out = str(tmp_path / "accum")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29589", os.path.join(ROOT, "tests", "dist_worker_accum.py"), golden, out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = [np.load(f"{out}.rank{k}.npz") for k in range(2)]
    windows = dist_worker_accum.WINDOWS
    buckets = int(got[0]["buckets"])
    assert buckets >= 2
    for k in range(2):
        assert got[k]["collectives"].tolist() == [0, buckets] * windows, got[k]["collectives"]
    for w in range(windows):
        assert np.array_equal(got[0][f"p{w}"].view(np.int32), got[1][f"p{w}"].view(np.int32)), w
    # the single process: frozen BatchNorm, so one model gives both micro-batches' gradients at the current parameters
    m, c, batches = dist_worker_accum.build(golden)
    m = m.cuda().train()
    flat = m.flatten_parameters()
    mom = torch.zeros_like(flat)
    groups, seg, names = m.group_ranges(), m._segments, m.trainable_parameter_names()
    trained = sorted((seg[n][0], seg[n][0] + seg[n][1]) for n in names)
    first = flat.cpu().numpy().copy()
    worst = []
    for w in range(windows):
        grads = []
        for img, cm, rm in ([t.cuda() for t in b] for b in batches):
            m._sync_tables(img.device)
            o = m._run_forward(img, training=True)
            _, g, _ = ops.criterion_fwd_bwd(o, cm.clone(), rm, c.n_templates, c.reg_weight, c.ohem_thresh, c.max_pos, c.max_neg,
                                            c._pos_keep, c._neg_keep, c._next_seed())
            grads.append(m._run_backward(img, g, persistent=True).clone())
        gsum = (grads[0] + grads[1]) + (grads[1] + grads[0])                    # rank 0's window + rank 1's window
        for a, b, mult in groups:
            if mult != 0.0:
                segs = [(max(s_, a), min(e_, b)) for s_, e_ in trained if e_ > a and s_ < b]
                ops.sgd_step_segments(flat, gsum, mom, segs, 1e-4 * mult, 0.9, 5e-4, 0.5)
        torch.cuda.synchronize()
        ref = flat.cpu().numpy()
        worst.append(float(np.abs(got[0][f"p{w}"] - ref).max() / (np.abs(ref).max() + 1e-30)))
    report("accum_dist_2_ranks_vs_single[resnet50,k=1]", worst_rel=str([f"{w:.2e}" for w in worst]), buckets=buckets)
    last = got[0][f"p{windows - 1}"]
    assert np.isfinite(last).all() and float(np.abs(last - first).max()) > 0.0
    assert worst[0] < 1e-5, worst
    assert worst[-1] < 1e-2, worst
