"""-m gpu: the focal form of the detection criterion (csrc/criterion.hip, tf_criterion_focal_fwd_bwd) against its float64 restatement
(tests/focal_ref.py), through ops, the autograd criterion and TrainEngine.step.

Bars: those of tests/test_gpu_criterion.py -- the two loss sums within rtol 1e-5, the gradient within rtol 1e-5 / atol 1e-6 --, and for
normalize="pos" image b's atol divided by max(1, npos_b) so that it does not swallow the normalised gradient (focal_ref.bars).
tests/test_focal_loss.py shows on the CPU that a kernel with any of five plausible mistakes misses these bars by a factor >= 100 on the
inputs used here.  Every parity case reports its worst error / bar ratios (profiles/focal_loss_parity.txt)."""
import os

import numpy as np
import pytest
import torch

import focal_ref as fr
import loss_cases as lc
from gpu_util import report
from redzone import assert_guards, assert_written, guarded, guarded_like, guarded_workspace

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(name, out, cm, rm, nt, gamma, alpha, normalize, reg_weight=1.0):
    """One call through ops against focal_ref: npos exact, class_map untouched, everything finite, loss and gradient inside the bars.
    -> (loss ratio, gradient ratio), each the worst error as a fraction of its bar."""
    from tinyfaces import ops
    ref = fr.focal_loss(out, cm, rm, nt, gamma, alpha, normalize, reg_weight=reg_weight)
    cm_d = cm.cuda()
    loss2, grad, npos = ops.criterion_focal_fwd_bwd(out.cuda(), cm_d, rm.cuda(), nt, reg_weight, gamma, alpha, normalize)
    loss2, grad = loss2.cpu(), grad.cpu()
    assert torch.equal(npos.cpu().long(), ref["npos"]), name
    assert torch.equal(cm_d.cpu(), cm), name                                       # read only
    assert bool(torch.isfinite(loss2).all()) and bool(torch.isfinite(grad).all()), name
    lr, gr = fr.worst_ratios(loss2, grad, ref, normalize)
    print(f"{name}: cls {float(loss2[0]):.9g} (ref {ref['cls']:.9g}) reg {float(loss2[1]):.9g} (ref {ref['reg']:.9g}) "
          f"loss error / bar {lr:.3g}, gradient error / bar {gr:.3g}")
    report(f"focal_parity[{name}]", cls=float(loss2[0]), cls_ref=ref["cls"], reg=float(loss2[1]), reg_ref=ref["reg"],
           loss_err_over_bar=lr, grad_err_over_bar=gr, grad_maxabs=float((grad.double() - ref["grad"]).abs().max()))
    assert lr <= 1.0, (name, "loss", lr)
    assert gr <= 1.0, (name, "gradient", gr)
    return lr, gr


@pytest.mark.parametrize("variant", fr.VARIANTS)
@pytest.mark.parametrize("shape", fr.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_parity_with_the_float64_reference(shape, variant):
    out, cm, rm = fr.case(shape, variant)
    for gamma, alpha in fr.PARAMS:
        for normalize in fr.NORMALIZE:
            _check(f"{'x'.join(map(str, shape))},{variant},g{gamma:g},a{alpha:g},{normalize}", out, cm, rm, shape[1], gamma, alpha, normalize)


def test_reg_weight_scales_the_regression_gradient_only():
    out, cm, rm = fr.case(fr.SHAPES[2])
    _check("2x25x9x9,drawn,reg_weight 0.3", out, cm, rm, 25, 2.0, 0.25, "pos", reg_weight=0.3)


def test_extreme_logits_stay_finite_and_inside_the_bars():
    out, cm, rm = fr.extreme_case()
    for gamma, alpha in fr.PARAMS:
        for normalize in fr.NORMALIZE:
            _check(f"extreme,g{gamma:g},a{alpha:g},{normalize}", out, cm, rm, 25, gamma, alpha, normalize)


def test_a_second_call_returns_the_same_bits():
    from tinyfaces import ops
    out, cm, rm = fr.case(fr.SHAPES[3])
    out_d, cm_d, rm_d = out.cuda(), cm.cuda(), rm.cuda()
    l1, g1, n1 = ops.criterion_focal_fwd_bwd(out_d, cm_d, rm_d)
    l2, g2, n2 = ops.criterion_focal_fwd_bwd(out_d, cm_d, rm_d, grad=torch.full_like(out_d, float("nan")))
    assert torch.equal(l1.view(torch.int64), l2.view(torch.int64)) and torch.equal(g1.view(torch.int32), g2.view(torch.int32))
    assert torch.equal(n1, n2) and torch.equal(cm_d.cpu(), cm)


@pytest.mark.parametrize("shape", fr.SHAPES[:4], ids=lambda s: "x".join(map(str, s)))
def test_gamma_0_without_alpha_or_normaliser_is_the_soft_margin_kernel_with_everything_kept(shape):
    """Against ops.criterion_fwd_bwd with ohem_thresh = 0 and all-ones keep flags.  The two kernels do not evaluate softplus the same
    way: loss within rtol 1e-6, gradient within rtol 1e-5 / atol 1e-6."""
    from tinyfaces import ops
    B, nt, H, W = shape
    out, cm, rm = fr.case(shape)
    keep = torch.ones(B, nt * H * W, dtype=torch.uint8)
    l0, g0, _ = ops.criterion_fwd_bwd(out.cuda(), cm.clone().cuda(), rm.cuda(), n_templates=nt, ohem_thresh=0.0, pos_keep=keep, neg_keep=keep)
    l1, g1, _ = ops.criterion_focal_fwd_bwd(out.cuda(), cm.cuda(), rm.cuda(), nt, 1.0, 0.0, -1.0, "none")
    l0, l1 = l0.cpu().numpy(), l1.cpu().numpy()
    print(f"degenerate {shape}: soft-margin kernel {l0}, focal kernel {l1}, gradient max abs diff {float((g0 - g1).abs().max()):.3g}")
    assert l0[0] > 0 and np.allclose(l1, l0, rtol=1e-6, atol=0)
    assert np.allclose(g1.cpu().numpy(), g0.cpu().numpy(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("shape", (fr.SHAPES[0], fr.SHAPES[2]), ids=["E=15", "E=2025"])
def test_writes_stay_inside_the_operands_and_the_gradient_is_written_completely(shape):
    """Every output and an exactly-sized workspace between guards, the inputs between guards too (a read past their end puts NaN into a
    result): nothing outside is touched, and every element of grad_out is written although nothing zeroed it."""
    from tinyfaces import _hip
    B, nt, H, W = shape
    out, cm, rm = fr.case(shape)
    dev = torch.device("cuda")
    l = _hip.lib()
    out_d, cm_d, rm_d = guarded_like(out, dev), guarded_like(cm, dev), guarded_like(rm, dev)
    grad = guarded(out.shape, torch.float32, dev, pitch_bytes=W * 4)
    loss = guarded((2,), torch.float64, dev)
    npos = guarded((B,), torch.int32, dev)
    wsb = l.tf_criterion_focal_workspace_bytes(B, nt, H, W)
    ws = guarded_workspace(wsb, dev)
    with torch.cuda.device(dev):
        _hip.check(l.tf_criterion_focal_fwd_bwd(_hip.ptr(out_d), _hip.ptr(cm_d), _hip.ptr(rm_d), B, nt, H, W, 2.0, 0.25, 1, 1.0, _hip.ptr(grad),
                                                _hip.ptr(loss), _hip.ptr(npos), _hip.ptr(ws), wsb, _hip.stream()), "tf_criterion_focal_fwd_bwd")
    torch.cuda.synchronize()
    for t, what in ((grad, "grad_out"), (loss, "loss_out"), (npos, "npos_out"), (ws, "workspace"), (out_d, "output"), (cm_d, "class_map"),
                    (rm_d, "reg_map")):
        assert_guards(t, what)
    assert_written(grad, what="grad_out")
    assert_written(loss, what="loss_out")
    assert_written(npos, what="npos_out")
    assert torch.equal(cm_d.cpu(), cm) and torch.equal(out_d.cpu(), out) and torch.equal(rm_d.cpu(), rm)
    ref = fr.focal_loss(out, cm, rm, nt, 2.0, 0.25, "pos")
    lr, gr = fr.worst_ratios(loss.cpu(), grad.cpu(), ref, "pos")
    assert lr <= 1.0 and gr <= 1.0 and torch.equal(npos.cpu().long(), ref["npos"]), (lr, gr)
    # npos_out is optional
    grad2 = guarded(out.shape, torch.float32, dev, pitch_bytes=W * 4)
    with torch.cuda.device(dev):
        _hip.check(l.tf_criterion_focal_fwd_bwd(_hip.ptr(out_d), _hip.ptr(cm_d), _hip.ptr(rm_d), B, nt, H, W, 2.0, 0.25, 1, 1.0, _hip.ptr(grad2),
                                                _hip.ptr(loss), None, _hip.ptr(ws), wsb, _hip.stream()), "tf_criterion_focal_fwd_bwd")
    torch.cuda.synchronize()
    assert_guards(grad2, "grad_out (no npos_out)")
    assert torch.equal(grad2.view(torch.int32), grad.view(torch.int32))


def test_autograd_path_scales_the_ops_gradient_and_feeds_the_meters_the_normalised_sums():
    from tinyfaces import ops
    from tinyfaces.models.loss import DetectionCriterion
    shape = fr.SHAPES[2]
    out, cm, rm = fr.case(shape)
    ref = fr.focal_loss(out, cm, rm, 25, 2.0, 0.25, "pos", reg_weight=2.0)
    crit = DetectionCriterion(25, reg_weight=2.0, cls_loss="focal")
    o = out.cuda().requires_grad_(True)
    cm_d = cm.cuda()
    total = crit(o, cm_d, rm.cuda())
    (3.0 * total).backward()
    _, g, _ = ops.criterion_focal_fwd_bwd(out.cuda(), cm.cuda(), rm.cuda(), 25, 2.0, 2.0, 0.25, "pos")
    assert torch.equal(o.grad, g * 3.0)
    assert crit.sampled_class_map.data_ptr() == cm_d.data_ptr() and torch.equal(cm_d.cpu(), cm)
    assert np.isclose(float(total.detach()), ref["cls"] + 2.0 * ref["reg"], rtol=1e-5)
    B = shape[0]
    assert np.isclose(crit.class_average.average, ref["cls"] / B, rtol=1e-5) and np.isclose(crit.reg_average.average, ref["reg"] / B, rtol=1e-5)
    assert crit.class_average.num_averaged == B
    lr, gr = fr.worst_ratios(torch.stack([crit.masked_class_loss, crit.masked_reg_loss]).cpu(), g.cpu(), ref, "pos")
    assert lr <= 1.0 and gr <= 1.0, (lr, gr)


def _focal_engine(**kw):
    import dist_worker_trunks
    from tinyfaces.engine import TrainEngine
    m, c, batches = dist_worker_trunks.build(os.path.join(ROOT, "tests", "golden", "trainer.npz"))
    m.freeze_batchnorm()
    c.cls_loss = "focal"
    c._pos_keep = c._neg_keep = None                                  # no injected sampling
    return TrainEngine(m, c, lr=1e-4, device="cuda", **kw), [[t.cuda() for t in b] for b in batches]


def test_engine_a_window_of_two_micro_batches_is_the_step_of_the_four_image_batch_and_its_loss_is_the_references():
    """ResNet-50, frozen BatchNorm, fp32, cls_loss="focal": per-image normalisation makes an image's loss independent of its batch, so the
    accumulated gradient of (b0, b1) is the gradient of [b0; b1]: <= 1e-3 relative L2 over the trained ranges (the bar of
    test_gpu_grad_accum.py).  The loss a step returns is focal_ref's on the model's own forward output, and class_map is left alone."""
    from test_gpu_grad_accum import _trained_mask
    acc, batches = _focal_engine(accum_steps=2)
    big, _ = _focal_engine()
    outs = []
    run_forward = big.model._run_forward
    big.model._run_forward = lambda x, training=True: (lambda o: (outs.append(o.detach().clone()), o)[1])(run_forward(x, training=training))
    for img, cm, rm in batches:
        acc.step(img, cm, rm)
    img, cm, rm = [torch.cat([batches[0][k], batches[1][k]]) for k in range(3)]
    cm_before = cm.clone()
    loss2 = big.step(img, cm, rm)
    torch.cuda.synchronize()
    assert (acc.steps, acc.micro_steps, big.steps) == (1, 2, 1)
    assert torch.equal(cm, cm_before)
    mk, _ = _trained_mask(acc.model)
    mk = mk.cuda()
    ga, gb = acc.model._grad_flat_persistent[mk].double(), big.model._grad_flat_persistent[mk].double()
    rel = float((ga - gb).norm() / gb.norm())
    ref = fr.focal_loss(outs[0].float().cpu(), cm.cpu(), rm.cpu(), 25, 2.0, 0.25, "pos")
    got = loss2.cpu().numpy()
    print(f"focal engine: accumulated vs 4-image gradient rel L2 {rel:.3g}; step loss {got} vs reference {[ref['cls'], ref['reg']]}; "
          f"positives per image {ref['npos'].tolist()}")
    report("focal_engine[resnet50,fp32,frozen]", grad_rel_l2=rel, cls=got[0], cls_ref=ref["cls"], reg=got[1], reg_ref=ref["reg"])
    assert float(gb.norm()) > 0.0 and rel <= 1e-3, rel
    assert ref["cls"] > 0 and np.allclose(got, [ref["cls"], ref["reg"]], rtol=1e-5, atol=0)
    acc.close()
    big.close()


def test_engine_on_a_default_criterion_steps_as_before(monkeypatch):
    """The focal entry point raises if touched: a default criterion's step makes the soft-margin call it always made, with the loss and the
    gradient handed to the backward pass that a direct call gives."""
    import dist_worker_trunks
    from tinyfaces import ops
    from tinyfaces.engine import TrainEngine

    def boom(*a, **kw):
        raise AssertionError("a default criterion called the focal entry point")

    monkeypatch.setattr(ops, "criterion_focal_fwd_bwd", boom)
    m, c, batches = dist_worker_trunks.build(os.path.join(ROOT, "tests", "golden", "trainer.npz"))
    m.freeze_batchnorm()
    eng = TrainEngine(m, c, lr=1e-4, device="cuda")
    seen = {}
    run_forward, run_backward = m._run_forward, m._run_backward
    m._run_forward = lambda x, training=True: (lambda o: (seen.update(out=o.detach().clone()), o)[1])(run_forward(x, training=training))

    def backward(x, grad, persistent=False):
        seen["grad"] = grad.detach().clone()
        return run_backward(x, grad, persistent=persistent)

    m._run_backward = backward
    img, cm, rm = [t.cuda() for t in batches[0]]
    loss2 = eng.step(img, cm.clone(), rm)
    torch.cuda.synchronize()
    assert eng.steps == 1 and c._calls == 1
    l0, g0, _ = ops.criterion_fwd_bwd(seen["out"], cm.clone(), rm, c.n_templates, c.reg_weight, c.ohem_thresh, c.max_pos, c.max_neg, c._pos_keep,
                                      c._neg_keep, (c._seed * 0x9E3779B97F4A7C15 + 1) & (2**64 - 1))
    assert torch.equal(seen["grad"], g0) and np.allclose(loss2.cpu().numpy(), l0.cpu().numpy(), rtol=1e-12, atol=0)
    eng.close()
