"""-m gpu: the quality focal form of the detection criterion (csrc/criterion_quality.hip, tf_criterion_quality_fwd_bwd) against its float64
restatement (tests/quality_loss_ref.py), through ops, the autograd criterion, TrainEngine.step and main.py.

Bars: those of tests/test_gpu_box_loss.py -- loss[0], loss[1] and loss[2] (the sum of the quality targets) within rtol 1e-5, loss[3] exactly
the number of positives, the gradient within rtol 1e-5 / atol 1e-6, image b's atol divided by max(1, npos_b) for normalize="pos"
(focal_ref.bars).  The class gradient is held to its bar on EVERY labelled anchor (q is continuous in the boxes: no kink exclusion); the four
regression gradients of the anchors next to a kink (box_loss_ref.kink_mask) are only required to be finite, as in that file.
tests/test_quality_loss.py shows on the CPU that a kernel with any of six plausible mistakes misses these bars, and that the kernel's
operations evaluated in float32 stay below a quarter of them.  Every parity case reports its worst error / bar ratios
(profiles/quality_loss_parity.txt)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import box_loss_ref as br
import focal_ref as fr
import quality_loss_ref as qr
from gpu_util import report
from redzone import assert_guards, assert_written, guarded, guarded_like, guarded_workspace

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tiny-faces-pytorch_amd")
IDS = lambda s: "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def _ref(shape, variant, regime, reg_loss, normalize, beta=2.0):
    """The float64 reference of one parity case and its kink mask, computed once.  Cached: do not modify."""
    out, cm, rm = br.case(shape, variant, regime)
    return qr.quality_loss(out, cm, rm, shape[1], reg_loss, br.template_wh(shape[1]), beta, normalize), br.kink_mask(out, cm, rm, shape[1])


def _check(name, out, cm, rm, nt, reg_loss, normalize, ref, kink, beta=2.0, reg_weight=1.0):
    """One call through ops against the reference: npos and loss[3] exact, class_map untouched, everything finite, the three sums inside their
    bars, the class gradient inside its bars everywhere and the regression gradient outside the kink mask.  -> (loss ratio, gradient ratio)."""
    from tinyfaces import ops
    cm_d = cm.cuda()
    loss4, grad, npos = ops.criterion_quality_fwd_bwd(out.cuda(), cm_d, rm.cuda(), nt, reg_weight, beta, normalize, reg_loss,
                                                      br.template_wh(nt).float())
    loss4, grad = loss4.cpu(), grad.cpu()
    assert loss4.shape == (4,) and loss4.dtype == torch.float64, name
    assert torch.equal(npos.cpu().long(), ref["npos"]), name
    assert float(loss4[3]) == float(ref["npos"].sum()), name
    assert torch.equal(cm_d.cpu(), cm), name                                       # read only
    assert bool(torch.isfinite(loss4).all()) and bool(torch.isfinite(grad).all()), name
    lr, gr = qr.worst_ratios(loss4, grad, ref, normalize, kink)
    _, gr_all = qr.worst_ratios(loss4, grad, ref, normalize)
    cls_r = float(((grad[:, :nt].double() - ref["grad"][:, :nt]).abs() / fr.bars(ref, normalize)[:, :nt]).max())
    mean_iou = float(loss4[2]) / max(1.0, float(loss4[3]))
    print(f"{name}: cls {float(loss4[0]):.9g} (ref {ref['cls']:.9g}) reg {float(loss4[1]):.9g} (ref {ref['reg']:.9g}) sum q {float(loss4[2]):.9g} "
          f"(ref {ref['qsum']:.9g}, mean IoU {mean_iou:.4f}) loss error / bar {lr:.3g}, gradient error / bar {gr:.3g} (class channel {cls_r:.3g}; "
          f"{gr_all:.3g} with the {int(kink.sum())} anchors next to a kink)")
    report(f"quality_loss_parity[{name}]", cls=float(loss4[0]), cls_ref=ref["cls"], reg=float(loss4[1]), reg_ref=ref["reg"], qsum=float(loss4[2]),
           qsum_ref=ref["qsum"], npos=int(loss4[3]), loss_err_over_bar=lr, grad_err_over_bar=gr, cls_grad_err_over_bar=cls_r,
           grad_err_over_bar_with_kinks=gr_all, kink_anchors=int(kink.sum()))
    assert lr <= 1.0, (name, "loss", lr)
    assert cls_r <= 1.0, (name, "class gradient", cls_r)
    assert gr <= 1.0, (name, "gradient", gr)
    return lr, gr


@pytest.mark.parametrize("regime", br.REGIMES)
@pytest.mark.parametrize("reg_loss", qr.REG_LOSSES)
@pytest.mark.parametrize("shape", fr.SHAPES, ids=IDS)
def test_parity_with_the_float64_reference(shape, reg_loss, regime):
    out, cm, rm = br.case(shape, "drawn", regime)
    for normalize in fr.NORMALIZE:
        ref, kink = _ref(shape, "drawn", regime, reg_loss, normalize)
        _check(f"{IDS(shape)},{reg_loss},{regime},{normalize},beta 2", out, cm, rm, shape[1], reg_loss, normalize, ref, kink)


@pytest.mark.parametrize("beta", qr.BETAS[1:])
@pytest.mark.parametrize("shape", (fr.SHAPES[2], fr.SHAPES[3]), ids=IDS)
def test_parity_at_other_exponents(shape, beta):
    """beta = 2.5 and 4 take the powf road of the kernel."""
    for regime in br.REGIMES:
        out, cm, rm = br.case(shape, "drawn", regime)
        for reg_loss in qr.REG_LOSSES:
            for normalize in fr.NORMALIZE:
                ref, kink = _ref(shape, "drawn", regime, reg_loss, normalize, beta)
                _check(f"{IDS(shape)},{reg_loss},{regime},{normalize},beta {beta:g}", out, cm, rm, shape[1], reg_loss, normalize, ref, kink, beta=beta)


@pytest.mark.parametrize("variant", fr.VARIANTS[1:])
@pytest.mark.parametrize("shape", fr.SHAPES[:2], ids=IDS)
def test_parity_on_images_without_positives_without_labels_and_fully_labelled(shape, variant):
    for regime in br.REGIMES:
        out, cm, rm = br.case(shape, variant, regime)
        for reg_loss in ("smooth_l1", "giou"):
            for normalize in fr.NORMALIZE:
                ref, kink = _ref(shape, variant, regime, reg_loss, normalize)
                _check(f"{IDS(shape)},{variant},{reg_loss},{regime},{normalize},beta 2", out, cm, rm, shape[1], reg_loss, normalize, ref, kink)


@pytest.mark.parametrize("beta", (2.0, 2.5))
def test_extreme_logits_over_near_boxes_stay_finite_and_inside_the_bars(beta):
    """Logits of +-100 and +-1e4 under both labels, the positives among them with a quality target well inside (0, 1)."""
    out, cm, rm = qr.extreme_case()
    kink = br.kink_mask(out, cm, rm, 25)
    for normalize in fr.NORMALIZE:
        ref = qr.quality_loss(out, cm, rm, 25, "iou", None, beta, normalize)
        _check(f"extreme,iou,{normalize},beta {beta:g}", out, cm, rm, 25, "iou", normalize, ref, kink, beta=beta)


@pytest.mark.parametrize("reg_loss", qr.REG_LOSSES)
def test_planted_anchors(reg_loss):
    """Predictions equal to their targets (q = 1), predictions beyond the clamp, centres far away (q = 0) and targets beyond the clamp, with the
    rest of the case: parity; the regression gradient of a clamped channel is exactly 0 under the overlap forms."""
    from tinyfaces import ops
    out, cm, rm, where = br.planted_case()
    nt = 25
    twh = br.template_wh(nt)
    ref, kink = qr.quality_loss(out, cm, rm, nt, reg_loss, twh, normalize="none"), br.kink_mask(out, cm, rm, nt)
    _check(f"planted,{reg_loss},none,beta 2", out, cm, rm, nt, reg_loss, "none", ref, kink)
    if reg_loss != "smooth_l1":
        _, grad, _ = ops.criterion_quality_fwd_bwd(out.cuda(), cm.cuda(), rm.cuda(), nt, 1.0, 2.0, "none", reg_loss, twh.float())
        grad = grad.cpu()
        for name, c in (("pw+", 2), ("pw-", 2), ("ph+", 3), ("ph-", 3)):
            for b, t, y, x in where[name]:
                assert float(grad[b, (c + 1) * nt + t, y, x]) == 0.0, name


def test_a_single_positive_with_equal_boxes_has_mean_iou_one():
    from tinyfaces import ops
    out, cm, rm = [v.clone() for v in br.case(fr.SHAPES[2])]
    nt = 25
    idx = (cm[0] == 1).nonzero()[0].tolist()
    cm[cm == 1] = -1.0
    cm[0][tuple(idx)] = 1.0
    t, y, x = idx
    for c in range(4):
        out[0, (c + 1) * nt + t, y, x] = rm[0, c * nt + t, y, x]
    loss4, grad, npos = ops.criterion_quality_fwd_bwd(out.cuda(), cm.cuda(), rm.cuda(), nt)
    loss4 = loss4.cpu()
    print(f"single positive, equal boxes: sum q {float(loss4[2])!r}, positives {float(loss4[3])}")
    assert float(loss4[3]) == 1.0 and npos.tolist() == [1, 0] and abs(float(loss4[2]) - 1.0) <= 1e-6
    assert float(loss4[1]) == 0.0 and bool(torch.isfinite(grad).all())


@pytest.mark.parametrize("reg_loss", qr.REG_LOSSES)
@pytest.mark.parametrize("shape", (fr.SHAPES[2], fr.SHAPES[3]), ids=IDS)
def test_nothing_flows_from_the_quality_target_into_the_regression_channels(shape, reg_loss):
    """q is a constant of the classification term and the regression term is the focal pass's own function (box_term, SmoothL1): loss[1] and the
    four regression channels of the gradient are those of the focal call with the same reg_loss.  Each of the two lies within one bar of the
    float64 reference, so they lie within two bars of each other (the compiler contracts multiply-adds per kernel: the last bit may differ;
    the number of elements that do is printed).  A gradient through q would miss this by five orders of magnitude (tests/test_quality_loss.py)."""
    from tinyfaces import ops
    out, cm, rm = br.case(shape, "drawn", "near")
    kink = br.kink_mask(out, cm, rm, shape[1])
    out, cm, rm = out.cuda(), cm.cuda(), rm.cuda()
    twh = br.template_wh(shape[1]).float()
    nt = shape[1]
    for normalize in fr.NORMALIZE:
        ref, _ = _ref(shape, "drawn", "near", reg_loss, normalize)
        l0, g0, n0 = ops.criterion_focal_box_fwd_bwd(out, cm, rm, nt, 1.0, 2.0, 0.25, normalize, reg_loss, twh)
        l1, g1, n1 = ops.criterion_quality_fwd_bwd(out, cm, rm, nt, 1.0, 2.0, normalize, reg_loss, twh)
        assert torch.equal(n0, n1)
        assert abs(float(l0[1]) - float(l1[1])) <= 2e-5 * abs(ref["reg"]), (reg_loss, normalize)
        d = (g0[:, nt:].cpu().double() - g1[:, nt:].cpu().double()).abs() / fr.bars(ref, normalize)[:, nt:]
        d = torch.where(kink.repeat(1, 4, 1, 1), torch.zeros_like(d), d)
        differ = int((g0[:, nt:].view(torch.int32) != g1[:, nt:].view(torch.int32)).sum())
        print(f"{IDS(shape)},{reg_loss},{normalize}: regression gradient of the qfl call against the focal call: worst difference {float(d.max()):.3g} bars, "
              f"{differ} of {g0[:, nt:].numel()} elements differ in their bits; loss[1] {float(l1[1])!r} against {float(l0[1])!r}")
        assert float(d.max()) <= 2.0, (reg_loss, normalize, float(d.max()))
        assert float(g1[:, nt:].abs().max()) > 0 and not torch.equal(g0[:, :nt], g1[:, :nt])


def test_reg_weight_scales_the_regression_gradient_only():
    from tinyfaces import ops
    out, cm, rm = [t.cuda() for t in br.case(fr.SHAPES[2])]
    l1, g1, _ = ops.criterion_quality_fwd_bwd(out, cm, rm, 25, 1.0, reg_loss="giou")
    l4, g4, _ = ops.criterion_quality_fwd_bwd(out, cm, rm, 25, 4.0, reg_loss="giou")
    assert torch.equal(l1, l4) and torch.equal(g1[:, :25], g4[:, :25])             # the loss vector is unweighted; the class gradient does not move
    assert torch.equal(g1[:, 25:] * 4.0, g4[:, 25:]) and float(g1[:, 25:].abs().max()) > 0      # (a power of two: exact)


@pytest.mark.parametrize("reg_loss", qr.REG_LOSSES)
def test_a_second_call_returns_the_same_bits(reg_loss):
    from tinyfaces import ops
    out, cm, rm = br.case(fr.SHAPES[3])
    out_d, cm_d, rm_d, twh = out.cuda(), cm.cuda(), rm.cuda(), br.template_wh(25).float().cuda()
    for beta in (2.0, 2.5):
        l1, g1, n1 = ops.criterion_quality_fwd_bwd(out_d, cm_d, rm_d, beta=beta, reg_loss=reg_loss, template_wh=twh)
        l2, g2, n2 = ops.criterion_quality_fwd_bwd(out_d, cm_d, rm_d, beta=beta, reg_loss=reg_loss, template_wh=twh, grad=torch.full_like(out_d, float("nan")))
        assert torch.equal(l1.view(torch.int64), l2.view(torch.int64)) and torch.equal(g1.view(torch.int32), g2.view(torch.int32))
        assert torch.equal(n1, n2) and torch.equal(cm_d.cpu(), cm) and bool(torch.isfinite(g2).all())


@pytest.mark.parametrize("reg_loss", qr.REG_LOSSES)
@pytest.mark.parametrize("shape", (fr.SHAPES[0], fr.SHAPES[2]), ids=["E=15", "E=2025"])
def test_writes_stay_inside_the_operands_and_the_gradient_is_written_completely(shape, reg_loss):
    """Every output and an exactly-sized workspace between guards, the inputs between guards too (a read past their end puts NaN into a
    result): nothing outside is touched, the inputs are left as they were, and every element of grad_out is written although nothing zeroed it."""
    from tinyfaces import _hip, ops
    B, nt, H, W = shape
    out, cm, rm = br.case(shape)
    twh = br.template_wh(nt).float()
    dev = torch.device("cuda")
    l = _hip.lib()
    out_d, cm_d, rm_d, twh_d = guarded_like(out, dev), guarded_like(cm, dev), guarded_like(rm, dev), guarded_like(twh, dev)
    grad = guarded(out.shape, torch.float32, dev, pitch_bytes=W * 4)
    loss = guarded((4,), torch.float64, dev)
    npos = guarded((B,), torch.int32, dev)
    wsb = l.tf_criterion_quality_workspace_bytes(B, nt, H, W)
    ws = guarded_workspace(wsb, dev)

    def call(g, n):
        with torch.cuda.device(dev):
            _hip.check(l.tf_criterion_quality_fwd_bwd(_hip.ptr(out_d), _hip.ptr(cm_d), _hip.ptr(rm_d), B, nt, H, W, 2.0, 1, 1.0,
                                                      ops.REG_LOSSES[reg_loss], _hip.ptr(twh_d), _hip.ptr(g), _hip.ptr(loss), None if n is None else _hip.ptr(n),
                                                      _hip.ptr(ws), wsb, _hip.stream()), "tf_criterion_quality_fwd_bwd")
        torch.cuda.synchronize()

    call(grad, npos)
    for t, what in ((grad, "grad_out"), (loss, "loss_out"), (npos, "npos_out"), (ws, "workspace"), (out_d, "output"), (cm_d, "class_map"),
                    (rm_d, "reg_map"), (twh_d, "template_wh")):
        assert_guards(t, what)
    assert_written(grad, what="grad_out")
    assert_written(loss, what="loss_out")
    assert_written(npos, what="npos_out")
    assert torch.equal(cm_d.cpu(), cm) and torch.equal(out_d.cpu(), out) and torch.equal(rm_d.cpu(), rm) and torch.equal(twh_d.cpu(), twh)
    ref, kink = _ref(shape, "drawn", "drawn", reg_loss, "pos")
    lr, gr = qr.worst_ratios(loss.cpu(), grad.cpu(), ref, "pos", kink)
    assert lr <= 1.0 and gr <= 1.0 and torch.equal(npos.cpu().long(), ref["npos"]), (lr, gr)
    grad2 = guarded(out.shape, torch.float32, dev, pitch_bytes=W * 4)             # npos_out is optional
    call(grad2, None)
    assert_guards(grad2, "grad_out (no npos_out)")
    assert torch.equal(grad2.view(torch.int32), grad.view(torch.int32))


def test_refusals_enqueue_nothing():
    """A workspace one byte short: TF_ERR_WORKSPACE; beta < 1 or NaN, an unknown form, DIoU without a table: TF_ERR_ARG.  The gradient, the loss
    and the workspace still hold their fill afterwards."""
    from tinyfaces import _hip
    B, nt, H, W = fr.SHAPES[2]
    out, cm, rm = [t.cuda() for t in br.case(fr.SHAPES[2])]
    dev = out.device
    l = _hip.lib()
    wsb = l.tf_criterion_quality_workspace_bytes(B, nt, H, W)
    grad, loss, ws = guarded(out.shape, torch.float32, dev), guarded((4,), torch.float64, dev), guarded_workspace(wsb, dev)

    def call(beta=2.0, form=0, twh=None, size=wsb):
        with torch.cuda.device(dev):
            rc = l.tf_criterion_quality_fwd_bwd(_hip.ptr(out), _hip.ptr(cm), _hip.ptr(rm), B, nt, H, W, beta, 1, 1.0, form, twh, _hip.ptr(grad), _hip.ptr(loss),
                                                None, _hip.ptr(ws), size, _hip.stream())
        torch.cuda.synchronize()
        return rc

    ERR_ARG, ERR_WORKSPACE = -1, -4
    assert call(size=wsb - 1) == ERR_WORKSPACE
    assert call(beta=0.99) == ERR_ARG and call(beta=float("nan")) == ERR_ARG and call(form=4) == ERR_ARG and call(form=3, twh=None) == ERR_ARG
    for t in (grad, loss, ws):
        assert unwritten_all(t)
    assert call() == 0
    assert_written(grad, what="grad_out")
    assert_written(loss, what="loss_out")


def unwritten_all(t):
    from redzone import unwritten
    return unwritten(t)[0] == t.numel()


def test_the_default_criteria_never_reach_the_new_symbols(monkeypatch):
    """A spy on the library: the soft-margin and the focal criteria make exactly the one call they always made and never touch
    tf_criterion_quality_*; the qfl criterion makes the workspace query and the one new call."""
    from tinyfaces import _hip
    from tinyfaces.models.loss import DetectionCriterion
    l = _hip.lib()
    seen = []

    def spy(name):
        real = getattr(l, name)

        def f(*a):
            seen.append(name)
            return real(*a)
        return f

    for name in ("tf_criterion_fwd_bwd", "tf_criterion_focal_fwd_bwd", "tf_criterion_focal_box_fwd_bwd", "tf_criterion_quality_fwd_bwd",
                 "tf_criterion_quality_workspace_bytes"):
        monkeypatch.setattr(l, name, spy(name))
    out, cm, rm = [t.cuda() for t in fr.case(fr.SHAPES[2])]
    for kw, want in ((dict(), "tf_criterion_fwd_bwd"), (dict(cls_loss="focal"), "tf_criterion_focal_fwd_bwd"),
                     (dict(cls_loss="focal", reg_loss="giou"), "tf_criterion_focal_box_fwd_bwd")):
        o = out.clone().requires_grad_(True)
        DetectionCriterion(25, **kw)(o, cm.clone(), rm).backward()
        assert seen == [want], (kw, seen)
        del seen[:]
    DetectionCriterion(25, cls_loss="qfl")(out.clone().requires_grad_(True), cm, rm)
    assert seen == ["tf_criterion_quality_workspace_bytes", "tf_criterion_quality_fwd_bwd"]


def test_autograd_path_scales_the_ops_gradient_and_feeds_the_three_meters():
    from tinyfaces import ops
    from tinyfaces.datasets.templates import load_templates
    from tinyfaces.models.loss import DetectionCriterion
    shape = fr.SHAPES[2]
    out, cm, rm = br.case(shape, "drawn", "near")
    twh = ops.template_wh(load_templates())
    ref = qr.quality_loss(out, cm, rm, 25, "diou", twh, 2.0, "pos", reg_weight=2.0)
    kink = br.kink_mask(out, cm, rm, 25)
    crit = DetectionCriterion(25, reg_weight=2.0, cls_loss="qfl", reg_loss="diou", templates=load_templates())
    o = out.cuda().requires_grad_(True)
    cm_d = cm.cuda()
    total = crit(o, cm_d, rm.cuda())
    (3.0 * total).backward()
    l4, g, _ = ops.criterion_quality_fwd_bwd(out.cuda(), cm.cuda(), rm.cuda(), 25, 2.0, 2.0, "pos", "diou", twh)
    assert torch.equal(o.grad, g * 3.0)                                             # scaled by the incoming gradient
    assert crit.sampled_class_map.data_ptr() == cm_d.data_ptr() and torch.equal(cm_d.cpu(), cm)
    assert np.isclose(float(total.detach()), ref["cls"] + 2.0 * ref["reg"], rtol=1e-5)          # total = cls + reg_weight reg
    B, npos = shape[0], int(ref["npos"].sum())
    assert np.isclose(crit.class_average.average, ref["cls"] / B, rtol=1e-5) and np.isclose(crit.reg_average.average, ref["reg"] / B, rtol=1e-5)
    assert crit.class_average.num_averaged == B and crit.quality_average.num_averaged == npos
    assert np.isclose(crit.quality_average.average, ref["qsum"] / npos, rtol=1e-5) and 0.3 < crit.quality_average.average < 1.0
    lr, gr = qr.worst_ratios(l4.cpu(), g.cpu(), ref, "pos", kink)
    assert lr <= 1.0 and gr <= 1.0, (lr, gr)
    crit(out.cuda(), cm_d, rm.cuda())                                               # a second batch: the mean over all positives seen
    assert crit.quality_average.num_averaged == 2 * npos and np.isclose(crit.quality_average.average, ref["qsum"] / npos, rtol=1e-5)


def _qfl_engine(**kw):
    import dist_worker_trunks
    from tinyfaces import ops
    from tinyfaces.datasets.templates import load_templates
    from tinyfaces.engine import TrainEngine
    m, c, batches = dist_worker_trunks.build(os.path.join(ROOT, "tests", "golden", "trainer.npz"))
    m.freeze_batchnorm()
    c.cls_loss, c.reg_loss, c.focal_normalize, c._template_wh = "qfl", "diou", "pos", ops.template_wh(load_templates())
    c._pos_keep = c._neg_keep = None                                  # no injected sampling
    return TrainEngine(m, c, lr=1e-4, device="cuda", **kw), [[t.cuda() for t in b] for b in batches]


def test_engine_a_window_of_two_micro_batches_is_the_step_of_the_four_image_batch_and_its_loss_is_the_references():
    """ResNet-50, frozen BatchNorm, fp32, cls_loss="qfl", reg_loss="diou", focal_normalize="pos": per-image normalisation makes an image's loss
    independent of its batch, so the accumulated gradient of (b0, b1) is the gradient of [b0; b1]: relative L2 of the flat gradient over the trained
    ranges below 1e-6 (the focal form measured 3.3e-8).  The 4-vector a step returns is the reference's on the model's own forward output."""
    from test_gpu_grad_accum import _trained_mask
    from tinyfaces import ops
    from tinyfaces.datasets.templates import load_templates
    acc, batches = _qfl_engine(accum_steps=2)
    big, _ = _qfl_engine()
    outs = []
    run_forward = big.model._run_forward
    big.model._run_forward = lambda x, training=True: (lambda o: (outs.append(o.detach().clone()), o)[1])(run_forward(x, training=training))
    for img, cm, rm in batches:
        acc.step(img, cm, rm)
    img, cm, rm = [torch.cat([batches[0][k], batches[1][k]]) for k in range(3)]
    cm_before = cm.clone()
    loss4 = big.step(img, cm, rm)
    torch.cuda.synchronize()
    assert (acc.steps, acc.micro_steps, big.steps) == (1, 2, 1)
    assert torch.equal(cm, cm_before) and loss4.shape == (4,)
    mk, _ = _trained_mask(acc.model)
    mk = mk.cuda()
    ga, gb = acc.model._grad_flat_persistent[mk].double(), big.model._grad_flat_persistent[mk].double()
    rel = float((ga - gb).norm() / gb.norm())
    ref = qr.quality_loss(outs[0].float().cpu(), cm.cpu(), rm.cpu(), 25, "diou", ops.template_wh(load_templates()), 2.0, "pos")
    got = loss4.cpu().numpy()
    want = [ref["cls"], ref["reg"], ref["qsum"], float(ref["npos"].sum())]
    print(f"qfl engine: accumulated vs 4-image gradient rel L2 {rel:.3g}; step loss {got} vs reference {want}; positives per image {ref['npos'].tolist()}")
    report("quality_loss_engine[resnet50,fp32,frozen,qfl,diou]", grad_rel_l2=rel, cls=got[0], cls_ref=ref["cls"], reg=got[1], reg_ref=ref["reg"],
           qsum=got[2], qsum_ref=ref["qsum"], npos=got[3])
    assert float(gb.norm()) > 0.0 and rel < 1e-6, rel
    assert ref["reg"] > 0 and np.allclose(got[:3], want[:3], rtol=1e-5, atol=0) and got[3] == want[3]
    acc.criterion.flush_meters()
    assert acc.criterion.quality_average.num_averaged == int(want[3])
    acc.close()
    big.close()


def test_main_trains_two_steps_with_the_quality_focal_loss(tmp_path):
    """main.py --cls-loss qfl --reg-loss diou --assigner atss: two steps, the start-up line names the loss, the mean IoU of the positives is
    printed and lies in [0, 1], no Epoch line holds a nan or an inf, and the checkpoint records the flags.  (--assigner atss does not go with
    the `synthetic` throughput crops -- main.py refuses it, tests/test_atss.py --, so the run is on synthetic-faces.)"""
    import re
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(PKG, "main.py"), "synthetic-faces", "synthetic-faces", "--epochs", "1", "--save-every", "1",
                        "--synthetic-len", "8", "--batch_size", "4", "--lr", "1e-5", "--cls-loss", "qfl", "--reg-loss", "diou", "--assigner", "atss"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=400, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    print(r.stdout[-2500:])
    assert "Epoch: [0][1/2]" in r.stdout
    assert "classification loss quality focal (beta 2, IoU of the predicted box as the target" in r.stdout
    assert "regression loss DIoU, one term per positive" in r.stdout and "--ohem-thresh is unused with --cls-loss qfl" in r.stdout
    values = [float(v) for v in re.findall(r"mean IoU of positives ([0-9.eE+-]+)", r.stdout)]
    assert values and all(0.0 <= v <= 1.0 for v in values), values
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("Epoch:") and ("nan" in ln.lower() or "inf" in ln.lower())]
    state = torch.load(tmp_path / "weights" / "checkpoint_1.pth", map_location="cpu", weights_only=False)
    assert state["args"]["cls_loss"] == "qfl" and state["args"]["qfl_beta"] == 2.0 and state["args"]["reg_loss"] == "diou"
