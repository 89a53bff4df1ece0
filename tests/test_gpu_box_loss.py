"""-m gpu: the overlap regression forms of the focal criterion (csrc/criterion.hip, tf_criterion_focal_box_fwd_bwd: IoU, GIoU, DIoU) against
their float64 restatement (tests/box_loss_ref.py), through ops, the autograd criterion, TrainEngine.step and main.py.

Bars: those of tests/test_gpu_focal_loss.py -- the two loss sums within rtol 1e-5 over ALL anchors, the gradient within rtol 1e-5 / atol 1e-6,
image b's atol divided by max(1, npos_b) for normalize="pos" (focal_ref.bars) -- with the four regression gradients of the anchors next to a
kink (box_loss_ref.kink_mask: at most max(1, 0.25 %) of the positives, tests/test_box_loss.py) only required to be finite.
tests/test_box_loss.py shows on the CPU that a kernel with any of seven plausible mistakes misses these bars on the inputs used here.  Every
parity case reports its worst error / bar ratios (profiles/box_loss_parity.txt)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import box_loss_ref as br
import focal_ref as fr
from gpu_util import report
from redzone import assert_guards, assert_written, guarded, guarded_like, guarded_workspace

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tiny-faces-pytorch_amd")
IDS = lambda s: "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def _ref(shape, variant, regime, form, normalize):
    """The float64 reference of one parity case and its kink mask, computed once.  Cached: do not modify."""
    out, cm, rm = br.case(shape, variant, regime)
    return br.box_loss(out, cm, rm, shape[1], form, br.template_wh(shape[1]), normalize=normalize), br.kink_mask(out, cm, rm, shape[1])


def _check(name, out, cm, rm, nt, form, normalize, ref, kink, reg_weight=1.0):
    """One call through ops against the reference: npos exact, class_map untouched, everything finite, loss inside its bar over all anchors and
    the gradient inside its bars outside the kink mask.  -> (loss ratio, gradient ratio), each the worst error as a fraction of its bar."""
    from tinyfaces import ops
    cm_d = cm.cuda()
    loss2, grad, npos = ops.criterion_focal_box_fwd_bwd(out.cuda(), cm_d, rm.cuda(), nt, reg_weight, 2.0, 0.25, normalize, form,
                                                        br.template_wh(nt).float())
    loss2, grad = loss2.cpu(), grad.cpu()
    assert torch.equal(npos.cpu().long(), ref["npos"]), name
    assert torch.equal(cm_d.cpu(), cm), name                                       # read only
    assert bool(torch.isfinite(loss2).all()) and bool(torch.isfinite(grad).all()), name
    lr, gr = br.worst_ratios(loss2, grad, ref, normalize, kink)
    _, gr_all = br.worst_ratios(loss2, grad, ref, normalize)
    share = float(kink.sum()) / max(1, int(ref["npos"].sum()))
    print(f"{name}: cls {float(loss2[0]):.9g} (ref {ref['cls']:.9g}) reg {float(loss2[1]):.9g} (ref {ref['reg']:.9g}) loss error / bar {lr:.3g}, "
          f"gradient error / bar {gr:.3g} ({gr_all:.3g} with the {int(kink.sum())} anchors next to a kink, {100 * share:.3f} % of the positives)")
    report(f"box_loss_parity[{name}]", cls=float(loss2[0]), cls_ref=ref["cls"], reg=float(loss2[1]), reg_ref=ref["reg"], loss_err_over_bar=lr,
           grad_err_over_bar=gr, grad_err_over_bar_with_kinks=gr_all, kink_anchors=int(kink.sum()), kink_share=share)
    assert lr <= 1.0, (name, "loss", lr)
    assert gr <= 1.0, (name, "gradient", gr)
    return lr, gr


@pytest.mark.parametrize("regime", br.REGIMES)
@pytest.mark.parametrize("form", br.REG_LOSSES)
@pytest.mark.parametrize("shape", fr.SHAPES, ids=IDS)
def test_parity_with_the_float64_reference(shape, form, regime):
    out, cm, rm = br.case(shape, "drawn", regime)
    for normalize in fr.NORMALIZE:
        ref, kink = _ref(shape, "drawn", regime, form, normalize)
        _check(f"{IDS(shape)},{form},{regime},{normalize}", out, cm, rm, shape[1], form, normalize, ref, kink)


@pytest.mark.parametrize("variant", fr.VARIANTS[1:])
@pytest.mark.parametrize("form", br.REG_LOSSES)
@pytest.mark.parametrize("shape", fr.SHAPES[:2], ids=IDS)
def test_parity_on_images_without_positives_without_labels_and_fully_labelled(shape, form, variant):
    """("drawn", the fourth of focal_ref.VARIANTS, is the test above.)"""
    for regime in br.REGIMES:
        out, cm, rm = br.case(shape, variant, regime)
        for normalize in fr.NORMALIZE:
            ref, kink = _ref(shape, variant, regime, form, normalize)
            _check(f"{IDS(shape)},{variant},{form},{regime},{normalize}", out, cm, rm, shape[1], form, normalize, ref, kink)


@pytest.mark.parametrize("form", br.REG_LOSSES)
def test_planted_anchors(form):
    """Predictions equal to their targets: the term is 0 within 1e-6 and the gradient finite; pw / ph = +-1e4: finite, and exactly 0 on the
    clamped channel; px = +-1e4: finite; targets beyond the clamp are not clamped (parity, with the rest of the case)."""
    from tinyfaces import ops
    out, cm, rm, where = br.planted_case()
    nt = 25
    twh = br.template_wh(nt)
    ref, kink = br.box_loss(out, cm, rm, nt, form, twh, normalize="none"), br.kink_mask(out, cm, rm, nt)
    _check(f"planted,{form},none", out, cm, rm, nt, form, "none", ref, kink)
    _, grad, _ = ops.criterion_focal_box_fwd_bwd(out.cuda(), cm.cuda(), rm.cuda(), nt, 1.0, 2.0, 0.25, "none", form, twh.float())
    grad = grad.cpu()
    assert bool(torch.isfinite(grad).all())
    for name, c in (("pw+", 2), ("pw-", 2), ("ph+", 3), ("ph-", 3)):
        for b, t, y, x in where[name]:
            assert float(grad[b, (c + 1) * nt + t, y, x]) == 0.0, name
    # the term of the anchors whose prediction IS the target: the loss with them minus the loss with their label taken away
    cm2 = cm.clone()
    for b, t, y, x in where["equal"]:
        cm2[b, t, y, x] = 0
    l1, _, _ = ops.criterion_focal_box_fwd_bwd(out.cuda(), cm.cuda(), rm.cuda(), nt, 1.0, 2.0, 0.25, "none", form, twh.float())
    l2, _, _ = ops.criterion_focal_box_fwd_bwd(out.cuda(), cm2.cuda(), rm.cuda(), nt, 1.0, 2.0, 0.25, "none", form, twh.float())
    ref2 = br.box_loss(out, cm2, rm, nt, form, twh, normalize="none")
    terms = float(l1[1] - l2[1])
    print(f"planted {form}: the {len(where['equal'])} terms of predictions equal to their targets sum to {terms:.3g}; regression sum {float(l1[1]):.9g}")
    assert abs(ref["reg"] - ref2["reg"]) <= 1e-12
    # (the difference of two fp64 sums of about 250 fp32 terms of order 1 carries none of their rounding: every other term is the same bits)
    assert abs(terms) <= 1e-6 * len(where["equal"])


def test_reg_weight_scales_the_regression_gradient_only():
    from tinyfaces import ops
    shape = fr.SHAPES[2]
    out, cm, rm = br.case(shape)
    twh = br.template_wh(25)
    ref, kink = br.box_loss(out, cm, rm, 25, "giou", twh, reg_weight=0.3), br.kink_mask(out, cm, rm, 25)
    _check("2x25x9x9,giou,drawn,pos,reg_weight 0.3", out, cm, rm, 25, "giou", "pos", ref, kink, reg_weight=0.3)
    l1, g1, _ = ops.criterion_focal_box_fwd_bwd(out.cuda(), cm.cuda(), rm.cuda(), 25, 1.0, reg_loss="giou")
    l4, g4, _ = ops.criterion_focal_box_fwd_bwd(out.cuda(), cm.cuda(), rm.cuda(), 25, 4.0, reg_loss="giou")
    assert torch.equal(l1, l4) and torch.equal(g1[:, :25], g4[:, :25])             # the loss pair is unweighted; the class gradient does not move
    assert torch.equal(g1[:, 25:] * 4.0, g4[:, 25:]) and float(g1[:, 25:].abs().max()) > 0      # (a power of two: exact)


@pytest.mark.parametrize("form", br.REG_LOSSES)
def test_a_second_call_returns_the_same_bits(form):
    from tinyfaces import ops
    out, cm, rm = br.case(fr.SHAPES[3])
    out_d, cm_d, rm_d, twh = out.cuda(), cm.cuda(), rm.cuda(), br.template_wh(25).float().cuda()
    l1, g1, n1 = ops.criterion_focal_box_fwd_bwd(out_d, cm_d, rm_d, reg_loss=form, template_wh=twh)
    l2, g2, n2 = ops.criterion_focal_box_fwd_bwd(out_d, cm_d, rm_d, reg_loss=form, template_wh=twh, grad=torch.full_like(out_d, float("nan")))
    assert torch.equal(l1.view(torch.int64), l2.view(torch.int64)) and torch.equal(g1.view(torch.int32), g2.view(torch.int32))
    assert torch.equal(n1, n2) and torch.equal(cm_d.cpu(), cm)


@pytest.mark.parametrize("shape", fr.SHAPES, ids=IDS)
def test_smooth_l1_through_the_new_entry_point_is_the_old_entry_point_bit_for_bit(shape):
    from tinyfaces import ops
    out, cm, rm = [t.cuda() for t in fr.case(shape)]
    for normalize in fr.NORMALIZE:
        l0, g0, n0 = ops.criterion_focal_fwd_bwd(out, cm, rm, shape[1], 0.7, 2.0, 0.25, normalize)
        l1, g1, n1 = ops.criterion_focal_box_fwd_bwd(out, cm, rm, shape[1], 0.7, 2.0, 0.25, normalize, "smooth_l1",
                                                     grad=torch.full_like(out, float("nan")))
        assert torch.equal(l0, l1) and torch.equal(g0, g1) and torch.equal(n0, n1)
        assert float(l0[1]) > 0 and bool(torch.isfinite(g1).all())


def test_the_default_criteria_launch_the_symbols_they_always_launched(monkeypatch):
    """A spy on the library: with reg_loss left at its default neither the soft-margin nor the focal criterion reaches the new entry point, and
    each makes exactly one call of its own, whose loss and gradient are those of a direct call; reg_loss="giou" does reach it."""
    from tinyfaces import _hip, ops
    from tinyfaces.models.loss import DetectionCriterion
    l = _hip.lib()
    seen = []

    def spy(name):
        real = getattr(l, name)

        def f(*a):
            seen.append(name)
            return real(*a)
        return f

    for name in ("tf_criterion_fwd_bwd", "tf_criterion_focal_fwd_bwd", "tf_criterion_focal_box_fwd_bwd"):
        monkeypatch.setattr(l, name, spy(name))
    out, cm, rm = [t.cuda() for t in fr.case(fr.SHAPES[2])]
    crit = DetectionCriterion(25, cls_loss="focal")
    o = out.clone().requires_grad_(True)
    crit(o, cm, rm).backward()
    assert seen == ["tf_criterion_focal_fwd_bwd"]
    l0, g0, _ = ops.criterion_focal_fwd_bwd(out, cm, rm)
    assert torch.equal(o.grad, g0) and torch.equal(torch.stack([crit.masked_class_loss, crit.masked_reg_loss]), l0)
    del seen[:]
    soft = DetectionCriterion(25, seed=3)
    labels = cm.clone()
    o = out.clone().requires_grad_(True)
    soft(o, labels, rm).backward()
    assert seen == ["tf_criterion_fwd_bwd"]
    l0, g0, _ = ops.criterion_fwd_bwd(out, cm.clone(), rm, 25, 1, 0.03, 128, 128, None, None, (3 * 0x9E3779B97F4A7C15 + 1) & (2**64 - 1))
    # (the soft-margin pass adds its block sums with fp64 atomics: the last bits of its loss depend on their order)
    assert torch.equal(o.grad, g0) and np.allclose(torch.stack([soft.masked_class_loss, soft.masked_reg_loss]).cpu().numpy(), l0.cpu().numpy(), rtol=1e-12, atol=0)
    del seen[:]
    DetectionCriterion(25, cls_loss="focal", reg_loss="giou")(out.clone().requires_grad_(True), cm, rm)
    assert seen == ["tf_criterion_focal_box_fwd_bwd"]


@pytest.mark.parametrize("form", br.REG_LOSSES)
@pytest.mark.parametrize("shape", (fr.SHAPES[0], fr.SHAPES[2]), ids=["E=15", "E=2025"])
def test_writes_stay_inside_the_operands_and_the_gradient_is_written_completely(shape, form):
    """Every output and an exactly-sized workspace between guards, the inputs between guards too (a read past their end puts NaN into a
    result): nothing outside is touched, class_map, reg_map and template_wh are left as they were, and every element of grad_out is written
    although nothing zeroed it."""
    from tinyfaces import _hip, ops
    B, nt, H, W = shape
    out, cm, rm = br.case(shape)
    twh = br.template_wh(nt).float()
    dev = torch.device("cuda")
    l = _hip.lib()
    out_d, cm_d, rm_d, twh_d = guarded_like(out, dev), guarded_like(cm, dev), guarded_like(rm, dev), guarded_like(twh, dev)
    grad = guarded(out.shape, torch.float32, dev, pitch_bytes=W * 4)
    loss = guarded((2,), torch.float64, dev)
    npos = guarded((B,), torch.int32, dev)
    wsb = l.tf_criterion_focal_workspace_bytes(B, nt, H, W)
    ws = guarded_workspace(wsb, dev)

    def call(g, n):
        with torch.cuda.device(dev):
            _hip.check(l.tf_criterion_focal_box_fwd_bwd(_hip.ptr(out_d), _hip.ptr(cm_d), _hip.ptr(rm_d), B, nt, H, W, 2.0, 0.25, 1, 1.0,
                                                        ops.REG_LOSSES[form], _hip.ptr(twh_d), _hip.ptr(g), _hip.ptr(loss), None if n is None else _hip.ptr(n),
                                                        _hip.ptr(ws), wsb, _hip.stream()), "tf_criterion_focal_box_fwd_bwd")
        torch.cuda.synchronize()

    call(grad, npos)
    for t, what in ((grad, "grad_out"), (loss, "loss_out"), (npos, "npos_out"), (ws, "workspace"), (out_d, "output"), (cm_d, "class_map"),
                    (rm_d, "reg_map"), (twh_d, "template_wh")):
        assert_guards(t, what)
    assert_written(grad, what="grad_out")
    assert_written(loss, what="loss_out")
    assert_written(npos, what="npos_out")
    assert torch.equal(cm_d.cpu(), cm) and torch.equal(out_d.cpu(), out) and torch.equal(rm_d.cpu(), rm) and torch.equal(twh_d.cpu(), twh)
    ref, kink = _ref(shape, "drawn", "drawn", form, "pos")
    lr, gr = br.worst_ratios(loss.cpu(), grad.cpu(), ref, "pos", kink)
    assert lr <= 1.0 and gr <= 1.0 and torch.equal(npos.cpu().long(), ref["npos"]), (lr, gr)
    # npos_out is optional
    grad2 = guarded(out.shape, torch.float32, dev, pitch_bytes=W * 4)
    call(grad2, None)
    assert_guards(grad2, "grad_out (no npos_out)")
    assert torch.equal(grad2.view(torch.int32), grad.view(torch.int32))


def test_autograd_path_scales_the_ops_gradient_and_feeds_the_meters_the_normalised_sums():
    from tinyfaces import ops
    from tinyfaces.datasets.templates import load_templates
    from tinyfaces.models.loss import DetectionCriterion
    shape = fr.SHAPES[2]
    out, cm, rm = br.case(shape)
    twh = ops.template_wh(load_templates())
    ref = br.box_loss(out, cm, rm, 25, "diou", twh, normalize="pos", reg_weight=2.0)
    kink = br.kink_mask(out, cm, rm, 25)
    crit = DetectionCriterion(25, reg_weight=2.0, cls_loss="focal", reg_loss="diou", templates=load_templates())
    o = out.cuda().requires_grad_(True)
    cm_d = cm.cuda()
    total = crit(o, cm_d, rm.cuda())
    (3.0 * total).backward()
    assert crit._template_wh.is_cuda and not list(crit.buffers())                   # moved on first use; still no registered buffer
    _, g, _ = ops.criterion_focal_box_fwd_bwd(out.cuda(), cm.cuda(), rm.cuda(), 25, 2.0, 2.0, 0.25, "pos", "diou", twh)
    assert torch.equal(o.grad, g * 3.0)
    assert crit.sampled_class_map.data_ptr() == cm_d.data_ptr() and torch.equal(cm_d.cpu(), cm)
    assert np.isclose(float(total.detach()), ref["cls"] + 2.0 * ref["reg"], rtol=1e-5)          # total = cls + reg_weight reg
    B = shape[0]
    assert np.isclose(crit.class_average.average, ref["cls"] / B, rtol=1e-5) and np.isclose(crit.reg_average.average, ref["reg"] / B, rtol=1e-5)
    assert crit.class_average.num_averaged == B
    lr, gr = br.worst_ratios(torch.stack([crit.masked_class_loss, crit.masked_reg_loss]).cpu(), g.cpu(), ref, "pos", kink)
    assert lr <= 1.0 and gr <= 1.0, (lr, gr)


def _giou_engine(**kw):
    import dist_worker_trunks
    from tinyfaces.engine import TrainEngine
    m, c, batches = dist_worker_trunks.build(os.path.join(ROOT, "tests", "golden", "trainer.npz"))
    m.freeze_batchnorm()
    c.cls_loss, c.reg_loss, c.focal_normalize = "focal", "giou", "pos"
    c._pos_keep = c._neg_keep = None                                  # no injected sampling
    return TrainEngine(m, c, lr=1e-4, device="cuda", **kw), [[t.cuda() for t in b] for b in batches]


def test_engine_a_window_of_two_micro_batches_is_the_step_of_the_four_image_batch_and_its_loss_is_the_references():
    """ResNet-50, frozen BatchNorm, fp32, cls_loss="focal", reg_loss="giou", focal_normalize="pos": per-image normalisation makes an image's loss
    independent of its batch, so the accumulated gradient of (b0, b1) is the gradient of [b0; b1]: relative L2 of the flat gradient over the trained
    ranges below 1e-6 (the focal form measured 3.3e-8).  The loss a step returns is the reference's on the model's own forward output."""
    from test_gpu_grad_accum import _trained_mask
    acc, batches = _giou_engine(accum_steps=2)
    big, _ = _giou_engine()
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
    ref = br.box_loss(outs[0].float().cpu(), cm.cpu(), rm.cpu(), 25, "giou", normalize="pos")
    got = loss2.cpu().numpy()
    print(f"giou engine: accumulated vs 4-image gradient rel L2 {rel:.3g}; step loss {got} vs reference {[ref['cls'], ref['reg']]}; "
          f"positives per image {ref['npos'].tolist()}")
    report("box_loss_engine[resnet50,fp32,frozen,giou]", grad_rel_l2=rel, cls=got[0], cls_ref=ref["cls"], reg=got[1], reg_ref=ref["reg"])
    assert float(gb.norm()) > 0.0 and rel < 1e-6, rel
    assert ref["reg"] > 0 and np.allclose(got, [ref["cls"], ref["reg"]], rtol=1e-5, atol=0)
    acc.close()
    big.close()


def test_main_trains_two_steps_with_the_giou_loss(tmp_path):
    """main.py --cls-loss focal --reg-loss giou --reg-weight 2 on the synthetic data set: two steps, and the start-up line says what is trained."""
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(PKG, "main.py"), "synthetic", "synthetic", "--epochs", "1", "--save-every", "1", "--synthetic-len", "8",
                        "--batch_size", "4", "--lr", "1e-5", "--cls-loss", "focal", "--reg-loss", "giou", "--reg-weight", "2"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=400, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    print(r.stdout[-1500:])
    assert "Epoch: [0][1/2]" in r.stdout
    assert "classification loss focal" in r.stdout and "regression loss GIoU, one term per positive, weight 2" in r.stdout
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("Epoch:") and ("nan" in ln.lower() or "inf" in ln.lower())]
