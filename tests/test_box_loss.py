"""IoU / GIoU / DIoU regression losses for DetectionCriterion, everything that needs no GPU: the float64 reference (tests/box_loss_ref.py)
against itself -- its hand-written gradient against autograd, the scale invariance that lets the kernel work in the anchor's own frame --,
that the inputs of tests/test_gpu_box_loss.py are what that file says they are and tell every plausible kernel mistake apart, the host-side
refusals of tf_criterion_focal_box_fwd_bwd, the command-line flags and the criterion's own checks."""
import ctypes as C
import importlib.util
import inspect
import os

import pytest
import torch

import box_loss_ref as br
import focal_ref as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tiny-faces-pytorch_amd")
IDS = lambda s: "x".join(map(str, s))


def _main():
    spec = importlib.util.spec_from_file_location("our_cli_main_box_loss", os.path.join(PKG, "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("shape", fr.SHAPES, ids=IDS)
def test_the_hand_written_gradient_is_the_autograd_gradient(shape):
    """Outside the kink mask (on a tie autograd splits the gradient between the two edges, the formula takes one side); the loss everywhere."""
    nt = shape[1]
    twh = br.template_wh(nt)
    for regime in br.REGIMES:
        out, cm, rm = br.case(shape, "drawn", regime)
        kink = br.kink_mask(out, cm, rm, nt)
        for form in br.REG_LOSSES:
            for normalize in fr.NORMALIZE:
                ref = br.box_loss(out, cm, rm, nt, form, twh, normalize=normalize, reg_weight=0.7)
                loss2, by_hand = br.box_grad_formula(out, cm, rm, nt, form, twh, normalize=normalize, reg_weight=0.7)
                lr, gr = br.worst_ratios(loss2, by_hand, ref, normalize, kink)
                assert lr <= 1e-6 and gr <= 1e-6, (regime, form, normalize, lr, gr)              # 1e-6 of the GPU file's bars
                assert bool(torch.isfinite(by_hand).all()) and bool(torch.isfinite(ref["grad"]).all())


def test_the_planted_anchors_are_finite_in_the_reference_and_the_clamped_channel_has_no_gradient():
    out, cm, rm, where = br.planted_case()
    nt = 25
    twh = br.template_wh(nt)
    kink = br.kink_mask(out, cm, rm, nt)
    for form in br.REG_LOSSES:
        ref = br.box_loss(out, cm, rm, nt, form, twh)
        loss2, by_hand = br.box_grad_formula(out, cm, rm, nt, form, twh)
        assert bool(torch.isfinite(ref["grad"]).all()) and bool(torch.isfinite(by_hand).all()) and bool(torch.isfinite(ref["term"]).all())
        assert max(br.worst_ratios(loss2, by_hand, ref, "pos", kink)) <= 1e-6
        for b, t, y, x in where["equal"]:
            assert kink[b, t, y, x] and abs(float(ref["term"][b, t, y, x])) <= 1e-12
        for name, c in (("pw+", 2), ("pw-", 2), ("ph+", 3), ("ph-", 3)):
            for b, t, y, x in where[name]:
                assert float(ref["grad"][b, (c + 1) * nt + t, y, x]) == 0.0 and float(by_hand[b, (c + 1) * nt + t, y, x]) == 0.0
                assert not kink[b, t, y, x] or name[:2] == "pw"                                 # (|iw| may still be small next to a huge box)
        for name in ("tw_beyond", "th_beyond"):
            assert all(not kink[i] for i in where[name])


def test_the_terms_do_not_change_under_the_per_axis_scaling_of_the_anchor_frame():
    """The claim the kernel rests on: the term of the two boxes in IMAGE coordinates -- centre (cx + px dw, cy + py dh), size (dw e^pw, dh e^ph),
    plain IoU / GIoU / DIoU with a = 1 -- is the term in the anchor's frame with a = dw / dh, whatever the anchor centre and the template."""
    shape = fr.SHAPES[2]
    nt = shape[1]
    out, cm, rm = br.case(shape)
    pos = cm > 0
    p, t = br._blocks(out.double(), rm.double(), nt)
    inside = pos & (p[2].abs() < br.C) & (p[3].abs() < br.C)                   # no clamp is hit
    assert int(inside.sum()) > 200
    twh = br.template_wh(nt)
    dw, dh = [twh[:, k].view(1, nt, 1, 1).expand_as(p[0])[inside] for k in range(2)]
    p, t = [v[inside] for v in p], [v[inside] for v in t]
    g = torch.Generator().manual_seed(5)
    cx, cy = [torch.rand(dw.shape, generator=g, dtype=torch.float64) * 500.0 for _ in range(2)]
    for form in br.REG_LOSSES:
        frame = br.anchor_terms(p, t, dw / dh, form)
        pe = br._edges(cx + p[0] * dw, cy + p[1] * dh, dw * torch.exp(p[2]), dh * torch.exp(p[3]))
        te = br._edges(cx + t[0] * dw, cy + t[1] * dh, dw * torch.exp(t[2]), dh * torch.exp(t[3]))
        image = br.terms_from_edges(pe, te, (pe[1] - pe[0]) * (pe[3] - pe[2]), (te[1] - te[0]) * (te[3] - te[2]), (p[0] - t[0]) * dw, (p[1] - t[1]) * dh,
                                    torch.ones_like(dw), form)
        # edges near 500 carry 500 * 2^-53 = 6e-14 of rounding against intersections of order 1..100: 1e-10 is generous and still 1e5 below the bars
        assert float((frame - image).abs().max()) <= 1e-10, form
        if form != "diou":                                                     # ... and IoU / GIoU need no aspect at all
            assert torch.equal(frame, br.anchor_terms(p, t, torch.ones_like(dw), form))
        else:
            assert float((frame - br.anchor_terms(p, t, torch.ones_like(dw), form)).abs().max()) > 1e-3


@pytest.mark.parametrize("shape", fr.SHAPES, ids=IDS)
def test_the_cases_are_what_the_gpu_tests_say_they_are(shape):
    """The kink mask leaves out at most max(1 anchor, 0.25 % of the positives) in both regimes; in `drawn` at least a quarter of the positives overlap
    their target and, from (3, 16, 8, 8) upward, at least one positive hits the clamp; `near` overlaps nearly everywhere."""
    nt = shape[1]
    for regime in br.REGIMES:
        out, cm, rm = br.case(shape, "drawn", regime)
        assert torch.equal(cm, fr.case(shape)[1]) and torch.equal(rm, fr.case(shape)[2])
        pos = cm > 0
        npos = int(pos.sum())
        kink = int(br.kink_mask(out, cm, rm, nt).sum())
        ref = br.box_loss(out, cm, rm, nt, "iou")
        overlap = float(((ref["term"] < 1.0) & pos).sum()) / npos
        p, _ = br._blocks(out, rm, nt)
        clamped = int((pos & ((p[2].abs() > br.C) | (p[3].abs() > br.C))).sum())
        print(f"{shape} {regime}: {npos} positives, {kink} next to a kink ({100.0 * kink / npos:.3f} %), {overlap:.3f} overlap their target, {clamped} clamped")
        assert kink <= max(1, int(0.0025 * npos)), (regime, kink, npos)
        if regime == "drawn":
            assert torch.equal(out, fr.case(shape)[0])
            assert overlap >= 0.25
            assert clamped >= 1 or shape == fr.SHAPES[0]
        else:
            assert overlap >= 0.9 and float((out[:, nt:] - rm).abs().max()) < 0.7


def _gpu_inputs(mutant):
    """(name, out, cm, rm, nt) of tests/test_gpu_box_loss.py's parity cases on which `mutant` has something to change."""
    clamp = mutant in ("no_clamp", "clamp_gradient_passes")
    if mutant != "target_clamped":
        for shape in fr.SHAPES:
            for regime in br.REGIMES:
                if clamp and (regime == "near" or shape == fr.SHAPES[0]):      # nothing is clamped there
                    continue
                yield (f"{IDS(shape)},{regime}",) + br.case(shape, "drawn", regime) + (shape[1],)
    if clamp or mutant == "target_clamped":
        yield ("planted",) + br.planted_case()[:3] + (25,)


@pytest.mark.parametrize("mutant", br.MUTANTS)
def test_every_mutant_misses_the_bars_on_the_gpu_tests_inputs(mutant):
    """On every input of tests/test_gpu_box_loss.py that can show it (normalize="pos", every form the mistake applies to), a kernel with this
    mistake misses the loss bar or the gradient bar outside the kink mask; the reference is 0 bars away from itself.  The two clamp mutants
    change nothing for a clamped box that does not overlap its target under the plain IoU form (term 1, gradient 0 either way): they have to
    show under giou and diou, whose second term sees the box's size wherever it is, and under iou on the two large shapes and the planted case."""
    seen = 0
    for name, out, cm, rm, nt in _gpu_inputs(mutant):
        twh = br.template_wh(nt)
        kink = br.kink_mask(out, cm, rm, nt)
        for form in br.REG_LOSSES:
            if br.ONLY_FORM.get(mutant, form) != form:
                continue
            ref = br.box_loss(out, cm, rm, nt, form, twh)
            bad = br.box_loss(out, cm, rm, nt, form, twh, mutant=mutant)
            lr, gr = br.worst_ratios([bad["cls"], bad["reg"]], bad["grad"], ref, "pos", kink)
            print(f"{mutant} {name} {form}: loss {lr:.3g} bars, gradient {gr:.3g} bars")
            assert br.worst_ratios([ref["cls"], ref["reg"]], ref["grad"], ref, "pos", kink) == (0.0, 0.0)
            if mutant in ("no_clamp", "clamp_gradient_passes") and form == "iou" and name.split(",")[0] in (IDS(fr.SHAPES[1]), IDS(fr.SHAPES[2])):
                continue
            assert not max(lr, gr) <= 1.0, (mutant, name, form, lr, gr)         # (a NaN -- exp of an unclamped 1e4 -- misses them too)
            seen += 1
    assert seen >= 2


def test_entry_point_refuses_bad_arguments_without_launching(hip):
    """tf_criterion_focal_box_fwd_bwd checks on the host before anything is enqueued.  Runs without a GPU."""
    l = hip.lib()
    ERR_ARG, ERR_WORKSPACE = -1, -4
    assert l.tf_version() >= 700 and "tf_criterion_focal_box_fwd_bwd" in hip.symbols()
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    need = l.tf_criterion_focal_workspace_bytes(2, 25, 9, 9)

    def call(out=p, cm=p, rm=p, B=2, nt=25, H=9, W=9, gamma=2.0, alpha=0.25, normalize=1, reg_weight=1.0, reg_form=2, twh=None, grad=p, loss=p,
             npos=p, ws=p, wsb=need):
        return l.tf_criterion_focal_box_fwd_bwd(out, cm, rm, B, nt, H, W, gamma, alpha, normalize, reg_weight, reg_form, twh, grad, loss, npos, ws, wsb, None)

    for name in ("out", "cm", "rm", "grad", "loss"):
        assert call(**{name: None}) == ERR_ARG, name
    for name in ("B", "nt", "H", "W"):
        for bad in (0, -3):
            assert call(**{name: bad}) == ERR_ARG, name
    for name, values in (("gamma", (-0.5, float("nan"), float("inf"))), ("alpha", (1.5, float("nan"), float("inf"), float("-inf"))),
                         ("reg_weight", (float("nan"), float("inf"), float("-inf"))), ("normalize", (-1, 2)), ("reg_form", (-1, 4, 17))):
        for bad in values:
            assert call(**{name: bad}) == ERR_ARG, (name, bad)
    assert call(reg_form=3, twh=None) == ERR_ARG                      # diou without the template table
    for form in (0, 1, 2):
        assert call(reg_form=form, ws=None) == ERR_WORKSPACE          # ... which the other forms do not need: judged fine, stopped at the workspace
    assert call(reg_form=3, twh=p, wsb=need - 1) == ERR_WORKSPACE
    assert call(out=None, ws=None) == ERR_ARG                         # the arguments are judged before the workspace
    assert not any(buf)                                               # nothing was written


def test_ops_wrappers_signatures_and_refusals():
    from tinyfaces import ops
    ps = inspect.signature(ops.criterion_focal_box_fwd_bwd).parameters
    assert list(ps) == ["output", "class_map", "regression_map", "n_templates", "reg_weight", "gamma", "alpha", "normalize", "reg_loss", "template_wh",
                        "grad"]
    assert (ps["reg_loss"].default, ps["template_wh"].default, ps["grad"].default) == ("smooth_l1", None, None)
    assert tuple(ops.REG_LOSSES) == ("smooth_l1", "iou", "giou", "diou") and [ops.REG_LOSSES[k] for k in ops.REG_LOSSES] == [0, 1, 2, 3]
    assert abs(ops.BOX_CLIP - br.C) < 1e-15
    from tinyfaces.datasets.templates import load_templates
    t = load_templates()
    wh = ops.template_wh(t)
    assert wh.shape == (25, 2) and wh.dtype == torch.float32
    assert torch.equal(wh.double(), torch.as_tensor(t[:, 2:4] - t[:, 0:2] + 1.0).float().double())
    assert torch.equal(ops.template_wh(torch.as_tensor(t)), wh)
    ops.check_reg_loss("smooth_l1")
    ops.check_reg_loss("giou", 2.0)
    ops.check_reg_loss("diou", 1.0, wh, 25)
    for bad in (("ciou",), ("iou", float("nan")), ("giou", float("inf")), ("diou",), ("diou", 1.0, None), ("diou", 1.0, wh, 7), ("diou", 1.0, wh[:, :1]),
                ("diou", 1.0, t)):
        with pytest.raises(ValueError, match="regression loss"):
            ops.check_reg_loss(*bad)
    for bad in (t[:, :3], t[0], torch.zeros(25, 4) - torch.arange(4.0)):
        with pytest.raises(ValueError, match="templates"):
            ops.template_wh(bad)
    out, cm, rm = fr.case(fr.SHAPES[0])
    with pytest.raises(RuntimeError, match="no CPU fallback|HIP"):
        ops.criterion_focal_box_fwd_bwd(out, cm, rm, n_templates=1, reg_loss="giou")


def test_main_flags_are_parsed_beside_the_other_additions():
    main = _main()
    a = main.trunk_arguments(["TRAIN", "VAL"])
    assert (a.reg_loss, a.reg_weight, a.cls_loss) == ("smooth_l1", 1.0, "soft_margin")
    assert "SmoothL1" in main.loss_description(a) and "weight 1" in main.loss_description(a)
    a = main.trunk_arguments(["TRAIN", "VAL", "--cls-loss", "focal", "--reg-loss", "giou", "--reg-weight", "2", "--lr", "0.01"])
    assert (a.reg_loss, a.reg_weight, a.cls_loss, a.lr, a.traindata) == ("giou", 2.0, "focal", 0.01, "TRAIN")
    d = main.loss_description(a)
    assert "focal" in d and "GIoU" in d and "weight 2" in d
    a = main.trunk_arguments(["TRAIN", "VAL", "--reg-weight", "0", "--cls-loss", "focal", "--reg-loss", "smooth-l1"])
    assert (a.reg_loss, a.reg_weight) == ("smooth_l1", 0.0)
    for form in ("iou", "diou"):
        assert main.trunk_arguments(["TRAIN", "VAL", "--cls-loss", "focal", "--reg-loss", form]).reg_loss == form
    for bad in (["--reg-loss", "ciou"], ["--reg-loss", "smooth_l1"], ["--reg-weight", "-1"], ["--reg-weight", "nan"], ["--reg-weight", "inf"],
                ["--reg-loss", "giou"], ["--reg-loss", "diou", "--cls-loss", "soft-margin"]):      # the last two: an overlap loss without the focal pass
        with pytest.raises(SystemExit):
            main.trunk_arguments(["TRAIN", "VAL"] + bad)
    plain = vars(main.arguments(["TRAIN", "VAL"]))
    assert not {"reg_loss", "reg_weight"} & set(plain)
    with pytest.raises(SystemExit):
        main.arguments(["TRAIN", "VAL", "--reg-loss", "giou"])
    assert "--reg-loss" in main.BOX_LOSS_HELP and "--reg-weight" in main.BOX_LOSS_HELP


def test_criterion_keywords_defaults_and_value_errors():
    from tinyfaces.datasets.templates import load_templates
    from tinyfaces.models.loss import DetectionCriterion
    ps = inspect.signature(DetectionCriterion.__init__).parameters
    assert (ps["reg_loss"].default, ps["templates"].default) == ("smooth_l1", None)
    assert DetectionCriterion.REG_LOSSES == ("smooth_l1", "iou", "giou", "diou")
    c = DetectionCriterion(25)
    assert (c.reg_loss, c.cls_loss, c._template_wh) == ("smooth_l1", "soft_margin", None)
    g = DetectionCriterion(25, reg_weight=2.0, cls_loss="focal", reg_loss="giou")
    assert (g.reg_loss, g.reg_weight) == ("giou", 2.0)
    d = DetectionCriterion(25, cls_loss="focal", reg_loss="diou", templates=load_templates())
    assert d._template_wh.shape == (25, 2) and not d._template_wh.is_cuda
    assert not list(d.buffers()) and not list(d.parameters()) and not d.state_dict()               # a plain tensor, not a registered buffer
    for kw in (dict(reg_loss="ciou"), dict(reg_loss="diou"), dict(reg_loss="diou", templates=load_templates()[:7]),
               dict(reg_loss="iou", reg_weight=float("nan"))):
        with pytest.raises(ValueError):
            DetectionCriterion(25, cls_loss="focal", **kw)
    for form in ("iou", "giou", "diou"):
        with pytest.raises(ValueError, match="soft-margin pass"):
            DetectionCriterion(25, reg_loss=form, templates=load_templates())
    DetectionCriterion(25, reg_loss="smooth_l1", templates=load_templates())                       # the default loss may carry a table it does not use


def test_the_criterion_dispatches_on_reg_loss(monkeypatch):
    """_fwd_bwd, which the autograd function and TrainEngine.step both call: a focal criterion with the default regression loss makes the call it
    always made and never touches the new entry point; an overlap loss makes the new call and hands it the template sizes."""
    from tinyfaces import ops
    from tinyfaces.datasets.templates import load_templates
    from tinyfaces.models.loss import DetectionCriterion
    calls = []
    loss2, grad = torch.zeros(2, dtype=torch.float64), torch.zeros(1)

    def recorder(kind):
        def f(*a, **kw):
            calls.append((kind, a, kw))
            return loss2, grad, torch.zeros(1, dtype=torch.int32)
        return f

    for name in ("criterion_fwd_bwd", "criterion_focal_fwd_bwd", "criterion_focal_box_fwd_bwd"):
        monkeypatch.setattr(ops, name, recorder(name))
    out, cm, rm = torch.zeros(1), object(), object()
    f = DetectionCriterion(25, reg_weight=2, cls_loss="focal")
    assert f._fwd_bwd(out, cm, rm)[2] is cm
    kind, a, kw = calls.pop()
    assert kind == "criterion_focal_fwd_bwd" and a == (out, cm, rm, 25, 2, 2.0, 0.25, "pos") and kw == {} and not calls
    g = DetectionCriterion(25, reg_weight=3, cls_loss="focal", focal_normalize="none", reg_loss="giou")
    assert g._fwd_bwd(out, cm, rm)[2] is cm
    kind, a, kw = calls.pop()
    assert kind == "criterion_focal_box_fwd_bwd" and a == (out, cm, rm, 25, 3, 2.0, 0.25, "none", "giou", None) and kw == {} and not calls
    d = DetectionCriterion(25, cls_loss="focal", reg_loss="diou", templates=load_templates())
    d._fwd_bwd(out, cm, rm)
    kind, a, kw = calls.pop()
    assert kind == "criterion_focal_box_fwd_bwd" and a[8] == "diou" and torch.equal(a[9], ops.template_wh(load_templates()))
    DetectionCriterion(25)._fwd_bwd(out, cm, rm)
    assert calls.pop()[0] == "criterion_fwd_bwd" and not calls
    g.cls_loss = "soft_margin"                                      # set behind the constructor's back: refused, not run with SmoothL1
    with pytest.raises(ValueError, match="soft-margin pass"):
        g._fwd_bwd(out, cm, rm)
    g.cls_loss, g.reg_loss = "focal", "ciou"
    with pytest.raises(ValueError, match="reg_loss"):
        g._fwd_bwd(out, cm, rm)
    assert not calls
