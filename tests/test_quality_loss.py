"""Quality focal loss for DetectionCriterion, everything that needs no GPU: the float64 reference (tests/quality_loss_ref.py) against itself --
its hand-written gradient against autograd, every plausible kernel mistake told apart, q on planted boxes --, the float32 evaluation of the
kernel's formula against float64 in units of the bars of tests/test_gpu_quality_loss.py, the host-side refusals of
tf_criterion_quality_fwd_bwd, the command-line flags, the criterion's keywords, dispatch and meters."""
import ctypes as C
import importlib.util
import inspect
import os

import pytest
import torch

import box_loss_ref as br
import focal_ref as fr
import quality_loss_ref as qr
from gpu_util import report

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tiny-faces-pytorch_amd")
IDS = lambda s: "x".join(map(str, s))


def _main():
    spec = importlib.util.spec_from_file_location("our_cli_main_quality_loss", os.path.join(PKG, "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------------------------- the reference itself
@pytest.mark.parametrize("shape", fr.SHAPES[:4], ids=IDS)
def test_the_hand_written_gradient_is_the_autograd_gradient(shape):
    """To 1e-12 (absolute, on the unnormalised scale): the class gradient everywhere, the loss sums, sum q and sum npos; the regression gradient
    is box_loss_ref's own formula, compared there.  beta = 1 is compared outside sigma = q exactly, where autograd's sign(0) = 0 agrees anyway."""
    nt = shape[1]
    twh = br.template_wh(nt)
    for regime in br.REGIMES:
        out, cm, rm = br.case(shape, "drawn", regime)
        for reg_loss in ("smooth_l1", "diou"):
            for beta in (1.0, 1.5, 2.0, 2.5, 4.0):
                for normalize in fr.NORMALIZE:
                    ref = qr.quality_loss(out, cm, rm, nt, reg_loss, twh, beta, normalize, reg_weight=0.7)
                    loss4, by_hand = qr.quality_grad_formula(out, cm, rm, nt, reg_loss, twh, beta, normalize, reg_weight=0.7)
                    assert float((by_hand[:, :nt] - ref["grad"][:, :nt]).abs().max()) <= 1e-12, (regime, reg_loss, beta, normalize)
                    want = torch.tensor([ref["cls"], ref["reg"], ref["qsum"], float(ref["npos"].sum())], dtype=torch.float64)
                    assert float(((loss4 - want).abs() / want.abs().clamp(min=1.0)).max()) <= 1e-12, (loss4, want)
                    assert float(loss4[3]) == float(ref["npos"].sum())
                    assert bool(torch.isfinite(by_hand).all()) and bool(torch.isfinite(ref["grad"]).all())
                    if reg_loss == "smooth_l1":
                        assert float((by_hand[:, nt:] - ref["grad"][:, nt:]).abs().max()) <= 1e-12


def _mutant_inputs():
    """The inputs on the geometry of fr.SHAPES[2] = (2, 25, 9, 9): both regimes of the drawn case and the planted case built on it."""
    shape = fr.SHAPES[2]
    for regime in br.REGIMES:
        yield (regime,) + br.case(shape, "drawn", regime)
    yield ("planted",) + br.planted_case()[:3]


@pytest.mark.parametrize("mutant", qr.MUTANTS)
def test_every_mutant_is_told_apart(mutant):
    """On fr.SHAPES[2] a kernel with this mistake misses the loss bar or the gradient bar of tests/test_gpu_quality_loss.py (normalize="pos",
    beta = 2.5 so that an ignored exponent shows; kink anchors left out as there), while the reference is 0 bars from itself."""
    nt, twh, told = 25, br.template_wh(25), []
    for name, out, cm, rm in _mutant_inputs():
        kink = br.kink_mask(out, cm, rm, nt)
        for reg_loss in ("smooth_l1", "giou"):
            ref = qr.quality_loss(out, cm, rm, nt, reg_loss, twh, 2.5)
            bad = qr.quality_loss(out, cm, rm, nt, reg_loss, twh, 2.5, mutant=mutant)
            assert qr.worst_ratios([ref["cls"], ref["reg"], ref["qsum"]], ref["grad"], ref, "pos", kink) == (0.0, 0.0)
            lr, gr = qr.worst_ratios([bad["cls"], bad["reg"], ref["qsum"]], bad["grad"], ref, "pos", kink)
            print(f"{mutant} {name} {reg_loss}: loss {lr:.3g} bars, gradient {gr:.3g} bars")
            told.append(not max(lr, gr) <= 1.0)
    assert any(told), mutant
    if mutant != "q_unclamped_sizes":                                  # (only a positive beyond the clamp that still overlaps can show that one)
        assert all(told[:4]), (mutant, told)                           # ... every other one shows on the drawn case itself, in both regimes


def test_planted_equal_boxes_give_q_one_and_disjoint_boxes_train_like_a_negative():
    out, cm, rm, where = br.planted_case()
    nt = 25
    ref = qr.quality_loss(out, cm, rm, nt)
    loss4, by_hand = qr.quality_grad_formula(out, cm, rm, nt)
    _, by_hand32 = qr.quality_grad_formula(out, cm, rm, nt, dtype=torch.float32)
    for b, t, y, x in where["equal"]:
        assert abs(float(ref["q"][b, t, y, x]) - 1.0) <= 1e-12
    assert bool(torch.isfinite(by_hand32).all())
    far = where["px+"] + where["px-"]
    assert far and all(float(ref["q"][i]) == 0.0 for i in far)
    # the same anchors under a -1 label: the same classification term and the same class gradient (the normaliser is off: npos changes)
    a = qr.quality_loss(out, cm, rm, nt, normalize="none")
    cm2 = cm.clone()
    for i in far:
        cm2[i] = -1.0
    b_ = qr.quality_loss(out, cm2, rm, nt, normalize="none")
    assert abs(a["cls"] - b_["cls"]) <= 1e-12 * abs(a["cls"])
    for b, t, y, x in far:
        assert float(a["grad"][b, t, y, x]) == float(b_["grad"][b, t, y, x]) != 0.0
    assert float(loss4[2]) == pytest.approx(ref["qsum"], rel=1e-12)


def test_the_extreme_case_is_finite_and_carries_qualities_inside_the_unit_interval():
    out, cm, rm = qr.extreme_case()
    ref = qr.quality_loss(out, cm, rm, 25)
    big = (out[:, :25].abs() >= 100) & (cm > 0)
    assert int(big.sum()) == 8 and bool(((ref["q"][big] > 0.05) & (ref["q"][big] < 1.0)).all())
    for dtype in (torch.float64, torch.float32):
        for beta in (1.0, 2.0, 2.5):
            loss4, g = qr.quality_grad_formula(out, cm, rm, 25, beta=beta, dtype=dtype)
            assert bool(torch.isfinite(loss4).all()) and bool(torch.isfinite(g).all())


# ------------------------------------------------------------------------------------------------------------------- float32 against float64
def _float32_ratios(shape, regime, beta, band=None):
    nt = shape[1]
    out, cm, rm = br.case(shape, "drawn", regime)
    twh, kink = br.template_wh(nt), br.kink_mask(out, cm, rm, nt)
    worst = (0.0, 0.0, 0.0)
    for reg_loss in ("smooth_l1", "giou"):
        for normalize in fr.NORMALIZE:
            ref = qr.quality_loss(out, cm, rm, nt, reg_loss, twh, beta, normalize)
            loss4, g = qr.quality_grad_formula(out, cm, rm, nt, reg_loss, twh, beta, normalize, dtype=torch.float32)
            mask = qr.band_mask(ref, out, nt, band) & (cm != 0) if band is not None else None
            lr, gr = qr.worst_ratios(loss4, g, ref, normalize, kink, mask)
            left = 0.0 if mask is None else float(mask.sum()) / max(1, int((cm != 0).sum()))
            worst = (max(worst[0], lr), max(worst[1], gr), max(worst[2], left))
    return worst


@pytest.mark.parametrize("beta", qr.BETAS)
def test_the_float32_formula_stays_inside_the_bars(beta):
    """The kernel's operations in float32 against the float64 reference on fr.SHAPES[1:] x {drawn, near}, in units of the bars (focal_ref.bars:
    rtol 1e-5, atol 1e-6 / max(1, npos_b); loss sums rtol 1e-5).  Measured with torch on the CPU: the worst gradient error is 0.14 of the bar
    at beta = 2, 0.16 at 2.5 and 0.23 at 4; the loss sums stay under 0.01 of theirs.  The figures go to the tests' report file (gpu_util.report),
    from which profiles/quality_loss_parity.txt is put together."""
    for shape in fr.SHAPES[1:]:
        for regime in br.REGIMES:
            lr, gr, _ = _float32_ratios(shape, regime, beta)
            print(f"float32 formula beta {beta:g} {IDS(shape)} {regime}: loss {lr:.3g} bars, gradient {gr:.3g} bars")
            report(f"quality_loss_float32_formula[{IDS(shape)},{regime},beta {beta:g}]", loss_err_over_bar=lr, grad_err_over_bar=gr)
            assert lr < 1.0 and gr < 1.0, (shape, regime, beta, lr, gr)


@pytest.mark.parametrize("beta", qr.LOW_BETAS)
def test_below_two_the_float32_formula_stays_inside_the_bars_outside_the_band_around_the_target(beta):
    """1 <= beta < 2: |d|^(beta - 1) has an unbounded slope at d = sigma - q = 0 (a jump for beta = 1), so the bar applies outside the labelled
    anchors with |sigma - q| < 0.05 in the reference, and those are at most 10 % of the labelled anchors (the reference leaves out 3.1 - 3.9 %)."""
    for shape in (fr.SHAPES[2], fr.SHAPES[3]):
        for regime in br.REGIMES:
            lr, gr, left = _float32_ratios(shape, regime, beta, qr.BAND)
            _, gr_all, _ = _float32_ratios(shape, regime, beta)
            print(f"float32 formula beta {beta:g} {IDS(shape)} {regime}: loss {lr:.3g} bars, gradient {gr:.3g} bars outside the band ({gr_all:.3g} with "
                  f"it), {100 * left:.2f} % of the labelled anchors left out")
            report(f"quality_loss_float32_formula[{IDS(shape)},{regime},beta {beta:g}]", loss_err_over_bar=lr, grad_err_over_bar=gr,
                   grad_err_over_bar_with_band=gr_all, band_share=left)
            assert left <= 0.10, (shape, regime, left)
            assert lr < 1.0 and gr < 1.0, (shape, regime, beta, lr, gr)


# ------------------------------------------------------------------------------------------------------------------- the C entry point
def test_entry_point_refuses_bad_arguments_without_launching(hip):
    """tf_criterion_quality_fwd_bwd checks on the host before anything is enqueued.  Runs without a GPU."""
    l = hip.lib()
    ERR_ARG, ERR_WORKSPACE = -1, -4
    names = {"tf_criterion_quality_workspace_bytes", "tf_criterion_quality_fwd_bwd"}
    assert l.tf_version() >= 790 and names <= set(hip.symbols()) and names <= set(hip._SIGNATURES)
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    need = l.tf_criterion_quality_workspace_bytes(2, 25, 9, 9)
    nblk = -(-25 * 81 // 1024)
    assert need >= 2 * nblk * (24 + 4) and need % 256 == 0
    # one double per block more than the focal pass (each of the two regions is rounded up to 256 bytes)
    blocks = 12 * -(-25 * 63 * 63 // 1024)
    a256 = lambda n: (n + 255) & ~255
    assert l.tf_criterion_quality_workspace_bytes(12, 25, 63, 63) == a256(blocks * 24) + a256(blocks * 4)
    assert l.tf_criterion_focal_workspace_bytes(12, 25, 63, 63) == a256(blocks * 16) + a256(blocks * 4)
    assert l.tf_criterion_quality_workspace_bytes(0, 25, 9, 9) == 0

    def call(out=p, cm=p, rm=p, B=2, nt=25, H=9, W=9, beta=2.0, normalize=1, reg_weight=1.0, reg_form=0, twh=None, grad=p, loss=p, npos=p, ws=p,
             wsb=need):
        return l.tf_criterion_quality_fwd_bwd(out, cm, rm, B, nt, H, W, beta, normalize, reg_weight, reg_form, twh, grad, loss, npos, ws, wsb, None)

    for name in ("out", "cm", "rm", "grad", "loss"):
        assert call(**{name: None}) == ERR_ARG, name
    for name in ("B", "nt", "H", "W"):
        for bad in (0, -3):
            assert call(**{name: bad}) == ERR_ARG, name
    for name, values in (("beta", (0.999, 0.0, -2.0, float("nan"), float("inf"), float("-inf"))), ("reg_weight", (float("nan"), float("inf"))),
                         ("normalize", (-1, 2)), ("reg_form", (-1, 4, 17))):
        for bad in values:
            assert call(**{name: bad}) == ERR_ARG, (name, bad)
    assert call(reg_form=3, twh=None) == ERR_ARG                      # diou without the template table
    for form in (0, 1, 2):
        assert call(reg_form=form, ws=None) == ERR_WORKSPACE          # judged fine, stopped at the workspace
    assert call(beta=1.0, ws=None) == ERR_WORKSPACE
    assert call(reg_form=3, twh=p, wsb=need - 1) == ERR_WORKSPACE and call(wsb=0) == ERR_WORKSPACE
    assert call(out=None, ws=None) == ERR_ARG                         # the arguments are judged before the workspace
    assert not any(buf)                                               # nothing was written


def test_ops_wrapper_signature_and_refusals():
    from tinyfaces import ops
    ps = inspect.signature(ops.criterion_quality_fwd_bwd).parameters
    assert list(ps) == ["output", "class_map", "regression_map", "n_templates", "reg_weight", "beta", "normalize", "reg_loss", "template_wh", "grad"]
    assert tuple(ps[k].default for k in list(ps)[3:]) == (25, 1.0, 2.0, "pos", "smooth_l1", None, None)
    ops.check_qfl(1.0, "none")
    ops.check_qfl(2, "pos")
    for bad in ((0.5, "pos"), (float("nan"), "pos"), (float("inf"), "pos"), (-1.0, "pos"), ("2", "pos"), (2.0, "batch")):
        with pytest.raises(ValueError, match="quality focal loss"):
            ops.check_qfl(*bad)
    out, cm, rm = fr.case(fr.SHAPES[0])
    with pytest.raises(RuntimeError, match="no CPU fallback|HIP"):
        ops.criterion_quality_fwd_bwd(out, cm, rm, n_templates=1)


# ------------------------------------------------------------------------------------------------------------------- command line
def test_main_flags_are_parsed_beside_the_other_additions():
    main = _main()
    a = main.trunk_arguments(["TRAIN", "VAL"])
    assert (a.cls_loss, a.qfl_beta, a.reg_loss) == ("soft_margin", 2.0, "smooth_l1")
    assert "soft-margin" in main.loss_description(a)
    a = main.trunk_arguments(["TRAIN", "VAL", "--cls-loss", "qfl", "--qfl-beta", "2.5", "--focal-normalize", "none", "--lr", "0.01", "--accum-steps", "2"])
    assert (a.cls_loss, a.qfl_beta, a.focal_normalize, a.reg_loss, a.lr, a.accum_steps, a.traindata) == ("qfl", 2.5, "none", "smooth_l1", 0.01, 2, "TRAIN")
    d = main.loss_description(a)
    assert "quality focal (beta 2.5, IoU of the predicted box as the target; not normalised" in d and "SmoothL1" in d
    a = main.trunk_arguments(["TRAIN", "VAL", "--reg-loss", "giou", "--cls-loss", "qfl", "--reg-weight", "2"])
    assert (a.cls_loss, a.reg_loss, a.reg_weight, a.qfl_beta) == ("qfl", "giou", 2.0, 2.0)
    d = main.loss_description(a)
    assert "quality focal (beta 2, IoU of the predicted box as the target; per image by its positives" in d and "GIoU" in d and "weight 2" in d
    for form in ("iou", "diou", "smooth-l1"):
        assert main.trunk_arguments(["TRAIN", "VAL", "--cls-loss", "qfl", "--reg-loss", form]).reg_loss == form.replace("-", "_")
    assert main.trunk_arguments(["TRAIN", "VAL", "--cls-loss", "qfl", "--qfl-beta", "1"]).qfl_beta == 1.0
    assert main.trunk_arguments(["TRAIN", "VAL", "--cls-loss", "focal", "--reg-loss", "giou"]).cls_loss == "focal"
    for bad in (["--qfl-beta", "0.5"], ["--qfl-beta", "nan"], ["--qfl-beta", "inf"], ["--qfl-beta", "x"], ["--cls-loss", "hinge"], ["--cls-loss", "QFL"],
                ["--reg-loss", "giou"], ["--reg-loss", "giou", "--cls-loss", "soft-margin"]):
        with pytest.raises(SystemExit):
            main.trunk_arguments(["TRAIN", "VAL"] + bad)
    plain = vars(main.arguments(["TRAIN", "VAL"]))                     # `arguments` keeps today's names
    assert not {"cls_loss", "qfl_beta"} & set(plain)
    for extra in (["--cls-loss", "qfl"], ["--qfl-beta", "2"]):
        with pytest.raises(SystemExit):
            main.arguments(["TRAIN", "VAL"] + extra)
    assert "--qfl-beta" in main.QFL_HELP and "--cls-loss qfl" in main.QFL_HELP


# ------------------------------------------------------------------------------------------------------------------- the criterion
def test_criterion_keywords_defaults_and_value_errors():
    from tinyfaces.datasets.templates import load_templates
    from tinyfaces.models.loss import AvgMeter, DetectionCriterion
    ps = inspect.signature(DetectionCriterion.__init__).parameters
    assert ps["qfl_beta"].default == 2.0 and ps["cls_loss"].default == "soft_margin"
    assert DetectionCriterion.CLS_LOSSES == ("soft_margin", "focal", "qfl")
    c = DetectionCriterion(25)
    assert (c.cls_loss, c.qfl_beta) == ("soft_margin", 2.0) and isinstance(c.quality_average, AvgMeter)
    q = DetectionCriterion(25, cls_loss="qfl", qfl_beta=3, focal_normalize="none")
    assert (q.cls_loss, q.qfl_beta, q.focal_normalize, q.reg_loss) == ("qfl", 3.0, "none", "smooth_l1")
    for form in ("iou", "giou"):
        assert DetectionCriterion(25, cls_loss="qfl", reg_loss=form).reg_loss == form
    d = DetectionCriterion(25, cls_loss="qfl", reg_loss="diou", templates=load_templates())
    assert d._template_wh.shape == (25, 2) and not list(d.buffers()) and not d.state_dict()
    for kw in (dict(qfl_beta=0.5), dict(qfl_beta=float("nan")), dict(qfl_beta=float("inf")), dict(qfl_beta=-2.0), dict(focal_normalize="batch"),
               dict(reg_loss="diou"), dict(reg_loss="ciou")):
        with pytest.raises(ValueError):
            DetectionCriterion(25, cls_loss="qfl", **kw)
    for form in ("iou", "giou", "diou"):                                # still refused with the soft-margin pass, in the words it always used
        with pytest.raises(ValueError, match="soft-margin pass"):
            DetectionCriterion(25, reg_loss=form, templates=load_templates())
    with pytest.raises(RuntimeError, match="inject_sampling"):
        q.inject_sampling(torch.ones(1, 15, dtype=torch.uint8), torch.ones(1, 15, dtype=torch.uint8))
    c.inject_sampling(None, None)


def test_the_criterion_dispatches_on_cls_loss(monkeypatch):
    """With every op replaced by a recorder: the default criterion and the focal criteria make exactly the calls they make today, qfl makes the
    new call with (out, cm, rm, nt, reg_weight, beta, normalize, reg_loss, template_wh) and returns class_map as the labels."""
    from tinyfaces import ops
    from tinyfaces.datasets.templates import load_templates
    from tinyfaces.models.loss import DetectionCriterion
    calls = []
    loss2, loss4, grad = torch.zeros(2, dtype=torch.float64), torch.zeros(4, dtype=torch.float64), torch.zeros(1)

    def recorder(kind):
        def f(*a, **kw):
            calls.append((kind, a, kw))
            return (loss4 if kind == "criterion_quality_fwd_bwd" else loss2), grad, ("sampled" if kind == "criterion_fwd_bwd" else torch.zeros(1, dtype=torch.int32))
        return f

    for name in ("criterion_fwd_bwd", "criterion_focal_fwd_bwd", "criterion_focal_box_fwd_bwd", "criterion_quality_fwd_bwd"):
        monkeypatch.setattr(ops, name, recorder(name))
    out, cm, rm = torch.zeros(1), object(), object()
    c = DetectionCriterion(25, reg_weight=2, seed=5)
    assert c._fwd_bwd(out, cm, rm, want_labels=True) == (loss2, grad, "sampled")
    kind, a, kw = calls.pop()
    assert kind == "criterion_fwd_bwd" and a == (out, cm, rm, 25, 2, 0.03, 128, 128, None, None, (5 * 0x9E3779B97F4A7C15 + 1) & (2**64 - 1)) \
        and kw == {"want_labels": True} and not calls
    f = DetectionCriterion(25, reg_weight=2, cls_loss="focal", focal_gamma=1.5, focal_alpha=0.3, focal_normalize="none", qfl_beta=3.0)
    assert f._fwd_bwd(out, cm, rm)[2] is cm
    kind, a, kw = calls.pop()
    assert kind == "criterion_focal_fwd_bwd" and a == (out, cm, rm, 25, 2, 1.5, 0.3, "none") and kw == {} and not calls
    g = DetectionCriterion(25, reg_weight=3, cls_loss="focal", reg_loss="giou")
    g._fwd_bwd(out, cm, rm)
    kind, a, kw = calls.pop()
    assert kind == "criterion_focal_box_fwd_bwd" and a == (out, cm, rm, 25, 3, 2.0, 0.25, "pos", "giou", None) and kw == {} and not calls
    q = DetectionCriterion(25, reg_weight=2, cls_loss="qfl", qfl_beta=2.5, focal_normalize="none", focal_gamma=7.0, focal_alpha=0.9)
    got = q._fwd_bwd(out, cm, rm)
    assert got[0] is loss4 and got[1] is grad and got[2] is cm and q._calls == 0
    kind, a, kw = calls.pop()
    assert kind == "criterion_quality_fwd_bwd" and a == (out, cm, rm, 25, 2, 2.5, "none", "smooth_l1", None) and kw == {} and not calls
    d = DetectionCriterion(25, cls_loss="qfl", reg_loss="diou", templates=load_templates())
    d._fwd_bwd(out, cm, rm)
    kind, a, kw = calls.pop()
    assert kind == "criterion_quality_fwd_bwd" and a[:8] == (out, cm, rm, 25, 1, 2.0, "pos", "diou") and torch.equal(a[8], ops.template_wh(load_templates()))
    q.cls_loss = "hinge"                                              # set behind the constructor's back
    with pytest.raises(ValueError, match="cls_loss"):
        q._fwd_bwd(out, cm, rm)
    assert not calls


def test_the_quality_meter_is_the_mean_iou_over_all_positives_seen():
    """flush_meters on loss vectors of four elements: update(sum q, sum npos), skipped for a batch without a positive; vectors of two elements
    (the other losses) leave the meter alone."""
    from tinyfaces.models.loss import DetectionCriterion
    c = DetectionCriterion(25, cls_loss="qfl", lazy_meters=True)
    t = lambda *v: torch.tensor(v, dtype=torch.float64)
    c._pending += [(t(4.0, 2.0, 1.5, 3.0), 2), (t(1.0, 0.0, 0.0, 0.0), 2), (t(2.0, 1.0, 4.5, 9.0), 4)]
    c.flush_meters(lag=1)
    assert (c.quality_average.average, c.quality_average.num_averaged) == (0.5, 3) and len(c._pending) == 1
    assert c.class_average.num_averaged == 4 and c.class_average.average == 5.0 / 4 and c.reg_average.average == 2.0 / 4
    c.flush_meters()
    assert c.quality_average.num_averaged == 12 and c.quality_average.average == pytest.approx(6.0 / 12, abs=1e-15)
    assert c.class_average.num_averaged == 8 and c.reg_average.average == pytest.approx(3.0 / 8)
    c.reset()
    assert (c.quality_average.average, c.quality_average.num_averaged, c.class_average.num_averaged) == (0, 0, 0)
    f = DetectionCriterion(25, cls_loss="focal", lazy_meters=True)
    f._pending.append((t(4.0, 2.0), 2))
    f.flush_meters()
    assert f.quality_average.num_averaged == 0 and f.class_average.average == 2.0


def test_print_quality_prints_for_qfl_only(capsys):
    from tinyfaces import trainer
    from tinyfaces.models.loss import DetectionCriterion
    q = DetectionCriterion(25, cls_loss="qfl")
    trainer.print_quality(0, 0, 2, q)                                  # no positive seen yet
    trainer.print_quality(0, 0, 2, DetectionCriterion(25, cls_loss="focal"))
    trainer.print_quality(0, 0, 2, DetectionCriterion(25))
    assert capsys.readouterr().out == ""
    q.quality_average.update(1.5, 4)
    trainer.print_quality(1, 3, 2, q)
    assert capsys.readouterr().out == "Epoch: [3][1/2]\tmean IoU of positives 0.3750 (4 positives)\n"
