"""Focal loss for DetectionCriterion, everything that needs no GPU: the float64 reference (tests/focal_ref.py) against itself -- its
hand-derived gradient against autograd, its degenerate case against the existing loss --, that the inputs of
tests/test_gpu_focal_loss.py tell every plausible kernel mistake apart by at least 100 times that file's bars, the host-side
refusals of tf_criterion_focal_fwd_bwd, the command-line flags and the criterion's own checks."""
import ctypes as C
import importlib.util
import inspect
import os

import pytest
import torch

import focal_ref as fr
import loss_cases as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tiny-faces-pytorch_amd")
SMALL = fr.SHAPES[:3]


def _main():
    spec = importlib.util.spec_from_file_location("our_cli_main_focal", os.path.join(PKG, "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("shape", SMALL + (fr.SHAPES[3],), ids=str)
def test_the_hand_derived_gradient_is_the_autograd_gradient(shape):
    out, cm, rm = fr.case(shape)
    for gamma, alpha in fr.PARAMS:
        for normalize in fr.NORMALIZE:
            ref = fr.focal_loss(out, cm, rm, shape[1], gamma, alpha, normalize, reg_weight=0.7)
            by_hand = fr.focal_grad_formula(out, cm, rm, shape[1], gamma, alpha, normalize, reg_weight=0.7)
            assert torch.allclose(by_hand, ref["grad"], rtol=1e-12, atol=1e-15), (gamma, alpha, normalize)
            assert torch.equal(ref["npos"], (cm == 1).reshape(shape[0], -1).sum(1))


def test_extreme_logits_stay_finite_in_the_reference():
    out, cm, rm = fr.extreme_case()
    assert float(out[:, :25].abs().max()) == 1e4
    for gamma, alpha in fr.PARAMS:
        ref = fr.focal_loss(out, cm, rm, 25, gamma, alpha, "pos")
        assert all(bool(torch.isfinite(ref[k]).all()) for k in ("grad", "cls_per_image", "reg_per_image"))
        assert torch.allclose(fr.focal_grad_formula(out, cm, rm, 25, gamma, alpha, "pos"), ref["grad"], rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize("shape", SMALL + (fr.SHAPES[3],), ids=str)
@pytest.mark.parametrize("variant", fr.VARIANTS)
def test_gamma_0_without_alpha_or_normaliser_is_the_soft_margin_loss_on_the_labels_as_given(shape, variant):
    out, cm, rm = fr.case(shape, variant)
    ref = fr.focal_loss(out, cm, rm, shape[1], 0.0, -1.0, "none", reg_weight=1.0)
    cls, reg, grad = lc.float64_loss(out, cm, rm, shape[1])
    assert abs(ref["cls"] - cls) <= 1e-12 * abs(cls) and abs(ref["reg"] - reg) <= 1e-12 * abs(reg)
    assert float((ref["grad"] - grad).abs().max()) <= 2e-9


def _visible(mutant, shape):
    """A mutant of the normalisation needs two images with positives to differ from a per-image one."""
    return mutant != "batch_normaliser" or shape[0] > 1


@pytest.mark.parametrize("mutant", fr.MUTANTS)
def test_every_mutant_is_at_least_100_bars_away_on_the_gpu_tests_inputs(mutant):
    """On the inputs tests/test_gpu_focal_loss.py runs ((gamma, alpha) = (2, 0.25), normalize="pos", the drawn labels of every shape),
    a kernel with this mistake misses the loss bar or the gradient bar by a factor of at least 100."""
    for shape in fr.SHAPES:
        if not _visible(mutant, shape):
            continue
        out, cm, rm = fr.case(shape)
        ref = fr.focal_loss(out, cm, rm, shape[1], 2.0, 0.25, "pos")
        bad = fr.focal_loss(out, cm, rm, shape[1], 2.0, 0.25, "pos", mutant=mutant)
        loss_ratio, grad_ratio = fr.worst_ratios([bad["cls"], bad["reg"]], bad["grad"], ref, "pos")
        assert max(loss_ratio, grad_ratio) >= 100.0, (mutant, shape, loss_ratio, grad_ratio)
        # ... and the reference itself is 0 bars away from itself
        assert fr.worst_ratios([ref["cls"], ref["reg"]], ref["grad"], ref, "pos") == (0.0, 0.0)


def test_the_drawn_cases_are_what_the_gpu_tests_say_they_are():
    for shape in fr.SHAPES:
        B, nt, H, W = shape
        E = nt * H * W
        npos = [(fr.case(shape, v)[1] == 1).reshape(B, -1).sum(1).tolist() for v in fr.VARIANTS]
        assert len(set(npos[0])) == B and (B == 1 or 0 in npos[0]), shape         # the counts differ and include 0
        assert npos[1][0] == 0 and int((fr.case(shape, "no_positive")[1][0] == -1).sum()) > 0
        assert not fr.case(shape, "no_label")[1][0].any()
        assert int((fr.case(shape, "fully_labelled")[1][0] != 0).sum()) == E
    assert [s[1] * s[2] * s[3] for s in fr.SHAPES[:3]] == [15, 1024, 2025]
    assert fr.SHAPES[3][0] * -(-fr.SHAPES[3][1] * 52 * 52 // 1024) == 335 and -(-fr.SHAPES[4][1] * 103 * 103 // 1024) > 256


def test_entry_point_refuses_bad_arguments_without_launching(hip):
    """tf_criterion_focal_fwd_bwd checks on the host before anything is enqueued.  Runs without a GPU."""
    l = hip.lib()
    ERR_ARG, ERR_WORKSPACE = -1, -4
    assert l.tf_version() >= 690
    assert {"tf_criterion_focal_workspace_bytes", "tf_criterion_focal_fwd_bwd"} <= set(hip.symbols())
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    need = l.tf_criterion_focal_workspace_bytes(2, 25, 9, 9)
    nblk = -(-25 * 81 // 1024)
    assert need >= 2 * nblk * (16 + 4) and need % 256 == 0
    assert l.tf_criterion_focal_workspace_bytes(12, 25, 63, 63) > need

    def call(out=p, cm=p, rm=p, B=2, nt=25, H=9, W=9, gamma=2.0, alpha=0.25, normalize=1, grad=p, loss=p, npos=p, ws=p, wsb=need):
        return l.tf_criterion_focal_fwd_bwd(out, cm, rm, B, nt, H, W, gamma, alpha, normalize, 1.0, grad, loss, npos, ws, wsb, None)

    for name in ("out", "cm", "rm", "grad", "loss"):
        assert call(**{name: None}) == ERR_ARG, name
    for name in ("B", "nt", "H", "W"):
        for bad in (0, -3):
            assert call(**{name: bad}) == ERR_ARG, name
    for bad in (-0.5, float("nan"), float("inf")):
        assert call(gamma=bad) == ERR_ARG, bad
    for bad in (1.5, float("nan"), float("inf"), float("-inf")):
        assert call(alpha=bad) == ERR_ARG, bad
    for bad in (-1, 2, 7):
        assert call(normalize=bad) == ERR_ARG, bad
    assert call(ws=None) == ERR_WORKSPACE
    assert call(wsb=need - 1) == ERR_WORKSPACE and call(wsb=0) == ERR_WORKSPACE
    assert call(out=None, ws=None) == ERR_ARG                       # the arguments are judged before the workspace
    assert not any(buf)                                             # nothing was written


def test_ops_wrapper_signature_and_refusals():
    from tinyfaces import ops
    ps = inspect.signature(ops.criterion_focal_fwd_bwd).parameters
    assert list(ps) == ["output", "class_map", "regression_map", "n_templates", "reg_weight", "gamma", "alpha", "normalize", "grad"]
    assert (ps["n_templates"].default, ps["reg_weight"].default, ps["gamma"].default, ps["alpha"].default, ps["normalize"].default,
            ps["grad"].default) == (25, 1.0, 2.0, 0.25, "pos", None)
    out, cm, rm = fr.case(fr.SHAPES[0])
    with pytest.raises(RuntimeError, match="no CPU fallback|HIP"):
        ops.criterion_focal_fwd_bwd(out, cm, rm, n_templates=1)


def test_main_flags_are_parsed_beside_the_other_additions():
    main = _main()
    a = main.trunk_arguments(["TRAIN", "VAL"])
    assert (a.cls_loss, a.focal_gamma, a.focal_alpha, a.focal_normalize) == ("soft_margin", 2.0, 0.25, "pos")
    a = main.trunk_arguments(["TRAIN", "VAL", "--cls-loss", "focal", "--focal-gamma", "1.5", "--focal-alpha", "-1", "--focal-normalize", "none",
                              "--lr", "0.01", "--accum-steps", "2"])
    assert (a.cls_loss, a.focal_gamma, a.focal_alpha, a.focal_normalize) == ("focal", 1.5, -1.0, "none")
    assert a.lr == 0.01 and a.accum_steps == 2 and a.traindata == "TRAIN" and a.ohem_thresh == 0.03
    assert "focal" in main.loss_description(a) and "no alpha weighting" in main.loss_description(a)
    assert "soft-margin" in main.loss_description(main.trunk_arguments(["TRAIN", "VAL"]))
    for bad in (["--cls-loss", "hinge"], ["--focal-gamma", "-1"], ["--focal-gamma", "nan"], ["--focal-alpha", "1.5"], ["--focal-alpha", "inf"],
                ["--focal-normalize", "batch"]):
        with pytest.raises(SystemExit):
            main.trunk_arguments(["TRAIN", "VAL"] + bad)
    # `arguments` resolves today's names only
    plain = vars(main.arguments(["TRAIN", "VAL"]))
    assert not {"cls_loss", "focal_gamma", "focal_alpha", "focal_normalize"} & set(plain)
    with pytest.raises(SystemExit):
        main.arguments(["TRAIN", "VAL", "--cls-loss", "focal"])
    assert "--cls-loss" in main.arguments.__globals__["FOCAL_HELP"]


def test_criterion_keywords_defaults_and_value_errors():
    from tinyfaces.models.loss import DetectionCriterion
    ps = inspect.signature(DetectionCriterion.__init__).parameters
    assert (ps["cls_loss"].default, ps["focal_gamma"].default, ps["focal_alpha"].default, ps["focal_normalize"].default) == \
        ("soft_margin", 2.0, 0.25, "pos")
    c = DetectionCriterion(25)
    assert c.cls_loss == "soft_margin" and (c.max_pos, c.max_neg, c.ohem_thresh) == (128, 128, 0.03)
    f = DetectionCriterion(25, cls_loss="focal", focal_gamma=1, focal_alpha=-1, focal_normalize="none")
    assert (f.cls_loss, f.focal_gamma, f.focal_alpha, f.focal_normalize) == ("focal", 1.0, -1.0, "none")
    for kw in (dict(cls_loss="hinge"), dict(focal_normalize="batch"), dict(focal_gamma=-0.1), dict(focal_gamma=float("nan")),
               dict(focal_alpha=1.01), dict(focal_alpha=float("inf"))):
        with pytest.raises(ValueError):
            DetectionCriterion(25, cls_loss=kw.pop("cls_loss", "focal"), **kw)
    with pytest.raises(RuntimeError, match="inject_sampling"):
        f.inject_sampling(torch.ones(1, 15, dtype=torch.uint8), torch.ones(1, 15, dtype=torch.uint8))
    c.inject_sampling(None, None)                                   # the default criterion keeps its parity hook


def test_the_criterion_dispatches_on_cls_loss(monkeypatch):
    """_fwd_bwd, which the autograd function and TrainEngine.step both call: the default criterion makes today's call of
    ops.criterion_fwd_bwd and never touches the focal entry point; the focal criterion makes the focal call, consumes no seed and
    reports the class_map it was given as the labels that entered."""
    from tinyfaces import ops
    from tinyfaces.models.loss import DetectionCriterion
    calls = []
    loss2, grad = torch.zeros(2, dtype=torch.float64), torch.zeros(1)

    def soft(*a, **kw):
        calls.append(("soft", a, kw))
        return loss2, grad, "sampled"

    def focal(*a, **kw):
        calls.append(("focal", a, kw))
        return loss2, grad, torch.zeros(1, dtype=torch.int32)

    monkeypatch.setattr(ops, "criterion_fwd_bwd", soft)
    monkeypatch.setattr(ops, "criterion_focal_fwd_bwd", focal)
    out, cm, rm = object(), object(), object()
    c = DetectionCriterion(25, reg_weight=2, seed=5)
    assert c._fwd_bwd(out, cm, rm, want_labels=True) == (loss2, grad, "sampled")
    kind, a, kw = calls.pop()
    assert kind == "soft" and a[:3] == (out, cm, rm) and a[3:10] == (25, 2, 0.03, 128, 128, None, None) and kw == {"want_labels": True}
    assert c._calls == 1 and a[10] == (5 * 0x9E3779B97F4A7C15 + 1) & (2**64 - 1)
    f = DetectionCriterion(25, reg_weight=2, cls_loss="focal", focal_gamma=1.5, focal_alpha=0.3, focal_normalize="none")
    got = f._fwd_bwd(out, cm, rm)
    assert got[0] is loss2 and got[1] is grad and got[2] is cm
    kind, a, kw = calls.pop()
    assert kind == "focal" and a == (out, cm, rm, 25, 2, 1.5, 0.3, "none") and kw == {} and f._calls == 0 and not calls
    f.cls_loss = "hinge"                                            # set behind the constructor's back: refused, not read as the default
    with pytest.raises(ValueError, match="cls_loss"):
        f._fwd_bwd(out, cm, rm)
    assert not calls


def test_engine_step_goes_through_the_criterion(monkeypatch):
    """TrainEngine.step with its device side replaced by recorders: a default criterion reaches ops.criterion_fwd_bwd while the focal entry
    point raises if touched; a focal criterion reaches the focal entry point while the other raises."""
    from tinyfaces import ops
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as zoo
    from tinyfaces.models.loss import DetectionCriterion

    def boom(*a, **kw):
        raise AssertionError("the other criterion's entry point was called")

    for cls_loss, mine, other in (("soft_margin", "criterion_fwd_bwd", "criterion_focal_fwd_bwd"),
                                  ("focal", "criterion_focal_fwd_bwd", "criterion_fwd_bwd")):
        eng = TrainEngine(zoo.DetectionModel(base_model=zoo.resnet50, num_templates=25), DetectionCriterion(25, cls_loss=cls_loss), device="cpu")
        m, seen = eng.model, []
        monkeypatch.setattr(m, "_check_partial_freeze", lambda: None)
        monkeypatch.setattr(m, "_sync_tables", lambda dev: None)
        monkeypatch.setattr(m, "_run_forward", lambda x, training=True: "OUT")
        monkeypatch.setattr(m, "_run_backward", lambda x, g, persistent=False, eng=eng: torch.zeros(eng.flat_p.numel()))
        monkeypatch.setattr(ops, mine, lambda *a, **kw: seen.append(a[:3]) or (torch.ones(2, dtype=torch.float64), None, None))
        monkeypatch.setattr(ops, other, boom)
        monkeypatch.setattr(ops, "sgd_step", lambda *a, **kw: None)
        loss2 = eng.step(torch.zeros(1, 3, 8, 8), "CM", "RM")
        assert seen == [("OUT", "CM", "RM")] and loss2.tolist() == [1.0, 1.0] and eng.steps == 1
