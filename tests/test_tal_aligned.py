"""CPU: TOOD's task-aligned loss -- step 7 of the task-aligned assignment and the aligned form of the criterion -- as far as it can be held
without a GPU: the restatement (tests/tal_aligned_ref.py) against its own identities, its mutants against the bars the kernels are held to in
tests/test_gpu_tal_aligned.py, the refusals of the two C entry points on host pointers, the Python surface and main.py's flags."""
import ctypes as C
import inspect
import json
import os

import numpy as np
import pytest
import torch

import box_loss_ref as br
import tal_aligned_ref as ar
import tal_cases as tc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ------------------------------------------------------------------------------------------------------------------ step 7, the restatement
ALL_PLANTED = tuple(ar.planted()) + ar.FROM_TAL_CASES


@pytest.mark.parametrize("name", ALL_PLANTED)
def test_planted_identities(name):
    """No planted face is ambiguous; the winner holding M_g gets exactly (float)U_g; a face with one winner gets (float)u; every target lies in
    [0, U_g]; everything that was not won is exactly 1; the two maps and match_count are tal_ref's."""
    case, ref = ar.planted_case(name), ar.planted_reference(name)
    assert ar.ambiguous(ref) == 0
    plain = tc.restate(case)
    for r, p in zip(ref, plain):
        assert np.array_equal(r["cm"], p[0]) and np.array_equal(r["rm"], p[1]) and np.array_equal(r["counts"], p[2])
        assert np.array_equal(r["won"], (r["cm"] == 1) & r["won"]) and int(r["won"].sum()) == int(r["counts"].sum())
        assert (r["align"][~r["won"]] == 1).all()
        flat = r["align"].reshape(-1)
        for g, f in enumerate(r["faces"]):
            own = sorted(r["owners"][g])
            if not own:
                assert r["M"][g] == 0 and r["U"][g] == 0
                continue
            v = flat[f["winners"][own]]
            assert (v >= 0).all() and (v <= np.float32(r["U"][g])).all()
            if r["M"][g] > 0:
                best = own[int(np.argmax(f["m"][own]))]
                assert flat[f["winners"][best]] == np.float32(r["U"][g])
            else:
                assert (v == 0).all()
            if len(own) == 1 and r["M"][g] > 0:
                assert v[0] == np.float32(f["u"][own[0]])


def test_the_cases_the_issue_names_are_what_they_say():
    r = ar.planted_reference("loser loses its best m")[0]
    a, fa = r["faces"][0], r["owners"][0]
    best = int(np.argmax(a["m"]))
    assert a["winners"][best] == 3 * 11 + 4 and best not in fa and 0 < len(fa) < len(a["winners"])          # face A lost its best-m anchor, to face B
    assert a["m"].max() > 1.3 * r["M"][0] and r["counts"][1] == 3                        # the maxima before and after the conflict differ
    r2 = ar.planted_reference("loser loses its best m, other order")[0]
    assert np.array_equal(r["align"], r2["align"]) and r2["counts"].tolist() == r["counts"].tolist()[::-1]
    r = ar.planted_reference("conflict by u")[0]
    assert 0 in r["counts"].tolist() and r["counts"].sum() > 0                           # a face that wins nothing
    assert ar.planted_reference("output 0, topk 1")[0]["counts"].tolist() == [1, 1, 1]    # exactly one winner
    assert ar.planted_reference("256 candidates")[0]["counts"].tolist() == [32]           # topk = 32 with 32 winners
    r = ar.planted_reference("M = 0")[0]
    assert (r["M"] == 0).all() and r["counts"].sum() > 0 and (r["align"][r["won"]] == 0).all() and (r["U"] > 0).all()
    r = ar.planted_reference("6-px face, output 0")[0]
    assert 0 < r["M"][0] < 2e-7 and 0.03 < r["U"][0] < 0.12 and r["counts"].tolist() == [13]
    r = ar.planted_reference("base maps with 0 and +1")[0]
    assert int(((r["cm"] == 1) & ~r["won"]).sum()) == 2                                  # +1 labels the call did not win: their align stays 1
    assert ar.planted_case("257 candidates")["t"].shape[0] > 64


@pytest.mark.parametrize("ci", range(len(ar.RANDOM)))
def test_random_seeds_have_no_ambiguous_face(ci):
    ref = ar.random_reference(ci)
    assert ar.ambiguous(ref) == 0 and sum(int(r["counts"].sum()) for r in ref) > 0
    for r in ref:
        assert (r["align"][~r["won"]] == 1).all() and (r["align"] >= 0).all() and (r["align"] <= 1).all()


def test_one_ulp_of_exp_moves_the_rounded_target_by_at_most_one_step():
    """The reason of the 1-ulp bar: exp moved by one ulp at random (what another math library may return) leaves every decision of these cases
    alone and moves the float32 target by one step at the most."""
    for name in ("loser loses its best m", "four faces, 25 templates", "6-px face, output 0"):
        case, ref = ar.planted_case(name), ar.planted_reference(name)
        for seed in (1, 2):
            other = ar.restate(case, exp=tc.tal_ref.ulp_exp(seed))
            assert all(np.array_equal(a["won"], b["won"]) for a, b in zip(ref, other))
            assert ar.hold_align(np.stack([o["align"] for o in other]), ref, name) <= 1


@pytest.mark.parametrize("mutant", ar.ASSIGN_MUTANTS)
def test_assignment_mutants_fail(mutant):
    """Maxima over the claimed list before conflicts, U_g omitted, maxima per image, mmdetection's + 1e-7: each misses the 1-ulp bar on its case."""
    name = ar.ASSIGN_MUTANT_CASES[mutant]
    case, ref = ar.planted_case(name), ar.planted_reference(name)
    assert ar.hold_align(np.stack([r["align"] for r in ref]), ref, name) == 0
    bad = ar.restate(case, mutant=mutant)
    with pytest.raises(AssertionError):
        ar.hold_align(np.stack([r["align"] for r in bad]), ref, name)
    if mutant == "epsilon":                                             # the header's figure: the epsilon cuts the 6-px face's targets to 0.56 of U_g
        r, b = ref[0], bad[0]
        ratio = b["align"][r["won"]].max() / np.float32(r["U"][0])
        assert 0.5 < ratio < 0.6, ratio


# ------------------------------------------------------------------------------------------------------------------ the loss, the restatement
def test_loss_restatement_identities():
    """align_map = 1 with "pos" is the hard-target quality form, i.e. the focal form with gamma = beta and no alpha (box_loss_ref); q = 0 at a
    positive trains it like a negative and gives its box no gradient; the planted 1.5, -0.5 and NaN are 1, 0 and 0."""
    shape = (2, 25, 9, 9)
    out, cm, rm, al = ar.loss_case(shape, "ones")
    twh = br.template_wh(25)
    for reg_loss in ("iou", "diou"):
        a = ar.aligned_loss(out, cm, rm, al, 25, reg_loss, twh, 2.0, "pos")
        f = br.box_loss(out, cm, rm, 25, reg_loss, twh, gamma=2.0, alpha=-1.0, normalize="pos")
        assert abs(a["cls"] - f["cls"]) <= 1e-12 * abs(f["cls"]) and abs(a["reg"] - f["reg"]) <= 1e-12 * abs(f["reg"])
        assert torch.allclose(a["grad"], f["grad"], rtol=1e-10, atol=1e-14)
    out, cm, rm, al = ar.loss_case(shape, "drawn")
    pos = cm > 0
    q = ar.target(al, pos)
    planted = q.view(2, -1)[0][torch.nonzero(cm.view(2, -1)[0] == 1).flatten()[:5]]
    assert planted.tolist() == [0.0, 1.0, 1.0, 0.0, 0.0]
    ref = ar.aligned_loss(out, cm, rm, al, 25, "giou", None, 2.0, "align")
    zero_q = pos & (q == 0)
    assert int(zero_q.sum()) >= 6 and not bool(ref["grad"][:, 25:][zero_q.repeat(1, 4, 1, 1)].any())
    neg = cm.clone()
    neg[zero_q] = -1
    ref2 = ar.aligned_loss(out, neg, rm, al, 25, "giou", None, 2.0, "none")
    ref1 = ar.aligned_loss(out, cm, rm, al, 25, "giou", None, 2.0, "none")
    assert torch.equal(ref1["grad"], ref2["grad"]) and ref1["cls"] == ref2["cls"]
    # the normaliser: "align" is 1 / max(1, sum of q), clamped on the image whose targets sum below 1 and on the image without positives
    s = ar.aligned_loss(*ar.loss_case(shape, "small_targets"), 25, "smooth_l1", None, 2.0, "align")
    assert float(s["qsum_per_image"][0]) < 1 and float(s["w"][0]) == 1.0 and abs(float(s["w"][1]) - 1 / float(s["qsum_per_image"][1])) < 1e-15
    n = ar.aligned_loss(*ar.loss_case(shape, "no_positive"), 25, "smooth_l1", None, 2.0, "align")
    assert int(n["npos"][0]) == 0 and float(n["w"][0]) == 1.0


@pytest.mark.parametrize("mutant", ar.LOSS_MUTANTS)
def test_loss_mutants_fail(mutant):
    """Regression not weighted by q, npos in place of the sum of q, q from the own box: each misses the bars on a committed case."""
    shape = (2, 25, 9, 9)
    out, cm, rm, al = ar.loss_case(shape, "drawn")
    twh = br.template_wh(25)
    ref = ar.loss_reference(shape, "drawn", "diou", 2.0, "align")
    assert max(ar.worst_ratios([ref["cls"], ref["reg"], ref["qsum"]], ref["grad"], ref)) == 0
    bad = ar.aligned_loss(out, cm, rm, al, 25, "diou", twh, 2.0, "align", mutant=mutant)
    assert max(ar.worst_ratios([bad["cls"], bad["reg"], ref["qsum"]], bad["grad"], ref)) > 1


@pytest.mark.parametrize("shape", ar.LOSS_SHAPES)
def test_loss_inputs_exclude_at_most_a_thousandth_of_the_positives(shape):
    """The regression gradient is checked outside box_loss_ref.kink_mask: on these inputs the restatement alone excludes at most 0.1 % of the
    positives (profiles/box_loss_parity.txt reports 0.09 % for such shapes)."""
    out, cm, rm, _ = ar.loss_case(shape, "drawn")
    kink = br.kink_mask(out, cm, rm, shape[1])
    assert int(kink.sum()) <= 0.001 * int((cm == 1).sum()), (int(kink.sum()), int((cm == 1).sum()))


# ------------------------------------------------------------------------------------------------------------------ the C entry points
def test_assigner_entry_point_refuses_before_it_enqueues(hip):
    """tf_targets_tal_aligned makes the refusals of tf_targets_tal, plus TF_ERR_ARG for a NULL align_map; its workspace is 8 bytes per winner
    slot larger and tf_targets_tal's query returns what it returned.  Runs without a GPU: the operands are host memory nobody dereferences."""
    l = hip.lib()
    ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -3, -4
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    for n in (0, 1, 10, 11):
        plain = l.tf_targets_tal_workspace_bytes(n, 2, 3, 5, 7)
        assert plain == max(n, 1) * (32 * 12 + 4) + 2 * 3 * 5 * 7 * 12 + 64
        assert l.tf_targets_tal_aligned_workspace_bytes(n, 2, 3, 5, 7) == plain + max(n, 1) * 32 * 8
    wsb = l.tf_targets_tal_aligned_workspace_bytes(10, 2, 3, 5, 7)

    def call(k=13, alpha=1.0, beta=6.0, out=p, ws=p, ws_bytes=wsb, cls=p, reg=p, al=p, tpl=p, offs=p, tstride=5, sty=8, stx=8, nt=3, vsy=5, vsx=7):
        return l.tf_targets_tal_aligned(out, p, offs, 2, tpl, nt, tstride, vsy, vsx, -1, -1, sty, stx, None, None, k, alpha, beta, None, cls, reg, al, ws,
                                        ws_bytes, None)

    assert call(al=None) == ERR_ARG
    for k in (0, -1, 33, 1 << 20):
        assert call(k=k) == ERR_ARG
    for a in (-1.0, float("nan"), float("inf")):
        assert call(alpha=a) == ERR_ARG
    for b in (0.0, -6.0, float("nan"), float("inf")):
        assert call(beta=b) == ERR_ARG
    assert call(out=None) == ERR_ARG and call(cls=None) == ERR_ARG and call(reg=None) == ERR_ARG and call(tpl=None) == ERR_ARG and call(offs=None) == ERR_ARG
    assert call(tstride=3) == ERR_ARG and call(sty=0) == ERR_ARG and call(stx=-8) == ERR_ARG
    small = l.tf_targets_tal_aligned_workspace_bytes(1, 2, 3, 5, 7)
    assert call(ws_bytes=small - 1) == ERR_WORKSPACE and call(ws_bytes=0) == ERR_WORKSPACE and call(ws=None) == ERR_WORKSPACE
    assert call(ws_bytes=l.tf_targets_tal_workspace_bytes(1, 2, 3, 5, 7)) == ERR_WORKSPACE          # the plain entry's size does not do
    assert call(k=0, ws=None, ws_bytes=0) == ERR_ARG and call(al=None, ws=None, ws_bytes=0) == ERR_ARG          # the arguments are judged first
    assert call(nt=1 << 12, vsy=1 << 10, vsx=1 << 10) == ERR_UNSUPPORTED
    assert call(vsx=1 << 20, stx=1 << 12) == ERR_UNSUPPORTED


def test_criterion_entry_point_refuses_before_it_enqueues(hip):
    """tf_criterion_aligned_fwd_bwd makes the refusals of the quality entry, plus a NULL align_map; TF_FOCAL_NORM_ALIGN (2) passed to any other
    entry stays TF_ERR_ARG.  Runs without a GPU."""
    l = hip.lib()
    ERR_ARG, ERR_WORKSPACE = -1, -4
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    wsb = l.tf_criterion_aligned_workspace_bytes(2, 3, 5, 7)
    assert wsb > l.tf_criterion_quality_workspace_bytes(2, 3, 5, 7) > 0 and l.tf_criterion_aligned_workspace_bytes(0, 3, 5, 7) == 0

    def call(out=p, cls=p, reg=p, al=p, B=2, nt=3, H=5, W=7, beta=2.0, norm=2, rw=1.0, form=0, twh=None, grad=p, loss=p, ws=p, ws_bytes=wsb):
        return l.tf_criterion_aligned_fwd_bwd(out, cls, reg, al, B, nt, H, W, beta, norm, rw, form, twh, grad, loss, None, ws, ws_bytes, None)

    assert call(al=None) == ERR_ARG
    assert call(out=None) == ERR_ARG and call(cls=None) == ERR_ARG and call(reg=None) == ERR_ARG and call(grad=None) == ERR_ARG and call(loss=None) == ERR_ARG
    assert call(B=0) == ERR_ARG and call(nt=0) == ERR_ARG and call(H=-1) == ERR_ARG and call(W=0) == ERR_ARG and call(B=65536) == ERR_ARG
    for beta in (0.99, 0.0, -2.0, float("nan"), float("inf")):
        assert call(beta=beta) == ERR_ARG
    assert call(rw=float("nan")) == ERR_ARG and call(rw=float("inf")) == ERR_ARG
    assert call(norm=3) == ERR_ARG and call(norm=-1) == ERR_ARG
    assert call(form=4) == ERR_ARG and call(form=-1) == ERR_ARG and call(form=3) == ERR_ARG          # TF_REG_DIOU without template_wh
    assert call(ws=None) == ERR_WORKSPACE and call(ws_bytes=wsb - 1) == ERR_WORKSPACE
    assert call(ws_bytes=l.tf_criterion_quality_workspace_bytes(2, 3, 5, 7)) == ERR_WORKSPACE
    assert call(norm=3, ws=None) == ERR_ARG                              # the arguments are judged first
    # TF_FOCAL_NORM_ALIGN belongs to this entry alone
    qws = l.tf_criterion_quality_workspace_bytes(2, 3, 5, 7)
    assert l.tf_criterion_quality_fwd_bwd(p, p, p, 2, 3, 5, 7, 2.0, 2, 1.0, 0, None, p, p, None, p, qws, None) == ERR_ARG
    fws = l.tf_criterion_focal_workspace_bytes(2, 3, 5, 7)
    assert l.tf_criterion_focal_fwd_bwd(p, p, p, 2, 3, 5, 7, 2.0, 0.25, 2, 1.0, p, p, None, p, fws, None) == ERR_ARG
    assert l.tf_criterion_focal_box_fwd_bwd(p, p, p, 2, 3, 5, 7, 2.0, 0.25, 2, 1.0, 1, None, p, p, None, p, fws, None) == ERR_ARG


# ------------------------------------------------------------------------------------------------------------------ the Python surface
def test_wrapper_signatures_and_value_errors(templates):
    from tinyfaces import ops
    from tinyfaces.models.loss import DetectionCriterion, TaskAligned
    for fn in (ops.tal_assign_device, ops.tal_assign):
        prm = list(inspect.signature(fn).parameters.values())
        assert prm[-1].name == "align_out" and prm[-1].default is None and prm[-2].name == "return_match_count"
    prm = inspect.signature(ops.criterion_aligned_fwd_bwd).parameters
    assert list(prm) == ["output", "class_map", "regression_map", "align_map", "n_templates", "reg_weight", "beta", "normalize", "reg_loss", "template_wh", "grad"]
    assert (prm["n_templates"].default, prm["reg_weight"].default, prm["beta"].default, prm["normalize"].default, prm["reg_loss"].default) == \
        (25, 1.0, 2.0, "align", "smooth_l1")
    # check_qfl and check_focal keep refusing what they refused; "align" is the new wrapper's own
    assert ops.FOCAL_NORMALIZE == {"none": 0, "pos": 1} and ops.ALIGNED_NORMALIZE == {"none": 0, "pos": 1, "align": 2}
    for bad in ("align", "batch"):
        with pytest.raises(ValueError):
            ops.check_qfl(2.0, bad)
        with pytest.raises(ValueError):
            ops.check_focal(2.0, 0.25, bad)
    ops.check_aligned(2.0, "align")
    ops.check_aligned(2.5, "pos")
    for beta, norm in ((0.5, "align"), (float("nan"), "align"), (2.0, "batch"), (2.0, None)):
        with pytest.raises(ValueError):
            ops.check_aligned(beta, norm)
    # TaskAligned
    prm = list(inspect.signature(TaskAligned.__init__).parameters.values())
    assert [p.name for p in prm] == ["self", "topk", "alpha", "beta", "aligned_targets"] and prm[-1].default is False
    assert TaskAligned().aligned_targets is False and repr(TaskAligned()) == "TaskAligned(topk=13, alpha=1.0, beta=6.0)"
    ta = TaskAligned(9, 0.5, 4.0, aligned_targets=True)
    assert ta.aligned_targets is True and "aligned_targets=True" in repr(ta)
    with pytest.raises(ValueError):
        TaskAligned(aligned_targets=1)
    # the criterion
    assert DetectionCriterion.CLS_LOSSES == ("soft_margin", "focal", "qfl")
    c = DetectionCriterion(25, cls_loss="qfl", reg_loss="diou", templates=templates, assigner=ta, focal_normalize="align")
    assert c.aligned_targets and c.focal_normalize == "align"
    assert DetectionCriterion(25, cls_loss="qfl", templates=templates, assigner=ta).focal_normalize == "pos"
    assert not DetectionCriterion(25, cls_loss="qfl", templates=templates, assigner=TaskAligned()).aligned_targets and not DetectionCriterion(25).aligned_targets
    for cls_loss in ("soft_margin", "focal"):
        with pytest.raises(ValueError, match="qfl"):
            DetectionCriterion(25, cls_loss=cls_loss, templates=templates, assigner=ta)
    with pytest.raises(ValueError, match="aligned_targets"):
        DetectionCriterion(25, cls_loss="qfl", focal_normalize="align")
    with pytest.raises(ValueError, match="aligned_targets"):
        DetectionCriterion(25, cls_loss="qfl", templates=templates, assigner=TaskAligned(), focal_normalize="align")
    with pytest.raises(ValueError):
        DetectionCriterion(25, cls_loss="qfl", templates=templates, assigner=ta, focal_normalize="batch")
    with pytest.raises(ValueError):
        DetectionCriterion(25, cls_loss="qfl", focal_normalize="batch")
    assert "mean TARGET" in DetectionCriterion.__doc__ and "varifocal" in DetectionCriterion.__doc__
    assert "score-weighted regression" not in DetectionCriterion.__doc__


def test_print_quality_names_the_target(capsys):
    from types import SimpleNamespace
    from tinyfaces import trainer
    from tinyfaces.models.loss import AvgMeter
    m = AvgMeter()
    m.update(3.0, 6)
    trainer.print_quality(1, 0, 2, SimpleNamespace(cls_loss="qfl", quality_average=m))
    assert "mean IoU of positives 0.5000 (6 positives)" in capsys.readouterr().out
    trainer.print_quality(1, 0, 2, SimpleNamespace(cls_loss="qfl", quality_average=m, aligned_targets=True))
    out = capsys.readouterr().out
    assert "mean aligned target of positives 0.5000 (6 positives)" in out and "IoU" not in out


# ------------------------------------------------------------------------------------------------------------------ main.py
def test_main_flags(capsys):
    import main
    base = ["synthetic-faces", "synthetic-faces"]
    on = base + ["--assigner", "tal", "--cls-loss", "qfl", "--tal-aligned-targets"]
    a = main.trunk_arguments(on)
    assert a.tal_aligned_targets is True and a.focal_normalize == "pos"
    d, ls = main.assigner_description(a), main.loss_description(a)
    assert "assigner TAL" in d and "aligned target m / max m * max IoU" in d and "the best 13 become" in d
    assert "task-aligned quality focal" in ls and "per image by its positives" in ls and "weighted by its aligned target" in ls
    a = main.trunk_arguments(on + ["--focal-normalize", "align", "--reg-loss", "diou", "--qfl-beta", "2.5"])
    assert a.focal_normalize == "align" and "per image by the sum of its aligned targets" in main.loss_description(a) and "beta 2.5" in main.loss_description(a)
    for bad, word in ((base + ["--tal-aligned-targets"], "--assigner tal --cls-loss qfl"),
                      (base + ["--assigner", "tal", "--tal-aligned-targets"], "--assigner tal --cls-loss qfl"),
                      (base + ["--assigner", "tal", "--cls-loss", "focal", "--tal-aligned-targets"], "--assigner tal --cls-loss qfl"),
                      (base + ["--assigner", "atss", "--cls-loss", "qfl", "--tal-aligned-targets"], "--assigner tal --cls-loss qfl"),
                      (base + ["--cls-loss", "qfl", "--focal-normalize", "align"], "needs --tal-aligned-targets"),
                      (base + ["--assigner", "tal", "--cls-loss", "qfl", "--focal-normalize", "align"], "needs --tal-aligned-targets"),
                      (base + ["--cls-loss", "focal", "--focal-normalize", "align"], "needs --tal-aligned-targets")):
        with pytest.raises(SystemExit):
            main.trunk_arguments(bad)
        assert word in capsys.readouterr().err


def test_every_earlier_flag_combination_parses_to_what_it_parsed():
    """tests/golden/main_flags.json: flag combinations from before --tal-aligned-targets with what main.trunk_arguments made of them then (every
    attribute) and the two start-up lines.  They parse to the same, plus tal_aligned_targets = False, and print the same lines."""
    import main
    with open(os.path.join(GOLDEN, "main_flags.json")) as fh:
        recorded = json.load(fh)
    assert len(recorded) >= 12
    for rec in recorded:
        a = main.trunk_arguments(list(rec["argv"]))
        got = json.loads(json.dumps(vars(a), default=str, sort_keys=True))
        assert got.pop("tal_aligned_targets") is False
        assert got == rec["args"], (rec["argv"], {k: (got.get(k), rec["args"].get(k)) for k in set(got) | set(rec["args"]) if got.get(k) != rec["args"].get(k)})
        assert main.assigner_description(a) == rec["assigner_description"] and main.loss_description(a) == rec["loss_description"]
