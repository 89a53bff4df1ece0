"""CPU: the rule of the task-aligned target assignment (include/tinyfaces_hip.h, "TAL") as tests/tal_ref.py restates it -- by hand and by
property --, the argument validation of its Python surface, of the C entry point and of main.py's flags, the ambiguity counts of the seeded
cases tests/test_gpu_tal.py holds the kernel to (profiles/tal_parity.txt) and the positives per face size at zero output
(profiles/tal_stats.txt).  Restatement only: nothing here runs the kernel."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

import atss_ref
import tal_cases as tc
import tal_ref
from oracle import targets as otgt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _anchor_iou(box, t, y, x):
    """dense_overlap's IoU of anchor (t, y, x) with the face (+1 pixel convention)."""
    cx, cy = -1.0 + 8 * x, -1.0 + 8 * y
    ax1, ay1, ax2, ay2 = t[0] + cx, t[1] + cy, t[2] + cx, t[3] + cy
    iw, ih = min(ax2, box[2]) - max(ax1, box[0]) + 1, min(ay2, box[3]) - max(ay1, box[1]) + 1
    if iw <= 0 or ih <= 0:
        return 0.0
    ia = iw * ih
    return ia / ((ax2 - ax1 + 1) * (ay2 - ay1 + 1) + (box[2] - box[0] + 1) * (box[3] - box[1] + 1) - ia)


def test_refusals():
    from tinyfaces import ops
    assert ops.check_tal() == (13, 1.0, 6.0) and ops.check_tal(np.int64(32), 0, 0.5) == (32, 0.0, 0.5) and ops.check_tal(1, 2.5, 1) == (1, 2.5, 1.0)
    for k in (0, 33, -1, 13.0, True, "13", None):
        with pytest.raises(ValueError, match="topk"):
            ops.check_tal(k)
    for a in (-0.1, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="alpha"):
            ops.check_tal(13, a)
    for b in (0, 0.0, -6, float("nan"), float("inf"), "6", None, False):
        with pytest.raises(ValueError, match="beta"):
            ops.check_tal(13, 1.0, b)
    assert "tal" in ops.ASSIGNERS and ops.check_assigner("tal") == ("tal", 9)
    with pytest.raises(ValueError, match="compensat"):
        ops.check_assigner("tal", compensate=(3, 0.1))
    assert ops.check_assigner("dense_overlap", 9, (3, 0.1)) == ("dense_overlap", 9)
    import torch
    z = torch.zeros(1, 5, 5, 7)
    with pytest.raises(ValueError, match="topk"):                     # refused before the device is looked at
        ops.tal_assign(z, z[:, :1], z[:, :4], [np.zeros((1, 4))], tc.T3[:1], topk=0)
    with pytest.raises(ValueError, match="beta"):
        ops.tal_assign_device(z, z[:, :1], z[:, :4], None, None, 0, None, beta=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.tal_assign(z, z[:, :1].clone(), z[:, :4].clone(), [np.zeros((1, 4))], tc.T3[:1])
    sig = inspect.signature(ops.tal_assign).parameters
    assert (sig["topk"].default, sig["alpha"].default, sig["beta"].default, sig["return_match_count"].default) == (13, 1.0, 6.0, False)


def test_entry_point_refuses_before_it_enqueues(hip):
    """tf_targets_tal: topk outside 1..32, alpha / beta out of range, NULL operands, tstride < 4, strides <= 0, a workspace that is too small
    and sizes beyond int32 come back as error codes.  Runs without a GPU: the operands are host memory nobody dereferences."""
    l = hip.lib()
    ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -3, -4
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    wsb = l.tf_targets_tal_workspace_bytes(10, 2, 3, 5, 7)
    assert wsb >= 10 * 32 * 12 + 2 * 3 * 5 * 7 * 12 and l.tf_targets_tal_workspace_bytes(11, 2, 3, 5, 7) > wsb
    assert l.tf_targets_tal_workspace_bytes(0, 2, 3, 5, 7) == l.tf_targets_tal_workspace_bytes(1, 2, 3, 5, 7)

    def call(k=13, alpha=1.0, beta=6.0, out=p, ws=p, ws_bytes=wsb, cls=p, reg=p, tpl=p, offs=p, tstride=5, sty=8, stx=8, nt=3, vsy=5, vsx=7):
        return l.tf_targets_tal(out, p, offs, 2, tpl, nt, tstride, vsy, vsx, -1, -1, sty, stx, None, None, k, alpha, beta, None, cls, reg, ws, ws_bytes, None)

    for k in (0, -1, 33, 1 << 20):
        assert call(k=k) == ERR_ARG
    for a in (-1.0, float("nan"), float("inf")):
        assert call(alpha=a) == ERR_ARG
    for b in (0.0, -6.0, float("nan"), float("inf")):
        assert call(beta=b) == ERR_ARG
    assert call(out=None) == ERR_ARG and call(cls=None) == ERR_ARG and call(reg=None) == ERR_ARG and call(tpl=None) == ERR_ARG and call(offs=None) == ERR_ARG
    assert call(tstride=3) == ERR_ARG and call(sty=0) == ERR_ARG and call(stx=-8) == ERR_ARG
    small = l.tf_targets_tal_workspace_bytes(1, 2, 3, 5, 7)
    assert call(ws_bytes=small - 1) == ERR_WORKSPACE and call(ws_bytes=0) == ERR_WORKSPACE and call(ws=None) == ERR_WORKSPACE
    assert call(k=0, ws=None, ws_bytes=0) == ERR_ARG                   # the arguments are judged first
    assert call(nt=1 << 12, vsy=1 << 10, vsx=1 << 10) == ERR_UNSUPPORTED
    assert call(vsx=1 << 20, stx=1 << 12) == ERR_UNSUPPORTED


def test_zero_output_and_alpha_zero_take_the_largest_anchor_ious():
    """output = 0: the predicted box is the anchor (in the continuous convention its IoU equals dense_overlap's up to rounding); alpha = 0
    removes the score.  Every face then wins its topk candidates of largest anchor IoU (one face per image: no conflicts)."""
    hm, t = (13, 11), tc.T3
    for box in tc.planted()["output 0, topk 13"]["boxes"][0]:
        for topk in (1, 5, 13):
            cm0, rm0 = tal_ref.base_maps(t, hm=hm)
            cm, rm, mc, faces = tal_ref.tal_maps(np.zeros((15,) + hm, np.float32), cm0, rm0, box[None], t, topk=topk, alpha=0.0, hm=hm, details=True)
            cand = [(_anchor_iou(box, t[k], y, x), k, y, x) for k in range(3) for y in range(hm[0]) for x in range(hm[1])
                    if box[0] < -1 + 8 * x < box[2] and box[1] < -1 + 8 * y < box[3]]
            ious = np.sort([c[0] for c in cand if c[0] > 0])[::-1]
            assert mc.tolist() == [min(topk, ious.size)]
            won = [_anchor_iou(box, t[k], y, x) for k, y, x in zip(*np.nonzero(cm == 1))]
            assert len(won) == mc[0] and min(won) >= ious[mc[0] - 1] * (1 - 1e-12)
            assert np.allclose(np.sort(faces[0]["u"])[::-1], ious[:mc[0]], rtol=1e-12, atol=0)


def test_planted_regression_target_has_u_one_and_is_won():
    """A prediction and the face it describes: from the float32 prediction (px, py, pw, ph) of anchor (t, y, x) the face with exactly that
    centre and size is built; its regression target at that anchor is the prediction, u is 1 to 1e-12, and with topk = 1 the anchor is won
    although its logit is the lowest of the window."""
    hm, t = (9, 11), tc.T3
    rng = np.random.RandomState(3)
    for k, y, x in ((0, 4, 5), (1, 3, 6), (2, 5, 4)):
        p = rng.uniform(-0.3, 0.3, 4).astype(np.float32)
        dw, dh = t[k, 2] - t[k, 0] + 1, t[k, 3] - t[k, 1] + 1
        bcx, bcy = (-1.0 + 8 * x) + float(p[0]) * dw, (-1.0 + 8 * y) + float(p[1]) * dh
        w, h = dw * np.exp(float(p[2])), dh * np.exp(float(p[3]))
        box = np.array([bcx - (w - 1) / 2, bcy - (h - 1) / 2, bcx + (w - 1) / 2, bcy + (h - 1) / 2])
        assert np.allclose(tal_ref.regression_target(box, t[k], y, x), p.astype(np.float64), rtol=0, atol=1e-12)
        case = tc.make(hm, t, [box[None]], rng.standard_normal((1, 15) + hm) * 0.05, topk=1)
        tc.plant(case, 0, k, y, x, (-2.0,) + tuple(p))
        cm, rm, mc, faces = tc.restate(case)[0]
        assert mc.tolist() == [1] and cm[k, y, x] == 1 and int((cm == 1).sum()) == 1
        assert abs(faces[0]["u"][0] - 1.0) <= 1e-12
        assert np.array_equal(rm[[k, 3 + k, 6 + k, 9 + k], y, x], tal_ref.regression_target(box, t[k], y, x).astype(np.float32))


def test_conflicts_resolve_the_same_way_in_both_orders():
    P = tc.planted()
    for suffix in ("", ", m = 0"):
        a, b = tc.planted_reference("conflict by u" + suffix)[0], tc.planted_reference("conflict by u, other order" + suffix)[0]
        assert a[2].tolist() == [0, 9] and b[2].tolist() == [9, 0]      # the face that overlaps the predicted box more takes the shared anchor
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0][0, 2, 3] == 1
        assert a[3][0]["conflict_gap"] > 0.05 and not a[3][0]["ambiguous"]
    r = tc.planted_reference("conflict by face index")[0]
    assert r[2].tolist()[2:] == [0, 0, 0] and r[2][0] == 13 and r[3][2]["conflict_gap"] == 0.0 and not r[3][2]["ambiguous"]
    assert P["conflict by face index"]["boxes"][0].shape == (5, 4)


def test_tiny_face_takes_the_nearest_cell_of_every_template():
    """[25, 17, 30, 22]: no anchor centre (x 23 / 31, y 15 / 23) is strictly inside.  Its centre (27.5, 19.5) is 4.5 and 3.5 from the columns
    23 and 31, 4.5 and 3.5 from the rows 15 and 23: the nearest cell of every template is (3, 4)."""
    case = tc.planted()["tiny face"]
    cm, rm, mc, faces = tc.planted_reference("tiny face")[0]
    cells = sorted((int(a) % 35) for a in faces[0]["winners"])
    assert set(cells) == {3 * 7 + 4} and mc[0] == len(faces[0]["winners"]) <= 3
    assert all(cm[k, 3, 4] == 1 for k in (int(a) // 35 for a in faces[0]["winners"]))
    # with the cell (3, 4) padded away the next nearest unpadded cell is taken; with every cell padded, nothing
    paste = [0, 0, 30, 22]                                            # the 9 x 11 template fits at (1, 1) .. (2, 3) only
    pad = atss_ref.padding(case["t"], paste, 0, otgt.RF, case["hm"])
    assert not pad[2, 3, 1] and pad[3, 4, 1] and pad[:, :, 0].all() and pad[:, :, 2].all()
    c2 = tc.make(case["hm"], case["t"], case["boxes"], case["out"], pastes=[paste], flips=[0])
    cm2, _, mc2, f2 = tc.restate(c2)[0]
    assert [int(a) for a in f2[0]["winners"]] == [(1 * 5 + 2) * 7 + 3] and mc2.tolist() == [1] and cm2[1, 2, 3] == 1
    # a face whose edges lie ON two anchor centres has no window either (strictly inside) and falls under the same rule
    e = tc.planted_reference("edges on the centres")[0]
    assert e[2].tolist() == [2] and sorted(int(a) % 35 for a in e[3][0]["winners"]) == [2 * 7 + 3] * 2


def test_fully_padded_and_empty_images():
    r = tc.planted_reference("padded, mirrored, fully padded")
    case = tc.planted()["padded, mirrored, fully padded"]
    assert r[0][2].tolist() == [0, 0, 0] and np.array_equal(r[0][0], case["cm"][0]) and (r[0][0] == -1).all() and not r[0][1].any()
    assert r[1][2].sum() > 0 and r[2][2].sum() > 0 and not np.array_equal(r[1][0], r[2][0])
    for b in (1, 2):                                                  # no positive on a padded anchor
        pad = atss_ref.padding(case["t"], case["pastes"][b], case["flips"][b], otgt.RF, case["hm"]).transpose(2, 0, 1)
        assert pad.any() and not ((r[b][0] == 1) & pad).any()
    ci = 6
    case, ref = tc.random_case(ci), tc.random_reference(ci)
    assert case["boxes"][1].shape[0] == 0 and ref[1][2].size == 0 and np.array_equal(ref[1][0], case["cm"][1]) and np.array_equal(ref[1][1], case["rm"][1])


def test_an_image_does_not_depend_on_its_batch():
    case, ref = tc.random_case(3), tc.random_reference(3)
    for b in (0, 2):
        alone = tal_ref.tal_maps(case["out"][b], case["cm"][b], case["rm"][b], case["boxes"][b], case["t"], case["pastes"][b], case["flips"][b],
                                 case["topk"], hm=case["hm"])
        assert all(np.array_equal(x, y) for x, y in zip(alone, ref[b][:3]))


def test_untouched_elements_and_ignored_anchors():
    case, (cm, rm, mc, faces) = tc.planted()["base maps with 0 and +1"], tc.planted_reference("base maps with 0 and +1")[0]
    won = np.zeros(cm.size, bool)
    for f in faces:
        won[f["winners"]] = True
    won = won.reshape(cm.shape)
    assert np.array_equal(cm[~won], case["cm"][0][~won]) and (cm[won] == 1).all() and (case["cm"][0][won] == 0).any()
    assert np.array_equal(rm[~np.tile(won, (4, 1, 1))], case["rm"][0][~np.tile(won, (4, 1, 1))])
    assert cm[1, 8, 9] == 1 and rm[1, 8, 9] == 7.0 and rm[5, 0, 0] == -2.5


def test_every_mutant_differs_from_the_rule():
    assert set(tc.MUTANT_CASES) == set(tal_ref.MUTANTS)
    for mutant, name in tc.MUTANT_CASES.items():
        want, got = tc.planted_reference(name), tc.restate(tc.planted()[name], mutant=mutant)
        with pytest.raises(AssertionError):
            for w, g in zip(want, got):
                tal_ref.compare(g[:3], w, tc.planted()[name]["hm"])


def test_ambiguity_caps_of_the_seeded_cases():
    """No planted face is ambiguous; of the random faces at most 1 % are, and the restatement perturbed by one ulp in exp stays equal to
    itself outside them (tal_ref.compare): the seeds the GPU test uses were chosen so.  Writes the counts to profiles/tal_parity.txt."""
    lines = ["# Ambiguous faces of the seeded cases of tests/test_gpu_tal.py (tests/tal_cases.py), by the restatement alone: a face is ambiguous where the",
             "# relative gap between its last winner and first loser, or at a conflict, is below 1e-9 without bit-identical operands.",
             "# Written by tests/test_tal.py::test_ambiguity_caps_of_the_seeded_cases (numpy, no GPU).  'perturbed': the same count with exp moved by one ulp.",
             "# case | faces | ambiguous | ambiguous (perturbed) | smallest cut gap | smallest conflict gap"]
    for name in tc.planted():
        faces = [f for im in tc.planted_reference(name) for f in im[3]]
        assert not any(f["ambiguous"] for f in faces), name
        lines.append(f"{name} | {len(faces)} | 0 | - | {min([f['cut_gap'] for f in faces] + [np.inf]):.3g} | {min([f['conflict_gap'] for f in faces] + [np.inf]):.3g}")
    total = amb = amb_p = 0
    for ci in range(len(tc.RANDOM)):
        case, ref = tc.random_case(ci), tc.random_reference(ci)
        pert = tc.restate(case, exp=tal_ref.ulp_exp(ci))
        faces, pfaces = [f for im in ref for f in im[3]], [f for im in pert for f in im[3]]
        for w, g in zip(ref, pert):
            tal_ref.compare(g[:3], w, case["hm"])
        n, a, ap = len(faces), sum(f["ambiguous"] for f in faces), sum(f["ambiguous"] for f in pfaces)
        total, amb, amb_p = total + n, amb + a, amb_p + ap
        lines.append(f"{case['name']} | {n} | {a} | {ap} | {min([f['cut_gap'] for f in faces] + [np.inf]):.3g} | {min([f['conflict_gap'] for f in faces] + [np.inf]):.3g}")
    lines.append(f"random cases together | {total} | {amb} | {amb_p} | |")
    try:
        with open(os.path.join(ROOT, "profiles", "tal_parity.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass
    assert total >= 150 and amb <= 0.01 * total and amb_p <= 0.01 * total


SIZES = (6, 8, 12, 16, 24, 40, 80, 160, 300)


def test_positives_per_face_size_at_zero_output(templates):
    """profiles/tal_stats.txt: what TAL gives at initialisation (output = 0: the metric is the anchor's IoU to the 6th) next to ATSS's
    positives, on the faces of profiles/atss_stats.txt (tests/test_atss.py::band_statistics: the same generator, the same seed)."""
    rng = np.random.RandomState(0)
    pad = np.zeros((63, 63, templates.shape[0]), bool)
    cm0, rm0 = tal_ref.base_maps(templates)
    out = np.zeros((125, 63, 63), np.float32)
    lines = ["# Positives per face at ZERO output (the head at initialisation: the predicted box is the anchor): TAL topk = 13, alpha = 1, beta = 6 next to",
             "# ATSS k = 9 (profiles/atss_stats.txt; the same 30 seeded faces per size, golden templates, 63 x 63 stride-8 grid, no padding, every face on",
             "# its own).  Written by tests/test_tal.py::test_positives_per_face_size_at_zero_output (numpy restatement, no GPU).  No accuracy claim.",
             "# face size (px) | TAL mean positives | min | faces with none | mean IoU of TAL's positives | ATSS mean positives (before its fallback)"]
    for size in SIZES:
        w = size * rng.uniform(0.9, 1.1, 30)
        h = w * rng.uniform(1.1, 1.4, 30)
        x, y = rng.uniform(0, 500 - w), rng.uniform(0, 500 - h)
        boxes = np.stack([x, y, x + w, y + h], 1)
        n, u = [], []
        for b in boxes:
            _, _, mc, faces = tal_ref.tal_maps(out, cm0, rm0, b[None], templates, details=True)
            n.append(int(mc[0]))
            u.extend(faces[0]["u"].tolist())
        atss = [len(atss_ref.face_claims(b, templates, pad, 9, otgt.RF, otgt.HEATMAP_SIZE)["positive"]) for b in boxes]
        n = np.array(n)
        lines.append(f"{size} | {n.mean():.1f} | {int(n.min())} | {int((n == 0).sum())} | {np.mean(u):.2f} | {np.mean(atss):.1f}")
        assert int((n == 0).sum()) == 0 and int(n.max()) <= 13, size       # every face overlaps its nearest anchor: none is left without a positive
        if size >= 40:
            assert int(n.min()) == 13, size                            # a window of more than 13 overlapping anchors: the face takes its full topk
    try:
        with open(os.path.join(ROOT, "profiles", "tal_stats.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass                                                         # a read-only checkout still checks the facts above


def test_python_surface(templates):
    """The loaders, the criterion, the engine and the trainer take the assigner; the defaults are what they were."""
    import torch
    from tinyfaces import ops, trainer
    from tinyfaces.datasets import ResidentFaces, SyntheticFaces, TargetAssigner, get_dataloader
    from tinyfaces.datasets.augment import collate_device
    from tinyfaces.datasets.wider_face import WIDERFace
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.loss import DetectionCriterion, TaskAligned
    for fn in (SyntheticFaces.__init__, TargetAssigner.__init__, WIDERFace.__init__, get_dataloader):
        sig = inspect.signature(fn).parameters
        assert (sig["assigner"].default, sig["tal_topk"].default, sig["tal_alpha"].default, sig["tal_beta"].default) == ("dense_overlap", 13, 1.0, 6.0)
    assert inspect.signature(collate_device).parameters["assigner"].default == "dense_overlap"
    for fn in (DetectionCriterion.forward, DetectionCriterion._fwd_bwd):
        assert inspect.signature(fn).parameters["faces"].default is None
    assert list(inspect.signature(TrainEngine.step).parameters) == ["self", "x", "class_map", "regression_map", "apply"]      # as it was
    assert list(inspect.signature(TrainEngine.step_with_faces).parameters) == ["self", "x", "class_map", "regression_map", "faces", "apply"]
    with pytest.raises(ValueError, match="compensat"):
        TargetAssigner(templates, assigner="tal", compensate=(3, 0.1))
    with pytest.raises(ValueError, match="compensat"):
        SyntheticFaces(templates, length=1, assigner="tal", anchor_compensation=(3, 0.1))
    with pytest.raises(ValueError, match="compensat"):
        collate_device([], None, assigner="tal", compensate=(3, 0.1))
    for bad in (dict(tal_topk=0), dict(tal_topk=33), dict(tal_alpha=-1.0), dict(tal_beta=0.0), dict(tal_beta=float("nan"))):
        with pytest.raises(ValueError, match="tal"):
            SyntheticFaces(templates, length=1, assigner="tal", **bad)
    ds = SyntheticFaces(templates, length=1, assigner="tal", tal_topk=7, tal_alpha=0.5, tal_beta=4.0)
    a = ds.assigner
    assert (a.assigner, a.tal_topk, a.tal_alpha, a.tal_beta) == ("tal", 7, 0.5, 4.0) and ds.compensation_stats.atss and ds.compensation_stats.label == "TAL"
    plain = SyntheticFaces(templates, length=1)
    assert plain.compensation_stats is None and SyntheticFaces(templates, length=1, assigner="atss").compensation_stats.label == "ATSS"
    with pytest.raises(ValueError, match="synthetic crops"):
        get_dataloader("synthetic", None, assigner="tal")
    t = TaskAligned()
    assert (t.topk, t.alpha, t.beta) == (13, 1.0, 6.0) and "topk=13" in repr(t)
    for bad in (dict(topk=0), dict(topk=2.0), dict(alpha=-1), dict(beta=0), dict(beta=float("inf"))):
        with pytest.raises(ValueError):
            TaskAligned(**bad)
    with pytest.raises(ValueError, match="templates"):
        DetectionCriterion(25, assigner=TaskAligned())
    with pytest.raises(ValueError, match="TaskAligned"):
        DetectionCriterion(25, templates=templates, assigner="tal")
    with pytest.raises(ValueError, match="n_templates"):
        DetectionCriterion(3, templates=templates, assigner=TaskAligned())
    crit = DetectionCriterion(25, cls_loss="qfl", reg_loss="giou", templates=templates, assigner=TaskAligned(5, 0.0, 2.0))
    assert crit.assigner.topk == 5 and DetectionCriterion(25).assigner is None
    z = torch.zeros(1, 125, 5, 7)
    rec = ResidentFaces(torch.zeros(1, 4, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), 0)
    assert len(rec) == 1 and rec.to("cpu") is rec and rec.stats is None
    with pytest.raises(ValueError, match="faces"):                    # refused before the device is looked at, both ways round
        crit(z, z[:, :25], z[:, :100])
    with pytest.raises(ValueError, match="assigner"):
        DetectionCriterion(25)(z, z[:, :25], z[:, :100], faces=rec)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(z, z[:, :25], z[:, :100], faces=rec)
    import contextlib
    import io
    from types import SimpleNamespace
    ds.compensation_stats._pending.append((torch.tensor([2, 1]), 5))    # what a push leaves: (at most 3, none) over 5 faces
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        trainer.print_compensation(3, 1, 9, SimpleNamespace(dataset=ds))
    assert buf.getvalue() == "Epoch: [1][3/9]\tTAL: 2 of 5 faces won at most 3 positives, 1 of them none\n"


def test_main_flags(capsys):
    import main
    base = ["synthetic-faces", "synthetic-faces"]
    a = main.trunk_arguments(base)
    assert a.assigner == "dense_overlap" and (a.tal_topk, a.tal_alpha, a.tal_beta) == (13, 1.0, 6.0) and "TAL" not in main.assigner_description(a)
    a = main.trunk_arguments(base + ["--assigner", "tal"])
    d = main.assigner_description(a)
    assert a.assigner == "tal" and "assigner TAL" in d and "the best 13 become" in d and "sigmoid(logit)^1 * IoU(predicted box, face)^6" in d
    a = main.trunk_arguments(base + ["--assigner", "tal", "--tal-topk", "32", "--tal-alpha", "0", "--tal-beta", "0.5"])
    assert (a.tal_topk, a.tal_alpha, a.tal_beta) == (32, 0.0, 0.5) and isinstance(a.tal_topk, int) and "the best 32 become" in main.assigner_description(a)
    for bad in (["--tal-topk", "0"], ["--tal-topk", "33"], ["--tal-topk", "2.5"], ["--tal-alpha", "-1"], ["--tal-alpha", "nan"], ["--tal-beta", "0"],
                ["--tal-beta", "inf"], ["--assigner", "TAL"], ["--assigner", "tal", "--anchor-compensation", "3", "0.1"]):
        with pytest.raises(SystemExit):
            main.trunk_arguments(base + bad)
    assert "--anchor-compensation" in capsys.readouterr().err
    with pytest.raises(SystemExit):                                  # a parser error, not a traceback from the loader
        main.trunk_arguments(["synthetic", "synthetic", "--assigner", "tal"])
    assert "synthetic crops" in capsys.readouterr().err
