"""CPU: the ignore regions -- the rule as tests/ignore_ref.py restates it, the argument validation of the Python surface, of the C entry
point and of main.py's flags, the augmentation bookkeeping of process_inputs(ignore_policy=) with a stand-in device image, and the
statistics that motivate the feature."""
import ctypes as C
import inspect
import os
from types import SimpleNamespace

import numpy as np
import pytest

import ignore_ref
from oracle import targets as otgt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T16 = np.array([[-7.5, -7.5, 7.5, 7.5, 1.0]])                       # one 16 x 16 template


# ------------------------------------------------------------------------------------------------ the rule
def test_hand_worked_rule():
    """5 x 7 cells, stride 8, offset -1, the 16 x 16 template: the anchor of cell (2, 3) is [15.5, 7.5, 30.5, 22.5]."""
    hm = (5, 7)
    F = -np.ones((5, 7, 1))
    F[2, 3, 0] = 1
    F[2, 4, 0] = 0
    box = np.array([[15.5, 7.5, 30.5, 22.5]])                        # the anchor of (2, 3) itself; its neighbours overlap it by half
    out, n = ignore_ref.apply_ignore(F, T16, box, "iof", 0.5, hm=hm)
    want = F.copy()
    want[1, 3, 0] = want[3, 3, 0] = want[2, 2, 0] = 0                # 8 of 16 rows / columns shared: ia / farea = 0.5 exactly
    assert np.array_equal(out, want) and n == 3 and F[1, 3, 0] == -1          # +1 and 0 survive, the input is not modified
    out, n = ignore_ref.apply_ignore(F, T16, box, "iou", 0.5, hm=hm)          # IoU of the half-overlapping neighbours is 1 / 3
    assert np.array_equal(out, F) and n == 0
    out, n = ignore_ref.apply_ignore(F, T16, box, "iof", float(np.nextafter(0.5, 1)), hm=hm)
    assert n == 0
    G = -np.ones((5, 7, 1))
    for measure in ("iof", "iou"):                                   # a box equal to an anchor at thresh 1.0
        out, n = ignore_ref.apply_ignore(G, T16, box, measure, 1.0, hm=hm)
        assert n == 1 and out[2, 3, 0] == 0
    # degenerate boxes are dropped, an empty list changes nothing
    assert ignore_ref.apply_ignore(G, T16, [[10, 10, 10, 90], [10, 10, 90, 5]], "iof", 0.01, hm=hm)[1] == 0
    assert ignore_ref.apply_ignore(G, T16, np.zeros((0, 4)), "iof", 0.5, hm=hm)[1] == 0
    # the rule is order-free in k
    rng = np.random.RandomState(0)
    boxes = rng.uniform(0, 40, (9, 2))
    boxes = np.concatenate([boxes, boxes + rng.uniform(3, 20, (9, 2))], 1)
    a, b = ignore_ref.apply_ignore(G, T16, boxes, "iou", 0.2, hm=hm), ignore_ref.apply_ignore(G, T16, boxes[::-1], "iou", 0.2, hm=hm)
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] > 0


def test_the_rule_does_not_know_the_regression_map():
    assert list(inspect.signature(ignore_ref.apply_ignore).parameters) == ["class_map_hwc", "templates", "ignore_boxes", "measure", "thresh", "rf", "hm"]


# ------------------------------------------------------------------------------------------------ validation
def test_check_ignore_refusals(templates):
    import torch
    from tinyfaces import ops
    assert ops.check_ignore(None) is None and ops.check_ignore(("iof", 0.5)) == ("iof", 0.5) and ops.check_ignore(["iou", 1]) == ("iou", 1.0)
    assert ops.check_ignore(("iof", np.float64(1e-9))) == ("iof", 1e-9) and ops.IGNORE_DEFAULT == ("iof", 0.5)
    bad = [("iof", 0.0), ("iof", 1.5), ("iof", -0.1), ("iof", float("nan")), ("iof", float("inf")), ("iof", "0.5"), ("iof", True), ("giou", 0.5),
           (0, 0.5), ("iof",), ("iof", 0.5, 1), 0.5, "iof"]
    for ig in bad:
        with pytest.raises(ValueError):
            ops.check_ignore(ig)
        with pytest.raises(ValueError):                               # refused before the device is looked at
            ops.dense_overlap_targets([np.zeros((1, 4))], templates, device="cpu", ignore_boxes=[np.zeros((0, 4))], ignore=ig)
        with pytest.raises(ValueError):
            ops.targets_apply_ignore(torch.zeros(1, 25, 63, 63), [np.zeros((0, 4))], templates, ignore=ig)
    with pytest.raises(ValueError):
        ops.dense_overlap_targets([np.zeros((1, 4))], templates, device="cpu", return_ignored_count=True)
    with pytest.raises(ValueError):
        ops.dense_overlap_targets([np.zeros((1, 4))], templates, device="cpu", ignore_boxes=[[], []])
    with pytest.raises(ValueError):
        ops.dense_overlap_targets_device(torch.zeros(1, 4, dtype=torch.float64), torch.zeros(2, dtype=torch.int32), 1, torch.zeros(25, 5, dtype=torch.float64),
                                         return_ignored_count=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):       # valid keywords go on to the usual refusal: there is no host path
        ops.dense_overlap_targets([np.zeros((1, 4))], templates, device="cpu", ignore_boxes=[np.zeros((0, 4))])
    for fn, names in ((ops.dense_overlap_targets, ("ignore_boxes", "ignore")), (ops.dense_overlap_targets_device, ("ignore_d", "ignore_offs_d", "ignore"))):
        for name in names:
            assert inspect.signature(fn).parameters[name].default is None
        assert inspect.signature(fn).parameters["return_ignored_count"].default is False


def test_check_ignore_policy_refusals():
    from tinyfaces.datasets import augment as da
    P = da.IgnorePolicy
    assert da.check_ignore_policy(None) is None
    assert da.check_ignore_policy(P(invalid=True)) == P(True, None, None, None, False)
    assert da.check_ignore_policy({"blur": 2, "min_size": 8}) == P(False, 2, None, 8.0, False)
    assert da.check_ignore_policy((False, None, np.int64(1), None, True)) == P(False, None, 1, None, True)
    bad = [P(), P(invalid=1), P(truncated="yes"), P(blur=0), P(blur=3), P(blur=1.0), P(blur=True), P(occlusion=0), P(occlusion=3),
           P(min_size=0), P(min_size=-4), P(min_size=float("nan")), P(min_size=float("inf")), P(min_size="8"), {"size": 8}, (True,) * 6, 3, "invalid"]
    for p in bad:
        with pytest.raises(ValueError):
            da.check_ignore_policy(p)
    with pytest.raises(ValueError, match="attributes"):              # a field that reads a column needs the column
        da.flagged_faces(P(invalid=True), np.zeros((2, 4)), None)
    with pytest.raises(ValueError, match="2 faces"):
        da.flagged_faces(P(blur=1), np.zeros((2, 4)), {"blur": np.zeros(3)})


def test_data_set_surface(templates):
    from tinyfaces.datasets import get_dataloader
    from tinyfaces.datasets.augment import IgnorePolicy, collate_device, crop_decisions, process_inputs
    from tinyfaces.datasets.synthetic import IgnoreStats, TargetAssigner
    from tinyfaces.datasets.wider_face import WIDERFace
    for fn, names in ((get_dataloader, ("ignore_policy", "ignore")), (WIDERFace.__init__, ("ignore_policy", "ignore")),
                      (collate_device, ("ignore_boxes", "ignore")), (TargetAssigner.__init__, ("ignore",)), (TargetAssigner.__call__, ("ignore_boxes",))):
        for name in names:
            assert inspect.signature(fn).parameters[name].default is None, (fn, name)
    for fn in (process_inputs, crop_decisions):                       # the existing part of the signatures is what it was; the additions are keyword-only
        ps = inspect.signature(fn).parameters
        assert ps["ignore_out"].kind is inspect.Parameter.KEYWORD_ONLY and ps["ignore_out"].default is None
    ps = inspect.signature(process_inputs).parameters
    assert list(ps)[:10] == ["image_u8", "bboxes", "input_size", "neg_thresh", "rng", "out", "mean", "std", "color_jitter", "chain_out"]
    assert ps["ignore_policy"].kind is inspect.Parameter.KEYWORD_ONLY and ps["attributes"].default is None
    assert TargetAssigner(templates).ignore_stats is None and TargetAssigner(templates, ignore=("iou", 0.4)).ignore == ("iou", 0.4)
    with pytest.raises(ValueError):
        TargetAssigner(templates, ignore=("iof", 0))
    with pytest.raises(ValueError):
        TargetAssigner(templates)([np.zeros((0, 4))], ignore_boxes=[np.zeros((0, 4))])
    with pytest.raises(ValueError, match="synthetic"):
        get_dataloader("synthetic-faces", SimpleNamespace(batch_size=1), ignore_policy=IgnorePolicy(invalid=True))
    import torch
    from tinyfaces import trainer
    st = IgnoreStats()
    assert st.pop() is None
    st.push(torch.tensor([0, 5, 3], dtype=torch.int32))
    st.push(torch.tensor([7], dtype=torch.int32))
    assert st.pop(lag=1) == (3, 8, 2) and st.pop(lag=1) is None and st.pop() == (1, 7, 1)


def test_print_ignore(capsys):
    import torch
    from tinyfaces import trainer
    from tinyfaces.datasets.synthetic import IgnoreStats
    trainer.print_ignore(0, 0, 1, SimpleNamespace(dataset=SimpleNamespace()))
    assert capsys.readouterr().out == ""
    st = IgnoreStats()
    st.push(torch.tensor([0, 30, 6, 0], dtype=torch.int32))
    trainer.print_ignore(4, 2, 9, SimpleNamespace(dataset=SimpleNamespace(ignore_stats=st)), lag=1)
    assert capsys.readouterr().out == ""
    trainer.print_ignore(4, 2, 9, SimpleNamespace(dataset=SimpleNamespace(ignore_stats=st)))
    assert capsys.readouterr().out == "Epoch: [2][4/9]\tignore regions: 9.0 anchors per image turned from negative to ignored, 50 % of 4 images with any\n"


def test_main_flags(capsys):
    import main
    from tinyfaces.datasets.augment import IgnorePolicy, check_ignore_policy
    base = ["train.txt", "val.txt"]
    off = main.trunk_arguments(base)
    assert off.ignore_policy is None and off.ignore is None and "off" in main.ignore_description(off)
    cases = [(["--ignore-invalid"], IgnorePolicy(invalid=True), "flagged invalid"),
             (["--ignore-blur", "2"], IgnorePolicy(blur=2), "blur >= 2"),
             (["--ignore-occlusion", "1"], IgnorePolicy(occlusion=1), "occlusion >= 1"),
             (["--ignore-min-size", "8"], IgnorePolicy(min_size=8.0), "below 8 px"),
             (["--ignore-truncated"], IgnorePolicy(truncated=True), "the crop drops")]
    for flags, policy, words in cases:
        a = main.trunk_arguments(base + flags)
        assert a.ignore_policy == policy == check_ignore_policy(a.ignore_policy) and a.ignore == ("iof", 0.5)
        assert words in main.ignore_description(a) and "intersection over the anchor's area >= 0.5" in main.ignore_description(a)
    a = main.trunk_arguments(base + ["--ignore-invalid", "--ignore-blur", "1", "--ignore-truncated", "--ignore-measure", "iou", "--ignore-thresh", "0.3",
                                     "--anchor-compensation", "3", "0.1"])
    assert a.ignore_policy == IgnorePolicy(True, 1, None, None, True) and a.ignore == ("iou", 0.3) and a.anchor_compensation == (3, 0.1)
    assert "IoU >= 0.3" in main.ignore_description(a)
    assert main.trunk_arguments(base + ["--ignore-truncated", "--ignore-thresh", "1"]).ignore == ("iof", 1.0)
    for bad in (["--ignore-measure", "iou"], ["--ignore-thresh", "0.4"],                       # the two given alone
                ["--ignore-blur", "0"], ["--ignore-blur", "3"], ["--ignore-blur", "1.5"], ["--ignore-occlusion", "3"], ["--ignore-min-size", "0"],
                ["--ignore-min-size", "nan"], ["--ignore-min-size", "-2"], ["--ignore-invalid", "--ignore-thresh", "0"],
                ["--ignore-invalid", "--ignore-thresh", "1.5"], ["--ignore-invalid", "--ignore-thresh", "nan"], ["--ignore-invalid", "--ignore-measure", "giou"]):
        with pytest.raises(SystemExit):
            main.trunk_arguments(base + bad)
    err = capsys.readouterr().err
    assert "--ignore-measure needs one of" in err and "--ignore-thresh needs one of" in err and "0 < T <= 1" in err and "1..2" in err


def test_entry_point_refuses_before_it_enqueues(hip):
    """tf_targets_apply_ignore: a thresh outside (0, 1] or not finite, an unknown measure and negative sizes come back as TF_ERR_ARG; no
    ignore box (NULL) is TF_OK.  Runs without a GPU: the operands are host memory nobody dereferences."""
    l = hip.lib()
    assert "tf_targets_apply_ignore" in hip.symbols() and "tf_targets_apply_ignore" in hip._SIGNATURES and l.tf_version() >= 770
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)

    def call(B=2, nt=3, vsy=5, vsx=7, tstride=5, measure=0, thresh=0.5, cls=p, boxes=p):
        return l.tf_targets_apply_ignore(cls, B, nt, vsy, vsx, p, tstride, -1, -1, 8, 8, boxes, p, measure, thresh, None, None)

    for thresh in (0.0, -0.5, 1.5, np.nextafter(1.0, 2.0), float("nan"), float("inf"), -float("inf")):
        assert call(thresh=thresh) == -1
    for measure in (-1, 2, 7):
        assert call(measure=measure) == -1
    for kw in (dict(B=-1), dict(nt=-1), dict(vsy=-3), dict(vsx=-1), dict(tstride=3), dict(cls=None)):
        assert call(**kw) == -1
    assert call(boxes=None) == 0 and call(boxes=None, thresh=1.0, measure=1) == 0 and call(B=0) == 0 and call(nt=0) == 0
    assert call(boxes=None, thresh=0.0) == -1                        # the arguments are judged first


# ------------------------------------------------------------------------------------------------ augmentation
class _DeviceImage:
    """What process_inputs asks of the image before the launch."""
    is_cuda = True

    def __init__(self, h, w):
        self.shape = (h, w, 3)


@pytest.fixture
def launches(monkeypatch):
    from tinyfaces import ops
    calls = []
    monkeypatch.setattr(ops, "image_prepare", lambda img, **kw: calls.append(kw) or "x")
    return calls


# a 600 x 800 image: two ordinary faces, an invalid one, a blur-2 one, a face of 10 px (5.5 px after the half-scale draw), and a large face
# that the 500-pixel crop of the doubled image cuts
BOXES = np.array([[100., 120., 180., 220.], [300., 310., 340., 360.], [420., 100., 470., 160.], [520., 300., 580., 380.], [250., 200., 259., 211.],
                  [330., 30., 640., 420.]])
ATTRS = {"invalid": np.array([0., 0., 1., 0., 0., 0.]), "blur": np.array([0., 1., 0., 2., 0., 0.]), "occlusion": np.array([0., 0., 0., 0., 2., 0.])}


def _decisions(seed, H=600, W=800):
    """The decisions process_inputs draws for this seed, by hand: (scale factor, crop, paste, flip) and the generator behind them."""
    from tinyfaces.datasets import augment as da
    ref = np.random.RandomState(seed)
    rnd = ref.rand()
    z = 0.5 if rnd < 1 / 3 else (2.0 if rnd > 2 / 3 else 1.0)
    crop, paste, _ = da.crop_decisions(int(z * H), int(z * W), np.zeros((0, 4)), rng=ref)
    return z, crop, paste, bool(ref.rand() > 0.5), ref


def test_policy_off_returns_what_it_returned_and_both_consume_the_same_stream(launches):
    from tinyfaces.datasets import augment as da
    policy = da.IgnorePolicy(invalid=True, blur=2, occlusion=2, min_size=8, truncated=True)
    for seed in range(12):
        z, crop, paste, flip, ref = _decisions(seed)
        rng0, rng1 = np.random.RandomState(seed), np.random.RandomState(seed)
        _, b0, paste0, flip0 = da.process_inputs(_DeviceImage(600, 800), BOXES, rng=rng0)
        got = []
        out = da.process_inputs(_DeviceImage(600, 800), BOXES, rng=rng1, ignore_policy=policy, attributes=ATTRS, ignore_out=got)
        assert len(out) == 4 and (out[2], out[3]) == (paste0, flip0) == (paste, flip)
        assert launches[-1] == launches[-2] and launches[-1]["crop"] == crop                 # the pixels do not know the policy
        nxt = ref.rand()
        assert rng0.rand() == nxt and rng1.rand() == nxt                                      # the feature draws nothing
        # off: today's boxes -- the reference bookkeeping with nothing flagged and nothing collected
        faces, _ = ignore_ref.policy_boxes(BOXES * z, None, SimpleNamespace(invalid=False, blur=None, occlusion=None, min_size=None, truncated=False),
                                           crop, paste, flip)
        assert np.array_equal(b0, faces)
        # None is the default, and an ignore_out without a policy stays untouched
        keep = ["untouched"]
        _, b2, _, _ = da.process_inputs(_DeviceImage(600, 800), BOXES, rng=np.random.RandomState(seed), ignore_policy=None, ignore_out=keep)
        assert np.array_equal(b2, b0) and keep == ["untouched"]


FIELDS = {"invalid": dict(invalid=True), "blur": dict(blur=2), "min_size": dict(min_size=8), "truncated": dict(truncated=True),
          "all": dict(invalid=True, blur=2, occlusion=2, min_size=8, truncated=True)}


@pytest.mark.parametrize("field", list(FIELDS))
def test_planted_faces_land_where_the_reference_says(launches, field):
    from tinyfaces.datasets import augment as da
    policy = da.IgnorePolicy(**FIELDS[field])
    seen = {"ignored": 0, "flip": 0, "half": 0, "cut": 0}
    for seed in range(40):
        z, crop, paste, flip, _ = _decisions(seed)
        got = []
        _, b, _, _ = da.process_inputs(_DeviceImage(600, 800), BOXES, rng=np.random.RandomState(seed), ignore_policy=policy, attributes=ATTRS, ignore_out=got)
        faces, ign = ignore_ref.policy_boxes(BOXES * z, ATTRS, policy, crop, paste, flip)
        got = np.array(got, dtype=np.float64).reshape(-1, 4)
        assert np.array_equal(b, faces) and np.array_equal(got, ign), (field, seed)
        assert got.dtype == np.float64 and bool((got[:, 2] > got[:, 0]).all()) and bool((got[:, 3] > got[:, 1]).all())
        assert got.min(initial=0) >= 0 and got.max(initial=0) <= 501
        seen["ignored"] += got.shape[0]
        seen["flip"] += int(flip and got.shape[0] > 0)
        seen["half"] += int(z == 0.5 and got.shape[0] > 0)
        if field == "truncated":
            seen["cut"] += got.shape[0]
        if field == "invalid":
            assert got.shape[0] <= 1 and not any(np.array_equal(r, g) for r in b for g in got)      # the flagged face owns no positive
        if field == "min_size":
            assert got.shape[0] == (1 if z == 0.5 else 0)            # 10 px at x1 and 20 at x2, 5.5 px after the half-scale draw (the half image fits the canvas whole)
    assert seen["ignored"] > 0 and seen["flip"] > 0
    if field == "min_size":
        assert seen["half"] > 0
    if field == "truncated":
        assert seen["cut"] > 0


def test_hand_worked_bookkeeping(launches):
    """A 500 x 500 image at scale 1 has one crop and one paste position: boxes stay where they are, up to the mirror."""
    from tinyfaces.datasets import augment as da
    boxes = np.array([[100., 100., 150., 160.], [300., 200., 380., 290.], [20., 400., 60., 450.]])
    attrs = {"invalid": [0, 1, 0], "blur": [2, 0, 0], "occlusion": [0, 0, 0]}
    done = set()
    for seed in range(60):
        rnd = np.random.RandomState(seed).rand()
        if not 1 / 3 <= rnd <= 2 / 3:
            continue
        got = []
        _, b, paste, flip = da.process_inputs(_DeviceImage(500, 500), boxes, rng=np.random.RandomState(seed), ignore_policy=da.IgnorePolicy(invalid=True, blur=2),
                                              attributes=attrs, ignore_out=got)
        assert paste == [0, 0, 500, 500]
        if flip:
            assert np.array_equal(b, [[441., 400., 481., 450.]]) and np.array_equal(got, [[351., 100., 401., 160.], [121., 200., 201., 290.]])
        else:
            assert np.array_equal(b, boxes[2:]) and np.array_equal(got, boxes[:2])
        done.add(flip)
    assert done == {True, False}


# ------------------------------------------------------------------------------------------------ the motivation figure
def crowd_layout(rng, H=768, W=1024, n=60):
    """n faces of log-uniform side 6-90 px (aspect 0.8) on an H x W image: a WIDER crowd picture in miniature."""
    s = np.exp(rng.uniform(np.log(6), np.log(90), n))
    x, y = rng.uniform(0, W - 0.8 * s), rng.uniform(0, H - s)
    return np.round(np.stack([x, y, x + 0.8 * s, y + s], 1), 2)


def crowd_statistics(templates, crops=200):
    """`crops` seeded crops (np.random.RandomState(1000 + i): layout, then process_inputs' own draws).  From the oracle alone: per crop the
    class map of the faces that survive; the negative anchors of it that sit with IoF >= 0.5 on what is left of the faces the crop dropped
    (policy truncated), and the faces min_size = 8 flags (counted where something of them is left in the crop) with the negatives on them."""
    from tinyfaces.datasets import augment as da
    tot = dict(crops=crops, faces_kept=0, faces_cut=0, faces_cut_8px=0, crops_with_cut=0, negatives_on_cut=0, faces_small=0, negatives_on_small=0, negatives=0)
    trunc = SimpleNamespace(invalid=False, blur=None, occlusion=None, min_size=None, truncated=True)
    small = SimpleNamespace(invalid=False, blur=None, occlusion=None, min_size=8.0, truncated=False)
    for i in range(crops):
        rng = np.random.RandomState(1000 + i)
        boxes = crowd_layout(rng)
        rnd = rng.rand()
        z = 0.5 if rnd < 1 / 3 else (2.0 if rnd > 2 / 3 else 1.0)
        crop, paste, _ = da.crop_decisions(int(z * 768), int(z * 1024), np.zeros((0, 4)), rng=rng)
        flip = bool(rng.rand() > 0.5)
        faces, cut = ignore_ref.policy_boxes(boxes * z, None, trunc, crop, paste, flip)
        _, tiny = ignore_ref.policy_boxes(boxes * z, None, small, crop, paste, flip)
        pad = otgt.get_padding(templates, paste)
        pad = np.fliplr(pad) if flip else pad
        cm, _, _ = otgt.get_heatmaps(faces.copy(), templates, pad, noise=np.zeros((63, 63, 25, faces.shape[0])))
        tot["faces_kept"] += faces.shape[0]
        tot["faces_cut"] += cut.shape[0]
        tot["faces_cut_8px"] += int((np.minimum(cut[:, 2] - cut[:, 0], cut[:, 3] - cut[:, 1]) + 1 >= 8).sum())
        tot["crops_with_cut"] += int(cut.shape[0] > 0)
        tot["negatives"] += int((cm == -1).sum())
        tot["negatives_on_cut"] += ignore_ref.apply_ignore(cm, templates, cut, "iof", 0.5)[1]
        tot["faces_small"] += tiny.shape[0]
        tot["negatives_on_small"] += ignore_ref.apply_ignore(cm, templates, tiny, "iof", 0.5)[1]
    return tot


def test_crowd_statistics(templates):
    t = crowd_statistics(templates)
    lines = ["# 200 seeded 500 x 500 training crops of crowd layouts (60 faces of 6-90 px on 768 x 1024, the scale / crop / paste / flip draws of",
             "# process_inputs), golden templates, numpy oracle only.  Written by tests/test_ignore_regions.py::test_crowd_statistics (no GPU).",
             "# cut = faces the crop drops for overlap < 0.3 whose clamped box is not degenerate (crop_image's clamp leaves a face that lies wholly",
             "# outside as a sliver one pixel wide on the border: those count, and cover at most 2 / width of an anchor); of them >= 8 px = both sides of what is left at",
             "# least 8 px; small = faces whose shorter side is below 8 px after the scale draw (min_size = 8), counted where they lie in the crop;",
             "# negatives on them = anchors labelled -1 with IoF >= 0.5 (no template is small enough to sit half inside a face below 8 px: the small",
             "# faces matter through the forced positive they lose, not through the anchors on them).",
             "# No accuracy claim: this counts training targets, it does not train.",
             "# crops | faces kept | faces cut | of them >= 8 px | crops with a cut face | negatives on cut faces | small faces | negatives on small faces | negatives in all",
             f"{t['crops']} | {t['faces_kept']} | {t['faces_cut']} | {t['faces_cut_8px']} | {t['crops_with_cut']} | {t['negatives_on_cut']} | {t['faces_small']} | "
             f"{t['negatives_on_small']} | {t['negatives']}"]
    try:
        with open(os.path.join(ROOT, "profiles", "ignore_regions_stats.txt"), "w") as f:
            f.write("\n".join(lines) + "\n")
    except OSError:
        pass                                                         # a read-only checkout still checks the facts below
    assert t["faces_cut"] > 0 and t["negatives_on_cut"] > 0          # the crop leaves visible parts of faces under negative anchors
    assert t["faces_small"] > 0
