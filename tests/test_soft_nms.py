"""CPU: the host side of Soft-NMS (csrc/soft_nms.hip): the new keywords and their defaults, evaluate_model.py's flags parsed apart from the
older parsers' options, the refusal of CPU tensors and of bad arguments, the C entry points' argument checks, the workspace query, and the
numpy restatement (tests/soft_nms_ref.py) on hand-computed cases.  The kernels run in tests/test_gpu_soft_nms.py."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import soft_nms_ref

# IoU exactly 0.5: inter 50, areas 100 and 50, 50 / (100 + 50 - 50)
PAIR = np.array([[0, 0, 10, 10], [0, 0, 10, 5]], dtype=np.float64)
PAIR_P = np.array([0.9, 0.8])


def test_keywords_exist_with_their_defaults():
    import evaluate_model
    from tinyfaces import evaluation, ops
    for fn in (evaluation.get_detections, evaluation.get_detections_batch, evaluate_model.run):
        p = inspect.signature(fn).parameters
        names = list(p)
        assert names[-3:] == ["soft_nms", "soft_nms_sigma", "soft_nms_score_thresh"], fn.__name__
        assert names[names.index("box_voting") + 1] == "soft_nms", fn.__name__          # appended after box_voting
        assert (p["soft_nms"].default, p["soft_nms_sigma"].default, p["soft_nms_score_thresh"].default) == (None, 0.5, 0.001), fn.__name__
        assert p["flip"].default is False and p["box_voting"].default is None
    p = inspect.signature(ops.soft_nms).parameters
    assert list(p) == ["boxes", "scores", "method", "iou_threshold", "sigma", "score_threshold", "score"]
    assert [p[k].default for k in list(p)[2:]] == ["linear", 0.3, 0.5, 0.001, "sigmoid"]
    p = inspect.signature(ops.soft_nms_batched).parameters
    assert list(p) == ["boxes", "scores", "seg_offsets", "method", "iou_threshold", "sigma", "score_threshold", "score", "mask_budget_bytes", "vote"]
    assert [p[k].default for k in list(p)[3:]] == ["linear", 0.3, 0.5, 0.001, "sigmoid", None, None]
    assert ops.SOFT_NMS_METHODS == {"linear": 1, "gaussian": 2} and ops.SOFT_NMS_MAX_BOXES >= 65536
    # signatures of existing functions do not change
    assert list(inspect.signature(ops.nms_batched).parameters) == ["boxes", "scores", "seg_offsets", "iou_threshold", "mask_budget_bytes", "vote"]
    assert list(inspect.signature(ops.nms).parameters) == ["boxes", "scores", "iou_threshold"]


def test_header_names_the_constants_the_binding_uses(hip):
    import os
    import re
    from tinyfaces import ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "tinyfaces_hip.h")).read()
    defs = dict(re.findall(r"#define (TF_SOFT_NMS_[A-Z_]+)\s+(\d+)", src))
    assert int(defs["TF_SOFT_NMS_LINEAR"]) == ops.SOFT_NMS_METHODS["linear"] == 1
    assert int(defs["TF_SOFT_NMS_GAUSSIAN"]) == ops.SOFT_NMS_METHODS["gaussian"] == 2
    assert int(defs["TF_SOFT_NMS_MAX_BOXES"]) == ops.SOFT_NMS_MAX_BOXES
    assert {"tf_soft_nms_f64", "tf_soft_nms_f64_batched", "tf_soft_nms_workspace_bytes", "tf_soft_nms_batched_workspace_bytes"} <= set(hip.symbols())
    assert hip.lib().tf_version() >= 680


def test_evaluate_model_flags_are_parsed_apart():
    import evaluate_model
    a = evaluate_model.soft_nms_arguments(["DATA"])
    assert (a.soft_nms, a.soft_nms_sigma, a.soft_nms_score_thresh) == (None, 0.5, 0.001)
    assert a.flip is False and a.box_voting is None and a.ema is False
    a = evaluate_model.soft_nms_arguments(["DATA", "--soft-nms", "gaussian", "--soft-nms-sigma", "0.25", "--soft-nms-score-thresh", "0.01",
                                           "--flip", "--box-voting", "0.5", "--ema", "--num-images", "1"])
    assert (a.soft_nms, a.soft_nms_sigma, a.soft_nms_score_thresh) == ("gaussian", 0.25, 0.01)
    assert a.flip is True and a.box_voting == 0.5 and a.ema is True and a.num_images == 1 and a.dataset == "DATA"
    a = evaluate_model.soft_nms_arguments(["--soft-nms=linear", "DATA", "--nms_thresh", "0.4", "--soft-nms-score-thresh", "0"])
    assert a.soft_nms == "linear" and a.nms_thresh == 0.4 and a.soft_nms_score_thresh == 0.0
    # the three older parsers keep their results and keep refusing the new flags
    for parse in (evaluate_model.arguments, evaluate_model.ema_arguments, evaluate_model.tta_arguments):
        assert not [k for k in vars(parse(["DATA"])) if k.startswith("soft_nms")]
        for argv in (["--soft-nms", "linear"], ["--soft-nms-sigma", "0.5"], ["--soft-nms-score-thresh", "0.01"]):
            with pytest.raises(SystemExit):
                parse(["DATA"] + argv)
    t = evaluate_model.tta_arguments(["DATA", "--flip", "--box-voting", "0.5", "--ema"])
    assert t.flip is True and t.box_voting == 0.5 and t.ema is True
    for bad in (["--soft-nms", "foo"], ["--soft-nms"], ["--soft-nms-sigma", "0"], ["--soft-nms-sigma", "-1"], ["--soft-nms-sigma", "nan"],
                ["--soft-nms-score-thresh", "-0.1"], ["--soft-nms-score-thresh", "nan"], ["--soft-nms-score-thresh", "abc"]):
        with pytest.raises(SystemExit):
            evaluate_model.soft_nms_arguments(["DATA"] + bad)


def test_cpu_tensors_and_bad_arguments_raise():
    from tinyfaces import evaluation, ops
    boxes, scores = torch.zeros(3, 4, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.soft_nms(boxes, scores)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.soft_nms_batched(boxes, scores, [0, 3], "gaussian")
    # bad methods and ranges: ValueError before anything is launched (the checks need no device)
    for kw in (dict(method="softer"), dict(score="softmax"), dict(iou_threshold=-0.1), dict(iou_threshold=1.5), dict(iou_threshold=float("nan")),
               dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(score_threshold=-1e-9), dict(score_threshold=float("nan"))):
        full = {"method": "linear", "iou_threshold": 0.3, "sigma": 0.5, "score_threshold": 0.001, "score": "sigmoid", **kw}
        with pytest.raises(ValueError):
            ops._soft_nms_mode(**full)
    assert ops._soft_nms_mode("gaussian", 0.0, 0.5, 0.0, "score") == (2, 0.0, 0.5, 0.0, 1)
    for kw in (dict(soft_nms="foo"), dict(soft_nms="linear", soft_nms_sigma=0.0), dict(soft_nms="gaussian", soft_nms_score_thresh=-1.0)):
        with pytest.raises(ValueError):
            evaluation.get_detections(None, None, None, None, None, device="cuda", **kw)
        with pytest.raises(ValueError):
            evaluation.get_detections_batch(None, [None], None, None, None, device="cuda", **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluation.get_detections(None, None, None, None, None, device="cpu", soft_nms="linear")


def test_entry_points_check_their_arguments_without_launching(hip):
    """Host-side refusals of the two entry points (nothing is enqueued; runs without a GPU)."""
    l = hip.lib()
    ERR_ARG = -1
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    off = (C.c_int32 * 3)(0, 2, 4)
    good = dict(method=1, iou=0.3, sigma=0.5, sthr=0.001, mode=0)

    def call(boxes=p, scores=p, offs=off, S=2, keep=p, score_out=p, num_keep=p, ws=p, wsb=1 << 20, **kw):
        a = {**good, **kw}
        return l.tf_soft_nms_f64_batched(boxes, scores, offs, S, a["method"], a["iou"], a["sigma"], a["sthr"], a["mode"], keep, score_out, num_keep,
                                         ws, wsb, None)

    for method in (0, 3, -1):
        assert call(method=method) == ERR_ARG                                  # unknown method
    for mode in (2, -1):
        assert call(mode=mode) == ERR_ARG                                      # unknown score mode
    for sigma in (0.0, -0.5, float("nan")):
        assert call(sigma=sigma) == ERR_ARG
    for iou in (-1e-9, 1.0 + 2.0 ** -52, float("nan")):
        assert call(iou=iou) == ERR_ARG
    for sthr in (-1e-300, float("nan")):
        assert call(sthr=sthr) == ERR_ARG
    assert call(S=0) == ERR_ARG and call(S=65) == ERR_ARG and call(offs=None) == ERR_ARG
    assert call(offs=(C.c_int32 * 3)(0, 4, 2)) == ERR_ARG                      # descending offsets
    assert call(offs=(C.c_int32 * 3)(1, 2, 4)) == ERR_ARG                      # offsets start at 0
    assert call(num_keep=None) == ERR_ARG
    assert call(boxes=None) == ERR_ARG and call(scores=None) == ERR_ARG and call(keep=None) == ERR_ARG and call(score_out=None) == ERR_ARG
    assert call(ws=None) == -4 and call(wsb=8) == -4                           # TF_ERR_WORKSPACE, still nothing launched
    too_long = (C.c_int32 * 2)(0, 65537)
    assert call(offs=too_long, S=1, wsb=1 << 40) == -3                         # TF_ERR_UNSUPPORTED: above TF_SOFT_NMS_MAX_BOXES
    # n == 0: nothing to do, nothing needed
    assert call(boxes=None, scores=None, offs=(C.c_int32 * 3)(0, 0, 0), keep=None, score_out=None, ws=None, wsb=0, method=2, mode=1) == 0
    assert l.tf_soft_nms_f64(p, p, -1, 1, 0.3, 0.5, 0.001, 0, p, p, p, p, 1 << 20, None) == ERR_ARG
    assert l.tf_soft_nms_f64(p, p, 4, 7, 0.3, 0.5, 0.001, 0, p, p, p, p, 1 << 20, None) == ERR_ARG
    assert l.tf_soft_nms_f64(None, None, 0, 1, 0.3, 0.5, 0.0, 0, None, None, p, None, 0, None) == 0


def test_workspace_bytes_are_monotone_and_zero_for_nothing(hip):
    l = hip.lib()
    assert l.tf_soft_nms_workspace_bytes(0) == 0 and l.tf_soft_nms_workspace_bytes(-3) == 0
    sizes = [l.tf_soft_nms_workspace_bytes(n) for n in (1, 2, 63, 64, 65, 130, 1025, 4097, 20000, 65536)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert sizes[-1] >= 65536 * 65536 // 8 + 65536 * 8                         # the bit matrix and the running scores
    assert l.tf_soft_nms_batched_workspace_bytes((C.c_int32 * 3)(0, 0, 0), 2) == 0
    both = l.tf_soft_nms_batched_workspace_bytes((C.c_int32 * 4)(0, 130, 130, 1155), 3)
    assert both >= l.tf_soft_nms_workspace_bytes(130) and both >= l.tf_soft_nms_workspace_bytes(1025)
    assert both <= l.tf_soft_nms_workspace_bytes(130) + l.tf_soft_nms_workspace_bytes(1025)


# --------------------------------------------------------------------------- the reference on hand-computed cases
def test_reference_linear_decay_and_the_score_threshold_is_inclusive():
    """Case 1: IoU exactly 0.5 > 0.3: the second score is 0.8 * (1 - 0.5) = 0.4 exactly; `>=`: kept at score_thresh = 0.4, dropped at the next
    double above it."""
    keep, sc, _, _ = soft_nms_ref.soft_nms(PAIR, PAIR_P, "linear", 0.3, 0.5, 0.4, score="score")
    assert keep.tolist() == [0, 1] and sc.tolist() == [0.9, 0.4]
    keep, sc, _, _ = soft_nms_ref.soft_nms(PAIR, PAIR_P, "linear", 0.3, 0.5, np.nextafter(0.4, 1.0), score="score")
    assert keep.tolist() == [0] and sc.tolist() == [0.9]


def test_reference_iou_threshold_is_strict():
    """Case 2: the same pair at iou_thresh = 0.5: `>` -- no decay."""
    keep, sc, _, _ = soft_nms_ref.soft_nms(PAIR, PAIR_P, "linear", 0.5, 0.5, 0.001, score="score")
    assert keep.tolist() == [0, 1] and sc.tolist() == [0.9, 0.8]
    keep, sc, _, _ = soft_nms_ref.soft_nms(PAIR, PAIR_P, "linear", np.nextafter(0.5, 0.0), 0.5, 0.001, score="score")
    assert sc.tolist() == [0.9, 0.4]


def test_reference_reranks():
    """Case 3: A (0.9), B (0.8, IoU 0.8 with A), C (0.7, disjoint): B falls to 0.8 * (1 - 0.8) behind C -- the order is A, C, B; the hard NMS
    at 0.3 drops B."""
    from oracle.nms import nms
    boxes = np.array([[0, 0, 10, 10], [0, 0, 10, 8], [20, 20, 30, 30]], dtype=np.float64)
    p = np.array([0.9, 0.8, 0.7])
    keep, sc, _, _ = soft_nms_ref.soft_nms(boxes, p, "linear", 0.3, 0.5, 0.001, score="score")
    assert keep.tolist() == [0, 2, 1] and sc.tolist() == [0.9, 0.7, 0.8 * (1.0 - 0.8)]
    assert np.asarray(nms(boxes, p, 0.3)).tolist() == [0, 2]


def test_reference_gaussian_factor():
    """Case 4: IoU 0.5, sigma 0.5: the factor is exp(-0.25 / 0.5) = exp(-0.5); iou_thresh plays no part."""
    for iou_thresh in (0.3, 0.9):
        keep, sc, _, _ = soft_nms_ref.soft_nms(PAIR, PAIR_P, "gaussian", iou_thresh, 0.5, 0.001, score="score")
        assert keep.tolist() == [0, 1] and sc.tolist() == [0.9, 0.8 * np.exp(-0.5)]
    # sigmoid mode: the scores are logits
    logits = np.array([2.0, 1.0])
    keep, sc, _, _ = soft_nms_ref.soft_nms(PAIR, logits, "gaussian", 0.3, 0.5, 0.001)
    w = 1.0 / (1.0 + np.exp(-logits))
    assert keep.tolist() == [0, 1] and sc.tolist() == [w[0], w[1] * np.exp(-0.5)]


def test_reference_exact_duplicate_with_equal_scores():
    """Case 5: the lower index goes first; linear: the other gets the factor 1 - 1 = 0 -- dropped for any score_thresh > 0, kept with score 0 at 0."""
    boxes = np.array([[3, 4, 13, 24], [3, 4, 13, 24]], dtype=np.float64)
    p = np.array([0.75, 0.75])
    keep, sc, rank_margin, _ = soft_nms_ref.soft_nms(boxes, p, "linear", 0.3, 0.5, 5e-324, score="score")
    assert keep.tolist() == [0] and sc.tolist() == [0.75]
    assert rank_margin == np.inf                                               # a bit-equal runner-up is no margin
    keep, sc, _, _ = soft_nms_ref.soft_nms(boxes, p, "linear", 0.3, 0.5, 0.0, score="score")
    assert keep.tolist() == [0, 1] and sc.tolist() == [0.75, 0.0]
    keep, sc, _, _ = soft_nms_ref.soft_nms(boxes, p, "gaussian", 0.3, 0.5, 0.001, score="score")
    assert keep.tolist() == [0, 1] and sc.tolist() == [0.75, 0.75 * np.exp(-2.0)]


def test_reference_zero_area_box_is_never_decayed_and_decays_nobody():
    """Case 6: a zero-area box has IoU 0 with everything else and 0 / 0 = NaN with itself and its duplicate."""
    boxes = np.array([[5, 5, 5, 9], [4, 4, 8, 16], [5, 5, 5, 9]], dtype=np.float64)
    p = np.array([0.95, 0.9, 0.5])
    for method in ("linear", "gaussian"):
        keep, sc, _, _ = soft_nms_ref.soft_nms(boxes, p, method, 0.0, 0.5, 0.001, score="score")
        assert keep.tolist() == [0, 1, 2] and sc.tolist() == [0.95, 0.9, 0.5]


def test_reference_margins_and_nan():
    """The two margins of a run, on numbers one can check by hand; a NaN score is never live."""
    boxes = np.array([[0, 0, 10, 10], [0, 0, 10, 5], [50, 50, 60, 60], [70, 70, 80, 80]], dtype=np.float64)
    p = np.array([0.8, 0.5, 0.75, np.nan])
    keep, sc, rank_margin, thresh_margin = soft_nms_ref.soft_nms(boxes, p, "linear", 0.3, 0.5, 0.2, score="score")
    assert keep.tolist() == [0, 2, 1] and sc.tolist() == [0.8, 0.75, 0.25]
    assert rank_margin == (0.8 - 0.75) / 0.8                                   # the closest race: 0.8 against 0.75
    assert thresh_margin == abs(0.25 - 0.2) / 0.2                              # the closest liveness test: 0.25 against 0.2
    res = soft_nms_ref.soft_nms_batched(np.concatenate([boxes, boxes]), np.concatenate([p, p]), [0, 4, 4, 8], method="linear", iou_thresh=0.3,
                                        score_thresh=0.2, score="score")
    assert [r[0].tolist() for r in res] == [[0, 2, 1], [], [4, 6, 5]]
    assert soft_nms_ref.score_bound(3) == 40 * 2.0 ** -52
    with pytest.raises(ValueError):
        soft_nms_ref.soft_nms(boxes, p, "softer")
