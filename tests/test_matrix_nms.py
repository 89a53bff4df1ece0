"""CPU: the host side of Matrix NMS (csrc/matrix_nms.hip): the numpy restatement (tests/matrix_nms_ref.py) on hand-worked cases and its
invariants, the signatures and constants of the binding, evaluate_model.py's parser, the refusals that need no device, and the condition on
the inputs of tests/test_gpu_matrix_nms.py (tests/matrix_nms_cases.py) under which that file may ask for equal keep lists.  The kernels run
there."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import matrix_nms_cases as mc
import matrix_nms_ref as ref
import vote_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# IoU exactly 0.5: inter 50, areas 100 and 50, 50 / (100 + 50 - 50)
PAIR = np.array([[0, 0, 10, 10], [0, 0, 10, 5]], dtype=np.float64)


def _run(boxes, p, method, **kw):
    kw = {"sigma": 0.5, "score_thresh": 0.001, "score": "score", **kw}
    keep, s, _, _, det = ref.matrix_nms(np.asarray(boxes, dtype=np.float64), np.asarray(p, dtype=np.float64), method, details=True, **kw)
    return keep.tolist(), s.tolist(), det


# --------------------------------------------------------------------------- the restatement on hand-worked cases
def test_reference_two_boxes():
    """IoU 0.5, comp_0 = 0.  Linear: d_1 = (1 - 0.5) / (1 - 0) = 0.5, s_1 = 0.8 * 0.5 = 0.4 exactly; emission is `>=`.  Gaussian, sigma 0.5:
    x_1 = 0.25 - 0, d_1 = exp(-0.5)."""
    assert _run(PAIR, [0.9, 0.8], "linear")[:2] == ([0, 1], [0.9, 0.4])
    assert _run(PAIR, [0.9, 0.8], "linear", score_thresh=0.4)[:2] == ([0, 1], [0.9, 0.4])
    assert _run(PAIR, [0.9, 0.8], "linear", score_thresh=float(np.nextafter(0.4, 1.0)))[:2] == ([0], [0.9])
    assert _run(PAIR, [0.9, 0.8], "gaussian")[:2] == ([0, 1], [0.9, 0.8 * np.exp(-0.5)])
    assert _run(PAIR, [0.9, 0.8], "gaussian", sigma=0.25)[:2] == ([0, 1], [0.9, 0.8 * np.exp(-1.0)])
    # the rank is by p, not by input order; sigmoid mode: the scores are logits
    assert _run(PAIR, [0.8, 0.9], "linear")[:2] == ([1, 0], [0.9, 0.4])
    logits = np.array([2.0, 1.0])
    w = 1.0 / (1.0 + np.exp(-logits))
    assert _run(PAIR, logits, "gaussian", score="sigmoid")[:2] == ([0, 1], [w[0], w[1] * np.exp(-0.5)])


def test_reference_three_boxes_by_hand_and_the_emission_order():
    """A = (0,0,10,10) 0.9; B = (0,0,10,8) 0.8, IoU(A,B) = 0.8; C = (20,20,30,30) 0.7, disjoint.  comp = 0, 0.8, 0.  Linear: d_B = 0.2 (rounded
    as 1 - 0.8), d_C = min(1 / 1, 1 / (1 - 0.8)) = 1: B falls behind C in the output."""
    abc = np.array([[0, 0, 10, 10], [0, 0, 10, 8], [20, 20, 30, 30]], dtype=np.float64)
    keep, s, det = _run(abc, [0.9, 0.8, 0.7], "linear")
    assert det["comp"].tolist() == [0.0, 0.8, 0.0] and det["d"].tolist() == [1.0, 1.0 - 0.8, 1.0]
    assert keep == [0, 2, 1] and s == [0.9, 0.7, 0.8 * (1.0 - 0.8)]
    keep, s, det = _run(abc, [0.9, 0.8, 0.7], "gaussian")
    assert det["arg"].tolist() == [0.0, 0.8 * 0.8, 0.0]                        # C: max(0 - 0, 0 - 0.64) = 0
    assert keep == [0, 2, 1] and s == [0.9, 0.7, 0.8 * np.exp(-(0.8 * 0.8) / 0.5)]
    assert _run(abc, [0.9, 0.8, 0.7], "linear", max_keep=2)[:2] == ([0, 2], [0.9, 0.7])


def test_reference_three_identical_boxes():
    """comp = 0, 1, 1.  Linear: d_1 = (1 - 1) / (1 - 0) = 0; for the third the second contributes no term (comp_1 >= 1: 0 / 0 otherwise) and the
    first gives 0: d = 1, 0, 0.  Gaussian: x_1 = 1 - 0, x_2 = max(1 - 0, 1 - 1) = 1: d = 1, e^(-1/sigma), e^(-1/sigma)."""
    same = np.array([[3, 4, 13, 24]] * 3, dtype=np.float64)
    keep, s, det = _run(same, [0.9, 0.8, 0.7], "linear", score_thresh=0.0)
    assert det["comp"].tolist() == [0.0, 1.0, 1.0] and det["d"].tolist() == [1.0, 0.0, 0.0]
    assert keep == [0, 1, 2] and s == [0.9, 0.0, 0.0]                          # bit-equal s: the better rank first
    assert _run(same, [0.9, 0.8, 0.7], "linear")[:2] == ([0], [0.9])
    for sigma in (0.5, 0.3):
        keep, s, det = _run(same, [0.9, 0.8, 0.7], "gaussian", sigma=sigma)
        e = np.exp(-1.0 / np.float64(sigma))
        assert det["d"].tolist() == [1.0, e, e] and keep == [0, 1, 2] and s == [0.9, 0.8 * e, 0.7 * e]


def test_reference_disjoint_boxes_keep_their_rank():
    far = np.array([[100.0 * i, 0, 100.0 * i + 10, 10] for i in range(9)])
    p = np.array([0.5, 0.7, 0.5, 0.9, 0.5, 0.7, 0.1, 0.5, 0.3])
    for method in ref.METHODS:
        keep, s, det = _run(far, p, method)
        assert det["d"].tolist() == [1.0] * 9 and det["comp"].tolist() == [0.0] * 9
        assert keep == [3, 1, 5, 0, 2, 4, 7, 8, 6] and s == sorted(p.tolist(), reverse=True)       # equal p: the lower input index first


def test_reference_compensation_raises_the_factor_of_a_chain():
    """A - B - C in a row: B overlaps A and C, A and C are disjoint.  Without compensation C would be decayed by its overlap with B alone; B is
    itself suppressed by A (comp_B), so C's factor is divided by 1 - comp_B (linear) / its argument lowered by comp_B^2 (gaussian)."""
    chain = np.array([[0, 0, 10, 10], [5, 0, 15, 10], [10.5, 0, 20.5, 10]], dtype=np.float64)
    iou_ab, iou_bc = 50.0 / 150.0, 45.0 / 155.0
    keep, s, det = _run(chain, [0.9, 0.8, 0.7], "linear")
    assert det["comp"].tolist() == [0.0, iou_ab, iou_bc]
    want = min(1.0, (1.0 - iou_bc) / (1.0 - iou_ab))
    assert det["d"][2] == want and want > 1.0 - iou_bc                          # above the uncompensated factor
    assert det["d"][2] == 1.0                                                   # here even to 1: B is suppressed harder than it suppresses C
    keep, s, det = _run(chain, [0.9, 0.8, 0.7], "gaussian")
    assert det["arg"][2] == max(0.0, iou_bc * iou_bc - iou_ab * iou_ab) == 0.0 and det["d"][2] == 1.0 > np.exp(-(iou_bc * iou_bc) / 0.5)
    # a chain whose middle box is suppressed LESS than it suppresses: the factor still rises above the uncompensated one, but stays below 1
    chain2 = np.array([[0, 0, 10, 10], [8, 0, 18, 10], [10, 0, 20, 10]], dtype=np.float64)
    iou_ab, iou_bc = 20.0 / 180.0, 80.0 / 120.0
    _, _, det = _run(chain2, [0.9, 0.8, 0.7], "linear")
    assert det["d"][2] == (1.0 - iou_bc) / (1.0 - iou_ab) and 1.0 - iou_bc < det["d"][2] < 1.0
    _, _, det = _run(chain2, [0.9, 0.8, 0.7], "gaussian")
    assert det["arg"][2] == iou_bc * iou_bc - iou_ab * iou_ab and np.exp(-(iou_bc * iou_bc) / 0.5) < det["d"][2] < 1.0


def test_reference_admission_nan_and_zero_area():
    """An unadmitted candidate (below score_thresh, or NaN) is never emitted and decays nothing; a zero-area box has IoU 0 (or 0 / 0, which
    counts as 0) with everything."""
    keep, s, det = _run(PAIR, [np.nan, 0.8], "linear")
    assert keep == [1] and s == [0.8] and det["order"].tolist() == [1]
    assert _run(PAIR, [0.0005, 0.8], "linear")[:2] == ([1], [0.8])
    zero = np.array([[5, 5, 5, 9], [4, 4, 8, 16], [5, 5, 5, 9]], dtype=np.float64)
    for method in ref.METHODS:
        assert _run(zero, [0.95, 0.9, 0.5], method)[:2] == ([0, 1, 2], [0.95, 0.9, 0.5])
    assert _run(np.zeros((0, 4)), np.zeros(0), "gaussian")[:2] == ([], [])
    with pytest.raises(ValueError):
        ref.matrix_nms(PAIR, [0.9, 0.8], "softer")
    res = ref.matrix_nms_batched(np.concatenate([PAIR, PAIR]), [0.9, 0.8, 0.8, 0.9], [0, 2, 2, 4], method="linear", score="score")
    assert [r[0].tolist() for r in res] == [[0, 1], [], [3, 2]]


def test_reference_margins_by_hand():
    boxes = np.array([[0, 0, 10, 10], [0, 0, 10, 5], [50, 50, 60, 60], [70, 70, 80, 80]], dtype=np.float64)
    p = np.array([0.8, 0.5, 0.75, np.nan])
    keep, s, gap, dist = ref.matrix_nms(boxes, p, "linear", 0.5, 0.2, "score")
    assert keep.tolist() == [0, 2, 1] and s.tolist() == [0.8, 0.75, 0.25]
    assert gap == (0.8 - 0.75) / 0.8                                            # the closest neighbours, among the s and among the p
    assert dist == abs(0.25 - 0.2) / 0.2                                        # the closest value to the threshold: s_1 = 0.25
    assert ref.matrix_nms(boxes, p, "linear", 0.5, 0.0, "score")[3] == np.inf


# --------------------------------------------------------------------------- invariants on seeded clustered sets
def _planted_duplicates(seed, n=400):
    boxes, logits = vote_ref.clustered_boxes(n, seed=seed)
    rng = np.random.RandomState(1000 + seed)
    src, dst = rng.choice(n // 2, 30, replace=False), n // 2 + rng.choice(n // 2, 30, replace=False)
    boxes[dst] = boxes[src]
    return boxes, logits


@pytest.mark.parametrize("seed", range(20))
def test_reference_invariants(seed):
    boxes, logits = _planted_duplicates(seed)
    for method in ref.METHODS:
        keep, s, _, _, det = ref.matrix_nms(boxes, logits, method, 0.5, 0.001, details=True)
        d = det["d"]
        assert not np.isnan(d).any() and (d >= 0).all() and (d <= 1).all() and d[0] == 1.0
        assert (det["comp"] >= 0).all() and (det["comp"] <= 1).all() and (det["comp"] == 1.0).sum() >= 30      # the planted duplicates
        assert (np.diff(s) <= 0).all() and len(set(keep.tolist())) == len(keep)
        assert (s <= det["p"][det["rows"]]).all()                               # a score only ever falls
    # the one-exp form is SOLOv2's minimum of exponentials, bit for bit
    assert np.array_equal(d, ref.decay_by_min_of_exponentials(boxes[det["order"]], det["comp"], 0.5))
    assert (det["arg"] >= 0).all()                                              # rank 0 contributes iou^2


# --------------------------------------------------------------------------- the binding
def test_signatures_defaults_and_constants(hip):
    from tinyfaces import ops
    p = inspect.signature(ops.matrix_nms).parameters
    assert list(p) == ["boxes", "scores", "method", "sigma", "score_threshold", "score", "max_keep"]
    assert [p[k].default for k in list(p)[2:]] == ["gaussian", 0.5, 0.001, "sigmoid", None]
    p = inspect.signature(ops.matrix_nms_batched).parameters
    assert list(p) == ["boxes", "scores", "seg_offsets", "method", "sigma", "score_threshold", "score", "max_keep", "vote"]
    assert [p[k].default for k in list(p)[3:]] == ["gaussian", 0.5, 0.001, "sigmoid", None, None]
    src = open(os.path.join(ROOT, "include", "tinyfaces_hip.h")).read()
    defs = dict(re.findall(r"#define (TF_MATRIX_NMS_[A-Z_]+)\s+(\d+)", src))
    assert ops.MATRIX_NMS_METHODS == {"linear": int(defs["TF_MATRIX_NMS_LINEAR"]), "gaussian": int(defs["TF_MATRIX_NMS_GAUSSIAN"])} == {"linear": 1, "gaussian": 2}
    assert int(defs["TF_MATRIX_NMS_MAX_BOXES"]) == ops.MATRIX_NMS_MAX_BOXES >= ops.SOFT_NMS_MAX_BOXES
    assert ops.SOFT_NMS_METHODS == {"linear": 1, "gaussian": 2}                 # Soft-NMS's own table stays what it was
    assert {"tf_matrix_nms_f64", "tf_matrix_nms_f64_batched", "tf_matrix_nms_workspace_bytes", "tf_matrix_nms_batched_workspace_bytes"} <= set(hip.symbols())
    assert hip.lib().tf_version() >= 810
    # the kernels' tile sizes the GPU cases are built around
    k = open(os.path.join(ROOT, "tiny-faces-pytorch_amd", "csrc", "matrix_nms.hip")).read()
    assert f"kRows = {mc.ROWS};" in k and f"kTile = {mc.TILE};" in k and f"tile[{mc.RANK_TILE}]" in k and f"nmax >= {mc.WIDE}" in k
    assert f"kRankBoxes = {mc.RANK_BOXES} * Q" in k
    for t in (mc.ROWS, mc.TILE, mc.RANK_BOXES, mc.RANK_TILE):
        assert {t - 1, t, t + 1, 2 * t + 1} <= set(mc.SIZES), t
    assert {f"n{mc.WIDE - 1}_sparse", f"n{mc.WIDE}_sparse"} <= set(mc.cases())


def test_evaluate_model_parser():
    import evaluate_model
    a = evaluate_model.matrix_nms_arguments(["DATA"])
    assert (a.soft_nms, a.soft_nms_sigma, a.soft_nms_score_thresh, a.pre_nms_topk, a.max_detections, a.ap) == (None, 0.5, 0.001, None, None, False)
    a = evaluate_model.matrix_nms_arguments(["DATA", "--soft-nms", "matrix-gaussian", "--soft-nms-sigma", "0.25", "--soft-nms-score-thresh", "0.01",
                                             "--flip", "--box-voting", "0.5", "--ema", "--num-images", "1", "--max-detections", "750",
                                             "--pre-nms-topk", "5000"])
    assert (a.soft_nms, a.soft_nms_sigma, a.soft_nms_score_thresh) == ("matrix_gaussian", 0.25, 0.01)
    assert a.flip is True and a.box_voting == 0.5 and a.ema is True and a.num_images == 1 and a.dataset == "DATA"
    assert (a.max_detections, a.pre_nms_topk) == (750, 5000)
    assert evaluate_model.matrix_nms_arguments(["--soft-nms=matrix-linear", "DATA"]).soft_nms == "matrix_linear"
    for old in ("linear", "gaussian"):                                          # the Soft-NMS choices pass through unchanged
        assert evaluate_model.matrix_nms_arguments(["DATA", "--soft-nms", old]).soft_nms == old
    for bad in (["--soft-nms", "foo"], ["--soft-nms"], ["--soft-nms", "matrix"], ["--soft-nms", "matrix_linear"], ["--soft-nms-sigma", "0"]):
        with pytest.raises(SystemExit):
            evaluate_model.matrix_nms_arguments(["DATA"] + bad)
    # the older parsers keep their choices and their results
    for parse in (evaluate_model.soft_nms_arguments, evaluate_model.limits_arguments):
        for new in ("matrix-linear", "matrix-gaussian"):
            with pytest.raises(SystemExit):
                parse(["DATA", "--soft-nms", new])
        assert parse(["DATA", "--soft-nms", "gaussian"]).soft_nms == "gaussian" and parse(["DATA"]).soft_nms is None
    for parse in (evaluate_model.arguments, evaluate_model.ema_arguments, evaluate_model.tta_arguments):
        with pytest.raises(SystemExit):
            parse(["DATA", "--soft-nms", "matrix-linear"])
    assert "matrix_nms_arguments()" in inspect.getsource(evaluate_model.main)


def test_host_refusals_need_no_device():
    from tinyfaces import evaluation, ops
    boxes, scores = torch.zeros(3, 4, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.matrix_nms(boxes, scores)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.matrix_nms_batched(boxes, scores, [0, 3], "linear")
    for kw in (dict(method="softer"), dict(method="matrix_linear"), dict(score="softmax"), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")),
               dict(score_threshold=-1e-9), dict(score_threshold=float("nan")), dict(max_keep=0), dict(max_keep=-1), dict(max_keep=2.5),
               dict(max_keep=True), dict(vote=(0.0, "sigmoid")), dict(vote=(0.5, "softmax"))):
        with pytest.raises(ValueError):                                         # before the device is asked for: these are CPU tensors
            ops.matrix_nms_batched(boxes, scores, [0, 3], **kw)
    assert ops._matrix_nms_mode("gaussian", 0.5, 0.0, "score", None) == (2, 0.5, 0.0, 1, 0)
    assert ops._matrix_nms_mode("linear", 2, 0.3, "sigmoid", 750) == (1, 2.0, 0.3, 0, 750)
    for kw in (dict(soft_nms="foo"), dict(soft_nms="matrix"), dict(soft_nms="matrix_linear", soft_nms_sigma=0.0),
               dict(soft_nms="matrix_gaussian", soft_nms_score_thresh=-1.0), dict(soft_nms="matrix_gaussian", max_detections=0)):
        with pytest.raises(ValueError):
            evaluation.get_detections(None, None, None, None, None, device="cuda", **kw)
        with pytest.raises(ValueError):
            evaluation.get_detections_batch(None, [None], None, None, None, device="cuda", **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        evaluation.get_detections(None, None, None, None, None, device="cpu", soft_nms="matrix_linear")
    # nms_thresh plays no part in the matrix methods: a value Soft-NMS's linear method refuses is not looked at
    evaluation._check_soft_nms("matrix_linear", 7.0, 0.5, 0.001)
    with pytest.raises(ValueError):
        evaluation._check_soft_nms("linear", 7.0, 0.5, 0.001)
    # no keyword was added: the tails of the signatures are what they were
    import evaluate_model
    for fn in (evaluation.get_detections, evaluation.get_detections_batch, evaluate_model.run):
        assert list(inspect.signature(fn).parameters)[-3:] == ["soft_nms", "soft_nms_sigma", "soft_nms_score_thresh"]


def test_entry_points_check_their_arguments_without_launching(hip):
    """Host-side refusals of the entry points (nothing is enqueued; runs without a GPU)."""
    l = hip.lib()
    ERR_ARG, ERR_UNSUPPORTED, ERR_WORKSPACE = -1, -3, -4
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    off = (C.c_int32 * 3)(0, 2, 4)
    good = dict(method=1, sigma=0.5, sthr=0.001, mode=0, cap=0)

    def call(boxes=p, scores=p, offs=off, S=2, keep=p, score_out=p, num_keep=p, ws=p, wsb=1 << 20, **kw):
        a = {**good, **kw}
        return l.tf_matrix_nms_f64_batched(boxes, scores, offs, S, a["method"], a["sigma"], a["sthr"], a["mode"], a["cap"], keep, score_out,
                                           num_keep, ws, wsb, None)

    for method in (0, 3, -1):
        assert call(method=method) == ERR_ARG
    for mode in (2, -1):
        assert call(mode=mode) == ERR_ARG
    for sigma in (0.0, -0.5, float("nan")):
        assert call(sigma=sigma) == ERR_ARG
    for sthr in (-1e-300, float("nan")):
        assert call(sthr=sthr) == ERR_ARG
    assert call(cap=-1) == ERR_ARG
    assert call(S=0) == ERR_ARG and call(S=65) == ERR_ARG and call(offs=None) == ERR_ARG
    assert call(offs=(C.c_int32 * 3)(0, 4, 2)) == ERR_ARG and call(offs=(C.c_int32 * 3)(1, 2, 4)) == ERR_ARG
    assert call(num_keep=None) == ERR_ARG
    assert call(boxes=None) == ERR_ARG and call(scores=None) == ERR_ARG and call(keep=None) == ERR_ARG and call(score_out=None) == ERR_ARG
    assert call(ws=None) == ERR_WORKSPACE and call(wsb=8) == ERR_WORKSPACE
    from tinyfaces import ops
    assert call(offs=(C.c_int32 * 2)(0, ops.MATRIX_NMS_MAX_BOXES + 1), S=1, wsb=1 << 40) == ERR_UNSUPPORTED
    # n == 0: nothing to do, nothing needed
    assert call(boxes=None, scores=None, offs=(C.c_int32 * 3)(0, 0, 0), keep=None, score_out=None, ws=None, wsb=0, method=2, mode=1) == 0
    assert l.tf_matrix_nms_f64(p, p, -1, 1, 0.5, 0.001, 0, 0, p, p, p, p, 1 << 20, None) == ERR_ARG
    assert l.tf_matrix_nms_f64(p, p, 4, 7, 0.5, 0.001, 0, 0, p, p, p, p, 1 << 20, None) == ERR_ARG
    assert l.tf_matrix_nms_f64(None, None, 0, 1, 0.5, 0.0, 0, 0, None, None, p, None, 0, None) == 0
    # the workspace is linear in n -- no n^2 / 8 adjacency bits
    assert l.tf_matrix_nms_workspace_bytes(0) == 0 and l.tf_matrix_nms_workspace_bytes(-3) == 0
    sizes = [l.tf_matrix_nms_workspace_bytes(n) for n in (1, 64, 65, 4097, 65536, ops.MATRIX_NMS_MAX_BOXES)]
    assert sizes[0] > 0 and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert 68 * 65536 <= sizes[4] <= 68 * 65536 + 6 * 256 and sizes[4] * 100 < l.tf_soft_nms_workspace_bytes(65536)
    assert l.tf_matrix_nms_batched_workspace_bytes((C.c_int32 * 3)(0, 0, 0), 2) == 0


# --------------------------------------------------------------------------- the condition on the GPU cases
@pytest.mark.parametrize("name", list(mc.cases()))
def test_gpu_cases_are_far_from_every_decision(name):
    """Both margins of every case of tests/test_gpu_matrix_nms.py are above 1e-9 (score_bound(1) is 5e-15: a last-bit difference of the
    device's exp cannot reorder two scores or cross the threshold), and bit-equal neighbouring emitted scores come from bit-equal
    (p, argument) pairs -- the device, which computes the same argument bits, then ties the same rows."""
    for method, score in (("linear", "score"), ("gaussian", "sigmoid"), ("linear", "sigmoid")):
        for keep, s, gap, dist, det in mc.reference(name, method, score):
            assert gap > mc.MARGIN and dist > mc.MARGIN, (method, score, gap, dist)
            rows = det["rows"]
            tied = np.nonzero(s[:-1] == s[1:])[0]
            for r in tied:
                a, b = rows[r], rows[r + 1]
                assert a < b and det["p"][a] == det["p"][b] and det["arg"][a] == det["arg"][b], (method, score, int(r))
