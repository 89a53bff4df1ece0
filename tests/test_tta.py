"""CPU: the host side of the test-time augmentation (horizontal flip + box voting): the new keywords and their defaults, evaluate_model.py's
flags parsed apart from the reference's options, the refusal of CPU tensors, the new C entry points' argument checks, and the numpy
restatement (tests/vote_ref.py) on three hand-computed cases.  The kernels run in tests/test_gpu_tta.py."""
import inspect

import numpy as np
import pytest
import torch

import vote_ref


def test_keywords_exist_with_their_defaults():
    import evaluate_model
    from tinyfaces import evaluation, ops
    for fn in (evaluation.get_detections, evaluation.get_detections_batch, evaluate_model.run):
        p = inspect.signature(fn).parameters
        assert p["flip"].default is False and p["box_voting"].default is None, fn.__name__
    p = inspect.signature(ops.box_voting).parameters
    assert list(p) == ["boxes", "scores", "keep", "vote_thresh", "weight", "num_keep", "return_votes"]
    assert (p["weight"].default, p["num_keep"].default, p["return_votes"].default) == ("sigmoid", None, False)
    p = inspect.signature(ops.box_voting_batched).parameters
    assert list(p)[:5] == ["boxes", "scores", "seg_offsets", "keeps", "vote_thresh"] and p["weight"].default == "sigmoid"
    assert list(inspect.signature(ops.boxes_unflip_).parameters) == ["dets", "first", "last", "max_rows", "c"]
    assert ops.VOTE_WEIGHTS == {"sigmoid": 0, "score": 1}            # TF_VOTE_WEIGHT_* of include/tinyfaces_hip.h


def test_evaluate_model_flags_are_parsed_apart():
    import evaluate_model
    a = evaluate_model.tta_arguments(["DATA"])
    assert a.flip is False and a.box_voting is None and a.ema is False
    a = evaluate_model.tta_arguments(["DATA", "--flip", "--box-voting", "0.5", "--ema", "--num-images", "1"])
    assert a.flip is True and a.box_voting == 0.5 and a.ema is True and a.num_images == 1 and a.dataset == "DATA"
    a = evaluate_model.tta_arguments(["--box-voting=0.25", "DATA", "--prob_thresh", "0.1"])
    assert a.flip is False and a.box_voting == 0.25 and a.prob_thresh == 0.1
    # the two older parsers keep their results and keep refusing the new flags
    assert "flip" not in vars(evaluate_model.arguments(["DATA"])) and "box_voting" not in vars(evaluate_model.arguments(["DATA"]))
    assert "flip" not in vars(evaluate_model.ema_arguments(["DATA", "--ema"]))
    for parse in (evaluate_model.arguments, evaluate_model.ema_arguments):
        for argv in (["--flip"], ["--box-voting", "0.5"]):
            with pytest.raises(SystemExit):
                parse(["DATA"] + argv)
    for bad in ("0", "1.5", "-0.1", "nan", "abc"):
        with pytest.raises(SystemExit):
            evaluate_model.tta_arguments(["DATA", "--box-voting", bad])


def test_cpu_tensors_raise():
    from tinyfaces import ops
    boxes, scores = torch.zeros(3, 4, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    keep = torch.zeros(1, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.box_voting(boxes, scores, keep, 0.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.box_voting_batched(boxes, scores, [0, 3], [keep], 0.5)
    one = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.boxes_unflip_(torch.zeros(3, 5, dtype=torch.float64), one, one, 3, 10.0)


def test_entry_points_check_their_arguments_without_launching(hip):
    """Host-side refusals of the three entry points (nothing is enqueued; runs without a GPU)."""
    import ctypes as C
    l = hip.lib()
    ERR_ARG = -1
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    off = (C.c_int32 * 3)(0, 2, 4)
    assert {"tf_box_vote_f64", "tf_box_vote_f64_batched", "tf_boxes_unflip_f64"} <= set(hip.symbols())
    assert l.tf_version() >= 660
    assert l.tf_box_vote_f64_batched(p, p, off, 0, p, p, 0.5, 0, p, None, None) == ERR_ARG                # S = 0
    assert l.tf_box_vote_f64_batched(p, p, off, 65, p, p, 0.5, 0, p, None, None) == ERR_ARG               # S > TF_NMS_MAX_SEGMENTS
    assert l.tf_box_vote_f64_batched(p, p, None, 2, p, p, 0.5, 0, p, None, None) == ERR_ARG
    assert l.tf_box_vote_f64_batched(p, p, off, 2, p, None, 0.5, 0, p, None, None) == ERR_ARG             # no counts
    assert l.tf_box_vote_f64_batched(p, p, (C.c_int32 * 3)(0, 4, 2), 2, p, p, 0.5, 0, p, None, None) == ERR_ARG      # descending offsets
    assert l.tf_box_vote_f64_batched(p, p, (C.c_int32 * 3)(1, 2, 4), 2, p, p, 0.5, 0, p, None, None) == ERR_ARG      # offsets start at 0
    assert l.tf_box_vote_f64_batched(p, p, off, 2, p, p, 0.5, 2, p, None, None) == ERR_ARG                # unknown weight mode
    for t in (0.0, -0.5, 1.0 + 2.0 ** -52, float("nan")):
        assert l.tf_box_vote_f64_batched(p, p, off, 2, p, p, t, 0, p, None, None) == ERR_ARG
    for args in ((None, p, off, 2, p, p), (p, None, off, 2, p, p), (p, p, off, 2, None, p)):
        assert l.tf_box_vote_f64_batched(*args, 0.5, 0, p, None, None) == ERR_ARG
    assert l.tf_box_vote_f64_batched(p, p, off, 2, p, p, 0.5, 0, None, None, None) == ERR_ARG             # no output
    assert l.tf_box_vote_f64_batched(None, None, (C.c_int32 * 3)(0, 0, 0), 2, None, p, 0.5, 1, None, None, None) == 0      # n == 0: nothing to do
    assert l.tf_box_vote_f64(p, p, -1, p, p, 0.5, 0, p, None, None) == ERR_ARG
    assert l.tf_box_vote_f64(None, None, 0, None, p, 1.0, 0, None, None, None) == 0
    assert l.tf_boxes_unflip_f64(None, p, p, 4, 1.0, None) == ERR_ARG
    assert l.tf_boxes_unflip_f64(p, None, p, 4, 1.0, None) == ERR_ARG
    assert l.tf_boxes_unflip_f64(p, p, None, 4, 1.0, None) == ERR_ARG
    assert l.tf_boxes_unflip_f64(p, p, p, -1, 1.0, None) == ERR_ARG
    assert l.tf_boxes_unflip_f64(p, p, p, 0, 1.0, None) == 0                                               # no rows: no launch


def test_reference_vote_at_the_threshold_is_a_vote():
    """[0,0,2,1] and [0,0,1,1]: inter 1, areas 2 and 1, IoU = 1 / (2 + 1 - 1) = 0.5 exactly.  `>=`: at 0.5 they vote for each other, at the next
    double above 0.5 they do not.  weight='score' with scores 3 and 1: the mean of the first row is (3 * [0,0,2,1] + 1 * [0,0,1,1]) / 4."""
    boxes = np.array([[0, 0, 2, 1], [0, 0, 1, 1]], dtype=np.float64)
    scores = np.array([3.0, 1.0])
    assert vote_ref.iou_one_to_many(boxes[0], boxes)[1] == 0.5
    out, votes = vote_ref.box_voting(boxes, scores, [0, 1], 0.5, weight="score")
    assert votes.tolist() == [2, 2]
    assert np.array_equal(out, [[0, 0, 1.75, 1, 3.0], [0, 0, 1.75, 1, 1.0]])
    out, votes = vote_ref.box_voting(boxes, scores, [0, 1], 0.5 + 2.0 ** -53, weight="score")
    assert votes.tolist() == [1, 1]
    assert np.array_equal(out, [[0, 0, 2, 1, 3.0], [0, 0, 1, 1, 1.0]])
    # sigmoid weights: w = 1 / (1 + e^-s); the same voter sets
    out, votes = vote_ref.box_voting(boxes, scores, [0], 0.5)
    w = 1.0 / (1.0 + np.exp(-scores))
    assert votes.tolist() == [2] and out[0, 2] == (w[0] * 2 + w[1] * 1) / (w[0] + w[1]) and out[0, 4] == 3.0


def test_reference_zero_area_kept_box_stays_with_no_votes():
    """A zero-area box: its IoU with itself is 0 / 0 = NaN and with anything else 0 -- nobody votes, the row is the box and its score."""
    boxes = np.array([[5, 5, 5, 9], [4, 4, 8, 16], [5, 5, 5, 9]], dtype=np.float64)
    scores = np.array([2.0, 1.0, 0.5])
    out, votes = vote_ref.box_voting(boxes, scores, [0, 1], 0.5)
    assert votes.tolist() == [0, 1]
    assert np.array_equal(out[0], [5, 5, 5, 9, 2.0])
    assert np.array_equal(out[1], [4, 4, 8, 16, 1.0])


def test_reference_score_weight_drops_non_positive_voters():
    """weight='score': three coincident boxes (IoU 1) with scores 2, 0 and -1 -- only the first votes; a kept box whose voters are all
    dropped stays unchanged with 0 votes; a NaN score is dropped as well."""
    boxes = np.array([[0, 0, 4, 4], [1, 0, 5, 4], [0, 0, 4, 4], [0, 0, 4, 4]], dtype=np.float64)
    boxes[1] = boxes[0]
    scores = np.array([2.0, 0.0, -1.0, np.nan])
    out, votes = vote_ref.box_voting(boxes, scores, [0, 1, 2], 0.5, weight="score")
    assert votes.tolist() == [1, 1, 1]
    assert np.array_equal(out[:, :4], boxes[:3]) and np.array_equal(out[:, 4], scores[:3])
    shifted = boxes.copy()
    shifted[0] = [2, 0, 6, 4]                                            # IoU with the others 1/3: below the threshold
    out, votes = vote_ref.box_voting(shifted, scores, [1, 0], 0.5, weight="score")
    assert votes.tolist() == [0, 1]                                      # box 1: its voters are boxes 1, 2, 3 (weights 0, -1, NaN) -> none
    assert np.array_equal(out[0], [0, 0, 4, 4, 0.0]) and np.array_equal(out[1], [2, 0, 6, 4, 2.0])


def test_reference_unflip():
    d = np.array([[-3.5, 1, 10.25, 7, 0.5], [100, 2, 140, 9, -1.0]])
    u = vote_ref.unflip(d, 199.0)
    assert np.array_equal(u, [[188.75, 1, 202.5, 7, 0.5], [59, 2, 99, 9, -1.0]])
    assert np.array_equal(vote_ref.unflip(u, 199.0), d)                  # (exact here: every value is a small dyadic number)


def test_generator_has_the_cases_it_promises():
    from oracle.nms import nms
    for n in (65, 257, 1025):
        boxes, scores = vote_ref.clustered_boxes(n, seed=n)
        assert boxes.min() < 0 and scores[0] == scores[3] and np.array_equal(boxes[7], boxes[5]) and boxes[11, 0] == boxes[11, 2]
        keep = nms(boxes, scores, 0.3)
        out, votes = vote_ref.box_voting(boxes, scores, keep, 0.5)
        r = int(np.nonzero(keep == 11)[0][0])                            # the zero-area box survives the NMS ...
        assert votes[r] == 0 and np.array_equal(out[r, :4], boxes[11])   # ... and nobody votes for it
        moved = (out[:, :4] != boxes[keep]).any(axis=1)
        assert moved.sum() >= len(keep) // 2                             # the vote does something on this input
        assert votes.max() > 4
