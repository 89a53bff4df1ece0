"""CPU: the host side of the device WIDER evaluator (csrc/wider_eval.hip, ops.wider_*, wider_eval.DeviceEvaluator): the new symbols, the
refusals that fire without a device, ops.wider_rows against the result-file round trip, the numpy restatement of the parallel form
(tests/wider_ref.py) against image_evaluation, the factored precision / recall / AP lines, and the command-line flags.  The kernels run in
tests/test_gpu_wider_eval.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import wider_ref
from tinyfaces import wider_eval as we

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------- the surface
def test_symbols_and_version(hip):
    new = {"tf_wider_match_workspace_bytes", "tf_wider_match_f64_batched", "tf_wider_pr_accumulate"}
    assert new <= set(hip._SIGNATURES) and new <= set(hip.symbols())
    header = open(os.path.join(ROOT, "include", "tinyfaces_hip.h")).read()
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, re.sub(r"/\*.*?\*/", "", header, flags=re.S)), name
    assert hip.lib().tf_version() >= 740
    from tinyfaces import ops
    assert int(re.search(r"#define\s+TF_WIDER_GT_TILE\s+(\d+)", header).group(1)) == ops.WIDER_GT_TILE


def test_entry_points_check_their_arguments_without_launching(hip):
    l = hip.lib()
    ERR_ARG = -1
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    off = lambda *v: (C.c_int32 * len(v))(*v)      # noqa: E731

    def match(rows=p, doff=off(0, 2, 3), gt=p, goff=off(0, 1, 2), S=2, keep=p, nset=1, thr=0.5, counted=p, recalled=p, ws=p, wsb=1 << 20):
        return l.tf_wider_match_f64_batched(rows, doff, gt, goff, S, keep, nset, thr, counted, recalled, ws, wsb, None)

    assert match(nset=0) == ERR_ARG and match(nset=-1) == ERR_ARG and match(thr=float("nan")) == ERR_ARG
    assert match(S=0) == ERR_ARG and match(S=-2) == ERR_ARG
    assert match(doff=None) == ERR_ARG and match(goff=None) == ERR_ARG
    assert match(doff=off(0, 3, 2)) == ERR_ARG and match(doff=off(1, 2, 3)) == ERR_ARG and match(doff=off(0, -1, 3)) == ERR_ARG
    assert match(goff=off(0, 2, 1)) == ERR_ARG and match(goff=off(1, 1, 2)) == ERR_ARG
    assert match(rows=None) == ERR_ARG and match(counted=None) == ERR_ARG and match(recalled=None) == ERR_ARG
    assert match(gt=None) == ERR_ARG and match(keep=None) == ERR_ARG
    assert match(ws=None) == ERR_ARG and match(wsb=8) == ERR_ARG
    # no detection: nothing is launched, whatever the other operands
    assert match(rows=None, doff=off(0, 0, 0), gt=None, keep=None, counted=None, recalled=None, ws=None, wsb=0) == 0
    assert l.tf_wider_match_workspace_bytes(0, 5) == 0 and l.tf_wider_match_workspace_bytes(-1, 5) == 0
    sizes = [l.tf_wider_match_workspace_bytes(n, g) for n, g in ((1, 0), (1, 1), (750, 2000), (3226 * 750, 40000))]
    assert sizes[0] >= 4 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[2] >= 4 * (750 + 2000)

    def pr(scores=p, doff=off(0, 2, 3), S=2, counted=p, recalled=p, nset=1, lo_d=p, thresh=p, T=7, table=p):
        return l.tf_wider_pr_accumulate(scores, doff, S, counted, recalled, nset, lo_d, thresh, T, table, None)

    assert pr(nset=0) == ERR_ARG and pr(T=-1) == ERR_ARG and pr(S=0) == ERR_ARG
    assert pr(doff=None) == ERR_ARG and pr(doff=off(0, 3, 2)) == ERR_ARG and pr(doff=off(2, 2, 3)) == ERR_ARG
    for name in ("scores", "counted", "recalled", "lo_d", "thresh", "table"):
        assert pr(**{name: None}) == ERR_ARG, name
    assert pr(scores=None, doff=off(0, 0, 0), counted=None, recalled=None, lo_d=None, thresh=None, table=None) == 0
    assert pr(T=0, thresh=None, table=None) == 0


def test_ops_refuse_on_the_host_and_have_no_cpu_fallback():
    from tinyfaces import ops
    rows, gt = torch.zeros(5, 5, dtype=torch.float64), torch.zeros(3, 4, dtype=torch.float64)
    keep = torch.ones(2, 3, dtype=torch.uint8)
    good = dict(rows=rows, det_offsets=[0, 2, 5], gt=gt, gt_offsets=[0, 3, 3], keep_masks=keep)
    for bad in (dict(det_offsets=[0, 6]), dict(det_offsets=[1, 2, 5]), dict(det_offsets=[0, 4, 2, 5]), dict(det_offsets=[0, 5]),
                dict(gt_offsets=[0, 2, 4]), dict(gt_offsets=[0]), dict(keep_masks=torch.ones(2, 4, dtype=torch.uint8)),
                dict(keep_masks=torch.ones(0, 3, dtype=torch.uint8)), dict(rows=torch.zeros(5, 4, dtype=torch.float64)),
                dict(gt=torch.zeros(3, 5, dtype=torch.float64)), dict(iou_thresh=float("nan"))):
        with pytest.raises(ValueError):
            ops.wider_match_batched(**{**good, **bad})
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # good arguments: the only thing missing is the device
        ops.wider_match_batched(**good)
    s = torch.zeros(5, dtype=torch.float64)
    cr = torch.zeros(2, 5, dtype=torch.int32)
    good = dict(scores=s, det_offsets=[0, 2, 5], counted=cr, recalled=cr, lo_d=torch.tensor([0.0, 1.0], dtype=torch.float64),
                thresh=torch.zeros(7, dtype=torch.float64), pr=torch.zeros(2, 7, 2, dtype=torch.int64))
    for bad in (dict(det_offsets=[0, 4]), dict(counted=torch.zeros(2, 4, dtype=torch.int32)), dict(counted=cr.long()),
                dict(recalled=torch.zeros(1, 5, dtype=torch.int32)), dict(lo_d=torch.zeros(2)), dict(thresh=torch.zeros(7)),
                dict(pr=torch.zeros(2, 7, 2, dtype=torch.int32)), dict(pr=torch.zeros(2, 8, 2, dtype=torch.int64))):
        with pytest.raises(ValueError):
            ops.wider_pr_accumulate(**{**good, **bad})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.wider_pr_accumulate(**good)
    with pytest.raises(ValueError):
        we.DeviceEvaluator((), device="cpu")
    with pytest.raises(ValueError):
        we.DeviceEvaluator(("all",), thresh_num=0, device="cpu")
    ev = we.DeviceEvaluator(("all",), device="cpu")
    with pytest.raises(ValueError):
        ev.add([np.zeros((0, 5))], [np.zeros((1, 4))], [[[0]], [[0]]])    # two settings' lists for one setting
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.add([np.array([[0.0, 0.0, 9.0, 9.0, 0.5]])], [np.array([[0.0, 0.0, 9.0, 9.0]])], [[[0]]])


# --------------------------------------------------------------------------- the in-memory path sees what the file path reads
def test_wider_rows_is_the_result_file_round_trip(tmp_path):
    from tinyfaces import ops
    from tinyfaces.evaluation import write_results
    rng = np.random.RandomState(5)
    xy = rng.randint(0, 400, (40, 2)) + rng.choice([0.0, 0.5, 0.25, -0.5], (40, 2))          # .5 geometry: half to even, both parities
    wh = rng.randint(1, 90, (40, 2)) + rng.choice([0.0, 0.5, 1.5, 0.49999999999], (40, 2))
    dets = np.column_stack([xy, xy + wh, rng.choice([0.125, 0.3, 0.7000000000000001, 1e-9, 0.9999999999999999], 40)])
    dets[3, :2] = [-0.3, -0.5]                                             # rounds to -0.0: the file says "0"
    dets[7:10, 4] = 0.3                                                    # repeated scores: the stable order is the input order
    write_results(dets, "ev/img.jpg", "val", results_dir=tmp_path)
    back = we.read_predictions(str(tmp_path))["ev"]["img"]
    rows = ops.wider_rows(dets)
    assert rows.dtype == np.float64 and rows.shape == (40, 5)
    mine = rows[np.argsort(-rows[:, 4], kind="stable")]                    # the evaluator's input order (read_predictions')
    assert np.array_equal(mine, back) and mine.tobytes() == back.tobytes()   # bit for bit, the sign of zero included
    t = ops.wider_rows(torch.from_numpy(dets))
    assert t.dtype == torch.float64 and t.numpy().tobytes() == rows.tobytes()
    # the device evaluator orders with torch's stable descending sort: the same permutation
    order = torch.sort(t[:, 4], descending=True, stable=True).indices.numpy()
    assert np.array_equal(order, np.argsort(-rows[:, 4], kind="stable"))
    assert ops.wider_rows(np.zeros((0, 5))).shape == (0, 5)


# --------------------------------------------------------------------------- the parallel form is the sequential one
def test_parallel_restatement_equals_image_evaluation():
    rng = np.random.RandomState(11)
    total = dups = ties = ignored = 0
    for i in range(300):
        N, G = int(rng.randint(0, 80)), int(rng.randint(1, 25))
        rows, gt, keep = wider_ref.random_image(rng, N, G, nset=2)
        total += N
        dups += int(len({tuple(b) for b in gt}) < G)
        ties += int(np.unique(rows[:, 4]).size < N)
        ignored += int((~keep).any())
        for k in range(2):
            pred_recall, proposal = we.image_evaluation(rows, gt, keep[k])
            counted, recalled, prop = wider_ref.parallel_evaluation(rows, gt, keep[k])
            assert np.array_equal(prop, proposal) and np.array_equal(recalled, pred_recall), i
            assert np.array_equal(counted, np.cumsum(proposal == 1))
    assert total > 8000 and dups > 100 and ties > 100 and ignored > 100    # the cases the restatement has to survive did occur
    rows, gt, keep = wider_ref.half_iou_image()
    best = wider_ref.best_match(rows, gt)
    assert best.tolist() == [0, 1, 2, 0, 2, -1, 0, -1]                     # exactly 0.5 is a match; the duplicate's lower index wins; touching boxes do not overlap
    g = gt.copy(); g[:, 2:] += g[:, :2]
    assert we.box_overlap(g, np.array([0.0, 0.0, 9.0, 4.0]))[0] == 0.5 and we.box_overlap(g, np.array([100.0, 100.0, 109.0, 109.0]))[1] == 0.5
    for k in range(3):
        pred_recall, proposal = we.image_evaluation(rows, gt, keep[k])
        counted, recalled, prop = wider_ref.parallel_evaluation(rows, gt, keep[k])
        assert np.array_equal(prop, proposal) and np.array_equal(recalled, pred_recall)
    assert we.image_evaluation(rows, gt, keep[0])[0].tolist() == [1, 2, 3, 3, 3, 3, 3, 3]
    assert we.image_evaluation(rows, gt, keep[1])[1].tolist() == [1, -1, 1, 1, 1, 1, 1, 1]


# --------------------------------------------------------------------------- one tail for both paths
def test_factored_tail_reproduces_evaluate_setting_on_the_hand_cases():
    gt = {"e": {"a": np.array([[10, 10, 20, 20], [100, 100, 30, 30.0]])}}
    keep = {"e": {"a": np.array([0, 1])}}
    perfect = {"e": {"a": np.array([[10, 10, 20, 20, 1.0], [100, 100, 30, 30, 0.5]])}}
    half = {"e": {"a": np.array([[10, 10, 20, 20, 1.0], [300, 300, 30, 30, 0.5]])}}
    keep_one = {"e": {"a": np.array([0])}}
    for preds, kp, want in ((perfect, keep, 1.0), (half, keep, 0.5), (perfect, keep_one, 1.0)):
        p = we.norm_scores(preds)
        ap, curve = we.evaluate_setting(p, gt, kp)
        assert abs(ap - want) < 1e-12
        # the table by hand: image_pr_info on the one image, then the factored lines
        mask = np.zeros(2, bool); mask[kp["e"]["a"]] = True
        pred_recall, proposal = we.image_evaluation(p["e"]["a"], gt["e"]["a"], mask)
        pr = we.image_pr_info(p["e"]["a"][:, 4], proposal, pred_recall)
        ap2, curve2 = we.precision_recall_ap(pr, len(kp["e"]["a"]))
        assert ap2 == ap and np.array_equal(curve2, curve)
        # ... and from the integer table a device would return
        ap3, curve3 = we.precision_recall_ap(pr.astype(np.int64).astype(np.float64), len(kp["e"]["a"]))
        assert ap3 == ap and np.array_equal(curve3, curve)
    ap, curve = we.precision_recall_ap(np.zeros((7, 2)), 0)
    assert ap == 0.0 and curve.shape == (7, 2) and not curve.any()
    # the integer table of the shared cases is image_pr_info's
    preds, gtb, keeps = wider_ref.synthetic_set(1, n_img=12, nset=2)
    normed = we.norm_scores(preds)
    for k in range(2):
        ap, curve = we.evaluate_setting(normed, gtb, keeps[k])
        pr = np.zeros((we.THRESH_NUM, 2))
        for name, g in gtb["ev"].items():
            p = normed["ev"][name]
            if g.shape[0] == 0 or p.shape[0] == 0:
                continue
            mask = np.zeros(g.shape[0], bool); mask[keeps[k]["ev"][name]] = True
            counted, recalled, prop = wider_ref.parallel_evaluation(p, g, mask)
            pr += we.image_pr_info(p[:, 4], prop, recalled)
        ap2, curve2 = we.precision_recall_ap(pr, sum(v.size for v in keeps[k]["ev"].values()))
        assert ap2 == ap and np.array_equal(curve2, curve)


# --------------------------------------------------------------------------- the command lines
def test_new_flags_default_to_off():
    import evaluate_model
    import main as train_main
    a = evaluate_model.limits_arguments(["DATA"])
    assert a.ap is False and a.gt_dir is None and a.pre_nms_topk is None and a.soft_nms is None and a.flip is False
    a = evaluate_model.limits_arguments(["DATA", "--ap", "--gt-dir", "GT", "--max-detections", "750", "--num-images", "2"])
    assert a.ap is True and a.gt_dir == "GT" and a.max_detections == 750 and a.num_images == 2 and a.dataset == "DATA"
    for parse in (evaluate_model.arguments, evaluate_model.soft_nms_arguments):        # the older parsers keep their results and refuse the new flags
        assert "ap" not in vars(parse(["DATA"])) and "gt_dir" not in vars(parse(["DATA"]))
        with pytest.raises(SystemExit):
            parse(["DATA", "--ap"])
    t = train_main.trunk_arguments(["TRAIN", "VAL"])
    assert t.val_every == 0 and t.val_gt_dir is None and t.val_num_images is None and t.valdata == "VAL" and t.model_ema is None
    assert (t.val_prob_thresh, t.val_nms_thresh) == (0.03, 0.3)                        # evaluate_model.py's defaults
    t = train_main.trunk_arguments(["TRAIN", "VAL", "--val-every", "2", "--val-prob-thresh", "0.1", "--val-nms-thresh", "0.4", "--val-num-images", "8",
                                    "--val-gt-dir", "GT", "--model-ema", "0.999", "--epochs", "3"])
    assert (t.val_every, t.val_prob_thresh, t.val_nms_thresh, t.val_num_images, t.val_gt_dir) == (2, 0.1, 0.4, 8, "GT")
    assert t.model_ema == 0.999 and t.epochs == 3
    for bad in (["--val-every", "-1"], ["--val-every", "1.5"], ["--val-num-images", "0"], ["--val-prob-thresh", "1.5"], ["--val-nms-thresh", "-0.1"]):
        with pytest.raises(SystemExit):
            train_main.trunk_arguments(["TRAIN", "VAL"] + bad)
    assert "val_every" not in vars(train_main.arguments(["TRAIN", "VAL"]))             # arguments() keeps resolving the reference's options
    with pytest.raises(SystemExit):
        train_main.arguments(["TRAIN", "VAL", "--val-every", "1"])


def test_ap_is_refused_under_several_ranks(monkeypatch):
    import evaluate_model
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="--ap"):
        evaluate_model.check_ap(evaluate_model.limits_arguments(["synthetic-faces", "--ap"]))
    evaluate_model.check_ap(evaluate_model.limits_arguments(["synthetic-faces"]))      # without --ap several ranks are fine
    monkeypatch.setenv("WORLD_SIZE", "1")
    evaluate_model.check_ap(evaluate_model.limits_arguments(["synthetic-faces", "--ap"]))
    with pytest.raises(SystemExit, match="--gt-dir"):                                  # a WIDER annotation file needs the ground-truth directory
        evaluate_model.check_ap(evaluate_model.limits_arguments(["wider_val.txt", "--ap"]))
