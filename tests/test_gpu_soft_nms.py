"""-m gpu: Soft-NMS (csrc/soft_nms.hip: tf_soft_nms_f64[_batched]; ops.soft_nms, ops.soft_nms_batched; get_detections / get_detections_batch /
evaluate_model.run with soft_nms=) against the numpy restatement tests/soft_nms_ref.py.

Bounds.  The kept indices must be EQUAL to the reference's: the IoU is evaluated bit for bit like numpy's, and the inputs are first shown (on the
CPU, by the reference's own margins) to be far from any decision a last-bit difference could change.  Scores: relative 8 * (K + 2) * 2^-52 for K
kept boxes (soft_nms_ref.score_bound: a score carries at most K factors, each with a couple of ulps of exp plus the multiply, on top of the
sigmoid).  With score="score" and the linear method only IEEE multiply, subtract and divide occur: bit-equal.  The batched form against single
calls, a second run, the guarded call against the plain one: bit-equal."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import soft_nms_ref
import vote_ref
from gpu_util import report
from redzone import assert_guards, assert_written, guarded, guarded_like, guarded_workspace, unwritten

pytestmark = pytest.mark.gpu

# one box, two, a wave edge (63 / 64 / 65), more than one bit-matrix word per row (130), more than one wave of word owners and a row of
# 17 / 33 / 65 words (1025 / 2049 / 4097: the last has more than 64 words, i.e. two waves of owners)
SIZES = [1, 2, 63, 64, 65, 130, 1025, 2049, 4097]
MARGIN = 1e-9


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C", copy=True))      # a copy: the cached inputs are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


@functools.lru_cache(maxsize=None)
def _inputs(n):
    boxes, logits = vote_ref.clustered_boxes(n, seed=n)
    boxes.setflags(write=False); logits.setflags(write=False)
    return boxes, logits


@functools.lru_cache(maxsize=None)
def _reference(n, method, score_thresh, score):
    boxes, logits = _inputs(n)
    scores = logits if score == "sigmoid" else vote_ref.weights(logits)
    res = soft_nms_ref.soft_nms(boxes, scores, method, 0.3, 0.5, score_thresh, score=score)
    for a in res[:2]:
        a.setflags(write=False)
    return res


def _rel(got, want):
    """Largest relative deviation of the scores (0 where both are 0)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.size == 0:
        return 0.0
    den = np.where(want != 0, np.abs(want), 1.0)
    return float((np.abs(got - want) / den).max())


# --------------------------------------------------------------------------- case 1: the kernels against the numpy restatement
@pytest.mark.parametrize("score_thresh", [0.001, 0.3])
@pytest.mark.parametrize("method", ["linear", "gaussian"])
@pytest.mark.parametrize("n", SIZES)
def test_soft_nms_kernel_vs_numpy(n, method, score_thresh):
    from tinyfaces import ops
    boxes, logits = _inputs(n)
    ref_keep, ref_scores, rank_margin, thresh_margin = _reference(n, method, score_thresh, "sigmoid")
    # a condition on the INPUTS: no selection and no liveness test of the reference run is within reach of a last-bit difference
    assert rank_margin >= MARGIN and thresh_margin >= MARGIN, (rank_margin, thresh_margin)
    keep, kept = ops.soft_nms(_dev(boxes), _dev(logits), method, 0.3, 0.5, score_thresh)
    assert keep.dtype == torch.int64 and kept.dtype == torch.float64 and keep.shape == kept.shape
    keep, kept = keep.cpu().numpy(), kept.cpu().numpy()
    K = len(ref_keep)
    bound = soft_nms_ref.score_bound(K)
    same = bool(np.array_equal(keep, ref_keep))
    dev = _rel(kept, ref_scores) if same else float("nan")
    report(f"soft_nms[n={n},{method},thr={score_thresh}]", kept=len(keep), ref_kept=K, keep_equal=same, score_maxrel=dev, score_bound=bound,
           rank_margin=rank_margin, thresh_margin=thresh_margin)
    print(f"soft_nms n={n} {method} score_thresh={score_thresh}: kept {len(keep)} (ref {K}) score_maxrel {dev:.3e} bound {bound:.3e} "
          f"margins {rank_margin:.3e} {thresh_margin:.3e}")
    assert same
    assert dev <= bound
    assert (np.diff(kept) <= 0).all()                                        # every factor is <= 1: the emitted scores never increase
    assert len(set(keep.tolist())) == len(keep) and (keep >= 0).all() and (keep < n).all()
    assert (kept >= score_thresh).all()


# --------------------------------------------------------------------------- case 2: exact mode
@pytest.mark.parametrize("score_thresh", [0.001, 0.3])
@pytest.mark.parametrize("n", SIZES)
def test_soft_nms_linear_on_probabilities_is_bit_exact(n, score_thresh):
    """score="score" fed the host's sigmoid, linear method: multiply, subtract and divide only -- the reference's bits, with the generator's
    tied scores (rows 0..3), exact duplicate (rows 5 and 7) and zero-area box (row 11) in the list."""
    from tinyfaces import ops
    boxes, logits = _inputs(n)
    probs = vote_ref.weights(logits)
    ref_keep, ref_scores, _, _ = _reference(n, "linear", score_thresh, "score")
    keep, kept = ops.soft_nms(_dev(boxes), _dev(probs), "linear", 0.3, 0.5, score_thresh, score="score")
    keep, kept = keep.cpu().numpy(), kept.cpu().numpy()
    report(f"soft_nms[n={n},linear,score,thr={score_thresh}]", kept=len(keep), keep_equal=bool(np.array_equal(keep, ref_keep)),
           scores_bit_equal=bool(np.array_equal(kept, ref_scores)))
    assert np.array_equal(keep, ref_keep)
    assert np.array_equal(kept, ref_scores)
    if n >= 16 and score_thresh == 0.001:
        r = int(np.nonzero(keep == 11)[0][0])                                # the zero-area box: never decayed
        assert kept[r] == probs[11]


# --------------------------------------------------------------------------- case 3: the hand-computed cases of tests/test_soft_nms.py
def _run(boxes, p, *args, **kw):
    from tinyfaces import ops
    keep, kept = ops.soft_nms(_dev(np.asarray(boxes, dtype=np.float64)), _dev(np.asarray(p, dtype=np.float64)), *args, **kw)
    return keep.cpu().numpy().tolist(), kept.cpu().numpy().tolist()


def test_soft_nms_hand_computed_cases():
    pair = np.array([[0, 0, 10, 10], [0, 0, 10, 5]], dtype=np.float64)       # IoU exactly 0.5
    p = [0.9, 0.8]
    # 1: 0.8 * (1 - 0.5) = 0.4 exactly; `>=` at score_thresh
    assert _run(pair, p, "linear", 0.3, 0.5, 0.4, score="score") == ([0, 1], [0.9, 0.4])
    assert _run(pair, p, "linear", 0.3, 0.5, float(np.nextafter(0.4, 1.0)), score="score") == ([0], [0.9])
    # 2: strict `>` at iou_thresh
    assert _run(pair, p, "linear", 0.5, 0.5, 0.001, score="score") == ([0, 1], [0.9, 0.8])
    assert _run(pair, p, "linear", float(np.nextafter(0.5, 0.0)), 0.5, 0.001, score="score") == ([0, 1], [0.9, 0.4])
    # 3: the re-ranking
    abc = np.array([[0, 0, 10, 10], [0, 0, 10, 8], [20, 20, 30, 30]], dtype=np.float64)
    assert _run(abc, [0.9, 0.8, 0.7], "linear", 0.3, 0.5, 0.001, score="score") == ([0, 2, 1], [0.9, 0.7, 0.8 * (1.0 - 0.8)])
    # 4: gaussian, IoU 0.5, sigma 0.5: exp(-0.5) (the device's exp: a couple of ulps)
    keep, kept = _run(pair, p, "gaussian", 0.9, 0.5, 0.001, score="score")
    assert keep == [0, 1] and kept[0] == 0.9 and abs(kept[1] - 0.8 * np.exp(-0.5)) <= soft_nms_ref.score_bound(2) * 0.8
    # 5: an exact duplicate with equal scores
    dup = np.array([[3, 4, 13, 24], [3, 4, 13, 24]], dtype=np.float64)
    assert _run(dup, [0.75, 0.75], "linear", 0.3, 0.5, 5e-324, score="score") == ([0], [0.75])
    assert _run(dup, [0.75, 0.75], "linear", 0.3, 0.5, 0.0, score="score") == ([0, 1], [0.75, 0.0])
    # 6: a zero-area box is never decayed and decays nobody
    zero = np.array([[5, 5, 5, 9], [4, 4, 8, 16], [5, 5, 5, 9]], dtype=np.float64)
    for method in ("linear", "gaussian"):
        assert _run(zero, [0.95, 0.9, 0.5], method, 0.0, 0.5, 0.001, score="score") == ([0, 1, 2], [0.95, 0.9, 0.5])
    # bit-equal scores on disjoint boxes: the lowest input index first, also across the words of two owners (rows 1 and 70)
    far = np.array([[100.0 * i, 0, 100.0 * i + 10, 10] for i in range(71)])
    p71 = np.full(71, 0.5)
    p71[[1, 3, 70]] = 0.7
    keep, kept = _run(far, p71, "linear", 0.3, 0.5, 0.001, score="score")
    assert keep == [1, 3, 70] + [i for i in range(70) if i not in (1, 3)] and kept == [0.7] * 3 + [0.5] * 68
    # a NaN score is never live; nothing at all
    assert _run(pair, [np.nan, 0.8], "linear", 0.3, 0.5, 0.001, score="score") == ([1], [0.8])
    assert _run(np.zeros((0, 4)), np.zeros(0), "linear") == ([], [])
    from tinyfaces import ops
    with pytest.raises(ValueError):
        ops.soft_nms(_dev(pair), _dev(np.array(p)), "softer")
    with pytest.raises(ValueError):
        ops.soft_nms(_dev(pair), _dev(np.array(p)), "gaussian", sigma=0.0)
    with pytest.raises(RuntimeError, match="TF_SOFT_NMS_MAX_BOXES"):
        ops.soft_nms(torch.zeros(ops.SOFT_NMS_MAX_BOXES + 1, 4, dtype=torch.float64, device="cuda"),
                     torch.zeros(ops.SOFT_NMS_MAX_BOXES + 1, dtype=torch.float64, device="cuda"))


# --------------------------------------------------------------------------- case 4: run-to-run determinism
@pytest.mark.parametrize("method", ["linear", "gaussian"])
def test_soft_nms_is_bit_identical_run_to_run(method):
    from tinyfaces import ops
    n = 20000
    boxes, logits = vote_ref.clustered_boxes(n, seed=7)
    b, s = _dev(boxes), _dev(logits)
    k1, s1 = ops.soft_nms(b, s, method)
    k2, s2 = ops.soft_nms(b, s, method)
    report(f"soft_nms[n={n},{method},twice]", kept=int(k1.numel()), same_bits=bool(torch.equal(k1, k2) and torch.equal(s1, s2)))
    assert k1.numel() > 1000
    assert torch.equal(k1, k2) and torch.equal(s1, s2)
    assert bool((s1[1:] <= s1[:-1]).all()) and int(torch.unique(k1).numel()) == int(k1.numel())


# --------------------------------------------------------------------------- case 5: the batched form
def _batch(sizes, seed):
    parts = [vote_ref.clustered_boxes(n, seed=seed + i) for i, n in enumerate(sizes)]
    boxes = np.concatenate([p[0].reshape(-1, 4) for p in parts])
    scores = np.concatenate([p[1] for p in parts])
    return boxes, scores, np.concatenate([[0], np.cumsum(sizes)]).astype(int).tolist()


@pytest.mark.parametrize("sizes", [(130, 0, 1025), tuple(1 + (11 * i) % 70 for i in range(64))], ids=["S3", "S64"])
def test_soft_nms_batched_equals_single_calls(sizes):
    from tinyfaces import ops
    assert len(sizes) in (3, 64) and (len(sizes) == 3 or {min(sizes), max(sizes)} == {1, 70})
    boxes, scores, offs = _batch(sizes, 80)
    b, s = _dev(boxes), _dev(scores)
    for method in ("linear", "gaussian"):
        res = ops.soft_nms_batched(b, s, offs, method)
        assert len(res) == len(sizes)
        for i, (a, e) in enumerate(zip(offs, offs[1:])):
            one_keep, one_scores = ops.soft_nms(b[a:e], s[a:e], method)
            assert torch.equal(res[i][0], one_keep + a), (method, i)         # indices into the concatenated input
            assert torch.equal(res[i][1], one_scores), (method, i)
            assert e > a or res[i][0].numel() == 0
        # a mask budget that splits the call into groups of segments: the same lists
        small = ops._mask_bytes(max(sizes))                                  # the largest segment alone fills it: at least two groups
        split = ops.soft_nms_batched(b, s, offs, method, mask_budget_bytes=small)
        assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(res, split)), method
    ref = soft_nms_ref.soft_nms_batched(boxes, scores, offs, method="gaussian")
    assert all(np.array_equal(x[0].cpu().numpy(), r[0]) for x, r in zip(res, ref))


def test_soft_nms_batched_chained_vote():
    """vote=(t, weight): the vote runs on the device-side keep list; membership and weights from the ORIGINAL scores, column 4 the Soft-NMS score."""
    from tinyfaces import ops
    sizes = (130, 0, 1025)
    boxes, scores, offs = _batch(sizes, 80)
    b, s = _dev(boxes), _dev(scores)
    res = ops.soft_nms_batched(b, s, offs, "linear")
    res_v, rows = ops.soft_nms_batched(b, s, offs, "linear", vote=(0.5, "sigmoid"))
    res_g, rows_g = ops.soft_nms_batched(b, s, offs, "linear", mask_budget_bytes=1, vote=(0.5, "sigmoid"))
    plain = ops.box_voting_batched(b, s, offs, [k for k, _ in res], 0.5)
    for i in range(3):
        assert torch.equal(res_v[i][0], res[i][0]) and torch.equal(res_v[i][1], res[i][1])
        assert torch.equal(rows[i][:, :4], plain[i][:, :4])                  # the vote as it is today, on the soft keep list
        assert torch.equal(rows[i][:, 4], res[i][1])                         # column 4: the decayed probability
        assert torch.equal(rows_g[i], rows[i]) and torch.equal(res_g[i][0], res[i][0])
    assert rows[1].shape == (0, 5)


# --------------------------------------------------------------------------- case 6: the write contract
@pytest.mark.parametrize("n", [65, 1025])
def test_soft_nms_writes_only_what_it_keeps(hip, n):
    from tinyfaces import ops
    boxes, logits = _inputs(n)
    b, s = guarded_like(torch.from_numpy(boxes.copy()), "cuda"), guarded_like(torch.from_numpy(logits.copy()), "cuda")
    for method, mid in (("linear", 1), ("gaussian", 2)):
        want_keep, want_scores = ops.soft_nms(_dev(boxes), _dev(logits), method, 0.3, 0.5, 0.3)
        K = int(want_keep.numel())
        assert 0 < K < n
        keep, kept = guarded((n,), torch.int64, "cuda"), guarded((n,), torch.float64, "cuda")
        cnt = guarded((1,), torch.int32, "cuda")
        cnt.zero_()
        wsb = hip.lib().tf_soft_nms_workspace_bytes(n)
        ws = guarded_workspace(wsb, "cuda", pitch_bytes=((n + 63) // 64) * 8)
        hip.check(hip.lib().tf_soft_nms_f64(hip.ptr(b), hip.ptr(s), n, mid, 0.3, 0.5, 0.3, 0, hip.ptr(keep), hip.ptr(kept), hip.ptr(cnt),
                                            hip.ptr(ws), wsb, hip.stream()), "tf_soft_nms_f64")
        torch.cuda.synchronize()
        for t, what in ((keep, "keep_out"), (kept, "score_out"), (cnt, "num_keep"), (ws, "workspace"), (b, "boxes"), (s, "scores")):
            assert_guards(t, f"{what} ({method}, n={n})")
        assert int(cnt.item()) == K
        assert_written(keep, slice(0, K), "kept indices"); assert_written(kept, slice(0, K), "kept scores")
        assert unwritten(keep, slice(K, None))[0] == n - K, "a keep row >= num_keep was written"
        assert unwritten(kept, slice(K, None))[0] == n - K, "a score row >= num_keep was written"
        assert torch.equal(keep[:K], want_keep) and torch.equal(kept[:K], want_scores)
        assert np.array_equal(b.cpu().numpy(), boxes) and np.array_equal(s.cpu().numpy(), logits)


# --------------------------------------------------------------------------- case 7: get_detections
@pytest.fixture(scope="module")
def detector(golden):
    """The fixture of tests/test_gpu_tta.py, rebuilt: the product model with the oracle's tamed weights, fp32, on the golden `detections`
    image; the calls several tests share are made once."""
    from oracle.model import OracleDetectionModel, tame_init_
    from oracle.targets import RF
    from tinyfaces import transforms
    from tinyfaces.evaluation import get_detections
    from tinyfaces.models.model import DetectionModel
    m = DetectionModel(num_templates=25)
    m.load_state_dict(tame_init_(OracleDetectionModel(num_templates=25), 0).state_dict(), strict=True)
    m = m.cuda().set_compute_dtype(torch.float32).eval()
    g = golden("detections")
    tf = transforms.Compose([transforms.ToTensor(), transforms.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])])
    kw = dict(prob_thresh=float(g["thr"]), nms_thresh=0.3, scales=tuple(g["scales"].tolist()), device="cuda")
    img = torch.from_numpy(g["img"])
    mirror = torch.from_numpy(np.ascontiguousarray(g["img"][..., ::-1]))
    templates = golden("targets")["templates"]

    def call(image, **extra):
        return get_detections(m, image, templates, RF, tf, **{**kw, **extra})

    shared = {"plain": call(img, return_candidates=True), "flip": call(img, flip=True, return_candidates=True)}
    return {"model": m, "img": img, "mirror": mirror, "templates": templates, "rf": RF, "tf": tf, "kw": kw, "call": call, **shared}


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("method", ["linear", "gaussian"])
def test_get_detections_soft_nms(detector, method, flip):
    res, cand, keep = detector["call"](detector["img"], soft_nms=method, flip=flip, return_candidates=True)
    _, cand0, keep0 = detector["flip" if flip else "plain"]
    assert cand.shape[0] > 0 and np.array_equal(cand, cand0)                 # the candidates are the hard path's
    ref_keep, ref_scores, rank_margin, thresh_margin = soft_nms_ref.soft_nms(cand[:, :4], cand[:, 4], method, 0.3, 0.5, 0.001)
    bound = soft_nms_ref.score_bound(len(ref_keep))
    same = bool(np.array_equal(keep, ref_keep))
    dev = _rel(res[:, 4], ref_scores) if same else float("nan")
    report(f"get_detections[soft_nms={method},flip={flip}]", candidates=cand.shape[0], kept=len(keep), kept_hard=len(keep0), keep_equal=same,
           score_maxrel=dev, score_bound=bound, rank_margin=rank_margin, thresh_margin=thresh_margin)
    print(f"get_detections soft_nms={method} flip={flip}: {cand.shape[0]} candidates, kept {len(keep)} (hard {len(keep0)}) "
          f"score_maxrel {dev:.3e} bound {bound:.3e} margins {rank_margin:.3e} {thresh_margin:.3e}")
    assert same
    assert res.shape == (len(keep), 5) and np.array_equal(res[:, :4], cand[keep][:, :4])      # rows are cand[keep] ...
    assert dev <= bound                                                      # ... with the decayed probability in column 4


def test_get_detections_soft_nms_with_box_voting(detector):
    for method in ("linear", "gaussian"):
        soft, cand, keep = detector["call"](detector["img"], soft_nms=method, return_candidates=True)
        res, cand_v, keep_v = detector["call"](detector["img"], soft_nms=method, box_voting=0.5, return_candidates=True)
        assert np.array_equal(cand_v, cand) and np.array_equal(keep_v, keep)  # the vote changes neither the candidates nor the selection
        ref, votes = vote_ref.box_voting(cand[:, :4], cand[:, 4], keep, 0.5)  # weights and membership from the ORIGINAL scores (logits)
        dev, bound = float(np.abs(res[:, :4] - ref[:, :4]).max()), vote_ref.coordinate_bound(cand.shape[0], cand[:, :4])
        moved = int((res[:, :4] != cand[keep][:, :4]).any(axis=1).sum())
        report(f"get_detections[soft_nms={method},box_voting]", candidates=cand.shape[0], kept=len(keep), moved=moved, coord_maxabs=dev,
               coord_bound=bound)
        assert res.shape == (len(keep), 5) and dev <= bound and moved > 0
        assert np.array_equal(res[:, 4], soft[:, 4])                          # column 4 is the Soft-NMS score, not the logit


def test_get_detections_batch_with_soft_nms_equals_the_loop(detector):
    from tinyfaces.evaluation import get_detections_batch
    d = detector
    imgs = [d["img"], d["mirror"]]
    for extra in (dict(soft_nms="linear"), dict(soft_nms="gaussian", flip=True), dict(soft_nms="gaussian", soft_nms_sigma=0.3, box_voting=0.5),
                  dict(soft_nms="linear", soft_nms_score_thresh=0.3)):
        loop = [d["call"](im, **extra) for im in imgs]
        batch = get_detections_batch(d["model"], imgs, d["templates"], d["rf"], d["tf"], **d["kw"], **extra)
        assert len(batch) == 2 and all(np.array_equal(a, b) for a, b in zip(batch, loop)), extra
        assert loop[0].shape[0] > 0


def test_soft_nms_keywords_at_their_defaults_change_nothing(detector):
    from tinyfaces.evaluation import get_detections_batch
    d = detector
    named = d["call"](d["img"], soft_nms=None, soft_nms_sigma=0.5, soft_nms_score_thresh=0.001, return_candidates=True)
    assert all(np.array_equal(a, b) for a, b in zip(named, d["plain"]))
    named = d["call"](d["img"], flip=True, soft_nms=None, soft_nms_sigma=0.5, soft_nms_score_thresh=0.001, return_candidates=True)
    assert all(np.array_equal(a, b) for a, b in zip(named, d["flip"]))
    batch = get_detections_batch(d["model"], [d["img"]], d["templates"], d["rf"], d["tf"], **d["kw"], soft_nms=None)
    assert np.array_equal(batch[0], d["plain"][0])
    # the parameters do arrive: another sigma, other scores; a higher threshold, fewer rows
    a = d["call"](d["img"], soft_nms="gaussian")
    b = d["call"](d["img"], soft_nms="gaussian", soft_nms_sigma=0.1)
    c = d["call"](d["img"], soft_nms="gaussian", soft_nms_score_thresh=0.6)
    assert a.shape[0] >= b.shape[0] and not np.array_equal(a, b) and c.shape[0] < a.shape[0]
    assert (c[:, 4] >= 0.6).all() and (a[:, 4] >= 0.001).all() and (a[:, 4] <= 1.0).all()


# --------------------------------------------------------------------------- case 8: evaluate_model.run
def test_evaluate_model_run_passes_the_keywords_through(tmp_path):
    import evaluate_model
    from bench import tame_init_
    from tinyfaces.evaluation import get_detections, write_results
    from tinyfaces.models.model import DetectionModel
    args = evaluate_model.soft_nms_arguments(["synthetic", "--num-images", "2", "--workers", "0", "--soft-nms", "gaussian", "--soft-nms-sigma", "0.3",
                                              "--soft-nms-score-thresh", "0.01", "--box-voting", "0.5"])
    loader, templates = evaluate_model.dataloader(args)
    device = torch.device("cuda")
    m = tame_init_(DetectionModel(num_objects=1, num_templates=25), seed=3).to(device).eval()
    # untrained scores sit at sigmoid(~0): a threshold only their tail passes, taken from one forward of the first image at full size
    img0 = next(iter(loader))[0][0]
    mean, std = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)
    with torch.no_grad():
        prob = torch.sigmoid(m(((img0 - mean) / std).unsqueeze(0).to(device))[0, :25].float()).flatten()
    thr = float(torch.quantile(prob, 0.999))
    soft = dict(soft_nms=args.soft_nms, soft_nms_sigma=args.soft_nms_sigma, soft_nms_score_thresh=args.soft_nms_score_thresh)
    assert soft == dict(soft_nms="gaussian", soft_nms_sigma=0.3, soft_nms_score_thresh=0.01)
    with torch.no_grad(), m.constant_weights():
        evaluate_model.run(m, loader, templates, thr, 0.3, device, "val", results_dir=str(tmp_path / "run"), box_voting=args.box_voting, **soft)
        evaluate_model.run(m, loader, templates, thr, 0.3, device, "val", results_dir=str(tmp_path / "plain"))
        names = []
        for img, filename in loader:
            dets = get_detections(m, img[0], templates, loader.dataset.rf, loader.dataset.transforms, thr, 0.3, device=device, pyramid_on_gpu=True,
                                  box_voting=0.5, soft_nms="gaussian", soft_nms_sigma=0.3, soft_nms_score_thresh=0.01)
            write_results(dets, filename[0], "val", str(tmp_path / "direct"))
            names.append(filename[0].replace("jpg", "txt"))
    assert len(names) == 2
    differs = 0
    for name in names:
        got, want = (tmp_path / "run" / name).read_text(), (tmp_path / "direct" / name).read_text()
        assert got == want, name
        assert int(got.split("\n")[1]) > 0
        differs += got != (tmp_path / "plain" / name).read_text()
    assert differs                                                           # the keywords did arrive: the plain run writes other rows
