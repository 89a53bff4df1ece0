"""-m gpu: Matrix NMS (csrc/matrix_nms.hip: tf_matrix_nms_f64[_batched]; ops.matrix_nms, ops.matrix_nms_batched; get_detections /
get_detections_batch with soft_nms="matrix_linear" | "matrix_gaussian") against the numpy restatement tests/matrix_nms_ref.py on the cases of
tests/matrix_nms_cases.py.

Bounds.  LINEAR on probabilities (score="score", fed the host's sigmoid): behind p every operation is a single IEEE float64 operation and max /
min are exact -- keep AND scores equal the restatement's bit for bit.  (Under score="sigmoid" the p themselves come from the device's exp, so
the same method is held to the gaussian bound there.)  GAUSSIAN on logits: keep EQUAL -- tests/test_matrix_nms.py shows on the CPU that no
emission order, admission or emission test of any case is within 1e-9 of a decision, and that bit-equal emitted scores come from bit-equal
(p, argument) pairs, so a last-bit difference in exp cannot reorder or cross the threshold -- and scores within the relative bound
soft_nms_ref.score_bound(1) = 24 * 2^-52, the project's allowance for one exp, a multiply and the sigmoid.  Every kernel call here is made on
guarded operands (tests/redzone.py): keep_out, score_out, num_keep and the workspace between 0xFF bands, the workspace itself filled with
0xFF (NaN bytes: a stale arena), rows beyond num_keep required to be untouched."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import matrix_nms_cases as mc
import matrix_nms_ref
import soft_nms_ref
import vote_ref
from gpu_util import report
from redzone import assert_guards, assert_written, guarded, guarded_like, guarded_workspace, unwritten

pytestmark = pytest.mark.gpu

BOUND = soft_nms_ref.score_bound(1)
METHOD_ID = {"linear": 1, "gaussian": 2}
SCORE_ID = {"sigmoid": 0, "score": 1}


@pytest.fixture(scope="module", autouse=True)
def _random_state_left_as_found():
    """The `detector` fixture below builds models (their initial weights draw from torch's global generator, and the oracle's tame_init_ re-seeds
    it).  Tests of other files that run later in the same process build unseeded models of their own (bench.tame_init_ does not seed) and derive
    thresholds from them: they must find the generators in the state they would have found without this file."""
    import random
    state = (random.getstate(), np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state_all())
    yield
    random.setstate(state[0]); np.random.set_state(state[1]); torch.set_rng_state(state[2]); torch.cuda.set_rng_state_all(state[3])


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C", copy=True))      # a copy: the cached inputs are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


def _rel(got, want):
    """Largest relative deviation of the scores (0 where both are 0)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.size == 0:
        return 0.0
    den = np.where(want != 0, np.abs(want), 1.0)
    return float((np.abs(got - want) / den).max())


@functools.lru_cache(maxsize=None)
def _operands(name, score):
    """The guarded device inputs of a case, shared by its calls (the kernels only read them; every call checks their guards)."""
    boxes = mc.cases()[name][0]
    return guarded_like(torch.from_numpy(boxes.copy()), "cuda"), guarded_like(torch.from_numpy(mc.scores_for(name, score).copy()), "cuda")


def _guarded_call(hip, name, method, score, max_keep=0, sigma=0.5, stale=True):
    """tf_matrix_nms_f64_batched on guarded operands -> [(keep, scores) numpy per segment].  Checks the write contract of the call."""
    boxes, _, offs, thr = mc.cases()[name]
    n, S = offs[-1], len(offs) - 1
    b, s = _operands(name, score)
    keep, kept = guarded((max(n, 1),), torch.int64, "cuda"), guarded((max(n, 1),), torch.float64, "cuda")
    cnt = guarded((S,), torch.int32, "cuda")
    cnt.zero_()
    host = (C.c_int32 * (S + 1))(*offs)
    wsb = hip.lib().tf_matrix_nms_batched_workspace_bytes(host, S)
    ws = guarded_workspace(max(wsb, 1), "cuda", pitch_bytes=32)
    if not stale:
        ws.zero_()
    hip.check(hip.lib().tf_matrix_nms_f64_batched(hip.ptr(b), hip.ptr(s), host, S, METHOD_ID[method], sigma, thr, SCORE_ID[score], max_keep,
                                                  hip.ptr(keep), hip.ptr(kept), hip.ptr(cnt), hip.ptr(ws), wsb, hip.stream()), "tf_matrix_nms_f64_batched")
    torch.cuda.synchronize()
    what = f"{name}, {method}, {score}, max_keep={max_keep}"
    for t, label in ((keep, "keep_out"), (kept, "score_out"), (cnt, "num_keep"), (ws, "workspace"), (b, "boxes"), (s, "scores")):
        assert_guards(t, f"{label} ({what})")
    assert np.array_equal(b.cpu().numpy(), boxes) and np.array_equal(s.cpu().numpy(), mc.scores_for(name, score), equal_nan=True)
    counts = cnt.cpu().numpy().tolist()
    written = torch.zeros(max(n, 1), dtype=torch.bool, device="cuda")
    out = []
    for i, (a, e) in enumerate(zip(offs, offs[1:])):
        assert 0 <= counts[i] <= e - a, (what, i, counts[i])
        written[a:a + counts[i]] = True
        out.append((keep[a:a + counts[i]].cpu().numpy(), kept[a:a + counts[i]].cpu().numpy()))
    if n:
        assert_written(keep, written, f"kept indices ({what})"); assert_written(kept, written, f"kept scores ({what})")
        rest = int((~written).sum())
        assert unwritten(keep, ~written)[0] == rest, f"a keep row >= num_keep was written ({what})"
        assert unwritten(kept, ~written)[0] == rest, f"a score row >= num_keep was written ({what})"
    return out


# --------------------------------------------------------------------------- the kernels against the numpy restatement
@pytest.mark.parametrize("name", list(mc.cases()))
def test_linear_on_probabilities_is_bit_exact(hip, name):
    ref = mc.reference(name, "linear", "score")
    got = _guarded_call(hip, name, "linear", "score")
    same = all(np.array_equal(g[0], r[0]) for g, r in zip(got, ref))
    bits = same and all(np.array_equal(g[1], r[1]) for g, r in zip(got, ref))
    report(f"matrix_nms[{name},linear,score]", kept=sum(len(g[0]) for g in got), ref_kept=sum(len(r[0]) for r in ref), keep_equal=same,
           scores_bit_equal=bits)
    print(f"matrix_nms {name} linear/score: kept {sum(len(g[0]) for g in got)} (ref {sum(len(r[0]) for r in ref)}) keep_equal {same} bit_equal {bits}")
    assert same and bits
    if name == "all_below":
        assert all(len(g[0]) == 0 for g in got)


@pytest.mark.parametrize("method", ["gaussian", "linear"])
@pytest.mark.parametrize("name", list(mc.cases()))
def test_on_logits_keep_is_equal_and_scores_within_one_exp(hip, name, method):
    ref = mc.reference(name, method, "sigmoid")
    gap, dist = min(r[2] for r in ref), min(r[3] for r in ref)
    assert gap > mc.MARGIN and dist > mc.MARGIN                                # (the condition tests/test_matrix_nms.py checks on the CPU)
    got = _guarded_call(hip, name, method, "sigmoid")
    same = all(np.array_equal(g[0], r[0]) for g, r in zip(got, ref))
    dev = max([_rel(g[1], r[1]) for g, r in zip(got, ref)]) if same else float("nan")
    report(f"matrix_nms[{name},{method},sigmoid]", kept=sum(len(g[0]) for g in got), ref_kept=sum(len(r[0]) for r in ref), keep_equal=same,
           score_maxrel=dev, score_bound=BOUND, gap_margin=gap, thresh_margin=dist)
    print(f"matrix_nms {name} {method}/sigmoid: kept {sum(len(g[0]) for g in got)} (ref {sum(len(r[0]) for r in ref)}) keep_equal {same} "
          f"score_maxrel {dev:.3e} bound {BOUND:.3e} margins {gap:.3e} {dist:.3e}")
    assert same
    assert dev <= BOUND
    thr = mc.cases()[name][3]
    for k, s in got:
        assert (np.diff(s) <= 0).all() and (s >= thr).all() and len(set(k.tolist())) == len(k)


def test_hand_worked_cases():
    from tinyfaces import ops

    def run(boxes, p, method, **kw):
        keep, kept = ops.matrix_nms(_dev(np.asarray(boxes, dtype=np.float64)), _dev(np.asarray(p, dtype=np.float64)), method, score="score", **kw)
        assert keep.dtype == torch.int64 and kept.dtype == torch.float64 and keep.shape == kept.shape
        return keep.cpu().numpy().tolist(), kept.cpu().numpy().tolist()

    pair = np.array([[0, 0, 10, 10], [0, 0, 10, 5]], dtype=np.float64)       # IoU exactly 0.5
    assert run(pair, [0.9, 0.8], "linear") == ([0, 1], [0.9, 0.4])
    assert run(pair, [0.9, 0.8], "linear", score_threshold=0.4) == ([0, 1], [0.9, 0.4])                      # emission is `>=`
    assert run(pair, [0.9, 0.8], "linear", score_threshold=float(np.nextafter(0.4, 1.0))) == ([0], [0.9])
    keep, kept = run(pair, [0.9, 0.8], "gaussian")
    assert keep == [0, 1] and kept[0] == 0.9 and abs(kept[1] - 0.8 * np.exp(-0.5)) <= BOUND * 0.8
    same = np.array([[3, 4, 13, 24]] * 3, dtype=np.float64)
    assert run(same, [0.9, 0.8, 0.7], "linear", score_threshold=0.0) == ([0, 1, 2], [0.9, 0.0, 0.0])         # 1, 0, 0; the tie by rank
    keep, kept = run(same, [0.9, 0.8, 0.7], "gaussian")
    assert keep == [0, 1, 2] and np.allclose(kept, [0.9, 0.8 * np.exp(-2.0), 0.7 * np.exp(-2.0)], rtol=BOUND, atol=0)
    abc = np.array([[0, 0, 10, 10], [0, 0, 10, 8], [20, 20, 30, 30]], dtype=np.float64)
    assert run(abc, [0.9, 0.8, 0.7], "linear") == ([0, 2, 1], [0.9, 0.7, 0.8 * (1.0 - 0.8)])
    assert run(abc, [0.9, 0.8, 0.7], "linear", max_keep=2) == ([0, 2], [0.9, 0.7])
    far = np.array([[100.0 * i, 0, 100.0 * i + 10, 10] for i in range(71)])
    p71 = np.full(71, 0.5)
    p71[[1, 3, 70]] = 0.7
    for method in ("linear", "gaussian"):
        assert run(far, p71, method) == ([1, 3, 70] + [i for i in range(70) if i not in (1, 3)], [0.7] * 3 + [0.5] * 68)
    assert run(pair, [np.nan, 0.8], "linear") == ([1], [0.8])
    assert run(np.zeros((0, 4)), np.zeros(0), "gaussian") == ([], [])
    with pytest.raises(ValueError):
        ops.matrix_nms(_dev(pair), _dev(np.array([0.9, 0.8])), "softer")
    with pytest.raises(RuntimeError, match="TF_MATRIX_NMS_MAX_BOXES"):
        ops.matrix_nms(torch.zeros(ops.MATRIX_NMS_MAX_BOXES + 1, 4, dtype=torch.float64, device="cuda"),
                       torch.zeros(ops.MATRIX_NMS_MAX_BOXES + 1, dtype=torch.float64, device="cuda"))


# --------------------------------------------------------------------------- the cap
@pytest.mark.parametrize("method,score", [("linear", "score"), ("gaussian", "sigmoid")])
def test_max_keep_returns_the_first_rows_of_the_uncapped_call(hip, method, score):
    name = "S3_empty_middle"                                                 # 257, 0 and 513 candidates: the cap acts per segment
    full = _guarded_call(hip, name, method, score)
    K = len(full[0][0])
    assert 3 < K < 257 + 1 and len(full[2][0]) > K
    for cap in (1, K - 1, K, K + 1):
        got = _guarded_call(hip, name, method, score, max_keep=cap)          # (rows beyond num_keep unwritten: checked inside)
        for g, f in zip(got, full):
            assert len(g[0]) == min(len(f[0]), cap)
            assert np.array_equal(g[0], f[0][:cap]) and np.array_equal(g[1], f[1][:cap])


# --------------------------------------------------------------------------- determinism, the arena
@pytest.mark.parametrize("method", ["linear", "gaussian"])
def test_same_bits_on_every_run_and_from_a_stale_workspace(hip, method):
    a = _guarded_call(hip, "n5000", method, "sigmoid")                      # the workspace holds 0xFF bytes: NaN wherever it is read as float64
    b = _guarded_call(hip, "n5000", method, "sigmoid")
    z = _guarded_call(hip, "n5000", method, "sigmoid", stale=False)         # ... and zeros
    assert len(a[0][0]) > 4000
    assert np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[0][1], b[0][1])
    assert np.array_equal(a[0][0], z[0][0]) and np.array_equal(a[0][1], z[0][1])
    from tinyfaces import ops
    boxes, logits = mc.cases()["n5000"][:2]
    keep, kept = ops.matrix_nms(_dev(boxes), _dev(logits), method)          # the binding: its own cached workspace
    assert np.array_equal(keep.cpu().numpy(), a[0][0]) and np.array_equal(kept.cpu().numpy(), a[0][1])


def test_batched_binding_equals_single_calls_and_the_raw_call(hip):
    from tinyfaces import ops
    for name in ("S3_empty_middle", "S64"):
        boxes, logits, offs, _ = mc.cases()[name]
        b, s = _dev(boxes), _dev(logits)
        for method in ("linear", "gaussian"):
            res = ops.matrix_nms_batched(b, s, offs, method)
            raw = _guarded_call(hip, name, method, "sigmoid")
            assert len(res) == len(offs) - 1
            for i, (a, e) in enumerate(zip(offs, offs[1:])):
                one_keep, one_scores = ops.matrix_nms(b[a:e], s[a:e], method)
                assert torch.equal(res[i][0], one_keep + a) and torch.equal(res[i][1], one_scores), (name, method, i)
                assert np.array_equal(res[i][0].cpu().numpy(), raw[i][0]) and np.array_equal(res[i][1].cpu().numpy(), raw[i][1])
                assert e > a or res[i][0].numel() == 0


# --------------------------------------------------------------------------- the vote chain
def test_chained_vote_equals_voting_on_the_restatements_keep_list():
    """vote=(t, weight): the vote runs on the device-side keep list and counts; membership and weights from the ORIGINAL scores, column 4 the
    Matrix NMS score."""
    from tinyfaces import ops
    name = "S3_empty_middle"
    boxes, logits, offs, _ = mc.cases()[name]
    b, s = _dev(boxes), _dev(logits)
    for method, cap in (("gaussian", None), ("linear", 40)):
        ref = mc.reference(name, method, "sigmoid")
        ref_keeps = [r[0][:cap] for r in ref]
        res, rows = ops.matrix_nms_batched(b, s, offs, method, max_keep=cap, vote=(0.5, "sigmoid"))
        plain = ops.matrix_nms_batched(b, s, offs, method, max_keep=cap)
        want, _ = vote_ref.box_voting_batched(boxes, logits, offs, ref_keeps, 0.5)
        bound = vote_ref.coordinate_bound(max(e - a for a, e in zip(offs, offs[1:])), boxes)
        for i in range(len(offs) - 1):
            assert np.array_equal(res[i][0].cpu().numpy(), ref_keeps[i]) and torch.equal(res[i][0], plain[i][0]) and torch.equal(res[i][1], plain[i][1])
            got = rows[i].cpu().numpy()
            assert got.shape == (len(ref_keeps[i]), 5)
            if got.size:
                assert float(np.abs(got[:, :4] - want[i][:, :4]).max()) <= bound
                assert np.array_equal(got[:, 4], res[i][1].cpu().numpy())     # column 4: the decayed probability
        assert rows[1].shape == (0, 5)
        moved = int((rows[2].cpu().numpy()[:, :4] != boxes[ref_keeps[2]]).any(axis=1).sum())
        assert moved > 0


# --------------------------------------------------------------------------- the call surface, on the planted head
@pytest.fixture(scope="module")
def detector():
    """tests/planted.py's case (planted image, planted head on the tame-init trunk), bf16, three pyramid levels."""
    from oracle.model import OracleDetectionModel, tame_init_
    from planted import load_plan, plant_head_, planted_image
    from tinyfaces import ops, transforms
    from tinyfaces.datasets.templates import load_templates
    from tinyfaces.evaluation import get_detections
    from tinyfaces.models.model import DetectionModel
    templates = load_templates()
    m = DetectionModel(num_templates=25)
    m.load_state_dict(plant_head_(tame_init_(OracleDetectionModel(num_templates=25), 0), load_plan()).state_dict(), strict=True)
    m = m.cuda().set_compute_dtype(torch.bfloat16).eval()
    imgs = [torch.from_numpy(planted_image(seed=seed)).permute(2, 0, 1).float().div(255) for seed in (0, 1, 2)]
    tf = transforms.Compose([transforms.ToTensor(), transforms.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])])
    kw = dict(prob_thresh=0.5, nms_thresh=0.3, scales=(-1, 0, 1), device="cuda", pyramid_on_gpu=True)

    def call(image, **extra):
        return get_detections(m, image, templates, ops.RF, tf, **{**kw, **extra})

    shared = {"plain": call(imgs[0], return_candidates=True), "flip": call(imgs[0], flip=True, return_candidates=True)}
    return {"model": m, "imgs": imgs, "templates": templates, "rf": ops.RF, "tf": tf, "kw": kw, "call": call, **shared}


@pytest.mark.parametrize("which", ["plain", "pre_nms_topk", "max_detections", "flip", "all"])
def test_get_detections_matrix_gaussian_equals_the_restatement_on_its_candidates(detector, which):
    n0, n1 = detector["plain"][1].shape[0], detector["flip"][1].shape[0]
    extra = {"plain": dict(), "pre_nms_topk": dict(pre_nms_topk=n0 // 2), "max_detections": dict(max_detections=5), "flip": dict(flip=True),
             "all": dict(flip=True, pre_nms_topk=(2 * n1) // 3, max_detections=7)}[which]
    res, cand, keep = detector["call"](detector["imgs"][0], soft_nms="matrix_gaussian", return_candidates=True, **extra)
    _, cand0, keep0 = detector["flip" if extra.get("flip") else "plain"]
    assert n0 >= 12 and n1 > n0 and np.array_equal(cand, cand0)              # the FULL candidate list of the hard path, whatever the cut
    sub = np.arange(cand.shape[0])
    topk = extra.get("pre_nms_topk")
    if topk is not None:                                                     # the K best in the hard NMS's order, kept in list order
        assert cand.shape[0] > topk
        sub = np.sort(np.argsort(-cand[:, 4], kind="stable")[:topk])
    ref_keep, ref_scores, gap, dist = matrix_nms_ref.matrix_nms(cand[sub, :4], cand[sub, 4], "gaussian", 0.5, 0.001, max_keep=extra.get("max_detections"))
    ref_keep = sub[ref_keep]
    assert gap > mc.MARGIN and dist > mc.MARGIN, (gap, dist)
    same = bool(np.array_equal(keep, ref_keep))
    dev = _rel(res[:, 4], ref_scores) if same else float("nan")
    report(f"get_detections[soft_nms=matrix_gaussian,{which}]", candidates=cand.shape[0], kept=len(keep), kept_hard=len(keep0), keep_equal=same,
           score_maxrel=dev, score_bound=BOUND, gap_margin=gap, thresh_margin=dist)
    print(f"get_detections matrix_gaussian {which}: {cand.shape[0]} candidates, kept {len(keep)} (hard {len(keep0)}) score_maxrel {dev:.3e} "
          f"margins {gap:.3e} {dist:.3e}")
    assert same and len(keep) > 0
    assert res.shape == (len(keep), 5) and np.array_equal(res[:, :4], cand[keep][:, :4])      # rows are cand[keep] ...
    assert dev <= BOUND                                                      # ... with the decayed probability in column 4
    if "max_detections" in extra:
        assert len(keep) == extra["max_detections"]


def test_get_detections_matrix_linear_and_box_voting(detector):
    res, cand, keep = detector["call"](detector["imgs"][0], soft_nms="matrix_linear", return_candidates=True, nms_thresh=0.9)      # nms_thresh: unused
    ref_keep, ref_scores, gap, dist = matrix_nms_ref.matrix_nms(cand[:, :4], cand[:, 4], "linear", 0.5, 0.001)
    assert gap > mc.MARGIN and dist > mc.MARGIN
    assert np.array_equal(keep, ref_keep) and _rel(res[:, 4], ref_scores) <= BOUND
    voted, cand_v, keep_v = detector["call"](detector["imgs"][0], soft_nms="matrix_linear", box_voting=0.5, return_candidates=True)
    assert np.array_equal(cand_v, cand) and np.array_equal(keep_v, keep)
    want, _ = vote_ref.box_voting(cand[:, :4], cand[:, 4], keep, 0.5)
    assert float(np.abs(voted[:, :4] - want[:, :4]).max()) <= vote_ref.coordinate_bound(cand.shape[0], cand[:, :4])
    assert np.array_equal(voted[:, 4], res[:, 4])
    # the keywords arrive: another sigma, other scores; a higher threshold, fewer rows; the default path is what it was
    a = detector["call"](detector["imgs"][0], soft_nms="matrix_gaussian")
    b = detector["call"](detector["imgs"][0], soft_nms="matrix_gaussian", soft_nms_sigma=0.1)
    c = detector["call"](detector["imgs"][0], soft_nms="matrix_gaussian", soft_nms_score_thresh=0.6)
    assert a.shape[0] >= b.shape[0] and not np.array_equal(a, b) and c.shape[0] < a.shape[0] and (c[:, 4] >= 0.6).all()
    with pytest.raises(ValueError):
        detector["call"](detector["imgs"][0], soft_nms="foo")


def test_get_detections_batch_of_three_equals_three_single_calls(detector):
    from tinyfaces.evaluation import get_detections_batch
    d = detector
    for extra in (dict(soft_nms="matrix_gaussian"), dict(soft_nms="matrix_linear", max_detections=6, box_voting=0.5),
                  dict(soft_nms="matrix_gaussian", soft_nms_sigma=0.3, pre_nms_topk=25, flip=True)):
        kw = {**d["kw"], "scales": (-1, 0), **extra}
        loop = [d["call"](im, **{"scales": (-1, 0), **extra}) for im in d["imgs"]]
        batch = get_detections_batch(d["model"], d["imgs"], d["templates"], d["rf"], d["tf"], **kw)
        assert len(batch) == 3 and all(np.array_equal(a, b) for a, b in zip(batch, loop)), extra
        assert all(r.shape[0] > 0 for r in loop)
