"""-m gpu: test-time augmentation (csrc/vote.hip: tf_box_vote_f64[_batched], tf_boxes_unflip_f64; ops.box_voting, ops.box_voting_batched,
ops.boxes_unflip_; get_detections / get_detections_batch / evaluate_model.run with flip= and box_voting=) against the numpy restatement
tests/vote_ref.py.

Bounds.  Vote counts must be EQUAL: membership is decided by the NMS's IoU expression, which the kernel evaluates bit for bit like numpy.
Coordinates: n * 2^-52 * max|coordinate| (vote_ref.coordinate_bound: at most n products and n sums per coordinate, each rounded once, plus
~3 ulp per sigmoid weight on either side of the quotient); leaving one voter out moves a box by >= 1e-4, five orders of magnitude above it.
Scores, the batched form against single calls, a second run, the un-mirroring against its formula: bit-equal."""
import ctypes as C

import numpy as np
import pytest
import torch

import vote_ref
from gpu_util import report
from redzone import assert_guards, assert_written, guarded, guarded_like, unwritten

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 512, 513, 1025, 4097]       # one wave, a wave edge, the 256 staging threads, the 512-candidate LDS tile and past it


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _keep_of(boxes_d, scores_d, thr=0.3):
    from tinyfaces import ops
    return ops.nms(boxes_d, scores_d, thr)


# --------------------------------------------------------------------------- case 1: the vote kernel against the numpy restatement
@pytest.mark.parametrize("n", SIZES)
def test_vote_kernel_vs_numpy(n):
    from tinyfaces import ops
    boxes, scores = vote_ref.clustered_boxes(n, seed=n)
    b, s = _dev(boxes), _dev(scores)
    keep = _keep_of(b, s)
    out, votes = ops.box_voting(b, s, keep, 0.5, return_votes=True)
    k = keep.cpu().numpy()
    ref, ref_votes = vote_ref.box_voting(boxes, scores, k, 0.5)
    out, votes = out.cpu().numpy(), votes.cpu().numpy()
    bound = vote_ref.coordinate_bound(n, boxes)
    dev = float(np.abs(out[:, :4] - ref[:, :4]).max())
    moved = int((out[:, :4] != boxes[k]).any(axis=1).sum())
    report(f"box_vote[n={n}]", kept=len(k), moved=moved, max_votes=int(votes.max()), votes_equal=bool(np.array_equal(votes, ref_votes)),
           coord_maxabs=dev, coord_bound=bound, score_bit_equal=bool(np.array_equal(out[:, 4], scores[k])))
    print(f"box_vote n={n}: kept {len(k)} moved {moved} coord_maxabs {dev:.3e} bound {bound:.3e}")
    assert out.shape == (len(k), 5) and votes.dtype == np.int32
    assert np.array_equal(votes, ref_votes)
    assert dev <= bound
    assert np.array_equal(out[:, 4], scores[k])                              # the kept box's own score, carried through bit for bit
    if n >= 16:
        r = int(np.nonzero(k == 11)[0][0])                                   # the zero-area box: kept by the NMS, no votes, unchanged
        assert votes[r] == 0 and np.array_equal(out[r, :4], boxes[11])
        assert moved >= len(k) // 2


def test_vote_threshold_is_inclusive_and_weights_filter():
    """The hand-computed cases of tests/test_tta.py on the device: IoU exactly 0.5 votes at 0.5 and not at the next double; weight='score'
    drops non-positive and NaN weights; a kept box left without voters stays as it is."""
    from tinyfaces import ops
    boxes = np.array([[0, 0, 2, 1], [0, 0, 1, 1]], dtype=np.float64)
    scores = np.array([3.0, 1.0])
    keep = _dev(np.array([0, 1], dtype=np.int64))
    out, votes = ops.box_voting(_dev(boxes), _dev(scores), keep, 0.5, weight="score", return_votes=True)
    assert votes.tolist() == [2, 2] and np.array_equal(out.cpu().numpy(), [[0, 0, 1.75, 1, 3.0], [0, 0, 1.75, 1, 1.0]])
    out, votes = ops.box_voting(_dev(boxes), _dev(scores), keep, 0.5 + 2.0 ** -53, weight="score", return_votes=True)
    assert votes.tolist() == [1, 1] and np.array_equal(out.cpu().numpy(), [[0, 0, 2, 1, 3.0], [0, 0, 1, 1, 1.0]])
    boxes = np.array([[2, 0, 6, 4], [0, 0, 4, 4], [0, 0, 4, 4], [0, 0, 4, 4]], dtype=np.float64)
    scores = np.array([2.0, 0.0, -1.0, np.nan])
    out, votes = ops.box_voting(_dev(boxes), _dev(scores), keep.flip(0), 0.5, weight="score", return_votes=True)
    ref, ref_votes = vote_ref.box_voting(boxes, scores, [1, 0], 0.5, weight="score")
    assert votes.tolist() == ref_votes.tolist() == [0, 1]
    assert np.array_equal(out.cpu().numpy(), ref) and np.array_equal(ref[0], [0, 0, 4, 4, 0.0])
    with pytest.raises(ValueError):
        ops.box_voting(_dev(boxes), _dev(scores), keep, 0.0)
    with pytest.raises(ValueError):
        ops.box_voting(_dev(boxes), _dev(scores), keep, 0.5, weight="softmax")


# --------------------------------------------------------------------------- case 2: a larger list, twice
def test_vote_large_is_bit_identical_run_to_run():
    from tinyfaces import ops
    n = 16385
    boxes, logits = vote_ref.clustered_boxes(n, seed=7)
    scores = np.exp(0.5 * logits)                                            # positive: weight="score" takes them as they are
    b, s = _dev(boxes), _dev(scores)
    keep = _keep_of(b, s)
    a_out, a_votes = ops.box_voting(b, s, keep, 0.3, weight="score", return_votes=True)
    b_out, b_votes = ops.box_voting(b, s, keep, 0.3, weight="score", return_votes=True)
    assert torch.equal(a_out, b_out) and torch.equal(a_votes, b_votes)
    k = keep.cpu().numpy()
    ref, ref_votes = vote_ref.box_voting(boxes, scores, k, 0.3, weight="score")
    dev, bound = float(np.abs(a_out.cpu().numpy()[:, :4] - ref[:, :4]).max()), vote_ref.coordinate_bound(n, boxes)
    report("box_vote[n=16385,score,0.3]", kept=len(k), max_votes=int(ref_votes.max()), coord_maxabs=dev, coord_bound=bound)
    assert np.array_equal(a_votes.cpu().numpy(), ref_votes) and dev <= bound
    assert np.array_equal(a_out.cpu().numpy()[:, 4], scores[k])


# --------------------------------------------------------------------------- case 3: the batched form
def test_vote_batched_equals_single_calls():
    from tinyfaces import ops
    sizes = [300, 0, 1, 130]                                                 # an empty segment in the middle, a segment of one box
    parts = [vote_ref.clustered_boxes(n, seed=40 + i) for i, n in enumerate(sizes)]
    boxes = np.concatenate([p[0].reshape(-1, 4) for p in parts])
    scores = np.concatenate([p[1] for p in parts])
    offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    b, s = _dev(boxes), _dev(scores)
    keeps = ops.nms_batched(b, s, offs, 0.3)
    rows, votes = ops.box_voting_batched(b, s, offs, keeps, 0.5, return_votes=True)
    assert [r.shape[0] for r in rows] == [k.numel() for k in keeps] and rows[1].shape == (0, 5) and rows[2].shape == (1, 5)
    for i, (a, e) in enumerate(zip(offs, offs[1:])):
        if e == a:
            continue
        one, one_votes = ops.box_voting(b[a:e], s[a:e], keeps[i] - a, 0.5, return_votes=True)
        assert torch.equal(rows[i], one) and torch.equal(votes[i], one_votes), i
    ref_rows, ref_votes = vote_ref.box_voting_batched(boxes, scores, offs, [k.cpu().numpy() for k in keeps], 0.5)
    for i in range(4):
        assert np.array_equal(votes[i].cpu().numpy(), ref_votes[i])
        assert np.abs(rows[i].cpu().numpy() - ref_rows[i]).max(initial=0.0) <= vote_ref.coordinate_bound(max(sizes), boxes)
    # the chained form (nms_batched(vote=...): the raw keep list and the device-side counts, one synchronisation) returns the same rows
    keeps2, rows2 = ops.nms_batched(b, s, offs, 0.3, vote=(0.5, "sigmoid"))
    assert all(torch.equal(x, y) for x, y in zip(keeps, keeps2)) and all(torch.equal(x, y) for x, y in zip(rows, rows2))
    # ... also when the mask budget splits the call into groups of segments
    keeps3, rows3 = ops.nms_batched(b, s, offs, 0.3, mask_budget_bytes=1, vote=(0.5, "sigmoid"))
    assert all(torch.equal(x, y) for x, y in zip(keeps, keeps3)) and all(torch.equal(x, y) for x, y in zip(rows, rows3))
    # num_keep[s] = 0 on a segment that has boxes: no row for it, the others as before
    none = [keeps[0][:0], keeps[1], keeps[2], keeps[3]]
    rows0 = ops.box_voting_batched(b, s, offs, none, 0.5)
    assert rows0[0].shape == (0, 5) and torch.equal(rows0[2], rows[2]) and torch.equal(rows0[3], rows[3])


# --------------------------------------------------------------------------- case 4: the write contract
def test_vote_writes_only_the_kept_rows(hip):
    sizes = [200, 70, 90]
    parts = [vote_ref.clustered_boxes(n, seed=60 + i) for i, n in enumerate(sizes)]
    boxes = np.concatenate([p[0] for p in parts])
    scores = np.concatenate([p[1] for p in parts])
    offs = np.concatenate([[0], np.cumsum(sizes)]).tolist()
    n = offs[-1]
    from tinyfaces import ops
    b, s = guarded_like(torch.from_numpy(boxes), "cuda"), guarded_like(torch.from_numpy(scores), "cuda")      # inputs read out of range would show as NaN rows
    keeps = ops.nms_batched(b, s, offs, 0.3)
    counts = [int(k.numel()) for k in keeps]
    counts[1] = 0                                                            # a segment with boxes and num_keep = 0
    keep = torch.full((n,), -1, dtype=torch.int64, device="cuda")            # rows >= num_keep of the keep list hold no index
    for i, k in enumerate(keeps):
        keep[offs[i]: offs[i] + counts[i]] = k[:counts[i]]
    cnt = torch.tensor(counts, dtype=torch.int32, device="cuda")
    out, votes = guarded((n, 5), torch.float64, "cuda"), guarded((n,), torch.int32, "cuda")
    host = (C.c_int32 * 4)(*offs)
    hip.check(hip.lib().tf_box_vote_f64_batched(hip.ptr(b), hip.ptr(s), host, 3, hip.ptr(keep), hip.ptr(cnt), 0.5, 0, hip.ptr(out), hip.ptr(votes),
                                                hip.stream()), "tf_box_vote_f64_batched")
    torch.cuda.synchronize()
    assert_guards(out, "voted rows"); assert_guards(votes, "vote counts"); assert_guards(b, "boxes"); assert_guards(s, "scores")
    ref_rows, ref_votes = vote_ref.box_voting_batched(boxes, scores, offs, [k.cpu().numpy()[:c] for k, c in zip(keeps, counts)], 0.5)
    for i, (a, e) in enumerate(zip(offs, offs[1:])):
        c = counts[i]
        assert_written(out, slice(a, a + c), f"voted rows of segment {i}")
        assert_written(votes, slice(a, a + c), f"vote counts of segment {i}")
        assert unwritten(out, slice(a + c, e))[0] == (e - a - c) * 5, f"segment {i}: a row >= num_keep was written"
        assert unwritten(votes, slice(a + c, e))[0] == e - a - c, f"segment {i}: a vote count >= num_keep was written"
        assert np.array_equal(votes[a:a + c].cpu().numpy(), ref_votes[i])
        assert np.abs(out[a:a + c].cpu().numpy() - ref_rows[i]).max(initial=0.0) <= vote_ref.coordinate_bound(max(sizes), boxes)
    # the single-segment entry, votes_out = NULL
    out1 = guarded((sizes[0], 5), torch.float64, "cuda")
    hip.check(hip.lib().tf_box_vote_f64(hip.ptr(b), hip.ptr(s), sizes[0], hip.ptr(keep), hip.ptr(cnt), 0.5, 0, hip.ptr(out1), None, hip.stream()),
              "tf_box_vote_f64")
    torch.cuda.synchronize()
    assert_guards(out1, "voted rows (single)")
    assert torch.equal(out1[:counts[0]], out[:counts[0]]) and unwritten(out1, slice(counts[0], None))[0] == (sizes[0] - counts[0]) * 5


def test_unflip_writes_only_its_row_range(hip):
    rs = np.random.RandomState(5)
    rows = rs.uniform(-50, 3000, (300, 5))
    for first, last, max_rows in ((100, 163, 64), (100, 100, 64), (0, 300, 300), (37, 38, 1), (10, 200, 512)):
        d = guarded_like(torch.from_numpy(rows), "cuda")
        f, l = torch.tensor([first], dtype=torch.int32, device="cuda"), torch.tensor([last], dtype=torch.int32, device="cuda")
        hip.check(hip.lib().tf_boxes_unflip_f64(hip.ptr(d), hip.ptr(f), hip.ptr(l), max_rows, 1279.0, hip.stream()), "tf_boxes_unflip_f64")
        torch.cuda.synchronize()
        assert_guards(d, f"unflip [{first}, {last})")
        want = rows.copy()
        want[first:last] = vote_ref.unflip(rows[first:last], 1279.0)
        assert np.array_equal(d.cpu().numpy(), want), (first, last)


# --------------------------------------------------------------------------- case 5: the un-mirroring
def test_unflip_is_the_formula_and_nearly_an_involution():
    """x1' = c - x2, x2' = c - x1 bit for bit, on negative and large coordinates.  Twice with the same c returns every row to within one ulp of
    the largest magnitude involved (c, x, c - x) -- NOT exactly, by construction: c - (c - x) rounds twice, each time by at most half an ulp
    of its result."""
    from tinyfaces import ops
    rs = np.random.RandomState(9)
    rows = np.concatenate([rs.uniform(-1e3, 1e3, (400, 5)), rs.uniform(-1e7, 1e7, (300, 5)), rs.uniform(-1e-3, 1e-3, (300, 5))])
    c = (1280 - 1) * (1 / 0.3)
    d = _dev(rows)
    n = torch.tensor([0], dtype=torch.int32, device="cuda"), torch.tensor([rows.shape[0]], dtype=torch.int32, device="cuda")
    ops.boxes_unflip_(d, n[0], n[1], rows.shape[0], c)
    once = d.cpu().numpy()
    assert np.array_equal(once, vote_ref.unflip(rows, c))
    assert np.array_equal(once[:, [1, 3, 4]], rows[:, [1, 3, 4]])
    ops.boxes_unflip_(d, n[0], n[1], rows.shape[0], c)
    twice = d.cpu().numpy()
    x = rows[:, [0, 2]]
    ulp = np.spacing(np.maximum(np.maximum(np.abs(x), np.abs(c - x)), abs(c)))
    worst = float((np.abs(twice[:, [0, 2]] - x) / ulp).max())
    report("boxes_unflip[twice]", rows=rows.shape[0], worst_ulps=worst, exact=int((twice[:, [0, 2]] == x).all()))
    assert worst <= 1.0
    assert np.array_equal(twice[:, [1, 3, 4]], rows[:, [1, 3, 4]])


# --------------------------------------------------------------------------- cases 6 and 7: get_detections
@pytest.fixture(scope="module")
def detector(golden):
    """The fixture of tests/test_gpu_model.py: the product model with the oracle's tamed weights, fp32, on the golden `detections` image; the
    calls several tests share are made once."""
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


def test_get_detections_flip_candidates_and_kept_set(detector):
    from oracle.nms import nms as onms
    call, kw = detector["call"], detector["kw"]
    res0, cand0, keep0 = detector["plain"]
    res, cand, keep = detector["flip"]
    n0 = cand0.shape[0]
    assert n0 > 0 and cand.shape[0] > n0
    assert np.array_equal(cand[:n0], cand0)                                  # the unmirrored levels first: exactly today's candidate list
    # the rest: level by level the candidates of the MIRRORED IMAGE, mirrored back about c = (W_level - 1) * (1 / scale)
    h, w = detector["img"].shape[1:]
    want = []
    for sx in kw["scales"]:
        scale = 2 ** sx
        size = int(min(h, w) * scale)
        w_level = size if w <= h else int(size * w / h)
        _, cs, _ = call(detector["mirror"], scales=(sx,), return_candidates=True)
        want.append(vote_ref.unflip(cs, (w_level - 1) * (1 / scale)))
    want = np.concatenate(want)
    report("get_detections[flip]", candidates=n0, mirrored=cand.shape[0] - n0, kept=len(keep), kept_plain=len(keep0))
    assert np.array_equal(cand[n0:], want)
    assert np.array_equal(keep, onms(cand[:, :4], cand[:, 4], 0.3))          # ONE NMS over the union
    assert np.array_equal(res, cand[keep])
    # pyramid_on_gpu: the mirrored levels come from tf_image_prepare(flip=True) -- the same rows bit for bit
    res_g, cand_g, keep_g = call(detector["img"], flip=True, pyramid_on_gpu=True, return_candidates=True)
    assert np.array_equal(cand_g, cand) and np.array_equal(keep_g, keep) and np.array_equal(res_g, res)


def test_get_detections_batch_with_flip_and_voting_equals_the_loop(detector):
    from tinyfaces.evaluation import get_detections_batch
    d = detector
    imgs = [d["img"], d["mirror"]]
    for extra in (dict(flip=True), dict(flip=True, box_voting=0.5), dict(box_voting=0.5)):
        loop = [d["call"](im, **extra) for im in imgs]
        batch = get_detections_batch(d["model"], imgs, d["templates"], d["rf"], d["tf"], **d["kw"], **extra)
        assert len(batch) == 2 and all(np.array_equal(a, b) for a, b in zip(batch, loop)), extra
    assert np.array_equal(d["call"](d["img"], flip=True), d["flip"][0])


def test_get_detections_box_voting(detector):
    call = detector["call"]
    for flip in (False, True):
        res, cand, keep = call(detector["img"], flip=flip, box_voting=0.5, return_candidates=True)
        _, cand0, keep0 = detector["flip" if flip else "plain"]
        assert np.array_equal(cand, cand0) and np.array_equal(keep, keep0)   # the vote changes neither the candidates nor the kept set
        ref, votes = vote_ref.box_voting(cand[:, :4], cand[:, 4], keep, 0.5)                # sigmoid weights: the candidates' scores are logits
        dev, bound = float(np.abs(res[:, :4] - ref[:, :4]).max()), vote_ref.coordinate_bound(cand.shape[0], cand[:, :4])
        moved = int((res[:, :4] != cand[keep][:, :4]).any(axis=1).sum())
        report(f"get_detections[box_voting,flip={flip}]", candidates=cand.shape[0], kept=len(keep), moved=moved, max_votes=int(votes.max()),
               coord_maxabs=dev, coord_bound=bound)
        assert res.shape == (len(keep), 5) and dev <= bound and moved > 0
        assert np.array_equal(res[:, 4], cand[keep][:, 4])
    # both defaults: the call that does not name the keywords, bit for bit
    named = call(detector["img"], flip=False, box_voting=None, return_candidates=True)
    assert all(np.array_equal(a, b) for a, b in zip(named, detector["plain"]))


# --------------------------------------------------------------------------- case 8: evaluate_model.run
def test_evaluate_model_run_passes_the_keywords_through(tmp_path):
    import evaluate_model
    from bench import tame_init_
    from tinyfaces.evaluation import get_detections, write_results
    from tinyfaces.models.model import DetectionModel
    args = evaluate_model.tta_arguments(["synthetic", "--num-images", "2", "--workers", "0", "--flip", "--box-voting", "0.5"])
    loader, templates = evaluate_model.dataloader(args)
    device = torch.device("cuda")
    m = tame_init_(DetectionModel(num_objects=1, num_templates=25), seed=3).to(device).eval()
    # untrained scores sit at sigmoid(~0): a threshold only their tail passes, taken from one forward of the first image at full size
    img0 = next(iter(loader))[0][0]
    mean, std = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1), torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)
    with torch.no_grad():
        prob = torch.sigmoid(m(((img0 - mean) / std).unsqueeze(0).to(device))[0, :25].float()).flatten()
    thr = float(torch.quantile(prob, 0.999))
    with torch.no_grad(), m.constant_weights():
        evaluate_model.run(m, loader, templates, thr, 0.3, device, "val", results_dir=str(tmp_path / "run"), flip=args.flip, box_voting=args.box_voting)
        evaluate_model.run(m, loader, templates, thr, 0.3, device, "val", results_dir=str(tmp_path / "plain"))
        names = []
        for img, filename in loader:
            dets = get_detections(m, img[0], templates, loader.dataset.rf, loader.dataset.transforms, thr, 0.3, device=device, pyramid_on_gpu=True,
                                  flip=True, box_voting=0.5)
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
