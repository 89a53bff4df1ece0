"""-m gpu: the pre-NMS top-k selection (csrc/topk.hip: tf_topk_select_f64[_batched]; ops.topk_select[_batched]), the Soft-NMS cap
(tf_soft_nms_f64[_batched]_capped; ops.soft_nms_capped, ops.soft_nms_batched_capped) and get_detections / get_detections_batch / evaluate_model.run with pre_nms_topk= /
max_detections=, against the numpy restatement tests/topk_ref.py.

Every result of the selection and of the cap is an integer or a copied bit pattern: those comparisons are EQUALITY.  The only bounds in this file
are the ones the Soft-NMS and voting tests already use for the arithmetic BEHIND the cut (soft_nms_ref.score_bound, vote_ref.coordinate_bound),
applied to the reference run on the restatement's subset."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import soft_nms_ref
import topk_ref
import vote_ref
from gpu_util import report
from oracle.nms import nms as oracle_nms
from redzone import assert_guards, assert_written, guarded, guarded_like, guarded_workspace, unwritten

pytestmark = pytest.mark.gpu

# one row, two, a wave edge (63 / 64 / 65), one tile of 4 096 not full (257 / 1025), two tiles (4097), eighteen tiles with a ragged tail (70 001)
SIZES = [1, 2, 63, 64, 65, 257, 1025, 4097, 70001]
PATTERNS = ["logits", "three_values", "all_equal", "zeros", "inf", "nan_few", "nan_many", "subnormal", "low_byte", "sign_only"]
MARGIN = 1e-9


def _ks(n):
    return sorted({k for k in (1, 2, 64, n - 1, n, n + 1, 5000) if k >= 1})


def _dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C", copy=True))
    return (t if dtype is None else t.to(dtype)).cuda()


def _scores(pattern, n, k):
    rng = np.random.RandomState(1000 + n)
    if pattern == "logits":
        return vote_ref.clustered_boxes(n, seed=n)[1].copy()
    if pattern == "three_values":                                          # the threshold bucket is crowded; its ties span waves, tiles, blocks
        return rng.choice([-1.5, 0.25, 2.0], n)
    if pattern == "all_equal":
        return np.full(n, 0.7)
    if pattern == "zeros":
        return rng.choice([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], n)
    s = rng.normal(0.0, 2.0, n)
    if pattern == "inf":
        s[rng.rand(n) < 0.2] = np.inf
        s[rng.rand(n) < 0.2] = -np.inf
        return s
    if pattern in ("nan_few", "nan_many"):                                 # fewer NaNs than n - k: none is selected; more: some must be
        spare = max(n - k, 0)
        cnt = spare // 2 if pattern == "nan_few" else min(n, spare + (min(k, n) + 1) // 2)
        s[rng.permutation(n)[:cnt]] = np.nan
        if cnt >= 2:
            s[np.nonzero(np.isnan(s))[0][0]] = -np.nan                     # a NaN with the sign bit set as well
        return s
    if pattern == "subnormal":
        return rng.randint(-50, 51, n) * 5e-324
    if pattern == "low_byte":                                              # equal in the seven upper digits: every digit pass matters
        return (np.float64(1.0).view(np.uint64) + rng.randint(0, 256, n).astype(np.uint64)).view(np.float64)
    if pattern == "sign_only":
        return rng.choice([1.5, -1.5], n)
    raise ValueError(pattern)


def _select(s_dev, n, k):
    """ops.topk_select as a plain index array (None = the list is its own top-k)."""
    from tinyfaces import ops
    idx, new = ops.topk_select(s_dev, k)
    assert new == [0, min(n, k)]
    if idx is None:
        assert n <= k
        return np.arange(n, dtype=np.int64)
    assert idx.dtype == torch.int64 and idx.shape == (min(n, k),) and idx.is_cuda
    return idx.cpu().numpy()


# --------------------------------------------------------------------------- case 1: the select against the restatement
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_topk_select_vs_numpy(n, pattern):
    for k in _ks(n):
        s = _scores(pattern, n, k)
        got = _select(_dev(s), n, k)
        want = topk_ref.topk_select(s, k)
        assert np.array_equal(got, want), (n, pattern, k)
    report(f"topk_select[n={n},{pattern}]", ks=len(_ks(n)), equal=True)


def test_topk_select_across_many_blocks():
    """n = 2^21 + 5: 513 tiles of 4 096 rows, the last one holding five: the per-tile counts, their scan and the ordered write span
    hundreds of blocks."""
    n, k = 2 ** 21 + 5, 5000
    s = np.random.RandomState(21).normal(0.0, 2.0, n)
    s[-3:] = 50.0                                                          # the tail tile contributes
    s[::4099] = s[0]                                                       # ties spread over the tiles
    got = _select(_dev(s), n, k)
    want = topk_ref.topk_select(s, k)
    assert np.array_equal(got, want) and got[-1] == n - 1
    s3 = np.random.RandomState(22).choice([0.0, 1.0, 1.0, 2.0], n)         # the threshold value fills a quarter of two million rows
    assert np.array_equal(_select(_dev(s3), n, k), topk_ref.topk_select(s3, k))


# --------------------------------------------------------------------------- case 2: segments
def _segments(sizes, seed):
    rng = np.random.RandomState(seed)
    s = rng.normal(0.0, 2.0, int(sum(sizes)))
    s[rng.rand(s.size) < 0.3] = 0.5                                        # ties inside and across the segments
    return s, np.concatenate([[0], np.cumsum(sizes)]).astype(int).tolist()


@pytest.mark.parametrize("sizes,k", [((5000,), 700), ((1025, 0, 130), 300), (tuple(1 + (977 * i) % 9000 for i in range(64)), 2000)],
                         ids=["S1", "S3_empty_middle_one_short", "S64"])
def test_topk_batched_equals_single_calls(sizes, k):
    from tinyfaces import ops
    assert len(sizes) == 1 or (min(sizes) <= k < max(sizes))               # a segment that is passed through next to one that is cut
    s, offs = _segments(sizes, 300 + len(sizes))
    sd = _dev(s)
    idx, new = ops.topk_select_batched(sd, offs, k)
    assert new == np.concatenate([[0], np.cumsum([min(m, k) for m in sizes])]).tolist() and idx.shape == (new[-1],)
    for i, (a, b) in enumerate(zip(offs, offs[1:])):
        one = _select(sd[a:b], b - a, k) + a                                 # indices into the concatenated input
        assert np.array_equal(idx[new[i]:new[i + 1]].cpu().numpy(), one), i
    ref_idx, ref_new = topk_ref.topk_select_batched(s, offs, k)
    assert ref_new == new and np.array_equal(idx.cpu().numpy(), ref_idx)
    again, _ = ops.topk_select_batched(sd, offs, k)                        # a second run: the same bits
    assert torch.equal(again, idx)
    # nothing to cut: nothing is launched, the list is its own top-k
    none, same = ops.topk_select_batched(sd, offs, max(sizes))
    assert none is None and same == offs


# --------------------------------------------------------------------------- case 3: the write contract
@pytest.mark.parametrize("n", [65, 1025, 70001])
def test_topk_writes_only_what_it_selects(hip, n):
    l = hip.lib()
    s = _scores("three_values", n, n // 3)
    sd = guarded_like(torch.from_numpy(s.copy()), "cuda")
    for sizes, k in (((n,), n // 3), ((n,), n + 7), ((n - 40, 0, 40), 33)):
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int).tolist()
        S, m = len(sizes), sum(min(x, k) for x in sizes)
        host = (C.c_int32 * (S + 1))(*offs)
        idx = guarded((n + 16,), torch.int64, "cuda")                        # longer than sum m_s: the rows beyond must stay untouched
        wsb = l.tf_topk_batched_workspace_bytes(host, S, k)
        assert wsb > 0
        ws = guarded_workspace(wsb, "cuda")
        hip.check(l.tf_topk_select_f64_batched(hip.ptr(sd), host, S, k, hip.ptr(idx), hip.ptr(ws), wsb, hip.stream()), "tf_topk_select_f64_batched")
        torch.cuda.synchronize()
        for t, what in ((idx, "idx_out"), (ws, "workspace"), (sd, "scores")):
            assert_guards(t, f"{what} (n={n}, sizes={sizes}, k={k})")
        assert_written(idx, slice(0, m), "selected indices")
        assert unwritten(idx, slice(m, None))[0] == n + 16 - m, "a row of idx_out beyond sum m_s was written"
        assert np.array_equal(idx[:m].cpu().numpy(), topk_ref.topk_select_batched(s, offs, k)[0])
        assert np.array_equal(sd.cpu().numpy(), s)                             # scores is only read
        short = l.tf_topk_select_f64_batched(hip.ptr(sd), host, S, k, hip.ptr(idx), hip.ptr(ws), wsb - 1, hip.stream())
        assert short == -1                                                     # TF_ERR_ARG, nothing launched


# --------------------------------------------------------------------------- case 4: the hard-NMS identity on the device
@pytest.mark.parametrize("n", [65, 1025, 4097])
def test_cut_commutes_with_the_hard_nms_on_the_device(n):
    from tinyfaces import ops
    boxes, scores = vote_ref.clustered_boxes(n, seed=n)
    b, s = _dev(boxes), _dev(scores)
    full = ops.nms(b, s, 0.3).cpu().numpy()
    rank = np.empty(n, np.int64)
    rank[topk_ref.order(scores)] = np.arange(n)
    for k in sorted({1, 2, 64, n // 3, n - 1, n, n + 1}):
        idx = torch.from_numpy(_select(s, n, k)).cuda()
        got = idx[ops.nms(b[idx], s[idx], 0.3)].cpu().numpy()
        want = full[rank[full] < k]
        assert np.array_equal(got, want), (n, k)
        assert np.array_equal(want, full[:want.size])                      # ... and those are a prefix of the uncut keep list


# --------------------------------------------------------------------------- case 5: the lifted limit
def test_a_list_too_long_for_the_nms_is_cut_to_one_it_takes():
    from tinyfaces import ops
    n, K = 600000, 5000
    assert n > ops.NMS_MAX_BOXES
    boxes, scores = vote_ref.clustered_boxes(n, seed=6)
    b, s = _dev(boxes), _dev(scores)
    with pytest.raises(RuntimeError):
        ops.nms(b, s, 0.3)                                                 # the plain call is refused
    idx, new = ops.topk_select(s, K)
    assert new == [0, K]
    want = topk_ref.topk_select(scores, K)
    assert np.array_equal(idx.cpu().numpy(), want)
    keep = idx[ops.nms(b[idx], s[idx], 0.3)].cpu().numpy()
    assert np.array_equal(keep, want[oracle_nms(boxes[want], scores[want], 0.3)]) and keep.size > 0


# --------------------------------------------------------------------------- case 6: the Soft-NMS cap
@functools.lru_cache(maxsize=None)
def _soft_inputs(n):
    boxes, logits = vote_ref.clustered_boxes(n, seed=n)
    boxes.setflags(write=False); logits.setflags(write=False)
    return boxes, logits


@pytest.mark.parametrize("method", ["linear", "gaussian"])
@pytest.mark.parametrize("n", [65, 1025, 4097])
def test_soft_nms_cap_returns_the_first_rows_of_the_uncapped_run(hip, n, method):
    from tinyfaces import ops
    boxes, logits = _soft_inputs(n)
    b, s = _dev(boxes), _dev(logits)
    keep, kept = ops.soft_nms(b, s, method, 0.3, 0.5, 0.3)
    K = int(keep.numel())
    assert 1 < K < n
    mid = ops.SOFT_NMS_METHODS[method]
    bg, sg = guarded_like(torch.from_numpy(boxes.copy()), "cuda"), guarded_like(torch.from_numpy(logits.copy()), "cuda")
    for mk in sorted({1, min(64, K), K, K + 1}):
        c = min(K, mk)
        ck, cs = ops.soft_nms_capped(b, s, mk, method, 0.3, 0.5, 0.3)
        assert ck.shape == (c,) and torch.equal(ck, keep[:c]) and torch.equal(cs, kept[:c]), (n, method, mk)
        # the C entry between guard bands: num_keep is the capped count and no row beyond it is written
        ko, so = guarded((n,), torch.int64, "cuda"), guarded((n,), torch.float64, "cuda")
        cnt = guarded((1,), torch.int32, "cuda")
        cnt.zero_()
        wsb = hip.lib().tf_soft_nms_workspace_bytes(n)
        ws = guarded_workspace(wsb, "cuda", pitch_bytes=((n + 63) // 64) * 8)
        hip.check(hip.lib().tf_soft_nms_f64_capped(hip.ptr(bg), hip.ptr(sg), n, mid, 0.3, 0.5, 0.3, 0, mk, hip.ptr(ko), hip.ptr(so), hip.ptr(cnt),
                                                   hip.ptr(ws), wsb, hip.stream()), "tf_soft_nms_f64_capped")
        torch.cuda.synchronize()
        for t, what in ((ko, "keep_out"), (so, "score_out"), (cnt, "num_keep"), (ws, "workspace"), (bg, "boxes"), (sg, "scores")):
            assert_guards(t, f"{what} ({method}, n={n}, max_keep={mk})")
        assert int(cnt.item()) == c
        assert_written(ko, slice(0, c), "kept indices"); assert_written(so, slice(0, c), "kept scores")
        assert unwritten(ko, slice(c, None))[0] == n - c, "a keep row beyond the capped count was written"
        assert unwritten(so, slice(c, None))[0] == n - c, "a score row beyond the capped count was written"
        assert torch.equal(ko[:c], keep[:c]) and torch.equal(so[:c], kept[:c])
    report(f"soft_nms_cap[n={n},{method}]", uncapped=K, equal=True)


def test_soft_nms_cap_batched_with_the_chained_vote():
    from tinyfaces import ops
    sizes = (130, 0, 1025)
    parts = [vote_ref.clustered_boxes(m, seed=80 + i) for i, m in enumerate(sizes)]
    boxes = np.concatenate([p[0].reshape(-1, 4) for p in parts])
    scores = np.concatenate([p[1] for p in parts])
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int).tolist()
    b, s = _dev(boxes), _dev(scores)
    for method in ("linear", "gaussian"):
        res, rows = ops.soft_nms_batched(b, s, offs, method, vote=(0.5, "sigmoid"))
        counts = [int(k.numel()) for k, _ in res]
        assert counts[1] == 0 and min(counts[0], counts[2]) >= 4
        mk = min(counts[0], counts[2]) // 2                                # a cap that binds in both non-empty segments
        cres, crows = ops.soft_nms_batched_capped(b, s, offs, mk, method, vote=(0.5, "sigmoid"))
        plain = ops.soft_nms_batched_capped(b, s, offs, mk, method)
        split, srows = ops.soft_nms_batched_capped(b, s, offs, mk, method, mask_budget_bytes=1, vote=(0.5, "sigmoid"))
        for i in range(3):
            c = min(counts[i], mk)
            assert cres[i][0].shape == (c,) and crows[i].shape == (c, 5)
            assert torch.equal(cres[i][0], res[i][0][:c]) and torch.equal(cres[i][1], res[i][1][:c])
            assert torch.equal(crows[i], rows[i][:c])                        # the voted rows are the uncapped call's first rows
            assert torch.equal(plain[i][0], res[i][0][:c]) and torch.equal(plain[i][1], res[i][1][:c])
            assert torch.equal(split[i][0], cres[i][0]) and torch.equal(srows[i], crows[i])


# --------------------------------------------------------------------------- case 7: get_detections
@pytest.fixture(scope="module")
def detector(golden):
    """The fixture of tests/test_gpu_soft_nms.py, rebuilt: the product model with the oracle's tamed weights, fp32, on the golden `detections`
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


def test_get_detections_limits_that_do_not_bind_change_nothing(detector):
    d = detector
    res, cand, keep = d["plain"]
    N, kept = cand.shape[0], keep.shape[0]
    assert N >= 8 and kept >= 4
    for extra in (dict(pre_nms_topk=None, max_detections=None), dict(pre_nms_topk=N), dict(pre_nms_topk=N + 1000), dict(max_detections=kept),
                  dict(max_detections=kept + 5), dict(pre_nms_topk=N, max_detections=kept)):
        got = d["call"](d["img"], return_candidates=True, **extra)
        assert all(np.array_equal(a, b) for a, b in zip(got, d["plain"])), extra
    got = d["call"](d["img"], flip=True, pre_nms_topk=d["flip"][1].shape[0], return_candidates=True)
    assert all(np.array_equal(a, b) for a, b in zip(got, d["flip"]))


def test_get_detections_pre_nms_topk(detector):
    d = detector
    res0, cand0, keep0 = d["plain"]
    N = cand0.shape[0]
    assert N >= 8
    K = N // 2
    res, cand, keep = d["call"](d["img"], pre_nms_topk=K, return_candidates=True)
    assert np.array_equal(cand, cand0)                                     # the full candidate list still comes back ...
    idx = topk_ref.topk_select(cand0[:, 4], K)
    want_keep = idx[oracle_nms(cand0[idx, :4], cand0[idx, 4], 0.3)]
    assert np.array_equal(keep, want_keep)                                 # ... and keep indexes it
    assert np.array_equal(res, cand0[want_keep])
    rank = np.empty(N, np.int64)
    rank[topk_ref.order(cand0[:, 4])] = np.arange(N)
    assert np.array_equal(keep, keep0[rank[keep0] < K])                    # the rows of the uncut call whose candidate ranks below K
    report("get_detections[pre_nms_topk]", candidates=N, K=K, kept=len(keep), kept_uncut=len(keep0))
    assert np.array_equal(d["call"](d["img"], pre_nms_topk=K), res)


def test_get_detections_max_detections(detector):
    d = detector
    res0, cand0, keep0 = d["plain"]
    assert keep0.shape[0] > 3
    res, cand, keep = d["call"](d["img"], max_detections=3, return_candidates=True)
    assert np.array_equal(res, res0[:3]) and np.array_equal(keep, keep0[:3]) and np.array_equal(cand, cand0)
    voted0 = d["call"](d["img"], box_voting=0.5)
    voted = d["call"](d["img"], box_voting=0.5, max_detections=3)
    assert voted.shape == (3, 5) and np.array_equal(voted, voted0[:3])
    for method in ("linear", "gaussian"):
        soft0, _, skeep0 = d["call"](d["img"], soft_nms=method, return_candidates=True)
        soft, _, skeep = d["call"](d["img"], soft_nms=method, max_detections=3, return_candidates=True)
        assert soft0.shape[0] > 3 and np.array_equal(soft, soft0[:3]) and np.array_equal(skeep, skeep0[:3])
        sv0 = d["call"](d["img"], soft_nms=method, box_voting=0.5)
        sv = d["call"](d["img"], soft_nms=method, box_voting=0.5, max_detections=3)
        assert np.array_equal(sv, sv0[:3])


@pytest.mark.parametrize("method", ["linear", "gaussian"])
def test_get_detections_soft_nms_on_the_cut_list(detector, method):
    d = detector
    _, cand0, _ = d["plain"]
    N = cand0.shape[0]
    assert N >= 8
    K = N // 2
    res, cand, keep = d["call"](d["img"], soft_nms=method, pre_nms_topk=K, return_candidates=True)
    assert np.array_equal(cand, cand0)
    idx = topk_ref.topk_select(cand0[:, 4], K)
    ref_keep, ref_scores, rank_margin, thresh_margin = soft_nms_ref.soft_nms(cand0[idx, :4], cand0[idx, 4], method, 0.3, 0.5, 0.001)
    # a condition on the INPUTS: no decision of the reference run on the subset is within reach of a last-bit difference
    assert rank_margin >= MARGIN and thresh_margin >= MARGIN, (rank_margin, thresh_margin)
    bound = soft_nms_ref.score_bound(len(ref_keep))
    same = bool(np.array_equal(keep, idx[ref_keep]))
    assert len(ref_keep) > 0
    den = np.where(ref_scores != 0, np.abs(ref_scores), 1.0)
    dev = float((np.abs(res[:, 4] - ref_scores) / den).max()) if same else float("nan")
    report(f"get_detections[soft_nms={method},pre_nms_topk]", candidates=N, K=K, kept=len(keep), keep_equal=same, score_maxrel=dev,
           score_bound=bound, rank_margin=rank_margin, thresh_margin=thresh_margin)
    print(f"get_detections soft_nms={method} pre_nms_topk={K} of {N}: kept {len(keep)} score_maxrel {dev:.3e} bound {bound:.3e} "
          f"margins {rank_margin:.3e} {thresh_margin:.3e}")
    assert same
    assert np.array_equal(res[:, :4], cand0[keep][:, :4])
    assert dev <= bound
    capped = d["call"](d["img"], soft_nms=method, pre_nms_topk=K, max_detections=2)
    assert np.array_equal(capped, res[:2])


def test_get_detections_flip_and_box_voting_on_the_cut_list(detector):
    d = detector
    _, cand0, _ = d["flip"]
    N = cand0.shape[0]
    assert N >= 8
    K = N // 2                                                             # the cut applies to the union of plain and mirrored candidates
    res, cand, keep = d["call"](d["img"], flip=True, box_voting=0.5, pre_nms_topk=K, return_candidates=True)
    assert np.array_equal(cand, cand0)
    idx = topk_ref.topk_select(cand0[:, 4], K)
    sub = cand0[idx]
    sub_keep = oracle_nms(sub[:, :4], sub[:, 4], 0.3)
    assert np.array_equal(keep, idx[sub_keep])
    ref, votes = vote_ref.box_voting(sub[:, :4], sub[:, 4], sub_keep, 0.5)  # the voters are the K retained candidates
    dev, bound = float(np.abs(res[:, :4] - ref[:, :4]).max()), vote_ref.coordinate_bound(K, sub[:, :4])
    moved = int((res[:, :4] != cand0[keep][:, :4]).any(axis=1).sum())
    report("get_detections[flip,box_voting,pre_nms_topk]", candidates=N, K=K, kept=len(keep), moved=moved, coord_maxabs=dev, coord_bound=bound)
    print(f"get_detections flip box_voting pre_nms_topk={K} of {N}: kept {len(keep)} moved {moved} coord_maxabs {dev:.3e} bound {bound:.3e}")
    assert res.shape == (len(keep), 5) and dev <= bound and moved > 0
    assert np.array_equal(res[:, 4], cand0[keep][:, 4])                    # the kept box's own score is carried through


def test_get_detections_batch_with_the_limits_equals_the_loop(detector):
    from tinyfaces.evaluation import get_detections_batch
    d = detector
    N = d["plain"][1].shape[0]
    imgs = [d["img"], d["mirror"]]
    for extra in (dict(pre_nms_topk=N // 2), dict(max_detections=3), dict(pre_nms_topk=N // 2, max_detections=2, box_voting=0.5),
                  dict(soft_nms="linear", pre_nms_topk=N // 2, max_detections=3), dict(soft_nms="gaussian", flip=True, pre_nms_topk=N // 3),
                  dict(soft_nms="gaussian", box_voting=0.5, max_detections=2), dict(pre_nms_topk=10 * N, max_detections=10 * N)):
        loop = [d["call"](im, **extra) for im in imgs]
        batch = get_detections_batch(d["model"], imgs, d["templates"], d["rf"], d["tf"], **d["kw"], **extra)
        assert len(batch) == 2 and all(np.array_equal(a, b) for a, b in zip(batch, loop)), extra
        assert loop[0].shape[0] > 0
    batch = get_detections_batch(d["model"], [d["img"]], d["templates"], d["rf"], d["tf"], **d["kw"], pre_nms_topk=None, max_detections=None)
    assert np.array_equal(batch[0], d["plain"][0])


# --------------------------------------------------------------------------- case 8: evaluate_model.run
def test_evaluate_model_run_passes_the_limits_through(tmp_path):
    import evaluate_model
    from bench import tame_init_
    from tinyfaces.evaluation import get_detections, write_results
    from tinyfaces.models.model import DetectionModel
    args = evaluate_model.limits_arguments(["synthetic", "--num-images", "2", "--workers", "0", "--pre-nms-topk", "40", "--max-detections", "5"])
    assert (args.pre_nms_topk, args.max_detections) == (40, 5)
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
        evaluate_model.run(m, loader, templates, thr, 0.3, device, "val", results_dir=str(tmp_path / "run"),
                           pre_nms_topk=args.pre_nms_topk, max_detections=args.max_detections)
        evaluate_model.run(m, loader, templates, thr, 0.3, device, "val", results_dir=str(tmp_path / "plain"))
        names = []
        for img, filename in loader:
            dets = get_detections(m, img[0], templates, loader.dataset.rf, loader.dataset.transforms, thr, 0.3, device=device, pyramid_on_gpu=True,
                                  pre_nms_topk=40, max_detections=5)
            write_results(dets, filename[0], "val", str(tmp_path / "direct"))
            names.append(filename[0].replace("jpg", "txt"))
    assert len(names) == 2
    differs = 0
    for name in names:
        got, want = (tmp_path / "run" / name).read_text(), (tmp_path / "direct" / name).read_text()
        assert got == want, name
        assert 0 < int(got.split("\n")[1]) <= 5
        differs += got != (tmp_path / "plain" / name).read_text()
    assert differs                                                         # the keywords did arrive: the plain run writes other rows
