"""Float64 numpy restatement of Matrix NMS (csrc/matrix_nms.hip; Wang et al., SOLOv2, NeurIPS 2020; PaddleDetection's matrix_nms) as
include/tinyfaces_hip.h states it, written from that definition.  Test infrastructure: a plain loop over the ranked candidates with the IoU of
tests/vote_ref.py (oracle/nms.py's: areas without +1, inter / (a_i + a_j - inter)); never imported by the package.

Besides the kept indices and their scores `matrix_nms` returns two MARGINS of its own run, which say how far the input is from a case where a
last-bit difference (the device's exp against numpy's, in the sigmoid or in the gaussian factor) could change a decision:
  gap_margin     the smallest relative gap (a - b) / a between neighbouring emitted scores s that are not bit-equal (a bit-equal pair is
                 ordered by rank, not by rounding) -- and, stricter than the emission alone needs, between neighbouring admitted p as well,
                 since the rank, and with it every comp and every factor, hangs on the order of the p;
  thresh_margin  the smallest relative distance |v - score_thresh| / score_thresh of any s_j, and of any p_i (the admission test), to the
                 threshold (inf for score_thresh == 0: a product of non-negative factors cannot round below 0)."""
import numpy as np

import vote_ref

METHODS = ("linear", "gaussian")


def _gaps(sorted_desc):
    """Smallest (a - b) / a over neighbours a > b of a descending array (finite, a > 0); inf when there is none."""
    v = np.asarray(sorted_desc, dtype=np.float64)
    if v.size < 2:
        return np.inf
    a, b = v[:-1], v[1:]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = (a != b) & np.isfinite(a) & np.isfinite(b) & (a > 0)
        g = (a[ok] - b[ok]) / a[ok]
    return float(g.min()) if g.size else np.inf


def _distance(values, thr):
    v = np.asarray(values, dtype=np.float64)
    v = v[np.isfinite(v)]
    if not thr > 0 or v.size == 0:
        return np.inf
    return float((np.abs(v - thr) / thr).min())


def iou_row(box, better):
    """iou(i, j) of candidate j (`box`) with the better-ranked candidates `better`: inter == 0 or a NaN quotient counts as 0."""
    o = vote_ref.iou_one_to_many(box, better)
    return np.where(np.isnan(o), 0.0, o)


def ranked(boxes, scores, score_thresh=0.001, score="sigmoid"):
    """Steps 1, 2 and 4 of the definition, which do not depend on the method: (order (input indices in rank order), p_all, comp)."""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    p_all = vote_ref.weights(np.asarray(scores, dtype=np.float64).reshape(-1), score)
    # 1 admission, 2 rank: p descending, the lower input index first (a stable sort; -0.0 == +0.0)
    with np.errstate(invalid="ignore"):
        idx = np.nonzero(p_all >= np.float64(score_thresh))[0]
    order = idx[np.argsort(-p_all[idx], kind="stable")]
    b = boxes[order]
    comp = np.zeros(order.size)
    # 4 compensation: comp_j = max_{i<j} iou(i, j)
    for j in range(1, order.size):
        comp[j] = iou_row(b[j], b[:j]).max()
    return order, p_all, comp


def matrix_nms(boxes, scores, method="gaussian", sigma=0.5, score_thresh=0.001, score="sigmoid", max_keep=None, details=False, rank=None):
    """-> (keep int64 (K,), kept scores float64 (K,), gap_margin, thresh_margin), rows by s descending, the better rank first on an equal s.
    details=True appends a dict of the run in RANK order: order (input index), p, comp, arg (the minimum itself for the linear method, x for the
    gaussian), d, s, emitted.  rank: what `ranked` returned for the same boxes, scores, score_thresh and score (shared between the methods)."""
    if method not in METHODS:
        raise ValueError(method)
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    thr, sigma = np.float64(score_thresh), np.float64(sigma)
    order, p_all, comp = ranked(boxes, scores, score_thresh, score) if rank is None else rank
    b, p = boxes[order], p_all[order]
    m = order.size
    arg, d = np.zeros(m), np.ones(m)
    if method == "linear":
        arg[:] = 1.0
    # 5 decay
    for j in range(1, m):
        o, c = iou_row(b[j], b[:j]), comp[:j]
        if method == "linear":
            sel = c < 1.0                                       # comp_i >= 1: an exact duplicate of a better box, no term
            arg[j] = ((1.0 - o[sel]) / (1.0 - c[sel])).min()    # rank 0 is always in sel
            d[j] = arg[j]
        else:
            arg[j] = (o * o - c * c).max()
            d[j] = np.exp(-arg[j] / sigma)                      # ONE exp, on the extremal argument
    # 6 emission
    with np.errstate(invalid="ignore"):
        s = p * d
        emitted = s >= thr
    e = np.nonzero(emitted)[0]
    rows = e[np.argsort(-s[e], kind="stable")]                  # s descending, the better rank first
    gap = min(_gaps(s[rows]), _gaps(p))
    dist = min(_distance(s, thr), _distance(p_all, thr))
    if max_keep is not None:
        rows = rows[:int(max_keep)]
    res = (order[rows].astype(np.int64), s[rows].astype(np.float64), gap, dist)
    if details:
        res += ({"order": order, "p": p, "comp": comp, "arg": arg, "d": d, "s": s, "emitted": emitted, "rows": rows},)
    return res


def decay_by_min_of_exponentials(boxes_ranked, comp, sigma):
    """SOLOv2's own form of the gaussian factor, min_i exp(-(iou^2 - comp_i^2) / sigma), for boxes already in rank order: what the one-exp
    form must equal."""
    m = len(comp)
    d = np.ones(m)
    for j in range(1, m):
        o, c = iou_row(boxes_ranked[j], boxes_ranked[:j]), comp[:j]
        d[j] = np.exp(-(o * o - c * c) / np.float64(sigma)).min()
    return d


def matrix_nms_batched(boxes, scores, seg_offsets, **kw):
    """Per segment; keep indexes the concatenated input, as ops.matrix_nms_batched returns it."""
    boxes, scores = np.asarray(boxes, dtype=np.float64).reshape(-1, 4), np.asarray(scores, dtype=np.float64).reshape(-1)
    res = []
    for a, b in zip(seg_offsets, seg_offsets[1:]):
        r = matrix_nms(boxes[a:b], scores[a:b], **kw)
        res.append((r[0] + a,) + tuple(r[1:]))
    return res
