"""Float64 numpy restatement of Soft-NMS (csrc/soft_nms.hip; Bodla et al., ICCV 2017; Detectron's soft_nms) as include/tinyfaces_hip.h states it.
Test infrastructure: a plain loop over the selections with the IoU of tests/vote_ref.py (oracle/nms.py's: areas without +1,
inter / (a_m + a_j - inter)); never imported by the package.

Besides the kept indices and their scores `soft_nms` returns two MARGINS of its own run, which say how far the input is from a case where
a last-bit difference (the device's exp against numpy's) could change a decision:
  rank_margin    the smallest relative gap (s_m - s_2) / s_m between a selected score and the runner-up, over the selections whose
                 runner-up is not bit-equal (a bit-equal tie is decided by the index, not by rounding);
  thresh_margin  the smallest relative distance |s - score_thresh| / score_thresh of any score to the threshold at any liveness test
                 (inf for score_thresh == 0: a product of non-negative factors cannot round below 0)."""
import numpy as np

import vote_ref

METHODS = ("linear", "gaussian")


def soft_nms(boxes, scores, method="linear", iou_thresh=0.3, sigma=0.5, score_thresh=0.001, score="sigmoid"):
    """-> (keep int64 (K,), kept scores float64 (K,), rank_margin, thresh_margin), keep in selection order."""
    if method not in METHODS:
        raise ValueError(method)
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    s = vote_ref.weights(np.asarray(scores, dtype=np.float64).reshape(-1), score)
    thr, iou_thr, sigma = np.float64(score_thresh), np.float64(iou_thresh), np.float64(sigma)
    margins = {"rank": np.inf, "thresh": np.inf}

    def alive(v):
        """The liveness test s >= score_thresh (a NaN fails it), noting how close it was."""
        v = np.asarray(v, dtype=np.float64)
        if thr > 0 and v.size:
            with np.errstate(invalid="ignore", over="ignore"):
                d = np.abs(v - thr) / thr
            d = d[~np.isnan(d)]
            if d.size:
                margins["thresh"] = min(margins["thresh"], float(d.min()))
        with np.errstate(invalid="ignore"):
            return v >= thr

    live = alive(s)
    keep, kept = [], []
    for _ in range(s.size):
        idx = np.nonzero(live)[0]
        if idx.size == 0:
            break
        vals = s[idx]
        top = int(np.argmax(vals))                           # the first maximum: the lowest input index on a bit-equal tie
        m, sm = int(idx[top]), vals[top]
        if idx.size > 1:
            second = np.delete(vals, top).max()
            if second != sm and sm > 0:
                margins["rank"] = min(margins["rank"], float((sm - second) / sm))
        keep.append(m)
        kept.append(sm)
        live[m] = False
        ovr = vote_ref.iou_one_to_many(boxes[m], boxes)      # NaN for 0 / 0; 0 wherever inter == 0
        with np.errstate(invalid="ignore"):
            if method == "linear":
                sel = live & (ovr > iou_thr)
                factor = 1.0 - ovr[sel]
            else:
                sel = live & (ovr > 0)
                factor = np.exp(-(ovr[sel] * ovr[sel]) / sigma)
        if sel.any():
            s[sel] = s[sel] * factor
            live[sel] = alive(s[sel])
    return np.asarray(keep, dtype=np.int64), np.asarray(kept, dtype=np.float64), margins["rank"], margins["thresh"]


def soft_nms_batched(boxes, scores, seg_offsets, **kw):
    """Per segment; keep indexes the concatenated input, as ops.soft_nms_batched returns it."""
    boxes, scores = np.asarray(boxes, dtype=np.float64).reshape(-1, 4), np.asarray(scores, dtype=np.float64).reshape(-1)
    res = []
    for a, b in zip(seg_offsets, seg_offsets[1:]):
        k, sc, rm, tm = soft_nms(boxes[a:b], scores[a:b], **kw)
        res.append((k + a, sc, rm, tm))
    return res


def score_bound(kept):
    """Relative bound on a kept score against this restatement: 8 * (K + 2) * 2^-52 for K kept boxes -- a score carries at most K factors, each
    with a couple of ulps of exp plus the multiply, on top of the sigmoid."""
    return 8.0 * (int(kept) + 2) * 2.0 ** -52
