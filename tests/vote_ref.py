"""Float64 numpy restatement of the test-time augmentation kernels (csrc/vote.hip): box voting (Gidaris & Komodakis, ICCV 2015; Detectron's
box_voting with scoring method ID) and the un-mirroring of a flipped pyramid level.  Test infrastructure: a plain loop over the kept boxes with
the IoU of oracle/nms.py (areas without +1, inter / (a_k + a_j - inter)); never imported by the package.  Also the seeded generator of
clustered candidate lists the GPU tests and scripts/tta_numbers.py share."""
import numpy as np


def iou_one_to_many(box, boxes):
    """IoU of `box` (4,) with every row of `boxes` (n, 4): oracle/nms.py's expression in its operation order (NaN for 0 / 0)."""
    zero = boxes.dtype.type(0)
    area = (box[2] - box[0]) * (box[3] - box[1])
    areas = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    xx1 = np.maximum(box[0], boxes[:, 0])
    yy1 = np.maximum(box[1], boxes[:, 1])
    xx2 = np.minimum(box[2], boxes[:, 2])
    yy2 = np.minimum(box[3], boxes[:, 3])
    w = np.maximum(zero, xx2 - xx1)
    h = np.maximum(zero, yy2 - yy1)
    inter = w * h
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / (area + areas - inter)


def weights(scores, weight="sigmoid"):
    scores = np.asarray(scores, dtype=np.float64)
    if weight == "sigmoid":
        with np.errstate(over="ignore"):
            return 1.0 / (1.0 + np.exp(-scores))
    if weight == "score":
        return scores.copy()
    raise ValueError(weight)


def box_voting(boxes, scores, keep, vote_thresh, weight="sigmoid"):
    """(K, 5) voted rows in keep order and (K,) int32 vote counts.  Row r: the weighted mean of every candidate j with
    IoU(box_keep[r], box_j) >= vote_thresh (a NaN IoU is no vote) and a weight > 0 (NaN weights dropped), and the kept box's own score;
    the kept box unchanged when nobody votes or the weight sum is not > 0."""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    scores = np.asarray(scores, dtype=np.float64).reshape(-1)
    keep = np.asarray(keep, dtype=np.int64).reshape(-1)
    w_all = weights(scores, weight)
    out = np.empty((keep.size, 5), dtype=np.float64)
    votes = np.zeros(keep.size, dtype=np.int32)
    thr = np.float64(vote_thresh)
    for r, k in enumerate(keep):
        iou = iou_one_to_many(boxes[k], boxes)
        with np.errstate(invalid="ignore"):
            v = (iou >= thr) & (w_all > 0)
        idx = np.nonzero(v)[0]
        sw = w_all[idx].sum()
        if idx.size and sw > 0:
            out[r, :4] = (w_all[idx, None] * boxes[idx]).sum(axis=0) / sw
        else:
            out[r, :4] = boxes[k]
        out[r, 4] = scores[k]
        votes[r] = idx.size
    return out, votes


def box_voting_batched(boxes, scores, seg_offsets, keeps, vote_thresh, weight="sigmoid"):
    """Per segment (keeps: indices into the concatenated input, as ops.nms_batched returns them)."""
    boxes, scores = np.asarray(boxes, dtype=np.float64), np.asarray(scores, dtype=np.float64)
    res = []
    for a, b, k in zip(seg_offsets, seg_offsets[1:], keeps):
        res.append(box_voting(boxes[a:b], scores[a:b], np.asarray(k, dtype=np.int64) - a, vote_thresh, weight))
    return [r[0] for r in res], [r[1] for r in res]


def unflip(dets, c):
    """Rows (x1, y1, x2, y2, score) mirrored about c: x1' = c - x2, x2' = c - x1; everything else as it is.  A new array."""
    out = np.array(dets, dtype=np.float64, copy=True)
    c = np.float64(c)
    out[:, 0] = c - np.asarray(dets)[:, 2]
    out[:, 2] = c - np.asarray(dets)[:, 0]
    return out


def coordinate_bound(n, boxes):
    """n * 2^-52 * max|coordinate|: at most n products and n sums per coordinate, each rounded once, plus ~3 ulp per sigmoid weight on either
    side of the quotient (the device's exp and numpy's differ in the last bits)."""
    boxes = np.asarray(boxes)
    return n * 2.0 ** -52 * (float(np.abs(boxes).max()) if boxes.size else 0.0)


def clustered_boxes(n, seed=0):
    """Seeded candidate list in the shape of a detector's: clusters of near-duplicates (centres in [-20, 1500], so some coordinates are
    negative; sizes 8..120; jitter 0.08 x size), score ties in the first rows, one exact duplicate, one zero-area box.  The zero-area
    box survives the NMS (its IoU with anything is 0 or NaN) and gets no vote."""
    rng = np.random.RandomState(seed)
    nc = max(1, n // 24)
    cx, cy = rng.uniform(-20, 1500, nc), rng.uniform(-20, 1500, nc)
    cx[0], cy[0] = -12.0, -6.0                                            # one cluster across the origin: negative coordinates at every n
    size = rng.uniform(8, 120, nc)
    which = rng.randint(0, nc, n)
    which[:3] = 0
    s = size[which]
    jx, jy = rng.normal(0, 0.08, n) * s, rng.normal(0, 0.08, n) * s
    w, h = s * rng.uniform(0.9, 1.1, n), s * rng.uniform(0.9, 1.1, n)
    x1, y1 = cx[which] + jx - w / 2, cy[which] + jy - h / 2
    boxes = np.stack([x1, y1, x1 + w, y1 + h], axis=1).astype(np.float64)
    scores = rng.normal(0.0, 2.0, n).astype(np.float64)               # logits
    if n >= 4:
        scores[:4] = scores[0]                                            # ties: the stable order decides
    if n >= 8:
        boxes[7] = boxes[5]                                               # one exact duplicate (IoU exactly 1)
    if n >= 16:
        boxes[11, 2] = boxes[11, 0]                                       # one zero-area box
        scores[11] = 9.0
    return boxes, scores
