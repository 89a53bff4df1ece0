"""Restatement of `torchvision.ops.nms` CPU kernel semantics (torchvision 0.18,
csrc/ops/cpu/nms_kernel.cpp -- third-party, NOT in /root/reference; PARITY UNPINNED).

Call site in the reference: tinyfaces/evaluation.py:84 with float64 boxes/scores.

Semantics restated:
  areas = (x2-x1)*(y2-y1)                      (no +1)
  order = argsort(scores, descending, STABLE)
  for i in order: if not suppressed[i]: keep i; for every later j in order:
        inter = max(0, min(x2)-max(x1)) * max(0, min(y2)-max(y1))
        ovr   = inter / (area_i + area_j - inter);  suppressed[j] |= ovr > thr   (strict)
  returns kept indices into the input, in descending-score order (int64).

Score order: the kernel sorts with scores.sort(stable=True, descending=True).  For ANY float64 vector that is: a NaN is greater than
every number, +inf included, and equal to every other NaN; -0.0 == +0.0; equal scores keep input order.  So NaNs come first in
input order, then +inf, ..., -inf last (tests/test_nms_cases.py pins `visiting_order` against torch.sort itself).
Threshold: any float is taken as given.  ovr > thr is false for a NaN ovr (0 / 0: two zero-area boxes), so such a pair never
suppresses; a negative thr suppresses disjoint boxes (ovr = 0 > thr); thr >= 1 suppresses nothing, exact duplicates included.
Box coordinates are finite: np.maximum propagates a NaN where std::max does not.
"""
import numpy as np


def visiting_order(scores):
    """Indices in the order torch.sort(scores, descending=True, stable=True) returns them, for any float64 vector.
    (np.argsort(-scores, kind="stable") is that order only without NaN: numpy sorts a NaN LAST.)"""
    s = np.asarray(scores, dtype=np.float64)
    nan = np.isnan(s)
    # np.lexsort is stable and takes its primary key last: NaN flag (NaN first), then -s ascending (-0.0 and +0.0 compare equal)
    return np.lexsort((np.where(nan, 0.0, -s), ~nan)).astype(np.int64)


def nms(boxes, scores, thr):
    boxes = np.asarray(boxes)
    scores = np.asarray(scores)
    n = boxes.shape[0]
    if n == 0:
        return np.empty((0,), dtype=np.int64)
    x1, y1, x2, y2 = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
    areas = (x2 - x1) * (y2 - y1)
    order = visiting_order(scores)
    suppressed = np.zeros(n, dtype=bool)
    keep = []
    thr = boxes.dtype.type(thr)
    for _i in range(n):
        i = order[_i]
        if suppressed[i]:
            continue
        keep.append(i)
        rest = order[_i + 1:]
        if rest.size == 0:
            continue
        xx1 = np.maximum(x1[i], x1[rest])
        yy1 = np.maximum(y1[i], y1[rest])
        xx2 = np.minimum(x2[i], x2[rest])
        yy2 = np.minimum(y2[i], y2[rest])
        w = np.maximum(boxes.dtype.type(0), xx2 - xx1)
        h = np.maximum(boxes.dtype.type(0), yy2 - yy1)
        inter = w * h
        with np.errstate(divide="ignore", invalid="ignore"):
            ovr = inter / (areas[i] + areas[rest] - inter)
        suppressed[rest[ovr > thr]] = True
    return np.asarray(keep, dtype=np.int64)
