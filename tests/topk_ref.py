"""numpy restatement of tf_topk_select_f64[_batched] (csrc/topk.hip; contract: include/tinyfaces_hip.h).  Never imported by the package.

The min(n, k) rows that come first in the order the hard NMS itself uses -- larger score first; on equal scores (-0.0 == +0.0) the lower
input index first; a NaN behind every number, -inf included, NaNs among themselves by index -- returned as ASCENDING input indices."""
import numpy as np


def order(scores):
    """All indices in the selection order: np.lexsort on (NaN last, score descending, index ascending)."""
    s = np.asarray(scores, dtype=np.float64)
    nan = np.isnan(s)
    neg = np.where(nan, 0.0, -s) + 0.0                                # -s: descending; + 0.0 turns -0.0 into +0.0 (they compare equal anyway)
    return np.lexsort((np.arange(s.size), neg, nan)).astype(np.int64)  # last key first: NaN flag, then score, then index


def topk_select(scores, k):
    """int64 indices of the min(n, k) best rows, ascending."""
    if k < 1:
        raise ValueError(f"k={k}")
    return np.sort(order(scores)[:k])


def topk_select_batched(scores, seg_offsets, k):
    """Per segment -> (indices into the concatenated input, back to back; the new offsets)."""
    s = np.asarray(scores, dtype=np.float64)
    offs = [int(o) for o in seg_offsets]
    parts = [topk_select(s[a:b], k) + a for a, b in zip(offs, offs[1:])]
    new = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(int).tolist()
    return (np.concatenate(parts) if parts else np.empty(0, np.int64)).astype(np.int64), new


def key(scores):
    """The order-preserving uint64 key of csrc/topk.hip: sign bit flipped for non-negatives, all bits for negatives, -0 -> +0, NaN -> 0."""
    s = np.array(scores, dtype=np.float64, copy=True).reshape(-1)
    b = s.view(np.uint64).copy()
    b[b == np.uint64(1 << 63)] = 0
    neg = (b >> np.uint64(63)).astype(bool)
    out = np.where(neg, ~b, b | np.uint64(1 << 63))
    out[np.isnan(s)] = 0
    return out
