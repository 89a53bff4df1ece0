"""The inputs of tests/test_gpu_matrix_nms.py, built here so that tests/test_matrix_nms.py can check them on the CPU: every case must keep the two
margins of tests/matrix_nms_ref.py above MARGIN, i.e. no emission order, admission or emission test of the reference run is within reach of a
last-bit difference between the device's exp and numpy's.  Test infrastructure; never imported by the package.

Sizes: n = 1, 2; 63 / 64 / 65 / 129 (T-1, T, T+1, 2T+1 for the 64 rows of a pair block); 255 / 256 / 257 / 513 (its 256-column LDS tile);
31 / 32 / 33 (the 32 boxes of a narrow rank block); 2047 / 2048 / 2049 / 4097 (the rank kernels' 2048-value tile); 16383 / 16384 (the rank
kernels switch from 32 to 128 boxes per block at 16 384; only ~700 candidates of these two lists are admitted, so that the restatement stays
quick while the rank kernels still walk all of them); 5000 clustered candidates (79 pair blocks, 20 column tiles, three rank tiles)."""
import functools

import numpy as np

import matrix_nms_ref
import vote_ref

MARGIN = 1e-9
ROWS, TILE, RANK_BOXES, RANK_TILE, WIDE = 64, 256, 32, 2048, 16384          # csrc/matrix_nms.hip: kRows, kTile, 32 * Q, the score tile, the Q switch
SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 129, 255, 256, 257, 513, 2047, 2048, 2049, 4097, 5000)
SEGMENTED = {
    "S2_empty_first": (0, 130),
    "S2_empty_last": (130, 0),
    "S3_empty_middle": (257, 0, 513),
    "S64": (0, 257, 64, 0, 65, 1, 256, 2, 63, 255) + tuple((7 * i) % 70 for i in range(10, 63)) + (0,),
}


def _clustered(n, seed):
    boxes, logits = vote_ref.clustered_boxes(n, seed=seed)
    return boxes, logits


def _sparse(n, seed, admitted=700):
    """n clustered candidates of which only `admitted` random ones pass score_thresh = 0.001 (the others sit at logit -20, p = 2e-9)."""
    boxes, logits = vote_ref.clustered_boxes(n, seed=seed)
    rng = np.random.RandomState(seed + 1)
    low = np.ones(n, dtype=bool)
    low[rng.choice(n, admitted, replace=False)] = False
    logits[low] = -20.0
    return boxes, logits


def _content():
    c = {}
    rng = np.random.RandomState(5)
    b, s = _clustered(300, 301)
    # exact duplicates: 40 rows copied from other rows, with the score copied too / with their own scores
    src, dst = rng.choice(150, 40, replace=False), 150 + rng.choice(150, 40, replace=False)
    bb, ss = b.copy(), s.copy()
    bb[dst] = bb[src]; ss[dst] = ss[src]
    c["dup_same_scores"] = (bb, ss, 0.001)
    bb = b.copy(); bb[dst] = bb[src]
    c["dup_other_scores"] = (bb, s.copy(), 0.001)
    bb = b.copy(); bb[::7, 2] = bb[::7, 0]; bb[3::11, 3] = bb[3::11, 1]
    c["zero_area"] = (bb, s.copy(), 0.001)
    # touching boxes: a 16 x 16 grid of 10 x 10 cells sharing their edges (inter == 0), and every fourth one grown to overlap its neighbours
    gx, gy = np.meshgrid(np.arange(16) * 10.0, np.arange(16) * 10.0)
    g = np.stack([gx.ravel(), gy.ravel(), gx.ravel() + 10, gy.ravel() + 10], axis=1)
    g[::4, 2:] += 3.0
    c["touching"] = (g, rng.normal(0, 2, 256), 0.001)
    ss = s.copy(); ss[::13] = np.inf; ss[5::17] = -np.inf; ss[2::19] = 1e4; ss[7::23] = -1e4
    c["extreme_logits"] = (b.copy(), ss, 0.001)
    ss = s.copy(); ss[::9] = np.nan; ss[299] = np.nan; ss[0] = np.nan
    c["nan_scores"] = (b.copy(), ss, 0.001)
    c["all_below"] = (b.copy(), np.minimum(s, -1.0), 0.3)                       # sigmoid(-1) = 0.27 < 0.3: nothing is admitted
    c["thresh_zero"] = (b.copy(), s.copy(), 0.0)
    c["all_equal"] = (b.copy(), np.full(300, 0.75), 0.001)
    return c


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (boxes (n, 4), logits (n,), seg_offsets, score_thresh)}, read-only arrays."""
    out = {}
    for n in SIZES:
        b, s = _clustered(n, n)
        out[f"n{n}"] = (b, s, (0, n), 0.001)
    for n in (WIDE - 1, WIDE):
        b, s = _sparse(n, n)
        out[f"n{n}_sparse"] = (b, s, (0, n), 0.001)
    for name, sizes in SEGMENTED.items():
        parts = [_clustered(n, 900 + 3 * i) for i, n in enumerate(sizes)]
        b = np.concatenate([p[0].reshape(-1, 4) for p in parts])
        s = np.concatenate([p[1] for p in parts])
        out[name] = (b, s, tuple(int(v) for v in np.concatenate([[0], np.cumsum(sizes)])), 0.001)
    for name, (b, s, thr) in _content().items():
        out[name] = (b, s, (0, len(s)), thr)
    for b, s, _, _ in out.values():
        b.setflags(write=False); s.setflags(write=False)
    return out


def scores_for(name, score):
    """The scores operand of a case under a score mode: the logits, or the host's sigmoid of them for score="score"."""
    logits = cases()[name][1]
    return logits if score == "sigmoid" else vote_ref.weights(logits)


@functools.lru_cache(maxsize=None)
def _ranked(name, score):
    boxes, _, offs, thr = cases()[name]
    sc = scores_for(name, score)
    return [matrix_nms_ref.ranked(boxes[a:b], sc[a:b], thr, score) for a, b in zip(offs, offs[1:])]


@functools.lru_cache(maxsize=None)
def reference(name, method, score="sigmoid", sigma=0.5):
    """Per segment (keep into the concatenated input, scores, gap_margin, thresh_margin, details) of the restatement; computed once."""
    boxes, _, offs, thr = cases()[name]
    sc = scores_for(name, score)
    res = []
    for (a, b), rk in zip(zip(offs, offs[1:]), _ranked(name, score)):
        k, s, gap, dist, det = matrix_nms_ref.matrix_nms(boxes[a:b], sc[a:b], method, sigma, thr, score, details=True, rank=rk)
        k, s = k + a, s
        k.setflags(write=False); s.setflags(write=False)
        res.append((k, s, gap, dist, det))
    return res
