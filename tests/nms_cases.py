"""Named inputs for the hard NMS (tf_nms_f64 / tf_nms_f64_batched, csrc/nms.hip), shared by tests/test_nms_cases.py (CPU: the closed forms
against oracle/nms.py, the oracle's order against torch.sort, a double loop against both) and tests/test_gpu_nms.py (the same cases through
the kernels).  Nothing here touches the GPU or imports torch.

A case is (boxes float64 [n, 4], scores float64 [n], thr, expected_keep or None).  expected_keep is the answer in closed form where there is
one -- it does not come from the oracle, so it tests the oracle as much as the kernel.  Structured lists are built in RANK order (rank r has
score -r) and then shuffled by `perm_seed`, the expected indices mapped along: the kernel's order[] is the identity only where a case is about
the identity (the tie cases).

Each family is aimed at one part of the kernel:
  chain                  every 64-box chunk holds kept rows that strike the next chunk: the in-LDS resolve and the push across 1024-box
                         super-chunks carry real bits over every boundary; four thresholds, 0.0 and 1.0 among them
  suppressed_suppressor  A keeps, B falls to A, C overlaps only B: C must survive, with A, B, C in the same chunk, in neighbouring chunks, in
                         neighbouring super-chunks
  far_pair               rank 0 suppresses rank n - 1 and nothing else does anything: the push kernel alone
  exact_threshold        an IoU that IS the threshold: the strict `>`
  threshold_edges        thr = -0.0, below 0 (the side of `inter == 0 && thr >= 0` that skips nothing), 1 and above; a 0 / 0 IoU
  degenerate             zero-width, inverted and duplicate boxes with tied scores at five thresholds
  ties                   all-equal, two-valued, rounded and signed-zero scores at the sizes where the rank kernel changes path: 1024 (a super-
                         chunk), 2048 (a score tile), 16 384 (one box per thread -> four)
  non_finite             NaN, +inf, -inf scores: the order is torch.sort's (NaN first), the rank a permutation whatever the scores

Out of scope: NaN box COORDINATES.  std::max (the reference), fmax (the kernel) and np.maximum (the oracle) each treat a NaN operand
differently; the header asks for finite coordinates."""
import functools

import numpy as np

from oracle import nms as onms

FILL_X0 = 0.0            # filler boxes live at x >= 0, the boxes a case is about at x <= -900


# ---------------------------------------------------------------------------------------------------------------------- helpers
def grid_boxes(m, first=0):
    """m pairwise disjoint 10 x 10 boxes on a 20-pixel grid, 64 to a row; `first` skips that many grid cells."""
    k = np.arange(first, first + m)
    x, y = FILL_X0 + 20.0 * (k % 64), 20.0 * (k // 64)
    return np.stack([x, y, x + 10.0, y + 10.0], 1)


def ranked(boxes_by_rank, expected_ranks, thr, perm_seed):
    """Boxes listed by rank (rank r gets score -r) -> a case whose input order is shuffled by perm_seed (None: left in rank order)."""
    boxes_by_rank = np.asarray(boxes_by_rank, dtype=np.float64)
    n = boxes_by_rank.shape[0]
    pos = np.arange(n) if perm_seed is None else np.random.RandomState(perm_seed).permutation(n)     # pos[r] = input index of rank r
    boxes, scores = np.empty((n, 4)), np.empty(n)
    boxes[pos], scores[pos] = boxes_by_rank, -np.arange(n, dtype=np.float64)
    return boxes, scores, thr, pos[np.asarray(expected_ranks, dtype=np.int64)].astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------- chain
CHAIN_SIZES = (64, 65, 1024, 1025, 2049, 3000)
CHAIN_STEP = {0.0: 3, 0.3: 2, 0.5: 1, 1.0: 1}           # thr -> every step-th box of the chain is kept


def chain(n, thr, perm_seed=11):
    """Boxes [4k, 0, 4k + 10, 10], score -k: neighbours overlap with IoU 60 / 140, next-but-one with 20 / 180, the third does not touch.
    thr = 0.3: every second box; 0.5 and 1.0: every box; 0.0: every third (box k + 3 starts at 4k + 12, clear of box k)."""
    k = np.arange(n, dtype=np.float64)
    boxes = np.stack([4 * k, 0 * k, 4 * k + 10, 0 * k + 10], 1)
    return ranked(boxes, np.arange(0, n, CHAIN_STEP[thr]), thr, perm_seed)


def chain_cases():
    return {f"chain-n{n}-thr{thr}": chain(n, thr, perm_seed=100 + n) for n in CHAIN_SIZES for thr in CHAIN_STEP}


# ---------------------------------------------------------------------------------------------------------------------- suppressed suppressor
SUPPRESSOR_RANKS = ((1, 2), (63, 64), (64, 1023), (70, 1024), (1023, 1024), (1030, 2050))


def suppressed_suppressor(r1, r2, thr=0.3, perm_seed=12):
    """A = rank 0, B = rank r1 = A moved 4 px (IoU 60 / 140 > thr), C = rank r2 = A moved 8 px (20 / 180 < thr with A, 60 / 140 with B).  Every
    other rank is a grid box clear of all.  n = r2 + 5.  Everything but B is kept: B is suppressed, so it suppresses nothing."""
    n = r2 + 5
    boxes = np.empty((n, 4))
    boxes[:] = grid_boxes(n)
    a = np.array([-1000.0, 0.0, -990.0, 10.0])
    boxes[0], boxes[r1], boxes[r2] = a, a + [4, 0, 4, 0], a + [8, 0, 8, 0]
    return ranked(boxes, np.delete(np.arange(n), r1), thr, perm_seed)


def suppressed_suppressor_cases():
    return {f"suppressor-r{r1}-r{r2}": suppressed_suppressor(r1, r2, perm_seed=200 + r2) for r1, r2 in SUPPRESSOR_RANKS}


# ---------------------------------------------------------------------------------------------------------------------- far pair
FAR_PAIR_SIZES = (1025, 2049, 3000)


def far_pair(n, thr=0.3, perm_seed=13):
    """n pairwise disjoint boxes, except that rank n - 1 is rank 0 moved by one pixel (IoU 90 / 110): all but the last rank are kept."""
    boxes = grid_boxes(n)
    boxes[n - 1] = boxes[0] + [1, 0, 1, 0]                  # [1, 11] x [0, 10]: clear of the grid box at x = 20
    return ranked(boxes, np.arange(n - 1), thr, perm_seed)


def far_pair_cases():
    return {f"far-n{n}": far_pair(n, perm_seed=300 + n) for n in FAR_PAIR_SIZES}


# ---------------------------------------------------------------------------------------------------------------------- exact threshold
# (first box, second box, their IoU): areas and intersection are small integers and the quotient a power of two, so the IoU is exact
EXACT_PAIRS = {0.5: ([-1000.0, 0, -998, 2], [-1000.0, 0, -998, 1]),           # 2 / (4 + 2 - 2)
               0.25: ([-1000.0, 0, -999, 1], [-1000.0, 0, -998, 2])}          # the smaller box first: 1 / (1 + 4 - 1)


def exact_threshold(iou, thr, ranks, perm_seed=14):
    """The pair of EXACT_PAIRS[iou] at `ranks` of a 70-box list of disjoint grid boxes.  The second box is kept iff not iou > thr."""
    n = 70
    boxes = grid_boxes(n)
    boxes[ranks[0]], boxes[ranks[1]] = EXACT_PAIRS[iou]
    keep = np.arange(n) if not iou > thr else np.delete(np.arange(n), ranks[1])
    return ranked(boxes, keep, thr, perm_seed)


def exact_threshold_cases():
    out = {}
    for iou in EXACT_PAIRS:
        below = float(np.nextafter(iou, 0.0))
        for thr, tag in ((iou, "at"), (below, "below")) + (((0.25, "quarter"),) if iou == 0.5 else ()):
            for ranks in ((0, 1), (63, 64)):
                out[f"exact-iou{iou}-{tag}-r{ranks[0]}"] = exact_threshold(iou, thr, ranks, perm_seed=400 + ranks[0])
    return out


# ---------------------------------------------------------------------------------------------------------------------- threshold edges
EDGE_BOXES = np.array([[-950.0, 50, -950, 50],        # 0  zero area, the top score: its IoU with every box is 0 / area, with box 5 it is 0 / 0
                       [-1000.0, 0, -999, 1],         # 1  unit box
                       [-999.0, 0, -998, 1],          # 2  touches box 1 along an edge: intersection 0
                       [-990.0, 0, -988, 2],          # 3
                       [-988.125, 0, -986.125, 2],    # 4  a sliver of box 3: IoU 0.25 / 7.75
                       [-950.0, 50, -950, 50],        # 5  zero area again
                       [-1000.0, 0, -999, 1]])        # 6  box 1 again: IoU exactly 1
EDGE_KEEP = {"0.0": [0, 1, 2, 3, 5], "-0.0": [0, 1, 2, 3, 5],        # touching boxes stay, the sliver and the duplicate go; NaN > 0 is false
             "-0.1": [0, 5],                                          # 0 > -0.1: box 0 suppresses all but box 5, whose IoU with it is NaN
             "1.0": [0, 1, 2, 3, 4, 5, 6], "1.5": [0, 1, 2, 3, 4, 5, 6]}    # 1 > 1 is false: not even the duplicate goes


def threshold_edges(thr_text, perm_seed=15):
    return ranked(EDGE_BOXES, EDGE_KEEP[thr_text], float(thr_text), perm_seed)


def threshold_edges_cases():
    return {f"edges-thr{t}": threshold_edges(t, perm_seed=500 + i) for i, t in enumerate(EDGE_KEEP)}


# ---------------------------------------------------------------------------------------------------------------------- degenerate boxes
DEGENERATE_THR = (-0.5, 0.0, 0.3, 0.999, 1.0)


def degenerate(thr, n=2000, seed=16):
    """Boxes of 10..80 px on a 900 x 700 canvas; every 7th has zero width, every 11th is inverted in x (a negative area), every 5th is a copy of
    the box 3 places before it; scores rounded to one decimal (about 60 values for n boxes).  No closed form: the oracle is the reference."""
    rng = np.random.RandomState(seed)
    c, w = rng.uniform(0, [900, 700], (n, 2)), rng.uniform(10, 80, (n, 2))
    boxes = np.round(np.concatenate([c - w / 2, c + w / 2], 1), 2)
    k = np.arange(n)
    zero, inv, dup = k % 7 == 3, k % 11 == 5, (k % 5 == 4) & (k >= 3)
    boxes[zero, 2] = boxes[zero, 0]
    boxes[inv] = boxes[inv][:, [2, 1, 0, 3]]
    boxes[dup] = boxes[k[dup] - 3]
    return boxes, np.round(rng.randn(n), 1), thr, None


def degenerate_cases(n=2000):
    return {f"degenerate-n{n}-thr{thr}": degenerate(thr, n) for thr in DEGENERATE_THR}


# ---------------------------------------------------------------------------------------------------------------------- tie structure
TIE_SIZES = (1023, 1024, 1025, 2047, 2048, 2049, 4097, 16383, 16384, 16385, 16513)
TIE_SCORES = ("zeros", "parity", "round1", "signed_zero")


def clustered_boxes(n, seed, centres=300):
    """n boxes around `centres` places of a 1500 x 1000 canvas: sides of 20..60 px per place, every coordinate jittered by up to 3 px.  Most
    boxes fall to the first of their place, so the oracle (kept x n) stays cheap at any n."""
    rng = np.random.RandomState(seed)
    c, side = rng.uniform(0, [1500, 1000], (centres, 2)), rng.uniform(20, 60, (centres, 2))
    which = rng.randint(0, centres, n)
    base = np.concatenate([c - side / 2, c + side / 2], 1)[which]
    return base + rng.uniform(-3, 3, (n, 4))


def tie_scores(kind, n, seed=0):
    if kind == "zeros":                                    # every pair ties: the order is the identity
        return np.zeros(n)
    if kind == "parity":                                   # two values, interleaved: every tile holds both
        return (np.arange(n) % 2).astype(np.float64)
    if kind == "round1":                                   # about 60 values
        return np.round(np.random.RandomState(seed).randn(n), 1)
    if kind == "signed_zero":                              # -0.0 == +0.0: ties, input order
        return np.where(np.arange(n) % 2 == 0, 0.0, -0.0)
    raise ValueError(kind)


def ties(n, kind, thr=0.3):
    return clustered_boxes(n, 1000 + n), tie_scores(kind, n, 2000 + n), thr, None


def tie_cases(sizes=TIE_SIZES):
    return {f"ties-n{n}-{kind}": ties(n, kind) for n in sizes for kind in TIE_SCORES}


# ---------------------------------------------------------------------------------------------------------------------- non-finite scores
VEC8 = np.array([0.5, np.nan, 0.7, np.nan, -np.inf, np.inf, 0.0, -0.0])
VEC8_ORDER = [1, 3, 5, 2, 0, 6, 7, 4]                      # torch.sort(descending=True, stable=True): NaN first, in input order, then +inf


def _sprinkle(scores, nan, pinf, ninf):
    scores = scores.copy()
    scores[list(nan)], scores[list(pinf)], scores[list(ninf)] = np.nan, np.inf, -np.inf
    scores[list(nan)[0]] = np.copysign(np.nan, -1.0)       # one NaN with the sign bit set: as much a NaN as the others
    return scores


def non_finite_scores(name):
    if name == "vec8":
        return VEC8.copy()
    if name == "n2100-few":                                # NaN on both sides of input index 2048 (a score-tile edge) and at both ends
        return _sprinkle(tie_scores("round1", 2100, 7), (0, 5, 2046, 2047, 2048, 2049, 2099), (1, 1000, 2050), (2, 1001, 2051))
    if name == "n2100-mostly":                             # 2050 NaN: their RANKS cross 2048, and every block of the rank kernel holds some
        s = np.full(2100, np.nan)
        k = np.arange(0, 2100, 42)
        s[k] = tie_scores("round1", k.size, 8)
        s[[42, 2058]] = np.inf, -np.inf
        return s
    if name == "n16385-sparse":                            # the four-boxes-per-thread form: blocks with and without a NaN of their own
        return _sprinkle(tie_scores("round1", 16385, 9), list(range(0, 16385, 997)) + [16383, 16384], (3, 8191, 16382), (4, 8192, 16381))
    raise ValueError(name)


NON_FINITE = ("vec8", "n2100-few", "n2100-mostly", "n16385-sparse")


def non_finite(name, thr=0.3):
    s = non_finite_scores(name)
    return clustered_boxes(s.size, 3000 + s.size, centres=2 if s.size < 100 else 300), s, thr, None


def non_finite_cases():
    return {f"nonfinite-{name}": non_finite(name) for name in NON_FINITE}


# ---------------------------------------------------------------------------------------------------------------------- batched layouts
LAYOUT_SIZES = (1, 63, 1025, 16385)                         # one call: the rank kernel's form is chosen by the LARGEST segment, so the 1- and 63-box
LAYOUT_SCORES = ("round1", "zeros", "non_finite")           # segments run four boxes per thread, which no single-list call of that size does


def layout_segments(kind, thr=0.3):
    """One case per size of LAYOUT_SIZES, to be packed into one batched call.  non_finite: rounded scores with a NaN at both ends of every
    segment and +inf / -inf inside."""
    out = {}
    for n in LAYOUT_SIZES:
        s = tie_scores("round1" if kind == "non_finite" else kind, n, 4000 + n)
        if kind == "non_finite":
            s[[0, n - 1]] = np.nan
            if n > 2:
                s[[n // 2, n // 3]] = np.inf, -np.inf
        out[f"layout-{kind}-n{n}"] = (clustered_boxes(n, 5000 + n), s, thr, None)
    return out


# ---------------------------------------------------------------------------------------------------------------------- everything
FAMILIES = {"chain": chain_cases, "suppressed_suppressor": suppressed_suppressor_cases, "far_pair": far_pair_cases,
            "exact_threshold": exact_threshold_cases, "threshold_edges": threshold_edges_cases, "degenerate": degenerate_cases,
            "ties": tie_cases, "non_finite": non_finite_cases}


@functools.lru_cache(maxsize=None)
def family(name):
    """{case name: (boxes, scores, thr, expected or None)} of one family, built once per process."""
    return FAMILIES[name]()


_ORACLE = {}


def oracle_keep(name, case):
    """oracle.nms.nms of a named case, computed once per process and returned read-only."""
    if name not in _ORACLE:
        boxes, scores, thr, _ = case
        keep = onms.nms(boxes, scores, thr)
        keep.setflags(write=False)
        _ORACLE[name] = keep
    return _ORACLE[name]


def score_vectors():
    """Every score vector this file can hand to a kernel, by name: what the oracle's visiting order is pinned on."""
    out = {f"{kind}-n{n}": tie_scores(kind, n, 2000 + n) for kind in TIE_SCORES for n in (1, 63, 1025, 2049)}
    out.update({f"nonfinite-{name}": non_finite_scores(name) for name in NON_FINITE})
    out.update({name: case[1] for name, case in layout_segments("non_finite").items()})
    out["degenerate"] = degenerate(0.3)[1]
    out["chain-shuffled"] = chain(65, 0.3)[1]
    out["inf-only"] = np.array([np.inf, -np.inf, np.inf, -np.inf, np.inf])
    out["nan-only"] = np.full(5, np.nan)
    return out


# ---------------------------------------------------------------------------------------------------------------------- restatements
def kernel_rank(scores, nan_aware=True):
    """The rank kernel's formula in numpy: rank[i] = #{j : s_j > s_i or (s_j == s_i and j < i)}.  nan_aware: `>` and `==` as torch.sort
    orders float64 (NaN above every number, NaN == NaN); otherwise IEEE compares, under which every compare against a NaN is false."""
    s = np.asarray(scores, dtype=np.float64)
    i = np.arange(s.size)
    sj, si = s[None, :], s[:, None]
    with np.errstate(invalid="ignore"):
        gt, eq = sj > si, sj == si
    if nan_aware:
        nj, ni = np.isnan(sj), np.isnan(si)
        gt, eq = (nj & ~ni) | (~nj & ~ni & gt), (nj & ni) | (~nj & ~ni & eq)
    return (gt | (eq & (i[None, :] < i[:, None]))).sum(axis=1)


def brute_force_nms(boxes, scores, thr):
    """Greedy NMS as a double loop over Python floats: its own order (a selection by repeated maximum, NaN above every number), its own IoU.
    Shares no code with oracle/nms.py.  For n <= 300."""
    b = [[float(v) for v in row] for row in boxes]
    s = [float(v) for v in scores]
    n = len(s)
    assert n <= 300

    def before(i, j):                                       # does i come before j?
        ni, nj = s[i] != s[i], s[j] != s[j]
        if ni or nj:
            return (ni and not nj) or (ni and nj and i < j)
        return s[i] > s[j] or (s[i] == s[j] and i < j)

    left, order = list(range(n)), []
    while left:
        m = left[0]
        for j in left[1:]:
            if before(j, m):
                m = j
        order.append(m)
        left.remove(m)
    dead, keep = [False] * n, []
    for a, i in enumerate(order):
        if dead[i]:
            continue
        keep.append(i)
        ai = (b[i][2] - b[i][0]) * (b[i][3] - b[i][1])
        for j in order[a + 1:]:
            w = max(0.0, min(b[i][2], b[j][2]) - max(b[i][0], b[j][0]))
            h = max(0.0, min(b[i][3], b[j][3]) - max(b[i][1], b[j][1]))
            inter = w * h
            union = ai + (b[j][2] - b[j][0]) * (b[j][3] - b[j][1]) - inter
            if union == 0.0:                                # Python raises where IEEE gives NaN (0 / 0) or an infinity
                ovr = float("nan") if inter == 0.0 else float("inf")
            else:
                ovr = inter / union
            if ovr > thr:
                dead[j] = True
    return np.asarray(keep, dtype=np.int64)
