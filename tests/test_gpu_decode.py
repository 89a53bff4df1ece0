"""-m gpu: tf_decode_compact (csrc/decode.hip) against tests/decode_ref.py, the float64 restatement, at operator level.

The decode is the gate between the network and everything the evaluator reports; the golden fixtures hold it to ONE receptive field
(stride (8, 8), offset (-1, -1)), nt = 25, tstride = 5, threshold 0.8, a counter that starts at 0 and a list with room for everything.  Here:
receptive fields whose axes differ, maps from one pixel to 1034 blocks, nt from 1 to the largest the kernel takes, template strides with
padding, both mask axes, thresholds with logits planted ulps around them, non-finite and overflowing operands, a counter that arrives
non-zero, a list that is too short, and the two host paths that call the kernel.

Every case (`_case`) asserts: the returned total equals the restatement's up to undecided entries (decode_ref: float64 probability within 4
fp32 spacings of the threshold -- none unless a case plants them, which is asserted); every decided candidate is there, no decided
non-candidate is, rows are in C order over (y, x, template) (a row's identity is recovered from its logit: all logits of a case are
distinct); column 4 is the logit bit for bit; box coordinates are within decode_ref.box_bound; rows at or behind the written count still
hold the NaN fill, rows in front of the incoming count their sentinel; the guards around dets, the counter and the workspace are intact;
a second call on the same inputs gives the same bytes."""
import numpy as np
import pytest
import torch

import decode_ref
from gpu_util import report
from redzone import assert_guards, guarded, guarded_like, guarded_workspace

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = -12345.5
GEOS = [(8, 8, -1, -1), (8, 16, -1, 5), (4, 8, 3, -2), (1, 3, 0, 7)]             # (sty, stx, ofy, ofx)
SHAPES = [(1, 1), (1, 64), (1, 65), (5, 13), (3, 64), (7, 31), (9, 70), (33, 2)]
SCALES = [0.5, 1, 2, 0.7]


# ------------------------------------------------------------------------------------------------ inputs
def make_templates(nt, tstride=5, seed=0):
    """(nt, tstride) float64: widths 8 + 6i, heights 11 + 6i in shuffled order -- all 2nt sizes distinct, cw != ch in every row, so that a
    cw / ch swap or a wrong template row shows --, off-centre corners, NaN in every padding column."""
    rng = np.random.RandomState(1000 + seed)
    order = rng.permutation(nt)
    w, h = 8.0 + 6 * order, 11.0 + 6 * rng.permutation(nt)
    T = np.full((nt, tstride), np.nan)
    T[:, 0] = -np.round(w / 2) + rng.randint(-2, 3, nt) + 0.25
    T[:, 1] = -np.round(h / 2) + rng.randint(-2, 3, nt) - 0.5
    T[:, 2], T[:, 3] = T[:, 0] + w - 1, T[:, 1] + h - 1
    assert np.all(T[:, 2] - T[:, 0] + 1 != T[:, 3] - T[:, 1] + 1)
    return T


def make_score(nt, H, W, thr, seed, density=0.1, hot=None):
    """(5nt, H, W) float32.  The class logits are a shuffled ladder of H*W*nt DISTINCT values from logit(thr) - 9 to logit(thr) + 9 d / (1 - d):
    the fraction `density` lies above the threshold, and no two entries share a logit.  hot (flat bool over (y, x, t)): the values above
    the threshold are dealt into these entries only.  Regression channels: tx, ty ~ N(0, 0.5), tw, th ~ N(0, 0.4)."""
    rng = np.random.RandomState(seed)
    n = H * W * nt
    L = float(decode_ref.logit32(thr))
    up = 9.0 * density / (1.0 - density)
    ladder = (np.linspace(L - 9.0, L + up, n + 2)[1:-1] + rng.uniform(-0.2, 0.2) * (9.0 + up) / (n + 2)).astype(np.float32)
    assert np.unique(ladder).size == n
    if hot is None:
        flat = rng.permutation(ladder)
    else:
        above = ladder > np.float32(L)
        pick = rng.choice(np.flatnonzero(hot), int(above.sum()), replace=False)
        flat = np.empty(n, np.float32)
        flat[pick] = ladder[above]
        flat[np.setdiff1d(np.arange(n), pick)] = rng.permutation(ladder[~above])
    cls = flat.reshape(H, W, nt).transpose(2, 0, 1)
    reg = np.concatenate([rng.randn(2 * nt, H, W) * 0.5, rng.randn(2 * nt, H, W) * 0.4])
    return np.ascontiguousarray(np.concatenate([cls, reg.astype(np.float32)]))


def cls_view(score, nt):
    """The class logits as a WRITABLE (H, W, nt) view of `score`, for planting."""
    return score[:nt].transpose(1, 2, 0)


class Case:
    """One decode call's operands (numpy) and where its rows go."""

    def __init__(self, score, T, thr, scale, geo, vx=None, vt=None, start=0, cap=None, direct=False, planted=False):
        self.score, self.T, self.thr, self.scale, self.geo = score, T, thr, scale, geo
        self.nt, (_, self.H, self.W) = T.shape[0], score.shape
        assert score.shape[0] == 5 * self.nt and score.dtype == np.float32
        self.vx = np.ones(self.W, np.uint8) if vx is None else np.asarray(vx, np.uint8)
        self.vt = np.ones(self.nt, np.uint8) if vt is None else np.asarray(vt, np.uint8)
        self.start, self.direct, self.planted = start, direct, planted
        self.cap = start + self.H * self.W * self.nt if cap is None else cap       # rows of dets: room for everything by default

    @property
    def stride(self):
        return self.geo[0], self.geo[1]

    @property
    def offset(self):
        return self.geo[2], self.geo[3]


# ------------------------------------------------------------------------------------------------ the call
def _body_ptr(t):
    z = t._redzone
    return z.alloc.data_ptr() + z.off              # also for a body of 0 bytes, whose tensor has no data pointer


def new_list(cap, start):
    """dets (cap, 5) float64 and the counter between guards; dets holds the NaN fill, rows in front of `start` a sentinel."""
    dets = guarded((cap, 5), torch.float64, DEV, pitch_bytes=40)
    if min(start, cap) > 0:
        dets[:min(start, cap)] = SENTINEL
    count = guarded((1,), torch.int32, DEV)
    count.fill_(start)
    return dets, count


def launch(c, dets, count):
    """One tf_decode_compact on the case's operands (inputs between guards too: a read out of range brings a NaN or an unmasked entry into
    the result).  direct: through the C ABI with the case's cap and a workspace of exactly tf_decode_workspace_bytes; else through
    ops.decode_compact (cap = the rows of dets, its own workspace).  Returns the workspace (or None)."""
    from tinyfaces import _hip, ops
    score, T = guarded_like(torch.from_numpy(c.score), DEV, pitch_bytes=c.W * 4), guarded_like(torch.from_numpy(c.T), DEV)
    vx, vt = guarded_like(torch.from_numpy(c.vx), DEV), guarded_like(torch.from_numpy(c.vt), DEV)
    rf = {"stride": [c.geo[0], c.geo[1]], "offset": [c.geo[2], c.geo[3]]}
    ws = None
    if c.direct:
        l = _hip.lib()
        wsb = l.tf_decode_workspace_bytes(c.H, c.W, c.nt)
        ws = guarded_workspace(wsb, DEV)
        rc = l.tf_decode_compact(score.data_ptr(), c.nt, c.H, c.W, T.data_ptr(), c.T.shape[1], vx.data_ptr(), vt.data_ptr(),
                                 float(np.float32(c.thr)), float(c.scale), c.geo[0], c.geo[1], c.geo[2], c.geo[3], _body_ptr(dets),
                                 count.data_ptr(), c.cap, ws.data_ptr(), wsb, _hip.stream())
        assert rc == 0, rc
    else:
        assert dets.shape[0] == c.cap
        ops.decode_compact(score, T, vx, vt, c.thr, c.scale, dets, count, rf)
    torch.cuda.synchronize()
    assert_guards(dets, "dets"); assert_guards(count, "count")
    if ws is not None:
        assert_guards(ws, "workspace")
    return ws


def run(c):
    """-> (dets as numpy, the counter afterwards) of a fresh call."""
    dets, count = new_list(c.cap, c.start)
    launch(c, dets, count)
    return dets.cpu().numpy().reshape(-1, 5), int(count.item())


# ------------------------------------------------------------------------------------------------ the comparison
def check(c, dets, after, front=True, tail=True, transform=None):
    """The asserts of the module docstring on rows [c.start, ...) of `dets` (numpy) and the counter `after`.  front / tail: rows in front of
    c.start must hold the sentinel, rows behind the written ones the fill.  transform(rows, bound) -> (rows, bound): what the caller did
    to the rows behind the kernel.  Returns figures for the report."""
    ref = decode_ref.decode(c.score, c.T, c.vx, c.vt, c.thr, c.scale, c.stride, c.offset, start=c.start, cap=c.cap)
    n_und = int(ref.undecided.sum())
    if not c.planted:
        assert n_und == 0, "precondition: this case plants nothing in the band, pick a seed that keeps it empty"
    cls = cls_view(c.score, c.nt).reshape(-1)                                  # C order over (y, x, t)
    known = np.flatnonzero(~np.isnan(cls))
    by_value = known[np.argsort(cls[known], kind="stable")]
    values = cls[by_value]
    assert np.all(values[1:] != values[:-1]), "precondition: all logits of a case are distinct"
    cand, und = np.flatnonzero(ref.candidate.reshape(-1)), np.flatnonzero(ref.undecided.reshape(-1))
    decided = np.setdiff1d(cand, und)
    total = after - c.start
    written = max(min(after, c.cap) - c.start, 0)
    assert decided.size <= total <= np.union1d(cand, und).size, (total, decided.size, cand.size, n_und)
    if n_und == 0:
        assert after == ref.total and written == ref.written
    # rows in front of the incoming count and behind the written ones are untouched
    if front:
        assert np.all(dets[:min(c.start, c.cap)] == SENTINEL), "a row in front of the incoming count was written"
    if tail:
        assert np.all(dets[c.start + written:].view(np.uint8) == 0xFF), "a row at or beyond the written count was written"
    got = dets[c.start:c.start + written]
    assert not np.isnan(got[:, 4]).any(), "a written row holds the fill or a NaN logit"
    # identity of every row from its logit; order; membership
    g32 = got[:, 4].astype(np.float32)
    assert np.array_equal(g32.astype(np.float64).view(np.int64), got[:, 4].view(np.int64)), "column 4 is not a float32 logit"
    at = np.minimum(np.searchsorted(values, g32), max(values.size - 1, 0))
    assert written == 0 or np.array_equal(values[at], g32), "column 4 holds a value that is no class logit of the map"
    flat = by_value[at] if written else np.empty(0, np.int64)
    assert np.all(np.diff(flat) > 0), "rows are not in C order over (y, x, template)"
    assert np.isin(flat, np.union1d(cand, und)).all(), "a decided non-candidate was admitted"
    if after <= c.cap:
        assert written == total and np.isin(decided, flat).all(), "a decided candidate is missing"
    else:
        assert n_und == 0                                                      # a truncated list is only checked without a band
    if n_und == 0:
        assert np.array_equal(flat, cand[:written])
    # the rows themselves
    y, x, t = np.unravel_index(flat, (c.H, c.W, c.nt))
    rows, half = decode_ref.rows_at(c.score, c.T, y, x, t, c.scale, c.stride, c.offset)
    assert np.array_equal(rows[:, 4].view(np.int64), got[:, 4].view(np.int64)), "column 4 is not the logit bit for bit"
    bound = decode_ref.box_bound(rows, half)
    if transform is not None:
        rows, bound = transform(rows, bound)
    fin = np.isfinite(rows[:, :4]) & np.isfinite(bound)
    with np.errstate(all="ignore"):
        diff = np.abs(got[:, :4] - rows[:, :4])
    assert np.all(diff[fin] <= bound[fin]), f"box error {float((diff[fin] / bound[fin]).max()):.3g} of its bound"
    assert np.array_equal(got[:, :4][~fin], rows[:, :4][~fin], equal_nan=True), "non-finite box coordinates differ"
    frac = float((diff[fin] / bound[fin]).max()) if fin.any() else 0.0
    return {"rows": int(written), "total": int(total), "box_err_of_bound": frac, "undecided": n_und,
            "undecided_admitted": int(np.isin(und, flat).sum()), "nonfinite_coords": int((~fin).sum())}


def _case(family, c, **kw):
    d1, a1 = run(c)
    d2, a2 = run(c)
    assert a1 == a2 and d1.tobytes() == d2.tobytes(), "a second call on the same inputs gave other bytes"
    out = check(c, d1, a1, **kw)
    report(f"decode_parity[{family}]", **out)
    return out, d1, a1


# ------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("si", range(len(SHAPES)), ids=[f"{h}x{w}" for h, w in SHAPES])
@pytest.mark.parametrize("gi", range(len(GEOS)), ids=["s8x8", "s8x16", "s4x8", "s1x3"])
def test_geometry(gi, si):
    """Receptive fields whose two axes differ (a swap of sty / stx or of ofy / ofx, in the kernel or in ops.decode_compact, is invisible with
    the project's (8, 8), (-1, -1)) on maps of one pixel, one block exactly, one block and a pixel, several rows in one block, blocks that
    straddle rows, H > W."""
    H, W = SHAPES[si]
    out, _, _ = _case("geometry", Case(make_score(25, H, W, 0.8, 10 * gi + si), make_templates(25, 5, si), 0.8, SCALES[(gi + si) % 4], GEOS[gi]))
    assert out["rows"] >= (H * W * 25) // 20                                    # the density is what make_score says


# ------------------------------------------------------------------------------------------------ nt, tstride
@pytest.mark.parametrize("tstride", [4, 5, 8])
@pytest.mark.parametrize("nt", [1, 3, 4, 25, 51])
def test_nt_and_tstride(nt, tstride):
    """nt = 1 (one wave of the inner loop holds a block), 3, 4 (64 * 4 = 256: exactly one pass), 25, 51 (the largest whose slab fits 64 KiB),
    with template rows of 4, 5 and 8 doubles, NaN in the padding."""
    out, _, _ = _case("nt_tstride", Case(make_score(nt, 7, 31, 0.8, 100 + nt), make_templates(nt, tstride, nt), 0.8, 0.7, GEOS[1]))
    assert out["rows"] >= 7 * 31 * nt // 20


# ------------------------------------------------------------------------------------------------ masks
def _mask_cases():
    nt, H, W = 5, 9, 70
    vt = np.ones(nt, np.uint8); vt[[0, 2, nt - 1]] = 0
    vx = np.ones(W, np.uint8); vx[[0, W - 1]] = 0
    return {"valid_t": (None, vt), "valid_x": (vx, None), "both": (vx, vt), "no_t": (None, np.zeros(nt, np.uint8)),
            "no_x": (np.zeros(W, np.uint8), None)}


@pytest.mark.parametrize("which", ["valid_t", "valid_x", "both", "no_t", "no_x"])
def test_masks(which):
    """valid_t with zeros at the first, the last and an interior template (mask_axis="template": the goldens only ever mask through valid_x),
    valid_x with zeros at x = 0 and x = W - 1, both, and masks that are all zero."""
    vx, vt = _mask_cases()[which]
    c = Case(make_score(5, 9, 70, 0.8, 200), make_templates(5), 0.8, 2, GEOS[2], vx=vx, vt=vt)
    out, _, after = _case("masks", c)
    unmasked = decode_ref.decode(c.score, c.T, np.ones(70, np.uint8), np.ones(5, np.uint8), 0.8, 2, c.stride, c.offset).total
    if which.startswith("no_"):
        assert after == 0 and out["rows"] == 0
    else:
        assert 0 < after < unmasked                                            # the mask removed candidates, and not all of them


def test_negative_threshold_admits_masked_entries_too():
    """thr = -0.5: a masked entry's probability is 0, which passes like every other: H * W * nt rows exactly, every one checked."""
    nt, H, W = 3, 5, 13
    vx = np.ones(W, np.uint8); vx[[0, 4, W - 1]] = 0
    c = Case(make_score(nt, H, W, 0.8, 210), make_templates(nt), -0.5, 0.5, GEOS[1], vx=vx, vt=[0, 1, 1])
    out, dets, after = _case("negative_threshold", c)
    assert after == H * W * nt == out["rows"]
    assert np.array_equal(dets[:, 4], cls_view(c.score, nt).reshape(-1).astype(np.float64))


# ------------------------------------------------------------------------------------------------ threshold
K_REQUIRED = [0, 1, -1, 2, -2, 8, -8, 64, -64, 4096, -4096]


def _plant_around(c_score, nt, thr, seed):
    """200 distinct logits around float32(logit(thr)): it shifted by k ulps for every k of K_REQUIRED, by 183 more k of -96 .. 95 (194 ulp shifts), and -- decided
    neighbours wherever the threshold lies, logit 0 of thr = 0.5 included, whose ulps are denormals -- moved by +-1.5, 3 and 5 times 2^-14.
    Planted over randomly chosen entries; the ladder of make_score keeps clear of them.  Returns the flat indices, K_REQUIRED's first."""
    L = decode_ref.logit32(thr)
    ks = K_REQUIRED + [k for k in range(-96, 97) if k not in K_REQUIRED][:183]
    vals = np.concatenate([decode_ref.ulp_shift(L, ks), (np.float64(L) + np.array([-5, -3, -1.5, 1.5, 3, 5]) * 2.0 ** -14).astype(np.float32)])
    assert vals.size == 200 and np.unique(vals).size == 200
    cls = cls_view(c_score, nt)
    flat = np.random.RandomState(seed).choice(cls.size, 200, replace=False)
    cls[np.unravel_index(flat, cls.shape)] = vals
    return flat, vals


@pytest.mark.parametrize("thr", [0.03, 0.5, 0.65, 0.8, 0.97])
def test_threshold_with_logits_planted_ulps_around_it(thr):
    """`>` in fp32 on an fp32 sigmoid.  Entries inside the band may go either way and take their ordered place when admitted; the planted
    neighbours outside it (from +-64 ulps, or +-1.5 * 2^-14 in the logit) are decided and held to the restatement."""
    nt, H, W = 4, 7, 31
    score = make_score(nt, H, W, thr, 300)
    flat, vals = _plant_around(score, nt, thr, 301)
    c = Case(score, make_templates(nt), thr, 1, GEOS[1], planted=True)
    ref = decode_ref.decode(c.score, c.T, c.vx, c.vt, thr, 1, c.stride, c.offset)
    und, cand = ref.undecided.reshape(-1)[flat], ref.candidate.reshape(-1)[flat]
    assert und[0] and (~und & cand).sum() >= 3 and (~und & ~cand).sum() >= 3    # k = 0 is in the band; decided neighbours on both sides
    assert ref.undecided.sum() == und.sum()                                     # nothing but planted entries is in the band
    out, dets, after = _case(f"threshold_{thr}", c)
    if thr == 0.5:
        # logit 0: exp(-0) = 1, 1 + 1 = 2, 1 / 2 = 0.5 in every arithmetic: the probability IS the threshold, and `>` does not admit it
        # (nor the denormal logits around it, whose exp rounds to 1): the one planted value where `>` and `>=` can be told apart
        assert vals[0] == 0 and np.all(np.abs(vals[:194]) < 1e-37) and not np.isin(vals[:194].astype(np.float64), dets[:after, 4]).any()


def test_threshold_zero_and_one():
    """thr = 0: sigmoid(-200) underflows to probability 0 in fp32 and does not pass, sigmoid(-80) = 1.8e-35 does; masked entries (probability
    0) do not.  thr = 1: nothing passes, although sigmoid(+200) is exactly 1."""
    nt, H, W = 3, 5, 13
    score = make_score(nt, H, W, 0.5, 310)
    cls = cls_view(score, nt)
    cls[1, 2, 0], cls[1, 2, 1], cls[4, 12, 2], cls[0, 0, 0] = -200.0, -80.0, 200.0, -80.5
    vx = np.ones(W, np.uint8); vx[5] = 0
    c = Case(score, make_templates(nt), 0.0, 2, GEOS[3], vx=vx, planted=True)       # -200 is `undecided` for float64: 1.4e-87 > 0
    out, dets, after = _case("threshold_0", c)
    assert after == H * (W - 1) * nt - 1 and out["undecided"] == 1 and out["undecided_admitted"] == 0
    assert -80.0 in dets[:after, 4] and -80.5 in dets[:after, 4] and -200.0 not in dets[:after, 4]
    c = Case(score, make_templates(nt), 1.0, 2, GEOS[3], vx=vx, planted=True)       # 1 - sigmoid(x) within 4 spacings of 1: the band
    out, dets, after = _case("threshold_1", c)
    assert after == 0 and out["rows"] == 0 and out["undecided"] >= 1


# ------------------------------------------------------------------------------------------------ non-finite and extreme operands
def test_nonfinite_and_extreme_operands():
    """Logits +inf (a candidate, its score column +inf), -inf and NaN (never candidates); tw / th of -200, 88, 89, +inf, NaN on candidates:
    with exp rounded to fp32 the box sizes are exactly 0, finite, inf, inf and NaN; tx / ty of +-1e30."""
    nt, H, W = 3, 5, 13
    score = make_score(nt, H, W, 0.8, 400, density=0.3)
    cls = cls_view(score, nt)
    cls[4, 11, 1], cls[2, 7, 0], cls[4, 12, 2], cls[1, 1, 1], cls[3, 0, 0] = np.inf, -np.inf, np.nan, np.nan, np.nan
    c = Case(score, make_templates(nt), 0.8, 0.7, GEOS[1])
    y, x, t = decode_ref.decode(score, c.T, c.vx, c.vt, 0.8, 0.7, c.stride, c.offset).index
    assert y.size >= 30
    extreme = [-200.0, 88.0, 89.0, np.inf, np.nan]
    for i, v in enumerate(extreme):                                            # tw alone, th alone, both
        for j, chans in enumerate([(3,), (4,), (3, 4)]):
            k = 3 * i + j
            for ch in chans:
                score[ch * nt + t[k], y[k], x[k]] = v
    for k, (ch, v) in enumerate([(1, 1e30), (1, -1e30), (2, 1e30), (2, -1e30)], start=16):
        score[ch * nt + t[k], y[k], x[k]] = v
    k = int(np.flatnonzero((y == 4) & (x == 11) & (t == 1))[0])                 # the +inf logit's row, with an overflowing width of its own
    assert k >= 20
    score[3 * nt + 1, 4, 11] = 89.0
    out, dets, after = _case("nonfinite", c)
    assert after == y.size and dets[k, 4] == np.inf and dets[k, 0] == -np.inf and dets[k, 2] == np.inf
    assert out["nonfinite_coords"] >= 2 * 9 + 2
    w = dets[:15, 2] - dets[:15, 0]
    with np.errstate(invalid="ignore"):
        assert w[0] == 0 and np.isfinite(w[3]) and w[3] > 1e38 and w[6] == np.inf and w[9] == np.inf and np.isnan(w[12])


# ------------------------------------------------------------------------------------------------ counter and cap
def test_three_maps_appended_through_one_counter():
    """Pyramid levels chain through *count: three maps of different geometry, shape and scale into one list, against the concatenation."""
    T = make_templates(4)
    parts = [Case(make_score(4, 5, 13, 0.8, 500), T, 0.8, 0.5, GEOS[1]), Case(make_score(4, 9, 70, 0.8, 501), T, 0.8, 1, GEOS[2]),
             Case(make_score(4, 1, 65, 0.8, 502), T, 0.8, 2, GEOS[3])]
    cap = sum(c.H * c.W * 4 for c in parts)
    runs = []
    for _ in range(2):
        dets, count = new_list(cap, 0)
        afters = []
        for c in parts:
            c.start, c.cap = (afters[-1] if afters else 0), cap
            launch(c, dets, count)
            afters.append(int(count.item()))
        runs.append((dets.cpu().numpy(), afters))
    assert runs[0][1] == runs[1][1] and runs[0][0].tobytes() == runs[1][0].tobytes()
    dets, afters = runs[0]
    assert 0 < afters[0] < afters[1] < afters[2]
    for i, c in enumerate(parts):
        c.start = afters[i - 1] if i else 0
        out = check(c, dets, afters[i], front=False, tail=(i == 2))            # a level's neighbours in the list are the other levels' rows
        report("decode_parity[counter_chain]", **out)
    want = np.concatenate([decode_ref.decode(c.score, T, c.vx, c.vt, 0.8, c.scale, c.stride, c.offset).rows for c in parts])
    assert want.shape[0] == afters[2] and np.array_equal(dets[:afters[2], 4], want[:, 4])


def _cap_case(start):
    score, T = make_score(3, 5, 13, 0.8, 510, density=0.2), make_templates(3)
    n = decode_ref.decode(score, T, np.ones(13, np.uint8), np.ones(3, np.uint8), 0.8, 0.7, (4, 8), (3, -2)).total
    return score, T, start + n


def test_incoming_count_is_where_the_rows_go():
    """A counter that arrives at 17: rows 0..16 keep their sentinel, the candidates follow from row 17."""
    score, T, total = _cap_case(17)
    out, _, after = _case("start_17", Case(score, T, 0.8, 0.7, GEOS[2], start=17))
    assert after == total and out["rows"] == total - 17 > 20


@pytest.mark.parametrize("start", [0, 17])
@pytest.mark.parametrize("cap", ["0", "1", "total-1", "total", "total+1"])
def test_cap(cap, start):
    """dets has `cap` rows and its rear guard right behind row cap - 1 (C ABI, exact workspace): the counter still comes back as the TRUE
    total, exactly rows [start, cap) are written and equal the restatement's first rows, nothing lands behind row cap - 1."""
    score, T, total = _cap_case(start)
    rows = {"0": 0, "1": 1, "total-1": total - 1, "total": total, "total+1": total + 1}[cap]
    out, _, after = _case("cap", Case(score, T, 0.8, 0.7, GEOS[2], start=start, cap=rows, direct=True))
    assert after == total and out["rows"] == max(min(total, rows) - start, 0)


def test_all_negative_map_moves_nothing():
    score = make_score(3, 5, 13, 0.8, 520)
    cls_view(score, 3)[...] -= 12.0
    out, _, after = _case("all_negative", Case(score, make_templates(3), 0.8, 1, GEOS[1], start=17, direct=True))
    assert after == 17 and out["rows"] == 0


# ------------------------------------------------------------------------------------------------ scan carry
SCAN_BLOCKS = (0, 1022, 1023, 1024, 1025, 1033)


@pytest.mark.parametrize("kind", ["planted_blocks", "uniform"])
def test_scan_carry_past_1024_blocks(kind):
    """nt = 2 on 130 x 509: 66 170 pixels = 1034 blocks, so decode_scan_kernel takes a second pass of its loop and the carry between the passes
    (and the incoming count, 17) decides where the rows of blocks 1024.. go.  Candidates only in blocks 0, 1022, 1023, 1024, 1025 and 1033 (the
    last one 58 pixels wide); then 1 % everywhere."""
    nt, H, W = 2, 130, 509
    assert (H * W + 63) // 64 == 1034
    if kind == "uniform":
        score = make_score(nt, H, W, 0.8, 600, density=0.01)
    else:
        hot = np.zeros(H * W, bool)                                            # pixels in block order
        for b in SCAN_BLOCKS:
            hot[64 * b:64 * (b + 1)] = True
        assert hot.sum() == 5 * 64 + 58
        score = make_score(nt, H, W, 0.8, 601, density=0.004, hot=np.repeat(hot, nt))
    c = Case(score, make_templates(nt), 0.8, 1, GEOS[1], start=17)
    out, dets, after = _case(f"scan_{kind}", c)
    assert out["rows"] > (1000 if kind == "uniform" else 400)
    if kind == "planted_blocks":
        ref = decode_ref.decode(c.score, c.T, c.vx, c.vt, 0.8, 1, c.stride, c.offset)
        blocks = (ref.index[0] * W + ref.index[1]) // 64
        assert set(blocks.tolist()) == set(SCAN_BLOCKS)


# ------------------------------------------------------------------------------------------------ the host wrappers
def _nhwc_case(H, W, seed):
    rng = np.random.RandomState(seed)
    ladder = np.linspace(-6.0, 3.0, H * W * 25 + 2)[1:-1].astype(np.float32)
    cls = rng.permutation(ladder).reshape(1, H, W, 25)
    reg = (rng.randn(1, H, W, 100) * 0.4).astype(np.float32)
    score = np.ascontiguousarray(np.concatenate([cls[0], reg[0]], axis=2).transpose(2, 0, 1))
    return cls, reg, score


def test_get_bboxes_with_an_asymmetric_receptive_field_and_the_template_mask(templates):
    """tinyfaces.models.utils.get_bboxes, the reference's call surface: rf is an argument there, and mask_axis="template" reaches valid_t."""
    from tinyfaces import ops
    from tinyfaces.models.utils import get_bboxes
    cls, reg, score = _nhwc_case(9, 40, 700)
    rf = {"stride": [8, 16], "offset": [-1, 5]}
    vx, vt = ops.template_masks(templates, 0.5, 40, "template")
    assert vx.all() and 0 < vt.sum() < 25
    ref = decode_ref.decode(score, templates, vx, vt, 0.65, 0.5, rf["stride"], rf["offset"])
    assert ref.undecided.sum() == 0 and ref.rows.shape[0] > 100
    b, s = get_bboxes(cls, reg, np.zeros_like(cls), templates, 0.65, rf, 0.5, mask_axis="template")
    assert b.shape == (ref.rows.shape[0], 4) and np.array_equal(s, ref.rows[:, 4:5].astype(np.float32))
    bound = decode_ref.box_bound(ref.rows, ref.half)
    assert np.all(np.abs(b - ref.rows[:, :4]) <= bound)
    report("decode_parity[get_bboxes]", rows=b.shape[0], box_err_of_bound=float((np.abs(b - ref.rows[:, :4]) / bound).max()))


def test_mirrored_level_is_decoded_then_mirrored_back(templates):
    """evaluation._decode_levels(mirrored=True) on one synthetic level: ops.decode_compact, then ops.boxes_unflip_ on the rows the level
    appended, with an asymmetric receptive field.  Equals the restatement of that map with x1' = c - x2, x2' = c - x1, c = (image width
    - 1) / scale, row for row (the map handed in IS the mirrored level's; the rows keep the order the decode gave them)."""
    from tinyfaces import evaluation
    cls, reg, score = _nhwc_case(7, 31, 710)
    rf = {"stride": [4, 8], "offset": [3, -2]}
    scale, thr, width = 2, 0.65, 251
    c = (width - 1) * (1 / scale)
    out = torch.from_numpy(score)[None].to(DEV)
    img = torch.zeros(1, 3, 60, width)
    t_d = torch.from_numpy(np.ascontiguousarray(templates)).to(DEV)
    case = Case(score, np.asarray(templates), thr, scale, (4, 8, 3, -2), vt=_template_vt(templates, scale), start=5)

    def mirror(rows, bound):
        m = rows.copy()
        m[:, 0], m[:, 2] = c - rows[:, 2], c - rows[:, 0]
        b = bound.copy()
        b[:, 0], b[:, 2] = bound[:, 2] + 4 * np.spacing(np.abs(m[:, 0])), bound[:, 0] + 4 * np.spacing(np.abs(m[:, 2]))
        return m, b

    runs = []
    for _ in range(2):
        dets, count = new_list(case.cap, case.start)
        evaluation._decode_levels(lambda x: out, [(scale, img)], templates, t_d, rf, thr, "template", dets, count, torch.device(DEV), mirrored=True)
        torch.cuda.synchronize()
        assert_guards(dets, "dets"); assert_guards(count, "count")
        runs.append((dets.cpu().numpy(), int(count.item())))
    assert runs[0][1] == runs[1][1] and runs[0][0].tobytes() == runs[1][0].tobytes()
    res = check(case, runs[0][0], runs[0][1], transform=mirror)
    assert res["rows"] > 100
    report("decode_parity[mirrored_level]", **res)


def _template_vt(templates, scale):
    from tinyfaces import ops
    return ops.template_masks(templates, scale, 31, "template")[1]


# ------------------------------------------------------------------------------------------------ the nt limit
def test_nt_52_is_refused_on_the_host_and_nothing_moves(hip):
    """nt = 52: the write pass's slab would not fit 64 KiB.  TF_ERR_UNSUPPORTED before anything is enqueued: the counter keeps its 17, dets its
    fill, and no launch error is left behind for the next call."""
    nt, H, W = 52, 3, 7
    l = hip.lib()
    dets, count = new_list(H * W * nt + 17, 17)
    score = torch.zeros(5 * nt, H, W, device=DEV) + 5.0                         # every entry a candidate, had it run
    T = torch.from_numpy(make_templates(nt)).to(DEV)
    vx, vt = torch.ones(W, dtype=torch.uint8, device=DEV), torch.ones(nt, dtype=torch.uint8, device=DEV)
    wsb = l.tf_decode_workspace_bytes(H, W, nt)
    ws = guarded_workspace(wsb, DEV)
    rc = l.tf_decode_compact(score.data_ptr(), nt, H, W, T.data_ptr(), 5, vx.data_ptr(), vt.data_ptr(), 0.5, 1.0, 8, 8, -1, -1, dets.data_ptr(),
                             count.data_ptr(), dets.shape[0], ws.data_ptr(), wsb, hip.stream())
    torch.cuda.synchronize()
    assert rc == -3                                                              # TF_ERR_UNSUPPORTED
    assert int(count.item()) == 17
    d = dets.cpu().numpy()
    assert np.all(d[:17] == SENTINEL) and np.all(d[17:].view(np.uint8) == 0xFF)
    assert np.all(ws.cpu().numpy() == 0xFF)
    assert_guards(dets, "dets"); assert_guards(count, "count"); assert_guards(ws, "workspace")
    # the same call with the largest nt that is taken goes through
    out, _, after = _case("nt_51_direct", Case(make_score(51, H, W, 0.8, 800), make_templates(51), 0.8, 1, GEOS[0], start=17, direct=True))
    assert after > 17
