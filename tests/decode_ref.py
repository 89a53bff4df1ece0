"""Float64 numpy restatement of the score-map decode (csrc/decode.hip, tf_decode_compact) as include/tinyfaces_hip.h states it: sigmoid,
threshold, template mask, candidates in C order over (y, x, template), regression refinement into float64 boxes.  Test infrastructure: plain
numpy over a (y, x, t) array, no blocks, no slabs, nothing from the package or from oracle/; never imported by the package.

What it restates, per entry (y, x, t) of a score map (5nt, H, W) float32 (channel t: class logit, nt + t .. 4nt + t: tx, ty, tw, th):

    prob = 1 / (1 + exp(-float64(logit))), 0 where valid_x[x] & valid_t[t] is 0
    candidate  <=>  prob > float64(float32(thr))                               (a NaN never is)
    cy = y * sty + ofy, cx = x * stx + ofx;  cw = T[t,2] - T[t,0] + 1, ch = T[t,3] - T[t,1] + 1
    rcx = cx + cw * tx, rcy = cy + ch * ty;  rcw = cw * float32(exp(float64(tw))), rch = ch * float32(exp(float64(th)))
    row = ((rcx - rcw/2) * f, (rcy - rch/2) * f, (rcx + rcw/2) * f, (rcy + rch/2) * f, logit),  f = 1 / scale

The kernel thresholds an fp32 sigmoid, this file a float64 one: an entry whose float64 probability lies within BAND fp32 spacings of the
threshold may legitimately be decided either way (`undecided`).  BAND = 4 is pinned by tests/test_decode_ref.py: the fp32 expression
1 / (1 + expf(-x)) stays within 2.2 fp32 ulps of the float64 value, and neither it nor torch.sigmoid decides an entry outside the band
differently from float64."""
from typing import NamedTuple

import numpy as np

BAND = 4


class Decoded(NamedTuple):
    rows: np.ndarray        # (N, 5) float64: every candidate in C order over (y, x, t), whatever the cap
    total: int              # start + N: the TRUE total the device counter must hold afterwards
    written: int            # rows[:written] land in dets[start : start + written]; rows at or beyond `cap` are not written
    undecided: np.ndarray   # (H, W, nt) bool
    index: tuple            # (y, x, t) of the rows
    half: np.ndarray        # (N, 2) float64: (rcw / 2, rch / 2) * (1 / scale), what the box tolerance is expressed in
    candidate: np.ndarray   # (H, W, nt) bool


def thr32(thr):
    return np.float64(np.float32(thr))


def probability(score, nt, valid_x, valid_t):
    """(H, W, nt) float64 probabilities of the class logits score[:nt], 0 where masked."""
    logit = np.asarray(score)[:nt].transpose(1, 2, 0).astype(np.float64)
    with np.errstate(all="ignore"):
        prob = 1.0 / (1.0 + np.exp(-logit))
    live = (np.asarray(valid_x) != 0)[None, :, None] & (np.asarray(valid_t) != 0)[None, None, :]
    return np.where(live, prob, 0.0), np.broadcast_to(live, prob.shape)


def rows_at(score, templates, y, x, t, scale, stride, offset):
    """The rows of the entries (y, x, t) (index arrays of one length), candidates or not, and their half sizes."""
    score = np.asarray(score)
    assert score.dtype == np.float32 and score.ndim == 3 and score.shape[0] % 5 == 0
    nt = score.shape[0] // 5
    T = np.asarray(templates, dtype=np.float64)
    y, x, t = (np.asarray(a, dtype=np.int64) for a in (y, x, t))
    cy = (y * int(stride[0]) + int(offset[0])).astype(np.float64)
    cx = (x * int(stride[1]) + int(offset[1])).astype(np.float64)
    cw = T[t, 2] - T[t, 0] + 1.0
    ch = T[t, 3] - T[t, 1] + 1.0
    tx, ty, tw, th = (score[k * nt + t, y, x].astype(np.float64) for k in (1, 2, 3, 4))
    with np.errstate(all="ignore"):
        rcx, rcy = cx + cw * tx, cy + ch * ty
        rcw = cw * np.exp(tw).astype(np.float32).astype(np.float64)
        rch = ch * np.exp(th).astype(np.float32).astype(np.float64)
        f = 1.0 / np.float64(scale)
        rows = np.stack([(rcx - rcw / 2) * f, (rcy - rch / 2) * f, (rcx + rcw / 2) * f, (rcy + rch / 2) * f,
                         score[t, y, x].astype(np.float64)], axis=1)
        half = np.stack([rcw / 2 * f, rch / 2 * f], axis=1)
    return rows, half


def decode(score, templates, valid_x, valid_t, thr, scale, stride, offset, start=0, cap=None):
    """-> Decoded.  score (5nt, H, W) float32, templates (nt, tstride) float64 (columns 0..3 are read), valid_x (W,), valid_t (nt,),
    stride = (sty, stx), offset = (ofy, ofx); start: the incoming counter, cap: the rows `dets` has (None: room for everything)."""
    score = np.asarray(score)
    nt = np.asarray(templates).shape[0]
    assert score.shape[0] == 5 * nt
    prob, live = probability(score, nt, valid_x, valid_t)
    th = thr32(thr)
    with np.errstate(invalid="ignore"):
        cand = prob > th
        undecided = live & (np.abs(prob - th) <= BAND * np.abs(np.float64(np.spacing(np.float32(thr)))))
    y, x, t = np.nonzero(cand)                                   # C order over (y, x, t)
    rows, half = rows_at(score, templates, y, x, t, scale, stride, offset)
    n = rows.shape[0]
    written = n if cap is None else int(min(max(int(cap) - int(start), 0), n))
    return Decoded(rows, int(start) + n, written, undecided, (y, x, t), half, cand)


def box_bound(rows, half):
    """(N, 4) float64: what a box coordinate may differ by.  One fp32 ulp of the rounded exp -- which a last-bit difference between two
    float64 exp routines can flip -- moves a corner by 2^-23 * (rcw / 2 or rch / 2) / scale; the float64 arithmetic around it (no FMA
    contraction on either side) is allowed 4 ulps of the coordinate."""
    with np.errstate(all="ignore"):
        return 2.0 ** -23 * np.abs(half[:, [0, 1, 0, 1]]) + 4 * np.spacing(np.abs(rows[:, :4]))


def logit32(thr):
    """float32(logit(float32(thr))): the logit the threshold is planted around."""
    t = np.float64(np.float32(thr))
    return np.float32(np.log(t) - np.log1p(-t))


def ulp_shift(x, k):
    """The float32 `k` representable steps above x (below for k < 0), through 0 and the denormals; x scalar, k an integer array."""
    b = np.int64(np.array([x], dtype=np.float32).view(np.int32)[0])
    o = (b if b >= 0 else -(b & 0x7FFFFFFF)) + np.asarray(k, dtype=np.int64)     # an integer line on which float32 order is integer order
    back = np.where(o >= 0, o, (-o) | 0x80000000).astype(np.uint32)
    return back.view(np.float32)


def sigmoid_f32(x):
    """numpy float32 emulation of the kernel's 1.0f / (1.0f + expf(-x))."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        return np.float32(1) / (np.float32(1) + np.exp(-x))
