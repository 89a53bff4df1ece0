"""CPU: what pins tests/decode_ref.py, the float64 restatement tests/test_gpu_decode.py holds csrc/decode.hip to.

  * it reproduces the four golden decode fixtures (produced by the reference's own source): same candidates, same order, boxes within the
    bar test_decode_golden uses (numpy's float32 exp against a rounded float64 exp: <= 1 fp32 ulp of exp());
  * it equals oracle.decode.get_bboxes where the fixtures cannot reach: a receptive field whose strides and offsets differ per axis, on
    both mask axes;
  * the width of its undecided band (decode_ref.BAND fp32 spacings around the threshold) rests on evidence, repeated here."""
import numpy as np
import pytest
import torch

import decode_ref
from oracle import decode as odec

THRS = (0.03, 0.5, 0.65, 0.8, 0.97)


def _chw(score_cls, score_reg):
    return np.ascontiguousarray(np.concatenate([score_cls[0], score_reg[0]], axis=2).transpose(2, 0, 1))


def _masks(templates, scale, W, mask_axis):
    inv = odec.invalid_template_ids(templates, scale)
    vx, vt = np.ones(W, np.uint8), np.ones(templates.shape[0], np.uint8)
    (vx if mask_axis == "w" else vt)[inv] = 0
    return vx, vt


def _assert_same(r, boxes, scores):
    assert r.rows.shape[0] == boxes.shape[0]
    assert np.array_equal(r.rows[:, 4].astype(np.float32).reshape(-1, 1), scores)
    if boxes.shape[0]:
        size = float(max((boxes[:, 2] - boxes[:, 0]).max(), (boxes[:, 3] - boxes[:, 1]).max()))
        assert np.abs(r.rows[:, :4] - boxes).max() <= 1.3e-7 * size


@pytest.mark.parametrize("ci", range(4))
def test_restatement_reproduces_the_golden_fixtures(golden, ci):
    from oracle.targets import RF
    g, t, tag = golden("decode"), golden("targets")["templates"], f"d{ci}"
    cls, reg, scale = g[f"{tag}_score_cls"], g[f"{tag}_score_reg"], float(g[f"{tag}_scale"])
    vx, vt = _masks(t, scale, cls.shape[2], "w")
    r = decode_ref.decode(_chw(cls, reg), t, vx, vt, float(g[f"{tag}_thr"]), scale, RF["stride"], RF["offset"])
    _assert_same(r, g[f"{tag}_boxes"], g[f"{tag}_scores"])
    assert r.total == r.rows.shape[0] == r.written and r.candidate.sum() == r.total


@pytest.mark.parametrize("mask_axis", ["w", "template"])
@pytest.mark.parametrize("stride,offset,scale,seed", [((8, 16), (-1, 5), 1, 0), ((4, 8), (3, -2), 0.5, 1)])
def test_restatement_equals_the_oracle_beyond_the_symmetric_receptive_field(golden, stride, offset, scale, seed, mask_axis):
    t = golden("targets")["templates"]
    rng = np.random.RandomState(100 + seed)
    H, W, nt = 9, 40, 25
    cls = (rng.randn(1, H, W, nt) * 1.5).astype(np.float32)
    reg = (rng.randn(1, H, W, 4 * nt) * 0.3).astype(np.float32)
    rf = {"stride": list(stride), "offset": list(offset)}
    vx, vt = _masks(t, scale, W, mask_axis)
    r = decode_ref.decode(_chw(cls, reg), t, vx, vt, 0.8, scale, stride, offset, start=3, cap=40)
    assert r.undecided.sum() == 0                               # else the oracle's fp32 sigmoid may decide otherwise: pick another seed
    b, s = odec.get_bboxes(cls, reg, decode_ref.sigmoid_f32(cls), t, 0.8, rf, scale, mask_axis=mask_axis)
    assert b.shape[0] > 40
    _assert_same(r, b, s)
    assert r.total == 3 + b.shape[0] and r.written == 37
    # a swap of the two axes of the receptive field is a different answer on these cases (it is not on the project's (8, 8), (-1, -1))
    sw = decode_ref.decode(_chw(cls, reg), t, vx, vt, 0.8, scale, stride[::-1], offset, start=3, cap=40)
    so = decode_ref.decode(_chw(cls, reg), t, vx, vt, 0.8, scale, stride, offset[::-1], start=3, cap=40)
    assert np.abs(sw.rows[:, :4] - b).max() > 1 and np.abs(so.rows[:, :4] - b).max() > 1


def test_cap_and_start_only_decide_what_is_written():
    rng = np.random.RandomState(5)
    score = rng.randn(15, 4, 6).astype(np.float32)
    T = np.array([[0, 0, 9, 19, 1], [0, 0, 4, 6, 1], [-3, -2, 3, 8, 1]], np.float64)
    full = decode_ref.decode(score, T, np.ones(6, np.uint8), np.ones(3, np.uint8), 0.5, 2, (4, 8), (3, -2))
    n = full.rows.shape[0]
    assert 10 < n < 72
    for start, cap, want in [(0, 0, 0), (0, 1, 1), (0, n - 1, n - 1), (0, n, n), (0, n + 1, n), (17, 0, 0), (17, 17, 0), (17, 18, 1),
                             (17, 17 + n, n), (17, 16 + n, n - 1)]:
        r = decode_ref.decode(score, T, np.ones(6, np.uint8), np.ones(3, np.uint8), 0.5, 2, (4, 8), (3, -2), start=start, cap=cap)
        assert r.total == start + n and r.written == want and np.array_equal(r.rows, full.rows)
    # a negative threshold admits the masked entries too (probability 0 > thr), all of them in C order
    r = decode_ref.decode(score, T, np.zeros(6, np.uint8), np.zeros(3, np.uint8), -0.5, 2, (4, 8), (3, -2))
    assert r.total == 72 and np.array_equal(r.rows[:, 4], score[:3].transpose(1, 2, 0).reshape(-1).astype(np.float64))
    assert decode_ref.decode(score, T, np.zeros(6, np.uint8), np.ones(3, np.uint8), 0.0, 2, (4, 8), (3, -2)).total == 0


def _neighbourhood(thr, reach):
    """The float32 logits within `reach` ulps of float32(logit(thr)), ascending."""
    x = decode_ref.ulp_shift(decode_ref.logit32(thr), np.arange(-reach, reach + 1))
    assert np.all(np.diff(x.astype(np.float64)) > 0) and x[reach] == decode_ref.logit32(thr)
    return x


@pytest.mark.parametrize("thr", THRS)
def test_the_undecided_band_rests_on_evidence(thr):
    """BAND: every float32 logit within 4096 ulps of logit(thr) -- a superset of any draw within +-64 ulps --, plus a fixed-seed draw of
    200 000 ordinary logits.  The fp32 expression of the kernel stays within 2.2 spacings of float32(thr) of the float64 probability
    within +-64 ulps (2.5 within +-4096: always below BAND), and outside the band neither it nor torch.sigmoid decides an entry
    differently from float64; inside the band the two DO differ from each other (next test), which is why the kernel is held to neither."""
    t32 = np.float32(thr)
    band = decode_ref.BAND * np.float64(np.spacing(t32))
    near = _neighbourhood(thr, 4096)
    x = np.concatenate([near, (np.random.RandomState(7).randn(200000) * 3).astype(np.float32)])
    p64 = 1.0 / (1.0 + np.exp(-x.astype(np.float64)))
    pk = decode_ref.sigmoid_f32(x)
    pt = torch.sigmoid(torch.from_numpy(x)).numpy()
    assert pk.dtype == np.float32 and pt.dtype == np.float32
    ulps = np.abs(pk[:near.size].astype(np.float64) - p64[:near.size]) / np.float64(np.spacing(t32))
    assert ulps[4096 - 64:4096 + 65].max() <= 2.2, ulps[4096 - 64:4096 + 65].max()      # within +-64 ulps of logit(thr)
    assert ulps.max() < decode_ref.BAND, ulps.max()          # an error below the band's width cannot flip a decision outside the band
    outside = np.abs(p64 - np.float64(t32)) > band
    want = p64 > np.float64(t32)
    assert outside.sum() > 100000 and (~outside[:near.size]).sum() >= 1         # both sides of the band's edge are populated
    assert np.array_equal((pk > t32)[outside], want[outside])
    assert np.array_equal((pt > t32)[outside], want[outside])


def test_kernel_form_and_torch_sigmoid_disagree_inside_the_band():
    n = 0
    for thr in THRS:
        x = _neighbourhood(thr, 64)
        n += int(((decode_ref.sigmoid_f32(x) > np.float32(thr)) != (torch.sigmoid(torch.from_numpy(x)).numpy() > np.float32(thr))).sum())
    assert n > 0
