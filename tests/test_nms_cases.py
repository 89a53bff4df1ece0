"""CPU: the cases of tests/nms_cases.py before any kernel sees them.  The closed forms against oracle/nms.py (they do not come from it, so
this tests the oracle); the oracle's visiting order against torch.sort(descending=True, stable=True), the sort of the reference's CPU
kernel, on every score vector of the case file, NaN and infinities included; a pure-Python double loop against both on the small cases; and
the rank kernel's counting formula restated in numpy: a permutation, and torch.sort's, once its compares order NaN as torch.sort does."""
import numpy as np
import pytest
import torch

import nms_cases as nc
from oracle import nms as onms

CLOSED = ("chain", "suppressed_suppressor", "far_pair", "exact_threshold", "threshold_edges")


def _closed_cases():
    return [(f, name) for f in CLOSED for name in nc.FAMILIES[f]()]


@pytest.mark.parametrize("fam,name", _closed_cases(), ids=[n for _, n in _closed_cases()])
def test_closed_form_equals_oracle(fam, name):
    case = nc.family(fam)[name]
    boxes, scores, thr, expected = case
    assert expected is not None and boxes.shape == (scores.size, 4) and boxes.dtype == scores.dtype == np.float64
    assert np.array_equal(nc.oracle_keep(name, case), expected)


def test_closed_form_counts():
    """The keep sizes the chain and the far pair are stated with: 3000 boxes keep 1500 / 3000 / 3000 / 1000 at thr 0.3 / 0.5 / 1.0 / 0.0."""
    assert [nc.chain(3000, t)[3].size for t in (0.3, 0.5, 1.0, 0.0)] == [1500, 3000, 3000, 1000]
    assert nc.far_pair(3000)[3].size == 2999
    for r1, r2 in nc.SUPPRESSOR_RANKS:
        assert nc.suppressed_suppressor(r1, r2)[3].size == r2 + 4


def test_structured_cases_are_shuffled():
    """perm_seed moves the input order and the expected indices with it: the same boxes are kept, and order[] is not the identity."""
    for build in (lambda s: nc.chain(65, 0.3, s), lambda s: nc.suppressed_suppressor(63, 64, perm_seed=s), lambda s: nc.far_pair(1025, perm_seed=s),
                  lambda s: nc.threshold_edges("-0.1", s), lambda s: nc.exact_threshold(0.5, 0.5, (63, 64), s)):
        (b0, s0, _, k0), (b1, s1, _, k1) = build(None), build(3)
        assert np.array_equal(np.argsort(-s0), np.arange(s0.size)) and not np.array_equal(np.argsort(-s1), np.arange(s1.size))
        assert np.array_equal(b0[k0], b1[k1]) and np.array_equal(s0[k0], s1[k1])
        assert np.array_equal(b0[np.argsort(-s0)], b1[np.argsort(-s1)])


@pytest.mark.parametrize("name", list(nc.score_vectors()))
def test_oracle_order_is_torch_sort(name):
    """oracle.nms visits the boxes in the order the reference's kernel does: scores.sort(stable=True, descending=True)."""
    s = nc.score_vectors()[name]
    want = torch.sort(torch.from_numpy(s), descending=True, stable=True).indices.numpy()
    assert np.array_equal(onms.visiting_order(s), want)
    if name == "nonfinite-vec8":
        assert want.tolist() == nc.VEC8_ORDER


def test_oracle_keeps_nan_scores_first():
    """Two overlapping boxes: the one with the NaN score is visited first and suppresses the other, whatever the other's score."""
    boxes = np.array([[0.0, 0, 10, 10], [1.0, 0, 11, 10]])
    assert onms.nms(boxes, np.array([np.inf, np.nan]), 0.3).tolist() == [1]
    assert onms.nms(boxes, np.array([np.nan, np.nan]), 0.3).tolist() == [0]
    assert onms.nms(boxes, np.array([-0.0, 0.0]), 0.3).tolist() == [0]


@pytest.mark.parametrize("name", [k for k, v in nc.score_vectors().items() if v.size <= 2100])
def test_rank_formula_is_a_permutation(name):
    """rank[i] = #{j : s_j > s_i or (s_j == s_i and j < i)} with torch.sort's compares scatters 0..n-1 into torch.sort's order."""
    s = nc.score_vectors()[name]
    rank = nc.kernel_rank(s)
    assert np.array_equal(np.sort(rank), np.arange(s.size))
    order = np.empty(s.size, np.int64)
    order[rank] = np.arange(s.size)
    assert np.array_equal(order, onms.visiting_order(s))


def test_rank_formula_with_ieee_compares_is_not():
    """What the formula gives when a NaN compares false against everything: three boxes of VEC8 share rank 0, ranks 6 and 7 are nobody's."""
    assert nc.kernel_rank(nc.VEC8, nan_aware=False).tolist() == [2, 0, 1, 0, 5, 0, 3, 4]
    assert nc.kernel_rank(nc.VEC8).tolist() == [4, 0, 3, 1, 7, 2, 5, 6]


def _small_cases():
    out = {}
    for n in (64, 65):
        for thr in nc.CHAIN_STEP:
            out[f"chain-n{n}-thr{thr}"] = nc.chain(n, thr, perm_seed=n)
    out.update({k: v for k, v in nc.suppressed_suppressor_cases().items() if v[1].size <= 300})
    out.update(nc.exact_threshold_cases())
    out.update(nc.threshold_edges_cases())
    out.update(nc.degenerate_cases(n=300))
    out.update(nc.tie_cases(sizes=(257,)))
    out["nonfinite-vec8"] = nc.non_finite("vec8")
    s = nc.non_finite_scores("n2100-few")[1900:2200]        # 200 scores around the NaNs at 2046..2049, the +-inf at 2050 / 2051 and the NaN at 2099
    out["nonfinite-n200"] = (nc.clustered_boxes(s.size, 5, centres=12), s, 0.3, None)
    return out


SMALL = _small_cases()


@pytest.mark.parametrize("name", list(SMALL))
def test_double_loop_equals_oracle(name):
    boxes, scores, thr, expected = SMALL[name]
    got = nc.brute_force_nms(boxes, scores, thr)
    assert np.array_equal(got, onms.nms(boxes, scores, thr))
    if expected is not None:
        assert np.array_equal(got, expected)
    assert 0 < got.size <= scores.size


def test_small_cases_exercise_what_they_name():
    """The inputs are what the families say: ties, NaN IoUs, negative areas, suppressed boxes at every threshold but >= 1."""
    b, s, _, _ = nc.degenerate(0.3)
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    assert (area == 0).sum() > 100 and (area < 0).sum() > 100 and np.unique(s).size < 100
    assert np.unique(b, axis=0).shape[0] < b.shape[0] - 100
    keeps = [nc.oracle_keep(k, v).size for k, v in nc.family("degenerate").items()]
    assert keeps[0] < keeps[1] < keeps[2] < keeps[3] <= keeps[4] == 2000, keeps
    for name in nc.NON_FINITE:
        v = nc.non_finite_scores(name)
        assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any()
    assert np.isnan(nc.non_finite_scores("n2100-mostly")).sum() > 2048
