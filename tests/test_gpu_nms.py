"""-m gpu: tf_nms_f64 / tf_nms_f64_batched (csrc/nms.hip) at operator level, on the named cases of tests/nms_cases.py (its header says which
part of the kernel each family is aimed at; tests/test_nms_cases.py checks the cases themselves on the CPU).

Every case goes through ops.nms, and the cases of a family are packed, several to a call, through ops.nms_batched.  The result is compared
with np.array_equal -- identical indices in identical order, no tolerance -- against oracle/nms.py and, where the case has one, against its
closed form.  Every call, whatever its scores, also has to return a keep without duplicates whose indices lie inside their segment, and the
same tensor when it is made again.  These checks read the returned keep on the host and never index with it."""
import numpy as np
import pytest
import torch

import nms_cases as nc
from gpu_util import report

pytestmark = pytest.mark.gpu

DEV = "cuda"
LARGER = "ties-n16385-round1"          # the call made in front of the non-finite cases: it leaves 16 385 order[] entries in the shared workspace


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _check_keep(got, lo, hi, what):
    assert got.dtype == np.int64, what
    assert np.unique(got).size == got.size, f"{what}: an index is kept twice"
    assert got.size == 0 or (lo <= got.min() and got.max() < hi), f"{what}: an index outside [{lo}, {hi})"


def _single(name, case):
    """The case through ops.nms, twice.  Returns the keep (numpy)."""
    from tinyfaces import ops
    boxes, scores, thr, expected = case
    want = nc.oracle_keep(name, case)
    B, S = _dev(boxes), _dev(scores)
    first, second = ops.nms(B, S, thr), ops.nms(B, S, thr)
    got = first.cpu().numpy()
    exact = np.array_equal(got, want) and (expected is None or np.array_equal(got, expected))
    report("nms_case", case=name, n=scores.size, kept=got.size, exact=exact)
    _check_keep(got, 0, scores.size, name)
    assert torch.equal(first, second), f"{name}: a second call differs"
    assert np.array_equal(got, want), f"{name}: differs from the oracle"
    if expected is not None:
        assert np.array_equal(got, expected), f"{name}: differs from the closed form"
    return got


def _batched(tag, cases, empty_at=None, singles=False):
    """[(name, case)] of ONE threshold as the segments of one ops.nms_batched call (an empty segment in front of position empty_at),
    twice.  singles: every segment also against ops.nms on its own slice."""
    from tinyfaces import ops
    cases = list(cases)
    if empty_at is not None:
        cases.insert(empty_at, (f"{tag}-empty", (np.empty((0, 4)), np.empty(0), cases[0][1][2], np.empty(0, np.int64))))
    thr = cases[0][1][2]
    assert all(np.float64(c[2]).tobytes() == np.float64(thr).tobytes() for _, c in cases)
    sizes = [c[1].size for _, c in cases]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    B, S = _dev(np.concatenate([c[0] for _, c in cases])), _dev(np.concatenate([c[1] for _, c in cases]))
    first, second = ops.nms_batched(B, S, offs.tolist(), thr), ops.nms_batched(B, S, offs.tolist(), thr)
    assert len(first) == len(second) == len(cases)
    bad = []
    for k, ((name, case), n, o) in enumerate(zip(cases, sizes, offs)):
        got = first[k].cpu().numpy()
        want = nc.oracle_keep(name, case) if n else np.empty(0, np.int64)
        exact = np.array_equal(got - o, want) and (case[3] is None or np.array_equal(got - o, case[3]))
        report("nms_case_batched", call=tag, segment=k, case=name, n=n, kept=got.size, exact=exact)
        _check_keep(got, o, o + n, f"{tag} segment {k} ({name})")
        assert torch.equal(first[k], second[k]), f"{tag} segment {k} ({name}): a second call differs"
        if not exact:
            bad.append(name)
        if singles and n:
            alone = ops.nms(B[o:o + n].contiguous(), S[o:o + n].contiguous(), thr).cpu().numpy()
            assert np.array_equal(alone + o, got), f"{tag} segment {k} ({name}): differs from the one-list call"
    assert not bad, f"{tag}: segments that differ from the oracle or the closed form: {bad}"


def _by_threshold(cases):
    groups = {}
    for name, case in cases.items():
        groups.setdefault(np.float64(case[2]).tobytes(), []).append((name, case))
    return list(groups.values())


def _family_params(fam):
    return pytest.mark.parametrize("name", list(nc.FAMILIES[fam]()))


# ------------------------------------------------------------------------------------------------ one list per call
@_family_params("chain")
def test_chain(name):
    """Kept rows in every chunk, each striking the next one: resolve across 64-box chunks, push across 1024-box super-chunks."""
    _single(name, nc.family("chain")[name])


@_family_params("suppressed_suppressor")
def test_suppressed_suppressor(name):
    """A box that was suppressed suppresses nothing, in the same chunk, the next chunk and the next super-chunk."""
    _single(name, nc.family("suppressed_suppressor")[name])


@_family_params("far_pair")
def test_far_pair(name):
    """Rank 0 suppresses rank n - 1 through the push kernel alone."""
    _single(name, nc.family("far_pair")[name])


@_family_params("exact_threshold")
def test_exact_threshold(name):
    """An IoU equal to the threshold does not suppress; one ulp less of threshold does."""
    _single(name, nc.family("exact_threshold")[name])


@_family_params("threshold_edges")
def test_threshold_edges(name):
    """thr = 0.0 and -0.0, a negative one (disjoint boxes are suppressed, a 0 / 0 IoU is not), 1.0 and 1.5 (nothing is)."""
    _single(name, nc.family("threshold_edges")[name])


@_family_params("degenerate")
def test_degenerate(name):
    """Zero-width, inverted and duplicate boxes with tied scores at thr = -0.5, 0.0, 0.3, 0.999, 1.0: whatever the oracle keeps."""
    _single(name, nc.family("degenerate")[name])


@_family_params("ties")
def test_ties(name):
    """Tied scores at the sizes where the rank kernel changes path.  Scores that are all equal (0.0, or +0.0 and -0.0) keep input order."""
    got = _single(name, nc.family("ties")[name])
    if name.endswith("zeros") or name.endswith("signed_zero"):
        assert np.all(np.diff(got) > 0), f"{name}: all scores tie, the keep must be strictly increasing"


@_family_params("non_finite")
def test_non_finite(name):
    """NaN, +inf and -inf scores, behind a call on 16 385 boxes that leaves its order[] in the workspace: a rank that is not a permutation
    would leave slots of that call in place, indices outside a shorter list among them."""
    _single(LARGER, nc.family("ties")[LARGER])
    _single(name, nc.family("non_finite")[name])


# ------------------------------------------------------------------------------------------------ several lists per call
@pytest.mark.parametrize("fam", [f for f in nc.FAMILIES if f != "non_finite"])
def test_family_batched(fam):
    """The cases of a family as the segments of one call per threshold."""
    for g, group in enumerate(_by_threshold(nc.family(fam))):
        _batched(f"{fam}-{g}", group)


def test_non_finite_batched():
    """The non-finite cases in one call, in both orders, again behind the larger call."""
    group = list(nc.family("non_finite").items())
    _single(LARGER, nc.family("ties")[LARGER])
    _batched("non_finite-forward", [c for c in group if c[1][1].size < 16385])        # shorter than the larger call in total: its slots are still there
    _batched("non_finite-all", group)
    _batched("non_finite-reverse", group[::-1], empty_at=2)


@pytest.mark.parametrize("kind", nc.LAYOUT_SCORES)
def test_batched_layouts(kind):
    """Segments of 1, 63, 1025 and 16 385 boxes in one call: the small ones run under the four-boxes-per-thread rank kernel.  Then the same
    four in reverse with an empty segment in the middle.  Every segment equals the one-list call on its own slice."""
    group = list(nc.layout_segments(kind).items())
    assert [c[1].size for _, c in group] == list(nc.LAYOUT_SIZES)
    _batched(f"layout-{kind}-forward", group, singles=True)
    _batched(f"layout-{kind}-reverse", group[::-1], empty_at=2, singles=True)
