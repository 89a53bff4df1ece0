"""CPU: the host side of the pre-NMS top-k and the detection cap (csrc/topk.hip, the *_capped Soft-NMS entries): the numpy restatement
(tests/topk_ref.py) on hand-written cases, the identity that ties the cut to the hard NMS, the new symbols and keywords, evaluate_model.py's
flags, and the refusals that fire without a device.  The kernels run in tests/test_gpu_topk.py."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import topk_ref
import vote_ref
from oracle.nms import nms as oracle_nms

INF, NAN = float("inf"), float("nan")


# --------------------------------------------------------------------------- the restatement
def test_reference_hand_written_cases():
    sel = lambda s, k: topk_ref.topk_select(np.array(s, dtype=np.float64), k).tolist()      # noqa: E731
    assert sel([0.1, 0.9, 0.5, 0.7], 2) == [1, 3]                          # ascending index, not score order
    assert sel([0.1, 0.9, 0.5, 0.7], 1) == [1]
    assert sel([0.5, 0.5, 0.5, 0.5], 2) == [0, 1]                          # ties: the lower index
    assert sel([0.5, 0.9, 0.5, 0.9, 0.5], 3) == [0, 1, 3]
    assert sel([0.0, -0.0, 0.0, -0.0], 2) == [0, 1] and sel([-0.0, 0.0, 1.0], 2) == [0, 2]  # -0.0 == +0.0
    assert sel([-INF, INF, 0.0, -1.0], 1) == [1] and sel([-INF, INF, 0.0, -1.0], 3) == [1, 2, 3]
    assert sel([NAN, -INF, 1.0], 2) == [1, 2]                              # a NaN ranks behind -inf
    assert sel([NAN, 2.0, NAN, 1.0], 3) == [0, 1, 3]                       # NaNs among themselves: by index
    assert sel([NAN, NAN, NAN], 2) == [0, 1]
    assert sel([3.0, 1.0, 2.0], 3) == [0, 1, 2] and sel([3.0, 1.0, 2.0], 4) == [0, 1, 2]   # k >= n: identity
    assert sel([], 3) == []
    assert sel([5e-324, 0.0, -5e-324], 1) == [0] and sel([5e-324, 0.0, -5e-324], 2) == [0, 1]
    with pytest.raises(ValueError):
        topk_ref.topk_select(np.zeros(3), 0)
    idx, new = topk_ref.topk_select_batched(np.array([1.0, 3.0, 2.0, 9.0, 5.0, 4.0, 6.0]), [0, 3, 3, 7], 2)
    assert idx.tolist() == [1, 2, 3, 6] and new == [0, 2, 2, 4] and idx.dtype == np.int64


def test_reference_key_orders_like_the_lexsort():
    rng = np.random.RandomState(3)
    s = np.concatenate([rng.normal(0, 2, 300), [0.0, -0.0, INF, -INF, NAN, NAN, 5e-324, -5e-324, 1.0, 1.0, -1.0, -1.0],
                        np.nextafter(1.0, 2.0) * np.ones(2), np.float64(2.0 ** -1040) * rng.randint(-5, 6, 40)])
    rng.shuffle(s)
    key = topk_ref.key(s)
    by_key = np.lexsort((np.arange(s.size), np.iinfo(np.uint64).max - key))           # larger key first, then the lower index
    assert np.array_equal(by_key, topk_ref.order(s))
    assert key[np.isnan(s)].max() == 0 and key[~np.isnan(s)].min() > 0
    assert topk_ref.key([0.0])[0] == topk_ref.key([-0.0])[0] == 1 << 63


@pytest.mark.parametrize("n", [63, 65, 257, 1025])
def test_cut_commutes_with_the_hard_nms(n):
    """idx[nms(b[idx], s[idx])] == the entries of nms(b, s) whose rank is below k, and those are a prefix of nms(b, s)."""
    boxes, scores = vote_ref.clustered_boxes(n, seed=n)
    full = oracle_nms(boxes, scores, 0.3)
    rank = np.empty(n, np.int64)
    rank[topk_ref.order(scores)] = np.arange(n)
    assert (np.diff(rank[full]) > 0).all()                                 # the keep list is in rank order
    for k in sorted({1, 2, 64, n // 3, n - 1, n, n + 1}):
        idx = topk_ref.topk_select(scores, k)
        assert idx.size == min(n, k) and (np.diff(idx) > 0).all()
        got = idx[oracle_nms(boxes[idx], scores[idx], 0.3)]
        want = full[rank[full] < k]
        assert np.array_equal(got, want), (n, k)
        assert np.array_equal(want, full[:want.size])


# --------------------------------------------------------------------------- the surface
def test_symbols_and_version(hip):
    new = {"tf_topk_workspace_bytes", "tf_topk_select_f64", "tf_topk_batched_workspace_bytes", "tf_topk_select_f64_batched",
           "tf_soft_nms_f64_capped", "tf_soft_nms_f64_batched_capped"}
    assert new <= set(hip._SIGNATURES) and new <= set(hip.symbols())
    assert hip.lib().tf_version() >= 720


def test_keywords_exist_with_their_defaults():
    import evaluate_model
    from tinyfaces import evaluation, ops
    for fn in (evaluation.get_detections, evaluation.get_detections_batch, evaluate_model.run):
        p = inspect.signature(fn).parameters
        names = list(p)
        assert names[names.index("flip") - 2: names.index("flip")] == ["pre_nms_topk", "max_detections"], fn.__name__   # in front of the TTA keywords
        assert p["pre_nms_topk"].default is None and p["max_detections"].default is None
        assert p["pre_nms_topk"].kind is p["flip"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    # the cap is a form of its own: max_keep right behind the operands, the rest as in the uncapped functions, whose signatures stay
    plain, capped = list(inspect.signature(ops.soft_nms).parameters), list(inspect.signature(ops.soft_nms_capped).parameters)
    assert capped == plain[:2] + ["max_keep"] + plain[2:] and "max_keep" not in plain
    plain, capped = list(inspect.signature(ops.soft_nms_batched).parameters), list(inspect.signature(ops.soft_nms_batched_capped).parameters)
    assert capped == plain[:3] + ["max_keep"] + plain[3:] and "max_keep" not in plain
    assert inspect.signature(ops.soft_nms_capped).parameters["max_keep"].default is inspect.Parameter.empty
    assert list(inspect.signature(ops.topk_select).parameters) == ["scores", "k"]
    assert list(inspect.signature(ops.topk_select_batched).parameters) == ["scores", "seg_offsets", "k"]


def test_evaluate_model_flags():
    import evaluate_model
    a = evaluate_model.limits_arguments(["DATA"])
    assert a.pre_nms_topk is None and a.max_detections is None and a.soft_nms is None and a.flip is False and a.ema is False
    a = evaluate_model.limits_arguments(["DATA", "--pre-nms-topk", "5000", "--max-detections", "750", "--soft-nms", "linear", "--flip",
                                         "--box-voting", "0.5", "--ema", "--num-images", "1"])
    assert (a.pre_nms_topk, a.max_detections) == (5000, 750) and a.soft_nms == "linear" and a.flip and a.box_voting == 0.5 and a.ema
    assert a.num_images == 1 and a.dataset == "DATA"
    a = evaluate_model.limits_arguments(["--max-detections=1", "DATA"])
    assert a.max_detections == 1 and a.pre_nms_topk is None
    for bad in (["--pre-nms-topk", "0"], ["--pre-nms-topk", "-3"], ["--pre-nms-topk", "2.5"], ["--pre-nms-topk", "abc"], ["--pre-nms-topk"],
                ["--max-detections", "0"], ["--max-detections", "-1"], ["--max-detections", "1e3"], ["--max-detections", "nan"]):
        with pytest.raises(SystemExit):
            evaluate_model.limits_arguments(["DATA"] + bad)
    # the older parsers keep their results and keep refusing the new flags
    for parse in (evaluate_model.arguments, evaluate_model.ema_arguments, evaluate_model.tta_arguments, evaluate_model.soft_nms_arguments):
        assert not [k for k in vars(parse(["DATA"])) if k in ("pre_nms_topk", "max_detections")]
        for argv in (["--pre-nms-topk", "5"], ["--max-detections", "5"]):
            with pytest.raises(SystemExit):
                parse(["DATA"] + argv)
    s = evaluate_model.soft_nms_arguments(["DATA", "--soft-nms", "gaussian", "--flip"])
    assert s.soft_nms == "gaussian" and s.flip is True


def test_host_refusals_fire_without_a_device():
    from tinyfaces import evaluation, ops
    s = torch.zeros(5, dtype=torch.float64)
    for k in (0, -1, 2.5, None, True):
        with pytest.raises(ValueError):
            ops.topk_select(s, k)
        with pytest.raises(ValueError):
            ops.topk_select_batched(s, [0, 5], k)
    for offs in ([0], [1, 5], [0, 3, 2, 5], [0, 4], list(range(0, 66)) + [5]):
        with pytest.raises(ValueError):
            ops.topk_select_batched(s, offs, 2)
    with pytest.raises(ValueError):
        ops.topk_select(torch.zeros(5, 2, dtype=torch.float64), 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # good arguments: the only thing missing is the device
        ops.topk_select(s, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.topk_select_batched(s, [0, 2, 5], 9)
    boxes = torch.zeros(5, 4, dtype=torch.float64)
    for mk in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError):
            ops.soft_nms_capped(boxes, s, mk)
        with pytest.raises(ValueError):
            ops.soft_nms_batched_capped(boxes, s, [0, 5], mk)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.soft_nms_capped(boxes, s, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.soft_nms_batched_capped(boxes, s, [0, 5], 3, "gaussian")
    for kw in (dict(pre_nms_topk=0), dict(pre_nms_topk=-5), dict(pre_nms_topk=1.5), dict(max_detections=0), dict(max_detections="3")):
        with pytest.raises(ValueError):
            evaluation.get_detections(None, None, None, None, None, device="cuda", **kw)
        with pytest.raises(ValueError):
            evaluation.get_detections_batch(None, [None], None, None, None, device="cuda", **kw)


def test_entry_points_check_their_arguments_without_launching(hip):
    l = hip.lib()
    ERR_ARG = -1
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    off = (C.c_int32 * 3)(0, 2, 8)

    def call(scores=p, offs=off, S=2, k=4, idx=p, ws=p, wsb=1 << 20):
        return l.tf_topk_select_f64_batched(scores, offs, S, k, idx, ws, wsb, None)

    assert call(k=0) == ERR_ARG and call(k=-1) == ERR_ARG
    assert call(S=0) == ERR_ARG and call(S=65) == ERR_ARG and call(offs=None) == ERR_ARG
    assert call(offs=(C.c_int32 * 3)(0, 8, 2)) == ERR_ARG and call(offs=(C.c_int32 * 3)(1, 2, 8)) == ERR_ARG
    assert call(scores=None) == ERR_ARG and call(idx=None) == ERR_ARG
    assert call(ws=None) == ERR_ARG and call(wsb=8) == ERR_ARG                # a short workspace is an argument error here
    assert call(scores=None, offs=(C.c_int32 * 3)(0, 0, 0), idx=None, ws=None, wsb=0) == 0     # n == 0: nothing is launched
    assert l.tf_topk_select_f64(p, -1, 4, p, p, 1 << 20, None) == ERR_ARG
    assert l.tf_topk_select_f64(p, 8, 0, p, p, 1 << 20, None) == ERR_ARG
    assert l.tf_topk_select_f64(None, 0, 4, None, None, 0, None) == 0
    # workspace: zero for nothing, monotone in n, and the bytes a call checks against
    assert l.tf_topk_workspace_bytes(0, 4) == 0 and l.tf_topk_workspace_bytes(-2, 4) == 0 and l.tf_topk_workspace_bytes(9, 0) == 0
    sizes = [l.tf_topk_workspace_bytes(n, 5000) for n in (1, 5000, 5001, 65536, 600000, 2 ** 21 + 5, 2 ** 31 - 1)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] < (64 << 20)
    assert l.tf_topk_batched_workspace_bytes((C.c_int32 * 3)(0, 0, 0), 2, 4) == 0
    # the capped Soft-NMS entries: max_keep < 0 is refused; every refusal of the uncapped entry stands
    soff = (C.c_int32 * 3)(0, 2, 4)
    capped = lambda mk, method=1: l.tf_soft_nms_f64_batched_capped(p, p, soff, 2, method, 0.3, 0.5, 0.001, 0, mk, p, p, p, p, 1 << 20, None)  # noqa: E731
    assert capped(-1) == ERR_ARG and capped(-(2 ** 31)) == ERR_ARG and capped(5, method=7) == ERR_ARG
    assert l.tf_soft_nms_f64_capped(p, p, 4, 1, 0.3, 0.5, 0.001, 0, -1, p, p, p, p, 1 << 20, None) == ERR_ARG
    assert l.tf_soft_nms_f64_capped(p, p, -1, 1, 0.3, 0.5, 0.001, 0, 3, p, p, p, p, 1 << 20, None) == ERR_ARG
    assert l.tf_soft_nms_f64_capped(None, None, 0, 1, 0.3, 0.5, 0.0, 0, 3, None, None, p, None, 0, None) == 0
