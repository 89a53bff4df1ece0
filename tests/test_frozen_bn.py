"""CPU: the frozen-BatchNorm mode (DetectionModel.freeze_batchnorm, executor mode 2) as far as it can be checked without a GPU -- the
Python surface, the workspace plan, the command line and the host-side argument checks of the new entry points."""
import ctypes as C
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tiny-faces-pytorch_amd")


def _main():
    spec = importlib.util.spec_from_file_location("our_cli_main_frozen", os.path.join(PKG, "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_freeze_batchnorm_is_a_mode_outside_the_state_dict(hip):
    from tinyfaces.models.model import DetectionModel
    m = DetectionModel(num_templates=25)
    keys = list(m.state_dict())
    assert len(keys) == 571
    assert m.batchnorm_frozen is False
    assert m.freeze_batchnorm() is m and m.batchnorm_frozen is True
    assert m.train().batchnorm_frozen and m.eval().batchnorm_frozen and m.train(True).batchnorm_frozen      # survives train() / eval()
    assert m.float().batchnorm_frozen and m.to("cpu").batchnorm_frozen                                       # ... and _apply
    assert list(m.state_dict()) == keys                                                                      # still the 571-key contract
    fresh = DetectionModel(num_templates=25)
    fresh.load_state_dict(m.state_dict())
    assert fresh.batchnorm_frozen is False                     # a mode, not a value: it does not travel with the weights
    assert m.freeze_batchnorm(False) is m and m.batchnorm_frozen is False
    with pytest.raises(AttributeError):
        m.batchnorm_frozen = True                              # read-only


def test_frozen_workspace_sits_between_eval_and_training(hip):
    """The frozen plan is the evaluation plan plus what the training plan also has (max-pool arg-max, transposed operands, per-block gradient
    buffers, head gradients), minus a1 / a2 / c3, the statistic regions and the downsample branch's BN-backward operand."""
    l = hip.lib()
    assert hip.TF_DETNET_FROZEN_BN == 2
    for dtype in (hip.TF_BF16, hip.TF_F32):
        ev, fz, tr = (l.tf_detnet_workspace_bytes(dtype, 12, 500, 500, 125, t) for t in (0, 2, 1))
        assert 0 < ev <= fz < tr, (dtype, ev, fz, tr)
    for blocks in ((3, 4, 6), (3, 4, 23), (3, 8, 36)):
        arr = (C.c_int * 3)(*blocks)
        ev, fz, tr = (l.tf_detnet_trunk_workspace_bytes(arr, hip.TF_BF16, 2, 203, 187, 125, t) for t in (0, 2, 1))
        assert 0 < ev <= fz < tr, (blocks, ev, fz, tr)
        pe, pf, pt = (l.tf_detnet_trunk_param_region_bytes(arr, hip.TF_BF16, 125, t) for t in (0, 2, 1))
        assert pe < pf and pe < pt                             # both training modes also hold the transposed operands
    # the evaluation layout is untouched: its parameter region does not depend on the new mode existing
    assert l.tf_detnet_param_region_bytes(hip.TF_BF16, 125, 0) == l.tf_detnet_trunk_param_region_bytes(None, hip.TF_BF16, 125, 0)


def test_freeze_bn_flag_is_parsed_beside_base_model():
    main = _main()
    args = main.trunk_arguments(["TRAIN", "VAL", "--freeze-bn"])
    assert args.freeze_bn is True and args.base_model == "resnet101" and args.traindata == "TRAIN"
    args = main.trunk_arguments(["TRAIN", "VAL", "--base-model", "resnet50", "--freeze-bn", "--lr", "0.01"])
    assert args.freeze_bn is True and args.base_model == "resnet50" and args.lr == 0.01
    assert main.trunk_arguments(["TRAIN", "VAL"]).freeze_bn is False
    # `arguments` resolves today's names only: the new flag is not one of them
    plain = vars(main.arguments(["TRAIN", "VAL"]))
    assert "freeze_bn" not in plain and "base_model" not in plain
    with pytest.raises(SystemExit):
        main.arguments(["TRAIN", "VAL", "--freeze-bn"])


def test_frozen_entry_points_refuse_bad_arguments_without_launching(hip):
    """Like the round-4 entry points: a NULL operand or fp16 comes back as TF_ERR_ARG / TF_ERR_UNSUPPORTED from the host, nothing is enqueued."""
    l = hip.lib()
    ERR_ARG, ERR_UNSUPPORTED = -1, -3
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    tab = (C.c_void_p * 1000)()
    r50 = (C.c_int * 3)(3, 4, 6)
    odd = (C.c_int * 3)(3, 4, 7)
    ok = dict(x=p, params=tab, grads=tab, gout=p, ws=p)

    def trunk(blocks, dtype, **kw):
        a = dict(ok, **kw)
        return l.tf_detnet_trunk_backward_frozen_ctx(blocks, None, None, dtype, a["x"], 1, 64, 64, 125, a["params"], a["grads"], a["gout"], None, 0,
                                                     a["ws"], 1 << 20, None)

    def default(dtype, **kw):
        a = dict(ok, **kw)
        return l.tf_detnet_backward_frozen_ctx(None, None, dtype, a["x"], 1, 64, 64, 125, a["params"], a["grads"], a["gout"], None, 0, a["ws"], 1 << 20, None)

    for name in ok:
        assert trunk(r50, hip.TF_BF16, **{name: None}) == ERR_ARG, name
        assert default(hip.TF_BF16, **{name: None}) == ERR_ARG, name
    assert trunk(r50, hip.TF_F16) == ERR_UNSUPPORTED and default(hip.TF_F16) == ERR_UNSUPPORTED       # fp16: inference only
    assert trunk(odd, hip.TF_BF16) == ERR_UNSUPPORTED                                                 # a trunk the executor does not take
    hooks = hip.DetnetHooks()
    hooks.n = 2                                                                                       # two hooks, no block table
    assert l.tf_detnet_trunk_backward_frozen_ctx(r50, None, C.byref(hooks), hip.TF_BF16, p, 1, 64, 64, 125, tab, tab, p, None, 0, p, 1 << 20, None) == ERR_ARG
    # the frozen forward refuses fp16 like the batch-statistics one
    out = (C.c_float * 64)()
    assert l.tf_detnet_forward_ctx(None, 0, hip.TF_F16, 2, p, 1, 64, 64, 125, tab, 1e-5, 0.1, out, p, 1 << 20, 0, None) == ERR_UNSUPPORTED
    # segment SGD: NULL buffers / table, ranges out of order
    seg = (C.c_int64 * 4)(0, 8, 4, 12)
    assert l.tf_sgd_step_segments(None, p, p, seg, 2, 0.1, 0.9, 0.0, 1.0, None) == ERR_ARG
    assert l.tf_sgd_step_segments(p, p, p, None, 2, 0.1, 0.9, 0.0, 1.0, None) == ERR_ARG
    assert l.tf_sgd_step_segments(p, p, p, seg, 2, 0.1, 0.9, 0.0, 1.0, None) == ERR_ARG               # overlapping
    assert l.tf_sgd_step_segments(p, p, p, seg, 0, 0.1, 0.9, 0.0, 1.0, None) == 0                     # nothing to do


def test_struct_mirrors_grew_at_their_end_only(hip):
    """tf_pack2_job / tf_wgrad_args grew by ONE trailing pointer whose zero value means "off": code that fills the older fields positionally
    (the existing tests do, through these ctypes mirrors) keeps its meaning."""
    names = [f[0] for f in hip.Pack2Job._fields_]
    assert names[-1] == "scale_t" and names[:-1] == ["src", "dst", "dst_t", "cout", "cin", "taps", "rows_pad", "cols_pad", "rows_pad_t", "cols_pad_t"]
    assert C.sizeof(hip.Pack2Job) == 64 and hip.Pack2Job().scale_t is None
    names = [f[0] for f in hip.WgradArgs._fields_]
    assert names[-1] == "row_scale" and names[-2] == "partial_ws_bytes" and hip.WgradArgs().row_scale is None
