"""CPU: partial freezing of the trunk (DetectionModel.set_trainable_layers, tf_detnet_trunk_backward_frozen_from_ctx) as far as it can be checked
without a GPU -- the mode, the list of trained tensors, the command line and the host-side argument checks of the new entry point."""
import ctypes as C
import importlib.util
import os
import pickle

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tiny-faces-pytorch_amd")

# tensors that receive a gradient with BatchNorm frozen, for k = 4, 3, 2, 1, 0: the conv weights of the trained stages + 2 head weights + 2 head biases
COUNTS = {"resnet50": (47, 46, 36, 23, 4), "resnet101": (98, 97, 87, 74, 4), "resnet152": (149, 148, 138, 113, 4)}
STAGES = ("model.layer3.", "model.layer2.", "model.layer1.", "model.conv1.")       # from the top


def _main():
    spec = importlib.util.spec_from_file_location("our_cli_main_trainable", os.path.join(PKG, "main.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_trainable_layers_is_a_mode_outside_the_state_dict(hip):
    from tinyfaces.models.model import DetectionModel
    m = DetectionModel(num_templates=25)
    keys = list(m.state_dict())
    assert len(keys) == 571
    assert m.trainable_layers == 4                                          # the default trains everything
    assert m.set_trainable_layers(2) is m and m.trainable_layers == 2
    for bad in (-1, 5, 2.0, True, "2", None):
        with pytest.raises(ValueError):
            m.set_trainable_layers(bad)
    assert m.trainable_layers == 2                                          # a refused value changes nothing
    with pytest.raises(AttributeError):
        m.trainable_layers = 3                                              # read-only
    assert m.train().trainable_layers == 2 and m.eval().trainable_layers == 2 and m.train(True).trainable_layers == 2
    assert m.float().trainable_layers == 2 and m.to("cpu").trainable_layers == 2
    assert pickle.loads(pickle.dumps(m)).trainable_layers == 2
    assert list(m.state_dict()) == keys                                     # still the 571-key contract
    fresh = DetectionModel(num_templates=25)
    fresh.load_state_dict(m.state_dict())
    assert fresh.trainable_layers == 4                                      # a mode, not a value: it does not travel with the weights
    for k in range(5):
        assert m.set_trainable_layers(k).trainable_layers == k
    # requires_grad flags are not touched, learnable_parameters() stays the reference's four groups
    m.set_trainable_layers(0).freeze_batchnorm()
    assert all(p.requires_grad for p in m.parameters())
    groups = m.learnable_parameters(1e-3)
    assert len(groups) == 4 and [g["lr"] for g in groups] == [1e-3, 1e-4, 1e-3, 0]
    assert len(list(groups[0]["params"])) == len(list(m.model.parameters()))


@pytest.mark.parametrize("trunk", ["resnet50", "resnet101", "resnet152"])
def test_trainable_parameter_names_follow_the_two_modes(hip, trunk):
    from tinyfaces.models import model as mm
    m = mm.DetectionModel(base_model=getattr(mm, trunk), num_templates=25)
    params = dict(m.named_parameters())
    bn = {f"{n}.{w}" for n, mod in m.named_modules() if isinstance(mod, mm.nn.BatchNorm2d) for w in ("weight", "bias")}
    l, tr = hip.lib(), (C.c_int * 3)(*m.trunk)
    order = [l.tf_detnet_trunk_param_name(tr, i).decode() for i in range(l.tf_detnet_trunk_num_params(tr))]
    full = m.trainable_parameter_names()                                    # batch statistics, k = 4: today's list
    n_conv = COUNTS[trunk][0] - 4
    assert len(full) == 3 * n_conv + 4 == {"resnet50": 133, "resnet101": 286, "resnet152": 439}[trunk]
    assert full == [n for n in order if n in params and n != "score4_upsample.weight"]
    m.freeze_batchnorm()
    heads = ["score_res3.weight", "score_res3.bias", "score_res4.weight", "score_res4.bias"]
    for k, want in zip((4, 3, 2, 1, 0), COUNTS[trunk]):
        names = m.set_trainable_layers(k).trainable_parameter_names()
        assert len(names) == want == len(set(names)), (trunk, k, len(names))
        assert names == [n for n in order if n in names]                    # executor order
        assert not [n for n in names if n in bn or n not in params]         # no BN vector, parameters only
        assert not [n for n in names if n.startswith(STAGES[k:])]           # nothing of a frozen stage
        assert all(n.endswith(".weight") for n in names if n.startswith("model."))
        assert names[-4:] == heads and "score4_upsample.weight" not in names
        for s in STAGES[:k]:
            assert any(n.startswith(s) for n in names), (k, s)
    assert m.set_trainable_layers(0).trainable_parameter_names() == heads
    # ... and the list follows freeze_batchnorm() whatever the order of the two setters
    assert m.freeze_batchnorm(False).set_trainable_layers(4).trainable_parameter_names() == full
    assert len(m.set_trainable_layers(2).freeze_batchnorm().trainable_parameter_names()) == COUNTS[trunk][2]


def test_trainable_layers_flag_is_parsed_beside_freeze_bn(capsys):
    main = _main()
    args = main.trunk_arguments(["TRAIN", "VAL", "--trainable-layers", "2", "--freeze-bn"])
    assert args.trainable_layers == 2 and args.freeze_bn is True and args.base_model == "resnet101" and args.traindata == "TRAIN"
    args = main.trunk_arguments(["TRAIN", "VAL", "--freeze-bn", "--base-model", "resnet50", "--trainable-layers", "0", "--lr", "0.01"])
    assert args.trainable_layers == 0 and args.base_model == "resnet50" and args.lr == 0.01
    with pytest.raises(SystemExit):
        main.trunk_arguments(["TRAIN", "VAL", "--trainable-layers", "2"])           # frozen stages sit on frozen BatchNorm
    assert "--freeze-bn" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        main.trunk_arguments(["TRAIN", "VAL", "--trainable-layers", "5", "--freeze-bn"])
    args = main.trunk_arguments(["TRAIN", "VAL", "--trainable-layers", "4"])        # everything trained: any BatchNorm mode
    assert args.trainable_layers == 4 and args.freeze_bn is False
    assert main.trunk_arguments(["TRAIN", "VAL"]).trainable_layers == 4
    # `arguments` resolves the reference's names (and the older additions) only
    assert "trainable_layers" not in vars(main.arguments(["TRAIN", "VAL"]))
    with pytest.raises(SystemExit):
        main.arguments(["TRAIN", "VAL", "--trainable-layers", "2"])


def test_cut_entry_point_refuses_bad_arguments_without_launching(hip):
    """The call shape of test_frozen_entry_points_refuse_bad_arguments_without_launching: a NULL operand, fp16, an unknown trunk or a cut that is
    not a stage boundary comes back from the host as TF_ERR_ARG / TF_ERR_UNSUPPORTED, nothing is enqueued (there is no device here)."""
    l = hip.lib()
    ERR_ARG, ERR_UNSUPPORTED = -1, -3
    assert l.tf_version() >= 630 and "tf_detnet_trunk_backward_frozen_from_ctx" in hip.symbols()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    tab = (C.c_void_p * 1000)()
    trunks = {(3, 4, 6): (-1, 0, 3, 7, 13), (3, 4, 23): (-1, 0, 3, 7, 30), (3, 8, 36): (-1, 0, 3, 11, 47)}
    odd = (C.c_int * 3)(3, 4, 7)
    ok = dict(x=p, params=tab, grads=tab, gout=p, ws=p)

    def call(blocks, dtype, first_block, **kw):
        a = dict(ok, **kw)
        return l.tf_detnet_trunk_backward_frozen_from_ctx(blocks, None, None, dtype, a["x"], 1, 64, 64, 125, a["params"], a["grads"], a["gout"], None, 0,
                                                          a["ws"], 1 << 20, None, first_block)

    for counts, cuts in trunks.items():
        arr = (C.c_int * 3)(*counts)
        nblocks = sum(counts)
        for first_block in cuts:
            for name in ok:
                assert call(arr, hip.TF_BF16, first_block, **{name: None}) == ERR_ARG, (counts, first_block, name)
            assert call(arr, hip.TF_F16, first_block) == ERR_UNSUPPORTED                     # fp16: inference only
            assert call(odd, hip.TF_BF16, first_block) == ERR_UNSUPPORTED                    # a trunk the executor does not take
        # everything that is not a stage boundary: below -1, inside layer 1 / 2 / 3, beyond the heads-only cut
        for first_block in (-2, 1, 2, cuts[2] + 1, cuts[3] + 1, cuts[3] + 2, nblocks - 1, nblocks + 1, 1 << 20):
            assert first_block not in cuts
            assert call(arr, hip.TF_BF16, first_block) == ERR_ARG, (counts, first_block)
            assert call(arr, hip.TF_F32, first_block) == ERR_ARG, (counts, first_block)
    assert call(None, hip.TF_BF16, 30, x=None) == ERR_ARG and call(None, hip.TF_BF16, 13) == ERR_ARG     # NULL = ResNet-101: 13 is mid-stage
    hooks = hip.DetnetHooks()
    hooks.n = 2                                                                              # two hooks, no block table
    r50 = (C.c_int * 3)(3, 4, 6)
    assert l.tf_detnet_trunk_backward_frozen_from_ctx(r50, None, C.byref(hooks), hip.TF_BF16, p, 1, 64, 64, 125, tab, tab, p, None, 0, p, 1 << 20, None,
                                                      3) == ERR_ARG
