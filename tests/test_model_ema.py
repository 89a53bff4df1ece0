"""CPU: the model EMA -- everything that can be checked without a GPU.  The decay schedule, the refusal of bad decays, main.py's and
evaluate_model.py's flags parsed apart from the reference's options, the refusal of a CPU model, get_model(ema=True), the three new C entry
points and their host-side argument checks, and a default engine that holds no average.  tests/test_gpu_model_ema.py holds the numbers."""
import ctypes as C
import inspect
import math

import numpy as np
import pytest
import torch

ERR_ARG = -1


def test_decay_schedule_with_and_without_the_warm_up():
    """d_t = min(decay, (1 + t) / (10 + t)) in double; the warm-up off gives the decay itself."""
    from tinyfaces.ema import ema_decay_at
    d = 0.9999
    want = {0: 1.0 / 10.0, 1: 2.0 / 11.0, 8: 9.0 / 18.0, 9: 10.0 / 19.0, 10 ** 6: d}
    for t, v in want.items():
        assert ema_decay_at(d, t) == v, t
        assert ema_decay_at(d, t, warmup=True) == v
        assert ema_decay_at(d, t, warmup=False) == d
    assert (1.0 + 10 ** 6) / (10.0 + 10 ** 6) > d                 # (at t = 10^6 the cap, not the ramp, decides)
    assert ema_decay_at(0.3, 8) == 0.3 and ema_decay_at(0.5, 8) == 0.5 and ema_decay_at(0.6, 8) == 0.5
    assert inspect.signature(ema_decay_at).parameters["warmup"].default is True


@pytest.mark.parametrize("bad", [0, 1, -0.1, float("nan")], ids=["0", "1", "-0.1", "nan"])
def test_bad_decays_are_refused(bad):
    import main
    from tinyfaces.ema import ModelEma, ema_decay_at
    for warmup in (True, False):
        with pytest.raises(ValueError):
            ema_decay_at(bad, 0, warmup=warmup)
    with pytest.raises(ValueError):                                # before anything touches the model (None has no parameters to ask for)
        ModelEma(None, bad)
    with pytest.raises(SystemExit):
        main.trunk_arguments(["train.txt", "val.txt", "--model-ema", repr(bad)])


def test_main_parses_model_ema_apart_from_the_reference_options(golden):
    import json
    import main
    pos = ["train.txt", "val.txt"]
    a = main.trunk_arguments(pos)
    assert a.model_ema is None                                     # off by default
    a = main.trunk_arguments(pos + ["--model-ema", "0.999", "--lr", "0.01"])
    assert a.model_ema == 0.999 and a.lr == 0.01 and a.fused is True
    a = main.trunk_arguments(["--model-ema=0.9", "--no-fused", "--freeze-bn"] + pos + ["--clip-grad-norm", "2"])
    assert a.model_ema == 0.9 and a.fused is False and a.freeze_bn and a.clip_grad_norm == 2.0
    assert a.traindata == "train.txt" and a.valdata == "val.txt"
    # `arguments` resolves what it resolved before: the reference's flags with the reference's defaults, and no --model-ema
    got = vars(main.arguments(["TRAIN", "VAL"]))
    assert "model_ema" not in got
    for k, v in json.loads(str(golden("cli")["main"])).items():
        assert got[k] == (v if k != "resume" else ""), k
    with pytest.raises(SystemExit):
        main.arguments(pos + ["--model-ema", "0.9"])
    with pytest.raises(SystemExit):
        main.trunk_arguments(pos + ["--model-ema", "abc"])
    # evaluate_model.py --ema, parsed apart in the same way
    import evaluate_model
    assert evaluate_model.ema_arguments(["DATA"]).ema is False
    e = evaluate_model.ema_arguments(["DATA", "--ema", "--num-images", "1"])
    assert e.ema is True and e.num_images == 1 and e.dataset == "DATA"
    assert "ema" not in vars(evaluate_model.arguments(["DATA"]))
    with pytest.raises(SystemExit):
        evaluate_model.arguments(["DATA", "--ema"])


def test_model_ema_on_a_cpu_model_raises():
    from tinyfaces.ema import ModelEma
    from tinyfaces.models import model as zoo
    m = zoo.DetectionModel(base_model=zoo.resnet50, num_templates=25)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ModelEma(m, 0.999)
    assert getattr(m, "_flat_params", None) is None                # nothing was flattened on the way
    from tinyfaces import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ema_update_segments(torch.zeros(8), torch.ones(8), [(0, 8)], 0.1)


def test_get_model_loads_the_averaged_weights_or_names_the_missing_key(tmp_path):
    from tinyfaces.evaluation import get_model
    from tinyfaces.models import model as zoo
    sd = zoo.DetectionModel(base_model=zoo.resnet50, num_templates=25).state_dict()
    sd = {k: v.detach().clone() for k, v in sd.items()}
    avg = {k: v.clone() for k, v in sd.items()}
    name = "model.layer2.1.conv2.weight"
    avg[name] = avg[name] + 0.25
    plain, both = str(tmp_path / "plain.pth"), str(tmp_path / "both.pth")
    torch.save({"epoch": 1, "model": sd}, plain)
    torch.save({"epoch": 1, "model": sd, "model_ema": avg, "ema": {"decay": 0.9, "warmup": True, "updates": 3}}, both)
    with pytest.raises(ValueError, match="model_ema"):
        get_model(plain, 25, ema=True)
    with pytest.raises(ValueError, match="model_ema"):
        get_model(None, 25, ema=True)
    live, mean = get_model(both, 25), get_model(both, 25, ema=True)
    assert live.trunk_name == mean.trunk_name == "resnet50"
    a, b = live.state_dict(), mean.state_dict()
    assert list(a) == list(b) == list(sd)
    for k in sd:
        assert torch.equal(a[k], sd[k]), k
        assert torch.equal(b[k], avg[k]), k
    assert not torch.equal(a[name], b[name])
    assert inspect.signature(get_model).parameters["ema"].default is False
    assert torch.equal(get_model(plain, 25).state_dict()[name], sd[name])       # the default path is the one of before
    only_avg = str(tmp_path / "only_avg.pth")
    torch.save({"epoch": 1, "model_ema": avg}, only_avg)
    with pytest.raises(KeyError, match="model"):                                # ... and so is its error for a checkpoint without "model"
        get_model(only_avg, 25)


def test_three_new_entry_points_are_exported_and_check_their_arguments(hip):
    l = hip.lib()
    assert l.tf_version() >= 650
    for name in ("tf_sgd_step_ema", "tf_sgd_step_segments_ema", "tf_ema_update_segments"):
        assert name in hip._SIGNATURES and name in hip.symbols(), name
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    stbuf = hip.ClipState()
    st = C.cast(C.pointer(stbuf), C.c_void_p)
    good = (C.c_int64 * 4)(0, 8, 8, 12)
    overlap = (C.c_int64 * 4)(0, 8, 4, 12)
    backwards = (C.c_int64 * 4)(0, 8, 20, 16)
    # (no GPU here: a launch would not come back as TF_ERR_ARG, and `n == 0` / `nseg == 0` must not launch at all)
    for state in (None, st):
        for k in range(4):
            ops = [p, p, p, p]
            ops[k] = None
            assert l.tf_sgd_step_ema(*ops, 64, 0.1, 0.9, 0.0, 1.0, 0.1, state, None) == ERR_ARG, k
            assert l.tf_sgd_step_segments_ema(*ops, good, 2, 0.1, 0.9, 0.0, 1.0, 0.1, state, None) == ERR_ARG, k
        assert l.tf_sgd_step_ema(p, p, p, p, -1, 0.1, 0.9, 0.0, 1.0, 0.1, state, None) == ERR_ARG
        assert l.tf_sgd_step_ema(p, p, p, p, 0, 0.1, 0.9, 0.0, 1.0, 0.1, state, None) == 0
        assert l.tf_sgd_step_segments_ema(p, p, p, p, None, 2, 0.1, 0.9, 0.0, 1.0, 0.1, state, None) == ERR_ARG
        assert l.tf_sgd_step_segments_ema(p, p, p, p, overlap, 2, 0.1, 0.9, 0.0, 1.0, 0.1, state, None) == ERR_ARG
        assert l.tf_sgd_step_segments_ema(p, p, p, p, backwards, 2, 0.1, 0.9, 0.0, 1.0, 0.1, state, None) == ERR_ARG
        assert l.tf_sgd_step_segments_ema(p, p, p, p, good, -1, 0.1, 0.9, 0.0, 1.0, 0.1, state, None) == ERR_ARG
        assert l.tf_sgd_step_segments_ema(p, p, p, p, good, 0, 0.1, 0.9, 0.0, 1.0, 0.1, state, None) == 0
        assert l.tf_ema_update_segments(None, p, good, 2, 0.1, state, None) == ERR_ARG
        assert l.tf_ema_update_segments(p, None, good, 2, 0.1, state, None) == ERR_ARG
        assert l.tf_ema_update_segments(p, p, None, 2, 0.1, state, None) == ERR_ARG
        assert l.tf_ema_update_segments(p, p, overlap, 2, 0.1, state, None) == ERR_ARG
        assert l.tf_ema_update_segments(p, p, backwards, 2, 0.1, state, None) == ERR_ARG
        assert l.tf_ema_update_segments(p, p, good, -1, 0.1, state, None) == ERR_ARG
        assert l.tf_ema_update_segments(p, p, good, 0, 0.1, state, None) == 0
    assert not any(buf)


def test_ops_keep_their_signatures_and_take_the_average_as_a_pair():
    from tinyfaces import ops, trainer
    for f in (ops.sgd_step, ops.sgd_step_segments):
        ps = inspect.signature(f).parameters
        assert ps["ema"].default is None and ps["ema_weight"].default is None and ps["clip_state"].default is None
        assert all(ps[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("ema", "ema_weight", "clip_state"))
        assert ps["grad_scale"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD
    assert list(inspect.signature(ops.ema_update_segments).parameters) == ["ema", "param", "segments", "weight", "clip_state"]
    assert inspect.signature(trainer.train).parameters["ema"].default is None
    with pytest.raises(ValueError, match="go together"):
        ops._ema_pair("sgd_step", torch.zeros(4), torch.zeros(4), None)
    with pytest.raises(ValueError, match="go together"):
        ops._ema_pair("sgd_step", torch.zeros(4), None, 0.1)
    assert ops._ema_pair("sgd_step", torch.zeros(4), None, None) is None


def test_next_weight_is_one_minus_the_decay_rounded_once_to_fp32():
    """ModelEma.next_weight without a model behind it: float32(1 - d_t) from double arithmetic, `updates` advancing by one per call."""
    from tinyfaces.ema import ModelEma, ema_decay_at
    e = ModelEma.__new__(ModelEma)
    e.decay, e.warmup, e.updates = 0.999, True, 0
    got = [e.next_weight() for _ in range(12)]
    assert e.updates == 12
    for t, w in enumerate(got):
        want = np.float32(1.0 - ema_decay_at(0.999, t))
        assert w == float(want) and np.float32(w) == want and isinstance(w, float), t
    assert got[0] == float(np.float32(0.9)) and math.isclose(got[9], 9.0 / 19.0, rel_tol=1e-7)
    e.warmup, e.updates = False, 0
    assert e.next_weight() == float(np.float32(1.0 - 0.999)) and e.settings() == {"decay": 0.999, "warmup": False, "updates": 1}


def test_default_engine_holds_no_average_and_a_cpu_engine_cannot_have_one():
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as zoo
    from tinyfaces.models.loss import DetectionCriterion
    ps = inspect.signature(TrainEngine.__init__).parameters
    assert ps["ema_decay"].default is None and ps["ema_warmup"].default is True
    m = zoo.DetectionModel(base_model=zoo.resnet50, num_templates=25)
    eng = TrainEngine(m, DetectionCriterion(25), device="cpu")
    assert eng.ema is None and eng._ema_weight is None
    for bad in (0.0, 1.0, float("nan")):
        with pytest.raises(ValueError):
            TrainEngine(m, DetectionCriterion(25), device="cpu", ema_decay=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TrainEngine(m, DetectionCriterion(25), device="cpu", ema_decay=0.999)
