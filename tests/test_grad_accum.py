"""CPU: gradient accumulation -- everything that can be checked without a GPU.  main.py's two flags parsed apart from the reference's
options, the new C entry point and its host-side argument checks, the window bookkeeping of TrainEngine (which micro-batch applies, the k
of the average), and the refusals.  tests/test_gpu_grad_accum.py holds the numbers."""
import ctypes as C
import inspect

import pytest
import torch

ERR_ARG = -1


def test_main_parses_the_two_flags_apart_from_the_reference_options(golden):
    import json
    import main
    pos = ["train.txt", "val.txt"]
    a = main.trunk_arguments(pos)
    assert a.accum_steps == 1 and a.accum_average is False                       # off by default
    a = main.trunk_arguments(pos + ["--accum-steps", "8", "--lr", "0.01"])
    assert a.accum_steps == 8 and a.accum_average is False and a.lr == 0.01 and a.fused is True
    a = main.trunk_arguments(["--accum-steps=4", "--accum-average", "--no-fused"] + pos + ["--clip-grad-norm", "2", "--model-ema", "0.9"])
    assert a.accum_steps == 4 and a.accum_average is True and a.fused is False and a.clip_grad_norm == 2.0 and a.model_ema == 0.9
    assert a.traindata == "train.txt" and a.valdata == "val.txt"
    for bad in ("0", "-2", "1.5", "abc"):
        with pytest.raises(SystemExit):
            main.trunk_arguments(pos + ["--accum-steps", bad])
    # `arguments` resolves what it resolved before: the reference's flags with the reference's defaults, and neither new flag
    got = vars(main.arguments(["TRAIN", "VAL"]))
    assert "accum_steps" not in got and "accum_average" not in got
    for k, v in json.loads(str(golden("cli")["main"])).items():
        assert got[k] == (v if k != "resume" else ""), k
    for extra in (["--accum-steps", "2"], ["--accum-average"]):
        with pytest.raises(SystemExit):
            main.arguments(pos + extra)


def test_the_entry_point_is_exported_and_checks_its_arguments(hip):
    l = hip.lib()
    assert l.tf_version() >= 670
    assert "tf_grad_accumulate_segments" in hip._SIGNATURES and "tf_grad_accumulate_segments" in hip.symbols()
    assert (hip.TF_ACCUM_STORE, hip.TF_ACCUM_ADD, hip.TF_ACCUM_FINISH) == (0, 1, 2)
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    good = (C.c_int64 * 4)(0, 8, 8, 12)
    overlap = (C.c_int64 * 4)(0, 8, 4, 12)
    backwards = (C.c_int64 * 4)(0, 8, 20, 16)
    # (no GPU here: a launch would not come back as TF_ERR_ARG, and `nseg == 0` must not launch at all)
    for mode in (0, 1, 2):
        assert l.tf_grad_accumulate_segments(None, p, good, 2, mode, None) == ERR_ARG
        assert l.tf_grad_accumulate_segments(p, None, good, 2, mode, None) == ERR_ARG
        assert l.tf_grad_accumulate_segments(p, p, None, 2, mode, None) == ERR_ARG
        assert l.tf_grad_accumulate_segments(p, p, overlap, 2, mode, None) == ERR_ARG
        assert l.tf_grad_accumulate_segments(p, p, backwards, 2, mode, None) == ERR_ARG
        assert l.tf_grad_accumulate_segments(p, p, good, -1, mode, None) == ERR_ARG
        assert l.tf_grad_accumulate_segments(p, p, good, 0, mode, None) == 0
        assert l.tf_grad_accumulate_segments(None, None, None, 0, mode, None) == 0
    for mode in (-1, 3, 7):
        assert l.tf_grad_accumulate_segments(p, p, good, 2, mode, None) == ERR_ARG
        assert l.tf_grad_accumulate_segments(p, p, good, 0, mode, None) == ERR_ARG     # an unknown mode is refused before anything else
    assert not any(buf)


def test_ops_wrapper_refuses_the_cpu_a_bad_mode_and_a_bad_table():
    from tinyfaces import ops
    assert (ops.ACCUM_STORE, ops.ACCUM_ADD, ops.ACCUM_FINISH) == (0, 1, 2)
    assert list(inspect.signature(ops.grad_accumulate).parameters) == ["acc", "grad", "segments", "mode"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grad_accumulate(torch.zeros(8), torch.ones(8), [(0, 8)], ops.ACCUM_STORE)


def _cpu_engine(**kw):
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as zoo
    from tinyfaces.models.loss import DetectionCriterion
    return TrainEngine(zoo.DetectionModel(base_model=zoo.resnet50, num_templates=25), DetectionCriterion(25), device="cpu", **kw)


def test_defaults_and_signatures():
    from tinyfaces import trainer
    from tinyfaces.engine import TrainEngine
    ps = inspect.signature(TrainEngine.__init__).parameters
    assert ps["accum_steps"].default == 1 and ps["accum_average"].default is False
    assert list(inspect.signature(TrainEngine.step).parameters) == ["self", "x", "class_map", "regression_map", "apply"]
    assert inspect.signature(TrainEngine.step).parameters["apply"].default is None
    ts = inspect.signature(trainer.train).parameters
    assert ts["accum_steps"].default == 1 and ts["accum_average"].default is False
    eng = _cpu_engine()
    assert (eng.accum_steps, eng.accum_average, eng.steps, eng.micro_steps, eng.pending_micro_batches) == (1, False, 0, 0, 0)
    assert eng._accum is None                                                    # no buffer unless the feature is used
    for bad in (0, -1):
        with pytest.raises(ValueError, match="accum_steps"):
            _cpu_engine(accum_steps=bad)
        with pytest.raises(ValueError, match="accum_steps"):
            trainer.train(torch.nn.Identity(), None, torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1), [], 0, "cpu",
                          accum_steps=bad)


def test_window_bookkeeping_which_micro_batch_applies():
    """_applies(apply) for the micro-batch about to run, with `_window` micro-batches already accumulated: None applies when this one fills
    the window, True always, False never -- and False is refused for the micro-batch that would fill it."""
    eng = _cpu_engine(accum_steps=3)
    want = {0: (False, True, False), 1: (False, True, False), 2: (True, True, ValueError)}
    for pending, (on_none, on_true, on_false) in want.items():
        eng._window = pending
        assert eng.pending_micro_batches == pending
        assert eng._applies(None) is on_none and eng._applies(True) is on_true
        if on_false is ValueError:
            with pytest.raises(ValueError, match="fills the window"):
                eng._applies(False)
        else:
            assert eng._applies(False) is on_false
    one = _cpu_engine()
    assert one._applies(None) is True and one._applies(True) is True
    with pytest.raises(ValueError, match="fills the window"):
        one._applies(False)
    with pytest.raises(ValueError, match="fills the window"):                    # ... refused by step() itself before any work is enqueued
        one.step(None, None, None, apply=False)
    assert one.micro_steps == 0


def test_an_open_window_refuses_a_checkpoint():
    eng = _cpu_engine(accum_steps=2)
    assert eng.optimizer_state_dict()["state"] == {}
    eng._window = 1
    with pytest.raises(RuntimeError, match="1 of 2 micro-batches"):
        eng.optimizer_state_dict()
    eng._window = 0
    assert len(eng.optimizer_state_dict()["param_groups"]) == 4


def test_per_bucket_updates_cannot_accumulate(monkeypatch):
    monkeypatch.setenv("TINYFACES_SGD_PER_BUCKET", "1")
    with pytest.raises(ValueError, match="TINYFACES_SGD_PER_BUCKET"):
        _cpu_engine(accum_steps=2)


class _Scripted:
    """A stand-in for the device side of TrainEngine.step: records what a window launches, computes nothing."""

    def __init__(self, eng, monkeypatch):
        from tinyfaces import ops
        self.log = []
        m = eng.model
        monkeypatch.setattr(m, "_check_partial_freeze", lambda: None)
        monkeypatch.setattr(m, "_sync_tables", lambda dev: None)
        monkeypatch.setattr(m, "_run_forward", lambda x, training=True: None)
        monkeypatch.setattr(m, "_run_backward", lambda x, g, persistent=False: torch.zeros(eng.flat_p.numel()))
        monkeypatch.setattr(ops, "criterion_fwd_bwd", lambda *a, **kw: (torch.zeros(2, dtype=torch.float64), None, None))
        monkeypatch.setattr(ops, "grad_accumulate", lambda acc, g, segs, mode: self.log.append(("accumulate", mode)))
        monkeypatch.setattr(ops, "sgd_step", lambda *a, **kw: self.log.append(("sgd", a[6])))


def test_a_window_launches_store_add_finish_and_scales_by_the_micro_batches_it_holds(monkeypatch):
    """The whole of step() on the host, its device calls replaced by recorders: micro-batches 1 .. N - 1 launch STORE / ADD and no update, the
    last one FINISH and the three group updates; `steps`, `micro_steps` and `pending_micro_batches` move as documented; accum_average passes
    grad_scale = 1 / k with k the micro-batches actually accumulated; a window of one micro-batch launches no accumulate at all."""
    from tinyfaces import ops
    eng = _cpu_engine(accum_steps=3, accum_average=True)
    rec = _Scripted(eng, monkeypatch)
    x = torch.zeros(1, 3, 8, 8)
    eng.step(x, None, None)
    eng.step(x, None, None)
    assert rec.log == [("accumulate", ops.ACCUM_STORE), ("accumulate", ops.ACCUM_ADD)]
    assert (eng.steps, eng.micro_steps, eng.pending_micro_batches) == (0, 2, 2) and eng._accum is not None
    eng.step(x, None, None)
    assert rec.log[2:] == [("accumulate", ops.ACCUM_FINISH)] + [("sgd", 1.0 / 3)] * 3
    assert (eng.steps, eng.micro_steps, eng.pending_micro_batches) == (1, 3, 0)
    del rec.log[:]
    eng.step(x, None, None, apply=False)
    eng.step(x, None, None, apply=True)                                          # the end of an epoch: k = 2 of 3
    assert rec.log == [("accumulate", ops.ACCUM_STORE), ("accumulate", ops.ACCUM_FINISH)] + [("sgd", 0.5)] * 3
    assert (eng.steps, eng.micro_steps, eng.pending_micro_batches) == (2, 5, 0)
    del rec.log[:]
    eng.step(x, None, None, apply=True)                                          # k = 1: the plain step
    assert rec.log == [("sgd", 1.0)] * 3 and (eng.steps, eng.micro_steps) == (3, 6)
    # the sum (the default): grad_scale stays 1 whatever the window holds
    eng.accum_average = False
    del rec.log[:]
    for _ in range(3):
        eng.step(x, None, None)
    assert [c for c in rec.log if c[0] == "sgd"] == [("sgd", 1.0)] * 3 and eng.steps == 4


def test_the_default_engine_never_reaches_the_accumulator(monkeypatch):
    eng = _cpu_engine()
    rec = _Scripted(eng, monkeypatch)
    x = torch.zeros(1, 3, 8, 8)
    for apply in (None, True, None):
        eng.step(x, None, None, apply=apply)
    assert rec.log == [("sgd", 1.0)] * 9 and eng._accum is None
    assert (eng.steps, eng.micro_steps, eng.pending_micro_batches) == (3, 3, 0)
