"""CPU: gradient-norm clipping and the non-finite-step guard -- everything that can be checked without a GPU.  The C entry points refuse bad
arguments on the host before any launch, the workspace query is exact, main.py parses the two flags apart from the reference's options, and
the fused engine with its defaults calls exactly what it called before the feature existed.  tests/test_gpu_grad_clip.py holds the numbers."""
import ctypes as C
import inspect

import pytest
import torch

ERR_ARG = -1


def test_abi_version_and_state_mirror(hip):
    l = hip.lib()
    assert l.tf_version() >= 640
    for name in ("tf_grad_norm_workspace_bytes", "tf_grad_clip_coef", "tf_sgd_step_clipped", "tf_sgd_step_segments_clipped", "tf_scale_segments"):
        assert name in hip.symbols() and name in hip._SIGNATURES, name
    # typedef struct tf_clip_state { double sumsq; double norm; float coef; int32_t skip; int64_t skipped; }
    assert C.sizeof(hip.ClipState) == 32
    assert [(f[0], getattr(hip.ClipState, f[0]).offset) for f in hip.ClipState._fields_] == [("sumsq", 0), ("norm", 8), ("coef", 16), ("skip", 20),
                                                                                            ("skipped", 24)]
    assert hip.TF_CLIP_SKIP_NONFINITE == 1


def test_entry_points_refuse_bad_arguments_without_launching(hip):
    """NULL operands, a table that is not ascending and disjoint, a workspace one byte short: TF_ERR_ARG from the host-side checks (no GPU
    here: a launch would not come back as TF_ERR_ARG).  `nseg == 0` with nothing to launch is fine for the SGD forms and the scaling."""
    l = hip.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    wsbuf = (C.c_double * 2048)()
    ws = C.cast(wsbuf, C.c_void_p)
    stbuf = hip.ClipState()
    st = C.cast(C.pointer(stbuf), C.c_void_p)
    good = (C.c_int64 * 4)(0, 8, 8, 12)
    overlap = (C.c_int64 * 4)(0, 8, 4, 12)
    backwards = (C.c_int64 * 4)(0, 8, 20, 16)
    need = l.tf_grad_norm_workspace_bytes(2)
    assert need == 8 * 2048

    def coef(grad=p, table=good, nseg=2, wsp=ws, nbytes=need, state=st):
        return l.tf_grad_clip_coef(grad, table, nseg, 1.0, 1.0, 0, wsp, nbytes, state, None)

    assert coef(grad=None) == ERR_ARG and coef(table=None) == ERR_ARG and coef(wsp=None) == ERR_ARG and coef(state=None) == ERR_ARG
    assert coef(table=overlap) == ERR_ARG and coef(table=backwards) == ERR_ARG
    assert coef(nbytes=need - 1) == ERR_ARG and coef(nbytes=0) == ERR_ARG
    assert coef(nseg=-1) == ERR_ARG
    assert coef(wsp=C.c_void_p(ws.value + 4)) == ERR_ARG                                     # doubles need 8-byte alignment
    assert l.tf_grad_clip_coef(None, None, 0, 1.0, 1.0, 0, None, 0, None, None) == ERR_ARG   # nseg == 0 still needs somewhere to write the state

    assert l.tf_sgd_step_clipped(p, p, p, 64, 0.1, 0.9, 0.0, 1.0, None, None) == ERR_ARG
    assert l.tf_sgd_step_clipped(None, p, p, 64, 0.1, 0.9, 0.0, 1.0, st, None) == ERR_ARG
    assert l.tf_sgd_step_clipped(p, None, p, 64, 0.1, 0.9, 0.0, 1.0, st, None) == ERR_ARG
    assert l.tf_sgd_step_clipped(p, p, None, 64, 0.1, 0.9, 0.0, 1.0, st, None) == ERR_ARG
    assert l.tf_sgd_step_clipped(p, p, p, -1, 0.1, 0.9, 0.0, 1.0, st, None) == ERR_ARG
    assert l.tf_sgd_step_clipped(p, p, p, 0, 0.1, 0.9, 0.0, 1.0, st, None) == 0                # nothing to do

    assert l.tf_sgd_step_segments_clipped(p, p, p, good, 2, 0.1, 0.9, 0.0, 1.0, None, None) == ERR_ARG
    assert l.tf_sgd_step_segments_clipped(None, p, p, good, 2, 0.1, 0.9, 0.0, 1.0, st, None) == ERR_ARG
    assert l.tf_sgd_step_segments_clipped(p, p, p, None, 2, 0.1, 0.9, 0.0, 1.0, st, None) == ERR_ARG
    assert l.tf_sgd_step_segments_clipped(p, p, p, overlap, 2, 0.1, 0.9, 0.0, 1.0, st, None) == ERR_ARG
    assert l.tf_sgd_step_segments_clipped(p, p, p, good, 0, 0.1, 0.9, 0.0, 1.0, st, None) == 0

    assert l.tf_scale_segments(None, good, 2, st, None) == ERR_ARG
    assert l.tf_scale_segments(p, None, 2, st, None) == ERR_ARG
    assert l.tf_scale_segments(p, good, 2, None, None) == ERR_ARG
    assert l.tf_scale_segments(p, overlap, 2, st, None) == ERR_ARG
    assert l.tf_scale_segments(p, good, 0, st, None) == 0
    # nothing ran: the host-side state and the operands are what they were
    assert (stbuf.sumsq, stbuf.norm, stbuf.coef, stbuf.skip, stbuf.skipped) == (0.0, 0.0, 0.0, 0, 0)
    assert not any(buf) and not any(wsbuf)


def test_workspace_is_one_double_per_block_of_every_launch(hip):
    l = hip.lib()
    blocks = 2048                                      # the capped grid of a memory-bound launch
    per_launch = hip.lib().tf_grad_norm_workspace_bytes(1)
    assert per_launch == 8 * blocks
    assert l.tf_grad_norm_workspace_bytes(0) == 0 and l.tf_grad_norm_workspace_bytes(-3) == 0
    prev = 0
    for nseg in (1, 2, 127, 128, 129, 256, 257, 300, 1000):
        launches = -(-nseg // 128)                     # TF_SGD_MAX_SEGMENTS ranges per launch
        got = l.tf_grad_norm_workspace_bytes(nseg)
        assert got == 8 * blocks * launches, nseg
        assert got >= prev
        prev = got


def test_main_parses_the_two_flags_apart_from_the_reference_options():
    import main
    pos = ["train.txt", "val.txt"]
    a = main.trunk_arguments(pos)
    assert a.clip_grad_norm is None and a.skip_nonfinite is False
    a = main.trunk_arguments(pos + ["--clip-grad-norm", "2.5", "--skip-nonfinite", "--lr", "0.01"])
    assert a.clip_grad_norm == 2.5 and a.skip_nonfinite is True and a.lr == 0.01
    a = main.trunk_arguments(["--clip-grad-norm=10", "--freeze-bn"] + pos + ["--trainable-layers", "2"])
    assert a.clip_grad_norm == 10.0 and a.skip_nonfinite is False and a.freeze_bn and a.trainable_layers == 2
    # `arguments` resolves what it resolved before: the two flags are not among its options
    assert a.traindata == "train.txt" and a.valdata == "val.txt"
    assert not hasattr(main.arguments(pos), "clip_grad_norm") and not hasattr(main.arguments(pos), "skip_nonfinite")
    for argv in (["--clip-grad-norm", "1.0"], ["--skip-nonfinite"]):
        with pytest.raises(SystemExit):
            main.arguments(pos + argv)
    main.trunk_arguments(pos + ["--clip-grad-norm", "1e-3"])
    for bad in ("0", "-1", "nan", "abc"):
        with pytest.raises(SystemExit):
            main.trunk_arguments(pos + ["--clip-grad-norm", bad])


def _engine_on_cpu(**kw):
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.loss import DetectionCriterion
    from tinyfaces.models.model import DetectionModel
    torch.manual_seed(0)
    m = DetectionModel(num_objects=1, num_templates=25)
    return TrainEngine(m, DetectionCriterion(25), lr=1e-4, momentum=0.9, weight_decay=5e-4, device="cpu", **kw)


def test_engine_constructs_with_clipping_and_refuses_what_it_cannot_do(monkeypatch):
    eng = _engine_on_cpu(max_grad_norm=1.0)
    assert eng.max_grad_norm == 1.0 and eng.skip_nonfinite is False and eng._clip_on()
    assert eng.last_grad_norm is None and eng.skipped_steps == 0                 # nothing stepped yet: no device state, no sync
    assert eng.set_max_grad_norm(None) is eng and not eng._clip_on()
    assert eng.set_max_grad_norm(3).max_grad_norm == 3.0
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            eng.set_max_grad_norm(bad)
    assert eng.max_grad_norm == 3.0
    eng = _engine_on_cpu(skip_nonfinite=True)
    assert eng.max_grad_norm is None and eng._clip_on()
    plain = _engine_on_cpu()
    assert plain.max_grad_norm is None and plain.skip_nonfinite is False and not plain._clip_on()
    assert "clip" not in str(sorted(plain.optimizer_state_dict()))               # nothing new goes into checkpoints
    # per-bucket SGD applies a bucket before the global norm exists
    monkeypatch.setenv("TINYFACES_SGD_PER_BUCKET", "1")
    monkeypatch.setattr("tinyfaces.engine.TrainEngine._setup_overlap", lambda self: None)      # (events need a device)
    for kw in (dict(max_grad_norm=1.0), dict(skip_nonfinite=True)):
        with pytest.raises(ValueError, match="TINYFACES_SGD_PER_BUCKET"):
            _engine_on_cpu(**kw)
    eng = _engine_on_cpu()                                                       # the knob alone stays what it was
    assert eng.sgd_per_bucket
    with pytest.raises(ValueError, match="TINYFACES_SGD_PER_BUCKET"):
        eng.set_max_grad_norm(1.0)


@pytest.mark.parametrize("frozen,k", [(False, 4), (True, 4), (True, 2), (True, 0)])
def test_norm_ranges_cover_the_trained_tensors_and_nothing_of_another_tensor(frozen, k):
    """The ranges the engine hands to tf_grad_clip_coef: every element of every trained tensor, no element of any other tensor, all bounds
    4-aligned (the 16-byte path), ascending and disjoint; what they hold beyond the trained tensors is the alignment pad of a trained slot."""
    eng = _engine_on_cpu(max_grad_norm=1.0)
    m = eng.model
    m.freeze_batchnorm(frozen).set_trainable_layers(k)
    segs = eng._norm_segments()
    assert segs == sorted(segs) and all(s % 4 == 0 and e % 4 == 0 and e > s for s, e in segs)
    assert all(a[1] < b[0] for a, b in zip(segs, segs[1:]))                      # touching ranges were joined
    inside = torch.zeros(eng.flat_p.numel(), dtype=torch.bool)
    for s, e in segs:
        inside[s:e] = True
    trained = set(m.trainable_parameter_names())
    assert trained
    pads = 0
    for n, (o, num) in m._segments.items():
        if n in trained:
            assert bool(inside[o:o + num].all()), n
            pads += (-num) % 4
        else:
            assert not bool(inside[o:o + (num + 3) // 4 * 4].any()), n
    assert int(inside.sum()) == sum(m._segments[n][1] for n in trained) + pads
    if not frozen:
        assert len(segs) <= 4                                                    # one launch instead of one range per tensor


def _stub_step(eng, monkeypatch):
    """Everything of TrainEngine.step that needs a device replaced by stubs; returns the call log."""
    from tinyfaces import ops
    m = eng.model
    calls = []
    monkeypatch.setattr(m, "_sync_tables", lambda dev: None)
    monkeypatch.setattr(m, "_run_forward", lambda x, training=True: torch.zeros(1))
    monkeypatch.setattr(m, "_run_backward", lambda x, grad, persistent=False: m._grad_flat_persistent)
    monkeypatch.setattr(ops, "criterion_fwd_bwd", lambda *a, **kw: (torch.zeros(2, dtype=torch.float64), torch.zeros(1), None))

    def sgd_step(*a, **kw):
        calls.append(("sgd_step", len(a), dict(kw)))

    def sgd_step_segments(*a, **kw):
        calls.append(("sgd_step_segments", len(a), dict(kw)))

    def grad_clip_coef(grad, segments, state, **kw):
        calls.append(("grad_clip_coef", list(segments), dict(kw)))
        return state

    monkeypatch.setattr(ops, "sgd_step", sgd_step)
    monkeypatch.setattr(ops, "sgd_step_segments", sgd_step_segments)
    monkeypatch.setattr(ops, "grad_clip_coef", grad_clip_coef)
    monkeypatch.setattr(ops, "ClipState", lambda device: "the state")
    return calls


@pytest.mark.parametrize("frozen", [False, True])
def test_default_step_calls_what_it_always_called(monkeypatch, frozen):
    eng = _engine_on_cpu()
    eng.model.freeze_batchnorm(frozen)
    calls = _stub_step(eng, monkeypatch)
    x = torch.zeros(1, 3, 8, 8)
    eng.step(x, x, x)
    name = "sgd_step_segments" if frozen else "sgd_step"
    assert [c[0] for c in calls] == [name] * 3                                   # trunk, score_res3, score_res4 (the upsample group has lr 0)
    assert all(c[1] == (8 if frozen else 7) and c[2] == {} for c in calls)      # positional arguments only, as before: no clip_state
    assert eng._clip_state is None and eng.skipped_steps == 0

    eng.set_max_grad_norm(2.0)
    del calls[:]
    eng.step(x, x, x)
    assert [c[0] for c in calls] == ["grad_clip_coef"] + [name] * 3              # one coefficient launch, in front of the updates
    assert calls[0][1] == eng._norm_segments()
    assert calls[0][2] == dict(grad_scale=1.0, max_norm=2.0, skip_nonfinite=False)
    assert all(c[2] == {"clip_state": "the state"} for c in calls[1:])

    eng.set_max_grad_norm(None)
    eng.skip_nonfinite = True
    del calls[:]
    eng.step(x, x, x)
    assert calls[0][0] == "grad_clip_coef" and calls[0][2] == dict(grad_scale=1.0, max_norm=None, skip_nonfinite=True)
    assert all(c[2] == {"clip_state": "the state"} for c in calls[1:])


def test_python_ops_have_no_cpu_fallback_and_keep_their_signatures():
    from tinyfaces import ops, trainer
    p = torch.nn.Parameter(torch.ones(8))
    p.grad = torch.ones(8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.clip_grad_norm_([p], 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ClipState("cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.grad_clip_coef(torch.ones(8), [(0, 8)], None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.scale_segments(torch.ones(8), [(0, 8)], None)
    assert torch.equal(p.grad, torch.ones(8))
    assert ops.clip_skipped_steps("cpu") == 0
    # keyword additions behind the existing signatures, off by default
    sig = inspect.signature(trainer.train)
    assert list(sig.parameters)[:6] == ["model", "loss_fn", "optimizer", "dataloader", "epoch", "device"]
    assert sig.parameters["max_grad_norm"].default is None and sig.parameters["skip_nonfinite"].default is False
    for f in (ops.sgd_step, ops.sgd_step_segments):
        ps = inspect.signature(f).parameters
        assert list(ps)[-1] == "clip_state" and ps["clip_state"].default is None and ps["grad_scale"].default == 1.0
    ps = inspect.signature(ops.grad_clip_coef).parameters
    assert list(ps) == ["grad_flat", "segments", "state", "grad_scale", "max_norm", "skip_nonfinite"]
