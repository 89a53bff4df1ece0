"""CPU: deterministic training -- everything that can be checked without a GPU.  The slice plan (tests/wgrad_det_ref.py against its own
invariants and against the library's workspace query, which is host code), the restatement's summation order on planted values, the switch
and what it does to the statistic rows, the refusals that must come back before anything is enqueued, and the argument checks of the new
engine, trainer and CLI keywords."""
import ctypes as C
import inspect
import itertools

import numpy as np
import pytest
import torch

import wgrad_det_ref as ref

ERR_ARG, ERR_UNSUPPORTED = -1, -3
F32, BF16 = 0, 1            # TF_F32, TF_BF16

SHAPES = [
    # M, Cin, Cout, taps
    (63, 64, 64, 1), (64, 64, 64, 1), (65, 64, 64, 1), (1, 40, 24, 1), (2700, 256, 1024, 1), (899, 512, 1024, 1), (110, 128, 128, 9),
    (12288, 1024, 256, 1), (6400, 64, 256, 1), (384, 147, 64, 1), (384, 512, 125, 1), (100000, 64, 64, 9),
]


@pytest.mark.parametrize("kernel", sorted(ref.KERNELS))
def test_slices_cover_the_pixels_exactly_none_is_empty_and_the_slab_caps_them(kernel):
    pk = ref.KERNELS[kernel]["PK"]
    for (M, Cin, Cout, taps), sk in itertools.product(SHAPES, [0, 1, 2, 3, 7, 16, 200, 5000]):
        if kernel == "all_taps":
            taps = 9
        sl = ref.plan(kernel, M, Cin, Cout, taps, sk)
        assert sl[0][0] == 0 and sl[-1][1] == M
        assert all(a < b for a, b in sl), "an empty slice"
        assert all(sl[i][1] == sl[i + 1][0] for i in range(len(sl) - 1))
        assert all((b - a) % pk == 0 for a, b in sl[:-1]), "only the last slice may end off a stage"
        assert len(sl) <= ref.requested_slices(kernel, M, Cin, Cout, taps, sk)
        one = ref.slice_bytes(kernel, Cin, Cout, taps)
        assert ref.preferred_bytes(kernel, M, Cin, Cout, taps, sk) == len(sl) * one > 0
        # the cap: a slab of k slices (and up to one slice less one byte more) never yields more than k, the plan stays a cover, no atomics
        for k in (1, 2, 3, len(sl)):
            capped = ref.plan(kernel, M, Cin, Cout, taps, sk, slab_bytes=k * one + one - 1)
            assert 1 <= len(capped) <= min(k, len(sl)) and capped[0][0] == 0 and capped[-1][1] == M and all(a < b for a, b in capped)
        assert ref.plan(kernel, M, Cin, Cout, taps, sk, slab_bytes=one - 1) is None
        assert ref.plan(kernel, M, Cin, Cout, taps, sk, slab_bytes=len(sl) * one) == sl


def _args(hip, dtype, N, H, W, Cin, Cout, K, stride, pad, ldx=None, lddy=None, tile=0, splitk=0, pro=False):
    buf = (C.c_float * 16)()
    p = C.cast(buf, C.c_void_p)
    a = hip.WgradArgs()
    OH, OW = (H + 2 * pad - K) // stride + 1, (W + 2 * pad - K) // stride + 1
    a.dtype = dtype
    a.N, a.H, a.W, a.Cin, a.OH, a.OW, a.Cout, a.KH, a.KW, a.stride, a.pad = N, H, W, Cin, OH, OW, Cout, K, K, stride, pad
    a.ldx, a.lddy, a.x, a.dy, a.dw_oihw, a.dw_ld = ldx or Cin, lddy or Cout, p, p, p, Cin * K * K
    a.tile, a.splitk = tile, splitk
    if pro:
        a.pro_scale, a.pro_shift = p, p
    a._keep = buf
    return a, N * OH * OW


CALLS = [
    # dtype, (N, H, W, Cin, Cout, K, stride, pad), ldx, lddy, tile, prologue -> kernel of tests/wgrad_det_ref.py
    (BF16, (1, 9, 7, 64, 64, 1, 1, 0), None, None, 0, False, "dma"),
    (BF16, (3, 30, 30, 256, 1024, 1, 1, 0), None, None, 1, False, "dma"),
    (BF16, (2, 21, 19, 128, 128, 3, 2, 1), None, None, 0, False, "dma"),
    (BF16, (2, 12, 16, 512, 125, 1, 1, 0), None, 128, 0, False, "dma"),
    (BF16, (2, 12, 16, 147, 64, 1, 1, 0), 192, None, 64, False, "reg64_bf16"),
    (BF16, (2, 12, 16, 128, 256, 3, 1, 1), None, None, 0, True, "reg64_bf16"),
    (BF16, (4, 40, 40, 64, 256, 1, 1, 0), None, None, 128, False, "reg128_bf16"),
    (F32, (1, 9, 7, 64, 64, 1, 1, 0), None, None, 0, False, "reg64_f32"),
    (F32, (2, 31, 29, 512, 1024, 1, 2, 0), None, None, 128, False, "reg128_f32"),
    (F32, (2, 20, 22, 64, 64, 3, 1, 1), None, None, 64, False, "reg64_f32"),
    (BF16, (2, 20, 22, 64, 64, 3, 1, 1), None, None, 0, False, "all_taps"),
    (BF16, (3, 32, 32, 256, 256, 3, 1, 1), None, None, 3, False, "all_taps"),
    (BF16, (1, 1, 1, 64, 64, 3, 1, 1), None, None, 3, False, "all_taps"),
]


@pytest.mark.parametrize("splitk", [0, 1, 3, 7, 1000])
@pytest.mark.parametrize("call", CALLS)
def test_the_workspace_query_is_the_restated_plan(hip, call, splitk):
    """tf_wgrad_det_workspace_bytes (host code) = slices x tiles x tile bytes of the plan tests/wgrad_det_ref.py restates, for every kernel the
    `tile` rules choose, and never 0 for a valid call; tf_wgrad_workspace_bytes keeps its zero where the all-taps kernel does not apply."""
    dtype, shape, ldx, lddy, tile, pro, kernel = call
    a, M = _args(hip, dtype, *shape, ldx=ldx, lddy=lddy, tile=tile, splitk=splitk, pro=pro)
    N, H, W, Cin, Cout, K = shape[:6]
    if kernel == "all_taps":
        M = N * (H + 2) * (W + 2)
    got = hip.lib().tf_wgrad_det_workspace_bytes(C.byref(a))
    assert got == ref.preferred_bytes(kernel, M, Cin, Cout, K * K, splitk) > 0
    assert (hip.lib().tf_wgrad_workspace_bytes(C.byref(a)) != 0) == (kernel == "all_taps")


def test_groups_are_a_function_of_the_slice_count(hip):
    for n in list(range(1, 40)) + [127, 128, 129, 255, 384, 1000]:
        assert hip.lib().tf_wgrad_det_groups(n) == ref.groups(n)
    assert [ref.groups(n) for n in (1, 15, 16, 31, 32, 127, 128)] == [1, 1, 2, 2, 4, 4, 16]


def test_refusals_come_back_before_anything_is_enqueued(hip):
    """No slab, a slab below one slice, a misaligned slab: TF_ERR_ARG.  (No GPU here: a launch would not come back as TF_ERR_ARG.)"""
    l = hip.lib()
    slab = (C.c_float * 64)()
    sp = C.cast(slab, C.c_void_p)
    for call in CALLS:
        dtype, shape, ldx, lddy, tile, pro, kernel = call
        a, _ = _args(hip, dtype, *shape, ldx=ldx, lddy=lddy, tile=tile, pro=pro)
        assert l.tf_conv2d_wgrad_det(C.byref(a), None) == ERR_ARG                                   # no slab
        a.partial_ws, a.partial_ws_bytes = sp, 256                                                  # below one slice (>= 16 KiB)
        assert l.tf_conv2d_wgrad_det(C.byref(a), None) == ERR_ARG
        a.partial_ws, a.partial_ws_bytes = C.c_void_p(sp.value + 4), 1 << 30                        # 16-byte stores need a 16-byte aligned slab
        assert l.tf_conv2d_wgrad_det(C.byref(a), None) == ERR_ARG
    assert l.tf_conv2d_wgrad_det(None, None) == ERR_ARG and l.tf_wgrad_det_workspace_bytes(None) == 0
    a, _ = _args(hip, BF16, 1, 9, 7, 64, 64, 1, 1, 0, ldx=60)                                       # the operand contract of tf_conv2d_wgrad
    assert l.tf_conv2d_wgrad_det(C.byref(a), None) == ERR_ARG and l.tf_wgrad_det_workspace_bytes(C.byref(a)) == 0
    a, _ = _args(hip, BF16, 2, 21, 19, 128, 128, 3, 2, 1, tile=3)                                   # stride 2 is not the all-taps kernel's
    a.partial_ws, a.partial_ws_bytes = sp, 1 << 30
    assert l.tf_conv2d_wgrad_det(C.byref(a), None) == ERR_UNSUPPORTED
    # stem
    p = sp
    assert l.tf_stem_wgrad_det_workspace_bytes(2, 37, 45) == 2 * 1 * 5 * 64 * 147 * 4              # tiles of 4 x 32 output pixels: 1 x 5 per image
    assert l.tf_stem_wgrad_det_workspace_bytes(12, 500, 500) == 384 * 64 * 147 * 4                 # the grid tf_stem_wgrad launches
    assert l.tf_stem_wgrad_det_workspace_bytes(0, 8, 8) == 0
    assert l.tf_stem_wgrad_det(1, p, 1, 8, 8, p, None, None, None, None, p, None, 1 << 20, None) == ERR_ARG       # no slab
    assert l.tf_stem_wgrad_det(1, p, 1, 8, 8, p, None, None, None, None, p, p, 64 * 147 * 4 - 1, None) == ERR_ARG  # below one tile
    assert l.tf_stem_wgrad_det(1, p, 1, 8, 8, p, p, None, None, None, p, p, 1 << 20, None) == ERR_ARG             # apply without coefficients
    assert l.tf_stem_wgrad_det(0, p, 1, 8, 8, p, None, None, None, None, p, p, 1 << 20, None) == ERR_UNSUPPORTED  # fp32
    assert not any(slab)


def test_the_restated_order_on_planted_values():
    """2^24 + 1 rounds to 2^24 in fp32: where the big slice sits in THE ORDER decides how many of the ones survive."""
    big, one = np.float32(2.0 ** 24), np.float32(1.0)
    for n in (1, 2, 3, 7, 15):                                   # one group: plain left-to-right
        p = np.full((n, 1), one, np.float32)
        p[0] = big
        assert ref.ordered_sum(p)[0] == big                      # every later 1 is lost
        p[0], p[-1] = one, big
        want = np.float32(n - 1) + big                           # n - 1 <= 14 first: even totals are exact, odd ones tie to even
        assert ref.ordered_sum(p)[0] == np.float32(float(n - 1) + 2.0 ** 24)
        assert want == ref.ordered_sum(p)[0]
    # 16 slices = 2 groups: group 0 takes the even slices, group 1 the odd ones, then t0 + t1
    p = np.full((16, 1), one, np.float32)
    p[0] = big
    assert ref.ordered_sum(p)[0] == np.float32(2.0 ** 24 + 8)    # group 0 loses its seven ones, group 1's eight arrive as one addend
    p = np.full((16, 1), one, np.float32)
    p[15] = big
    assert ref.ordered_sum(p)[0] == np.float32(2.0 ** 24 + 8 + 7 + 1)        # t0 = 8 exact; t1 = 7 + 2^24 ties up to 2^24 + 8
    # 32 slices = 4 groups of 8, 128 = 16 groups of 8; against a direct transcription of the header's loops
    rng = np.random.RandomState(0)
    for n in (16, 31, 32, 33, 127, 128, 200, 384):
        p = (rng.randn(n, 5, 3) * 10.0 ** rng.randint(-3, 4, (n, 1, 1))).astype(np.float32)
        G = ref.groups(n)
        t = [np.zeros((5, 3), np.float32) for _ in range(G)]
        for s in range(n):
            t[s % G] = t[s % G] + p[s]
        tot = t[0]
        for g in range(1, G):
            tot = tot + t[g]
        assert tot.dtype == np.float32 and np.array_equal(ref.ordered_sum(p), tot)
    # the row scale rides on the total, the total is added ONCE into what dw held
    p = np.array([[3.0, 5.0], [1.0, 1.0]], np.float32).reshape(2, 2, 1)
    got = ref.reduce_into(np.array([[10.0], [20.0]], np.float32), p, row_scale=[0.5, 2.0])
    assert np.array_equal(got, np.array([[12.0], [32.0]], np.float32))


def test_the_switch_unfolds_the_rows_and_gives_back_what_was_set(hip):
    from tinyfaces import ops
    l = hip.lib()
    assert "tf_set_deterministic" in hip.symbols() and "tf_conv2d_wgrad_det" in hip.symbols() and "tf_stem_wgrad_det" in hip.symbols()
    assert l.tf_version() >= 750
    rows0 = l.tf_get_stat_rows()
    try:
        assert l.tf_get_deterministic() == 0 and ops.is_deterministic() is False
        l.tf_set_stat_rows(4)
        assert ops.set_deterministic(True) is False
        assert ops.is_deterministic() is True and l.tf_get_stat_rows() > 16                 # unfolded while on
        l.tf_set_stat_rows(6)                                                               # kept for when the switch goes off
        assert l.tf_get_stat_rows() > 16
        assert ops.set_deterministic(True) is True                                          # nested: the previous state comes back
        assert ops.set_deterministic(False) is True
        assert l.tf_get_deterministic() == 0 and l.tf_get_stat_rows() == 6
        l.tf_set_stat_rows(0)
        assert ops.set_deterministic(True) is False and ops.set_deterministic(False) is True and l.tf_get_stat_rows() > 16
    finally:
        l.tf_set_deterministic(0)
        l.tf_set_stat_rows(rows0 if rows0 <= 16 else 0)


def _cpu_engine(**kw):
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as zoo
    from tinyfaces.models.loss import DetectionCriterion
    return TrainEngine(zoo.DetectionModel(base_model=zoo.resnet50, num_templates=25), DetectionCriterion(25), device="cpu", **kw)


def test_engine_and_trainer_keywords(monkeypatch):
    from tinyfaces import ops, trainer
    from tinyfaces.engine import TrainEngine
    ps = inspect.signature(TrainEngine.__init__).parameters
    assert list(ps)[-1] == "deterministic" and ps["deterministic"].default is False
    assert list(inspect.signature(TrainEngine.step).parameters) == ["self", "x", "class_map", "regression_map", "apply"]
    ts = inspect.signature(trainer.train).parameters
    assert list(ts)[-1] == "deterministic" and ts["deterministic"].default is False
    assert "False (the default): no new call" in TrainEngine.__init__.__doc__ and "False (the default): no new call" in trainer.train.__doc__
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="deterministic"):
            _cpu_engine(deterministic=bad)
        with pytest.raises(ValueError, match="deterministic"):
            trainer.train(torch.nn.Identity(), None, torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1), [], 0, "cpu", deterministic=bad)
    # the engine turns the switch on for the duration of a step and puts back what it found; a default engine never touches it
    seen = []
    for det in (False, True):
        eng = _cpu_engine(deterministic=det)
        assert eng.deterministic is det
        m = eng.model
        monkeypatch.setattr(m, "_check_partial_freeze", lambda: None)
        monkeypatch.setattr(m, "_sync_tables", lambda dev: None)
        monkeypatch.setattr(m, "_run_forward", lambda x, training=True: seen.append(ops.is_deterministic()))
        monkeypatch.setattr(m, "_run_backward", lambda x, g, persistent=False, eng=eng: torch.zeros(eng.flat_p.numel()))
        monkeypatch.setattr(ops, "criterion_fwd_bwd", lambda *a, **kw: (torch.zeros(2, dtype=torch.float64), None, None))
        monkeypatch.setattr(ops, "sgd_step", lambda *a, **kw: None)
        calls = []
        real = ops.set_deterministic
        monkeypatch.setattr(ops, "set_deterministic", lambda on: (calls.append(on), real(on))[1])
        eng.step(torch.zeros(1, 3, 8, 8), None, None)
        assert ops.is_deterministic() is False and calls == ([True, False] if det else [])
        monkeypatch.setattr(ops, "set_deterministic", real)
        if det:                                                   # ... also when the step raises, and when the switch was already on
            monkeypatch.setattr(m, "_run_forward", lambda x, training=True: (_ for _ in ()).throw(RuntimeError("boom")))
            with pytest.raises(RuntimeError, match="boom"):
                eng.step(torch.zeros(1, 3, 8, 8), None, None)
            assert ops.is_deterministic() is False
            ops.set_deterministic(True)
            try:
                with pytest.raises(RuntimeError, match="boom"):
                    eng.step(torch.zeros(1, 3, 8, 8), None, None)
                assert ops.is_deterministic() is True
            finally:
                ops.set_deterministic(False)
    assert seen == [False, True]
    # trainer.train: on for the duration of the call (an empty loader: nothing runs), back afterwards
    trainer.train(torch.nn.Identity(), None, torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1), [], 0, "cpu", deterministic=True)
    assert ops.is_deterministic() is False


def test_main_parses_the_flag_apart_from_the_reference_options():
    import main
    pos = ["train.txt", "val.txt"]
    assert main.trunk_arguments(pos).deterministic is False
    a = main.trunk_arguments(["--deterministic"] + pos + ["--lr", "0.01"])
    assert a.deterministic is True and a.lr == 0.01 and a.traindata == "train.txt"
    assert "deterministic" not in vars(main.arguments(pos))
    with pytest.raises(SystemExit):
        main.arguments(pos + ["--deterministic"])
    with pytest.raises(SystemExit):
        main.trunk_arguments(pos + ["--deterministic", "--no-such-flag"])
    line = main.deterministic_description()
    for word in ("bit for bit", "per process", "soft-margin", "multi-rank", "data loader"):
        assert word in line
