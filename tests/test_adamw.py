"""CPU: the host side of the AdamW optimizer -- the float32 restatement the GPU tests compare the kernels with (tests/adamw_ref.py) against
torch.optim.AdamW itself, the integer power of the bias correction, the warm-up closed form against LinearLR, the flag parsers, and the
format of the exported optimizer state.

Where the bar of the first test comes from: the restatement and torch's own fp32 single-tensor path are two fp32 evaluation orders of one
formula (torch folds sqrt(bias2) and the step size differently), so neither is the other's reference.  Both are measured against torch's
float64 result from the same fp32 state; the yardstick is the error of torch's fp32 result, and the restatement may be at most 2 x as far
away.  Measured values go through gpu_util.report (profiles/adamw_parity.txt)."""
import argparse
import math

import numpy as np
import pytest
import torch

import adamw_ref
from gpu_util import report

N = 200_000
HYPER = [(1e-4, 5e-4, 1e-8), (1e-3, 1e-2, 1e-8), (3e-2, 0.1, 1e-6)]            # (lr, weight decay, eps)
BETAS = (0.9, 0.999)


def _i32(a):
    return np.ascontiguousarray(a).view(np.int32)


def _planted(gen, n):
    """Order 1 with planted x 1e3, x 1e-6 and exact zeros."""
    x = torch.randn(n, generator=gen, dtype=torch.float64)
    x[::97] *= 1e3
    x[5::89] *= 1e-6
    x[11::101] = 0.0
    return x


def _torch_step(p, g, m, v, step, lr, wd, eps, dtype):
    """One step of torch.optim.AdamW(foreach=False) from the given state, in `dtype`: (p, exp_avg, exp_avg_sq) after it."""
    w = torch.nn.Parameter(p.to(dtype).clone())
    opt = torch.optim.AdamW([w], lr=lr, betas=BETAS, eps=eps, weight_decay=wd, foreach=False)
    opt.state[w] = {"step": torch.tensor(float(step)), "exp_avg": m.to(dtype).clone(), "exp_avg_sq": v.to(dtype).clone()}
    w.grad = g.to(dtype).clone()
    opt.step()
    st = opt.state[w]
    assert int(st["step"]) == step + 1
    return w.detach(), st["exp_avg"], st["exp_avg_sq"]


_STATE = {}


def _common_state(lr, wd, eps):
    """What five float64 steps of torch's AdamW leave, rounded to float32, and the gradient of step 6; computed once per hyper-parameter set."""
    key = (lr, wd, eps)
    if key not in _STATE:
        gen = torch.Generator().manual_seed(1234)
        p = _planted(gen, N)
        w = torch.nn.Parameter(p.clone())
        opt = torch.optim.AdamW([w], lr=lr, betas=BETAS, eps=eps, weight_decay=wd, foreach=False)
        for _ in range(5):
            w.grad = torch.randn(N, generator=gen, dtype=torch.float64)
            opt.step()
        st = opt.state[w]
        assert int(st["step"]) == 5
        p5 = w.detach().float()
        p5[11::101] = 0.0                                                      # exact zeros in p as well
        _STATE[key] = (p5, st["exp_avg"].float(), st["exp_avg_sq"].float(), _planted(gen, N).float())
    return _STATE[key]


@pytest.mark.parametrize("lr,wd,eps", HYPER, ids=[f"lr{h[0]:g}_wd{h[1]:g}_eps{h[2]:g}" for h in HYPER])
def test_restatement_is_as_close_to_float64_adamw_as_torchs_own_float32_step(lr, wd, eps):
    p, m, v, g = _common_state(lr, wd, eps)
    assert int((p == 0).sum()) > 1000 and int((g == 0).sum()) > 1000 and float(v.min()) > 0.0
    p64, m64, v64 = _torch_step(p, g, m, v, 5, lr, wd, eps, torch.float64)
    p32, m32, v32 = _torch_step(p, g, m, v, 5, lr, wd, eps, torch.float32)
    rp, rm, rv = adamw_ref.adamw_step(p.numpy(), g.numpy(), m.numpy(), v.numpy(), 6, lr, BETAS, eps, wd)
    assert rp.dtype == rm.dtype == rv.dtype == np.float32

    def worst(x, x64, scale):
        return float(((torch.as_tensor(x).double() - x64).abs() / scale).max())

    sp, sv = p64.abs() + lr, v64.abs()
    assert float(sv.min()) > 0.0
    yard_p, yard_v = worst(p32, p64, sp), worst(v32, v64, sv)
    mine_p, mine_v = worst(rp, p64, sp), worst(rv, v64, sv)
    report("adamw_restatement_vs_torch", lr=lr, wd=wd, eps=eps, elements=N, p_yardstick=yard_p, p_restatement=mine_p, p_ratio=mine_p / yard_p,
           v_yardstick=yard_v, v_restatement=mine_v, v_ratio=mine_v / yard_v)
    print(f"adamw restatement lr={lr:g} wd={wd:g} eps={eps:g}: p {mine_p:.3e} / {yard_p:.3e} = {mine_p / yard_p:.3f}, "
          f"v {mine_v:.3e} / {yard_v:.3e} = {mine_v / yard_v:.3f}")
    assert yard_p > 0.0 and yard_v > 0.0
    assert mine_p <= 2.0 * yard_p
    assert mine_v <= 2.0 * yard_v
    assert np.array_equal(_i32(rm), _i32(m32.numpy()))                         # exp_avg: torch.lerp, bit for bit
    assert np.isfinite(rp).all() and np.isfinite(rv).all()


U = 2.0 ** -53
POW_STEPS = sorted(set(list(range(1, 300)) + [2 ** k for k in range(1, 20)] + [2 ** k - 1 for k in range(2, 21)] + [999_983, 10 ** 6]
                       + np.random.default_rng(7).integers(1, 10 ** 6, 500).tolist()))
POW_BETAS = (0.9, 0.999, 0.99, 0.5, 0.95)


def test_pow_int_tracks_the_float_power_up_to_a_million_steps():
    """pow_int(beta, t) against beta ** t for t up to 10^6 (where the power is a normal double): relative difference <= 64 * 2^-53.

    Square-and-multiply in plain double products cannot hold that bar: every squaring doubles the relative error its operand carries, up to
    (t - 1) * 2^-53 in all (measured with such a loop: 108 * 2^-53 at beta = 0.9, t = 511; 56850 * 2^-53 at beta = 0.999, t = 707923).  So
    every product of the loop is a double-double product (Dekker), still built from plain double operations the host repeats one for one:
    each carries about 2^-100 of relative error, forty of them nothing that shows, and the high word is the true power rounded once.
    Against exact rational arithmetic (t < 400, far from underflow) that is asserted as 2^-53 (1 + 2^-10); against Python's power, itself
    within an ulp, the measured worst is 1.8 * 2^-53, at the power next to the smallest normal double, where the low words are subnormal."""
    import fractions
    worst, worst_at, small = 0.0, None, 0.0
    for beta in POW_BETAS:
        for t in POW_STEPS:
            want = beta ** t
            got = adamw_ref.pow_int(beta, t)
            if want == 0.0:
                assert got == 0.0
                continue
            if want < 2.3e-308:                                                # subnormal powers have no relative accuracy to speak of
                continue
            rel = abs(got - want) / want
            if rel > worst:
                worst, worst_at = rel, (beta, t)
            if t <= 64:
                small = max(small, rel)
    assert adamw_ref.pow_int(0.9, 0) == 1.0 and adamw_ref.pow_int(0.0, 3) == 0.0 and adamw_ref.pow_int(0.9, 1) == 0.9
    exact = 0.0
    for beta in (0.9, 0.999):
        for t in range(1, 400):
            true = fractions.Fraction(beta) ** t
            exact = max(exact, float(abs(fractions.Fraction(adamw_ref.pow_int(beta, t)) - true) / true))
    report("adamw_pow_int", worst_rel=worst, worst_in_u=worst / U, worst_at=worst_at, worst_rel_t_le_64=small, bound=64 * U, exponents=len(POW_STEPS),
           worst_rel_against_exact_t_lt_400=exact)
    print(f"pow_int: worst relative difference {worst:.3e} = {worst / U:.2f} x 2^-53 at (beta, t) = {worst_at}; t <= 64: {small / U:.2f} x 2^-53; "
          f"against exact arithmetic, t < 400: {exact / U:.3f} x 2^-53")
    assert exact <= U * (1.0 + 2.0 ** -10)
    assert worst <= 64 * U, (worst_at, worst)


def test_bias_correction_from_pow_int_is_accurate():
    """What the kernels read is bias = 1 - pow_int(beta, t).  pow_int is within 2 u of beta^t (u = 2^-53; one rounding, doubled for the
    powers next to the underflow threshold, which are negligible against 1 anyway), libm's pow within 2 u (one ulp), and each subtraction
    from 1 rounds once: |bias - (1 - beta ** t)| <= 4 u beta^t + 2 u."""
    worst = 0.0
    for beta in POW_BETAS:
        for t in POW_STEPS:
            want = 1.0 - beta ** t
            got = adamw_ref.bias_corrections((beta, beta), t)[0]
            bound = 4 * U * beta ** t + 2 * U
            assert abs(got - want) <= bound, (beta, t, got, want)
            assert 0.0 < got <= 1.0
            worst = max(worst, abs(got - want) / want)
    report("adamw_bias_correction", worst_rel=worst)


@pytest.mark.parametrize("iters,factor", [(1, 1e-3), (3, 1e-3), (10, 0.1), (7, 1.0), (1000, 1e-3)])
def test_warmup_closed_form_is_linear_lr(iters, factor):
    import main
    from tinyfaces import trainer
    base = 1e-4
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([w], lr=base)
    sched = torch.optim.lr_scheduler.LinearLR(opt, start_factor=factor, total_iters=iters)
    for t in range(min(iters, 40) + 5):
        want = sched.get_last_lr()[0]
        got = base * trainer.warmup_factor(t, iters, factor)
        assert got == pytest.approx(want, rel=1e-12), (t, got, want)            # (LinearLR's chained form rounds a little differently step by step)
        assert main.lr_with_warmup(base, 0, t, iters, factor) == got
        opt.step()
        sched.step()
    assert trainer.warmup_factor(iters, iters, factor) == 1.0 and trainer.warmup_factor(10 ** 9, iters, factor) == 1.0
    assert trainer.warmup_factor(0, iters, factor) == pytest.approx(factor)
    # multiplied into StepLR's closed form; a resumed run lands on the same value
    assert main.lr_with_warmup(base, 25, 25 * 3 + 1, iters, factor) == main.lr_at(base, 25) * trainer.warmup_factor(76, iters, factor)


def test_warmup_off_and_refusals():
    import main
    from tinyfaces import trainer
    assert trainer.warmup_factor(0, 0, 1e-3) == 1.0 and trainer.warmup_factor(5, 0, 0.5) == 1.0
    assert main.lr_with_warmup(1e-4, 20, 0) == main.lr_at(1e-4, 20)
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            trainer.warmup_factor(0, 3, bad)
    with pytest.raises(ValueError):
        trainer.warmup_factor(0, -1, 0.5)
    assert main.steps_per_epoch(7, 2) == 4 and main.steps_per_epoch(6, 2) == 3 and main.steps_per_epoch(5, 1) == 5


def test_flag_parsers_and_their_refusals(capsys):
    import main
    args = main.trunk_arguments(["synthetic", "synthetic"])
    assert (args.optimizer, args.adam_beta1, args.adam_beta2, args.adam_eps) == ("sgd", 0.9, 0.999, 1e-8)
    assert (args.warmup_iters, args.warmup_factor) == (0, 1e-3)
    args = main.trunk_arguments(["synthetic", "synthetic", "--optimizer", "adamw", "--adam-beta1", "0.8", "--adam-beta2", "0.99", "--adam-eps", "1e-6",
                                 "--warmup-iters", "3", "--warmup-factor", "0.5", "--lr", "1e-3"])
    assert (args.optimizer, args.adam_beta1, args.adam_beta2, args.adam_eps) == ("adamw", 0.8, 0.99, 1e-6)
    assert (args.warmup_iters, args.warmup_factor, args.lr) == (3, 0.5, 1e-3)
    assert main._adam_beta("0") == 0.0 and main._warmup_factor("1") == 1.0 and main._warmup_iters("0") == 0
    for parser, bad in ((main._adam_beta, "1"), (main._adam_beta, "-0.1"), (main._adam_beta, "nan"), (main._adam_eps, "0"), (main._adam_eps, "-1e-8"),
                        (main._adam_eps, "inf"), (main._adam_eps, "nan"), (main._warmup_iters, "-1"), (main._warmup_factor, "0"),
                        (main._warmup_factor, "1.01"), (main._warmup_factor, "nan")):
        with pytest.raises(argparse.ArgumentTypeError):
            parser(bad)
    for argv in (["--optimizer", "adam"], ["--adam-beta2", "1"], ["--adam-eps", "0"], ["--warmup-iters", "-2"], ["--warmup-factor", "2"]):
        with pytest.raises(SystemExit):
            main.trunk_arguments(["synthetic", "synthetic"] + argv)
    capsys.readouterr()
    # the new flags are not part of the reference's table
    assert not [n for n, _ in main.REFERENCE_FLAGS + main.EXTRA_FLAGS if "adam" in n or "warmup" in n or n == "--optimizer"]


def test_exported_group_keys_are_a_real_adamws():
    """The engine's exporter without an engine (no GPU here): a stand-in object with the attributes _adamw_state_dict reads."""
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as zoo
    m = zoo.DetectionModel(base_model=zoo.resnet50, num_templates=25)
    lr, betas, eps, wd = 1e-3, (0.85, 0.995), 1e-7, 0.02
    real = torch.optim.AdamW(m.learnable_parameters(lr), lr=lr, betas=betas, eps=eps, weight_decay=wd).state_dict()
    eng = TrainEngine.__new__(TrainEngine)
    eng.model, eng.optimizer, eng.betas, eng.eps, eng.weight_decay, eng.lr, eng.steps, eng._window = m, "adamw", betas, eps, wd, lr, 0, 0
    m._segments = {}
    sd = eng.optimizer_state_dict(base_lr=lr)
    assert sd["state"] == {} and len(sd["param_groups"]) == len(real["param_groups"]) == 4
    for mine, theirs in zip(sd["param_groups"], real["param_groups"]):
        assert set(mine) == set(theirs) | {"initial_lr"}
        assert mine["params"] == theirs["params"]
        for k in theirs:
            if k not in ("params", "lr"):
                assert mine[k] == theirs[k], k
        assert mine["lr"] == pytest.approx(theirs["lr"]) and mine["initial_lr"] == pytest.approx(theirs["lr"])
    assert sd["param_groups"][0]["betas"] == betas and sd["param_groups"][0]["eps"] == eps and sd["param_groups"][0]["weight_decay"] == wd
    # ... and a real AdamW takes it
    opt = torch.optim.AdamW(m.learnable_parameters(lr), lr=lr, betas=betas, eps=eps, weight_decay=wd)
    opt.load_state_dict(sd)


def test_engine_refuses_bad_adam_arguments_before_it_touches_a_device():
    from tinyfaces import ops
    for betas, eps in (((1.0, 0.999), 1e-8), ((0.9, -0.1), 1e-8), ((0.9, 0.999), 0.0), ((0.9, 0.999), float("nan"))):
        with pytest.raises(ValueError):
            ops._adam_hyper("test", 1e-3, betas, eps, 0.0)
    assert ops._adam_hyper("test", 1e-3, (0.0, 0.5), 1e-8, 0.1) == (1e-3, 0.0, 0.5, 1e-8, 0.1)


def test_library_declares_the_adamw_entry_points(hip):
    l = hip.lib()
    assert l.tf_version() >= 710 and {"tf_adamw_advance", "tf_adamw_step", "tf_adamw_step_segments"} <= set(hip.symbols())
    import ctypes as C
    assert C.sizeof(hip.AdamState) == 24
    # argument errors are answered on the host, without a launch
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    tab = (hip.i64 * 2)(0, 8)
    bad = (hip.i64 * 4)(8, 16, 0, 4)
    ok = (1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0, 0.0)
    assert l.tf_adamw_advance(None, 0.9, 0.999, None, None) == -1 and l.tf_adamw_advance(p, 1.0, 0.999, None, None) == -1
    assert l.tf_adamw_step(None, p, p, p, None, 8, *ok, p, None, None) == -1
    assert l.tf_adamw_step(p, p, p, p, None, 8, *ok, None, None, None) == -1                                   # no state
    assert l.tf_adamw_step(p, p, p, p, None, 8, 1e-3, 0.9, 0.999, 0.0, 1e-2, 1.0, 0.0, p, None, None) == -1       # eps == 0
    assert l.tf_adamw_step(p, p, p, p, None, 8, 1e-3, 0.9, 0.999, -1e-8, 1e-2, 1.0, 0.0, p, None, None) == -1
    assert l.tf_adamw_step(p, p, p, p, None, 8, 1e-3, 0.9, 1.0, 1e-8, 1e-2, 1.0, 0.0, p, None, None) == -1
    assert l.tf_adamw_step(p, p, p, p, None, -1, *ok, p, None, None) == -1
    assert l.tf_adamw_step(None, None, None, None, None, 0, *ok, None, None, None) == 0                        # n == 0: nothing to launch
    assert l.tf_adamw_step_segments(p, p, p, None, None, tab, 1, *ok, p, None, None) == -1
    assert l.tf_adamw_step_segments(p, p, p, p, None, None, 1, *ok, p, None, None) == -1
    assert l.tf_adamw_step_segments(p, p, p, p, None, bad, 2, *ok, p, None, None) == -1                        # unordered table
    assert l.tf_adamw_step_segments(p, p, p, p, None, tab, 1, 1e-3, 0.9, 0.999, 0.0, 1e-2, 1.0, 0.0, p, None, None) == -1
    assert l.tf_adamw_step_segments(None, None, None, None, None, None, 0, *ok, None, None, None) == 0
