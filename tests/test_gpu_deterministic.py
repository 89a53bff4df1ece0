"""-m gpu: the deterministic switch on the whole training step (tf_set_deterministic, TrainEngine(deterministic=True)).

ResNet-50, N = 2, 3 x 160 x 192, seeds fixed.  With the switch on, two passes over the same weights and batch must agree in EVERY bit: the flat
gradient (fp32 and bf16, the batch-statistics and the frozen-BN graph) and, after three engine steps, the parameters, the optimizer state, the
BatchNorm buffers and the model EMA (sha256).  Nothing here asserts that the default mode differs between runs.  Parity: the comparison
tests/test_gpu_model.py makes against the reference's golden vectors and the float64 oracle, bars unchanged, run with the switch on."""
import hashlib

import pytest
import torch

from gpu_util import report

pytestmark = pytest.mark.gpu

SHAPE = (2, 3, 160, 192)


def _model(dtype, frozen, seed=6):
    from test_gpu_frozen_bn import _oracle, _product
    m = _product(_oracle("resnet50", seed=seed), "resnet50").set_compute_dtype(dtype)
    if frozen:
        m.freeze_batchnorm().set_trainable_layers(4)          # every stage and the stem trained: the stem weight gradient runs
    return m.cuda().train()


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _state(lib):
    return lib.tf_get_deterministic(), lib.tf_get_stat_rows()


@pytest.mark.parametrize("frozen", [False, True], ids=["batch_stats", "frozen_bn"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_flat_gradient_repeats_bit_for_bit(dtype, frozen):
    from tinyfaces import ops
    from tinyfaces._hip import lib
    x = torch.randn(*SHAPE, generator=torch.Generator().manual_seed(5)).cuda()
    before = _state(lib())
    runs = []
    prev = ops.set_deterministic(True)
    try:
        assert lib().tf_get_stat_rows() > 16
        gy = None
        for _ in range(2):
            m = _model(dtype, frozen)                          # the same weights and buffers each time
            y = m(x)
            if gy is None:
                gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(6)).cuda()
            y.backward(gy)
            torch.cuda.synchronize()
            runs.append((y.detach().clone(), m._last_grad_flat.clone(), {k: v.clone() for k, v in m.state_dict().items()}))
    finally:
        ops.set_deterministic(prev)
    assert _state(lib()) == before
    (ya, ga, sa), (yb, gb, sb) = runs
    differing = int((ga.view(torch.int32) != gb.view(torch.int32)).sum())
    report(f"deterministic_flat_gradient[{dtype},{'frozen' if frozen else 'batch_stats'}]", elements=ga.numel(), differing=differing,
           nonzero=int((ga != 0).sum()))
    print(f"deterministic_flat_gradient[{dtype},frozen={frozen}] {differing} of {ga.numel()} elements differ")
    assert torch.isfinite(ga).all() and int((ga != 0).sum()) > ga.numel() // 4
    assert torch.equal(ya, yb)
    assert torch.equal(ga.view(torch.int32), gb.view(torch.int32))
    assert all(torch.equal(sa[k], sb[k]) for k in sa)          # running statistics, counters


ENGINES = {
    "sgd": dict(),
    "adamw_clip_ema": dict(optimizer="adamw", max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.999),
    "accum2": dict(accum_steps=2),
}


@pytest.mark.parametrize("frozen", [False, True], ids=["batch_stats", "frozen_bn"])
@pytest.mark.parametrize("config", sorted(ENGINES))
def test_two_engines_end_with_the_same_bits(config, frozen):
    """Three optimizer steps (accum_steps = 2: six micro-batches) from the same weights and data, twice: parameters, momentum / moments, BN
    buffers and the EMA equal by sha256.  Afterwards the switch and the statistic rows are what they were, and a default engine in the same
    process runs with folded rows again."""
    from tinyfaces._hip import lib
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.loss import DetectionCriterion
    g = torch.Generator().manual_seed(3)
    N, _, H, W = SHAPE
    xs = [torch.randn(*SHAPE, generator=g).cuda() for _ in range(3)]
    cm = torch.where(torch.rand(N, 25, H // 8, W // 8, generator=g) < 0.02, 1.0, -1.0).cuda()
    rm = torch.randn(N, 100, H // 8, W // 8, generator=g).cuda()
    kw = ENGINES[config]
    before = _state(lib())
    assert before[0] == 0 and before[1] <= 16
    digests = []
    for _ in range(2):
        m = _model(torch.bfloat16, frozen)
        eng = TrainEngine(m, DetectionCriterion(25, seed=11), lr=1e-3, momentum=0.9, weight_decay=5e-4, device="cuda", deterministic=True, **kw)
        for k in range(3 * eng.accum_steps):
            eng.step(xs[k % 3], cm.clone(), rm)
            assert _state(lib()) == before                      # on for the duration of the step only
        torch.cuda.synchronize()
        assert eng.steps == 3 and torch.isfinite(eng.flat_p).all()
        d = {"params": _sha(eng.flat_p), "momentum": _sha(eng.flat_m), "grad": _sha(m._grad_flat_persistent)}
        if config == "adamw_clip_ema":
            d["exp_avg_sq"], d["ema"] = _sha(eng.flat_v), _sha(eng.ema.flat)
        for k, v in m.state_dict().items():
            if "running_" in k or "num_batches" in k:
                d[k] = _sha(v)
        digests.append(d)
        eng.close()
    a, b = digests
    bad = [k for k in a if a[k] != b[k]]
    report(f"deterministic_engine[{config},{'frozen' if frozen else 'batch_stats'}]", digests=len(a), differing=str(bad))
    assert not bad, bad
    # a default engine afterwards: the library is back on its usual path (folded statistic rows, the switch off) during its step
    seen = []
    m = _model(torch.bfloat16, frozen)
    eng = TrainEngine(m, DetectionCriterion(25, seed=11), lr=1e-3, device="cuda")
    fwd = m._run_forward
    m._run_forward = lambda x, training: (seen.append(_state(lib())), fwd(x, training))[1]
    eng.step(xs[0], cm.clone(), rm)
    torch.cuda.synchronize()
    eng.close()
    assert seen == [before] and _state(lib()) == before


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_parity_bars_of_the_default_path_hold_with_the_switch_on(golden, dtype):
    """tests/test_gpu_model.py::test_train_forward_backward_vs_reference_golden, unchanged, inside the switch: the golden forward, the golden
    and float64-oracle gradient bars, the running statistics."""
    import test_gpu_model
    from tinyfaces import ops
    from tinyfaces._hip import lib
    before = _state(lib())
    prev = ops.set_deterministic(True)
    try:
        test_gpu_model.test_train_forward_backward_vs_reference_golden(golden, 2, dtype)
    finally:
        ops.set_deterministic(prev)
    assert _state(lib()) == before
