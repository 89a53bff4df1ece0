"""-m gpu: fine-tuning with FROZEN BatchNorm (DetectionModel.freeze_batchnorm, executor mode 2: csrc/detnet.hip).

Reference = the CPU oracle (oracle/model.py, plain nn.BatchNorm2d) in train() with every BatchNorm2d in eval() and its parameters
requires_grad = False: what torchvision's FrozenBatchNorm2d computes.  Bars are the project's existing ones for the same quantities:
fp32 maps within 1e-3, every gradient tensor cosine > 0.9999 and median relative error < 5e-3 (tests/test_gpu_fullsize.py:120-121);
bf16 maps < 1.8e-2, every tensor >= 0.90, 5th percentile > 0.93, median > 0.96 (tests/test_gpu_fullsize.py:134-136, without the
layer-1 BN exception: BN vectors have no gradient here); the optimisation loop 2e-2 against the reference and 2e-3 / 1e-1 engine against
trainer (tests/test_gpu_model.py).  Measured values are written through gpu_util.report (committed: profiles/frozen_bn_parity.txt)."""
import io
import os
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from gpu_util import err, report

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BS, SIDE = 12, 500
ODD = (2, 203, 187)
BN_FIELDS = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def _cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float(a @ b / (a.norm() * b.norm() + 1e-30))


def _freeze_oracle(om):
    """The reference semantics: train() mode, every BatchNorm2d in eval(), its parameters without a gradient."""
    om.train()
    for mod in om.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eval()
            for p in mod.parameters():
                p.requires_grad_(False)
    return om


def _perturb_bn(om, seed):
    """Running statistics and affines away from their initial (0, 1, 1, 0): a frozen BN must be a NON-trivial affine in the test."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in om.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.copy_(0.1 * torch.randn(mod.running_mean.shape, generator=g))
                mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=g))
                mod.weight.mul_(0.8 + 0.4 * torch.rand(mod.weight.shape, generator=g))
                mod.bias.add_(0.05 * torch.randn(mod.bias.shape, generator=g))
    return om


def _oracle(trunk="resnet101", seed=0):
    from oracle.model import OracleDetectionModel, tame_init_
    om = OracleDetectionModel(num_templates=25)
    if trunk != "resnet101":
        from oracle.resnet import ResNet
        om.model = ResNet({"resnet50": (3, 4, 6, 3), "resnet152": (3, 8, 36, 3)}[trunk])
        del om.model.layer4
    return _perturb_bn(tame_init_(om, seed), seed + 1)


def _product(om, trunk="resnet101"):
    from tinyfaces.models import model as mm
    m = mm.DetectionModel(base_model=getattr(mm, trunk), num_templates=25)
    m.load_state_dict(om.state_dict(), strict=True)
    return m


def _bn_snapshot(m):
    sd = m.state_dict()
    return {k: v.detach().clone().cpu() for k, v in sd.items()
            if (".bn" in k or "downsample.1." in k) and k.rsplit(".", 1)[1] in BN_FIELDS}


def _oracle_pass(om, x, gy):
    """Forward + backward of the frozen oracle on the CPU: (y, {name: gradient})."""
    torch.set_num_threads(min(64, os.cpu_count() or 8))
    om = _freeze_oracle(om)
    for p in om.parameters():
        p.grad = None
    y = om(x)
    y.backward(gy)
    return y.detach(), {k: p.grad.clone() for k, p in om.named_parameters() if p.grad is not None}


@pytest.fixture(scope="module")
def full_case():
    """The bs = 12 500 x 500 batch of tests/test_gpu_fullsize.py::train_case (same seeds, same target maps) and the FROZEN oracle's pass over
    it; the upstream gradient is the oracle criterion's on the oracle's own output."""
    from oracle import criterion as ocrit
    from oracle import targets as otgt
    from tinyfaces.datasets.synthetic import random_boxes
    from tinyfaces.datasets.templates import load_templates
    torch.set_num_threads(min(64, os.cpu_count() or 8))
    templates = load_templates()
    x = torch.randn(BS, 3, SIDE, SIDE, generator=torch.Generator().manual_seed(0))
    rng = np.random.RandomState(0)
    boxes = [random_boxes(rng) for _ in range(BS)]
    pad = otgt.get_padding(templates, [0, 0, SIDE, SIDE])
    noise = [np.random.RandomState(100 + i).rand(63, 63, 25, b.shape[0]) for i, b in enumerate(boxes)]
    maps = [otgt.get_heatmaps(b.copy(), templates, pad, noise=n) for b, n in zip(boxes, noise)]
    cm = torch.from_numpy(np.ascontiguousarray(np.stack([c.transpose(2, 0, 1) for c, _, _ in maps]))).float()
    rm = torch.from_numpy(np.ascontiguousarray(np.stack([r.transpose(2, 0, 1) for _, r, _ in maps]))).float()
    om = _freeze_oracle(_oracle())
    sd0 = {k: v.clone() for k, v in om.state_dict().items()}
    with torch.no_grad():
        y0 = om(x)
    np.random.seed(11)
    gy = ocrit.criterion(y0, cm, rm)["grad"]
    y, grads = _oracle_pass(om, x, gy)
    return dict(om=om, sd0=sd0, x=x, gy=gy, y=y, grads=grads)


def _compare_pass(m, case, dtype, name, n_tensors):
    """Frozen forward + backward of the product against the oracle's; returns (map error, cosines, relative errors)."""
    m = m.cuda().set_compute_dtype(dtype).freeze_batchnorm().train()
    before = _bn_snapshot(m)
    y = m(case["x"].cuda())
    assert y.grad_fn is not None
    dy = err(y.detach().cpu().numpy(), case["y"].numpy())
    y.backward(case["gy"].cuda())
    params = dict(m.named_parameters())
    rel, cos = {}, {}
    for k, go in case["grads"].items():
        if k.startswith("score4_upsample"):
            continue                                              # lr 0 (model.py:84): defined as zero
        a = params[k].grad.cpu()
        rel[k] = float((a - go).abs().max() / (go.abs().max() + 1e-30))
        cos[k] = _cos(a, go)
    up = params["score4_upsample.weight"].grad
    assert up is not None and float(up.abs().max()) == 0.0
    bn_names = m._bn_param_names
    assert len(bn_names) == 2 * (n_tensors - 4)                    # one BatchNorm behind every conv of the trunk
    assert all(params[k].grad is None for k in bn_names), [k for k in bn_names if params[k].grad is not None][:3]
    after = _bn_snapshot(m)
    assert all(torch.equal(before[k], after[k]) for k in before)
    relv, cosv = np.array(list(rel.values())), np.array(list(cos.values()))
    worst = min(cos, key=cos.get)
    report(name, y_maxabs=dy[0], y_maxref=dy[1], tensors=len(rel), grad_rel_med=float(np.median(relv)), grad_rel_p90=float(np.quantile(relv, .9)),
           grad_rel_max=float(relv.max()), cos_min=float(cosv.min()), cos_p05=float(np.quantile(cosv, .05)), cos_med=float(np.median(cosv)), worst=worst)
    print(name, "y_maxabs", dy[0], "cos_min", cosv.min(), "cos_p05", np.quantile(cosv, .05), "cos_med", np.median(cosv), "rel_med", np.median(relv), worst)
    assert len(rel) == n_tensors, len(rel)
    return dy, cosv, relv, worst, cos


def _assert_fp32(dy, cosv, relv, worst, cos):
    assert dy[0] < 1e-3                                            # north_star: per-anchor cls / reg maps within 1e-3 in fp32
    assert cosv.min() > 0.9999 and np.median(relv) < 5e-3, (worst, cos[worst])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_frozen_step_bs12_500x500_vs_oracle(full_case, dtype):
    """ResNet-101, 12 x 3 x 500 x 500: maps and all 98 gradient tensors (94 conv weights, 2 head weights, 2 head biases)."""
    m = _product(full_case["om"])
    m.load_state_dict(full_case["sd0"], strict=True)
    dy, cosv, relv, worst, cos = _compare_pass(m, full_case, dtype, f"frozen_fullsize[{dtype}]", 98)
    if dtype == torch.float32:
        _assert_fp32(dy, cosv, relv, worst, cos)
    else:
        assert dy[0] < 1.8e-2
        assert cosv.min() >= 0.90, (worst, cos[worst])            # EVERY tensor (no layer-1 BN exception: BN vectors have no gradient here)
        assert np.quantile(cosv, .05) > 0.93 and np.median(cosv) > 0.96, (float(np.quantile(cosv, .05)), float(np.median(cosv)))


@pytest.mark.parametrize("trunk,shape,n_tensors", [("resnet101", ODD, 98), ("resnet50", (2, 160, 192), 47), ("resnet152", (2, 160, 192), 149)])
def test_frozen_step_fp32_odd_and_other_trunks_vs_oracle(trunk, shape, n_tensors):
    """The same fp32 assertions at an odd size (every stride-2 stage rounds up, partial tiles everywhere) and, at a small size, for the
    ResNet-50 / ResNet-152 trunks against the oracle of the same depth.  Upstream gradient: seeded normal values of the size of a
    criterion gradient (the backward pass is linear in it)."""
    om = _oracle(trunk, seed=3)
    x = torch.randn(shape[0], 3, shape[1], shape[2], generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        y0 = _freeze_oracle(om)(x)
    gy = 1e-2 * torch.randn(y0.shape, generator=torch.Generator().manual_seed(6))
    y, grads = _oracle_pass(om, x, gy)
    case = dict(x=x, gy=gy, y=y, grads=grads)
    _assert_fp32(*_compare_pass(_product(om, trunk), case, torch.float32, f"frozen_small[{trunk},{shape}]", n_tensors))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(BS, SIDE, SIDE), ODD])
def test_frozen_training_forward_is_the_eval_forward(dtype, shape):
    """What is fine-tuned is what is deployed: the frozen-mode training forward equals model.eval()'s forward bit for bit, with and
    without gradients enabled, and writes nothing."""
    m = _product(_oracle(seed=2)).cuda().set_compute_dtype(dtype)
    x = torch.randn(shape[0], 3, shape[1], shape[2], generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        ref = m.eval()(x).clone()
    before = _bn_snapshot(m)
    m.freeze_batchnorm().train()
    y = m(x)
    assert y.grad_fn is not None and torch.equal(y.detach(), ref)
    with torch.no_grad():
        y2 = m(x)
    assert y2.grad_fn is None and torch.equal(y2, ref)
    m.eval()
    y3 = m(x)
    assert y3.grad_fn is None and torch.equal(y3, ref)             # eval(): today's path
    after = _bn_snapshot(m)
    assert all(torch.equal(before[k], after[k]) for k in before)


def _golden_batches(golden, dtype_cm=np.float32):
    g = golden("trainer")
    return [(torch.from_numpy(g[f"b{i}_img"]), torch.from_numpy(g[f"b{i}_cm"].astype(dtype_cm)), torch.from_numpy(g[f"b{i}_rm"]).float())
            for i in range(2)]


def _fresh(om, keep, dtype=torch.float32, frozen=True):
    from tinyfaces.models.loss import DetectionCriterion
    m = _product(om).set_compute_dtype(dtype).freeze_batchnorm(frozen)
    c = DetectionCriterion(25)
    c.inject_sampling(keep, keep)
    return m, c


def _keep():
    keep = torch.ones(2, 25 * 16 * 16, dtype=torch.uint8)          # deterministic sampling: the first 128 of each kind
    keep[:, 128:] = 0
    return keep


def test_bn_tensors_are_never_written_and_unfreezing_restores_the_statistics_step(golden):
    """3 steps through trainer.train + torch.optim.SGD(weight_decay) and 3 TrainEngine steps: every BN weight, bias, running_mean,
    running_var, num_batches_tracked unchanged (weight decay included), BN .grad None on the autograd path, conv weights did move; with
    the mode off again the batch-statistics step runs as before (running means move, counters count)."""
    from tinyfaces import trainer
    from tinyfaces.engine import TrainEngine
    batches = _golden_batches(golden)
    three = [batches[0], batches[1], batches[0]]
    om = _oracle(seed=4)
    # autograd path
    m, c = _fresh(om, _keep())
    opt = torch.optim.SGD(m.learnable_parameters(1e-3), lr=1e-3, momentum=0.9, weight_decay=5e-4)
    m = m.cuda()
    before, w0 = _bn_snapshot(m), m.model.layer3[5].conv2.weight.detach().clone()
    assert len(before) == 5 * 94                                    # stem + 30 x 3 + 3 downsample BatchNorms
    with redirect_stdout(io.StringIO()):
        trainer.train(m, c, opt, three, 0, torch.device("cuda"))
    after = _bn_snapshot(m)
    assert m.training and m.batchnorm_frozen
    assert all(torch.equal(before[k], after[k]) for k in before), [k for k in before if not torch.equal(before[k], after[k])][:5]
    params = dict(m.named_parameters())
    assert all(params[k].grad is None for k in m._bn_param_names)
    assert params["model.conv1.weight"].grad is not None and not torch.equal(w0, m.model.layer3[5].conv2.weight.detach())
    # fused engine
    m2, c2 = _fresh(om, _keep())
    eng = TrainEngine(m2, c2, lr=1e-3, momentum=0.9, weight_decay=5e-4, device="cuda")
    before2, w2 = _bn_snapshot(m2), m2.model.layer3[5].conv2.weight.detach().clone()
    for img, cm, rm in three:
        eng.step(img.cuda(), cm.cuda(), rm.cuda())
    torch.cuda.synchronize()
    after2 = _bn_snapshot(m2)
    assert all(torch.equal(before2[k], after2[k]) for k in before2), [k for k in before2 if not torch.equal(before2[k], after2[k])][:5]
    assert not torch.equal(w2, m2.model.layer3[5].conv2.weight.detach())
    seg = m2._segments
    for k in m2._bn_param_names:                                    # no momentum either
        o, n = seg[k]
        assert float(eng.flat_m[o:o + n].abs().max()) == 0.0, k
    osd = eng.optimizer_state_dict()
    assert len([i for g in osd["param_groups"] for i in g["params"]]) == len(list(m2.parameters()))      # torch.optim.SGD's numbering
    # frozen off again: the batch-statistics step as before
    m2.freeze_batchnorm(False)
    eng.step(three[0][0].cuda(), three[0][1].cuda(), three[0][2].cuda())
    torch.cuda.synchronize()
    after3 = _bn_snapshot(m2)
    assert int(after3["model.bn1.num_batches_tracked"]) == int(before2["model.bn1.num_batches_tracked"]) + 1
    assert not torch.equal(after3["model.layer2.1.bn2.running_mean"], before2["model.layer2.1.bn2.running_mean"])
    assert not torch.equal(after3["model.layer2.1.bn2.weight"], before2["model.layer2.1.bn2.weight"])
    eng.close()


@pytest.mark.parametrize("trunk", ["resnet101", "resnet50"])
def test_frozen_step_zeroes_the_bn_slices_a_statistics_step_left_in_the_flat_gradient(trunk):
    """The split memset skips [layer3.1.conv1.weight, score_res3.weight) of the persistent flat gradient on the promise that everything in
    it is overwritten; the BN segments in it have no writer in frozen mode.  After a batch-statistics step (which fills them) a frozen step
    must leave every BN slice of the flat gradient zero, and the engine must not move the BN vectors."""
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.loss import DetectionCriterion
    om = _oracle(trunk, seed=6)
    m = _product(om, trunk).set_compute_dtype(torch.bfloat16)       # bf16: the grouped layer-3 weight gradients, i.e. the split memset
    c = DetectionCriterion(25)
    eng = TrainEngine(m, c, lr=1e-3, momentum=0.0, weight_decay=5e-4, device="cuda")
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 256, 256, generator=g).cuda()
    cm = torch.where(torch.rand(2, 25, 32, 32, generator=g) < 0.02, 1.0, -1.0).cuda()
    rm = torch.randn(2, 100, 32, 32, generator=g).cuda()
    eng.step(x, cm.clone(), rm)                                     # batch statistics: BN gradients land in the flat buffer
    torch.cuda.synchronize()
    gflat, seg = m._grad_flat_persistent, m._segments
    inside = [k for k in m._bn_param_names if k.startswith("model.layer3.") and not k.startswith("model.layer3.0.")]
    assert inside and max(float(gflat[seg[k][0]:seg[k][0] + seg[k][1]].abs().max()) for k in inside) > 0.0
    m.freeze_batchnorm()
    before = _bn_snapshot(m)
    eng.step(x, cm.clone(), rm)
    torch.cuda.synchronize()
    dirty = [k for k in m._bn_param_names if float(gflat[seg[k][0]:seg[k][0] + seg[k][1]].abs().max()) != 0.0]
    assert not dirty, dirty[:5]
    after = _bn_snapshot(m)
    assert all(torch.equal(before[k], after[k]) for k in before)
    assert float(gflat[seg["model.layer3.4.conv2.weight"][0]:][:1000].abs().max()) > 0.0
    eng.close()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_frozen_dual_stream_backward_equals_single_stream(dtype):
    """Race screen of the frozen backward's own forks (as test_dual_stream_backward_equals_single_stream for the training graph): the
    weight-gradient stream must produce the single-stream gradients; only fp32-atomic summation order may differ."""
    m = _product(_oracle(seed=7)).cuda().set_compute_dtype(dtype).freeze_batchnorm().train()
    x = torch.randn(3, 3, 224, 288, generator=torch.Generator().manual_seed(7)).cuda()

    def grads(dual):
        m.single_stream = not dual
        m.zero_grad(set_to_none=True)
        y = m(x)
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(9)).cuda()
        y.backward(gy)
        torch.cuda.synchronize()
        return {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    try:
        ref = grads(False)
        worst = 0.0
        for rep in range(4):
            got = grads(True)
            assert set(got) == set(ref)
            for k in ref:
                worst = max(worst, float((got[k] - ref[k]).abs().max() / (ref[k].abs().max() + 1e-30)))
    finally:
        m.single_stream = False
    report(f"frozen_dual_stream[{dtype}]", worst_rel=worst)
    assert worst < 1e-4


def test_frozen_grad_ready_events_are_recorded_in_backward_order():
    """The frozen backward's gradient-ready hooks (test_grad_ready_events_are_recorded_in_backward_order's method): events complete in
    backward order, and once the last (-1) has, the gradients equal those of a run without events."""
    import ctypes as C
    m = _product(_oracle(seed=8)).cuda().set_compute_dtype(torch.bfloat16).freeze_batchnorm().train()
    x = torch.randn(2, 3, 160, 192, generator=torch.Generator().manual_seed(11)).cuda()

    def grads():
        m.zero_grad(set_to_none=True)
        y = m(x)
        y.backward(torch.ones_like(y))
        return y

    blocks_py = [22, 14, 7, -1]
    evs = [torch.cuda.Event(enable_timing=True) for _ in blocks_py]
    for e in evs:
        e.record()
    torch.cuda.synchronize()
    blocks = (C.c_int * 4)(*blocks_py)
    handles = (C.c_void_p * 4)(*[int(e.cuda_event) for e in evs])
    try:
        m._grad_events = (blocks, handles, 4)
        t0 = torch.cuda.Event(enable_timing=True)
        t0.record()
        grads()
        evs[-1].synchronize()
        got = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
        times = [t0.elapsed_time(e) for e in evs]
        m._grad_events = None
        grads()
        torch.cuda.synchronize()
    finally:
        m._grad_events = None
    assert all(t > 0 for t in times) and times == sorted(times), times
    worst = max(float((got[k] - p.grad).abs().max() / (p.grad.abs().max() + 1e-30)) for k, p in m.named_parameters() if p.grad is not None)
    report("frozen_grad_events", times_ms=[round(t, 3) for t in times], worst_rel=worst)
    assert worst < 1e-3


def test_frozen_two_rank_engine_equals_single_process_on_the_summed_micro_batches(tmp_path):
    """2 gloo ranks sharing cuda:0 with freeze_batchnorm() (tests/dist_worker_frozen.py) against ONE process that sums the gradients of the
    same two micro-batches and takes the segment-aware step."""
    from tinyfaces import ops
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dist_worker_frozen
    golden = os.path.join(ROOT, "tests", "golden", "trainer.npz")
    out = str(tmp_path / "rank0.npz")
    steps = 3
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29573", os.path.join(ROOT, "tests", "dist_worker_frozen.py"), golden, out, str(steps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.load(out)
    assert int(got["buckets"]) >= 2
    dist = [got[f"arr_{i}"] for i in range(steps)]
    reps = []
    for r_ in range(2):
        m, c, batches = dist_worker_frozen.build(golden)
        m = m.cuda().train()
        flat = m.flatten_parameters()
        reps.append(dict(m=m, c=c, flat=flat, mom=torch.zeros_like(flat), batch=[t.cuda() for t in batches[r_]]))
    m0 = reps[0]["m"]
    groups = m0.group_ranges()
    trained = sorted((o, o + n) for k, (o, n) in m0._segments.items() if k not in m0._bn_param_names)
    first = reps[0]["flat"].cpu().numpy().copy()
    worst = []
    for s in range(steps):
        grads = []
        for rp in reps:
            m, c = rp["m"], rp["c"]
            img, cm, rm = rp["batch"]
            m._sync_tables(img.device)
            o = m._run_forward(img, training=True)
            _, g, _ = ops.criterion_fwd_bwd(o, cm.clone(), rm, c.n_templates, c.reg_weight, c.ohem_thresh, c.max_pos, c.max_neg,
                                            c._pos_keep, c._neg_keep, c._next_seed())
            grads.append(m._run_backward(img, g, persistent=True).clone())
        gsum = grads[0] + grads[1]
        for rp in reps:
            for a, b, mult in groups:
                if mult != 0.0:
                    segs = [(max(s_, a), min(e_, b)) for s_, e_ in trained if e_ > a and s_ < b]
                    ops.sgd_step_segments(rp["flat"], gsum, rp["mom"], segs, 1e-4 * mult, 0.9, 5e-4, 0.5)
        torch.cuda.synchronize()
        ref = reps[0]["flat"].cpu().numpy()
        worst.append(float(np.abs(dist[s] - ref).max() / (np.abs(ref).max() + 1e-30)))
    report("frozen_dist_2_ranks_vs_single[resnet50]", worst_rel=str([f"{w:.2e}" for w in worst]))
    assert all(np.isfinite(d).all() for d in dist) and all(np.isfinite(w) for w in worst), worst
    assert float(np.abs(dist[-1] - first).max()) > 0.0                 # the ranks did train
    seg = m0._segments
    for k in m0._bn_param_names:                                       # ... and left every BN vector alone
        o, n = seg[k]
        assert np.array_equal(dist[-1][o:o + n], first[o:o + n]), k
    assert worst[0] < 1e-5, worst
    assert worst[-1] < 1e-2, worst


def test_frozen_optimisation_loop_vs_oracle_and_engine_vs_trainer(golden, monkeypatch):
    """fp32, the two batches of tests/golden/trainer.npz, deterministic sampling (the first 128 of each kind), lr 1e-3, momentum 0.9,
    weight decay 5e-4.  (a) two trainer.train steps against two steps of torch.optim.SGD on the CPU oracle with its BN in eval(): within
    2e-2 relative-to-max (the bar of test_trainer_two_steps_vs_reference_golden); (b) TrainEngine against trainer.train + torch.optim.SGD:
    2e-3 after one step, 1e-1 after two (the bars of test_fused_engine_equals_autograd_trainer for the default statistics mode)."""
    from oracle import criterion as ocrit
    from tinyfaces import trainer
    from tinyfaces.engine import TrainEngine
    batches = _golden_batches(golden)
    keep = _keep()

    def first128(label_cls, pos_fraction=0.5, sample_size=256, rng=None, record=None):
        flat = label_cls.reshape(-1)
        pos = np.flatnonzero(flat == 1)
        flat[pos[128:]] = 0
        neg = np.flatnonzero(flat == -1)
        flat[neg[128:]] = 0
        return label_cls
    monkeypatch.setattr(ocrit, "balance_sampling", first128)          # the oracle criterion with the same deterministic rule

    def worst_diff(a, b):
        w, name = 0.0, ""
        for k in a:
            if a[k].is_floating_point():
                d = err(b[k].cpu().numpy(), a[k].cpu().numpy())[2]
                if d > w:
                    w, name = d, k
        return w, name

    # (a) reference: the oracle on the CPU
    torch.set_num_threads(min(64, os.cpu_count() or 8))
    om = _freeze_oracle(_oracle(seed=9))
    sd0 = {k: v.clone() for k, v in om.state_dict().items()}
    oopt = torch.optim.SGD(om.learnable_parameters(1e-3), lr=1e-3, momentum=0.9, weight_decay=5e-4)
    for img, cm, rm in batches:
        out = om(img)
        gy = ocrit.criterion(out.detach(), cm, rm)["grad"]
        oopt.zero_grad()
        out.backward(gy)
        oopt.step()
    ref_sd = om.state_dict()
    om0 = _oracle(seed=9)
    om0.load_state_dict(sd0)
    res = {}
    for nsteps in (1, 2):
        m1, c1 = _fresh(om0, keep)
        opt = torch.optim.SGD(m1.learnable_parameters(1e-3), lr=1e-3, momentum=0.9, weight_decay=5e-4)
        with redirect_stdout(io.StringIO()):
            trainer.train(m1, c1, opt, batches[:nsteps], 0, torch.device("cuda"))
        m2, c2 = _fresh(om0, keep)
        eng = TrainEngine(m2, c2, lr=1e-3, momentum=0.9, weight_decay=5e-4, device="cuda")
        for img, cm, rm in batches[:nsteps]:
            eng.step(img.cuda(), cm.cuda(), rm.cuda())
        torch.cuda.synchronize()
        res[nsteps] = worst_diff(m1.state_dict(), m2.state_dict())
        assert list(m2.state_dict().keys()) == list(m1.state_dict().keys())
        eng.close()
        if nsteps == 2:
            vs_oracle = worst_diff(ref_sd, m1.state_dict())
            moved = worst_diff(sd0, m1.state_dict())
    report("frozen_loop", trainer_vs_oracle_2steps=vs_oracle[0], tensor=vs_oracle[1], moved=moved[0], engine_step1=res[1][0], engine_step1_tensor=res[1][1],
           engine_step2=res[2][0], engine_step2_tensor=res[2][1])
    print("frozen_loop", vs_oracle, moved, res)
    assert moved[0] > 1e-4                                             # the two steps did move the weights
    assert vs_oracle[0] < 2e-2, vs_oracle
    assert res[1][0] < 2e-3, res[1]
    assert res[2][0] < 1e-1, res[2]


_SPLIT_MEMSET_SCRIPT = r'''
import os, sys
import numpy as np
import torch
for p in (ROOT, os.path.join(ROOT, "tiny-faces-pytorch_amd")):
    sys.path.insert(0, p)
from tinyfaces.engine import TrainEngine
from tinyfaces.models import model as mm
from tinyfaces.models.loss import DetectionCriterion
trunk = sys.argv[2]
torch.manual_seed(0)
m = mm.DetectionModel(base_model=getattr(mm, trunk), num_templates=25).set_compute_dtype(torch.bfloat16).freeze_batchnorm()
with torch.no_grad():                                   # tamed initialisation: a random 101- / 152-layer trunk overflows otherwise
    for k, p in m.named_parameters():
        if k.endswith("bn3.weight"):
            p.fill_(0.1)
    m.score_res3.weight.mul_(0.05)
    m.score_res4.weight.mul_(0.05)
eng = TrainEngine(m, DetectionCriterion(25), lr=0.0, momentum=0.0, weight_decay=0.0, device="cuda")
g = torch.Generator().manual_seed(3)
x = torch.randn(2, 3, 256, 256, generator=g).cuda()
cm = torch.where(torch.rand(2, 25, 32, 32, generator=g) < 0.02, 1.0, -1.0).cuda()
rm = torch.randn(2, 100, 32, 32, generator=g).cuda()
m._grad_flat_persistent.fill_(7.0)                     # what an earlier step left behind
eng.step(x, cm, rm)
torch.cuda.synchronize()
gf = m._grad_flat_persistent.cpu().numpy()
names = list(m._segments)
np.savez(sys.argv[1], g=gf, names=np.array(names), off=np.array([m._segments[k][0] for k in names]), num=np.array([m._segments[k][1] for k in names]),
         bn=np.array(sorted(m._bn_param_names)))
'''


@pytest.mark.parametrize("trunk", ["resnet50", "resnet101", "resnet152"])
def test_frozen_split_memset_is_taken_and_its_bn_slices_are_zeroed_by_the_range_kernel(tmp_path, trunk):
    """Which path the frozen backward takes cannot be seen in its results, so this test removes the weight gradients
    (TINYFACES_DBG_SKIP_WGRAD, read once per process: a subprocess) over a flat gradient full of a sentinel.  With the split memset taken, the
    conv weights of layer 3's identity bottlenecks keep the sentinel (the memset skipped them, their only writer is switched off), every
    tensor outside the range is zero (memset), and every BatchNorm slice INSIDE the range is zero too -- which only zero_ranges_kernel can
    have done.  A full memset (the fall-back when the table of ranges does not fit) would leave no sentinel at all.  All three trunks:
    66 / 15 / 105 merged ranges for ResNet-101 / -50 / -152."""
    out = str(tmp_path / f"split_{trunk}.npz")
    env = dict(os.environ, TINYFACES_DBG_SKIP_WGRAD="1")
    env.pop("TINYFACES_GRAD_MEMSET_FULL", None)
    r = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + _SPLIT_MEMSET_SCRIPT, out, trunk], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(out)
    g, bn = z["g"], set(str(k) for k in z["bn"])
    kept, bn_inside = 0, 0
    for k, o, n in zip((str(k) for k in z["names"]), z["off"], z["num"]):
        v = g[o:o + n]
        identity_l3 = k.startswith("model.layer3.") and not k.startswith("model.layer3.0.")
        if k in bn:
            assert not v.any(), k                                        # no BN slice carries anything, inside the range or outside
            bn_inside += identity_l3
        elif identity_l3 and k.endswith(".weight"):
            assert (v == 7.0).all(), k                                   # skipped by the memset: the split path was taken
            kept += 1
        elif (k.startswith("score_res") and k.endswith(".bias")) or k == "model.conv1.weight":
            assert np.isfinite(v).all() and not (v == 7.0).any(), k      # written all the same: the head's column sums, the stem's direct weight gradient
        else:
            assert not v.any(), k                                        # outside the range: memset (weight gradients are switched off)
    blocks = {"resnet50": 6, "resnet101": 23, "resnet152": 36}[trunk]
    assert kept == 3 * (blocks - 1) and bn_inside == 6 * (blocks - 1), (kept, bn_inside)


def test_sgd_step_segments_equals_a_torch_reference_on_every_path():
    """tf_sgd_step_segments against the same update written in torch, on the paths the training loop does not reach: 4-aligned ranges
    (float4 path), unaligned starts / lengths (scalar path), empty ranges, one-element ranges, more than TF_SGD_MAX_SEGMENTS = 128 ranges
    (two launches), a second step (momentum), and untouched elements outside the ranges bit for bit."""
    from tinyfaces import ops
    g = torch.Generator().manual_seed(0)
    n = 40000
    lr, mu, wd, gs = 0.05, 0.9, 5e-4, 0.5

    def check(segs, name):
        p = torch.randn(n, generator=g).cuda()
        gr = torch.randn(n, generator=g).cuda()
        m = torch.zeros(n).cuda()
        rp, rm_ = p.clone(), m.clone()
        worst = 0.0
        for step in range(2):
            ops.sgd_step_segments(p, gr, m, segs, lr, mu, wd, gs)
            mask = torch.zeros(n, dtype=torch.bool, device="cuda")
            for a, b in segs:
                mask[a:b] = True
            d = gr * gs + wd * rp
            new_m = mu * rm_ + d
            rm_ = torch.where(mask, new_m, rm_)
            rp = torch.where(mask, rp - lr * new_m, rp)
            torch.cuda.synchronize()
            assert torch.equal(p[~mask], rp[~mask]) and torch.equal(m[~mask], rm_[~mask]), name       # outside: untouched
            worst = max(worst, float((p - rp).abs().max()), float((m - rm_).abs().max()))
        report(f"sgd_segments[{name}]", segments=len(segs), worst_abs=worst)
        assert worst < 1e-6, (name, worst)            # values of order 1 in fp32: one rounding of an fma contraction apart at most

    check([(0, 64), (128, 4096), (8192, 8196), (20000, 39996)], "aligned")
    check([(3, 10), (10, 10), (17, 18), (101, 4099), (9001, 9002), (20001, 39999)], "unaligned_empty_single")
    many = [(100 * i, 100 * i + 4 * (1 + i % 20)) for i in range(300)]                          # 300 ranges: three launches, 4-aligned
    check(many, "300_aligned")
    check([(100 * i + 1, 100 * i + 3 + i % 50) for i in range(300)], "300_unaligned")
    check([(0, n)], "whole")
