"""-m gpu: fine-tuning with the lower trunk stages frozen (DetectionModel.set_trainable_layers on top of freeze_batchnorm; the frozen-BN backward
cut at a stage boundary, tf_detnet_trunk_backward_frozen_from_ctx in csrc/detnet.hip).

Reference = the CPU oracle of tests/test_gpu_frozen_bn.py (every BatchNorm2d in eval(), its parameters without a gradient) with, in addition,
requires_grad_(False) on every parameter of the frozen stages.  The bars are the existing ones for the same quantities: fp32 maps within 1e-3,
every gradient tensor cosine > 0.9999 and median relative error < 5e-3 (_assert_fp32); cut against full graph within what fp32-atomic summation
order allows, 1e-4 (test_frozen_dual_stream_backward_equals_single_stream); hooks 1e-3 (test_frozen_grad_ready_events_are_recorded_in_backward_order);
engine against trainer 2e-3 after one step, 1e-1 after two (test_frozen_optimisation_loop_vs_oracle_and_engine_vs_trainer); two ranks 1e-5 after the
first step, 1e-2 after the last.  Measured values go through gpu_util.report.

NOT YET RUN on an MI355X: no GPU could be had while these tests were written; the oracle side of the first test (shapes, tensor counts) was
checked on the CPU.  The first GPU run is to commit the report as profiles/trainable_layers_parity.txt, beside profiles/frozen_bn_parity.txt."""
import ctypes as C
import io
import os
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest
import torch

from gpu_util import err, report
from redzone import assert_guards, assert_written, guarded, guarded_workspace, unwritten
from test_gpu_frozen_bn import ODD, _assert_fp32, _bn_snapshot, _cos, _golden_batches, _keep, _oracle, _oracle_pass, _product

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tensors that receive a gradient with BatchNorm frozen, for k = 4, 3, 2, 1, 0
COUNTS = {"resnet50": (47, 46, 36, 23, 4), "resnet101": (98, 97, 87, 74, 4), "resnet152": (149, 148, 138, 113, 4)}
STAGES = ("model.layer3.", "model.layer2.", "model.layer1.", ("model.conv1.", "model.bn1."))      # from the top; the stem is conv1 + bn1
UPSAMPLE = "score4_upsample.weight"
HEADS = ["score_res3.weight", "score_res3.bias", "score_res4.weight", "score_res4.bias"]


def _frozen_prefixes(k):
    out = []
    for s in STAGES[k:]:
        out += list(s) if isinstance(s, tuple) else [s]
    return tuple(out)


_ORACLE_INPUTS = {}


def _oracle_inputs(trunk, shape):
    """One oracle, one input and one upstream gradient per (trunk, shape), shared by the cuts (the inputs of
    test_frozen_step_fp32_odd_and_other_trunks_vs_oracle: same seeds)."""
    if (trunk, shape) not in _ORACLE_INPUTS:
        om = _oracle(trunk, seed=3)
        x = torch.randn(shape[0], 3, shape[1], shape[2], generator=torch.Generator().manual_seed(5))
        H3, W3 = -(-shape[1] // 8), -(-shape[2] // 8)
        gy = 1e-2 * torch.randn(shape[0], 125, H3, W3, generator=torch.Generator().manual_seed(6))
        _ORACLE_INPUTS[(trunk, shape)] = (om, {n: v.clone() for n, v in om.state_dict().items()}, x, gy)
    return _ORACLE_INPUTS[(trunk, shape)]


@pytest.mark.parametrize("trunk,shape,k", [("resnet50", (2, 160, 192), k) for k in (0, 1, 2, 3)] + [("resnet101", ODD, 2), ("resnet101", ODD, 1)])
def test_partial_freeze_step_fp32_vs_oracle(trunk, shape, k):
    """The output map and every trained tensor's gradient against autograd on the oracle with its BatchNorm in eval() and the frozen stages'
    parameters requires_grad_(False); everything else has no gradient (score4_upsample.weight: exactly zero), no BN tensor is written.  At the
    odd size every stride-2 stage rounds up and the cut sits on a stride-2 downsample block."""
    om, sd0, x, gy = _oracle_inputs(trunk, shape)
    for p in om.parameters():
        p.requires_grad_(True)
    frozen = _frozen_prefixes(k)
    for n, p in om.named_parameters():
        if n.startswith(frozen):
            p.requires_grad_(False)
    y_ref, g_ref = _oracle_pass(om, x, gy)                    # (_freeze_oracle inside: BN in eval(), its parameters without a gradient)
    assert tuple(y_ref.shape) == tuple(gy.shape)
    g_ref.pop(UPSAMPLE, None)                                  # lr 0 (model.py:84): defined as zero
    want = COUNTS[trunk][4 - k]
    assert len(g_ref) == want, (len(g_ref), want)             # the oracle itself trains exactly the table's tensors

    m = _product(om, trunk)
    m.load_state_dict(sd0, strict=True)
    m = m.cuda().set_compute_dtype(torch.float32).set_trainable_layers(k).freeze_batchnorm().train()
    assert m.trainable_parameter_names() == [n for n in m.trainable_parameter_names() if n in g_ref] and len(m.trainable_parameter_names()) == want
    before = _bn_snapshot(m)
    y = m(x.cuda())
    assert y.grad_fn is not None
    dy = err(y.detach().cpu().numpy(), y_ref.numpy())
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    params = dict(m.named_parameters())
    rel, cos = {}, {}
    for n, go in g_ref.items():
        assert params[n].grad is not None, n
        a = params[n].grad.cpu()
        rel[n] = float((a - go).abs().max() / (go.abs().max() + 1e-30))
        cos[n] = _cos(a, go)
    up = params[UPSAMPLE].grad
    assert up is not None and float(up.abs().max()) == 0.0
    stray = [n for n, p in params.items() if n not in g_ref and n != UPSAMPLE and p.grad is not None]
    assert not stray, stray[:5]
    after = _bn_snapshot(m)
    assert all(torch.equal(before[n], after[n]) for n in before)
    relv, cosv = np.array(list(rel.values())), np.array(list(cos.values()))
    worst = min(cos, key=cos.get)
    name = f"partial_freeze[{trunk},{shape},k={k}]"
    report(name, y_maxabs=dy[0], y_maxref=dy[1], tensors=len(rel), grad_rel_med=float(np.median(relv)), grad_rel_max=float(relv.max()),
           cos_min=float(cosv.min()), cos_med=float(np.median(cosv)), worst=worst)
    print(name, "y_maxabs", dy[0], "tensors", len(rel), "cos_min", cosv.min(), "rel_med", np.median(relv), "rel_max", relv.max(), worst)
    assert len(rel) == want
    _assert_fp32(dy, cosv, relv, worst, cos)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cut_backward_equals_the_full_graph_on_the_trained_tensors(dtype):
    """Same kernels, fewer launches: for every k < 4 the forward output is the k = 4 output bit for bit and every trained tensor's gradient is the
    one of the k = 4 backward on the same input, up to the summation order of the fp32 atomics."""
    m = _product(_oracle(seed=7)).cuda().set_compute_dtype(dtype).freeze_batchnorm().train()
    x = torch.randn(3, 3, 224, 288, generator=torch.Generator().manual_seed(7)).cuda()

    def run(k):
        m.set_trainable_layers(k)
        m.zero_grad(set_to_none=True)
        y = m(x)
        gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(9)).cuda()
        y.backward(gy)
        torch.cuda.synchronize()
        return y.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    y4, g4 = run(4)
    assert len(g4) == 98 + 1
    for k in (3, 2, 1, 0):
        y, g = run(k)
        assert torch.equal(y, y4), k
        assert set(g) == set(m.trainable_parameter_names()) | {UPSAMPLE} and len(g) == COUNTS["resnet101"][4 - k] + 1, (k, len(g))
        assert all(torch.isfinite(v).all() for v in g.values()), k
        worst = max(float((g[n] - g4[n]).abs().max() / (g4[n].abs().max() + 1e-30)) for n in g if n != UPSAMPLE)
        assert float(g[UPSAMPLE].abs().max()) == 0.0
        report(f"cut_vs_full[{dtype},k={k}]", tensors=len(g) - 1, worst_rel=worst)
        print("cut_vs_full", dtype, k, len(g) - 1, worst)
        assert worst < 1e-4, (k, worst)


@pytest.mark.parametrize("k,blocks_py", [(2, [22, 7, 2, -1]), (0, [22, 14, 7, -1])])
def test_hooks_below_the_cut_fire_at_the_end_of_the_shortened_pass(k, blocks_py):
    """test_frozen_grad_ready_events_are_recorded_in_backward_order's method with a cut: block 2 lies below the k = 2 cut (first trained block 3),
    every block below the k = 0 cut.  An event that never fired keeps its pre-test record and shows as a negative time."""
    m = _product(_oracle(seed=8)).cuda().set_compute_dtype(torch.bfloat16).freeze_batchnorm().set_trainable_layers(k).train()
    x = torch.randn(2, 3, 160, 192, generator=torch.Generator().manual_seed(11)).cuda()

    def grads():
        m.zero_grad(set_to_none=True)
        y = m(x)
        y.backward(torch.ones_like(y))
        return y

    grads()                                                            # (first call: allocations, module load -- not between t0 and the events)
    torch.cuda.synchronize()
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
        assert all(e.query() for e in evs)                             # the -1 event is the last: every other one has completed by now
        got = {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}
        times = [t0.elapsed_time(e) for e in evs]
        m._grad_events = None
        grads()
        torch.cuda.synchronize()
    finally:
        m._grad_events = None
    assert all(t > 0 for t in times) and times == sorted(times), times
    assert len(got) == COUNTS["resnet101"][4 - k] + 1
    worst = max(float((got[n] - p.grad).abs().max() / (p.grad.abs().max() + 1e-30)) for n, p in m.named_parameters()
                if p.grad is not None and n != UPSAMPLE)
    report(f"cut_grad_events[k={k}]", times_ms=[round(t, 3) for t in times], worst_rel=worst)
    assert worst < 1e-3


@pytest.mark.parametrize("trunk", ["resnet50", "resnet101"])
def test_engine_leaves_the_frozen_stages_alone_and_their_gradient_slices_zero(trunk):
    """After a batch-statistics step that fills the whole persistent flat gradient: two steps at k = 2 move neither the parameters nor the momentum
    of any stem / layer-1 tensor or BN vector (weight decay 5e-4, momentum 0.9) and leave their gradient slices exactly zero, while layer 2,
    layer 3 and the heads train; then two steps at k = 0 (one full memset, no split) move the four head tensors only."""
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.loss import DetectionCriterion
    om = _oracle(trunk, seed=6)
    m = _product(om, trunk).set_compute_dtype(torch.bfloat16)
    eng = TrainEngine(m, DetectionCriterion(25), lr=1e-3, momentum=0.9, weight_decay=5e-4, device="cuda")
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 256, 256, generator=g).cuda()
    cm = torch.where(torch.rand(2, 25, 32, 32, generator=g) < 0.02, 1.0, -1.0).cuda()
    rm = torch.randn(2, 100, 32, 32, generator=g).cuda()
    eng.step(x, cm.clone(), rm)                                     # batch statistics: every slice of the flat gradient is filled
    torch.cuda.synchronize()
    gflat, seg = m._grad_flat_persistent, m._segments

    def sl(t, n):
        return t[seg[n][0]:seg[n][0] + seg[n][1]]

    low = [n for n in seg if n.startswith(("model.conv1.", "model.bn1.", "model.layer1."))]
    assert len(low) == 3 + 3 * 10 and min(float(sl(gflat, n).abs().max()) for n in low) > 0.0
    assert min(float(sl(eng.flat_m, n).abs().max()) for n in low) > 0.0

    def two_steps(k):
        m.freeze_batchnorm().set_trainable_layers(k)
        p0, m0 = eng.flat_p.clone(), eng.flat_m.clone()
        bn0 = _bn_snapshot(m)
        for _ in range(2):
            eng.step(x, cm.clone(), rm)
        torch.cuda.synchronize()
        bn1 = _bn_snapshot(m)
        assert all(torch.equal(bn0[n], bn1[n]) for n in bn0)
        trained = set(m.trainable_parameter_names())
        assert len(trained) == COUNTS[trunk][4 - k]
        for n in seg:
            if n in trained:
                continue
            assert torch.equal(sl(eng.flat_p, n), sl(p0, n)) and torch.equal(sl(eng.flat_m, n), sl(m0, n)), (k, n)
            assert float(sl(gflat, n).abs().max()) == 0.0, (k, n)
        moved = [n for n in trained if not torch.equal(sl(eng.flat_p, n), sl(p0, n))]
        assert torch.isfinite(eng.flat_p).all()
        return trained, moved

    trained, moved = two_steps(2)
    assert not [n for n in low + sorted(m._bn_param_names) if n in trained]
    assert set(moved) == trained                                    # every trained tensor trains ...
    for n in ("model.layer2.1.conv2.weight", "model.layer3.4.conv2.weight", "model.layer3.0.downsample.0.weight", "score_res3.weight"):
        assert n in moved, n                                        # ... a layer-2 tensor, layer-3 tensors and a head among them
    trained, moved = two_steps(0)
    assert sorted(trained) == sorted(HEADS) and sorted(moved) == sorted(HEADS)
    eng.close()


def test_engine_equals_trainer_with_frozen_stages(golden):
    """fp32, ResNet-50, k = 2, the first batch of tests/golden/trainer.npz twice, deterministic sampling, lr 1e-3, momentum 0.9, weight decay
    5e-4: the fused TrainEngine against trainer.train + torch.optim.SGD(model.learnable_parameters(lr)) -- 2e-3 after one step, 1e-1 after two
    (the bars of the frozen-BN test this one is modelled on); the tensors of the frozen stages and every BN tensor are the initial ones bit
    for bit on both sides (torch.optim.SGD skips a parameter whose .grad is None: no weight decay either)."""
    from tinyfaces import trainer
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.loss import DetectionCriterion
    batch = _golden_batches(golden)[0]
    om = _oracle("resnet50", seed=9)
    sd0 = {n: v.clone() for n, v in om.state_dict().items()}

    def fresh():
        m = _product(om, "resnet50").set_compute_dtype(torch.float32).freeze_batchnorm().set_trainable_layers(2)
        c = DetectionCriterion(25)
        c.inject_sampling(_keep(), _keep())
        return m, c

    res = {}
    for nsteps in (1, 2):
        m1, c1 = fresh()
        opt = torch.optim.SGD(m1.learnable_parameters(1e-3), lr=1e-3, momentum=0.9, weight_decay=5e-4)
        with redirect_stdout(io.StringIO()):
            trainer.train(m1, c1, opt, [batch] * nsteps, 0, torch.device("cuda"))
        m2, c2 = fresh()
        eng = TrainEngine(m2, c2, lr=1e-3, momentum=0.9, weight_decay=5e-4, device="cuda")
        for img, cm, rm in [batch] * nsteps:
            eng.step(img.cuda(), cm.cuda(), rm.cuda())
        torch.cuda.synchronize()
        eng.close()
        s1, s2 = m1.state_dict(), m2.state_dict()
        assert list(s1) == list(s2)
        trained = set(m2.trainable_parameter_names())
        assert len(trained) == 36
        w, wname, moved = 0.0, "", 0
        for n in s1:
            if n in trained:
                d = err(s2[n].cpu().numpy(), s1[n].cpu().numpy())[2]
                if d > w:
                    w, wname = d, n
                moved += not torch.equal(s1[n].cpu(), sd0[n])
            else:                                                   # frozen stages, BN tensors and buffers, upsample, fc: untouched on both sides
                assert torch.equal(s1[n].cpu(), sd0[n]) and torch.equal(s2[n].cpu(), sd0[n]), (nsteps, n)
        assert moved == len(trained)
        assert all(p.grad is None for n, p in m1.named_parameters() if n not in trained and n != UPSAMPLE)
        res[nsteps] = (w, wname)
    report("partial_freeze_loop[resnet50,k=2]", engine_step1=res[1][0], engine_step1_tensor=res[1][1], engine_step2=res[2][0], engine_step2_tensor=res[2][1])
    print("partial_freeze_loop", res)
    assert res[1][0] < 2e-3, res[1]
    assert res[2][0] < 1e-1, res[2]


def test_cut_entry_point_writes_the_trained_slots_only(hip):
    """The write contract of tf_detnet_trunk_backward_frozen_from_ctx, one call at k = 2 (ResNet-50, fp32, 1 x 96 x 128): the arena is a guarded view
    of exactly tf_detnet_trunk_workspace_bytes(..., 2) bytes, the gradient table points into a guard-banded, NaN-filled buffer that grad_flat does
    not cover (no memset on its behalf).  Guards intact; every trained slot (and the zero gradient of score4_upsample.weight) fully written;
    the slots of the stem, of layer 1 and of every BN vector still hold the fill."""
    from tinyfaces.models import model as mm
    from tinyfaces._hip import ptr, stream
    lib = hip.lib()
    m = _product(_oracle("resnet50", seed=5), "resnet50").cuda().set_compute_dtype(torch.float32).freeze_batchnorm().set_trainable_layers(2).train()
    x = torch.randn(1, 3, 96, 128, generator=torch.Generator().manual_seed(2)).cuda()
    N, _, H, W = x.shape
    tr = mm._trunk_arg(m.trunk)
    nbytes = lib.tf_detnet_trunk_workspace_bytes(tr, m.compute_dtype, N, H, W, m.num_out, hip.TF_DETNET_FROZEN_BN)
    ws = guarded_workspace(nbytes, x.device, pitch_bytes=4096)
    m._sync_tables(x.device)
    m._ws = ws
    try:
        y = m._run_forward(x, training=True)
        assert m._ws is ws and m._ws_mode == hip.TF_DETNET_FROZEN_BN
        gy = (0.1 * torch.randn(y.shape, generator=torch.Generator().manual_seed(3))).cuda()
        offs, o = {}, 0
        for n, num in zip(m._grad_names, m._grad_numels):
            offs[n] = (o, num)
            o += (num + 3) // 4 * 4
        gbuf = guarded((o,), torch.float32, x.device)
        table = (C.c_void_p * len(m._names))(*[gbuf.data_ptr() + 4 * offs[n][0] if n in offs else 0 for n in m._names])
        rc = lib.tf_detnet_trunk_backward_frozen_from_ctx(tr, m._ctx(x.device), None, m.compute_dtype, ptr(x), N, H, W, m.num_out, m._param_ptrs, table,
                                                          ptr(gy), None, 0, ptr(ws), ws.numel(), stream(), m._first_block(2))
        torch.cuda.synchronize()
    finally:
        m._ws = None
    assert rc == 0, rc
    assert_guards(ws, f"arena of exactly {nbytes} bytes")
    assert_guards(gbuf, "gradient table")
    trained = set(m.trainable_parameter_names())
    assert len(trained) == 36
    for n, (a, num) in offs.items():
        if n in trained or n == UPSAMPLE:
            assert_written(gbuf, slice(a, a + num), n)
            assert torch.isfinite(gbuf[a:a + num]).all(), n
        else:
            assert unwritten(gbuf, slice(a, a + num))[0] == num, n          # stem, layer 1, BN vectors: no writer
    assert float(gbuf[offs[UPSAMPLE][0]:][:offs[UPSAMPLE][1]].abs().max()) == 0.0
    assert float(gbuf[offs["model.layer2.0.conv1.weight"][0]:][:offs["model.layer2.0.conv1.weight"][1]].abs().max()) > 0.0


def test_partial_freeze_without_frozen_batchnorm_is_refused_before_anything_runs():
    m = _product(_oracle("resnet50", seed=2), "resnet50").cuda().set_compute_dtype(torch.bfloat16)
    x = torch.randn(2, 3, 96, 128, generator=torch.Generator().manual_seed(1)).cuda()
    with torch.no_grad():
        ref_eval = m.eval()(x).clone()
    before = _bn_snapshot(m)
    from tinyfaces import _hip
    prev = _hip.lib().tf_get_stat_rows()
    try:
        _hip.lib().tf_set_stat_rows(0)                                # unfolded statistic sums: a batch-statistics forward repeats bit for bit
        with torch.no_grad():
            ref_train = m.train()(x).clone()                          # k = 4: the batch-statistics forward (it updates the running statistics)
        m.load_state_dict({n: v for n, v in before.items()}, strict=False)
        assert all(torch.equal(v, _bn_snapshot(m)[n]) for n, v in before.items())
        m.set_trainable_layers(2).train()
        with pytest.raises(RuntimeError, match="freeze_batchnorm"):
            m(x)
        torch.cuda.synchronize()
        after = _bn_snapshot(m)
        assert all(torch.equal(before[n], after[n]) for n in before) # refused before anything was launched
        with torch.no_grad():
            assert torch.equal(m(x), ref_train)                       # no_grad: never affected (the k = 4 result)
    finally:
        _hip.lib().tf_set_stat_rows(prev)
    m.load_state_dict({n: v for n, v in before.items()}, strict=False)
    assert torch.equal(m.eval()(x), ref_eval)                         # eval(): never affected
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.loss import DetectionCriterion
    eng = TrainEngine(m, DetectionCriterion(25), device="cuda")
    g = torch.Generator().manual_seed(3)
    cm = torch.where(torch.rand(2, 25, 12, 16, generator=g) < 0.02, 1.0, -1.0).cuda()
    rm = torch.randn(2, 100, 12, 16, generator=g).cuda()
    before = _bn_snapshot(m)
    with pytest.raises(RuntimeError, match="freeze_batchnorm"):
        eng.step(x, cm.clone(), rm)
    after = _bn_snapshot(m)
    assert all(torch.equal(before[n], after[n]) for n in before)
    m.freeze_batchnorm()                                              # the order of the two setters does not matter
    eng.step(x, cm.clone(), rm)
    torch.cuda.synchronize()
    eng.close()


def test_two_rank_engine_with_frozen_stages_equals_single_process_on_the_summed_micro_batches(tmp_path):
    """2 gloo ranks sharing cuda:0 at k = 1 (tests/dist_worker_trainable.py) against ONE process that sums the gradients of the same two
    micro-batches and takes the segment-aware step over the trained tensors."""
    from tinyfaces import ops
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dist_worker_trainable
    golden = os.path.join(ROOT, "tests", "golden", "trainer.npz")
    out = str(tmp_path / "rank0.npz")
    steps = 3
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29577", os.path.join(ROOT, "tests", "dist_worker_trainable.py"), golden, out, str(steps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.load(out)
    assert int(got["buckets"]) >= 2
    dist = [got[f"arr_{i}"] for i in range(steps)]
    reps = []
    for r_ in range(2):
        m, c, batches = dist_worker_trainable.build(golden)
        m = m.cuda().train()
        flat = m.flatten_parameters()
        reps.append(dict(m=m, c=c, flat=flat, mom=torch.zeros_like(flat), batch=[t.cuda() for t in batches[r_]]))
    m0 = reps[0]["m"]
    assert m0.trainable_layers == 1 and m0.batchnorm_frozen
    groups = m0.group_ranges()
    seg = m0._segments
    names = m0.trainable_parameter_names()
    assert len(names) == COUNTS["resnet50"][3]
    trained = sorted((seg[n][0], seg[n][0] + seg[n][1]) for n in names)
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
    report("partial_freeze_dist_2_ranks_vs_single[resnet50,k=1]", worst_rel=str([f"{w:.2e}" for w in worst]))
    assert all(np.isfinite(d).all() for d in dist) and all(np.isfinite(w) for w in worst), worst
    assert float(np.abs(dist[-1] - first).max()) > 0.0                 # the ranks did train
    for n, (o, num) in seg.items():                                    # ... and left every frozen tensor alone
        if n not in names:
            assert np.array_equal(dist[-1][o:o + num], first[o:o + num]), n
    for n in ("model.layer3.0.conv1.weight", "score_res4.weight"):
        o, num = seg[n]
        assert not np.array_equal(dist[-1][o:o + num], first[o:o + num]), n
    assert worst[0] < 1e-5, worst
    assert worst[-1] < 1e-2, worst
