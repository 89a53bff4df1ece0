"""-m gpu: the ResNet-50 / ResNet-152 trunks of DetectionModel(base_model=...) on the executor (tf_detnet_trunk_*): fp32 parity with the CPU
oracle of the same depth, the bf16 training step at the benchmarked size, the fused engine, the data-parallel exchange, detection, the
entry scripts -- and ResNet-101 through the trunk-aware entry points equal to the default ones."""
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
PKG = os.path.join(ROOT, "tiny-faces-pytorch_amd")
BLOCKS = {"resnet50": (3, 4, 6), "resnet101": (3, 4, 23), "resnet152": (3, 8, 36)}


def _cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float(a @ b / (a.norm() * b.norm() + 1e-30))


def oracle_model(name, seed=0):
    """The CPU oracle (oracle/model.py) with torchvision's ResNet of this depth in place of resnet101, layer4 deleted, tamed init."""
    from oracle.model import OracleDetectionModel, tame_init_
    from oracle.resnet import ResNet
    om = OracleDetectionModel(num_templates=25)
    om.model = ResNet(BLOCKS[name] + (3,))
    del om.model.layer4
    return tame_init_(om, seed)


def product_model(name, om=None, dtype=torch.float32):
    from tinyfaces.models import model as mm
    m = mm.DetectionModel(base_model=getattr(mm, name), num_templates=25)
    if om is not None:
        m.load_state_dict(om.state_dict(), strict=True)
    return m.cuda().set_compute_dtype(dtype)


@pytest.mark.parametrize("training", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("name", ["resnet50", "resnet101", "resnet152"])
def test_fp32_vs_oracle_of_the_same_depth(name, training):
    """bs 2 at an odd 131 x 157: maps within 1e-3 (measured 3e-7 .. 1.7e-6), running statistics within 1e-5, every conv / head gradient
    cosine > 0.9999 and every BatchNorm vector > 0.999.  The BN vectors are sums over the 680 pixels of a layer-3 map that largely cancel, and
    a ReLU whose input sits within fp32 rounding of 0 masks a pixel in one implementation and not in the other: measured down to 0.99982
    (ResNet-152, layer3.15.bn2.bias).  A ResNet-152 that ran a 23-block layer 3 misses every bar."""
    om = oracle_model(name).train(training)
    m = product_model(name, om).train(training)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 131, 157, generator=g)
    yo = om(x)
    y = m(x.cuda())
    dy = err(y.detach().cpu().numpy(), yo.detach().numpy())
    res = dict(map_maxabs=dy[0], map_maxref=dy[1])
    if training:
        gy = torch.randn(yo.shape, generator=g) * 0.1
        yo.backward(gy)
        y.backward(gy.cuda())
        pd = dict(m.named_parameters())
        cos = {k: _cos(pd[k].grad.cpu(), p.grad) for k, p in om.named_parameters() if p.grad is not None and not k.startswith("score4_upsample")}
        assert len(cos) == sum(1 for k in pd if not k.startswith(("score4_upsample", "model.fc."))), "a trunk tensor got no gradient"
        worst = min(cos, key=cos.get)
        conv = {k: v for k, v in cos.items() if pd[k].dim() == 4 or k.startswith("score_res")}
        worst_conv = min(conv, key=conv.get)
        sd, osd = m.state_dict(), om.state_dict()
        drs = max(err(sd[k].cpu().numpy(), osd[k].numpy())[2] for k in osd if k.endswith(("running_mean", "running_var")))
        res.update(cos_min=cos[worst], worst=worst, cos_min_conv=conv[worst_conv], worst_conv=worst_conv, running_rel=drs, tensors=len(cos))
        report(f"trunk_fp32_vs_oracle[{name},train]", **res)
        assert dy[0] < 1e-3
        assert conv[worst_conv] > 0.9999, (worst_conv, conv[worst_conv])
        assert cos[worst] > 0.999, (worst, cos[worst])
        assert drs < 1e-5
    else:
        report(f"trunk_fp32_vs_oracle[{name},eval]", **res)
        assert dy[0] < 1e-3


@pytest.fixture(scope="module")
def fullsize_batch():
    """One seeded bs = 12, 500 x 500 batch with the oracle's target maps (as tests/test_gpu_fullsize.py builds it)."""
    from oracle import targets as otgt
    from tinyfaces.datasets.synthetic import random_boxes
    from tinyfaces.datasets.templates import load_templates
    templates = load_templates()
    g = torch.Generator().manual_seed(0)
    x = torch.randn(12, 3, 500, 500, generator=g)
    rng = np.random.RandomState(0)
    boxes = [random_boxes(rng) for _ in range(12)]
    pad = otgt.get_padding(templates, [0, 0, 500, 500])
    noise = [np.random.RandomState(100 + i).rand(63, 63, 25, b.shape[0]) for i, b in enumerate(boxes)]
    maps = [otgt.get_heatmaps(b.copy(), templates, pad, noise=n) for b, n in zip(boxes, noise)]
    cm = torch.from_numpy(np.ascontiguousarray(np.stack([c.transpose(2, 0, 1) for c, _, _ in maps]))).float()
    rm = torch.from_numpy(np.ascontiguousarray(np.stack([r.transpose(2, 0, 1) for _, r, _ in maps]))).float()
    return x, cm, rm


@pytest.mark.parametrize("name", ["resnet50", "resnet152"])
def test_bf16_train_step_bs12_500x500_vs_fp32(fullsize_batch, name):
    """The benchmarked step (grouped layer-3 weight gradients: one group of 5 identity blocks for ResNet-50, five of 7 for ResNet-152) against
    the fp32 path of the same trunk on the GPU.  ResNet-50 is held to the bf16 bars of ResNet-101 (tests/test_gpu_fullsize.py; measured maps
    1.3e-2, gradient cosines 0.954 minimum / 0.971 5th percentile / 0.984 median).  ResNet-152 rounds its activations to bf16 at 47 block
    outputs instead of 30 and the error grows with the depth: measured maps 2.1e-2 of a 1.11 range, cosines 0.878 minimum (a cancelling
    layer-1 BN sum, as for ResNet-101) / 0.903 outside layer-1 BN / 0.920 5th percentile / 0.944 median: its bars are those values with a
    margin, scaled like the map bar by the depth (1.8e-2 x 47 / 30)."""
    bars = dict(resnet50=dict(y=1.8e-2, rest=0.90, p05=0.93, med=0.96), resnet152=dict(y=2.8e-2, rest=0.87, p05=0.90, med=0.93))[name]
    from oracle import criterion as ocrit
    x, cm, rm = fullsize_batch
    om = oracle_model(name)
    m32 = product_model(name, om, torch.float32).train()
    y32 = m32(x.cuda())
    np.random.seed(11)
    gy = ocrit.criterion(y32.detach().cpu(), cm, rm)["grad"]
    y32.backward(gy.cuda())
    mb = product_model(name, om, torch.bfloat16).train()
    yb = mb(x.cuda())
    yb.backward(gy.cuda())
    dy = err(yb.detach().cpu().numpy(), y32.detach().cpu().numpy())
    p32, pb = dict(m32.named_parameters()), dict(mb.named_parameters())
    cos = {k: _cos(pb[k].grad.cpu(), p32[k].grad.cpu()) for k in p32 if p32[k].grad is not None and not k.startswith("score4_upsample")}
    cosv = np.array(list(cos.values()))
    low = sorted((v, k) for k, v in cos.items() if v < 0.90)
    is_l1_bn = lambda k: ".bn" in k and "layer1" in k                 # noqa: E731
    rest_min = min(v for k, v in cos.items() if not is_l1_bn(k))
    s32, sb = m32.state_dict(), mb.state_dict()
    drm = max(err(sb[k].cpu().numpy(), s32[k].cpu().numpy())[2] for k in s32 if k.endswith("running_mean") and ".layer" in k)
    drv = max(err(sb[k].cpu().numpy(), s32[k].cpu().numpy())[2] for k in s32 if k.endswith("running_var"))
    report(f"trunk_bf16_fullsize[{name}]", y_maxabs=dy[0], y_maxref=dy[1], cos_min=float(cosv.min()), cos_p05=float(np.quantile(cosv, .05)),
           cos_med=float(np.median(cosv)), lowest=str(low[:3]), rest_min=rest_min, running_mean_rel=drm, running_var_rel=drv, tensors=len(cos))
    assert len(cos) == 3 * sum(BLOCKS[name]) * 3 + 3 * 3 + 3 + 4      # every conv / BN of the trunk, the stem, the heads
    assert dy[0] < bars["y"]
    assert rest_min >= bars["rest"], rest_min                          # every tensor but the layer-1 BN sums
    assert np.quantile(cosv, .05) > bars["p05"] and np.median(cosv) > bars["med"]
    assert cosv.min() > 0.85 and all(is_l1_bn(k) for _, k in low if _ < bars["rest"]), low
    assert drm < 2e-2 and drv < 2e-2


def _oracle_weights_for(m, name):
    m.load_state_dict(oracle_model(name).state_dict(), strict=True)
    return m


@pytest.mark.parametrize("stat_rows", [0, 8])
def test_fused_engine_equals_autograd_trainer_resnet50(golden, stat_rows):
    """TrainEngine against trainer.train + torch.optim.SGD (main.py:67-70), ResNet-50, bars of tests/test_gpu_model.py."""
    from tinyfaces import _hip, trainer
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as mm
    from tinyfaces.models.loss import DetectionCriterion
    g = golden("trainer")
    batches = [(torch.from_numpy(g[f"b{i}_img"]), torch.from_numpy(g[f"b{i}_cm"].astype(np.float32)), torch.from_numpy(g[f"b{i}_rm"]).float())
               for i in range(2)]
    keep = torch.ones(2, 25 * 16 * 16, dtype=torch.uint8)
    keep[:, 128:] = 0

    def fresh():
        m = _oracle_weights_for(mm.DetectionModel(base_model=mm.resnet50, num_templates=25), "resnet50").set_compute_dtype(torch.float32)
        c = DetectionCriterion(25)
        c.inject_sampling(keep, keep)
        return m, c

    def worst_diff(a, b):
        return max((err(b[k].cpu().numpy(), a[k].cpu().numpy())[2], k) for k in a if a[k].is_floating_point())

    res = {}
    prev = _hip.lib().tf_get_stat_rows()
    try:
        _hip.lib().tf_set_stat_rows(stat_rows)
        for nsteps in (1, 2):
            m1, c1 = fresh()
            opt = torch.optim.SGD(m1.learnable_parameters(1e-3), lr=1e-3, momentum=0.9, weight_decay=5e-4)
            with redirect_stdout(io.StringIO()):
                trainer.train(m1, c1, opt, batches[:nsteps], 0, torch.device("cuda"))
            m2, c2 = fresh()
            eng = TrainEngine(m2, c2, lr=1e-3, momentum=0.9, weight_decay=5e-4, device="cuda")
            for img, cm, rm in batches[:nsteps]:
                eng.step(img.cuda(), cm.cuda(), rm.cuda())
            res[nsteps] = worst_diff(m1.state_dict(), m2.state_dict())
            assert int(m2.state_dict()["model.bn1.num_batches_tracked"]) == nsteps
            assert list(m2.state_dict()) == list(m1.state_dict()) and len(m1.state_dict()) == 265
            eng.close()
    finally:
        _hip.lib().tf_set_stat_rows(prev if prev <= 16 else 0)
    report(f"trunk_engine_vs_trainer[resnet50,rows={stat_rows}]", step1=res[1][0], step1_tensor=res[1][1], step2=res[2][0], step2_tensor=res[2][1])
    assert res[1][0] < (1e-6 if stat_rows == 0 else 2e-3), res[1]
    assert res[2][0] < (1e-2 if stat_rows == 0 else 1e-1), res[2]


def test_two_rank_engine_equals_single_process_gradient_average_resnet50(tmp_path):
    """2 gloo ranks sharing cuda:0 (tests/dist_worker_trunks.py: the ResNet-50 engine with its own buckets) against ONE process that averages
    the gradients of the same two micro-batches."""
    from tinyfaces import _hip, ops
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dist_worker_trunks
    golden = os.path.join(ROOT, "tests", "golden", "trainer.npz")
    out = str(tmp_path / "rank0.npz")
    steps = 3
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29571", os.path.join(ROOT, "tests", "dist_worker_trunks.py"), golden, out, str(steps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=500, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = np.load(out)
    assert int(got["buckets"]) >= 2
    dist = [got[f"arr_{i}"] for i in range(steps)]
    prev = _hip.lib().tf_get_stat_rows()
    try:
        _hip.lib().tf_set_stat_rows(0)
        reps = []
        for r_ in range(2):
            m, c, batches = dist_worker_trunks.build(golden)
            m = m.cuda().train()
            flat = m.flatten_parameters()
            reps.append(dict(m=m, c=c, flat=flat, mom=torch.zeros_like(flat), batch=[t.cuda() for t in batches[r_]]))
        groups = reps[0]["m"].group_ranges()
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
                        ops.sgd_step(rp["flat"][a:b], gsum[a:b], rp["mom"][a:b], 1e-4 * mult, 0.9, 5e-4, 0.5)
            torch.cuda.synchronize()
            ref = reps[0]["flat"].cpu().numpy()
            worst.append(float(np.abs(dist[s] - ref).max() / (np.abs(ref).max() + 1e-30)))
    finally:
        _hip.lib().tf_set_stat_rows(prev if prev <= 16 else 0)
    report("trunk_dist_2_ranks_vs_single[resnet50]", worst_rel=str([f"{w:.2e}" for w in worst]))
    assert all(np.isfinite(d).all() for d in dist) and all(np.isfinite(w) for w in worst), worst
    assert worst[0] < 1e-5, worst
    assert worst[-1] < 1e-2, worst


def test_detections_resnet50_lanes_and_oracle(monkeypatch):
    """get_detections on a ResNet-50: 3 lanes bit-identical to 1 lane; fp32 candidates and surviving index set equal to the oracle pipeline's
    (oracle/pyramid.py) on a small image, with the threshold in the widest gap between candidate probabilities."""
    from oracle import pyramid
    from oracle.nms import nms as onms
    from oracle.refstub import Compose, Normalize, ToTensor, to_pil_image
    from oracle.targets import RF
    from tinyfaces import transforms
    from tinyfaces.datasets.templates import load_templates
    from tinyfaces.evaluation import get_detections
    templates = load_templates()
    om = oracle_model("resnet50", 2).eval()
    img = torch.rand(3, 336, 448, generator=torch.Generator().manual_seed(4))   # (the reference's decode masks the width axis with template ids, D1: >= 25 columns at 1/2)
    otf = Compose([ToTensor(), Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])])
    with torch.no_grad():                       # a first cut that lets ~0.5 % of the full-size level's anchors through (a bounded candidate list)
        p0 = torch.sigmoid(om(otf(to_pil_image(img)).unsqueeze(0))[:, :25]).flatten()
    first = float(torch.quantile(p0, 0.995))
    _, ocand, _ = pyramid.get_detections(om, img, templates, RF, otf, prob_thresh=first, nms_thresh=0.3, scales=(-1, 0, 1), return_candidates=True)
    prob = np.sort(torch.sigmoid(torch.from_numpy(ocand[:, 4].astype(np.float32))).numpy())[::-1]
    lo, hi = prob.size // 4, (3 * prob.size) // 4
    assert hi > lo + 10, prob.size
    j = lo + int(np.argmax(prob[lo:hi] - prob[lo + 1:hi + 1]))
    thr = float(np.float32((np.float64(prob[j]) + np.float64(prob[j + 1])) / 2))
    _, ocand, okeep = pyramid.get_detections(om, img, templates, RF, otf, prob_thresh=thr, nms_thresh=0.3, scales=(-1, 0, 1), return_candidates=True)
    m = product_model("resnet50", om, torch.float32).eval()
    tf = transforms.Compose([transforms.ToTensor(), transforms.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])])
    kw = dict(prob_thresh=thr, nms_thresh=0.3, scales=(-1, 0, 1), device="cuda", return_candidates=True)
    runs = {}
    for lanes in ("1", "3"):
        monkeypatch.setenv("TINYFACES_EVAL_LANES", lanes)
        with m.constant_weights():
            runs[lanes] = get_detections(m, img, templates, RF, tf, **kw)
    dets, cand, keep = runs["3"]
    same_n = cand.shape[0] == ocand.shape[0]
    dc = err(cand[:, :4], ocand[:, :4])[0] if same_n else -1
    ds = err(cand[:, 4], ocand[:, 4])[0] if same_n else -1
    report("trunk_detections[resnet50]", candidates=cand.shape[0], ref_candidates=ocand.shape[0], kept=dets.shape[0], cand_maxabs=dc,
           score_maxabs=ds, thr=thr, margin=float(min(prob[j] - thr, thr - prob[j + 1])))
    assert all(np.array_equal(a, b) for a, b in zip(runs["1"], runs["3"]))
    assert cand.shape[0] > 10 and same_n and dc < 1e-2 and ds < 1e-3
    assert np.array_equal(keep, onms(cand[:, :4], cand[:, 4], 0.3))
    assert np.array_equal(np.sort(keep), np.sort(okeep))


class _LegacyAbi:
    """The library with every tf_detnet_trunk_* call answered by the entry point of the same name without `trunk_` (the ResNet-101 ABI),
    the trunk argument dropped: what DetectionModel did before the trunk-aware forms existed."""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name.startswith("tf_detnet_trunk_"):
            legacy = getattr(self._lib, name.replace("tf_detnet_trunk_", "tf_detnet_"))
            return lambda blocks, *args: legacy(*args)
        return getattr(self._lib, name)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_resnet101_through_the_trunk_entry_points_equals_the_default_path(monkeypatch, dtype):
    """Same model, same input, once through tf_detnet_trunk_*({3, 4, 23}) and once through the entry points without a trunk: forward outputs
    torch.equal (training with reproducible statistics, and eval), and every gradient torch.equal wherever two runs of the default path are
    themselves bit-identical (the split-K weight gradients add with fp32 atomics: there the bar is that run-to-run spread)."""
    from tinyfaces._hip import lib
    from tinyfaces.models import model as mm
    om = oracle_model("resnet101")
    x = torch.randn(2, 3, 160, 192, generator=torch.Generator().manual_seed(5)).cuda()
    gy = None

    def run(legacy):
        nonlocal gy
        with monkeypatch.context() as mp:
            if legacy:
                mp.setattr(mm, "lib", lambda: _LegacyAbi(lib()))
            m = product_model("resnet101", om, dtype).train()
            y = m(x)
            if gy is None:
                gy = torch.randn(y.shape, generator=torch.Generator().manual_seed(6)).cuda()
            y.backward(gy)
            m.eval()
            with m.constant_weights():
                ye = m(x)
            torch.cuda.synchronize()
            return y.detach(), ye, {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}, \
                {k: v.clone() for k, v in m.state_dict().items()}

    prev = lib().tf_get_stat_rows()
    try:
        lib().tf_set_stat_rows(0)
        a, b, new = run(True), run(True), run(False)
    finally:
        lib().tf_set_stat_rows(prev if prev <= 16 else 0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])            # the default path is reproducible here
    assert torch.equal(new[0], a[0]) and torch.equal(new[1], a[1])
    assert all(torch.equal(new[3][k], a[3][k]) for k in a[3])              # running statistics, counters
    exact, worst = 0, 0.0
    for k in a[2]:
        if torch.equal(a[2][k], b[2][k]):
            exact += 1
            assert torch.equal(new[2][k], a[2][k]), k
        else:                                   # fp32-atomic summation order only: the bar of test_gpu_model.py's dual-stream race screen
            worst = max(worst, float((new[2][k] - a[2][k]).abs().max() / (a[2][k].abs().max() + 1e-30)))
    report(f"trunk_resnet101_abi_equal[{dtype}]", gradients=len(a[2]), bit_identical=exact, worst_rel_of_the_rest=worst)
    assert len(new[2]) == len(a[2]) == 287 and worst < 1e-4               # (286 trained tensors + the lr-0 upsample)


def test_scripts_end_to_end_resnet50(tmp_path):
    """main.py --base-model resnet50 trains one short epoch and writes a checkpoint; evaluate_model.py loads it with no trunk flag
    (evaluation.get_model reads the trunk off the keys) and writes result files."""
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def run(args):
        r = subprocess.run([sys.executable] + args, cwd=tmp_path, capture_output=True, text=True, timeout=400, env=env)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
        return r.stdout
    out = run([os.path.join(PKG, "main.py"), "synthetic", "synthetic", "--base-model", "resnet50", "--epochs", "1", "--save-every", "1",
               "--synthetic-len", "8", "--batch_size", "4", "--lr", "1e-5"])
    assert "Epoch: [0][1/2]" in out
    state = torch.load(tmp_path / "weights" / "checkpoint_1.pth", map_location="cpu")
    assert len(state["model"]) == 265 and "model.layer3.5.conv3.weight" in state["model"] and "model.layer3.6.conv1.weight" not in state["model"]
    # evaluate a checkpoint of that trunk with the heads scaled down (bench.py's random-init recipe: finite boxes)
    sys.path.insert(0, ROOT)
    from bench import tame_init_
    from tinyfaces.models import model as mm
    m = mm.DetectionModel(base_model=mm.resnet50, num_objects=1, num_templates=25)
    m.load_state_dict(state["model"])
    tame_init_(m, seed=3)
    with torch.no_grad():
        for head in (m.score_res3, m.score_res4):
            head.bias[:25] -= 3.0
    ck = tmp_path / "weights" / "tame50.pth"
    torch.save({"epoch": 1, "batch_size": 4, "model": m.state_dict(), "optimizer": {}}, ck)
    run([os.path.join(PKG, "evaluate_model.py"), "synthetic", "--checkpoint", str(ck), "--num-images", "2", "--prob_thresh", "0.5",
         "--results_dir", str(tmp_path / "res")])
    assert sorted(os.listdir(tmp_path / "res" / "synthetic")) == ["img_0.txt", "img_1.txt"]
