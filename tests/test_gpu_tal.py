"""-m gpu: the task-aligned target assignment (tf_targets_tal, csrc/targets_tal.hip) against tests/tal_ref.py, the numpy restatement of the
rule in include/tinyfaces_hip.h ("TAL").  Every case of tests/tal_cases.py is one small call held to: class map, regression map and
match_count array_equal to the restatement.  exp and pow are not bit-reproducible between numpy and the device: a face the restatement calls
AMBIGUOUS (tests/tal_ref.py) is only held to the number of its winners and to their metric reaching its cut; no planted face may be ambiguous
and at most 1 % of the random ones (the counts of the restatement alone: profiles/tal_parity.txt)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import redzone
import tal_cases as tc
import tal_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tiny-faces-pytorch_amd")


def _operands(case, dev="cuda"):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return d(case["out"]), d(case["cm"]), d(case["rm"])


def _call(case, **kw):
    from tinyfaces import ops
    out, cm, rm = _operands(case)
    keep = out.clone()
    res = ops.tal_assign(out, cm, rm, case["boxes"], case["t"], paste_boxes=case["pastes"], flips=case["flips"], topk=case["topk"], alpha=case["alpha"],
                         beta=case["beta"], return_match_count=True, **kw)
    assert res[0] is cm and res[1] is rm and res[2].dtype == torch.int32 and torch.equal(out.view(torch.int32), keep.view(torch.int32))
    return cm.cpu().numpy(), rm.cpu().numpy(), res[2].cpu().numpy()


def _hold(case, ref, got):
    """-> the number of ambiguous faces of the case."""
    cm, rm, mc = got
    at = amb = 0
    for b, want in enumerate(ref):
        n = want[2].size
        try:
            amb += tal_ref.compare((cm[b], rm[b], mc[at:at + n]), want, case["hm"])
        except AssertionError as e:
            raise AssertionError(f"{case['name']}: image {b}: {e}") from None
        at += n
    assert at == mc.size
    return amb


@pytest.mark.parametrize("name", list(tc.planted()))
def test_planted(name):
    case, ref = tc.planted()[name], tc.planted_reference(name)
    assert not any(f["ambiguous"] for im in ref for f in im[3])
    assert _hold(case, ref, _call(case)) == 0


@pytest.mark.parametrize("ci", range(len(tc.RANDOM)))
def test_random(ci):
    """Maps from 5 x 7 to 63 x 63, 1 / 3 / 25 templates, topk 1 / 13 / 32, B = 1..4 with an image without faces first, in the middle and last,
    padded and mirrored, outputs from N(0, 1) and N(0, 0.1)."""
    case, ref = tc.random_case(ci), tc.random_reference(ci)
    total = sum(len(im[3]) for c in range(len(tc.RANDOM)) for im in tc.random_reference(c))
    assert _hold(case, ref, _call(case)) <= 0.01 * total
    assert int(sum(im[2].sum() for im in ref)) > 0


@pytest.mark.parametrize("mutant", tal_ref.MUTANTS)
def test_mutants_of_the_restatement_fail(mutant):
    """The anchor's IoU instead of the predicted box's, no clamp, >= instead of strictly inside, conflicts by m instead of u, topk + 1 winners:
    each restatement so mutated must fail the comparison the kernel passes."""
    name = tc.MUTANT_CASES[mutant]
    case, got = tc.planted()[name], None
    got = _call(case)
    assert _hold(case, tc.planted_reference(name), got) == 0
    with pytest.raises(AssertionError):
        _hold(case, tc.restate(case, mutant=mutant), got)


def test_the_same_call_twice_gives_the_same_bits():
    for case in (tc.random_case(6), tc.planted()["output 0, topk 13"], tc.planted()["conflict by face index"]):
        a, b = _call(case), _call(case)
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def test_an_image_does_not_depend_on_its_batch():
    from tinyfaces import ops
    case = tc.random_case(3)
    cm, rm, mc = _call(case)
    out, cm0, rm0 = _operands(case)
    at = 0
    for b in range(len(case["boxes"])):
        r = ops.tal_assign(out[b:b + 1].contiguous(), cm0[b:b + 1].clone(), rm0[b:b + 1].clone(), [case["boxes"][b]], case["t"], paste_boxes=[case["pastes"][b]],
                           flips=[case["flips"][b]], topk=case["topk"], return_match_count=True)
        n = r[2].numel()
        assert np.array_equal(r[0][0].cpu().numpy(), cm[b]) and np.array_equal(r[1][0].cpu().numpy(), rm[b]) and np.array_equal(r[2].cpu().numpy(), mc[at:at + n])
        at += n
    assert at == mc.size


def _raw_call(case, ws_boxes=None):
    """tf_targets_tal called directly, every operand and the workspace between guard bands; match_count arrives filled with 0xFF.
    ws_boxes: size the workspace for that many boxes instead of the batch's own number."""
    from tinyfaces import _hip
    dev = torch.device("cuda")
    kept = [tal_ref.atss_ref.valid(b) for b in case["boxes"]]
    offs = np.cumsum([0] + [x.shape[0] for x in kept]).astype(np.int32)
    total, B, (vsy, vsx), nt = int(offs[-1]), len(kept), case["hm"], case["t"].shape[0]
    g = lambda a: redzone.guarded_like(torch.from_numpy(np.ascontiguousarray(a)), dev)
    boxes_d = g(np.concatenate(kept) if total else np.zeros((1, 4)))
    offs_d, t_d, out_d, cls, reg = g(offs), g(case["t"]), g(case["out"]), g(case["cm"]), g(case["rm"])
    paste_d = None if case["pastes"] is None else g(np.asarray(case["pastes"], dtype=np.int32).reshape(B, 4))
    flips_d = None if case["flips"] is None else g(np.asarray(case["flips"], dtype=np.int32))
    mc = redzone.guarded((max(total, 1),), torch.int32, dev)
    l = _hip.lib()
    wsb = l.tf_targets_tal_workspace_bytes(total if ws_boxes is None else ws_boxes, B, nt, vsy, vsx)
    ws = redzone.guarded_workspace(wsb, dev)
    p = _hip.ptr
    rc = l.tf_targets_tal(p(out_d), p(boxes_d), p(offs_d), B, p(t_d), nt, case["t"].shape[1], vsy, vsx, -1, -1, 8, 8, p(paste_d), p(flips_d),
                          case["topk"], case["alpha"], case["beta"], p(mc), p(cls), p(reg), p(ws), wsb, _hip.stream())
    assert rc == 0
    torch.cuda.synchronize()
    named = dict(output=out_d, boxes=boxes_d, offsets=offs_d, templates=t_d, class_map=cls, reg_map=reg, match_count=mc, workspace=ws)
    if paste_d is not None:
        named.update(paste=paste_d, flips=flips_d)
    for name, x in named.items():
        redzone.assert_guards(x, name)
    assert np.array_equal(out_d.cpu().numpy().view(np.int32), case["out"].view(np.int32))
    return cls, reg, mc, total


@pytest.mark.parametrize("which", ["random 3", "random 6", "257 candidates", "window of many tiles", "padded, mirrored, fully padded"])
def test_guard_bands_on_every_operand(which):
    case, ref = (tc.random_case(int(which[7:])), tc.random_reference(int(which[7:]))) if which.startswith("random") else (tc.planted()[which], tc.planted_reference(which))
    cls, reg, mc, total = _raw_call(case)
    redzone.assert_written(mc, what="match_count")                     # every face's count is written, over the NaN pattern it arrived with
    _hold(case, ref, (cls.cpu().numpy(), reg.cpu().numpy(), mc[:total].cpu().numpy()))


def test_workspace_too_small_for_the_device_total_writes_nothing():
    case = tc.random_case(2)
    total = sum(tal_ref.atss_ref.valid(b).shape[0] for b in case["boxes"])
    for ws_boxes in (1, total - 1):
        cls, reg, mc, _ = _raw_call(case, ws_boxes=ws_boxes)
        assert redzone.unwritten(mc)[0] == mc.numel()
        assert np.array_equal(cls.cpu().numpy(), case["cm"]) and np.array_equal(reg.cpu().numpy(), case["rm"])


def test_resident_entry_and_no_face_enqueues_nothing(monkeypatch):
    from tinyfaces import _hip, ops
    case = tc.random_case(6)
    want = _call(case)
    kept = [tal_ref.atss_ref.valid(b) for b in case["boxes"]]
    offs = np.cumsum([0] + [x.shape[0] for x in kept])
    out, cm, rm = _operands(case)
    r = dict(boxes_d=torch.from_numpy(np.concatenate(kept)).cuda(), offs_d=torch.tensor(offs, dtype=torch.int32).cuda(), total_boxes=int(offs[-1]),
             templates_d=torch.from_numpy(np.ascontiguousarray(case["t"])).cuda(), paste_d=torch.tensor(case["pastes"], dtype=torch.int32).cuda(),
             flips_d=torch.tensor(case["flips"], dtype=torch.int32).cuda())
    res = ops.tal_assign_device(out, cm, rm, heatmap_size=case["hm"], topk=case["topk"], return_match_count=True, **r)
    assert res[0] is cm and res[1] is rm
    assert all(np.array_equal(x.cpu().numpy(), y) for x, y in zip(res, want))
    assert len(ops.tal_assign_device(out, cm, rm, topk=case["topk"], **r)) == 2
    with pytest.raises(ValueError, match="heatmap_size"):
        ops.tal_assign_device(out, cm, rm, heatmap_size=(5, 7), **r)
    # a batch without a face: the maps stay, nothing is enqueued
    seen, real = [], _hip.lib()

    class Spy:
        def __getattr__(self, name):
            seen.append(name)
            return getattr(real, name)

    monkeypatch.setattr(ops, "lib", lambda: Spy())
    out, cm, rm = _operands(case)
    res = ops.tal_assign(out, cm, rm, [np.zeros((0, 4))] * 4, case["t"], paste_boxes=case["pastes"], flips=case["flips"], return_match_count=True)
    assert seen == [] and res[2].numel() == 0 and np.array_equal(cm.cpu().numpy(), case["cm"]) and np.array_equal(rm.cpu().numpy(), case["rm"])
    ops.tal_assign(out, cm, rm, case["boxes"], case["t"], paste_boxes=case["pastes"], flips=case["flips"])
    assert seen == ["tf_targets_tal_workspace_bytes", "tf_targets_tal"]


# ------------------------------------------------------------------------------------------------ the criterion, the engine, the loaders, main.py
def _spy(monkeypatch):
    from tinyfaces import _hip, ops
    seen, real = [], _hip.lib()

    class Spy:
        def __getattr__(self, name):
            seen.append(name)
            return getattr(real, name)

    monkeypatch.setattr(ops, "lib", lambda: Spy())
    return seen


def test_default_call_is_the_old_call(templates, monkeypatch):
    """Without assigner / faces the criterion, the engine and the loaders make the library calls they made: nothing of TAL is called."""
    import loss_cases as lc
    from tinyfaces.datasets import SyntheticFaces, TargetAssigner
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as zoo
    from tinyfaces.models.loss import DetectionCriterion
    seen = _spy(monkeypatch)
    g = torch.Generator().manual_seed(0)
    out = torch.randn(2, 125, 9, 11, generator=g).cuda()
    cm = (torch.randint(0, 20, (2, 25, 9, 11), generator=g) == 0).float().cuda() * 2 - 1
    rm = (torch.randn(2, 100, 9, 11, generator=g) * 0.2).cuda()
    crit = DetectionCriterion(25, cls_loss="qfl", reg_loss="diou", templates=templates)
    assert crit.assigner is None
    crit(out.clone().requires_grad_(True), cm, rm).backward()
    assert seen == ["tf_criterion_quality_workspace_bytes", "tf_criterion_quality_fwd_bwd"]
    del seen[:]
    DetectionCriterion(25)(out.clone().requires_grad_(True), cm.clone(), rm)
    assert seen == ["tf_criterion_workspace_bytes", "tf_criterion_fwd_bwd"]
    del seen[:]
    m = lc.mixed_batch()
    TargetAssigner(templates)(m["boxes"], paste_boxes=m["paste"], flips=m["flips"])
    assert seen == ["tf_targets_workspace_bytes", "tf_dense_overlap_targets"]
    del seen[:]
    ds = SyntheticFaces(templates, length=2, seed=0)
    batch = ds.collate([ds[0], ds[1]])
    assert len(batch) == 3 and not [n for n in seen if "tal" in n]
    model = zoo.DetectionModel(base_model=zoo.resnet50, num_templates=25).set_compute_dtype(torch.bfloat16)
    model.freeze_batchnorm(True)
    eng = TrainEngine(model, DetectionCriterion(25, cls_loss="qfl", reg_loss="diou", templates=templates), lr=1e-4, device="cuda")
    del seen[:]
    eng.step(batch[0].float(), batch[1], batch[2])
    first = list(seen)
    del seen[:]
    eng.step(batch[0].float(), batch[1], batch[2])
    torch.cuda.synchronize()
    assert first[:2] == ["tf_criterion_quality_workspace_bytes", "tf_criterion_quality_fwd_bwd"] and not [n for n in first + seen if "tal" in n]
    with pytest.raises(ValueError, match="assigner"):                  # faces without an assigner
        eng.step_with_faces(batch[0].float(), batch[1], batch[2], object())
    with pytest.raises(ValueError, match="assigner"):
        crit(out.clone().requires_grad_(True), cm, rm, faces=object())
    eng.close()


def _tal_engine(templates, assign=True, **kw):
    """ResNet-50, frozen BatchNorm, fp32, qfl + diou on the golden trainer batches (2 x 2 images); deterministic weight gradients."""
    import dist_worker_trunks
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.loss import DetectionCriterion, TaskAligned
    m, _, batches = dist_worker_trunks.build(os.path.join(ROOT, "tests", "golden", "trainer.npz"))
    m.freeze_batchnorm()
    c = DetectionCriterion(25, cls_loss="qfl", reg_loss="diou", focal_normalize="pos", templates=templates, lazy_meters=True,
                           assigner=TaskAligned() if assign else None)
    return TrainEngine(m, c, lr=1e-4, device="cuda", deterministic=True, **kw), [b[0].cuda() for b in batches], (batches[0][1].shape[2], batches[0][1].shape[3])


def _faces_for(images, hm, seed):
    """Per image a few faces of 8-60 px on the picture (hm cells of 8 px)."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(images):
        s = np.exp(rng.uniform(np.log(8), np.log(60), 5))
        x, y = rng.uniform(0, 8 * hm[1] - s), rng.uniform(0, 8 * hm[0] - s)
        out.append(np.round(np.stack([x, y, x + 0.8 * s, y + s], 1), 3))
    return out


def test_engine_step_with_faces_is_the_step_on_the_maps_assigned_by_hand(templates):
    """TrainEngine.step_with_faces(..., faces) with qfl + diou equals the same step given the maps ops.tal_assign makes from the same forward output by
    hand: loss vector and flat gradient bit for bit.  The autograd path criterion(output, cm, rm, faces=) gives the same gradient."""
    from tinyfaces import ops
    from tinyfaces.datasets import TargetAssigner
    from tinyfaces.datasets.targets import ResidentFaces
    from tinyfaces.models.loss import DetectionCriterion, TaskAligned
    tal, imgs, hm = _tal_engine(templates)
    plain, _, _ = _tal_engine(templates, assign=False)
    img = imgs[0]
    H, W = img.shape[2:]
    boxes = _faces_for(img.shape[0], hm, 1)
    paste = [[0, 0, W, H]] * img.shape[0]
    assigner = TargetAssigner(templates, heatmap_size=hm, assigner="tal")
    cm0, rm0, faces = assigner(boxes, paste_boxes=paste, device="cuda")
    assert isinstance(faces, ResidentFaces) and faces.total == 10 and len(faces) == 2 and faces.stats is assigner.stats and assigner.stats.label == "TAL"
    assert set(torch.unique(cm0).tolist()) <= {-1.0, 0.0} and not bool(rm0.any()) and faces.to("cuda") is faces
    outs = []
    fwd = tal.model._run_forward
    tal.model._run_forward = lambda x, training=True: (lambda o: (outs.append(o.detach().clone()), o)[1])(fwd(x, training=training))
    cm1, rm1 = cm0.clone(), rm0.clone()
    loss1 = tal.step_with_faces(img, cm1, rm1, faces).clone()
    g1 = tal.model._grad_flat_persistent.clone()
    cm2, rm2, mc = ops.tal_assign(outs[0].float().contiguous(), cm0.clone(), rm0.clone(), boxes, templates, paste_boxes=paste, return_match_count=True)
    assert torch.equal(cm1, cm2) and torch.equal(rm1, rm2) and int((cm2 == 1).sum()) == int(mc.sum()) > 0      # the step completed its maps in place
    loss2 = plain.step(img, cm2, rm2)
    torch.cuda.synchronize()
    assert torch.equal(loss1, loss2) and float(loss1[3]) == float(mc.sum())
    assert torch.equal(g1.view(torch.int32), plain.model._grad_flat_persistent.view(torch.int32)) and float(g1.abs().sum()) > 0
    got = assigner.stats.pop()
    assert got == (10, int((mc <= 3).sum()), int((mc == 0).sum()))
    # autograd: d(total) / d(output) through criterion(..., faces=) is the gradient of the loss pass on the assigned maps
    crit = DetectionCriterion(25, cls_loss="qfl", reg_loss="diou", templates=templates, assigner=TaskAligned())
    o = outs[0].float().clone().requires_grad_(True)
    cm3, rm3 = cm0.clone(), rm0.clone()
    faces.stats = None
    crit(o, cm3, rm3, faces=faces).backward()
    _, want, _ = ops.criterion_quality_fwd_bwd(outs[0].float().contiguous(), cm2, rm2, 25, 1.0, 2.0, "pos", "diou", ops.template_wh(templates))
    assert torch.equal(cm3, cm2) and torch.equal(rm3, rm2) and torch.equal(o.grad, want)
    with pytest.raises(ValueError, match="faces"):                    # an assigner without faces
        crit(o, cm3, rm3)
    with pytest.raises(ValueError, match="faces"):
        tal.step(img, cm1, rm1)
    tal.close()
    plain.close()


def test_engine_a_window_of_two_micro_batches_against_the_batch_of_their_four_images(templates):
    """The assignment reads the forward output, and under frozen BatchNorm an image's forward output does not depend on its batch; qfl with
    focal_normalize="pos" makes its loss independent too.  So the accumulated gradient of (b0, b1) is the gradient of [b0; b1] up to the
    summation order of the weight gradients: relative L2 below 1e-6, QFL's bar (its figure: 3.3e-8).  The figure is printed and reported."""
    from gpu_util import report
    from test_gpu_grad_accum import _trained_mask
    from tinyfaces.datasets import TargetAssigner
    acc, imgs, hm = _tal_engine(templates, accum_steps=2)
    big, _, _ = _tal_engine(templates)
    H, W = imgs[0].shape[2:]
    boxes = _faces_for(4, hm, 2)
    assigner = TargetAssigner(templates, heatmap_size=hm, assigner="tal")
    won = []
    for k in range(2):
        cm, rm, faces = assigner(boxes[2 * k:2 * k + 2], paste_boxes=[[0, 0, W, H]] * 2, device="cuda")
        acc.step_with_faces(imgs[k], cm, rm, faces)
        won.append(cm == 1)
    cm, rm, faces = assigner(boxes, paste_boxes=[[0, 0, W, H]] * 4, device="cuda")
    big.step_with_faces(torch.cat(imgs), cm, rm, faces)
    torch.cuda.synchronize()
    assert (acc.steps, acc.micro_steps, big.steps) == (1, 2, 1)
    same_assignment = bool(torch.equal(torch.cat(won), cm == 1))
    mk, _ = _trained_mask(acc.model)
    mk = mk.cuda()
    ga, gb = acc.model._grad_flat_persistent[mk].double(), big.model._grad_flat_persistent[mk].double()
    rel = float((ga - gb).norm() / gb.norm())
    print(f"tal engine: accumulated vs 4-image gradient rel L2 {rel:.3g} (QFL on loader-side maps: 3.3e-8); same positives in both: {same_assignment}; "
          f"positives {int((cm == 1).sum())}")
    report("tal_engine_window_vs_big_batch[resnet50,fp32,frozen,qfl,diou]", grad_rel_l2=rel, same_assignment=same_assignment, positives=int((cm == 1).sum()))
    assert same_assignment and float(gb.norm()) > 0 and rel < 1e-6, rel
    acc.close()
    big.close()


def test_wider_dataloader_delivers_four_elements(tmp_path, templates):
    """A miniature WIDER tree through get_dataloader(..., assigner="tal"): the images of the plain loader's draw, the base maps (the
    dense_overlap path without a face: every label -1, regression map 0) and the ResidentFaces record of the batch."""
    from types import SimpleNamespace
    from PIL import Image
    from test_gpu_augment import synth_image
    from tinyfaces import ops, transforms
    from tinyfaces.datasets import ResidentFaces, get_dataloader
    root = tmp_path / "WIDER_train" / "images" / "0--Parade"
    root.mkdir(parents=True)
    ann = ""
    for k, (H, W) in enumerate([(600, 800), (420, 380), (700, 1000)]):
        name = f"0--Parade/img{k}.png"
        Image.fromarray(synth_image(40 + k, H, W), "RGB").save(tmp_path / "WIDER_train" / "images" / name)
        ann += f"{name}\n2\n{50 + 10 * k} {60 + 5 * k} 120 150 0 0 0 0 0 0\n{200 + k} {180 + k} 40 48 0 0 0 0 0 0\n"
    ann_file = tmp_path / "train.txt"
    ann_file.write_text(ann)
    args = SimpleNamespace(batch_size=3, workers=0, dataset_root=str(tmp_path), debug=False)
    tf = transforms.Compose([transforms.ToTensor(), transforms.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])])
    np.random.seed(123)
    loader, _ = get_dataloader(ann_file, args, img_transforms=tf, train=False, split="train", assigner="tal", tal_topk=7, tal_alpha=0.5, tal_beta=4.0)
    (x, cm, rm, faces), = list(loader)
    assert x.shape == (3, 3, 500, 500) and cm.shape == (3, 25, 63, 63) and rm.shape == (3, 100, 63, 63) and isinstance(faces, ResidentFaces)
    assert set(torch.unique(cm).tolist()) == {-1.0} and not bool(rm.any())
    assert len(faces) == 3 and faces.offs_d.tolist()[-1] == faces.total == faces.boxes_d.shape[0] and faces.paste_d.shape == (3, 4) and faces.flips_d.shape == (3,)
    ds = loader.dataset
    assert (ds.assigner, ds._targets.tal_topk, ds._targets.tal_alpha, ds._targets.tal_beta) == ("tal", 7, 0.5, 4.0) and faces.stats is ds.compensation_stats
    np.random.seed(123)
    plain, _ = get_dataloader(ann_file, args, img_transforms=tf, train=False, split="train")
    (x2, cm2, rm2), = list(plain)
    assert torch.equal(x, x2) and int((cm2 == 1).sum()) > 0
    # the record feeds the assignment: from a zero output the faces win anchors, none on padding
    out = torch.zeros(3, 125, 63, 63, device="cuda")
    c, r, mc = ops.tal_assign_device(out, cm.clone(), rm.clone(), faces.boxes_d, faces.offs_d, faces.total, torch.from_numpy(templates).cuda(),
                                     paste_d=faces.paste_d, flips_d=faces.flips_d, return_match_count=True)
    pad = np.stack([tal_ref.atss_ref.padding(templates, p, f, tal_ref.otgt.RF, (63, 63)).transpose(2, 0, 1)
                    for p, f in zip(faces.paste_d.tolist(), faces.flips_d.tolist())])
    assert int(mc.sum()) == int((c == 1).sum()) > 0 and pad.any() and not bool(((c == 1).cpu().numpy() & pad).any())


def test_main_trains_two_epochs_with_the_task_aligned_assigner(tmp_path):
    """main.py --assigner tal on synthetic-faces: two short epochs; the start-up line names the assigner in words, the match-count line is
    printed, no Epoch line holds a nan or an inf, and the checkpoint records the assigner under "args"."""
    import re
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(PKG, "main.py"), "synthetic-faces", "synthetic-faces", "--epochs", "2", "--save-every", "1",
                        "--synthetic-len", "8", "--batch_size", "4", "--lr", "1e-5", "--cls-loss", "qfl", "--reg-loss", "diou", "--assigner", "tal",
                        "--tal-topk", "9"], cwd=tmp_path, capture_output=True, text=True, timeout=400, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    print(r.stdout[-3000:])
    assert "Epoch: [0][1/2]" in r.stdout and "Epoch: [1][1/2]" in r.stdout
    assert "assigner TAL: every step, from the network's own output" in r.stdout and "the best 9 become its positives" in r.stdout
    counts = re.findall(r"TAL: (\d+) of (\d+) faces won at most 3 positives, (\d+) of them none", r.stdout)
    assert counts and all(int(a) <= int(b) and int(c) <= int(a) for a, b, c in counts) and sum(int(b) for _, b, _ in counts) > 0, counts
    values = [float(v) for v in re.findall(r"mean IoU of positives ([0-9.eE+-]+)", r.stdout)]
    assert values and all(0.0 <= v <= 1.0 for v in values), values
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("Epoch:") and ("nan" in ln.lower() or "inf" in ln.lower())]
    state = torch.load(tmp_path / "weights" / "checkpoint_2.pth", map_location="cpu", weights_only=False)
    assert state["args"]["assigner"] == "tal" and (state["args"]["tal_topk"], state["args"]["tal_alpha"], state["args"]["tal_beta"]) == (9, 1.0, 6.0)
