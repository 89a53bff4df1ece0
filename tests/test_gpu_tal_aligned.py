"""-m gpu: TOOD's task-aligned loss on the device against tests/tal_aligned_ref.py.
tf_targets_tal_aligned (csrc/targets_tal.hip): class map, regression map and match_count array_equal to the restatement AND to what tf_targets_tal
writes from the same operands; align_map within 1 float32 ulp of the restatement at the won anchors (exp and pow differ between numpy and the
device in the last bits of a double, which can move the final rounding to float32 by one step and no more) and exactly 1.0f everywhere else.
No face of these cases is ambiguous (tests/test_tal_aligned.py asserts it on the CPU).
tf_criterion_aligned_fwd_bwd (csrc/criterion_aligned.hip): loss sums and gradient within the project's bars (rtol 1e-5, atol 1e-6 divided by the
image's normaliser) of the float64 restatement, and of the focal kernel where the two coincide.  Then the criterion, the engine and main.py."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import box_loss_ref as br
import redzone
import tal_aligned_ref as ar
import tal_cases as tc
import tal_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tiny-faces-pytorch_amd")


# ------------------------------------------------------------------------------------------------------------------ the assigner
def _operands(case, dev="cuda"):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return d(case["out"]), d(case["cm"]), d(case["rm"])


def _call(case, aligned=True):
    """ops.tal_assign on fresh copies of the case's operands; align_out arrives NaN-filled.  -> (cm, rm, mc[, align]) as numpy."""
    from tinyfaces import ops
    out, cm, rm = _operands(case)
    keep = out.clone()
    kw = {}
    if aligned:
        kw["align_out"] = torch.full_like(cm, float("nan"))
    res = ops.tal_assign(out, cm, rm, case["boxes"], case["t"], paste_boxes=case["pastes"], flips=case["flips"], topk=case["topk"], alpha=case["alpha"],
                         beta=case["beta"], return_match_count=True, **kw)
    assert res[0] is cm and res[1] is rm and len(res) == 3 and torch.equal(out.view(torch.int32), keep.view(torch.int32))
    return (cm.cpu().numpy(), rm.cpu().numpy(), res[2].cpu().numpy()) + ((kw["align_out"].cpu().numpy(),) if aligned else ())


def _hold(case, ref, got, what):
    """Maps and counts exactly, align_map by tal_aligned_ref.hold_align.  -> the largest ulp distance."""
    cm, rm, mc, al = got
    at = 0
    for b, r in enumerate(ref):
        n = r["counts"].size
        assert np.array_equal(cm[b], r["cm"]), f"{what}: image {b}: class map differs at {np.argwhere(cm[b] != r['cm'])[:5].tolist()}"
        assert np.array_equal(rm[b], r["rm"]), f"{what}: image {b}: regression map differs"
        assert np.array_equal(mc[at:at + n], r["counts"]), f"{what}: image {b}: match_count {mc[at:at + n].tolist()} != {r['counts'].tolist()}"
        at += n
    assert at == mc.size
    return ar.hold_align(al, ref, what)


def _same_as_plain(case, got):
    plain = _call(case, aligned=False)
    assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip(got[:3], plain)), f"{case['name']}: tf_targets_tal writes other bits"


@pytest.mark.parametrize("name", tuple(ar.planted()) + ar.FROM_TAL_CASES)
def test_planted(name):
    """The conflict in which the loser loses its best-m anchor (both orders), a face that wins nothing, exactly one winner, 32 winners, M_g = 0,
    the 6-px face at zero output, more than 64 templates, base maps with a +1 the call does not win, padded / mirrored / fully padded images."""
    case, ref = ar.planted_case(name), ar.planted_reference(name)
    got = _call(case)
    _hold(case, ref, got, name)
    _same_as_plain(case, got)


@pytest.mark.parametrize("ci", range(len(ar.RANDOM)))
def test_random(ci):
    """Maps from 5 x 7 to 63 x 63, 1 / 3 / 25 templates, topk 1 / 13 / 32, B = 1..4 with an image without faces first, in the middle and last,
    padded and mirrored, outputs from N(0, 1) and N(0, 0.1)."""
    case, ref = ar.random_case(ci), ar.random_reference(ci)
    got = _call(case)
    worst = _hold(case, ref, got, case["name"])
    _same_as_plain(case, got)
    print(f"{case['name']}: {int(sum(r['won'].sum() for r in ref))} won anchors, align_map at most {worst} ulp from the restatement")


@pytest.mark.parametrize("mutant", ar.ASSIGN_MUTANTS)
def test_mutants_of_the_restatement_fail(mutant):
    """Maxima before the conflicts, U_g omitted, maxima per image, mmdetection's + 1e-7: each restatement so mutated must fail the comparison the
    kernel passes (the epsilon on the 6-px face at zero output)."""
    name = ar.ASSIGN_MUTANT_CASES[mutant]
    case = ar.planted_case(name)
    got = _call(case)
    _hold(case, ar.planted_reference(name), got, name)
    with pytest.raises(AssertionError):
        _hold(case, ar.restate(case, mutant=mutant), got, name)


def test_the_same_call_twice_gives_the_same_bits():
    for case in (ar.random_case(5), ar.planted_case("loser loses its best m"), ar.planted_case("conflict by face index")):
        a, b = _call(case), _call(case)
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(a, b))


def test_an_image_does_not_depend_on_its_batch():
    from tinyfaces import ops
    case = ar.random_case(3)
    cm, rm, mc, al = _call(case)
    out, cm0, rm0 = _operands(case)
    for b in range(len(case["boxes"])):
        a1 = torch.full_like(cm0[b:b + 1], float("nan"))
        ops.tal_assign(out[b:b + 1].contiguous(), cm0[b:b + 1].clone(), rm0[b:b + 1].clone(), [case["boxes"][b]], case["t"], paste_boxes=[case["pastes"][b]],
                       flips=[case["flips"][b]], topk=case["topk"], align_out=a1)
        assert np.array_equal(a1[0].cpu().numpy().view(np.int32), al[b].view(np.int32))       # (an image without faces: filled with 1 by the wrapper)


def _raw_call(case, ws_boxes=None):
    """tf_targets_tal_aligned called directly, every operand and the workspace between guard bands; match_count and align_map arrive filled with 0xFF
    (a NaN pattern).  ws_boxes: size the workspace for that many boxes instead of the batch's own number."""
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
    al = redzone.guarded(case["cm"].shape, torch.float32, dev)
    l = _hip.lib()
    wsb = l.tf_targets_tal_aligned_workspace_bytes(total if ws_boxes is None else ws_boxes, B, nt, vsy, vsx)
    ws = redzone.guarded_workspace(wsb, dev)
    p = _hip.ptr
    rc = l.tf_targets_tal_aligned(p(out_d), p(boxes_d), p(offs_d), B, p(t_d), nt, case["t"].shape[1], vsy, vsx, -1, -1, 8, 8, p(paste_d), p(flips_d),
                                  case["topk"], case["alpha"], case["beta"], p(mc), p(cls), p(reg), p(al), p(ws), wsb, _hip.stream())
    assert rc == 0
    torch.cuda.synchronize()
    named = dict(output=out_d, boxes=boxes_d, offsets=offs_d, templates=t_d, class_map=cls, reg_map=reg, match_count=mc, align_map=al, workspace=ws)
    if paste_d is not None:
        named.update(paste=paste_d, flips=flips_d)
    for name, x in named.items():
        redzone.assert_guards(x, name)
    assert np.array_equal(out_d.cpu().numpy().view(np.int32), case["out"].view(np.int32))
    return cls, reg, mc, al, total


@pytest.mark.parametrize("which", ["random 3", "random 5", "257 candidates", "window of many tiles", "padded, mirrored, fully padded", "loser loses its best m"])
def test_guard_bands_on_every_operand(which):
    case, ref = (ar.random_case(int(which[7:])), ar.random_reference(int(which[7:]))) if which.startswith("random") else (ar.planted_case(which), ar.planted_reference(which))
    cls, reg, mc, al, total = _raw_call(case)
    redzone.assert_written(mc, what="match_count")
    redzone.assert_written(al, what="align_map")                       # written completely, over the NaN pattern it arrived with
    _hold(case, ref, (cls.cpu().numpy(), reg.cpu().numpy(), mc[:total].cpu().numpy(), al.cpu().numpy()), which)


def test_workspace_too_small_for_the_device_total_writes_nothing():
    case = ar.random_case(2)
    total = sum(tal_ref.atss_ref.valid(b).shape[0] for b in case["boxes"])
    for ws_boxes in (1, total - 1):
        cls, reg, mc, al, _ = _raw_call(case, ws_boxes=ws_boxes)
        assert redzone.unwritten(mc)[0] == mc.numel() and redzone.unwritten(al)[0] == al.numel()
        assert np.array_equal(cls.cpu().numpy(), case["cm"]) and np.array_equal(reg.cpu().numpy(), case["rm"])


def test_wrapper_selects_the_entry_and_fills_a_batch_without_faces(monkeypatch):
    from tinyfaces import ops
    case = ar.random_case(2)
    seen = _spy(monkeypatch)
    out, cm, rm = _operands(case)
    al = torch.full_like(cm, float("nan"))
    ops.tal_assign(out, cm, rm, case["boxes"], case["t"], paste_boxes=case["pastes"], flips=case["flips"], align_out=al)
    assert seen == ["tf_targets_tal_aligned_workspace_bytes", "tf_targets_tal_aligned"]
    del seen[:]
    ops.tal_assign(out, cm, rm, case["boxes"], case["t"], paste_boxes=case["pastes"], flips=case["flips"])
    assert seen == ["tf_targets_tal_workspace_bytes", "tf_targets_tal"]
    del seen[:]
    al = torch.full_like(cm, float("nan"))
    ops.tal_assign(out, cm, rm, [np.zeros((0, 4))] * 3, case["t"], paste_boxes=case["pastes"], flips=case["flips"], align_out=al)
    assert seen == [] and bool((al == 1).all())
    for bad in (al.double(), al[:, :, :, :-1], al[:1], al.cpu()):
        with pytest.raises(ValueError, match="align_out"):
            ops.tal_assign(out, cm, rm, case["boxes"], case["t"], paste_boxes=case["pastes"], flips=case["flips"], align_out=bad)


# ------------------------------------------------------------------------------------------------------------------ the criterion
REG_AND_NORM = [(r, n) for r in ar.REG_LOSSES for n in ar.NORMALIZE]


def _crit(shape, variant, reg_loss, beta, normalize, reg_weight=1.0):
    from tinyfaces import ops
    out, cm, rm, al = ar.loss_case(shape, variant)
    nt = shape[1]
    twh = br.template_wh(nt) if reg_loss == "diou" else None
    loss, grad, npos = ops.criterion_aligned_fwd_bwd(out.cuda(), cm.cuda(), rm.cuda(), al.cuda(), nt, reg_weight, beta, normalize, reg_loss,
                                                     None if twh is None else twh.float())
    return loss.cpu(), grad.cpu(), npos.cpu()


def _hold_loss(shape, variant, reg_loss, beta, normalize):
    out, cm, rm, al = ar.loss_case(shape, variant)
    ref = ar.loss_reference(shape, variant, reg_loss, beta, normalize)
    loss, grad, npos = _crit(shape, variant, reg_loss, beta, normalize)
    kink = br.kink_mask(out, cm, rm, shape[1])
    lr, rc, rr = ar.worst_ratios(loss, grad, ref, kink)
    print(f"aligned {shape} {variant} {reg_loss} beta {beta} {normalize}: loss {lr:.3f}, class gradient {rc:.3f}, regression gradient {rr:.3f} of the bar; "
          f"{int(kink.sum())} of {int((cm == 1).sum())} positives next to a kink")
    assert float(loss[3]) == float(ref["npos"].sum()) and np.array_equal(npos.numpy(), ref["npos"].numpy().astype(np.int32))       # exact
    assert lr <= 1 and rc <= 1 and rr <= 1, (lr, rc, rr)
    assert not bool(grad[:, :][(cm == 0).repeat(1, 5, 1, 1)].any())     # y = 0: all five channels are 0
    return loss, grad


@pytest.mark.parametrize("reg_loss,normalize", REG_AND_NORM)
@pytest.mark.parametrize("shape", ar.LOSS_SHAPES[:4])
def test_criterion_against_the_restatement(shape, reg_loss, normalize):
    """E = 15 up to many blocks, every reg_loss, the three normalisers, beta = 2 and 2.5; align_map values 0, 1, 1.5, -0.5 and NaN on positives,
    random values under the negatives (never read)."""
    for beta in (2.0, 2.5):
        _hold_loss(shape, "drawn", reg_loss, beta, normalize)


@pytest.mark.parametrize("reg_loss", ar.REG_LOSSES)
def test_criterion_on_one_full_map(reg_loss):
    _hold_loss(ar.LOSS_SHAPES[4], "drawn", reg_loss, 2.0, "align")


@pytest.mark.parametrize("variant", ["no_positive", "small_targets"])
@pytest.mark.parametrize("normalize", ar.NORMALIZE)
def test_criterion_images_without_positives_and_the_clamp(variant, normalize):
    """An image without positives, and an image whose targets sum to less than 1: the max(1, .) clamp."""
    for reg_loss in ("smooth_l1", "diou"):
        _hold_loss((2, 25, 9, 9), variant, reg_loss, 2.0, normalize)
        _hold_loss((3, 25, 20, 20), variant, reg_loss, 2.5, normalize)


@pytest.mark.parametrize("reg_loss", ar.REG_LOSSES)
def test_criterion_with_targets_of_one_is_the_focal_kernel(reg_loss):
    """align_map = 1 and "pos": the call agrees within the same bars with ops.criterion_focal_box_fwd_bwd(gamma = beta, alpha = -1), an existing
    kernel serving as a second yardstick."""
    from tinyfaces import ops
    for shape, beta in (((2, 25, 9, 9), 2.0), ((3, 25, 20, 20), 2.5)):
        out, cm, rm, al = ar.loss_case(shape, "ones")
        nt = shape[1]
        twh = br.template_wh(nt).float() if reg_loss == "diou" else None
        loss, grad, _ = _crit(shape, "ones", reg_loss, beta, "pos")
        l2, g2, _ = ops.criterion_focal_box_fwd_bwd(out.cuda(), cm.cuda(), rm.cuda(), nt, 1.0, beta, -1.0, "pos", reg_loss, twh)
        ref = ar.loss_reference(shape, "ones", reg_loss, beta, "pos")
        assert torch.allclose(loss[:2], l2.cpu(), rtol=1e-5, atol=0) and float(loss[2]) == float(loss[3])
        r = (grad.double() - g2.cpu().double()).abs() / ar.bars(ref)
        kink = br.kink_mask(out, cm, rm, nt)
        r[:, nt:] = torch.where(kink.repeat(1, 4, 1, 1), torch.zeros_like(r[:, nt:]), r[:, nt:])
        assert float(r.max()) <= 1, float(r.max())


def test_criterion_mutants_of_the_restatement_fail():
    """Regression not weighted by q, npos in place of the sum of q, q from the own box: each fails the bars the kernel passes."""
    shape = (2, 25, 9, 9)
    out, cm, rm, al = ar.loss_case(shape, "drawn")
    loss, grad = _hold_loss(shape, "drawn", "diou", 2.0, "align")
    for mutant in ar.LOSS_MUTANTS:
        bad = ar.aligned_loss(out, cm, rm, al, 25, "diou", br.template_wh(25), 2.0, "align", mutant=mutant)
        assert max(ar.worst_ratios(loss, grad, bad, br.kink_mask(out, cm, rm, 25))) > 1, mutant


def test_criterion_two_runs_give_identical_bits_and_reg_weight_scales_the_box_gradient():
    for shape, reg_loss, normalize in (((3, 25, 20, 20), "diou", "align"), ((1, 25, 63, 63), "smooth_l1", "align"), ((3, 16, 8, 8), "giou", "pos")):
        a, b = _crit(shape, "drawn", reg_loss, 2.0, normalize), _crit(shape, "drawn", reg_loss, 2.0, normalize)
        assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        c = _crit(shape, "drawn", reg_loss, 2.0, normalize, reg_weight=4.0)
        nt = shape[1]
        assert torch.equal(c[0], a[0]) and torch.equal(c[1][:, :nt], a[1][:, :nt]) and torch.allclose(c[1][:, nt:], 4.0 * a[1][:, nt:], rtol=1e-6, atol=0)


def test_criterion_guard_bands_and_a_gradient_written_completely():
    """tf_criterion_aligned_fwd_bwd called directly with every operand and the workspace between guard bands; grad_out, loss_out and npos_out arrive
    NaN-filled and are written completely."""
    from tinyfaces import _hip
    dev = torch.device("cuda")
    for shape, form in (((3, 25, 20, 20), 3), ((1, 1, 3, 5), 0)):
        out, cm, rm, al = ar.loss_case(shape, "drawn")
        B, nt, H, W = shape
        g = lambda a: redzone.guarded_like(a.contiguous(), dev)
        o, c, r, a_, twh = g(out), g(cm), g(rm), g(al), g(br.template_wh(nt).float())
        grad, loss, npos = redzone.guarded(out.shape, torch.float32, dev), redzone.guarded((4,), torch.float64, dev), redzone.guarded((B,), torch.int32, dev)
        l, p = _hip.lib(), _hip.ptr
        wsb = l.tf_criterion_aligned_workspace_bytes(B, nt, H, W)
        ws = redzone.guarded_workspace(wsb, dev)
        assert l.tf_criterion_aligned_fwd_bwd(p(o), p(c), p(r), p(a_), B, nt, H, W, 2.0, 2, 1.0, form, p(twh), p(grad), p(loss), p(npos), p(ws), wsb, _hip.stream()) == 0
        torch.cuda.synchronize()
        for name, x in dict(output=o, class_map=c, reg_map=r, align_map=a_, template_wh=twh, grad=grad, loss=loss, npos=npos, workspace=ws).items():
            redzone.assert_guards(x, name)
        for name, x in dict(grad=grad, loss=loss, npos=npos).items():
            redzone.assert_written(x, what=name)
        want = _crit(shape, "drawn", ("smooth_l1", "iou", "giou", "diou")[form], 2.0, "align")
        assert torch.equal(grad.cpu(), want[1]) and torch.equal(loss.cpu(), want[0])
        assert all(torch.equal(x.cpu(), y) for x, y in ((o, out), (c, cm), (r, rm)))          # only read


# ------------------------------------------------------------------------------------------------ the criterion module, the engine, main.py
def _spy(monkeypatch):
    from tinyfaces import _hip, ops
    seen, real = [], _hip.lib()

    class Spy:
        def __getattr__(self, name):
            seen.append(name)
            return getattr(real, name)

    monkeypatch.setattr(ops, "lib", lambda: Spy())
    return seen


def _spy_calls(monkeypatch, names):
    """Record (name, args, kwargs) of the named ops functions as the criterion calls them."""
    from tinyfaces import ops
    calls = []
    for n in names:
        real = getattr(ops, n)
        monkeypatch.setattr(ops, n, (lambda n_, real_: lambda *a, **k: (calls.append((n_, a, k)), real_(*a, **k))[1])(n, real))
    return calls


def test_default_call_is_the_old_call(templates, monkeypatch):
    """With aligned_targets=False the criterion makes the calls it made, argument for argument: tal_assign_device without align_out,
    criterion_quality_fwd_bwd with its ten positional arguments; and the library entries are the old ones."""
    from tinyfaces.datasets import TargetAssigner
    from tinyfaces.models.loss import DetectionCriterion, TaskAligned
    g = torch.Generator().manual_seed(0)
    out = (torch.randn(2, 125, 9, 11, generator=g) * 0.3).cuda()
    boxes = _faces_for(2, (9, 11), 3)
    assigner = TargetAssigner(templates, heatmap_size=(9, 11), assigner="tal")
    cm0, rm0, faces = assigner(boxes, paste_boxes=[[0, 0, 88, 72]] * 2, device="cuda")
    faces.stats = None
    calls = _spy_calls(monkeypatch, ("tal_assign_device", "criterion_quality_fwd_bwd", "criterion_aligned_fwd_bwd"))
    seen = _spy(monkeypatch)
    crit = DetectionCriterion(25, cls_loss="qfl", reg_loss="diou", templates=templates, assigner=TaskAligned(9, 0.5, 4.0))
    cm, rm = cm0.clone(), rm0.clone()
    crit(out.clone().requires_grad_(True), cm, rm, faces=faces).backward()
    assert [c[0] for c in calls] == ["tal_assign_device", "criterion_quality_fwd_bwd"]
    (_, a, k), (_, a2, k2) = calls
    assert len(a) == 14 and a[1] is cm and a[2] is rm and a[3] is faces.boxes_d and a[7] is None and a[11:] == (9, 0.5, 4.0) and k == {"return_match_count": False}
    assert len(a2) == 9 and a2[1] is cm and a2[2] is rm and a2[3:8] == (25, 1, 2.0, "pos", "diou") and k2 == {}
    assert seen == ["tf_targets_tal_workspace_bytes", "tf_targets_tal", "tf_criterion_quality_workspace_bytes", "tf_criterion_quality_fwd_bwd"]
    assert crit._align_map is None
    # ... and with aligned_targets=True the new ones
    del calls[:], seen[:]
    crit = DetectionCriterion(25, cls_loss="qfl", reg_loss="diou", templates=templates, assigner=TaskAligned(9, 0.5, 4.0, aligned_targets=True),
                              focal_normalize="align", qfl_beta=2.5)
    cm, rm = cm0.clone(), rm0.clone()
    crit(out.clone().requires_grad_(True), cm, rm, faces=faces).backward()
    assert [c[0] for c in calls] == ["tal_assign_device", "criterion_aligned_fwd_bwd"]
    assert calls[0][2]["align_out"] is crit._align_map and calls[1][1][3] is crit._align_map and crit._align_map.shape == cm.shape
    assert calls[1][1][4:9] == (25, 1, 2.5, "align", "diou")
    assert seen == ["tf_targets_tal_aligned_workspace_bytes", "tf_targets_tal_aligned", "tf_criterion_aligned_workspace_bytes", "tf_criterion_aligned_fwd_bwd"]
    first = crit._align_map
    crit(out.clone().requires_grad_(True), cm0.clone(), rm0.clone(), faces=faces)
    assert crit._align_map is first                                    # the buffer is kept
    v = crit._loss2.tolist()
    assert crit.quality_average.num_averaged == 2 * int(v[3]) and abs(crit.quality_average.average - v[2] / v[3]) < 1e-12       # the mean target


def _tal_engine(templates, aligned=True, assign=True, **kw):
    """ResNet-50, frozen BatchNorm, fp32, qfl + diou on the golden trainer batches (2 x 2 images); deterministic weight gradients."""
    import dist_worker_trunks
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models.loss import DetectionCriterion, TaskAligned
    m, _, batches = dist_worker_trunks.build(os.path.join(ROOT, "tests", "golden", "trainer.npz"))
    m.freeze_batchnorm()
    c = DetectionCriterion(25, cls_loss="qfl", reg_loss="diou", focal_normalize="align" if aligned else "pos", templates=templates, lazy_meters=True,
                           assigner=TaskAligned(aligned_targets=aligned) if assign else None)
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
    """TrainEngine.step_with_faces with qfl + diou, aligned_targets=True and "align" equals, bit for bit, the backward pass from the gradient
    ops.criterion_aligned_fwd_bwd returns for maps and align_map made by hand (ops.tal_assign(align_out=)) from the same forward output: the loss
    vector, and the flat gradient against an engine whose criterion is handed that very gradient."""
    from tinyfaces import ops
    from tinyfaces.datasets import TargetAssigner
    tal, imgs, hm = _tal_engine(templates)
    plain, _, _ = _tal_engine(templates, aligned=False, assign=False)
    img = imgs[0]
    H, W = img.shape[2:]
    boxes = _faces_for(img.shape[0], hm, 1)
    paste = [[0, 0, W, H]] * img.shape[0]
    assigner = TargetAssigner(templates, heatmap_size=hm, assigner="tal")
    cm0, rm0, faces = assigner(boxes, paste_boxes=paste, device="cuda")
    outs = []
    fwd = tal.model._run_forward
    tal.model._run_forward = lambda x, training=True: (lambda o: (outs.append(o.detach().clone()), o)[1])(fwd(x, training=training))
    cm1, rm1 = cm0.clone(), rm0.clone()
    loss1 = tal.step_with_faces(img, cm1, rm1, faces).clone()
    g1 = tal.model._grad_flat_persistent.clone()
    al2 = torch.full_like(cm0, float("nan"))
    cm2, rm2, mc = ops.tal_assign(outs[0].float().contiguous(), cm0.clone(), rm0.clone(), boxes, templates, paste_boxes=paste, return_match_count=True,
                                  align_out=al2)
    assert torch.equal(cm1, cm2) and torch.equal(rm1, rm2) and int((cm2 == 1).sum()) == int(mc.sum()) > 0
    assert torch.equal(tal.criterion._align_map, al2) and float(al2[cm2 == 1].max()) <= 1 and float(al2[cm2 == 1].min()) >= 0
    # the plain engine's criterion is made to return the aligned pass on the hand-made maps
    crit = plain.criterion
    crit._fwd_bwd = lambda out, cm, rm, want_labels=False, faces=None: ops.criterion_aligned_fwd_bwd(
        out, cm, rm, al2, 25, crit.reg_weight, crit.qfl_beta, "align", "diou", crit._template_wh_on(out.device))[:2] + (cm,)
    loss2 = plain.step(img, cm2, rm2)
    torch.cuda.synchronize()
    assert torch.equal(loss1, loss2) and float(loss1[3]) == float(mc.sum()) and 0 < float(loss1[2]) < float(loss1[3])
    assert torch.equal(g1.view(torch.int32), plain.model._grad_flat_persistent.view(torch.int32)) and float(g1.abs().sum()) > 0
    tal.close()
    plain.close()


def test_engine_a_window_of_two_micro_batches_against_the_batch_of_their_four_images(templates):
    """Under frozen BatchNorm an image's forward output does not depend on its batch, the assignment is per image, and every normaliser of the
    aligned loss ("align": the image's own sum of targets) is per image.  So the accumulated gradient of (b0, b1) is the gradient of [b0; b1] up to
    the summation order of the weight gradients: relative L2 below 1e-6, the bar QFL (3.3e-8) and TAL (3.0e-8) are held to.  Printed and reported."""
    from gpu_util import report
    from test_gpu_grad_accum import _trained_mask
    from tinyfaces.datasets import TargetAssigner
    acc, imgs, hm = _tal_engine(templates, accum_steps=2)
    big, _, _ = _tal_engine(templates)
    H, W = imgs[0].shape[2:]
    boxes = _faces_for(4, hm, 2)
    assigner = TargetAssigner(templates, heatmap_size=hm, assigner="tal")
    won, al = [], []
    for k in range(2):
        cm, rm, faces = assigner(boxes[2 * k:2 * k + 2], paste_boxes=[[0, 0, W, H]] * 2, device="cuda")
        acc.step_with_faces(imgs[k], cm, rm, faces)
        won.append(cm == 1)
        al.append(acc.criterion._align_map.clone())
    cm, rm, faces = assigner(boxes, paste_boxes=[[0, 0, W, H]] * 4, device="cuda")
    big.step_with_faces(torch.cat(imgs), cm, rm, faces)
    torch.cuda.synchronize()
    assert (acc.steps, acc.micro_steps, big.steps) == (1, 2, 1)
    same_assignment = bool(torch.equal(torch.cat(won), cm == 1))
    same_targets = bool(torch.equal(torch.cat(al), big.criterion._align_map))
    mk, _ = _trained_mask(acc.model)
    mk = mk.cuda()
    ga, gb = acc.model._grad_flat_persistent[mk].double(), big.model._grad_flat_persistent[mk].double()
    rel = float((ga - gb).norm() / gb.norm())
    print(f"tal aligned engine: accumulated vs 4-image gradient rel L2 {rel:.3g} (QFL on loader-side maps: 3.3e-8, TAL + QFL: 3.0e-8); same positives in "
          f"both: {same_assignment}; same aligned targets: {same_targets}; positives {int((cm == 1).sum())}")
    report("tal_aligned_engine_window_vs_big_batch[resnet50,fp32,frozen,qfl,diou,align]", grad_rel_l2=rel, same_assignment=same_assignment,
           same_targets=same_targets, positives=int((cm == 1).sum()))
    assert same_assignment and same_targets and float(gb.norm()) > 0 and rel < 1e-6, rel
    acc.close()
    big.close()


def test_main_trains_two_epochs_with_the_aligned_targets(tmp_path):
    """main.py --assigner tal --cls-loss qfl --tal-aligned-targets --focal-normalize align on synthetic-faces: two short epochs; the start-up lines
    say the new thing in words, the quality line reports the mean aligned target, no Epoch line holds a nan or an inf, and the checkpoint records
    the flag under "args"."""
    import re
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(PKG, "main.py"), "synthetic-faces", "synthetic-faces", "--epochs", "2", "--save-every", "1",
                        "--synthetic-len", "8", "--batch_size", "4", "--lr", "1e-5", "--cls-loss", "qfl", "--reg-loss", "diou", "--assigner", "tal",
                        "--tal-aligned-targets", "--focal-normalize", "align"], cwd=tmp_path, capture_output=True, text=True, timeout=400, env=env)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    print(r.stdout[-3000:])
    assert "Epoch: [0][1/2]" in r.stdout and "Epoch: [1][1/2]" in r.stdout
    assert "aligned target m / max m * max IoU" in r.stdout and "task-aligned quality focal" in r.stdout and "by the sum of its aligned targets" in r.stdout
    values = [float(v) for v in re.findall(r"mean aligned target of positives ([0-9.eE+-]+)", r.stdout)]
    assert values and all(0.0 <= v <= 1.0 for v in values) and "mean IoU of positives" not in r.stdout, values
    assert re.findall(r"TAL: (\d+) of (\d+) faces won at most 3 positives", r.stdout)
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("Epoch:") and ("nan" in ln.lower() or "inf" in ln.lower())]
    state = torch.load(tmp_path / "weights" / "checkpoint_2.pth", map_location="cpu", weights_only=False)
    assert state["args"]["assigner"] == "tal" and state["args"]["tal_aligned_targets"] is True and state["args"]["focal_normalize"] == "align"
