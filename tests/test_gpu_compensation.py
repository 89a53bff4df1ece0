"""-m gpu: the scale-compensated anchor matching (tf_dense_overlap_targets_comp, csrc/targets.hip) against tests/comp_ref.py, the numpy
restatement of the rule in include/tinyfaces_hip.h on top of oracle.targets.  Every case is one small launch, held to: the class map
array_equal to the reference (three values, no tolerance), match_count equal to the reference's counts, the regression map bit for bit
the map of the uncompensated call on the same operands."""
import numpy as np
import pytest
import torch

import comp_ref
import loss_cases as lc
import redzone
from oracle import targets as otgt

pytestmark = pytest.mark.gpu

RF = otgt.RF
# small template sets for the small maps (x1, y1, x2, y2, scale): 17 x 21, 9 x 11 and 33 x 41 pixels
T3 = np.array([[-8.0, -10.0, 8.0, 10.0, 1.0], [-4.0, -5.0, 4.0, 5.0, 1.0], [-16.0, -20.0, 16.0, 20.0, 1.0]])


def _hwc(x):
    return x.cpu().numpy().transpose(0, 2, 3, 1)


def _reference(boxes, t, hm, pastes, flips, noise, N, T, neg=0.3, pos=0.7):
    """Per image (plain class map, compensated class map, counts), from the rule."""
    out = []
    for b, bx in enumerate(boxes):
        paste = pastes[b] if pastes is not None else [-10 ** 6, -10 ** 6, 10 ** 6, 10 ** 6]
        flip = flips[b] if flips is not None else 0
        cm, F, _, counts = comp_ref.compensated_maps(lc.valid(bx), t, paste, flip, noise[b], N, T, hm=hm, pos_thresh=pos, neg_thresh=neg)
        out.append((cm, F, counts))
    return out


def _run(boxes, t, hm, pastes, flips, noise, N, T, neg=0.3, pos=0.7, name=""):
    """One compensated call + the uncompensated call on the same operands, held to the three bars.  Returns (reference, cm, mc)."""
    from tinyfaces import ops
    kw = dict(heatmap_size=hm, paste_boxes=pastes, flips=flips, noise=noise, pos_thresh=pos, neg_thresh=neg)
    cm0, rm0 = ops.dense_overlap_targets(boxes, t, **kw)
    cm, rm, mc = ops.dense_overlap_targets(boxes, t, compensate=(N, T), return_match_count=True, **kw)
    ref = _reference(boxes, t, hm, pastes, flips, noise, N, T, neg, pos)
    assert torch.equal(rm, rm0), f"{name}: the regression map changed"
    got0, got = _hwc(cm0), _hwc(cm)
    for b, (pcm, F, _) in enumerate(ref):
        assert np.array_equal(got0[b], pcm), f"{name}: image {b}: the uncompensated class map differs from the oracle"
        assert np.array_equal(got[b], F), f"{name}: image {b}: {int((got[b] != F).sum())} labels differ from the rule"
    want = np.concatenate([r[2] for r in ref]) if ref else np.zeros(0, np.int32)
    assert mc.dtype == torch.int32 and np.array_equal(mc.cpu().numpy(), want), f"{name}: match_count"
    return ref, cm, mc


def _faces(rng, g, hm, t):
    """g faces on the map: tiny ones (only a forced anchor, or nothing, is positive), copies of a template on a cell (count >= N), faces at a
    corner, hanging over the canvas, larger than the map, and overlapping pairs that compete for owners."""
    vsy, vsx = hm
    W, H = 8.0 * vsx, 8.0 * vsy
    out = []
    for i in range(g):
        kind = i % 6
        if kind == 0:                                             # tiny
            w, h = rng.uniform(4, 9, 2)
            x, y = rng.uniform(0, W - 8), rng.uniform(0, H - 8)
        elif kind == 1:                                           # a template, centred on a cell
            k = t[int(rng.randint(0, t.shape[0]))]
            cx, cy = -1 + 8 * int(rng.randint(0, vsx)), -1 + 8 * int(rng.randint(0, vsy))
            out.append([cx + k[0], cy + k[1], cx + k[2], cy + k[3]])
            continue
        elif kind == 2:                                           # at a corner / hanging over the canvas
            w, h = rng.uniform(6, 30, 2)
            x, y = rng.choice([-w / 2, W - w / 2, -2.0]), rng.choice([-h / 2, H - h / 2, -2.0])
        elif kind == 3:                                           # larger than the map
            w, h = W * rng.uniform(1.1, 1.6), H * rng.uniform(1.1, 1.6)
            x, y = -rng.uniform(0, w - W), -rng.uniform(0, h - H)
        elif kind == 4 and out:                                   # overlapping the previous face
            p = out[-1]
            dx, dy = rng.uniform(-4, 4, 2)
            out.append([p[0] + dx, p[1] + dy, p[2] + dx, p[3] + dy])
            continue
        else:                                                     # anything
            w, h = rng.uniform(5, 40, 2)
            x, y = rng.uniform(-5, W - 5), rng.uniform(-5, H - 5)
        out.append([x, y, x + w, y + h])
    return np.round(np.array(out, dtype=np.float64).reshape(-1, 4), 3)


GRID = [(hm, nt, g) for hm in ((5, 7), (9, 13)) for nt in (1, 3) for g in (0, 1, 2, 63, 64, 65, 257)]


@pytest.mark.parametrize("ci", range(len(GRID)))
def test_small_maps_box_counts_and_parameters(ci):
    """5 x 7 and 9 x 13 maps, 1 and 3 templates, 0 .. 257 boxes; N in {1, 3, 64} (64 exceeds the candidates of most faces), T below, on and
    above neg_thresh; with and without padding and flip."""
    hm, nt, g = GRID[ci]
    rng = np.random.RandomState(500 + ci)
    t = T3[:nt]
    boxes = [_faces(rng, g, hm, t)]
    noise = [rng.rand(hm[0], hm[1], nt, lc.valid(boxes[0]).shape[0])]
    N, T = (1, 3, 64)[ci % 3], (0.1, 0.3, 0.5)[(ci // 3) % 3]
    pastes, flips = [None, ([[6, 4, 8 * hm[1] - 9, 8 * hm[0] - 5]], [0]), ([[6, 4, 8 * hm[1] - 9, 8 * hm[0] - 5]], [1])][ci % 3] or (None, None)
    ref, cm, mc = _run(boxes, t, hm, pastes, flips, noise, N, T, name=f"grid[{hm},{nt},{g}]")
    if g >= 63 and T < 0.5:
        assert int((ref[0][1] != ref[0][0]).sum()) > 0                  # the stage did something


def test_golden_templates_batch_with_empty_images_and_its_reverse(templates):
    """63 x 63, the 25 golden templates, five images with the empty ones first, in the middle and last; the reversed batch gives the
    reversed maps and counts."""
    rng = np.random.RandomState(77)
    s = rng.uniform(8, 40, 12)
    x, y = rng.uniform(0, 500 - s), rng.uniform(0, 500 - s)
    small = np.round(np.stack([x, y, x + 0.8 * s, y + s], 1), 3)
    none = np.zeros((0, 4))
    boxes = [none, small, none, lc.mixed_batch()["boxes"][0], none]
    pastes = [[0, 0, 500, 500], [0, 0, 500, 500], [7, 3, 250, 333], [91, 93, 491, 493], [0, 0, 500, 500]]
    flips = [0, 1, 0, 1, 1]
    noise = [np.random.RandomState(900 + b).rand(63, 63, 25, lc.valid(bx).shape[0]) for b, bx in enumerate(boxes)]
    ref, cm, mc = _run(boxes, templates, (63, 63), pastes, flips, noise, 3, 0.1, name="golden batch")
    assert int((ref[1][1] != ref[1][0]).sum()) > 0
    _, cm2, mc2 = _run(boxes[::-1], templates, (63, 63), pastes[::-1], flips[::-1], noise[::-1], 3, 0.1, name="golden batch reversed")
    assert torch.equal(cm2, cm.flip(0))
    assert np.array_equal(mc2.cpu().numpy(), np.concatenate([r[2] for r in ref[::-1]]))


@pytest.mark.parametrize("B", [1, 2, 3, 4, 5])
def test_batches_of_one_to_five_images(B):
    rng = np.random.RandomState(40 + B)
    hm = (9, 13)
    boxes = [np.zeros((0, 4)) if (b + B) % 3 == 0 else _faces(rng, 5 + b, hm, T3) for b in range(B)]
    noise = [rng.rand(9, 13, 3, lc.valid(bx).shape[0]) for bx in boxes]
    pastes = [[2 * b, 3, 100 - b, 70] for b in range(B)]
    flips = [b % 2 for b in range(B)]
    ref, cm, mc = _run(boxes, T3, hm, pastes, flips, noise, 3, 0.1, name=f"batch {B}")
    _, cm2, _ = _run(boxes[::-1], T3, hm, pastes[::-1], flips[::-1], noise[::-1], 3, 0.1, name=f"batch {B} reversed")
    assert torch.equal(cm2, cm.flip(0))


def test_only_the_middle_image_is_under_matched(templates):
    """What resetting the whole map, or recomputing the regression, would break: images 0 and 2 hold faces equal to a template on a cell
    (count >= N: nothing to do), image 1 one tiny face."""
    k = templates[12]
    full = np.array([[-1 + 8 * 30 + k[0], -1 + 8 * 25 + k[1], -1 + 8 * 30 + k[2], -1 + 8 * 25 + k[3]]])
    tiny = np.array([[201.0, 303.0, 210.0, 314.0]])
    boxes = [full, tiny, full + 16.0]
    noise = [np.random.RandomState(60 + b).rand(63, 63, 25, 1) for b in range(3)]
    ref, cm, mc = _run(boxes, templates, (63, 63), [[0, 0, 500, 500]] * 3, [0, 0, 0], noise, 3, 0.1, name="middle image")
    for b in (0, 2):
        assert np.array_equal(ref[b][0], ref[b][1]) and ref[b][2][0] >= 3
    assert int((ref[1][0] == 1).sum()) <= 1 and int((ref[1][1] == 1).sum()) == 3


def test_best_planted_exactly_on_the_threshold():
    """best(a) == T is a candidate (>=), the next double above it is not: explicit noise, one face, one template."""
    hm, t = (5, 7), T3[:1]
    box = np.array([[20.0, 9.0, 26.0, 17.0]])                          # 7 x 9 under a 17 x 21 template: IoU < 0.3, no forced anchor
    noise = [np.full((5, 7, 1, 1), 0.5)]
    iou = otgt.dense_overlap(-1, -1, 8, 8, 7, 5, t[:, 0], t[:, 1], t[:, 2], t[:, 3], box[:, 0], box[:, 1], box[:, 2], box[:, 3])
    v = np.unique(iou + 1e-6 * noise[0])[::-1]
    assert 0.01 < v[1] < v[0] < 0.3                                     # two distinct levels below neg_thresh
    on = float(v[1])
    ref, _, mc = _run([box], t, hm, None, None, noise, 64, on, name="best == T")
    assert int(mc[0]) == int((iou + 1e-6 * noise[0] >= on).sum()) >= 2
    above = float(np.nextafter(on, 1.0))
    ref2, _, mc2 = _run([box], t, hm, None, None, noise, 64, above, name="best just below T")
    assert int(mc2[0]) < int(mc[0])


def test_ties_go_to_the_lower_flat_index():
    """All-zero noise, a face centred between two cells: both anchors see the same best.  With no forced anchor (IoU below neg_thresh) and
    N = 1 the lower flat index is promoted; with a forced anchor (the first arg-max) and N = 2 the stage adds the other one."""
    hm, t = (5, 7), T3[:1]
    cx, cy = -1 + 8 * 3 + 4.0, -1 + 8 * 2                                # midway between cells x = 3 and x = 4 of row 2
    for (hw, hh), N, T in (((3.0, 4.0), 1, 0.05), ((8.0, 10.0), 2, 0.2)):
        box = np.array([[cx - hw, cy - hh, cx + hw, cy + hh]])
        noise = [np.zeros((5, 7, 1, 1))]
        ref, cm, mc = _run([box], t, hm, None, None, noise, N, T, name=f"tie {hw}")
        pcm, F, counts = ref[0]
        iou = otgt.dense_overlap(-1, -1, 8, 8, 7, 5, t[:, 0], t[:, 1], t[:, 2], t[:, 3], box[:, 0], box[:, 1], box[:, 2], box[:, 3])[..., 0]
        assert iou[2, 3, 0] == iou[2, 4, 0] == iou.max()                 # the tie is real
        assert int(counts[0]) == N and F[2, 3, 0] == 1
        assert (F[2, 4, 0] == 1) == (N == 2)
        assert int((pcm == 1).sum()) == N - 1


def _raw_call(boxes, t, hm, pastes, flips, noise, N, T, neg=0.3, pos=0.7, seed=0):
    """tf_dense_overlap_targets_comp called directly, every operand and the workspace between guard bands; class map, regression map and
    match_count arrive filled with 0xFF (NaN / -1)."""
    from tinyfaces import _hip
    dev = torch.device("cuda")
    kept = [lc.valid(b) for b in boxes]
    offs = np.cumsum([0] + [k.shape[0] for k in kept]).astype(np.int32)
    total, B, (vsy, vsx), nt = int(offs[-1]), len(boxes), hm, t.shape[0]
    g = lambda a: redzone.guarded_like(torch.from_numpy(np.ascontiguousarray(a)), dev)
    boxes_d = g(np.concatenate(kept) if total else np.zeros((1, 4)))
    offs_d, t_d = g(offs), g(np.asarray(t, dtype=np.float64))
    paste_d = g(np.asarray(pastes, dtype=np.int32).reshape(B, 4))
    flips_d = g(np.asarray(flips, dtype=np.int32))
    noise_d = noff_d = None
    if noise is not None:
        noise_d = g(np.concatenate([n.reshape(-1) for n in noise] + [np.zeros(1)]))
        noff_d = g(np.cumsum([0] + [n.size for n in noise]).astype(np.int64))
    cls = redzone.guarded((B, nt, vsy, vsx), torch.float32, dev)
    reg = redzone.guarded((B, 4 * nt, vsy, vsx), torch.float32, dev)
    mc = redzone.guarded((max(total, 1),), torch.int32, dev)
    l = _hip.lib()
    wsb = l.tf_targets_comp_workspace_bytes(total, B, nt, vsy, vsx)
    ws = redzone.guarded_workspace(wsb, dev)
    p = _hip.ptr
    rc = l.tf_dense_overlap_targets_comp(p(boxes_d), p(offs_d), B, p(t_d), nt, t.shape[1], vsy, vsx, -1, -1, 8, 8, p(paste_d), p(flips_d), p(noise_d),
                                         p(noff_d), seed, pos, neg, N, T, p(mc), p(cls), p(reg), p(ws), wsb, _hip.stream())
    assert rc == 0
    torch.cuda.synchronize()
    for name, x in dict(boxes=boxes_d, offsets=offs_d, templates=t_d, paste=paste_d, flips=flips_d, class_map=cls, reg_map=reg, match_count=mc,
                        workspace=ws, **({} if noise is None else dict(noise=noise_d, noise_offsets=noff_d))).items():
        redzone.assert_guards(x, name)
    redzone.assert_written(cls, what="class_map")
    redzone.assert_written(reg, what="reg_map")
    if total:
        redzone.assert_written(mc, what="match_count")
    else:
        assert int(mc[0]) == -1                                          # no face: nothing to write
    return cls, reg, mc[:total]


@pytest.mark.parametrize("which", ["small", "golden"])
def test_guard_bands_and_garbage_outputs(templates, which):
    rng = np.random.RandomState(5)
    if which == "small":
        hm, t = (9, 13), T3
        boxes = [_faces(rng, 9, hm, t), np.zeros((0, 4)), _faces(rng, 65, hm, t)]
        pastes, flips = [[0, 0, 104, 72], [3, 3, 90, 60], [6, 4, 95, 67]], [0, 1, 1]
    else:
        hm, t = (63, 63), templates
        s = rng.uniform(8, 30, 7)
        x, y = rng.uniform(0, 470, 7), rng.uniform(0, 470, 7)
        boxes = [np.round(np.stack([x, y, x + 0.8 * s, y + s], 1), 3), lc.mixed_batch()["boxes"][0]]
        pastes, flips = [[0, 0, 500, 500], [91, 93, 491, 493]], [1, 0]
    noise = [rng.rand(hm[0], hm[1], t.shape[0], lc.valid(b).shape[0]) for b in boxes]
    cls, reg, mc = _raw_call(boxes, t, hm, pastes, flips, noise, 3, 0.1)
    ref = _reference(boxes, t, hm, pastes, flips, noise, 3, 0.1)
    got = _hwc(cls)
    for b, (_, F, _) in enumerate(ref):
        assert np.array_equal(got[b], F)
    assert np.array_equal(mc.cpu().numpy(), np.concatenate([r[2] for r in ref]))
    from tinyfaces import ops
    _, rm0 = ops.dense_overlap_targets(boxes, t, heatmap_size=hm, paste_boxes=pastes, flips=flips, noise=noise)
    assert torch.equal(reg, rm0)
    # no box in the whole batch: every label -1, nothing else touched
    cls, reg, mc = _raw_call([np.zeros((0, 4))] * 2, t, hm, pastes[:2], flips[:2], None, 3, 0.1)
    assert bool((cls == -1).all()) and not bool(reg.any())


def test_resident_entry_and_seed_mode(templates):
    """The resident-operand entry against the list entry, and seed mode twice: the same bits."""
    from tinyfaces import ops
    m = lc.mixed_batch()
    rng = np.random.RandomState(3)
    s = rng.uniform(8, 30, 9)
    x, y = rng.uniform(0, 470, 9), rng.uniform(0, 470, 9)
    m["boxes"][1] = np.round(np.stack([x, y, x + 0.8 * s, y + s], 1), 3)
    kw = dict(paste_boxes=m["paste"], flips=m["flips"], seed=5, compensate=(3, 0.1), return_match_count=True)
    cm, rm, mc = ops.dense_overlap_targets(m["boxes"], templates, **kw)
    cm2, rm2, mc2 = ops.dense_overlap_targets(m["boxes"], templates, **kw)
    assert torch.equal(cm, cm2) and torch.equal(rm, rm2) and torch.equal(mc, mc2)
    cm0, rm0 = ops.dense_overlap_targets(m["boxes"], templates, paste_boxes=m["paste"], flips=m["flips"], seed=5)
    assert torch.equal(rm, rm0)
    grown = (cm == 1) & (cm0 != 1)
    assert int(grown.sum()) > 0 and not bool(((cm != cm0) & ~grown).any())          # promotions only
    kept = [lc.valid(b) for b in m["boxes"]]
    offs = np.cumsum([0] + [k.shape[0] for k in kept])
    r = dict(boxes_d=torch.from_numpy(np.concatenate(kept)).cuda(), offs_d=torch.tensor(offs, dtype=torch.int32).cuda(), total_boxes=int(offs[-1]),
             templates_d=torch.from_numpy(np.ascontiguousarray(templates)).cuda(), paste_d=torch.tensor(m["paste"], dtype=torch.int32).cuda(),
             flips_d=torch.tensor(m["flips"], dtype=torch.int32).cuda())
    dcm, drm, dmc = ops.dense_overlap_targets_device(seed=5, compensate=(3, 0.1), return_match_count=True, **r)
    assert torch.equal(dcm, cm) and torch.equal(drm, rm) and torch.equal(dmc, mc)
    out = ops.dense_overlap_targets_device(seed=5, compensate=(3, 0.1), **r)
    assert len(out) == 2 and torch.equal(out[0], cm)
    # the seeded noise is below 1e-6: against the noiseless rule only labels within 1e-6 of a threshold or a tie may differ; the counts of
    # faces whose candidates are not contested that closely are the rule's
    assert int(mc.min()) >= 0 and int(mc.numel()) == int(offs[-1])


def test_default_call_is_the_old_call(templates, hip):
    """compensate=None: the wrapper makes the call it always made -- bit for bit what tf_dense_overlap_targets gives when called directly."""
    from tinyfaces import ops
    m = lc.mixed_batch()
    out = ops.dense_overlap_targets(m["boxes"], templates, paste_boxes=m["paste"], flips=m["flips"], seed=9, compensate=None)
    assert len(out) == 2
    kept = [lc.valid(b) for b in m["boxes"]]
    offs = np.cumsum([0] + [k.shape[0] for k in kept])
    boxes_d, offs_d = torch.from_numpy(np.concatenate(kept)).cuda(), torch.tensor(offs, dtype=torch.int32).cuda()
    t_d = torch.from_numpy(np.ascontiguousarray(templates)).cuda()
    paste_d, flips_d = torch.tensor(m["paste"], dtype=torch.int32).cuda(), torch.tensor(m["flips"], dtype=torch.int32).cuda()
    cls, reg = torch.empty_like(out[0]), torch.empty_like(out[1])
    l = hip.lib()
    wsb = l.tf_targets_workspace_bytes(int(offs[-1]))
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    p = hip.ptr
    assert l.tf_dense_overlap_targets(p(boxes_d), p(offs_d), 6, p(t_d), 25, 5, 63, 63, -1, -1, 8, 8, p(paste_d), p(flips_d), None, None, 9, 0.7, 0.3,
                                      p(cls), p(reg), p(ws), wsb, hip.stream()) == 0
    assert torch.equal(out[0], cls) and torch.equal(out[1], reg)
    with pytest.raises(ValueError):
        ops.dense_overlap_targets(m["boxes"], templates, return_match_count=True)


def test_synthetic_faces_and_one_engine_step(templates, capsys):
    """SyntheticFaces(anchor_compensation=(3, 0.1)): at least as many positives per image as without it, more in total; one fused step with
    ResNet-50, frozen BatchNorm and the focal criterion normalised by positives returns a finite loss."""
    from tinyfaces.datasets import SyntheticFaces
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as zoo
    from tinyfaces.models.loss import DetectionCriterion
    plain = SyntheticFaces(templates, length=2, seed=0)
    comp = SyntheticFaces(templates, length=2, seed=0, anchor_compensation=(3, 0.1))
    img0, cm0, rm0 = plain.collate([plain[0], plain[1]])
    img, cm, rm = comp.collate([comp[0], comp[1]])
    p0, p1 = (cm0 == 1).sum(dim=(1, 2, 3)), (cm == 1).sum(dim=(1, 2, 3))
    assert bool((p1 >= p0).all()) and int(p1.sum()) > int(p0.sum())
    assert torch.equal(rm, rm0) and torch.equal(img, img0)
    # the counters the training loop prints next to the loss meters: nothing without the stage, one line with it, and then they are read
    from types import SimpleNamespace
    from tinyfaces import trainer
    trainer.print_compensation(0, 0, 1, SimpleNamespace(dataset=plain))
    assert plain.compensation_stats is None and capsys.readouterr().out == ""
    trainer.print_compensation(0, 0, 1, SimpleNamespace(dataset=comp), lag=1)          # the only batch is still "in flight"
    assert capsys.readouterr().out == ""
    trainer.print_compensation(0, 0, 1, SimpleNamespace(dataset=comp))
    line = capsys.readouterr().out
    faces = sum(len(comp[i][1]) for i in range(2))
    assert line.startswith("Epoch: [0][0/1]\tanchor compensation: ") and f" of {faces} faces hold at most N = 3 positives" in line
    assert comp.compensation_stats.pop() is None
    m = zoo.DetectionModel(base_model=zoo.resnet50, num_templates=25).set_compute_dtype(torch.bfloat16)
    m.freeze_batchnorm(True)
    eng = TrainEngine(m, DetectionCriterion(25, cls_loss="focal", focal_normalize="pos"), lr=1e-4, momentum=0.9, weight_decay=5e-4, device="cuda")
    loss = eng.step(img.float(), cm, rm)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(torch.as_tensor(loss)).all())
    eng.close()
