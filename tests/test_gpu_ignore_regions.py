"""-m gpu: the ignore regions (tf_targets_apply_ignore, csrc/targets_ignore.hip) against tests/ignore_ref.py, the numpy restatement of the
rule in include/tinyfaces_hip.h on top of oracle.targets.  Every case is one small launch, held to: the class map array_equal to the
reference (three values, no tolerance), the per-image counters equal to the reference's, every +1 and 0 of the plain call still there, the
regression map bit for bit the map of the plain call."""
import numpy as np
import pytest
import torch

import comp_ref
import ignore_ref
import loss_cases as lc
import redzone
from oracle import targets as otgt
from test_gpu_compensation import T3, _faces

pytestmark = pytest.mark.gpu

RF = otgt.RF
T16 = np.array([[-7.5, -7.5, 7.5, 7.5, 1.0]])                       # one 16 x 16 template
DEGENERATE = np.array([[10.0, 12.0, 10.0, 40.0], [30.0, 20.0, 50.0, 20.0], [40.0, 40.0, 35.0, 60.0]])
NO_PASTE = [-10 ** 6, -10 ** 6, 10 ** 6, 10 ** 6]


def _hwc(x):
    return x.cpu().numpy().transpose(0, 2, 3, 1)


def _plain_reference(boxes, t, hm, pastes, flips, noise):
    """Per image the class map (HWC) the three phases leave, from the oracle."""
    return [lc.oracle_maps(lc.valid(bx), t, pastes[b] if pastes is not None else NO_PASTE, flips[b] if flips is not None else 0, noise[b], hm=hm)[0]
            for b, bx in enumerate(boxes)]


def _hold(name, cm, rm, ic, cm0, rm0, base, ign, t, hm, ignore):
    """cm / rm / ic of a call with ignore boxes against: `base` (per image, the reference map in front of the pass), the plain call cm0 / rm0."""
    got = _hwc(cm)
    want_counts = []
    for b, F in enumerate(base):
        want, n = ignore_ref.apply_ignore(F, t, ign[b], ignore[0], ignore[1], RF, hm)
        assert np.array_equal(got[b], want), f"{name}: image {b}: {int((got[b] != want).sum())} labels differ from the rule"
        want_counts.append(n)
    assert ic.dtype == torch.int32 and ic.shape == (len(base),) and ic.cpu().tolist() == want_counts, f"{name}: changed = {ic.cpu().tolist()}, rule {want_counts}"
    assert torch.equal(rm, rm0), f"{name}: the regression map changed"
    assert bool((cm[cm0 == 1] == 1).all()) and bool((cm[cm0 == 0] == 0).all()), f"{name}: a +1 or a 0 of the plain call changed"
    return want_counts


def _run(boxes, ign, t, hm, pastes, flips, noise, ignore, name=""):
    from tinyfaces import ops
    kw = dict(heatmap_size=hm, paste_boxes=pastes, flips=flips, noise=noise)
    cm0, rm0 = ops.dense_overlap_targets(boxes, t, **kw)
    cm, rm, ic = ops.dense_overlap_targets(boxes, t, ignore_boxes=ign, ignore=ignore, return_ignored_count=True, **kw)
    base = _plain_reference(boxes, t, hm, pastes, flips, noise)
    for b, F in enumerate(base):
        assert np.array_equal(_hwc(cm0)[b], F), f"{name}: image {b}: the plain class map differs from the oracle"
    counts = _hold(name, cm, rm, ic, cm0, rm0, base, ign, t, hm, ignore)
    return cm0, cm, ic, counts


GRID = [(hm, nt, k) for hm in ((5, 7), (9, 13)) for nt in (1, 3) for k in (0, 1, 2, 255, 256, 257, 513)]


@pytest.mark.parametrize("ci", range(len(GRID)))
def test_small_maps_box_counts_batches_and_measures(ci):
    """5 x 7 and 9 x 13 maps, 1 and 3 templates, K = 0 .. 513 ignore boxes around the LDS tile of 256 (plus degenerate ones that are dropped);
    1 to 3 images, the one without ignore boxes first, in the middle or last; both measures; plain, padded, padded and flipped."""
    hm, nt, K = GRID[ci]
    rng = np.random.RandomState(900 + ci)
    t = T3[:nt]
    B = 1 + ci % 3
    empty = (ci // 3) % B if B > 1 else -1                              # which image has no ignore boxes
    boxes = [_faces(rng, 3 + b, hm, t) for b in range(B)]
    ign = []
    for b in range(B):
        k = 0 if b == empty else (K if b == (empty + 1) % B or B == 1 else 5)
        r = _faces(rng, k, hm, t)
        ign.append(np.concatenate([DEGENERATE[:1], r[: k // 2], DEGENERATE[1:], r[k // 2:]]) if k else (DEGENERATE if b % 2 else np.zeros((0, 4))))
        assert lc.valid(ign[-1]).shape[0] == k
    noise = [rng.rand(hm[0], hm[1], nt, lc.valid(bx).shape[0]) for bx in boxes]
    paste = [6, 4, 8 * hm[1] - 9, 8 * hm[0] - 5]
    pastes, flips = [(None, None), ([paste] * B, [0] * B), ([paste] * B, [(b + 1) % 2 for b in range(B)])][ci % 3]
    ignore = (("iof", 0.5), ("iou", 0.3), ("iof", 0.25), ("iou", 0.5))[ci % 4]
    _, _, _, counts = _run(boxes, ign, t, hm, pastes, flips, noise, ignore, name=f"grid[{hm},{nt},{K},B={B}]")
    if empty >= 0:
        assert counts[empty] == 0
    if K >= 255:
        assert sum(counts) > 0                                          # the pass did something


def _one_anchor(box, ignore, cell=(2, 3)):
    """One ignore box on the all-negative 5 x 7 map of the 16 x 16 template; returns the label of `cell` afterwards (the whole map is held too)."""
    hm = (5, 7)
    none = [np.zeros((0, 4))]
    _, cm, ic, counts = _run(none, [np.array([box], dtype=np.float64)], T16, hm, None, None, [np.zeros((5, 7, 1, 0))], ignore, name=f"box {box} {ignore}")
    return float(cm[0, 0, cell[0], cell[1]])


def test_on_the_threshold():
    """The anchor of cell (2, 3) is [15.5, 7.5, 30.5, 22.5], 16 x 16 = 256 pixels."""
    half = [15.5, 7.5, 30.5, 14.5]                                      # its upper 8 rows: ia = 128, ov = 0.5 exactly
    assert _one_anchor(half, ("iof", 0.5)) == 0.0
    assert _one_anchor(half, ("iof", float(np.nextafter(0.5, 1)))) == -1.0
    assert _one_anchor(half, ("iou", 0.5)) == 0.0                       # the box lies inside the anchor: the union is the anchor
    assert _one_anchor(half, ("iou", float(np.nextafter(0.5, 1)))) == -1.0
    same = [15.5, 7.5, 30.5, 22.5]                                      # the anchor itself at thresh = 1.0
    assert _one_anchor(same, ("iof", 1.0)) == 0.0 and _one_anchor(same, ("iou", 1.0)) == 0.0
    assert _one_anchor([15.5, 7.5, 30.5, 22.0], ("iou", 1.0)) == -1.0   # half a row short
    assert _one_anchor([10.0, 0.0, 40.0, 30.0], ("iof", 1.0)) == 0.0    # a box around it: IoF 1, IoU 256 / 961
    assert _one_anchor([10.0, 0.0, 40.0, 30.0], ("iou", 0.3)) == -1.0
    tiny = float(np.nextafter(0.0, 1.0))
    for touching in ([31.5, 7.5, 60.0, 22.5], [15.5, 23.5, 30.5, 60.0], [0.0, 7.5, 14.5, 22.5]):      # iw == 0 or ih == 0
        assert _one_anchor(touching, ("iof", tiny)) == -1.0 and _one_anchor(touching, ("iou", tiny)) == -1.0
    corner = [30.5, 22.5, 60.0, 60.0]                                   # the one pixel the +1 convention counts: iw = ih = 1
    assert _one_anchor(corner, ("iof", 1.0 / 256)) == 0.0
    assert _one_anchor(corner, ("iof", float(np.nextafter(1.0 / 256, 1)))) == -1.0


def test_positives_and_ignored_labels_survive(templates):
    """Ignore boxes laid over real faces on the 63 x 63 map: every +1 and every 0 of the plain call is still there, the regression map is the
    plain call's, and negatives around the faces were turned."""
    m = lc.mixed_batch()
    ign = [np.concatenate([lc.valid(b), lc.valid(b) + 6.0]) if lc.valid(b).shape[0] else np.array([[40.0, 50.0, 200.0, 260.0]]) for b in m["boxes"]]
    cm0, cm, ic, counts = _run(m["boxes"], ign, templates, (63, 63), m["paste"], m["flips"], m["noise"], ("iof", 0.5), name="over the faces")
    assert int((cm0 == 1).sum()) > 0 and int((cm == 1).sum()) == int((cm0 == 1).sum()) and sum(counts) > 0
    assert int((cm == 0).sum()) == int((cm0 == 0).sum()) + sum(counts) and int((cm == -1).sum()) == int((cm0 == -1).sum()) - sum(counts)


def test_composes_with_the_compensation_stage(templates):
    """compensate=(3, 0.1) together with ignore boxes = the rule applied to comp_ref's compensated map; match_count is the compensated call's."""
    from tinyfaces import ops
    rng = np.random.RandomState(77)
    s = rng.uniform(8, 40, 12)
    x, y = rng.uniform(0, 500 - s), rng.uniform(0, 500 - s)
    small = np.round(np.stack([x, y, x + 0.8 * s, y + s], 1), 3)
    boxes = [small, np.zeros((0, 4)), lc.mixed_batch()["boxes"][0]]
    pastes, flips = [[0, 0, 500, 500], [7, 3, 250, 333], [91, 93, 491, 493]], [1, 0, 1]
    noise = [np.random.RandomState(900 + b).rand(63, 63, 25, lc.valid(bx).shape[0]) for b, bx in enumerate(boxes)]
    ign = [small[:6] + np.array([-6.0, -6.0, 6.0, 6.0]), np.array([[100.0, 100.0, 180.0, 200.0]]), np.zeros((0, 4))]
    kw = dict(paste_boxes=pastes, flips=flips, noise=noise, compensate=(3, 0.1), return_match_count=True)
    cmc, rmc, mc0 = ops.dense_overlap_targets(boxes, templates, **kw)
    out = ops.dense_overlap_targets(boxes, templates, ignore_boxes=ign, ignore=("iof", 0.5), return_ignored_count=True, **kw)
    assert len(out) == 4
    cm, rm, mc, ic = out
    base = [comp_ref.compensated_maps(lc.valid(bx), templates, pastes[b], flips[b], noise[b], 3, 0.1)[1] for b, bx in enumerate(boxes)]
    counts = _hold("composition", cm, rm, ic, cmc, rmc, base, ign, templates, (63, 63), ("iof", 0.5))
    assert torch.equal(mc, mc0) and sum(counts) > 0
    out = ops.dense_overlap_targets(boxes, templates, ignore_boxes=ign, paste_boxes=pastes, flips=flips, noise=noise, compensate=(3, 0.1))
    assert len(out) == 2 and torch.equal(out[0], cm)                    # the tuple grows only when a return_* keyword asks for it


def test_entry_points_agree(templates):
    """The resident entry point equals the list entry point; targets_apply_ignore on the plain map equals the fused keyword; the default pair."""
    from tinyfaces import ops
    m = lc.mixed_batch()
    ign = [np.array([[60.0 + 30 * b, 80.0, 180.0 + 30 * b, 240.0], [300.0, 310.0 - 20 * b, 420.0, 470.0]]) if b % 2 == 0 else np.zeros((0, 4)) for b in range(6)]
    kw = dict(paste_boxes=m["paste"], flips=m["flips"], seed=5)
    cm0, rm0 = ops.dense_overlap_targets(m["boxes"], templates, **kw)
    cm, rm, ic = ops.dense_overlap_targets(m["boxes"], templates, ignore_boxes=ign, ignore=("iou", 0.2), return_ignored_count=True, **kw)
    assert torch.equal(rm, rm0) and int(ic.sum()) > 0 and ic.cpu().tolist()[1::2] == [0, 0, 0]
    # the list entry point twice: the same bits
    cm2, rm2, ic2 = ops.dense_overlap_targets(m["boxes"], templates, ignore_boxes=ign, ignore=("iou", 0.2), return_ignored_count=True, **kw)
    assert torch.equal(cm, cm2) and torch.equal(rm, rm2) and torch.equal(ic, ic2)
    # the stand-alone pass on the plain map
    mine = cm0.clone()
    got, n = ops.targets_apply_ignore(mine, ign, templates, ignore=("iou", 0.2), return_count=True)
    assert got is mine and torch.equal(mine, cm) and torch.equal(n, ic)
    assert ops.targets_apply_ignore(cm0.clone(), ign, templates, ignore=("iou", 0.2)).shape == cm.shape
    # ignore_boxes without ignore= uses ("iof", 0.5)
    d1 = ops.dense_overlap_targets(m["boxes"], templates, ignore_boxes=ign, **kw)
    d2 = ops.dense_overlap_targets(m["boxes"], templates, ignore_boxes=ign, ignore=("iof", 0.5), **kw)
    assert len(d1) == 2 and torch.equal(d1[0], d2[0]) and torch.equal(d1[0], ops.targets_apply_ignore(cm0.clone(), ign, templates))
    # the resident entry point
    kept = [lc.valid(b) for b in m["boxes"]]
    offs = np.cumsum([0] + [k.shape[0] for k in kept])
    ioffs = np.cumsum([0] + [k.shape[0] for k in ign])
    r = dict(boxes_d=torch.from_numpy(np.concatenate(kept)).cuda(), offs_d=torch.tensor(offs, dtype=torch.int32).cuda(), total_boxes=int(offs[-1]),
             templates_d=torch.from_numpy(np.ascontiguousarray(templates)).cuda(), paste_d=torch.tensor(m["paste"], dtype=torch.int32).cuda(),
             flips_d=torch.tensor(m["flips"], dtype=torch.int32).cuda(), seed=5)
    i = dict(ignore_d=torch.from_numpy(np.concatenate(ign)).cuda(), ignore_offs_d=torch.tensor(ioffs, dtype=torch.int32).cuda(), total_ignore=int(ioffs[-1]))
    dcm, drm, dic = ops.dense_overlap_targets_device(ignore=("iou", 0.2), return_ignored_count=True, **r, **i)
    assert torch.equal(dcm, cm) and torch.equal(drm, rm) and torch.equal(dic, ic)
    out = ops.dense_overlap_targets_device(ignore=("iou", 0.2), **r, **i)
    assert len(out) == 2 and torch.equal(out[0], cm)
    out = ops.dense_overlap_targets_device(compensate=(3, 0.1), return_match_count=True, return_ignored_count=True, **r, **i)
    assert len(out) == 4 and out[2].dtype == torch.int32 and out[3].shape == (6,)
    plain = ops.dense_overlap_targets_device(**r)
    assert len(plain) == 2 and torch.equal(plain[0], cm0) and torch.equal(plain[1], rm0)
    # no ignore box in the whole batch: the plain maps, zero counters
    ecm, erm, eic = ops.dense_overlap_targets(m["boxes"], templates, ignore_boxes=[np.zeros((0, 4))] * 6, return_ignored_count=True, **kw)
    assert torch.equal(ecm, cm0) and torch.equal(erm, rm0) and eic.dtype == torch.int32 and eic.cpu().tolist() == [0] * 6


def _raw_call(cm_start, ign, t, hm, measure, thresh, count=True):
    """tf_targets_apply_ignore called directly, every operand between guard bands.  Returns (rc, class map, counter)."""
    from tinyfaces import _hip
    dev = torch.device("cuda")
    kept = [lc.valid(b) for b in ign]
    offs = np.cumsum([0] + [k.shape[0] for k in kept]).astype(np.int32)
    total, (B, nt, vsy, vsx) = int(offs[-1]), cm_start.shape
    g = lambda a: redzone.guarded_like(torch.from_numpy(np.ascontiguousarray(a)), dev)
    cls = redzone.guarded_like(cm_start.cpu(), dev)
    ign_d = g(np.concatenate(kept) if total else np.zeros((1, 4)))
    offs_d, t_d = g(offs), g(np.asarray(t, dtype=np.float64))
    changed = g(np.zeros(B, dtype=np.int32))
    p = _hip.ptr
    rc = _hip.lib().tf_targets_apply_ignore(p(cls), B, nt, vsy, vsx, p(t_d), t.shape[1], -1, -1, 8, 8, p(ign_d) if total else None, p(offs_d), measure, thresh,
                                            p(changed) if count else None, _hip.stream())
    torch.cuda.synchronize()
    for name, x in dict(class_map=cls, ignore_boxes=ign_d, ignore_offsets=offs_d, templates=t_d, changed=changed).items():
        redzone.assert_guards(x, name)
    return rc, cls, changed


@pytest.mark.parametrize("which", ["small", "golden"])
def test_contract_guard_bands_and_refusals(templates, which):
    from tinyfaces import ops
    rng = np.random.RandomState(11)
    if which == "small":
        hm, t = (9, 13), T3
        boxes = [_faces(rng, 4, hm, t), np.zeros((0, 4)), _faces(rng, 6, hm, t)]
        ign = [_faces(rng, 300, hm, t), np.zeros((0, 4)), np.concatenate([DEGENERATE, _faces(rng, 7, hm, t)])]
        pastes, flips = [[0, 0, 104, 72], [3, 3, 90, 60], [6, 4, 95, 67]], [0, 1, 1]
    else:
        hm, t = (63, 63), templates
        boxes = [lc.mixed_batch()["boxes"][0], lc.mixed_batch()["boxes"][3]]
        ign = [np.array([[10.0, 20.0, 300.0, 280.0], [350.0, 300.0, 520.0, 505.0]]), np.array([[100.0, 60.0, 260.0, 230.0]])]
        pastes, flips = [[0, 0, 500, 500], [91, 93, 491, 493]], [1, 0]
    noise = [rng.rand(hm[0], hm[1], t.shape[0], lc.valid(b).shape[0]) for b in boxes]
    cm0, _ = ops.dense_overlap_targets(boxes, t, heatmap_size=hm, paste_boxes=pastes, flips=flips, noise=noise)
    base = _plain_reference(boxes, t, hm, pastes, flips, noise)
    for measure, name in ((0, "iof"), (1, "iou")):
        rc, cls, changed = _raw_call(cm0, ign, t, hm, measure, 0.4)
        assert rc == 0 and changed.dtype == torch.int32
        want = [ignore_ref.apply_ignore(F, t, ign[b], name, 0.4, RF, hm) for b, F in enumerate(base)]
        for b, (w, n) in enumerate(want):
            assert np.array_equal(_hwc(cls)[b], w) and int(changed[b]) == n
        assert sum(n for _, n in want) > 0
        rc2, cls2, changed2 = _raw_call(cm0, ign, t, hm, measure, 0.4)                 # the same bits on every run
        assert rc2 == 0 and torch.equal(cls2, cls) and torch.equal(changed2, changed)
        rc3, cls3, changed3 = _raw_call(cm0, ign, t, hm, measure, 0.4, count=False)    # NULL counter: the same map, nothing counted
        assert rc3 == 0 and torch.equal(cls3, cls) and not bool(changed3.any())
    # refused before any launch, the map untouched
    for thresh in (0.0, 1.5, float("nan")):
        rc, cls, changed = _raw_call(cm0, ign, t, hm, 0, thresh)
        assert rc == -1 and torch.equal(cls, cm0) and not bool(changed.any())
        mine = cm0.clone()
        with pytest.raises(ValueError):
            ops.targets_apply_ignore(mine, ign, t, ignore=("iof", thresh))
        assert torch.equal(mine, cm0)
    rc, cls, changed = _raw_call(cm0, ign, t, hm, 2, 0.5)
    assert rc == -1 and torch.equal(cls, cm0)
    # no ignore box at all: nothing is enqueued, nothing changes
    rc, cls, changed = _raw_call(cm0, [np.zeros((0, 4))] * len(ign), t, hm, 0, 0.5)
    assert rc == 0 and torch.equal(cls, cm0) and not bool(changed.any())


def test_default_call_is_the_old_call(templates, monkeypatch):
    """Without the keywords the wrappers make the library calls they made: tf_targets_apply_ignore is never reached."""
    from tinyfaces import _hip, ops
    m = lc.mixed_batch()
    real = _hip.lib()
    seen = []

    class Spy:
        def __getattr__(self, name):
            seen.append(name)
            return getattr(real, name)

    want = ops.dense_overlap_targets(m["boxes"], templates, paste_boxes=m["paste"], flips=m["flips"], seed=9)
    monkeypatch.setattr(ops, "lib", lambda: Spy())
    got = ops.dense_overlap_targets(m["boxes"], templates, paste_boxes=m["paste"], flips=m["flips"], seed=9)
    assert seen == ["tf_targets_workspace_bytes", "tf_dense_overlap_targets"] and len(got) == 2
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    del seen[:]
    ops.dense_overlap_targets(m["boxes"], templates, paste_boxes=m["paste"], flips=m["flips"], seed=9, ignore=("iof", 0.5))      # a pair without boxes: nothing to do
    assert seen == ["tf_targets_workspace_bytes", "tf_dense_overlap_targets"]
    del seen[:]
    ops.dense_overlap_targets(m["boxes"], templates, paste_boxes=m["paste"], flips=m["flips"], seed=9, ignore_boxes=[np.array([[5.0, 5.0, 90.0, 90.0]])] * 6)
    assert seen == ["tf_targets_workspace_bytes", "tf_dense_overlap_targets", "tf_targets_apply_ignore"]


def test_wider_tree_with_and_without_the_policy(tmp_path, capsys):
    """A miniature WIDER tree whose annotations carry an invalid and a blur-2 record.  With ignore_policy the batch equals the same steps done
    by hand through ignore_ref; without it the batch is today's: same seed, torch.equal on all three tensors."""
    from types import SimpleNamespace
    from PIL import Image
    from test_oracle_augment import synth_image
    from tinyfaces import ops, trainer, transforms
    from tinyfaces.datasets import augment as da
    from tinyfaces.datasets import get_dataloader
    root = tmp_path / "WIDER_train" / "images" / "0--Parade"
    root.mkdir(parents=True)
    ann, imgs = "", {}
    for k, (H, W) in enumerate([(600, 800), (420, 380), (700, 1000)]):
        name = f"0--Parade/img{k}.png"
        arr = synth_image(40 + k, H, W)
        Image.fromarray(arr, "RGB").save(tmp_path / "WIDER_train" / "images" / name)          # PNG: lossless, decode == arr
        imgs[name] = arr
        ann += (f"{name}\n4\n{50 + 10 * k} {60 + 5 * k} 120 150 0 0 0 0 0 0\n{200 + k} {180 + k} 40 48 0 0 0 1 0 0\n"
                f"{120 + k} {250 + k} 60 70 2 0 0 0 0 0\n{260 + k} {90 + k} 50 64 1 0 0 0 1 0\n")
    ann_file = tmp_path / "train.txt"
    ann_file.write_text(ann)
    args = SimpleNamespace(batch_size=3, workers=0, dataset_root=str(tmp_path), debug=False)
    tf = transforms.Compose([transforms.ToTensor(), transforms.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])])
    policy = da.IgnorePolicy(invalid=True, blur=2, truncated=True)

    def decisions(d):
        """process_inputs' draws for one sample from the global generator, by hand."""
        H, W = imgs[d["img_path"]].shape[:2]
        rnd = np.random.rand()
        z = 0.5 if rnd < 1 / 3 else (2.0 if rnd > 2 / 3 else 1.0)
        crop, paste, _ = da.crop_decisions(int(z * H), int(z * W), np.zeros((0, 4)))
        return z, crop, paste, bool(np.random.rand() > 0.5)

    # without the policy: today's batch
    loader, templates = get_dataloader(ann_file, args, img_transforms=tf, train=False, split="train")
    assert loader.dataset.ignore_policy is None and loader.dataset.ignore_stats is None and len(loader.dataset[0]) == 2
    np.random.seed(123)
    (x0, cm0, rm0), = list(loader)
    np.random.seed(123)
    hand = [da.process_inputs(torch.from_numpy(imgs[d["img_path"]]).cuda(), d["bboxes"]) for d in loader.dataset.data]
    hcm, hrm = ops.dense_overlap_targets([h[1] for h in hand], templates, paste_boxes=[h[2] for h in hand], flips=[int(h[3]) for h in hand], seed=1)
    assert torch.equal(x0, torch.stack([h[0] for h in hand])) and torch.equal(cm0, hcm) and torch.equal(rm0, hrm)
    # with it
    loader, _ = get_dataloader(ann_file, args, img_transforms=tf, train=False, split="train", ignore_policy=policy, ignore=("iof", 0.4))
    ds = loader.dataset
    assert ds.ignore_policy == policy and ds.ignore == ("iof", 0.4) and len(ds[0]) == 3 and ds[0][2]["invalid"].tolist() == [0, 1, 0, 0]
    np.random.seed(123)
    (x, cm, rm), = list(loader)
    assert torch.equal(x, x0)                                           # the pixels do not know the policy
    np.random.seed(123)
    faces, ign, pastes, flips = [], [], [], []
    for d in ds.data:
        z, crop, paste, flip = decisions(d)
        f, i = ignore_ref.policy_boxes(d["bboxes"] * z, d, policy, crop, paste, flip)
        faces.append(f); ign.append(i); pastes.append(paste); flips.append(int(flip))
    assert all(f.shape[0] <= 2 for f in faces) and sum(i.shape[0] for i in ign) > 0      # the invalid and the blur-2 record own no positive
    pcm, prm = ops.dense_overlap_targets(faces, templates, paste_boxes=pastes, flips=flips, seed=1)
    assert torch.equal(rm, prm)
    got, plain = _hwc(cm), _hwc(pcm)
    counts = []
    for b in range(3):
        want, n = ignore_ref.apply_ignore(plain[b], templates, ign[b], "iof", 0.4)
        assert np.array_equal(got[b], want), b
        counts.append(n)
    assert sum(counts) > 0
    trainer.print_ignore(0, 0, 1, loader)
    line = capsys.readouterr().out.splitlines()[-1]
    assert line == (f"Epoch: [0][0/1]\tignore regions: {sum(counts) / 3:.1f} anchors per image turned from negative to ignored, "
                    f"{100.0 * sum(c > 0 for c in counts) / 3:.0f} % of 3 images with any")
    # together with the compensation stage: the loader runs, and both counters arrive
    loader, _ = get_dataloader(ann_file, args, img_transforms=tf, train=False, split="train", ignore_policy=policy, anchor_compensation=(3, 0.1))
    np.random.seed(123)
    (x2, cm2, rm2), = list(loader)
    assert torch.equal(x2, x0) and torch.equal(rm2, rm) and loader.dataset.ignore == ("iof", 0.5)
    assert loader.dataset.compensation_stats.pop() is not None and loader.dataset.ignore_stats.pop()[0] == 3
