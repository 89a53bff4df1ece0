"""-m gpu: csrc/targets.hip (tf_dense_overlap_targets) against oracle.targets run one image at a time, beyond the one square golden
geometry: maps that are not square and other template counts, one call over a mixed batch, exact ties, seed mode, and the
resident-operand entry point.  The bars are those of test_gpu_small_ops.py::test_targets_vs_reference_golden: labels identical,
tx / ty bit-equal, tw / th within rtol 2e-7 with at most max(1, size // 100000) entries differing at all.
tests/test_loss_front_end_fixtures.py shows on the CPU that every case here can tell its bug apart."""
import numpy as np
import pytest
import torch

import loss_cases as lc
from gpu_util import report

pytestmark = pytest.mark.gpu


def _hwc(x):
    return x.cpu().numpy().transpose(0, 2, 3, 1)


def _check_image(name, cm, rm, boxes, t, paste, flip, noise, hm=(63, 63), rf=lc.RF):
    """One image's maps (HWC) against the oracle run on that image alone."""
    ocm, orm, _ = lc.oracle_maps(boxes, t, paste, flip, noise, hm, rf)
    cls_mismatch = int((cm != ocm).sum())
    reg_differ = int((rm != orm.astype(np.float32)).sum())
    report(name, cls_mismatch=cls_mismatch, reg_differ=reg_differ, positives=int((ocm == 1).sum()), zeros=int((ocm == 0).sum()))
    assert cls_mismatch == 0, name
    lc.assert_regression(rm, orm, name)


@pytest.mark.parametrize("ci", range(14))
def test_targets_off_square_maps_and_other_template_counts(templates, ci):
    from tinyfaces import ops
    from oracle import targets as otgt
    c = lc.geometry_cases(templates)[ci]
    t, b, (vsy, vsx), rf = c["t"], c["boxes"], c["hm"], c["rf"]
    (ofy, ofx), (sty, stx) = rf["offset"], rf["stride"]
    iou = ops.dense_overlap_iou(b, t, heatmap_size=c["hm"], rf=rf).cpu().numpy()
    ref_iou = otgt.dense_overlap(ofx, ofy, stx, sty, vsx, vsy, t[:, 0], t[:, 1], t[:, 2], t[:, 3], b[:, 0], b[:, 1], b[:, 2], b[:, 3])
    assert iou.shape == ref_iou.shape and np.array_equal(iou, ref_iou)          # float64, bit-exact
    cm, rm = ops.dense_overlap_targets([b], t, heatmap_size=c["hm"], rf=rf, paste_boxes=[c["paste"]], flips=[c["flip"]], noise=[c["noise"]])
    assert cm.shape == (1, c["nt"], vsy, vsx) and rm.shape == (1, 4 * c["nt"], vsy, vsx)
    _check_image(f"targets_geometry[{c['name']}]", _hwc(cm)[0], _hwc(rm)[0], b, t, c["paste"], c["flip"], c["noise"], c["hm"], rf)


def test_targets_mixed_batch_in_one_call(templates):
    from tinyfaces import ops
    m = lc.mixed_batch()
    cm, rm = ops.dense_overlap_targets(m["boxes"], templates, paste_boxes=m["paste"], flips=m["flips"], noise=m["noise"])
    for b in range(6):
        _check_image(f"targets_mixed_batch[{b}]", _hwc(cm)[b], _hwc(rm)[b], m["boxes"][b], templates, m["paste"][b], m["flips"][b], m["noise"][b])
    for b in (1, 2, 5):                                                          # no box, or none that survives: nothing to learn from
        assert bool((cm[b] == -1).all()) and not bool(rm[b].any())
    # the same images in reversed order: the reversed result, bit for bit
    cm2, rm2 = ops.dense_overlap_targets(m["boxes"][::-1], templates, paste_boxes=m["paste"][::-1], flips=m["flips"][::-1], noise=m["noise"][::-1])
    assert torch.equal(cm2, cm.flip(0)) and torch.equal(rm2, rm.flip(0))


def test_targets_exact_ties_take_the_first(templates):
    from tinyfaces import ops
    c = lc.tie_case()
    cm, rm = ops.dense_overlap_targets([c["boxes"]], templates, paste_boxes=[c["paste"]], flips=[c["flip"]], noise=[c["noise"]])
    _, _, iou = lc.oracle_maps(c["boxes"], templates, c["paste"], c["flip"], c["noise"])
    anchor_ties, box_ties = lc.tie_counts(iou)
    report("targets_ties", anchors_with_tied_boxes=anchor_ties, boxes_with_tied_best_anchor=box_ties)
    _check_image("targets_ties_maps", _hwc(cm)[0], _hwc(rm)[0], c["boxes"], templates, c["paste"], c["flip"], c["noise"])


def _resident(m, templates):
    kept = [lc.valid(b) for b in m["boxes"]]
    offs = np.cumsum([0] + [k.shape[0] for k in kept])
    boxes_d = torch.from_numpy(np.concatenate(kept) if offs[-1] else np.zeros((1, 4))).cuda()
    return dict(boxes_d=boxes_d, offs_d=torch.tensor(offs, dtype=torch.int32).cuda(), total_boxes=int(offs[-1]),
                templates_d=torch.from_numpy(np.ascontiguousarray(templates)).cuda(),
                paste_d=torch.tensor(m["paste"], dtype=torch.int32).cuda(), flips_d=torch.tensor(m["flips"], dtype=torch.int32).cuda())


def _check_seed_mode_batch(name, cm, rm, m, templates):
    cm, rm = _hwc(cm), _hwc(rm)
    tot = lc.seed_mode_totals()
    for b in range(len(m["boxes"])):
        lc.check_seed_mode_image(cm[b], rm[b], m["boxes"][b], templates, m["paste"][b], m["flips"][b], tot, f"{name} image {b}")
    report(name, **tot)
    assert tot["unexplained"] == 0, tot
    assert tot["settled"] > 1000                               # (an anchor that overlaps no box is not: the noise picks its box)


def test_targets_seed_mode_regression_and_labels(templates):
    """What every training step runs: the tie-break noise comes from the device's counter RNG, in [0, 1e-6).  A label may differ from
    the noiseless oracle's only within 1e-6 of a threshold or where a box's best anchor is contested within 1e-6; a box's unique
    best anchor may not."""
    from tinyfaces import ops
    m = lc.mixed_batch()
    cm, rm = ops.dense_overlap_targets(m["boxes"], templates, paste_boxes=m["paste"], flips=m["flips"], seed=5)
    _check_seed_mode_batch("targets_seed_mode", cm, rm, m, templates)


def test_targets_device_entry(templates):
    """ops.dense_overlap_targets_device: what bench.py and the training step call."""
    from tinyfaces import ops
    m = lc.mixed_batch()
    cm, rm = ops.dense_overlap_targets(m["boxes"], templates, paste_boxes=m["paste"], flips=m["flips"], seed=5)
    r = _resident(m, templates)
    dcm, drm = ops.dense_overlap_targets_device(seed=5, **r)
    assert torch.equal(dcm, cm) and torch.equal(drm, rm)
    assert int((cm == 1).sum()) > 0
    # a second call into the same out= pair with another batch: no trace of the first
    o = lc.other_batch()
    ocm, orm = ops.dense_overlap_targets(o["boxes"], templates, paste_boxes=o["paste"], flips=o["flips"], seed=6)
    assert not torch.equal(ocm, cm)
    out = ops.dense_overlap_targets_device(seed=6, out=(dcm, drm), **_resident(o, templates))
    assert out[0] is dcm and out[1] is drm
    assert torch.equal(dcm, ocm) and torch.equal(drm, orm)
    _check_seed_mode_batch("targets_device_entry_reused_out", dcm, drm, o, templates)      # ... by the oracle too, not the kernel alone
    # no box in the whole batch
    e = _resident(dict(boxes=[np.zeros((0, 4))] * 6, paste=m["paste"], flips=m["flips"]), templates)
    assert e["total_boxes"] == 0
    ops.dense_overlap_targets_device(seed=7, out=(dcm, drm), **e)
    assert bool((dcm == -1).all()) and not bool(drm.any())
    report("targets_device_entry", bit_equal=True, positives=int((cm == 1).sum()))
