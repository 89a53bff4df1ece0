"""Reference of the ignore regions: the rule of tf_targets_apply_ignore (include/tinyfaces_hip.h) and the augmentation policy of
datasets/augment.py (IgnorePolicy), in numpy.  `apply_ignore` works on the HWC class map oracle.targets.get_heatmaps (or tests/comp_ref.py)
leaves; `policy_boxes` repeats the bookkeeping of process_inputs from the scale draw on, given the decisions that were drawn.
Nothing here touches the GPU."""
import numpy as np

from oracle import targets as otgt


def coverage(templates, ignore_boxes, measure, rf=otgt.RF, hm=otgt.HEATMAP_SIZE):
    """ov[y, x, t, k] of the rule, in its operation order (plain float64, one rounding per operation)."""
    ofy, ofx = rf["offset"]
    sty, stx = rf["stride"]
    vsy, vsx = hm
    t = np.asarray(templates, dtype=np.float64)
    r = np.asarray(ignore_boxes, dtype=np.float64).reshape(-1, 4)
    nt, K = t.shape[0], r.shape[0]
    cx = (ofx + np.arange(vsx) * (stx / 1)).reshape(1, vsx, 1, 1)
    cy = (ofy + np.arange(vsy) * (sty / 1)).reshape(vsy, 1, 1, 1)
    d = lambda a: a.reshape(1, 1, nt, 1)
    g = lambda a: a.reshape(1, 1, 1, K)
    ax1, ay1, ax2, ay2 = d(t[:, 0]) + cx, d(t[:, 1]) + cy, d(t[:, 2]) + cx, d(t[:, 3]) + cy
    farea = d((t[:, 2] - t[:, 0] + 1) * (t[:, 3] - t[:, 1] + 1))
    rarea = g((r[:, 2] - r[:, 0] + 1) * (r[:, 3] - r[:, 1] + 1))
    iw = np.minimum(ax2, g(r[:, 2])) - np.maximum(ax1, g(r[:, 0])) + 1
    ih = np.minimum(ay2, g(r[:, 3])) - np.maximum(ay1, g(r[:, 1])) + 1
    ia = iw * ih
    if measure == "iof":
        den = np.broadcast_to(farea, ia.shape)
    elif measure == "iou":
        den = farea + rarea - ia
    else:
        raise ValueError(measure)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((iw > 0) & (ih > 0), ia / den, 0.0)


def apply_ignore(class_map_hwc, templates, ignore_boxes, measure="iof", thresh=0.5, rf=otgt.RF, hm=otgt.HEATMAP_SIZE):
    """class_map_hwc (vsy, vsx, nt) with labels in {-1, 0, 1}; ignore_boxes (K, 4), degenerate ones (x2 <= x1 or y2 <= y1) dropped as faces
    are.  Returns (the map with every covered -1 turned to 0, the number of labels turned).  The input is not modified."""
    out = np.array(class_map_hwc, copy=True)
    r = np.asarray(ignore_boxes, dtype=np.float64).reshape(-1, 4)
    r = r[~((r[:, 2] <= r[:, 0]) | (r[:, 3] <= r[:, 1]))]
    if r.shape[0] == 0:
        return out, 0
    covered = (coverage(templates, r, measure, rf, hm) >= thresh).any(axis=3)
    turn = covered & (out == -1)
    out[turn] = 0
    return out, int(turn.sum())


def _rect_overlap(I, J):
    """1 - rect_dist of tinyfaces/metrics.py:44-74 (what crop_image compares with neg_thresh), restated."""
    aI = (I[:, 2] - I[:, 0] + 1) * (I[:, 3] - I[:, 1] + 1)
    aJ = (J[:, 2] - J[:, 0] + 1) * (J[:, 3] - J[:, 1] + 1)
    x1, y1 = np.maximum(I[:, 0], J[:, 0]), np.maximum(I[:, 1], J[:, 1])
    x2, y2 = np.minimum(I[:, 2], J[:, 2]), np.minimum(I[:, 3], J[:, 3])
    aIJ = (x2 - x1 + 1) * (y2 - y1 + 1) * np.logical_and(x2 > x1, y2 > y1)
    with np.errstate(all="ignore"):
        iou = aIJ / (aI + aJ - aIJ)
    iou[~np.isfinite(iou)] = 0
    return 1 - np.maximum(0.0, np.minimum(1.0, 1 - iou))


def _shift_clamp(b, crop, paste, input_size):
    ih, iw = input_size
    crop_y1, crop_x1 = crop[0], crop[1]
    b = np.array(b, dtype=np.float64).reshape(-1, 4)
    for k, (c, p) in enumerate(((crop_x1, paste[0]), (crop_y1, paste[1]), (crop_x1, paste[0]), (crop_y1, paste[1]))):
        b[:, k] = b[:, k] - c + p
    b[:, 0] = np.minimum(iw, np.maximum(0, b[:, 0]))
    b[:, 1] = np.minimum(ih, np.maximum(0, b[:, 1]))
    b[:, 2] = np.minimum(iw, np.maximum(1, b[:, 2]))
    b[:, 3] = np.minimum(ih, np.maximum(1, b[:, 3]))
    return b


def _mirror(b, input_size):
    b = b.copy()
    b[:, 0], b[:, 2] = input_size[1] - np.array(b[:, 2]) + 1, input_size[1] - np.array(b[:, 0]) + 1
    return b


def policy_boxes(bboxes, attributes, policy, crop, paste, flip, input_size=(500, 500), neg_thresh=0.3):
    """The bookkeeping of process_inputs(ignore_policy=) from the scale draw on.  bboxes (G, 4): the faces AFTER the scale draw; attributes:
    mapping with "invalid", "blur", "occlusion" ((G,) each) or None; policy: anything with the fields invalid, blur, occlusion, min_size,
    truncated; crop = (crop_y1, crop_x1, crop_h, crop_w), paste = [x1, y1, x2, y2] and flip as they were drawn.
    Returns (faces (G', 4), ignore boxes (K, 4)): flagged faces first, then the truncated ones, each in face order."""
    b = np.array(bboxes, dtype=np.float64).reshape(-1, 4)
    flagged = np.zeros(b.shape[0], dtype=bool)
    if policy.invalid:
        flagged |= np.asarray(attributes["invalid"]) >= 1
    if policy.blur is not None:
        flagged |= np.asarray(attributes["blur"]) >= policy.blur
    if policy.occlusion is not None:
        flagged |= np.asarray(attributes["occlusion"]) >= policy.occlusion
    if policy.min_size is not None:
        flagged |= np.minimum(b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]) + 1 < policy.min_size
    degenerate = lambda x: (x[:, 2] <= x[:, 0]) | (x[:, 3] <= x[:, 1])
    ign = _shift_clamp(b[flagged], crop, paste, input_size)
    ign = ign[~degenerate(ign)]
    faces = b[~flagged]
    crop_y1, crop_x1, crop_h, crop_w = crop
    t = faces.copy()
    t[:, 0], t[:, 1] = np.maximum(t[:, 0], crop_x1), np.maximum(t[:, 1], crop_y1)
    t[:, 2], t[:, 3] = np.minimum(t[:, 2], crop_x1 + crop_w), np.minimum(t[:, 3], crop_y1 + crop_h)
    overlap = _rect_overlap(t, faces) if faces.shape[0] else np.zeros(0)
    moved = _shift_clamp(faces, crop, paste, input_size)
    low = overlap < neg_thresh
    if policy.truncated:
        ign = np.concatenate([ign, moved[low & ~degenerate(moved)]])
    faces = moved[~(degenerate(moved) | low)]
    if flip:
        faces, ign = _mirror(faces, input_size), _mirror(ign, input_size)
    return faces, ign
