"""Training-time augmentation of the reference (WIDERFace.process_inputs, tinyfaces/datasets/wider_face.py:133-192, and
DataProcessor.crop_image, tinyfaces/datasets/processor.py:41-112) with the image work on the GPU.

Division of labour: the random decisions (scale, crop origin, paste origin, flip) and the bounding-box bookkeeping are a few
dozen floats per image and stay on the host, drawn from np.random in the reference's order so that a seeded run makes the
same decisions; the pixels -- resize, crop, paste on the mean colour, flip, ToTensor + Normalize -- are ONE HIP kernel per
image (ops.image_prepare) that only resamples the 500x500 window instead of resizing the whole image on the CPU.
The output tensor is bit-identical to the reference's CPU pipeline followed by main.py:44-46's transforms.

Optional colour jitter (`color_jitter=(b, c, s, h)`, off by default): torchvision's ColorJitter on the augmented uint8 image in front of
ToTensor, computed inside the same launch(es) (ops.image_prepare(jitter=)); its order and factors are drawn here, after the flip draw.

Optional ignore regions (`ignore_policy=IgnorePolicy(...)`, off by default): flagged, tiny and cropped-away faces are carried through scale,
crop and flip as ignore boxes for ops.dense_overlap_targets(ignore_boxes=) instead of becoming positives or plain background; pure
bookkeeping, nothing is drawn."""
from collections import namedtuple
from collections.abc import Mapping
from copy import deepcopy

import numpy as np
import torch

from .. import ops


def rect_dist(I, J):
    """tinyfaces/metrics.py:44-74: 1 - IoU (with the +1 pixel convention), clipped to [0, 1]; undefined ratios count as IoU 0."""
    I, J = np.atleast_2d(I).astype(np.float64), np.atleast_2d(J).astype(np.float64)
    aI = (I[:, 2] - I[:, 0] + 1) * (I[:, 3] - I[:, 1] + 1)
    aJ = (J[:, 2] - J[:, 0] + 1) * (J[:, 3] - J[:, 1] + 1)
    x1, y1 = np.maximum(I[:, 0], J[:, 0]), np.maximum(I[:, 1], J[:, 1])
    x2, y2 = np.minimum(I[:, 2], J[:, 2]), np.minimum(I[:, 3], J[:, 3])
    aIJ = (x2 - x1 + 1) * (y2 - y1 + 1) * np.logical_and(x2 > x1, y2 > y1)
    with np.errstate(all="ignore"):
        iou = aIJ / (aI + aJ - aIJ)
    iou[~np.isfinite(iou)] = 0
    return np.maximum(0.0, np.minimum(1.0, 1 - iou))


class IgnorePolicy(namedtuple("IgnorePolicy", "invalid blur occlusion min_size truncated", defaults=(False, None, None, None, False))):
    """Which faces of a training sample become ignore regions instead of positives (`process_inputs(ignore_policy=)`):
      invalid    bool: faces whose WIDER `invalid` column is set
      blur       None or a level in 1..2: faces with blur >= level          occlusion   likewise
      min_size   None or a number of pixels: faces whose shorter side min(x2 - x1, y2 - y1) + 1, measured after the scale draw, is below it
      truncated  bool: faces the crop drops only because too little of them is left (overlap < neg_thresh): the part that is left
    Build it through `check_ignore_policy`."""
    __slots__ = ()


def check_ignore_policy(policy):
    """None, or an IgnorePolicy / a mapping of its fields / a 5-tuple in field order -> a validated IgnorePolicy.  ValueError on anything else,
    on a field out of range, and on a policy that selects nothing."""
    if policy is None:
        return None
    try:
        p = IgnorePolicy(**policy) if isinstance(policy, Mapping) else IgnorePolicy(*policy)
    except TypeError:
        raise ValueError(f"ignore_policy: expected None, an IgnorePolicy, a mapping of {IgnorePolicy._fields} or a 5-tuple, got {policy!r}") from None
    for name in ("invalid", "truncated"):
        if not isinstance(getattr(p, name), (bool, np.bool_)):
            raise ValueError(f"ignore_policy: {name} must be a bool, got {getattr(p, name)!r}")
    for name in ("blur", "occlusion"):
        v = getattr(p, name)
        if v is not None and (isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= 2):
            raise ValueError(f"ignore_policy: {name} must be None or a level in 1..2, got {v!r}")
    s = p.min_size
    if s is not None and (isinstance(s, (bool, np.bool_)) or not isinstance(s, (int, float, np.integer, np.floating)) or not np.isfinite(s) or not s > 0):
        raise ValueError(f"ignore_policy: min_size must be None or a finite number of pixels > 0, got {s!r}")
    p = IgnorePolicy(bool(p.invalid), None if p.blur is None else int(p.blur), None if p.occlusion is None else int(p.occlusion),
                     None if s is None else float(s), bool(p.truncated))
    if not (p.invalid or p.blur or p.occlusion or p.min_size or p.truncated):
        raise ValueError("ignore_policy: no field is set (pass None to switch the feature off)")
    return p


def flagged_faces(policy, bboxes, attributes):
    """bool (G,): the faces `policy` turns into ignore regions by their attributes or their size; bboxes as they are after the scale draw.
    attributes: the datum's columns (a mapping with "invalid", "blur", "occlusion", each (G,)); needed only for the fields that read them."""
    g = bboxes.shape[0]
    flagged = np.zeros(g, dtype=bool)
    for name, level in (("invalid", 1 if policy.invalid else None), ("blur", policy.blur), ("occlusion", policy.occlusion)):
        if level is None:
            continue
        if attributes is None or name not in attributes:
            raise ValueError(f"ignore_policy: the {name} field needs attributes[{name!r}], one value per face")
        col = np.asarray(attributes[name], dtype=np.float64).reshape(-1)
        if col.shape[0] != g:
            raise ValueError(f"ignore_policy: attributes[{name!r}] has {col.shape[0]} values for {g} faces")
        flagged |= col >= level
    if policy.min_size is not None and g:
        flagged |= np.minimum(bboxes[:, 2] - bboxes[:, 0], bboxes[:, 3] - bboxes[:, 1]) + 1 < policy.min_size
    return flagged


def crop_decisions(img_h, img_w, bboxes, input_size=(500, 500), neg_thresh=0.3, rng=np.random, *, flagged=None, truncated=False, ignore_out=None):
    """The host half of DataProcessor.crop_image (processor.py:41-112): the crop window, where it is pasted, and the boxes
    that survive (shifted, clamped, filtered by overlap with their cropped part).  Same np.random draws, same order.
    ignore_out (a list; None = off, and then nothing below happens): receives the (K, 4) float64 ignore boxes of this crop -- the boxes of
    `flagged` ((F, 4), in the frame of `bboxes`) shifted and clamped like a face, those that are not degenerate; then, with `truncated`, the
    clamped boxes of the faces that are dropped ONLY because overlap < neg_thresh.  Draws nothing."""
    ih, iw = input_size
    max_crop_x = max(1, img_w - iw + 1)
    max_crop_y = max(1, img_h - ih + 1)
    crop_x1 = rng.randint(0, max_crop_x)
    crop_y1 = rng.randint(0, max_crop_y)
    crop_x2 = min(img_w, crop_x1 + iw)
    crop_y2 = min(img_h, crop_y1 + ih)
    crop_h, crop_w = crop_y2 - crop_y1, crop_x2 - crop_x1
    paste = [0, 0, 0, 0]
    paste[0] = rng.randint(0, iw - crop_w + 1)
    paste[1] = rng.randint(0, ih - crop_h + 1)
    paste[2], paste[3] = paste[0] + crop_w, paste[1] + crop_h
    bboxes = np.array(bboxes, dtype=np.float64).reshape(-1, 4)
    cut_boxes = None
    if bboxes.shape[0] > 0:
        tbox = deepcopy(bboxes)
        tbox[:, 0] = np.maximum(tbox[:, 0], crop_x1)
        tbox[:, 1] = np.maximum(tbox[:, 1], crop_y1)
        tbox[:, 2] = np.minimum(tbox[:, 2], crop_x2)
        tbox[:, 3] = np.minimum(tbox[:, 3], crop_y2)
        overlap = 1 - rect_dist(tbox, bboxes)
        bboxes[:, 0] = bboxes[:, 0] - crop_x1 + paste[0]        # (b - c) + p, in the reference's order: the last bit matters
        bboxes[:, 1] = bboxes[:, 1] - crop_y1 + paste[1]
        bboxes[:, 2] = bboxes[:, 2] - crop_x1 + paste[0]
        bboxes[:, 3] = bboxes[:, 3] - crop_y1 + paste[1]
        bboxes[:, 0] = np.minimum(iw, np.maximum(0, bboxes[:, 0]))
        bboxes[:, 1] = np.minimum(ih, np.maximum(0, bboxes[:, 1]))
        bboxes[:, 2] = np.minimum(iw, np.maximum(1, bboxes[:, 2]))
        bboxes[:, 3] = np.minimum(ih, np.maximum(1, bboxes[:, 3]))
        invalid = (bboxes[:, 2] <= bboxes[:, 0]) | (bboxes[:, 3] <= bboxes[:, 1]) | (overlap < neg_thresh)
        if ignore_out is not None and truncated:
            cut = (overlap < neg_thresh) & ~((bboxes[:, 2] <= bboxes[:, 0]) | (bboxes[:, 3] <= bboxes[:, 1]))
            cut_boxes = bboxes[cut]                              # what is left to see of them
        bboxes = bboxes[~invalid]
    if ignore_out is not None:
        parts = []
        f = np.array([] if flagged is None else flagged, dtype=np.float64).reshape(-1, 4)
        if f.shape[0] > 0:
            f[:, 0] = f[:, 0] - crop_x1 + paste[0]               # the face's own shift and clamp
            f[:, 1] = f[:, 1] - crop_y1 + paste[1]
            f[:, 2] = f[:, 2] - crop_x1 + paste[0]
            f[:, 3] = f[:, 3] - crop_y1 + paste[1]
            f[:, 0] = np.minimum(iw, np.maximum(0, f[:, 0]))
            f[:, 1] = np.minimum(ih, np.maximum(0, f[:, 1]))
            f[:, 2] = np.minimum(iw, np.maximum(1, f[:, 2]))
            f[:, 3] = np.minimum(ih, np.maximum(1, f[:, 3]))
            parts.append(f[~((f[:, 2] <= f[:, 0]) | (f[:, 3] <= f[:, 1]))])
        if cut_boxes is not None:
            parts.append(cut_boxes)
        ignore_out[:] = list(np.concatenate(parts)) if parts else []      # one (4,) row per ignore box: np.array(ignore_out).reshape(-1, 4)
    return (crop_y1, crop_x1, crop_h, crop_w), paste, bboxes


JITTER_ORDER = ("brightness", "contrast", "saturation", "hue")      # ColorJitter's numbering of its four ops


def check_color_jitter(color_jitter):
    """None, or the four amplitudes (brightness, contrast, saturation, hue) of torchvision's ColorJitter as a tuple of floats: finite, >= 0,
    hue <= 0.5."""
    if color_jitter is None:
        return None
    try:
        amps = tuple(float(v) for v in color_jitter)
    except (TypeError, ValueError):
        raise ValueError(f"color_jitter: expected four numbers (brightness, contrast, saturation, hue), got {color_jitter!r}")
    if len(amps) != 4:
        raise ValueError(f"color_jitter: expected four numbers (brightness, contrast, saturation, hue), got {color_jitter!r}")
    for name, a in zip(JITTER_ORDER, amps):
        if not (np.isfinite(a) and a >= 0.0):
            raise ValueError(f"color_jitter: the {name} amplitude must be finite and >= 0, got {a}")
    if amps[3] > 0.5:
        raise ValueError(f"color_jitter: the hue amplitude must be <= 0.5, got {amps[3]}")
    return amps


def draw_color_jitter(color_jitter, rng=np.random):
    """The chain [(kind, factor)] of one image: order = rng.permutation(4), then one rng.uniform for each of brightness, contrast, saturation,
    hue whose amplitude a is > 0 -- from [max(0, 1 - a), 1 + a], for the hue from [-a, a] -- and the drawn ops in `order`.  An amplitude of 0
    draws nothing and applies nothing."""
    amps = check_color_jitter(color_jitter)
    order = rng.permutation(4)
    factors = {}
    for k, (name, a) in enumerate(zip(JITTER_ORDER, amps)):
        if a > 0.0:
            factors[k] = float(rng.uniform(-a, a) if name == "hue" else rng.uniform(max(0.0, 1.0 - a), 1.0 + a))
    return [(JITTER_ORDER[k], factors[k]) for k in order.tolist() if k in factors]


def process_inputs(image_u8, bboxes, input_size=(500, 500), neg_thresh=0.3, rng=np.random, out=None, mean=ops.IMAGE_MEAN,
                   std=ops.IMAGE_STD, color_jitter=None, chain_out=None, *, ignore_policy=None, attributes=None, ignore_out=None):
    """WIDERFace.process_inputs up to get_heatmaps, for a decoded uint8 (H, W, 3) image that is already on the device.
    Returns (x float32 (3, ih, iw) device tensor = Normalize(ToTensor(augmented image)), bboxes float64 (G', 4),
    paste_box [x1, y1, x2, y2], flip) -- paste_box / flip are what ops.dense_overlap_targets* take for the padding mask.
    color_jitter = (b, c, s, h): torchvision's ColorJitter(b, c, s, h) on the augmented uint8 image in front of ToTensor, in the same launch
    (ops.image_prepare(jitter=)); its draws (draw_color_jitter) come AFTER the flip draw and only when it is not None, so a seeded run without it
    makes the decisions it always made.  chain_out: a list that receives the drawn [(kind, factor)] chain.
    ignore_policy (an IgnorePolicy, see check_ignore_policy; None = off): the faces it flags -- by `attributes`, the datum's attribute columns,
    or by their size after the scale draw -- leave the face list before the crop filters it, so they own no positive, and go through the same
    shift, clamp and flip as a face; what is left of them, and with `truncated` of the faces the crop drops for overlap < neg_thresh, are the
    ignore boxes of ops.dense_overlap_targets(ignore_boxes=).  ignore_out: a list that receives them, one (4,) float64 row each, in the
    augmented frame and mirrored.  The feature draws nothing from rng."""
    if not image_u8.is_cuda:
        raise RuntimeError("process_inputs: the image must be on the GPU (no CPU fallback for the hot path)")
    color_jitter = check_color_jitter(color_jitter)
    ignore_policy = check_ignore_policy(ignore_policy)
    H, W = int(image_u8.shape[0]), int(image_u8.shape[1])
    bboxes = np.array(bboxes, dtype=np.float64).reshape(-1, 4)
    rnd = rng.rand()                                             # wider_face.py:135
    rh, rw = H, W
    if rnd < 1 / 3:
        rh, rw = int(0.5 * H), int(0.5 * W)
        bboxes = bboxes / 2
    elif rnd > 2 / 3:
        rh, rw = int(2 * H), int(2 * W)
        bboxes = bboxes * 2
    if ignore_policy is None:
        crop, paste, bboxes = crop_decisions(rh, rw, bboxes, input_size, neg_thresh, rng)
    else:
        flagged = flagged_faces(ignore_policy, bboxes, attributes)
        ign = []
        crop, paste, bboxes = crop_decisions(rh, rw, bboxes[~flagged], input_size, neg_thresh, rng, flagged=bboxes[flagged],
                                             truncated=ignore_policy.truncated, ignore_out=ign)
        ign = np.array(ign, dtype=np.float64).reshape(-1, 4)
    flip = bool(rng.rand() > 0.5)                                # wider_face.py:155
    if flip:
        lx1, lx2 = np.array(bboxes[:, 0]), np.array(bboxes[:, 2])
        bboxes[:, 0] = input_size[1] - lx2 + 1
        bboxes[:, 2] = input_size[1] - lx1 + 1
    if ignore_policy is not None:
        if flip:
            lx1, lx2 = np.array(ign[:, 0]), np.array(ign[:, 2])
            ign[:, 0] = input_size[1] - lx2 + 1
            ign[:, 2] = input_size[1] - lx1 + 1
        if ignore_out is not None:
            ignore_out[:] = list(ign)
    chain = None
    if color_jitter is not None:
        chain = draw_color_jitter(color_jitter, rng)
        if chain_out is not None:
            chain_out[:] = chain
    x = ops.image_prepare(image_u8, resized_hw=(rh, rw), crop=crop, paste=(paste[1], paste[0]), flip=flip, out_hw=input_size, mean=mean,
                          std=std, out=out, jitter=chain)
    return x, bboxes, paste, flip


def collate_device(samples, templates_d, seed=0, compensate=None, ignore_boxes=None, ignore=None, assigner="dense_overlap", atss_topk=ops.ATSS_TOPK):
    """[(x, bboxes, paste_box, flip)] -> (img (B,3,H,W), class_map, regression_map) with the targets assigned on the GPU
    (what WIDERFace.__getitem__ + the default collate yield, wider_face.py:219-222).  compensate = (N, T): scale-compensated matching
    (ops.dense_overlap_targets(compensate=)); None = off.  ignore_boxes: per sample the (K, 4) ignore boxes process_inputs(ignore_out=)
    collected, ignore = (measure, thresh) (ops.dense_overlap_targets(ignore_boxes=, ignore=)); None = off.
    assigner = "atss": the targets come from ops.atss_targets(topk=atss_topk) (no seed, no thresholds; compensate is refused).
    assigner = "tal": the maps are the base maps (no face assigned; the ignore pass as always) and a fourth element follows, the ResidentFaces
    of the batch (datasets/targets.py): the criterion assigns from the predictions (compensate is refused)."""
    assigner, atss_topk = ops.check_assigner(assigner, atss_topk, compensate)
    xs = torch.stack([s[0] for s in samples])
    extra = {} if ignore_boxes is None else {"ignore_boxes": [np.array(b, dtype=np.float64).reshape(-1, 4) for b in ignore_boxes], "ignore": ignore}
    if assigner == "tal":
        from .targets import TargetAssigner
        ta = TargetAssigner(templates_d, ignore=None if ignore_boxes is None else (ignore or ops.IGNORE_DEFAULT), assigner="tal")
        cm, rm, faces = ta([s[1] for s in samples], paste_boxes=[s[2] for s in samples], flips=[int(s[3]) for s in samples], device=xs.device,
                           ignore_boxes=extra.get("ignore_boxes"))
        faces.stats = None                                    # nobody reads the counters of a one-off assigner
        return xs, cm, rm, faces
    if assigner == "atss":
        cm, rm = ops.atss_targets([s[1] for s in samples], templates_d, paste_boxes=[s[2] for s in samples], flips=[int(s[3]) for s in samples],
                                  topk=atss_topk, device=xs.device, **extra)
        return xs, cm, rm
    cm, rm = ops.dense_overlap_targets([s[1] for s in samples], templates_d, paste_boxes=[s[2] for s in samples],
                                       flips=[int(s[3]) for s in samples], seed=seed, device=xs.device,      # boxes are already mirrored; flips mirrors the padding mask
                                       compensate=compensate, **extra)
    return xs, cm, rm
