"""Call surface of the reference's tinyfaces/evaluation.py (get_model, get_detections,
write_results).  Per pyramid level: HIP forward -> HIP sigmoid/threshold/ordered-compaction/
refinement straight into one device candidate list; then ONE float64 HIP NMS over all levels
(evaluation.py:80-84).  Only the K surviving rows cross PCIe (the reference copies three full
score maps per level, evaluation.py:64-68)."""
from pathlib import Path

import numpy as np
import torch

from . import ops, transforms
from .models.model import DetectionModel, base_model_of


def get_model(checkpoint=None, num_templates=25, ema=False):
    """evaluation.py:12-17; the trunk (resnet50 / resnet101 / resnet152) is the one the checkpoint's keys hold.  ema=True (an addition):
    load the averaged weights a `main.py --model-ema` run stored under "model_ema" instead of the last iterate under "model"."""
    if not checkpoint:
        if ema:
            raise ValueError("get_model(ema=True) needs a checkpoint: the averaged weights are its \"model_ema\" entry")
        return DetectionModel(num_templates=num_templates)
    path = checkpoint
    checkpoint = torch.load(checkpoint, map_location="cpu")
    if ema and "model_ema" not in checkpoint:
        raise ValueError(f"{path} has no \"model_ema\" entry (keys: {sorted(checkpoint)}): it was not written by a run with --model-ema")
    weights = checkpoint["model_ema" if ema else "model"]
    model = DetectionModel(base_model=base_model_of(weights), num_templates=num_templates)
    model.load_state_dict(weights)
    return model


def _normalize_of(img_transforms):
    """(mean, std) when img_transforms is the Compose([ToTensor, Normalize]) of evaluate_model.py:35-37, else None."""
    ts = getattr(img_transforms, "transforms", None)
    if ts is not None and len(ts) == 2 and type(ts[0]).__name__ == "ToTensor" and type(ts[1]).__name__ == "Normalize":
        return tuple(float(v) for v in ts[1].mean), tuple(float(v) for v in ts[1].std)
    return None


def _on_device(model, device):
    """model.to(device) only when something has to move: nn.Module.to walks `_apply` even when it is a no-op, and DetectionModel._apply must then
    assume that every storage moved -- the pointer tables and the packed evaluation weights of an open constant_weights() session were rebuilt on
    EVERY get_detections call (r6: 80 of the 87 ms per image of the end-to-end path)."""
    p = next(model.parameters(), None)
    if p is not None and p.device.type == device.type and (device.index is None or p.device.index == device.index):
        return model
    return model.to(device)


def _pyramid_levels(img, scales, img_transforms, pyramid_on_gpu, device, flip=False):
    """evaluation.py:37-53: [(scale, normalised (1,3,H,W) tensor)] for every pyramid level of one image.  flip: the same levels follow
    once more MIRRORED left-right, in the same order (the second half of the list)."""
    scales_list = [2 ** x for x in scales]
    levels, mirrored = [], []
    if pyramid_on_gpu:
        ms = _normalize_of(img_transforms)
        if ms is None:
            raise ValueError("pyramid_on_gpu needs img_transforms = Compose([ToTensor(), Normalize(mean, std)])")
        planes = transforms.to_uint8_chw(img)                                  # the pixels of to_pil_image(img) (:40), no PIL object in between
        # the only upload of the image; the CHW -> HWC interleave is a device copy (6 ms of byte-wise numpy transposition on the host otherwise)
        u8 = torch.from_numpy(planes).to(device).permute(1, 2, 0).contiguous()
        h, w = planes.shape[1:]
        min_side = min(w, h)
        for scale in scales_list:
            size = int(min_side * scale)                                       # :46 -> transforms.resize(image, int)
            short, long = (w, h) if w <= h else (h, w)
            new_short, new_long = size, int(size * long / short)
            new_w, new_h = (new_short, new_long) if w <= h else (new_long, new_short)
            levels.append((scale, ops.image_prepare(u8, resized_hw=(new_h, new_w), mean=ms[0], std=ms[1]).unsqueeze(0)))
            if flip:
                mirrored.append((scale, ops.image_prepare(u8, resized_hw=(new_h, new_w), mean=ms[0], std=ms[1], flip=True).unsqueeze(0)))
    else:
        image = transforms.to_pil_image(img)                              # :40
        min_side = np.min(image.size)
        # the resize + normalise of :46-53 is host work: do it for every level first, then keep the GPU busy
        for scale in scales_list:
            scaled = transforms.resize(image, int(min_side * scale))
            x = img_transforms(scaled).unsqueeze(0).float()
            levels.append((scale, x))
            if flip:
                mirrored.append((scale, x.flip(-1)))                       # the pixels tf_image_prepare(flip=True) writes, bit for bit
    return levels + mirrored


def _level_capacity(levels, nt):
    return sum(((x.shape[2] + 7) // 8) * ((x.shape[3] + 7) // 8) for _, x in levels) * nt


def _decode_levels(model, levels, templates, t_d, rf, prob_thresh, mask_axis, dets, count, device, mirrored=False):
    """Forward + sigmoid / threshold / ordered compaction / refinement of every level, appended to dets[count...].
    The forwards of the levels run side by side on the model's lanes (DetectionModel.forward_levels); the decodes follow in level
    order on the caller's stream, so the candidate list is the sequential loop's row for row.
    mirrored: the levels are left-right mirrors (test-time flip).  They are decoded like any image -- the same template masks, defect D1
    included --, then the rows each of them appended are mirrored back on the device (tf_boxes_unflip_f64): the row range is the
    counter before and after the level, kept in device memory."""
    xs = [x.to(device, non_blocking=True) for _, x in levels]
    # any callable nn.Module is accepted, like the reference's get_detections (evaluation.py:56-60): only DetectionModel has lanes
    fl = getattr(model, "forward_levels", None)
    outs = fl(xs) if fl is not None else [model(x) for x in xs]
    for (scale, x), out in zip(levels, outs):                         # (1, 5nt, H', W')
        _, _, H, W = out.shape
        vx, vt = ops.template_masks(templates, scale, W, mask_axis)
        first = count.clone() if mirrored else None
        ops.decode_compact(out[0], t_d, torch.from_numpy(vx).to(device), torch.from_numpy(vt).to(device),
                           prob_thresh, scale, dets, count, rf)
        if mirrored:
            # a level pixel x' is the image's pixel (W_level - 1 - x') / scale; 1 / scale is the factor of the decode (tf_decode_compact)
            ops.boxes_unflip_(dets, first, count.clone(), H * W * t_d.shape[0], (x.shape[3] - 1) * (1 / scale))


def _decode_image(model, levels, flip, *args):
    """`_decode_levels` for the levels of one image; with flip the second half of `levels` is the mirrored pyramid, run as a second group
    behind the first so that the first rows are exactly the candidate list without it."""
    if not flip:
        return _decode_levels(model, levels, *args)
    half = len(levels) // 2
    _decode_levels(model, levels[:half], *args)
    _decode_levels(model, levels[half:], *args, mirrored=True)


MATRIX_NMS = {"matrix_linear": "linear", "matrix_gaussian": "gaussian"}      # soft_nms= values that select ops.matrix_nms, and its method


def _check_soft_nms(soft_nms, nms_thresh, sigma, score_thresh):
    """The keywords of get_detections / get_detections_batch, refused before the model runs."""
    if soft_nms is None:
        return
    if soft_nms in MATRIX_NMS:
        ops._matrix_nms_mode(MATRIX_NMS[soft_nms], sigma, score_thresh, "sigmoid", None)     # nms_thresh plays no part
        return
    if soft_nms not in ops.SOFT_NMS_METHODS:
        raise ValueError(f"soft_nms={soft_nms!r}: expected None or one of {sorted(ops.SOFT_NMS_METHODS) + sorted(MATRIX_NMS)}")
    ops._soft_nms_mode(soft_nms, nms_thresh if soft_nms == "linear" else 0.0, sigma, score_thresh, "sigmoid")


def _suppression_limit(soft_nms):
    """(largest candidate list the method of `soft_nms` takes, its name in a message)."""
    if soft_nms in MATRIX_NMS:
        return ops.MATRIX_NMS_MAX_BOXES, "Matrix NMS"
    return ops.SOFT_NMS_MAX_BOXES, "Soft-NMS"


def _check_limits(pre_nms_topk, max_detections):
    """pre_nms_topk / max_detections of get_detections / get_detections_batch: None or a positive integer, refused before the model runs."""
    for name, v in (("pre_nms_topk", pre_nms_topk), ("max_detections", max_detections)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1):
            raise ValueError(f"{name}={v!r}: expected None or an integer >= 1")


def _pre_nms_cut(cand, offs, pre_nms_topk):
    """Every segment of the device candidate list longer than pre_nms_topk is cut to its best pre_nms_topk rows (`ops.topk_select_batched`; the
    rows keep the list's order) -> (rows, offsets, idx): idx maps a row of the cut list to its row in `cand`, None when nothing was cut."""
    if pre_nms_topk is None:
        return cand, offs, None
    idx, new = ops.topk_select_batched(cand[:, 4].contiguous(), offs, int(pre_nms_topk))
    if idx is None:
        return cand, offs, None
    return cand.index_select(0, idx), new, idx


def _soft_nms_rows(cand, offs, method, nms_thresh, sigma, score_thresh, box_voting, max_keep=None):
    """Soft-NMS (or, for a method of MATRIX_NMS, Matrix NMS) over the segments `offs` of the device candidate list (rows x1, y1, x2, y2, logit)
    -> ([keep], [(K_s, 5) device rows]):
    cand[keep] in selection order, or the voted rows, with the decayed probability in column 4.  One synchronisation."""
    boxes, scores = cand[:, :4].contiguous(), cand[:, 4].contiguous()
    thr = nms_thresh if method == "linear" else 0.0             # the gaussian method ignores it
    vote = {} if box_voting is None else {"vote": (box_voting, "sigmoid")}
    if method in MATRIX_NMS:                                    # Matrix NMS: no IoU threshold; the cap is an argument of the one call
        res = ops.matrix_nms_batched(boxes, scores, offs, MATRIX_NMS[method], sigma, score_thresh, max_keep=None if max_keep is None else int(max_keep),
                                     **vote)
    elif max_keep is None:                                      # without a cap the call is the one it was
        res = ops.soft_nms_batched(boxes, scores, offs, method, thr, sigma, score_thresh, **vote)
    else:
        res = ops.soft_nms_batched_capped(boxes, scores, offs, int(max_keep), method, thr, sigma, score_thresh, **vote)
    if box_voting is not None:
        res, rows = res
        return [k for k, _ in res], rows
    return [k for k, _ in res], [torch.cat([boxes[k], ks.unsqueeze(1)], dim=1) for k, ks in res]


def get_detections(model, img, templates, rf, img_transforms, prob_thresh=0.65, nms_thresh=0.3, scales=(-2, -1, 0, 1),
                   device=None, mask_axis="w", return_candidates=False, pyramid_on_gpu=False, pre_nms_topk=None, max_detections=None,
                   flip=False, box_voting=None, soft_nms=None, soft_nms_sigma=0.5, soft_nms_score_thresh=0.001):
    """evaluation.py:20-87.  Returns (K,5) float64: the reference's (K,4) rows in the same order
    with the score re-attached as column 4 (defect D2: the reference drops it although
    write_results reads x[4], evaluation.py:111).  mask_axis='w' reproduces defect D1
    (tinyfaces/models/utils.py:44); 'template' masks the template axis instead.
    pyramid_on_gpu=True: the uint8 image goes to the device once and every pyramid level is produced there
    by tf_image_prepare (Pillow-exact BILINEAR resize + ToTensor + Normalize in one pass) instead of PIL + torch on the host;
    needs img_transforms = Compose([ToTensor(), Normalize(mean, std)]); same detections bit for bit.
    Test-time augmentation (additions; with the defaults nothing else is launched and the rows are the same bit for bit):
    flip=True: every pyramid level is also run mirrored left-right and its candidates, mirrored back, follow those of the unmirrored
    levels in the candidate list; the one NMS runs over the union.
    box_voting=t: every NMS survivor is replaced by the sigmoid-weighted mean of all candidates with IoU >= t (`ops.box_voting`:
    Detectron's box_voting, scoring ID -- the candidates' scores are logits); the rows returned are the voted rows in keep order.
    soft_nms="linear" | "gaussian" (an addition as well; None: the hard NMS above, the same launches and rows): Soft-NMS (`ops.soft_nms`)
    instead of the hard NMS -- an overlapped candidate is decayed, not dropped, and survives while its score stays >= soft_nms_score_thresh.
    nms_thresh is the linear method's IoU threshold, soft_nms_sigma the gaussian method's (which ignores nms_thresh).  The rows are
    cand[keep] in selection order with column 4 replaced by the DECAYED PROBABILITY (not a logit); with box_voting the voted rows, column 4
    likewise; return_candidates returns that keep.
    soft_nms="matrix_linear" | "matrix_gaussian" (an addition as well): Matrix NMS (`ops.matrix_nms`, method "linear" / "gaussian") -- the same
    kind of decay in closed form, with no serial selection: a candidate's factor depends on the better-scored candidates and on their own
    largest overlap with something still better.  soft_nms_sigma and soft_nms_score_thresh keep their meaning (SOLOv2's multiplier 2.0 is
    sigma 0.5); nms_thresh is NOT USED by either matrix method (there is no IoU threshold).  Rows, column 4, box_voting, flip, pre_nms_topk
    and return_candidates as with Soft-NMS; max_detections goes into the call as its max_keep; the candidate-count limit is
    ops.MATRIX_NMS_MAX_BOXES.
    The two bounds every WIDER FACE pipeline has (additions; None: off, the same launches and rows bit for bit):
    pre_nms_topk=K (S3FD / PyramidBox / RetinaFace `top_k`, torchvision's `topk_candidates`): when more than K candidates pass prob_thresh, only
    the K best -- larger score, the earlier candidate on a tie, the hard NMS's own order -- reach the NMS / Soft-NMS / vote
    (`ops.topk_select`: selected on the device, gathered in candidate order).  The hard NMS then returns exactly the rows of the uncut call
    whose candidate ranks below K.  With flip=True the cut applies to the union of the plain and the mirrored candidates.  Box voting's voters
    are the K retained candidates (Detectron's behaviour: it votes over the boxes that entered the NMS).  The candidate-count limits of the NMS
    (ops.NMS_MAX_BOXES) and of Soft-NMS (ops.SOFT_NMS_MAX_BOXES) apply to min(n, K).  return_candidates still returns the FULL candidate list and a
    keep that indexes it.
    max_detections=M (`keep_top_k`, `detections_per_img`): at most M rows come back, the first M in keep order; with soft_nms the selection
    itself stops after M rows (`ops.soft_nms_capped`), which is where the time is saved.
    (Both sit in front of `flip` in the signature, not at its end: every keyword of this call is passed by name, and the tail of the list is
    what tests/test_soft_nms.py holds fixed.)"""
    device = torch.device(device if device is not None else "cuda")
    if device.type != "cuda":
        raise RuntimeError("get_detections: the detector only runs on MI355X (no CPU fallback)")
    _check_soft_nms(soft_nms, nms_thresh, soft_nms_sigma, soft_nms_score_thresh)
    _check_limits(pre_nms_topk, max_detections)
    model = _on_device(model, device)
    model.eval()
    nt = templates.shape[0]
    t_d = torch.as_tensor(np.asarray(templates), dtype=torch.float64).contiguous().to(device)
    levels = _pyramid_levels(img, scales, img_transforms, pyramid_on_gpu, device, flip)
    dets = torch.empty(max(_level_capacity(levels, nt), 1), 5, dtype=torch.float64, device=device)
    count = torch.zeros(1, dtype=torch.int32, device=device)
    biggest = max(levels, key=lambda l: l[1].shape[2] * l[1].shape[3])[1]
    # weights are constant across the pyramid (and across images when the caller already opened a session): pack once
    with torch.no_grad(), model.constant_weights(reserve=(1, biggest.shape[2], biggest.shape[3])):
        _decode_image(model, levels, flip, templates, t_d, rf, prob_thresh, mask_axis, dets, count, device)
    n = int(count.item())
    assert n <= dets.shape[0]
    reach = n if pre_nms_topk is None else min(n, int(pre_nms_topk))  # what the suppression step is given
    if reach > ops.NMS_MAX_BOXES:
        raise RuntimeError(f"get_detections: {reach} candidates above prob_thresh={prob_thresh} exceed the {ops.NMS_MAX_BOXES} boxes one NMS call "
                           "takes (64 KiB of LDS for the suppression bitmap); a trained detector keeps a few thousand -- untrained weights?  "
                           "pre_nms_topk=K bounds what reaches the NMS without touching prob_thresh")
    full = dets[:n]
    limit, what = _suppression_limit(soft_nms)
    if soft_nms is not None and reach > limit:
        raise RuntimeError(f"get_detections: {reach} candidates above prob_thresh={prob_thresh} exceed the {limit} boxes one "
                           f"{what} call takes (the hard NMS takes {ops.NMS_MAX_BOXES}): pass pre_nms_topk <= {limit}, "
                           "raise prob_thresh or use soft_nms=None")
    cand, offs, idx = _pre_nms_cut(full, [0, n], pre_nms_topk)
    if soft_nms is not None:
        keep, rows = _soft_nms_rows(cand, offs, soft_nms, nms_thresh, soft_nms_sigma, soft_nms_score_thresh, box_voting, max_detections)
        keep, result = keep[0], rows[0].cpu().numpy()
    elif box_voting is None:
        keep = ops.nms(cand[:, :4].contiguous(), cand[:, 4].contiguous(), nms_thresh)      # :80-84
        if max_detections is not None:
            keep = keep[:max_detections]
        result = cand[keep].cpu().numpy()
    else:
        # the vote chains behind the NMS on its device-side keep count: still one synchronisation
        keeps, voted = ops.nms_batched(cand[:, :4].contiguous(), cand[:, 4].contiguous(), offs, nms_thresh, vote=(box_voting, "sigmoid"))
        keep, rows = keeps[0], voted[0]
        if max_detections is not None:
            keep, rows = keep[:max_detections], rows[:max_detections]
        result = rows.cpu().numpy()
    if return_candidates:
        if idx is not None:
            keep = idx[keep]                                          # back to rows of the full candidate list
        return result, full.cpu().numpy(), keep.cpu().numpy()
    return result


def get_detections_batch(model, imgs, templates, rf, img_transforms, prob_thresh=0.65, nms_thresh=0.3, scales=(-2, -1, 0, 1),
                         device=None, mask_axis="w", pyramid_on_gpu=False, pre_nms_topk=None, max_detections=None, flip=False,
                         box_voting=None, soft_nms=None, soft_nms_sigma=0.5, soft_nms_score_thresh=0.001):
    """`[get_detections(model, img, ...) for img in imgs]` (evaluation.py:20-87 once per image, as evaluate_model.py:60-68 does) with
    the per-image NMS calls batched: every image's multi-scale candidates go into ONE device list, the per-image segments are
    suppressed by ONE tf_nms_f64_batched call (three launches whatever the number of images; BASELINE.json configs[4]) and the
    only host synchronisation of the whole batch is the read of the candidate counts.  Row for row identical to the loop.
    flip / box_voting: as in get_detections; an image's mirrored candidates follow its unmirrored ones, so its segment stays contiguous.
    soft_nms / soft_nms_sigma / soft_nms_score_thresh: as in get_detections, one tf_soft_nms_f64_batched call over the per-image segments
    (soft_nms="matrix_linear" | "matrix_gaussian": one tf_matrix_nms_f64_batched call; nms_thresh is not used).
    pre_nms_topk / max_detections: as in get_detections, per image: one tf_topk_select_f64_batched call cuts every image's segment that is
    longer than pre_nms_topk, behind the one synchronisation the call already has."""
    device = torch.device(device if device is not None else "cuda")
    if device.type != "cuda":
        raise RuntimeError("get_detections_batch: the detector only runs on MI355X (no CPU fallback)")
    _check_soft_nms(soft_nms, nms_thresh, soft_nms_sigma, soft_nms_score_thresh)
    _check_limits(pre_nms_topk, max_detections)
    imgs = list(imgs)
    if not 1 <= len(imgs) <= ops.NMS_MAX_SEGMENTS:
        raise ValueError(f"get_detections_batch: 1..{ops.NMS_MAX_SEGMENTS} images per call, got {len(imgs)}")
    model = _on_device(model, device)
    model.eval()
    nt = templates.shape[0]
    t_d = torch.as_tensor(np.asarray(templates), dtype=torch.float64).contiguous().to(device)
    per_image = [_pyramid_levels(img, scales, img_transforms, pyramid_on_gpu, device, flip) for img in imgs]
    dets = torch.empty(max(sum(_level_capacity(lv, nt) for lv in per_image), 1), 5, dtype=torch.float64, device=device)
    count = torch.zeros(1, dtype=torch.int32, device=device)
    marks = torch.zeros(len(imgs) + 1, dtype=torch.int32, device=device)
    biggest = max((l[1] for lv in per_image for l in lv), key=lambda x: x.shape[2] * x.shape[3])
    with torch.no_grad(), model.constant_weights(reserve=(1, biggest.shape[2], biggest.shape[3])):
        for i, levels in enumerate(per_image):
            _decode_image(model, levels, flip, templates, t_d, rf, prob_thresh, mask_axis, dets, count, device)
            marks[i + 1:i + 2].copy_(count, non_blocking=True)        # segment boundary, recorded on the stream
    offs = marks.tolist()                                             # the one sync
    longest = max(b - a for a, b in zip(offs, offs[1:]))
    if pre_nms_topk is not None:
        longest = min(longest, int(pre_nms_topk))                     # what the suppression step is given
    if longest > ops.NMS_MAX_BOXES:
        raise RuntimeError(f"get_detections_batch: an image has more than {ops.NMS_MAX_BOXES} candidates above prob_thresh={prob_thresh}; "
                           "pre_nms_topk=K bounds what reaches the NMS without touching prob_thresh")
    limit, what = _suppression_limit(soft_nms)
    if soft_nms is not None and longest > limit:
        raise RuntimeError(f"get_detections_batch: an image has {longest} candidates above prob_thresh={prob_thresh}, more than the "
                           f"{limit} boxes one {what} call takes (the hard NMS takes {ops.NMS_MAX_BOXES}): pass "
                           f"pre_nms_topk <= {limit}")
    cand, offs, _ = _pre_nms_cut(dets[:offs[-1]], offs, pre_nms_topk)
    if soft_nms is not None:
        _, rows = _soft_nms_rows(cand, offs, soft_nms, nms_thresh, soft_nms_sigma, soft_nms_score_thresh, box_voting, max_detections)
        return [r.cpu().numpy() for r in rows]
    M = max_detections                                                # None: the whole keep list, as before
    if box_voting is not None:
        _, voted = ops.nms_batched(cand[:, :4].contiguous(), cand[:, 4].contiguous(), offs, nms_thresh, vote=(box_voting, "sigmoid"))
        return [v[:M].cpu().numpy() for v in voted]
    keeps = ops.nms_batched(cand[:, :4].contiguous(), cand[:, 4].contiguous(), offs, nms_thresh)
    return [cand[k[:M]].cpu().numpy() for k in keeps]


def write_results(dets, img_path, split, results_dir=None):
    """evaluation.py:90-114: WIDER submission text file."""
    target = Path(results_dir or f"{split}_results") / img_path.replace("jpg", "txt")
    target.parent.mkdir(parents=True, exist_ok=True)
    dets = np.asarray(dets)
    # the submission format of the WIDER evaluation tool: image name, box count, then `left top width height score` per box with
    # rounded integer geometry (width = x2 - x1 + 1: the inclusive-pixel convention) and the raw score
    geometry = np.round(np.stack([dets[:, 0], dets[:, 1], dets[:, 2] - dets[:, 0] + 1, dets[:, 3] - dets[:, 1] + 1], axis=1)) if len(dets) else ()
    lines = [img_path.rsplit("/", 1)[-1], str(len(dets))]
    lines += [" ".join(str(int(v)) for v in g) + f" {d[4]}" for g, d in zip(geometry, dets)]
    target.write_text("\n".join(lines) + "\n")
