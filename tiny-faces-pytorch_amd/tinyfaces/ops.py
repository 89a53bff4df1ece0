"""Host-side wrappers of the HIP entry points (device tensors in, device tensors out).

Each function is the MI355X replacement of the reference call cited in its docstring
(file:line relative to the reference repo).  PyTorch only supplies memory and streams.
"""
import contextlib
import ctypes as C
import math

import numpy as np
import torch

from . import _hip
from ._hip import check, lib, ptr, require_gpu, stream

RF = {"size": [859, 859], "stride": [8, 8], "offset": [-1, -1]}      # tinyfaces/datasets/wider_face.py:55

_ws_cache = {}


def _workspace(key, nbytes, device):
    """Grow-only scratch buffers keyed by purpose + device (kernels never allocate)."""
    k = (key, str(device))
    buf = _ws_cache.get(k)
    # grow-only, except that a buffer of more than 1 GiB is given back once a request needs less than a quarter of it (one unusually
    # long candidate list must not pin gigabytes of NMS bit matrix for the rest of the process)
    if buf is None or buf.numel() < nbytes or (buf.numel() > (1 << 30) and nbytes * 4 < buf.numel()):
        _ws_cache.pop(k, None)
        buf = None
        buf = torch.empty(int(nbytes * 1.25) + 256, dtype=torch.uint8, device=device)
        _ws_cache[k] = buf
    return buf


# --------------------------------------------------------------------------- targets
def check_compensate(compensate, pos_thresh=0.7):
    """compensate=(N, T) of the scale-compensated matching (include/tinyfaces_hip.h): N an integer in 1..64, T finite with
    0.01 <= T < pos_thresh.  Returns (int N, float T), or None for None; anything else raises ValueError."""
    if compensate is None:
        return None
    try:
        n, t = compensate
    except (TypeError, ValueError):
        raise ValueError(f"compensate must be None or a pair (N, T), not {compensate!r}") from None
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= 64:
        raise ValueError(f"compensate: N must be an integer in 1..64, not {n!r}")
    if isinstance(t, bool) or not isinstance(t, (int, float, np.integer, np.floating)) or not math.isfinite(float(t)) \
            or not 0.01 <= float(t) < float(pos_thresh):
        raise ValueError(f"compensate: T must be finite with 0.01 <= T < pos_thresh = {pos_thresh}, not {t!r}")
    return int(n), float(t)


IGNORE_MEASURES = {"iof": 0, "iou": 1}                    # TF_IGNORE_* (include/tinyfaces_hip.h)
IGNORE_DEFAULT = ("iof", 0.5)
_NO_GUARD = contextlib.nullcontext()                      # the resident entries launch on the caller's current device


def check_ignore(ignore):
    """ignore=(measure, thresh) of the ignore regions (include/tinyfaces_hip.h): measure "iof" (intersection over the anchor's area) or "iou",
    thresh finite in (0, 1].  Returns (str measure, float thresh), or None for None; anything else raises ValueError."""
    if ignore is None:
        return None
    try:
        measure, thresh = ignore
    except (TypeError, ValueError):
        raise ValueError(f"ignore must be None or a pair (measure, thresh), not {ignore!r}") from None
    if not isinstance(measure, str) or measure not in IGNORE_MEASURES:
        raise ValueError(f"ignore: measure must be one of {sorted(IGNORE_MEASURES)}, not {measure!r}")
    if isinstance(thresh, bool) or not isinstance(thresh, (int, float, np.integer, np.floating)) or not math.isfinite(float(thresh)) \
            or not 0.0 < float(thresh) <= 1.0:
        raise ValueError(f"ignore: thresh must be finite with 0 < thresh <= 1, not {thresh!r}")
    return measure, float(thresh)


def _valid_boxes(boxes_per_image):
    """Per image the non-degenerate rows (processor.py:228-232) of (G_i, 4) arrays / tensors as float64 -> (list of kept, offsets)."""
    kept, offs = [], [0]
    for b in boxes_per_image:
        b = torch.as_tensor(np.asarray(b.cpu() if torch.is_tensor(b) else b), dtype=torch.float64).reshape(-1, 4)
        valid = ~((b[:, 2] <= b[:, 0]) | (b[:, 3] <= b[:, 1]))
        kept.append(b[valid])
        offs.append(offs[-1] + int(valid.sum()))
    return kept, offs


def _upload_boxes(boxes_per_image, device):
    """`_valid_boxes` on `device`, for faces and ignore boxes alike -> (boxes_d (total, 4) f64 -- one zero row when there is none --,
    offs_d (B + 1,) i32, total)."""
    kept, offs = _valid_boxes(boxes_per_image)
    boxes_d = (torch.cat(kept) if offs[-1] else torch.zeros(1, 4, dtype=torch.float64)).contiguous().to(device)
    return boxes_d, torch.tensor(offs, dtype=torch.int32, device=device), offs[-1]


def _upload_templates(templates, device):
    """The template table as a contiguous float64 tensor on `device`, from an ndarray, a CPU tensor or a device tensor; one that already is
    all of that comes back as it is, without a copy."""
    if torch.is_tensor(templates) and templates.is_cuda:
        return templates.to(device=device, dtype=torch.float64).contiguous()
    return torch.as_tensor(np.asarray(templates), dtype=torch.float64).contiguous().to(device)


def _launch_ignore(cls, t_d, rf, ign_d, ioffs_d, total, ign, want_count):
    """tf_targets_apply_ignore on resident operands, in place on cls (B, nt, vsy, vsx).  Returns the (B,) int32 counter of labels turned
    (zeroed here) or None.  No ignore box in the batch: nothing is enqueued."""
    B, nt, vsy, vsx = cls.shape
    changed = torch.zeros(B, dtype=torch.int32, device=cls.device) if want_count else None
    if int(total) > 0:
        ofy, ofx = rf["offset"]
        sty, stx = rf["stride"]
        check(lib().tf_targets_apply_ignore(ptr(cls), B, nt, vsy, vsx, ptr(t_d), t_d.shape[1], ofy, ofx, sty, stx, ptr(ign_d), ptr(ioffs_d),
                                            IGNORE_MEASURES[ign[0]], ign[1], ptr(changed), stream()), "tf_targets_apply_ignore")
    return changed


def targets_apply_ignore(class_map, ignore_boxes_per_image, templates, rf=RF, ignore=IGNORE_DEFAULT, return_count=False):
    """Ignore regions on a class map (B, nt, vsy, vsx) f32 on the device, IN PLACE (tf_targets_apply_ignore; the rule is in
    include/tinyfaces_hip.h): a negative anchor (-1) that one of its image's ignore boxes covers by at least thresh becomes 0; +1 and 0 stay.
    ignore_boxes_per_image: list of (K_i, 4) float64 arrays / tensors (x1, y1, x2, y2) in the frame of the targets; degenerate ones
    (x2 <= x1 or y2 <= y1) are dropped as faces are.  ignore = (measure, thresh), measure "iof" | "iou".
    Returns class_map [, the (B,) int32 device tensor of labels turned per image]."""
    ign = check_ignore(ignore)
    if ign is None:
        raise ValueError("targets_apply_ignore: ignore=(measure, thresh) is required")
    require_gpu(class_map, "targets_apply_ignore")
    if class_map.dtype != torch.float32 or class_map.dim() != 4 or not class_map.is_contiguous():
        raise ValueError("targets_apply_ignore: class_map is a contiguous float32 (B, nt, vsy, vsx) tensor")
    if len(ignore_boxes_per_image) != class_map.shape[0]:
        raise ValueError(f"targets_apply_ignore: {len(ignore_boxes_per_image)} lists of ignore boxes for {class_map.shape[0]} images")
    dev = class_map.device
    t_d = _upload_templates(templates, dev)
    with torch.cuda.device(dev):
        changed = _launch_ignore(class_map, t_d, rf, *_upload_boxes(ignore_boxes_per_image, dev), ign, return_count)
    return (class_map, changed) if return_count else class_map


def _launch_targets(comp, total, boxes_d, offs_d, B, t_d, nt, tstride, vsy, vsx, rf, paste_d, flips_d, noise_d, noff_d, seed, pos_thresh,
                    neg_thresh, cls, reg, device, return_match_count):
    """The one place both target wrappers call the library from: tf_dense_overlap_targets, or with comp = (N, T) its compensated form.
    Returns the match-count tensor (total,) int32, or None."""
    ofy, ofx = rf["offset"]
    sty, stx = rf["stride"]
    if comp is None:
        wsb = lib().tf_targets_workspace_bytes(total)
        ws = _workspace("targets", wsb, device)
        check(lib().tf_dense_overlap_targets(ptr(boxes_d), ptr(offs_d), B, ptr(t_d), nt, tstride, vsy, vsx, ofy, ofx, sty, stx,
                                             ptr(paste_d), ptr(flips_d), ptr(noise_d), ptr(noff_d), int(seed) & (2**64 - 1),
                                             float(pos_thresh), float(neg_thresh), ptr(cls), ptr(reg), ptr(ws), wsb, stream()),
              "tf_dense_overlap_targets")
        return None
    mc = torch.empty(total, dtype=torch.int32, device=device) if return_match_count else None
    wsb = lib().tf_targets_comp_workspace_bytes(total, B, nt, vsy, vsx)
    ws = _workspace("targets_comp", wsb, device)
    check(lib().tf_dense_overlap_targets_comp(ptr(boxes_d), ptr(offs_d), B, ptr(t_d), nt, tstride, vsy, vsx, ofy, ofx, sty, stx,
                                              ptr(paste_d), ptr(flips_d), ptr(noise_d), ptr(noff_d), int(seed) & (2**64 - 1),
                                              float(pos_thresh), float(neg_thresh), comp[0], comp[1], ptr(mc) if total else None,
                                              ptr(cls), ptr(reg), ptr(ws), wsb, stream()), "tf_dense_overlap_targets_comp")
    return mc


def _upload_lists(who, boxes_per_image, templates, paste_boxes, flips, ignore_boxes, device):
    """What the two list entries hand to `_assign_resident`: their host operands on `device`, in the layout it takes."""
    if ignore_boxes is not None and len(ignore_boxes) != len(boxes_per_image):
        raise ValueError(f"{who}: {len(ignore_boxes)} lists of ignore boxes for {len(boxes_per_image)} images")
    device = torch.device(device if device is not None else "cuda")
    if device.type != "cuda":
        raise RuntimeError(f"{who}: HIP kernel only (no CPU fallback)")
    B = len(boxes_per_image)
    faces, t_d = _upload_boxes(boxes_per_image, device), _upload_templates(templates, device)
    paste_d = None if paste_boxes is None else torch.as_tensor(np.asarray(paste_boxes), dtype=torch.int32).reshape(B, 4).to(device)
    flips_d = None if flips is None else torch.as_tensor(np.asarray(flips), dtype=torch.int32).reshape(B).to(device)
    return faces, t_d, paste_d, flips_d, None if ignore_boxes is None else _upload_boxes(ignore_boxes, device), None, None


def _resident_operands(who, boxes_d, offs_d, total_boxes, templates_d, paste_d, flips_d, ignore_d, ignore_offs_d, total_ignore):
    """What the two resident entries hand to `_assign_resident`: their operands as they are, in the layout it takes."""
    if ignore_d is not None and (ignore_offs_d is None or ignore_offs_d.numel() != offs_d.numel()):
        raise ValueError(f"{who}: ignore_offs_d is an int32 (B + 1,) device tensor next to ignore_d")
    return ((boxes_d, offs_d, int(total_boxes)), templates_d, paste_d, flips_d,
            None if ignore_d is None else (ignore_d, ignore_offs_d, int(total_ignore)), None, None)


def _assign_resident(who, operands, heatmap_size, rf, out, has_ignore, ignore_names, ignore, return_match_count, return_ignored_count, comp=None,
                     topk=None, seed=0, pos_thresh=0.7, neg_thresh=0.3):
    """The one path of the four target entries (`who` names the caller in messages).  operands = ((boxes_d, offs_d, total), templates_d, paste_d,
    flips_d, (ignore_d, ignore_offs_d, total_ignore) or None, noise_d, noise_offs_d), all resident -- or a function that uploads and returns
    them, called under the guard of its device once every keyword has passed.  topk: the ATSS assigner; else dense_overlap, with comp = (N, T)
    its compensated form.  Returns cls, reg[, match_count][, ignored_count]."""
    ign = check_ignore(ignore)
    if return_match_count and comp is None and topk is None:
        raise ValueError("return_match_count needs compensate=(N, T)")
    if return_ignored_count and not has_ignore:
        raise ValueError(f"return_ignored_count needs {ignore_names}")
    guard = _NO_GUARD
    if callable(operands):
        operands = operands()
        guard = torch.cuda.device(operands[1].device)
    (boxes_d, offs_d, total), t_d, paste_d, flips_d, ignores, noise_d, noff_d = operands
    require_gpu(boxes_d, who)
    B, (vsy, vsx), (nt, tstride), dev = offs_d.numel() - 1, heatmap_size, t_d.shape, boxes_d.device
    if out is None:
        out = (torch.empty(B, nt, vsy, vsx, dtype=torch.float32, device=dev), torch.empty(B, 4 * nt, vsy, vsx, dtype=torch.float32, device=dev))
    cls, reg = out
    with guard:
        if topk is not None:
            mc = _launch_atss(total, boxes_d, offs_d, B, t_d, vsy, vsx, rf, paste_d, flips_d, topk, cls, reg, dev, return_match_count)
        else:
            mc = _launch_targets(comp, total, boxes_d, offs_d, B, t_d, nt, tstride, vsy, vsx, rf, paste_d, flips_d, noise_d, noff_d, seed,
                                 pos_thresh, neg_thresh, cls, reg, dev, return_match_count)
        res = (cls, reg) + ((mc,) if return_match_count else ())
        if ignores is not None:
            ic = _launch_ignore(cls, t_d, rf, *ignores, ign or IGNORE_DEFAULT, return_ignored_count)
            if return_ignored_count:
                res += (ic,)
    return res


def dense_overlap_targets(boxes_per_image, templates, heatmap_size=(63, 63), rf=RF, paste_boxes=None, flips=None,
                          noise=None, seed=0, pos_thresh=0.7, neg_thresh=0.3, device=None, compensate=None, return_match_count=False,
                          ignore_boxes=None, ignore=None, return_ignored_count=False):
    """compute_dense_overlap + DataProcessor.get_padding/get_regression/get_heatmaps fused
    (tinyfaces/datasets/dense_overlap.py:4-75, tinyfaces/datasets/processor.py:114-277).

    boxes_per_image: list of (G_i, 4) float64 arrays/tensors (x1,y1,x2,y2).
    noise: optional list of (vsy,vsx,nt,G_i_valid) float64 arrays = the np.random.rand draw of
           processor.py:195 (for bit-parity tests); default: device counter RNG seeded by `seed`.
    compensate: None, or (N, T): every face is topped up to N positive anchors from its own best anchors with perturbed IoU >= T
           (scale-compensated matching, the rule in include/tinyfaces_hip.h); the regression map does not change.
    return_match_count: with compensate, also return the (total_valid_boxes,) int32 device tensor of positives per face.
    ignore_boxes: None, or a list of (K_i, 4) float64 ignore boxes per image, in the frame of `boxes_per_image` (already mirrored where the
           image is): behind everything else a negative anchor that one of them covers gets the don't-care label 0 (`targets_apply_ignore`,
           the rule in include/tinyfaces_hip.h); positives and the regression map do not change.  ignore = (measure, thresh), None = ("iof", 0.5).
    return_ignored_count: with ignore_boxes, also return the (B,) int32 device tensor of labels turned per image.
    Returns class_map (B,nt,vsy,vsx) f32 and regression_map (B,4nt,vsy,vsx) f32 on `device`
    -- the CHW layout WIDERFace.__getitem__ hands to the trainer (wider_face.py:186-187) -- [, match_count][, ignored_count]."""
    comp = check_compensate(compensate, pos_thresh)

    def upload():
        operands = _upload_lists("dense_overlap_targets", boxes_per_image, templates, paste_boxes, flips, ignore_boxes, device)
        if noise is None:
            return operands
        t_d, (vsy, vsx) = operands[1], heatmap_size
        flat, noff, offs = [], [0], _valid_boxes(boxes_per_image)[1]
        for i, nz in enumerate(noise):
            nz = np.ascontiguousarray(np.asarray(nz, dtype=np.float64))
            assert nz.shape == (vsy, vsx, t_d.shape[0], offs[i + 1] - offs[i]), nz.shape
            flat.append(nz.reshape(-1))
            noff.append(noff[-1] + nz.size)
        cat = np.concatenate(flat) if noff[-1] else np.zeros(1)
        return operands[:5] + (torch.from_numpy(cat).to(t_d.device), torch.tensor(noff, dtype=torch.int64, device=t_d.device))

    return _assign_resident("dense_overlap_targets", upload, heatmap_size, rf, None, ignore_boxes is not None, "ignore_boxes", ignore,
                            return_match_count, return_ignored_count, comp=comp, seed=seed, pos_thresh=pos_thresh, neg_thresh=neg_thresh)


def dense_overlap_targets_device(boxes_d, offs_d, total_boxes, templates_d, heatmap_size=(63, 63), rf=RF, paste_d=None, flips_d=None,
                                 seed=0, pos_thresh=0.7, neg_thresh=0.3, out=None, compensate=None, return_match_count=False,
                                 ignore_d=None, ignore_offs_d=None, total_ignore=0, ignore=None, return_ignored_count=False):
    """Same kernel as dense_overlap_targets with every operand already resident in HBM:
    boxes_d (total,4) f64 (degenerate boxes removed), offs_d (B+1,) i32, templates_d (nt,5) f64, paste_d (B,4) i32.
    compensate / return_match_count: as in dense_overlap_targets.
    ignore_d (total_ignore, 4) f64 (degenerate boxes removed) under ignore_offs_d (B+1,) i32, total_ignore the host's copy of its last entry:
    the ignore regions of dense_overlap_targets(ignore_boxes=); ignore / return_ignored_count as there."""
    comp = check_compensate(compensate, pos_thresh)
    operands = _resident_operands("dense_overlap_targets_device", boxes_d, offs_d, total_boxes, templates_d, paste_d, flips_d, ignore_d, ignore_offs_d,
                                  total_ignore)
    return _assign_resident("dense_overlap_targets_device", operands, heatmap_size, rf, out, ignore_d is not None, "ignore_d / ignore_offs_d", ignore,
                            return_match_count, return_ignored_count, comp=comp, seed=seed, pos_thresh=pos_thresh, neg_thresh=neg_thresh)


ASSIGNERS = ("dense_overlap", "atss", "tal")
ATSS_TOPK = 9                                             # ATSSAssigner's default


def check_assigner(assigner, atss_topk=ATSS_TOPK, compensate=None):
    """assigner "dense_overlap" (the reference's fixed thresholds), "atss" (include/tinyfaces_hip.h, "ATSS") or "tal" (there, "TAL": the loader
    delivers the base maps and the resident faces, the criterion assigns from the predictions; its own parameters go through `check_tal`);
    atss_topk an integer in 1..16, the candidates per template and face.  compensate next to "atss" or "tal" is refused: the compensation stage is defined on the perturbed-IoU owner
    of dense_overlap's first stage, which ATSS does not compute.  Returns (str assigner, int atss_topk); anything else raises ValueError."""
    if not isinstance(assigner, str) or assigner not in ASSIGNERS:
        raise ValueError(f"assigner must be one of {list(ASSIGNERS)}, not {assigner!r}")
    if isinstance(atss_topk, bool) or not isinstance(atss_topk, (int, np.integer)) or not 1 <= int(atss_topk) <= 16:
        raise ValueError(f"atss_topk must be an integer in 1..16, not {atss_topk!r}")
    if assigner == "atss" and compensate is not None:
        raise ValueError("assigner='atss' does not take compensate / anchor_compensation: the compensation stage tops up the owner that the "
                         "dense_overlap assignment computes; ATSS already gives every face a comparable number of positives")
    if assigner == "tal" and compensate is not None:
        raise ValueError("assigner='tal' does not take compensate / anchor_compensation: the compensation stage tops up the owner that the "
                         "dense_overlap assignment computes; TAL gives every face up to tal_topk positives of its own choosing")
    return assigner, int(atss_topk)


def _launch_atss(total, boxes_d, offs_d, B, t_d, vsy, vsx, rf, paste_d, flips_d, k, cls, reg, device, return_match_count):
    """tf_targets_atss on resident operands.  Returns the match-count tensor (total,) int32, or None."""
    ofy, ofx = rf["offset"]
    sty, stx = rf["stride"]
    nt, tstride = t_d.shape
    mc = torch.empty(total, dtype=torch.int32, device=device) if return_match_count else None
    wsb = lib().tf_targets_atss_workspace_bytes(total, B, nt, vsy, vsx)
    ws = _workspace("targets_atss", wsb, device)
    check(lib().tf_targets_atss(ptr(boxes_d), ptr(offs_d), B, ptr(t_d), nt, tstride, vsy, vsx, ofy, ofx, sty, stx, ptr(paste_d), ptr(flips_d),
                                k, ptr(mc) if total else None, ptr(cls), ptr(reg), ptr(ws), wsb, stream()), "tf_targets_atss")
    return mc


def atss_targets(boxes_per_image, templates, heatmap_size=(63, 63), rf=RF, paste_boxes=None, flips=None, topk=ATSS_TOPK, device=None,
                 return_match_count=False, ignore_boxes=None, ignore=None, return_ignored_count=False):
    """ATSS target assignment (tf_targets_atss; the rule is in include/tinyfaces_hip.h): per face the `topk` unpadded cells of every template
    nearest to its centre are candidates, positive from mean + std of their IoUs when the anchor centre lies inside the face, the best
    candidate when there is none; an anchor two faces claim goes to the larger IoU.  No thresholds, no noise, no seed.
    The operands and the two maps are those of dense_overlap_targets: class_map (B,nt,vsy,vsx) f32 in {-1, +1} (0 only through ignore_boxes),
    regression_map (B,4nt,vsy,vsx) f32, zero away from the positives.
    return_match_count: also the (total_valid_boxes,) int32 device tensor of anchors each face won.
    ignore_boxes / ignore / return_ignored_count: the ignore pass behind the call, as in dense_overlap_targets; passing the faces themselves with
    ignore=("iou", t) makes a grey band of near-miss negatives around them."""
    _, k = check_assigner("atss", topk)
    return _assign_resident("atss_targets", lambda: _upload_lists("atss_targets", boxes_per_image, templates, paste_boxes, flips, ignore_boxes, device),
                            heatmap_size, rf, None, ignore_boxes is not None, "ignore_boxes", ignore, return_match_count, return_ignored_count, topk=k)


def atss_targets_device(boxes_d, offs_d, total_boxes, templates_d, heatmap_size=(63, 63), rf=RF, paste_d=None, flips_d=None, topk=ATSS_TOPK,
                        out=None, return_match_count=False, ignore_d=None, ignore_offs_d=None, total_ignore=0, ignore=None,
                        return_ignored_count=False):
    """Same kernels as atss_targets with every operand already resident in HBM, as dense_overlap_targets_device takes them:
    boxes_d (total,4) f64 (degenerate boxes removed), offs_d (B+1,) i32, templates_d (nt,5) f64, paste_d (B,4) i32, flips_d (B,) i32;
    out = (class_map, regression_map) to write into; ignore_d / ignore_offs_d / total_ignore / ignore / return_ignored_count as there."""
    _, k = check_assigner("atss", topk)
    operands = _resident_operands("atss_targets_device", boxes_d, offs_d, total_boxes, templates_d, paste_d, flips_d, ignore_d, ignore_offs_d, total_ignore)
    return _assign_resident("atss_targets_device", operands, heatmap_size, rf, out, ignore_d is not None, "ignore_d / ignore_offs_d", ignore,
                            return_match_count, return_ignored_count, topk=k)


TAL_TOPK, TAL_ALPHA, TAL_BETA = 13, 1.0, 6.0              # mmdetection's TaskAlignedAssigner defaults


def check_tal(topk=TAL_TOPK, alpha=TAL_ALPHA, beta=TAL_BETA):
    """The parameters of the task-aligned assignment (include/tinyfaces_hip.h, "TAL"): topk an integer in 1..32, alpha finite and >= 0, beta
    finite and > 0.  Returns (int topk, float alpha, float beta); anything else raises ValueError."""
    if isinstance(topk, bool) or not isinstance(topk, (int, np.integer)) or not 1 <= int(topk) <= 32:
        raise ValueError(f"tal: topk must be an integer in 1..32, not {topk!r}")
    for name, v, ok in (("alpha", alpha, lambda x: x >= 0), ("beta", beta, lambda x: x > 0)):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(float(v)) or not ok(float(v)):
            raise ValueError(f"tal: {name} must be a finite number {'>= 0' if name == 'alpha' else '> 0'}, not {v!r}")
    return int(topk), float(alpha), float(beta)


def tal_assign_device(output, class_map, regression_map, boxes_d, offs_d, total_boxes, templates_d, heatmap_size=None, rf=RF, paste_d=None,
                      flips_d=None, topk=TAL_TOPK, alpha=TAL_ALPHA, beta=TAL_BETA, return_match_count=False, align_out=None):
    """Task-aligned assignment (tf_targets_tal; the rule is in include/tinyfaces_hip.h, "TAL") with every operand resident, IN PLACE on the two
    maps: per face the anchors whose centre lies strictly inside it are measured by sigmoid(logit)^alpha * IoU(predicted box, face)^beta, the
    face claims its `topk` best, an anchor two faces claim goes to the larger IoU, and every won anchor gets +1 and the face's four regression
    values.  Nothing else of either map is written: they arrive as the base maps (an assignment without faces, ignore pass applied).
    output (B, 5 nt, vsy, vsx) f32 contiguous, the head's output (only read; nothing flows back into it); class_map (B, nt, vsy, vsx) f32,
    regression_map (B, 4 nt, vsy, vsx) f32, both contiguous; boxes_d (total, 4) f64 (degenerate boxes removed), offs_d (B + 1,) i32, total_boxes
    the host's copy of its last entry, templates_d (nt, >= 4) f64, paste_d (B, 4) i32, flips_d (B,) i32.  heatmap_size, if given, must be the maps'.
    align_out: a contiguous float32 tensor of class_map's shape selects tf_targets_tal_aligned (step 7 of the rule): the same assignment, and
    align_out is written COMPLETELY (it may arrive holding anything): 1 everywhere, and at every won anchor TOOD's normalised alignment
    m / max m * max u, the maxima over the anchors the face won.  It is the align_map of criterion_aligned_fwd_bwd.
    Returns (class_map, regression_map[, match_count (total,) int32]).  No face in the batch: nothing is enqueued (align_out is filled with 1)."""
    k, a, bt = check_tal(topk, alpha, beta)
    require_gpu(output, "tal_assign_device")
    if align_out is not None and (not torch.is_tensor(align_out) or align_out.dtype != torch.float32 or not align_out.is_contiguous() or
                                  align_out.device != output.device or align_out.shape != class_map.shape):
        raise ValueError("tal_assign_device: align_out is a contiguous float32 tensor of class_map's shape on the output's device")
    for name, v in (("output", output), ("class_map", class_map), ("regression_map", regression_map)):
        if not torch.is_tensor(v) or v.dtype != torch.float32 or v.dim() != 4 or not v.is_contiguous() or v.device != output.device:
            raise ValueError(f"tal_assign_device: {name} is a contiguous float32 4-d tensor on the output's device")
    B, nt, vsy, vsx = class_map.shape
    if output.shape != (B, 5 * nt, vsy, vsx) or regression_map.shape != (B, 4 * nt, vsy, vsx):
        raise ValueError(f"tal_assign_device: output {tuple(output.shape)} / regression_map {tuple(regression_map.shape)} do not go with the "
                         f"class map {tuple(class_map.shape)}")
    if heatmap_size is not None and tuple(heatmap_size) != (vsy, vsx):
        raise ValueError(f"tal_assign_device: heatmap_size {tuple(heatmap_size)} is not the maps' {(vsy, vsx)}")
    if offs_d.numel() != B + 1 or templates_d.dim() != 2 or templates_d.shape[0] != nt or templates_d.dtype != torch.float64 or boxes_d.dtype != torch.float64:
        raise ValueError("tal_assign_device: offs_d is (B + 1,) int32, templates_d (nt, >= 4) float64 and boxes_d (total, 4) float64")
    total, dev = int(total_boxes), output.device
    mc = torch.empty(total, dtype=torch.int32, device=dev) if return_match_count else None
    if total > 0 and align_out is not None:
        ofy, ofx = rf["offset"]
        sty, stx = rf["stride"]
        wsb = lib().tf_targets_tal_aligned_workspace_bytes(total, B, nt, vsy, vsx)
        ws = _workspace("targets_tal_aligned", wsb, dev)
        check(lib().tf_targets_tal_aligned(ptr(output), ptr(boxes_d), ptr(offs_d), B, ptr(templates_d), nt, templates_d.shape[1], vsy, vsx, ofy, ofx, sty,
                                           stx, ptr(paste_d), ptr(flips_d), k, a, bt, ptr(mc), ptr(class_map), ptr(regression_map), ptr(align_out),
                                           ptr(ws), wsb, stream()), "tf_targets_tal_aligned")
    elif align_out is not None:
        align_out.fill_(1.0)
    elif total > 0:
        ofy, ofx = rf["offset"]
        sty, stx = rf["stride"]
        wsb = lib().tf_targets_tal_workspace_bytes(total, B, nt, vsy, vsx)
        ws = _workspace("targets_tal", wsb, dev)
        check(lib().tf_targets_tal(ptr(output), ptr(boxes_d), ptr(offs_d), B, ptr(templates_d), nt, templates_d.shape[1], vsy, vsx, ofy, ofx, sty, stx,
                                   ptr(paste_d), ptr(flips_d), k, a, bt, ptr(mc), ptr(class_map), ptr(regression_map), ptr(ws), wsb, stream()),
              "tf_targets_tal")
    return (class_map, regression_map) + ((mc,) if return_match_count else ())


def tal_assign(output, class_map, regression_map, boxes_per_image, templates, rf=RF, paste_boxes=None, flips=None, topk=TAL_TOPK,
               alpha=TAL_ALPHA, beta=TAL_BETA, return_match_count=False, align_out=None):
    """`tal_assign_device` from host lists: boxes_per_image a list of (G_i, 4) float64 arrays / tensors (degenerate ones are dropped), templates
    the (nt, 4 or 5) table, paste_boxes (B, 4) and flips (B,) as dense_overlap_targets takes them.  IN PLACE on the two device maps.  align_out as
    tal_assign_device takes it."""
    check_tal(topk, alpha, beta)
    require_gpu(output, "tal_assign")
    if len(boxes_per_image) != output.shape[0]:
        raise ValueError(f"tal_assign: {len(boxes_per_image)} lists of boxes for {output.shape[0]} images")
    with torch.cuda.device(output.device):
        (boxes_d, offs_d, total), t_d, paste_d, flips_d, _, _, _ = _upload_lists("tal_assign", boxes_per_image, templates, paste_boxes, flips, None,
                                                                                 output.device)
        if align_out is None:
            return tal_assign_device(output, class_map, regression_map, boxes_d, offs_d, total, t_d, None, rf, paste_d, flips_d, topk, alpha, beta,
                                     return_match_count)
        return tal_assign_device(output, class_map, regression_map, boxes_d, offs_d, total, t_d, None, rf, paste_d, flips_d, topk, alpha, beta,
                                 return_match_count, align_out=align_out)


def dense_overlap_iou(boxes, templates, heatmap_size=(63, 63), rf=RF, device="cuda"):
    """Raw rounded IoU tensor (vsy,vsx,nt,G) f64 of compute_dense_overlap (dense_overlap.py:4-75); test hook."""
    vsy, vsx = heatmap_size
    b = torch.as_tensor(np.asarray(boxes), dtype=torch.float64).reshape(-1, 4).contiguous().to(device)
    t = torch.as_tensor(np.asarray(templates), dtype=torch.float64).contiguous().to(device)
    G = b.shape[0]
    out = torch.zeros(vsy, vsx, t.shape[0], G, dtype=torch.float64, device=device)
    if G:
        ofy, ofx = rf["offset"]
        sty, stx = rf["stride"]
        check(lib().tf_dense_overlap_iou(ptr(b), G, ptr(t), t.shape[0], t.shape[1], vsy, vsx, ofy, ofx, sty, stx, ptr(out), stream()),
              "tf_dense_overlap_iou")
    return out


def pairwise_iou_distance(boxes, device="cuda"):
    """1 - IoU for every pair of (x1, y1, x2, y2) float64 boxes: the distance matrix of the template clustering
    (tinyfaces/clustering/cluster.py:28-37), (n, n) float64 device tensor, bit-exact with the reference's double loop."""
    b = torch.as_tensor(np.asarray(boxes), dtype=torch.float64).reshape(-1, 4).contiguous().to(device)
    require_gpu(b, "pairwise_iou_distance")
    n = b.shape[0]
    out = torch.empty(n, n, dtype=torch.float64, device=b.device)
    with torch.cuda.device(b.device):
        check(lib().tf_pairwise_iou_distance(ptr(b), n, ptr(out), stream()), "tf_pairwise_iou_distance")
    return out


# --------------------------------------------------------------------------- NMS
def nms(boxes, scores, iou_threshold):
    """torchvision.ops.nms semantics on float64 device tensors (call site tinyfaces/evaluation.py:84).
    Returns int64 indices of kept boxes in descending-score order.
    Score order (tf_nms_f64, include/tinyfaces_hip.h): that of torch.sort(scores, descending=True, stable=True) for ANY scores -- a NaN
    ranks above every number, +inf included, NaNs among themselves by input index; -0.0 == +0.0; equal scores keep input order.  The keep
    is always a duplicate-free list of indices into the input.  Box coordinates must be finite.  Any iou_threshold is taken as given:
    suppression is the strict `IoU > iou_threshold`, so a negative one suppresses disjoint boxes too (IoU 0), one >= 1 suppresses nothing,
    exact duplicates included, and a NaN IoU (0 / 0: two zero-area boxes) never suppresses."""
    require_gpu(boxes, "nms")
    boxes = boxes.to(torch.float64).contiguous()
    scores = scores.to(torch.float64).contiguous()
    n = boxes.shape[0]
    keep = torch.empty(max(n, 1), dtype=torch.int64, device=boxes.device)
    cnt = torch.zeros(1, dtype=torch.int32, device=boxes.device)
    wsb = lib().tf_nms_workspace_bytes(n)
    ws = _workspace("nms", wsb, boxes.device)
    with torch.cuda.device(boxes.device):
        check(lib().tf_nms_f64(ptr(boxes), ptr(scores), n, float(iou_threshold), ptr(keep), ptr(cnt), ptr(ws), wsb, stream()), "tf_nms_f64")
    return keep[: int(cnt.item())]


NMS_MAX_SEGMENTS = 64                                     # TF_NMS_MAX_SEGMENTS (include/tinyfaces_hip.h)
NMS_MASK_BUDGET_BYTES = 2 << 30                           # suppression bit matrices of ONE tf_nms_f64_batched call (n_s^2 / 8 bytes per segment)


def _mask_bytes(n):
    return n * ((n + 63) // 64) * 8


def nms_batched(boxes, scores, seg_offsets, iou_threshold, mask_budget_bytes=None, vote=None):
    """`_nms_batched_call` over groups of consecutive segments whose bit matrices fit `mask_budget_bytes` (default 2 GiB): at the
    evaluation default prob_thresh = 0.03 an image can have tens of thousands of candidates (300 MB of matrix each), so a 64-image
    batch in one call would ask for tens of GB of workspace.  A single segment larger than the budget still goes alone.
    Score order and threshold per segment as `nms`: torch.sort's order for any scores (NaN first, by input index; -0.0 == +0.0; ties keep
    input order), finite box coordinates, any iou_threshold (strict `>`: a negative one suppresses disjoint boxes).
    vote = (vote_thresh, weight): as in `_nms_batched_call`, returns (keeps, voted rows)."""
    offs = [int(o) for o in seg_offsets]
    budget = NMS_MASK_BUDGET_BYTES if mask_budget_bytes is None else int(mask_budget_bytes)
    S = len(offs) - 1
    sizes = [_mask_bytes(b - a) for a, b in zip(offs, offs[1:])]
    extra = () if vote is None else (vote,)                   # without a vote the calls are the ones they were
    if S < 1 or sum(sizes) <= budget:
        return _nms_batched_call(boxes, scores, offs, iou_threshold, *extra)
    out, rows, first, acc = [], [], 0, 0
    for s in range(S + 1):
        if s == S or (s > first and acc + sizes[s] > budget):
            a, b = offs[first], offs[s]
            keeps = _nms_batched_call(boxes[a:b], scores[a:b], [o - a for o in offs[first:s + 1]], iou_threshold, *extra)
            if vote is not None:
                keeps, voted = keeps
                rows += voted
            out += [k + a for k in keeps]                     # indices into the caller's concatenated input
            first, acc = s, 0
        if s < S:
            acc += sizes[s]
    return out if vote is None else (out, rows)


def _nms_batched_call(boxes, scores, seg_offsets, iou_threshold, vote=None):
    """S independent NMS problems in one call (BASELINE.json configs[4]: batched multi-scale NMS): segment s = rows
    [seg_offsets[s], seg_offsets[s+1]) of `boxes` / `scores` (float64, device) -- the multi-scale candidate list of image s of an
    evaluation batch (one evaluation.py:80-84 per image), or one list per pyramid level.  Returns a list of S int64 tensors: the kept
    indices INTO THE CONCATENATED INPUT of each segment, in descending-score order (torchvision.ops.nms semantics per segment).
    vote = (vote_thresh, weight): the box vote (`box_voting_batched`) is enqueued behind the NMS on its raw keep list and device-side
    counts, before the one synchronisation that reads the counts; returns (keeps, [(K_s, 5) voted rows in keep order])."""
    require_gpu(boxes, "nms_batched")
    offs = [int(o) for o in seg_offsets]
    S = len(offs) - 1
    if S < 1 or S > NMS_MAX_SEGMENTS or offs[0] != 0 or any(b < a for a, b in zip(offs, offs[1:])) or offs[-1] != boxes.shape[0]:
        raise ValueError(f"nms_batched: bad segment offsets {offs[:4]}... for {boxes.shape[0]} boxes (1..{NMS_MAX_SEGMENTS} segments)")
    boxes = boxes.to(torch.float64).contiguous()
    scores = scores.to(torch.float64).contiguous()
    n = offs[-1]
    keep = torch.empty(max(n, 1), dtype=torch.int64, device=boxes.device)
    cnt = torch.zeros(S, dtype=torch.int32, device=boxes.device)
    host = (C.c_int32 * (S + 1))(*offs)
    wsb = lib().tf_nms_batched_workspace_bytes(host, S)
    ws = _workspace("nms", wsb, boxes.device)
    with torch.cuda.device(boxes.device):
        check(lib().tf_nms_f64_batched(ptr(boxes), ptr(scores), host, S, float(iou_threshold), ptr(keep), ptr(cnt), ptr(ws), wsb, stream()),
              "tf_nms_f64_batched")
    voted = None if vote is None else _box_vote_launch(boxes, scores, host, S, keep, cnt, vote[0], vote[1])[0]
    counts = cnt.tolist()
    keeps = [keep[offs[s]: offs[s] + counts[s]] for s in range(S)]
    if vote is None:
        return keeps
    return keeps, [voted[offs[s]: offs[s] + counts[s]] for s in range(S)]


# --------------------------------------------------------------------------- test-time augmentation: box voting, un-mirroring
VOTE_WEIGHTS = {"sigmoid": 0, "score": 1}                 # TF_VOTE_WEIGHT_* (include/tinyfaces_hip.h)


def _vote_mode(vote_thresh, weight):
    if weight not in VOTE_WEIGHTS:
        raise ValueError(f"box_voting: weight={weight!r}, expected one of {sorted(VOTE_WEIGHTS)}")
    t = float(vote_thresh)
    if not 0.0 < t <= 1.0:
        raise ValueError(f"box_voting: vote_thresh={vote_thresh!r} is outside (0, 1]")
    return t, VOTE_WEIGHTS[weight]


def _box_vote_launch(boxes, scores, host_offs, S, keep, cnt, vote_thresh, weight, want_votes=False):
    """tf_box_vote_f64_batched on the raw device operands: keep (n,) int64 and cnt (S,) int32 as tf_nms_f64_batched left them.
    Returns ((n, 5) rows, (n,) int32 votes or None); rows >= cnt[s] of a segment are not written.  No host synchronisation."""
    t, mode = _vote_mode(vote_thresh, weight)
    n = boxes.shape[0]
    out = torch.empty(max(n, 1), 5, dtype=torch.float64, device=boxes.device)
    votes = torch.empty(max(n, 1), dtype=torch.int32, device=boxes.device) if want_votes else None
    with torch.cuda.device(boxes.device):
        check(lib().tf_box_vote_f64_batched(ptr(boxes), ptr(scores), host_offs, S, ptr(keep), ptr(cnt), t, mode, ptr(out), ptr(votes), stream()),
              "tf_box_vote_f64_batched")
    return out, votes


def box_voting_batched(boxes, scores, seg_offsets, keeps, vote_thresh, weight="sigmoid", num_keep=None, return_votes=False):
    """Box voting (Gidaris & Komodakis, ICCV 2015; Detectron's box_voting, scoring method ID) behind `nms_batched`, per segment: every
    kept box is replaced by the weighted mean of all candidates of its segment with IoU >= vote_thresh (the NMS's IoU, bit for bit); its own
    score stays.  weight: "sigmoid" (w = 1 / (1 + exp(-score)): decode_compact's scores are logits) or "score" (w = score); voters with
    w <= 0 or NaN are dropped, a kept box without voters stays as it is.  boxes (n, 4) / scores (n,) float64 device tensors.
    keeps: the list of S int64 index tensors `nms_batched` returns (indices into the concatenated input) -> a list of S (K_s, 5) tensors
    (x1, y1, x2, y2, score) in keep order [, a list of S (K_s,) int32 vote counts].
    num_keep (device int32 (S,)): `keeps` is then the RAW (n,) keep buffer of tf_nms_f64_batched and num_keep its device-side counts; nothing
    is synchronised and the raw (n, 5) rows [, (n,) votes] come back, of which only the first num_keep[s] of each segment are written."""
    require_gpu(boxes, "box_voting")
    offs = [int(o) for o in seg_offsets]
    S = len(offs) - 1
    if S < 1 or S > NMS_MAX_SEGMENTS or offs[0] != 0 or any(b < a for a, b in zip(offs, offs[1:])) or offs[-1] != boxes.shape[0]:
        raise ValueError(f"box_voting_batched: bad segment offsets {offs[:4]}... for {boxes.shape[0]} boxes (1..{NMS_MAX_SEGMENTS} segments)")
    _vote_mode(vote_thresh, weight)
    boxes = boxes.to(torch.float64).contiguous()
    scores = scores.to(torch.float64).contiguous()
    n, dev = offs[-1], boxes.device
    host = (C.c_int32 * (S + 1))(*offs)
    if num_keep is not None:
        require_gpu(num_keep, "box_voting")
        if num_keep.dtype != torch.int32 or num_keep.numel() != S or keeps.dtype != torch.int64 or keeps.numel() < n:
            raise ValueError("box_voting_batched: with num_keep, keeps is the raw int64 (n,) keep buffer and num_keep an int32 (S,) device tensor")
        out, votes = _box_vote_launch(boxes, scores, host, S, keeps.contiguous(), num_keep.contiguous(), vote_thresh, weight, return_votes)
        return (out, votes) if return_votes else out
    keeps = list(keeps)
    if len(keeps) != S:
        raise ValueError(f"box_voting_batched: {len(keeps)} keep lists for {S} segments")
    counts = [int(k.numel()) for k in keeps]
    if any(c > b - a for c, a, b in zip(counts, offs, offs[1:])):
        raise ValueError("box_voting_batched: a keep list is longer than its segment")
    keep = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
    for s, k in enumerate(keeps):
        if counts[s]:
            keep[offs[s]: offs[s] + counts[s]] = k.to(device=dev, dtype=torch.int64)
    cnt = torch.tensor(counts, dtype=torch.int32).to(dev)
    out, votes = _box_vote_launch(boxes, scores, host, S, keep, cnt, vote_thresh, weight, return_votes)
    rows = [out[offs[s]: offs[s] + counts[s]] for s in range(S)]
    if return_votes:
        return rows, [votes[offs[s]: offs[s] + counts[s]] for s in range(S)]
    return rows


def box_voting(boxes, scores, keep, vote_thresh, weight="sigmoid", num_keep=None, return_votes=False):
    """`box_voting_batched` for one candidate list: keep = the int64 indices `nms` returned -> (K, 5) voted rows in keep order
    [, (K,) int32 votes]; with num_keep (device int32 (1,)) keep is the raw (n,) keep buffer and the raw (n, 5) rows come back."""
    require_gpu(boxes, "box_voting")
    offs = [0, int(boxes.shape[0])]
    if num_keep is not None:
        return box_voting_batched(boxes, scores, offs, keep, vote_thresh, weight, num_keep, return_votes)
    res = box_voting_batched(boxes, scores, offs, [keep], vote_thresh, weight, None, return_votes)
    return (res[0][0], res[1][0]) if return_votes else res[0]


def boxes_unflip_(dets, first, last, max_rows, c):
    """In place: rows [first, last) of the (cap, 5) float64 candidate list `dets` get x1' = c - x2, x2' = c - x1 (tf_boxes_unflip_f64): the rows a
    MIRRORED pyramid level appended, mirrored back with c = (W_level - 1) * (1 / scale).  first / last: int32 device tensors of one element
    (copies of decode_compact's counter before and after the level); max_rows: host bound on last - first.  No host synchronisation."""
    require_gpu(dets, "boxes_unflip_")
    require_gpu(first, "boxes_unflip_")
    require_gpu(last, "boxes_unflip_")
    if dets.dtype != torch.float64 or dets.dim() != 2 or dets.shape[1] != 5 or not dets.is_contiguous():
        raise ValueError("boxes_unflip_: expected a contiguous float64 (cap, 5) tensor")
    if first.dtype != torch.int32 or last.dtype != torch.int32 or first.numel() != 1 or last.numel() != 1:
        raise ValueError("boxes_unflip_: first and last are int32 device tensors of one element")
    with torch.cuda.device(dets.device):
        check(lib().tf_boxes_unflip_f64(ptr(dets), ptr(first), ptr(last), int(max_rows), float(c), stream()), "tf_boxes_unflip_f64")
    return dets


# --------------------------------------------------------------------------- Soft-NMS
SOFT_NMS_METHODS = {"linear": 1, "gaussian": 2}           # TF_SOFT_NMS_* (include/tinyfaces_hip.h)
SOFT_NMS_MAX_BOXES = 65536                                # TF_SOFT_NMS_MAX_BOXES: one segment is selected inside one 1024-thread workgroup


def _soft_nms_mode(method, iou_threshold, sigma, score_threshold, score):
    """The host-side refusals of tf_soft_nms_f64_batched, raised before anything is launched."""
    if method not in SOFT_NMS_METHODS:
        raise ValueError(f"soft_nms: method={method!r}, expected one of {sorted(SOFT_NMS_METHODS)}")
    if score not in VOTE_WEIGHTS:
        raise ValueError(f"soft_nms: score={score!r}, expected one of {sorted(VOTE_WEIGHTS)}")
    t, sg, st = float(iou_threshold), float(sigma), float(score_threshold)
    if not 0.0 <= t <= 1.0:
        raise ValueError(f"soft_nms: iou_threshold={iou_threshold!r} is outside [0, 1]")
    if not sg > 0.0:
        raise ValueError(f"soft_nms: sigma={sigma!r} is not > 0")
    if not st >= 0.0:
        raise ValueError(f"soft_nms: score_threshold={score_threshold!r} is negative or NaN")
    return SOFT_NMS_METHODS[method], t, sg, st, VOTE_WEIGHTS[score]


def _max_keep(max_keep, what):
    """The cap of the *_capped forms: a positive integer."""
    if isinstance(max_keep, bool) or not isinstance(max_keep, (int, np.integer)) or max_keep < 1:
        raise ValueError(f"{what}: max_keep={max_keep!r}, expected an integer >= 1")
    return min(int(max_keep), 2**31 - 1)


def soft_nms(boxes, scores, method="linear", iou_threshold=0.3, sigma=0.5, score_threshold=0.001, score="sigmoid"):
    """Soft-NMS (Bodla et al., ICCV 2017; Detectron's soft_nms) on float64 device tensors, tf_soft_nms_f64: the best live candidate is
    selected, every live candidate that overlaps it is decayed -- "linear": s *= 1 - IoU where IoU > iou_threshold; "gaussian":
    s *= exp(-IoU^2 / sigma) where IoU > 0 --, the list is re-ranked, and a candidate lives while s >= score_threshold.
    score: "sigmoid" (s = 1 / (1 + exp(-score)): decode_compact's scores are logits) or "score" (s = score as given).
    Returns (keep int64 (K,), kept_scores float64 (K,)) in selection order: the decayed probabilities, non-increasing."""
    require_gpu(boxes, "soft_nms")
    res = soft_nms_batched(boxes, scores, [0, int(boxes.shape[0])], method, iou_threshold, sigma, score_threshold, score)
    return res[0]


def soft_nms_capped(boxes, scores, max_keep, method="linear", iou_threshold=0.3, sigma=0.5, score_threshold=0.001, score="sigmoid"):
    """`soft_nms` whose selection stops after max_keep rows (tf_soft_nms_f64_capped): the first max_keep rows of the uncapped call, bit for
    bit, without the serial rounds behind them.  A form of its own: the signature of `soft_nms` stays as it is."""
    _max_keep(max_keep, "soft_nms_capped")
    require_gpu(boxes, "soft_nms_capped")
    res = soft_nms_batched_capped(boxes, scores, [0, int(boxes.shape[0])], max_keep, method, iou_threshold, sigma, score_threshold, score)
    return res[0]


def soft_nms_batched_capped(boxes, scores, seg_offsets, max_keep, method="linear", iou_threshold=0.3, sigma=0.5, score_threshold=0.001,
                            score="sigmoid", mask_budget_bytes=None, vote=None):
    """`soft_nms_batched` with every segment's selection stopped after max_keep rows (tf_soft_nms_f64_batched_capped); a chained vote sees the
    capped counts on the device."""
    cap = _max_keep(max_keep, "soft_nms_batched_capped")
    return _soft_nms_segments(boxes, scores, seg_offsets, method, iou_threshold, sigma, score_threshold, score, mask_budget_bytes, vote, cap)


def soft_nms_batched(boxes, scores, seg_offsets, method="linear", iou_threshold=0.3, sigma=0.5, score_threshold=0.001, score="sigmoid",
                     mask_budget_bytes=None, vote=None):
    """`soft_nms` per segment [seg_offsets[s], seg_offsets[s+1]) in one tf_soft_nms_f64_batched call per group of consecutive segments whose
    adjacency bit matrices (n_s^2 / 8 bytes each) fit `mask_budget_bytes` (default NMS_MASK_BUDGET_BYTES), exactly as `nms_batched` groups.
    Returns a list of S (keep, kept_scores): keep indexes the CONCATENATED input.
    vote = (vote_thresh, weight): `box_voting_batched` is enqueued behind the selection on its device-side keep list and counts, before the
    one synchronisation; the vote's weights and membership use the candidates' ORIGINAL scores, column 4 of a voted row is the Soft-NMS
    score.  Returns (the list above, [(K_s, 5) voted rows in selection order])."""
    return _soft_nms_segments(boxes, scores, seg_offsets, method, iou_threshold, sigma, score_threshold, score, mask_budget_bytes, vote, 0)


def _soft_nms_segments(boxes, scores, seg_offsets, method, iou_threshold, sigma, score_threshold, score, mask_budget_bytes, vote, cap):
    """`soft_nms_batched` (cap = 0) and `soft_nms_batched_capped` (cap = max_keep)."""
    require_gpu(boxes, "soft_nms_batched")
    require_gpu(scores, "soft_nms_batched")
    mode = _soft_nms_mode(method, iou_threshold, sigma, score_threshold, score)
    if vote is not None:
        _vote_mode(vote[0], vote[1])
    offs = [int(o) for o in seg_offsets]
    S = len(offs) - 1
    if S < 1 or S > NMS_MAX_SEGMENTS or offs[0] != 0 or any(b < a for a, b in zip(offs, offs[1:])) or offs[-1] != boxes.shape[0]:
        raise ValueError(f"soft_nms_batched: bad segment offsets {offs[:4]}... for {boxes.shape[0]} boxes (1..{NMS_MAX_SEGMENTS} segments)")
    longest = max(b - a for a, b in zip(offs, offs[1:]))
    if longest > SOFT_NMS_MAX_BOXES:
        raise RuntimeError(f"soft_nms_batched: a segment of {longest} boxes exceeds the {SOFT_NMS_MAX_BOXES} one Soft-NMS selection takes "
                           f"(TF_SOFT_NMS_MAX_BOXES; the hard NMS takes {NMS_MAX_BOXES})")
    budget = NMS_MASK_BUDGET_BYTES if mask_budget_bytes is None else int(mask_budget_bytes)
    sizes = [_mask_bytes(b - a) for a, b in zip(offs, offs[1:])]
    boxes = boxes.to(torch.float64).contiguous()
    scores = scores.to(torch.float64).contiguous()
    # the calls of every group are enqueued first; the counts are read afterwards: one synchronisation whatever the number of groups
    calls, first, acc = [], 0, 0
    for s in range(S + 1):
        if s == S or (s > first and acc + sizes[s] > budget):
            a = offs[first]
            calls.append((first, s, _soft_nms_call(boxes[a:offs[s]], scores[a:offs[s]], [o - a for o in offs[first:s + 1]], mode, vote, cap)))
            first, acc = s, 0
        if s < S:
            acc += sizes[s]
    res, rows = [], []
    for first, last, (keep, kept, cnt, voted) in calls:
        counts, a = cnt.tolist(), offs[first]
        for s in range(first, last):
            lo, c = offs[s] - a, counts[s - first]
            k = keep[lo: lo + c]
            res.append((k + a if a else k, kept[lo: lo + c]))         # indices into the caller's concatenated input
            if voted is not None:
                rows.append(voted[lo: lo + c])
    return res if vote is None else (res, rows)


def _soft_nms_call(boxes, scores, offs, mode, vote, cap=0):
    """One tf_soft_nms_f64_batched[_capped] call [+ the chained vote] on contiguous float64 operands; nothing is synchronised.  Returns the raw
    (keep (n,), kept scores (n,), counts (S,), voted rows (n, 5) or None): only the first counts[s] rows of a segment are written."""
    method, t, sigma, st, smode = mode
    S, n, dev = len(offs) - 1, offs[-1], boxes.device
    keep = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    kept = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
    cnt = torch.zeros(S, dtype=torch.int32, device=dev)
    host = (C.c_int32 * (S + 1))(*offs)
    wsb = lib().tf_soft_nms_batched_workspace_bytes(host, S)
    ws = _workspace("soft_nms", wsb, dev)
    with torch.cuda.device(dev):
        if cap:
            check(lib().tf_soft_nms_f64_batched_capped(ptr(boxes), ptr(scores), host, S, method, t, sigma, st, smode, cap, ptr(keep), ptr(kept),
                                                       ptr(cnt), ptr(ws), wsb, stream()), "tf_soft_nms_f64_batched_capped")
        else:
            check(lib().tf_soft_nms_f64_batched(ptr(boxes), ptr(scores), host, S, method, t, sigma, st, smode, ptr(keep), ptr(kept), ptr(cnt),
                                                ptr(ws), wsb, stream()), "tf_soft_nms_f64_batched")
    voted = None
    if vote is not None:
        voted = _box_vote_launch(boxes, scores, host, S, keep, cnt, vote[0], vote[1])[0]
        voted[:, 4] = kept                                    # the vote kernel wrote the original score there; rows >= counts[s] hold nothing either way
    return keep, kept, cnt, voted


# --------------------------------------------------------------------------- Matrix NMS
MATRIX_NMS_METHODS = {"linear": 1, "gaussian": 2}         # TF_MATRIX_NMS_* (include/tinyfaces_hip.h)
MATRIX_NMS_MAX_BOXES = 524160                             # TF_MATRIX_NMS_MAX_BOXES: the hard NMS's limit; nothing of a segment lives in one workgroup


def _matrix_nms_mode(method, sigma, score_threshold, score, max_keep):
    """The host-side refusals of tf_matrix_nms_f64_batched, raised before anything is launched."""
    if method not in MATRIX_NMS_METHODS:
        raise ValueError(f"matrix_nms: method={method!r}, expected one of {sorted(MATRIX_NMS_METHODS)}")
    if score not in VOTE_WEIGHTS:
        raise ValueError(f"matrix_nms: score={score!r}, expected one of {sorted(VOTE_WEIGHTS)}")
    sg, st = float(sigma), float(score_threshold)
    if not sg > 0.0:
        raise ValueError(f"matrix_nms: sigma={sigma!r} is not > 0")
    if not st >= 0.0:
        raise ValueError(f"matrix_nms: score_threshold={score_threshold!r} is negative or NaN")
    cap = 0 if max_keep is None else _max_keep(max_keep, "matrix_nms")
    return MATRIX_NMS_METHODS[method], sg, st, VOTE_WEIGHTS[score], cap


def matrix_nms(boxes, scores, method="gaussian", sigma=0.5, score_threshold=0.001, score="sigmoid", max_keep=None):
    """Matrix NMS (Wang et al., SOLOv2; PaddleDetection's matrix_nms) on float64 device tensors, tf_matrix_nms_f64: Soft-NMS's kind of decay in
    closed form, with no serial selection.  Every candidate with p >= score_threshold is ranked by p; comp_j = its largest IoU with a better
    one; "linear": d_j = min over the better i (comp_i < 1) of (1 - IoU(i, j)) / (1 - comp_i); "gaussian": d_j = exp(-max_i (IoU(i, j)^2 -
    comp_i^2) / sigma) (SOLOv2's multiplier 2.0 is sigma = 0.5); s = p * d, emitted while s >= score_threshold.  There is no IoU threshold.
    score: "sigmoid" (p = 1 / (1 + exp(-score)): decode_compact's scores are logits) or "score" (p = score as given).  max_keep: at most that
    many rows, the first ones of the uncapped call.
    Returns (keep int64 (K,), kept_scores float64 (K,)) by s descending: the decayed probabilities."""
    res = matrix_nms_batched(boxes, scores, [0, int(boxes.shape[0])], method, sigma, score_threshold, score, max_keep)
    return res[0]


def matrix_nms_batched(boxes, scores, seg_offsets, method="gaussian", sigma=0.5, score_threshold=0.001, score="sigmoid", max_keep=None, vote=None):
    """`matrix_nms` per segment [seg_offsets[s], seg_offsets[s+1]) in ONE tf_matrix_nms_f64_batched call (the workspace is 68 bytes per
    candidate: there is no bit matrix to budget for, hence no grouping).  Returns a list of S (keep, kept_scores): keep indexes the CONCATENATED
    input.
    vote = (vote_thresh, weight): `box_voting_batched` is enqueued behind the call on its device-side keep list and counts, before the one
    synchronisation, as for `soft_nms_batched`: weights and membership from the candidates' ORIGINAL scores, column 4 of a voted row the
    decayed score.  Returns (the list above, [(K_s, 5) voted rows in keep order])."""
    method, sigma, st, smode, cap = _matrix_nms_mode(method, sigma, score_threshold, score, max_keep)     # ValueError: needs no device
    if vote is not None:
        _vote_mode(vote[0], vote[1])
    require_gpu(boxes, "matrix_nms_batched")
    require_gpu(scores, "matrix_nms_batched")
    offs = [int(o) for o in seg_offsets]
    S = len(offs) - 1
    if S < 1 or S > NMS_MAX_SEGMENTS or offs[0] != 0 or any(b < a for a, b in zip(offs, offs[1:])) or offs[-1] != boxes.shape[0]:
        raise ValueError(f"matrix_nms_batched: bad segment offsets {offs[:4]}... for {boxes.shape[0]} boxes (1..{NMS_MAX_SEGMENTS} segments)")
    longest = max(b - a for a, b in zip(offs, offs[1:]))
    if longest > MATRIX_NMS_MAX_BOXES:
        raise RuntimeError(f"matrix_nms_batched: a segment of {longest} boxes exceeds the {MATRIX_NMS_MAX_BOXES} one call takes (TF_MATRIX_NMS_MAX_BOXES)")
    boxes = boxes.to(torch.float64).contiguous()
    scores = scores.to(torch.float64).contiguous()
    n, dev = offs[-1], boxes.device
    keep = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
    kept = torch.empty(max(n, 1), dtype=torch.float64, device=dev)
    cnt = torch.zeros(S, dtype=torch.int32, device=dev)
    host = (C.c_int32 * (S + 1))(*offs)
    wsb = lib().tf_matrix_nms_batched_workspace_bytes(host, S)
    ws = _workspace("matrix_nms", wsb, dev)
    with torch.cuda.device(dev):
        check(lib().tf_matrix_nms_f64_batched(ptr(boxes), ptr(scores), host, S, method, sigma, st, smode, cap, ptr(keep), ptr(kept), ptr(cnt),
                                              ptr(ws), wsb, stream()), "tf_matrix_nms_f64_batched")
    voted = None
    if vote is not None:
        voted = _box_vote_launch(boxes, scores, host, S, keep, cnt, vote[0], vote[1])[0]
        voted[:, 4] = kept                                    # the vote kernel wrote the original score there; rows >= counts[s] hold nothing either way
    counts = cnt.tolist()                                     # the one synchronisation
    res = [(keep[offs[s]: offs[s] + counts[s]], kept[offs[s]: offs[s] + counts[s]]) for s in range(S)]
    if vote is None:
        return res
    return res, [voted[offs[s]: offs[s] + counts[s]] for s in range(S)]


# --------------------------------------------------------------------------- top-k selection in front of the suppression
def _topk_arguments(scores, seg_offsets, k, what):
    """The host-side refusals of tf_topk_select_f64_batched, raised before anything is enqueued (and before a device is asked for)."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError(f"{what}: k={k!r}, expected an integer >= 1")
    if not isinstance(scores, torch.Tensor) or scores.dim() != 1:
        raise ValueError(f"{what}: scores is a 1-d tensor of one score per candidate")
    offs = [int(o) for o in seg_offsets]
    S = len(offs) - 1
    if S < 1 or S > NMS_MAX_SEGMENTS or offs[0] != 0 or any(b < a for a, b in zip(offs, offs[1:])) or offs[-1] != scores.shape[0]:
        raise ValueError(f"{what}: bad segment offsets {offs[:4]}... for {scores.shape[0]} scores (1..{NMS_MAX_SEGMENTS} segments)")
    if offs[-1] > 2**31 - 1:
        raise ValueError(f"{what}: {offs[-1]} scores exceed the int32 segment offsets")
    k = min(int(k), 2**31 - 1)
    new = [0]
    for a, b in zip(offs, offs[1:]):
        new.append(new[-1] + min(b - a, k))
    return offs, k, new


def topk_select_batched(scores, seg_offsets, k):
    """Per segment [seg_offsets[s], seg_offsets[s+1]) of the float64 device tensor `scores`: the min(n_s, k) candidates that come first in
    the hard NMS's own order -- larger score, the lower index on a tie (-0.0 == +0.0), NaN behind every number -- as int64 indices into the
    CONCATENATED input in ASCENDING index order (tf_topk_select_f64_batched: a radix select, linear in n, the same bits on every run).
    Returns (idx, new_offsets): segment s of the compacted list is idx[new_offsets[s]: new_offsets[s+1]]; gather rows with index_select.
    Nothing is synchronised.  When no segment is longer than k nothing is launched and idx is None (the list is its own top-k)."""
    offs, k, new = _topk_arguments(scores, seg_offsets, k, "topk_select_batched")
    require_gpu(scores, "topk_select_batched")
    if new == offs:
        return None, new
    scores = scores.to(torch.float64).contiguous()
    S, dev = len(offs) - 1, scores.device
    idx = torch.empty(new[-1], dtype=torch.int64, device=dev)
    host = (C.c_int32 * (S + 1))(*offs)
    wsb = lib().tf_topk_batched_workspace_bytes(host, S, k)
    ws = _workspace("topk", wsb, dev)
    with torch.cuda.device(dev):
        check(lib().tf_topk_select_f64_batched(ptr(scores), host, S, k, ptr(idx), ptr(ws), wsb, stream()), "tf_topk_select_f64_batched")
    return idx, new


def topk_select(scores, k):
    """`topk_select_batched` for one candidate list -> (idx int64 (min(n, k),) ascending, or None when n <= k; [0, min(n, k)])."""
    n = int(scores.shape[0]) if isinstance(scores, torch.Tensor) and scores.dim() == 1 else 0
    offs, k, new = _topk_arguments(scores, [0, n], k, "topk_select")
    return topk_select_batched(scores, offs, k)


# --------------------------------------------------------------------------- WIDER evaluation: matching and the PR table on the device
WIDER_GT_TILE = 256                                       # TF_WIDER_GT_TILE: ground-truth boxes per LDS tile of the match kernel


def wider_rows(dets):
    """The rounding of evaluation.write_results on an (K,5) x1 y1 x2 y2 score array (numpy or tensor): rows in result-file form
    round([x1, y1, x2 - x1 + 1, y2 - y1 + 1]) half to even, the score untouched -- what read_predictions parses back from the file, so the
    in-memory path to the evaluator sees exactly what the file path reads.  Returns the type it was given, float64."""
    if isinstance(dets, torch.Tensor):
        d = dets.to(torch.float64).reshape(-1, 5)
        geometry = torch.round(torch.stack([d[:, 0], d[:, 1], d[:, 2] - d[:, 0] + 1, d[:, 3] - d[:, 1] + 1], dim=1)) + 0.0
        return torch.cat([geometry, d[:, 4:5]], dim=1)
    d = np.asarray(dets, dtype=np.float64).reshape(-1, 5)
    geometry = np.round(np.stack([d[:, 0], d[:, 1], d[:, 2] - d[:, 0] + 1, d[:, 3] - d[:, 1] + 1], axis=1)) + 0.0      # (the file holds "0", never "-0")
    return np.concatenate([geometry, d[:, 4:5]], axis=1)


def _wider_offsets(offsets, total, what, name):
    offs = [int(o) for o in offsets]
    if len(offs) < 2 or offs[0] != 0 or any(b < a for a, b in zip(offs, offs[1:])) or offs[-1] != total:
        raise ValueError(f"{what}: bad {name} offsets {offs[:4]}... for {total} rows (they start at 0, never descend and end at the row count)")
    if offs[-1] > 2**31 - 1:
        raise ValueError(f"{what}: {offs[-1]} rows exceed the int32 segment offsets")
    return offs


def wider_match_batched(rows, det_offsets, gt, gt_offsets, keep_masks, iou_thresh=0.5):
    """WIDER matching of a batch of images (tf_wider_match_f64_batched; host reference: wider_eval.image_evaluation).  rows (n,5) float64
    x, y, w, h, score, every segment [det_offsets[s], det_offsets[s+1]) score-descending; gt (g,4) x, y, w, h under gt_offsets (the same number
    of segments); keep_masks (nset, g) uint8 / bool, 1 = the box counts in that setting.  Returns (counted, recalled), int32 (nset, n): the
    running number of detections with proposal == 1 and pred_recall, per setting.  Nothing is synchronised."""
    what = "wider_match_batched"
    for name, t, cols in (("rows", rows, 5), ("gt", gt, 4)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[1] != cols:
            raise ValueError(f"{what}: {name} is a 2-d tensor of {cols} columns")
    if not isinstance(keep_masks, torch.Tensor) or keep_masks.dim() != 2 or keep_masks.shape[0] < 1 or keep_masks.shape[1] != gt.shape[0]:
        raise ValueError(f"{what}: keep_masks is an (nset >= 1, {gt.shape[0]}) tensor, one row per setting")
    if not math.isfinite(float(iou_thresh)):
        raise ValueError(f"{what}: iou_thresh={iou_thresh!r}")
    n, g, nset = int(rows.shape[0]), int(gt.shape[0]), int(keep_masks.shape[0])
    doffs, goffs = _wider_offsets(det_offsets, n, what, "detection"), _wider_offsets(gt_offsets, g, what, "ground-truth")
    if len(doffs) != len(goffs):
        raise ValueError(f"{what}: {len(doffs) - 1} detection segments but {len(goffs) - 1} ground-truth segments")
    require_gpu(rows, what)
    S, dev = len(doffs) - 1, rows.device
    rows = rows.to(torch.float64).contiguous()
    gt = gt.to(device=dev, dtype=torch.float64).contiguous()
    keep = keep_masks.to(device=dev, dtype=torch.uint8).contiguous()
    counted = torch.empty(nset, n, dtype=torch.int32, device=dev)
    recalled = torch.empty(nset, n, dtype=torch.int32, device=dev)
    if n == 0:
        return counted, recalled
    wsb = lib().tf_wider_match_workspace_bytes(n, g)
    ws = _workspace("wider_match", wsb, dev)
    with torch.cuda.device(dev):
        check(lib().tf_wider_match_f64_batched(ptr(rows), (C.c_int32 * (S + 1))(*doffs), ptr(gt), (C.c_int32 * (S + 1))(*goffs), S, ptr(keep), nset,
                                               float(iou_thresh), ptr(counted), ptr(recalled), ptr(ws), wsb, stream()), "tf_wider_match_f64_batched")
    return counted, recalled


def wider_pr_accumulate(scores, det_offsets, counted, recalled, lo_d, thresh, pr):
    """Adds image_pr_info, summed over the segments, into pr (nset, T, 2) int64 in place (tf_wider_pr_accumulate).  scores (n,) float64 raw
    scores, every segment non-increasing; counted / recalled (nset, n) int32 from `wider_match_batched`; lo_d: device float64 (2,) = (lo, d)
    of norm_scores; thresh: device float64 (T,) = 1 - (t + 1) / T.  Nothing is synchronised.  Returns pr."""
    what = "wider_pr_accumulate"
    if not isinstance(scores, torch.Tensor) or scores.dim() != 1:
        raise ValueError(f"{what}: scores is a 1-d tensor of one score per detection")
    n = int(scores.shape[0])
    offs = _wider_offsets(det_offsets, n, what, "detection")
    for name, t in (("counted", counted), ("recalled", recalled)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] != n or t.dtype != torch.int32:
            raise ValueError(f"{what}: {name} is an int32 (nset >= 1, {n}) tensor")
    nset = int(counted.shape[0])
    if recalled.shape[0] != nset:
        raise ValueError(f"{what}: counted has {nset} settings, recalled {recalled.shape[0]}")
    if not isinstance(lo_d, torch.Tensor) or lo_d.dtype != torch.float64 or lo_d.numel() != 2:
        raise ValueError(f"{what}: lo_d is a float64 tensor of (lo, d)")
    if not isinstance(thresh, torch.Tensor) or thresh.dtype != torch.float64 or thresh.dim() != 1:
        raise ValueError(f"{what}: thresh is a 1-d float64 tensor")
    T = int(thresh.shape[0])
    if not isinstance(pr, torch.Tensor) or pr.dtype != torch.int64 or tuple(pr.shape) != (nset, T, 2) or not pr.is_contiguous():
        raise ValueError(f"{what}: pr is a contiguous int64 ({nset}, {T}, 2) tensor")
    require_gpu(scores, what)
    for name, t in (("counted", counted), ("recalled", recalled), ("lo_d", lo_d), ("thresh", thresh), ("pr", pr)):
        if t.device != scores.device:
            raise ValueError(f"{what}: {name} is on {t.device}, scores on {scores.device}")
    scores, counted, recalled = scores.to(torch.float64).contiguous(), counted.contiguous(), recalled.contiguous()
    lo_d, thresh = lo_d.contiguous(), thresh.contiguous()
    S = len(offs) - 1
    with torch.cuda.device(scores.device):
        check(lib().tf_wider_pr_accumulate(ptr(scores), (C.c_int32 * (S + 1))(*offs), S, ptr(counted), ptr(recalled), nset, ptr(lo_d), ptr(thresh), T,
                                           ptr(pr), stream()), "tf_wider_pr_accumulate")
    return pr


# --------------------------------------------------------------------------- decode
def template_masks(templates, scale, width, mask_axis="w"):
    """Validity masks reproducing tinyfaces/models/utils.py:17-44.  mask_axis='w' is the
    reference's behaviour (defect D1: the invalid TEMPLATE ids index the W axis, IndexError
    when W <= max id); 'template' is the evidently intended masking."""
    nt = templates.shape[0]
    all_scale = np.arange(4, 12)
    one_scale = np.arange(18, 25)
    ignored = np.setdiff1d(np.arange(25), np.concatenate((all_scale, one_scale)))
    ts = np.asarray(templates)[:, 4]
    inv = np.where(ts[one_scale] >= 1.0) if scale < 1 else np.where(ts[one_scale] != 1.0)
    invalid = np.concatenate((ignored, one_scale[inv]))
    vx, vt = np.ones(width, np.uint8), np.ones(nt, np.uint8)
    if mask_axis == "w":
        if invalid.max() >= width:
            raise IndexError(f"index {invalid.max()} is out of bounds for axis 2 with size {width}")   # same failure as utils.py:44
        vx[invalid] = 0
    else:
        vt[invalid[invalid < nt]] = 0
    return vx, vt


def decode_compact(score, templates_d, valid_x, valid_t, prob_thresh, scale, dets, count, rf=RF):
    """sigmoid + threshold + ordered compaction + regression refinement of one score map
    (tinyfaces/evaluation.py:61-78, tinyfaces/models/utils.py:46-100).  score (5nt,H,W) f32 device;
    appends rows (x1,y1,x2,y2,score) f64 to dets[count...] and advances the device counter."""
    require_gpu(score, "decode_compact")
    nt = templates_d.shape[0]
    _, H, W = score.shape
    wsb = lib().tf_decode_workspace_bytes(H, W, nt)
    ws = _workspace("decode", wsb, score.device)
    sty, stx = rf["stride"]
    ofy, ofx = rf["offset"]
    with torch.cuda.device(score.device):
        check(lib().tf_decode_compact(ptr(score), nt, H, W, ptr(templates_d), templates_d.shape[1], ptr(valid_x), ptr(valid_t),
                                      float(np.float32(prob_thresh)), float(scale), sty, stx, ofy, ofx, ptr(dets), ptr(count),
                                      dets.shape[0], ptr(ws), wsb, stream()), "tf_decode_compact")


# --------------------------------------------------------------------------- criterion
def _criterion_operands(output, class_map, regression_map, n_templates, grad, loss_len, template_wh=None, npos=True):
    """What the four criterion wrappers do to their operands before they call the library: the dtype / shape / contiguity checks, then
    -> (output and regression_map made contiguous, (B, nt, H, W), device, template_wh as float32 on the device or None, grad -- the caller's,
    checked, or a new one --, loss (loss_len,) f64, npos (B,) int32 or None)."""
    assert output.dtype == torch.float32 and class_map.dtype == torch.float32 and regression_map.dtype == torch.float32
    output, regression_map = output.contiguous(), regression_map.contiguous()
    assert class_map.is_contiguous()
    B, C5, H, W = output.shape
    nt = n_templates
    assert C5 == 5 * nt and class_map.shape == (B, nt, H, W) and regression_map.shape == (B, 4 * nt, H, W)
    dev = output.device
    twh = None if template_wh is None else template_wh.to(device=dev, dtype=torch.float32).contiguous()
    if grad is None:
        grad = torch.empty_like(output)
    assert grad.shape == output.shape and grad.dtype == torch.float32 and grad.is_contiguous() and grad.device == dev
    loss = torch.empty(loss_len, dtype=torch.float64, device=dev)
    return output, regression_map, (B, nt, H, W), dev, twh, grad, loss, torch.empty(B, dtype=torch.int32, device=dev) if npos else None


def criterion_fwd_bwd(output, class_map, regression_map, n_templates=25, reg_weight=1.0, ohem_thresh=0.03, max_pos=128,
                      max_neg=128, pos_keep=None, neg_keep=None, seed=0, want_labels=False, grad=None):
    """DetectionCriterion.forward + backward (tinyfaces/models/loss.py:59-93).  class_map is mined in place.
    Returns (loss[2] f64 device tensor = [sum cls, sum reg], grad wrt output, labels or None).
    grad: write the gradient into this contiguous fp32 tensor of output's shape (every element is written exactly once, no memset needed)."""
    require_gpu(output, "criterion")
    output, regression_map, (B, nt, H, W), dev, _, grad, loss, _ = _criterion_operands(output, class_map, regression_map, n_templates, grad, 2, npos=False)
    labels = torch.empty_like(class_map) if want_labels else None
    wsb = lib().tf_criterion_workspace_bytes(B, nt, H, W)
    ws = _workspace("criterion", wsb, dev)
    pk = None if pos_keep is None else pos_keep.to(device=dev, dtype=torch.uint8).contiguous()
    nk = None if neg_keep is None else neg_keep.to(device=dev, dtype=torch.uint8).contiguous()
    with torch.cuda.device(dev):
        check(lib().tf_criterion_fwd_bwd(ptr(output), ptr(class_map), ptr(regression_map), B, nt, H, W, float(ohem_thresh), int(max_pos),
                                         int(max_neg), float(reg_weight), ptr(pk), ptr(nk), int(seed) & (2**64 - 1), ptr(labels),
                                         ptr(grad), ptr(loss), None, ptr(ws), wsb, stream()), "tf_criterion_fwd_bwd")
    return loss, grad, labels


FOCAL_NORMALIZE = {"none": 0, "pos": 1}                  # TF_FOCAL_NORM_*


def check_focal(gamma, alpha, normalize):
    """ValueError unless gamma is finite and >= 0, alpha finite and <= 1 (negative: no alpha weighting) and normalize one of FOCAL_NORMALIZE."""
    if not (np.isfinite(gamma) and gamma >= 0):
        raise ValueError(f"focal loss: gamma must be a finite number >= 0, got {gamma}")
    if not (np.isfinite(alpha) and alpha <= 1):
        raise ValueError(f"focal loss: alpha must be a finite number <= 1 (negative switches the weighting off), got {alpha}")
    if normalize not in FOCAL_NORMALIZE:
        raise ValueError(f"focal loss: normalize must be one of {sorted(FOCAL_NORMALIZE)}, got {normalize!r}")


def criterion_focal_fwd_bwd(output, class_map, regression_map, n_templates=25, reg_weight=1.0, gamma=2.0, alpha=0.25, normalize="pos",
                            grad=None):
    """Sigmoid focal loss over every labelled element + SmoothL1 over every positive, loss and d(total)/d(output) in one device pass
    (tf_criterion_focal_fwd_bwd): no OHEM, no sampling, class_map is only read.  normalize="pos": image b's sums and gradient times
    1 / max(1, npos_b), images summed; "none": the plain sum.  alpha < 0: no alpha weighting.
    Returns (loss[2] f64 device tensor = [sum cls, sum reg], grad wrt output, npos[B] int32 = the +1 labels of every image).
    grad: write the gradient into this contiguous fp32 tensor of output's shape (every element is written exactly once, no memset needed)."""
    require_gpu(output, "criterion_focal")
    check_focal(gamma, alpha, normalize)
    output, regression_map, (B, nt, H, W), dev, _, grad, loss, npos = _criterion_operands(output, class_map, regression_map, n_templates, grad, 2)
    wsb = lib().tf_criterion_focal_workspace_bytes(B, nt, H, W)
    ws = _workspace("criterion_focal", wsb, dev)
    with torch.cuda.device(dev):
        check(lib().tf_criterion_focal_fwd_bwd(ptr(output), ptr(class_map), ptr(regression_map), B, nt, H, W, float(gamma), float(alpha),
                                               FOCAL_NORMALIZE[normalize], float(reg_weight), ptr(grad), ptr(loss), ptr(npos),
                                               ptr(ws), wsb, stream()), "tf_criterion_focal_fwd_bwd")
    return loss, grad, npos


REG_LOSSES = {"smooth_l1": 0, "iou": 1, "giou": 2, "diou": 3}      # TF_REG_*
BOX_CLIP = float(np.log(1000.0 / 16.0))                           # the clamp of the predicted log sizes (torchvision's bbox_xform_clip)


def template_wh(templates):
    """(nt, 2) float32 (dw, dh) = (x2 - x1 + 1, y2 - y1 + 1) of the (nt, >= 4) template table (tinyfaces/datasets/templates.py): the sizes the
    regression targets are normalised by, of which the DIoU loss needs the aspect ratio."""
    t = torch.as_tensor(np.asarray(templates.detach().cpu() if torch.is_tensor(templates) else templates, dtype=np.float64))
    if t.dim() != 2 or t.shape[1] < 4:
        raise ValueError(f"templates must be an (nt, >= 4) table of (x1, y1, x2, y2[, scale]), got shape {tuple(t.shape)}")
    wh = torch.stack([t[:, 2] - t[:, 0] + 1.0, t[:, 3] - t[:, 1] + 1.0], 1)
    if not (bool(torch.isfinite(wh).all()) and bool((wh > 0).all())):
        raise ValueError("templates: every template needs a finite positive width and height")
    return wh.float().contiguous()


def check_reg_loss(reg_loss, reg_weight=1.0, template_wh=None, n_templates=None):
    """ValueError unless reg_loss is one of REG_LOSSES, reg_weight is finite, and -- for "diou" -- template_wh is an (nt, 2) tensor."""
    if reg_loss not in REG_LOSSES:
        raise ValueError(f"regression loss: reg_loss must be one of {tuple(REG_LOSSES)}, got {reg_loss!r}")
    if not np.isfinite(reg_weight):
        raise ValueError(f"regression loss: reg_weight must be finite, got {reg_weight}")
    if reg_loss == "diou":
        if template_wh is None:
            raise ValueError("regression loss: reg_loss='diou' needs template_wh (the (dw, dh) of every template: ops.template_wh(templates))")
        if not torch.is_tensor(template_wh) or template_wh.dim() != 2 or template_wh.shape[1] != 2 or \
                (n_templates is not None and template_wh.shape[0] != n_templates):
            raise ValueError(f"regression loss: template_wh must be an (n_templates, 2) tensor, got {getattr(template_wh, 'shape', template_wh)!r}")


def criterion_focal_box_fwd_bwd(output, class_map, regression_map, n_templates=25, reg_weight=1.0, gamma=2.0, alpha=0.25, normalize="pos",
                                reg_loss="smooth_l1", template_wh=None, grad=None):
    """criterion_focal_fwd_bwd with the regression loss `reg_loss` (tf_criterion_focal_box_fwd_bwd): "iou", "giou" and "diou" put ONE overlap
    term per positive in place of the four SmoothL1 terms (include/tinyfaces_hip.h has the definition); "smooth_l1" runs the kernels of
    criterion_focal_fwd_bwd through this entry point (the same bits).  template_wh: (nt, 2) (dw, dh) of the templates, needed by "diou" only.
    Same returns as criterion_focal_fwd_bwd; loss[1] is the sum of the overlap terms."""
    require_gpu(output, "criterion_focal_box")
    check_focal(gamma, alpha, normalize)
    check_reg_loss(reg_loss, reg_weight, template_wh, n_templates)
    output, regression_map, (B, nt, H, W), dev, twh, grad, loss, npos = _criterion_operands(output, class_map, regression_map, n_templates, grad, 2,
                                                                                            template_wh if reg_loss == "diou" else None)
    wsb = lib().tf_criterion_focal_workspace_bytes(B, nt, H, W)
    ws = _workspace("criterion_focal", wsb, dev)
    with torch.cuda.device(dev):
        check(lib().tf_criterion_focal_box_fwd_bwd(ptr(output), ptr(class_map), ptr(regression_map), B, nt, H, W, float(gamma), float(alpha),
                                                   FOCAL_NORMALIZE[normalize], float(reg_weight), REG_LOSSES[reg_loss], ptr(twh),
                                                   ptr(grad), ptr(loss), ptr(npos), ptr(ws), wsb, stream()), "tf_criterion_focal_box_fwd_bwd")
    return loss, grad, npos


def check_qfl(beta, normalize):
    """ValueError unless beta is finite and >= 1 and normalize one of FOCAL_NORMALIZE.  (For 1 <= beta < 2 the gradient is ill-conditioned where
    sigmoid(s) is close to the quality target, and for beta = 1 it jumps there: include/tinyfaces_hip.h.)"""
    if not (isinstance(beta, (int, float, np.floating, np.integer)) and np.isfinite(beta) and beta >= 1):
        raise ValueError(f"quality focal loss: beta must be a finite number >= 1, got {beta}")
    if normalize not in FOCAL_NORMALIZE:
        raise ValueError(f"quality focal loss: normalize must be one of {sorted(FOCAL_NORMALIZE)}, got {normalize!r}")


def criterion_quality_fwd_bwd(output, class_map, regression_map, n_templates=25, reg_weight=1.0, beta=2.0, normalize="pos",
                              reg_loss="smooth_l1", template_wh=None, grad=None):
    """Quality focal loss (Li et al. 2020) over every labelled element + the regression loss `reg_loss` over every positive, loss and
    d(total)/d(output) in one device pass (tf_criterion_quality_fwd_bwd): the class logit of a positive is trained towards q = min(1, IoU) of
    its own predicted box with its target, that of a negative towards 0, QFL = |sigmoid(s) - q|^beta (softplus(s) - q s); q is a constant of
    the classification term (include/tinyfaces_hip.h has the definition).  normalize, reg_loss and template_wh as in
    criterion_focal_box_fwd_bwd; class_map is only read.
    Returns (loss[4] f64 device tensor = [sum cls, sum reg, sum of q over the positives (not normalised), number of positives], grad wrt output,
    npos[B] int32): loss[2] / loss[3] is the mean IoU of the predicted boxes of the positives with their targets.
    grad: write the gradient into this contiguous fp32 tensor of output's shape (every element is written exactly once, no memset needed)."""
    require_gpu(output, "criterion_quality")
    check_qfl(beta, normalize)
    check_reg_loss(reg_loss, reg_weight, template_wh, n_templates)
    output, regression_map, (B, nt, H, W), dev, twh, grad, loss, npos = _criterion_operands(output, class_map, regression_map, n_templates, grad, 4,
                                                                                            template_wh if reg_loss == "diou" else None)
    wsb = lib().tf_criterion_quality_workspace_bytes(B, nt, H, W)
    ws = _workspace("criterion_quality", wsb, dev)
    with torch.cuda.device(dev):
        check(lib().tf_criterion_quality_fwd_bwd(ptr(output), ptr(class_map), ptr(regression_map), B, nt, H, W, float(beta),
                                                 FOCAL_NORMALIZE[normalize], float(reg_weight), REG_LOSSES[reg_loss], ptr(twh),
                                                 ptr(grad), ptr(loss), ptr(npos), ptr(ws), wsb, stream()), "tf_criterion_quality_fwd_bwd")
    return loss, grad, npos


ALIGNED_NORMALIZE = {"none": 0, "pos": 1, "align": 2}    # TF_FOCAL_NORM_*: "align" belongs to the task-aligned form alone


def check_aligned(beta, normalize):
    """ValueError unless beta is finite and >= 1 (check_qfl's bound) and normalize one of ALIGNED_NORMALIZE."""
    check_qfl(beta, "pos")
    if normalize not in ALIGNED_NORMALIZE:
        raise ValueError(f"task-aligned loss: normalize must be one of {sorted(ALIGNED_NORMALIZE)}, got {normalize!r}")


def criterion_aligned_fwd_bwd(output, class_map, regression_map, align_map, n_templates=25, reg_weight=1.0, beta=2.0, normalize="align",
                              reg_loss="smooth_l1", template_wh=None, grad=None):
    """TOOD's task-aligned loss (Feng et al. 2021; tf_criterion_aligned_fwd_bwd, the definition is in include/tinyfaces_hip.h): the quality focal
    form with the target of a positive READ from align_map (what tal_assign_device(..., align_out=) wrote: the face's normalised alignment),
    q = min(1, max(0, a)), a NaN giving 0, and the regression term of every positive -- `reg_loss`, as in criterion_quality_fwd_bwd --
    weighted by the same q.  align_map: float32 of class_map's shape, read at the +1 labels only.  normalize: "none", "pos" (per image by
    max(1, its positives)) or "align": per image by max(1, the sum of q over its positives), TOOD's avg_factor taken per image, so that an
    image's loss still does not depend on its batch.  class_map is only read.
    Returns (loss[4] f64 device tensor = [sum cls, sum of q-weighted reg, sum of q over the positives (not normalised), number of positives],
    grad wrt output, npos[B] int32): loss[2] / loss[3] is the mean target of the positives.
    grad: write the gradient into this contiguous fp32 tensor of output's shape (every element is written exactly once, no memset needed)."""
    require_gpu(output, "criterion_aligned")
    check_aligned(beta, normalize)
    check_reg_loss(reg_loss, reg_weight, template_wh, n_templates)
    output, regression_map, (B, nt, H, W), dev, twh, grad, loss, npos = _criterion_operands(output, class_map, regression_map, n_templates, grad, 4,
                                                                                            template_wh if reg_loss == "diou" else None)
    if not torch.is_tensor(align_map) or align_map.dtype != torch.float32 or not align_map.is_contiguous() or align_map.device != dev or \
            align_map.shape != class_map.shape:
        raise ValueError("criterion_aligned_fwd_bwd: align_map is a contiguous float32 tensor of class_map's shape on the output's device")
    wsb = lib().tf_criterion_aligned_workspace_bytes(B, nt, H, W)
    ws = _workspace("criterion_aligned", wsb, dev)
    with torch.cuda.device(dev):
        check(lib().tf_criterion_aligned_fwd_bwd(ptr(output), ptr(class_map), ptr(regression_map), ptr(align_map), B, nt, H, W, float(beta),
                                                 ALIGNED_NORMALIZE[normalize], float(reg_weight), REG_LOSSES[reg_loss], ptr(twh),
                                                 ptr(grad), ptr(loss), ptr(npos), ptr(ws), wsb, stream()), "tf_criterion_aligned_fwd_bwd")
    return loss, grad, npos


# --------------------------------------------------------------------------- SGD
NMS_MAX_BOXES = 524160                                   # csrc/nms.hip: (n/64 + 2) 8-byte words must fit 64 KiB of LDS
IMAGE_MEAN, IMAGE_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)        # main.py:44-46


JITTER_KINDS = {"brightness": 0, "contrast": 1, "saturation": 2, "hue": 3}        # TF_JITTER_* (include/tinyfaces_hip.h)
JITTER_MAX_PIXELS = 1 << 24


def jitter_chain(jitter):
    """[(kind, factor)] -> ([TF_JITTER_* code], [float factor]) as tf_image_prepare_jitter takes them: every kind at most once, factors finite and
    >= 0; for "hue" the factor is torchvision's hue_factor in [-0.5, 0.5] and becomes the shift int(hue_factor * 255) mod 256 of the uint8 hue
    (truncated toward zero, wrapped like its np.uint8)."""
    codes, factors = [], []
    for item in jitter:
        kind, f = item
        if kind not in JITTER_KINDS:
            raise ValueError(f"image_prepare: unknown jitter op {kind!r} (one of {sorted(JITTER_KINDS)})")
        if JITTER_KINDS[kind] in codes:
            raise ValueError(f"image_prepare: jitter op {kind!r} appears twice")
        f = float(f)
        if kind == "hue":
            if not (math.isfinite(f) and -0.5 <= f <= 0.5):
                raise ValueError(f"image_prepare: hue factor must be in [-0.5, 0.5], got {f}")
            f = float(int(f * 255) % 256)
        elif not (math.isfinite(f) and f >= 0.0):
            raise ValueError(f"image_prepare: {kind} factor must be finite and >= 0, got {f}")
        codes.append(JITTER_KINDS[kind])
        factors.append(f)
    return codes, factors


def image_prepare(img_u8, resized_hw=None, crop=None, paste=(0, 0), flip=False, out_hw=None, mean=IMAGE_MEAN, std=IMAGE_STD,
                  out=None, jitter=None):
    """uint8 (H, W, 3) device image -> normalised float32 (3, OH, OW) device tensor in one HIP pass (tf_image_prepare):
    PIL-exact BILINEAR resize to `resized_hw`, window `crop` = (y, x, h, w) of the resized image pasted at `paste` = (y, x)
    on the mean colour, optional mirror, ToTensor + Normalize.  Defaults: no resize, whole image, out_hw = window size
    (the evaluation pyramid level of tinyfaces/evaluation.py:46-53); training passes the 500x500 crop parameters of
    tinyfaces/datasets/processor.py:41-76.
    jitter: a sequence of (kind, factor), kind in "brightness" | "contrast" | "saturation" | "hue", applied in this order to the uint8 OH x OW
    image (padding included) before ToTensor -- torchvision's ColorJitter on the PIL image, bit for bit (tf_image_prepare_jitter: one launch,
    two when contrast is in the chain).  None or empty: tf_image_prepare, exactly as without the argument."""
    require_gpu(img_u8, "image_prepare")
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 3 or img_u8.shape[2] != 3:
        raise ValueError("image_prepare: expected a uint8 (H, W, 3) tensor")
    img_u8 = img_u8.contiguous()
    H, W = int(img_u8.shape[0]), int(img_u8.shape[1])
    RH, RW = (H, W) if resized_hw is None else (int(resized_hw[0]), int(resized_hw[1]))
    cy, cx, ch, cw = (0, 0, RH, RW) if crop is None else [int(v) for v in crop]
    OH, OW = (ch, cw) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    if out is None:
        out = torch.empty(3, OH, OW, dtype=torch.float32, device=img_u8.device)
    a = _hip.ImagePrepareArgs()
    a.img, a.H, a.W, a.RH, a.RW = ptr(img_u8), H, W, RH, RW
    a.crop_y, a.crop_x, a.crop_h, a.crop_w = cy, cx, ch, cw
    a.paste_y, a.paste_x, a.flip, a.OH, a.OW = int(paste[0]), int(paste[1]), int(bool(flip)), OH, OW
    for c in range(3):
        a.mean[c], a.std[c] = float(mean[c]), float(std[c])
        a.bg[c] = int(np.int8(np.float64(mean[c]) * 255)) & 0xFF          # processor.py:66-71: (mean * 255).astype(int8)
    a.out = ptr(out)
    if not jitter:
        with torch.cuda.device(img_u8.device):
            check(lib().tf_image_prepare(C.byref(a), stream()), "tf_image_prepare")
        return out
    codes, factors = jitter_chain(jitter)
    if OH * OW > JITTER_MAX_PIXELS:
        raise ValueError(f"image_prepare: jitter is defined for at most 2^24 output pixels, got {OH} x {OW}")
    n = len(codes)
    op, fac = (C.c_int * 4)(*codes), (C.c_float * 4)(*factors)
    with torch.cuda.device(img_u8.device):
        st = stream()
        wsb = lib().tf_image_prepare_jitter_workspace_bytes(OH, OW, n, op)
        ws = None
        if wsb:
            # one buffer per device AND stream: WIDERFace.collate builds its batch on an input stream of its own while another stream may prepare images too
            ws = _workspace(f"image_jitter@{st}", wsb, img_u8.device)
            ws.record_stream(torch.cuda.current_stream())
        check(lib().tf_image_prepare_jitter(C.byref(a), n, op, fac, ptr(ws), wsb, st), "tf_image_prepare_jitter")
    return out


class ClipState:
    """The 32 bytes of device memory a clipped step keeps its verdict in (tf_clip_state, include/tinyfaces_hip.h): written by
    `grad_clip_coef`, read by `sgd_step(..., clip_state=)`, `sgd_step_segments(..., clip_state=)` and `scale_segments` on the device.  The
    readers below copy it to the host, i.e. they synchronise; `norm_tensor()` is a 0-d device view and does not."""

    def __init__(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"ClipState: device {device}; the tiny-faces hot path only exists as HIP kernels for MI355X (gfx950) -- "
                               "there is no CPU fallback.")
        self.buf = torch.zeros(C.sizeof(_hip.ClipState), dtype=torch.uint8, device=device)

    def read(self):
        """The whole state as a host-side _hip.ClipState (synchronises)."""
        return _hip.ClipState.from_buffer_copy(self.buf.cpu().numpy().tobytes())

    def norm_tensor(self):
        """The norm as a 0-d float64 device tensor sharing the state's memory (no sync): it shows the latest grad_clip_coef."""
        return self.buf[8:16].view(torch.float64).view(())

    def sumsq(self):
        return float(self.read().sumsq)

    def norm(self):
        return float(self.read().norm)

    def coef(self):
        return float(self.read().coef)

    def skip(self):
        return int(self.read().skip)

    def skipped(self):
        return int(self.read().skipped)


def _segment_table(what, segments, n):
    """[(start, end)] -> the ctypes table of the *_segments entry points (empty ranges dropped); ValueError when out of order or outside n."""
    segments = [(int(s), int(e)) for s, e in segments if e > s]
    prev = 0
    for s, e in segments:
        if s < prev or e > n:
            raise ValueError(f"{what}: range ({s}, {e}) is out of order or outside the {n} elements of the buffers")
        prev = e
    return (C.c_int64 * (2 * len(segments)))(*[v for se in segments for v in se]), len(segments)


def grad_clip_coef(grad_flat, segments, state, grad_scale=1.0, max_norm=None, skip_nonfinite=False):
    """The first half of torch.nn.utils.clip_grad_norm_ (the spot between loss.backward() and optimizer.step(), tinyfaces/trainer.py:86-87):
    the global L2 norm of `grad_scale * grad_flat` over the element ranges `segments` ([(start, end)], ascending, disjoint), the clip
    coefficient min(1, max_norm / (norm + 1e-6)) (max_norm None: 1) and, with skip_nonfinite, the verdict "skip this step" for a norm that
    is not finite -- all left in `state` (ClipState) on the device, no host sync.  Deterministic: fp64 sums in a fixed order, no atomics."""
    require_gpu(grad_flat, "grad_clip_coef")
    assert grad_flat.dtype == torch.float32 and grad_flat.is_contiguous() and state.buf.device == grad_flat.device
    table, nseg = _segment_table("grad_clip_coef", segments, grad_flat.numel())
    need = int(lib().tf_grad_norm_workspace_bytes(nseg))
    ws = _workspace("grad_norm", need, grad_flat.device)
    flags = _hip.TF_CLIP_SKIP_NONFINITE if skip_nonfinite else 0
    with torch.cuda.device(grad_flat.device):
        check(lib().tf_grad_clip_coef(ptr(grad_flat), table, nseg, float(grad_scale), 0.0 if max_norm is None else float(max_norm), flags,
                                      ptr(ws), ws.numel(), ptr(state.buf), stream()), "tf_grad_clip_coef")
    return state


def scale_segments(grad_flat, segments, state):
    """grad_flat[ranges] *= state.coef on the device (zeros behind a skipped step), everything else untouched: the second half of
    clip_grad_norm_ for the autograd path, where torch.optim.SGD applies the update (tinyfaces/trainer.py:86-87)."""
    require_gpu(grad_flat, "scale_segments")
    assert grad_flat.dtype == torch.float32 and grad_flat.is_contiguous() and state.buf.device == grad_flat.device
    table, nseg = _segment_table("scale_segments", segments, grad_flat.numel())
    if nseg == 0:
        return
    with torch.cuda.device(grad_flat.device):
        check(lib().tf_scale_segments(ptr(grad_flat), table, nseg, ptr(state.buf), stream()), "tf_scale_segments")


_clip_states = {}


def clip_grad_norm_(parameters, max_norm, skip_nonfinite=False):
    """Drop-in for torch.nn.utils.clip_grad_norm_(parameters, max_norm) (L2, error_if_nonfinite=False) on this model's gradients, between
    loss.backward() and optimizer.step() (tinyfaces/trainer.py:86-87): two launches of the norm pass and one scaling pass instead of a few
    hundred small kernels, and no host round trip.  The fp32 CUDA `.grad`s are addressed as element ranges from the lowest data_ptr()
    (views of one flat buffer and separately allocated tensors alike; nothing between the tensors is read or written).  Returns the norm
    as a 0-d float64 device tensor without synchronising; it is overwritten by the next call on the same device.  With skip_nonfinite a
    norm that is not finite ZEROES the gradients instead of scaling them: the optimizer then still applies weight decay and momentum."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    if not grads:
        raise ValueError("clip_grad_norm_: no parameter has a gradient")
    for g in grads:
        require_gpu(g, "clip_grad_norm_")
        if g.dtype != torch.float32 or not g.is_contiguous():
            raise ValueError("clip_grad_norm_: gradients must be contiguous fp32 tensors")
        if g.device != grads[0].device:
            raise ValueError("clip_grad_norm_: gradients live on more than one device")
    dev = grads[0].device
    spans = sorted({(g.data_ptr(), g.numel()) for g in grads if g.numel()})
    base = spans[0][0] if spans else 0
    segs = [((a - base) // 4, (a - base) // 4 + n) for a, n in spans]
    for (_, e0), (s1, _) in zip(segs, segs[1:]):
        if s1 < e0:
            raise ValueError("clip_grad_norm_: gradients overlap in memory")
    state = _clip_states.get(dev)
    if state is None:
        state = _clip_states[dev] = ClipState(dev)
    table = (C.c_int64 * (2 * len(segs)))(*[v for se in segs for v in se])
    need = int(lib().tf_grad_norm_workspace_bytes(len(segs)))
    ws = _workspace("grad_norm", need, dev)
    with torch.cuda.device(dev):
        check(lib().tf_grad_clip_coef(base, table, len(segs), 1.0, float(max_norm), _hip.TF_CLIP_SKIP_NONFINITE if skip_nonfinite else 0,
                                      ptr(ws), ws.numel(), ptr(state.buf), stream()), "tf_grad_clip_coef")
        if segs:
            check(lib().tf_scale_segments(base, table, len(segs), ptr(state.buf), stream()), "tf_scale_segments")
    return state.norm_tensor()


def clip_skipped_steps(device):
    """How many calls of clip_grad_norm_(..., skip_nonfinite=True) on `device` met a gradient norm that was not finite (synchronises)."""
    state = _clip_states.get(torch.device(device))
    return 0 if state is None else state.skipped()


def _ema_pair(what, param, ema, ema_weight):
    """(ema, weight) checked, or None when neither was given: the fused model EMA of sgd_step / sgd_step_segments."""
    if ema is None and ema_weight is None:
        return None
    if ema is None or ema_weight is None:
        raise ValueError(f"{what}: ema and ema_weight go together")
    assert ema.dtype == torch.float32 and ema.is_contiguous() and ema.device == param.device and ema.numel() == param.numel()
    return ema, float(ema_weight)


def sgd_step(param, grad, momentum_buf, lr, momentum, weight_decay, grad_scale=1.0, *, ema=None, ema_weight=None, clip_state=None):
    """torch.optim.SGD.step for one flat fp32 segment (main.py:67-70).  clip_state (ClipState, filled by grad_clip_coef on this stream): the
    step behind clip_grad_norm_ -- grad_scale * coef, nothing at all when the state says skip.
    ema, ema_weight (together): the model EMA in the same launch, ema = fmaf(ema_weight, param_after - ema, ema) (tf_sgd_step_ema; a skipped
    step leaves ema alone too).  Without them the calls are the ones above, unchanged."""
    require_gpu(param, "sgd_step")
    assert param.dtype == grad.dtype == momentum_buf.dtype == torch.float32
    assert param.is_contiguous() and grad.is_contiguous() and momentum_buf.is_contiguous()
    avg = _ema_pair("sgd_step", param, ema, ema_weight)
    with torch.cuda.device(param.device):
        if avg is not None:
            check(lib().tf_sgd_step_ema(ptr(param), ptr(grad), ptr(momentum_buf), ptr(avg[0]), param.numel(), float(lr), float(momentum),
                                        float(weight_decay), float(grad_scale), avg[1], None if clip_state is None else ptr(clip_state.buf),
                                        stream()), "tf_sgd_step_ema")
            return
        if clip_state is not None:
            check(lib().tf_sgd_step_clipped(ptr(param), ptr(grad), ptr(momentum_buf), param.numel(), float(lr), float(momentum),
                                            float(weight_decay), float(grad_scale), ptr(clip_state.buf), stream()), "tf_sgd_step_clipped")
            return
        check(lib().tf_sgd_step(ptr(param), ptr(grad), ptr(momentum_buf), param.numel(), float(lr), float(momentum),
                                float(weight_decay), float(grad_scale), stream()), "tf_sgd_step")


def sgd_step_segments(param, grad, momentum_buf, segments, lr, momentum, weight_decay, grad_scale=1.0, *, ema=None, ema_weight=None,
                      clip_state=None):
    """torch.optim.SGD.step over the element ranges `segments` ([(start, end)], ascending, disjoint) of three flat fp32 buffers;
    everything outside the ranges is left untouched (tf_sgd_step_segments: parameters without a gradient, e.g. frozen BatchNorm vectors).
    clip_state: as in sgd_step (tf_sgd_step_segments_clipped).  ema, ema_weight: as in sgd_step (tf_sgd_step_segments_ema), a fourth flat
    buffer of the same length whose elements outside the ranges stay untouched as well."""
    require_gpu(param, "sgd_step_segments")
    assert param.dtype == grad.dtype == momentum_buf.dtype == torch.float32
    assert param.is_contiguous() and grad.is_contiguous() and momentum_buf.is_contiguous()
    n = param.numel()
    assert grad.numel() == n and momentum_buf.numel() == n
    avg = _ema_pair("sgd_step_segments", param, ema, ema_weight)
    segments = [(int(s), int(e)) for s, e in segments if e > s]
    prev = 0
    for s, e in segments:
        if s < prev or e > n:
            raise ValueError(f"sgd_step_segments: range ({s}, {e}) is out of order or outside the {n} elements of the buffers")
        prev = e
    if not segments:
        return
    table = (C.c_int64 * (2 * len(segments)))(*[v for se in segments for v in se])
    with torch.cuda.device(param.device):
        if avg is not None:
            check(lib().tf_sgd_step_segments_ema(ptr(param), ptr(grad), ptr(momentum_buf), ptr(avg[0]), table, len(segments), float(lr),
                                                 float(momentum), float(weight_decay), float(grad_scale), avg[1],
                                                 None if clip_state is None else ptr(clip_state.buf), stream()), "tf_sgd_step_segments_ema")
            return
        if clip_state is not None:
            check(lib().tf_sgd_step_segments_clipped(ptr(param), ptr(grad), ptr(momentum_buf), table, len(segments), float(lr),
                                                     float(momentum), float(weight_decay), float(grad_scale), ptr(clip_state.buf), stream()),
                  "tf_sgd_step_segments_clipped")
            return
        check(lib().tf_sgd_step_segments(ptr(param), ptr(grad), ptr(momentum_buf), table, len(segments), float(lr), float(momentum),
                                         float(weight_decay), float(grad_scale), stream()), "tf_sgd_step_segments")


def ema_update_segments(ema, param, segments, weight, clip_state=None):
    """ema[ranges] = fmaf(weight, param - ema, ema) on the device, everything else untouched (tf_ema_update_segments): what
    torch.optim.swa_utils.AveragedModel.update_parameters does behind optimizer.step() (tinyfaces/trainer.py:87), in one launch per
    TF_SGD_MAX_SEGMENTS ranges and without a per-parameter loop.  `ema` and `param` are flat fp32 buffers of one length (or views at the
    same offset of two such buffers).  clip_state: a state that says skip makes the call a no-op on the device."""
    require_gpu(ema, "ema_update_segments")
    assert ema.dtype == param.dtype == torch.float32 and ema.is_contiguous() and param.is_contiguous()
    assert ema.device == param.device and ema.numel() == param.numel()
    table, nseg = _segment_table("ema_update_segments", segments, ema.numel())
    if nseg == 0:
        return
    with torch.cuda.device(ema.device):
        check(lib().tf_ema_update_segments(ptr(ema), ptr(param), table, nseg, float(weight), None if clip_state is None else ptr(clip_state.buf),
                                           stream()), "tf_ema_update_segments")


class AdamState:
    """The 24 bytes of device memory AdamW keeps its step counter and bias corrections in (tf_adam_state, include/tinyfaces_hip.h): advanced
    by `adamw_advance` once per optimizer step (not at all on a step the non-finite guard drops), read by `adamw_step` /
    `adamw_step_segments` on the device.  The readers below copy it to the host, i.e. they synchronise."""

    def __init__(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"AdamState: device {device}; the tiny-faces hot path only exists as HIP kernels for MI355X (gfx950) -- "
                               "there is no CPU fallback.")
        self.buf = torch.zeros(C.sizeof(_hip.AdamState), dtype=torch.uint8, device=device)

    def read(self):
        """The whole state as a host-side _hip.AdamState (synchronises)."""
        return _hip.AdamState.from_buffer_copy(self.buf.cpu().numpy().tobytes())

    def step(self):
        return int(self.read().step)

    def bias1(self):
        return float(self.read().bias1)

    def bias2(self):
        return float(self.read().bias2)

    def set_step(self, t):
        """Resume: the counter becomes t (>= 0); bias1 and bias2 are zeroed, the next adamw_advance recomputes them for t + 1."""
        t = int(t)
        if t < 0:
            raise ValueError(f"AdamState.set_step: step must be >= 0, got {t}")
        host = torch.zeros(3, dtype=torch.int64)
        host[0] = t
        self.buf.copy_(host.view(torch.uint8))
        return self


def _adam_hyper(what, lr, betas, eps, weight_decay):
    b1, b2 = (float(b) for b in betas)
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"{what}: betas must lie in [0, 1), got {betas!r}")
    if not float(eps) > 0.0:
        raise ValueError(f"{what}: eps must be positive, got {eps!r}")
    return float(lr), b1, b2, float(eps), float(weight_decay)


def adamw_advance(state, betas=(0.9, 0.999), clip_state=None):
    """One optimizer step of the AdamW bookkeeping on the device (tf_adamw_advance): step += 1 and the two bias corrections, unless
    clip_state (filled by grad_clip_coef earlier on this stream) says skip.  Call it once per optimizer step, in front of the step's
    adamw_step / adamw_step_segments launches."""
    _, b1, b2, _, _ = _adam_hyper("adamw_advance", 0.0, betas, 1.0, 0.0)
    with torch.cuda.device(state.buf.device):
        check(lib().tf_adamw_advance(ptr(state.buf), b1, b2, None if clip_state is None else ptr(clip_state.buf), stream()),
              "tf_adamw_advance")
    return state


def adamw_step(param, grad, exp_avg, exp_avg_sq, state, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0, *, ema=None,
               ema_weight=None, clip_state=None):
    """torch.optim.AdamW.step for one flat fp32 segment (tf_adamw_step), with the bias corrections `state` (AdamState) holds on the device:
    adamw_advance comes first.  ema, ema_weight, clip_state: as in sgd_step -- the model EMA in the same launch, grad_scale * coef, and
    nothing at all (param, both moments and ema keep their bits) when the state says skip."""
    require_gpu(param, "adamw_step")
    assert param.dtype == grad.dtype == exp_avg.dtype == exp_avg_sq.dtype == torch.float32
    assert param.is_contiguous() and grad.is_contiguous() and exp_avg.is_contiguous() and exp_avg_sq.is_contiguous()
    n = param.numel()
    assert grad.numel() == n and exp_avg.numel() == n and exp_avg_sq.numel() == n and state.buf.device == param.device
    lr, b1, b2, eps, wd = _adam_hyper("adamw_step", lr, betas, eps, weight_decay)
    avg = _ema_pair("adamw_step", param, ema, ema_weight)
    with torch.cuda.device(param.device):
        check(lib().tf_adamw_step(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), None if avg is None else ptr(avg[0]), n, lr, b1, b2,
                                  eps, wd, float(grad_scale), 0.0 if avg is None else avg[1], ptr(state.buf),
                                  None if clip_state is None else ptr(clip_state.buf), stream()), "tf_adamw_step")


def adamw_step_segments(param, grad, exp_avg, exp_avg_sq, state, segments, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                        grad_scale=1.0, *, ema=None, ema_weight=None, clip_state=None):
    """adamw_step over the element ranges `segments` ([(start, end)], ascending, disjoint) of four (with ema: five) flat fp32 buffers of one
    length; everything outside the ranges is left untouched (tf_adamw_step_segments)."""
    require_gpu(param, "adamw_step_segments")
    assert param.dtype == grad.dtype == exp_avg.dtype == exp_avg_sq.dtype == torch.float32
    assert param.is_contiguous() and grad.is_contiguous() and exp_avg.is_contiguous() and exp_avg_sq.is_contiguous()
    n = param.numel()
    assert grad.numel() == n and exp_avg.numel() == n and exp_avg_sq.numel() == n and state.buf.device == param.device
    lr, b1, b2, eps, wd = _adam_hyper("adamw_step_segments", lr, betas, eps, weight_decay)
    avg = _ema_pair("adamw_step_segments", param, ema, ema_weight)
    table, nseg = _segment_table("adamw_step_segments", segments, n)
    if nseg == 0:
        return
    with torch.cuda.device(param.device):
        check(lib().tf_adamw_step_segments(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), None if avg is None else ptr(avg[0]), table,
                                           nseg, lr, b1, b2, eps, wd, float(grad_scale), 0.0 if avg is None else avg[1], ptr(state.buf),
                                           None if clip_state is None else ptr(clip_state.buf), stream()), "tf_adamw_step_segments")


ACCUM_STORE, ACCUM_ADD, ACCUM_FINISH = _hip.TF_ACCUM_STORE, _hip.TF_ACCUM_ADD, _hip.TF_ACCUM_FINISH


def grad_accumulate(acc, grad, segments, mode):
    """One micro-batch of a gradient-accumulation window over the element ranges `segments` ([(start, end)], ascending, disjoint) of two flat
    fp32 buffers of one length (tf_grad_accumulate_segments), what autograd does when loss.backward() runs again before optimizer.step()
    (tinyfaces/trainer.py:85-87): ACCUM_STORE acc = grad (the first one: acc is not read), ACCUM_ADD acc = acc + grad, ACCUM_FINISH
    grad = acc + grad (the last one: the sum lands in `grad`, acc keeps its bits).  Plain fp32 adds, left to right; everything outside the
    ranges is untouched."""
    require_gpu(acc, "grad_accumulate")
    if mode not in (ACCUM_STORE, ACCUM_ADD, ACCUM_FINISH):
        raise ValueError(f"grad_accumulate: mode must be ACCUM_STORE, ACCUM_ADD or ACCUM_FINISH, got {mode!r}")
    assert acc.dtype == grad.dtype == torch.float32 and acc.is_contiguous() and grad.is_contiguous()
    assert acc.device == grad.device and acc.numel() == grad.numel()
    table, nseg = _segment_table("grad_accumulate", segments, acc.numel())
    if nseg == 0:
        return
    with torch.cuda.device(acc.device):
        check(lib().tf_grad_accumulate_segments(ptr(acc), ptr(grad), table, nseg, int(mode), stream()), "tf_grad_accumulate_segments")


# --------------------------------------------------------------------------- conv engine (used directly by the parity tests)
def pack_weight(w_oihw, dtype, transpose=False, cols_pad=None):
    require_gpu(w_oihw, "pack_weight")
    w = w_oihw.float().contiguous()
    cout, cin, kh, kw = w.shape
    rows = cin if transpose else cout
    cols = cout if transpose else cin
    rows_pad = (rows + 127) // 128 * 128
    cols_pad = cols_pad or cols
    tfd = _hip.tf_dtype(dtype)
    out = torch.empty(rows_pad, kh * kw, cols_pad, dtype=_hip.torch_dtype(tfd), device=w.device)
    check(lib().tf_pack_weight(ptr(w), cout, cin, kh, kw, int(transpose), tfd, ptr(out), rows_pad, cols_pad, stream()), "tf_pack_weight")
    return out


def stem_conv(x_nchw, w_oihw, dtype, epi=0, scale=None, shift=None):
    """conv1 of the trunk (7x7 / stride 2 / pad 3, 3 -> 64; model.py:90) straight from the NCHW fp32 image (tf_stem_conv, r4): returns
    y (N, OH, OW, 64) of `dtype` (bf16 | fp16) [, statistic rows (rows, 2, 64) with epi = EPI_STATS].  `w_oihw` (64, 3, 7, 7) fp32."""
    require_gpu(x_nchw, "stem_conv")
    x = x_nchw.float().contiguous()
    N, _, H, W = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    wp = pack_weight(w_oihw.reshape(64, 147, 1, 1), dtype, cols_pad=192)
    tfd = _hip.tf_dtype(dtype)
    y = torch.empty(N, OH, OW, 64, dtype=dtype, device=x.device)
    st = torch.zeros(lib().tf_get_stat_rows(), 2, 64, device=x.device) if epi == _hip.EPI_STATS else None
    rows = C.c_int(0)
    check(lib().tf_stem_conv(tfd, ptr(x), N, H, W, ptr(wp), 192, ptr(y), int(epi), ptr(scale) if scale is not None else None,
                             ptr(shift) if shift is not None else None, ptr(st) if st is not None else None, C.byref(rows), stream()), "tf_stem_conv")
    return (y, st[:rows.value]) if st is not None else y


def set_deterministic(on):
    """Process-wide deterministic switch of the library (tf_set_deterministic): while on, the BatchNorm statistic rows are unfolded and the
    training step takes the slab forms of its weight gradients -- no floating-point atomics, the same bits on every run.  Returns the
    previous state."""
    prev = bool(lib().tf_get_deterministic())
    check(lib().tf_set_deterministic(int(bool(on))), "tf_set_deterministic")
    return prev


def is_deterministic():
    """Whether the library's deterministic switch is on (tf_get_deterministic)."""
    return bool(lib().tf_get_deterministic())


def _det_slab(key, want, ws_bytes, slab, device):
    """(pointer, bytes, keep-alive) of the slab a deterministic weight gradient gets: `slab` (a uint8 tensor, used whole) | ws_bytes bytes of the
    cached workspace (less than the query: the capped plan; 0: none, the call is refused) | the query's preferred size."""
    if slab is not None:
        return ptr(slab), slab.numel() * slab.element_size(), slab
    nbytes = want if ws_bytes is None else int(ws_bytes)
    if nbytes <= 0:
        return None, 0, None
    ws = _workspace(key, nbytes, device)
    return ptr(ws), nbytes, ws


def stem_wgrad(x_nchw, g_nhwc, x_conv=None, cA=None, cB=None, cD=None, deterministic=False, ws_bytes=None, slab=None, out=None):
    """Weight gradient of conv1 straight from the image (tf_stem_wgrad, r4): x (N,3,H,W) fp32, g (N,OH,OW,64) bf16 | fp16 -> (64,3,7,7) fp32.
    With x_conv (N,OH,OW,64) and cA / cB / cD (64,) fp32 the gradient operand is cA * g + cB * x_conv + cD (the stem's BN-backward apply).
    deterministic: tf_stem_wgrad_det -- one tile per block in a slab of tf_stem_wgrad_det_workspace_bytes (ws_bytes: a smaller one; slab: the
    caller's own uint8 tensor), summed in a fixed order.  out: accumulate into this (64,3,7,7) fp32 tensor."""
    require_gpu(x_nchw, "stem_wgrad")
    x = x_nchw.float().contiguous()
    N, _, H, W = x.shape
    g = g_nhwc.contiguous()
    dw = torch.zeros(64, 3, 7, 7, dtype=torch.float32, device=x.device) if out is None else out
    opt = [ptr(t.contiguous()) if t is not None else None for t in (x_conv, cA, cB, cD)]
    if deterministic:
        want = lib().tf_stem_wgrad_det_workspace_bytes(N, H, W)
        sp, sb, keep = _det_slab("stem_wgrad_det", want, ws_bytes, slab, x.device)
        with torch.cuda.device(x.device):
            check(lib().tf_stem_wgrad_det(_hip.tf_dtype(g.dtype), ptr(x), N, H, W, ptr(g), *opt, ptr(dw), sp, sb, stream()), "tf_stem_wgrad_det")
        return dw
    check(lib().tf_stem_wgrad(_hip.tf_dtype(g.dtype), ptr(x), N, H, W, ptr(g), *opt, ptr(dw), stream()), "tf_stem_wgrad")
    return dw


def conv2d_nhwc(x, w_packed, Cout, KH, KW, stride, pad, mode=0, out_hw=None, ldy=None, pro=None, epi=0, epi_scale=None,
                epi_shift=None, aux=None, aux2=None, aux3=None, mask=None, want_stats=False, tile=0, out=None, stats_into=None):
    """x (N,H,W,Cin) dtype bf16|f32 contiguous; returns y (N,OH,OW,ldy) [, stat partials (mtiles,2,ldy)].
    ldy: row stride of y / aux / aux2 / aux3 and length of the per-channel vectors, >= Cout and a multiple of 4 (fp32) / 8 (bf16, fp16) -- the
    rule of include/tinyfaces_hip.h (tf_conv2d returns TF_ERR_ARG otherwise); default: Cout rounded up to it.
    out: write into this (N,OH,OW,ldy) tensor (with aux=out and TF_EPI_RES the scattered stride-2 data gradient accumulates in place);
    stats_into: add the statistic sums into these existing rows instead of fresh zeros."""
    require_gpu(x, "conv2d_nhwc")
    N, H, W, Cin = x.shape
    if out_hw is None:
        assert mode == 0
        out_hw = ((H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1)
    OH, OW = out_hw
    eps = 16 // x.element_size()                             # elements per 16-byte chunk of a row
    ldy = ldy or (Cout + eps - 1) // eps * eps
    a = _hip.ConvArgs()
    a.dtype, a.mode = _hip.tf_dtype(x.dtype), mode
    a.N, a.H, a.W, a.Cin, a.OH, a.OW, a.Cout, a.KH, a.KW, a.stride, a.pad = N, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad
    a.ldy, a.epi, a.tile = ldy, epi, tile
    y = torch.empty(N, OH, OW, ldy, dtype=x.dtype, device=x.device) if out is None else out
    a.x, a.w, a.y = ptr(x), ptr(w_packed), ptr(y)
    keep = [x, w_packed, y]
    if pro is not None:
        ps, ph, relu = pro
        a.pro_scale, a.pro_shift, a.pro_relu = ptr(ps), ptr(ph), int(relu)
        keep += [ps, ph]
    if epi_scale is not None:
        a.epi_scale, a.epi_shift = ptr(epi_scale), ptr(epi_shift)
    for name, t in (("aux", aux), ("aux2", aux2), ("aux3", aux3)):
        if t is not None:
            setattr(a, name, ptr(t))
    if mask is not None:
        a.mask_scale, a.mask_shift = ptr(mask[0]), ptr(mask[1])
    stats = None
    if want_stats:
        mt = lib().tf_conv_mtiles(C.byref(a))
        check(min(mt, 0), "tf_conv_mtiles")              # negative: the requested tile code does not take this launch
        stats = torch.zeros(mt, 2, ldy, dtype=torch.float32, device=x.device) if stats_into is None else stats_into
        a.stat_out = ptr(stats)
    with torch.cuda.device(x.device):
        check(lib().tf_conv2d(C.byref(a), stream()), "tf_conv2d")
    return (y, stats) if want_stats else y


def _wgrad_args(x, dy, dw, Cin, Cout, KH, KW, stride, pad, pro=None, splitk=0, tile=0, packed=False, row_scale=None):
    """tf_wgrad_args of one weight-gradient call (x (N,H,W,ldx), dy (N,OH,OW,lddy), dw or any device tensor standing in for it)."""
    N, H, W, ldx = x.shape
    _, OH, OW, lddy = dy.shape
    a = _hip.WgradArgs()
    a.tile = tile
    a.packed = int(packed)
    a.dtype = _hip.tf_dtype(x.dtype)
    a.N, a.H, a.W, a.Cin, a.OH, a.OW, a.Cout, a.KH, a.KW, a.stride, a.pad = N, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad
    a.ldx, a.lddy, a.x, a.dy, a.dw_oihw, a.dw_ld, a.splitk = ldx, lddy, ptr(x), ptr(dy), ptr(dw), Cin * KH * KW, splitk
    if pro is not None:
        a.pro_scale, a.pro_shift, a.pro_relu = ptr(pro[0]), ptr(pro[1]), int(pro[2])
    if row_scale is not None:
        a.row_scale = ptr(row_scale)
    return a


def conv2d_wgrad(x, dy, Cin, Cout, KH, KW, stride, pad, pro=None, splitk=0, tile=0, out=None, packed=False, two_phase=False, row_scale=None,
                 deterministic=False, ws_bytes=None, slab=None):
    """x (N,H,W,ldx), dy (N,OH,OW,lddy) -> dW (Cout,Cin,KH,KW) fp32.  two_phase: hand the all-taps 3x3 kernel a partial-tile
    workspace so that its split-K slices are summed by a second kernel instead of fp32 atomics.  row_scale (Cout,) fp32: dW[co] *= it.
    deterministic: tf_conv2d_wgrad_det -- every kernel's slices through a slab of tf_wgrad_det_workspace_bytes (ws_bytes: a smaller one, the
    plan is capped to it; slab: the caller's own uint8 tensor), summed in a fixed order and added once into dW: no atomics."""
    require_gpu(x, "conv2d_wgrad")
    dw = torch.zeros(Cout, Cin, KH, KW, dtype=torch.float32, device=x.device) if out is None else out
    a = _wgrad_args(x, dy, dw, Cin, Cout, KH, KW, stride, pad, pro, splitk, tile, packed, row_scale)
    ws = None
    if deterministic:
        want = lib().tf_wgrad_det_workspace_bytes(C.byref(a))
        sp, sb, ws = _det_slab("wgrad_det", want, ws_bytes, slab, x.device)
        a.partial_ws, a.partial_ws_bytes = sp, sb
        with torch.cuda.device(x.device):
            check(lib().tf_conv2d_wgrad_det(C.byref(a), stream()), "tf_conv2d_wgrad_det")
        return dw
    if two_phase:
        nbytes = lib().tf_wgrad_workspace_bytes(C.byref(a))
        if nbytes:
            ws = _workspace("wgrad3", nbytes, x.device)
            a.partial_ws, a.partial_ws_bytes = ptr(ws), nbytes
    with torch.cuda.device(x.device):
        check(lib().tf_conv2d_wgrad(C.byref(a), stream()), "tf_conv2d_wgrad")
    return dw


def wgrad_det_workspace_bytes(x, dy, Cin, Cout, KH, KW, stride, pad, pro=None, splitk=0, tile=0):
    """tf_wgrad_det_workspace_bytes of the call conv2d_wgrad(..., deterministic=True) would make: the preferred slab, in bytes."""
    return int(lib().tf_wgrad_det_workspace_bytes(C.byref(_wgrad_args(x, dy, x, Cin, Cout, KH, KW, stride, pad, pro, splitk, tile))))


def conv2d_wgrad_group(problems, K, pad, out=None):
    """The weight gradients of a GROUP of convolutions in one launch (tf_conv2d_wgrad_group: every output tile reduced over all pixels
    in-block, dW overwritten).  problems: [(x (N,H,W,ldx), dy (N,H,W,lddy), Cin, Cout)] bf16, stride 1; K = 1 (pad 0; any channel counts,
    one pixel count) or K = 3 (pad 1; identical shapes).  Returns the list of dW (Cout,Cin,K,K) fp32, allocated with NaN so that an
    element the launch does not write is seen.  out: write into these (Cout,Cin,K,K) fp32 tensors instead, one per problem."""
    args = (_hip.WgradArgs * len(problems))()
    outs = []
    for i, (a, (x, dy, Cin, Cout)) in enumerate(zip(args, problems)):
        require_gpu(x, "conv2d_wgrad_group")
        N, H, W, ldx = x.shape
        dw = torch.full((Cout, Cin, K, K), float("nan"), dtype=torch.float32, device=x.device) if out is None else out[i]
        assert dw.shape == (Cout, Cin, K, K) and dw.dtype == torch.float32 and dw.is_contiguous()
        a.dtype = _hip.tf_dtype(x.dtype)
        a.N, a.H, a.W, a.Cin, a.OH, a.OW, a.Cout, a.KH, a.KW, a.stride, a.pad = N, H, W, Cin, H, W, Cout, K, K, 1, pad
        a.ldx, a.lddy, a.x, a.dy, a.dw_oihw, a.dw_ld = ldx, dy.shape[3], ptr(x), ptr(dy), ptr(dw), Cin * K * K
        outs.append(dw)
    with torch.cuda.device(problems[0][0].device):
        check(lib().tf_conv2d_wgrad_group(args, len(problems), stream()), "tf_conv2d_wgrad_group")
    return outs

