"""The device-side target assigner of the loaders (replaces DataProcessor.get_heatmaps) and the counters it feeds.  SyntheticCrops,
SyntheticFaces and WIDERFace each own ONE TargetAssigner; it is the only place a loader calls ops for targets from."""
import numpy as np
import torch

from .. import ops

HEATMAP_SIZE = (63, 63)          # tinyfaces/datasets/wider_face.py:25
POS_THRESH, NEG_THRESH = 0.7, 0.3   # :26-27


class _PendingStats:
    """Per-batch counters kept on the device until the training loop reads them next to the loss meters (DetectionCriterion.flush_meters):
    a push enqueues two reductions and keeps (their stacked results, the number of rows they ran over); popping reads the batches the
    meters have already waited for."""

    def __init__(self):
        self._pending = []

    def pop(self, lag=0):
        """(rows, first counter, second counter) summed over all but the `lag` most recent batches; None when there is none."""
        n = max(0, len(self._pending) - lag)
        if n == 0:
            return None
        rows = first = second = 0
        for counts, total in self._pending[:n]:
            a, b = counts.tolist()
            rows, first, second = rows + total, first + a, second + b
        self._pending = self._pending[n:]
        return rows, first, second


class CompensationStats(_PendingStats):
    """Counters of the scale-compensated matching; `pop` returns (faces, faces with at most N positives after the stage, faces still below
    N).  The ATSS assigner (`atss=True`) pushes its match counts into the same object: the counters are then the faces that won at most
    n = 3 positives and the faces that won none.  So does the task-aligned assignment, from the criterion's pass; `label` names the assigner
    in the line the training loop prints."""

    def __init__(self, n, atss=False, label="ATSS"):
        super().__init__()
        self.n, self.atss, self.label = int(n), bool(atss), label
        self._below = 1 if atss else self.n

    def push(self, match_count):
        self._pending.append((torch.stack([(match_count <= self.n).sum(), (match_count < self._below).sum()]), int(match_count.numel())))


class IgnoreStats(_PendingStats):
    """Counters of the ignore regions (ops.dense_overlap_targets(return_ignored_count=True)); `pop` returns (images, anchors turned from
    negative to ignored, images with any)."""

    def push(self, ignored_count):
        self._pending.append((torch.stack([ignored_count.sum(), (ignored_count > 0).sum()]), int(ignored_count.numel())))


class ResidentFaces:
    """The resident faces of a batch, as the task-aligned assignment reads them between the forward pass and the criterion
    (ops.tal_assign_device): boxes_d (total, 4) f64 (degenerate boxes removed), offs_d (B + 1,) i32, total = the host's copy of its last
    entry, paste_d (B, 4) i32 or None, flips_d (B,) i32 or None.  `stats`: the CompensationStats the criterion pushes the match counts into,
    or None.  The fourth element of a batch under assigner="tal"; `to(device)` moves it as a tensor's would."""

    __slots__ = ("boxes_d", "offs_d", "total", "paste_d", "flips_d", "stats")

    def __init__(self, boxes_d, offs_d, total, paste_d=None, flips_d=None, stats=None):
        self.boxes_d, self.offs_d, self.total, self.paste_d, self.flips_d, self.stats = boxes_d, offs_d, int(total), paste_d, flips_d, stats

    def to(self, device, non_blocking=False):
        mv = lambda t: None if t is None else t.to(device, non_blocking=non_blocking)
        moved = [mv(t) for t in (self.boxes_d, self.offs_d, self.paste_d, self.flips_d)]
        if all(a is b for a, b in zip(moved, (self.boxes_d, self.offs_d, self.paste_d, self.flips_d))):
            return self                                       # already there
        return ResidentFaces(moved[0], moved[1], self.total, moved[2], moved[3], self.stats)

    def __len__(self):
        return self.offs_d.numel() - 1


class TargetAssigner:
    """boxes (+ paste box / flip) -> (class_map, regression_map) on the GPU.
    Replaces DataProcessor.get_padding/get_heatmaps (tinyfaces/datasets/processor.py:114-277).
    compensate = (N, T): scale-compensated matching (ops.dense_overlap_targets(compensate=)); `stats` then collects its counters.
    ignore = (measure, thresh): a call may then pass `ignore_boxes` (ops.dense_overlap_targets(ignore_boxes=)); `ignore_stats` collects the counters.
    assigner = "atss": the maps come from ops.atss_targets(topk=atss_topk) instead; pos_thresh, neg_thresh, seed and noise are then unused, and
    `stats` collects the faces that won at most 3 positives and those that won none.
    assigner = "tal": the call returns the BASE maps -- the dense_overlap path with no faces (-1 on unpadded anchors, 0 over padding and
    border, regression map 0), then the ignore pass as always -- and, as a third element, the ResidentFaces of the batch: the criterion
    assigns from the predictions (DetectionCriterion(assigner=TaskAligned(tal_topk, tal_alpha, tal_beta))) and pushes its match counts into `stats`."""

    def __init__(self, templates, heatmap_size=HEATMAP_SIZE, rf=ops.RF, pos_thresh=POS_THRESH, neg_thresh=NEG_THRESH, seed=0, compensate=None,
                 ignore=None, assigner="dense_overlap", atss_topk=ops.ATSS_TOPK, tal_topk=ops.TAL_TOPK, tal_alpha=ops.TAL_ALPHA, tal_beta=ops.TAL_BETA):
        self.templates, self.heatmap_size, self.rf = templates, heatmap_size, rf
        self.pos_thresh, self.neg_thresh, self.seed, self.calls = pos_thresh, neg_thresh, seed, 0
        self.compensate = ops.check_compensate(compensate, pos_thresh)
        self.assigner, self.atss_topk = ops.check_assigner(assigner, atss_topk, self.compensate)
        self.stats = None if self.compensate is None else CompensationStats(self.compensate[0])
        self.tal_topk, self.tal_alpha, self.tal_beta = ops.check_tal(tal_topk, tal_alpha, tal_beta)
        if self.assigner == "atss":
            self.stats = CompensationStats(3, atss=True)
        if self.assigner == "tal":
            self.stats = CompensationStats(3, atss=True, label="TAL")
        self.ignore = ops.check_ignore(ignore)
        self.ignore_stats = None if self.ignore is None else IgnoreStats()

    def __call__(self, boxes_per_image, paste_boxes=None, flips=None, device="cuda", noise=None, ignore_boxes=None, seed=None):
        """seed: the seed of the dense_overlap sampling, passed on as it is; None = self.seed * 1000003 + the number of this call."""
        self.calls += 1
        if ignore_boxes is not None and self.ignore is None:
            raise ValueError("TargetAssigner: ignore_boxes needs ignore=(measure, thresh) at construction")
        kw = dict(paste_boxes=paste_boxes, flips=flips, device=device)
        if self.assigner == "tal":
            return self._base_maps(boxes_per_image, kw, ignore_boxes)
        if self.assigner == "atss":
            fn = ops.atss_targets
            kw.update(topk=self.atss_topk, return_match_count=True)
        else:
            fn = ops.dense_overlap_targets
            kw.update(noise=noise, seed=self.seed * 1000003 + self.calls if seed is None else seed, pos_thresh=self.pos_thresh, neg_thresh=self.neg_thresh)
            if self.compensate is not None:
                kw.update(compensate=self.compensate, return_match_count=True)
        if ignore_boxes is not None:
            kw.update(ignore_boxes=ignore_boxes, ignore=self.ignore, return_ignored_count=True)
        out = fn(boxes_per_image, self.templates, self.heatmap_size, self.rf, **kw)
        if self.stats is not None:
            self.stats.push(out[2])
        if ignore_boxes is not None:
            self.ignore_stats.push(out[-1])
        return out[0], out[1]

    def _base_maps(self, boxes_per_image, kw, ignore_boxes):
        """assigner = "tal": (class_map, regression_map, ResidentFaces)."""
        none = [torch.zeros(0, 4, dtype=torch.float64)] * len(boxes_per_image)
        if ignore_boxes is not None:
            kw.update(ignore_boxes=ignore_boxes, ignore=self.ignore, return_ignored_count=True)
        out = ops.dense_overlap_targets(none, self.templates, self.heatmap_size, self.rf, pos_thresh=self.pos_thresh, neg_thresh=self.neg_thresh, **kw)
        if ignore_boxes is not None:
            self.ignore_stats.push(out[-1])
        dev, B = out[0].device, len(boxes_per_image)
        boxes_d, offs_d, total = ops._upload_boxes(boxes_per_image, dev)
        paste, flips = kw["paste_boxes"], kw["flips"]
        paste_d = None if paste is None else torch.as_tensor(np.asarray(paste), dtype=torch.int32).reshape(B, 4).to(dev)
        flips_d = None if flips is None else torch.as_tensor(np.asarray(flips), dtype=torch.int32).reshape(B).to(dev)
        return out[0], out[1], ResidentFaces(boxes_d, offs_d, total, paste_d, flips_d, self.stats)
