"""DetectionCriterion -- call surface of the reference's tinyfaces/models/loss.py:7-97, computed by
one fused HIP pass (csrc/criterion.hip): OHEM, balance sampling, masked SoftMargin + SmoothL1 sums
and d(total)/d(output), with no device->host->device round trip (loss.py:47-57 does one per step).
`cls_loss="focal"` is the one addition to that surface: sigmoid focal loss over every labelled anchor, no mining and no sampling, by the
focal form of the same pass (tf_criterion_focal_fwd_bwd); `reg_loss="iou" | "giou" | "diou"` gives that form an overlap regression loss, one
term per positive in place of the four SmoothL1 terms (tf_criterion_focal_box_fwd_bwd).  `cls_loss="qfl"` is the quality focal form of that pass
(tf_criterion_quality_fwd_bwd): a positive's logit is trained towards the IoU of its own predicted box with its target.
`assigner=TaskAligned(...)` puts the task-aligned target assignment (tf_targets_tal) in front of whichever pass is chosen: the maps arrive
without a face assigned and the positives are chosen from the output itself; `TaskAligned(aligned_targets=True)` also keeps the assignment's
normalised alignment of every positive and trains towards it with TOOD's loss (tf_targets_tal_aligned, tf_criterion_aligned_fwd_bwd)."""
import torch
from torch import nn

from .. import ops


class AvgMeter:
    """The running per-image loss the trainer prints (attributes `average`, `num_averaged` and methods `update` / `reset` of the
    reference's meter, loss.py:7-21; it is never reset between epochs there).  A batch contributes its SUMMED loss with weight
    `size`, so the value is sum(loss) / sum(size) -- kept as that quotient's incremental update so that a printed value equals
    the reference's digit for digit (trainer two-step golden log, tests/test_gpu_model.py)."""

    __slots__ = ("average", "num_averaged")

    def __init__(self):
        self.reset()

    def reset(self):
        self.average, self.num_averaged = 0, 0

    def update(self, loss, size):
        seen = self.num_averaged
        self.num_averaged = seen + size
        self.average = (seen * self.average + float(loss)) / self.num_averaged


class TaskAligned:
    """The parameters of the task-aligned assignment (TOOD's TaskAlignedAssigner; the rule is in include/tinyfaces_hip.h, "TAL"): every face
    claims its `topk` anchors of largest sigmoid(logit)^alpha * IoU(predicted box, face)^beta among those whose centre lies inside it.
    topk an integer in 1..32, alpha finite and >= 0, beta finite and > 0 (ValueError otherwise).  Hand it to DetectionCriterion(assigner=).
    aligned_targets=True: TOOD's loss on top of its assignment (step 7 of the rule).  The assignment also stores every won anchor's normalised
    alignment t = m / max m * max u (the maxima over the anchors its face won), and the criterion -- cls_loss="qfl" is required -- trains the
    class logit of a positive towards t instead of the IoU of its own box and weights its regression term by t."""

    __slots__ = ("topk", "alpha", "beta", "aligned_targets")

    def __init__(self, topk=ops.TAL_TOPK, alpha=ops.TAL_ALPHA, beta=ops.TAL_BETA, aligned_targets=False):
        self.topk, self.alpha, self.beta = ops.check_tal(topk, alpha, beta)
        if not isinstance(aligned_targets, bool):
            raise ValueError(f"TaskAligned: aligned_targets must be True or False, got {aligned_targets!r}")
        self.aligned_targets = aligned_targets

    def __repr__(self):
        return f"TaskAligned(topk={self.topk}, alpha={self.alpha}, beta={self.beta}" + (", aligned_targets=True)" if self.aligned_targets else ")")


class _CriterionFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, output, owner, class_map, regression_map, faces=None):
        if faces is None:
            loss2, grad, labels = owner._fwd_bwd(output.detach(), class_map, regression_map, want_labels=owner.keep_labels)
        else:
            loss2, grad, labels = owner._fwd_bwd(output.detach(), class_map, regression_map, want_labels=owner.keep_labels, faces=faces)
        ctx.save_for_backward(grad)
        owner._loss2 = loss2
        owner.sampled_class_map = labels
        total = loss2[0] + owner.reg_weight * loss2[1]
        return total.to(output.dtype)

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g.to(grad.dtype), None, None, None, None


class DetectionCriterion(nn.Module):
    """The loss for the Tiny Faces detector (loss.py:24-97).

    `lazy_meters=True` (used by the fast trainer) defers the two `float(loss)` host syncs of
    loss.py:90-91 to the moment `.class_average.average` is read.

    `cls_loss="focal"`: sigmoid focal loss (Lin et al. 2017) with `focal_gamma` and `focal_alpha` (torchvision's sigmoid_focal_loss
    convention: a negative alpha switches the weighting off) over EVERY labelled anchor, SmoothL1 over every positive; no OHEM, no
    sampling (`ohem_thresh`, `max_pos` / `max_neg`, the seed and `inject_sampling` do not apply) and `class_map` is only read.
    `focal_normalize="pos"`: every image's two sums and its gradient are divided by max(1, its number of positives) and the images are
    summed, so an image's loss does not depend on the batch it is in; "none": the plain sums.  The meters receive the normalised sums.

    `reg_loss="iou" | "giou" | "diou"` (with cls_loss="focal" only): every positive's regression term is 1 - IoU (plus GIoU's enclosing-box
    term, Rezatofighi et al. 2019, or DIoU's centre-distance term, Zheng et al. 2020) of the predicted and the target box in the anchor's
    template-normalised frame, predicted log sizes clamped to +-log(1000 / 16); include/tinyfaces_hip.h has the definition.  One term per
    positive, so `reg_average` receives a sum bounded by 2 per positive: `reg_weight` is normally raised with it.  `templates`: the (nt, 4 or 5)
    table of tinyfaces/datasets/templates.py, required for "diou" (its centre distance needs every template's aspect ratio).  It is held as a plain
    tensor and moved to the output's device on first use, not as a registered buffer: the criterion stays a module without state.

    `cls_loss="qfl"`: quality focal loss (Li et al. 2020, Generalized Focal Loss; the classification loss of SCRFD) with exponent `qfl_beta`
    over EVERY labelled anchor: with sigma = sigmoid(logit), QFL = |sigma - q|^beta (softplus(logit) - q logit), q = 0 for a negative and
    q = min(1, IoU) of the positive's OWN predicted box with its target (the IoU of the overlap losses above, computed in the same pass; q is a
    constant: nothing flows from it into the regression channels), so the score says "face, and this well localised".  Every `reg_loss` goes
    with it; no OHEM and no sampling, as with focal; `focal_gamma` and `focal_alpha` are unused, `focal_normalize` keeps its meaning.
    `qfl_beta` must be finite and >= 1; for 1 <= beta < 2 the gradient is ill-conditioned where sigma is close to q, and for beta = 1 it
    jumps at sigma = q.  The loss vector then has four elements, [cls, reg, sum of q over the positives, number of positives], and
    `quality_average` (a third AvgMeter, fed with the last two) is the mean IoU of the predicted boxes of all positives seen with their targets.

    `assigner=TaskAligned(topk, alpha, beta)`: task-aligned target assignment (Feng et al. 2021, TOOD) from the network's own output, on the device,
    between the forward pass and the loss pass above (ops.tal_assign_device; the rule is in include/tinyfaces_hip.h, "TAL").  `forward` /
    `_fwd_bwd` then take `faces`, the ResidentFaces of the batch (tinyfaces/datasets/targets.py; what a loader with assigner="tal" delivers as its
    fourth element), and `class_map` / `regression_map` arrive as the base maps (no face assigned) and are completed IN PLACE, under no_grad,
    before the loss pass reads them: every `cls_loss` / `reg_loss` combination works unchanged.  `templates` (the (nt, 4 or 5) table) and `rf`
    (the receptive-field geometry) are required with it.  The match counts go to `faces.stats` (the loader's CompensationStats) when there is
    one.  `faces` without an assigner, and an assigner without `faces`, is a ValueError.

    `assigner=TaskAligned(..., aligned_targets=True)` (with cls_loss="qfl" only; ValueError otherwise): TOOD's task-aligned loss.  The assignment
    also writes every won anchor's normalised alignment t = m / max m * max u, the maxima over the anchors its face won (step 7 of the rule;
    ops.tal_assign_device(align_out=) into a buffer of the maps' shape the criterion keeps), and the loss pass is tf_criterion_aligned_fwd_bwd
    (ops.criterion_aligned_fwd_bwd): the quality focal form with q = min(1, max(0, t)) as the target of a positive, and every positive's
    regression term -- whichever `reg_loss` -- weighted by q.  `focal_normalize="align"` (accepted only here) divides every image's sums and
    gradient by max(1, the sum of q over its positives): TOOD's avg_factor, per image.  `quality_average` then reports the mean TARGET of all
    positives seen (sum of q / number of positives), not a mean IoU.  Not implemented: varifocal loss."""

    CLS_LOSSES = ("soft_margin", "focal", "qfl")
    REG_LOSSES = ("smooth_l1", "iou", "giou", "diou")

    def __init__(self, n_templates=25, reg_weight=1, pos_fraction=0.5, seed=0, lazy_meters=False, keep_labels=False,
                 cls_loss="soft_margin", focal_gamma=2.0, focal_alpha=0.25, focal_normalize="pos", reg_loss="smooth_l1", templates=None,
                 qfl_beta=2.0, assigner=None, rf=None):
        super().__init__()
        if assigner is not None:
            if not isinstance(assigner, TaskAligned):
                raise ValueError(f"DetectionCriterion: assigner must be None or a TaskAligned, got {assigner!r}")
            if templates is None:
                raise ValueError("DetectionCriterion: assigner=TaskAligned(...) needs templates (the anchors the predictions are decoded against)")
            t = ops._upload_templates(templates, "cpu")
            if t.dim() != 2 or t.shape[0] != n_templates or t.shape[1] < 4:
                raise ValueError(f"DetectionCriterion: templates must be an (n_templates, >= 4) table, got shape {tuple(t.shape)}")
            self._templates_f64 = t
        self.assigner, self.rf = assigner, (ops.RF if rf is None else rf)
        if cls_loss not in self.CLS_LOSSES:
            raise ValueError(f"DetectionCriterion: cls_loss must be one of {self.CLS_LOSSES}, got {cls_loss!r}")
        self.aligned_targets = bool(getattr(assigner, "aligned_targets", False))
        if self.aligned_targets and cls_loss != "qfl":
            raise ValueError(f"DetectionCriterion: TaskAligned(aligned_targets=True) needs cls_loss='qfl' (the aligned target takes the place of the IoU "
                             f"in the quality focal form), got cls_loss={cls_loss!r}")
        if focal_normalize == "align" and not self.aligned_targets:
            raise ValueError("DetectionCriterion: focal_normalize='align' divides by the sum of the aligned targets: it needs "
                             "assigner=TaskAligned(..., aligned_targets=True)")
        ops.check_focal(focal_gamma, focal_alpha, "pos" if focal_normalize == "align" else focal_normalize)
        ops.check_qfl(qfl_beta, "pos" if focal_normalize == "align" else focal_normalize)
        self._align_map = None
        self._template_wh = None if templates is None else ops.template_wh(templates)
        ops.check_reg_loss(reg_loss, reg_weight, self._template_wh, n_templates)
        self._check_reg_with_cls(reg_loss, cls_loss)
        self.reg_loss = reg_loss
        self.cls_loss = cls_loss
        self.focal_gamma, self.focal_alpha, self.focal_normalize = float(focal_gamma), float(focal_alpha), focal_normalize
        self.qfl_beta = float(qfl_beta)
        self.n_templates = n_templates
        self.reg_weight = reg_weight
        self.pos_fraction = pos_fraction
        sample_size = 256                                                  # utils.py:103
        self.max_pos = int(sample_size * pos_fraction)                     # utils.py:111
        self.max_neg = int(self.max_pos * (1 - pos_fraction) / pos_fraction)   # utils.py:126
        self.ohem_thresh = 0.03                                            # loss.py:62
        self.class_average = AvgMeter()
        self.reg_average = AvgMeter()
        self.quality_average = AvgMeter()                                  # cls_loss="qfl" only: the mean IoU of the positives' predicted boxes
        self.masked_class_loss = None
        self.masked_reg_loss = None
        self.total_loss = None
        self.keep_labels = keep_labels
        self.lazy_meters = lazy_meters
        self._seed, self._calls = int(seed), 0
        self._pos_keep = self._neg_keep = None
        self._pending = []

    @staticmethod
    def _check_reg_with_cls(reg_loss, cls_loss):
        if reg_loss != "smooth_l1" and cls_loss == "soft_margin":
            raise ValueError(f"DetectionCriterion: reg_loss={reg_loss!r} needs cls_loss='focal'; the soft-margin pass is the reference's surface (OHEM, "
                             "the 256-sample draw, SmoothL1) and its kernels are left as they are")

    def _next_seed(self):
        self._calls += 1
        return (self._seed * 0x9E3779B97F4A7C15 + self._calls) & (2**64 - 1)

    def inject_sampling(self, pos_keep, neg_keep):
        """Parity hook: keep flags indexed by C-order rank of the positive / negative labels of
        each image, (B, nt*H*W) uint8 -- replays the reference's np.random.permutation draws."""
        if self.cls_loss == "focal":
            raise RuntimeError("DetectionCriterion.inject_sampling: cls_loss='focal' samples nothing (every labelled anchor contributes)")
        if self.cls_loss == "qfl":
            raise RuntimeError("DetectionCriterion.inject_sampling: cls_loss='qfl' samples nothing (every labelled anchor contributes)")
        self._pos_keep, self._neg_keep = pos_keep, neg_keep

    def _template_wh_on(self, device):
        """The (dw, dh) table of the overlap losses, moved to `device` the first time it is asked for there (None stays None)."""
        if self._template_wh is not None and self._template_wh.device != device:
            self._template_wh = self._template_wh.to(device)
        return self._template_wh

    def _assign(self, out, class_map, regression_map, faces):
        """The task-aligned assignment in front of the loss pass: completes the two maps in place from `out` (only read, under no_grad)."""
        if self.assigner is None:
            raise ValueError("DetectionCriterion: faces= needs assigner=TaskAligned(...) at construction")
        if self._templates_f64.device != out.device:
            self._templates_f64 = self._templates_f64.to(out.device)
        want = getattr(faces, "stats", None) is not None
        more = {}
        if getattr(self, "aligned_targets", False):                     # the aligned targets of this step's positives: a buffer of the maps' shape, kept
            if self._align_map is None or self._align_map.shape != class_map.shape or self._align_map.device != class_map.device:
                self._align_map = torch.empty_like(class_map, dtype=torch.float32, memory_format=torch.contiguous_format)
            more["align_out"] = self._align_map
        with torch.no_grad():
            res = ops.tal_assign_device(out.contiguous(), class_map, regression_map, faces.boxes_d, faces.offs_d, faces.total, self._templates_f64, None, self.rf,
                                        faces.paste_d, faces.flips_d, self.assigner.topk, self.assigner.alpha, self.assigner.beta, return_match_count=want,
                                        **more)
        if want:
            faces.stats.push(res[2])

    def _fwd_bwd(self, out, class_map, regression_map, want_labels=False, faces=None):
        """The fused loss + gradient pass of this criterion's `cls_loss`, for the autograd function above and for TrainEngine.step:
        (loss[2] f64 device tensor, d(total)/d(out), labels that entered the loss).  soft_margin mines `class_map` in place and returns
        the sampled labels if `want_labels`, else None; focal and qfl only read `class_map`, which IS the labels that entered.  With qfl the
        loss tensor has four elements: [cls, reg, sum of q over the positives, number of positives].
        faces (with assigner=TaskAligned(...) only, and then required): the two maps are first completed in place by the task-aligned assignment."""
        if faces is not None:
            self._assign(out, class_map, regression_map, faces)
        elif getattr(self, "assigner", None) is not None:
            raise ValueError("DetectionCriterion: assigner=TaskAligned(...) needs faces= (the ResidentFaces of the batch)")
        if self.reg_loss != "smooth_l1":
            ops.check_reg_loss(self.reg_loss, self.reg_weight, self._template_wh, self.n_templates)
            self._check_reg_with_cls(self.reg_loss, self.cls_loss)
        if getattr(self, "aligned_targets", False):
            if self.cls_loss != "qfl":
                raise ValueError(f"DetectionCriterion: TaskAligned(aligned_targets=True) needs cls_loss='qfl', got cls_loss={self.cls_loss!r}")
            loss4, grad, _ = ops.criterion_aligned_fwd_bwd(out, class_map, regression_map, self._align_map, self.n_templates, self.reg_weight, self.qfl_beta,
                                                           self.focal_normalize, self.reg_loss, self._template_wh_on(out.device))
            return loss4, grad, class_map
        if self.cls_loss == "qfl":
            loss4, grad, _ = ops.criterion_quality_fwd_bwd(out, class_map, regression_map, self.n_templates, self.reg_weight, self.qfl_beta,
                                                           self.focal_normalize, self.reg_loss, self._template_wh_on(out.device))
            return loss4, grad, class_map
        if self.cls_loss == "focal" and self.reg_loss != "smooth_l1":
            loss2, grad, _ = ops.criterion_focal_box_fwd_bwd(out, class_map, regression_map, self.n_templates, self.reg_weight, self.focal_gamma,
                                                             self.focal_alpha, self.focal_normalize, self.reg_loss, self._template_wh_on(out.device))
            return loss2, grad, class_map
        if self.cls_loss == "focal":
            loss2, grad, _ = ops.criterion_focal_fwd_bwd(out, class_map, regression_map, self.n_templates, self.reg_weight, self.focal_gamma,
                                                         self.focal_alpha, self.focal_normalize)
            return loss2, grad, class_map
        if self.cls_loss != "soft_margin":
            raise ValueError(f"DetectionCriterion: cls_loss must be one of {self.CLS_LOSSES}, got {self.cls_loss!r}")
        return ops.criterion_fwd_bwd(out, class_map, regression_map, self.n_templates, self.reg_weight, self.ohem_thresh, self.max_pos,
                                     self.max_neg, self._pos_keep, self._neg_keep, self._next_seed(), want_labels=want_labels)

    def flush_meters(self, lag=0):
        """Feed the loss meters from the device values of the steps enqueued so far.  `lag` = the number of MOST RECENT steps left pending: reading a
        step's loss waits for that step, so a training loop that flushes everything after every step (lag = 0) never has the next batch in preparation
        while the GPU works; with lag = 1 the host stays one step ahead and the printed averages trail by one step."""
        n = max(0, len(self._pending) - lag)
        for loss2, size in self._pending[:n]:
            v = loss2.tolist()
            self._update_meters(v, size)
        self._pending = self._pending[n:]

    def _update_meters(self, v, size):
        """v: the host copy of one step's loss vector.  Elements 2 and 3 (qfl only) are the sum of q over the step's positives and their
        number: `quality_average` is the mean IoU over all positives seen (with aligned targets: their mean target); a step without a positive
        leaves it alone."""
        self.class_average.update(v[0], size)
        self.reg_average.update(v[1], size)
        if len(v) >= 4 and v[3] > 0:
            self.quality_average.update(v[2], int(v[3]))

    def forward(self, output, class_map, regression_map, faces=None):
        if (faces is None) != (self.assigner is None):
            raise ValueError("DetectionCriterion: faces= and assigner=TaskAligned(...) go together" if faces is not None else
                             "DetectionCriterion: assigner=TaskAligned(...) needs faces= (the ResidentFaces of the batch)")
        if not output.is_cuda:
            raise RuntimeError("DetectionCriterion: HIP kernel only (no CPU fallback)")
        if class_map.dtype != torch.float32 or not class_map.is_contiguous():
            class_map = class_map.float().contiguous()
        if faces is None:
            total = _CriterionFunction.apply(output, self, class_map, regression_map.float())
        else:
            total = _CriterionFunction.apply(output, self, class_map, regression_map.float().contiguous(), faces)
        self.total_loss = total
        loss2 = self._loss2
        self.masked_class_loss, self.masked_reg_loss = loss2[0], loss2[1]   # already summed (loss.py:87-91 only uses .sum())
        if self.lazy_meters:
            self._pending.append((loss2, output.size(0)))
        else:
            self._update_meters(loss2.tolist(), output.size(0))            # one sync instead of two (loss.py:90-91)
        return total

    def reset(self):
        self.class_average.reset()
        self.reg_average.reset()
        self.quality_average.reset()
