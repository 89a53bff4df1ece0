"""Training entry point with the reference's flags (main.py:18-36) on the MI355X hot path.

    python main.py <traindata> <valdata> [--dataset-root ...]          # reference usage (Makefile:11-12)
    python main.py synthetic synthetic --epochs 1                      # seeded 500x500 crops, no dataset needed
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 main.py synthetic synthetic   # data parallel

Additions (existing flags keep their names and defaults): --fused / --no-fused (TrainEngine vs torch.optim.SGD through
autograd), --dtype bf16|fp32, --synthetic-len.  The schedule is the reference's: SGD(momentum, weight decay), StepLR(20),
a checkpoint every --save-every epochs (main.py:39-104); --optimizer adamw, --warmup-iters, --color-jitter and
--val-every (the AP on `valdata` after every N-th epoch; without it `valdata` is ignored, as in the reference) are opt-in."""
import argparse
import math
import os
from pathlib import Path

import torch
from torch import optim

from tinyfaces import ops, parallel, trainer, transforms
from tinyfaces.datasets import get_dataloader
from tinyfaces.datasets.templates import load_templates
from tinyfaces.ema import ModelEma, ema_decay_at
from tinyfaces.engine import TrainEngine
from tinyfaces.models.loss import DetectionCriterion, TaskAligned
from tinyfaces.models import model as model_zoo
from tinyfaces.models.model import DetectionModel

NUM_TEMPLATES = 25
LR_STEP = 20            # StepLR(step_size=20, gamma=0.1), main.py:81-83

# the reference's command line (name, argparse keyword arguments), then this repo's additions
REFERENCE_FLAGS = [
    ("traindata", {}), ("valdata", {}),
    ("--dataset-root", dict(default="")), ("--dataset", dict(default="WIDERFace")),
    ("--lr", dict(default=1e-4, type=float)), ("--weight-decay", dict(default=0.0005, type=float)), ("--momentum", dict(default=0.9, type=float)),
    ("--batch_size", dict(default=12, type=int)), ("--workers", dict(default=8, type=int)),
    ("--start-epoch", dict(default=0, type=int)), ("--epochs", dict(default=50, type=int)), ("--save-every", dict(default=10, type=int)),
    ("--resume", dict(default="", help="checkpoint path (the reference declares it store_true but uses it as a path, main.py:33,74)")),
    ("--debug", dict(action="store_true")),
]
EXTRA_FLAGS = [
    ("--fused", dict(dest="fused", action="store_true", default=True)), ("--no-fused", dict(dest="fused", action="store_false")),
    ("--dtype", dict(default="bf16", choices=["bf16", "fp32"])), ("--synthetic-len", dict(dest="synthetic_len", default=240, type=int)),
    ("--seed", dict(default=0, type=int, help="synthetic data / sampling seed (each rank derives its own from it)")),
    ("--pretrained", dict(default="", help="local torchvision-format state_dict (.pth) of the --base-model trunk: the reference starts "
                                           "from ResNet101_Weights.IMAGENET1K_V1 (model.py:13-14), which it downloads; there is no network here")),
    ("--init", dict(default="tame", choices=["tame", "kaiming"],
                    help="from-scratch runs only (no --resume / --pretrained): `tame` = the last BN of every bottleneck at 0.1 and the head weights x 0.05 "
                         "(plain kaiming saturates the sigmoid of a 101-layer random trunk: SURVEY.md 7.1); `kaiming` = torch's defaults")),
    ("--save-path", dict(dest="save_path", default="weights", help="directory of the checkpoints (the reference writes ./weights, trainer.py:20-28)")),
    ("--ohem-thresh", dict(dest="ohem_thresh", default=0.03, type=float,
                           help="loss.py:62 zeroes every label -- positives too -- whose soft-margin loss is below this (0.03: y*logit > 3.49; defect D7): a positive "
                                "the classifier is sure of also leaves the REGRESSION loss, so the boxes of a detector trained from scratch stop improving as soon "
                                "as its scores are confident (tests/test_gpu_e2e.py).  0 switches the mining off")),
]


def tame_init_(model):
    """From-scratch initialisation that trains: bn3.weight = 0.1 in every bottleneck (the residual branches start small), head weights x 0.05."""
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("bn3.weight"):
                p.fill_(0.1)
        for name in ("score_res3", "score_res4"):
            getattr(model, name).weight.mul_(0.05)
    return model


TRUNK_HELP = ("--base-model {resnet50,resnet101,resnet152}: trunk of the detector (DetectionModel(base_model=...), model.py:12-23), "
              "default resnet101 (the reference's)")


FREEZE_HELP = ("--freeze-bn: fine-tune with every BatchNorm of the trunk frozen on its pretrained statistics and affine "
               "(DetectionModel.freeze_batchnorm: torchvision's FrozenBatchNorm2d), default off")


TRAINABLE_HELP = ("--trainable-layers {0,1,2,3,4}: train the heads and the top K of the trunk's stages layer3, layer2, layer1, stem "
                  "(DetectionModel.set_trainable_layers: torchvision's trainable_backbone_layers), default 4 = everything; K < 4 needs --freeze-bn")


CLIP_HELP = ("--clip-grad-norm FLOAT: clip the global L2 norm of the gradient to FLOAT before every update (torch.nn.utils.clip_grad_norm_ "
             "between backward() and optimizer.step(); computed and applied on the device), default off")


SKIP_HELP = ("--skip-nonfinite: a step whose gradient norm is NaN or Inf is not applied (the fused engine leaves parameters and momentum "
             "untouched; the autograd path zeroes the gradient), default off")


EMA_HELP = ("--model-ema DECAY: keep an exponential moving average of the weights with this decay, 0 < DECAY < 1 (torchvision's --model-ema, "
            "AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(DECAY)); warmed up as min(DECAY, (1 + t) / (10 + t)); updated on the device) and store "
            "it in every checkpoint as \"model_ema\" (evaluate_model.py --ema), default off")


ACCUM_HELP = ("--accum-steps N: one optimizer step per N batches (gradient accumulation: the gradients of N micro-batches are summed, as N "
              "calls of loss.backward() before one optimizer.step() would; the effective batch is batch_size x N x world size), N >= 1, default 1")


ACCUM_AVERAGE_HELP = ("--accum-average: apply the MEAN of the accumulated gradients instead of their sum (the `loss / N` of torch loops; the "
                      "reference's loss is a sum over the batch, so the sum is what a batch N times as large gives), default off")


DETERMINISTIC_HELP = ("--deterministic: run every training step without floating-point atomics (unfolded BatchNorm statistic rows, weight "
                      "gradients summed from per-block slabs in a fixed order): the same seed, weights and batches give the same checkpoint bit "
                      "for bit; slower than the default step, default off")


def deterministic_description():
    """What --deterministic guarantees and what it does not, as the start-up line prints it."""
    return ("deterministic step: same weights, optimizer state and batches in -> same weights out, bit for bit, per process (no floating-point "
            "atomics in the forward, the backward or the update); NOT covered: the soft-margin loss meters (fp64 atomics, logging only), the "
            "order inside a multi-rank gradient exchange, the data loader's worker order")


FOCAL_HELP = ("--cls-loss {soft-margin,focal}: classification loss of the criterion; focal = sigmoid focal loss (Lin et al. 2017) over every "
              "labelled anchor and SmoothL1 over every positive, with no OHEM and no 256-sample draw (--ohem-thresh is unused), default soft-margin; "
              "--focal-gamma G: its focusing exponent, G >= 0, default 2; --focal-alpha A: weight A on positives and 1 - A on negatives, A <= 1, "
              "negative = no weighting, default 0.25; --focal-normalize {pos,none,align}: pos divides every image's loss by max(1, its positives) "
              "before the images are summed, none leaves the plain sum, align (with --tal-aligned-targets only) divides it by max(1, the sum of its "
              "aligned targets), default pos")


QFL_HELP = ("--cls-loss qfl: quality focal loss (Li et al. 2020, Generalized Focal Loss; the classification loss of SCRFD) over every labelled "
            "anchor: a positive's score is trained towards the IoU of its own predicted box with its target, a negative's towards 0, on the device; "
            "no OHEM and no 256-sample draw, --focal-gamma and --focal-alpha are unused, --focal-normalize keeps its meaning, every --reg-loss goes "
            "with it; --qfl-beta B: its exponent, finite, B >= 1, default 2 (below 2 the gradient is ill-conditioned where the score meets its target)")


BOX_LOSS_HELP = ("--reg-loss {smooth-l1,iou,giou,diou}: regression loss of the criterion; iou / giou / diou (Rezatofighi et al. 2019, Zheng et al. 2020) "
                 "put one box-overlap term per positive anchor in place of the four SmoothL1 terms and need --cls-loss focal or qfl (the soft-margin pass "
                 "keeps the reference's SmoothL1), default smooth-l1; --reg-weight W: weight of the regression loss in the total, finite, W >= 0, "
                 "default 1 (an overlap loss is bounded by 2 per anchor and is normally weighted up)")


OPTIMIZER_HELP = ("--optimizer {sgd,adamw}: the update rule; adamw = torch.optim.AdamW's arithmetic (decoupled --weight-decay; --momentum is unused), "
                  "fused into the engine's update launches or torch's own on the autograd path, default sgd; --adam-beta1 B / --adam-beta2 B: its "
                  "decay rates, 0 <= B < 1, defaults 0.9 / 0.999; --adam-eps E: added to the denominator, E > 0, default 1e-8")


WARMUP_HELP = ("--warmup-iters N: linear learning-rate warm-up over the first N optimizer steps (torch.optim.lr_scheduler.LinearLR multiplied into "
               "the StepLR schedule; what torchvision's detection references do in epoch 0), N >= 0, default 0 = off; --warmup-factor F: the factor "
               "of step 0, 0 < F <= 1, default 1e-3")


JITTER_HELP = ("--color-jitter B C S H: torchvision's ColorJitter(brightness=B, contrast=C, saturation=S, hue=H) on every training image between the "
               "augmentation and ToTensor (brightness, contrast and saturation factors from [max(0, 1 - x), 1 + x], the hue factor from [-H, H], the four "
               "ops in a random order; computed on the device), four finite numbers >= 0 with H <= 0.5, default off")


COMPENSATION_HELP = ("--anchor-compensation N T: scale-compensated anchor matching (S3FD, Zhang et al. 2017) for the training targets: a face that owns "
                     "fewer than N positive anchors is topped up, on the device, with its own best-overlapping unpadded anchors of IoU >= T, best first; "
                     "N an integer in 1..64, T a number with 0.01 <= T < 0.7 (the positive threshold; below 0.3 the stage promotes negatives too), "
                     "default off")


TAL_ALIGNED_HELP = ("--tal-aligned-targets (with --assigner tal --cls-loss qfl): TOOD's task-aligned loss.  Every positive keeps the assigner's "
                    "normalised alignment m / max m * max IoU (the maxima over the anchors its face won) as its classification target in place of the "
                    "IoU of its own box, and its regression term is weighted by it; --focal-normalize align then divides every image's loss by "
                    "max(1, the sum of its aligned targets)")
ASSIGNER_HELP = ("--assigner atss: ATSS target assignment (Zhang et al. 2020; what SCRFD and TinaFace train with) for the training targets instead of "
                 "the fixed IoU thresholds: per face the --atss-topk K (1..16, default 9) unpadded cells of every template nearest to its centre are "
                 "candidates, positive from mean + std of their IoUs when the anchor centre lies inside the face; not together with "
                 "--anchor-compensation; default dense-overlap (positive from IoU 0.7, negative below 0.3). "
                 "--assigner tal: task-aligned assignment (Feng et al. 2021, TOOD; the YOLO-style face detectors after it) from the network's own output, "
                 "every step, on the device between the forward pass and the loss: per face the anchors whose centre lies inside it are ranked by "
                 "sigmoid(logit)^A * IoU(predicted box, face)^B and the best K become its positives, --tal-topk K (1..32, default 13), --tal-alpha A "
                 "(>= 0, default 1), --tal-beta B (> 0, default 6); not together with --anchor-compensation")


IGNORE_HELP = ("ignore regions for the training targets of a WIDER annotation file (S3FD, PyramidBox, RetinaFace; mmdetection's gt_bboxes_ignore): a face "
               "the policy flags owns no positive anchor, and a negative anchor that what is left of it covers gets the don't-care label on the device. "
               "--ignore-invalid: faces with invalid = 1; --ignore-blur L / --ignore-occlusion L: faces with blur / occlusion >= L, L in 1..2; "
               "--ignore-min-size S: faces whose shorter side after the scale draw is below S pixels, S > 0; --ignore-truncated: what is left of the "
               "faces the crop drops; any of them switches the feature on. --ignore-measure {iof,iou} (default iof: intersection over the anchor's "
               "area) and --ignore-thresh T (0 < T <= 1, default 0.5) set when an anchor counts as covered; alone they are an error. Default off")


def _ignore_level(text):
    value = int(text)
    if not 1 <= value <= 2:
        raise argparse.ArgumentTypeError(f"must be a level in 1..2, got {text}")
    return value


def _ignore_min_size(text):
    value = float(text)
    if not (math.isfinite(value) and value > 0):
        raise argparse.ArgumentTypeError(f"must be a finite number of pixels > 0, got {text}")
    return value


def _ignore_thresh(text):
    value = float(text)
    if not (math.isfinite(value) and 0.0 < value <= 1.0):
        raise argparse.ArgumentTypeError(f"must be a finite number with 0 < T <= 1, got {text}")
    return value


def _atss_topk(text):
    try:
        k = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--atss-topk takes an integer in 1..16, got {text!r}") from None
    if not 1 <= k <= 16:
        raise argparse.ArgumentTypeError(f"--atss-topk takes an integer in 1..16, got {text!r}")
    return k


def _tal_topk(text):
    try:
        k = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"--tal-topk takes an integer in 1..32, got {text!r}") from None
    if not 1 <= k <= 32:
        raise argparse.ArgumentTypeError(f"--tal-topk takes an integer in 1..32, got {text!r}")
    return k


def _tal_alpha(text):
    value = float(text)
    if not (math.isfinite(value) and value >= 0):
        raise argparse.ArgumentTypeError(f"--tal-alpha takes a finite number >= 0, got {text}")
    return value


def _tal_beta(text):
    value = float(text)
    if not (math.isfinite(value) and value > 0):
        raise argparse.ArgumentTypeError(f"--tal-beta takes a finite number > 0, got {text}")
    return value


def _compensation_value(text):
    """One of the two values of --anchor-compensation: what either may be (N is narrowed to an integer in 1..64 once both are known)."""
    value = float(text)
    if not (math.isfinite(value) and 0.01 <= value <= 64.0):
        raise argparse.ArgumentTypeError(f"must be an integer N in 1..64 or a threshold T with 0.01 <= T < 0.7, got {text}")
    return value


VAL_HELP = ("--val-every N: after every N-th epoch rank 0 runs the detector over `valdata` (synthetic-faces, or a WIDER annotation file with "
            "--val-gt-dir DIR, the eval_tools ground-truth directory) on the averaged weights under --model-ema, else the live ones, prints one "
            "`Val: [epoch] AP ...` line (matched and accumulated on the device, no result file), stores \"val_ap\" in the checkpoints and keeps "
            "checkpoint_best.pth, the best first setting so far; N >= 0, default 0 = off (`valdata` is then ignored); --val-prob-thresh P / "
            "--val-nms-thresh T: the detector's thresholds, in [0, 1], defaults 0.03 / 0.3 (evaluate_model.py's); --val-num-images M: the first M "
            "validation images only, M >= 1, default all")


def _val_every(text):
    value = int(text)
    if value < 0:
        raise argparse.ArgumentTypeError(f"must be an integer >= 0, got {text}")
    return value


def _val_count(text):
    value = int(text)
    if value < 1:
        raise argparse.ArgumentTypeError(f"must be an integer >= 1, got {text}")
    return value


def _unit_interval(text):
    value = float(text)
    if not 0.0 <= value <= 1.0:
        raise argparse.ArgumentTypeError(f"must be a number in [0, 1], got {text}")
    return value


def _jitter_amplitude(text):
    value = float(text)
    if not (math.isfinite(value) and value >= 0.0):
        raise argparse.ArgumentTypeError(f"must be a finite number >= 0, got {text}")
    return value


def _adam_beta(text):
    value = float(text)
    if not (math.isfinite(value) and 0.0 <= value < 1.0):
        raise argparse.ArgumentTypeError(f"must be a number in [0, 1), got {text}")
    return value


def _adam_eps(text):
    value = float(text)
    if not (math.isfinite(value) and value > 0.0):
        raise argparse.ArgumentTypeError(f"must be a finite number > 0, got {text}")
    return value


def _warmup_iters(text):
    value = int(text)
    if value < 0:
        raise argparse.ArgumentTypeError(f"must be an integer >= 0, got {text}")
    return value


def _warmup_factor(text):
    value = float(text)
    if not (math.isfinite(value) and 0.0 < value <= 1.0):
        raise argparse.ArgumentTypeError(f"must be a number in (0, 1], got {text}")
    return value


def _reg_weight(text):
    value = float(text)
    if not (math.isfinite(value) and value >= 0.0):
        raise argparse.ArgumentTypeError(f"must be a finite number >= 0, got {text}")
    return value


def _focal_gamma(text):
    value = float(text)
    if not (math.isfinite(value) and value >= 0.0):
        raise argparse.ArgumentTypeError(f"must be a finite number >= 0, got {text}")
    return value


def _focal_alpha(text):
    value = float(text)
    if not (math.isfinite(value) and value <= 1.0):
        raise argparse.ArgumentTypeError(f"must be a finite number <= 1 (negative: no weighting), got {text}")
    return value


def _qfl_beta(text):
    value = float(text)
    if not (math.isfinite(value) and value >= 1.0):
        raise argparse.ArgumentTypeError(f"must be a finite number >= 1, got {text}")
    return value


def _accum_steps(text):
    value = int(text)
    if value < 1:
        raise argparse.ArgumentTypeError(f"must be an integer >= 1, got {text}")
    return value


def _ema_decay(text):
    try:
        ema_decay_at(float(text), 0)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))
    return float(text)


def _positive_float(text):
    value = float(text)
    if not value > 0.0:
        raise argparse.ArgumentTypeError(f"must be a positive number, got {text}")
    return value


def arguments(argv=None):
    parser = argparse.ArgumentParser(epilog="; ".join((TRUNK_HELP, FREEZE_HELP, TRAINABLE_HELP, CLIP_HELP, SKIP_HELP, EMA_HELP, ACCUM_HELP, ACCUM_AVERAGE_HELP, FOCAL_HELP, QFL_HELP, BOX_LOSS_HELP, OPTIMIZER_HELP, WARMUP_HELP, JITTER_HELP, VAL_HELP, DETERMINISTIC_HELP, COMPENSATION_HELP, IGNORE_HELP)))
    for name, kw in REFERENCE_FLAGS + EXTRA_FLAGS:
        parser.add_argument(name, **kw)
    return parser.parse_args(argv)


def trunk_arguments(argv=None):
    """`arguments` plus `base_model` from --base-model, `freeze_bn` from --freeze-bn, `trainable_layers` from --trainable-layers, `clip_grad_norm`
    from --clip-grad-norm, `skip_nonfinite` from --skip-nonfinite, `model_ema` from --model-ema, `accum_steps` from --accum-steps and `accum_average`
    from --accum-average, `cls_loss` ("soft_margin" | "focal" | "qfl") from --cls-loss, `qfl_beta` from --qfl-beta, `focal_gamma`, `focal_alpha` and `focal_normalize` from
    --focal-gamma, --focal-alpha and --focal-normalize, `reg_loss` ("smooth_l1" | "iou" | "giou" | "diou") from --reg-loss and `reg_weight` from
    --reg-weight, `optimizer` ("sgd" | "adamw"), `adam_beta1`, `adam_beta2` and `adam_eps` from --optimizer, --adam-beta1, --adam-beta2 and --adam-eps,
    `warmup_iters` and `warmup_factor` from --warmup-iters and --warmup-factor, `color_jitter` (None or the four amplitudes) from --color-jitter,
    `anchor_compensation` (None or (N, T)) from --anchor-compensation, `assigner` ("dense_overlap" | "atss" | "tal"), `atss_topk` and `tal_topk` / `tal_alpha` / `tal_beta` from --assigner, --tal-* and
    --atss-topk, `ignore_policy` (None or an augment.IgnorePolicy) and `ignore` (None or
    (measure, thresh)) from the --ignore-* flags,
    `val_every`, `val_prob_thresh`, `val_nms_thresh`, `val_num_images` and `val_gt_dir` from --val-every and its companions.  Parsed apart, so that `arguments` keeps resolving exactly the reference's
    options and the additions above."""
    parser = argparse.ArgumentParser(add_help=False)
    parser.add_argument("--base-model", dest="base_model", default="resnet101", choices=list(model_zoo.TRUNKS), help=TRUNK_HELP)
    parser.add_argument("--freeze-bn", dest="freeze_bn", action="store_true", help=FREEZE_HELP)
    parser.add_argument("--trainable-layers", dest="trainable_layers", default=4, type=int, choices=range(5), help=TRAINABLE_HELP)
    parser.add_argument("--clip-grad-norm", dest="clip_grad_norm", default=None, type=_positive_float, help=CLIP_HELP)
    parser.add_argument("--skip-nonfinite", dest="skip_nonfinite", action="store_true", help=SKIP_HELP)
    parser.add_argument("--model-ema", dest="model_ema", default=None, type=_ema_decay, metavar="DECAY", help=EMA_HELP)
    parser.add_argument("--accum-steps", dest="accum_steps", default=1, type=_accum_steps, metavar="N", help=ACCUM_HELP)
    parser.add_argument("--accum-average", dest="accum_average", action="store_true", help=ACCUM_AVERAGE_HELP)
    parser.add_argument("--cls-loss", dest="cls_loss", default="soft-margin", choices=["soft-margin", "focal", "qfl"], help=FOCAL_HELP)
    parser.add_argument("--qfl-beta", dest="qfl_beta", default=2.0, type=_qfl_beta, metavar="B", help=QFL_HELP)
    parser.add_argument("--focal-gamma", dest="focal_gamma", default=2.0, type=_focal_gamma, metavar="G", help=FOCAL_HELP)
    parser.add_argument("--focal-alpha", dest="focal_alpha", default=0.25, type=_focal_alpha, metavar="A", help=FOCAL_HELP)
    parser.add_argument("--focal-normalize", dest="focal_normalize", default="pos", choices=["pos", "none", "align"], help=FOCAL_HELP)
    parser.add_argument("--reg-loss", dest="reg_loss", default="smooth-l1", choices=["smooth-l1", "iou", "giou", "diou"], help=BOX_LOSS_HELP)
    parser.add_argument("--reg-weight", dest="reg_weight", default=1.0, type=_reg_weight, metavar="W", help=BOX_LOSS_HELP)
    parser.add_argument("--optimizer", dest="optimizer", default="sgd", choices=["sgd", "adamw"], help=OPTIMIZER_HELP)
    parser.add_argument("--adam-beta1", dest="adam_beta1", default=0.9, type=_adam_beta, metavar="B", help=OPTIMIZER_HELP)
    parser.add_argument("--adam-beta2", dest="adam_beta2", default=0.999, type=_adam_beta, metavar="B", help=OPTIMIZER_HELP)
    parser.add_argument("--adam-eps", dest="adam_eps", default=1e-8, type=_adam_eps, metavar="E", help=OPTIMIZER_HELP)
    parser.add_argument("--warmup-iters", dest="warmup_iters", default=0, type=_warmup_iters, metavar="N", help=WARMUP_HELP)
    parser.add_argument("--warmup-factor", dest="warmup_factor", default=1e-3, type=_warmup_factor, metavar="F", help=WARMUP_HELP)
    parser.add_argument("--color-jitter", dest="color_jitter", default=None, type=_jitter_amplitude, nargs=4, metavar=("B", "C", "S", "H"), help=JITTER_HELP)
    parser.add_argument("--val-every", dest="val_every", default=0, type=_val_every, metavar="N", help=VAL_HELP)
    parser.add_argument("--val-prob-thresh", dest="val_prob_thresh", default=0.03, type=_unit_interval, metavar="P", help=VAL_HELP)
    parser.add_argument("--val-nms-thresh", dest="val_nms_thresh", default=0.3, type=_unit_interval, metavar="T", help=VAL_HELP)
    parser.add_argument("--val-num-images", dest="val_num_images", default=None, type=_val_count, metavar="M", help=VAL_HELP)
    parser.add_argument("--val-gt-dir", dest="val_gt_dir", default=None, metavar="DIR", help=VAL_HELP)
    parser.add_argument("--deterministic", dest="deterministic", action="store_true", help=DETERMINISTIC_HELP)
    parser.add_argument("--anchor-compensation", dest="anchor_compensation", default=None, type=_compensation_value, nargs=2, metavar=("N", "T"),
                        help=COMPENSATION_HELP)
    parser.add_argument("--assigner", dest="assigner", default="dense-overlap", choices=["dense-overlap", "atss", "tal"], help=ASSIGNER_HELP)
    parser.add_argument("--atss-topk", dest="atss_topk", default=9, type=_atss_topk, metavar="K", help=ASSIGNER_HELP)
    parser.add_argument("--tal-topk", dest="tal_topk", default=13, type=_tal_topk, metavar="K", help=ASSIGNER_HELP)
    parser.add_argument("--tal-alpha", dest="tal_alpha", default=1.0, type=_tal_alpha, metavar="A", help=ASSIGNER_HELP)
    parser.add_argument("--tal-beta", dest="tal_beta", default=6.0, type=_tal_beta, metavar="B", help=ASSIGNER_HELP)
    parser.add_argument("--tal-aligned-targets", dest="tal_aligned_targets", action="store_true", help=TAL_ALIGNED_HELP)
    parser.add_argument("--ignore-invalid", dest="ignore_invalid", action="store_true", help=IGNORE_HELP)
    parser.add_argument("--ignore-blur", dest="ignore_blur", default=None, type=_ignore_level, metavar="L", help=IGNORE_HELP)
    parser.add_argument("--ignore-occlusion", dest="ignore_occlusion", default=None, type=_ignore_level, metavar="L", help=IGNORE_HELP)
    parser.add_argument("--ignore-min-size", dest="ignore_min_size", default=None, type=_ignore_min_size, metavar="S", help=IGNORE_HELP)
    parser.add_argument("--ignore-truncated", dest="ignore_truncated", action="store_true", help=IGNORE_HELP)
    parser.add_argument("--ignore-measure", dest="ignore_measure", default=None, choices=["iof", "iou"], help=IGNORE_HELP)
    parser.add_argument("--ignore-thresh", dest="ignore_thresh", default=None, type=_ignore_thresh, metavar="T", help=IGNORE_HELP)
    known, rest = parser.parse_known_args(argv)
    ignore_on = (known.ignore_invalid or known.ignore_truncated or known.ignore_blur is not None or known.ignore_occlusion is not None
                 or known.ignore_min_size is not None)
    if not ignore_on and known.ignore_measure is not None:
        parser.error("--ignore-measure needs one of --ignore-invalid, --ignore-blur, --ignore-occlusion, --ignore-min-size, --ignore-truncated")
    if not ignore_on and known.ignore_thresh is not None:
        parser.error("--ignore-thresh needs one of --ignore-invalid, --ignore-blur, --ignore-occlusion, --ignore-min-size, --ignore-truncated")
    if known.anchor_compensation is not None and known.assigner == "atss":
        parser.error("--anchor-compensation tops up the owners that the dense-overlap assignment computes; it does not go with --assigner atss")
    if known.anchor_compensation is not None and known.assigner == "tal":
        parser.error("--anchor-compensation tops up the owners that the dense-overlap assignment computes; it does not go with --assigner tal")
    if known.tal_aligned_targets and (known.assigner != "tal" or known.cls_loss != "qfl"):
        parser.error("--tal-aligned-targets trains towards the alignment values of the task-aligned assignment in the quality focal form: it needs "
                     "--assigner tal --cls-loss qfl")
    if known.focal_normalize == "align" and not known.tal_aligned_targets:
        parser.error("--focal-normalize align divides by the sum of the aligned targets: it needs --tal-aligned-targets")
    if known.anchor_compensation is not None:
        n, t = known.anchor_compensation
        if n != int(n) or not 1 <= int(n) <= 64:
            parser.error(f"--anchor-compensation: N must be an integer in 1..64, got {n:g}")
        if not 0.01 <= t < 0.7:
            parser.error(f"--anchor-compensation: T must satisfy 0.01 <= T < 0.7 (the positive threshold), got {t:g}")
    if known.color_jitter is not None and known.color_jitter[3] > 0.5:
        parser.error(f"--color-jitter: the hue amplitude H must be <= 0.5, got {known.color_jitter[3]:g}")
    if known.trainable_layers < 4 and not known.freeze_bn:
        parser.error(f"--trainable-layers {known.trainable_layers} freezes stages of the trunk, which is defined on frozen BatchNorm only: add --freeze-bn")
    if known.reg_loss != "smooth-l1" and known.cls_loss not in ("focal", "qfl"):
        parser.error(f"--reg-loss {known.reg_loss} needs --cls-loss focal or qfl: the soft-margin pass keeps the reference's SmoothL1")
    args = arguments(rest)
    args.base_model = known.base_model
    args.freeze_bn = known.freeze_bn
    args.trainable_layers = known.trainable_layers
    args.clip_grad_norm = known.clip_grad_norm
    args.skip_nonfinite = known.skip_nonfinite
    args.model_ema = known.model_ema
    args.accum_steps = known.accum_steps
    args.accum_average = known.accum_average
    args.cls_loss = known.cls_loss.replace("-", "_")
    args.qfl_beta = known.qfl_beta
    args.focal_gamma = known.focal_gamma
    args.focal_alpha = known.focal_alpha
    args.focal_normalize = known.focal_normalize
    args.reg_loss = known.reg_loss.replace("-", "_")
    args.reg_weight = known.reg_weight
    args.optimizer = known.optimizer
    args.adam_beta1, args.adam_beta2, args.adam_eps = known.adam_beta1, known.adam_beta2, known.adam_eps
    args.warmup_iters, args.warmup_factor = known.warmup_iters, known.warmup_factor
    args.color_jitter = None if known.color_jitter is None else tuple(known.color_jitter)
    args.val_every, args.val_num_images, args.val_gt_dir = known.val_every, known.val_num_images, known.val_gt_dir
    args.val_prob_thresh, args.val_nms_thresh = known.val_prob_thresh, known.val_nms_thresh
    args.deterministic = known.deterministic
    args.anchor_compensation = None if known.anchor_compensation is None else (int(known.anchor_compensation[0]), float(known.anchor_compensation[1]))
    args.assigner, args.atss_topk = known.assigner.replace("-", "_"), known.atss_topk
    args.tal_topk, args.tal_alpha, args.tal_beta = known.tal_topk, known.tal_alpha, known.tal_beta
    args.tal_aligned_targets = known.tal_aligned_targets
    if args.assigner != "dense_overlap" and (str(args.traindata) == "synthetic" or getattr(args, "synthetic", False)):
        parser.error(f"--assigner {args.assigner} applies to a WIDER annotation file or to synthetic-faces: the synthetic crops are a throughput workload of the "
                     "dense-overlap assigner")
    args.ignore_policy = args.ignore = None
    if ignore_on:
        from tinyfaces.datasets.augment import IgnorePolicy
        args.ignore_policy = IgnorePolicy(invalid=known.ignore_invalid, blur=known.ignore_blur, occlusion=known.ignore_occlusion,
                                          min_size=known.ignore_min_size, truncated=known.ignore_truncated)
        args.ignore = (known.ignore_measure or "iof", 0.5 if known.ignore_thresh is None else known.ignore_thresh)
    return args


def ignore_description(args):
    """The ignore regions as the start-up line prints them."""
    p, ig = getattr(args, "ignore_policy", None), getattr(args, "ignore", None)
    if p is None:
        return "ignore regions off (every anchor outside the IoU band, the padding and the border is a negative)"
    who = [text for on, text in ((p.invalid, "faces flagged invalid"), (p.blur, f"faces with blur >= {p.blur}"),
                                 (p.occlusion, f"faces with occlusion >= {p.occlusion}"),
                                 (p.min_size, f"faces whose shorter side is below {p.min_size:g} px after the scale draw" if p.min_size else ""),
                                 (p.truncated, "what is left of the faces the crop drops")) if on]
    measure = "intersection over the anchor's area" if ig[0] == "iof" else "IoU"
    return (f"ignore regions: {'; '.join(who)} own no positive anchor, and a negative anchor they cover by {measure} >= {ig[1]:g} "
            "gets the don't-care label (on the device; positives and the regression targets do not change)")


def assigner_description(args):
    """The target assigner as the start-up line prints it."""
    if getattr(args, "assigner", "dense_overlap") == "tal" and getattr(args, "tal_aligned_targets", False):
        return (f"assigner TAL: every step, from the network's own output: per face the anchors whose centre lies inside it are ranked by "
                f"m = sigmoid(logit)^{args.tal_alpha:g} * IoU(predicted box, face)^{args.tal_beta:g} and the best {args.tal_topk} become its positives, an "
                "anchor two faces claim goes to the larger IoU, and every positive keeps its aligned target m / max m * max IoU over the anchors its face "
                "won; everything else keeps the label of a map without faces (on the device, between the forward pass and the loss; the two IoU "
                "thresholds only filter crops)")
    if getattr(args, "assigner", "dense_overlap") == "tal":
        return (f"assigner TAL: every step, from the network's own output: per face the anchors whose centre lies inside it are ranked by "
                f"sigmoid(logit)^{args.tal_alpha:g} * IoU(predicted box, face)^{args.tal_beta:g} and the best {args.tal_topk} become its positives, an anchor "
                "two faces claim goes to the larger IoU; everything else keeps the label of a map without faces (on the device, between the forward "
                "pass and the loss; the two IoU thresholds only filter crops)")
    if getattr(args, "assigner", "dense_overlap") != "atss":
        return ("assigner dense-overlap: positives from the data set's positive IoU threshold plus every face's best anchor, negatives below its negative "
                "threshold, the band between them ignored (0.7 / 0.3 for WIDER and the synthetic crops; synthetic-faces: 0.7 / 0.7 unless FACES_POS / FACES_NEG say otherwise)")
    return (f"assigner ATSS: per face the {args.atss_topk} nearest unpadded cells of every template are candidates, positive from the mean plus the "
            "standard deviation of their IoUs when the anchor centre lies inside the face, the best candidate otherwise; everything else is a "
            "negative (on the device; the two IoU thresholds only filter crops)")


def compensation_description(args):
    """The anchor matching as the start-up line prints it."""
    ac = getattr(args, "anchor_compensation", None)
    if ac is None:
        return "anchor compensation off (positives from IoU 0.7 plus every face's best anchor)"
    return (f"anchor compensation: every face topped up to {ac[0]} positive anchors from its own unpadded anchors of IoU >= {ac[1]:g}, best first "
            "(on the device; the regression targets do not change)")


def jitter_description(args):
    """The colour jitter as the start-up line prints it."""
    cj = getattr(args, "color_jitter", None)
    if cj is None:
        return "colour jitter off"
    return f"colour jitter brightness {cj[0]:g}, contrast {cj[1]:g}, saturation {cj[2]:g}, hue {cj[3]:g} (on the device, in front of ToTensor)"


def loss_description(args):
    """The criterion's two losses as the start-up line prints them."""
    reg_loss, reg_weight = getattr(args, "reg_loss", "smooth_l1"), getattr(args, "reg_weight", 1.0)
    reg = {"smooth_l1": "SmoothL1 on the four offsets", "iou": "IoU, one term per positive", "giou": "GIoU, one term per positive",
           "diou": "DIoU, one term per positive"}[reg_loss]
    reg = f"; regression loss {reg}, weight {reg_weight:g}"
    if args.cls_loss == "qfl" and getattr(args, "tal_aligned_targets", False):
        norm = {"pos": "per image by its positives", "align": "per image by the sum of its aligned targets"}.get(args.focal_normalize, "not normalised")
        return (f"classification loss task-aligned quality focal (beta {getattr(args, 'qfl_beta', 2.0):g}, the assigner's aligned target of the positive as "
                f"the target; {norm}; every labelled anchor, every positive regresses, weighted by its aligned target)") + reg
    if args.cls_loss == "qfl":
        norm = "per image by its positives" if args.focal_normalize == "pos" else "not normalised"
        return (f"classification loss quality focal (beta {getattr(args, 'qfl_beta', 2.0):g}, IoU of the predicted box as the target; {norm}; every labelled "
                "anchor, every positive regresses)") + reg
    if args.cls_loss != "focal":
        return f"classification loss soft-margin (OHEM threshold {args.ohem_thresh:g}, 128 + 128 samples per image)" + reg
    alpha = f"alpha {args.focal_alpha:g}" if args.focal_alpha >= 0 else "no alpha weighting"
    norm = "per image by its positives" if args.focal_normalize == "pos" else "not normalised"
    return f"classification loss focal (gamma {args.focal_gamma:g}, {alpha}, {norm}; every labelled anchor, every positive regresses)" + reg


def lr_at(base_lr, epoch):
    return base_lr * 0.1 ** (epoch // LR_STEP)


def steps_per_epoch(n_batches, accum_steps=1):
    """Optimizer steps of one epoch: the last window of an epoch is applied full or not."""
    return -(-int(n_batches) // int(accum_steps))


def lr_with_warmup(base_lr, epoch, step, warmup_iters=0, warmup_factor=1e-3):
    """lr_at(base_lr, epoch) * (F + (1 - F) * min(T, N) / N) for the global optimizer-step index T = `step` (epoch * steps_per_epoch + s):
    StepLR's closed form times LinearLR's (trainer.warmup_factor), so a resumed run lands on the same value.  N = 0: lr_at alone."""
    return lr_at(base_lr, epoch) * trainer.warmup_factor(step, warmup_iters, warmup_factor)


def run_fused_epoch(engine, loss_fn, loader, epoch, device, base_lr, warmup=None):
    """warmup = (N, F): engine.set_lr(lr_with_warmup(...)) once per optimizer step while the warm-up lasts; None / N = 0: once per epoch."""
    engine.set_lr(lr_at(base_lr, epoch))
    total = len(loader)
    warm = warmup is not None and int(warmup[0]) > 0
    first = epoch * steps_per_epoch(total, engine.accum_steps)
    steps0 = engine.steps
    for idx, batch in enumerate(loader):
        if warm:
            engine.set_lr(lr_with_warmup(base_lr, epoch, first + (engine.steps - steps0), warmup[0], warmup[1]))
        # the epoch's last batch ends its window, full or not: no checkpoint is ever written with gradients accumulated and not applied
        # (a loader with --assigner tal delivers a fourth element, the resident faces of the batch: a record that is moved, not a tensor to convert)
        maps = tuple(t.float().to(device, non_blocking=True) for t in batch[:3])
        if len(batch) > 3:
            engine.step_with_faces(*maps, batch[3].to(device, non_blocking=True), apply=True if idx + 1 == total else None)
        else:
            engine.step(*maps, apply=True if idx + 1 == total else None)
        if parallel.rank() == 0:
            loss_fn.flush_meters(lag=0 if idx + 1 == total else 1)      # one step behind: the host prepares batch idx + 1 while the GPU runs step idx
            trainer.print_state(idx, epoch, total, loss_fn.class_average.average, loss_fn.reg_average.average)
            trainer.print_quality(idx, epoch, total, loss_fn)                                            # (nothing unless --cls-loss qfl)
            trainer.print_compensation(idx, epoch, total, loader, lag=0 if idx + 1 == total else 1)      # (nothing unless --anchor-compensation)
            trainer.print_ignore(idx, epoch, total, loader, lag=0 if idx + 1 == total else 1)            # (nothing unless an --ignore-* policy)


def load_pretrained_trunk(model, path):
    """The reference's default `pretrained_weights=ResNet101_Weights.IMAGENET1K_V1` (model.py:13-14,20) from a local file:
    a torchvision resnet101 state_dict (keys `conv1.weight`, `layer1.0...`, `fc.*`; `layer4.*` is dropped like model.py:23)
    or a checkpoint of this package / the reference (`{"model": {...}}` with `model.`-prefixed keys); the same for resnet50 / resnet152
    when the model has that trunk (--base-model), and another trunk's file is refused."""
    sd = torch.load(path, map_location="cpu", weights_only=True)      # a state_dict of tensors: nothing else is unpickled
    sd = sd.get("model", sd)
    try:
        model.check_trunk_of(sd, f"--pretrained {path}")
    except ValueError as e:
        raise SystemExit(str(e))
    if any(k.startswith("model.") for k in sd):
        missing, unexpected = model.load_state_dict(sd, strict=False)
    else:
        sd = {k: v for k, v in sd.items() if not k.startswith("layer4.")}
        missing, unexpected = model.model.load_state_dict(sd, strict=False)
    if unexpected:
        raise SystemExit(f"--pretrained {path}: unexpected keys {list(unexpected)[:5]} ... (not a {model.trunk_name} state_dict?)")
    return missing


def main():
    args = trunk_arguments()
    if not torch.cuda.is_available():
        raise SystemExit("this build of the tiny-faces hot path runs on MI355X only (no CPU fallback)")
    if args.ignore_policy is not None and (str(args.traindata) in ("synthetic", "synthetic-faces") or getattr(args, "synthetic", False)):
        raise SystemExit("the --ignore-* flags apply to a WIDER annotation file: the synthetic data sets carry no attributes and no crop")
    parallel.init_from_env(os.environ.get("TINYFACES_DIST_BACKEND"))      # (gloo: several ranks on one device, the functional tests of a 1-GPU box)
    device = torch.device("cuda", torch.cuda.current_device())
    preprocess = transforms.Compose([transforms.ToTensor(), transforms.Normalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225])])
    train_loader, _ = get_dataloader(args.traindata, args, NUM_TEMPLATES, img_transforms=preprocess, color_jitter=args.color_jitter,
                                     anchor_compensation=args.anchor_compensation,
                                     **({} if args.assigner == "dense_overlap" else {"assigner": args.assigner, "atss_topk": args.atss_topk}),
                                     **({"tal_topk": args.tal_topk, "tal_alpha": args.tal_alpha, "tal_beta": args.tal_beta} if args.assigner == "tal" else {}),
                                     **({} if args.ignore_policy is None else {"ignore_policy": args.ignore_policy, "ignore": args.ignore}))
    model = DetectionModel(base_model=getattr(model_zoo, args.base_model), num_objects=1, num_templates=NUM_TEMPLATES).set_compute_dtype(args.dtype)
    model.freeze_batchnorm(args.freeze_bn).set_trainable_layers(args.trainable_layers)
    if parallel.rank() == 0:
        print(f"trunk {args.base_model}, {args.dtype}, BatchNorm {'frozen' if args.freeze_bn else 'on batch statistics'}, trainable layers "
              f"{args.trainable_layers} of 4 ({len(model.trainable_parameter_names())} trained tensors)")
        print(f"effective batch {args.batch_size * args.accum_steps * parallel.world_size()} = batch_size {args.batch_size} x accum-steps "
              f"{args.accum_steps} x world {parallel.world_size()}" + (", gradients averaged over the window" if args.accum_average and args.accum_steps > 1 else ""))
    loss_fn = DetectionCriterion(NUM_TEMPLATES, reg_weight=args.reg_weight, seed=args.seed * parallel.world_size() + parallel.rank(), lazy_meters=True,
                                 cls_loss=args.cls_loss, focal_gamma=args.focal_gamma, focal_alpha=args.focal_alpha, focal_normalize=args.focal_normalize,
                                 reg_loss=args.reg_loss, templates=load_templates(NUM_TEMPLATES) if args.reg_loss == "diou" or args.assigner == "tal" else None,
                                 **({"qfl_beta": args.qfl_beta} if args.cls_loss == "qfl" else {}),
                                 **({"assigner": TaskAligned(args.tal_topk, args.tal_alpha, args.tal_beta, **({"aligned_targets": True} if args.tal_aligned_targets else {}))}
                                    if args.assigner == "tal" else {}))
    loss_fn.ohem_thresh = args.ohem_thresh
    if parallel.rank() == 0:
        print(loss_description(args))
        print(jitter_description(args))
        print(assigner_description(args))
        print(compensation_description(args))
        print(ignore_description(args))
        if args.deterministic:
            print(deterministic_description())
        if args.cls_loss in ("focal", "qfl"):
            print(f"--ohem-thresh is unused with --cls-loss {args.cls_loss}: nothing is mined or sampled")

    first_epoch = args.start_epoch
    state = None
    if args.resume:                                              # main.py:73-79 (there `--resume` is a flag used as a path: defect D3)
        state = torch.load(args.resume, map_location="cpu")
        model.load_state_dict(state["model"])
        first_epoch = first_epoch or state["epoch"]
    elif args.pretrained:
        load_pretrained_trunk(model, args.pretrained)
    else:
        if args.init == "tame":
            tame_init_(model)
        if parallel.rank() == 0:
            print(f"WARNING: training starts from RANDOM ({args.init}) weights. The reference starts from ImageNet ResNet-101 "
                  "(model.py:13-14); its lr / schedule will not reproduce its results from scratch. Pass --pretrained <resnet101.pth>.")

    engine = optimizer = scheduler = ema = None
    if args.fused:
        engine = TrainEngine(model, loss_fn, lr=args.lr, momentum=args.momentum, weight_decay=args.weight_decay, device=device,
                             max_grad_norm=args.clip_grad_norm, skip_nonfinite=args.skip_nonfinite, ema_decay=args.model_ema,
                             accum_steps=args.accum_steps, accum_average=args.accum_average, optimizer=args.optimizer,
                             betas=(args.adam_beta1, args.adam_beta2), eps=args.adam_eps, deterministic=args.deterministic)
        ema = engine.ema                  # (built from the weights --resume / --pretrained left in the model)
        if state is not None:
            engine.load_optimizer_state_dict(state.get("optimizer"))      # momentum buffers / moments (a torch.optim.SGD / AdamW state_dict)
    else:
        model = model.to(device)          # before load_state_dict: torch casts the momentum buffers to the device the parameters are on THEN
        if args.optimizer == "adamw":
            optimizer = optim.AdamW(model.learnable_parameters(args.lr), lr=args.lr, betas=(args.adam_beta1, args.adam_beta2), eps=args.adam_eps,
                                    weight_decay=args.weight_decay)
        else:
            optimizer = optim.SGD(model.learnable_parameters(args.lr), lr=args.lr, momentum=args.momentum, weight_decay=args.weight_decay)
        if state is not None and state.get("optimizer", {}).get("param_groups"):
            theirs = "adamw" if "betas" in state["optimizer"]["param_groups"][0] else "sgd"
            if theirs == args.optimizer:
                optimizer.load_state_dict(state["optimizer"])             # main.py:76
            elif parallel.rank() == 0:
                print(f"WARNING: {args.resume} holds the state of optimizer {theirs}, this run uses {args.optimizer}: "
                      f"the moments of {args.optimizer} start from zero")
        for mult, g in zip((1.0, 0.1, 1.0, 0.0), optimizer.param_groups):
            g.setdefault("initial_lr", args.lr * mult)                    # StepLR(last_epoch >= 0) requires it (main.py:81-83)
        scheduler = optim.lr_scheduler.StepLR(optimizer, step_size=LR_STEP, last_epoch=first_epoch - 1)
        # StepLR's constructor takes one step() from the lr it finds in the groups: a checkpoint saved at a multiple of LR_STEP epochs
        # already carries the decayed lr and would be decayed AGAIN (the reference has this quirk, main.py:76-83).  Here the fused and
        # the autograd path must train a resumed run at the SAME lr: put every group on the closed form the fused engine uses.
        # Deliberate divergence from the reference on resume (documented in INTEGRATION.md): the lr stored in the checkpoint's optimizer
        # state is REPLACED by the closed form of --lr, so a checkpoint trained with a different --lr continues at the new one -- say so.
        for mult, g in zip((1.0, 0.1, 1.0, 0.0), optimizer.param_groups):
            want = lr_at(args.lr, first_epoch) * mult
            if state is not None and abs(g["lr"] - want) > 1e-12 * max(1.0, abs(want)) and abs(g["lr"] - want * 0.1) > 1e-12 and parallel.rank() == 0:
                print(f"WARNING: resumed optimizer group has lr {g['lr']:.3g}; continuing at {want:.3g} (closed form of --lr {args.lr:g} at epoch {first_epoch})")
            g["lr"] = want
        scheduler._last_lr = [g["lr"] for g in optimizer.param_groups]       # what get_last_lr() reports must be what the groups hold
        if args.model_ema is not None:
            ema = ModelEma(model, args.model_ema)      # flattens the model; the optimizer's nn.Parameters keep their identity
    if ema is not None and state is not None:
        if "model_ema" in state and "ema" in state:
            ema.load_state_dict(state["model_ema"], state["ema"]["updates"])
            ema.warmup = bool(state["ema"].get("warmup", ema.warmup))
            stored = state["ema"].get("decay")
            if stored is not None and stored != ema.decay and parallel.rank() == 0:
                print(f"WARNING: {args.resume} was averaged with decay {stored:g}; continuing with --model-ema {ema.decay:g}")
        elif parallel.rank() == 0:
            print(f"WARNING: {args.resume} holds no model EMA; the average starts at the loaded weights")
    elif ema is None and state is not None and "model_ema" in state and parallel.rank() == 0:
        print(f"WARNING: {args.resume} holds a model EMA, which this run drops: pass --model-ema DECAY to continue it")

    validator, val_ap, best_ap = None, None, None
    if args.val_every > 0 and parallel.rank() == 0:              # off (the default): nothing below is imported, allocated or launched
        from tinyfaces.validation import Validator
        validator = Validator(args.valdata, NUM_TEMPLATES, device, preprocess, prob_thresh=args.val_prob_thresh, nms_thresh=args.val_nms_thresh,
                              num_images=args.val_num_images, gt_dir=args.val_gt_dir, dataset_root=args.dataset_root, seed=args.seed)
        if state is not None and isinstance(state.get("val_ap"), dict) and validator.settings[0] in state["val_ap"]:
            best_ap = float(state["val_ap"][validator.settings[0]])      # (a resumed run does not overwrite a better checkpoint_best.pth with a worse one)

    def snapshot_of(done):
        if engine is not None:
            engine.set_lr(lr_at(args.lr, done))                       # what StepLR would have left in the param groups
        snapshot = {"epoch": done, "batch_size": train_loader.batch_size, "model": model.state_dict(),          # main.py:97-102
                    "optimizer": optimizer.state_dict() if optimizer is not None else engine.optimizer_state_dict(base_lr=args.lr)}
        if ema is not None:
            snapshot["model_ema"], snapshot["ema"] = ema.state_dict(), ema.settings()
        if args.anchor_compensation is not None:
            snapshot["args"] = {"anchor_compensation": list(args.anchor_compensation)}      # what the targets of this run were matched with
        if args.assigner == "atss":
            snapshot.setdefault("args", {}).update(assigner=args.assigner, atss_topk=args.atss_topk)
        if args.assigner == "tal":
            snapshot.setdefault("args", {}).update(assigner=args.assigner, tal_topk=args.tal_topk, tal_alpha=args.tal_alpha, tal_beta=args.tal_beta)
            if args.tal_aligned_targets:
                snapshot["args"].update(tal_aligned_targets=True)
        if args.cls_loss == "qfl":
            snapshot.setdefault("args", {}).update(cls_loss=args.cls_loss, qfl_beta=args.qfl_beta, focal_normalize=args.focal_normalize,
                                                   reg_loss=args.reg_loss, reg_weight=args.reg_weight)
        if args.ignore_policy is not None:
            snapshot.setdefault("args", {}).update(ignore_policy=dict(args.ignore_policy._asdict()), ignore=list(args.ignore))
        if val_ap is not None:
            snapshot["val_ap"] = dict(val_ap)                         # of the last validation pass at or before this epoch
        return snapshot

    skipped = 0
    for epoch in range(first_epoch, args.epochs):
        if hasattr(train_loader, "set_epoch"):
            train_loader.set_epoch(epoch)                                 # reshuffle the rank shards
        elif hasattr(getattr(train_loader, "sampler", None), "set_epoch"):
            train_loader.sampler.set_epoch(epoch)
        if engine is not None:
            run_fused_epoch(engine, loss_fn, train_loader, epoch, device, args.lr, warmup=(args.warmup_iters, args.warmup_factor))
        else:
            trainer.train(model, loss_fn, optimizer, train_loader, epoch, device=device, max_grad_norm=args.clip_grad_norm,
                          skip_nonfinite=args.skip_nonfinite, ema=ema, accum_steps=args.accum_steps, accum_average=args.accum_average,
                          warmup=(args.warmup_iters, args.warmup_factor, epoch * steps_per_epoch(len(train_loader), args.accum_steps)),
                          deterministic=args.deterministic)
            scheduler.step()
        if args.skip_nonfinite and parallel.rank() == 0:
            total = engine.skipped_steps if engine is not None else ops.clip_skipped_steps(device)
            if total != skipped:
                print(f"Epoch: [{epoch}]\t{total - skipped} step(s) skipped: the gradient norm was not finite ({total} since the start)")
                skipped = total
        done = epoch + 1
        if args.val_every > 0 and done % args.val_every == 0:
            if validator is not None:                                     # rank 0; the weights are copied into the validator's own model
                val_ap = validator.run(ema.state_dict() if ema is not None else model.state_dict())
                print(f"Val: [{epoch}] AP " + ", ".join(f"{s} {v!r}" for s, v in val_ap.items()) + (" (model EMA)" if ema is not None else ""))
                first = val_ap[validator.settings[0]]
                if best_ap is None or first > best_ap:
                    best_ap = first
                    trainer.save_checkpoint(snapshot_of(done), filename="checkpoint_best.pth", save_path=Path(args.save_path))
            if parallel.is_distributed():
                torch.distributed.barrier()                               # the other ranks wait for rank 0's pass
        if done % args.save_every == 0 and parallel.rank() == 0:
            trainer.save_checkpoint(snapshot_of(done), filename=f"checkpoint_{done}.pth", save_path=Path(args.save_path))


if __name__ == "__main__":
    main()
