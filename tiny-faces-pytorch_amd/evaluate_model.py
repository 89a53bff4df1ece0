"""Evaluation entry point with the reference's flags (evaluate_model.py:17-31) on the MI355X hot path.
`dataset` = a WIDER val/test annotation file (+ --dataset-root), as in the reference's `make evaluate`, or `synthetic` for seeded
random images (no WIDER files needed); results are written in the WIDER submission format by write_results exactly like
evaluate_model.py:47-68.  The pyramid levels are built on the GPU."""
import argparse
import os

import torch

from types import SimpleNamespace

from tinyfaces import parallel, transforms
from tinyfaces.datasets import get_dataloader
from tinyfaces.evaluation import get_detections, get_model, write_results


# the reference's command line (evaluate_model.py:17-31) + one addition for the synthetic data set
FLAGS = [
    ("dataset", {}), ("--split", dict(default="val")), ("--dataset-root", {}),
    ("--checkpoint", dict(default="", help="The path to the model checkpoint")),
    ("--prob_thresh", dict(type=float, default=0.03)), ("--nms_thresh", dict(type=float, default=0.3)),
    ("--workers", dict(default=8, type=int)), ("--batch_size", dict(default=1, type=int)),
    ("--results_dir", dict(default=None)), ("--debug", dict(action="store_true")),
    ("--num-images", dict(default=4, type=int, help="synthetic dataset only")),
    ("--mask-axis", dict(dest="mask_axis", default="w", choices=["w", "template"],
                         help="`w` (default) = the reference's template mask as written (it indexes the heat-map WIDTH: defect D1, tinyfaces/models/utils.py:44); "
                              "`template` = the mask on the template axis it was meant for")),
]


def arguments(argv=None):
    parser = argparse.ArgumentParser("Model Evaluator", epilog=EMA_HELP)
    for name, kw in FLAGS:
        parser.add_argument(name, **kw)
    return parser.parse_args(argv)


EMA_HELP = "--ema: evaluate the averaged weights of a `main.py --model-ema` run (the checkpoint's \"model_ema\") instead of the last iterate"


def ema_arguments(argv=None):
    """`arguments` plus `ema` from --ema.  Parsed apart, so that `arguments` keeps resolving exactly the reference's options and the additions above."""
    parser = argparse.ArgumentParser(add_help=False)
    parser.add_argument("--ema", action="store_true", help=EMA_HELP)
    known, rest = parser.parse_known_args(argv)
    args = arguments(rest)
    args.ema = known.ema
    return args


TTA_HELP = ("--flip: run every pyramid level mirrored left-right as well and suppress the union of both candidate lists; "
            "--box-voting T: replace every NMS survivor by the score-weighted mean of all candidates with IoU >= T (0 < T <= 1)")


def _vote_thresh(text):
    t = float(text)
    if not 0.0 < t <= 1.0:
        raise argparse.ArgumentTypeError(f"--box-voting {text}: the IoU threshold of the vote lies in (0, 1]")
    return t


def tta_arguments(argv=None):
    """`ema_arguments` plus `flip` / `box_voting` from --flip / --box-voting T (test-time augmentation), parsed apart in the same way."""
    parser = argparse.ArgumentParser(add_help=False)
    parser.add_argument("--flip", action="store_true", help=TTA_HELP)
    parser.add_argument("--box-voting", dest="box_voting", type=_vote_thresh, default=None, metavar="T", help=TTA_HELP)
    known, rest = parser.parse_known_args(argv)
    args = ema_arguments(rest)
    args.flip, args.box_voting = known.flip, known.box_voting
    return args


SOFT_NMS_HELP = ("--soft-nms {linear,gaussian}: Soft-NMS instead of the hard NMS -- an overlapped candidate is decayed (linear: by 1 - IoU above "
                 "--nms_thresh; gaussian: by exp(-IoU^2 / S) with --soft-nms-sigma S) and kept while its score stays >= --soft-nms-score-thresh T; "
                 "the scores written are the decayed probabilities")


def _positive(text):
    v = float(text)
    if not v > 0.0:
        raise argparse.ArgumentTypeError(f"--soft-nms-sigma {text}: the gaussian decay needs sigma > 0")
    return v


def _non_negative(text):
    v = float(text)
    if not v >= 0.0:
        raise argparse.ArgumentTypeError(f"--soft-nms-score-thresh {text}: the score threshold is >= 0")
    return v


def soft_nms_arguments(argv=None):
    """`tta_arguments` plus `soft_nms` / `soft_nms_sigma` / `soft_nms_score_thresh` from --soft-nms / --soft-nms-sigma / --soft-nms-score-thresh,
    parsed apart in the same way."""
    parser = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    parser.add_argument("--soft-nms", dest="soft_nms", choices=["linear", "gaussian"], default=None, help=SOFT_NMS_HELP)
    parser.add_argument("--soft-nms-sigma", dest="soft_nms_sigma", type=_positive, default=0.5, metavar="S", help=SOFT_NMS_HELP)
    parser.add_argument("--soft-nms-score-thresh", dest="soft_nms_score_thresh", type=_non_negative, default=0.001, metavar="T", help=SOFT_NMS_HELP)
    known, rest = parser.parse_known_args(argv)
    args = tta_arguments(rest)
    args.soft_nms, args.soft_nms_sigma, args.soft_nms_score_thresh = known.soft_nms, known.soft_nms_sigma, known.soft_nms_score_thresh
    return args


LIMITS_HELP = ("--pre-nms-topk K: when more than K candidates pass --prob_thresh, only the K best reach the NMS / Soft-NMS / vote (the `top_k` of "
               "S3FD / RetinaFace, e.g. 5000); --max-detections M: at most M detections per image are written (`keep_top_k`, e.g. 750)")


def _count(flag):
    def parse(text):
        try:
            v = int(text)
        except ValueError:
            v = 0
        if v < 1:
            raise argparse.ArgumentTypeError(f"{flag} {text}: a positive integer")
        return v
    return parse


AP_HELP = ("--ap: after the run, print the average precision of the detections (`AP <setting> = ...`), matched and accumulated on the device "
           "(wider_eval.DeviceEvaluator, fed image by image; the result files are written as before); synthetic-faces: against the pasted boxes, "
           "one setting `all`; a WIDER annotation file: --gt-dir DIR with the eval_tools ground truth (wider_face_val.mat, wider_{easy,medium,hard}_val.mat), "
           "settings easy / medium / hard.  One rank only")


def limits_arguments(argv=None):
    """`soft_nms_arguments` plus `pre_nms_topk` / `max_detections` from --pre-nms-topk K / --max-detections M and `ap` / `gt_dir` from
    --ap / --gt-dir DIR, parsed apart in the same way."""
    parser = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    parser.add_argument("--pre-nms-topk", dest="pre_nms_topk", type=_count("--pre-nms-topk"), default=None, metavar="K", help=LIMITS_HELP)
    parser.add_argument("--max-detections", dest="max_detections", type=_count("--max-detections"), default=None, metavar="M", help=LIMITS_HELP)
    parser.add_argument("--ap", dest="ap", action="store_true", help=AP_HELP)
    parser.add_argument("--gt-dir", dest="gt_dir", default=None, metavar="DIR", help=AP_HELP)
    known, rest = parser.parse_known_args(argv)
    args = soft_nms_arguments(rest)
    args.pre_nms_topk, args.max_detections = known.pre_nms_topk, known.max_detections
    args.ap, args.gt_dir = known.ap, known.gt_dir
    return args


MATRIX_NMS_HELP = ("--soft-nms {matrix-linear,matrix-gaussian}: Matrix NMS -- Soft-NMS's decay in closed form, with no serial selection (linear: "
                   "min (1 - IoU) / (1 - comp); gaussian: exp(-(IoU^2 - comp^2) / S) with --soft-nms-sigma S, comp being the better candidate's own "
                   "largest overlap); --soft-nms-score-thresh as for Soft-NMS; --nms_thresh is not used")


def matrix_nms_arguments(argv=None):
    """`limits_arguments` with --soft-nms also taking matrix-linear / matrix-gaussian (`soft_nms` = "matrix_linear" / "matrix_gaussian", the
    values get_detections takes), parsed apart in the same way: the flag is resolved here and the older parsers, whose choices stay as they
    are, see the rest."""
    parser = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    parser.add_argument("--soft-nms", dest="soft_nms", choices=["linear", "gaussian", "matrix-linear", "matrix-gaussian"], default=None,
                        help=MATRIX_NMS_HELP)
    known, rest = parser.parse_known_args(argv)
    args = limits_arguments(rest)
    args.soft_nms = None if known.soft_nms is None else known.soft_nms.replace("-", "_")
    return args


def check_ap(args):
    """--ap is refused, before anything is loaded, where it cannot be answered: under several ranks (every rank sees a shard of the images; the
    table is not reduced across ranks) and for a WIDER annotation file without --gt-dir."""
    if not getattr(args, "ap", False):
        return
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        raise SystemExit(f"--ap runs on one rank only (WORLD_SIZE={world}): every rank evaluates a shard of the images and the precision / recall "
                         "table is not reduced across ranks; run `python evaluate_model.py ... --ap` without torchrun, or evaluate the result "
                         "files afterwards with `python -m tinyfaces.wider_eval`")
    if args.dataset != "synthetic-faces" and not args.gt_dir:
        raise SystemExit(f"--ap on {args.dataset} needs --gt-dir DIR, the eval_tools ground-truth directory (only synthetic-faces carries its own boxes)")


def ap_ground_truth(args, dataset):
    """(settings, gt_boxes {event: {image: (G,4)}}, keep_lists per setting {event: {image: indices}}) for --ap."""
    import numpy as np
    from tinyfaces import wider_eval
    if args.dataset == "synthetic-faces":
        gt = {"faces": dataset.ground_truth()}
        return ("all",), gt, [{"faces": {k: np.arange(v.shape[0]) for k, v in gt["faces"].items()}}]
    settings = ("easy", "medium", "hard")
    loaded = [wider_eval.load_ground_truth(args.gt_dir, s) for s in settings]
    return settings, loaded[0][0], [keep for _, keep in loaded]


def feed_evaluator(evaluator, dets, img_path, gt_boxes, keep_lists):
    """One image's detections (x1 y1 x2 y2 score, as write_results takes them) into a DeviceEvaluator, under the name its result file gets."""
    import numpy as np
    from tinyfaces import ops
    event, name = os.path.split(img_path.replace("jpg", "txt"))
    name = name[:-4] if name.endswith(".txt") else name
    gt = gt_boxes.get(event, {}).get(name)
    if gt is None:                                              # not in the ground truth: evaluate_setting never visits it, norm_scores does
        gt = np.zeros((0, 4))
    keeps = [[k.get(event, {}).get(name, [])] for k in keep_lists]
    evaluator.add([ops.wider_rows(dets)], [gt], keeps)
    return event, name


def run_ap(model, val_loader, templates, prob_thresh, nms_thresh, device, split, evaluator, gt_boxes, keep_lists, results_dir=None, debug=False,
           **detection_keywords):
    """`run` with every image's detections fed to `evaluator` as well: the same calls in the same order, the same result files."""
    import numpy as np
    dets, seen, done = None, set(), set()
    for _, (img, filename) in enumerate(val_loader):
        dets = get_detections(model, img[0], templates, val_loader.dataset.rf, val_loader.dataset.transforms, prob_thresh, nms_thresh,
                              device=device, pyramid_on_gpu=True, **detection_keywords)
        write_results(dets, filename[0], split, results_dir)
        if filename[0] not in seen:                             # (a data set longer than its images walks them again: one result file per name)
            seen.add(filename[0])
            done.add(feed_evaluator(evaluator, dets, filename[0], gt_boxes, keep_lists))
        if debug:
            print(f"{filename[0]}: {dets.shape[0]} detections")
    # evaluate_setting walks the GROUND TRUTH: an image that was not run still counts its boxes in the recall
    for event, images in gt_boxes.items():
        for name, gt in images.items():
            if (event, name) not in done:
                evaluator.add([np.zeros((0, 5))], [gt], [[k.get(event, {}).get(name, [])] for k in keep_lists])
    return dets


def dataloader(args):
    """evaluate_model.py:34-45."""
    tf = transforms.Compose([transforms.ToTensor(), transforms.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])])
    largs = SimpleNamespace(batch_size=args.batch_size, workers=args.workers, dataset_root=args.dataset_root or "", debug=args.debug,
                            synthetic_len=args.num_images)
    return get_dataloader(args.dataset, largs, train=False, split=args.split, img_transforms=tf)


def run(model, val_loader, templates, prob_thresh, nms_thresh, device, split, results_dir=None, debug=False, mask_axis="w",
        pre_nms_topk=None, max_detections=None,
        flip=False, box_voting=None, soft_nms=None, soft_nms_sigma=0.5, soft_nms_score_thresh=0.001):
    """evaluate_model.py:48-68, statement for statement: `img[0]` / `filename[0]` undo the batch axis the loader adds.  The
    only addition is the keyword that builds the pyramid levels on the GPU (same detections bit for bit).
    flip / box_voting: get_detections' test-time augmentation, off by default.  soft_nms / soft_nms_sigma / soft_nms_score_thresh:
    get_detections' Soft-NMS, off by default.  pre_nms_topk / max_detections: get_detections' bounds on the candidates that reach the
    suppression step and on the rows that come back, off by default."""
    dets = None
    for _, (img, filename) in enumerate(val_loader):
        dets = get_detections(model, img[0], templates, val_loader.dataset.rf, val_loader.dataset.transforms, prob_thresh, nms_thresh,
                              device=device, pyramid_on_gpu=True, mask_axis=mask_axis, flip=flip, box_voting=box_voting,
                              soft_nms=soft_nms, soft_nms_sigma=soft_nms_sigma, soft_nms_score_thresh=soft_nms_score_thresh,
                              pre_nms_topk=pre_nms_topk, max_detections=max_detections)
        write_results(dets, filename[0], split, results_dir)
        if debug:
            print(f"{filename[0]}: {dets.shape[0]} detections")
    return dets


def main():
    args = matrix_nms_arguments()
    check_ap(args)
    if not torch.cuda.is_available():
        raise SystemExit("this build of the tiny-faces hot path runs on MI355X only (no CPU fallback)")
    # Multi-GPU evaluation = replicas only: under torchrun every rank takes a strided shard of the image list
    # (datasets.get_dataloader) and writes the result files of ITS images into the shared results tree; no collective on the
    # data path, one barrier at the end.  A plain `python evaluate_model.py` is rank 0 of a world of 1, exactly the reference's loop
    # (evaluate_model.py:56-68).  TINYFACES_DIST_BACKEND=gloo + TINYFACES_SHARE_GPU=1: several ranks on one device (functional tests).
    distributed = parallel.init_from_env(os.environ.get("TINYFACES_DIST_BACKEND"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    share = os.environ.get("TINYFACES_SHARE_GPU") == "1"
    device = torch.device(f"cuda:{local % torch.cuda.device_count() if share else local}")
    torch.cuda.set_device(device)
    val_loader, templates = dataloader(args)
    model = get_model(args.checkpoint, num_templates=templates.shape[0], ema=args.ema)
    model = model.to(device).eval()
    evaluator = None
    if args.ap:
        from tinyfaces.wider_eval import DeviceEvaluator
        settings, gt_boxes, keep_lists = ap_ground_truth(args, val_loader.dataset)
        evaluator = DeviceEvaluator(settings, device=device)
    with torch.no_grad(), model.constant_weights():          # the checkpoint does not change between images: pack the weights once
        keywords = dict(mask_axis=args.mask_axis, flip=args.flip, box_voting=args.box_voting,
                        soft_nms=args.soft_nms, soft_nms_sigma=args.soft_nms_sigma, soft_nms_score_thresh=args.soft_nms_score_thresh,
                        pre_nms_topk=args.pre_nms_topk, max_detections=args.max_detections)
        debug = args.debug or args.dataset == "synthetic"
        if evaluator is None:
            run(model, val_loader, templates, args.prob_thresh, args.nms_thresh, device, args.split, results_dir=args.results_dir, debug=debug, **keywords)
        else:
            run_ap(model, val_loader, templates, args.prob_thresh, args.nms_thresh, device, args.split, evaluator, gt_boxes, keep_lists,
                   results_dir=args.results_dir, debug=debug, **keywords)
            for setting, (ap, _) in evaluator.finish().items():
                print(f"AP {setting} = {ap!r}")              # repr: every digit, so that the line can be compared with the host evaluator's float
    if distributed:
        torch.distributed.barrier()
        if parallel.rank() == 0:
            print(f"evaluated on {parallel.world_size()} ranks")
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
