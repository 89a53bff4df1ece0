"""Validation AP inside a training run (`main.py --val-every N`): the detector over the validation images, the detections matched and
accumulated on the device (wider_eval.DeviceEvaluator), no result file.  Imported only when validation is on.

The training model is not touched.  The weights under test (the EMA's or the live ones) are COPIED into a second DetectionModel that only
ever runs in eval mode: the training model keeps its mode, its workspace, its packed operands and its BatchNorm buffers, so a run with
validation ends on the very bits of a run without it (tests/test_gpu_wider_eval.py).  The detector is evaluate_model.py's: the same
pyramid, thresholds of its own (--val-prob-thresh / --val-nms-thresh), the template mask on the template axis."""
from types import SimpleNamespace

import numpy as np
import torch

from . import ops
from .datasets import get_dataloader
from .datasets.templates import load_templates
from .evaluation import get_detections_batch
from .models.model import DetectionModel, base_model_of
from .wider_eval import DeviceEvaluator, load_ground_truth

IMAGES_PER_CALL = 8           # images per get_detections_batch call (one synchronisation and one NMS call each)


def _event_and_name(img_path):
    """The (event, image) a result file of this image would be read back under (evaluation.write_results / wider_eval.read_predictions)."""
    head, _, tail = img_path.replace("jpg", "txt").rpartition("/")
    return head, tail[:-4] if tail.endswith(".txt") else tail


class Validator:
    """The validation set, its ground truth and the evaluation copy of the model.  `run(state_dict)` -> {setting: AP}."""

    def __init__(self, valdata, num_templates, device, img_transforms, prob_thresh=0.03, nms_thresh=0.3, num_images=None, gt_dir=None,
                 dataset_root="", seed=0):
        if str(valdata) == "synthetic" or (str(valdata) != "synthetic-faces" and not gt_dir):
            raise SystemExit(f"--val-every: valdata {valdata} carries no ground truth: use synthetic-faces, or a WIDER annotation file with "
                             "--val-gt-dir DIR (the eval_tools ground-truth directory)")
        self.device, self.prob_thresh, self.nms_thresh = torch.device(device), float(prob_thresh), float(nms_thresh)
        largs = SimpleNamespace(batch_size=1, workers=0, dataset_root=dataset_root, debug=False, seed=seed,
                                synthetic_len=int(num_images) if num_images else 8)
        # the data set behind the loader is walked directly: rank 0 evaluates every image, whatever shard a loader of this rank would hold
        self.dataset = get_dataloader(valdata, largs, num_templates, train=False, split="val", img_transforms=img_transforms)[0].dataset
        self.templates = load_templates(num_templates)
        self.num_images = min(len(self.dataset), int(num_images)) if num_images else len(self.dataset)
        if str(valdata) == "synthetic-faces":
            self.settings = ("all",)
            gt = {"faces": self.dataset.ground_truth()}
            self.gt_boxes, self.keep_lists = gt, [{"faces": {k: np.arange(v.shape[0]) for k, v in gt["faces"].items()}}]
        else:
            self.settings = ("easy", "medium", "hard")
            loaded = [load_ground_truth(gt_dir, s) for s in self.settings]
            self.gt_boxes, self.keep_lists = loaded[0][0], [keep for _, keep in loaded]
        self.model = None

    def _model_for(self, state_dict):
        if self.model is None:
            # the constructor draws an initialisation that load_state_dict overwrites: the draw must not advance the run's generator
            with torch.random.fork_rng(devices=[]):
                self.model = DetectionModel(base_model=base_model_of(state_dict), num_templates=self.templates.shape[0])
            self.model = self.model.to(self.device).eval()
        self.model.load_state_dict(state_dict)                # a copy: nothing of the training model is shared
        return self.model

    def run(self, state_dict):
        """{setting: AP} of the weights in `state_dict` over the first `num_images` validation images.  An image that occurs twice (a synthetic
        data set longer than its images) counts once; only the images that were run count their boxes."""
        model = self._model_for(state_dict)
        ds = self.dataset
        evaluator = DeviceEvaluator(self.settings, device=self.device)
        seen = set()
        for first in range(0, self.num_images, IMAGES_PER_CALL):
            items = [ds[i] for i in range(first, min(first + IMAGES_PER_CALL, self.num_images))]
            items = [(img, path) for img, path in items if not (path in seen or seen.add(path))]
            if not items:
                continue
            dets = get_detections_batch(model, [img for img, _ in items], self.templates, ds.rf, ds.transforms, self.prob_thresh, self.nms_thresh,
                                        device=self.device, mask_axis="template", pyramid_on_gpu=True)
            keys = [_event_and_name(path) for _, path in items]
            gts = [self.gt_boxes.get(e, {}).get(n, np.zeros((0, 4))) for e, n in keys]
            keeps = [[k.get(e, {}).get(n, []) for e, n in keys] for k in self.keep_lists]
            evaluator.add([ops.wider_rows(d) for d in dets], gts, keeps)
        return {s: ap for s, (ap, _) in evaluator.finish().items()}
