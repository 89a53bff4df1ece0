"""What the colour jitter costs on one MI355X, one JSON line per measurement (profiles/color_jitter.jsonl).  The yardstick of every item is
the feature-off leg of the same process -- the path the parent commit runs.

  --step kernels   ops.image_prepare on the 500 x 500 training window (a 768 x 1024 uint8 image, x0.5 / x1 / x2, window pasted with padding):
                   plain | a three-op chain without contrast (one launch) | the full four-op chain (two launches) | contrast alone (two launches),
                   device events around --batch consecutive calls, warm-up first, the legs ALTERNATING in one process, --pairs rounds, median;
                   `same_bits`: two runs returned the same bytes.
  --step batch     the batch building of bench.py --with-augment (12 images of 768 x 1024 through augment.process_inputs on an input stream of
                   its own, then the target assignment), with color_jitter=None and with (0.4, 0.4, 0.4, 0.1), ALTERNATING, wall clock around
                   the synchronous build, median of --runs.

    bash scripts/gpu_job.sh color-jitter        (one process and one time limit per step) -> profiles/color_jitter.jsonl"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tiny-faces-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

CHAINS = {"plain": None,
          "three_ops_no_contrast": [("brightness", 1.2), ("hue", 0.05), ("saturation", 0.8)],
          "four_ops": [("brightness", 1.2), ("contrast", 0.9), ("hue", 0.05), ("saturation", 0.8)],
          "contrast_only": [("contrast", 0.9)]}
# resized_hw, crop (y, x, h, w), paste (y, x), flip: the three scales of the training augmentation on a 768 x 1024 image
WINDOWS = {"x0.5": ((384, 512), (0, 0, 384, 500), (58, 0), True), "x1": ((768, 1024), (131, 262, 500, 500), (0, 0), False),
           "x2": ((1536, 2048), (517, 1001, 500, 500), (0, 0), True)}


def kernels(args, ident):
    from tinyfaces import ops
    img = torch.randint(0, 256, (768, 1024, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(7)).cuda()
    out = torch.empty(args.batch, 3, 500, 500, device="cuda")
    for wname, (rhw, crop, paste, flip) in WINDOWS.items():
        times, bits, same = {k: [] for k in CHAINS}, {}, True
        for _ in range(args.pairs + 2):                                    # the first two rounds are warm-up
            for name, chain in CHAINS.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for k in range(args.batch):
                    ops.image_prepare(img, resized_hw=rhw, crop=crop, paste=paste, flip=flip, out_hw=(500, 500), out=out[k], jitter=chain)
                e1.record()
                torch.cuda.synchronize()
                times[name].append(1e3 * e0.elapsed_time(e1) / args.batch)
                now = out[0].clone()
                same = same and (name not in bits or torch.equal(bits[name], now))
                bits[name] = now
        med = {k: float(np.median(v[2:])) for k, v in times.items()}
        rec = {"step": "kernels", "window": wname, "out_hw": [500, 500], "calls_per_timing": args.batch, "pairs": args.pairs,
               "us_per_image": {k: round(v, 2) for k, v in med.items()},
               "min_us_per_image": {k: round(float(np.min(v[2:])), 2) for k, v in times.items()},
               "extra_us_per_image": {k: round(med[k] - med["plain"], 2) for k in CHAINS if k != "plain"},
               "launches": {"plain": 1, "three_ops_no_contrast": 1, "four_ops": 2, "contrast_only": 2},
               "workspace_bytes_with_contrast": int(ops.lib().tf_image_prepare_jitter_workspace_bytes(500, 500, 1, (ctypes.c_int * 1)(1))),
               "same_bits": bool(same), "build_id": ident["build_id"]}
        print(json.dumps(rec), flush=True)


def batch(args, ident):
    from tinyfaces import ops
    from tinyfaces.datasets import augment as aug
    from tinyfaces.datasets.synthetic import random_boxes
    from tinyfaces.datasets.templates import load_templates
    device = torch.device("cuda:0")
    templates = load_templates()
    gi = torch.Generator().manual_seed(7)
    raw = [(torch.randint(0, 256, (768, 1024, 3), dtype=torch.uint8, generator=gi).to(device),
            random_boxes(np.random.RandomState(50 + k)) * np.array([1024 / 500, 768 / 500] * 2)) for k in range(args.batch)]
    in_stream = torch.cuda.Stream(device=device)
    legs = {"off": None, "on": (0.4, 0.4, 0.4, 0.1)}
    times = {k: [] for k in legs}
    for it in range(args.runs + 2):
        for name, cj in legs.items():
            arng = np.random.RandomState(it)                               # the same geometric decisions for both legs of a round
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.cuda.stream(in_stream):
                x = torch.empty(args.batch, 3, 500, 500, device=device)
                boxes, pastes, flips = [], [], []
                for k, (u8, bb) in enumerate(raw):
                    _, b2, paste, flip = aug.process_inputs(u8, bb, rng=arng, out=x[k], color_jitter=cj)
                    boxes.append(b2); pastes.append(paste); flips.append(int(flip))
                ops.dense_overlap_targets(boxes, templates, paste_boxes=pastes, flips=flips, seed=it, device=device)
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0))
    med = {k: float(np.median(v[2:])) for k, v in times.items()}
    rec = {"step": "batch", "images": args.batch, "source": "768x1024 uint8, resident", "color_jitter": list(legs["on"]), "runs": args.runs,
           "ms_per_batch": {k: round(v, 3) for k, v in med.items()}, "min_ms_per_batch": {k: round(float(np.min(v[2:])), 3) for k, v in times.items()},
           "extra_ms_per_batch": round(med["on"] - med["off"], 3), "extra_us_per_image": round(1e3 * (med["on"] - med["off"]) / args.batch, 2),
           "build_id": ident["build_id"]}
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernels", "batch"], required=True)
    ap.add_argument("--batch", type=int, default=12)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--runs", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scripts/color_jitter_numbers.py measures on an MI355X: no GPU, no numbers")
    from tinyfaces import _hip
    {"kernels": kernels, "batch": batch}[args.step](args, _hip.identity())


if __name__ == "__main__":
    main()
