"""Per-trunk numbers of DetectionModel(base_model=resnet50 / resnet101 / resnet152) on one MI355X, one JSON line per trunk:

  * train_img_s: the bf16 training step of bench.py's headline (TrainEngine, bs 12, 500 x 500, targets on the device), img/s over --steps;
  * pyramid_ms:  the 3-scale evaluation pyramid of bench.py's eval line (480x640 + 960x1280 + 1920x2560, bf16, levels side by side on the
                 model's lanes, inside one constant_weights() session), median ms per image of the forwards over --runs.

Random tamed weights (bench.py's recipe); the numbers are about the executor, not about accuracy.
    python scripts/trunk_numbers.py [--steps 30 --warmup 5 --runs 20] > profiles/trunks.jsonl"""
import argparse
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


def train_img_s(name, steps, warmup, device):
    from bench import synthetic_batch, tame_init_
    from tinyfaces import ops
    from tinyfaces.datasets.templates import load_templates
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as mm
    from tinyfaces.models.loss import DetectionCriterion
    torch.manual_seed(0)
    model = tame_init_(mm.DetectionModel(base_model=getattr(mm, name), num_templates=25), 0).set_compute_dtype(torch.bfloat16)
    eng = TrainEngine(model, DetectionCriterion(25), lr=1e-4, device=device)
    t_d = torch.as_tensor(load_templates(), dtype=torch.float64, device=device)
    pool = [synthetic_batch(s, 12, device, None) for s in range(4)]

    def step(i):
        b = pool[i % len(pool)]
        cm, rm = ops.dense_overlap_targets_device(b["boxes"], b["offs"], b["total"], t_d, paste_d=b["paste"], seed=i)
        return eng.step(b["x"], cm, rm)
    for i in range(warmup):
        step(i)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        loss2 = step(warmup + i)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    loss = loss2.cpu().tolist()
    eng.close()
    return 12 * steps / dt, 1e3 * dt / steps, loss


def pyramid_ms(name, runs, device):
    from bench import tame_init_
    from tinyfaces.models import model as mm
    torch.manual_seed(0)
    model = tame_init_(mm.DetectionModel(base_model=getattr(mm, name), num_templates=25), 0).to(device).set_compute_dtype(torch.bfloat16).eval()
    g = torch.Generator().manual_seed(0)
    levels = [torch.randn(1, 3, h, w, generator=g).to(device) for h, w in ((480, 640), (960, 1280), (1920, 2560))]
    times = []
    with torch.no_grad(), model.constant_weights(reserve=(1, 1920, 2560)):
        for it in range(runs + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.forward_levels(levels)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(times[2:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--trunks", default="resnet50,resnet101,resnet152")
    args = ap.parse_args()
    from tinyfaces import _hip
    from tinyfaces.models.model import TRUNKS
    device = torch.device("cuda:0")
    for name in args.trunks.split(","):
        ips, ms_step, loss = train_img_s(name, args.steps, args.warmup, device)
        pm = pyramid_ms(name, args.runs, device)
        print(json.dumps({"trunk": name, "blocks": TRUNKS[name], "train_img_s": round(ips, 1), "ms_per_step": round(ms_step, 3),
                          "pyramid_ms": round(pm, 3), "loss": [round(v, 4) for v in loss], "batch": 12, "side": 500, "dtype": "bf16",
                          "steps": args.steps, "runs": args.runs, "tf_version": int(_hip.lib().tf_version()),
                          "gpu": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
