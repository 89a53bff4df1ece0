"""The frozen-BatchNorm training step with the lower trunk stages frozen as well (DetectionModel.set_trainable_layers(k)) on one MI355X: one
engine per k in {4, 3, 2, 1, 0}, ALTERNATING in one process on one box, one JSON line per round:

  * k<k>_ms / k<k>_img_s: the bf16 step of scripts/frozen_bn_numbers.py's frozen leg (TrainEngine, bs 12, 500 x 500, targets on the device, the
                          trunk's BatchNorm frozen) with the heads and the top k of layer3, layer2, layer1, stem trained; k = 4 is that leg itself;
  * k<k>_over_k4:         k4_ms / k<k>_ms.

Five models with the same tamed random weights (bench.py's recipe) live side by side; each leg of a round runs --steps steps behind --warmup
warm-up steps.  --only K runs that leg alone (the form a kernel trace is taken of).
    python scripts/trainable_layers_numbers.py [--rounds 3 --steps 30 --warmup 5] > profiles/trainable_layers.jsonl"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tiny-faces-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

LEGS = (4, 3, 2, 1, 0)


def make_engine(k, device):
    from bench import tame_init_
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as mm
    from tinyfaces.models.loss import DetectionCriterion
    torch.manual_seed(0)
    model = tame_init_(mm.DetectionModel(num_templates=25), 0).set_compute_dtype(torch.bfloat16)
    model.freeze_batchnorm().set_trainable_layers(k)
    return TrainEngine(model, DetectionCriterion(25), lr=1e-4, device=device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", type=int, choices=LEGS, default=None)
    args = ap.parse_args()
    from bench import synthetic_batch
    from tinyfaces import _hip, ops
    from tinyfaces.datasets.templates import load_templates
    device = torch.device("cuda:0")
    t_d = torch.as_tensor(load_templates(), dtype=torch.float64, device=device)
    pool = [synthetic_batch(s, 12, device, None) for s in range(4)]
    legs = [k for k in LEGS if args.only in (None, k)]
    engines = {k: make_engine(k, device) for k in legs}

    def run(eng, n, first):
        for i in range(n):
            b = pool[(first + i) % len(pool)]
            cm, rm = ops.dense_overlap_targets_device(b["boxes"], b["offs"], b["total"], t_d, paste_d=b["paste"], seed=first + i)
            loss2 = eng.step(b["x"], cm, rm)
        return loss2

    ident = _hip.identity()
    for rnd in range(args.rounds):
        rec = {"round": rnd, "dtype": "bf16", "batch": 12, "side": 500, "steps": args.steps, "build_id": ident["build_id"]}
        for k in legs:
            eng = engines[k]
            run(eng, args.warmup, 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss2 = run(eng, args.steps, args.warmup)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            rec[f"k{k}_ms"] = round(1e3 * dt / args.steps, 4)
            rec[f"k{k}_img_s"] = round(12 * args.steps / dt, 1)
            rec[f"k{k}_trained_tensors"] = len(eng.model.trainable_parameter_names())
            rec[f"k{k}_loss"] = [round(v, 4) for v in loss2.cpu().tolist()]
        if 4 in legs:
            for k in legs:
                if k != 4:
                    rec[f"k{k}_over_k4"] = round(rec["k4_ms"] / rec[f"k{k}_ms"], 4)
        print(json.dumps(rec), flush=True)
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
