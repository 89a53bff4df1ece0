"""The batch-statistics training step against the frozen-BatchNorm step (DetectionModel.freeze_batchnorm) on one MI355X, ALTERNATING in
one process on one box, one JSON line per pair:

  * stats_ms / stats_img_s:   the bf16 training step of bench.py's headline (TrainEngine, bs 12, 500 x 500, targets on the device);
  * frozen_ms / frozen_img_s: the same step with the trunk's BatchNorm frozen (folded-BN forward, three data-gradient launches per identity
                              bottleneck, segment-aware SGD).

Two engines (two models with the same tamed random weights, bench.py's recipe) live side by side; each leg of a pair runs --steps steps
behind --warmup warm-up steps.  --only frozen runs the frozen leg alone (the form a kernel trace is taken of).
    python scripts/frozen_bn_numbers.py [--pairs 3 --steps 30 --warmup 5] > profiles/frozen_bn.jsonl"""
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


def make_engine(frozen, device):
    from bench import tame_init_
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as mm
    from tinyfaces.models.loss import DetectionCriterion
    torch.manual_seed(0)
    model = tame_init_(mm.DetectionModel(num_templates=25), 0).set_compute_dtype(torch.bfloat16)
    if frozen:
        model.freeze_batchnorm()
    return TrainEngine(model, DetectionCriterion(25), lr=1e-4, device=device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["stats", "frozen"], default=None)
    args = ap.parse_args()
    from bench import synthetic_batch
    from tinyfaces import _hip, ops
    from tinyfaces.datasets.templates import load_templates
    device = torch.device("cuda:0")
    t_d = torch.as_tensor(load_templates(), dtype=torch.float64, device=device)
    pool = [synthetic_batch(s, 12, device, None) for s in range(4)]
    legs = [n for n in ("stats", "frozen") if args.only in (None, n)]
    engines = {n: make_engine(n == "frozen", device) for n in legs}

    def run(eng, n, first):
        for i in range(n):
            b = pool[(first + i) % len(pool)]
            cm, rm = ops.dense_overlap_targets_device(b["boxes"], b["offs"], b["total"], t_d, paste_d=b["paste"], seed=first + i)
            loss2 = eng.step(b["x"], cm, rm)
        return loss2

    ident = _hip.identity()
    for pair in range(args.pairs):
        rec = {"pair": pair, "dtype": "bf16", "batch": 12, "side": 500, "steps": args.steps, "build_id": ident["build_id"]}
        for name in legs:
            eng = engines[name]
            run(eng, args.warmup, 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss2 = run(eng, args.steps, args.warmup)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            rec[f"{name}_ms"] = round(1e3 * dt / args.steps, 4)
            rec[f"{name}_img_s"] = round(12 * args.steps / dt, 1)
            rec[f"{name}_loss"] = [round(v, 4) for v in loss2.cpu().tolist()]
        if len(legs) == 2:
            rec["frozen_over_stats"] = round(rec["stats_ms"] / rec["frozen_ms"], 4)
        print(json.dumps(rec), flush=True)
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
