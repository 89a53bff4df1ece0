"""What gradient-norm clipping costs the fused training step (TrainEngine(max_grad_norm=...)) on one MI355X: two engines ALTERNATING in one
process on one box, one JSON line per pair:

  * plain_ms / plain_img_s: the bf16 training step of bench.py's headline (TrainEngine, bs 12, 500 x 500, targets on the device);
  * clip_ms / clip_img_s:   the same step with max_grad_norm = 1e9 -- the norm pass over the trained slices of the flat gradient, the
                            one-block finalize and the clipped form of the SGD launches all run, the coefficient stays 1, so both engines'
                            weights evolve identically (`same_weights` says whether they did, bit for bit).

Two models with the same tamed random weights (bench.py's recipe) live side by side; each leg of a pair runs --steps steps behind --warmup
warm-up steps.  --freeze-bn times the pair on the frozen-BatchNorm step (the range-table forms of the kernels).  --only clip runs that leg alone
(the form a kernel trace is taken of).  The yardstick of the absolute numbers is bench.py's headline of the parent commit in the same job.
    python scripts/grad_clip_numbers.py [--pairs 3 --steps 30 --warmup 5] > profiles/grad_clip.jsonl"""
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


def make_engine(clip, frozen, device):
    from bench import tame_init_
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as mm
    from tinyfaces.models.loss import DetectionCriterion
    torch.manual_seed(0)
    model = tame_init_(mm.DetectionModel(num_templates=25), 0).set_compute_dtype(torch.bfloat16)
    if frozen:
        model.freeze_batchnorm()
    return TrainEngine(model, DetectionCriterion(25, seed=0), lr=1e-4, device=device, max_grad_norm=1e9 if clip else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--freeze-bn", dest="freeze_bn", action="store_true")
    ap.add_argument("--only", choices=["plain", "clip"], default=None)
    args = ap.parse_args()
    from bench import synthetic_batch
    from tinyfaces import _hip, ops
    from tinyfaces.datasets.templates import load_templates
    device = torch.device("cuda:0")
    t_d = torch.as_tensor(load_templates(), dtype=torch.float64, device=device)
    pool = [synthetic_batch(s, 12, device, None) for s in range(4)]
    legs = [n for n in ("plain", "clip") if args.only in (None, n)]
    engines = {n: make_engine(n == "clip", args.freeze_bn, device) for n in legs}

    def run(eng, n, first):
        for i in range(n):
            b = pool[(first + i) % len(pool)]
            cm, rm = ops.dense_overlap_targets_device(b["boxes"], b["offs"], b["total"], t_d, paste_d=b["paste"], seed=first + i)
            loss2 = eng.step(b["x"], cm, rm)
        return loss2

    ident = _hip.identity()
    for pair in range(args.pairs):
        rec = {"pair": pair, "dtype": "bf16", "batch": 12, "side": 500, "steps": args.steps, "batchnorm": "frozen" if args.freeze_bn else "batch statistics",
               "build_id": ident["build_id"]}
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
            rec["clip_over_plain"] = round(rec["clip_ms"] / rec["plain_ms"], 4)
            rec["clip_extra_us"] = round(1e3 * (rec["clip_ms"] - rec["plain_ms"]), 1)
            rec["same_weights"] = bool(torch.equal(engines["plain"].flat_p, engines["clip"].flat_p))
        if "clip" in engines:
            st = engines["clip"]._clip_state.read()
            rec["grad_norm"], rec["coef"] = round(st.norm, 4), st.coef
            rec["norm_ranges"] = len(engines["clip"]._norm_segments())
        print(json.dumps(rec), flush=True)
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
