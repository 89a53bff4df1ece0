"""What AdamW costs the fused training step (TrainEngine(optimizer="adamw")) against the default SGD step on one MI355X: two engines
ALTERNATING in one process on one box, timed with device events, one JSON line per pair:

  * sgd_ms / sgd_img_s:      the bf16 training step of bench.py's headline (TrainEngine, bs 12, 500 x 500, targets on the device);
  * adamw_ms / adamw_img_s:  the same step with optimizer="adamw" -- one launch of tf_adamw_advance and the AdamW update launches, which read
                             and write one more fp32 buffer (exp_avg_sq): 28 B per element instead of 20 B.

`estimate_us` is the extra traffic (8 B per element the update launches walk) at --hbm-gbs (default 4000: half the 8 TB/s peak, an
assumption, not a measurement); `adamw_extra_us` is what was measured.  The last line (`"summary"`) gives the median difference next to the
spread of each leg between the pairs of this job: a difference inside that spread is noise, and the line says so (`inside_spread`).

Two models with the same tamed random weights (bench.py's recipe) live side by side; each leg of a pair runs --steps steps behind --warmup
warm-up steps.  --freeze-bn times the pair on the frozen-BatchNorm step (the range-table forms of the kernels).  The two optimizers train
different weights from the first step on, so the losses differ; both must stay finite (`finite`).
    python scripts/adamw_numbers.py [--pairs 4 --steps 30 --warmup 5] >> profiles/adamw.jsonl"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tiny-faces-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

LEGS = ("sgd", "adamw")


def make_engine(optimizer, frozen, device):
    from bench import tame_init_
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as mm
    from tinyfaces.models.loss import DetectionCriterion
    torch.manual_seed(0)
    model = tame_init_(mm.DetectionModel(num_templates=25), 0).set_compute_dtype(torch.bfloat16)
    if frozen:
        model.freeze_batchnorm()
    return TrainEngine(model, DetectionCriterion(25, seed=0), lr=1e-4, device=device, optimizer=optimizer)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--freeze-bn", dest="freeze_bn", action="store_true")
    ap.add_argument("--hbm-gbs", dest="hbm_gbs", type=float, default=4000.0)
    args = ap.parse_args()
    from bench import synthetic_batch
    from tinyfaces import _hip, ops
    from tinyfaces.datasets.templates import load_templates
    device = torch.device("cuda:0")
    t_d = torch.as_tensor(load_templates(), dtype=torch.float64, device=device)
    pool = [synthetic_batch(s, 12, device, None) for s in range(4)]
    engines = {n: make_engine(n, args.freeze_bn, device) for n in LEGS}
    eng0 = engines["sgd"]
    if args.freeze_bn:
        walked = sum(e - s for s, e in eng0._trained_segments())
    else:
        walked = sum(e - s for s, e, mult in eng0.groups if mult != 0.0)
    estimate_us = round(8.0 * walked / (args.hbm_gbs * 1e9) * 1e6, 1)
    recs = []

    def run(eng, n, first):
        for i in range(n):
            b = pool[(first + i) % len(pool)]
            cm, rm = ops.dense_overlap_targets_device(b["boxes"], b["offs"], b["total"], t_d, paste_d=b["paste"], seed=first + i)
            loss2 = eng.step(b["x"], cm, rm)
        return loss2

    ident = _hip.identity()
    for pair in range(args.pairs):
        rec = {"pair": pair, "dtype": "bf16", "batch": 12, "side": 500, "steps": args.steps, "batchnorm": "frozen" if args.freeze_bn else "batch statistics",
               "timer": "device events", "build_id": ident["build_id"]}
        for name in LEGS:
            eng = engines[name]
            run(eng, args.warmup, 0)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            loss2 = run(eng, args.steps, args.warmup)
            stop.record()
            stop.synchronize()
            ms = start.elapsed_time(stop)
            rec[f"{name}_ms"] = round(ms / args.steps, 4)
            rec[f"{name}_img_s"] = round(12 * args.steps / (ms * 1e-3), 1)
            rec[f"{name}_loss"] = [round(v, 4) for v in loss2.cpu().tolist()]
        rec["update_elements"], rec["estimate_us"] = walked, estimate_us
        rec["adamw_over_sgd"] = round(rec["adamw_ms"] / rec["sgd_ms"], 4)
        rec["adamw_extra_us"] = round(1e3 * (rec["adamw_ms"] - rec["sgd_ms"]), 1)
        rec["adamw_device_step"] = engines["adamw"].adam_state.step()
        rec["finite"] = bool(all(torch.isfinite(e.flat_p).all() for e in engines.values()) and torch.isfinite(engines["adamw"].flat_v).all())
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    if len(recs) > 1:
        extra = sorted(r["adamw_extra_us"] for r in recs)
        spread = {n: round(1e3 * (max(r[f"{n}_ms"] for r in recs) - min(r[f"{n}_ms"] for r in recs)), 1) for n in LEGS}
        median = extra[len(extra) // 2] if len(extra) % 2 else round(0.5 * (extra[len(extra) // 2 - 1] + extra[len(extra) // 2]), 1)
        print(json.dumps({"summary": True, "batchnorm": recs[0]["batchnorm"], "pairs": len(recs), "adamw_extra_us_median": median,
                          "adamw_extra_us_min": extra[0], "adamw_extra_us_max": extra[-1], "sgd_spread_us": spread["sgd"],
                          "adamw_spread_us": spread["adamw"], "estimate_us": estimate_us,
                          "inside_spread": bool(abs(median) <= max(spread.values())), "build_id": ident["build_id"]}), flush=True)
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
