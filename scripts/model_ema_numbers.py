"""What the model EMA costs the fused training step (TrainEngine(ema_decay=...)) on one MI355X: two engines ALTERNATING in one process on
one box, one JSON line per pair:

  * plain_ms / plain_img_s: the bf16 training step of bench.py's headline (TrainEngine, bs 12, 500 x 500, targets on the device);
  * ema_ms / ema_img_s:     the same step with ema_decay = 0.9999 -- the EMA instantiations of the SGD launches, which read and write one
                            more fp32 value per trained element (28 B instead of 20 B).  The parameters do not depend on the average:
                            `same_weights` says whether the two engines' weights stayed equal bit for bit (the step's fp32 atomic sums are
                            not ordered, so after some tens of steps they usually have not, with or without the average).

`estimate_us` is the extra traffic (8 B per element the SGD launches walk) at --hbm-gbs (default 4000: half the 8 TB/s
peak, an assumption, not a measurement); `ema_extra_us` is what was measured.  The last line (`"summary"`) gives the median difference next to the spread of each leg
between the pairs of this job: a difference inside that spread is noise, and the line says so (`inside_spread`).

Two models with the same tamed random weights (bench.py's recipe) live side by side; each leg of a pair runs --steps steps behind --warmup
warm-up steps.  --freeze-bn times the pair on the frozen-BatchNorm step (the range-table forms of the kernels).  --only ema runs that leg alone
(the form a kernel trace is taken of).  The yardstick of the absolute numbers is bench.py's headline of the parent commit in the same job.
    python scripts/model_ema_numbers.py [--pairs 3 --steps 30 --warmup 5] >> profiles/model_ema.jsonl"""
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


def make_engine(ema, frozen, device):
    from bench import tame_init_
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as mm
    from tinyfaces.models.loss import DetectionCriterion
    torch.manual_seed(0)
    model = tame_init_(mm.DetectionModel(num_templates=25), 0).set_compute_dtype(torch.bfloat16)
    if frozen:
        model.freeze_batchnorm()
    return TrainEngine(model, DetectionCriterion(25, seed=0), lr=1e-4, device=device, ema_decay=0.9999 if ema else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--freeze-bn", dest="freeze_bn", action="store_true")
    ap.add_argument("--only", choices=["plain", "ema"], default=None)
    ap.add_argument("--hbm-gbs", dest="hbm_gbs", type=float, default=4000.0)
    args = ap.parse_args()
    from bench import synthetic_batch
    from tinyfaces import _hip, ops
    from tinyfaces.datasets.templates import load_templates
    device = torch.device("cuda:0")
    t_d = torch.as_tensor(load_templates(), dtype=torch.float64, device=device)
    pool = [synthetic_batch(s, 12, device, None) for s in range(4)]
    legs = [n for n in ("plain", "ema") if args.only in (None, n)]
    engines = {n: make_engine(n == "ema", args.freeze_bn, device) for n in legs}
    any_eng = next(iter(engines.values()))
    if args.freeze_bn:
        walked = sum(e - s for s, e in any_eng._trained_segments())
    else:
        walked = sum(e - s for s, e, mult in any_eng.groups if mult != 0.0)
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
        rec["sgd_elements"], rec["estimate_us"] = walked, estimate_us
        if len(legs) == 2:
            rec["ema_over_plain"] = round(rec["ema_ms"] / rec["plain_ms"], 4)
            rec["ema_extra_us"] = round(1e3 * (rec["ema_ms"] - rec["plain_ms"]), 1)
            rec["same_weights"] = bool(torch.equal(engines["plain"].flat_p, engines["ema"].flat_p))
        if "ema" in engines:
            e = engines["ema"].ema
            rec["ema_updates"] = e.updates
            rec["ema_differs_from_weights"] = bool(not torch.equal(e.flat, engines["ema"].flat_p)) and bool(torch.isfinite(e.flat).all())
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    if len(legs) == 2 and len(recs) > 1:
        extra = sorted(r["ema_extra_us"] for r in recs)
        spread = {n: round(1e3 * (max(r[f"{n}_ms"] for r in recs) - min(r[f"{n}_ms"] for r in recs)), 1) for n in legs}
        median = extra[len(extra) // 2] if len(extra) % 2 else round(0.5 * (extra[len(extra) // 2 - 1] + extra[len(extra) // 2]), 1)
        print(json.dumps({"summary": True, "batchnorm": recs[0]["batchnorm"], "pairs": len(recs), "ema_extra_us_median": median,
                          "ema_extra_us_min": extra[0], "ema_extra_us_max": extra[-1], "plain_spread_us": spread["plain"],
                          "ema_spread_us": spread["ema"], "estimate_us": estimate_us,
                          "inside_spread": bool(abs(median) <= max(spread.values())), "build_id": ident["build_id"]}), flush=True)
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
