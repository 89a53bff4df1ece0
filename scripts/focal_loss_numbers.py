"""What the focal form of the criterion (DetectionCriterion(cls_loss="focal"), tf_criterion_focal_fwd_bwd) costs next to the soft-margin
form on one MI355X, both ALTERNATING in one process on one box, one JSON line per pair:

  * "call" lines: device-event time of ONE ops.criterion_focal_fwd_bwd call and of ONE ops.criterion_fwd_bwd call on the operands of the
    training step (bs 12, 25 x 63 x 63: logits ~ N(0, 1.5^2), targets of bench.py's synthetic batch from the device target kernel), median
    over --calls calls of each leg.  The soft-margin call mines class_map in place, so it gets a fresh copy made outside the timed region;
  * "step" lines: the bf16 bs 12 500 x 500 training step of bench.py's headline with each criterion, two engines with the same tamed random
    weights, median over --steps steps behind --warmup warm-up ones.

`estimate_us` is the traffic of one pass over the operands -- 10 floats per element (label, five logits read, ... five gradients written;
the four regression pairs of positives on top) -- at --hbm-gbs (default 4000: half the 8 TB/s peak, an assumption, not a measurement).
The last line of each kind (`"summary"`) puts the median difference next to the spread of each leg between the pairs of this job: a
difference inside that spread is noise, and the line says so.
    python scripts/focal_loss_numbers.py [--pairs 5 --calls 200 --steps 24 --warmup 6] >> profiles/focal_loss.jsonl"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tiny-faces-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def make_engine(cls_loss, device):
    from bench import tame_init_
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as mm
    from tinyfaces.models.loss import DetectionCriterion
    torch.manual_seed(0)
    model = tame_init_(mm.DetectionModel(num_templates=25), 0).set_compute_dtype(torch.bfloat16)
    return TrainEngine(model, DetectionCriterion(25, seed=0, cls_loss=cls_loss), lr=1e-4, device=device)


def median_ms(pairs):
    return round(statistics.median(a.elapsed_time(b) for a, b in pairs), 4)


def summary(kind, recs, a, b, extra):
    def spread(key):
        return round(1e3 * (max(r[key] for r in recs) - min(r[key] for r in recs)), 1)

    diff = round(statistics.median(1e3 * (r[a] - r[b]) for r in recs), 1)
    noise = max(spread(a), spread(b))
    return {"summary": True, "kind": kind, "pairs": len(recs), f"{a}_median": round(statistics.median(r[a] for r in recs), 4),
            f"{b}_median": round(statistics.median(r[b] for r in recs), 4), "focal_minus_soft_margin_us_median": diff,
            f"{a}_spread_us": spread(a), f"{b}_spread_us": spread(b), "difference_inside_spread": bool(abs(diff) <= noise), **extra}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--hbm-gbs", dest="hbm_gbs", type=float, default=4000.0)
    ap.add_argument("--skip-steps", dest="skip_steps", action="store_true", help="the call timings only")
    args = ap.parse_args()
    from bench import synthetic_batch
    from tinyfaces import _hip, ops
    from tinyfaces.datasets.templates import load_templates
    device = torch.device("cuda:0")
    ident = _hip.identity()
    t_d = torch.as_tensor(load_templates(), dtype=torch.float64, device=device)
    pool = [synthetic_batch(s, 12, device, None) for s in range(4)]

    def targets(i):
        b = pool[i % len(pool)]
        return ops.dense_overlap_targets_device(b["boxes"], b["offs"], b["total"], t_d, paste_d=b["paste"], seed=i)

    # ---- the call alone
    out = torch.randn(12, 125, 63, 63, generator=torch.Generator().manual_seed(0)).mul_(1.5).to(device)
    cm, rm = targets(0)
    E = cm[0].numel()
    npos = int((cm == 1).sum())
    labelled = int((cm != 0).sum())
    estimate_us = round(4.0 * (10 * 12 * E + 8 * npos) / (args.hbm_gbs * 1e9) * 1e6, 1)
    grad = torch.empty_like(out)
    copies = [cm.clone() for _ in range(args.calls + 8)]
    legs = {"focal": lambda labels, i: ops.criterion_focal_fwd_bwd(out, cm, rm, grad=grad),
            "soft_margin": lambda labels, i: ops.criterion_fwd_bwd(out, labels, rm, seed=i, grad=grad)}
    recs = []
    for pair in range(args.pairs):
        rec = {"kind": "call", "pair": pair, "batch": 12, "map": [25, 63, 63], "elements": 12 * E, "positives": npos, "labelled": labelled,
               "calls": args.calls, "estimate_us": estimate_us, "build_id": ident["build_id"]}
        for name, call in legs.items():
            for i in range(args.calls, args.calls + 8):
                call(copies[i].copy_(cm), i)
            torch.cuda.synchronize()
            marks = []
            for i in range(args.calls):
                labels = copies[i].copy_(cm)                         # (outside the events)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                call(labels, i)
                ev[1].record()
                marks.append(ev)
            torch.cuda.synchronize()
            rec[f"{name}_ms"] = median_ms(marks)
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    if len(recs) > 1:
        print(json.dumps(summary("call", recs, "focal_ms", "soft_margin_ms", {"estimate_us": estimate_us, "build_id": ident["build_id"]})), flush=True)
    if args.skip_steps:
        return

    # ---- the training step
    engines = {"focal": make_engine("focal", device), "soft_margin": make_engine("soft_margin", device)}

    def run(eng, n, first, timed):
        marks = []
        for i in range(n):
            b = pool[(first + i) % len(pool)]
            c, r = targets(first + i)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            eng.step(b["x"], c, r)
            ev[1].record()
            if timed:
                marks.append(ev)
        return marks

    recs = []
    for pair in range(args.pairs):
        rec = {"kind": "step", "pair": pair, "dtype": "bf16", "batch": 12, "side": 500, "steps": args.steps, "build_id": ident["build_id"]}
        for name, eng in engines.items():
            run(eng, args.warmup, 0, False)
            torch.cuda.synchronize()
            marks = run(eng, args.steps, args.warmup, True)
            torch.cuda.synchronize()
            rec[f"{name}_step_ms"] = median_ms(marks)
            rec[f"{name}_img_s"] = round(12 / rec[f"{name}_step_ms"] * 1e3, 1)
        rec["finite"] = bool(all(torch.isfinite(e.flat_p).all() for e in engines.values()))
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    if len(recs) > 1:
        print(json.dumps(summary("step", recs, "focal_step_ms", "soft_margin_step_ms", {"build_id": ident["build_id"]})), flush=True)
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
