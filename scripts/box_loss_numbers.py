"""What the overlap regression forms of the focal criterion (DetectionCriterion(cls_loss="focal", reg_loss="iou" | "giou" | "diou"),
tf_criterion_focal_box_fwd_bwd) cost next to the focal criterion with SmoothL1 on one MI355X, the legs ALTERNATING in one process on one box,
one JSON line per pair:

  * "call" lines: device-event time of ONE criterion call of each form and of ONE ops.criterion_focal_fwd_bwd call (the yardstick: SmoothL1,
    measured in the same process) on the operands of the training step (bs 12, 25 x 63 x 63: logits ~ N(0, 1.5^2), targets of bench.py's
    synthetic batch from the device target kernel), median over --calls calls of each leg;
  * "step" lines: the bf16 bs 12 500 x 500 training step of bench.py's headline with each regression loss, one engine per loss with the same
    tamed random weights, median over --steps steps behind --warmup warm-up ones.

The new forms read what the SmoothL1 form reads and add about six transcendentals per positive.  The last line of each kind (`"summary"`)
puts every form's median difference to the SmoothL1 leg next to the spread of the legs between the pairs of this job: a difference inside
that spread is noise, and the line says so.
    python scripts/box_loss_numbers.py [--pairs 5 --calls 200 --steps 24 --warmup 6] >> profiles/box_loss.jsonl"""
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

FORMS = ("iou", "giou", "diou")
LEGS = ("smooth_l1",) + FORMS


def make_engine(reg_loss, device):
    from bench import tame_init_
    from tinyfaces.datasets.templates import load_templates
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as mm
    from tinyfaces.models.loss import DetectionCriterion
    torch.manual_seed(0)
    model = tame_init_(mm.DetectionModel(num_templates=25), 0).set_compute_dtype(torch.bfloat16)
    return TrainEngine(model, DetectionCriterion(25, seed=0, cls_loss="focal", reg_loss=reg_loss, templates=load_templates()), lr=1e-4, device=device)


def median_ms(pairs):
    return round(statistics.median(a.elapsed_time(b) for a, b in pairs), 4)


def summary(kind, recs, suffix, extra):
    def spread(key):
        return round(1e3 * (max(r[key] for r in recs) - min(r[key] for r in recs)), 1)

    base = f"smooth_l1{suffix}"
    out = {"summary": True, "kind": kind, "pairs": len(recs), f"{base}_median": round(statistics.median(r[base] for r in recs), 4),
           f"{base}_spread_us": spread(base)}
    for form in FORMS:
        key = f"{form}{suffix}"
        diff = round(statistics.median(1e3 * (r[key] - r[base]) for r in recs), 1)
        noise = max(spread(key), spread(base))
        out.update({f"{key}_median": round(statistics.median(r[key] for r in recs), 4), f"{key}_spread_us": spread(key),
                    f"{form}_minus_smooth_l1_us_median": diff, f"{form}_difference_inside_spread": bool(abs(diff) <= noise)})
    return {**out, **extra}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--skip-steps", dest="skip_steps", action="store_true", help="the call timings only")
    args = ap.parse_args()
    from bench import synthetic_batch
    from tinyfaces import _hip, ops
    from tinyfaces.datasets.templates import load_templates
    device = torch.device("cuda:0")
    ident = _hip.identity()
    t_d = torch.as_tensor(load_templates(), dtype=torch.float64, device=device)
    twh = ops.template_wh(load_templates()).to(device)
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
    grad = torch.empty_like(out)
    legs = {"smooth_l1": lambda: ops.criterion_focal_fwd_bwd(out, cm, rm, grad=grad)}
    for form in FORMS:
        legs[form] = lambda form=form: ops.criterion_focal_box_fwd_bwd(out, cm, rm, reg_loss=form, template_wh=twh, grad=grad)
    recs = []
    for pair in range(args.pairs):
        rec = {"kind": "call", "pair": pair, "batch": 12, "map": [25, 63, 63], "elements": 12 * E, "positives": npos, "labelled": labelled,
               "calls": args.calls, "build_id": ident["build_id"]}
        for name, call in legs.items():
            for _ in range(8):
                call()
            torch.cuda.synchronize()
            marks = []
            for _ in range(args.calls):
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                call()
                ev[1].record()
                marks.append(ev)
            torch.cuda.synchronize()
            rec[f"{name}_ms"] = median_ms(marks)
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    if len(recs) > 1:
        print(json.dumps(summary("call", recs, "_ms", {"build_id": ident["build_id"]})), flush=True)
    if args.skip_steps:
        return

    # ---- the training step
    engines = {name: make_engine(name, device) for name in LEGS}

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
        print(json.dumps(summary("step", recs, "_step_ms", {"build_id": ident["build_id"]})), flush=True)
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
