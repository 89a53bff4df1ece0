"""What the quality focal form of the criterion (DetectionCriterion(cls_loss="qfl"), tf_criterion_quality_fwd_bwd) costs next to the focal form
with the SAME regression loss on one MI355X, the two legs ALTERNATING in one process on one box, one JSON line per pair:

  * --step calls: device-event time of ONE ops.criterion_quality_fwd_bwd call and of ONE focal call of the same reg_loss (the yardstick,
    measured in the same pair) on the operands of the training step (bs 12, 25 x 63 x 63: logits ~ N(0, 1.5^2), targets of bench.py's
    synthetic batch from the device target kernel), median over --calls calls of each leg; every reg_loss in turn, and beta = 2.5 (the powf
    road) once;
  * --step steps: the bf16 bs 12 500 x 500 training step of bench.py's headline with cls_loss="qfl" and with cls_loss="focal" (reg_loss
    "diou"), two engines with the same tamed random weights alternating, median over --steps steps behind --warmup warm-up ones.

The pass is bound by its 10 E B floats of traffic and under 1 % of the anchors are positive: the expectation is the focal call's time plus a
few microseconds.  The last line of each kind (`"summary"`) puts the median difference of the legs next to the spread of the focal leg between
the pairs of this job and gives the ratio qfl / focal; above 1.25 the README owes the cause.
    python scripts/quality_loss_numbers.py --step calls [--pairs 5 --calls 200] >> profiles/quality_loss.jsonl
    python scripts/quality_loss_numbers.py --step steps [--pairs 5 --steps 24 --warmup 6] >> profiles/quality_loss.jsonl"""
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

REG_LOSSES = ("smooth_l1", "iou", "giou", "diou")


def make_engine(cls_loss, device):
    from bench import tame_init_
    from tinyfaces.datasets.templates import load_templates
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as mm
    from tinyfaces.models.loss import DetectionCriterion
    torch.manual_seed(0)
    model = tame_init_(mm.DetectionModel(num_templates=25), 0).set_compute_dtype(torch.bfloat16)
    return TrainEngine(model, DetectionCriterion(25, seed=0, cls_loss=cls_loss, reg_loss="diou", templates=load_templates()), lr=1e-4, device=device)


def median_ms(pairs):
    return round(statistics.median(a.elapsed_time(b) for a, b in pairs), 4)


def summary(kind, recs, a, b, extra):
    """a: the qfl key, b: the focal key of the pair records."""
    spread = lambda key: round(1e3 * (max(r[key] for r in recs) - min(r[key] for r in recs)), 1)
    diff = round(statistics.median(1e3 * (r[a] - r[b]) for r in recs), 1)
    ma, mb = statistics.median(r[a] for r in recs), statistics.median(r[b] for r in recs)
    return {"summary": True, "kind": kind, "pairs": len(recs), f"{a}_median": round(ma, 4), f"{b}_median": round(mb, 4), f"{a}_spread_us": spread(a),
            f"{b}_spread_us": spread(b), "qfl_minus_focal_us_median": diff, "qfl_over_focal": round(ma / mb, 4),
            "difference_inside_focal_spread": bool(abs(diff) <= spread(b)), **extra}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["calls", "steps"], required=True)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=6)
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

    if args.step == "calls":
        out = torch.randn(12, 125, 63, 63, generator=torch.Generator().manual_seed(0)).mul_(1.5).to(device)
        cm, rm = targets(0)
        E = cm[0].numel()
        grad = torch.empty_like(out)
        loss4, _, _ = ops.criterion_quality_fwd_bwd(out, cm, rm, reg_loss="diou", template_wh=twh, grad=grad)
        v = loss4.tolist()
        base = {"kind": "call", "batch": 12, "map": [25, 63, 63], "elements": 12 * E, "positives": int(v[3]), "labelled": int((cm != 0).sum()),
                "mean_iou_of_positives": round(v[2] / max(1.0, v[3]), 4), "calls": args.calls, "build_id": ident["build_id"]}
        for reg_loss, beta in [(r, 2.0) for r in REG_LOSSES] + [("diou", 2.5)]:
            legs = {"qfl_ms": lambda: ops.criterion_quality_fwd_bwd(out, cm, rm, beta=beta, reg_loss=reg_loss, template_wh=twh, grad=grad),
                    "focal_ms": lambda: ops.criterion_focal_box_fwd_bwd(out, cm, rm, reg_loss=reg_loss, template_wh=twh, grad=grad)}
            recs = []
            for pair in range(args.pairs):
                rec = {**base, "reg_loss": reg_loss, "beta": beta, "pair": pair}
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
                    rec[name] = median_ms(marks)
                recs.append(rec)
                print(json.dumps(rec), flush=True)
            if len(recs) > 1:
                print(json.dumps(summary("call", recs, "qfl_ms", "focal_ms", {"reg_loss": reg_loss, "beta": beta, "build_id": ident["build_id"]})), flush=True)
        return

    engines = {"qfl": make_engine("qfl", device), "focal": make_engine("focal", device)}

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
        rec = {"kind": "step", "pair": pair, "dtype": "bf16", "batch": 12, "side": 500, "reg_loss": "diou", "steps": args.steps, "build_id": ident["build_id"]}
        for name, eng in engines.items():
            run(eng, args.warmup, 0, False)
            torch.cuda.synchronize()
            marks = run(eng, args.steps, args.warmup, True)
            torch.cuda.synchronize()
            rec[f"{name}_step_ms"] = median_ms(marks)
            rec[f"{name}_img_s"] = round(12 / rec[f"{name}_step_ms"] * 1e3, 1)
        rec["finite"] = bool(all(torch.isfinite(e.flat_p).all() for e in engines.values()))
        engines["qfl"].criterion.flush_meters()
        rec["mean_iou_of_positives"] = round(float(engines["qfl"].criterion.quality_average.average), 4)
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    if len(recs) > 1:
        print(json.dumps(summary("step", recs, "qfl_step_ms", "focal_step_ms", {"build_id": ident["build_id"]})), flush=True)
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
