"""What gradient accumulation costs the fused training step (TrainEngine(accum_steps=...)) on one MI355X: two engines ALTERNATING in one
process on one box, one JSON line per pair.  Every call of step() is bracketed by device events on the training stream, and a third event is
recorded right behind the backward pass, so each micro-batch gives two times:

  * plain_fb_ms / plain_step_ms: accum_steps = 1, the bf16 training step of bench.py's headline (bs 12, 500 x 500, targets on the device) --
                                 up to the end of its backward pass, and the whole step;
  * store_ms / add_ms:           accum_steps = 4, a micro-batch that only accumulates (forward, criterion, backward, one STORE or ADD launch)
                                 -- the first of a window and the ones in between;
  * finish_ms:                   the window's last micro-batch (the same, a FINISH launch, then the tail of the plain step).

`add_extra_us` = add_ms - plain_fb_ms is what an accumulating micro-batch costs over a plain forward and backward, `finish_extra_us` =
finish_ms - plain_step_ms what a finishing one costs over a plain step.  `estimate_us` is the traffic of one launch (12 B per element of the
ranges the engine accumulates over; 8 B for STORE) at --hbm-gbs (default 4000: half the 8 TB/s peak, an assumption, not a measurement).  The
last line (`"summary"`) gives the medians next to the spread of each leg between the pairs of this job: a difference inside that spread is
noise, and the line says so.  All times are medians over the micro-batches of a leg.

Two models with the same tamed random weights (bench.py's recipe) live side by side; each leg of a pair runs --steps micro-batches behind
--warmup warm-up ones (both multiples of 4, so a leg is whole windows).  --freeze-bn times the pair on the frozen-BatchNorm step.  The
yardstick of the absolute numbers is bench.py's headline of the parent commit in the same job.
    python scripts/grad_accum_numbers.py [--pairs 3 --steps 32 --warmup 8] >> profiles/grad_accum.jsonl"""
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

ACCUM = 4


def make_engine(accum_steps, frozen, device):
    from bench import tame_init_
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as mm
    from tinyfaces.models.loss import DetectionCriterion
    torch.manual_seed(0)
    model = tame_init_(mm.DetectionModel(num_templates=25), 0).set_compute_dtype(torch.bfloat16)
    if frozen:
        model.freeze_batchnorm()
    eng = TrainEngine(model, DetectionCriterion(25, seed=0), lr=1e-4, device=device, accum_steps=accum_steps)
    run_backward = model._run_backward
    eng.behind_backward = None

    def marked(x, grad, persistent=False):
        out = run_backward(x, grad, persistent=persistent)
        if eng.behind_backward is not None:
            eng.behind_backward.record()
        return out

    model._run_backward = marked
    return eng


def median_ms(pairs):
    return round(statistics.median(a.elapsed_time(b) for a, b in pairs), 4) if pairs else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--freeze-bn", dest="freeze_bn", action="store_true")
    ap.add_argument("--hbm-gbs", dest="hbm_gbs", type=float, default=4000.0)
    args = ap.parse_args()
    if args.steps % ACCUM or args.warmup % ACCUM or args.steps <= 0:
        ap.error(f"--steps and --warmup must be multiples of {ACCUM}")
    from bench import synthetic_batch
    from tinyfaces import _hip, ops
    from tinyfaces.datasets.templates import load_templates
    device = torch.device("cuda:0")
    t_d = torch.as_tensor(load_templates(), dtype=torch.float64, device=device)
    pool = [synthetic_batch(s, 12, device, None) for s in range(4)]
    engines = {"plain": make_engine(1, args.freeze_bn, device), "accum": make_engine(ACCUM, args.freeze_bn, device)}
    walked = sum(e - s for s, e in engines["accum"]._norm_segments())
    estimate_us = round(12.0 * walked / (args.hbm_gbs * 1e9) * 1e6, 1)
    recs = []

    def run(eng, n, first, timed):
        """n micro-batches; timed: [(kind, start, behind the backward pass, end)] device events, read after the leg's synchronise."""
        marks = []
        for i in range(n):
            b = pool[(first + i) % len(pool)]
            cm, rm = ops.dense_overlap_targets_device(b["boxes"], b["offs"], b["total"], t_d, paste_d=b["paste"], seed=first + i)
            if not timed:
                eng.step(b["x"], cm, rm)
                continue
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            k = eng.pending_micro_batches
            kind = "plain" if eng.accum_steps == 1 else "store" if k == 0 else "finish" if k + 1 == eng.accum_steps else "add"
            eng.behind_backward = ev[1]
            ev[0].record()
            eng.step(b["x"], cm, rm)
            ev[2].record()
            eng.behind_backward = None
            marks.append((kind, *ev))
        return marks

    ident = _hip.identity()
    for pair in range(args.pairs):
        rec = {"pair": pair, "dtype": "bf16", "batch": 12, "side": 500, "micro_batches": args.steps, "accum_steps": ACCUM,
               "batchnorm": "frozen" if args.freeze_bn else "batch statistics", "build_id": ident["build_id"]}
        for name, eng in engines.items():
            run(eng, args.warmup, 0, False)
            torch.cuda.synchronize()
            marks = run(eng, args.steps, args.warmup, True)
            torch.cuda.synchronize()
            if name == "plain":
                rec["plain_fb_ms"] = median_ms([(m[1], m[2]) for m in marks])
                rec["plain_step_ms"] = median_ms([(m[1], m[3]) for m in marks])
            else:
                for kind in ("store", "add", "finish"):
                    rec[f"{kind}_ms"] = median_ms([(m[1], m[3]) for m in marks if m[0] == kind])
                rec["window_ms"] = round(rec["store_ms"] + (ACCUM - 2) * rec["add_ms"] + rec["finish_ms"], 4)
                rec["window_img_s"] = round(12 * ACCUM / rec["window_ms"] * 1e3, 1)
        rec["store_extra_us"] = round(1e3 * (rec["store_ms"] - rec["plain_fb_ms"]), 1)
        rec["add_extra_us"] = round(1e3 * (rec["add_ms"] - rec["plain_fb_ms"]), 1)
        rec["finish_extra_us"] = round(1e3 * (rec["finish_ms"] - rec["plain_step_ms"]), 1)
        rec["accumulated_elements"], rec["estimate_us"] = walked, estimate_us
        rec["optimizer_steps"] = {n: e.steps for n, e in engines.items()}
        rec["finite"] = bool(all(torch.isfinite(e.flat_p).all() for e in engines.values()))
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    if len(recs) > 1:
        def med(key):
            return round(statistics.median(r[key] for r in recs), 1)

        def spread(key):
            return round(1e3 * (max(r[key] for r in recs) - min(r[key] for r in recs)), 1)

        noise = max(spread(k) for k in ("plain_fb_ms", "plain_step_ms", "add_ms", "finish_ms"))
        print(json.dumps({"summary": True, "batchnorm": recs[0]["batchnorm"], "pairs": len(recs), "add_extra_us_median": med("add_extra_us"),
                          "store_extra_us_median": med("store_extra_us"), "finish_extra_us_median": med("finish_extra_us"),
                          "plain_fb_spread_us": spread("plain_fb_ms"), "plain_step_spread_us": spread("plain_step_ms"),
                          "add_spread_us": spread("add_ms"), "finish_spread_us": spread("finish_ms"), "estimate_us": estimate_us,
                          "add_inside_spread": bool(abs(med("add_extra_us")) <= noise),
                          "finish_inside_spread": bool(abs(med("finish_extra_us")) <= noise), "build_id": ident["build_id"]}), flush=True)
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
