"""What TOOD's task-aligned loss (TaskAligned(aligned_targets=True): tf_targets_tal_aligned + tf_criterion_aligned_fwd_bwd) costs on one MI355X
next to TAL + qfl, the legs ALTERNATING in one process on one box, one JSON line per pair (scripts/tal_numbers.py's method):

  * --step calls: device-event time of ONE call, median over --calls calls of each leg.  Assigner: ops.tal_assign_device with align_out against
    the plain call of the same pair, on the outputs of a real forward pass, for the bs 12 operands bench.py builds ("bench") and for the seeded
    bs 12 batch of 192 faces of 8-16 px ("tiny"); the added work is one fp32 store per anchor in the clear launch (4.8 MB at bs 12) plus a few
    bytes per winner.  Criterion: ops.criterion_aligned_fwd_bwd against ops.criterion_quality_fwd_bwd of the same reg_loss on the maps that
    assignment made; it reads one more fp32 per positive.  The base maps are refilled outside the timed region.
  * --step steps: the bf16 bs 12 500 x 500 training step of bench.py's headline with TAL + qfl + diou: an engine with aligned targets and
    focal_normalize="align" alternates with an engine without; median over --steps steps behind --warmup warm-up ones.
  * --step epochs: main.py on synthetic-faces for two epochs with --assigner tal --cls-loss qfl --reg-loss diou, without and with
    --tal-aligned-targets --focal-normalize align, each in a child process: the last quality line and the summed match-count lines.  Figures
    about pasted faces, no accuracy claim.

    python scripts/tal_aligned_numbers.py --step calls [--pairs 5 --calls 200] >> profiles/tal_aligned.jsonl"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tiny-faces-pytorch_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)


def make_engine(aligned, device):
    from bench import tame_init_
    from tinyfaces.datasets.templates import load_templates
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as mm
    from tinyfaces.models.loss import DetectionCriterion, TaskAligned
    torch.manual_seed(0)
    model = tame_init_(mm.DetectionModel(num_templates=25), 0).set_compute_dtype(torch.bfloat16)
    crit = DetectionCriterion(25, seed=0, cls_loss="qfl", reg_loss="diou", templates=load_templates(), lazy_meters=True,
                              focal_normalize="align" if aligned else "pos", assigner=TaskAligned(aligned_targets=aligned))
    return TrainEngine(model, crit, lr=1e-4, device=device)


def epochs(args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for aligned in (False, True):
        more = ["--tal-aligned-targets", "--focal-normalize", "align"] if aligned else []
        with tempfile.TemporaryDirectory() as tmp:
            r = subprocess.run([sys.executable, os.path.join(PKG, "main.py"), "synthetic-faces", "synthetic-faces", "--epochs", "2", "--save-every", "10",
                                "--synthetic-len", "32", "--batch_size", "4", "--lr", "1e-4", "--cls-loss", "qfl", "--reg-loss", "diou", "--assigner", "tal"] + more,
                               cwd=tmp, capture_output=True, text=True, timeout=280, env=env)
        if r.returncode != 0:
            print(json.dumps({"kind": "epochs", "aligned_targets": aligned, "error": r.stderr[-400:]}), flush=True)
            raise SystemExit(r.returncode)
        q = re.findall(r"mean (IoU|aligned target) of positives ([0-9.eE+-]+) \((\d+) positives\)", r.stdout)
        counts = re.findall(r"TAL: (\d+) of (\d+) faces won at most 3 positives, (\d+) of them none", r.stdout)
        print(json.dumps({"kind": "epochs", "aligned_targets": aligned, "epochs": 2, "images": 32, "batch": 4, "lr": 1e-4, "cls_loss": "qfl", "reg_loss": "diou",
                          "quality_line": f"mean {q[-1][0]} of positives" if q else None, "quality_last": float(q[-1][1]) if q else None,
                          "positives_seen": int(q[-1][2]) if q else 0, "faces": sum(int(c[1]) for c in counts),
                          "faces_with_at_most_3_positives": sum(int(c[0]) for c in counts), "faces_without_positive": sum(int(c[2]) for c in counts)}), flush=True)


def timed(call, calls, refill=None):
    for _ in range(8):
        call()
    torch.cuda.synchronize()
    marks = []
    for _ in range(calls):
        if refill is not None:
            refill()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        call()
        ev[1].record()
        marks.append(ev)
    torch.cuda.synchronize()
    return round(1e3 * statistics.median(x.elapsed_time(y) for x, y in marks), 1)


def summary(recs, kind, a, b, ident, **more):
    s = {"summary": True, "kind": kind, "pairs": len(recs), "build_id": ident["build_id"], **more}
    for name in (a, b):
        vals = [r[f"{name}_us"] for r in recs]
        s[f"{name}_us_median"], s[f"{name}_us_spread"] = round(statistics.median(vals), 1), round(max(vals) - min(vals), 1)
    diffs = [r[f"{a}_us"] - r[f"{b}_us"] for r in recs]
    s[f"{a}_minus_{b}_us_median"], s[f"{a}_minus_{b}_us_spread"] = round(statistics.median(diffs), 1), round(max(diffs) - min(diffs), 1)
    s[f"{a}_ratio_to_{b}_median"] = round(statistics.median(r[f"{a}_us"] / r[f"{b}_us"] for r in recs), 3)
    print(json.dumps(s), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["calls", "steps", "epochs"], required=True)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=6)
    args = ap.parse_args()
    if args.step == "epochs":
        return epochs(args)
    from anchor_compensation_numbers import tiny_batch
    from bench import synthetic_batch
    from tal_numbers import forward_output, median_ms
    from tinyfaces import _hip, ops
    from tinyfaces.datasets.targets import ResidentFaces
    from tinyfaces.datasets.templates import load_templates
    device = torch.device("cuda:0")
    ident = _hip.identity()
    t_d = torch.as_tensor(load_templates(), dtype=torch.float64, device=device)
    pool = [synthetic_batch(s, 12, device, None) for s in range(4)]

    if args.step == "calls":
        eng = make_engine(False, device)
        got, fwd = forward_output(eng, None)
        b0 = pool[0]
        eng.step_with_faces(b0["x"], torch.full((12, 25, 63, 63), -1.0, device=device), torch.zeros(12, 100, 63, 63, device=device),
                            ResidentFaces(b0["boxes"], b0["offs"], b0["total"], b0["paste"]))
        eng.model._run_forward = fwd
        out = got[0].contiguous()
        twh = ops.template_wh(load_templates()).to(device)
        for kind, b in (("bench", b0), ("tiny", tiny_batch(device))):
            base = (torch.full((12, 25, 63, 63), -1.0, device=device), torch.zeros(12, 100, 63, 63, device=device))
            maps = (torch.empty_like(base[0]), torch.empty_like(base[1]))
            align = torch.empty_like(base[0])

            def refill():
                maps[0].copy_(base[0]); maps[1].copy_(base[1])

            def plain():
                return ops.tal_assign_device(out, maps[0], maps[1], b["boxes"], b["offs"], b["total"], t_d, paste_d=b["paste"])

            def aligned():
                return ops.tal_assign_device(out, maps[0], maps[1], b["boxes"], b["offs"], b["total"], t_d, paste_d=b["paste"], align_out=align)

            refill()
            aligned()
            pos = maps[0] == 1
            facts = {"faces": int(b["total"]), "positives": int(pos.sum()), "mean_target": round(float(align[pos].mean()), 4) if bool(pos.any()) else None,
                     "anchors": int(maps[0].numel())}
            recs = []
            for pair in range(args.pairs):
                rec = {"kind": f"assign_{kind}", "pair": pair, "batch": 12, "map": [25, 63, 63], "calls": args.calls, "build_id": ident["build_id"], **facts}
                rec["tal_us"] = timed(plain, args.calls, refill)
                rec["tal_aligned_us"] = timed(aligned, args.calls, refill)
                recs.append(rec)
                print(json.dumps(rec), flush=True)
            summary(recs, f"assign_{kind}", "tal_aligned", "tal", ident, align_map_bytes=4 * int(maps[0].numel()))
            # the criterion on the maps this assignment made
            refill()
            aligned()
            grad = torch.empty_like(out)
            for reg_loss in ("smooth_l1", "diou"):
                recs = []
                for pair in range(args.pairs):
                    rec = {"kind": f"criterion_{kind}_{reg_loss}", "pair": pair, "batch": 12, "calls": args.calls, "build_id": ident["build_id"], **facts}
                    rec["qfl_us"] = timed(lambda: ops.criterion_quality_fwd_bwd(out, maps[0], maps[1], 25, 1.0, 2.0, "pos", reg_loss, twh, grad=grad), args.calls)
                    rec["aligned_us"] = timed(lambda: ops.criterion_aligned_fwd_bwd(out, maps[0], maps[1], align, 25, 1.0, 2.0, "align", reg_loss, twh, grad=grad),
                                              args.calls)
                    recs.append(rec)
                    print(json.dumps(rec), flush=True)
                summary(recs, f"criterion_{kind}_{reg_loss}", "aligned", "qfl", ident)
        eng.close()
        return

    engines = {"tal_qfl": make_engine(False, device), "tal_aligned": make_engine(True, device)}

    def run(eng, n, first, keep):
        marks = []
        for i in range(n):
            b = pool[(first + i) % len(pool)]
            c, r = torch.full((12, 25, 63, 63), -1.0, device=device), torch.zeros(12, 100, 63, 63, device=device)
            faces = ResidentFaces(b["boxes"], b["offs"], b["total"], b["paste"])
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            eng.step_with_faces(b["x"], c, r, faces)
            ev[1].record()
            if keep:
                marks.append(ev)
        return marks

    recs = []
    for pair in range(args.pairs):
        rec = {"kind": "step", "pair": pair, "dtype": "bf16", "batch": 12, "side": 500, "cls_loss": "qfl", "reg_loss": "diou", "steps": args.steps,
               "build_id": ident["build_id"]}
        for name, eng in engines.items():
            run(eng, args.warmup, 0, False)
            torch.cuda.synchronize()
            marks = run(eng, args.steps, args.warmup, True)
            torch.cuda.synchronize()
            rec[f"{name}_step_ms"] = median_ms(marks)
            rec[f"{name}_img_s"] = round(12 / rec[f"{name}_step_ms"] * 1e3, 1)
            eng.criterion.flush_meters()
            rec[f"{name}_quality_average"] = round(float(eng.criterion.quality_average.average), 4)
        rec["finite"] = bool(all(torch.isfinite(e.flat_p).all() for e in engines.values()))
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    if len(recs) > 1:
        spread = lambda key: round(1e3 * (max(r[key] for r in recs) - min(r[key] for r in recs)), 1)
        diffs = [1e3 * (r["tal_aligned_step_ms"] - r["tal_qfl_step_ms"]) for r in recs]
        ma, mb = statistics.median(r["tal_aligned_step_ms"] for r in recs), statistics.median(r["tal_qfl_step_ms"] for r in recs)
        print(json.dumps({"summary": True, "kind": "step", "pairs": len(recs), "tal_aligned_step_ms_median": round(ma, 4), "tal_qfl_step_ms_median": round(mb, 4),
                          "tal_aligned_step_ms_spread_us": spread("tal_aligned_step_ms"), "tal_qfl_step_ms_spread_us": spread("tal_qfl_step_ms"),
                          "aligned_minus_qfl_us_median": round(statistics.median(diffs), 1), "aligned_minus_qfl_us_min_max": [round(min(diffs), 1), round(max(diffs), 1)],
                          "share_of_the_step_percent": round(100.0 * statistics.median(diffs) / (1e3 * ma), 2), "build_id": ident["build_id"]}), flush=True)
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
