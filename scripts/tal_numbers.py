"""What the task-aligned target assignment (ops.tal_assign_device, tf_targets_tal) costs on one MI355X, the legs ALTERNATING in one process on
one box, one JSON line per pair:

  * --step calls: device-event time of ONE call of the resident entry point on the outputs of a real forward pass (the bf16 detector with
    tamed random weights on the batch's images), median over --calls calls of each leg.  "bench" lines: the bs 12 operands bench.py builds
    (1-16 boxes of 8-200 px per image); "tiny" lines: the seeded bs 12 batch of 192 faces of 8-16 px (scripts/anchor_compensation_numbers.py:
    tiny_batch).  The yardstick is ops.atss_targets_device at k = 9 in the same pair, never an absolute figure; above 3 x the README owes
    the cause.  The base maps are refilled outside the timed region (the call only writes the won anchors).
  * --step steps: the bf16 bs 12 500 x 500 training step of bench.py's headline with qfl + diou: an engine fed ATSS maps (assigned in front of
    the timed region, as a loader does while the previous step runs) alternates with an engine that assigns by TAL inside its step; median
    over --steps steps behind --warmup warm-up ones.  The difference is all on the critical path of the step.
  * --step epochs: main.py on synthetic-faces for two epochs under --assigner atss and under --assigner tal (qfl + diou), each in a child
    process: the last mean IoU of the positives and the summed match-count lines.  Figures about pasted faces, no accuracy claim.

    python scripts/tal_numbers.py --step calls [--pairs 5 --calls 200] >> profiles/tal.jsonl"""
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


def make_engine(assign, device):
    from bench import tame_init_
    from tinyfaces.datasets.templates import load_templates
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as mm
    from tinyfaces.models.loss import DetectionCriterion, TaskAligned
    torch.manual_seed(0)
    model = tame_init_(mm.DetectionModel(num_templates=25), 0).set_compute_dtype(torch.bfloat16)
    crit = DetectionCriterion(25, seed=0, cls_loss="qfl", reg_loss="diou", templates=load_templates(), lazy_meters=True,
                              assigner=TaskAligned() if assign else None)
    return TrainEngine(model, crit, lr=1e-4, device=device)


def median_ms(pairs):
    return round(statistics.median(a.elapsed_time(b) for a, b in pairs), 4)


def forward_output(eng, x):
    """The head's output for x as TrainEngine.step sees it (one step of `eng` with the forward tapped)."""
    got = []
    fwd = eng.model._run_forward
    eng.model._run_forward = lambda x, training=True: (lambda o: (got.append(o.detach().float().clone()), o)[1])(fwd(x, training=training))
    return got, fwd


def epochs(args):
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for assigner in ("atss", "tal"):
        with tempfile.TemporaryDirectory() as tmp:
            r = subprocess.run([sys.executable, os.path.join(PKG, "main.py"), "synthetic-faces", "synthetic-faces", "--epochs", "2", "--save-every", "10",
                                "--synthetic-len", "32", "--batch_size", "4", "--lr", "1e-4", "--cls-loss", "qfl", "--reg-loss", "diou", "--assigner", assigner],
                               cwd=tmp, capture_output=True, text=True, timeout=280, env=env)
        if r.returncode != 0:
            print(json.dumps({"kind": "epochs", "assigner": assigner, "error": r.stderr[-400:]}), flush=True)
            raise SystemExit(r.returncode)
        iou = re.findall(r"mean IoU of positives ([0-9.eE+-]+) \((\d+) positives\)", r.stdout)
        counts = re.findall(r"(?:ATSS|TAL): (\d+) of (\d+) faces won at most 3 positives, (\d+) of them none", r.stdout)
        print(json.dumps({"kind": "epochs", "assigner": assigner, "epochs": 2, "images": 32, "batch": 4, "lr": 1e-4, "cls_loss": "qfl", "reg_loss": "diou",
                          "mean_iou_of_positives_last": float(iou[-1][0]) if iou else None, "positives_seen": int(iou[-1][1]) if iou else 0,
                          "faces": sum(int(c[1]) for c in counts), "faces_with_at_most_3_positives": sum(int(c[0]) for c in counts),
                          "faces_without_positive": sum(int(c[2]) for c in counts)}), flush=True)


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
        eng.step(b0["x"], *ops.atss_targets_device(b0["boxes"], b0["offs"], b0["total"], t_d, paste_d=b0["paste"]))
        eng.model._run_forward = fwd
        out = got[0].contiguous()
        for kind, b in (("bench", b0), ("tiny", tiny_batch(device))):
            base = (torch.full((12, 25, 63, 63), -1.0, device=device), torch.zeros(12, 100, 63, 63, device=device))
            maps = (torch.empty_like(base[0]), torch.empty_like(base[1]))

            def tal(topk=13):
                return ops.tal_assign_device(out, maps[0], maps[1], b["boxes"], b["offs"], b["total"], t_d, paste_d=b["paste"], topk=topk)

            def atss():
                return ops.atss_targets_device(b["boxes"], b["offs"], b["total"], t_d, paste_d=b["paste"], topk=9, out=maps)

            legs = [("atss_k9", atss, False), ("tal_k13", tal, True), ("tal_k32", lambda: tal(32), True)]
            maps[0].copy_(base[0]); maps[1].copy_(base[1])
            _, _, mc = ops.tal_assign_device(out, maps[0], maps[1], b["boxes"], b["offs"], b["total"], t_d, paste_d=b["paste"], return_match_count=True)
            facts = {"faces": int(b["total"]), "positives_tal_k13": int((maps[0] == 1).sum()), "faces_without_positive_tal_k13": int((mc == 0).sum()),
                     "positives_atss_k9": int((atss()[0] == 1).sum())}
            recs = []
            for pair in range(args.pairs):
                rec = {"kind": kind, "pair": pair, "batch": 12, "map": [25, 63, 63], "calls": args.calls, "build_id": ident["build_id"], **facts}
                for name, call, refill in legs:
                    for _ in range(8):
                        call()
                    torch.cuda.synchronize()
                    marks = []
                    for _ in range(args.calls):
                        if refill:
                            maps[0].copy_(base[0]); maps[1].copy_(base[1])
                        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                        ev[0].record()
                        call()
                        ev[1].record()
                        marks.append(ev)
                    torch.cuda.synchronize()
                    rec[f"{name}_us"] = round(1e3 * statistics.median(x.elapsed_time(y) for x, y in marks), 1)
                recs.append(rec)
                print(json.dumps(rec), flush=True)
            if len(recs) > 1:
                s = {"summary": True, "kind": kind, "pairs": len(recs), "build_id": ident["build_id"]}
                for name, _, _ in legs:
                    vals = [r[f"{name}_us"] for r in recs]
                    s[f"{name}_us_median"], s[f"{name}_us_spread"] = round(statistics.median(vals), 1), round(max(vals) - min(vals), 1)
                    if name != "atss_k9":
                        s[f"{name}_ratio_to_atss_k9_median"] = round(statistics.median(r[f"{name}_us"] / r["atss_k9_us"] for r in recs), 2)
                print(json.dumps(s), flush=True)
        eng.close()
        return

    engines = {"atss": make_engine(False, device), "tal": make_engine(True, device)}

    def run(name, eng, n, first, timed):
        marks = []
        for i in range(n):
            b = pool[(first + i) % len(pool)]
            if name == "atss":
                c, r = ops.atss_targets_device(b["boxes"], b["offs"], b["total"], t_d, paste_d=b["paste"])
                faces = None
            else:
                c, r = torch.full((12, 25, 63, 63), -1.0, device=device), torch.zeros(12, 100, 63, 63, device=device)
                faces = ResidentFaces(b["boxes"], b["offs"], b["total"], b["paste"])
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            if faces is None:
                eng.step(b["x"], c, r)
            else:
                eng.step_with_faces(b["x"], c, r, faces)
            ev[1].record()
            if timed:
                marks.append(ev)
        return marks

    recs = []
    for pair in range(args.pairs):
        rec = {"kind": "step", "pair": pair, "dtype": "bf16", "batch": 12, "side": 500, "cls_loss": "qfl", "reg_loss": "diou", "steps": args.steps,
               "build_id": ident["build_id"]}
        for name, eng in engines.items():
            run(name, eng, args.warmup, 0, False)
            torch.cuda.synchronize()
            marks = run(name, eng, args.steps, args.warmup, True)
            torch.cuda.synchronize()
            rec[f"{name}_step_ms"] = median_ms(marks)
            rec[f"{name}_img_s"] = round(12 / rec[f"{name}_step_ms"] * 1e3, 1)
            eng.criterion.flush_meters()
            rec[f"{name}_mean_iou_of_positives"] = round(float(eng.criterion.quality_average.average), 4)
        rec["finite"] = bool(all(torch.isfinite(e.flat_p).all() for e in engines.values()))
        recs.append(rec)
        print(json.dumps(rec), flush=True)
    if len(recs) > 1:
        spread = lambda key: round(1e3 * (max(r[key] for r in recs) - min(r[key] for r in recs)), 1)
        diff = statistics.median(1e3 * (r["tal_step_ms"] - r["atss_step_ms"]) for r in recs)
        ma, mb = statistics.median(r["tal_step_ms"] for r in recs), statistics.median(r["atss_step_ms"] for r in recs)
        print(json.dumps({"summary": True, "kind": "step", "pairs": len(recs), "tal_step_ms_median": round(ma, 4), "atss_step_ms_median": round(mb, 4),
                          "tal_step_ms_spread_us": spread("tal_step_ms"), "atss_step_ms_spread_us": spread("atss_step_ms"),
                          "tal_minus_atss_us_median": round(diff, 1), "share_of_the_tal_step_percent": round(100.0 * diff / (1e3 * ma), 2),
                          "build_id": ident["build_id"]}), flush=True)
    for eng in engines.values():
        eng.close()


if __name__ == "__main__":
    main()
