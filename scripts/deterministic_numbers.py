"""What the deterministic mode costs on one MI355X (TrainEngine(deterministic=True); tf_conv2d_wgrad_det, tf_stem_wgrad_det), one JSON line per
measurement -> profiles/deterministic.jsonl.  bf16, bs 12, 500 x 500, the headline configuration of bench.py.

  --step engine [--freeze-bn]   a default and a deterministic engine ALTERNATING in one process, --pairs pairs of legs, every step() bracketed
                                by device events on the training stream; per pair the median step of both legs and the cost of the mode against
                                the default leg of the SAME pair; a last "summary" line with the medians and the spread of each leg between
                                the pairs (a difference inside that spread is noise).  The deterministic leg pays for three things at once:
                                unfolded BatchNorm statistic rows (separate finalize kernels, no fused epilogues), the loss of the grouped
                                and direct-stem launches that depend on folded rows, and the slab form of the weight gradients.
                                Before the first pair the deterministic engine's flat gradient is checked to repeat bit for bit.
  --step shapes                 the distinct weight-gradient shapes of that step one by one, back-to-back launches between two device events:
                                the atomic form (tf_conv2d_wgrad as the default step calls it: the all-taps kernel with its partial workspace)
                                against the slab form (tf_conv2d_wgrad_det, preferred slab).  A shape whose slab form is not slower is a
                                candidate for a later change of default.

    python scripts/deterministic_numbers.py --step engine >> profiles/deterministic.jsonl"""
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

N = 12
SHAPES = [  # name, launches per batch-statistics step (ResNet-101), H, W, OH, OW, Cin, Cout, K, stride, ldx, lddy
    ("stem im2col 147->64", 1, 1, N * 250 * 250, 1, N * 250 * 250, 147, 64, 1, 1, 192, 64),      # one image of N * 250 * 250 rows: the executor's call
    ("l1.c1 64->64", 1, 125, 125, 125, 125, 64, 64, 1, 1, 64, 64), ("l1.c1 256->64", 2, 125, 125, 125, 125, 256, 64, 1, 1, 256, 64),
    ("l1.c2 3x3 64", 3, 125, 125, 125, 125, 64, 64, 3, 1, 64, 64), ("l1.c3/ds 64->256", 4, 125, 125, 125, 125, 64, 256, 1, 1, 64, 256),
    ("l2.c1 256->128", 1, 125, 125, 125, 125, 256, 128, 1, 1, 256, 128), ("l2.c2 3x3 s2", 1, 125, 125, 63, 63, 128, 128, 3, 2, 128, 128),
    ("l2.ds 256->512 s2", 1, 125, 125, 63, 63, 256, 512, 1, 2, 256, 512), ("l2.c1 512->128", 3, 63, 63, 63, 63, 512, 128, 1, 1, 512, 128),
    ("l2.c2 3x3 128", 3, 63, 63, 63, 63, 128, 128, 3, 1, 128, 128), ("l2.c3 128->512", 4, 63, 63, 63, 63, 128, 512, 1, 1, 128, 512),
    ("l3.c1 512->256", 1, 63, 63, 63, 63, 512, 256, 1, 1, 512, 256), ("l3.c2 3x3 s2", 1, 63, 63, 32, 32, 256, 256, 3, 2, 256, 256),
    ("l3.ds 512->1024 s2", 1, 63, 63, 32, 32, 512, 1024, 1, 2, 512, 1024), ("l3.c3 256->1024", 23, 32, 32, 32, 32, 256, 1024, 1, 1, 256, 1024),
    ("l3.c1 1024->256", 22, 32, 32, 32, 32, 1024, 256, 1, 1, 1024, 256), ("l3.c2 3x3 256", 22, 32, 32, 32, 32, 256, 256, 3, 1, 256, 256),
    ("head3 512->125", 1, 63, 63, 63, 63, 512, 125, 1, 1, 512, 128), ("head4 1024->125", 1, 32, 32, 32, 32, 1024, 125, 1, 1, 1024, 128),
]


def make_engine(deterministic, frozen, device):
    from bench import tame_init_
    from tinyfaces.engine import TrainEngine
    from tinyfaces.models import model as mm
    from tinyfaces.models.loss import DetectionCriterion
    torch.manual_seed(0)
    model = tame_init_(mm.DetectionModel(num_templates=25), 0).set_compute_dtype(torch.bfloat16)
    if frozen:
        model.freeze_batchnorm()
    return TrainEngine(model, DetectionCriterion(25, seed=0), lr=1e-4, device=device, deterministic=deterministic)


def step_engine(args):
    from bench import synthetic_batch
    from tinyfaces import _hip, ops
    from tinyfaces.datasets.templates import load_templates
    device = torch.device("cuda:0")
    t_d = torch.as_tensor(load_templates(), dtype=torch.float64, device=device)
    pool = [synthetic_batch(s, N, device, None) for s in range(4)]
    engines = {"default": make_engine(False, args.freeze_bn, device), "deterministic": make_engine(True, args.freeze_bn, device)}
    ident = _hip.identity()
    bn = "frozen" if args.freeze_bn else "batch statistics"

    def batch(i):
        b = pool[i % len(pool)]
        cm, rm = ops.dense_overlap_targets_device(b["boxes"], b["offs"], b["total"], t_d, paste_d=b["paste"], seed=i)
        return b["x"], cm, rm

    # the claim itself, at the size that is timed: forward + backward of the deterministic engine's model twice on one batch
    eng = engines["deterministic"]
    m, crit = eng.model, eng.criterion
    x, cm, rm = batch(0)
    # (the soft-margin criterion draws new samples on every call: the upstream gradient of the first pass feeds both backward passes)
    grads, outs, upstream = [], [], None
    prev = ops.set_deterministic(True)
    try:
        for _ in range(2):
            m._sync_tables(x.device)
            outs.append(m._run_forward(x, training=True).clone())
            if upstream is None:
                _, grad, _ = crit._fwd_bwd(outs[0], cm.clone(), rm)
                upstream = grad.clone()
                if hasattr(crit, "_pending"):
                    crit._pending.clear()
            grads.append(m._run_backward(x, upstream, persistent=True).clone())
    finally:
        ops.set_deterministic(prev)
    torch.cuda.synchronize()
    differing = int((grads[0].view(torch.int32) != grads[1].view(torch.int32)).sum())
    print(json.dumps({"check": "two forward + backward passes over one batch and one upstream gradient, switch on", "batchnorm": bn,
                      "outputs_equal": bool(torch.equal(outs[0], outs[1])), "gradient_elements": grads[0].numel(), "gradient_elements_differing": differing,
                      "gradient_nonzero": int((grads[0] != 0).sum()), "build_id": ident["build_id"]}), flush=True)
    del grads, outs, upstream

    def run(eng, n, first, timed):
        marks = []
        for i in range(n):
            x, cm, rm = batch(first + i)
            if not timed:
                eng.step(x, cm, rm)
                continue
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.step(x, cm, rm)
            b.record()
            marks.append((a, b))
        return marks

    recs = []
    for pair in range(args.pairs):
        rec = {"pair": pair, "dtype": "bf16", "batch": N, "side": 500, "steps": args.steps, "batchnorm": bn, "build_id": ident["build_id"]}
        for name, eng in engines.items():
            run(eng, args.warmup, 0, False)
            torch.cuda.synchronize()
            marks = run(eng, args.steps, args.warmup, True)
            torch.cuda.synchronize()
            ms = sorted(a.elapsed_time(b) for a, b in marks)
            rec[f"{name}_step_ms"] = round(statistics.median(ms), 4)
            rec[f"{name}_img_s"] = round(N / statistics.median(ms) * 1e3, 1)
        rec["cost_ms"] = round(rec["deterministic_step_ms"] - rec["default_step_ms"], 4)
        rec["cost_pct"] = round(100.0 * rec["cost_ms"] / rec["default_step_ms"], 2)
        rec["finite"] = bool(all(torch.isfinite(e.flat_p).all() for e in engines.values()))
        recs.append(rec)
        print(json.dumps(rec), flush=True)

    def spread(key):
        return round(max(r[key] for r in recs) - min(r[key] for r in recs), 4)

    print(json.dumps({"summary": True, "batchnorm": bn, "pairs": len(recs),
                      "default_step_ms_median": round(statistics.median(r["default_step_ms"] for r in recs), 4),
                      "deterministic_step_ms_median": round(statistics.median(r["deterministic_step_ms"] for r in recs), 4),
                      "cost_pct_median": round(statistics.median(r["cost_pct"] for r in recs), 2),
                      "default_spread_ms": spread("default_step_ms"), "deterministic_spread_ms": spread("deterministic_step_ms"),
                      "build_id": ident["build_id"]}), flush=True)
    for eng in engines.values():
        eng.close()


def timeit(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3


def step_shapes(args):
    from tinyfaces import _hip, ops
    ident = _hip.identity()
    dt = torch.bfloat16
    tot = {"atomic": 0.0, "slab": 0.0}
    for name, n, H, W, OH, OW, Cin, Cout, K, s, ldx, lddy in SHAPES:
        nn = 1 if name.startswith("stem") else N
        x = torch.randn(nn, H, W, ldx, device="cuda").to(dt)
        gy = torch.randn(nn, OH, OW, lddy, device="cuda").to(dt)
        out = torch.zeros(Cout, Cin, K, K, device="cuda")
        two = K == 3 and s == 1
        atomic = [timeit(lambda: ops.conv2d_wgrad(x, gy, Cin, Cout, K, K, s, K // 2, out=out, two_phase=two), args.reps) for _ in range(args.repeats)]
        slab = [timeit(lambda: ops.conv2d_wgrad(x, gy, Cin, Cout, K, K, s, K // 2, out=out, deterministic=True), args.reps) for _ in range(args.repeats)]
        rec = {"shape": name, "launches_per_step": n, "M": nn * OH * OW, "Cin": Cin, "Cout": Cout, "K": K, "stride": s,
               "atomic_us": round(statistics.median(atomic), 1), "slab_us": round(statistics.median(slab), 1),
               "atomic_spread_us": round(max(atomic) - min(atomic), 1), "slab_spread_us": round(max(slab) - min(slab), 1),
               "slab_bytes": ops.wgrad_det_workspace_bytes(x, gy, Cin, Cout, K, K, s, K // 2), "build_id": ident["build_id"]}
        rec["slab_over_atomic"] = round(rec["slab_us"] / rec["atomic_us"], 3)
        rec["slab_not_slower"] = bool(rec["slab_us"] <= rec["atomic_us"] + max(rec["atomic_spread_us"], rec["slab_spread_us"]))
        tot["atomic"] += rec["atomic_us"] * n
        tot["slab"] += rec["slab_us"] * n
        print(json.dumps(rec), flush=True)
    print(json.dumps({"summary": "weight-gradient shapes, launches per step weighted", "atomic_us": round(tot["atomic"], 1), "slab_us": round(tot["slab"], 1),
                      "note": "stand-alone launches: in the step they overlap the data-gradient chain on a second stream", "build_id": ident["build_id"]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["engine", "shapes"], default="engine")
    ap.add_argument("--pairs", type=int, default=4)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--freeze-bn", dest="freeze_bn", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("deterministic_numbers.py measures on an MI355X: no GPU, no number")
    if args.pairs < 1 or args.steps < 1:
        ap.error("--pairs and --steps must be >= 1")
    (step_engine if args.step == "engine" else step_shapes)(args)


if __name__ == "__main__":
    main()
