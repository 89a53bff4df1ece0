"""What Matrix NMS costs on one MI355X, one JSON line per measurement (profiles/matrix_nms.jsonl), and its parity against the numpy restatement
(profiles/matrix_nms_parity.txt):

  --step kernels   tf_matrix_nms_f64 next to tf_nms_f64 (the yardstick) and tf_soft_nms_f64 (uncapped, and capped at max_keep = 750) on the
                   65 536-candidate clustered list scripts/soft_nms_numbers.py times (tests/vote_ref.py: clustered_boxes), both methods of
                   either at score_thresh 0.001, iou_thresh 0.3, sigma 0.5, sigmoid scores.  Device events around every call, warm-up first,
                   the legs ALTERNATING in one process, median of --iters (5) rounds.  `rank_ms` is the matrix call at a score_thresh nobody
                   passes (2.0: admission, both rank passes and pair passes that return at once), `pair_ms` the difference to the full call:
                   the two all-pairs passes.  The kept counts at score_thresh 0.001 and 0.3 come from calls outside the timing.
                   `same_bits`: every round returned the same bytes.  The last line says whether the expectation the feature was proposed
                   with holds: several times faster than uncapped Soft-NMS, within a small multiple of the hard NMS.
  --step parity    the kernels against tests/matrix_nms_ref.py at n = 4 097 and 5 000 (gaussian and linear on logits; linear on
                   probabilities): kept indices equal, largest relative score deviation, the bound soft_nms_ref.score_bound(1) and the
                   reference's two margins.
  --step pyramid   evaluation.get_detections(pyramid_on_gpu=True) on bench.py's 1280 x 960 end-to-end image, scales (-1, 0, 1), bf16, inside one
                   constant_weights() session: plain, soft_nms="linear", "matrix_linear", "matrix_gaussian" -- ALTERNATING, median of --runs.

    bash scripts/gpu_job.sh matrix-nms      (one process and one time limit per step) -> profiles/matrix_nms.jsonl, profiles/matrix_nms_parity.txt"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tiny-faces-pytorch_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def kernels(args, ident):
    import vote_ref
    from tinyfaces import ops
    n = args.n
    boxes, scores = vote_ref.clustered_boxes(n, seed=n)
    b, s = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
    variants = {"nms": lambda: ops.nms(b, s, 0.3)}
    for method in ("linear", "gaussian"):
        variants[f"soft_{method}"] = lambda method=method: ops.soft_nms(b, s, method, 0.3, 0.5, 0.001)
        variants[f"soft_{method}_cap750"] = lambda method=method: ops.soft_nms_capped(b, s, 750, method, 0.3, 0.5, 0.001)
        variants[f"matrix_{method}"] = lambda method=method: ops.matrix_nms(b, s, method, 0.5, 0.001)
        variants[f"matrix_{method}_rank"] = lambda method=method: ops.matrix_nms(b, s, method, 0.5, 2.0)
    times, outs, same = {k: [] for k in variants}, {}, {}
    for it in range(args.iters + 2):
        for name, fn in variants.items():
            ms, out = _timed(fn)
            times[name].append(ms)
            if name in outs and name != "nms":
                same[name] = same.get(name, True) and torch.equal(out[0], outs[name][0]) and torch.equal(out[1], outs[name][1])
            outs[name] = out
    med = {k: float(np.median(v[2:])) for k, v in times.items()}
    lo = {k: float(np.min(v[2:])) for k, v in times.items()}
    kept03 = {"nms": int(outs["nms"].numel())}
    for method in ("linear", "gaussian"):
        kept03[f"soft_{method}"] = int(ops.soft_nms(b, s, method, 0.3, 0.5, 0.3)[0].numel())
        kept03[f"matrix_{method}"] = int(ops.matrix_nms(b, s, method, 0.5, 0.3)[0].numel())
    print(json.dumps({"step": "kernels", "variant": "nms", "n": n, "iou_thresh": 0.3, "kept": int(outs["nms"].numel()), "iters": args.iters,
                      "ms": round(med["nms"], 4), "min_ms": round(lo["nms"], 4), "build_id": ident["build_id"]}), flush=True)
    for method in ("linear", "gaussian"):
        for name in (f"soft_{method}", f"soft_{method}_cap750"):
            print(json.dumps({"step": "kernels", "variant": name, "method": method, "n": n, "iou_thresh": 0.3, "sigma": 0.5, "score_thresh": 0.001,
                              "kept": int(outs[name][0].numel()), "kept_at_0.3": kept03.get(name), "iters": args.iters, "ms": round(med[name], 4),
                              "min_ms": round(lo[name], 4), "over_nms": round(med[name] / med["nms"], 3), "same_bits": bool(same[name]),
                              "build_id": ident["build_id"]}), flush=True)
    for method in ("linear", "gaussian"):
        name = f"matrix_{method}"
        kept = outs[name][1]
        print(json.dumps({"step": "kernels", "variant": name, "method": method, "n": n, "sigma": 0.5, "score_thresh": 0.001,
                          "kept": int(outs[name][0].numel()), "kept_at_0.3": kept03[name], "iters": args.iters, "ms": round(med[name], 4),
                          "min_ms": round(lo[name], 4), "rank_ms": round(med[name + "_rank"], 4), "pair_ms": round(med[name] - med[name + "_rank"], 4),
                          "over_nms": round(med[name] / med["nms"], 3), "soft_uncapped_over_this": round(med[f"soft_{method}"] / med[name], 2),
                          "soft_cap750_over_this": round(med[f"soft_{method}_cap750"] / med[name], 2),
                          "scores_non_increasing": bool((kept[1:] <= kept[:-1]).all()), "same_bits": bool(same[name]),
                          "workspace_bytes": int(ops.lib().tf_matrix_nms_workspace_bytes(n)), "soft_workspace_bytes": int(ops.lib().tf_soft_nms_workspace_bytes(n)),
                          "build_id": ident["build_id"]}), flush=True)
    worst = max(med["matrix_linear"], med["matrix_gaussian"])
    faster = min(med["soft_linear"], med["soft_gaussian"]) / worst
    multiple = worst / med["nms"]
    met = faster >= 3.0 and multiple <= 4.0
    print(json.dumps({"step": "kernels", "variant": "expectation", "text": "several times (>= 3x) faster than uncapped Soft-NMS and within a small multiple "
                      "(<= 4x) of the hard NMS", "uncapped_soft_over_matrix_at_least": round(faster, 2), "matrix_over_nms_at_most": round(multiple, 3),
                      "verdict": "met" if met else "not met", "build_id": ident["build_id"]}), flush=True)


def parity(args, ident):
    import matrix_nms_ref
    import soft_nms_ref
    import vote_ref
    from tinyfaces import ops
    bound = soft_nms_ref.score_bound(1)
    print(f"# Matrix NMS kernels against tests/matrix_nms_ref.py, clustered_boxes(n, seed=n), sigma 0.5, score_thresh 0.001; bound = score_bound(1) = "
          f"{bound:.3e}; build {ident['build_id']}")
    worst = 0.0
    for n in (4097, 5000):
        boxes, scores = vote_ref.clustered_boxes(n, seed=n)
        b, s = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
        rank = matrix_nms_ref.ranked(boxes, scores, 0.001, "sigmoid")
        for method in ("gaussian", "linear"):
            keep, kept = ops.matrix_nms(b, s, method, 0.5, 0.001)
            rk, rs, gap, dist = matrix_nms_ref.matrix_nms(boxes, scores, method, 0.5, 0.001, rank=rank)
            keep, kept = keep.cpu().numpy(), kept.cpu().numpy()
            equal = bool(np.array_equal(keep, rk))
            rel = float((np.abs(kept - rs) / np.abs(rs)).max()) if equal and rs.size else float("nan")
            worst = max(worst, rel)
            print(f"n {n:5d} {method:8s} on logits        kept {len(keep):5d} ref {len(rk):5d} keep_equal {equal} score_maxrel {rel:.3e} "
                  f"gap_margin {gap:.3e} thresh_margin {dist:.3e}", flush=True)
        probs = vote_ref.weights(scores)
        keep, kept = ops.matrix_nms(b, torch.from_numpy(probs).cuda(), "linear", 0.5, 0.001, score="score")
        rk, rs, _, _ = matrix_nms_ref.matrix_nms(boxes, probs, "linear", 0.5, 0.001, score="score")
        print(f"n {n:5d} linear   on probabilities  kept {len(rk):5d} keep_equal {bool(np.array_equal(keep.cpu().numpy(), rk))} "
              f"scores_bit_equal {bool(np.array_equal(kept.cpu().numpy(), rs))}", flush=True)
    print(f"largest observed relative score error {worst:.3e} (bound {bound:.3e})", flush=True)


def pyramid(args, ident):
    from bench import tame_init_
    from tinyfaces import evaluation, ops, transforms
    from tinyfaces.datasets.templates import load_templates
    from tinyfaces.models.model import DetectionModel
    device = torch.device("cuda:0")
    templates = load_templates()
    model = tame_init_(DetectionModel(num_templates=25), 0).set_compute_dtype(torch.bfloat16).to(device).eval()
    rs = np.random.RandomState(11)                                         # bench.py: bench_eval_end_to_end's image
    base = rs.randint(0, 256, (60, 80, 3)).astype(np.uint8)
    u8 = np.kron(base, np.ones((16, 16, 1), np.uint8)) ^ rs.randint(0, 32, (960, 1280, 3)).astype(np.uint8)
    img = torch.from_numpy(u8).permute(2, 0, 1).float().div(255)
    tfm = transforms.Compose([transforms.ToTensor(), transforms.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])])
    variants = {"plain": {}, "soft_linear": {"soft_nms": "linear"}, "matrix_linear": {"soft_nms": "matrix_linear"},
                "matrix_gaussian": {"soft_nms": "matrix_gaussian"}}
    with torch.no_grad(), model.constant_weights(reserve=(1, 1920, 2560)):
        levels = evaluation._pyramid_levels(img, (-1, 0, 1), tfm, True, device)
        outs = model.forward_levels([x for _, x in levels])
        allp = torch.cat([torch.sigmoid(o[0, :25]).flatten() for o in outs])
        thr = float(torch.quantile(allp[torch.randperm(allp.numel(), device=device)[:1000000]], 0.995))
        times = {k: [] for k in variants}
        kept = {}
        for it in range(args.runs + 2):
            for name, kw in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                d = evaluation.get_detections(model, img, templates, ops.RF, tfm, prob_thresh=thr, nms_thresh=0.3, scales=(-1, 0, 1), device=device,
                                              pyramid_on_gpu=True, **kw)
                times[name].append(1e3 * (time.perf_counter() - t0))
                kept[name] = int(d.shape[0])
        cands = int(evaluation.get_detections(model, img, templates, ops.RF, tfm, prob_thresh=thr, nms_thresh=0.3, scales=(-1, 0, 1), device=device,
                                              pyramid_on_gpu=True, return_candidates=True)[1].shape[0])
    med = {k: float(np.median(v[2:])) for k, v in times.items()}
    rec = {"step": "pyramid", "image": "1280x960", "scales": [-1, 0, 1], "dtype": "bf16", "runs": args.runs, "prob_thresh": round(thr, 6),
           "candidates": cands, "kept": kept, "ms_per_image": {k: round(v, 3) for k, v in med.items()},
           "min_ms_per_image": {k: round(float(np.min(v[2:])), 3) for k, v in times.items()},
           "extra_ms_over_plain": {k: round(med[k] - med["plain"], 3) for k in variants if k != "plain"}, "build_id": ident["build_id"]}
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernels", "parity", "pyramid"], required=True)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--runs", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scripts/matrix_nms_numbers.py measures on an MI355X: no GPU, no numbers")
    from tinyfaces import _hip
    {"kernels": kernels, "parity": parity, "pyramid": pyramid}[args.step](args, _hip.identity())


if __name__ == "__main__":
    main()
