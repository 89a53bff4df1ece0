"""What Soft-NMS costs on one MI355X, one JSON line per measurement (profiles/soft_nms.jsonl), and its parity against the numpy restatement
(profiles/soft_nms_parity.txt):

  --step kernels   tf_soft_nms_f64 next to tf_nms_f64 (the yardstick, same process) on the 65 536-candidate clustered list the NMS and the vote
                   are timed on (tests/vote_ref.py: clustered_boxes), both methods at score_thresh 0.001 and 0.3, iou_thresh 0.3, sigma 0.5,
                   sigmoid scores.  Device events around every call, warm-up first, the variants ALTERNATING in one process, median of --iters.
                   The call is two launches: the adjacency matrix and the selection.  `matrix_ms` is the same call at a score_thresh nobody
                   passes (2.0: the matrix launch, the initial scores and one empty round), `select_ms` the difference to the full call;
                   `ms_per_1000_survivors` = select_ms per thousand survivors.  `same_bits`: two runs returned the same bytes.
  --step parity    the kernels against tests/soft_nms_ref.py at n = 4 097 (both methods, both thresholds): kept indices equal, largest relative
                   score deviation, the bound 8 (K + 2) 2^-52 and the reference's two margins.
  --step pyramid   evaluation.get_detections(pyramid_on_gpu=True) on bench.py's 1280 x 960 end-to-end image, scales (-1, 0, 1), bf16, inside one
                   constant_weights() session: plain, soft linear, soft gaussian -- ALTERNATING, median of --runs.

    bash scripts/gpu_job.sh soft-nms        (one process and one time limit per step) -> profiles/soft_nms.jsonl, profiles/soft_nms_parity.txt"""
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
        variants[f"{method}_matrix"] = lambda method=method: ops.soft_nms(b, s, method, 0.3, 0.5, 2.0)
        for thr in (0.001, 0.3):
            variants[f"{method}_{thr}"] = lambda method=method, thr=thr: ops.soft_nms(b, s, method, 0.3, 0.5, thr)
    times, outs, same = {k: [] for k in variants}, {}, {}
    for it in range(args.iters + 2):
        for name, fn in variants.items():
            ms, out = _timed(fn)
            times[name].append(ms)
            if name in outs and name != "nms":
                same[name] = same.get(name, True) and torch.equal(out[0], outs[name][0]) and torch.equal(out[1], outs[name][1])
            outs[name] = out
    med = {k: float(np.median(v[2:])) for k, v in times.items()}
    print(json.dumps({"step": "kernels", "variant": "nms", "n": n, "iou_thresh": 0.3, "kept": int(outs["nms"].numel()), "iters": args.iters,
                      "ms": round(med["nms"], 4), "min_ms": round(float(np.min(times["nms"][2:])), 4), "build_id": ident["build_id"]}), flush=True)
    for method in ("linear", "gaussian"):
        matrix = med[f"{method}_matrix"]
        for thr in (0.001, 0.3):
            name = f"{method}_{thr}"
            K = int(outs[name][0].numel())
            sel = med[name] - matrix
            kept = outs[name][1]
            rec = {"step": "kernels", "variant": "soft_nms", "method": method, "n": n, "iou_thresh": 0.3, "sigma": 0.5, "score_thresh": thr,
                   "survivors": K, "iters": args.iters, "ms": round(med[name], 4), "min_ms": round(float(np.min(times[name][2:])), 4),
                   "matrix_ms": round(matrix, 4), "select_ms": round(sel, 4),
                   "ms_per_1000_survivors": round(1e3 * sel / max(K, 1), 4), "over_nms": round(med[name] / med["nms"], 3),
                   "scores_non_increasing": bool((kept[1:] <= kept[:-1]).all()), "same_bits": bool(same[name]), "build_id": ident["build_id"]}
            print(json.dumps(rec), flush=True)


def parity(args, ident):
    import soft_nms_ref
    import vote_ref
    from tinyfaces import ops
    n = 4097
    boxes, scores = vote_ref.clustered_boxes(n, seed=n)
    b, s = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
    print(f"# Soft-NMS kernels against tests/soft_nms_ref.py, clustered_boxes({n}, seed={n}), iou_thresh 0.3, sigma 0.5, sigmoid scores; build {ident['build_id']}")
    for method in ("linear", "gaussian"):
        for thr in (0.001, 0.3):
            keep, kept = ops.soft_nms(b, s, method, 0.3, 0.5, thr)
            rk, rs, rank_margin, thresh_margin = soft_nms_ref.soft_nms(boxes, scores, method, 0.3, 0.5, thr)
            keep, kept = keep.cpu().numpy(), kept.cpu().numpy()
            equal = bool(np.array_equal(keep, rk))
            rel = float((np.abs(kept - rs) / np.abs(rs)).max()) if equal and rs.size else float("nan")
            print(f"{method:8s} score_thresh {thr:<5} kept {len(keep):5d} ref {len(rk):5d} keep_equal {equal} score_maxrel {rel:.3e} "
                  f"bound {soft_nms_ref.score_bound(len(rk)):.3e} rank_margin {rank_margin:.3e} thresh_margin {thresh_margin:.3e}", flush=True)
    probs = vote_ref.weights(scores)
    keep, kept = ops.soft_nms(b, torch.from_numpy(probs).cuda(), "linear", 0.3, 0.5, 0.001, score="score")
    rk, rs, _, _ = soft_nms_ref.soft_nms(boxes, probs, "linear", 0.3, 0.5, 0.001, score="score")
    print(f"linear   on probabilities (score mode): keep_equal {bool(np.array_equal(keep.cpu().numpy(), rk))} "
          f"scores_bit_equal {bool(np.array_equal(kept.cpu().numpy(), rs))}", flush=True)


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
    variants = {"plain": {}, "soft_linear": {"soft_nms": "linear"}, "soft_gaussian": {"soft_nms": "gaussian"}}
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
           "soft_linear_extra_ms": round(med["soft_linear"] - med["plain"], 3), "soft_gaussian_extra_ms": round(med["soft_gaussian"] - med["plain"], 3),
           "build_id": ident["build_id"]}
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernels", "parity", "pyramid"], required=True)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--runs", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scripts/soft_nms_numbers.py measures on an MI355X: no GPU, no numbers")
    from tinyfaces import _hip
    {"kernels": kernels, "parity": parity, "pyramid": pyramid}[args.step](args, _hip.identity())


if __name__ == "__main__":
    main()
