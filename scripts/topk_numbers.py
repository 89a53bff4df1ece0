"""What the pre-NMS top-k and the detection cap cost and save on one MI355X, one JSON line per measurement (profiles/topk.jsonl).  The
yardstick of every item is the feature-off leg of the same process -- the path the parent commit runs.

  --step kernels   the clustered candidate list the NMS, the vote and Soft-NMS are timed on (tests/vote_ref.py: clustered_boxes), device events
                   around every call, warm-up first, all legs ALTERNATING in one process, median of --iters:
                     n = 65 536:   hard NMS of the full list | select K = 5000 + gather + NMS of the 5 000 | the select alone | the NMS of the
                                   cut list alone (is the select dearer than the suppression it feeds?)
                     n = 600 000:  select + gather + NMS and the select alone (the plain call is refused above ops.NMS_MAX_BOXES)
                     Soft-NMS, linear and gaussian, n = 65 536, score_thresh 0.001: uncapped | max_keep = 750
                   `same_bits`: two runs returned the same bytes.
  --step pyramid   evaluation.get_detections(pyramid_on_gpu=True) on bench.py's 1280 x 960 end-to-end image, scales (-1, 0, 1), bf16, inside one
                   constant_weights() session: plain | soft_nms="linear" | soft_nms="linear", pre_nms_topk=5000, max_detections=750 --
                   ALTERNATING, wall clock around the synchronous call, median of --runs.

    bash scripts/gpu_job.sh topk        (one process and one time limit per step) -> profiles/topk.jsonl"""
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


def _alternate(variants, iters):
    """Every variant once per round, iters + 2 rounds (the first two are warm-up) -> (median ms, min ms, last output, same bits twice)."""
    times, outs, same = {k: [] for k in variants}, {}, {}
    for _ in range(iters + 2):
        for name, fn in variants.items():
            ms, out = _timed(fn)
            times[name].append(ms)
            flat = out if isinstance(out, (tuple, list)) else (out,)
            if name in outs:
                prev = outs[name] if isinstance(outs[name], (tuple, list)) else (outs[name],)
                same[name] = same.get(name, True) and all(torch.equal(a, b) for a, b in zip(flat, prev))
            outs[name] = out
    med = {k: float(np.median(v[2:])) for k, v in times.items()}
    mn = {k: float(np.min(v[2:])) for k, v in times.items()}
    return med, mn, outs, same


def kernels(args, ident):
    import vote_ref
    from tinyfaces import ops
    K, M = args.k, args.max_keep
    for n in (args.n, 600000):
        boxes, scores = vote_ref.clustered_boxes(n, seed=n)
        b, s = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()

        def select_nms():
            idx, _ = ops.topk_select(s, K)
            return idx[ops.nms(b.index_select(0, idx), s.index_select(0, idx), 0.3)]

        cut = ops.topk_select(s, K)[0]
        bc, sc = b.index_select(0, cut).contiguous(), s.index_select(0, cut).contiguous()
        variants = {"select_nms": select_nms, "select": lambda: ops.topk_select(s, K)[0], "nms_of_cut": lambda: ops.nms(bc, sc, 0.3)}
        if n <= ops.NMS_MAX_BOXES:
            variants = {"nms_full": lambda: ops.nms(b, s, 0.3), **variants}
        med, mn, outs, same = _alternate(variants, args.iters)
        rec = {"step": "kernels", "item": "select", "n": n, "k": K, "iou_thresh": 0.3, "iters": args.iters,
               "ms": {k: round(v, 4) for k, v in med.items()}, "min_ms": {k: round(v, 4) for k, v in mn.items()},
               "kept": {k: int(outs[k].numel()) for k in variants if k != "select"}, "same_bits": bool(all(same.values())),
               "build_id": ident["build_id"]}
        if "nms_full" in med:
            full = outs["nms_full"]
            rec["select_nms_over_nms_full"] = round(med["select_nms"] / med["nms_full"], 4)
            rec["expected_select_nms_beats_nms_full"] = "met" if med["select_nms"] < med["nms_full"] else "not met"
            rec["rows_are_a_prefix_of_the_full_keep"] = bool(torch.equal(outs["select_nms"], full[: outs["select_nms"].numel()]))
        rec["select_over_nms_of_cut"] = round(med["select"] / med["nms_of_cut"], 4)
        print(json.dumps(rec), flush=True)
        if n != args.n:
            continue
        for method in ("linear", "gaussian"):
            variants = {"uncapped": lambda method=method: ops.soft_nms(b, s, method, 0.3, 0.5, 0.001),
                        "capped": lambda method=method: ops.soft_nms_capped(b, s, M, method, 0.3, 0.5, 0.001)}
            med, mn, outs, same = _alternate(variants, args.iters)
            c = int(outs["capped"][0].numel())
            rec = {"step": "kernels", "item": "soft_nms_cap", "method": method, "n": n, "max_keep": M, "iou_thresh": 0.3, "sigma": 0.5,
                   "score_thresh": 0.001, "iters": args.iters, "survivors": {"uncapped": int(outs["uncapped"][0].numel()), "capped": c},
                   "ms": {k: round(v, 4) for k, v in med.items()}, "min_ms": {k: round(v, 4) for k, v in mn.items()},
                   "capped_over_uncapped": round(med["capped"] / med["uncapped"], 4),
                   "expected_capped_beats_uncapped": "met" if med["capped"] < med["uncapped"] else "not met",
                   "first_rows_bit_equal": bool(torch.equal(outs["capped"][0], outs["uncapped"][0][:c]) and
                                                torch.equal(outs["capped"][1], outs["uncapped"][1][:c])),
                   "same_bits": bool(all(same.values())), "build_id": ident["build_id"]}
            print(json.dumps(rec), flush=True)


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
    variants = {"plain": {}, "soft_linear": {"soft_nms": "linear"},
                "soft_linear_topk_cap": {"soft_nms": "linear", "pre_nms_topk": args.k, "max_detections": args.max_keep}}
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
           "candidates": cands, "pre_nms_topk": args.k, "max_detections": args.max_keep, "kept": kept,
           "ms_per_image": {k: round(v, 3) for k, v in med.items()},
           "min_ms_per_image": {k: round(float(np.min(v[2:])), 3) for k, v in times.items()},
           "soft_linear_extra_ms": round(med["soft_linear"] - med["plain"], 3),
           "soft_linear_topk_cap_extra_ms": round(med["soft_linear_topk_cap"] - med["plain"], 3), "build_id": ident["build_id"]}
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernels", "pyramid"], required=True)
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--k", type=int, default=5000)
    ap.add_argument("--max-keep", dest="max_keep", type=int, default=750)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--runs", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scripts/topk_numbers.py measures on an MI355X: no GPU, no numbers")
    from tinyfaces import _hip
    {"kernels": kernels, "pyramid": pyramid}[args.step](args, _hip.identity())


if __name__ == "__main__":
    main()
