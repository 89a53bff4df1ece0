"""What the test-time augmentation of get_detections costs on one MI355X, one JSON line per measurement (profiles/tta.jsonl):

  --step kernels   tf_box_vote_f64 next to tf_nms_f64 on the same clustered candidate list (tests/vote_ref.py: clustered_boxes), n = 4 096 and
                   65 536, K = the survivors of the NMS at 0.3, vote_thresh 0.5, sigmoid weights.  The vote is timed on the NMS's raw keep
                   list and device-side count (device events around --iters launches); the NMS by a host clock around ops.nms, which ends in
                   the read of the keep count.  `same_bits`: two vote runs returned the same bytes.
  --step pyramid   evaluation.get_detections(pyramid_on_gpu=True) on bench.py's 1280 x 960 end-to-end image, scales (-1, 0, 1), bf16, inside one
                   constant_weights() session: plain, flip, box_voting = 0.5, and both -- the four variants ALTERNATING, median of --runs.

    bash scripts/gpu_job.sh tta        (one process and one time limit per step) -> profiles/tta.jsonl"""
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


def kernels(args, ident):
    import vote_ref
    from tinyfaces import ops
    for n in (4096, 65536):
        boxes, scores = vote_ref.clustered_boxes(n, seed=n)
        b, s = torch.from_numpy(boxes).cuda(), torch.from_numpy(scores).cuda()
        keep = ops.nms(b, s, 0.3)
        K = int(keep.numel())
        keep_buf = torch.zeros(n, dtype=torch.int64, device="cuda")
        keep_buf[:K] = keep
        cnt = torch.tensor([K], dtype=torch.int32, device="cuda")
        nms_ms = []
        for _ in range(args.iters + 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ops.nms(b, s, 0.3)
            nms_ms.append(1e3 * (time.perf_counter() - t0))
        first = ops.box_voting(b, s, keep_buf, 0.5, num_keep=cnt)[:K].clone()
        for _ in range(3):
            out = ops.box_voting(b, s, keep_buf, 0.5, num_keep=cnt)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            out = ops.box_voting(b, s, keep_buf, 0.5, num_keep=cnt)
        e1.record()
        torch.cuda.synchronize()
        vote_ms = e0.elapsed_time(e1) / args.iters
        ref, votes = vote_ref.box_voting(boxes, scores, keep.cpu().numpy(), 0.5)
        rec = {"step": "kernels", "n": n, "kept": K, "vote_thresh": 0.5, "weight": "sigmoid", "iters": args.iters,
               "nms_ms": round(float(np.median(nms_ms[2:])), 4), "vote_ms": round(vote_ms, 4),
               "vote_over_nms": round(vote_ms / float(np.median(nms_ms[2:])), 4), "pairs": K * n, "pairs_per_us": round(K * n / (1e3 * vote_ms), 1),
               "mean_votes": round(float(votes.mean()), 2), "coord_maxabs_vs_numpy": float(np.abs(out[:K, :4].cpu().numpy() - ref[:, :4]).max()),
               "same_bits": bool(torch.equal(out[:K], first)), "build_id": ident["build_id"]}
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
    variants = {"plain": {}, "flip": {"flip": True}, "vote": {"box_voting": 0.5}, "flip_vote": {"flip": True, "box_voting": 0.5}}
    with torch.no_grad(), model.constant_weights(reserve=(1, 1920, 2560)):
        levels = evaluation._pyramid_levels(img, (-1, 0, 1), tfm, True, device)
        outs = model.forward_levels([x for _, x in levels])
        allp = torch.cat([torch.sigmoid(o[0, :25]).flatten() for o in outs])
        thr = float(torch.quantile(allp[torch.randperm(allp.numel(), device=device)[:1000000]], 0.995))
        times = {k: [] for k in variants}
        kept, cands = {}, {}
        for it in range(args.runs + 2):
            for name, kw in variants.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                d = evaluation.get_detections(model, img, templates, ops.RF, tfm, prob_thresh=thr, nms_thresh=0.3, scales=(-1, 0, 1), device=device,
                                              pyramid_on_gpu=True, **kw)
                times[name].append(1e3 * (time.perf_counter() - t0))
                kept[name] = int(d.shape[0])
        for name, kw in variants.items():
            if "box_voting" not in kw:
                cands[name] = int(evaluation.get_detections(model, img, templates, ops.RF, tfm, prob_thresh=thr, nms_thresh=0.3, scales=(-1, 0, 1),
                                                            device=device, pyramid_on_gpu=True, return_candidates=True, **kw)[1].shape[0])
    med = {k: float(np.median(v[2:])) for k, v in times.items()}
    rec = {"step": "pyramid", "image": "1280x960", "scales": [-1, 0, 1], "dtype": "bf16", "runs": args.runs, "prob_thresh": round(thr, 6),
           "candidates": cands, "kept": kept, "ms_per_image": {k: round(v, 3) for k, v in med.items()},
           "min_ms_per_image": {k: round(float(np.min(v[2:])), 3) for k, v in times.items()},
           "flip_over_plain": round(med["flip"] / med["plain"], 4), "vote_extra_ms": round(med["vote"] - med["plain"], 3),
           "flip_vote_over_plain": round(med["flip_vote"] / med["plain"], 4), "build_id": ident["build_id"]}
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["kernels", "pyramid"], required=True)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--runs", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scripts/tta_numbers.py measures on an MI355X: no GPU, no numbers")
    from tinyfaces import _hip
    {"kernels": kernels, "pyramid": pyramid}[args.step](args, _hip.identity())


if __name__ == "__main__":
    main()
