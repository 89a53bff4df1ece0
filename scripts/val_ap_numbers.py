"""What the device WIDER evaluator costs and saves on one MI355X, one JSON line per measurement (profiles/val_ap.jsonl).  The yardstick is
the host evaluator (tinyfaces.wider_eval.evaluate_setting) in the same process on the same arrays.

  --step evaluator   a seeded prediction set shaped like WIDER val: --images (3 226) images, rows per image up to 750, boxes per image from a
                     long-tailed distribution up to ~2 000, three settings.  Device: DeviceEvaluator.add over the whole set in batches of
                     --batch images + finish(), wall clock between a device synchronisation and the return of finish() (which ends in the one
                     host read).  Host: evaluate_setting(norm_scores(...)) for the three settings.  The host takes minutes on the whole set,
                     so the PAIRS run on the first --host-fraction of the images (stated in the record), device and host alternating, --pairs
                     pairs; the device alone is then timed on the whole set.  The record says whether AP and curve were equal.
  --step kernels     the two kernels alone at the whole-set size: ops.wider_match_batched and ops.wider_pr_accumulate between device events,
                     median of --iters after a warm-up.
  --step val         `main.py synthetic-faces synthetic-faces` (the configuration of tests/test_gpu_e2e.py, two epochs) with and without
                     --val-every 1, alternating, wall clock of the child processes: the cost of a validation pass is reported, not bounded.

    python scripts/val_ap_numbers.py --step evaluator --step kernels --step val --out profiles/val_ap.jsonl"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tiny-faces-pytorch_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

SETTINGS = ("easy", "medium", "hard")


def wider_like_set(n_images, seed=0, max_rows=750):
    """{event: {image: rows}}, {event: {image: gt}}, [keep per setting]: integer geometry, scores on a fine grid (ties), boxes per image
    long-tailed (most images a handful, a few up to ~2 000), detections = jittered boxes + background."""
    rng = np.random.RandomState(seed)
    preds, gtb, keeps = {"ev": {}}, {"ev": {}}, [{"ev": {}} for _ in SETTINGS]
    for i in range(n_images):
        G = int(min(2000, np.floor(rng.pareto(1.1) * 4) + (rng.rand() < 0.95)))
        gt = np.column_stack([rng.randint(0, 1000, (G, 2)), rng.randint(6, 120, (G, 2))]).astype(np.float64)
        N = int(min(max_rows, 3 * G + rng.randint(50, 1500)))    # about half of the images reach the cap
        rows = np.zeros((N, 5))
        on = rng.rand(N) < (0.6 if G else 0.0)
        k = int(on.sum())
        if k:
            rows[on, :4] = gt[rng.randint(G, size=k)] + rng.randint(-5, 6, (k, 4))
        rows[~on, :4] = np.column_stack([rng.randint(0, 1000, (N - k, 2)), rng.randint(6, 120, (N - k, 2))])
        rows[:, 4] = np.round(np.where(on, rng.beta(4, 2, N), rng.beta(1.5, 4, N)) * 4096) / 4096
        rows = rows[np.argsort(-rows[:, 4], kind="stable")]
        name = f"img_{i}"
        preds["ev"][name], gtb["ev"][name] = rows, gt
        size = gt[:, 3] if G else np.zeros(0)
        for s, lim in enumerate((50, 25, 0)):                 # easy: the tall faces; hard: all of them -- nested like WIDER's
            keeps[s]["ev"][name] = np.nonzero(size >= lim)[0]
    return preds, gtb, keeps


def _subset(d, names):
    return {"ev": {n: d["ev"][n] for n in names}}


def _device(preds, gtb, keeps, names, batch):
    from tinyfaces.wider_eval import DeviceEvaluator
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev = DeviceEvaluator(SETTINGS, device="cuda")
    for first in range(0, len(names), batch):
        chunk = names[first:first + batch]
        ev.add([preds["ev"][n] for n in chunk], [gtb["ev"][n] for n in chunk], [[k["ev"][n] for n in chunk] for k in keeps])
    out = ev.finish()
    return time.perf_counter() - t0, out


def _host(preds, gtb, keeps, names):
    from tinyfaces import wider_eval as we
    t0 = time.perf_counter()
    normed = we.norm_scores(_subset(preds, names))
    g = _subset(gtb, names)
    out = {s: we.evaluate_setting(normed, g, _subset(keeps[k], names)) for k, s in enumerate(SETTINGS)}
    return time.perf_counter() - t0, out


def evaluator(args, ident, emit):
    preds, gtb, keeps = wider_like_set(args.images, seed=args.seed)
    names = list(preds["ev"])
    part = names[:max(1, int(round(len(names) * args.host_fraction)))]
    shape = {"images": len(names), "rows": int(sum(v.shape[0] for v in preds["ev"].values())), "boxes": int(sum(v.shape[0] for v in gtb["ev"].values())),
             "max_rows": int(max(v.shape[0] for v in preds["ev"].values())), "max_boxes": int(max(v.shape[0] for v in gtb["ev"].values())), "settings": len(SETTINGS)}
    _device(preds, gtb, keeps, part[:64], args.batch)                      # warm-up: library load, workspaces
    dev_s, host_s, equal = [], [], True
    for _ in range(args.pairs):
        td, od = _device(preds, gtb, keeps, part, args.batch)
        th, oh = _host(preds, gtb, keeps, part)
        dev_s.append(td); host_s.append(th)
        equal = equal and all(od[s][0] == oh[s][0] and np.array_equal(od[s][1], oh[s][1]) for s in SETTINGS)
    part_shape = {"images": len(part), "rows": int(sum(preds["ev"][n].shape[0] for n in part)), "boxes": int(sum(gtb["ev"][n].shape[0] for n in part))}
    emit({"step": "evaluator", "item": "pairs", "set": shape, "timed_on": part_shape, "host_fraction": args.host_fraction, "pairs": args.pairs, "batch": args.batch,
          "device_s": [round(t, 5) for t in dev_s], "host_s": [round(t, 3) for t in host_s],
          "ratio_host_over_device": [round(h / d, 1) for h, d in zip(host_s, dev_s)], "ap_and_curve_equal": bool(equal),
          "ap": {s: oh[s][0] for s in SETTINGS}, "build_id": ident["build_id"]})
    full = [_device(preds, gtb, keeps, names, args.batch)[0] for _ in range(args.pairs)]
    emit({"step": "evaluator", "item": "device_whole_set", "set": shape, "batch": args.batch, "device_s": [round(t, 5) for t in full],
          "host_s_extrapolated_from_fraction": round(float(np.median(host_s)) * shape["rows"] / max(part_shape["rows"], 1), 1), "build_id": ident["build_id"]})


def kernels(args, ident, emit):
    from tinyfaces import ops
    preds, gtb, keeps = wider_like_set(args.images, seed=args.seed)
    names = [n for n in preds["ev"] if preds["ev"][n].shape[0] and gtb["ev"][n].shape[0]]
    rows = torch.from_numpy(np.concatenate([preds["ev"][n] for n in names])).cuda()
    gt = torch.from_numpy(np.concatenate([gtb["ev"][n] for n in names])).cuda()
    doff = np.concatenate([[0], np.cumsum([preds["ev"][n].shape[0] for n in names])]).tolist()
    goff = np.concatenate([[0], np.cumsum([gtb["ev"][n].shape[0] for n in names])]).tolist()
    masks = np.zeros((len(SETTINGS), goff[-1]), np.uint8)
    for k in range(len(SETTINGS)):
        for j, n in enumerate(names):
            masks[k, goff[j]:goff[j + 1]][keeps[k]["ev"][n]] = 1
    masks = torch.from_numpy(masks).cuda()
    T = 1000
    thresh = torch.tensor([1 - (t + 1) / T for t in range(T)], dtype=torch.float64).cuda()
    lo_d = torch.tensor([0.0, 1.0], dtype=torch.float64).cuda()
    scores = rows[:, 4].contiguous()
    pr = torch.zeros(len(SETTINGS), T, 2, dtype=torch.int64, device="cuda")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    tm, tp = [], []
    for _ in range(args.iters + 2):
        ms, (counted, recalled) = timed(lambda: ops.wider_match_batched(rows, doff, gt, goff, masks, 0.5))
        tm.append(ms)
        ms, _ = timed(lambda: ops.wider_pr_accumulate(scores, doff, counted, recalled, lo_d, thresh, pr))
        tp.append(ms)
    emit({"step": "kernels", "images": len(names), "rows": doff[-1], "boxes": goff[-1], "settings": len(SETTINGS), "thresholds": T, "iters": args.iters,
          "match_ms": {"median": round(float(np.median(tm[2:])), 4), "min": round(float(np.min(tm[2:])), 4), "max": round(float(np.max(tm[2:])), 4)},
          "pr_ms": {"median": round(float(np.median(tp[2:])), 4), "min": round(float(np.min(tp[2:])), 4), "max": round(float(np.max(tp[2:])), 4)},
          "launches": {"match": -(-len(names) // 256), "pr": -(-len(names) // 256)}, "build_id": ident["build_id"]})


def val(args, ident, emit):
    import tempfile
    common = ["synthetic-faces", "synthetic-faces", "--epochs", "2", "--synthetic-len", "3200", "--batch_size", "32", "--lr", "2e-4", "--save-every", "2",
              "--dtype", "bf16", "--ohem-thresh", "0"]
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + os.environ.get("PYTHONPATH", ""))
    walls = {"plain": [], "val_every_1": []}
    aps = []
    for _ in range(args.val_pairs):
        for name, extra in (("plain", []), ("val_every_1", ["--val-every", "1", "--val-prob-thresh", "0.1"])):
            d = tempfile.mkdtemp()
            t0 = time.perf_counter()
            r = subprocess.run([sys.executable, os.path.join(PKG, "main.py")] + common + ["--save-path", os.path.join(d, "w")] + extra, cwd=d, env=env,
                               capture_output=True, text=True, timeout=600)
            walls[name].append(time.perf_counter() - t0)
            if r.returncode != 0:
                raise SystemExit(r.stderr[-3000:])
            aps += [ln for ln in r.stdout.splitlines() if ln.startswith("Val:")]
    diff = [b - a for a, b in zip(walls["plain"], walls["val_every_1"])]
    emit({"step": "val", "command": "main.py " + " ".join(common), "validation": "8 images, 4-level pyramid, prob_thresh 0.1, two passes per run",
          "wall_s": {k: [round(t, 2) for t in v] for k, v in walls.items()}, "extra_s_per_run": [round(t, 2) for t in diff],
          "extra_s_per_pass": [round(t / 2, 2) for t in diff], "note": "the first pass of a run also builds the evaluation copy of the model and its workspaces",
          "val_lines": aps, "build_id": ident["build_id"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="append", choices=["evaluator", "kernels", "val"], required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "val_ap.jsonl"))
    ap.add_argument("--images", type=int, default=3226)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--host-fraction", dest="host_fraction", type=float, default=0.1)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--val-pairs", dest="val_pairs", type=int, default=2)
    args = ap.parse_args()
    from tinyfaces import _hip
    ident = _hip.identity()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")

    for step in args.step:
        {"evaluator": evaluator, "kernels": kernels, "val": val}[step](args, ident, emit)


if __name__ == "__main__":
    main()
