"""What the ignore-region pass (ops.dense_overlap_targets_device(ignore_d=, ...), tf_targets_apply_ignore) costs next to the plain call on one
MI355X: both ALTERNATING in one process on one box, device-event time of ONE call, median over --calls calls of each leg, one JSON line per
pair.

  * "bench" lines: the bs 12 face operands bench.py builds (1-16 boxes of 8-200 px per image), unchanged; the ignore boxes are what the
    `truncated` policy yields for a seeded 500-pixel crop of each image's own layout doubled (augment.crop_decisions(truncated=True)):
    the faces that crop cuts below neg_thresh, clamped;
  * "crowd" lines: a seeded bs 12 batch with 500 ignore boxes of 6-40 px per image (two LDS tiles per block) next to bench.py's faces.

Legs: the plain call; the call with ignore boxes, ("iof", 0.5); the same with the per-image counter.  The yardstick is the plain call of the
same pair, never an absolute figure.  The last line of each kind (`"summary"`) puts the median added time next to the spread of each leg
between the pairs of this job.
    python scripts/ignore_regions_numbers.py [--pairs 5 --calls 200] >> profiles/ignore_regions.jsonl"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tiny-faces-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def resident(per_image, device):
    kept = [np.asarray(b, dtype=np.float64).reshape(-1, 4) for b in per_image]
    kept = [b[~((b[:, 2] <= b[:, 0]) | (b[:, 3] <= b[:, 1]))] for b in kept]
    offs = np.cumsum([0] + [b.shape[0] for b in kept]).astype(np.int32)
    cat = np.concatenate(kept) if offs[-1] else np.zeros((1, 4))
    return dict(ignore_d=torch.from_numpy(cat).to(device), ignore_offs_d=torch.from_numpy(offs).to(device), total_ignore=int(offs[-1]))


def truncated_boxes(host_boxes, seed=0):
    """Per image the ignore boxes of the `truncated` policy for a seeded 500-pixel crop of the layout at twice its size."""
    from tinyfaces.datasets.augment import crop_decisions
    rng = np.random.RandomState(seed)
    out = []
    for b in host_boxes:
        got = []
        crop_decisions(1000, 1000, b * 2, rng=rng, truncated=True, ignore_out=got)
        out.append(np.array(got, dtype=np.float64).reshape(-1, 4))
    return out


def crowd_boxes(bs=12, per_image=500, seed=0):
    rng = np.random.RandomState(seed)
    s = rng.uniform(6, 40, (bs, per_image))
    x, y = rng.uniform(0, 500 - 0.8 * s), rng.uniform(0, 500 - s)
    return list(np.stack([x, y, x + 0.8 * s, y + s], 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    from bench import synthetic_batch
    from tinyfaces import _hip, ops
    from tinyfaces.datasets.templates import load_templates
    device = torch.device("cuda:0")
    ident = _hip.identity()
    t_d = torch.as_tensor(load_templates(), dtype=torch.float64, device=device)
    b = synthetic_batch(0, 12, device, None)
    sets = {"bench": resident(truncated_boxes(b["host_boxes"]), device), "crowd": resident(crowd_boxes(), device)}
    out = (torch.empty(12, 25, 63, 63, device=device), torch.empty(12, 100, 63, 63, device=device))
    for kind, ign in sets.items():

        def call(leg, i):
            extra = {} if leg == "plain" else dict(ign, ignore=("iof", 0.5), return_ignored_count=leg == "ignore_count")
            return ops.dense_overlap_targets_device(b["boxes"], b["offs"], b["total"], t_d, paste_d=b["paste"], seed=i, out=out, **extra)

        legs = ["plain", "ignore", "ignore_count"]
        negatives = int((call("plain", 0)[0] == -1).sum())
        turned = call("ignore_count", 0)[2]
        facts = {"faces": int(b["total"]), "ignore_boxes": ign["total_ignore"], "negatives_plain": negatives, "anchors_turned": int(turned.sum()),
                 "images_with_any": int((turned > 0).sum())}
        recs = []
        for pair in range(args.pairs):
            rec = {"kind": kind, "pair": pair, "batch": 12, "map": [25, 63, 63], "calls": args.calls, "build_id": ident["build_id"], **facts}
            for leg in legs:
                for i in range(8):
                    call(leg, i)
                torch.cuda.synchronize()
                marks = []
                for i in range(args.calls):
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    ev[0].record()
                    call(leg, i)
                    ev[1].record()
                    marks.append(ev)
                torch.cuda.synchronize()
                rec[f"{leg}_us"] = round(1e3 * statistics.median(x.elapsed_time(y) for x, y in marks), 1)
            recs.append(rec)
            print(json.dumps(rec), flush=True)
        if len(recs) > 1:
            s = {"summary": True, "kind": kind, "pairs": len(recs), "build_id": ident["build_id"]}
            for leg in legs:
                vals = [r[f"{leg}_us"] for r in recs]
                s[f"{leg}_us_median"], s[f"{leg}_us_spread"] = round(statistics.median(vals), 1), round(max(vals) - min(vals), 1)
                if leg != "plain":
                    s[f"{leg}_added_us_median"] = round(statistics.median(r[f"{leg}_us"] - r["plain_us"] for r in recs), 1)
            print(json.dumps(s), flush=True)


if __name__ == "__main__":
    main()
