"""What the scale-compensated anchor matching (ops.dense_overlap_targets_device(compensate=(N, T)), tf_dense_overlap_targets_comp) costs
next to the plain call on one MI355X: both ALTERNATING in one process on one box, device-event time of ONE call, median over --calls
calls of each leg, one JSON line per pair.

  * "bench" lines: the bs 12 operands bench.py builds (1-16 boxes of 8-200 px per image), compensate=(3, 0.1);
  * "tiny" lines: a seeded bs 12 batch of 16 faces of 8-16 px per image -- the worst case of the selection, every face runs its rounds --
    with N = 1, 3 and 16: the plain call and N = 1 differ by the owner / best store, the count pass and ONE selection round, the step from
    N = 1 to 3 to 16 is further rounds alone.

The yardstick is the plain call of the same pair, never an absolute figure.  The last line of each kind (`"summary"`) puts the median
added time next to the spread of each leg between the pairs of this job.
    python scripts/anchor_compensation_numbers.py [--pairs 5 --calls 200] >> profiles/anchor_compensation.jsonl"""
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


def tiny_batch(device, bs=12, faces=16, seed=0):
    rng = np.random.RandomState(seed)
    s = rng.uniform(8, 16, (bs, faces))
    a = rng.uniform(0.7, 1.0, (bs, faces))
    x, y = rng.uniform(0, 500 - s * a), rng.uniform(0, 500 - s)
    boxes = np.stack([x, y, x + s * a, y + s], 2).reshape(-1, 4)
    return {"boxes": torch.from_numpy(boxes).to(device), "offs": torch.arange(0, bs * faces + 1, faces, dtype=torch.int32, device=device),
            "total": bs * faces, "paste": torch.tensor([[0, 0, 500, 500]] * bs, dtype=torch.int32, device=device)}


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
    batches = {"bench": (synthetic_batch(0, 12, device, None), [("comp_n3", (3, 0.1))]),
               "tiny": (tiny_batch(device), [("comp_n1", (1, 0.1)), ("comp_n3", (3, 0.1)), ("comp_n16", (16, 0.1))])}
    for kind, (b, comps) in batches.items():
        out = (torch.empty(12, 25, 63, 63, device=device), torch.empty(12, 100, 63, 63, device=device))

        def call(comp, i):
            return ops.dense_overlap_targets_device(b["boxes"], b["offs"], b["total"], t_d, paste_d=b["paste"], seed=i, out=out, compensate=comp)

        legs = [("plain", None)] + comps
        base = int((call(None, 0)[0] == 1).sum())
        facts = {"faces": int(b["total"]), "positives_plain": base}
        for name, comp in comps:
            cm, _, mc = ops.dense_overlap_targets_device(b["boxes"], b["offs"], b["total"], t_d, paste_d=b["paste"], seed=0, compensate=comp,
                                                         return_match_count=True)
            facts[f"positives_{name}"] = int((cm == 1).sum())
            facts[f"faces_below_n_{name}"] = int((mc < comp[0]).sum())
        recs = []
        for pair in range(args.pairs):
            rec = {"kind": kind, "pair": pair, "batch": 12, "map": [25, 63, 63], "calls": args.calls, "build_id": ident["build_id"], **facts}
            for name, comp in legs:
                for i in range(8):
                    call(comp, i)
                torch.cuda.synchronize()
                marks = []
                for i in range(args.calls):
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    ev[0].record()
                    call(comp, i)
                    ev[1].record()
                    marks.append(ev)
                torch.cuda.synchronize()
                rec[f"{name}_us"] = round(1e3 * statistics.median(x.elapsed_time(y) for x, y in marks), 1)
            recs.append(rec)
            print(json.dumps(rec), flush=True)
        if len(recs) > 1:
            s = {"summary": True, "kind": kind, "pairs": len(recs), "build_id": ident["build_id"]}
            for name, _ in legs:
                vals = [r[f"{name}_us"] for r in recs]
                s[f"{name}_us_median"], s[f"{name}_us_spread"] = round(statistics.median(vals), 1), round(max(vals) - min(vals), 1)
                if name != "plain":
                    s[f"{name}_added_us_median"] = round(statistics.median(r[f"{name}_us"] - r["plain_us"] for r in recs), 1)
            print(json.dumps(s), flush=True)


if __name__ == "__main__":
    main()
