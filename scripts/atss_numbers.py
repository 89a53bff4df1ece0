"""What the ATSS target assignment (ops.atss_targets_device, tf_targets_atss) costs next to the plain dense_overlap call on one MI355X: both
ALTERNATING in one process on one box, device-event time of ONE call of the resident entry point, median over --calls calls of each leg, one
JSON line per pair.

  * "bench" lines: the bs 12 operands bench.py builds (1-16 boxes of 8-200 px per image);
  * "tiny" lines: the seeded bs 12 batch of 192 faces of 8-16 px (scripts/anchor_compensation_numbers.py: tiny_batch);
each with k = 1, 9 and 16.

The yardstick is the plain call of the same pair, never an absolute figure: the last line of each kind (`"summary"`) gives every leg's median
and spread between the pairs of this job and the ATSS call's time as a ratio to the plain call.
    python scripts/atss_numbers.py [--pairs 5 --calls 200] >> profiles/atss.jsonl"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tiny-faces-pytorch_amd"), os.path.join(ROOT, "scripts")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args()
    from anchor_compensation_numbers import tiny_batch
    from bench import synthetic_batch
    from tinyfaces import _hip, ops
    from tinyfaces.datasets.templates import load_templates
    device = torch.device("cuda:0")
    ident = _hip.identity()
    t_d = torch.as_tensor(load_templates(), dtype=torch.float64, device=device)
    ks = (1, 9, 16)
    for kind, b in (("bench", synthetic_batch(0, 12, device, None)), ("tiny", tiny_batch(device))):
        out = (torch.empty(12, 25, 63, 63, device=device), torch.empty(12, 100, 63, 63, device=device))

        def call(k, i):
            if k is None:
                return ops.dense_overlap_targets_device(b["boxes"], b["offs"], b["total"], t_d, paste_d=b["paste"], seed=i, out=out)
            return ops.atss_targets_device(b["boxes"], b["offs"], b["total"], t_d, paste_d=b["paste"], topk=k, out=out)

        legs = [("plain", None)] + [(f"atss_k{k}", k) for k in ks]
        facts = {"faces": int(b["total"]), "positives_plain": int((call(None, 0)[0] == 1).sum())}
        for k in ks:
            cm, _, mc = ops.atss_targets_device(b["boxes"], b["offs"], b["total"], t_d, paste_d=b["paste"], topk=k, return_match_count=True)
            facts[f"positives_atss_k{k}"] = int((cm == 1).sum())
            facts[f"faces_without_positive_atss_k{k}"] = int((mc == 0).sum())
        recs = []
        for pair in range(args.pairs):
            rec = {"kind": kind, "pair": pair, "batch": 12, "map": [25, 63, 63], "calls": args.calls, "build_id": ident["build_id"], **facts}
            for name, k in legs:
                for i in range(8):
                    call(k, i)
                torch.cuda.synchronize()
                marks = []
                for i in range(args.calls):
                    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                    ev[0].record()
                    call(k, i)
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
                    s[f"{name}_ratio_to_plain_median"] = round(statistics.median(r[f"{name}_us"] / r["plain_us"] for r in recs), 2)
            print(json.dumps(s), flush=True)


if __name__ == "__main__":
    main()
