"""Worker of tests/test_gpu_grad_accum.py: one data-parallel rank of the fused TrainEngine with gradient accumulation (accum_steps = 2), on
the model of tests/dist_worker_trainable.py (ResNet-50, fp32, BatchNorm and the lower stages frozen; gloo rendezvous, every rank on cuda:0 of
a 1-GPU box).  Rank r runs two windows over the micro-batches (b[r % 2], b[(r + 1) % 2]) and writes its parameters after each window to
<out>.rank<r>.npz.  It counts the dist.all_reduce calls of every micro-batch: none before a window's last one."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tiny-faces-pytorch_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

WINDOWS = 2


def build(golden_path):
    import dist_worker_trainable
    return dist_worker_trainable.build(golden_path)


def main():
    golden_path, out_path = sys.argv[1], sys.argv[2]
    import torch.distributed as dist
    from tinyfaces import parallel
    from tinyfaces.engine import TrainEngine
    parallel.init_from_env("gloo")
    rank = parallel.rank()
    torch.cuda.set_device(0)
    m, c, batches = build(golden_path)
    eng = TrainEngine(m, c, lr=1e-4, momentum=0.9, weight_decay=5e-4, device="cuda:0", bucket_mb=10, accum_steps=2)
    assert eng._overlap is not None and eng._native is None and m._grad_callback is None        # no gradient-ready hook in this mode
    ranges = eng._overlap["ranges"]
    calls = [0]
    all_reduce = dist.all_reduce

    def counted(*a, **kw):
        calls[0] += 1
        return all_reduce(*a, **kw)

    dist.all_reduce = counted
    order = [[t.cuda() for t in batches[(rank + k) % 2]] for k in range(2)]
    out, per_micro = {}, []
    for w in range(WINDOWS):
        for k, (img, cm, rm) in enumerate(order):
            before = calls[0]
            eng.step(img, cm.clone(), rm)
            torch.cuda.synchronize()
            per_micro.append(calls[0] - before)
            assert eng.pending_micro_batches == (1 if k == 0 else 0)
        assert per_micro[-2] == 0, per_micro                       # nothing was exchanged before the window's last micro-batch
        assert per_micro[-1] == len(ranges), (per_micro, len(ranges))      # ... and then the engine's bucket ranges, once each
        out[f"p{w}"] = eng.flat_p.detach().cpu().numpy().copy()
    dist.all_reduce = all_reduce
    assert (eng.steps, eng.micro_steps) == (WINDOWS, 2 * WINDOWS)
    out["collectives"] = np.array(per_micro)
    out["buckets"] = np.array(len(ranges))
    np.savez(f"{out_path}.rank{rank}.npz", **out)
    dist.barrier()
    eng.close()


if __name__ == "__main__":
    main()
