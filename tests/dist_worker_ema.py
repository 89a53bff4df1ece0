"""Worker of tests/test_gpu_model_ema.py: one data-parallel rank of the fused TrainEngine with the model EMA on, on the model of
tests/dist_worker_clip.py (ResNet-50, fp32, BatchNorm and the lower stages frozen; gloo rendezvous, every rank on cuda:0 of a 1-GPU box).
Rank r trains on micro-batch r % 2 for two steps and writes its parameters and its average after each to <out>.rank<r>.npz."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tiny-faces-pytorch_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def build(golden_path):
    import dist_worker_trainable
    return dist_worker_trainable.build(golden_path)


def main():
    golden_path, out_path = sys.argv[1], sys.argv[2]
    from tinyfaces import parallel
    from tinyfaces.engine import TrainEngine
    parallel.init_from_env("gloo")
    rank = parallel.rank()
    torch.cuda.set_device(0)
    m, c, batches = build(golden_path)
    eng = TrainEngine(m, c, lr=1e-4, momentum=0.9, weight_decay=5e-4, device="cuda:0", bucket_mb=10, ema_decay=0.999)
    assert eng.ema is not None and eng._overlap is not None
    seg = m._segments
    trained = np.zeros(eng.flat_p.numel(), dtype=bool)
    for k in m.trainable_parameter_names():
        trained[seg[k][0]:seg[k][0] + seg[k][1]] = True
    out = {"trained": trained, "e_init": eng.ema.flat.detach().cpu().numpy().copy()}
    img, cm, rm = [t.cuda() for t in batches[rank % 2]]
    for s in range(2):
        eng.step(img, cm.clone(), rm)
        torch.cuda.synchronize()
        out[f"p{s}"] = eng.flat_p.detach().cpu().numpy().copy()
        out[f"e{s}"] = eng.ema.flat.detach().cpu().numpy().copy()
    out["updates"] = np.array(eng.ema.updates)
    np.savez(f"{out_path}.rank{rank}.npz", **out)
    torch.distributed.barrier()
    eng.close()


if __name__ == "__main__":
    main()
