"""Worker of tests/test_gpu_adamw.py: one data-parallel rank of the fused TrainEngine with optimizer="adamw", on the model of
tests/dist_worker_ema.py (ResNet-50, fp32, BatchNorm and the lower stages frozen; gloo rendezvous, every rank on cuda:0 of a 1-GPU box).
Rank r trains on micro-batch r % 2 for two steps and writes its parameters, both moments and the device step to <out>.rank<r>.npz."""
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
    eng = TrainEngine(m, c, lr=1e-4, weight_decay=1e-2, device="cuda:0", bucket_mb=10, optimizer="adamw", max_grad_norm=1e3)
    assert eng._overlap is not None and eng.flat_v is not None
    seg = m._segments
    trained = np.zeros(eng.flat_p.numel(), dtype=bool)
    for k in m.trainable_parameter_names():
        trained[seg[k][0]:seg[k][0] + seg[k][1]] = True
    out = {"trained": trained, "p_init": eng.flat_p.detach().cpu().numpy().copy()}
    img, cm, rm = [t.cuda() for t in batches[rank % 2]]
    for s in range(2):
        eng.step(img, cm.clone(), rm)
        torch.cuda.synchronize()
        for name, t in (("p", eng.flat_p), ("m", eng.flat_m), ("v", eng.flat_v)):
            out[f"{name}{s}"] = t.detach().cpu().numpy().copy()
    st = eng.adam_state.read()
    out["step"], out["bias"] = np.array(st.step), np.array([st.bias1, st.bias2])
    np.savez(f"{out_path}.rank{rank}.npz", **out)
    torch.distributed.barrier()
    eng.close()


if __name__ == "__main__":
    main()
