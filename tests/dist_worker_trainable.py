"""Worker of tests/test_gpu_trainable_layers.py: one data-parallel rank of the fused TrainEngine with the BatchNorm of the trunk frozen AND the
stem, layer 1 and layer 2 frozen (DetectionModel.set_trainable_layers(1)) on a ResNet-50 trunk -- gloo rendezvous, every rank on cuda:0 of a
1-GPU box.  Rank r trains on micro-batch r % 2 for STEPS steps; rank 0 writes the flat parameter buffer after every step."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tiny-faces-pytorch_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

TRAINABLE_LAYERS = 1


def build(golden_path):
    import dist_worker_trunks
    m, c, batches = dist_worker_trunks.build(golden_path)
    return m.freeze_batchnorm().set_trainable_layers(TRAINABLE_LAYERS), c, batches


def main():
    golden_path, out_path, steps = sys.argv[1], sys.argv[2], int(sys.argv[3])
    from tinyfaces import parallel
    from tinyfaces.engine import TrainEngine
    parallel.init_from_env("gloo")
    rank = parallel.rank()
    torch.cuda.set_device(0)
    m, c, batches = build(golden_path)
    eng = TrainEngine(m, c, lr=1e-4, momentum=0.9, weight_decay=5e-4, device="cuda:0", bucket_mb=10)
    assert eng.model.batchnorm_frozen and eng.model.trainable_layers == TRAINABLE_LAYERS
    ranges = eng._overlap["ranges"]                       # the bucket plan is the full model's: the frozen ranges are reduced as zeros
    assert ranges[-1][0] == -1 and ranges[-1][1] == 0
    img, cm, rm = [t.cuda() for t in batches[rank % 2]]
    snaps = []
    for s in range(steps):
        eng.step(img, cm.clone(), rm)
        torch.cuda.synchronize()
        snaps.append(eng.flat_p.detach().cpu().numpy().copy())
    if rank == 0:
        np.savez(out_path, *snaps, buckets=np.array(len(ranges)))
    torch.distributed.barrier()
    eng.close()


if __name__ == "__main__":
    main()
