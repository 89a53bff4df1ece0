"""Worker of tests/test_gpu_trunks.py: one data-parallel rank of the fused TrainEngine on a ResNet-50 trunk (gloo rendezvous, every rank on
cuda:0 of a 1-GPU box).  Rank r trains on micro-batch r % 2 for STEPS steps; rank 0 writes the flat parameter buffer after every step."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tiny-faces-pytorch_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def build(golden_path):
    from oracle.model import OracleDetectionModel, tame_init_
    from oracle.resnet import ResNet
    from tinyfaces.models import model as mm
    from tinyfaces.models.loss import DetectionCriterion
    g = np.load(golden_path, allow_pickle=False)
    batches = [(torch.from_numpy(g[f"b{i}_img"]), torch.from_numpy(g[f"b{i}_cm"].astype(np.float32)), torch.from_numpy(g[f"b{i}_rm"]).float())
               for i in range(2)]
    om = OracleDetectionModel(num_templates=25)
    om.model = ResNet((3, 4, 6, 3))
    del om.model.layer4
    m = mm.DetectionModel(base_model=mm.resnet50, num_templates=25)
    m.load_state_dict(tame_init_(om, 0).state_dict(), strict=True)
    m.set_compute_dtype(torch.float32)
    E = 25 * batches[0][1].shape[2] * batches[0][1].shape[3]
    keep = torch.ones(batches[0][0].shape[0], E, dtype=torch.uint8)
    keep[:, 128:] = 0                                     # deterministic balance sampling: the first 128 of each kind
    c = DetectionCriterion(25)
    c.inject_sampling(keep, keep)
    return m, c, batches


def main():
    golden_path, out_path, steps = sys.argv[1], sys.argv[2], int(sys.argv[3])
    from tinyfaces import _hip, parallel
    from tinyfaces.engine import TrainEngine
    parallel.init_from_env("gloo")
    rank = parallel.rank()
    torch.cuda.set_device(0)
    _hip.lib().tf_set_stat_rows(0)                        # reproducible BN statistics
    m, c, batches = build(golden_path)
    eng = TrainEngine(m, c, lr=1e-4, momentum=0.9, weight_decay=5e-4, device="cuda:0", bucket_mb=10)
    ranges = eng._overlap["ranges"]
    first_l3 = m.trunk[0] + m.trunk[1]
    assert ranges[-1][0] == -1 and all(first_l3 <= r[0] < sum(m.trunk) for r in ranges[:-1]), ranges
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
