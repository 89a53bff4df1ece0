"""Worker of tests/test_gpu_grad_clip.py: one data-parallel rank of the fused TrainEngine with gradient-norm clipping and the non-finite-step
guard, on the model of tests/dist_worker_trainable.py (ResNet-50, fp32, BatchNorm and the lower stages frozen; gloo rendezvous, every rank on
cuda:0 of a 1-GPU box).  Rank r trains on micro-batch r % 2: one clipped step at max_grad_norm = argv[3], then one step whose gradient
carries ONE NaN planted on rank 1 alone (behind the real backward pass, in front of the exchange), then one clean step.  Every rank writes
what it saw to <out>.rank<r>.npz."""
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
    golden_path, out_path, max_norm = sys.argv[1], sys.argv[2], float(sys.argv[3])
    from tinyfaces import parallel
    from tinyfaces.engine import TrainEngine
    parallel.init_from_env("gloo")
    rank = parallel.rank()
    torch.cuda.set_device(0)
    m, c, batches = build(golden_path)
    eng = TrainEngine(m, c, lr=1e-4, momentum=0.9, weight_decay=5e-4, device="cuda:0", bucket_mb=10, max_grad_norm=max_norm, skip_nonfinite=True)
    # the exchange of this test is the torch.distributed callback, issued from inside the backward call: the NaN has to be in the bucket
    # before its all-reduce is, so it is planted by the callback's own wrapper (rank 1, second step only)
    assert eng._native is None and eng._overlap is not None and not eng._use_comm_stream
    seg = m._segments
    victim = seg["model.layer3.2.conv2.weight"][0] + 17
    plant, planted_at = [False], []
    on_bucket = eng._on_bucket

    def planted(block, stream_ptr, user):
        try:
            start, end = eng._block_range[block]
            if plant[0] and start <= victim < end:
                cur = torch.cuda.current_stream(eng.device)
                own = (stream_ptr or 0) == cur.cuda_stream
                with torch.cuda.stream(cur if own else torch.cuda.ExternalStream(stream_ptr, device=eng.device)):
                    m._grad_flat_persistent[victim] = float("nan")        # behind the bucket's last gradient kernel, in front of its all-reduce
                planted_at.append(block)
        except BaseException as e:       # (nothing may unwind through the executor's C frames)
            eng._cb_error = e
        on_bucket(block, stream_ptr, user)

    import ctypes as C
    eng._cb = C.CFUNCTYPE(None, C.c_int, C.c_void_p, C.c_void_p)(planted)
    m._grad_callback = eng._cb
    img, cm, rm = [t.cuda() for t in batches[rank % 2]]
    out = {}
    for s in range(3):
        plant[0] = s == 1 and rank == 1
        eng.step(img, cm.clone(), rm)
        torch.cuda.synchronize()
        st = eng._clip_state.read()
        out[f"p{s}"] = eng.flat_p.detach().cpu().numpy().copy()
        out[f"m{s}"] = eng.flat_m.detach().cpu().numpy().copy()
        out[f"state{s}"] = np.array([st.sumsq, st.norm, st.coef, st.skip, st.skipped], dtype=np.float64)
        out[f"norm{s}"] = np.array(float(eng.last_grad_norm))
        out[f"skipped{s}"] = np.array(eng.skipped_steps)
    assert len(planted_at) == (1 if rank == 1 else 0), planted_at
    np.savez(f"{out_path}.rank{rank}.npz", **out)
    torch.distributed.barrier()
    eng.close()


if __name__ == "__main__":
    main()
