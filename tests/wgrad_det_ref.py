"""numpy restatement of the deterministic weight gradients' contract (include/tinyfaces_hip.h at tf_conv2d_wgrad_det): THE PLAN -- how many
split-K slices a call makes, which pixels each one owns, how a slab that is too small caps them -- and THE ORDER in which the summing kernel
adds the slices of one output element.  Nothing here reads the library: tests/test_wgrad_det.py checks the restatement against planted
values, tests/test_gpu_wgrad_det.py checks the kernels against the restatement bit for bit."""
import numpy as np

# (pixels per stage, channels per tile side, block target of the automatic split, fewest stages per block) of the three kernels
KERNELS = {
    "dma": dict(PK=64, BC=64, target=512, min_stages=4),              # wgrad_dma_kernel: bf16, no prologue (tile 0 | 1)
    "reg64_bf16": dict(PK=64, BC=64, target=640, min_stages=4),       # wgrad_kernel<bf16, 64> (tile 64; tile 0 with a prologue)
    "reg128_bf16": dict(PK=64, BC=128, target=640, min_stages=4),
    "reg64_f32": dict(PK=32, BC=64, target=640, min_stages=4),        # wgrad_kernel<float, 64> (tile 0 | 64)
    "reg128_f32": dict(PK=32, BC=128, target=640, min_stages=4),
    "all_taps": dict(PK=64, BC=64, target=128, min_stages=6),         # wgrad3x3_kernel: M is the zero-padded raster N * (H+2) * (W+2)
}


def cdiv(a, b):
    return -(-a // b)


def tiles(kernel, Cin, Cout, taps):
    """Output tiles of one slice (the all-taps kernel holds its nine taps inside a tile)."""
    bc = KERNELS[kernel]["BC"]
    return cdiv(Cout, bc) * cdiv(Cin, bc) * (1 if kernel == "all_taps" else taps)


def slice_bytes(kernel, Cin, Cout, taps):
    bc = KERNELS[kernel]["BC"]
    return tiles(kernel, Cin, Cout, taps) * bc * bc * 4 * (9 if kernel == "all_taps" else 1)


def requested_slices(kernel, M, Cin, Cout, taps, splitk=0):
    """sk of the contract before the cap: the caller's, or the kernel's own choice."""
    if splitk > 0:
        return splitk
    k = KERNELS[kernel]
    sk = cdiv(k["target"], tiles(kernel, Cin, Cout, taps))
    return max(1, min(sk, cdiv(M, k["min_stages"] * k["PK"])))


def plan(kernel, M, Cin, Cout, taps, splitk=0, slab_bytes=None):
    """[(first pixel, one past the last pixel)] of every slice; None when not even one slice fits the slab (TF_ERR_ARG)."""
    pk = KERNELS[kernel]["PK"]
    sk = requested_slices(kernel, M, Cin, Cout, taps, splitk)
    if slab_bytes is not None:
        fit = slab_bytes // slice_bytes(kernel, Cin, Cout, taps)
        if fit < 1:
            return None
        sk = min(sk, fit)
    chunk = cdiv(cdiv(M, sk), pk) * pk
    n = cdiv(M, chunk)
    return [(s * chunk, min(M, (s + 1) * chunk)) for s in range(n)]


def preferred_bytes(kernel, M, Cin, Cout, taps, splitk=0):
    return len(plan(kernel, M, Cin, Cout, taps, splitk)) * slice_bytes(kernel, Cin, Cout, taps)


def groups(slices):
    """tf_wgrad_det_groups."""
    return 16 if slices >= 128 else 4 if slices >= 32 else 2 if slices >= 16 else 1


def ordered_sum(partials):
    """partials [slices, ...] fp32 -> the total the summing kernel forms, fp32, every add rounded."""
    p = np.asarray(partials, dtype=np.float32)
    n, G = p.shape[0], groups(p.shape[0])
    t = []
    for g in range(G):
        acc = np.zeros(p.shape[1:], np.float32)
        for s in range(g, n, G):
            acc = (acc + p[s]).astype(np.float32)
        t.append(acc)
    total = t[0]
    for g in range(1, G):
        total = (total + t[g]).astype(np.float32)
    return total


def reduce_into(dw_in, partials, row_scale=None):
    """dw = dw_in + row_scale * total, each step rounded to fp32 (row_scale broadcasts over the leading, output-channel axis)."""
    total = ordered_sum(partials)
    if row_scale is not None:
        rs = np.asarray(row_scale, np.float32).reshape((-1,) + (1,) * (total.ndim - 1))
        total = (total * rs).astype(np.float32)
    return (np.asarray(dw_in, np.float32) + total).astype(np.float32)
