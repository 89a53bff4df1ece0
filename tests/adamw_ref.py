"""numpy float32 restatement of the fused AdamW step (include/tinyfaces_hip.h, csrc/adamw.hip), operation for operation:

    host, in double, each rounded once to float32:
        decay = 1 - lr * wd      w1 = 1 - beta1      b2 = beta2      w2 = 1 - beta2      e = eps
    uniform, in double from the step counter:
        bias1 = 1 - pow_int(beta1, step)      bias2 = 1 - pow_int(beta2, step)
        ss = float32(lr / bias1)              c2 = float32(sqrt(bias2))
        gs = float32(grad_scale) [* float32(coef): one fp32 product]
    per element, every line one fp32 operation:
        g = grad * gs
        p = p * decay
        m = fmaf(w1, g - m, m)
        v = (b2 * v) + ((w2 * g) * g)
        d = (sqrt(v) / c2) + e
        p = p - ss * (m / d)
        ema = fmaf(ema_weight, p - ema, ema)

Everything is np.float32, scalars and arrays alike; the two fused lines go through the exactly rounded fmaf of tests/test_gpu_model_ema.py
(`_fmaf`, which also asserts that it equals torch.lerp for a weight below 0.5).  `pow_int` is the device's square-and-multiply, least significant
bit first, every product a double-double product built from plain double operations, so the bias corrections are equal to the device's to
the bit and beta ** t is right to about one ulp for every step count."""
import math

import numpy as np
import torch

F = np.float32


_SPLIT = 134217729.0                                                            # 2^27 + 1 (Veltkamp)


def _two_prod(a, b):
    """(p, e) with p = fl(a * b) and p + e = a * b exactly (Dekker), in plain double operations."""
    p = a * b
    ca = _SPLIT * a
    ah = ca - (ca - a)
    al = a - ah
    cb = _SPLIT * b
    bh = cb - (cb - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def _dd_mul(xh, xl, yh, yl):
    """The product of the double-double values (xh, xl) and (yh, yl), renormalised."""
    p, e = _two_prod(xh, yh)
    e = e + (xh * yl + xl * yh)
    s = p + e
    return s, e - (s - p)


def pow_int(beta, t):
    """beta ** t as the device computes it: square-and-multiply, least significant bit first, every product a double-double product
    built from plain double operations; the high word of the result."""
    rh, rl, xh, xl, t = 1.0, 0.0, float(beta), 0.0, int(t)
    while t:
        if t & 1:
            rh, rl = _dd_mul(rh, rl, xh, xl)
        xh, xl = _dd_mul(xh, xl, xh, xl)
        t >>= 1
    return rh


def bias_corrections(betas, step):
    """(bias1, bias2) in double for the step counter `step` (>= 1): what tf_adamw_advance leaves in the device state."""
    return 1.0 - pow_int(betas[0], step), 1.0 - pow_int(betas[1], step)


def fmaf(w, b, c):
    """fmaf(w, b - c, c) on float32 arrays b, c and the float32 scalar w, exactly rounded."""
    from test_gpu_model_ema import _fmaf
    r, _ = _fmaf(torch.from_numpy(np.ascontiguousarray(c, dtype=F)), torch.from_numpy(np.ascontiguousarray(b, dtype=F)), float(F(w)))
    return r.numpy()


def adamw_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0, coef=None):
    """One update with the step counter ALREADY advanced to `step`.  p, g, m, v: float32 arrays of one shape; coef: the fp32 clip coefficient
    or None.  Returns the new (p, m, v)."""
    p, g, m, v = (np.asarray(t, dtype=F) for t in (p, g, m, v))
    lr, b1, b2, eps, wd = float(lr), float(betas[0]), float(betas[1]), float(eps), float(weight_decay)
    decay, w1, fb2, w2, e = F(1.0 - lr * wd), F(1.0 - b1), F(b2), F(1.0 - b2), F(eps)
    bias1, bias2 = bias_corrections((b1, b2), step)
    ss, c2 = F(lr / bias1), F(math.sqrt(bias2))
    gs = F(grad_scale)
    if coef is not None:
        gs = gs * F(coef)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        g = g * gs
        p = p * decay
        m = fmaf(w1, g, m)
        v = (fb2 * v) + ((w2 * g) * g)
        d = (np.sqrt(v) / c2) + e
        p = p - ss * (m / d)
    assert p.dtype == m.dtype == v.dtype == F
    return p, m, v


def ema_step(ema, p, weight):
    """ema = fmaf(weight, p - ema, ema) on the parameter the update has just produced."""
    return fmaf(F(weight), np.asarray(p, dtype=F), np.asarray(ema, dtype=F))
