"""TEST INFRASTRUCTURE ONLY.  numpy restatement of the colour jitter of include/tinyfaces_hip.h (tf_image_prepare_jitter):
torchvision.transforms.ColorJitter on a PIL image = Pillow's ImageEnhance (Image.blend against a degenerate image) and, for the hue,
a round trip through Pillow's "HSV" mode.  Every function maps uint8 (H, W, 3) to uint8 (H, W, 3).  tests/test_color_jitter.py pins each
piece to Pillow itself; tests/test_gpu_color_jitter.py compares the kernel with it bit for bit."""
import numpy as np

KINDS = ("brightness", "contrast", "saturation", "hue")
F32 = np.float32


def blend(d, x, f):
    """Image.blend(degenerate d, image x, factor f) per channel: t = f32(d) + f32(f) * (f32(x) - f32(d)); 0 <= f <= 1: truncated;
    otherwise clipped to 0 ... 255, then truncated."""
    d, x = np.broadcast_arrays(np.asarray(d), np.asarray(x))
    f = F32(f)
    d, x = d.astype(F32), x.astype(F32)
    t = (d + (f * (x - d)).astype(F32)).astype(F32)
    if 0.0 <= f <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    out = np.where(t <= 0, 0, np.where(t >= 255, 255, np.minimum(np.maximum(t, 0), 255).astype(np.int32)))
    return out.astype(np.uint8)


def luma(img):
    """Pillow's RGB -> L: (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16."""
    i = img.astype(np.int64)
    return ((i[..., 0] * 19595 + i[..., 1] * 38470 + i[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def mean_int(S, n):
    """floor(S / n + 0.5) in integers (what the kernel computes)."""
    return (2 * int(S) + int(n)) // (2 * int(n))


def mean_double(S, n):
    """ImageEnhance.Contrast: int(ImageStat.Stat(L).mean[0] + 0.5), in Python floats."""
    return int(int(S) / int(n) + 0.5)


def brightness(img, f):
    return blend(0, img, f)


def saturation(img, f):
    return blend(luma(img)[..., None], img, f)


def contrast_mean(img):
    l = luma(img)
    return mean_int(int(l.astype(np.int64).sum()), l.size)


def contrast(img, f):
    return blend(contrast_mean(img), img, f)


def rgb_to_hsv(img):
    """Pillow's rgb2hsv (src/libImaging/Convert.c): s and rc / gc / bc in float32, the hue through double."""
    r, g, b = (img[..., c].astype(np.int32) for c in range(3))
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = mx == mn
    with np.errstate(all="ignore"):
        cr = (mx - mn).astype(F32)
        s = cr / mx.astype(F32)
        rc, gc, bc = ((mx - c).astype(F32) / cr for c in (r, g, b))
        rc64, gc64, bc64 = rc.astype(np.float64), gc.astype(np.float64), bc.astype(np.float64)
        h = np.where(r == mx, bc64 - gc64, np.where(g == mx, 2.0 + rc64 - bc64, 4.0 + gc64 - rc64)).astype(F32)
        h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(F32)
        uh = np.clip((h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
        us = np.clip((s * F32(255.0)).astype(F32).astype(np.int64), 0, 255)
    uh, us = np.where(grey, 0, uh), np.where(grey, 0, us)
    return np.stack([uh, us, mx], -1).astype(np.uint8)


def hsv_to_rgb(hsv):
    """Pillow's hsv2rgb, evaluated in double (float32 gives the same bytes on all 2^24 inputs)."""
    h, s, v = (hsv[..., c].astype(np.float64) for c in range(3))
    fh = h * 6.0 / 255.0
    i = np.floor(fh)
    f = fh - i
    fs = s / 255.0

    def rnd(x):
        return np.clip(np.floor(x + 0.5), 0, 255)
    p, q, t = rnd(v * (1.0 - fs)), rnd(v * (1.0 - fs * f)), rnd(v * (1.0 - fs * (1.0 - f)))
    k = i.astype(np.int64) % 6
    table = [(v, t, p), (q, v, p), (p, v, t), (p, q, v), (t, p, v), (v, p, q)]
    out = np.zeros(hsv.shape, np.float64)
    for n, (rr, gg, bb) in enumerate(table):
        m = k == n
        out[..., 0][m], out[..., 1][m], out[..., 2][m] = rr[m], gg[m], bb[m]
    grey = hsv[..., 1] == 0
    out[grey] = v[grey][..., None]
    return out.astype(np.uint8)


def hue_shift_of(hue_factor):
    """torchvision's `np_h += np.uint8(hue_factor * 255)`: truncated toward zero, modulo 256."""
    return int(hue_factor * 255) % 256


def hue(img, shift):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + int(shift)) & 255).astype(np.uint8)
    return hsv_to_rgb(hsv)


def apply_chain(img, chain):
    """chain: [(kind, factor)] in application order; for "hue" the factor is the hue_factor in [-0.5, 0.5]."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    for kind, f in chain:
        if kind == "brightness":
            img = brightness(img, f)
        elif kind == "contrast":
            img = contrast(img, f)
        elif kind == "saturation":
            img = saturation(img, f)
        elif kind == "hue":
            img = hue(img, hue_shift_of(f))
        else:
            raise ValueError(kind)
    return img
