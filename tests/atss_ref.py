"""The ATSS target assignment (the rule in include/tinyfaces_hip.h, "ATSS") restated in numpy float64, operation for operation: serial sums in
list order, the rule's own tie rules, no rounding and no noise.  Test infrastructure only: tests/test_atss.py checks it by hand and by
property, tests/test_gpu_atss.py holds tf_targets_atss to it bit for bit."""
import numpy as np

from oracle import targets as otgt

NO_PASTE = [-10 ** 6, -10 ** 6, 10 ** 6, 10 ** 6]


def valid(boxes):
    """The non-degenerate rows (processor.py:228-232), in input order."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    return b[~((b[:, 2] <= b[:, 0]) | (b[:, 3] <= b[:, 1]))]


def padding(templates, paste, flip, rf, hm):
    pad = otgt.get_padding(templates, NO_PASTE if paste is None else paste, rf, hm)
    return np.fliplr(pad) if (flip and paste is not None) else pad


def face_claims(box, templates, pad, k, rf, hm):
    """Steps 1-5 for one face.  Returns a dict: cand = [(t, y, x)] in list order, v = their IoUs, mean, var, passing = the positions that pass
    step 3, positive = those of step 4, fallback = the position of step 5 or None, claims = the positions the face claims."""
    ofy, ofx = rf["offset"]
    sty, stx = rf["stride"]
    vsy, vsx = hm
    fx1, fy1, fx2, fy2 = (float(c) for c in box)
    fcx, fcy = (fx1 + fx2) / 2, (fy1 + fy2) / 2
    barea = (fx2 - fx1 + 1) * (fy2 - fy1 + 1)
    cx = ofx + np.arange(vsx) * (stx / 1)
    cy = ofy + np.arange(vsy) * (sty / 1)
    cand, v, centres = [], [], []
    for t in range(templates.shape[0]):
        dx1, dy1, dx2, dy2 = (float(c) for c in templates[t, :4])
        ax1, ay1, ax2, ay2 = dx1 + cx, dy1 + cy, dx2 + cx, dy2 + cy
        acx, acy = (ax1 + ax2) / 2, (ay1 + ay2) / 2
        ex, ey = (acx - fcx) * (acx - fcx), (acy - fcy) * (acy - fcy)
        d = ex[None, :] + ey[:, None]                                 # (vsy, vsx): the x term first
        ys, xs = np.nonzero(~pad[:, :, t])
        cell = ys * vsx + xs
        order = np.lexsort((cell, d[ys, xs]))[:k]                     # distance ascending, then the lower cell index
        farea = (dx2 - dx1 + 1) * (dy2 - dy1 + 1)
        for o in order:
            y, x = int(ys[o]), int(xs[o])
            iw = min(ax2[x], fx2) - max(ax1[x], fx1) + 1
            ih = min(ay2[y], fy2) - max(ay1[y], fy1) + 1
            ov = 0.0
            if ih > 0 and iw > 0:
                ia = iw * ih
                ov = ia / (farea + barea - ia)
            cand.append((t, y, x))
            v.append(float(ov))
            centres.append((float(acx[x]), float(acy[y])))
    n = len(cand)
    out = dict(cand=cand, v=v, mean=0.0, var=0.0, passing=[], positive=[], fallback=None, claims=[])
    if n == 0:
        return out
    s = 0.0
    for u in v:
        s = s + u
    mean = s / n
    acc = 0.0
    for u in v:
        acc = acc + (u - mean) * (u - mean)
    var = acc / (n - 1) if n > 1 else 0.0
    passing = [i for i, u in enumerate(v) if (u - mean) >= 0 and (u - mean) * (u - mean) >= var]
    positive = [i for i in passing if fx1 < centres[i][0] < fx2 and fy1 < centres[i][1] < fy2]
    fallback = None
    if not positive:
        fallback = int(np.argmax(np.asarray(v)))                      # the first of the largest
    out.update(mean=mean, var=var, passing=passing, positive=positive, fallback=fallback, claims=positive if positive else [fallback])
    return out


def atss_maps(boxes, templates, paste=None, flip=0, k=9, rf=otgt.RF, hm=otgt.HEATMAP_SIZE, details=False):
    """One image -> class_map (vsy, vsx, nt) float64 in {-1, +1}, regression_map (vsy, vsx, 4 nt) float32, match_count (G,) int32
    [, the per-face dicts of face_claims and the owner map (vsy, vsx, nt), -1 = nobody]."""
    templates = np.asarray(templates, dtype=np.float64)
    boxes = valid(boxes)
    vsy, vsx = hm
    nt, G = templates.shape[0], boxes.shape[0]
    ofy, ofx = rf["offset"]
    sty, stx = rf["stride"]
    pad = padding(templates, paste, flip, rf, hm)
    cm = -np.ones((vsy, vsx, nt))
    rm = np.zeros((vsy, vsx, 4 * nt), dtype=np.float32)
    owner = -np.ones((vsy, vsx, nt), dtype=np.int64)
    best = np.zeros((vsy, vsx, nt))
    faces = [face_claims(boxes[g], templates, pad, k, rf, hm) for g in range(G)]
    for g, f in enumerate(faces):                                     # ascending g with a strict > : the lower g keeps a tie
        for i in f["claims"]:
            t, y, x = f["cand"][i]
            if owner[y, x, t] < 0 or f["v"][i] > best[y, x, t]:
                owner[y, x, t], best[y, x, t] = g, f["v"][i]
    counts = np.zeros(G, dtype=np.int32)
    for y, x, t in zip(*np.nonzero(owner >= 0)):
        g = int(owner[y, x, t])
        fx1, fy1, fx2, fy2 = boxes[g]
        dw, dh = templates[t, 2] - templates[t, 0] + 1, templates[t, 3] - templates[t, 1] + 1
        cm[y, x, t] = 1
        rm[y, x, t] = ((fx1 + fx2) / 2 - (ofx + x * stx)) / dw         # get_regression (processor.py:181-191)
        rm[y, x, nt + t] = ((fy1 + fy2) / 2 - (ofy + y * sty)) / dh
        rm[y, x, 2 * nt + t] = np.log((fx2 - fx1 + 1) / dw)
        rm[y, x, 3 * nt + t] = np.log((fy2 - fy1 + 1) / dh)
        counts[g] += 1
    return (cm, rm, counts, faces, owner) if details else (cm, rm, counts)
