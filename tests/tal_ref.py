"""The task-aligned target assignment (the rule in include/tinyfaces_hip.h, "TAL") restated in numpy float64, operation for operation.  Test
infrastructure only: tests/test_tal.py checks it by hand and by property, tests/test_gpu_tal.py holds tf_targets_tal to it bit for bit.

exp and pow are not bit-reproducible between numpy and the device, so the restatement also reports where a decision hangs on less than that:
per face the relative gap between its last winner and its first loser (`cut_gap`) and the relative gap of u at every conflict it takes part in
(`conflict_gap`).  A face is AMBIGUOUS where such a gap is below AMBIGUOUS_GAP and the two sides do not have bit-identical operands (identical
operands tie exactly on every platform and the index decides; so do two logits below -710, whose sigmoid is exactly 0)."""
import numpy as np

from oracle import targets as otgt

import atss_ref

BOX_CLIP = 4.135166556742356                                          # log(1000 / 16) as the kernel spells it
AMBIGUOUS_GAP = 1e-9
MUTANTS = ("anchor_iou", "no_clamp", "ge_inside", "conflict_m", "topk_plus_1")


def _rel_gap(a, b):
    hi = max(abs(a), abs(b))
    return 0.0 if hi == 0 else abs(a - b) / hi


def face_candidates(out, box, templates, pad, alpha, beta, rf, hm, mutant=None, exp=np.exp):
    """Steps 1-2 for one face.  out: (5 nt, vsy, vsx) float32.  Returns the arrays flat ((t * vsy + y) * vsx + x), m, u and ops (the
    (z, pw, ph) each m and u were formed from), candidates only, in flat order."""
    ofy, ofx = rf["offset"]
    sty, stx = rf["stride"]
    vsy, vsx = hm
    nt = templates.shape[0]
    fx1, fy1, fx2, fy2 = (float(c) for c in box)
    fcx, fcy = (fx1 + fx2) / 2, (fy1 + fy2) / 2
    bw, bh = fx2 - fx1 + 1, fy2 - fy1 + 1
    barea = bw * bh
    gx1, gx2, gy1, gy2 = fcx - bw / 2, fcx + bw / 2, fcy - bh / 2, fcy + bh / 2
    cx = ofx + np.arange(vsx) * (stx / 1)
    cy = ofy + np.arange(vsy) * (sty / 1)
    rects, any_inside = [], False
    for t in range(nt):
        dx1, dy1, dx2, dy2 = (float(c) for c in templates[t, :4])
        acx, acy = ((dx1 + cx) + (dx2 + cx)) / 2, ((dy1 + cy) + (dy2 + cy)) / 2
        if mutant == "ge_inside":
            inx, iny = (fx1 <= acx) & (acx <= fx2), (fy1 <= acy) & (acy <= fy2)
        else:
            inx, iny = (fx1 < acx) & (acx < fx2), (fy1 < acy) & (acy < fy2)
        ins = iny[:, None] & inx[None, :] & ~pad[:, :, t]
        any_inside |= bool(ins.any())
        rects.append((ins, acx, acy))
    flat, ms, us, ops = [], [], [], []
    for t in range(nt):
        ins, acx, acy = rects[t]
        if any_inside:
            ys, xs = np.nonzero(ins)
        else:                                                         # the nearest unpadded cell of this template, ATSS's order
            ys, xs = np.nonzero(~pad[:, :, t])
            if ys.size:
                ex, ey = (acx - fcx) * (acx - fcx), (acy - fcy) * (acy - fcy)
                d = ex[None, :] + ey[:, None]
                o = np.lexsort((ys * vsx + xs, d[ys, xs]))[:1]
                ys, xs = ys[o], xs[o]
        if ys.size == 0:
            continue
        dx1, dy1, dx2, dy2 = (float(c) for c in templates[t, :4])
        dw, dh = dx2 - dx1 + 1, dy2 - dy1 + 1
        z = out[t, ys, xs].astype(np.float64)
        px, py, pw, ph = (out[(c + 1) * nt + t, ys, xs].astype(np.float64) for c in range(4))
        with np.errstate(all="ignore"):
            if mutant == "anchor_iou":
                px, py, pw, ph = (np.where(np.isfinite(v), 0.0, v) for v in (px, py, pw, ph))
            pwc, phc = (pw, ph) if mutant == "no_clamp" else (np.minimum(np.maximum(pw, -BOX_CLIP), BOX_CLIP), np.minimum(np.maximum(ph, -BOX_CLIP), BOX_CLIP))
            bcx, bcy = cx[xs] + px * dw, cy[ys] + py * dh
            w, h = dw * exp(pwc), dh * exp(phc)
            hx, hy = w / 2, h / 2
            iw = np.minimum(bcx + hx, gx2) - np.maximum(bcx - hx, gx1)
            ih = np.minimum(bcy + hy, gy2) - np.maximum(bcy - hy, gy1)
            ia = iw * ih
            u = np.where((iw > 0) & (ih > 0), ia / (w * h + barea - ia), 0.0)
            s = 1 / (1 + exp(-z))
            m = np.power(s, alpha) * np.power(u, beta)
            ok = np.isfinite(z) & np.isfinite(px) & np.isfinite(py) & np.isfinite(pw) & np.isfinite(ph) & (u > 0) & np.isfinite(m)
        flat.append(((t * vsy + ys) * vsx + xs)[ok])
        ms.append(m[ok]); us.append(u[ok]); ops.append(np.stack([z, pw, ph], 1)[ok])
    if not flat:
        return np.zeros(0, np.int64), np.zeros(0), np.zeros(0), np.zeros((0, 3))
    flat, ms, us, ops = np.concatenate(flat), np.concatenate(ms), np.concatenate(us), np.concatenate(ops)
    o = np.argsort(flat, kind="stable")
    return flat[o], ms[o], us[o], ops[o]


def tal_maps(out, class_map, regression_map, boxes, templates, paste=None, flip=0, topk=13, alpha=1.0, beta=6.0, rf=otgt.RF, hm=otgt.HEATMAP_SIZE,
             details=False, mutant=None, exp=np.exp):
    """One image, device layout: out (5 nt, vsy, vsx) f32, class_map (nt, vsy, vsx) f32 and regression_map (4 nt, vsy, vsx) f32 = the base maps.
    -> copies of the two maps with the won anchors written, match_count (G,) int32 [, the per-face dicts: winners (flat), m, u, cut (the m of the
    last winner), near (the flat indices with m >= cut (1 - AMBIGUOUS_GAP)), cut_gap, conflict_gap, ambiguous]."""
    templates = np.asarray(templates, dtype=np.float64)
    out = np.asarray(out, dtype=np.float32)
    boxes = atss_ref.valid(boxes)
    vsy, vsx = hm
    nt, G = templates.shape[0], boxes.shape[0]
    ofy, ofx = rf["offset"]
    sty, stx = rf["stride"]
    pad = atss_ref.padding(templates, paste, flip, rf, hm)
    k = topk + 1 if mutant == "topk_plus_1" else topk
    faces = []
    for g in range(G):
        flat, m, u, ops = face_candidates(out, boxes[g], templates, pad, alpha, beta, rf, hm, mutant, exp)
        order = np.lexsort((flat, -m))                                # m descending, then the lower flat index
        win, lose = order[:k], order[k:]
        f = dict(winners=flat[win], m=m[win], u=u[win], ops=ops[win], cut=float(m[win[-1]]) if win.size else 0.0, cut_gap=np.inf,
                 conflict_gap=np.inf, ambiguous=False, near=flat[win])
        if win.size and lose.size:
            a, b = win[-1], lose[0]
            f["cut_gap"] = _rel_gap(m[a], m[b])
            same = m[a] == m[b] and u[a] == u[b] and np.array_equal(ops[a], ops[b])
            same = same or (alpha > 0 and ops[a][0] < -710 and ops[b][0] < -710)       # exp(-z) overflows: s and m are exactly 0 on every platform
            f["ambiguous"] = bool(f["cut_gap"] < AMBIGUOUS_GAP and not same)
            f["near"] = flat[m >= f["cut"] * (1 - AMBIGUOUS_GAP)]
        faces.append(f)
    claims = {}
    for g, f in enumerate(faces):
        for i, a in enumerate(f["winners"]):
            claims.setdefault(int(a), []).append((g, i))
    cm, rm = np.array(class_map, dtype=np.float32), np.array(regression_map, dtype=np.float32)
    counts = np.zeros(G, dtype=np.int32)
    key = "m" if mutant == "conflict_m" else "u"
    for a, cl in claims.items():
        best = cl[0]                                                  # ascending g with a strict > : the lower g keeps a tie
        for c in cl[1:]:
            if faces[c[0]][key][c[1]] > faces[best[0]][key][best[1]]:
                best = c
        for c in cl:
            if c is best or len(cl) == 1:
                continue
            fa, fb = faces[c[0]], faces[best[0]]
            gap = _rel_gap(fa["u"][c[1]], fb["u"][best[1]])
            same = fa["u"][c[1]] == fb["u"][best[1]] and np.array_equal(fa["ops"][c[1]][1:], fb["ops"][best[1]][1:])
            for f in (fa, fb):
                f["conflict_gap"] = min(f["conflict_gap"], gap)
                f["ambiguous"] = bool(f["ambiguous"] or (gap < AMBIGUOUS_GAP and not same))
        g = best[0]
        t, cell = divmod(a, vsy * vsx)
        y, x = divmod(cell, vsx)
        fx1, fy1, fx2, fy2 = boxes[g]
        dw, dh = templates[t, 2] - templates[t, 0] + 1, templates[t, 3] - templates[t, 1] + 1
        cm[t, y, x] = 1
        rm[t, y, x] = ((fx1 + fx2) / 2 - (ofx + x * stx)) / dw        # get_regression (processor.py:181-191)
        rm[nt + t, y, x] = ((fy1 + fy2) / 2 - (ofy + y * sty)) / dh
        rm[2 * nt + t, y, x] = np.log((fx2 - fx1 + 1) / dw)
        rm[3 * nt + t, y, x] = np.log((fy2 - fy1 + 1) / dh)
        counts[g] += 1
    return (cm, rm, counts, faces) if details else (cm, rm, counts)


def base_maps(templates, paste=None, flip=0, rf=otgt.RF, hm=otgt.HEATMAP_SIZE):
    """The maps of an image without faces as the loaders deliver them (the dense_overlap path with no box), device layout: every label -1
    -- padded anchors too: the reference's padding only turns labels that are not negative, as ATSS's maps show --, regression map 0."""
    nt = np.asarray(templates).shape[0]
    return -np.ones((nt,) + tuple(hm), dtype=np.float32), np.zeros((4 * nt,) + tuple(hm), dtype=np.float32)


def regression_target(box, template, y, x, rf=otgt.RF):
    """get_regression's four values of `box` at cell (y, x) of `template`, float64."""
    fx1, fy1, fx2, fy2 = (float(c) for c in box)
    dw, dh = template[2] - template[0] + 1, template[3] - template[1] + 1
    return np.array([((fx1 + fx2) / 2 - (rf["offset"][1] + x * rf["stride"][1])) / dw, ((fy1 + fy2) / 2 - (rf["offset"][0] + y * rf["stride"][0])) / dh,
                     np.log((fx2 - fx1 + 1) / dw), np.log((fy2 - fy1 + 1) / dh)])


def ulp_exp(seed):
    """np.exp moved by one ulp up or down, at random: what another math library may return."""
    rng = np.random.RandomState(seed)

    def f(v):
        with np.errstate(all="ignore"):
            e = np.exp(v)
        return np.nextafter(e, np.where(rng.rand(*np.shape(e)) < 0.5, -np.inf, np.inf))
    return f


def compare(got, want_details, hm):
    """Hold one image's device result (cm, rm, mc) to the restatement's (cm, rm, mc, faces): equal everywhere, except that an AMBIGUOUS face
    only has to win as many anchors and each of them with a restated m of at least its cut (1 - AMBIGUOUS_GAP).  Returns the number of
    ambiguous faces; raises AssertionError otherwise."""
    gcm, grm, gmc = got
    wcm, wrm, wmc, faces = want_details
    amb = [g for g, f in enumerate(faces) if f["ambiguous"]]
    if not amb:
        assert np.array_equal(gcm, wcm), f"class map differs at {np.argwhere(gcm != wcm)[:5].tolist()}"
        assert np.array_equal(grm, wrm), f"regression map differs at {np.argwhere(grm != wrm)[:5].tolist()}"
        assert np.array_equal(gmc, wmc), f"match_count {gmc.tolist()} != {wmc.tolist()}"
        return 0
    free = np.zeros(wcm.size, dtype=bool)                             # the anchors an ambiguous face may or may not hold
    for g in amb:
        free[faces[g]["near"]] = True
        if faces[g]["conflict_gap"] >= AMBIGUOUS_GAP:                  # only its cut is in doubt: the number of winners is not
            assert int(gmc[g]) == int(wmc[g]), f"ambiguous face {g} won {gmc[g]} anchors, the restatement {wmc[g]}"
        assert int(gmc[g]) <= len(faces[g]["winners"]), f"ambiguous face {g} won {gmc[g]} anchors, more than its {len(faces[g]['winners'])} claims"
    keep = ~free.reshape(wcm.shape)                                   # outside: equal, so a device winner is a restated winner or in a near set
    keep4 = np.tile(keep, (4, 1, 1))
    assert np.array_equal(gcm[keep], wcm[keep]) and np.array_equal(grm[keep4], wrm[keep4])
    rest = [g for g, f in enumerate(faces) if not free[f["winners"]].any()]
    assert np.array_equal(gmc[rest], wmc[rest])
    return len(amb)
