"""The inputs tests/test_tal.py (CPU: the restatement alone) and tests/test_gpu_tal.py (the kernel against it) share: the seeded random
images and the planted ones, each with its restated result computed once.  A case is a dict: hm, t (templates), boxes / pastes / flips per
image, out (B, 5 nt, vsy, vsx) float32, cm / rm (the maps as they arrive, device layout), topk, alpha, beta."""
import functools
import os

import numpy as np

import tal_ref
from oracle import targets as otgt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# small template sets for the small maps (x1, y1, x2, y2, scale): 17 x 21, 9 x 11 and 33 x 41 pixels
T3 = np.array([[-8.0, -10.0, 8.0, 10.0, 1.0], [-4.0, -5.0, 4.0, 5.0, 1.0], [-16.0, -20.0, 16.0, 20.0, 1.0]])


def golden_templates():
    return np.load(os.path.join(GOLDEN, "targets.npz"), allow_pickle=False)["templates"]


def templates_for(nt):
    return {1: T3[:1], 2: T3[:2], 3: T3, 25: golden_templates()}[nt]


def many_templates(nt):
    """nt templates of widths 9 px upward in steps of 1 / 8 px (more than one tile of 64 templates)."""
    w = 4.0 + np.arange(nt) / 16.0
    return np.stack([-w, -np.round(1.25 * w, 3), w, np.round(1.25 * w, 3), np.ones(nt)], 1)


def faces(rng, g, hm):
    """g faces on the map: tiny, medium, hanging over the canvas, larger than the map, overlapping pairs."""
    vsy, vsx = hm
    W, H = 8.0 * vsx, 8.0 * vsy
    out = []
    for i in range(g):
        kind = i % 5
        if kind == 0:
            w, h = rng.uniform(4, 9, 2)
            x, y = rng.uniform(0, W - 8), rng.uniform(0, H - 8)
        elif kind == 1:
            w, h = rng.uniform(10, 40, 2)
            x, y = rng.uniform(-5, W - 5), rng.uniform(-5, H - 5)
        elif kind == 2:
            w, h = rng.uniform(6, 30, 2)
            x, y = rng.choice([-w / 2, W - w / 2, -2.0]), rng.choice([-h / 2, H - h / 2, -2.0])
        elif kind == 3:
            w, h = W * rng.uniform(0.3, 1.3), H * rng.uniform(0.3, 1.3)
            x, y = rng.uniform(-0.2 * w, W - 0.8 * w), rng.uniform(-0.2 * h, H - 0.8 * h)
        else:
            p = out[-1]
            dx, dy = rng.uniform(-4, 4, 2)
            out.append([p[0] + dx, p[1] + dy, p[2] + dx + 3, p[3] + dy + 2])
            continue
        out.append([x, y, x + w, y + h])
    return np.round(np.array(out, dtype=np.float64).reshape(-1, 4), 3)


def make(hm, t, boxes, out, pastes=None, flips=None, topk=13, alpha=1.0, beta=6.0, cm=None, rm=None, name=""):
    B = len(boxes)
    base = [tal_ref.base_maps(t, None if pastes is None else pastes[b], 0 if flips is None else flips[b], hm=hm) for b in range(B)]
    return dict(hm=hm, t=np.asarray(t, dtype=np.float64), boxes=[np.asarray(b, dtype=np.float64).reshape(-1, 4) for b in boxes], pastes=pastes, flips=flips,
                out=np.ascontiguousarray(out, dtype=np.float32), topk=topk, alpha=alpha, beta=beta, name=name,
                cm=np.stack([b[0] for b in base]) if cm is None else np.ascontiguousarray(cm, dtype=np.float32),
                rm=np.stack([b[1] for b in base]) if rm is None else np.ascontiguousarray(rm, dtype=np.float32))


def restate(case, mutant=None, exp=np.exp):
    """Per image (cm, rm, match_count, faces) of the restatement."""
    res = []
    for b, bx in enumerate(case["boxes"]):
        res.append(tal_ref.tal_maps(case["out"][b], case["cm"][b], case["rm"][b], bx, case["t"], None if case["pastes"] is None else case["pastes"][b],
                                    0 if case["flips"] is None else case["flips"][b], case["topk"], case["alpha"], case["beta"], hm=case["hm"],
                                    details=True, mutant=mutant, exp=exp))
    return res


# (map, templates, topk, images, the images without faces, faces per image, sigma of the output, padded and mirrored?, seed)
RANDOM = [((5, 7), 1, 1, 1, (), 4, 1.0, False, 0), ((5, 7), 3, 13, 2, (0,), 5, 0.1, True, 1), ((9, 11), 3, 13, 3, (1,), 7, 1.0, True, 2),
          ((17, 13), 3, 32, 4, (3,), 8, 0.1, True, 3), ((13, 17), 1, 13, 2, (), 9, 1.0, False, 4), ((31, 63), 25, 32, 2, (), 10, 1.0, True, 5),
          ((63, 63), 25, 13, 4, (1,), 12, 0.1, True, 6), ((63, 63), 25, 1, 2, (), 12, 1.0, False, 7), ((63, 47), 25, 13, 3, (0, 2), 14, 1.0, True, 8)]


@functools.lru_cache(maxsize=None)
def random_case(ci):
    hm, nt, topk, B, empty, g, sigma, padded, seed = RANDOM[ci]
    rng = np.random.RandomState(9000 + seed)
    t = templates_for(nt)
    boxes = [np.zeros((0, 4)) if b in empty else faces(rng, g + b, hm) for b in range(B)]
    pastes = flips = None
    if padded:
        pastes = [[2 * b, 3, 8 * hm[1] - 2 - 3 * b, 8 * hm[0] - 4] for b in range(B)]
        flips = [b % 2 for b in range(B)]
    out = (rng.standard_normal((B, 5 * nt) + tuple(hm)) * sigma).astype(np.float32)
    return make(hm, t, boxes, out, pastes, flips, topk, name=f"random[{ci}] {hm} nt {nt} topk {topk} B {B} sigma {sigma}")


@functools.lru_cache(maxsize=None)
def random_reference(ci):
    return restate(random_case(ci))


def plant(case, b, t, y, x, values):
    """Write (z, px, py, pw, ph) -- None = leave -- into image b's output at anchor (t, y, x)."""
    nt = case["t"].shape[0]
    for c, v in enumerate(values):
        if v is not None:
            case["out"][b, c * nt + t, y, x] = v
    return case


def _cell(y, x):
    """The centre of cell (y, x) of the stride-8 grid with offset -1: (cx, cy)."""
    return -1.0 + 8 * x, -1.0 + 8 * y


def _noise(seed, B, nt, hm, sigma):
    return (np.random.RandomState(seed).standard_normal((B, 5 * nt) + tuple(hm)) * sigma).astype(np.float32)


@functools.lru_cache(maxsize=None)
def planted():
    """name -> case.  Every decision in them is either exact or far from a tie: no face may be ambiguous."""
    P = {}
    # 12 candidates (3 x 4 cells of one template) against topk = 13, 12, 11
    f12 = np.array([[20.0, 12.0, 42.0, 42.0]])
    for k in (13, 12, 11):
        P[f"12 candidates, topk {k}"] = make((9, 11), T3[:1], [f12], _noise(1, 1, 1, (9, 11), 0.1), topk=k)
    # 255 = 15 x 17 and 256 = 16 x 16 cells of one template; 257 templates on one cell (five tiles of 64 templates)
    P["255 candidates"] = make((19, 21), T3[:1], [np.array([[12.0, 4.0, 130.0, 138.0]])], _noise(2, 1, 1, (19, 21), 1.0), topk=13)
    P["256 candidates"] = make((19, 21), T3[:1], [np.array([[12.0, 4.0, 138.0, 130.0]])], _noise(3, 1, 1, (19, 21), 1.0), topk=32)
    P["257 candidates"] = make((5, 7), many_templates(257), [np.array([[19.0, 10.0, 27.0, 20.0]])], _noise(4, 1, 257, (5, 7), 1.0), topk=32)
    # a window of many tiles under 70 templates (two tiles of templates), next to a small face
    P["window of many tiles"] = make((21, 23), many_templates(70), [np.array([[10.0, 6.0, 150.0, 160.0], [60.0, 50.0, 75.0, 70.0]])],
                                     _noise(5, 1, 70, (21, 23), 1.0), topk=13)
    # output = 0: the predicted box is the anchor, mirrored anchors tie exactly and the lower index decides.  Faces centred on a cell, on
    # the midpoint of two cells and on the corner of four; integer coordinates keep every operation exact
    (cx, cy) = _cell(4, 5)
    zero = [np.array([[cx - 9, cy - 12, cx + 9, cy + 12], [cx + 4 - 20, cy - 60, cx + 4 + 20, cy - 20], [cx - 36, cy + 4 + 8, cx - 10, cy + 4 + 40]])]
    for k in (1, 13, 32):
        P[f"output 0, topk {k}"] = make((13, 11), T3, zero, np.zeros((1, 15, 13, 11)), topk=k)
    P["output 0, alpha 0, mirrored"] = make((13, 11), T3, zero, np.zeros((1, 15, 13, 11)), pastes=[[3, 2, 85, 100]], flips=[1], topk=13, alpha=0.0)
    # logits of +-100 and +-1e4 in stripes over a random output
    c = make((9, 11), T3, [faces(np.random.RandomState(6), 6, (9, 11))], _noise(6, 1, 3, (9, 11), 1.0), topk=13)
    for i, z in enumerate((100.0, -100.0, 1e4, -1e4)):
        c["out"][0, :3, :, i::5] = z
    P["logits +-100 and +-1e4"] = c
    # the clamp: a face of the clamp's own size, 62.5 x the 9 x 11 template, around the map.  Anchor A = (0, 4, 5) predicts pw = ph = 6, far
    # beyond the clamp (clamped: u close to 1; unclamped: 0.024), anchor B = (0, 4, 6) predicts 4.0 (u = 0.76): topk = 1 takes A
    big = 62.5 * np.array([9.0, 11.0])
    (cx, cy) = _cell(4, 5)
    fc = np.array([[cx - (big[0] - 1) / 2, cy - (big[1] - 1) / 2, cx + (big[0] - 1) / 2, cy + (big[1] - 1) / 2]])
    c = make((9, 11), T3[1:2], [fc], np.full((1, 5, 9, 11), -3.0), topk=1)
    c["out"][0, 1:3] = 0.0
    plant(c, 0, 0, 4, 5, (0.0, 0.0, 0.0, 6.0, 6.0))
    plant(c, 0, 0, 4, 6, (0.0, -1.0, 0.0, 4.0, 4.0))
    P["pw beyond the clamp"] = c
    c = make((9, 11), T3[1:2], [fc], _noise(7, 1, 1, (9, 11), 0.3), topk=13)
    at = np.float32(tal_ref.BOX_CLIP)
    for x, v in enumerate((at, np.nextafter(at, np.float32(9)), np.nextafter(at, np.float32(0)), -at, np.nextafter(-at, np.float32(-9)), 50.0, -50.0, 3.0e38)):
        plant(c, 0, 0, 4, 1 + x, (None, None, None, v, -v if x % 2 else v))
    P["pw at the clamp"] = c
    # NaN and Inf in a would-be winner's logit and regression outputs: 12 candidates, three of them poisoned
    c = make((9, 11), T3[:1], [f12], _noise(1, 1, 1, (9, 11), 0.1), topk=13)
    plant(c, 0, 0, 2, 3, (np.nan, None, None, None, None))
    plant(c, 0, 0, 3, 4, (None, None, None, np.inf, None))
    plant(c, 0, 0, 4, 5, (None, -np.inf, None, None, None))
    plant(c, 0, 0, 5, 3, (np.inf, None, None, None, None))
    plant(c, 0, 0, 5, 4, (None, None, np.nan, None, None))
    P["NaN and Inf in would-be winners"] = c
    # a conflict decided by u (tests/test_atss.py's pair: both claim (t0, 2, 3), the second face overlaps its predicted box more), in both
    # orders; with the logit -1e4 there m is exactly 0 for both, and u still decides
    f0, f1 = [17.0, 7.0, 29.0, 23.0], [14.0, 4.0, 34.0, 28.0]
    for name, bx in (("conflict by u", [f0, f1]), ("conflict by u, other order", [f1, f0])):
        c = make((5, 7), T3[:1], [np.array(bx)], np.zeros((1, 5, 5, 7)), topk=13)
        P[name] = c
        c = make((5, 7), T3[:1], [np.array(bx)], np.zeros((1, 5, 5, 7)), topk=13)
        plant(c, 0, 0, 2, 3, (-1e4, None, None, None, None))
        P[name + ", m = 0"] = c
    # ... and by the face index: identical faces, every u bit-identical
    P["conflict by face index"] = make((9, 9), T3, [np.array([f1, f0, f1, f0, f1])], _noise(8, 1, 3, (9, 9), 0.2), topk=13)
    # base maps that arrive with ignored (0) anchors under a face and with +1 and regression values elsewhere: won anchors become +1, the rest stays
    c = make((9, 11), T3, [np.array([[20.0, 12.0, 42.0, 42.0], [50.0, 30.0, 80.0, 66.0]])], _noise(9, 1, 3, (9, 11), 0.5), topk=13)
    c["cm"][0, :, 1:6, 2:7] = 0.0
    c["cm"][0, 1, 8, 9] = 1.0
    c["cm"][0, 2, 0, 0] = 1.0
    c["rm"][0, :, 8, 9] = 7.0
    c["rm"][0, 5, 0, 0] = -2.5
    P["base maps with 0 and +1"] = c
    # a fully padded image, a padded one and a padded mirrored one in one batch
    bx = np.array([[10.0, 8.0, 30.0, 34.0], [3.0, 30.0, 12.0, 41.0], [40.0, 40.0, 70.0, 71.0]])
    P["padded, mirrored, fully padded"] = make((9, 9), T3, [bx, bx, bx], _noise(10, 3, 3, (9, 9), 0.5), pastes=[[30, 30, 34, 34], [22, 20, 71, 71], [22, 20, 71, 71]],
                                              flips=[0, 0, 1], topk=13)
    # a 6-px face between the centres of the grid: per template the nearest unpadded cell; and one whose edges lie ON two anchor centres
    P["tiny face"] = make((5, 7), T3, [np.array([[25.0, 17.0, 30.0, 22.0]])], _noise(11, 1, 3, (5, 7), 0.3), topk=13)
    P["edges on the centres"] = make((5, 7), T3[:2], [np.array([[23.0, 7.0, 31.0, 23.0]])], _noise(12, 1, 2, (5, 7), 0.3), topk=13)
    for name, c in P.items():
        c["name"] = name
    return P


@functools.lru_cache(maxsize=None)
def planted_reference(name):
    return restate(planted()[name])


# the planted case on which each mutant of the restatement must differ from the rule
MUTANT_CASES = {"anchor_iou": "12 candidates, topk 11", "no_clamp": "pw beyond the clamp", "ge_inside": "edges on the centres",
                "conflict_m": "conflict by u, m = 0", "topk_plus_1": "12 candidates, topk 11"}
