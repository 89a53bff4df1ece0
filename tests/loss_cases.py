"""Inputs and references shared by the loss-front-end tests: tests/test_loss_front_end_fixtures.py builds every case on the CPU and
shows that it can tell a bug apart; tests/test_gpu_targets.py and tests/test_gpu_criterion.py run the same cases through the kernels.
Nothing here touches the GPU."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import criterion as ocrit
from oracle import targets as otgt

RF = otgt.RF


# ----------------------------------------------------------------------------------------------------------------- targets
def valid(b):
    b = np.asarray(b, dtype=np.float64).reshape(-1, 4)
    return b[~np.logical_or(b[:, 2] <= b[:, 0], b[:, 3] <= b[:, 1])]


def oracle_maps(boxes, t, paste, flip, noise, hm=(63, 63), rf=RF):
    """oracle.targets for one image, as wider_face.py:160-170 calls it: (labels HWC, regression HWC f64, perturbed IoU)."""
    pad = otgt.get_padding(t, paste, rf=rf, heatmap_size=hm)
    if flip:
        pad = np.fliplr(pad)
    return otgt.get_heatmaps(np.asarray(boxes, dtype=np.float64).reshape(-1, 4).copy(), t, pad, noise=noise, rf=rf, heatmap_size=hm)


def chw(a):
    return np.ascontiguousarray(a.transpose(2, 0, 1))


# paste boxes (x1, y1, x2, y2), none symmetric in x and y.  The (7, 9) map spans 56 x 72 pixels, less than the smallest of the
# first seven templates, so its paste box reaches past the map: the arithmetic of processor.py:143-148 is the same.
GEOMETRY_PASTE = {(43, 63): [121, 21, 471, 318], (63, 40): [12, 83, 230, 455], (7, 9): [-20, -30, 75, 70], (43, 32): [121, 21, 471, 318]}
# the receptive field every training run uses has stride 8 and offset -1 on both axes; the (43, 32) map is the (43, 63) image
# under one whose stride and offset differ between y and x (listed y first, like RF)
RF_YX = {"size": [859, 859], "stride": [8, 16], "offset": [-1, 3]}


def geometry_cases(templates):
    """Case 1: maps that are not square x {25, 7} templates x {no flip, flip}; then one map under RF_YX, 25 templates."""
    cases = []
    for hi, hm in enumerate(GEOMETRY_PASTE):
        vsy, vsx = hm
        rf = RF_YX if hm == (43, 32) else RF
        (ofy, ofx), (sty, stx) = rf["offset"], rf["stride"]
        for nt in (25, 7) if rf is RF else (25,):
            t = templates[:nt]
            rng = np.random.RandomState(1000 + 10 * hi + nt)
            g = 6
            # boxes sized like templates that fit the map: one on each edge of the paste box, where the padding mask decides
            # the labels, the rest anywhere on the anchor grid
            fits = [k for k in range(nt) if t[k, 2] * 2 < stx * vsx + 40 and t[k, 3] * 2 < sty * vsy + 40] or [nt - 1]
            k = rng.choice(fits, g)
            w, h = (t[k, 2] - t[k, 0]) * rng.uniform(0.9, 1.1, g), (t[k, 3] - t[k, 1]) * rng.uniform(0.9, 1.1, g)
            cx, cy = rng.uniform(8, stx * vsx - 16, g), rng.uniform(8, sty * vsy - 16, g)
            p = GEOMETRY_PASTE[hm]
            cx[:2], cy[2:4] = (p[0] + w[0] / 2 + 3, p[2] - w[1] / 2 - 3), (p[1] + h[2] / 2 + 3, p[3] - h[3] / 2 - 3)
            boxes = np.round(np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1), 3)
            for flip in (0, 1):
                noise = np.random.RandomState(7 + flip).rand(vsy, vsx, nt, g)
                cases.append(dict(name=f"{vsy}x{vsx}-nt{nt}-flip{flip}", hm=hm, nt=nt, t=t, boxes=boxes, paste=GEOMETRY_PASTE[hm],
                                  flip=flip, noise=noise, rf=rf))
    return cases


def geometry_mutants(c):
    """The oracle's maps (labels then regression, CHW, flat) for a case, and for the exchanges a kernel could make without any
    test at 63 x 63 under RF noticing: the paste box's x and y, the unflipped mask, vsy and vsx (the same flat buffers read with the
    other map shape), and, where they differ, the receptive field's y and x entries."""
    t, p, (vsy, vsx), rf = c["t"], c["paste"], c["hm"], c["rf"]
    right = oracle_maps(c["boxes"], t, p, c["flip"], c["noise"], c["hm"], rf)
    swapped = oracle_maps(c["boxes"], t, [p[1], p[0], p[3], p[2]], c["flip"], c["noise"], c["hm"], rf)
    unflipped = oracle_maps(c["boxes"], t, p, 1 - c["flip"], c["noise"], c["hm"], rf)
    transposed = oracle_maps(c["boxes"], t, p, c["flip"], c["noise"].reshape(vsx, vsy, c["nt"], -1), (vsx, vsy), rf)
    flat = lambda r: np.concatenate([chw(r[0]).ravel(), chw(r[1]).ravel()])
    mutants = dict(paste_xy=flat(swapped), flip=flat(unflipped), map_yx=flat(transposed))
    if rf["stride"][0] != rf["stride"][1]:
        for key in ("stride", "offset"):
            other = dict(rf, **{key: rf[key][::-1]})
            mutants[f"rf_{key}_yx"] = flat(oracle_maps(c["boxes"], t, p, c["flip"], c["noise"], c["hm"], other))
    return flat(right), mutants


def mixed_batch():
    """Case 2: six images on the 63 x 63 map in ONE call: 16 boxes / none / all degenerate / two identical + one / one / none."""
    rng = np.random.RandomState(99)
    w = np.exp(rng.uniform(np.log(12), np.log(180), 16))
    h = w * rng.uniform(1.0, 1.5, 16)
    x1, y1 = rng.uniform(-20, 490, 16), rng.uniform(-20, 490, 16)
    many = np.round(np.stack([x1, y1, x1 + w, y1 + h], 1), 3)
    none = np.zeros((0, 4))
    degenerate = np.array([[50.0, 60.0, 50.0, 90.0], [200.0, 210.0, 260.0, 210.0], [300.0, 300.0, 280.0, 350.0]])
    twin = np.array([[140.5, 96.25, 196.0, 170.75], [140.5, 96.25, 196.0, 170.75], [300.0, 310.0, 336.0, 352.0]])
    one = np.array([[215.0, 330.0, 262.0, 391.0]])
    boxes = [many, none, degenerate, twin, one, none]
    paste = [[0, 0, 500, 500], [91, 193, 491, 493], [0, 120, 500, 380], [150, 10, 420, 345], [215, 200, 470, 498], [7, 3, 250, 333]]
    flips = [1, 0, 1, 1, 0, 0]
    noise = [np.random.RandomState(300 + b).rand(63, 63, 25, valid(bx).shape[0]) for b, bx in enumerate(boxes)]
    return dict(boxes=boxes, paste=paste, flips=flips, noise=noise)


def other_batch():
    """Another batch of the same shape as mixed_batch() (no image shares its boxes): what a reused out= pair is overwritten with."""
    m = mixed_batch()
    order = [4, 0, 3, 1, 5, 2]
    return dict(boxes=[m["boxes"][i] + (7.0 if m["boxes"][i].size else 0.0) for i in order], paste=[m["paste"][i] for i in order[::-1]],
                flips=[1 - f for f in m["flips"]])


def tie_case():
    """Case 3: noise identically zero, boxes centred exactly midway between four cells (cells sit at -1 + 8 k, so at 3 + 8 k) and
    sized like a template whose size is a dyadic number, so the four surrounding anchors of every template see the same IoU: the
    per-box arg-max over anchors has exact ties.  Two neighbouring such boxes of one size tie at the anchors between them, and
    one box is there twice: the per-anchor arg-max over boxes has exact ties too."""
    def box(cx, cy, hw, hh):
        return [cx - hw, cy - hh, cx + hw, cy + hh]
    boxes = np.array([box(3 + 8 * 12, 3 + 8 * 20, 17.5, 25.5),        # template 10
                      box(3 + 8 * 13, 3 + 8 * 20, 17.5, 25.5),        # its neighbour: ties at column 13
                      box(3 + 8 * 40, 3 + 8 * 9, 20.0, 22.5),         # template 9
                      box(3 + 8 * 40, 3 + 8 * 9, 20.0, 22.5),         # ... twice
                      box(3 + 8 * 30, 3 + 8 * 45, 28.5, 38.0),        # template 6
                      box(3 + 8 * 5, 3 + 8 * 50, 17.5, 25.5),
                      box(3 + 8 * 50, 3 + 8 * 30, 9.5, 10.5),         # about template 24: small enough that no anchor reaches 0.7,
                      box(3 + 8 * 22, 3 + 8 * 33, 9.6613, 10.6161)])  # so its label comes from the best-anchor rule alone
    return dict(boxes=boxes, paste=[16, 40, 480, 470], flip=1, noise=np.zeros((63, 63, 25, boxes.shape[0])))


def tie_counts(iou, neg_thresh=otgt.NEG_THRESH, pos_thresh=otgt.POS_THRESH):
    """(anchors whose maximum over boxes is positive and attained more than once, boxes whose maximum over anchors is attained more
    than once and lies in (neg, pos), where only the best-anchor rule makes the label)."""
    best = iou.max(axis=3, keepdims=True)
    anchor_ties = int((((iou == best) & (best > 0)).sum(axis=3) > 1).sum())
    per = iou.reshape(-1, iou.shape[3])
    top = per.max(axis=0)
    box_ties = int((((per == top).sum(axis=0) > 1) & (top > neg_thresh) & (top < pos_thresh)).sum())
    return anchor_ties, box_ties


def seed_mode_masks(iou, eps=1e-6, pos_thresh=otgt.POS_THRESH, neg_thresh=otgt.NEG_THRESH):
    """From the oracle's noiseless IoU (vsy, vsx, nt, G), G > 0, what a tie-break noise in [0, eps) can and cannot move:
    `settled`  = anchors whose two largest IoUs differ by more than eps: their box, hence their regression target, is fixed;
    `near_thr` = anchors whose best IoU lies within eps of a threshold: their label may change;
    `tie`      = anchors within eps of the maximum of a box whose best anchor is contested: at least two anchors lie within eps of
                 that maximum, or the maximum lies within eps of neg_thresh (whether the best-anchor rule applies at all).
    The best anchor of every other box is unique by more than eps: the noise cannot move it, and it is in none of the two."""
    s = np.sort(iou, axis=3)
    best = s[..., -1]
    settled = (best - s[..., -2] > eps) if iou.shape[3] > 1 else np.ones(best.shape, bool)
    near_thr = (np.abs(best - pos_thresh) <= eps) | (np.abs(best - neg_thresh) <= eps)
    top = iou.max(axis=(0, 1, 2))
    close = iou >= top - eps
    contested = ((close.sum(axis=(0, 1, 2)) > 1) & (top > neg_thresh - eps)) | (np.abs(top - neg_thresh) <= eps)
    tie = (close & contested).any(axis=3)
    return settled, near_thr, tie


def check_seed_mode_image(cm, rm, boxes, t, paste, flip, tot, what=""):
    """One image's seed-mode maps (HWC) against the noiseless oracle: the regression map at every settled anchor whose label no
    threshold can change (the padding rule zeroes tx where the label is not -1), by the bars of assert_regression; every label
    that differs is counted into `tot` by kind, `unexplained` if the noise cannot account for it."""
    bv = valid(boxes)
    ocm, orm, iou = oracle_maps(bv, t, paste, flip, np.zeros(cm.shape + (bv.shape[0],)))
    diff = cm != ocm
    if bv.shape[0] == 0:
        assert not diff.any() and not rm.any(), what
        return
    settled, near_thr, tie = seed_mode_masks(iou)
    tot["label_diff"] += int(diff.sum())
    tot["near_threshold"] += int((diff & near_thr).sum())
    tot["best_anchor_tie"] += int((diff & tie & ~near_thr).sum())
    tot["unexplained"] += int((diff & ~near_thr & ~tie).sum())
    pinned = settled & ~near_thr
    tot["settled"] += int(pinned.sum())
    tot["anchors"] += pinned.size
    keep = np.tile(pinned, (1, 1, 4))                          # entries of the other anchors are zeroed on both sides
    tot["reg_differ"] += assert_regression(np.where(keep, rm, 0), np.where(keep, orm, 0), what)


def seed_mode_totals():
    return dict(label_diff=0, near_threshold=0, best_anchor_tie=0, unexplained=0, settled=0, anchors=0, reg_differ=0)


def assert_regression(rm, orm, what=""):
    """The bars of test_targets_vs_reference_golden on (..., 4 nt) regression maps: tx / ty bit-equal, tw / th within rtol 2e-7 with
    at most max(1, size // 100000) entries differing at all.  Returns the number of differing entries."""
    ref = orm.astype(np.float32)
    n2 = ref.shape[-1] // 2
    assert np.array_equal(rm[..., :n2], ref[..., :n2]), f"{what}: tx / ty differ"
    mism = int((rm != ref).sum())
    assert mism <= max(1, rm.size // 100000), f"{what}: {mism} regression entries differ"
    assert np.allclose(rm, ref, rtol=2e-7, atol=0), what
    return mism


# --------------------------------------------------------------------------------------------------------------- criterion
def crit_inputs(B, nt, H, W, seed, npos, nneg, scale=1.5):
    """Random logits / labels / regression targets the way oracle/tools/make_golden.py draws the golden criterion cases.
    npos / nneg: one number, or one per image."""
    g = torch.Generator().manual_seed(seed)
    E = nt * H * W
    out = torch.randn(B, 5 * nt, H, W, generator=g) * scale
    cm = torch.zeros(B, E)
    npos = [npos] * B if np.isscalar(npos) else npos
    nneg = [nneg] * B if np.isscalar(nneg) else nneg
    for b in range(B):
        perm = torch.randperm(E, generator=g)
        cm[b, perm[:npos[b]]] = 1
        cm[b, perm[npos[b]:npos[b] + nneg[b]]] = -1
    rm = torch.randn(B, 4 * nt, H, W, generator=g) * 0.7
    return out, cm.view(B, nt, H, W), rm


def scan_case():
    """Case 1: B = 2, nt = 25, 52 x 52: E = 67 600 = 67 blocks of 1024, so the one-wave scan needs a second chunk (blocks 64..66).
    Image 0 has every positive label beyond element 65 536 (in that second chunk) and negatives everywhere."""
    out, cm, rm = crit_inputs(2, 25, 52, 52, 21, [0, 400], [4600, 4600])
    E = 25 * 52 * 52
    g = torch.Generator().manual_seed(22)
    flat = cm.view(2, E)
    tail = 65536 + torch.randperm(E - 65536, generator=g)[:400]
    flat[0, tail] = 1
    return out, cm, rm


def keep_flags(records, B, E):
    pk = np.ones((B, E), np.uint8)
    nk = np.ones((B, E), np.uint8)
    for b, r in enumerate(records):
        pk[b, :r["pos_keep"].size] = r["pos_keep"]
        nk[b, :r["neg_keep"].size] = r["neg_keep"]
    return torch.from_numpy(pk), torch.from_numpy(nk)


def oracle_criterion(out, cm, rm, nt, seed, ohem_thresh=0.03):
    """oracle.criterion with its permutation draws seeded, plus the keep flags that replay them and the OHEM-mined class map."""
    np.random.seed(seed)
    r = ocrit.criterion(out, cm, rm, n_templates=nt, ohem_thresh=ohem_thresh)
    B = out.shape[0]
    r["pos_keep"], r["neg_keep"] = keep_flags(r["records"], B, cm[0].numel())
    mined = cm.clone()
    mined[F.soft_margin_loss(out[:, :nt], cm, reduction="none") < ohem_thresh] = 0
    r["mined"] = mined
    return r


def block_edge_inputs(B):
    """Case 2: E = 15 (less than a wave), E = 1024 (exactly one block), E = 8192 (exactly eight)."""
    return [(1, 3, 5, crit_inputs(B, 1, 3, 5, 31 + B, 5, 6)),
            (16, 8, 8, crit_inputs(B, 16, 8, 8, 32 + B, 300, 500)),
            (32, 16, 16, crit_inputs(B, 32, 16, 16, 33 + B, 400, 3000))]


CAP_COUNTS = [(p, n) for p in (127, 128, 129) for n in (127, 128, 129)]


def cap_case():
    """Case 3: nine images, every pair of counts in {127, 128, 129}; run with ohem_thresh = 0 so the counts stay what they are."""
    return crit_inputs(9, 25, 8, 8, 41, [p for p, _ in CAP_COUNTS], [n for _, n in CAP_COUNTS])


def rng_mode_inputs():
    """The 63 x 63 inputs of test_gpu_small_ops.py::test_criterion_rng_mode."""
    g = torch.Generator().manual_seed(0)
    out = torch.randn(3, 125, 63, 63, generator=g) * 1.5
    cm0 = torch.zeros(3, 25 * 63 * 63)
    for b in range(3):
        perm = torch.randperm(cm0.shape[1], generator=g)
        cm0[b, perm[:400]] = 1
        cm0[b, perm[400:60000]] = -1
    rm = torch.randn(3, 100, 63, 63, generator=g)
    return out, cm0.view(3, 25, 63, 63), rm


def float64_loss(out, labels, rm, nt, reg_weight=1.0):
    """loss.py:74-88 in float64 on GIVEN labels: (sum cls, sum reg, d total / d output)."""
    o = out.double().clone().requires_grad_(True)
    lab = labels.double()
    cls = (F.soft_margin_loss(o[:, :nt], lab, reduction="none") * (lab != 0)).sum()
    reg = (F.smooth_l1_loss(o[:, nt:], rm.double(), reduction="none") * (lab > 0).repeat(1, 4, 1, 1)).sum()
    (cls + reg_weight * reg).backward()
    return float(cls), float(reg), o.grad


def uniformity_case():
    """Case 6: E = 1600, 200 positives and 300 negatives at fixed places."""
    out, cm, rm = crit_inputs(1, 25, 8, 8, 51, 200, 300)
    return out, cm, rm


UNIFORMITY_SEEDS = 2000


def uniformity_stats(count, T, keep=128):
    """count[i] = how often candidate i (C-order rank) was kept in T draws of `keep` out of n.  Under a uniform sampler every count is
    Binomial(T, p), p = keep / n: z has mean 0 and variance 1, and corr(z, rank) * sqrt(n) is standard normal too.
    Returns (max |z|, |corr(z, rank)| * sqrt(n), sum z^2 / (n - 1))."""
    count = np.asarray(count, dtype=np.float64)
    n = count.size
    p = keep / n
    z = (count - T * p) / np.sqrt(T * p * (1 - p))
    corr = np.corrcoef(z, np.arange(n))[0, 1]
    return float(np.abs(z).max()), float(abs(corr) * np.sqrt(n)), float((z ** 2).sum() / (n - 1))
