"""Float64 restatement of the overlap regression forms of the focal criterion (csrc/criterion.hip, tf_criterion_focal_box_fwd_bwd) as
include/tinyfaces_hip.h states them, with torch autograd on the CPU.  Test infrastructure; never imported by the package.

For every anchor with label +1, p = (px, py, pw, ph) from channel blocks 1..4 of `out` and t = (tx, ty, tw, th) from `reg_map`; pw and ph are
clamped to [-C, C], C = log(1000 / 16) (gradient 1 inside the closed interval, 0 outside: torch.clamp), the targets are not.  The predicted box
is [px -+ e^pw / 2] x [py -+ e^ph / 2], the target box the same from t;

    iw = max(0, min(x2) - max(x1)), ih likewise, I = iw ih, U = e^(pw + ph) + e^(tw + th) - I, IoU = I / U
    cw = max(x2) - min(x1), ch likewise, Cbox = cw ch
    iou   1 - IoU
    giou  1 - IoU + (Cbox - U) / Cbox
    diou  1 - IoU + ((a dx)^2 + dy^2) / ((a cw)^2 + ch^2),   a = dw / dh of the anchor's template, dx = px - tx, dy = py - ty

ONE term per positive anchor in place of the four SmoothL1 terms; the classification half, the normaliser and total = cls + reg_weight reg are
focal_ref.focal_loss's.  `box_loss(..., mutant=NAME)` computes what a kernel with one plausible mistake would (MUTANTS);
tests/test_box_loss.py shows that every mutant misses the bars of tests/test_gpu_box_loss.py on that file's inputs.

The gradient is not defined on a kink -- two edges tie, iw or ih is exactly 0, |pw| or |ph| is exactly C -- and next to one a float32
evaluation may take the other side: `kink_mask` marks those anchors, whose regression gradient is only required to be finite.

The inputs both files use are built here too (REGIMES, `case`, `planted_case`, `template_wh`)."""
import functools
import math

import torch

import focal_ref as fr

C = math.log(1000.0 / 16.0)
REG_LOSSES = ("iou", "giou", "diou")
REGIMES = ("drawn", "near")
MUTANTS = ("no_clamp", "clamp_gradient_passes", "giou_without_enclosing_term", "diou_ignores_aspect", "four_terms_per_anchor", "reg_unnormalised",
           "target_clamped")
# the mutants that only one form can show
ONLY_FORM = {"giou_without_enclosing_term": "giou", "diou_ignores_aspect": "diou"}
KINK_REL = 2e-5


def template_wh(nt):
    """(nt, 2) float64 (dw, dh) with aspect ratios from 0.55 to 1.4, none of them 1: the table the tests hand to the diou form."""
    k = torch.arange(nt, dtype=torch.float64)
    dh = 20.0 + 7.0 * k
    a = 0.55 + 0.85 * ((k * 7) % max(nt, 2)) / max(nt, 2) + 0.013
    return torch.stack([dh * a, dh], 1)


def _blocks(out, reg_map, nt):
    """-> (p, t): each a list of four (B, nt, H, W) views, the channel blocks px | py | pw | ph of `out` and tx | ty | tw | th of `reg_map`."""
    return [out[:, (c + 1) * nt:(c + 2) * nt] for c in range(4)], [reg_map[:, c * nt:(c + 1) * nt] for c in range(4)]


def _edges(cx, cy, w, h):
    return cx - 0.5 * w, cx + 0.5 * w, cy - 0.5 * h, cy + 0.5 * h


def terms_from_edges(pe, te, area_p, area_t, dx, dy, a, form, mutant=None):
    """The term of `form` from the edges (x1, x2, y1, y2) of two boxes, their areas, the centre offsets and the aspect weight a."""
    px1, px2, py1, py2 = pe
    tx1, tx2, ty1, ty2 = te
    iw = (torch.minimum(px2, tx2) - torch.maximum(px1, tx1)).clamp(min=0)
    ih = (torch.minimum(py2, ty2) - torch.maximum(py1, ty1)).clamp(min=0)
    inter = iw * ih
    union = area_p + area_t - inter
    term = 1.0 - inter / union
    cw = torch.maximum(px2, tx2) - torch.minimum(px1, tx1)
    ch = torch.maximum(py2, ty2) - torch.minimum(py1, ty1)
    if form == "giou" and mutant != "giou_without_enclosing_term":
        cbox = cw * ch
        term = term + (cbox - union) / cbox
    elif form == "diou":
        if mutant == "diou_ignores_aspect":
            a = torch.ones_like(a)
        term = term + ((a * dx) ** 2 + dy ** 2) / ((a * cw) ** 2 + ch ** 2)
    elif form not in REG_LOSSES:
        raise ValueError(form)
    return term


def anchor_terms(p, t, a, form, mutant=None):
    """The term of every anchor from its four predictions and four targets (tensors of one shape) and the aspect ratio a."""
    px, py, pw, ph = p
    tx, ty, tw, th = t
    if mutant == "clamp_gradient_passes":
        pw, ph = pw + (pw.clamp(-C, C) - pw).detach(), ph + (ph.clamp(-C, C) - ph).detach()
    elif mutant != "no_clamp":
        pw, ph = pw.clamp(-C, C), ph.clamp(-C, C)
    if mutant == "target_clamped":
        tw, th = tw.clamp(-C, C), th.clamp(-C, C)
    wp, hp, wt, ht = torch.exp(pw), torch.exp(ph), torch.exp(tw), torch.exp(th)
    return terms_from_edges(_edges(px, py, wp, hp), _edges(tx, ty, wt, ht), torch.exp(pw + ph), torch.exp(tw + th), px - tx, py - ty, a, form, mutant)


def box_loss(out, class_map, reg_map, nt, reg_loss, twh=None, gamma=2.0, alpha=0.25, normalize="pos", reg_weight=1.0, mutant=None):
    """-> dict(cls_per_image, reg_per_image (B,) float64, normalised; cls, reg: their sums over the images (floats);
    grad: d(cls + reg_weight reg)/d(out), float64, out's shape; npos (B,) int64; term (B, nt, H, W): every positive's term, 0 elsewhere)."""
    if reg_loss not in REG_LOSSES or normalize not in fr.NORMALIZE or (mutant is not None and mutant not in MUTANTS):
        raise ValueError((reg_loss, normalize, mutant))
    B = out.shape[0]
    half = fr.focal_loss(out, class_map, reg_map, nt, gamma, alpha, normalize, reg_weight=0.0)          # the classification half
    o = out.detach().double().clone().requires_grad_(True)
    pos = class_map.double() > 0
    p, t = _blocks(o, reg_map.double(), nt)
    zero = torch.zeros_like(p[0])
    p, t = [torch.where(pos, v, zero) for v in p], [torch.where(pos, v, zero) for v in t]                # (nothing flows from the other anchors)
    a = torch.ones(nt, dtype=torch.float64) if twh is None else twh[:, 0].double() / twh[:, 1].double()
    if reg_loss == "diou" and twh is None:
        raise ValueError("diou needs the template table")
    term = torch.where(pos, anchor_terms(p, t, a.view(1, nt, 1, 1).expand_as(zero), reg_loss, mutant), zero)
    if mutant == "four_terms_per_anchor":
        term = 4.0 * term
    _, _, wr = fr._normalisers(class_map.double(), normalize, "reg_unnormalised" if mutant == "reg_unnormalised" else None)
    reg_b = term.reshape(B, -1).sum(1) * wr
    (reg_weight * reg_b.sum()).backward()
    grad = half["grad"] + (torch.zeros_like(o) if o.grad is None else o.grad)
    return dict(cls_per_image=half["cls_per_image"], reg_per_image=reg_b.detach(), cls=half["cls"], reg=float(reg_b.detach().sum()), grad=grad,
                npos=half["npos"], term=term.detach())


def box_grad_formula(out, class_map, reg_map, nt, reg_loss, twh=None, gamma=2.0, alpha=0.25, normalize="pos", reg_weight=1.0, dtype=torch.float64):
    """(loss pair, gradient) written out by hand -- the formulas of the kernel -- instead of taken by autograd.  dtype=torch.float32 evaluates the
    per-anchor geometry in float32 the way the kernel does (the sums stay float64)."""
    lab = class_map.double()
    pos = lab > 0
    p, t = _blocks(out.to(dtype), reg_map.to(dtype), nt)
    zero = torch.zeros_like(p[0])
    px, py, pw, ph = [torch.where(pos, v, zero) for v in p]
    tx, ty, tw, th = [torch.where(pos, v, zero) for v in t]
    one = torch.ones_like(zero)
    mw, mh = torch.where((pw >= -C) & (pw <= C), one, zero), torch.where((ph >= -C) & (ph <= C), one, zero)
    hwp, hhp = 0.5 * torch.exp(pw.clamp(-C, C)), 0.5 * torch.exp(ph.clamp(-C, C))
    hwt, hht = 0.5 * torch.exp(tw), 0.5 * torch.exp(th)
    # the edges through their differences, as the kernel takes them: x2p - x2t = dx + (hwp - hwt), x1p - x1t = dx - (hwp - hwt);
    # min(x2) - max(x1) = min(2u, 2v, u + v - |d|) and max(x2) - min(x1) = max(2u, 2v, u + v + |d|) for half widths u, v and centre distance d
    dx, dy = px - tx, py - ty
    rx2, rx1, ry2, ry1 = dx + (hwp - hwt), dx - (hwp - hwt), dy + (hhp - hht), dy - (hhp - hht)
    iwr = torch.minimum(2.0 * torch.minimum(hwp, hwt), hwp + hwt - dx.abs())
    ihr = torch.minimum(2.0 * torch.minimum(hhp, hht), hhp + hht - dy.abs())
    iw, ih = iwr.clamp(min=0), ihr.clamp(min=0)
    cw = torch.maximum(2.0 * torch.maximum(hwp, hwt), hwp + hwt + dx.abs())
    ch = torch.maximum(2.0 * torch.maximum(hhp, hht), hhp + hht + dy.abs())
    ap, at = 4.0 * hwp * hhp, 4.0 * hwt * hht
    inter = iw * ih
    union = ap + at - inter
    iou = inter / union
    f = lambda cond: torch.where(cond, one, zero)
    ox, oy = f(iwr > 0), f(ihr > 0)
    ix2, ix1, iy2, iy1 = f(rx2 < 0) * ox, f(rx1 > 0) * ox, f(ry2 < 0) * oy, f(ry1 > 0) * oy
    dI = [ih * (ix2 - ix1), iw * (iy2 - iy1), ih * hwp * (ix2 + ix1), iw * hhp * (iy2 + iy1)]
    dU = [-dI[0], -dI[1], ap - dI[2], ap - dI[3]]
    term = (union - inter) / union
    g = [-(dI[k] - iou * dU[k]) / union for k in range(4)]
    if reg_loss in ("giou", "diou"):
        ex2, ex1, ey2, ey1 = f(rx2 > 0), f(rx1 < 0), f(ry2 > 0), f(ry1 < 0)
        dcw, dch = [ex2 - ex1, zero, hwp * (ex2 + ex1), zero], [zero, ey2 - ey1, zero, hhp * (ey2 + ey1)]
        if reg_loss == "giou":
            cbox = cw * ch
            term = term + (cbox - union) / cbox
            g = [g[k] - (dU[k] - union / cbox * (ch * dcw[k] + cw * dch[k])) / cbox for k in range(4)]
        else:
            a = (twh[:, 0].double() / twh[:, 1].double()).to(dtype).view(1, nt, 1, 1)
            a2 = a * a
            num, den = a2 * dx * dx + dy * dy, a2 * cw * cw + ch * ch
            r = num / den
            dN = [2.0 * a2 * dx, 2.0 * dy, zero, zero]
            term = term + r
            g = [g[k] + (dN[k] - r * 2.0 * (a2 * cw * dcw[k] + ch * dch[k])) / den for k in range(4)]
    elif reg_loss != "iou":
        raise ValueError(reg_loss)
    g[2], g[3] = g[2] * mw, g[3] * mh
    _, w, _ = fr._normalisers(lab, normalize)
    B = out.shape[0]
    term = torch.where(pos, term, zero).double()
    reg = float((term.reshape(B, -1).sum(1) * w).sum())
    grad = fr.focal_grad_formula(out, class_map, reg_map, nt, gamma, alpha, normalize, reg_weight=0.0)
    dreg = torch.cat([torch.where(pos, v, zero).double() for v in g], 1) * reg_weight * w.view(-1, 1, 1, 1)
    grad = torch.cat([grad[:, :nt], dreg], 1)
    cls = fr.focal_loss(out, class_map, reg_map, nt, gamma, alpha, normalize, reg_weight=0.0)["cls"]
    return (cls, reg), grad


def kink_mask(out, class_map, reg_map, nt):
    """(B, nt, H, W) bool: the positives next to a kink.  The smallest of the four edge differences, |iw| and |ih| (both before the max with 0) is
    below 2e-5 max(1, largest |edge coordinate|), or ||pw| - C| or ||ph| - C| is below 2e-5 C."""
    pos = class_map.double() > 0
    p, t = _blocks(out.double(), reg_map.double(), nt)
    px, py, pw, ph = p
    tx, ty, tw, th = t
    pe = _edges(px, py, torch.exp(pw.clamp(-C, C)), torch.exp(ph.clamp(-C, C)))
    te = _edges(tx, ty, torch.exp(tw), torch.exp(th))
    iwr = torch.minimum(pe[1], te[1]) - torch.maximum(pe[0], te[0])
    ihr = torch.minimum(pe[3], te[3]) - torch.maximum(pe[2], te[2])
    small = torch.stack([(pe[k] - te[k]).abs() for k in range(4)] + [iwr.abs(), ihr.abs()]).min(0).values
    scale = torch.stack([v.abs() for v in pe + te]).max(0).values.clamp(min=1.0)
    near_clamp = ((pw.abs() - C).abs() < KINK_REL * C) | ((ph.abs() - C).abs() < KINK_REL * C)
    return pos & ((small < KINK_REL * scale) | near_clamp)


def worst_ratios(loss2, grad, ref, normalize, kink=None):
    """focal_ref.worst_ratios with the four regression gradients of the `kink` anchors left out of the gradient ratio."""
    got = torch.as_tensor(loss2, dtype=torch.float64)
    want = torch.tensor([ref["cls"], ref["reg"]], dtype=torch.float64)
    d = (got - want).abs()
    lr = torch.where(d == 0, torch.zeros_like(d), d / (1e-5 * want.abs()))
    r = (grad.double() - ref["grad"]).abs() / fr.bars(ref, normalize)
    if kink is not None:
        keep = torch.cat([torch.ones_like(kink), ~kink.repeat(1, 4, 1, 1)], 1)
        r = torch.where(keep, r, torch.zeros_like(r))
    return float(lr.max()), float(r.max())


# ------------------------------------------------------------------------------------------------------------------- the inputs
@functools.lru_cache(maxsize=None)
def case(shape, variant="drawn", regime="drawn"):
    """(out, class_map, reg_map) of focal_ref.case; regime "near": the same labels and targets with the four predictions of every anchor set to
    target + 0.1 randn -- the high-overlap regime of a trained model, where Cbox - U cancels.  Cached: do not modify."""
    out, cm, rm = fr.case(shape, variant)
    if regime == "drawn":
        return out, cm, rm
    if regime != "near":
        raise ValueError(regime)
    nt = shape[1]
    g = torch.Generator().manual_seed(4100 + sum(shape))
    out = out.clone()
    out[:, nt:] = rm + 0.1 * torch.randn(rm.shape, generator=g)
    return out, cm, rm


PLANTED = ("equal", "equal", "pw+", "pw-", "ph+", "ph-", "px+", "px-", "tw_beyond", "th_beyond")


@functools.lru_cache(maxsize=None)
def planted_case():
    """(out, class_map, reg_map, {name: [(b, t, y, x), ...]}) on (2, 25, 9, 9): under the first positives of each image, in PLANTED's order:
    predictions equal to their targets (twice); pw = +-1e4; ph = +-1e4; px = +-1e4; targets tw = 4.6 and th = -4.6, beyond the clamp that the
    targets do not get, under predictions centred 0.3 and -0.2 off theirs.  Cached: do not modify."""
    nt = 25
    out, cm, rm = [v.clone() for v in fr.case(fr.SHAPES[2])]
    where = {}
    for b in (0, 1) if int((cm[1] == 1).sum()) >= len(PLANTED) else (0,):
        idx = (cm[b] == 1).nonzero()[:len(PLANTED)]
        assert idx.shape[0] == len(PLANTED)
        for name, (t, y, x) in zip(PLANTED, idx.tolist()):
            where.setdefault(name, []).append((b, t, y, x))
            if name == "equal":
                for c in range(4):
                    out[b, (c + 1) * nt + t, y, x] = rm[b, c * nt + t, y, x]
            elif name[0] == "p":
                c = {"px": 0, "pw": 2, "ph": 3}[name[:2]]
                out[b, (c + 1) * nt + t, y, x] = 1e4 if name[2] == "+" else -1e4
            else:
                c, v = (2, 4.6) if name == "tw_beyond" else (3, -4.6)
                rm[b, c * nt + t, y, x] = v
                out[b, 1 * nt + t, y, x] = rm[b, 0 * nt + t, y, x] + 0.3          # centres close enough that the boxes overlap
                out[b, 2 * nt + t, y, x] = rm[b, 1 * nt + t, y, x] - 0.2
    return out, cm, rm, where
