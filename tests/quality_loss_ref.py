"""Float64 restatement of the quality focal form of the detection criterion (csrc/criterion_quality.hip, tf_criterion_quality_fwd_bwd) as
include/tinyfaces_hip.h states it, with torch autograd on the CPU.  Test infrastructure; never imported by the package.

Labels y in class_map are +1, -1 and 0 (ignore); s is the class logit, sigma = sigmoid(s).  The quality target q is 0 for y = -1 and, for
y = +1, min(1, IoU) of the anchor's predicted box [px -+ e^pw / 2] x [py -+ e^ph / 2] (pw, ph clamped to +-log(1000 / 16)) with its target
box (not clamped), taken from the box EDGES here (box_loss_ref) and detached: a constant of the classification term.  Per element with y != 0

    d = sigma - q,   BCE = softplus(s) - q s
    QFL     = |d|^beta BCE
    dQFL/ds = |d|^beta d + beta |d|^(beta - 1) sgn(d) sigma (1 - sigma) BCE,   sgn(0) = 0

There is no alpha.  The regression half (SmoothL1 or one IoU / GIoU / DIoU term per positive), the normaliser (normalize="pos": both sums of
image b times 1 / max(1, npos_b), the images SUMMED) and total = cls + reg_weight reg are focal_ref's and box_loss_ref's.

`quality_loss(..., mutant=NAME)` computes what a kernel with one plausible mistake would (MUTANTS); tests/test_quality_loss.py shows that every
mutant misses the bars of tests/test_gpu_quality_loss.py.  `quality_grad_formula` is the loss and the gradient written out by hand, the kernel's
operations; with dtype=torch.float32 the per-anchor arithmetic runs in float32 the way the kernel's does (the sums stay float64).

The inputs are focal_ref's and box_loss_ref's (`case`, `planted_case`, `extreme_case`)."""
import functools

import torch

import box_loss_ref as br
import focal_ref as fr

MUTANTS = ("quality_not_detached", "hard_target", "beta_ignored", "q_unclamped_sizes", "positive_without_overlap_skipped", "cls_unnormalised")
REG_LOSSES = ("smooth_l1",) + br.REG_LOSSES
BETAS = (2.0, 2.5, 4.0)                   # the exponents of the parity grid; LOW_BETAS are held to the bars outside a band around sigma = q
LOW_BETAS = (1.0, 1.5)
BAND = 0.05


def quality(p, t, pos, clamp=True):
    """min(1, IoU) of every positive's predicted box with its target from the box edges, 0 elsewhere.  p, t: four (B, nt, H, W) tensors each."""
    zero = torch.zeros_like(p[0])
    px, py, pw, ph = [torch.where(pos, v, zero) for v in p]
    tx, ty, tw, th = [torch.where(pos, v, zero) for v in t]
    if clamp:
        pw, ph = pw.clamp(-br.C, br.C), ph.clamp(-br.C, br.C)
    pe = br._edges(px, py, torch.exp(pw), torch.exp(ph))
    te = br._edges(tx, ty, torch.exp(tw), torch.exp(th))
    iw = (torch.minimum(pe[1], te[1]) - torch.maximum(pe[0], te[0])).clamp(min=0)
    ih = (torch.minimum(pe[3], te[3]) - torch.maximum(pe[2], te[2])).clamp(min=0)
    inter = iw * ih
    iou = inter / (torch.exp(pw + ph) + torch.exp(tw + th) - inter)
    return torch.where(pos, iou.clamp(max=1.0), zero)


def _reg_half(out, class_map, reg_map, nt, reg_loss, twh, normalize, reg_weight):
    """The regression half by the references that exist: (reg sum, its gradient in out's shape with zeros in the class channels)."""
    if reg_loss == "smooth_l1":
        ref = fr.focal_loss(out, class_map, reg_map, nt, normalize=normalize, reg_weight=reg_weight)
    else:
        ref = br.box_loss(out, class_map, reg_map, nt, reg_loss, twh, normalize=normalize, reg_weight=reg_weight)
    g = ref["grad"].clone()
    g[:, :nt] = 0
    return ref["reg"], g


def quality_loss(out, class_map, reg_map, nt, reg_loss="smooth_l1", twh=None, beta=2.0, normalize="pos", reg_weight=1.0, mutant=None):
    """-> dict(cls, reg: the normalised sums over the images (floats); grad: d(cls + reg_weight reg)/d(out), float64, out's shape; npos (B,)
    int64; q (B, nt, H, W): every positive's quality target, 0 elsewhere; qsum = q.sum(); cls_per_image (B,))."""
    if reg_loss not in REG_LOSSES or normalize not in fr.NORMALIZE or (mutant is not None and mutant not in MUTANTS):
        raise ValueError((reg_loss, normalize, mutant))
    B = out.shape[0]
    o = out.detach().double().clone().requires_grad_(True)
    lab = class_map.double()
    pos = lab > 0
    p, t = br._blocks(o, reg_map.double(), nt)
    q_true = quality(p, t, pos).detach()
    q = quality(p, t, pos, clamp=mutant != "q_unclamped_sizes")
    if mutant != "quality_not_detached":
        q = q.detach()
    if mutant == "hard_target":
        q = pos.double()
    labelled = lab != 0
    if mutant == "positive_without_overlap_skipped":
        labelled = labelled & ~(pos & (q.detach() == 0))
    s = o[:, :nt]
    d = torch.sigmoid(s) - q
    bce = fr.softplus(s) - q * s
    b = 0.0 if mutant == "beta_ignored" else beta
    qfl = torch.where(labelled, d.abs() ** b * bce, torch.zeros_like(s))
    npos, w, _ = fr._normalisers(lab, normalize)
    wc = torch.ones_like(w) if mutant == "cls_unnormalised" else w
    cls_b = qfl.reshape(B, -1).sum(1) * wc
    cls_b.sum().backward()
    reg, greg = _reg_half(out, class_map, reg_map, nt, reg_loss, twh, normalize, reg_weight)
    return dict(cls=float(cls_b.detach().sum()), reg=reg, grad=o.grad + greg, npos=npos, q=q_true, qsum=float(q_true.sum()),
                cls_per_image=cls_b.detach())


def quality_grad_formula(out, class_map, reg_map, nt, reg_loss="smooth_l1", twh=None, beta=2.0, normalize="pos", reg_weight=1.0,
                         dtype=torch.float64):
    """(loss[4] = [cls, reg, sum q, sum npos], gradient) written out by hand -- the operations of the kernel -- instead of taken by autograd.
    dtype=torch.float32 evaluates the per-anchor arithmetic in float32 (the sums and the regression half of SmoothL1 stay float64)."""
    lab = class_map.double()
    pos, labelled = lab > 0, lab != 0
    p, t = br._blocks(out.to(dtype), reg_map.to(dtype), nt)
    zero = torch.zeros_like(p[0])
    px, py, pw, ph = [torch.where(pos, v, zero) for v in p]
    tx, ty, tw, th = [torch.where(pos, v, zero) for v in t]
    # q from the centre offset and the half sizes: box_term's road to its `iou`
    hwp, hhp = 0.5 * torch.exp(pw.clamp(-br.C, br.C)), 0.5 * torch.exp(ph.clamp(-br.C, br.C))
    hwt, hht = 0.5 * torch.exp(tw), 0.5 * torch.exp(th)
    dx, dy = px - tx, py - ty
    iw = torch.minimum(2.0 * torch.minimum(hwp, hwt), hwp + hwt - dx.abs()).clamp(min=0)
    ih = torch.minimum(2.0 * torch.minimum(hhp, hht), hhp + hht - dy.abs()).clamp(min=0)
    inter = iw * ih
    union = 4.0 * hwp * hhp + 4.0 * hwt * hht - inter
    q = torch.where(pos, (inter * (1.0 / union)).clamp(max=1.0), zero)
    s = out[:, :nt].to(dtype)
    ez = torch.exp(-s.abs())
    r = 1.0 / (1.0 + ez)
    sp = s.clamp(min=0) + torch.log1p(ez)
    sg = torch.where(s >= 0, r, ez * r)
    d, bce = sg - q, sp - q * s
    if beta == 2.0:
        wgt, dwgt = d * d, 2.0 * d
    else:
        w1 = d.abs() ** (beta - 1.0)                       # one pow, as in the kernel: |d|^beta = |d|^(beta - 1) |d|
        wgt, dwgt = w1 * d.abs(), beta * w1 * torch.sign(d)
    _, w, _ = fr._normalisers(lab, normalize)
    wv = w.view(-1, 1, 1, 1)
    B = out.shape[0]
    cls = float((torch.where(labelled, wgt * bce, zero).double().reshape(B, -1).sum(1) * w).sum())
    dcls = torch.where(labelled, wgt * d + dwgt * (ez * r * r) * bce, zero).double() * wv
    if reg_loss == "smooth_l1":
        diff = torch.cat([torch.where(pos, a - b, zero) for a, b in zip(p, t)], 1)
        ad = diff.abs()
        sl1 = torch.where(ad < 1, 0.5 * diff * diff, ad - 0.5).double()
        reg = float((sl1.reshape(B, -1).sum(1) * w).sum())
        dreg = reg_weight * diff.clamp(-1.0, 1.0).double() * wv
    else:
        (_, reg), g = br.box_grad_formula(out, class_map, reg_map, nt, reg_loss, twh, normalize=normalize, reg_weight=reg_weight, dtype=dtype)
        dreg = g[:, nt:]
    loss4 = torch.tensor([cls, reg, float(q.double().sum()), float(pos.sum())], dtype=torch.float64)
    return loss4, torch.cat([dcls, dreg], 1)


def band_mask(ref, out, nt, width=BAND):
    """(B, nt, H, W) bool: |sigmoid(s) - q| < width in the reference -- where the gradient of an exponent below 2 is ill-conditioned."""
    return (torch.sigmoid(out[:, :nt].double()) - ref["q"]).abs() < width


def worst_ratios(loss4, grad, ref, normalize, kink=None, band=None):
    """(loss error / its bar over loss[0], loss[1] and loss[2], gradient error / its bar) in the bars of focal_ref: rtol 1e-5 on the sums, `bars`
    on the gradient, with the four regression gradients of the `kink` anchors and the class gradient of the `band` anchors left out."""
    got = torch.as_tensor(loss4, dtype=torch.float64)[:3]
    want = torch.tensor([ref["cls"], ref["reg"], ref["qsum"]], dtype=torch.float64)
    d = (got - want).abs()
    lr = torch.where(d == 0, torch.zeros_like(d), d / (1e-5 * want.abs()))
    r = (grad.double() - ref["grad"]).abs() / fr.bars(ref, normalize)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    nt = r.shape[1] // 5
    keep = torch.ones_like(r, dtype=torch.bool)
    if kink is not None:
        keep[:, nt:] = ~kink.repeat(1, 4, 1, 1)
    if band is not None:
        keep[:, :nt] = ~band
    r = torch.where(keep, r, torch.zeros_like(r))
    lr = torch.where(torch.isnan(lr), torch.full_like(lr, float("inf")), lr)
    return float(lr.max()), float(r.max())


@functools.lru_cache(maxsize=None)
def extreme_case():
    """focal_ref.extreme_case's logits (scaled by 8, with +-100 and +-1e4 planted under a +1 and under a -1 label of each image) over boxes of the
    near regime: predictions = targets + 0.1 randn, so the positives under the extreme logits carry a q well inside (0, 1).  Cached: do not modify."""
    out, cm, rm = fr.extreme_case()
    nt = 25
    g = torch.Generator().manual_seed(4177)
    out = out.clone()
    out[:, nt:] = rm + 0.1 * torch.randn(rm.shape, generator=g)
    return out, cm, rm
