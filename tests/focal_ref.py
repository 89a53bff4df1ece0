"""Float64 restatement of the focal form of the detection criterion (csrc/criterion.hip, tf_criterion_focal_fwd_bwd) as
include/tinyfaces_hip.h states it, with torch autograd on the CPU.  Test infrastructure; never imported by the package.

Labels y in class_map are +1, -1 and 0 (ignore); s is the class logit, x = y s, softplus(v) = max(v, 0) + log1p(exp(-|v|));
a_t = alpha for y = +1 and 1 - alpha for y = -1, or 1 when alpha < 0.  Per element with y != 0

    FL     = a_t exp(-gamma softplus(x)) softplus(-x)
    dFL/ds = -y a_t exp(-gamma softplus(x)) (gamma sigmoid(x) softplus(-x) + sigmoid(-x))

plus SmoothL1 (beta = 1) over the four regression channels of every y > 0 element.  normalize="pos": both sums of image b times
1 / max(1, npos_b); the images are SUMMED.  total = cls + reg_weight reg.

`focal_loss(..., mutant=NAME)` computes what a kernel with one plausible mistake would (MUTANTS); tests/test_focal_loss.py shows that
every mutant moves the loss or the gradient on the inputs of tests/test_gpu_focal_loss.py far beyond that file's bars.

The inputs both files use are built here too (SHAPES, VARIANTS, PARAMS, `case`, `extreme_case`)."""
import functools

import torch
import torch.nn.functional as F

import loss_cases as lc

MUTANTS = ("alpha_on_negatives", "gamma_ignored", "batch_normaliser", "reg_unnormalised", "ignored_included")
NORMALIZE = ("pos", "none")


def softplus(v):
    return v.clamp(min=0) + torch.log1p(torch.exp(-v.abs()))


def _alpha_t(lab, alpha, mutant=None):
    if alpha < 0:
        return torch.ones_like(lab)
    pos, neg = (alpha, 1.0 - alpha) if mutant != "alpha_on_negatives" else (1.0 - alpha, alpha)
    return torch.where(lab > 0, torch.full_like(lab, pos), torch.full_like(lab, neg))


def _normalisers(lab, normalize, mutant=None):
    """(B,) float64 factors of the classification sums; the regression's are the same unless a mutant says otherwise."""
    B = lab.shape[0]
    npos = (lab == 1).reshape(B, -1).sum(1)
    if normalize == "none":
        w = torch.ones(B, dtype=torch.float64)
    elif mutant == "batch_normaliser":
        w = torch.full((B,), 1.0 / max(1, int(npos.sum())), dtype=torch.float64)
    else:
        w = 1.0 / npos.clamp(min=1).double()
    return npos, w, (torch.ones(B, dtype=torch.float64) if mutant == "reg_unnormalised" else w)


def focal_loss(out, class_map, reg_map, nt, gamma=2.0, alpha=0.25, normalize="pos", reg_weight=1.0, mutant=None):
    """-> dict(cls_per_image, reg_per_image (B,) float64, normalised; cls, reg: their sums over the images (floats);
    grad: d(cls + reg_weight reg)/d(out), float64, out's shape; npos (B,) int64)."""
    if normalize not in NORMALIZE or (mutant is not None and mutant not in MUTANTS):
        raise ValueError((normalize, mutant))
    B = out.shape[0]
    o = out.detach().double().clone().requires_grad_(True)
    lab = class_map.double()
    if mutant == "ignored_included":
        lab = torch.where(lab == 0, -torch.ones_like(lab), lab)
    s = o[:, :nt]
    x = lab * s
    g = 0.0 if mutant == "gamma_ignored" else gamma
    fl = _alpha_t(lab, alpha, mutant) * torch.exp(-g * softplus(x)) * softplus(-x) * (lab != 0)
    sl1 = F.smooth_l1_loss(o[:, nt:], reg_map.double(), reduction="none", beta=1.0) * (class_map.double() > 0).repeat(1, 4, 1, 1)
    npos, wc, wr = _normalisers(class_map.double(), normalize, mutant)
    cls_b = fl.reshape(B, -1).sum(1) * wc
    reg_b = sl1.reshape(B, -1).sum(1) * wr
    (cls_b.sum() + reg_weight * reg_b.sum()).backward()
    return dict(cls_per_image=cls_b.detach(), reg_per_image=reg_b.detach(), cls=float(cls_b.detach().sum()), reg=float(reg_b.detach().sum()), grad=o.grad,
                npos=npos)


def focal_grad_formula(out, class_map, reg_map, nt, gamma=2.0, alpha=0.25, normalize="pos", reg_weight=1.0):
    """The gradient written out by hand (the formula of the header and of the kernel) instead of taken by autograd."""
    o, lab = out.double(), class_map.double()
    s = o[:, :nt]
    x = lab * s
    dfl = -lab * _alpha_t(lab, alpha) * torch.exp(-gamma * softplus(x)) * (gamma * torch.sigmoid(x) * softplus(-x) + torch.sigmoid(-x))
    dfl = dfl * (lab != 0)
    d = o[:, nt:] - reg_map.double()
    dreg = reg_weight * d.clamp(-1.0, 1.0) * (lab > 0).repeat(1, 4, 1, 1)
    _, w, _ = _normalisers(lab, normalize)
    return torch.cat([dfl, dreg], 1) * w.view(-1, 1, 1, 1)


# ------------------------------------------------------------------------------------------------------------------- the inputs
# (B, nt, H, W): E = 15 (less than a wave), 1024 (exactly one block), 2025 (a ragged last block), 67 blocks per image x 5 images =
# 335 partials, and 260 blocks in ONE image (E = 265 225): the kernels add an image's per-block counts and partials with 256 threads,
# so only more than 256 blocks per image take their loops a second time
SHAPES = ((1, 1, 3, 5), (3, 16, 8, 8), (2, 25, 9, 9), (5, 25, 52, 52), (1, 25, 103, 103))
# what image 0 of the drawn batch is replaced with
VARIANTS = ("drawn", "no_positive", "no_label", "fully_labelled")
PARAMS = ((2.0, 0.25), (0.0, -1.0), (0.5, 0.75), (5.0, 0.25))


def _counts(B, E):
    """Per-image (+1, -1) counts that differ and, from two images on, include an image without positives."""
    pos = [max(1, E // 7), 0, max(1, E // 50), 3, max(1, E // 400)][:B] if B > 1 else [max(1, E // 3)]
    neg = [max(1, E // 2), max(1, E // 3), E // 5, 0, E // 4][:B] if B > 1 else [max(1, E // 3)]
    return pos, neg


@functools.lru_cache(maxsize=None)
def case(shape, variant="drawn"):
    """(out, class_map, reg_map) for one of SHAPES x VARIANTS, drawn by loss_cases.crit_inputs.  Cached: do not modify."""
    B, nt, H, W = shape
    E = nt * H * W
    pos, neg = _counts(B, E)
    out, cm, rm = lc.crit_inputs(B, nt, H, W, 700 + E % 97 + B, pos, neg)
    cm = cm.clone()
    flat = cm.view(B, E)
    if variant == "no_positive":
        flat[0][flat[0] == 1] = -1
    elif variant == "no_label":
        flat[0] = 0
    elif variant == "fully_labelled":
        flat[0][flat[0] == 0] = -1
    elif variant != "drawn":
        raise ValueError(variant)
    return out, cm, rm


@functools.lru_cache(maxsize=None)
def extreme_case():
    """(2, 25, 9, 9) with logits scaled by 8 and +-100, +-1e4 planted under a +1 and under a -1 label of each image."""
    nt = 25
    out, cm, rm = lc.crit_inputs(2, nt, 9, 9, 777, [40, 7], [500, 900])
    out[:, :nt] *= 8.0
    E = cm[0].numel()
    for b in range(2):
        lab, logit = cm[b].view(E), out[b, :nt].reshape(E)
        for sign in (1.0, -1.0):
            idx = (lab == sign).nonzero().flatten()[:4]
            assert idx.numel() == 4
            logit[idx] = torch.tensor([100.0, -100.0, 1e4, -1e4])
        out[b, :nt] = logit.view(nt, 9, 9)
    return out, cm, rm


def bars(ref, normalize, rtol=1e-5, atol=1e-6):
    """The elementwise gradient bar of tests/test_gpu_criterion.py (rtol 1e-5, atol 1e-6); for normalize="pos" image b's atol is
    divided by max(1, npos_b), so that it does not swallow the normalised gradient.  -> tensor of ref["grad"]'s shape."""
    a = torch.full((ref["grad"].shape[0],), atol, dtype=torch.float64)
    if normalize == "pos":
        a = a / ref["npos"].clamp(min=1).double()
    return a.view(-1, 1, 1, 1) + rtol * ref["grad"].abs()


def worst_ratios(loss2, grad, ref, normalize):
    """(loss error / its bar, gradient error / its bar), worst case of each; a loss whose reference is 0 must be 0."""
    got = torch.as_tensor(loss2, dtype=torch.float64)
    want = torch.tensor([ref["cls"], ref["reg"]], dtype=torch.float64)
    d = (got - want).abs()
    lr = torch.where(d == 0, torch.zeros_like(d), d / (1e-5 * want.abs()))          # (d > 0 over a bar of 0 is inf)
    gr = ((grad.double() - ref["grad"]).abs() / bars(ref, normalize)).max()
    return float(lr.max()), float(gr)
