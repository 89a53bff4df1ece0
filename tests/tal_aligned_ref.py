"""TOOD's task-aligned loss restated on the CPU, in two parts.  Test infrastructure only; never imported by the package.

1  Step 7 of the task-aligned assignment (include/tinyfaces_hip.h, "TAL, step 7") in numpy float64 on top of tests/tal_ref.py's steps 1-6:
   after the conflicts let W_g be the anchors face g WON; M_g = max m and U_g = max u over W_g; t(a) = (m_a / M_g) * U_g, 0 when M_g == 0,
   stored as float32; every other element of align_map is 1.  `aligned_maps` returns the map with M_g and U_g.  exp and pow differ between
   numpy and the device in the last bits of a double, which can move the final rounding to float32 by one step and no more: `ulp_distance`
   measures that, `hold_align` holds a device map to 1 ulp at the won anchors and to exactly 1.0f elsewhere.

2  The aligned form of the detection criterion (tf_criterion_aligned_fwd_bwd) as a float64 autograd function next to tests/quality_loss_ref.py:
   q = min(1, max(0, a)) at a positive (NaN -> 0), 0 at a negative; QFL with that q; the regression term of `reg_loss` times q; normaliser
   "none", "pos" (1 / max(1, npos_b)) or "align" (1 / max(1, sum of q over image b's positives)), the images summed.

Both parts carry mutants -- what a kernel with one plausible mistake would compute -- and tests/test_tal_aligned.py shows that each misses the
bars on a committed case.  The extra planted inputs of the assignment (`planted`) and the inputs of the criterion (`loss_case`) are here too."""
import functools

import numpy as np
import torch

import box_loss_ref as br
import focal_ref as fr
import quality_loss_ref as qr
import tal_cases as tc
import tal_ref

ASSIGN_MUTANTS = ("before_conflicts", "no_best_iou", "per_image", "epsilon")
LOSS_MUTANTS = ("reg_unweighted", "npos_normaliser", "q_own_iou")
NORMALIZE = ("none", "pos", "align")
REG_LOSSES = qr.REG_LOSSES


# ------------------------------------------------------------------------------------------------------------------ step 7
def aligned_maps(out, class_map, regression_map, boxes, templates, paste=None, flip=0, topk=13, alpha=1.0, beta=6.0, hm=None, mutant=None, exp=np.exp):
    """One image, device layout, as tal_ref.tal_maps takes it.  -> dict(cm, rm, counts, faces: tal_maps' own results; align (nt, vsy, vsx) float32;
    t (nt, vsy, vsx) float64: the alignment before its rounding, 1 elsewhere; won (nt, vsy, vsx) bool: the anchors this call won; M, U (G,) float64:
    the two maxima of every face, 0 for a face that won nothing; owners: per face the indices into its claim list that it won)."""
    if mutant is not None and mutant not in ASSIGN_MUTANTS:
        raise ValueError(mutant)
    cm, rm, counts, faces = tal_ref.tal_maps(out, class_map, regression_map, boxes, templates, paste, flip, topk, alpha, beta, hm=hm, details=True, exp=exp)
    G = len(faces)
    claims = {}
    for g, f in enumerate(faces):
        for i, a in enumerate(f["winners"]):
            claims.setdefault(int(a), []).append((g, i))
    owners = [[] for _ in range(G)]
    for a, cl in claims.items():
        best = cl[0]                                                  # step 4: the larger u, the lower g on a tie
        for c in cl[1:]:
            if faces[c[0]]["u"][c[1]] > faces[best[0]]["u"][best[1]]:
                best = c
        owners[best[0]].append(best[1])
    assert [len(o) for o in owners] == counts.tolist()
    t = np.ones(cm.size, dtype=np.float64)
    won = np.zeros(cm.size, dtype=bool)
    M, U = np.zeros(G), np.zeros(G)
    for g, f in enumerate(faces):
        if owners[g]:
            idx = np.array(sorted(owners[g]))
            M[g], U[g] = f["m"][idx].max(), f["u"][idx].max()
    all_m = [faces[g]["m"][i] for g in range(G) for i in owners[g]]
    all_u = [faces[g]["u"][i] for g in range(G) for i in owners[g]]
    for g, f in enumerate(faces):
        if not owners[g]:
            continue
        idx = np.array(sorted(owners[g]))
        Mg, Ug = M[g], U[g]
        if mutant == "before_conflicts":                              # the maxima over everything the face CLAIMED
            Mg, Ug = f["m"].max(), f["u"].max()
        elif mutant == "per_image":
            Mg, Ug = max(all_m), max(all_u)
        m = f["m"][idx]
        with np.errstate(all="ignore"):
            if mutant == "epsilon":                                   # mmdetection's TaskAlignedAssigner
                v = (m / (Mg + 1e-7)) * Ug
            elif mutant == "no_best_iou":
                v = m / Mg if Mg != 0 else np.zeros_like(m)
            else:
                v = (m / Mg) * Ug if Mg != 0 else np.zeros_like(m)
        t[f["winners"][idx]] = v
        won[f["winners"][idx]] = True
    return dict(cm=cm, rm=rm, counts=counts, faces=faces, align=t.astype(np.float32).reshape(cm.shape), t=t.reshape(cm.shape), won=won.reshape(cm.shape),
                M=M, U=U, owners=owners)


def restate(case, mutant=None, exp=np.exp):
    """Per image the dict of aligned_maps for a case of tests/tal_cases.py."""
    return [aligned_maps(case["out"][b], case["cm"][b], case["rm"][b], bx, case["t"], None if case["pastes"] is None else case["pastes"][b],
                         0 if case["flips"] is None else case["flips"][b], case["topk"], case["alpha"], case["beta"], hm=case["hm"], mutant=mutant, exp=exp)
            for b, bx in enumerate(case["boxes"])]


def ambiguous(ref):
    return sum(bool(f["ambiguous"]) for im in ref for f in im["faces"])


def ulp_distance(a, b):
    """Elementwise distance of two float32 arrays of non-negative finite values in units in the last place (adjacent floats: 1)."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def hold_align(got, ref, what=""):
    """Hold a device align_map (B, nt, vsy, vsx) to the restatement of every image: within 1 float32 ulp at the won anchors, exactly 1.0f elsewhere,
    nothing negative, NaN or above 1.  -> the largest ulp distance met.  AssertionError otherwise."""
    worst = 0
    for b, r in enumerate(ref):
        g = np.asarray(got[b], dtype=np.float32)
        assert np.isfinite(g).all() and (g >= 0).all() and (g <= 1).all(), f"{what}: image {b}: align_map leaves [0, 1]"
        assert np.array_equal(g[~r["won"]].view(np.int32), np.ones(int((~r["won"]).sum()), np.float32).view(np.int32)), \
            f"{what}: image {b}: align_map is not exactly 1.0f at {np.argwhere((g != 1) & ~r['won'])[:5].tolist()}"
        if r["won"].any():
            d = ulp_distance(g[r["won"]], r["align"][r["won"]])
            assert d.max() <= 1, f"{what}: image {b}: align_map is {int(d.max())} ulp off at {np.argwhere(r['won'])[np.argmax(d)].tolist()}"
            worst = max(worst, int(d.max()))
    return worst


@functools.lru_cache(maxsize=None)
def planted():
    """name -> case (tests/tal_cases.py's dicts): the inputs step 7 needs beyond tal_cases.planted().  No face may be ambiguous."""
    P = {}
    # A conflict in which the loser loses its best-m anchor.  Face A (51 x 55) holds many cells of the one 17 x 21 template; face B IS the anchor
    # box of cell (3, 4), whose logit is 5 and whose regression outputs are 0: A's largest m sits there, B claims the anchor with u = 1 and wins
    # it.  A's maxima before and after the conflict differ.  Both input orders.
    A, Bx = [10.0, 6.0, 60.0, 60.0], [23.0, 13.0, 39.0, 33.0]
    for name, bx in (("loser loses its best m", [A, Bx]), ("loser loses its best m, other order", [Bx, A])):
        c = tc.make((9, 11), tc.T3[:1], [np.array(bx)], tc._noise(21, 1, 1, (9, 11), 0.02), topk=13)
        tc.plant(c, 0, 0, 3, 4, (5.0, 0.0, 0.0, 0.0, 0.0))
        P[name] = c
    # M_g = 0: logits of -1e4 with alpha = 1 make every sigmoid, hence every m, exactly 0; the lower indices win and every target is 0
    c = tc.make((9, 11), tc.T3, [np.array([[20.0, 12.0, 42.0, 42.0], [50.0, 30.0, 80.0, 66.0]])], tc._noise(22, 1, 3, (9, 11), 0.3), topk=13, alpha=1.0)
    c["out"][0, :3] = -1e4
    P["M = 0"] = c
    # the 6-px face at zero output under the 25 templates of training: it lies inside the smallest anchor (20.3 x 22.2 px), u = 36 / 452 = 0.080,
    # m = 0.5 * 0.080^6 = 1.3e-7, the size of mmdetection's epsilon
    P["6-px face, output 0"] = tc.make((5, 7), tc.templates_for(25), [np.array([[25.0, 17.0, 30.0, 22.0]])], np.zeros((1, 125, 5, 7)), topk=13)
    # several faces of different quality in one image (per-face, not per-image maxima), 25 templates
    rng = np.random.RandomState(23)
    P["four faces, 25 templates"] = tc.make((17, 13), tc.templates_for(25), [tc.faces(rng, 4, (17, 13))], tc._noise(24, 1, 25, (17, 13), 0.5), topk=13)
    for name, c in P.items():
        c["name"] = name
    return P


# the planted cases of tal_cases.planted() step 7 is also held on: a face that wins nothing (the loser of "conflict by u"), exactly one winner
# (topk 1), 32 winners of topk 32, more than 64 templates, base maps that hold a +1 the call does not win, padded / mirrored / fully padded images
FROM_TAL_CASES = ("conflict by u", "conflict by u, other order", "output 0, topk 1", "pw beyond the clamp", "256 candidates", "257 candidates",
                  "window of many tiles", "base maps with 0 and +1", "padded, mirrored, fully padded", "conflict by face index")
# the case on which each mutant of step 7 must differ from the rule by more than 1 ulp
ASSIGN_MUTANT_CASES = {"before_conflicts": "loser loses its best m", "no_best_iou": "four faces, 25 templates", "per_image": "four faces, 25 templates",
                       "epsilon": "6-px face, output 0"}


def planted_case(name):
    return planted()[name] if name in planted() else tc.planted()[name]


@functools.lru_cache(maxsize=None)
def planted_reference(name):
    return restate(planted_case(name))


# seeded random images in tal_cases.RANDOM's format; the seeds were chosen on the CPU so that no face is ambiguous (tests/test_tal_aligned.py
# asserts it).  B = 1..4 with an image without faces first, in the middle and last, padded and mirrored, topk 1 / 13 / 32, 1 / 3 / 25 templates.
RANDOM = [((5, 7), 1, 1, 1, (), 4, 1.0, False, 100), ((5, 7), 3, 13, 2, (0,), 5, 0.1, True, 101), ((9, 11), 3, 13, 3, (1,), 7, 1.0, True, 102),
          ((17, 13), 3, 32, 4, (3,), 8, 0.1, True, 103), ((31, 63), 25, 32, 2, (), 10, 1.0, True, 105), ((63, 63), 25, 13, 4, (1,), 12, 0.1, True, 106),
          ((63, 47), 25, 13, 3, (0, 2), 14, 1.0, True, 108)]


@functools.lru_cache(maxsize=None)
def random_case(ci):
    hm, nt, topk, B, empty, g, sigma, padded, seed = RANDOM[ci]
    rng = np.random.RandomState(9000 + seed)
    t = tc.templates_for(nt)
    boxes = [np.zeros((0, 4)) if b in empty else tc.faces(rng, g + b, hm) for b in range(B)]
    pastes = flips = None
    if padded:
        pastes = [[2 * b, 3, 8 * hm[1] - 2 - 3 * b, 8 * hm[0] - 4] for b in range(B)]
        flips = [b % 2 for b in range(B)]
    out = (rng.standard_normal((B, 5 * nt) + tuple(hm)) * sigma).astype(np.float32)
    return tc.make(hm, t, boxes, out, pastes, flips, topk, name=f"aligned random[{ci}] {hm} nt {nt} topk {topk} B {B} sigma {sigma}")


@functools.lru_cache(maxsize=None)
def random_reference(ci):
    return restate(random_case(ci))


# ------------------------------------------------------------------------------------------------------------------ the loss
def target(align_map, pos):
    """q of the header: min(1, max(0, a)) at a positive with a NaN giving 0; 0 elsewhere.  float64."""
    a = align_map.double()
    a = torch.where(torch.isnan(a), torch.zeros_like(a), a).clamp(0.0, 1.0)
    return torch.where(pos, a, torch.zeros_like(a))


def aligned_loss(out, class_map, reg_map, align_map, nt, reg_loss="smooth_l1", twh=None, beta=2.0, normalize="align", reg_weight=1.0, mutant=None):
    """-> dict(cls, reg: the normalised sums over the images (floats; reg is the q-weighted sum, not weighted by reg_weight); grad:
    d(cls + reg_weight reg)/d(out), float64; npos (B,) int64; q (B, nt, H, W); qsum = q.sum(); qsum_per_image (B,); w (B,): every image's factor)."""
    if reg_loss not in REG_LOSSES or normalize not in NORMALIZE or (mutant is not None and mutant not in LOSS_MUTANTS):
        raise ValueError((reg_loss, normalize, mutant))
    B = out.shape[0]
    o = out.detach().double().clone().requires_grad_(True)
    lab = class_map.double()
    pos, labelled = lab > 0, lab != 0
    p, t = br._blocks(o, reg_map.double(), nt)
    q_true = target(align_map, pos)
    q = qr.quality(p, t, pos).detach() if mutant == "q_own_iou" else q_true
    s = o[:, :nt]
    d = torch.sigmoid(s) - q
    bce = fr.softplus(s) - q * s
    qfl = torch.where(labelled, d.abs() ** beta * bce, torch.zeros_like(s))
    zero = torch.zeros_like(p[0])
    pm, tm = [torch.where(pos, v, zero) for v in p], [torch.where(pos, v, zero) for v in t]       # (nothing flows from the other anchors)
    if reg_loss == "smooth_l1":
        term = zero
        for a, b in zip(pm, tm):
            df = a - b
            term = term + torch.where(df.abs() < 1, 0.5 * df * df, df.abs() - 0.5)
    else:
        if reg_loss == "diou" and twh is None:
            raise ValueError("diou needs the template table")
        asp = torch.ones(nt, dtype=torch.float64) if twh is None else twh[:, 0].double() / twh[:, 1].double()
        term = br.anchor_terms(pm, tm, asp.view(1, nt, 1, 1).expand_as(zero), reg_loss)
    term = torch.where(pos, term * (1.0 if mutant == "reg_unweighted" else q), zero)
    npos = (lab == 1).reshape(B, -1).sum(1)
    qb = q.reshape(B, -1).sum(1)
    if normalize == "none":
        w = torch.ones(B, dtype=torch.float64)
    elif normalize == "pos" or mutant == "npos_normaliser":
        w = 1.0 / npos.clamp(min=1).double()
    else:
        w = 1.0 / qb.detach().clamp(min=1.0)
    cls_b, reg_b = qfl.reshape(B, -1).sum(1) * w, term.reshape(B, -1).sum(1) * w
    (cls_b.sum() + reg_weight * reg_b.sum()).backward()
    return dict(cls=float(cls_b.detach().sum()), reg=float(reg_b.detach().sum()), grad=o.grad, npos=npos, q=q_true, qsum=float(q_true.sum()),
                qsum_per_image=q_true.reshape(B, -1).sum(1), w=w)


def bars(ref, rtol=1e-5, atol=1e-6):
    """The project's elementwise gradient bar (rtol 1e-5, atol 1e-6) with image b's atol divided by its normaliser (times ref["w"][b]), so that it
    does not swallow the normalised gradient."""
    return (atol * ref["w"]).view(-1, 1, 1, 1) + rtol * ref["grad"].abs()


def worst_ratios(loss4, grad, ref, kink=None):
    """(loss error / its bar over loss[0..2] -- rtol 1e-5, a sum whose reference is 0 must be 0 --, class-gradient error / its bar over every
    element, regression-gradient error / its bar with the `kink` anchors left out)."""
    got = torch.as_tensor(loss4, dtype=torch.float64)[:3]
    want = torch.tensor([ref["cls"], ref["reg"], ref["qsum"]], dtype=torch.float64)
    d = (got - want).abs()
    lr = torch.where(d == 0, torch.zeros_like(d), d / (1e-5 * want.abs()))
    lr = torch.where(torch.isnan(lr), torch.full_like(lr, float("inf")), lr)
    r = (grad.double() - ref["grad"]).abs() / bars(ref)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    nt = r.shape[1] // 5
    rc, rr = r[:, :nt], r[:, nt:]
    if kink is not None:
        rr = torch.where(kink.repeat(1, 4, 1, 1), torch.zeros_like(rr), rr)
    return float(lr.max()), float(rc.max()), float(rr.max())


# (B, nt, H, W): E = 15 (less than a wave), exactly one block, 2025 = two blocks with a tail, many blocks, and one 25 x 63 x 63 image
LOSS_SHAPES = ((1, 1, 3, 5), (3, 16, 8, 8), (2, 25, 9, 9), (3, 25, 20, 20), (1, 25, 63, 63))
PLANTED_TARGETS = (0.0, 1.0, 1.5, -0.5, float("nan"))


@functools.lru_cache(maxsize=None)
def loss_case(shape, variant="drawn"):
    """(out, class_map, reg_map, align_map) on `shape`: labels and targets drawn by loss_cases.crit_inputs, the four predictions of every anchor
    = target + 0.1 randn (the high-overlap regime, where an anchor next to a kink is rare), align_map uniform in (0, 1) everywhere -- a kernel that
    reads it at a negative shows -- with PLANTED_TARGETS on the first positives of every image that has five.  Variants: "drawn"; "no_positive":
    image 0 has none; "small_targets": every target of image 0 scaled so that its sum stays below 1 (the max(1, .) clamp); "ones": align_map = 1.
    Cached: do not modify."""
    B, nt, H, W = shape
    E = nt * H * W
    g = torch.Generator().manual_seed(5200 + E % 101 + B)
    npos = [max(2, min(E // 8, 40 + 13 * b)) for b in range(B)]
    nneg = [max(3, min(E // 2, 300 + 50 * b)) for b in range(B)]
    import loss_cases as lc
    out, cm, rm = lc.crit_inputs(B, nt, H, W, 5300 + E % 97 + B, npos, nneg)
    out, cm = out.clone(), cm.clone()
    out[:, nt:] = rm + 0.1 * torch.randn(rm.shape, generator=g)
    al = torch.rand(cm.shape, generator=g)
    flat, lab = al.view(B, E), cm.view(B, E)
    if variant == "ones":
        al.fill_(1.0)
        return out, cm, rm, al
    for b in range(B):
        idx = torch.nonzero(lab[b] == 1).flatten()
        if idx.numel() >= 2 * len(PLANTED_TARGETS):
            flat[b, idx[:len(PLANTED_TARGETS)]] = torch.tensor(PLANTED_TARGETS)
    if variant == "no_positive":
        lab[0][lab[0] == 1] = -1
    elif variant == "small_targets":
        idx = torch.nonzero(lab[0] == 1).flatten()
        flat[0, idx] = flat[0, idx].nan_to_num(0.0).clamp(0, 1) * (0.7 / max(1.0, float(flat[0, idx].nan_to_num(0.0).clamp(0, 1).sum())))
    elif variant != "drawn":
        raise ValueError(variant)
    return out, cm, rm, al


@functools.lru_cache(maxsize=None)
def loss_reference(shape, variant, reg_loss, beta, normalize):
    out, cm, rm, al = loss_case(shape, variant)
    nt = shape[1]
    return aligned_loss(out, cm, rm, al, nt, reg_loss, br.template_wh(nt) if reg_loss == "diou" else None, beta, normalize)
