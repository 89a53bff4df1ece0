"""-m gpu: csrc/criterion.hip (tf_criterion_fwd_bwd) beyond the golden shapes: the block-count scan past 64 blocks, block edges,
the sampling caps' boundaries, inputs with nothing to learn from, and seed mode (the device RNG every training step uses): that the
kept labels are a subset of the candidates, that loss and gradient belong to the labels reported, and that the subset is uniform.

References and bars.  With injected keep flags: oracle.criterion with its permutation replayed, by the bars of
test_gpu_small_ops.py::test_criterion_golden (labels and the in-place OHEM map identical, the two loss sums within rtol 1e-5, the
gradient within rtol 1e-5 / atol 1e-6).  In seed mode: loss.py:74-88 restated in float64 (loss_cases.float64_loss) on the labels
the kernel returns, same bars.  tests/test_loss_front_end_fixtures.py shows on the CPU what each case can tell apart."""
import numpy as np
import pytest
import torch

import loss_cases as lc
from gpu_util import err, report

pytestmark = pytest.mark.gpu


def _assert_loss_grad(name, loss, grad, cls_ref, reg_ref, grad_ref, **extra):
    loss = loss.cpu().numpy()
    g = grad.cpu().numpy()
    gd = err(g, grad_ref.numpy())[0]
    report(name, cls=loss[0], cls_ref=cls_ref, reg=loss[1], reg_ref=reg_ref, grad_maxabs=gd, **extra)
    assert np.allclose([loss[0], loss[1]], [cls_ref, reg_ref], rtol=1e-5), name
    assert np.allclose(g, grad_ref.numpy(), rtol=1e-5, atol=1e-6), name


def _check_injected(name, out, cm, rm, nt, seed, ohem=0.03):
    from tinyfaces import ops
    r = lc.oracle_criterion(out, cm, rm, nt, seed, ohem_thresh=ohem)
    cm_d = cm.clone().cuda()
    loss, grad, labels = ops.criterion_fwd_bwd(out.cuda(), cm_d, rm.cuda(), n_templates=nt, ohem_thresh=ohem, pos_keep=r["pos_keep"],
                                               neg_keep=r["neg_keep"], want_labels=True)
    lab_mis = int((labels.cpu() != r["class_map_final"]).sum())
    ohem_mis = int((cm_d.cpu() != r["mined"]).sum())
    _assert_loss_grad(name, loss, grad, r["cls"], r["reg"], r["grad"], label_mismatch=lab_mis, ohem_mismatch=ohem_mis,
                      kept_pos=int((labels == 1).sum()), kept_neg=int((labels == -1).sum()))
    assert lab_mis == 0 and ohem_mis == 0, name
    return r


def _check_seed_mode(name, out, cm, rm, nt, seed, ohem=0.03, cap=128):
    """Seed mode is what it says: the labels are the mined candidates or 0, min(n, cap) of each sign per image, and loss and
    gradient are those of exactly these labels.  Returns (labels, mined) on the CPU."""
    from tinyfaces import ops
    cm_d = cm.clone().cuda()
    loss, grad, labels = ops.criterion_fwd_bwd(out.cuda(), cm_d, rm.cuda(), n_templates=nt, ohem_thresh=ohem, seed=seed, want_labels=True)
    lab, mined = labels.cpu(), cm_d.cpu()
    ref_mined = cm.clone()
    ref_mined[torch.nn.functional.soft_margin_loss(out[:, :nt], cm, reduction="none") < ohem] = 0
    assert torch.equal(mined, ref_mined), name
    assert bool(((lab == mined) | (lab == 0)).all()), name                     # a subset of the candidates
    for b in range(lab.shape[0]):
        for sign in (1, -1):
            n, k = int((mined[b] == sign).sum()), int((lab[b] == sign).sum())
            assert k == min(n, cap), (name, b, sign, n, k)
    c, rg, g = lc.float64_loss(out, lab, rm, nt)
    _assert_loss_grad(name, loss, grad, c, rg, g, kept_pos=int((lab == 1).sum()), kept_neg=int((lab == -1).sum()))
    return lab, mined


# ------------------------------------------------------------------------------------------------------------- 1: the scan
def test_criterion_scan_across_chunks():
    out, cm, rm = lc.scan_case()
    _check_injected("criterion_scan[flags]", out, cm, rm, 25, 5)
    lab, mined = _check_seed_mode("criterion_scan[seed]", out, cm, rm, 25, 17)
    assert int((lab.view(2, -1)[0, :65536] == 1).sum()) == 0 and int((lab[0] == 1).sum()) == 128


# ------------------------------------------------------------------------------------------------------------ 2: block edges
@pytest.mark.parametrize("B", [1, 12])
@pytest.mark.parametrize("si", range(3))
def test_criterion_block_edges(si, B):
    nt, H, W, (out, cm, rm) = lc.block_edge_inputs(B)[si]
    E = nt * H * W
    _check_injected(f"criterion_edges[E={E},B={B},flags]", out, cm, rm, nt, 60 + si)
    _check_seed_mode(f"criterion_edges[E={E},B={B},seed]", out, cm, rm, nt, 70 + si)


# ---------------------------------------------------------------------------------------------------------- 3: cap boundaries
def test_criterion_cap_boundaries():
    out, cm, rm = lc.cap_case()
    _check_injected("criterion_caps[flags]", out, cm, rm, 25, 6, ohem=0.0)
    lab, mined = _check_seed_mode("criterion_caps[seed]", out, cm, rm, 25, 23, ohem=0.0)
    assert torch.equal(mined, cm)
    for b, (p, n) in enumerate(lc.CAP_COUNTS):
        assert int((lab[b] == 1).sum()) == min(p, 128) and int((lab[b] == -1).sum()) == min(n, 128)
        if p <= 128:
            assert torch.equal(lab[b] == 1, cm[b] == 1)                        # at or under the cap: every label kept
        if n <= 128:
            assert torch.equal(lab[b] == -1, cm[b] == -1)


# ------------------------------------------------------------------------------------------------------ 4: nothing to learn
def test_criterion_nothing_to_learn_from():
    from tinyfaces import ops
    nt, H, W = 25, 9, 11
    # (a) an all-zero class map
    out, cm, rm = lc.crit_inputs(2, nt, H, W, 81, 0, 0)
    grad = torch.full_like(out, float("nan")).cuda()
    loss, g, lab = ops.criterion_fwd_bwd(out.cuda(), cm.clone().cuda(), rm.cuda(), seed=3, want_labels=True, grad=grad)
    assert g is grad
    assert loss.tolist() == [0.0, 0.0] and not bool(lab.any())
    assert bool((grad == 0).all())                                             # every element written, none NaN
    # (b) labels present, every logit so confident that OHEM mines all of them
    out, cm, rm = lc.crit_inputs(2, nt, H, W, 82, 300, 1500)
    out[:, :nt] = torch.where(cm != 0, 10.0 * cm, out[:, :nt])                 # soft margin = log1p(exp(-10)) = 4.5e-5 < 0.03
    cm_d = cm.clone().cuda()
    grad.fill_(float("nan"))
    loss, g, lab = ops.criterion_fwd_bwd(out.cuda(), cm_d, rm.cuda(), seed=3, want_labels=True, grad=grad)
    assert int((cm != 0).sum()) == 2 * 1800 and not bool(cm_d.any())           # zeroed in place
    assert loss.tolist() == [0.0, 0.0] and not bool(lab.any()) and bool((grad == 0).all())
    # (c) only one image of three has labels
    out, cm, rm = lc.crit_inputs(3, nt, H, W, 83, [0, 300, 0], [0, 1500, 0])
    r = lc.oracle_criterion(out, cm, rm, nt, 9)
    grad = torch.full_like(out, float("nan")).cuda()
    loss, _, lab = ops.criterion_fwd_bwd(out.cuda(), cm.clone().cuda(), rm.cuda(), pos_keep=r["pos_keep"], neg_keep=r["neg_keep"],
                                         want_labels=True, grad=grad)
    _assert_loss_grad("criterion_one_of_three", loss, grad, r["cls"], r["reg"], r["grad"])
    assert torch.equal(lab.cpu(), r["class_map_final"])
    assert bool((grad[0] == 0).all()) and bool((grad[2] == 0).all())
    l1 = lab[1].cpu()
    assert int((l1 == 1).sum()) == 128 and int((l1 == -1).sum()) == 128
    g1 = grad[1].cpu()
    assert bool((g1[:nt][l1 == 0] == 0).all()) and bool((g1[nt:][(l1 <= 0).repeat(4, 1, 1)] == 0).all())
    assert int((g1[:nt] != 0).sum()) == 256
    # ... and image 1 alone gives image 1's result
    loss_a, grad_a, lab_a = ops.criterion_fwd_bwd(out[1:2].cuda(), cm[1:2].clone().cuda(), rm[1:2].cuda(), pos_keep=r["pos_keep"][1:2],
                                                  neg_keep=r["neg_keep"][1:2], want_labels=True)
    assert torch.equal(lab_a[0], lab[1]) and torch.equal(grad_a[0], grad[1])
    assert np.allclose(loss_a.cpu().numpy(), loss.cpu().numpy(), rtol=1e-5)    # the same terms, summed by atomics in another order


# --------------------------------------------------------------------------------------------- 5: seed mode is what it says
def _golden_criterion(golden, tag):
    g = golden("criterion")
    return (torch.from_numpy(g[f"{tag}_output"]), torch.from_numpy(g[f"{tag}_class_map"].astype(np.float32)), torch.from_numpy(g[f"{tag}_reg_map"]))


@pytest.mark.parametrize("which", ["scan", "k1", "k3", "rng63"])
def test_criterion_seed_mode_is_what_it_says(golden, which):
    out, cm, rm = {"scan": lc.scan_case, "rng63": lc.rng_mode_inputs}[which]() if which in ("scan", "rng63") else _golden_criterion(golden, which)
    # image 0 once more at the end of the batch: identical inputs, another image index
    out, cm, rm = (torch.cat([x, x[:1]]) for x in (out, cm, rm))
    lab, mined = _check_seed_mode(f"criterion_seed_mode[{which}]", out, cm, rm, 25, 11)
    B = lab.shape[0]
    assert torch.equal(mined[0], mined[B - 1])
    assert max(int((mined[0] == 1).sum()), int((mined[0] == -1).sum())) > 128  # there is something to sample
    assert not torch.equal(lab[0], lab[B - 1])                                 # ... and the two images keep different subsets
    # another seed, another subset
    lab2, _ = _check_seed_mode(f"criterion_seed_mode[{which},seed 12]", out, cm, rm, 25, 12)
    assert not torch.equal(lab, lab2)


def test_criterion_seed_mode_signs_draw_apart():
    """n_pos == n_neg: the two signs of one image must not keep the same set of ranks."""
    out, cm, rm = lc.crit_inputs(2, 25, 8, 8, 91, 200, 200)
    lab, mined = _check_seed_mode("criterion_equal_counts", out, cm, rm, 25, 4, ohem=0.0)
    for b in range(2):
        m, l = mined[b].reshape(-1), lab[b].reshape(-1)
        pos_ranks = torch.nonzero(l[m == 1] == 1).flatten()
        neg_ranks = torch.nonzero(l[m == -1] == -1).flatten()
        assert pos_ranks.numel() == 128 and neg_ranks.numel() == 128
        assert not torch.equal(pos_ranks, neg_ranks)


# ------------------------------------------------------------------------------------------------- 6: the subset is uniform
def test_criterion_seed_mode_subset_is_uniform():
    """2000 seeds, 128 of 200 positives and 128 of 300 negatives each time.  Under a uniform sampler each candidate's count is
    Binomial(T, 128 / n): max |z| <= 5 and |corr(z, rank)| sqrt(n) <= 5 are five standard deviations of the null hypothesis, and the
    kernel and the seeds are deterministic.  The CPU file holds the reference's np.random.permutation to the same statistic, and shows
    that a sampler leaning 5 % towards low ranks fails it."""
    from tinyfaces import ops
    out, cm, rm = lc.uniformity_case()
    out_d, cm_d, rm_d = out.cuda(), cm.cuda(), rm.cuda()
    grad = torch.empty_like(out_d)
    T = lc.UNIFORMITY_SEEDS
    kept_pos = torch.zeros(cm.shape, dtype=torch.int32, device="cuda")
    kept_neg = torch.zeros_like(kept_pos)
    for seed in range(T):
        _, _, lab = ops.criterion_fwd_bwd(out_d, cm_d, rm_d, ohem_thresh=0.0, seed=seed, want_labels=True, grad=grad)
        kept_pos += lab == 1
        kept_neg += lab == -1
    assert torch.equal(cm_d.cpu(), cm)                                         # ohem_thresh = 0 mines nothing
    flat = cm.reshape(-1)
    for sign, kept, n in ((1, kept_pos, 200), (-1, kept_neg, 300)):
        kept = kept.cpu().reshape(-1)
        assert int(kept[flat != sign].sum()) == 0 and int(kept.sum()) == 128 * T
        count = kept[flat == sign].numpy()                                     # C-order = rank order
        assert count.size == n
        zmax, corr, chi = lc.uniformity_stats(count, T)
        report(f"criterion_uniformity[{'pos' if sign > 0 else 'neg'},n={n}]", seeds=T, max_abs_z=zmax, corr_scaled=corr, z2_over_dof=chi)
        assert zmax <= 5 and corr <= 5


# ------------------------------------------------------------------------------------------------------------ 7: small ends
def test_criterion_grad_buffer_and_no_labels():
    from tinyfaces import ops
    out, cm, rm = lc.crit_inputs(3, 25, 16, 16, 95, 400, 4000)
    out_d, rm_d = out.cuda(), rm.cuda()
    _, g0, lab = ops.criterion_fwd_bwd(out_d, cm.clone().cuda(), rm_d, seed=8, want_labels=True)
    buf = torch.full_like(out_d, float("nan"))
    _, g1, none = ops.criterion_fwd_bwd(out_d, cm.clone().cuda(), rm_d, seed=8, want_labels=False, grad=buf)
    assert none is None and g1 is buf and lab is not None
    assert torch.equal(g0, buf)
