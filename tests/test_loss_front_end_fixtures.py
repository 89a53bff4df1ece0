"""CPU: what the GPU tests of the loss front end (tests/test_gpu_targets.py, tests/test_gpu_criterion.py) stand on.
  * the oracle of the target assignment equals the reference's own code on maps that are not square
    (tests/golden/targets_geometry.npz, written by oracle/tools/make_golden.py), by the rule test_oracle_small_ops.py applies at 63 x 63;
  * every case of tests/loss_cases.py can tell apart the bug it is there for: run on the oracle with that bug made, it gives another answer."""
import numpy as np
import pytest
import torch

import loss_cases as lc
from gpu_util import report
from oracle import targets as otgt


# ------------------------------------------------------------------------------------------------------ oracle vs reference
@pytest.mark.parametrize("ci", range(4))
def test_targets_oracle_matches_reference_off_square(golden, ci):
    g = golden("targets_geometry")
    tag = f"g{ci}"
    nt = int(g[f"{tag}_nt"])
    t = golden("targets")["templates"][:nt]
    vsy, vsx = (int(v) for v in g[f"{tag}_heatmap_size"])
    assert vsy != vsx
    rf = {"size": [859, 859], "stride": g[f"{tag}_rf_stride"].tolist(), "offset": g[f"{tag}_rf_offset"].tolist()}
    (ofy, ofx), (sty, stx) = rf["offset"], rf["stride"]
    boxes = g[f"{tag}_boxes"]
    assert 3 <= boxes.shape[0] <= 6 and lc.valid(boxes).shape[0] == boxes.shape[0]
    iou = otgt.dense_overlap(ofx, ofy, stx, sty, vsx, vsy, t[:, 0], t[:, 1], t[:, 2], t[:, 3], boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3])
    assert np.array_equal(iou[::4, ::4], g[f"{tag}_iou"])             # bit-exact, float64
    assert iou.sum() == float(g[f"{tag}_iou_sum"])
    pad = otgt.get_padding(t, g[f"{tag}_paste"], rf=rf, heatmap_size=(vsy, vsx))
    if int(g[f"{tag}_flip"]):
        pad = np.fliplr(pad)
    assert np.array_equal(np.packbits(pad), g[f"{tag}_pad"])
    np.random.seed(int(g[f"{tag}_seed"]))
    noise = np.random.rand(vsy, vsx, nt, boxes.shape[0])
    cm, rm, ioup = otgt.get_heatmaps(boxes.copy(), t, pad, noise=noise, rf=rf, heatmap_size=(vsy, vsx))
    assert np.array_equal(cm.astype(np.int8), g[f"{tag}_class"])
    assert np.array_equal(rm[::4, ::4], g[f"{tag}_reg"])
    assert rm.sum() == float(g[f"{tag}_reg_sum"])
    assert np.array_equal(ioup.max(axis=(0, 1, 2)), g[f"{tag}_ioupert_max"])
    assert (cm == 1).sum() > 0 and (cm == 0).sum() > 0


def test_targets_fixture_geometries(golden):
    g = golden("targets_geometry")
    seen = {(tuple(g[f"{c}_input_size"]), tuple(g[f"{c}_heatmap_size"])) for c in g["cases"]}
    assert seen == {((340, 500), (43, 63)), ((500, 316), (63, 40)), ((340, 500), (43, 32))}
    assert [g[f"{c}_rf_stride"].tolist() for c in g["cases"]] == [[8, 8]] * 3 + [[8, 16]]
    assert {int(g[f"{c}_flip"]) for c in g["cases"]} == {0, 1}
    for c in g["cases"]:
        p = g[f"{c}_paste"]
        assert (p[0], p[2]) != (p[1], p[3])


# ------------------------------------------------------------------------------------------------ targets: discrimination
def test_geometry_cases_tell_the_exchanges_apart(templates):
    cases = lc.geometry_cases(templates)
    assert {c["hm"] for c in cases} == {(43, 63), (63, 40), (7, 9), (43, 32)} and {c["nt"] for c in cases} == {25, 7} and len(cases) == 14
    assert sum(c["rf"] is lc.RF_YX for c in cases) == 2
    for c in cases:
        right, mutants = lc.geometry_mutants(c)
        n = right.size // 5
        assert (right[:n] == 1).sum() > 0 and (right[:n] == 0).sum() > 0, c["name"]
        for what, m in mutants.items():
            assert not np.array_equal(right[:n], m[:n]), f"{c['name']}: labels blind to {what}"
            assert not np.array_equal(right[n:], m[n:]), f"{c['name']}: regression blind to {what}"


def test_mixed_batch_is_mixed(templates):
    m = lc.mixed_batch()
    assert [lc.valid(b).shape[0] for b in m["boxes"]] == [16, 0, 0, 3, 1, 0] and m["boxes"][2].shape[0] == 3
    assert m["flips"] == [1, 0, 1, 1, 0, 0] and len({tuple(p) for p in m["paste"]}) == 6
    t = m["boxes"][3]
    assert np.array_equal(t[0], t[1]) and not np.array_equal(t[0], t[2])
    # an owner search that stops at the images without boxes, or a paste / flip row taken from a neighbour, changes labels:
    # image 3 and image 4 get other labels under each other's paste box and flip
    for b, o in ((3, 4), (4, 3)):
        own = lc.oracle_maps(m["boxes"][b], templates, m["paste"][b], m["flips"][b], m["noise"][b])[0]
        for paste, flip in ((m["paste"][o], m["flips"][b]), (m["paste"][b], 1 - m["flips"][b])):
            assert not np.array_equal(own, lc.oracle_maps(m["boxes"][b], templates, paste, flip, m["noise"][b])[0])


def test_tie_case_holds_exact_ties_on_both_axes(templates):
    c = lc.tie_case()
    assert not c["noise"].any()
    cm, rm, iou = lc.oracle_maps(c["boxes"], templates, c["paste"], c["flip"], c["noise"])
    anchor_ties, box_ties = lc.tie_counts(iou)
    assert anchor_ties > 0 and box_ties > 0, (anchor_ties, box_ties)
    # ... and the choice among the tied shows: taking the LAST arg-max instead of the first gives other maps
    rev = iou[..., ::-1]
    last_box = iou.shape[3] - 1 - rev.argmax(axis=3)
    assert (last_box != iou.argmax(axis=3)).any()
    per = iou.reshape(-1, iou.shape[3])
    top = per.max(axis=0)
    first, last = per.argmax(axis=0), per.shape[0] - 1 - per[::-1].argmax(axis=0)
    moved = [g for g in range(per.shape[1]) if otgt.NEG_THRESH < top[g] < otgt.POS_THRESH and first[g] != last[g]]
    assert any(cm.reshape(-1)[first[g]] == 1 and cm.reshape(-1)[last[g]] != 1 for g in moved)


def test_seed_mode_masks_exempt_only_what_the_noise_can_move(templates):
    for m in (lc.mixed_batch(), lc.other_batch()):
        for b in range(6):
            bv = lc.valid(m["boxes"][b])
            if not bv.shape[0]:
                continue
            _, _, iou = lc.oracle_maps(bv, templates, m["paste"][b], m["flips"][b], np.zeros((63, 63, 25, bv.shape[0])))
            settled, near_thr, tie = lc.seed_mode_masks(iou)
            best = iou.max(axis=3)
            twins = bv.shape[0] == 3                                       # two identical boxes tie wherever they are the best
            assert settled[best > 0].mean() > (0.0 if twins else 0.5)
            per = iou.reshape(-1, iou.shape[3])
            top = per.max(axis=0)
            for g in range(per.shape[1]):
                first = per[:, g].argmax()
                runner_up = np.delete(per[:, g], first).max()
                if top[g] - runner_up > 1e-6 and abs(top[g] - otgt.NEG_THRESH) > 1e-6:
                    # a unique best anchor is exempt from nothing (unless another box's contest runs through it)
                    others = [h for h in range(per.shape[1]) if h != g and per[first, h] >= top[h] - 1e-6]
                    assert others or not tie.reshape(-1)[first], (b, g)
            assert tie.sum() + near_thr.sum() < 40
    # the mixed batch does hold boxes whose label comes from the best-anchor rule alone and whose best anchor is unique:
    # dropping or misplacing phase B / C in seed mode shows as an unexplained difference
    m = lc.mixed_batch()
    pinned_best = 0
    for b in (0, 3, 4):
        bv = lc.valid(m["boxes"][b])
        ocm, _, iou = lc.oracle_maps(bv, templates, m["paste"][b], m["flips"][b], np.zeros((63, 63, 25, bv.shape[0])))
        _, near_thr, tie = lc.seed_mode_masks(iou)
        per = iou.reshape(-1, iou.shape[3])
        for g in range(per.shape[1]):
            first = per[:, g].argmax()
            if otgt.NEG_THRESH < per[first, g] and per[first].max() < otgt.POS_THRESH and ocm.reshape(-1)[first] == 1:
                pinned_best += not (tie.reshape(-1)[first] or near_thr.reshape(-1)[first])
    assert pinned_best >= 1, pinned_best


# ---------------------------------------------------------------------------------------------- criterion: discrimination
def test_scan_case_needs_the_carry():
    out, cm, rm = lc.scan_case()
    E = cm[0].numel()
    assert E == 67600 and (E + 1023) // 1024 == 67
    r = lc.oracle_criterion(out, cm, rm, 25, 5)
    mined = r["mined"].view(2, E)
    assert int((mined[0, :65536] == 1).sum()) == 0 and int((mined[0] == 1).sum()) > 128
    for b in range(2):
        for sign, keep in ((1, r["pos_keep"]), (-1, r["neg_keep"])):
            n = int((mined[b] == sign).sum())
            base = int((mined[b, :65536] == sign).sum())       # what the scan must carry into block 64
            assert n > 128 and n - base > 0
            kept = keep[b, :n].numpy()
            assert kept.sum() == 128
            if base:
                # with the carry lost, the labels of blocks 64.. read the flags of ranks 0.. instead of base..: these differ
                assert not np.array_equal(kept[base:n], kept[:n - base]), (b, sign)
            assert kept[base:n].min() != kept[base:n].max(), (b, sign)
    lab = r["class_map_final"].view(2, E)
    assert int((lab[0] == 1).sum()) == 128 and int((lab[0] == -1).sum()) == 128


def test_block_edge_and_cap_cases_are_what_they_say():
    for B in (1, 12):
        shapes = [(nt * H * W) for nt, H, W, _ in lc.block_edge_inputs(B)]
        assert shapes == [15, 1024, 8192]
    out, cm, rm = lc.cap_case()
    r = lc.oracle_criterion(out, cm, rm, 25, 6, ohem_thresh=0.0)
    assert torch.equal(r["mined"], cm)                          # nothing mined
    for b, (p, n) in enumerate(lc.CAP_COUNTS):
        assert int((cm[b] == 1).sum()) == p and int((cm[b] == -1).sum()) == n
        fin = r["class_map_final"][b]
        assert int((fin == 1).sum()) == min(p, 128) and int((fin == -1).sum()) == min(n, 128)


def test_float64_loss_is_the_oracle_on_its_labels(golden):
    g = golden("criterion")
    out, cm, rm = (torch.from_numpy(g[f"k1_{k}"].astype(np.float32)) for k in ("output", "class_map", "reg_map"))
    r = lc.oracle_criterion(out, cm, rm, 25, int(g["k1_seed"]))
    c, rg, grad = lc.float64_loss(out, r["class_map_final"], rm, 25)
    assert np.allclose([c, rg], [r["cls"], r["reg"]], rtol=1e-6)
    assert np.allclose(grad.numpy(), r["grad"].numpy(), rtol=1e-6, atol=1e-7)


def test_uniformity_statistic_passes_the_reference_sampler_and_has_power():
    T = lc.UNIFORMITY_SEEDS
    rng = np.random.RandomState(0)
    for n in (300, 200):
        count = np.zeros(n)
        for _ in range(T):
            count[rng.permutation(n)[:128]] += 1                  # utils.py:155: the reference's own sampler
        zmax, corr, chi = lc.uniformity_stats(count, T)
        report(f"uniformity_reference_sampler[{n}]", max_abs_z=zmax, corr_scaled=corr, z2_over_dof=chi)
        assert zmax <= 5 and corr <= 5
        # a sampler whose keep probability falls by +-5 % from the first rank to the last must fail
        w = 1 + 0.05 * (1 - 2 * np.arange(n) / (n - 1))
        biased = np.zeros(n)
        for _ in range(T):
            biased[np.argsort(rng.exponential(size=n) / w)[:128]] += 1     # weighted draw without replacement
        bzmax, bcorr, _ = lc.uniformity_stats(biased, T)
        report(f"uniformity_biased_sampler[{n}]", max_abs_z=bzmax, corr_scaled=bcorr)
        assert bcorr > 5
