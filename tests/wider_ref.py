"""numpy restatement of the PARALLEL form of the WIDER matching (csrc/wider_eval.hip), and the seeded cases the CPU and the GPU tests share.
Never imported by the package.  The sequential reference is tinyfaces.wider_eval.image_evaluation / image_pr_info; tests/test_wider_device.py
holds this restatement to it exactly, tests/test_gpu_wider_eval.py holds the kernels to it exactly.

    best[h]      = argmax_j IoU(det h, box j) (lowest index on a tie) if that IoU >= iou_thresh, else -1      -- independent of the other detections
    first[j]     = min{h : best[h] == j}                                                                      -- an integer min
    proposal[h]  = -1 iff best[h] >= 0 and the box is not kept
    recalled[h]  = prefix sum of (best[h] >= 0 and kept[best[h]] and first[best[h]] == h)
    counted[h]   = prefix sum of (proposal[h] == 1)"""
import numpy as np

from tinyfaces import wider_eval as we


def best_match(pred, gt, iou_thresh=0.5):
    N, G = pred.shape[0], gt.shape[0]
    best = np.full(N, -1, dtype=np.int64)
    if G == 0:
        return best
    p = pred[:, :4].astype(np.float64).copy(); p[:, 2] += p[:, 0]; p[:, 3] += p[:, 1]
    g = gt[:, :4].astype(np.float64).copy(); g[:, 2] += g[:, 0]; g[:, 3] += g[:, 1]
    for h in range(N):
        ov = we.box_overlap(g, p[h])
        j = int(np.argmax(ov))
        if ov[j] >= iou_thresh:
            best[h] = j
    return best


def parallel_evaluation(pred, gt, keep_mask, iou_thresh=0.5):
    """(counted, recalled, proposal) of one image in the parallel form."""
    N, G = pred.shape[0], gt.shape[0]
    best = best_match(pred, gt, iou_thresh)
    keep_mask = np.asarray(keep_mask, dtype=bool)
    first = np.full(G, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(first, best[best >= 0], np.nonzero(best >= 0)[0])
    matched = best >= 0
    kept = np.zeros(N, dtype=bool)
    kept[matched] = keep_mask[best[matched]]
    proposal = np.where(matched & ~kept, -1, 1)
    new = np.zeros(N, dtype=bool)
    new[matched] = kept[matched] & (first[best[matched]] == np.nonzero(matched)[0])
    return np.cumsum(proposal == 1), np.cumsum(new), proposal


def host_counts(pred, gt, keep_mask, iou_thresh=0.5):
    """(counted, recalled) from the sequential reference; an image without boxes matches nothing."""
    if gt.shape[0] == 0:
        return np.arange(1, pred.shape[0] + 1), np.zeros(pred.shape[0], dtype=np.int64)
    pred_recall, proposal = we.image_evaluation(pred, gt, np.asarray(keep_mask, dtype=bool), iou_thresh)
    return np.cumsum(proposal == 1), pred_recall


def random_image(rng, N, G, nset=1, dup=True, ties=True, quantum=None):
    """pred (N,5) score-descending, gt (G,4), keep masks (nset, G) bool.  Integer geometry (result-file form).  With dup some boxes are
    repeated, which gives bit-equal IoUs (the lowest index must win); with ties scores repeat; about a third of the boxes is ignored in
    every setting, independently, so a box is ignored in one setting and kept in another."""
    gt = np.column_stack([rng.randint(0, 300, (G, 2)), rng.randint(4, 80, (G, 2))]).astype(np.float64)
    if dup and G >= 2:
        for _ in range(max(1, G // 4)):
            a, b = rng.randint(G), rng.randint(G)
            gt[b] = gt[a]
    rows = np.zeros((N, 5))
    for h in range(N):
        r = rng.rand()
        if G and r < 0.55:                                    # a jittered copy of a box: several detections land on one box
            rows[h, :4] = gt[rng.randint(G)] + rng.randint(-4, 5, 4)
        elif G and r < 0.7:                                   # an exact copy: IoU 1 with every duplicate of that box
            rows[h, :4] = gt[rng.randint(G)]
        else:
            rows[h, :4] = np.concatenate([rng.randint(0, 300, 2), rng.randint(4, 80, 2)])
    scores = rng.rand(N) if quantum is None else np.round(rng.rand(N) * quantum) / quantum
    if ties and N >= 2:
        scores[rng.randint(N, size=max(1, N // 3))] = scores[rng.randint(N)]
    rows[:, 4] = scores
    rows = rows[np.argsort(-rows[:, 4], kind="stable")]
    keep = rng.rand(nset, G) > 0.35
    return rows, gt, keep


def half_iou_image():
    """Integer boxes whose IoU with a detection is EXACTLY 0.5 (so `>= 0.5` must say match), a zero-area overlap (boxes that touch: w == 0),
    several detections on one box, a duplicated box and a box ignored in setting 1 only.  +1 convention: a box (x, y, w, h) covers
    (w + 1) x (h + 1) pixels.  gt 0 = (0, 0, 9, 9): area 100; det (0, 0, 9, 4): area 50, inside it: IoU 50 / 100 = 0.5.
    gt 1 = (100, 100, 9, 19): area 200; det (100, 100, 9, 9): area 100, inside: IoU 0.5."""
    gt = np.array([[0, 0, 9, 9], [100, 100, 9, 19], [200, 200, 9, 9], [200, 200, 9, 9], [300, 0, 9, 9]], dtype=np.float64)
    rows = np.array([[0, 0, 9, 4, 0.9],             # IoU exactly 0.5 with gt 0
                     [100, 100, 9, 9, 0.8],         # IoU exactly 0.5 with gt 1
                     [200, 200, 9, 9, 0.8],         # IoU 1 with gt 2 AND gt 3 (a duplicate): gt 2 wins; same score as the row before
                     [0, 0, 9, 9, 0.7],             # gt 0 again: already recalled
                     [201, 200, 9, 9, 0.6],         # gt 2 / gt 3 again, tie again
                     [310, 0, 9, 9, 0.5],           # touches gt 4: w = 309 - 310 + 1 = 0 -> overlap 0 by the rule, not by the quotient
                     [0, 5, 9, 4, 0.4],             # the other half of gt 0: IoU exactly 0.5 again
                     [300, 0, 9, 3, 0.3]],          # IoU 0.4 with gt 4: no match
                    dtype=np.float64)
    keep = np.array([[1, 1, 1, 1, 1], [1, 0, 1, 1, 1], [0, 1, 0, 1, 0]], dtype=bool)
    return rows, gt, keep


def concat(images):
    """images: [(rows, gt, keep)] -> rows (n,5), det offsets, gt (g,4), gt offsets, keep (nset, g) uint8."""
    nset = images[0][2].shape[0]
    rows = np.concatenate([r.reshape(-1, 5) for r, _, _ in images]) if images else np.zeros((0, 5))
    gt = np.concatenate([g.reshape(-1, 4) for _, g, _ in images]) if images else np.zeros((0, 4))
    keep = np.concatenate([k.reshape(nset, -1) for _, _, k in images], axis=1).astype(np.uint8)
    doff = np.concatenate([[0], np.cumsum([r.shape[0] for r, _, _ in images])]).astype(np.int64)
    goff = np.concatenate([[0], np.cumsum([g.shape[0] for _, g, _ in images])]).astype(np.int64)
    return rows, doff.tolist(), gt, goff.tolist(), keep


def host_counts_batched(images, iou_thresh=0.5):
    """(counted, recalled) int64 (nset, n) of the concatenation, from the sequential reference."""
    nset = images[0][2].shape[0]
    cs, rs = [], []
    for k in range(nset):
        per = [host_counts(r, g, kp[k], iou_thresh) for r, g, kp in images]
        cs.append(np.concatenate([c for c, _ in per]) if per else np.zeros(0, np.int64))
        rs.append(np.concatenate([r for _, r in per]) if per else np.zeros(0, np.int64))
    return np.stack(cs).astype(np.int64), np.stack(rs).astype(np.int64)


def host_pr_table(scores, doff, counted, recalled, lo, d, T):
    """sum over the segments of image_pr_info on the normalised scores, as integers (nset, T, 2)."""
    nset = counted.shape[0]
    pr = np.zeros((nset, T, 2), dtype=np.int64)
    for a, b in zip(doff, doff[1:]):
        if b == a:
            continue
        s = (scores[a:b] - lo) / d
        for k in range(nset):
            # image_pr_info takes proposal and cumsums it: rebuild a proposal whose cumsum is `counted`
            proposal = np.where(np.diff(np.concatenate([[0], counted[k, a:b]])) == 1, 1, -1)
            info = we.image_pr_info(s, proposal, recalled[k, a:b], T)
            assert np.array_equal(info, np.round(info))
            pr[k] += info.astype(np.int64)
    return pr


def synthetic_set(seed, n_img=40, nset=3):
    """A prediction set in evaluate_setting's form + the same content as lists: preds {event: {image: (N,5)}} (score-descending), gt_boxes,
    keep_lists per setting; images without boxes, images without rows, an image that is in the predictions but not in the ground truth
    (its scores still enter the normalisation)."""
    rng = np.random.RandomState(seed)
    names = [f"img_{i}" for i in range(n_img)]
    preds, gtb, keeps = {"ev": {}}, {"ev": {}}, [{"ev": {}} for _ in range(nset)]
    for i, name in enumerate(names):
        N = 0 if i % 11 == 3 else int(rng.randint(1, 60))
        G = 0 if i % 13 == 5 else int(rng.randint(1, 12))
        rows, gt, keep = random_image(rng, N, G, nset, quantum=64)
        preds["ev"][name], gtb["ev"][name] = rows, gt
        for k in range(nset):
            keeps[k]["ev"][name] = np.nonzero(keep[k])[0]
    extra = np.array([[5.0, 5.0, 20.0, 20.0, 1.5], [50.0, 50.0, 10.0, 10.0, -0.25]])        # not in the ground truth: widens (lo, hi) only
    preds["ev"]["stray"] = extra
    return preds, gtb, keeps
