"""Reference of the scale-compensated anchor matching (the rule in include/tinyfaces_hip.h), in numpy on top of oracle.targets:
get_heatmaps gives the class map the three existing phases leave and the perturbed IoU, get_padding the padding predicate.
Nothing here touches the GPU."""
import numpy as np

from oracle import targets as otgt


def compensate(class_map, iou, pad, N, T):
    """class_map (vsy, vsx, nt) and perturbed iou (vsy, vsx, nt, G) as get_heatmaps returns them, pad (vsy, vsx, nt) bool.
    Returns (the compensated class map, match_count (G,) int32 = positives each face owns afterwards).  The regression map is
    neither read nor written: the rule does not know it."""
    F = class_map.copy()
    G = iou.shape[3]
    counts = np.zeros(G, np.int32)
    if G == 0:
        return F, counts
    own, best = iou.argmax(axis=3), iou.max(axis=3)               # first arg-max, like phase A
    flat = np.arange(best.size).reshape(best.shape)               # (y * vsx + x) * nt + t
    out = F.reshape(-1)
    for g in range(G):
        mine = own == g
        count = int((mine & (class_map == 1)).sum())
        cand = mine & ~pad & (class_map != 1) & (best >= T)
        idx, b = flat[cand], best[cand]
        take = idx[np.lexsort((idx, -b))][:max(0, N - count)]
        out[take] = 1
        counts[g] = count + take.size
    return F, counts


def owned_positives(class_map, iou):
    """count(g) of the rule: anchors labelled +1 whose owner is g."""
    G = iou.shape[3]
    if G == 0:
        return np.zeros(0, np.int32)
    own = iou.argmax(axis=3)
    return np.bincount(own[class_map == 1], minlength=G).astype(np.int32)


def compensated_maps(boxes, t, paste, flip, noise, N, T, hm=(63, 63), rf=otgt.RF, pos_thresh=otgt.POS_THRESH, neg_thresh=otgt.NEG_THRESH):
    """One image (valid boxes only): (plain class map, compensated class map, regression map, match_count), maps HWC."""
    pad = otgt.get_padding(t, paste, rf=rf, heatmap_size=hm)
    if flip:
        pad = np.fliplr(pad)
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    cm, rm, iou = otgt.get_heatmaps(boxes.copy(), t, pad, noise=noise, rf=rf, heatmap_size=hm, pos_thresh=pos_thresh, neg_thresh=neg_thresh)
    F, counts = compensate(cm, iou, pad, N, T)
    return cm, F, rm, counts
