"""Native WIDER FACE evaluator: average precision for the easy / medium / hard settings from the
result files `write_results` produces (tinyfaces/evaluation.py:90-114) -- the step the reference delegates to the external
MATLAB/Octave `eval_tools` (Makefile:20-21, README.md:49).

PARITY UNPINNED: eval_tools is third-party MATLAB code that is neither part of the reference repository nor runnable here, and the WIDER
ground-truth .mat files are not available offline.  This module restates the published protocol (eval_tools: wider_eval.m,
evaluation.m, image_evaluation / image_pr_info / dataset_pr_info, norm_score.m, boxoverlap.m, VOCap.m):
  * scores min-max normalised over the whole prediction set;
  * per image, detections in descending score order are matched to the ground-truth box of highest IoU (+1 pixel areas);
    IoU >= 0.5 with an IGNORED box (not in the setting's keep list) removes the detection from the precision count, with a kept
    box not yet recalled it counts as a true positive;
  * precision / recall accumulated over 1000 score thresholds, AP = VOC 2010+ area under the monotone precision envelope.
Host-side numpy; tests/test_host_logic.py checks it on hand-computed cases and against a brute-force re-derivation."""
import os

import numpy as np

THRESH_NUM = 1000


def box_overlap(gt, det):
    """IoU of every row of gt (G,4: x1,y1,x2,y2) with one det box, MATLAB pixel convention (+1 on widths / heights)."""
    x1 = np.maximum(gt[:, 0], det[0]); y1 = np.maximum(gt[:, 1], det[1])
    x2 = np.minimum(gt[:, 2], det[2]); y2 = np.minimum(gt[:, 3], det[3])
    w, h = x2 - x1 + 1, y2 - y1 + 1
    inter = w * h
    a = (gt[:, 2] - gt[:, 0] + 1) * (gt[:, 3] - gt[:, 1] + 1)
    b = (det[2] - det[0] + 1) * (det[3] - det[1] + 1)
    o = inter / (a + b - inter)
    o[(w <= 0) | (h <= 0)] = 0
    return o


def image_evaluation(pred, gt, keep_mask, iou_thresh=0.5):
    """pred (N,5: x,y,w,h,score; score-descending), gt (G,4: x,y,w,h), keep_mask (G,) bool.  Returns pred_recall (N,) = number of
    kept ground-truth boxes recalled by the first h detections, proposal (N,) = 1 (counts towards precision) or -1 (ignored)."""
    N, G = pred.shape[0], gt.shape[0]
    p = pred[:, :4].astype(np.float64).copy(); p[:, 2] += p[:, 0]; p[:, 3] += p[:, 1]
    g = gt[:, :4].astype(np.float64).copy(); g[:, 2] += g[:, 0]; g[:, 3] += g[:, 1]
    recall = np.zeros(G, dtype=np.int64)
    proposal = np.ones(N, dtype=np.int64)
    pred_recall = np.zeros(N, dtype=np.int64)
    for h in range(N):
        ov = box_overlap(g, p[h])
        idx = int(np.argmax(ov))
        if ov[idx] >= iou_thresh:
            if not keep_mask[idx]:
                recall[idx] = -1
                proposal[h] = -1
            elif recall[idx] == 0:
                recall[idx] = 1
        pred_recall[h] = int((recall == 1).sum())
    return pred_recall, proposal


def image_pr_info(scores, proposal, pred_recall, thresh_num=THRESH_NUM):
    """Per threshold t (1 - t/thresh_num, t = 1..thresh_num): (# counted detections with score >= t, # recalled boxes)."""
    out = np.zeros((thresh_num, 2), dtype=np.float64)
    counted = np.cumsum(proposal == 1)
    for t in range(thresh_num):
        thresh = 1 - (t + 1) / thresh_num
        idx = np.nonzero(scores >= thresh)[0]
        if idx.size:
            r = idx[-1]
            out[t, 0] = counted[r]
            out[t, 1] = pred_recall[r]
    return out


def voc_ap(rec, prec):
    """VOCap.m: area under the monotonically decreasing precision envelope."""
    mrec = np.concatenate(([0.0], rec, [1.0]))
    mpre = np.concatenate(([0.0], prec, [0.0]))
    for i in range(mpre.size - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    i = np.nonzero(mrec[1:] != mrec[:-1])[0] + 1
    return float(np.sum((mrec[i] - mrec[i - 1]) * mpre[i]))


def norm_scores(preds):
    """norm_score.m: min-max over every score of the prediction set.  preds: {event: {image: (N,5)}} -> new dict."""
    allv = [v[:, 4] for ev in preds.values() for v in ev.values() if v.shape[0]]
    if not allv:
        return preds
    lo, hi = min(float(v.min()) for v in allv), max(float(v.max()) for v in allv)
    d = hi - lo if hi > lo else 1.0
    return {e: {k: np.column_stack([v[:, :4], (v[:, 4] - lo) / d]) if v.shape[0] else v for k, v in ev.items()} for e, ev in preds.items()}


def evaluate_setting(preds, gt_boxes, keep_lists, iou_thresh=0.5, thresh_num=THRESH_NUM):
    """preds {event: {image: (N,5) score-descending, normalised}}, gt_boxes {event: {image: (G,4) x,y,w,h}},
    keep_lists {event: {image: 0-based indices of the boxes that count in this setting}}.  Returns (AP, pr_curve (T,2))."""
    pr = np.zeros((thresh_num, 2))
    count_face = 0
    for e, images in gt_boxes.items():
        for name, gt in images.items():
            keep = np.asarray(keep_lists.get(e, {}).get(name, []), dtype=np.int64).reshape(-1)
            count_face += keep.size
            pred = preds.get(e, {}).get(name)
            if gt.shape[0] == 0 or pred is None or pred.shape[0] == 0:
                continue
            mask = np.zeros(gt.shape[0], dtype=bool)
            mask[keep] = True
            pred_recall, proposal = image_evaluation(pred, gt, mask, iou_thresh)
            pr += image_pr_info(pred[:, 4], proposal, pred_recall, thresh_num)
    return precision_recall_ap(pr, count_face)


def precision_recall_ap(pr, count_face):
    """The tail of evaluate_setting, shared with DeviceEvaluator so that the two cannot drift: pr (T,2) float64 = (# counted detections,
    # recalled boxes) per threshold, summed over the images; count_face = the boxes that count.  Returns (AP, pr_curve (T,2))."""
    thresh_num = pr.shape[0]
    precision = np.divide(pr[:, 1], pr[:, 0], out=np.zeros(thresh_num), where=pr[:, 0] > 0)      # MATLAB's max() skips the 0/0 NaNs
    recall = pr[:, 1] / max(count_face, 1)
    return voc_ap(recall, precision), np.stack([precision, recall], 1)


class DeviceEvaluator:
    """evaluate_setting(norm_scores(...)) for several settings at once with the matching and the PR table on the device
    (ops.wider_match_batched / ops.wider_pr_accumulate), held to the host functions above bit for bit: the table is integers.

        ev = DeviceEvaluator(("easy", "medium", "hard"))
        for every batch of images:  ev.add(rows, gt, keep_lists)
        {setting: (ap, pr_curve)} = ev.finish()

    Every image of the ground truth is added once, with an empty (0,5) array when it has no detection: its kept boxes count in the
    recall.  Nothing is read back before finish(), which makes one host read of the nset x T x 2 table."""

    def __init__(self, settings, iou_thresh=0.5, thresh_num=THRESH_NUM, device="cuda"):
        import torch
        self.settings = tuple(settings)
        if not self.settings:
            raise ValueError("DeviceEvaluator: at least one setting")
        if isinstance(thresh_num, bool) or not isinstance(thresh_num, (int, np.integer)) or thresh_num < 1:
            raise ValueError(f"DeviceEvaluator: thresh_num={thresh_num!r}, expected an integer >= 1")
        self.iou_thresh, self.thresh_num, self.device = float(iou_thresh), int(thresh_num), torch.device(device)
        self.reset()

    def reset(self):
        self.count_face = [0] * len(self.settings)
        self._scores, self._counted, self._recalled, self._offsets = [], [], [], [0]
        self._lo = self._hi = None

    def _keep_of(self, keep_lists, n_images):
        per_setting = [keep_lists[s] for s in self.settings] if isinstance(keep_lists, dict) else list(keep_lists)
        if len(per_setting) != len(self.settings) or any(len(k) != n_images for k in per_setting):
            raise ValueError(f"DeviceEvaluator.add: keep_lists holds one list of {n_images} index lists for each of the {len(self.settings)} settings")
        return [[np.asarray(k, dtype=np.int64).reshape(-1) for k in ks] for ks in per_setting]

    def add(self, rows, gt, keep_lists):
        """One batch of images.  rows: per image an (K,5) array x, y, w, h, score in result-file form (ops.wider_rows), numpy or tensor, in
        any order; gt: per image an (G,4) array x, y, w, h; keep_lists: per setting (a sequence in the order of `settings`, or a dict by
        setting) one list per image of the 0-based indices of the boxes that count, as evaluate_setting takes them."""
        import torch
        from . import ops
        dev = self.device
        rows, gt = list(rows), list(gt)
        if len(rows) != len(gt):
            raise ValueError(f"DeviceEvaluator.add: {len(rows)} row arrays for {len(gt)} ground-truth arrays")
        keeps = self._keep_of(keep_lists, len(gt))
        gts = [np.asarray(g.cpu() if torch.is_tensor(g) else g, dtype=np.float64).reshape(-1, 4) for g in gt]
        for k, ks in enumerate(keeps):
            self.count_face[k] += sum(int(x.size) for x in ks)

        def on_device(r):
            if torch.is_tensor(r):
                return r.detach().to(device=dev, dtype=torch.float64).reshape(-1, 5)
            return torch.from_numpy(np.ascontiguousarray(np.asarray(r, dtype=np.float64).reshape(-1, 5))).to(dev)

        if rows and not any(torch.is_tensor(r) for r in rows):           # host arrays: one upload
            lens = [int(np.asarray(r).reshape(-1, 5).shape[0]) for r in rows]
            every = on_device(np.concatenate([np.asarray(r, dtype=np.float64).reshape(-1, 5) for r in rows])) if sum(lens) else None
            parts = list(torch.split(every, lens)) if every is not None else [torch.zeros(0, 5, dtype=torch.float64, device=dev)] * len(rows)
        else:
            parts = [on_device(r) for r in rows]
        if sum(int(p.shape[0]) for p in parts) == 0:
            return
        # norm_scores: every score of the prediction set, the images that are skipped below included
        lo, hi = torch.aminmax(torch.cat([p[:, 4] for p in parts]))
        self._lo = lo if self._lo is None else torch.minimum(self._lo, lo)
        self._hi = hi if self._hi is None else torch.maximum(self._hi, hi)
        # evaluate_setting: an image without boxes or without rows adds nothing to the table
        live = [i for i in range(len(gts)) if gts[i].shape[0] and parts[i].shape[0]]
        if not live:
            return
        lens = [int(parts[i].shape[0]) for i in live]
        glens = [int(gts[i].shape[0]) for i in live]
        doffs, goffs = np.concatenate([[0], np.cumsum(lens)]), np.concatenate([[0], np.cumsum(glens)])
        n, g = int(doffs[-1]), int(goffs[-1])
        cat = torch.cat([parts[i] for i in live])
        # read_predictions: a stable descending sort by score inside every image = a stable sort of everything by score, then a stable
        # sort by segment (the segments lie back to back, so the second sort only gathers them again); no length is read from the device
        seg = torch.repeat_interleave(torch.from_numpy(np.asarray(lens, dtype=np.int64)).to(dev), output_size=n)
        by_score = torch.sort(cat[:, 4], descending=True, stable=True).indices
        order = by_score[torch.sort(seg[by_score], stable=True).indices]
        cat = cat[order].contiguous()
        masks = np.zeros((len(self.settings), g), dtype=np.uint8)
        for k, ks in enumerate(keeps):
            for j, i in enumerate(live):
                masks[k, goffs[j]:goffs[j + 1]][ks[i]] = 1                  # (a view of the image's boxes: evaluate_setting's mask[keep] = True)
        counted, recalled = ops.wider_match_batched(cat, doffs.tolist(), torch.from_numpy(np.concatenate([gts[i] for i in live])).to(dev),
                                                    goffs.tolist(), torch.from_numpy(masks).to(dev), self.iou_thresh)
        self._scores.append(cat[:, 4].contiguous())
        self._counted.append(counted)
        self._recalled.append(recalled)
        self._offsets += [self._offsets[-1] + int(o) for o in doffs[1:]]

    def finish(self):
        """{setting: (AP, pr_curve (T,2))}: norm_scores' (lo, d) on the device, one tf_wider_pr_accumulate call over everything that was
        added, one host read of the table, then evaluate_setting's own lines (precision_recall_ap)."""
        import torch
        from . import ops
        T, nset = self.thresh_num, len(self.settings)
        pr = torch.zeros(nset, T, 2, dtype=torch.int64, device=self.device)
        if self._scores:
            d = torch.where(self._hi > self._lo, self._hi - self._lo, torch.ones_like(self._lo))
            thresh = torch.tensor([1 - (t + 1) / T for t in range(T)], dtype=torch.float64).to(self.device)       # image_pr_info's expression
            ops.wider_pr_accumulate(torch.cat(self._scores), self._offsets, torch.cat(self._counted, dim=1), torch.cat(self._recalled, dim=1),
                                    torch.stack([self._lo, d]), thresh, pr)
        table = pr.cpu().numpy().astype(np.float64)                        # the one host read; counts far below 2^53: exact
        return {s: precision_recall_ap(table[k], self.count_face[k]) for k, s in enumerate(self.settings)}


def read_predictions(pred_dir):
    """The tree write_results creates: <pred_dir>/<event>/<image>.txt = name, count, then `x y w h score` rows."""
    preds = {}
    for event in sorted(os.listdir(pred_dir)):
        ed = os.path.join(pred_dir, event)
        if not os.path.isdir(ed):
            continue
        preds[event] = {}
        for fn in sorted(os.listdir(ed)):
            if not fn.endswith(".txt"):
                continue
            lines = open(os.path.join(ed, fn)).read().split("\n")
            n = int(lines[1]) if len(lines) > 1 and lines[1].strip() else 0
            rows = np.array([[float(v) for v in l.split()[:5]] for l in lines[2:2 + n] if l.strip()], dtype=np.float64).reshape(-1, 5)
            order = np.argsort(-rows[:, 4], kind="stable")
            preds[event][fn[:-4]] = rows[order]
    return preds


def load_ground_truth(gt_dir, setting):
    """wider_face_val.mat (face_bbx_list, event_list, file_list) + wider_<setting>_val.mat (gt_list, 1-based indices)."""
    from scipy.io import loadmat
    base = loadmat(os.path.join(gt_dir, "wider_face_val.mat"))
    sub = loadmat(os.path.join(gt_dir, f"wider_{setting}_val.mat"))
    gt_boxes, keep = {}, {}
    for i in range(len(base["event_list"])):
        event = str(base["event_list"][i][0][0])
        gt_boxes[event], keep[event] = {}, {}
        files, boxes, kl = base["file_list"][i][0], base["face_bbx_list"][i][0], sub["gt_list"][i][0]
        for j in range(len(files)):
            name = str(files[j][0][0])
            gt_boxes[event][name] = np.asarray(boxes[j][0], dtype=np.float64).reshape(-1, 4)
            keep[event][name] = np.asarray(kl[j][0], dtype=np.int64).reshape(-1) - 1
    return gt_boxes, keep


def evaluate(pred_dir, gt_dir, settings=("easy", "medium", "hard"), iou_thresh=0.5):
    """AP per setting for a directory of result files against the WIDER val ground truth."""
    preds = norm_scores(read_predictions(pred_dir))
    return {s: evaluate_setting(preds, *load_ground_truth(gt_dir, s), iou_thresh=iou_thresh)[0] for s in settings}


if __name__ == "__main__":      # python -m tinyfaces.wider_eval <results dir> <eval_tools/ground_truth dir>   (replaces `make evaluate`'s MATLAB step)
    import sys
    for setting, ap in evaluate(sys.argv[1], sys.argv[2]).items():
        print(f"{setting:7s} AP = {ap:.4f}")
