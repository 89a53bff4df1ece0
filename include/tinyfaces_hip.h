/* tinyfaces_hip.h -- C ABI of libtinyfaces_hip.so (gfx950 / MI355X).
 *
 * The reference (varunagrawal/tiny-faces-pytorch) has no FFI of its own: its hot path is
 * Python calling torch / torchvision / numpy.  Each entry point below replaces the
 * framework call(s) cited next to it (reference file:line, relative to /root/reference).
 * The Python package tiny-faces-pytorch_amd/tinyfaces binds them with ctypes
 * (tinyfaces/_hip.py) -- see INTEGRATION.md for the stub a maintainer would add.
 *
 * Conventions
 *   - plain pointers + sizes only; every pointer is a DEVICE pointer unless named host_*;
 *   - the caller owns all memory; kernels never allocate or free; scratch is passed in
 *     (`ws`, sized by the matching *_workspace_bytes());
 *   - everything is enqueued on `stream` (a hipStream_t passed as void*), no host sync
 *     unless stated; stateless and therefore thread-safe per stream;
 *   - return 0 (TF_OK) or a negative TF_ERR_* code; no exceptions cross the boundary.
 *   - activations of the network kernels are NHWC ("pixels x channels" matrices), dtype
 *     TF_F32, TF_BF16 or (inference) TF_F16; maps handed to / from the reference call surface are NCHW float32.
 */
#ifndef TINYFACES_HIP_H
#define TINYFACES_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TF_OK 0
#define TF_ERR_ARG (-1)
#define TF_ERR_LAUNCH (-2)
#define TF_ERR_UNSUPPORTED (-3)
#define TF_ERR_WORKSPACE (-4)

#define TF_F32 0
#define TF_BF16 1
#define TF_F16 2      /* IEEE half operands, fp32 accumulation: inference only (BASELINE.json configs[4]); the training entry points refuse it */

int tf_version(void);
/* r6: digest (16 hex digits of a sha256) of the sources and compiler flags the library was built from; profiles/ files are stamped with it */
const char* tf_build_id(void);
/* number of exported symbols a binding must resolve; names via tf_symbol_name(i) */
int tf_symbol_count(void);
const char* tf_symbol_name(int i);

/* ---- dense_overlap + heat-map target assignment ------------------------------------
 * Replaces compute_dense_overlap (tinyfaces/datasets/dense_overlap.py:4-75) fused with
 * DataProcessor.get_padding / get_regression / get_heatmaps
 * (tinyfaces/datasets/processor.py:114-277).  float64 arithmetic, IoU rounded to 14
 * decimals exactly like the reference; the 63x63x25xG IoU tensor is never materialised.
 *   boxes        [total][4] f64 (x1,y1,x2,y2), degenerate boxes already removed
 *                (processor.py:228-232 is done by the host wrapper)
 *   box_offsets  [B+1] i32   image b owns boxes [box_offsets[b], box_offsets[b+1])
 *   templates    [nt][tstride] f64 (x1,y1,x2,y2,...)
 *   paste_boxes  [B][4] i32 (x1,y1,x2,y2) or NULL (= whole image, no padding)
 *   flips        [B] i32 or NULL: pad mask mirrored in x (tinyfaces/datasets/wider_face.py:165)
 *   noise        f64 uniform[0,1) tie-break draws of processor.py:195, per image laid out
 *                (y,x,t,g) at element offset noise_offsets[b]; NULL -> counter RNG(seed)
 *   class_map    [B][nt][vsy][vsx] f32 in {-1,0,1};  reg_map [B][4nt][vsy][vsx] f32
 */
size_t tf_targets_workspace_bytes(int total_boxes);
int tf_dense_overlap_targets(const double* boxes, const int32_t* box_offsets, int B,
                             const double* templates, int nt, int tstride,
                             int vsy, int vsx, int ofy, int ofx, int sty, int stx,
                             const int32_t* paste_boxes, const int32_t* flips,
                             const double* noise, const int64_t* noise_offsets, uint64_t seed,
                             double pos_thresh, double neg_thresh,
                             float* class_map, float* reg_map,
                             void* ws, size_t ws_bytes, void* stream);
/* ---- scale-compensated anchor matching (S3FD, Zhang et al. 2017): top-N positives per face ----------------------------
 * tf_dense_overlap_targets_comp is tf_dense_overlap_targets followed by an optional second stage that tops every face up to N
 * positive anchors.  The reference has no such stage; the rule below is the contract.  All symbols are per image.
 *   v[a, g]   the perturbed IoU the first stage forms: iou14 + 1e-6 * noise
 *   own(a)    the first arg-max over g of v[a, g];  best(a) = v[a, own(a)]
 *   pad(a)    the padding predicate of the first stage (paste_boxes / flips)
 *   F         the class map exactly as the first stage leaves it
 *   1. count(g) = number of anchors with F = 1 and own(a) = g.  A face's forced best anchor counts for the face that OWNS it,
 *      not for the face that forced it.
 *   2. if count(g) < N, the candidates of g are the anchors with own(a) = g, !pad(a), F(a) != 1 and best(a) >= T.
 *   3. the N - count(g) best candidates get F = 1: larger best first, on a tie the lower reference flat index (y * vsx + x) * nt + t.
 *   4. if fewer candidates exist, all of them are promoted.
 *   5. nothing else changes.
 * Consequences: reg_map is bit for bit the map of the uncompensated call (an owned anchor already carries its owner's offsets, an
 * unpadded anchor never had tx zeroed); every anchor has one owner, so two faces never claim the same anchor; one image's result does
 * not depend on the rest of its batch.  Integer atomics only, no grid barrier, no host synchronisation: the same bits on every run
 * (explicit noise, or the same seed).
 *   N            1..64
 *   T            finite, 0.01 <= T < pos_thresh; may lie below neg_thresh (the stage then promotes negatives as well as ignored anchors)
 *   match_count  [total_boxes] i32 or NULL: the final number of positives each face owns, count(g) + its promotions
 *   ws           sized by tf_targets_comp_workspace_bytes(total_boxes, B, nt, vsy, vsx); sty, stx > 0
 * Refused before anything is enqueued: N or T out of range (TF_ERR_ARG), a workspace below the size for one box (TF_ERR_WORKSPACE).
 * The number of boxes is only known on the device: if box_offsets[B] exceeds the slots the workspace holds, every kernel of the call
 * returns without writing anything. */
size_t tf_targets_comp_workspace_bytes(int total_boxes, int B, int nt, int vsy, int vsx);
int tf_dense_overlap_targets_comp(const double* boxes, const int32_t* box_offsets, int B,
                                  const double* templates, int nt, int tstride,
                                  int vsy, int vsx, int ofy, int ofx, int sty, int stx,
                                  const int32_t* paste_boxes, const int32_t* flips,
                                  const double* noise, const int64_t* noise_offsets, uint64_t seed,
                                  double pos_thresh, double neg_thresh,
                                  int N, double T, int32_t* match_count,
                                  float* class_map, float* reg_map,
                                  void* ws, size_t ws_bytes, void* stream);
/* ---- ignore regions of the training targets (S3FD / PyramidBox / RetinaFace pipelines; mmdetection's gt_bboxes_ignore) ----------
 * tf_targets_apply_ignore is one pass over the class map tf_dense_overlap_targets[_comp] left, in place: a negative anchor that an
 * ignore box of its image covers gets the don't-care label 0, which both criteria skip.  The reference has no such pass; the rule
 * below is the contract.  Image b has the ignore boxes r_0 .. r_{K-1} = rows [ign_offsets[b], ign_offsets[b + 1]) of ign_boxes
 * (x1, y1, x2, y2, float64, in the augmented frame, already mirrored where the image is).  Anchor a = template t at cell (y, x):
 *   cx = ofx + x * stx, cy = ofy + y * sty;  ax1 = dx1 + cx, ay1 = dy1 + cy, ax2 = dx2 + cx, ay2 = dy2 + cy   (tf_dense_overlap_targets' anchor)
 *   farea = (dx2 - dx1 + 1) * (dy2 - dy1 + 1);  rarea = (rx2 - rx1 + 1) * (ry2 - ry1 + 1)
 *   iw = min(ax2, rx2) - max(ax1, rx1) + 1,  ih = min(ay2, ry2) - max(ay1, ry1) + 1                            (the +1 pixel convention)
 *   if iw > 0 and ih > 0:  ia = iw * ih and
 *        TF_IGNORE_IOF   ov = ia / farea                     (intersection over the ANCHOR's area: mmdetection's ignore_wrt_candidates)
 *        TF_IGNORE_IOU   ov = ia / (farea + rarea - ia)
 *   else ov = 0.
 *   No rounding to 14 decimals, no noise; plain float64 in this operation order, without FMA contraction.
 *   a is covered when ov >= thresh for ANY k (order-free in k).  thresh finite, in (0, 1].
 *   A covered anchor whose label is -1 becomes 0.  Labels +1 and 0 are never changed: a real face keeps its positives inside an
 *   ignore region.  Nothing else is written; the regression map is not an operand.
 * Consequences: the pass runs behind everything else (phase C, and the compensation stage when that is on), so it composes with
 * either call; one image's result does not depend on the rest of its batch.
 *   class_map     [B][nt][vsy][vsx] f32, in place
 *   ign_boxes     [total][4] f64; NULL = no ignore box in the batch: TF_OK, nothing is enqueued
 *   ign_offsets   [B + 1] i32 on the device, ascending from 0
 *   changed       [B] i32 or NULL: the number of labels turned is ADDED per image (integer atomics, one per wave that turned any);
 *                 the caller zeroes it.  NULL: nothing is counted.
 * One launch; no floating-point atomics, no grid barrier, no workspace, no host synchronisation: the same bits on every run.
 * Refused before anything is enqueued (TF_ERR_ARG): thresh outside (0, 1] or not finite, an unknown measure, a negative size,
 * tstride < 4, a NULL class_map / templates / ign_offsets next to ign_boxes.  B > 65535 or nt * vsy * vsx >= 2^31: TF_ERR_UNSUPPORTED. */
#define TF_IGNORE_IOF 0
#define TF_IGNORE_IOU 1
int tf_targets_apply_ignore(float* class_map, int B, int nt, int vsy, int vsx,
                            const double* templates, int tstride,
                            int ofy, int ofx, int sty, int stx,
                            const double* ign_boxes, const int32_t* ign_offsets,
                            int measure, double thresh, int32_t* changed, void* stream);
/* ---- ATSS target assignment (Zhang et al. 2020, "Bridging the Gap Between Anchor-based and Anchor-free Detection"; mmdetection's
 * ATSSAssigner; what SCRFD and TinaFace train with) ---------------------------------------------------------------------------------
 * tf_targets_atss is an assigner of its own next to tf_dense_overlap_targets: the same operands and the same two maps in the same layout,
 * no fixed thresholds.  The reference has no such assigner; the rule below is the contract (numpy restatement: tests/atss_ref.py).
 * All symbols are per image.  Faces g = 0 .. G-1 = rows [box_offsets[b], box_offsets[b + 1]) of boxes (degenerate ones removed by the
 * caller, input order).  Anchor a = template t at cell (y, x), exactly tf_dense_overlap_targets' anchor:
 *   cx = ofx + x * stx, cy = ofy + y * sty;  ax1 = dx1 + cx, ay1 = dy1 + cy, ax2 = dx2 + cx, ay2 = dy2 + cy
 *   anchor centre acx = (ax1 + ax2) / 2, acy = (ay1 + ay2) / 2;  pad(a) = get_padding's predicate (paste_boxes, mirrored in x where flips says so)
 * Plain float64 in the stated operation order, without FMA contraction; no rounding to 14 decimals, no noise, no RNG: the result is a pure
 * function of boxes, templates, geometry and k.
 *   1 candidates  for face g and template t: the k unpadded cells of t nearest to the face centre fcx = (fx1 + fx2) / 2, fcy = (fy1 + fy2) / 2,
 *                 by (acx - fcx)^2 + (acy - fcy)^2 ascending, the lower cell index y * vsx + x first on a tie; a template with fewer than k
 *                 unpadded cells contributes all of them.  k in 1..16.  The face's list: t ascending, then that rank; length n <= k * nt.
 *   2 IoU         v of each candidate with the face in dense_overlap's operation order (+1 pixel convention, 0 unless iw > 0 and ih > 0), unrounded.
 *   3 threshold   mean = (v_0 + v_1 + ... + v_{n-1}) / n, summed serially in list order; var = sum (v_i - mean)^2 / (n - 1) in the same order
 *                 (unbiased, torch.std's form), 0 when n = 1.  A candidate passes when d = v - mean >= 0 and d * d >= var: v >= mean + std
 *                 without a square root.
 *   4 positives   a passing candidate whose anchor centre lies strictly inside the face (fx1 < acx < fx2 and fy1 < acy < fy2) is a claim of g.
 *   5 fallback    a face with candidates but no claim claims its single best candidate (largest v, the earlier list position on a tie), even
 *                 when v is 0 or the centre lies outside: the counterpart of the reference's forced best anchor.  n = 0 claims nothing.
 *   6 conflicts   an anchor claimed by several faces goes to the larger v, the lower g on a tie; the losers are not compensated.
 *   7 output      class_map = +1 at every won claim, -1 everywhere else, padded anchors included (no grey band; tf_targets_apply_ignore
 *                 behind this call, with the faces as ignore boxes, makes one).  reg_map = get_regression's four values of the winning face
 *                 ((fcx - cx) / dw, (fcy - cy) / dh, log(fw / dw), log(fh / dh); f64, stored as f32) at every +1 anchor, exactly 0.f
 *                 everywhere else.  Every element of both maps is written; they may arrive holding garbage.
 *                 match_count [total_boxes] i32 or NULL: the number of anchors each face won.
 *   8 one image's result does not depend on the rest of its batch.
 * Four launches (fill, claim, owner, write); conflicts are resolved with 64- and 32-bit integer atomics only (max of the IoU's bit pattern,
 * then min of the face index), so the bits are the same on every run; no grid barrier, no host synchronisation.  The claims of a face are
 * kept in the workspace, not recomputed.  The number of boxes is only known on the device: a workspace too small for box_offsets[B] makes
 * every kernel return without writing.
 * Refused before anything is enqueued: k outside 1..16, a NULL class_map / reg_map / templates / box_offsets, a non-positive size,
 * tstride < 4, a stride <= 0 (TF_ERR_ARG); a workspace below the size for one box (TF_ERR_WORKSPACE); nt * vsy * vsx >= 2^31 or a cell
 * coordinate beyond int32 (TF_ERR_UNSUPPORTED). */
size_t tf_targets_atss_workspace_bytes(int total_boxes, int B, int nt, int vsy, int vsx);
int tf_targets_atss(const double* boxes, const int32_t* box_offsets, int B,
                    const double* templates, int nt, int tstride,
                    int vsy, int vsx, int ofy, int ofx, int sty, int stx,
                    const int32_t* paste_boxes, const int32_t* flips,
                    int k, int32_t* match_count,
                    float* class_map, float* reg_map,
                    void* ws, size_t ws_bytes, void* stream);
/* ---- TAL: task-aligned target assignment (Feng et al. 2021, "TOOD: Task-aligned One-stage Object Detection"; mmdetection's
 * TaskAlignedAssigner, defaults topk = 13, alpha = 1, beta = 6) ------------------------------------------------------------------------
 * tf_targets_tal assigns from the network's own output: an anchor is positive for a face when the head already scores it highly AND its
 * predicted box localises that face well.  It runs between the forward pass and the criterion, IN PLACE on two maps that arrive holding an
 * assignment without faces (the base maps: tf_dense_overlap_targets with no box -- every label -1, padded anchors too, as after
 * tf_targets_atss --, then 0 where tf_targets_apply_ignore turned a negative; regression map 0); the reference has no such assigner, the rule
 * below is the contract (numpy restatement: tests/tal_ref.py).
 * Symbols, faces, anchors, acx / acy and pad(a) are those of ATSS above.  output [B][5 nt][vsy][vsx] f32 is the head's output in the layout the
 * criterion reads: channel t the class logit z of template t, channels nt + t, 2 nt + t, 3 nt + t, 4 nt + t its px, py, pw, ph.  Every operand is
 * widened to float64 first; plain float64 in the stated operation order, without FMA contraction; exp and pow are the math library's.
 *   1 metric      dw = dx2 - dx1 + 1, dh = dy2 - dy1 + 1 (the regression target's own normalisers), C = 4.135166556742356 (log(1000 / 16), the
 *                 clamp of the overlap losses).  The predicted box of anchor a: centre bcx = cx + px * dw, bcy = cy + py * dh, size
 *                 w = dw * exp(min(max(pw, -C), C)), h = dh * exp(min(max(ph, -C), C)), corners bcx -+ w / 2, bcy -+ h / 2.  The face as the
 *                 target kernel measures it: centre fcx = (fx1 + fx2) / 2, fcy = (fy1 + fy2) / 2, size bw = fx2 - fx1 + 1, bh = fy2 - fy1 + 1,
 *                 corners fcx -+ bw / 2, fcy -+ bh / 2.  iw = min(right edges) - max(left edges), ih alike (no + 1: both boxes are continuous);
 *                 u = iw * ih / (w * h + bw * bh - iw * ih) when iw > 0 and ih > 0, else 0.  No epsilon.  A prediction equal to the anchor's
 *                 regression target for g has u = 1.  s = 1 / (1 + exp(-z));  m = pow(s, alpha) * pow(u, beta).
 *   2 candidates  of face g: every template at every unpadded cell whose anchor centre lies strictly inside the face (fx1 < acx < fx2 and
 *                 fy1 < acy < fy2).  A face for which no template has such a cell (a 6-px face between the centres of the stride-8 grid) takes, per
 *                 template, the single unpadded cell nearest its centre: ATSS's candidate at k = 1, in its distance and tie order.  Of these,
 *                 one whose z, px, py, pw or ph is not finite, whose u is not > 0, or whose m is not finite is not a candidate.
 *   3 selection   the face claims its topk candidates of largest m, the lower flat index (t * vsy + y) * vsx + x first on a tie; fewer if
 *                 it has fewer.  topk in 1..32; alpha finite and >= 0; beta finite and > 0.
 *   4 conflicts   an anchor claimed by several faces goes to the larger u, the lower g on a tie (ATSS's rule with the predicted box's IoU); the
 *                 losers are not compensated.  There is no fallback: a face whose candidates all have u = 0 wins nothing.
 *   5 output      class_map = +1 and reg_map = get_regression's four values of the winning face (as ATSS writes them) at every won anchor, even
 *                 where the map held 0.  NOTHING else of either map is written: what arrived stays.  match_count [total_boxes] i32 or NULL:
 *                 the number of anchors each face won.
 *   6 one image's result does not depend on the rest of its batch; the same operands give the same bits on every run.
 * Four launches (clear of the workspace's claim words, claim, owner, write).  claim: one 256-thread workgroup per face walks the face's window
 * in tiles of 256 candidates and keeps its running topk in LDS (per-tile partial top-k, merged by counting ranks); neither the number of
 * faces, nor a window's size, nor nt is bounded by LDS, and no candidate list exists in global memory.  Conflicts are resolved with 64- and
 * 32-bit integer atomics only (max of u's bit pattern, then min of the face index); no floating-point atomic, no grid barrier, no host
 * synchronisation, no memset of the maps.  The number of boxes is only known on the device: a workspace too small for box_offsets[B] makes
 * every kernel return without writing.
 * Refused before anything is enqueued: topk outside 1..32, alpha not finite or < 0, beta not finite or <= 0, a NULL output / class_map /
 * reg_map / templates / box_offsets, a non-positive size, tstride < 4, a stride <= 0 (TF_ERR_ARG); a workspace below the size for one box
 * (TF_ERR_WORKSPACE); nt * vsy * vsx >= 2^31 or a cell coordinate beyond int32 (TF_ERR_UNSUPPORTED). */
size_t tf_targets_tal_workspace_bytes(int total_boxes, int B, int nt, int vsy, int vsx);
int tf_targets_tal(const float* output, const double* boxes, const int32_t* box_offsets, int B,
                   const double* templates, int nt, int tstride,
                   int vsy, int vsx, int ofy, int ofx, int sty, int stx,
                   const int32_t* paste_boxes, const int32_t* flips,
                   int topk, double alpha, double beta, int32_t* match_count,
                   float* class_map, float* reg_map,
                   void* ws, size_t ws_bytes, void* stream);
/* ---- TAL, step 7: the normalised alignment of every won anchor (TOOD's target of the classification loss and weight of the box loss) ----
 * tf_targets_tal_aligned is tf_targets_tal -- the same operands, the same rule, the same bits in class_map, reg_map and match_count -- and
 * one more output, align_map [B][nt][vsy][vsx] f32:
 *   7 alignment   after step 4 let W_g be the anchors face g WON (not the anchors it claimed: a claim lost in a conflict does not count).  For a
 *                 non-empty W_g:  M_g = max of m over W_g,  U_g = max of u over W_g  (comparisons: exact given the operands), with m and u the
 *                 very float64 values steps 1-4 ranked and resolved by.  For a in W_g
 *                     t(a) = (m_a / M_g) * U_g      float64, the division first, then the product, without contraction;
 *                     t(a) = 0                      when M_g == 0 (every winner's sigmoid underflowed: logits of -1e4 with alpha = 1);
 *                 align_map(a) = (float)t(a).  Every OTHER element of align_map is 1.0f: the map is written completely by every call, is never
 *                 memset and may arrive holding anything (NaN included); an anchor whose +1 label is not this call's keeps the hard target 1.
 *                 The face's best winner gets exactly (float)U_g, and 0 <= t <= U_g <= 1.
 *                 NO epsilon.  mmdetection's TaskAlignedAssigner divides by (M_g + 1e-7).  At zero output a 6-px face lies inside the smallest
 *                 of the 25 anchors (20.3 x 22.2 px): u = 36 / 452 = 0.080 and m = 0.5 * 0.080^6 = 1.3e-7, so that epsilon would cut every target
 *                 of the face to 0.56 of U_g, and to a fifth for a face whose best u is 0.06 (m = 2e-8): the faces this detector exists for
 *                 would be trained towards scores that are too low by such a factor at the start of training.  This project adds no epsilon
 *                 anywhere; M_g == 0 is the one case a quotient is undefined in, and it is defined above.
 * The same four launches: the clear also stores the 1.0f of every anchor, claim keeps every winner's m (its bits, not a value formed again)
 * next to its key in the workspace, and write -- one wave per face -- reduces M_g and U_g over the lanes that won by wave shuffles and stores
 * t beside the +1.  No further atomics, no fifth launch, no floating-point atomic, no grid barrier, no host synchronisation; the same bits on
 * every run.  The workspace is 8 bytes per winner slot larger (tf_targets_tal_aligned_workspace_bytes); as in tf_targets_tal, a workspace too
 * small for box_offsets[B] makes every kernel return without writing, align_map included.
 * Refused before anything is enqueued: what tf_targets_tal refuses, and a NULL align_map (TF_ERR_ARG). */
size_t tf_targets_tal_aligned_workspace_bytes(int total_boxes, int B, int nt, int vsy, int vsx);
int tf_targets_tal_aligned(const float* output, const double* boxes, const int32_t* box_offsets, int B,
                           const double* templates, int nt, int tstride,
                           int vsy, int vsx, int ofy, int ofx, int sty, int stx,
                           const int32_t* paste_boxes, const int32_t* flips,
                           int topk, double alpha, double beta, int32_t* match_count,
                           float* class_map, float* reg_map, float* align_map /*[B][nt][vsy][vsx]*/,
                           void* ws, size_t ws_bytes, void* stream);
/* test hook: the raw rounded IoU tensor [vsy][vsx][nt][G] f64 for ONE image */
int tf_dense_overlap_iou(const double* boxes, int G, const double* templates, int nt, int tstride,
                         int vsy, int vsx, int ofy, int ofx, int sty, int stx,
                         double* iou_out, void* stream);

/* ---- template clustering: distance matrix of the k-medoids ------------------------------
 * Replaces compute_distances (tinyfaces/clustering/cluster.py:28-37, a Python double loop over jaccard_index,
 * tinyfaces/metrics.py:8-40): out[i][j] = 1 - IoU(boxes[i], boxes[j]) in float64, plain areas, IoU = 0 when the union is not
 * positive; bit-exact with the reference's arithmetic.  boxes [n][4] (x1,y1,x2,y2), out [n][n]. */
int tf_pairwise_iou_distance(const double* boxes, int n, double* out, void* stream);

/* ---- greedy NMS, float64 -----------------------------------------------------------
 * Replaces torchvision.ops.nms as called at tinyfaces/evaluation.py:84 (float64 boxes and
 * scores): stable descending sort, areas without +1, strict `>` on IoU.  keep_out holds the
 * surviving INPUT indices in descending-score order; *num_keep (device int32) their count.
 * Score order: the one torch.sort(scores, descending, stable) hands the reference's kernel, for ANY float64 scores: a NaN ranks above
 * every number, +inf included, and NaNs among themselves by input index; -0.0 == +0.0; equal scores keep input order.  The order is a
 * permutation of 0..n-1 whatever the scores: every element of the workspace's order / sorted-box arrays in [0, n) is written on every
 * call, and keep_out holds each input index at most once.  Box coordinates must be finite (the reference's std::max, fmax and
 * numpy's maximum each treat a NaN operand differently).  Any iou_thresh is accepted as given: a pair suppresses iff IoU > iou_thresh
 * (strict), so a negative threshold suppresses disjoint boxes too (their IoU is 0), one >= 1 suppresses nothing, exact duplicates
 * included (IoU 1), and a NaN IoU (0 / 0: two zero-area boxes) never suppresses.  -0.0 is 0.0. */
size_t tf_nms_workspace_bytes(int n);
int tf_nms_f64(const double* boxes /*[n][4]*/, const double* scores /*[n]*/, int n, double iou_thresh,
               int64_t* keep_out /*[n]*/, int32_t* num_keep, void* ws, size_t ws_bytes, void* stream);
/* Batched multi-scale form (BASELINE.json configs[4]): S <= TF_NMS_MAX_SEGMENTS independent candidate lists -- the multi-scale
 * candidates of each image of an evaluation batch (the reference runs evaluation.py:80-84 once per image), or one list per pyramid
 * level -- laid out back to back; segment s = rows [host_seg_offsets[s], host_seg_offsets[s+1]) (HOST int32 array, [0] == 0).
 * One NMS per segment with the semantics of tf_nms_f64, all of them in the same three launches.  The survivors of segment s are
 * written to keep_out[host_seg_offsets[s] ...] as indices into the CONCATENATED input (descending score inside the segment),
 * num_keep[s] (device) their count.  Largest segment <= 524 160 boxes.  ws: tf_nms_batched_workspace_bytes(). */
#define TF_NMS_MAX_SEGMENTS 64
size_t tf_nms_batched_workspace_bytes(const int32_t* host_seg_offsets, int num_segments);
int tf_nms_f64_batched(const double* boxes /*[n][4]*/, const double* scores /*[n]*/, const int32_t* host_seg_offsets /*[S+1]*/,
                       int num_segments, double iou_thresh, int64_t* keep_out /*[n]*/, int32_t* num_keep /*[S]*/,
                       void* ws, size_t ws_bytes, void* stream);

/* ---- test-time augmentation: box voting and the un-mirroring of a flipped pyramid level, float64 ----------------
 * Additions to the reference's evaluation (tinyfaces/evaluation.py:80-87 keeps the NMS survivors as they are): the two test-time
 * steps WIDER FACE results are usually reported with.
 *
 * Box voting (Gidaris & Komodakis, ICCV 2015; Detectron's box_voting with scoring method ID): for segment s and r < num_keep[s],
 * with k = keep[off[s] + r] (an index into the concatenated input),
 *     V = { j in [off[s], off[s+1]) : IoU(box_k, box_j) >= vote_thresh }     (`>=`, Detectron's; the NMS suppresses on `>`)
 *     out[off[s] + r] = (sum_V w_j * box_j / sum_V w_j, score_k)             (the kept box's own score is carried through)
 * The IoU is tf_nms_f64's expression in the same operation order (areas without +1, inter / (a_k + a_j - inter)), so membership
 * is decided by the very bits the NMS compared; a NaN IoU (0 / 0: a zero-area box) is not a vote.  Voters whose weight is <= 0 or
 * NaN are dropped; with no voter left, or a weight sum that is not > 0, the row is (box_k, score_k) unchanged.
 * votes_out[off[s] + r] (optional) = the number of voters after the weight filter.  Rows r >= num_keep[s] of out / votes_out are
 * NOT written.  keep / num_keep are tf_nms_f64_batched's keep_out / num_keep as it left them, in DEVICE memory: the call chains
 * behind the NMS on the same stream with no host synchronisation.  The sums are taken in a fixed order without atomics: the same
 * bits on every run.  Nothing is launched for n == 0; S outside 1..TF_NMS_MAX_SEGMENTS, descending offsets, an unknown weight_mode
 * or a vote_thresh outside (0, 1] are TF_ERR_ARG. */
#define TF_VOTE_WEIGHT_SIGMOID 0   /* w = 1 / (1 + exp(-score)): the scores tf_decode_compact emits are LOGITS (tinyfaces/models/utils.py:37) */
#define TF_VOTE_WEIGHT_SCORE   1   /* w = score as given (a caller that holds probabilities) */
int tf_box_vote_f64_batched(const double* boxes /*[n][4]*/, const double* scores /*[n]*/, const int32_t* host_seg_offsets /*[S+1]*/,
                            int num_segments, const int64_t* keep /*device [n]*/, const int32_t* num_keep /*device [S]*/,
                            double vote_thresh, int weight_mode, double* out /*[n][5]*/, int32_t* votes_out /*[n] or NULL*/, void* stream);
/* one segment: the batched form with S = 1, as tf_nms_f64 is of tf_nms_f64_batched */
int tf_box_vote_f64(const double* boxes /*[n][4]*/, const double* scores /*[n]*/, int n, const int64_t* keep /*device [n]*/,
                    const int32_t* num_keep /*device [1]*/, double vote_thresh, int weight_mode, double* out /*[n][5]*/,
                    int32_t* votes_out /*[n] or NULL*/, void* stream);
/* Rows [*first, *last) of a tf_decode_compact candidate list (first / last: DEVICE int32, copies of its counter taken before and after a
 * MIRRORED pyramid level) are mirrored back: x1' = c - x2, x2' = c - x1, both read before either is written; y1, y2 and the score
 * stay, rows outside the range are not written.  c = (W_level - 1) * (1 / scale) is the caller's.  max_rows: a host bound on
 * *last - *first that sizes the grid (rows beyond it are left alone); 0 launches nothing, < 0 is TF_ERR_ARG. */
int tf_boxes_unflip_f64(double* dets /*[cap][5]*/, const int32_t* first, const int32_t* last, int max_rows, double c, void* stream);

/* ---- Soft-NMS, float64 (Bodla et al., ICCV 2017, "Improving object detection with one line of code"; Detectron's soft_nms) ----------
 * An addition next to tf_nms_f64: a candidate that overlaps a better one is not dropped; its score is decayed, the list is re-ranked,
 * and it survives unless its score falls under score_thresh.  Per segment (batching as tf_nms_f64_batched: S <= TF_NMS_MAX_SEGMENTS
 * segments described by a HOST offset table, side by side in the same two launches):
 *   1. s_j = 1 / (1 + exp(-scores[j])) with score_mode TF_VOTE_WEIGHT_SIGMOID (tf_decode_compact emits logits; the vote's expression),
 *      s_j = scores[j] with TF_VOTE_WEIGHT_SCORE.  Candidate j is live iff s_j >= score_thresh; a NaN is never live.
 *   2. While a candidate is live: m = the live candidate with the largest s, the LOWEST input index on a bit-equal tie;
 *      keep_out[off + r] = m (an index into the CONCATENATED input), score_out[off + r] = s_m, ++r; m is no longer live.
 *   3. Every j still live is decayed: ovr = tf_nms_f64's IoU in the same operation order (areas without +1,
 *      inter / (a_m + a_j - inter); the file is compiled without FMA contraction, so these are the very bits the hard NMS compares).
 *      inter == 0 or a NaN ovr: s_j unchanged.  TF_SOFT_NMS_LINEAR: if ovr > iou_thresh (strict, as the hard NMS) s_j = s_j * (1 - ovr).
 *      TF_SOFT_NMS_GAUSSIAN: if ovr > 0, s_j = s_j * exp(-(ovr * ovr) / sigma) (iou_thresh is ignored).  Then j stays live iff
 *      s_j >= score_thresh.
 *   4. num_keep[s] = r.  Every factor is <= 1: the emitted scores never increase.  They are decayed PROBABILITIES (not logits).
 * Rows r >= num_keep[s] of keep_out / score_out are NOT written, nothing outside [off[s], off[s] + num_keep[s]) is.  No atomics: the same
 * bits on every run.  An unknown method or score mode, sigma that is not > 0, iou_thresh outside [0, 1], a negative or NaN score_thresh and
 * bad segment tables (S outside 1..TF_NMS_MAX_SEGMENTS, offsets that do not start at 0 or descend) are TF_ERR_ARG.  n == 0 launches
 * nothing and leaves num_keep as the caller zeroed it.  A segment longer than TF_SOFT_NMS_MAX_BOXES is TF_ERR_UNSUPPORTED (the selection
 * of a segment runs inside one 1024-thread workgroup, one 64-candidate word per thread).  ws: tf_soft_nms_batched_workspace_bytes()
 * (n_s^2 / 8 bytes of adjacency bits per segment plus the running scores; 0 for n == 0). */
#define TF_SOFT_NMS_LINEAR   1
#define TF_SOFT_NMS_GAUSSIAN 2
#define TF_SOFT_NMS_MAX_BOXES 65536   /* largest segment (the hard NMS takes 524 160) */
size_t tf_soft_nms_batched_workspace_bytes(const int32_t* host_seg_offsets, int num_segments);
int tf_soft_nms_f64_batched(const double* boxes /*[n][4]*/, const double* scores /*[n]*/, const int32_t* host_seg_offsets /*[S+1]*/,
                            int num_segments, int method, double iou_thresh, double sigma, double score_thresh,
                            int score_mode /* TF_VOTE_WEIGHT_* */, int64_t* keep_out /*[n], indices into the concatenated input*/,
                            double* score_out /*[n]*/, int32_t* num_keep /*device [S]*/, void* ws, size_t ws_bytes, void* stream);
/* one segment: the batched form with S = 1, as tf_nms_f64 is of tf_nms_f64_batched */
size_t tf_soft_nms_workspace_bytes(int n);
int tf_soft_nms_f64(const double* boxes /*[n][4]*/, const double* scores /*[n]*/, int n, int method, double iou_thresh, double sigma,
                    double score_thresh, int score_mode, int64_t* keep_out /*[n]*/, double* score_out /*[n]*/,
                    int32_t* num_keep /*device [1]*/, void* ws, size_t ws_bytes, void* stream);
/* The same with a cap on the number of selections: max_keep inserted before keep_out.  max_keep == 0: no cap -- the entries above ARE these
 * with 0, the same launches and bits.  max_keep < 0: TF_ERR_ARG.  max_keep > 0: the selection loop of a segment ends when r == max_keep,
 * so num_keep[s] = min(uncapped count, max_keep) and the rows written are the first num_keep[s] rows of the uncapped run, bit for bit (a
 * later round never changes an earlier row); rows beyond are NOT written.  The selection costs milliseconds per thousand survivors and no
 * WIDER evaluation reads more than a few hundred detections per image: this is where `max_detections` saves its time.  A chained
 * tf_box_vote_f64_batched reads the capped count from the device as before.  Workspace and every other refusal as above. */
int tf_soft_nms_f64_batched_capped(const double* boxes /*[n][4]*/, const double* scores /*[n]*/, const int32_t* host_seg_offsets /*[S+1]*/,
                                   int num_segments, int method, double iou_thresh, double sigma, double score_thresh, int score_mode,
                                   int max_keep, int64_t* keep_out /*[n]*/, double* score_out /*[n]*/, int32_t* num_keep /*device [S]*/,
                                   void* ws, size_t ws_bytes, void* stream);
int tf_soft_nms_f64_capped(const double* boxes /*[n][4]*/, const double* scores /*[n]*/, int n, int method, double iou_thresh, double sigma,
                           double score_thresh, int score_mode, int max_keep, int64_t* keep_out /*[n]*/, double* score_out /*[n]*/,
                           int32_t* num_keep /*device [1]*/, void* ws, size_t ws_bytes, void* stream);

/* ---- Matrix NMS, float64 (Wang et al., SOLOv2, NeurIPS 2020; PaddleDetection's matrix_nms, used for boxes in PP-YOLO) ----------
 * An addition next to Soft-NMS: the same kind of decay in closed form.  A candidate's factor depends only on the better-scored candidates
 * and on THEIR largest overlap with something still better, so nothing is selected in turn and nothing is serial.  Per segment (batching
 * as tf_nms_f64_batched), with p_i the vote weight of scores[i] under score_mode (TF_VOTE_WEIGHT_SIGMOID: 1 / (1 + exp(-scores[i])),
 * TF_VOTE_WEIGHT_SCORE: scores[i]):
 *   1. Admission.  Candidate i is admitted iff p_i >= score_thresh; a NaN fails the test.  An unadmitted candidate is never emitted and
 *      decays nothing (a candidate is only ever decayed by better-scored ones, so dropping them first loses nothing).
 *   2. Rank.  The admitted are ranked by p descending, the lower input index first on an equal p (-0.0 == +0.0).  Below, i < j means
 *      "ranked above".
 *   3. IoU.  iou(i, j) is tf_nms_f64's IoU in the same operation order: areas without +1, inter / (a_i + a_j - inter); the file is
 *      compiled without FMA contraction.  inter == 0 or a NaN quotient counts as 0, as in Soft-NMS.
 *   4. Compensation.  comp_j = max_{i<j} iou(i, j); 0 for the best candidate.
 *   5. Decay.  d_0 = 1.  For j > 0:
 *      TF_MATRIX_NMS_LINEAR:   d_j = min over {i < j : comp_i < 1} of (1 - iou(i, j)) / (1 - comp_i), each term one float64 subtract,
 *        subtract, divide.  A candidate with comp_i >= 1 is an exact duplicate of a better box, which stands in for it: it contributes no
 *        term.  Rank 0 always contributes a term <= 1, so 0 <= d_j <= 1.  There is no IoU threshold.
 *      TF_MATRIX_NMS_GAUSSIAN: x_j = max_{i<j} (iou(i, j) * iou(i, j) - comp_i * comp_i), d_j = exp(-x_j / sigma): ONE exp per candidate, on
 *        the extremal argument.  sigma is the Soft-NMS sigma, a divisor (SOLOv2's and Paddle's multiplier 2.0 is sigma = 0.5).  x_j >= 0:
 *        rank 0 contributes iou^2.
 *   6. Emission.  s_j = p_j * d_j; candidate j is emitted iff s_j >= score_thresh.  Rows are ordered by s descending, the better rank
 *      first on an equal s: keep_out[off + r] = the candidate (an index into the CONCATENATED input), score_out[off + r] = s, the decayed
 *      PROBABILITY as in Soft-NMS.  num_keep[s] = min(K_s, max_keep) for K_s emitted candidates; max_keep == 0: no cap.
 * Rows r >= num_keep[s] of keep_out / score_out are NOT written, nothing outside [off[s], off[s] + num_keep[s]) is.  max and min are exact
 * and order-independent and there is no floating-point atomic: the same bits on every run; the linear method is a chain of single IEEE
 * operations behind p.  Five launches whatever n and S; no memset is asked of the caller beyond num_keep for n == 0, no host
 * synchronisation.  An unknown method or score mode, sigma that is not > 0, a negative or NaN score_thresh, max_keep < 0 and bad segment
 * tables (S outside 1..TF_NMS_MAX_SEGMENTS, offsets that do not start at 0 or descend) are TF_ERR_ARG.  n == 0 launches nothing and leaves
 * num_keep as the caller zeroed it.  A segment longer than TF_MATRIX_NMS_MAX_BOXES is TF_ERR_UNSUPPORTED.  ws:
 * tf_matrix_nms_batched_workspace_bytes(): 68 bytes per candidate (no n^2 / 8 adjacency bits), every byte read is written by the call
 * first; 0 for n == 0. */
#define TF_MATRIX_NMS_LINEAR   1
#define TF_MATRIX_NMS_GAUSSIAN 2
#define TF_MATRIX_NMS_MAX_BOXES 524160   /* the hard NMS's largest segment: the kernels hold nothing per segment in one workgroup, so they need no less */
size_t tf_matrix_nms_batched_workspace_bytes(const int32_t* host_seg_offsets, int num_segments);
int tf_matrix_nms_f64_batched(const double* boxes /*[n][4]*/, const double* scores /*[n]*/, const int32_t* host_seg_offsets /*[S+1]*/,
                              int num_segments, int method, double sigma, double score_thresh, int score_mode /* TF_VOTE_WEIGHT_* */,
                              int max_keep, int64_t* keep_out /*[n], indices into the concatenated input*/, double* score_out /*[n]*/,
                              int32_t* num_keep /*device [S]*/, void* ws, size_t ws_bytes, void* stream);
/* one segment: the batched form with S = 1 */
size_t tf_matrix_nms_workspace_bytes(int n);
int tf_matrix_nms_f64(const double* boxes /*[n][4]*/, const double* scores /*[n]*/, int n, int method, double sigma, double score_thresh,
                      int score_mode, int max_keep, int64_t* keep_out /*[n]*/, double* score_out /*[n]*/, int32_t* num_keep /*device [1]*/,
                      void* ws, size_t ws_bytes, void* stream);

/* ---- deterministic top-k selection on float64 scores (the `top_k` / `topk_candidates` step in front of the suppression) ----------
 * An addition in front of tf_nms_f64 / tf_soft_nms_f64, both O(n^2): it bounds the candidates that reach them, and cuts a list too long
 * for either to one they take.  Segments as for tf_nms_f64_batched: a HOST offset table, [0] == 0, S <= TF_NMS_MAX_SEGMENTS.  For segment
 * s with n_s rows the call writes m_s = min(n_s, k) indices INTO THE CONCATENATED INPUT to idx_out[sum_{r<s} m_r ...]; every m_s is known
 * on the host, so there is no device-side count and no synchronisation.
 *   Which rows: the m_s rows that come first in the order the hard NMS itself uses (rank[i] = #{j : s_j > s_i or (s_j == s_i and j < i)}):
 *     larger score first; on equal scores the lower input index first (-0.0 and +0.0 are equal); a NaN ranks behind every number, -inf
 *     included, NaNs among themselves by index (HERE a NaN is never preferred to a number; tf_nms_f64 visits NaNs first, as torch.sort
 *     does: the identity below is stated for scores without NaN).
 *   In which order: ASCENDING input index, not score order -- the compacted list keeps the candidate list's order, so a later stable sort,
 *     tie-break or voter sum sees the rows it would have seen.  Hence, with idx the output for one segment and nms() = tf_nms_f64's keep
 *     list:  idx[nms(boxes[idx], scores[idx])] == the entries of nms(boxes, scores) whose rank is below k, and those are a prefix of it.
 *   n_s <= k: the segment is passed through whole (idx = off_s ... off_s + n_s - 1).
 * k < 1, a bad segment table (S outside 1..TF_NMS_MAX_SEGMENTS, offsets that do not start at 0 or descend), a NULL scores / idx_out / ws
 * with n > 0 or a workspace shorter than tf_topk_batched_workspace_bytes() are TF_ERR_ARG.  n == 0 launches nothing.  Nothing but
 * idx_out[0 .. sum m_s) and the workspace is written; scores is only read.  A segment is as long as the int32 offsets allow.
 * How: an MSB-first radix select over an order-preserving uint64 key, 8 passes of 8 bits, each a per-segment digit histogram (integer
 * atomics only: the counts do not depend on arrival order), then an ordered compaction (count, scan, write).  Work linear in n per pass;
 * 12 enqueues whatever n and S; no grid barrier, no cooperative launch, no spinning on another workgroup; the same bits on every run. */
size_t tf_topk_batched_workspace_bytes(const int32_t* host_seg_offsets, int num_segments, int k);
int tf_topk_select_f64_batched(const double* scores /*[n]*/, const int32_t* host_seg_offsets /*[S+1]*/, int num_segments, int k,
                               int64_t* idx_out /*[sum_s min(n_s, k)]*/, void* ws, size_t ws_bytes, void* stream);
/* one segment: the batched form with S = 1 */
size_t tf_topk_workspace_bytes(int n, int k);
int tf_topk_select_f64(const double* scores /*[n]*/, int n, int k, int64_t* idx_out /*[min(n, k)]*/, void* ws, size_t ws_bytes, void* stream);

/* ---- WIDER FACE evaluation on the device: matching and the precision / recall table ----------
 * The device form of tinyfaces/wider_eval.py's image_evaluation and image_pr_info, held to them bit for bit (every output is an integer).
 * Segments are images: HOST int32 offset tables that start at 0 and never descend, as tf_nms_f64_batched takes them, but with no bound on
 * the number of segments (the tables ride in the kernel arguments, 256 segments per launch).  Empty segments are legal.
 *
 * tf_wider_match_f64_batched.  rows: detections in result-file form (x, y, w, h, score), each segment score-descending (the score is not
 * read here).  gt: boxes (x, y, w, h) with an offset table of their own over the SAME num_segments.  keep[k][j] != 0: box j counts in
 * setting k.  Once for all settings, per detection h of an image:
 *     corners    x + w, y + h: one fp64 addition each, for detections and boxes alike;
 *     IoU        wider_eval.box_overlap: w = min(x2) - max(x1) + 1, h likewise, 0 when w <= 0 or h <= 0 (decided before the division), else
 *                inter / ((a + b) - inter) with a, b the +1 areas; every operation rounded on its own (the file is built without FMA
 *                contraction).  Coordinates are finite numbers;
 *     best[h]    the box of largest IoU, the LOWEST index on a tie (np.argmax); a match iff that IoU >= iou_thresh.
 * Per setting k:  proposal[h] = -1 iff h matched a box with keep[k] == 0, else 1;
 *     counted[k][h]  = #{h' <= h in the segment : proposal[h'] == 1}                       (np.cumsum(proposal == 1))
 *     recalled[k][h] = #{boxes j with keep[k][j] : some h' <= h matched j}                 (pred_recall)
 * computed as first[j] = min{h : best[h] == j} (an integer min) and two prefix sums.  An image without boxes matches nothing: counted is
 * 1, 2, 3, ..., recalled 0.  One 256-thread workgroup per image; the boxes pass through LDS in tiles of TF_WIDER_GT_TILE, so their number
 * is not bounded by LDS.  Writes counted / recalled rows [0, n) of every setting and the workspace, nothing else; no floating-point
 * atomics, no grid barrier, no memset, no host synchronisation; the same bits on every run.  ws: tf_wider_match_workspace_bytes(n, g).
 * TF_ERR_ARG before anything is enqueued: nset < 1, a NaN iou_thresh, num_segments < 1, a NULL table or one that does not start at 0 or
 * descends, a NULL rows / counted / recalled / ws with n > 0, a NULL gt / keep with g > 0, a short workspace.  n == 0 launches nothing. */
#define TF_WIDER_GT_TILE 256
size_t tf_wider_match_workspace_bytes(int n, int g);
int tf_wider_match_f64_batched(const double* rows /*[n][5]*/, const int32_t* host_det_offsets /*[S+1]*/, const double* gt /*[g][4]*/,
                               const int32_t* host_gt_offsets /*[S+1]*/, int num_segments, const uint8_t* keep /*[nset][g]*/, int nset,
                               double iou_thresh, int32_t* counted /*[nset][n]*/, int32_t* recalled /*[nset][n]*/, void* ws, size_t ws_bytes,
                               void* stream);
/* tf_wider_pr_accumulate ADDS image_pr_info, summed over the segments, into pr[nset][T][2] (int64; the caller zeroes it once).  scores[n]:
 * the raw scores under the same detection table, each segment non-increasing.  lo_d: DEVICE double[2] = (lo, d) of norm_scores, so no
 * host read sits between the matching and the table.  thresh: DEVICE double[T], filled by the host with 1 - (t + 1) / T.  For segment s
 * and threshold t: r = the last row of s with (scores[r] - lo) / d >= thresh[t] (one fp64 subtraction, one fp64 division: norm_scores'
 * bits; found by binary search, the normalisation being monotone); if there is one, pr[k][t][0] += counted[k][r] and
 * pr[k][t][1] += recalled[k][r].  64-bit integer atomics only: the same table in any arrival order.  TF_ERR_ARG as above (nset < 1,
 * T < 0, a bad table, a NULL operand with n > 0 and T > 0); n == 0 or T == 0 launches nothing. */
int tf_wider_pr_accumulate(const double* scores /*[n]*/, const int32_t* host_det_offsets /*[S+1]*/, int num_segments,
                           const int32_t* counted /*[nset][n]*/, const int32_t* recalled /*[nset][n]*/, int nset,
                           const double* lo_d /*device [2]*/, const double* thresh /*device [T]*/, int num_thresh,
                           int64_t* pr /*[nset][T][2]*/, void* stream);

/* ---- score map -> boxes: sigmoid + threshold + ORDERED compaction + refinement ------
 * Replaces evaluation.py:61-78 + get_bboxes / regression_refinement
 * (tinyfaces/models/utils.py:4-100).  score [5nt][H][W] f32 (one image, NCHW).
 * Candidates are appended to dets[*count ...] as rows (x1,y1,x2,y2,score) f64 in the
 * reference's order: C-order over (y, x, template).  valid_x[W] / valid_t[nt] (u8) express
 * the template mask; the reference's defect D1 (utils.py:44 masks the W axis) is
 * reproduced by the caller passing it through valid_x.  A masked entry has probability 0
 * (it passes only a negative prob_thresh); an entry is a candidate iff prob > prob_thresh,
 * both fp32; a NaN logit is never one.  templates [nt][tstride] f64, tstride >= 4: columns
 * 0..3 are read, the rest is padding.
 * *count (DEVICE int32) is read as the row the first candidate goes to and comes back as
 * *count + the TRUE number of candidates of this map, whatever cap is: a caller chains maps
 * through it and checks *count <= cap once at the end.  Rows r >= cap are NOT written, so
 * exactly rows [*count before, min(*count after, cap)) are; no other row of dets is touched.
 * nt is bounded by the write pass's LDS slab: 5 * nt * 64 * 4 bytes plus the kernel's 20
 * static bytes must fit 64 KiB, i.e. nt <= 51; a larger nt is TF_ERR_UNSUPPORTED, refused
 * on the host before anything is launched (*count and dets stay as they were). */
size_t tf_decode_workspace_bytes(int H, int W, int nt);
int tf_decode_compact(const float* score, int nt, int H, int W,
                      const double* templates, int tstride,
                      const uint8_t* valid_x, const uint8_t* valid_t,
                      float prob_thresh, double scale, int sty, int stx, int ofy, int ofx,
                      double* dets /*[cap][5]*/, int32_t* count /*device, in/out*/, int cap,
                      void* ws, size_t ws_bytes, void* stream);

/* ---- detection criterion: OHEM + balance sampling + masked SoftMargin / SmoothL1 ----
 * Replaces DetectionCriterion.forward and its autograd backward
 * (tinyfaces/models/loss.py:59-93, tinyfaces/models/utils.py:103-163) with no host
 * round trip.  output [B][5nt][H][W] f32; class_map [B][nt][H][W] f32 is mined IN PLACE
 * (loss.py:62); label_out receives the labels after balance sampling; grad_out =
 * d(total)/d(output); loss_out[0] = sum cls, loss_out[1] = sum reg (unweighted).
 * pos_keep/neg_keep: optional u8 [B][nt*H*W] keep flags indexed by the C-order RANK of the
 * positive / negative label inside its image (injects the reference's np.random
 * permutation); NULL -> uniformly random subset from the counter RNG(seed). */
size_t tf_criterion_workspace_bytes(int B, int nt, int H, int W);
int tf_criterion_fwd_bwd(const float* output, float* class_map, const float* reg_map,
                         int B, int nt, int H, int W, float ohem_thresh, int max_pos, int max_neg,
                         float reg_weight, const uint8_t* pos_keep, const uint8_t* neg_keep, uint64_t seed,
                         float* label_out, float* grad_out, double* loss_out /*[2]*/,
                         int32_t* counts_out /*[B][2] or NULL*/, void* ws, size_t ws_bytes, void* stream);

/* ---- detection criterion, focal form: sigmoid focal loss over EVERY labelled element + SmoothL1 over every positive ----
 * No OHEM, no sampling, no RNG; class_map (labels +1 / -1 / 0 = ignore) is only read.  Same layout as tf_criterion_fwd_bwd.
 * With s the class logit, x = y s, softplus(v) = max(v, 0) + log1p(exp(-|v|)) and a_t = alpha (y = +1), 1 - alpha (y = -1), or 1 when
 * alpha < 0 (torchvision's sigmoid_focal_loss convention):
 *   FL     = a_t exp(-gamma softplus(x)) softplus(-x)                  ( = -a_t (1 - p_t)^gamma log p_t )
 *   dFL/ds = -y a_t exp(-gamma softplus(x)) (gamma sigmoid(x) softplus(-x) + sigmoid(-x))
 * Regression: SmoothL1 (beta = 1) over the four channels of every y = +1 element, gradient times reg_weight.
 * normalize = TF_FOCAL_NORM_POS: both sums and all five gradient channels of image b are multiplied by 1 / max(1, npos_b), npos_b = its
 * number of +1 labels, and the images are SUMMED (an image's loss does not depend on its batch); TF_FOCAL_NORM_NONE: the plain sum.
 * loss_out[0] = sum cls, loss_out[1] = sum reg (unweighted), both normalised as above; npos_out[b] = npos_b.  grad_out is written
 * completely (no memset needed).  No floating-point atomics: the same bits on every run.  TF_ERR_ARG: a NULL operand, a non-positive
 * dimension, gamma negative or not finite, alpha not finite or > 1, an unknown normalize. */
#define TF_FOCAL_NORM_NONE 0
#define TF_FOCAL_NORM_POS  1
size_t tf_criterion_focal_workspace_bytes(int B, int nt, int H, int W);
int tf_criterion_focal_fwd_bwd(const float* output, const float* class_map, const float* reg_map, int B, int nt, int H, int W,
                               float gamma, float alpha, int normalize, float reg_weight,
                               float* grad_out, double* loss_out /*[2]*/, int32_t* npos_out /*[B], may be NULL*/,
                               void* ws, size_t ws_bytes, void* stream);

/* ---- detection criterion, focal form with an overlap regression loss: IoU, GIoU (Rezatofighi et al. 2019), DIoU (Zheng et al. 2020) ----
 * tf_criterion_focal_fwd_bwd with the SmoothL1 regression replaced: same operands, same workspace query (tf_criterion_focal_workspace_bytes),
 * same three launches, same classification loss, normaliser, summation order and determinism.  reg_form = TF_REG_SMOOTH_L1 runs the
 * kernels of tf_criterion_focal_fwd_bwd itself (the same bits).  Otherwise, for every element with label +1, with p = (px, py, pw, ph) from
 * channel blocks 1..4 of output and t = (tx, ty, tw, th) from reg_map (tx = (fcx - cx) / dw, tw = log(fw / dw), ...: in the anchor's
 * template-normalised frame a prediction is the box with centre (px, py) and size (e^pw, e^ph)):
 *   clamp   pw, ph to [-C, C], C = log(1000 / 16) (torchvision's bbox_xform_clip); the gradient through the clamp is 1 inside the closed
 *           interval and 0 outside (torch.clamp); the targets are not clamped
 *   boxes   predicted [px -+ e^pw / 2] x [py -+ e^ph / 2], target the same from t;
 *           iw = max(0, min(x2) - max(x1)), ih likewise, I = iw ih, U = e^(pw + ph) + e^(tw + th) - I, IoU = I / U;
 *           enclosing box cw = max(x2) - min(x1), ch likewise, Cbox = cw ch.  All areas are > 0 under the clamp: no epsilon anywhere
 *   TF_REG_IOU   1 - IoU
 *   TF_REG_GIOU  1 - IoU + (Cbox - U) / Cbox
 *   TF_REG_DIOU  1 - IoU + ((a dx)^2 + dy^2) / ((a cw)^2 + ch^2), a = dw / dh of the anchor's template (template_wh[t] = (dw, dh),
 *                dw = x2 - x1 + 1 of the template box), dx = px - tx, dy = py - ty
 * IoU and GIoU do not change under a per-axis scaling, so they need neither the anchor centre nor the template table.
 * ONE term per positive element (not four) is added to loss_out[1]; its four partial derivatives, times reg_weight and the image's
 * normaliser, go to the four regression channels of grad_out.  The loss is continuous; on a kink (two edges tie, iw or ih exactly 0, |pw|
 * or |ph| exactly C) the gradient is some finite one-sided value.  Arithmetic per element is fp32, the sums fp64.
 * template_wh: [nt][2] f32 on the device, required for TF_REG_DIOU and ignored otherwise.
 * TF_ERR_ARG: as tf_criterion_focal_fwd_bwd, and reg_weight not finite, an unknown reg_form, TF_REG_DIOU without template_wh. */
#define TF_REG_SMOOTH_L1 0
#define TF_REG_IOU       1
#define TF_REG_GIOU      2
#define TF_REG_DIOU      3
int tf_criterion_focal_box_fwd_bwd(const float* output, const float* class_map, const float* reg_map, int B, int nt, int H, int W,
                                   float gamma, float alpha, int normalize, float reg_weight,
                                   int reg_form, const float* template_wh /*[nt][2], device; may be NULL unless TF_REG_DIOU*/,
                                   float* grad_out, double* loss_out /*[2]*/, int32_t* npos_out /*[B], may be NULL*/,
                                   void* ws, size_t ws_bytes, void* stream);

/* ---- detection criterion, quality focal form (QFL; Li et al. 2020, Generalized Focal Loss): IoU-aware classification targets ----
 * The focal form with the hard target 1 of a positive replaced by the quality q of ITS OWN predicted box: same operands, same layout, the
 * same three launches, normaliser, summation order and determinism as tf_criterion_focal_box_fwd_bwd.  There is no alpha.  For an element
 * with label y, class logit s, p = (px, py, pw, ph) from channel blocks 1..4 of output and t = (tx, ty, tw, th) from reg_map:
 *   y =  0   contributes nothing; all five gradient channels are 0
 *   y = -1   q = 0
 *   y = +1   q = min(1, IoU), the IoU of the overlap-loss section above: pw, ph clamped to [-C, C], C = log(1000 / 16), the targets not
 *            clamped, no epsilon, fp32 from the centre offset and the half sizes (u = e^pw / 2, v = e^tw / 2, dx = px - tx:
 *            iw = max(0, min(2u, 2v, u + v - |dx|)), ih likewise, I = iw ih, U = 4 u u' + 4 v v' - I, IoU = I (1 / U)).  A positive whose
 *            boxes do not meet has q = 0 and its class logit is trained exactly like a negative's
 *   sigma = sigmoid(s), d = sigma - q, BCE = softplus(s) - q s, softplus(v) = max(v, 0) + log1p(exp(-|v|)), with e = exp(-|s|):
 *            sigma = 1 / (1 + e) for s >= 0 and e / (1 + e) otherwise, sigma (1 - sigma) = e / (1 + e)^2: finite for s = +-1e4
 *   QFL      = |d|^beta BCE
 *   dQFL/ds  = |d|^beta d + beta |d|^(beta - 1) sgn(d) sigma (1 - sigma) BCE,  sgn(0) = 0;  beta = 2 is d d and 2 d, without powf; any other
 *            beta takes one powf, |d|^beta = |d|^(beta - 1) |d|
 * q is a CONSTANT of the classification term: nothing flows from it into the four regression channels.  The regression term of a positive
 * and its gradient are those of reg_form (TF_REG_*), by the arithmetic of tf_criterion_focal_box_fwd_bwd; with TF_REG_SMOOTH_L1 the IoU is
 * computed for q alone.  normalize as in the focal form: both sums and all five gradient channels of image b times 1 / max(1, npos_b), the
 * images summed.  beta must be finite and >= 1: below 1 the gradient is unbounded at sigma = q.  For 1 <= beta < 2 it is ill-conditioned
 * where sigma is close to q (the factor |d|^(beta - 1) has an unbounded slope there), and for beta = 1 it jumps at sigma = q.
 * loss_out[0] = sum cls, loss_out[1] = sum reg (unweighted), both normalised; loss_out[2] = sum of q over all positives of the batch, NOT
 * normalised; loss_out[3] = sum_b npos_b as a double: [2] / [3] is the mean IoU of the predicted boxes with their targets.
 * grad_out is written completely, every element exactly once (no memset needed).  No floating-point atomics: the same bits on every run.
 * The workspace is one double per block larger than tf_criterion_focal_workspace_bytes.
 * TF_ERR_ARG: a NULL operand, a non-positive dimension, beta not finite or < 1, reg_weight not finite, an unknown normalize or reg_form,
 * TF_REG_DIOU without template_wh; TF_ERR_WORKSPACE: ws NULL or too small.  Nothing is enqueued in either case. */
size_t tf_criterion_quality_workspace_bytes(int B, int nt, int H, int W);
int tf_criterion_quality_fwd_bwd(const float* output, const float* class_map, const float* reg_map, int B, int nt, int H, int W,
                                 float beta, int normalize, float reg_weight,
                                 int reg_form, const float* template_wh /*[nt][2], device; may be NULL unless TF_REG_DIOU*/,
                                 float* grad_out, double* loss_out /*[4]*/, int32_t* npos_out /*[B], may be NULL*/,
                                 void* ws, size_t ws_bytes, void* stream);

/* ---- detection criterion, task-aligned form (Feng et al. 2021, TOOD): the assigner's normalised alignment as target and box weight ----
 * tf_criterion_quality_fwd_bwd with the target of a positive READ from align_map [B][nt][H][W] f32 (what tf_targets_tal_aligned wrote) in
 * place of the IoU of its own box, and with the regression term of every positive weighted by that target: same layout, three launches,
 * summation order and determinism.  For an element with label y, class logit s and map value a:
 *   y =  0   contributes nothing; all five gradient channels are 0
 *   y = -1   q = 0; a is not read
 *   y = +1   q = fminf(1, fmaxf(0, a)): a NaN gives 0
 *   classification  exactly the QFL arithmetic above with this q: sigma, d = sigma - q, BCE = softplus(s) - q s in their stable forms,
 *            QFL = |d|^beta BCE and its derivative, beta = 2 without powf.  q is a constant
 *   regression      the term of reg_form (all four TF_REG_*, by the arithmetic of tf_criterion_focal_box_fwd_bwd; TF_REG_SMOOTH_L1: the sum of
 *            the four SmoothL1 terms, added in fp32) TIMES q; its four derivatives times q * (reg_weight * normaliser)
 *   normalize       TF_FOCAL_NORM_NONE and TF_FOCAL_NORM_POS as in the focal form.  TF_FOCAL_NORM_ALIGN: both sums and all five gradient
 *            channels of image b times 1 / max(1, Q_b), Q_b = the sum of q over ITS positives: TOOD's avg_factor, taken per image and not per
 *            batch, so that an image's loss still depends neither on its batch nor on the number of ranks.  Q_b is an fp64 sum of per-block fp64
 *            partials added in a fixed order by every block that needs it; the gradient's factor is (float)(1 / max(1, Q_b))
 * loss_out[0] = sum cls, loss_out[1] = sum of the q-weighted regression terms (not weighted by reg_weight), both normalised;
 * loss_out[2] = sum of q over all positives of the batch, NOT normalised; loss_out[3] = sum_b npos_b: [2] / [3] is the mean target.
 * grad_out is written completely, every element exactly once.  No floating-point atomics: the same bits on every run.
 * TF_ERR_ARG: what tf_criterion_quality_fwd_bwd refuses, a NULL align_map, a normalize outside the three values (TF_FOCAL_NORM_ALIGN passed to
 * any other entry point stays TF_ERR_ARG); TF_ERR_WORKSPACE: ws NULL or below tf_criterion_aligned_workspace_bytes.  Nothing is enqueued then. */
#define TF_FOCAL_NORM_ALIGN 2
size_t tf_criterion_aligned_workspace_bytes(int B, int nt, int H, int W);
int tf_criterion_aligned_fwd_bwd(const float* output, const float* class_map, const float* reg_map, const float* align_map,
                                 int B, int nt, int H, int W, float beta, int normalize, float reg_weight,
                                 int reg_form, const float* template_wh /*[nt][2], device; may be NULL unless TF_REG_DIOU*/,
                                 float* grad_out, double* loss_out /*[4]*/, int32_t* npos_out /*[B], may be NULL*/,
                                 void* ws, size_t ws_bytes, void* stream);

/* ---- fused SGD step (momentum, weight decay) over a flat fp32 segment ---------------
 * Replaces torch.optim.SGD.step as configured at main.py:67-70 for one parameter group. */
int tf_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n,
                float lr, float momentum, float weight_decay, float grad_scale, void* stream);
/* The same update over a TABLE of element ranges of the three flat buffers: host_segments[nseg][2] = (start, end), ascending and disjoint
 * (HOST memory; the table travels as kernel arguments, TF_SGD_MAX_SEGMENTS ranges per launch).  Elements outside the ranges are neither
 * read nor written: no weight decay, no momentum.  Replaces torch.optim.SGD.step (main.py:67-70) for a parameter group whose BatchNorm
 * vectors have no gradient (requires_grad = False: torch skips them) while they sit interleaved with the conv weights in the flat buffer. */
#define TF_SGD_MAX_SEGMENTS 128
int tf_sgd_step_segments(float* param, const float* grad, float* momentum_buf, const int64_t* host_segments, int nseg,
                         float lr, float momentum, float weight_decay, float grad_scale, void* stream);

/* ---- gradient-norm clipping and the non-finite-step guard ------------------------------
 * Replaces torch.nn.utils.clip_grad_norm_ at the spot between loss.backward() and optimizer.step() (tinyfaces/trainer.py:86-87), which the
 * reference leaves empty: the global L2 norm of the gradient, the clip coefficient and the skip verdict stay in DEVICE memory (one
 * tf_clip_state, 32 bytes), and the SGD entry points below read them from there -- the step stays free of host syncs.
 *   sumsq    sum of squares of the gradient elements inside the ranges (fp64, unscaled)
 *   norm     |grad_scale| * sqrt(sumsq)
 *   coef     min(1, max_norm / (norm + 1e-6)) as torch defines it (fp64 arithmetic, stored as float); 1 when max_norm <= 0 or +inf
 *   skip     1: norm is not finite and TF_CLIP_SKIP_NONFINITE was given (coef = 0 then); else 0
 *   skipped  how many times skip was set since the caller zeroed the state (a plain counter, advanced by tf_grad_clip_coef alone) */
typedef struct tf_clip_state { double sumsq; double norm; float coef; int32_t skip; int64_t skipped; } tf_clip_state;
#define TF_CLIP_SKIP_NONFINITE 1
/* tf_grad_clip_coef: one deterministic pass over the ranges host_segments[nseg][2] (as tf_sgd_step_segments: HOST memory, ascending and
 * disjoint, TF_SGD_MAX_SEGMENTS per launch) of the flat fp32 gradient.  Every element is squared and summed in fp64; each block stores ONE
 * partial sum into ws (no atomics: the result is bit-identical from run to run), a one-block launch adds the partials in index order and
 * writes *state.  Elements outside the ranges are never read; grad is never written.  ws: tf_grad_norm_workspace_bytes(nseg) bytes (exact:
 * one double per block of every launch at their capped grid; less is TF_ERR_ARG), 8-byte aligned, written in full or in part, never read
 * beyond what this call wrote.  nseg == 0: norm 0, coef 1 (grad and ws may be NULL). */
size_t tf_grad_norm_workspace_bytes(int nseg);
int tf_grad_clip_coef(const float* grad, const int64_t* host_segments, int nseg, float grad_scale, float max_norm, int flags,
                      void* ws, size_t ws_bytes, tf_clip_state* state /*device*/, void* stream);
/* tf_sgd_step / tf_sgd_step_segments with the verdict of a tf_grad_clip_coef enqueued earlier on the same stream (replaces optimizer.step()
 * behind clip_grad_norm_, tinyfaces/trainer.py:86-87): grad_scale * state->coef (one fp32 product) takes the place of grad_scale, and with
 * state->skip set neither param nor momentum_buf is touched.  state == NULL is TF_ERR_ARG (call the plain entry points instead). */
int tf_sgd_step_clipped(float* param, const float* grad, float* momentum_buf, int64_t n,
                        float lr, float momentum, float weight_decay, float grad_scale, const tf_clip_state* state, void* stream);
int tf_sgd_step_segments_clipped(float* param, const float* grad, float* momentum_buf, const int64_t* host_segments, int nseg,
                                 float lr, float momentum, float weight_decay, float grad_scale, const tf_clip_state* state, void* stream);
/* grad[i] *= state->coef over the ranges; with state->skip set nothing is read and ZEROS are stored (coef is 0 then, but NaN * 0 is NaN:
 * the gradient an optimizer sees behind a skipped step is the zero it was scaled to).  Elements outside the ranges are neither read nor
 * written.  The in-place scaling clip_grad_norm_ does at tinyfaces/trainer.py:86-87 when torch.optim.SGD applies the update (the autograd path). */
int tf_scale_segments(float* grad, const int64_t* host_segments, int nseg, const tf_clip_state* state, void* stream);

/* ---- model EMA: an exponential moving average of the weights, kept on the device ------------
 * Replaces torch.optim.swa_utils.AveragedModel.update_parameters (multi_avg_fn = get_ema_multi_avg_fn(d)) behind optimizer.step() at
 * tinyfaces/trainer.py:87, which the reference does not have.  One update is  ema[i] = fmaf(ema_weight, param[i] - ema[i], ema[i])  in fp32,
 * explicitly fused (torch.lerp(ema, param, ema_weight) for ema_weight < 0.5), with ema_weight = (float)(1 - decay_t) rounded once by the
 * caller; `ema` is a flat fp32 buffer laid out like `param`.  In all three, `state` may be NULL (not clipped, not guarded); a state whose
 * skip is set (tf_grad_clip_coef earlier on the stream) makes the call a no-op on the device: param, momentum_buf and ema keep their bits.
 *
 * tf_sgd_step_ema / tf_sgd_step_segments_ema: tf_sgd_step[_clipped] / tf_sgd_step_segments[_clipped] (param and momentum_buf bit for bit
 * theirs) with the average taken on the updated parameter while it is still in registers: one more read and one more write of 4 B per
 * element, 28 B instead of 20 B.  The 16-byte path needs all four bases 16-byte aligned (and a 4-aligned table); element-wise otherwise.
 * ema NULL with n > 0 / nseg > 0 is TF_ERR_ARG; other argument errors and n == 0 / nseg == 0 as in the plain entries. */
int tf_sgd_step_ema(float* param, const float* grad, float* momentum_buf, float* ema, int64_t n, float lr, float momentum, float weight_decay,
                    float grad_scale, float ema_weight, const tf_clip_state* state /*may be NULL*/, void* stream);
int tf_sgd_step_segments_ema(float* param, const float* grad, float* momentum_buf, float* ema, const int64_t* host_segments, int nseg,
                             float lr, float momentum, float weight_decay, float grad_scale, float ema_weight,
                             const tf_clip_state* state /*may be NULL*/, void* stream);
/* The average alone over the ranges host_segments[nseg][2] (as tf_scale_segments: HOST memory, ascending and disjoint, TF_SGD_MAX_SEGMENTS per
 * launch), for the autograd path where torch.optim.SGD has applied the update (AveragedModel.update_parameters right behind optimizer.step(),
 * tinyfaces/trainer.py:87): reads param and ema, writes ema, touches nothing outside the ranges.  16-byte moves on a 4-aligned table and a
 * 16-byte-aligned pair of bases, element-wise moves otherwise.  A null or unordered table is TF_ERR_ARG; nseg == 0 is TF_OK, no launch. */
int tf_ema_update_segments(float* ema, const float* param, const int64_t* host_segments, int nseg, float ema_weight,
                           const tf_clip_state* state /*may be NULL*/, void* stream);

/* ---- gradient accumulation: several micro-batches per optimizer step ---------------------------
 * Replaces what autograd does when loss.backward() runs more than once between optimizer.zero_grad() and optimizer.step()
 * (tinyfaces/trainer.py:85-87): the fused backward pass rewrites the flat gradient on every call, so the sum over a window of micro-batches is
 * kept in a second flat fp32 buffer `acc`, laid out like `grad`, over the ranges host_segments[nseg][2] (as tf_scale_segments: HOST memory,
 * ascending and disjoint, TF_SGD_MAX_SEGMENTS per launch).
 *   TF_ACCUM_STORE   acc = grad          first micro-batch of a window: acc is written without being read or zeroed, so nothing of an
 *                                        earlier window (a NaN included) survives
 *   TF_ACCUM_ADD     acc = acc + grad    micro-batches in between; grad is read only
 *   TF_ACCUM_FINISH  grad = acc + grad   last micro-batch: the sum is written into grad, the buffer the norm, the exchange and the update
 *                                        read; acc is read only
 * One plain fp32 add per element with acc as the left operand: a window of N adds as ((g1 + g2) + g3) + ..., the order in which torch
 * accumulates .grad.  No atomics; elements outside the ranges are neither read nor written.  16-byte moves on a 4-aligned table and a
 * 16-byte-aligned pair of bases, element-wise moves otherwise.  A null pointer, nseg < 0, an unordered table or an unknown mode is
 * TF_ERR_ARG; nseg == 0 is TF_OK, no launch. */
#define TF_ACCUM_STORE 0
#define TF_ACCUM_ADD 1
#define TF_ACCUM_FINISH 2
int tf_grad_accumulate_segments(float* acc, float* grad, const int64_t* host_segments, int nseg, int mode, void* stream);

/* ---- fused AdamW step (decoupled weight decay) -------------------------------------------------
 * Replaces torch.optim.AdamW.step (single-tensor path; amsgrad, maximize, capturable off) where main.py:67-70 builds torch.optim.SGD, for one
 * parameter group.  Four flat fp32 buffers laid out alike (param, grad, exp_avg, exp_avg_sq) and, optionally, the model EMA as a fifth.
 *
 * The step counter and the two bias corrections live in DEVICE memory (one tf_adam_state, 24 bytes, zeroed by the caller), because the verdict
 * of the non-finite guard lives there too: bias correction must not advance on a step the guard dropped, and the host learns of that only
 * through a sync.  tf_adamw_advance (one thread, once per optimizer step, behind tf_grad_clip_coef when there is one): with clip given and
 * clip->skip set it returns without touching *st; otherwise  step += 1, bias1 = 1 - beta1^step, bias2 = 1 - beta2^step.  The power is
 * square-and-multiply, least significant bit first, on double-double values (hi, lo), the result being r.hi:
 *     r = (1, 0); x = (beta, 0); t = step; while (t) { if (t & 1) r = mul(r, x); x = mul(x, x); t >>= 1; }
 *     mul(x, y):       (p, e) = two_prod(x.hi, y.hi);  e = e + (x.hi * y.lo + x.lo * y.hi);  s = p + e;  return (s, e - (s - p))
 *     two_prod(a, b):  p = a * b;  ca = 134217729 * a;  ah = ca - (ca - a);  al = a - ah;  cb, bh, bl likewise from b;
 *                      e = ((ah * bh - p) + ah * bl + al * bh) + al * bl;  return (p, e)          (Dekker's exact product, no fma)
 * Every operation is one plain double operation in the order written, so a host can repeat it operation for operation (libm's pow
 * gives no such promise), and the power is right to about one ulp for every step count: with plain double products the squarings
 * would carry up to (step - 1) * 2^-53 of relative error.
 *
 * The hyper-parameters travel as doubles: every per-element constant is derived once on the host in double and rounded once to float
 * (1 - beta2 taken from a float32 beta2 costs 1.3e-5 relative accuracy in exp_avg_sq).
 *     host:      decay = (float)(1 - lr*wd)   w1 = (float)(1 - beta1)   b2 = (float)beta2   w2 = (float)(1 - beta2)   e = (float)eps
 *     prologue:  ss = (float)(lr / st->bias1)   c2 = (float)sqrt(st->bias2)      (double arithmetic, uniform)
 *                gs = grad_scale [* clip->coef, one fp32 product, as the SGD entry points do]
 *     element:   g = grad * gs
 *                p = p * decay
 *                m = fmaf(w1, g - m, m)                  (torch.lerp(m, g, w1) for w1 < 0.5, explicitly fused)
 *                v = (b2 * v) + ((w2 * g) * g)
 *                d = (sqrtf(v) / c2) + e
 *                p = p - ss * (m / d)
 *                ema = fmaf(ema_weight, p - ema, ema)    (ema != NULL: on the updated p, as tf_sgd_step_ema)
 * Every line is one fp32 operation rounded to nearest (sqrt and the divisions correctly rounded), nothing else is contracted.
 *
 * tf_adamw_step / tf_adamw_step_segments mirror tf_sgd_step_ema / tf_sgd_step_segments_ema: the same range table (HOST memory, ascending and
 * disjoint, TF_SGD_MAX_SEGMENTS per launch), 16-byte moves when every base is 16-byte aligned (and the table 4-aligned), element-wise
 * otherwise, nothing outside [0, n) / the ranges read or written.  ema and clip may be NULL.  With clip->skip set the launch is a no-op:
 * param, both moments and ema keep their bits.  n == 0 / nseg == 0: TF_OK without a launch.  A null operand or state, an unordered table, a
 * beta outside [0, 1) or eps <= 0 is TF_ERR_ARG -- eps > 0 is required because a launch may walk alignment pads where grad, exp_avg and
 * exp_avg_sq are all zero, and 0 / (0 + 0) would plant NaNs there.  28 B per element (36 B with the EMA), no LDS, no atomics. */
typedef struct tf_adam_state { int64_t step; double bias1; double bias2; } tf_adam_state;
int tf_adamw_advance(tf_adam_state* st /*device*/, double beta1, double beta2, const tf_clip_state* clip /*may be NULL*/, void* stream);
int tf_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema /*may be NULL*/, int64_t n,
                  double lr, double beta1, double beta2, double eps, double weight_decay, float grad_scale, float ema_weight,
                  const tf_adam_state* st /*device*/, const tf_clip_state* clip /*may be NULL*/, void* stream);
int tf_adamw_step_segments(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema /*may be NULL*/,
                           const int64_t* host_segments, int nseg,
                           double lr, double beta1, double beta2, double eps, double weight_decay, float grad_scale, float ema_weight,
                           const tf_adam_state* st /*device*/, const tf_clip_state* clip /*may be NULL*/, void* stream);

/* Linear learning-rate warm-up (host arithmetic, main.py --warmup-iters N --warmup-factor F; no entry point):
 *     lr(epoch, T) = lr_at(base, epoch) * (F + (1 - F) * min(T, N) / N),   T = epoch * S + s,  S = ceil(len(loader) / accum_steps)
 * i.e. torch.optim.lr_scheduler.LinearLR(start_factor=F, total_iters=N) multiplied into StepLR's closed form; N = 0 turns it off. */

/* ---- convolution as MFMA implicit GEMM (NHWC) --------------------------------------
 * Replaces every nn.Conv2d on the path (tinyfaces/models/model.py:25-32,90-106 and the
 * torchvision Bottleneck convs) plus the BN / ReLU / residual passes fused around them.
 *   x  [N][H][W][Cin]  (dtype), w packed [CoutPad][KH*KW][Cin] K-contiguous (tf_pack_weight),
 *   y  [M][ldy] with M = N*OH*OW, ldy >= Cout, multiple of 4 (fp32) / 8 (bf16, fp16): rows are moved in 16-byte chunks.  Another ldy is
 *      TF_ERR_ARG from tf_conv2d and tf_conv_mtiles; nothing is launched.
 *   Write contract: rows [0, M) of y, ALL ldy columns of each (the pad columns [Cout, ldy) included: zero-padded weights make them the
 *      epilogue of zero), rows [0, tf_conv_mtiles()) of stat_out, stat_shift_out[0, ldy); nothing else.  aux / aux2 / aux3 are read over the
 *      same rows and columns, the per-channel vectors (epi_scale, epi_shift, mask_scale, mask_shift, stat_shift) over [0, ldy).
 * mode 0: y[p,co] = sum x[gather(p,tap),ci] w[co,tap,ci]            (forward conv)
 * mode 1: transposed gather: "x" is dY [N][H][W][Cin'=Cout_fwd] of a conv with (stride,pad)
 *         and y is dX [N][OH][OW][Cout'=Cin_fwd]  (data gradient)
 * prologue (per input channel, fwd only): x <- relu?(x*pro_scale + pro_shift), padding stays 0
 * epilogue flags (TF_EPI_*):
 *   AFFINE  v = v*epi_scale[c] + epi_shift[c]     RES   v += aux[p,c]      RELU  v = max(v,0)
 *   STATS   stat_out[mtile][0][c] += v, [1][c] += v*v  (raw accumulator, before AFFINE)
 *   MASK    v = (aux[p,c]*mask_scale[c]+mask_shift[c] > 0) ? v : 0        (dgrad through ReLU(BN(aux)))
 *   STATS2  stat_out[mtile][0][c] = sum v, [1][c] = sum v*aux[p,c]        (after MASK)
 *   JOIN    v += (aux2[p,c] > 0) ? aux3[p,c] : 0                          (residual-join gradient)
 *   MASK2   v = (aux2[p,c] > 0) ? v : 0    (after RES: gradient through the ReLU that produced aux2; LDS-DMA kernel only)
 *   STATS3  stat_out[mtile][0][c] = sum v, [1][c] = sum v*aux3[p,c]       (after MASK2; LDS-DMA kernel only)
 *           RES|MASK2|STATS3 on the last data-gradient conv of a Bottleneck hands the next block (in backward order)
 *           its already-masked output gradient together with the BN3-backward sums.
 */
#define TF_EPI_AFFINE 1
#define TF_EPI_RES 2
#define TF_EPI_RELU 4
#define TF_EPI_STATS 8
#define TF_EPI_MASK 16
#define TF_EPI_STATS2 32
#define TF_EPI_JOIN 64
#define TF_EPI_MASK2 128
#define TF_EPI_STATS3 256
/* partial-sum rows of one launch are folded (atomics) into at most this many rows; consumers pass clear=1 to the
 * last finalize that reads them so that the buffer is zero again for the next producer */
#define TF_STAT_ROWS 16
/* rows <= 0: do not fold (one partial row per tile / block, plain stores: bit-reproducible statistics; the executor then
 * uses the separate finalize kernels); 1..TF_STAT_ROWS: folded rows (fp32 atomics); default 8 */
int tf_set_stat_rows(int rows);
int tf_get_stat_rows(void);

struct tf_bn_fwd_desc;
typedef struct tf_conv_args {
  int dtype, mode;
  int N, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad;
  int ldy;            /* row stride (elements) of y, aux, aux2, aux3 */
  int epi;
  int pro_relu;
  const void* x; const void* w; void* y;
  const float* pro_scale; const float* pro_shift;
  const float* epi_scale; const float* epi_shift;
  const void* aux; const void* aux2; const void* aux3;
                      /* r6: mode 1, 1x1, stride 2 (the data gradient of a downsample conv) with TF_EPI_RES and aux == y: IN PLACE -- the launch adds its rows to the
                         even-even pixels of a raster that already holds another launch's result, touches no other pixel, and TF_EPI_MASK2 / TF_EPI_STATS3
                         then apply to those rows only (the sums take the increment).  With aux != y the raster is initialised first (zero, or aux). */
  const float* mask_scale; const float* mask_shift;
  float* stat_out;    /* [mtiles][2][ldy] fp32 partial sums, mtiles = tf_conv_mtiles() */
  int tile;           /* 0 = auto (recommended).  Else a kernel / tile code, pixels x channels: 11 128x128, 12 128x64, 13 64x64 on the LDS-DMA
                         kernel (3-deep ring; 2x = 4-deep, 3x = ring-less, 4x = 2-deep; x4 / x5 / x6 = 128x128 / 128x64 / 64x128 on 32x32x16
                         fragments), 50 = halo-resident 3x3 kernel, 70 = conv_pws (r5: wave-streaming pointwise kernel with resident weights).
                         conv_pws takes EXACTLY: 1x1 / stride 1 / pad 0, bf16 or fp16, no prologue, ldy == Cout, M >= 16 384 pixels,
                         (Cin, Cout) in {(64, 256), (256, 64), (64, 64), (256, 128)}, epilogue sets AFFINE[+RELU], AFFINE+RES+RELU (both types) and, bf16
                         only, none, STATS, MASK+STATS2, RES[+MASK2[+STATS3]]; statistic epilogues only with folded rows (tf_get_stat_rows() <=
                         TF_STAT_ROWS).  0 picks it for those launches (an explicit tile code reaches the tiled kernel there); tile = 70 on anything else is TF_ERR_UNSUPPORTED from
                         tf_conv2d and from tf_conv_mtiles (negative return).
                         Codes 1-3 (the register-staged kernel of round 1, removed in r4) and code 60 (a register-staged pointwise kernel with
                         BatchNorm prologues, measured slower on every layer and removed) are TF_ERR_UNSUPPORTED from tf_conv2d and from
                         tf_conv_mtiles, like a prologue (pro_scale != NULL) -- tf_conv2d_wgrad keeps its prologue. */
  /* TF_EPI_STATS only (r3): per-channel value subtracted from every output BEFORE it enters the two sums, so that the consumer computes
   * var = E[(x-s)^2] - E[x-s]^2 around a shift s close to the mean instead of E[x^2] - mean^2 (which loses (mean/std)^2 of the
   * significant bits in fp32).  The executor passes the BN's running mean.  stat_shift [ldy] is read and stat_shift_out [ldy] receives the shift that was used
   * (written by the launch's first pixel tile) -- the consumer reads it from there, never from a buffer that is updated meanwhile.
   * NULL: no shift (sums of x and x^2 as before). */
  const float* stat_shift; float* stat_shift_out;
  /* RESERVED (the layout is ABI): an in-LDS BatchNorm + ReLU prologue of the ring-less pointwise kernel lived here in r3-r6; it was measured
   * slower than tf_bn_relu_fused + tf_conv2d and removed.  bnf must be NULL: tf_conv2d returns TF_ERR_UNSUPPORTED otherwise, before anything
   * is launched; the other five fields are ignored. */
  const struct tf_bn_fwd_desc* bnf; void* bnf_out; int bnf_rows; float bnf_count, bnf_eps, bnf_momentum;
  int alg_k, alg_n;   /* measurement hooks only: the UNPADDED reduction length (taps * channels) and output-channel count when the
                         operands are zero-padded (stem: 147 of 192, heads: 125 of 128); 0 = Cin*KH*KW / Cout */
} tf_conv_args;

int tf_conv_mtiles(const tf_conv_args* a);   /* rows of stat_out this launch writes (<= TF_STAT_ROWS for the DMA kernel) */
int tf_conv2d(const tf_conv_args* a, void* stream);

/* OIHW fp32 -> packed [CoutPad][KH*KW][CinPad] (dtype); transpose=1 packs the data-gradient
 * operand [CinPad'][KH*KW][Cout] (roles swapped).  Pads are zero-filled. */
int tf_pack_weight(const float* w_oihw, int Cout, int Cin, int KH, int KW, int transpose,
                   int dtype, void* out, int rows_pad, int cols_pad, void* stream);
/* the same for many weights in one or two launches (job table passed as kernel arguments, no H2D copy) */
typedef struct tf_pack_job { const float* src; void* dst; int cout, cin, taps, transpose, rows_pad, cols_pad; } tf_pack_job;
int tf_pack_weights_batched(int dtype, const tf_pack_job* host_jobs, int njobs, void* stream);
/* both layouts of a weight from ONE read of the fp32 master (LDS-tiled): dst = [rows_pad >= cout][taps][cols_pad >= cin]
 * (forward operand), dst_t = [rows_pad_t >= cin][taps][cols_pad_t >= cout] (data-gradient operand); either may be NULL;
 * padding is written as zeros.  A training forward packs both, so the backward call packs nothing. */
typedef struct tf_pack2_job {
  const float* src; void* dst; void* dst_t;
  int cout, cin, taps, rows_pad, cols_pad, rows_pad_t, cols_pad_t;
  /* frozen-BN graph: dst_t[ci][tap][co] = src * scale_t[co] (a BatchNorm folded to its per-channel scale rides in the data-gradient
   * operand of the conv in front of it: autograd of tinyfaces/trainer.py:86 over model.py:89-128 with the trunk's BN in eval mode);
   * dst is never scaled.  NULL: off. */
  const float* scale_t;
} tf_pack2_job;
int tf_pack_weights_tiled(int dtype, const tf_pack2_job* host_jobs, int njobs, void* stream);

/* weight gradient: dW[co][ci][kh][kw] (+)= sum_p dY[p,co] * xhat[gather(p,tap),ci] (fp32 atomics
 * into dw_oihw, which the caller zeroes).  Same prologue semantics as tf_conv2d. */
typedef struct tf_wgrad_args {
  int dtype;
  int N, H, W, Cin, OH, OW, Cout, KH, KW, stride, pad;
  int ldx, lddy;      /* row strides (elements) of x and dy: >= Cin / Cout, multiples of 4 (fp32) / 8 (bf16) -- 16-byte chunks; else TF_ERR_ARG */
  int pro_relu;
  const void* x; const void* dy; float* dw_oihw;
  const float* pro_scale; const float* pro_shift;
  int dw_ld;          /* elements between consecutive co rows of dw (= Cin*KH*KW normally) */
  int splitk;         /* 0 = auto */
  int tile;           /* 0 = auto; 64 or 128 = channels per tile side */
  int packed;         /* 1: dw is [Cout][KH*KW][Cin] (coalesced atomics; tf_unpack_dw -> OIHW) */
  void* partial_ws;   /* optional scratch of >= tf_wgrad_workspace_bytes(a) bytes: the all-taps 3x3 kernel then reduces its split-K */
  size_t partial_ws_bytes;   /* slices through it (plain stores + one summing kernel) instead of fp32 atomics; NULL / too small: atomics */
  /* tile: 0 = auto, 1 = per-tap LDS-DMA kernel, 3 = all-taps 3x3 kernel (stride 1, pad 1, bf16), 64 / 128 = register-staged kernel */
  const float* row_scale;    /* frozen-BN graph: dW[co][...] = row_scale[co] * (the gradient above) -- the folded scale of the BatchNorm behind the conv,
                                applied to the tile before it is stored / added (autograd of tinyfaces/trainer.py:86 with the trunk's BN in eval mode).
                                Pointwise problems and the register-staged kernel; the all-taps 3x3 kernels do not take it (tf_conv2d_wgrad then uses
                                the per-tap kernel, a 3x3 tf_conv2d_wgrad_group returns TF_ERR_UNSUPPORTED).  NULL: off. */
} tf_wgrad_args;
int tf_conv2d_wgrad(const tf_wgrad_args* a, void* stream);
size_t tf_wgrad_workspace_bytes(const tf_wgrad_args* a);   /* 0 when the all-taps kernel does not apply to `a` */
/* r4: the weight gradients of a GROUP of convolutions in ONE launch, every output tile reduced over ALL pixels inside its block: no
 * split-K, no atomics, no partial-tile workspace -- dw_oihw of every problem is OVERWRITTEN (plain stores), the caller need not zero it.
 * Replaces the autograd weight gradients (tinyfaces/trainer.py:86) of the 22 identity Bottlenecks of layer 3, whose shapes are identical:
 * one such gradient alone has 16 output tiles for 256 CUs; a group of eight bottlenecks has 256.
 *   all problems 1x1 / stride 1 / pad 0 (any channel counts, ONE pixel count N*OH*OW), n <= 48: 128 x 128 tiles (csrc/wgrad_group.hip);
 *   all problems the SAME 3x3 / stride 1 / pad 1 shape, n <= 24: the all-taps kernel with splitk = 1 (csrc/wgrad3x3.hip).
 * bf16, no prologue.  TF_ERR_UNSUPPORTED: nothing was launched, call tf_conv2d_wgrad per problem (into zeroed gradients). */
int tf_conv2d_wgrad_group(const tf_wgrad_args* problems, int n, void* stream);
/* [Cout][taps][Cin] fp32 -> OIHW fp32 (overwrites) */
int tf_unpack_dw(const float* packed, int Cout, int Cin, int taps, float* dw_oihw, void* stream);

/* ---- deterministic weight gradients: the slab form of tf_conv2d_wgrad (no floating-point atomics; the same bits on every run) ----------
 * tf_conv2d_wgrad_det takes the arguments, the operand contract and the kernel choice (`tile`) of tf_conv2d_wgrad.  Every block of the
 * split-K kernel stores its fp32 tile with plain stores into its own place of the slab a->partial_ws (a->partial_ws_bytes bytes, 16-byte
 * aligned; never read by that kernel, need not be zeroed), and one summing kernel adds the slices of every output element ONCE into dw:
 *   dw = dw_in + row_scale[co] * total     (one writer per element; `packed`, dw_ld and the co < Cout, ci < Cin masks as in tf_conv2d_wgrad)
 * THE PLAN.  M = N*OH*OW pixels (the all-taps 3x3 kernel: Mp = N*(H+2)*(W+2), the zero-padded raster), PK = 64 pixels per stage (fp32: 32),
 * BC = 64 channels per tile side (the register-staged kernel with tile = 128: 128), tiles = KH*KW * ceil(Cout/BC) * ceil(Cin/BC).
 *   sk     = a->splitk when > 0, else the kernel's own choice (that of tf_conv2d_wgrad);
 *   sk     = min(sk, partial_ws_bytes / (tiles * BC*BC * 4))          -- a slab that is too small means fewer slices, never atomics;
 *                                                                        TF_ERR_ARG (nothing enqueued) when not even one slice fits;
 *   chunk  = ceil(ceil(M / sk) / PK) * PK;   slices = ceil(M / chunk); slice s reduces the pixels [s*chunk, min(M, (s+1)*chunk)): the slices
 *            cover [0, M) exactly and none is empty.
 * Slab layout: [slice][tap][co tile][ci tile][BC co][BC ci] fp32 (all-taps 3x3 kernel: [slice][co tile][ci tile][tap][64][64]).
 * THE ORDER.  G = tf_wgrad_det_groups(slices) = 16 (slices >= 128) | 4 (>= 32) | 2 (>= 16) | 1.  For g in 0 .. G-1:
 *   t_g = 0.0f; for s = g, g + G, g + 2G ... < slices: t_g = t_g + partial[s]        (fp32, rising s)
 * total = t_0; for g = 1 .. G-1: total = total + t_g; then total = total * row_scale[co] (rounded, when given); dw = dw + total.
 * tests/wgrad_det_ref.py restates both in numpy.  tf_wgrad_det_workspace_bytes: the preferred slab (slices uncapped) for any call
 * tf_conv2d_wgrad accepts, never 0 for a valid call. */
size_t tf_wgrad_det_workspace_bytes(const tf_wgrad_args* a);
int tf_conv2d_wgrad_det(const tf_wgrad_args* a, void* stream);
int tf_wgrad_det_groups(int slices);
/* tf_stem_wgrad in the same form: every block of the grid stores its [64][147] fp32 tile into `slab` (16-byte aligned), the tiles are summed
 * in THE ORDER above (slices = blocks) and added once into dw_oihw.  Preferred slab: the grid tf_stem_wgrad launches; a smaller slab means
 * fewer blocks, below one tile TF_ERR_ARG. */
size_t tf_stem_wgrad_det_workspace_bytes(int N, int H, int W);
int tf_stem_wgrad_det(int dtype, const float* x_nchw, int N, int H, int W, const void* g, const void* x_conv, const float* cA, const float* cB,
                      const float* cD, float* dw_oihw, void* slab, size_t slab_bytes, void* stream);
/* Process-wide switch, like tf_set_stat_rows.  While on: tf_get_stat_rows() reports unfolded rows (plain-store BatchNorm statistics; the
 * rows set with tf_set_stat_rows are kept and come back when the switch goes off) and the executor (tf_detnet_*backward*) takes only the
 * deterministic weight-gradient entries above, with its own arena as the slab.  Same inputs, same weights in -> the same gradient bits out. */
int tf_set_deterministic(int on);
int tf_get_deterministic(void);


/* ---- HBM-bound companions of the conv engine (NHWC, dtype TF_F32 | TF_BF16) ---------- */
/* conv1 (7x7 s2 p3, 3->64; model.py:90): x NCHW fp32 -> im2col [N*OH*OW][ldc], k = c*49+kh*7+kw
 * (the OIHW order of conv1.weight), zero padded to ldc (>= 147, multiple of 8 for every dtype; else TF_ERR_ARG); all ldc columns of every row are written. */
int tf_stem_im2col(const float* x_nchw, int N, int H, int W, int dtype, void* col, int ldc, void* stream);
/* r4: conv1 straight from the NCHW fp32 image, no im2col matrix (dtype TF_BF16 | TF_F16; TF_F32 keeps tf_stem_im2col + tf_conv2d):
 * y [N*OH*OW][64] = conv(x, W) with w_packed = conv1.weight as tf_pack_weight* writes it for the im2col GEMM ([>= 64 rows][ldw],
 * k = c*49 + kh*7 + kw, ldw >= 160 and a multiple of 8).  epi: 0 | TF_EPI_STATS (stat_out[rows][2][64] += per-channel sum and sum of
 * squares of the fp32 results, rows = *host_rows_out <= tf_get_stat_rows(), zero on entry; TF_ERR_UNSUPPORTED with unfolded rows) |
 * TF_EPI_AFFINE|TF_EPI_RELU (y = relu(conv * scale + shift): the folded BatchNorm of the evaluation graph). */
int tf_stem_conv(int dtype, const float* x_nchw, int N, int H, int W, const void* w_packed, int ldw, void* y, int epi,
                 const float* scale, const float* shift, float* stat_out, int* host_rows_out, void* stream);
/* r4: weight gradient of conv1 straight from the image (autograd of model.py:90; dtype TF_BF16 | TF_F16): dw_oihw[64][147] (fp32, the OIHW
 * order of conv1.weight) += sum over output pixels of g[px][co] * patch[px][k]; g [N*OH*OW][64] of `dtype`; dw holds zeros (or what is to be
 * accumulated into) on entry.  Replaces tf_stem_im2col + tf_conv2d_wgrad over the 147-column matrix.  x_conv != NULL (with cA, cB, cD: 64
 * floats each): the gradient operand is  cA * g + cB * x_conv + cD  per channel, rounded to `dtype` -- tf_bn_bwd_apply of the stem's BatchNorm
 * (x_conv = the conv output the statistics were taken of) folded into the kernel, whose output has no other reader. */
int tf_stem_wgrad(int dtype, const float* x_nchw, int N, int H, int W, const void* g, const void* x_conv, const float* cA, const float* cB,
                  const float* cD, float* dw_oihw, void* stream);
/* nn.MaxPool2d(3,2,1) (model.py:93) with the stem's BN+ReLU fused in front when scale/shift are
 * given (training: the un-normalised conv output is read once).  argmax (u8, optional) feeds _bwd. */
int tf_maxpool_fwd(int dtype, const void* x, int N, int H, int W, int C, const float* scale, const float* shift,
                   void* y, uint8_t* argmax, void* stream);
int tf_maxpool_bwd(int dtype, const void* g, const uint8_t* argmax, const void* x, const float* scale, const float* shift,
                   int N, int H, int W, int C, void* gz, void* stream);
/* r4: tf_maxpool_bwd that also takes the column sums of the stem's BatchNorm backward (autograd of model.py:91-93) in the same pass:
 * stat_out[rows][2][C] += (sum gz, sum gz * x), rows = *host_rows_out <= tf_get_stat_rows(), zero on entry -- what
 * tf_colstats(gz, NULL, x) would compute from a second read of both tensors.  TF_ERR_UNSUPPORTED with unfolded rows (tf_set_stat_rows(0)). */
int tf_maxpool_bwd_stats(int dtype, const void* g, const uint8_t* argmax, const void* x, const float* scale, const float* shift,
                         int N, int H, int W, int C, void* gz, float* stat_out, int* host_rows_out, void* stream);
/* per-channel sums over the rows of an [M][ld] matrix, block partials [nblk][nk][C]:
 * k0 = sum g', k1 = sum g'*a, k2 = sum g'*b, g' = g*(y>0) when y != NULL.  nblk = tf_colstats_blocks(). */
int tf_colstats_blocks(int M, int C, int dtype);
int tf_colstats(int dtype, const void* g, const void* y, const void* a, const void* b, int M, int C, int ld,
                float* partial, void* stream);
/* nn.BatchNorm2d in training mode (torchvision Bottleneck / model.py:91): partial (sum, sumsq)
 * -> y = x*scale + shift, saved mean / invstd, running statistics (momentum, unbiased var). */
int tf_bn_finalize(const float* partial, int nblk, int ld, int C, float count, const float* gamma, const float* beta,
                   float eps, float momentum, float* scale, float* shift, float* mean, float* invstd,
                   float* running_mean, float* running_var, int clear, void* stream);
/* eval-mode BN as a per-channel affine (folded into the conv epilogue) */
int tf_bn_fold(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
               int C, float* scale, float* shift, void* stream);
/* BN backward: partial sums (k0 = sum gz, kidx = sum gz*x) -> dgamma, dbeta and g_x = A*gz + B*x + D */
int tf_bn_bwd_finalize(const float* partial, int nblk, int nk, int kidx, int ld, int C, float count, const float* gamma,
                       const float* mean, const float* invstd, float* dgamma, float* dbeta, float* cA, float* cB,
                       float* cD, int clear, void* stream);
int tf_bn_bwd_apply(int dtype, const void* g, const void* y, const void* x, const float* cA, const float* cB,
                    const float* cD, int64_t M, int C, void* out, void* stream);
/* y = relu(x*scale + shift): BN + ReLU materialised for the 3x3 conv's LDS-DMA operand pipeline */
int tf_bn_relu(int dtype, const void* x, const float* scale, const float* shift, int64_t M, int C, void* y, void* stream);
/* Bottleneck output in training mode: y = relu(x*s1+h1 + (r*s2+h2 | r)) */
int tf_bn_add_relu(int dtype, const void* x, const float* s1, const float* h1, const void* r, const float* s2,
                   const float* h2, int64_t M, int C, void* y, void* stream);
/* ---- training-mode BN consumers that finalize the batch statistics in-kernel (no separate finalize launch) ----
 * The producer (tf_conv2d with TF_EPI_STATS/STATS2, tf_colstats) leaves `rows` = tf_get_stat_rows() <= TF_STAT_ROWS
 * partial rows [rows][nk][C] in a region that was zero before it ran; every block re-derives the coefficients of its
 * 64-channel slice; the first row-block of each slice publishes scale/shift/mean/invstd (+ running statistics update)
 * or dgamma/dbeta.  Same arithmetic as tf_bn_finalize / tf_bn_bwd_finalize (torch.nn.BatchNorm2d training semantics of
 * the torchvision trunk built at tinyfaces/models/model.py:17-23).                                                    */
typedef struct tf_bn_fwd_desc {
  const float* stat;                 /* [rows][2][C] sum, sum of squares */
  const float* gamma; const float* beta;
  float* scale; float* shift; float* mean; float* invstd;        /* published */
  float* running_mean; float* running_var;                        /* updated in place (may be NULL) */
  const float* stat_shift;           /* [C] the shift the producer subtracted (tf_conv_args.stat_shift_out); NULL: none */
} tf_bn_fwd_desc;
typedef struct tf_bn_bwd_desc {
  const float* stat;                 /* [rows][nk][C]: k = 0 sum gz, k = kidx sum gz*x */
  const float* gamma; const float* mean; const float* invstd;
  float* dgamma; float* dbeta;       /* published (may be NULL) */
  int nk, kidx;
} tf_bn_bwd_desc;
int tf_bn_relu_fused(int dtype, const void* x, const tf_bn_fwd_desc* bn, int rows, int64_t M, int C, float count,
                     float eps, float momentum, void* y, void* stream);
int tf_bn_add_relu_fused(int dtype, const void* x, const tf_bn_fwd_desc* bn, const void* r, const tf_bn_fwd_desc* bn_r /* NULL: identity */,
                         int rows, int64_t M, int C, float count, float eps, float momentum, void* y, void* stream);
int tf_bn_bwd_apply_fused(int dtype, const void* g, const void* y /* NULL: no ReLU mask */, const void* x, const tf_bn_bwd_desc* bn,
                          int rows, int64_t M, int C, float count, void* out, void* stream);
/* score4_upsample (frozen bilinear ConvTranspose2d k4 s2 p1, model.py:34-40,107) + crop (:110-124)
 * + add (:126); wup_diag [C][4][4] = the channel diagonal of the (C,C,4,4) weight; output NCHW fp32.
 * ldc = row stride (elements) of s3 / s4 / g3 / g4: >= C, a multiple of 4 (fp32) / 8 (bf16, fp16) forward and of 32 backward (TF_ERR_ARG /
 * TF_ERR_UNSUPPORTED otherwise, nothing launched); the backward writes all ldc columns of g3 and g4 (zeros in [C, ldc)). */
int tf_upsample_add_crop(int dtype, const void* s3, const void* s4, const float* wup_diag, int B, int C, int ldc,
                         int H3, int W3, int H4, int W4, float* out_nchw, void* stream);
int tf_upsample_add_crop_bwd(int dtype, const float* g_nchw, const float* wup_diag, int B, int C, int ldc,
                             int H3, int W3, int H4, int W4, void* g3, void* g4, void* stream);
int tf_reduce_partials(const float* partial, int nblk, int nk, int k, int ld, int C, float* out, int clear, void* stream);

/* ---- the detector network as one native graph executor -----------------------------
 * Replaces DetectionModel.forward (tinyfaces/models/model.py:89-128) and its autograd
 * backward (tinyfaces/trainer.py:78,86): ResNet-101 trunk minus layer4, heads, upsample+add
 * (ResNet-50 / ResNet-152 trunks: the tf_detnet_trunk_* forms further below).
 * params / grads: tables of device pointers in tf_detnet_param_name(i) order (fp32, the
 * layouts of the reference state_dict: OIHW conv weights, [C] BN vectors).
 * ws: scratch of tf_detnet_workspace_bytes() bytes, carved deterministically per call; the
 * activations a backward needs live there until tf_detnet_backward is called.            */
int tf_detnet_num_params(void);
const char* tf_detnet_param_name(int i);      /* state_dict key, e.g. "model.layer3.22.bn3.running_var" */
int64_t tf_detnet_param_numel(int i, int num_out);
/* training: 0 = evaluation graph (BN folded into the conv epilogues, no backward), 1 = batch-statistics training graph,
 * 2 = FROZEN BatchNorm (TF_DETNET_FROZEN_BN): the launches of the evaluation forward plus what tf_detnet_backward_frozen_ctx needs (max-pool
 * arg-max, transposed weight operands, per-block gradient buffers); running statistics, gamma and beta are read, never written. */
#define TF_DETNET_FROZEN_BN 2
size_t tf_detnet_workspace_bytes(int dtype, int N, int H, int W, int num_out, int training);
int tf_detnet_out_shape(int H, int W, int* H3, int* W3);
/* flags: TF_DETNET_WEIGHTS_READY (eval only) = the front of `ws` (tf_detnet_param_region_bytes bytes, whose layout depends on
 * dtype/num_out/training but not on N,H,W) still holds the packed weights + folded BN of an earlier eval forward with the
 * SAME parameter values: skip re-packing.  The image pyramid of evaluation.py:49-82 runs 3-5 forwards per image on
 * constant weights; the caller owns the guarantee.                                                                       */
#define TF_DETNET_WEIGHTS_READY 1
size_t tf_detnet_param_region_bytes(int dtype, int num_out, int training);
int tf_detnet_forward(int dtype, int training, const float* x_nchw, int N, int H, int W, int num_out,
                      void* const* params, float bn_eps, float bn_momentum,
                      float* out_nchw, void* ws, size_t ws_bytes, int flags, void* stream);
/* ---- executor context + gradient-ready hooks (r4) ------------------------------------------------------------------------------------
 * tf_detnet_ctx owns what the executor needs beyond `ws`: the second HIP stream of the device it was created on (weight gradients of the
 * backward pass run there, concurrently with the data-gradient chain; the weights of layer 3 are packed there beside the start of a
 * training forward) and its pool of fork / join events.  One context per model (or per thread that drives models): two contexts never
 * share a stream or an event, a context must only be used on the device that was current when it was created.  NULL selects the
 * process-wide default context of the current device (the behaviour of rounds 1-3).
 * tf_detnet_hooks is the data-parallel interface of ONE backward call (the reference has no distributed path; this serves the 8-GPU
 * data-parallel row of SURVEY.md section 8e): when the gradients of all bottlenecks >= blocks[k] (and of the heads) are enqueued
 * (blocks[k] = -1: at the very end, stem included), events[k] -- a hipEvent_t, may be NULL -- is recorded on the stream that carries them
 * and fn(blocks[k], stream, user) is called on the calling thread: work the callee enqueues on `stream` (or orders behind it) sees the
 * bucket final, e.g. tf_comm_allreduce_hook below.  BN gamma / beta gradients of a block are written on the caller's stream BEFORE the
 * fork that precedes the event's stream position, so one event covers them too.  single_stream = 1: no second stream (A/B, race tests). */
typedef struct tf_detnet_ctx tf_detnet_ctx;
int tf_detnet_ctx_create(tf_detnet_ctx** out);       /* binds to the CURRENT device */
int tf_detnet_ctx_destroy(tf_detnet_ctx* ctx);       /* waits for the context's streams, then frees them */
typedef void (*tf_grad_ready_fn)(int block, void* stream, void* user);
typedef struct tf_detnet_hooks {
  const int* blocks; void* const* events; int n;
  tf_grad_ready_fn fn; void* user;
  int single_stream;
} tf_detnet_hooks;
int tf_detnet_forward_ctx(tf_detnet_ctx* ctx, int single_stream, int dtype, int training, const float* x_nchw, int N, int H, int W, int num_out,
                          void* const* params, float bn_eps, float bn_momentum, float* out_nchw, void* ws, size_t ws_bytes, int flags, void* stream);
/* grad_flat (optional): when every entry of `grads` lies inside [grad_flat, grad_flat + grad_flat_bytes) the ranges that are accumulated
 * into are zeroed with at most two memsets instead of one per weight gradient. */
int tf_detnet_backward_ctx(tf_detnet_ctx* ctx, const tf_detnet_hooks* hooks /* NULL: none */, int dtype, const float* x_nchw, int N, int H, int W,
                           int num_out, void* const* params, void* const* grads, const float* gout_nchw,
                           void* grad_flat, size_t grad_flat_bytes, void* ws, size_t ws_bytes, void* stream);
/* Context-free forms of rounds 1-3, kept for callers that drive ONE model from ONE thread: they use the default context of the current
 * device and hooks registered PROCESS-WIDE with the three setters below (not thread-safe; the Python surface no longer uses them). */
int tf_detnet_set_dual_stream(int on);               /* 1 (default): second stream; 0: everything on the caller's stream */
int tf_detnet_set_grad_events(const int* blocks, void* const* events, int n);      /* n = 0 clears */
int tf_detnet_set_grad_callback(tf_grad_ready_fn fn, void* user);                  /* NULL: off */
int tf_detnet_backward(int dtype, const float* x_nchw, int N, int H, int W, int num_out,
                       void* const* params, void* const* grads, const float* gout_nchw,
                       void* grad_flat, size_t grad_flat_bytes,
                       void* ws, size_t ws_bytes, void* stream);
/* ---- trunk-aware forms (version 610) -------------------------------------------------------------------------------------------------
 * The entry points above describe ONE network: the ResNet-101 trunk.  The forms below take the trunk as its Bottleneck block counts in
 * layers 1-3, blocks[3]: {3, 4, 6} (torchvision resnet50), {3, 4, 23} (resnet101) or {3, 8, 36} (resnet152); blocks = NULL means
 * {3, 4, 23}.  Every other argument, the parameter table order (stem, the bottlenecks in order, heads, upsample) and every error code are
 * those of the form without `trunk_`; with blocks = {3, 4, 23} or NULL they are the same call.  Another block count: the queries return
 * TF_ERR_UNSUPPORTED (num_params, param_numel), NULL (param_name) or 0 (the byte counts), the passes TF_ERR_UNSUPPORTED.
 * tf_detnet_trunk_param_name's pointers stay valid for the life of the process (one table per trunk, built once, thread-safe). */
int tf_detnet_trunk_num_params(const int* blocks);                 /* resnet50 220, resnet101 475, resnet152 730 */
const char* tf_detnet_trunk_param_name(const int* blocks, int i);
int64_t tf_detnet_trunk_param_numel(const int* blocks, int i, int num_out);
size_t tf_detnet_trunk_workspace_bytes(const int* blocks, int dtype, int N, int H, int W, int num_out, int training);
size_t tf_detnet_trunk_param_region_bytes(const int* blocks, int dtype, int num_out, int training);
int tf_detnet_trunk_forward_ctx(const int* blocks, tf_detnet_ctx* ctx, int single_stream, int dtype, int training, const float* x_nchw, int N, int H,
                                int W, int num_out, void* const* params, float bn_eps, float bn_momentum, float* out_nchw, void* ws, size_t ws_bytes,
                                int flags, void* stream);
int tf_detnet_trunk_backward_ctx(const int* blocks, tf_detnet_ctx* ctx, const tf_detnet_hooks* hooks, int dtype, const float* x_nchw, int N, int H,
                                 int W, int num_out, void* const* params, void* const* grads, const float* gout_nchw, void* grad_flat,
                                 size_t grad_flat_bytes, void* ws, size_t ws_bytes, void* stream);
/* ---- frozen BatchNorm (fine-tuning on the pretrained statistics) ----------------------------------------------------------------------
 * The backward pass of a forward run with training = TF_DETNET_FROZEN_BN: autograd of tinyfaces/trainer.py:86 over model.py:89-128 with
 * every BatchNorm2d of the trunk in eval() mode and its parameters requires_grad = False (torchvision's FrozenBatchNorm2d).  Every BN is
 * the constant map v -> v * s + h (tf_bn_fold), so a bottleneck's chain is its three data-gradient convs: the scale of bn1 / bn2 rides in
 * the epilogue of the data gradient above it (TF_EPI_AFFINE | TF_EPI_MASK, the stored post-ReLU activation is its own mask), the scale of
 * bn3 / the downsample BN in the transposed packed operand (tf_pack2_job.scale_t) and in the weight-gradient rows (tf_wgrad_args.row_scale).
 * Same arguments, hooks, streams and error codes as tf_detnet_trunk_backward_ctx; the conv weights, head weights and head biases receive
 * their gradients, the entries of `grads` that belong to BN gamma / beta are left untouched except inside the range of grad_flat that the
 * split memset skips, where they are zeroed. */
int tf_detnet_trunk_backward_frozen_ctx(const int* blocks, tf_detnet_ctx* ctx, const tf_detnet_hooks* hooks, int dtype, const float* x_nchw, int N,
                                        int H, int W, int num_out, void* const* params, void* const* grads, const float* gout_nchw,
                                        void* grad_flat, size_t grad_flat_bytes, void* ws, size_t ws_bytes, void* stream);
int tf_detnet_backward_frozen_ctx(tf_detnet_ctx* ctx, const tf_detnet_hooks* hooks, int dtype, const float* x_nchw, int N, int H, int W,
                                  int num_out, void* const* params, void* const* grads, const float* gout_nchw,
                                  void* grad_flat, size_t grad_flat_bytes, void* ws, size_t ws_bytes, void* stream);
/* ---- partial freeze (version 630): the frozen-BN backward cut at a stage boundary ------------------------------------------------------
 * tf_detnet_trunk_backward_frozen_ctx with the stem and the lowest stages of the trunk frozen as well (torchvision's
 * trainable_backbone_layers, Detectron's FREEZE_AT): autograd as above with, in addition, requires_grad = False on every parameter below
 * the cut.  first_block = the index of the lowest bottleneck that receives weight gradients:
 *   -1 the stem too (the call above, launch for launch) | 0 layer 1 and up | n1 layer 2 and up | n1 + n2 layer 3 and up |
 *   n1 + n2 + n3 the two heads only        (blocks = {n1, n2, n3}; ResNet-101: -1, 0, 3, 7, 30)
 * Any other value is TF_ERR_ARG before anything is launched (a cut inside a stage is not taken).  The forward is the same
 * training = TF_DETNET_FROZEN_BN forward with the same workspace; the pass launches a strict subset of the full pass: nothing below block
 * first_block, no input gradient of that block, no max-pool backward or stem weight gradient, and no head data gradient without a reader.
 * Writes: the conv weights of the blocks >= first_block, the head weights and biases and score4_upsample.weight (zero) receive their
 * gradients.  The tensors below the cut have NO writer, like BN gamma / beta: inside grad_flat their slots are zero after the call (the
 * memset covers them; the split memset is only taken while layer 3 is trained), entries of `grads` outside grad_flat are left untouched
 * and may be NULL there.
 * Hooks: every registered hook still fires exactly once.  Those of the blocks >= first_block fire where they always do; those of the
 * blocks below the cut, in the order they were registered, and then the -1 hook fire at the end of the shortened pass on the caller's
 * stream, behind the join with the weight-gradient stream and behind the memset of their (all-zero) ranges. */
int tf_detnet_trunk_backward_frozen_from_ctx(const int* blocks, tf_detnet_ctx* ctx, const tf_detnet_hooks* hooks, int dtype, const float* x_nchw,
                                             int N, int H, int W, int num_out, void* const* params, void* const* grads, const float* gout_nchw,
                                             void* grad_flat, size_t grad_flat_bytes, void* ws, size_t ws_bytes, void* stream, int first_block);

/* ---- gradient exchange of the data-parallel path over RCCL (the reference has no distributed code) -------------
 * One process per GPU; the gradients are SUMMED over the ranks bucket by bucket while the backward pass runs, the 1/world goes into
 * tf_sgd_step's grad_scale.  librccl.so is resolved at run time (the copy already mapped into the process first): tf_comm_available() == 0
 * on a host without it, and every other entry then returns TF_ERR_UNSUPPORTED.
 *   tf_comm_unique_id  rank 0 draws the 128-byte identifier of a new communicator (HOST memory); ship it to the other ranks out of band
 *   tf_comm_init       collective over all ranks; binds to the CURRENT device; owns a communication stream (default priority) + events
 *   tf_allreduce_bucket  buf[0..n) <- sum over ranks, in place, on the communicator's stream, ordered behind the current tail of `after`
 *                        (the executor stream that carries the bucket: tf_detnet_hooks) without holding that stream up
 *   tf_comm_join       `stream` waits for every collective issued so far (call it on the training stream before tf_sgd_step)
 *   tf_comm_allreduce_hook  a ready-made tf_grad_ready_fn: tf_detnet_hooks.fn = tf_comm_allreduce_hook, .user = a tf_comm_plan that maps
 *                        the registered blocks to element ranges of the flat gradient; plan.rc keeps the first error, plan.issued counts,
 *                        plan.status[k] says which buckets were issued (a caller with another exchange at hand reduces the others itself) */
#define TF_COMM_ID_BYTES 128
typedef struct tf_comm tf_comm;
int tf_comm_available(void);
int tf_comm_unique_id(void* host_id_out /*[TF_COMM_ID_BYTES]*/);
int tf_comm_init(const void* host_id /*[TF_COMM_ID_BYTES]*/, int rank, int world, tf_comm** out);
int tf_comm_destroy(tf_comm* comm);
int tf_comm_rank(const tf_comm* comm);
int tf_comm_world(const tf_comm* comm);
int tf_allreduce_bucket(tf_comm* comm, float* buf, size_t n, void* after_stream);
int tf_comm_join(tf_comm* comm, void* stream);
typedef struct tf_comm_plan {
  void* comm;                    /* tf_comm* */
  float* grad_flat;              /* the flat fp32 gradient the buckets are slices of */
  int n; const int* blocks;      /* the blocks registered in tf_detnet_hooks (backward order; -1 = the end of the pass) */
  const int64_t* start; const int64_t* end;      /* element range of bucket k */
  int rc, issued;                /* out: first error (TF_OK), collectives issued since the caller reset it */
  int* status;                   /* r6, optional [n], out: 1 = bucket k's collective was issued, < 0 = its error code, untouched = hook not reached */
} tf_comm_plan;
void tf_comm_allreduce_hook(int block, void* stream, void* user /* tf_comm_plan* */);

/* ---- image preparation in front of the detector -----------------------------------
 * One pass from the decoded uint8 RGB image to the normalised fp32 CHW tensor: PIL BILINEAR resize (bit-exact with Pillow's
 * 8-bit two-pass resample; tinyfaces/datasets/wider_face.py:136-146 and tinyfaces/evaluation.py:46 through
 * torchvision.transforms.functional.resize), crop + paste on the mean colour (tinyfaces/datasets/processor.py:41-76),
 * horizontal flip (tinyfaces/datasets/wider_face.py:155-157), ToTensor + Normalize (main.py:44-46).  Only the pixels of the
 * window are resampled.  Training: OH = OW = 500; evaluation: crop = the whole resized image, paste (0,0), OH x OW = RH x RW. */
typedef struct tf_image_prepare_args {
  const unsigned char* img;              /* device, [H][W][3] uint8 */
  int H, W;                              /* decoded size */
  int RH, RW;                            /* size after the resize (== H, W: no resize) */
  int crop_y, crop_x, crop_h, crop_w;    /* window of the RESIZED image */
  int paste_y, paste_x;                  /* top-left corner of the window in the output */
  int flip;                              /* 1: the finished buffer is mirrored (np.fliplr) */
  int OH, OW;                            /* output size */
  float mean[3], std[3];                 /* Normalize */
  unsigned char bg[3];                   /* colour outside the window: (mean * 255) truncated = 123, 116, 103 */
  float* out;                            /* device, fp32 [3][OH][OW] */
} tf_image_prepare_args;
int tf_image_prepare(const tf_image_prepare_args* a, void* stream);

/* ---- f1: colour jitter between the augmented uint8 image and ToTensor + Normalize ---------------------------------------
 * torchvision.transforms.ColorJitter acting on the PIL image that the reference's process_inputs returns (the pasted, flipped
 * OH x OW image, mean-colour padding included), i.e. Pillow's ImageEnhance plus an HSV round trip, restated in integers and
 * float32 (tests/color_jitter_ref.py is the same arithmetic in numpy, pinned to Pillow by tests/test_color_jitter.py).
 * Every op maps a uint8 RGB image to a uint8 RGB image; f32(.) rounds to float32, nothing is contracted into an FMA:
 *   blend(d, x, f)   t = f32(d) + f32(f) * (f32(x) - f32(d)); 0 <= f <= 1: t truncated; else 0 if t <= 0, 255 if t >= 255, else t truncated
 *   L(r, g, b)       (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16
 *   brightness(f)    blend(0, x, f)
 *   saturation(f)    blend(L(pixel), x, f) on the three channels
 *   contrast(f)      blend(m, x, f), m = (2 S + n) / (2 n) in integers (= floor(S / n + 0.5)), S = the sum of L over the n = OH * OW
 *                    pixels of the image as it stands at that point of the chain
 *   hue(shift)       RGB -> HSV (Pillow's rgb2hsv: float32 s and rc / gc / bc, h through double), h = (h + shift) & 255, HSV -> RGB
 *                    (Pillow's hsv2rgb, evaluated in DOUBLE here: fh = h * 6.0 / 255.0, fs = s / 255.0, floor(x + 0.5) rounding).
 *                    A shift of 0 still makes the round trip, which is not the identity.
 * op[i] is one of TF_JITTER_*, each kind at most once, applied in the order given; factor[i] >= 0 is the enhancement factor, for
 * TF_JITTER_HUE the integer shift 0 ... 255.  n_ops = 0 runs the plain pass.
 * Launches: a chain without contrast is ONE launch (resample, the chain in registers, normalise; `ws` is not touched and may be NULL).
 * A chain with contrast is TWO: the first applies the ops in front of contrast, writes the uint8 image to `ws` and one integer partial
 * sum of L per block; the second sums the partials (integers: no order dependence), applies contrast and the rest, normalises.
 * No memset, no atomics, no host sync: the first launch writes every word the second reads.
 * Workspace: tf_image_prepare_jitter_workspace_bytes(OH, OW, n_ops, op) = 0 without contrast, else
 *   round_up(4 * ceil(OW / 64) * ceil(OH / 4), 256) + 3 * OH * OW.
 * Refused before anything is enqueued (TF_ERR_ARG; TF_ERR_WORKSPACE for a workspace that is too small): what tf_image_prepare refuses,
 * n_ops outside 0 ... 4, an unknown or repeated kind, a negative or non-finite factor, a hue shift that is no integer in 0 ... 255,
 * OH * OW > 2^24 (the bound up to which the integer mean equals Pillow's double form). */
#define TF_JITTER_BRIGHTNESS 0
#define TF_JITTER_CONTRAST 1
#define TF_JITTER_SATURATION 2
#define TF_JITTER_HUE 3
size_t tf_image_prepare_jitter_workspace_bytes(int OH, int OW, int n_ops, const int* op);
int tf_image_prepare_jitter(const tf_image_prepare_args* a, int n_ops, const int* op /*[n_ops]*/, const float* factor /*[n_ops]*/,
                            void* ws, size_t ws_bytes, void* stream);

/* ---- measurement hooks (bench.py `roofline`) ------------------------------------------
 * While enabled, every MFMA kernel launch (conv_igemm / wgrad) is bracketed by HIP events on
 * the stream it is launched on.  tf_profile_collect blocks until they completed and writes
 * rows of 6 doubles to HOST memory: kind, launches, total_ms, ALGORITHMIC flops (2 x the MACs of the
 * forward convolution the launch belongs to, unpadded channels: a stride-2 data gradient counts the
 * forward conv's MACs, not the zero-inserted gather it executes), algorithmic bytes, EXECUTED flops
 * (2*M*N*K of the GEMM the kernel ran, padding and zero taps included).  kind 0..5 = conv_igemm (dtype*3 + tile-1), 8..11 = wgrad (8 + dtype*2 + (tile==128)),
 * 12/13/15 = conv_dma f32/bf16/f16, 14 = wgrad_dma bf16, 6/7 = conv3x3h bf16/f16, 16 = wgrad3x3 bf16 (both launches of its two-phase form), 17 = retired (conv_pwx, a removed kernel: not reused),
 * 18 / 19 = the grouped pointwise / 3x3 weight gradients (tf_conv2d_wgrad_group: flops and bytes of the whole group). */
int tf_profile_enable(int every);   /* 0 = off, 1 = bracket every launch, n = every n-th launch (sampling keeps the timed region undisturbed) */
int tf_profile_collect(double* host_out, int max_rows);
/* per layer shape, for the records consumed by the LAST tf_profile_collect: rows of 12 doubles
 * (kind, M pixels, N output channels, K reduction length, taps, mode (0 fwd, 1 dgrad, 2 wgrad), epilogue flags, launches, total_ms,
 *  algorithmic flops, algorithmic bytes, executed flops) */
int tf_profile_shapes(double* host_out, int max_rows);
/* (r4: the debugging / measurement probes -- tf_debug_conv3x3h_trace, tf_debug_probe, tf_debug_probe_chain, tf_probe_tr16 -- are not part of
 * this ABI any more: tiny-faces-pytorch_amd/csrc/debug_api.h, bound by the test-suite and scripts/ only.) */

#ifdef __cplusplus
}
#endif
#endif /* TINYFACES_HIP_H */
