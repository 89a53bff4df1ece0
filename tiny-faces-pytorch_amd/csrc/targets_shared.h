// What the target-assignment files share: csrc/targets.hip (dense_overlap and its compensation stage), csrc/targets_ignore.hip (the ignore
// pass) csrc/targets_atss.hip (ATSS) and csrc/targets_tal.hip (TAL).  The float64 geometry of one anchor (anchor_at) is defined HERE and nowhere else: the three files
// agree bit for bit on every anchor because they call it, not because they restate it.  Next to it the lookup of the image that owns a box
// (image_of) and the operand block both entry points of csrc/targets.hip fill (TgtParams, base_params).  Everything sits in an anonymous
// namespace: each translation unit gets its own copy, and nothing here leaves the library.
// The including files are compiled with -ffp-contract=off (build.py EXACT): every f64 op must round exactly like numpy's.
#pragma once
#include "common.h"

namespace {

// the anchor of template (dx1, dy1, dx2, dy2) at cell (y, x): corners, width, height and area in dense_overlap.py:32-52's operation order
struct Anchor { double x1, y1, x2, y2, fw, fh, farea; };

__device__ __forceinline__ Anchor anchor_at(double dx1, double dy1, double dx2, double dy2, int ofy, int ofx, int sty, int stx, int y, int x) {
  const double cx = (double)ofx + (double)x * ((double)stx / 1.0);     // dense_overlap.py:50
  const double cy = (double)ofy + (double)y * ((double)sty / 1.0);
  Anchor a;
  a.x1 = dx1 + cx; a.y1 = dy1 + cy; a.x2 = dx2 + cx; a.y2 = dy2 + cy;
  a.fh = dy2 - dy1 + 1.0; a.fw = dx2 - dx1 + 1.0;
  a.farea = a.fw * a.fh;
  return a;
}

// ---- the unpadded cells of a template and the distance of an anchor centre to a face centre: csrc/targets_atss.hip and csrc/targets_tal.hip
// the two halves of get_padding's predicate along one axis, as pad_at of csrc/targets.hip forms them: c = of + i * st in int32, then double
__device__ __forceinline__ bool pad_lo(int of, int st, int i, double d1, int lim) { return (double)(of + i * st) + d1 < (double)(lim + 1); }
__device__ __forceinline__ bool pad_hi(int of, int st, int i, double d2, int lim) { return (double)(of + i * st) + d2 > (double)lim; }

__device__ __forceinline__ int clamp_to_int(double v, int lo, int hi) {          // (a NaN goes to lo)
  return v >= (double)hi ? hi : (v > (double)lo ? (int)v : lo);
}

// [lo, hi] = the indices i in [0, n) with neither half of the predicate set (empty: lo > hi)
__device__ __forceinline__ void unpadded_range(int of, int st, int n, double d1, double d2, int lim_lo, int lim_hi, int& lo, int& hi) {
  lo = clamp_to_int(ceil(((double)(lim_lo + 1) - d1 - (double)of) / (double)st), 0, n);
  while (lo > 0 && !pad_lo(of, st, lo - 1, d1, lim_lo)) --lo;
  while (lo < n && pad_lo(of, st, lo, d1, lim_lo)) ++lo;
  hi = clamp_to_int(floor(((double)lim_hi - d2 - (double)of) / (double)st), -1, n - 1);
  while (hi < n - 1 && !pad_hi(of, st, hi + 1, d2, lim_hi)) ++hi;
  while (hi >= 0 && pad_hi(of, st, hi, d2, lim_hi)) --hi;
}

// the anchor centre along one axis: ((d1 + c) + (d2 + c)) / 2 with c = of + i * st as targets_kernel forms it
__device__ __forceinline__ double centre(int of, int st, int i, double d1, double d2) {
  const double c = (double)of + (double)i * ((double)st / 1.0);
  return ((d1 + c) + (d2 + c)) / 2.0;
}
__device__ __forceinline__ double sqdist(int of, int st, int i, double d1, double d2, double fc) {
  const double d = centre(of, st, i, d1, d2) - fc;
  return d * d;
}

// first index of the w (<= hi - lo + 1) indices of [lo, hi] nearest to fc: squared distance ascending, the lower index on a tie
__device__ __forceinline__ int nearest_window(int of, int st, int lo, int hi, int w, double d1, double d2, double fc) {
  int c0 = clamp_to_int(floor((fc - (d1 + d2) / 2.0 - (double)of) / (double)st) - (double)(w / 2), lo, hi - w + 1);
  while (c0 > lo && sqdist(of, st, c0 - 1, d1, d2, fc) <= sqdist(of, st, c0 + w - 1, d1, d2, fc)) --c0;
  while (c0 + w <= hi && sqdist(of, st, c0 + w, d1, d2, fc) < sqdist(of, st, c0, d1, d2, fc)) ++c0;
  return c0;
}

// which image owns box gi of the concatenated list (box_off: B + 1 ascending offsets, gi < box_off[B])
__device__ __forceinline__ int image_of(const int32_t* box_off, int gi) {
  int b = 0;
  while (box_off[b + 1] <= gi) ++b;
  return b;
}

struct TgtParams {
  const double* boxes; const int32_t* box_off; const double* tpl; int nt, tstride;
  int vsy, vsx, ofy, ofx, sty, stx;
  const int32_t* paste; const int32_t* flips;
  const double* noise; const int64_t* noise_off; uint64_t seed;
  double pos_thresh, neg_thresh;
  float* cls; float* reg;
  unsigned long long* gmax; unsigned int* gidx;
};

// the argument checks tf_dense_overlap_targets and tf_dense_overlap_targets_comp share, then their operands -> p (gmax / gidx are
// carved out of the workspace by the caller).  TF_OK or TF_ERR_ARG.
inline int base_params(TgtParams& p, const double* boxes, const int32_t* box_offsets, int B, const double* templates, int nt, int tstride,
                       int vsy, int vsx, int ofy, int ofx, int sty, int stx, const int32_t* paste_boxes, const int32_t* flips,
                       const double* noise, const int64_t* noise_offsets, uint64_t seed, double pos_thresh, double neg_thresh,
                       float* class_map, float* reg_map) {
  if (B <= 0 || nt <= 0 || vsy <= 0 || vsx <= 0 || !box_offsets || !templates || !class_map || !reg_map) return TF_ERR_ARG;
  if (noise && !noise_offsets) return TF_ERR_ARG;
  p.boxes = boxes; p.box_off = box_offsets; p.tpl = templates; p.nt = nt; p.tstride = tstride;
  p.vsy = vsy; p.vsx = vsx; p.ofy = ofy; p.ofx = ofx; p.sty = sty; p.stx = stx;
  p.paste = paste_boxes; p.flips = flips; p.noise = noise; p.noise_off = noise_offsets; p.seed = seed;
  p.pos_thresh = pos_thresh; p.neg_thresh = neg_thresh; p.cls = class_map; p.reg = reg_map;
  return TF_OK;
}

}  // namespace
