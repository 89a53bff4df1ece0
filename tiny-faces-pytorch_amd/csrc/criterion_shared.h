// What the passes of the detection criterion share: csrc/criterion.hip (soft-margin and focal forms), csrc/criterion_quality.hip (quality
// focal form) and csrc/criterion_aligned.hip (task-aligned form).  The block geometry, the parameter block of the focal-shaped passes, the
// overlap term of one positive (box_term), the weight of the quality focal forms (qfl_weight), the per-block count of +1 labels
// (focal_count_kernel) and the per-image total every block forms from it (focal_image_npos).  Everything sits in an
// anonymous namespace: each translation unit gets its own copy of the kernels, and nothing here leaves the library.
#pragma once
#include <cmath>

#include "common.h"

namespace {

constexpr int EPB = 1024;   // elements per block (4 per thread, 256-strided => coalesced)

size_t a256(size_t x) { return (x + 255) & ~(size_t)255; }

struct FocalParams {
  const float* out; const float* cls; const float* reg;
  int B, E, nblk;
  float gamma, alpha; int normalize; float reg_weight;
  float* grad; double* loss; int* npos_out;
  double* partial;        // [B][nblk][2]
  int* blkpos;            // [B][nblk]
  const float* twh;       // [nt][2] template (dw, dh): the DIoU form only
  int HW;                 // elements per template: e / HW is the template of element e
};

// Overlap forms of the regression term (tf_criterion_focal_box_fwd_bwd; the definition is in include/tinyfaces_hip.h).  In the anchor's
// template-normalised frame the prediction is the box with centre (px, py) and size (e^pw, e^ph), pw / ph clamped to [-C, C], the target the
// same from t; IoU and GIoU do not change under a per-axis scaling, DIoU needs the template's aspect a = dw / dh.  One term per positive.
enum { REG_SMOOTH_L1 = 0, REG_IOU = 1, REG_GIOU = 2, REG_DIOU = 3 };
constexpr float BOX_CLIP = 4.135166556742356f;     // log(1000 / 16), torchvision's bbox_xform_clip

// -> the term; g[0..3] = its derivatives with respect to px, py, pw, ph.  All areas are > 0 under the clamp: no epsilon.  On a kink (two edges
// tie, iw or ih exactly 0, |pw| or |ph| exactly C) the one-sided choice below is taken: finite.
template <int REG>
__device__ __forceinline__ float box_term(float px, float py, float pw, float ph, float tx, float ty, float tw, float th, float a, float* g) {
  const float mw = (pw >= -BOX_CLIP && pw <= BOX_CLIP) ? 1.f : 0.f, mh = (ph >= -BOX_CLIP && ph <= BOX_CLIP) ? 1.f : 0.f;   // torch.clamp's gradient
  const float hwp = 0.5f * expf(fminf(fmaxf(pw, -BOX_CLIP), BOX_CLIP)), hhp = 0.5f * expf(fminf(fmaxf(ph, -BOX_CLIP), BOX_CLIP));
  const float hwt = 0.5f * expf(tw), hht = 0.5f * expf(th);
  // The edges enter only through their differences, taken from the centre offset and the half sizes so that nothing is lost to the size of
  // the centres themselves: x2p - x2t = dx + (hwp - hwt), x1p - x1t = dx - (hwp - hwt), and for two intervals of half widths u, v whose centres
  // are d apart  min(x2) - max(x1) = min(2u, 2v, u + v - |d|),  max(x2) - min(x1) = max(2u, 2v, u + v + |d|).  Equal boxes give exactly 0.
  const float dx = px - tx, dy = py - ty;
  const float rx2 = dx + (hwp - hwt), rx1 = dx - (hwp - hwt), ry2 = dy + (hhp - hht), ry1 = dy - (hhp - hht);
  const float iwr = fminf(2.f * fminf(hwp, hwt), hwp + hwt - fabsf(dx)), ihr = fminf(2.f * fminf(hhp, hht), hhp + hht - fabsf(dy));
  const float iw = fmaxf(iwr, 0.f), ih = fmaxf(ihr, 0.f);
  const float cw = fmaxf(2.f * fmaxf(hwp, hwt), hwp + hwt + fabsf(dx)), ch = fmaxf(2.f * fmaxf(hhp, hht), hhp + hht + fabsf(dy));
  const float ap = 4.f * hwp * hhp, at = 4.f * hwt * hht;
  const float I = iw * ih, U = ap + at - I, rU = 1.f / U, iou = I * rU;
  // d iw / d (px, pw) and d ih / d (py, ph): which of the prediction's edges bound the intersection
  const float ox = iwr > 0.f ? 1.f : 0.f, oy = ihr > 0.f ? 1.f : 0.f;
  const float ix2 = rx2 < 0.f ? ox : 0.f, ix1 = rx1 > 0.f ? ox : 0.f, iy2 = ry2 < 0.f ? oy : 0.f, iy1 = ry1 > 0.f ? oy : 0.f;
  const float dI[4] = {ih * (ix2 - ix1), iw * (iy2 - iy1), ih * hwp * (ix2 + ix1), iw * hhp * (iy2 + iy1)};
  const float dU[4] = {-dI[0], -dI[1], ap - dI[2], ap - dI[3]};
  float term = (U - I) * rU;                                          // 1 - IoU
#pragma unroll
  for (int k = 0; k < 4; ++k) g[k] = -(dI[k] - iou * dU[k]) * rU;
  if (REG == REG_GIOU || REG == REG_DIOU) {
    // ... and which bound the enclosing box
    const float ex2 = rx2 > 0.f ? 1.f : 0.f, ex1 = rx1 < 0.f ? 1.f : 0.f, ey2 = ry2 > 0.f ? 1.f : 0.f, ey1 = ry1 < 0.f ? 1.f : 0.f;
    const float dcw[4] = {ex2 - ex1, 0.f, hwp * (ex2 + ex1), 0.f}, dch[4] = {0.f, ey2 - ey1, 0.f, hhp * (ey2 + ey1)};
    if (REG == REG_GIOU) {
      const float Cb = cw * ch, rC = 1.f / Cb, uc = U * rC;
      term += (Cb - U) * rC;
#pragma unroll
      for (int k = 0; k < 4; ++k) g[k] -= (dU[k] - uc * (ch * dcw[k] + cw * dch[k])) * rC;
    } else {
      const float a2 = a * a;
      const float N = a2 * dx * dx + dy * dy, D = a2 * cw * cw + ch * ch, rD = 1.f / D, R = N * rD;
      const float dN[4] = {2.f * a2 * dx, 2.f * dy, 0.f, 0.f};
      term += R;
#pragma unroll
      for (int k = 0; k < 4; ++k) g[k] += (dN[k] - R * 2.f * (a2 * cw * dcw[k] + ch * dch[k])) * rD;
    }
  }
  g[2] *= mw; g[3] *= mh;
  return term;
}

// The weight of the quality focal forms (csrc/criterion_quality.hip, csrc/criterion_aligned.hip), d = sigma - q:
// |d|^beta and beta |d|^(beta - 1) sgn(d); beta = 2 takes no powf, any other beta ONE: |d|^beta = |d|^(beta - 1) |d| (every labelled element
// pays for it, and a second powf made the pass 1.3 times the focal one).  beta >= 1, so the exponent is not negative: finite at d = 0, where
// both are 0 (sgn(0) = 0, also for beta = 1 where powf(0, 0) = 1).
__device__ __forceinline__ void qfl_weight(float d, float beta, float& w, float& dw) {
  if (beta == 2.f) { w = d * d; dw = 2.f * d; return; }
  const float ad = fabsf(d), sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  const float w1 = powf(ad, beta - 1.f);
  w = w1 * ad;
  dw = beta * w1 * sg;
}

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// the +1 labels of image b, from the per-block counts: every thread of the (256-thread) block returns the total
__device__ __forceinline__ int focal_image_npos(const FocalParams& p, int b, int* wn /*[4], shared*/) {
  int n = 0;
  for (int i = threadIdx.x; i < p.nblk; i += 256) n += p.blkpos[(size_t)b * p.nblk + i];
  n = wave_sum_int(n);
  if ((threadIdx.x & 63) == 0) wn[threadIdx.x >> 6] = n;
  __syncthreads();
  return wn[0] + wn[1] + wn[2] + wn[3];
}

__global__ void __launch_bounds__(256) focal_count_kernel(FocalParams p) {
  const int b = blockIdx.y, blk = blockIdx.x;
  __shared__ int wn[4];
  int n = 0;
#pragma unroll
  for (int k = 0; k < EPB / 256; ++k) {
    const int e = blk * EPB + k * 256 + threadIdx.x;
    const bool isp = e < p.E && p.cls[(size_t)b * p.E + e] == 1.f;
    n += __popcll(__ballot(isp));
  }
  if ((threadIdx.x & 63) == 0) wn[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) p.blkpos[(size_t)b * p.nblk + blk] = wn[0] + wn[1] + wn[2] + wn[3];
}

}  // namespace
