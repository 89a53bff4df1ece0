// Ignore regions of the training targets (the rule: include/tinyfaces_hip.h, "ignore regions"; numpy restatement: tests/ignore_ref.py).
// One pass behind tf_dense_overlap_targets[_comp] over the [B][nt][vsy][vsx] float class map, in place: a NEGATIVE anchor (label -1) that
// an ignore box of its image covers by at least `thresh` gets the don't-care label 0.  Labels +1 and 0 are never touched, the regression
// map is not an operand.  The anchor it tests is anchor_at of csrc/targets_shared.h, the single definition csrc/targets.hip and
// csrc/targets_atss.hip use too, so an anchor has the same corners and area in all three files; the rest of the pass is this file's own.
// Compiled with -ffp-contract=off (build.py EXACT): every f64 op must round exactly like numpy's.
//
// One thread per (t, y, x) anchor, x fastest, 256 per block, grid (ceil(nt * cells / 256), B): targets_kernel's own geometry, so the map is
// read (and, where a label turns, written) coalesced.  A block whose image has no ignore boxes leaves before it loads anything of the map.
// The image's boxes go through LDS in tiles of kTile as corners + area (the area is computed once per tile, 10 KiB), so their number is not
// bounded by LDS; inside a tile every lane reads the same LDS word (a broadcast).  A lane whose label is not -1 only takes part in the
// barriers; a lane stops testing at its first covering box.  `changed[b]` (optional) adds the labels turned: ballot + popcount, one integer
// atomic per wave that turned any.  No floating-point atomic, no grid barrier, no host synchronisation: the same bits on every run.
#include "targets_shared.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 256;                        // ignore boxes per LDS tile: 5 doubles each

template <int MEASURE>
__global__ void __launch_bounds__(kThreads) targets_ignore_kernel(float* __restrict__ cls, int nt, int vsy, int vsx,
                                                                  const double* __restrict__ tpl, int tstride,
                                                                  int ofy, int ofx, int sty, int stx,
                                                                  const double* __restrict__ ign, const int32_t* __restrict__ ign_off,
                                                                  double thresh, int32_t* __restrict__ changed) {
  __shared__ double rx1[kTile], ry1[kTile], rx2[kTile], ry2[kTile], ra[kTile];
  const int b = blockIdx.y;
  const int k0 = ign_off[b], K = ign_off[b + 1] - k0;
  if (K <= 0) return;                                                  // block-uniform: nothing of the map is loaded
  const int cells = vsy * vsx;
  const int idx = blockIdx.x * kThreads + threadIdx.x;                 // (t, y, x), x fastest
  const bool active = idx < nt * cells;
  const int t = active ? idx / cells : 0;
  const int cell = active ? idx - t * cells : 0;
  const int y = cell / vsx, x = cell - y * vsx;
  const double* tp = tpl + (size_t)t * tstride;
  const double dx1 = tp[0], dy1 = tp[1], dx2 = tp[2], dy2 = tp[3];
  const Anchor an = anchor_at(dx1, dy1, dx2, dy2, ofy, ofx, sty, stx, y, x);
  float* label = cls + (size_t)b * nt * cells + idx;
  const bool negative = active && *label == -1.f;

  bool covered = false;
  for (int j0 = 0; j0 < K; j0 += kTile) {                              // block-uniform trip count
    const int m = min(kTile, K - j0);
    __syncthreads();                                                   // the previous tile's readers are done
    if ((int)threadIdx.x < m) {
      const double* r = ign + 4 * (size_t)(k0 + j0 + threadIdx.x);
      const double x1 = r[0], y1 = r[1], x2 = r[2], y2 = r[3];
      rx1[threadIdx.x] = x1; ry1[threadIdx.x] = y1; rx2[threadIdx.x] = x2; ry2[threadIdx.x] = y2;
      ra[threadIdx.x] = (x2 - x1 + 1.0) * (y2 - y1 + 1.0);
    }
    __syncthreads();
    if (negative && !covered) {
      for (int j = 0; j < m; ++j) {
        const double iw = fmin(an.x2, rx2[j]) - fmax(an.x1, rx1[j]) + 1.0;
        const double ih = fmin(an.y2, ry2[j]) - fmax(an.y1, ry1[j]) + 1.0;
        if (iw > 0.0 && ih > 0.0) {
          const double ia = iw * ih;
          const double ov = MEASURE == TF_IGNORE_IOF ? ia / an.farea : ia / (an.farea + ra[j] - ia);
          if (ov >= thresh) { covered = true; break; }
        }
      }
    }
  }
  if (covered) *label = 0.f;
  if (changed) {                                                       // kernel-uniform
    const unsigned long long turned = __ballot(covered);
    if (turned && tf::lane_id() == 0) atomicAdd(&changed[b], (int)__popcll(turned));
  }
}

}  // namespace

extern "C" int tf_targets_apply_ignore(float* class_map, int B, int nt, int vsy, int vsx,
                                       const double* templates, int tstride,
                                       int ofy, int ofx, int sty, int stx,
                                       const double* ign_boxes, const int32_t* ign_offsets,
                                       int measure, double thresh, int32_t* changed, void* stream_) {
  if (B < 0 || nt < 0 || vsy < 0 || vsx < 0 || tstride < 4) return TF_ERR_ARG;
  if (measure != TF_IGNORE_IOF && measure != TF_IGNORE_IOU) return TF_ERR_ARG;
  if (!(thresh > 0.0) || !(thresh <= 1.0)) return TF_ERR_ARG;          // (a NaN fails both)
  const size_t anchors = (size_t)nt * (size_t)vsy * (size_t)vsx;
  if (B == 0 || anchors == 0 || !ign_boxes) return TF_OK;              // no anchors, or no ignore box in the batch: nothing is enqueued
  if (!class_map || !templates || !ign_offsets) return TF_ERR_ARG;
  if (anchors > (size_t)0x7fffffff - kThreads || B > 65535) return TF_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)((anchors + kThreads - 1) / kThreads), (unsigned)B);
  hipStream_t stream = (hipStream_t)stream_;
  if (measure == TF_IGNORE_IOF)
    hipLaunchKernelGGL(targets_ignore_kernel<TF_IGNORE_IOF>, grid, dim3(kThreads), 0, stream, class_map, nt, vsy, vsx, templates, tstride,
                       ofy, ofx, sty, stx, ign_boxes, ign_offsets, thresh, changed);
  else
    hipLaunchKernelGGL(targets_ignore_kernel<TF_IGNORE_IOU>, grid, dim3(kThreads), 0, stream, class_map, nt, vsy, vsx, templates, tstride,
                       ofy, ofx, sty, stx, ign_boxes, ign_offsets, thresh, changed);
  TF_CHECK_LAUNCH();
  return TF_OK;
}
