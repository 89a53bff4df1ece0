// Test-time augmentation between csrc/decode.hip and the rows get_detections returns (tinyfaces/evaluation.py:80-87), float64.
// Compiled with -ffp-contract=off: the IoU below is nms_mask_kernel's (csrc/nms.hip) bit for bit.
//
//   box voting  (Gidaris & Komodakis, ICCV 2015; Detectron's box_voting, scoring method ID): every box that survived the NMS is replaced by the
//               weighted mean of ALL candidates of its segment that overlap it by at least vote_thresh (`>=`, where the NMS suppresses on `>`);
//               its own score stays.  One wave per kept box, kVoteWaves kept boxes per workgroup; the segment's candidates pass through LDS in
//               tiles of kVoteTile, structure of arrays, so that consecutive lanes read consecutive doubles (ds_read_b64, conflict-free).  A lane
//               takes the candidates j with j % 64 == lane in ascending order, one xor butterfly over the 64 lanes finishes the six sums: no
//               atomics, the same bits on every run.  The weight (a sigmoid: the scores tf_decode_compact emits are logits) is evaluated for
//               the voters only -- a few dozen of the N candidates --, so there is no weight pass and no workspace.  Bound by the fp64 VALU:
//               K waves x N candidates x one IoU (~20 operations, the division only for boxes that intersect).
//   unflip      the rows a mirrored pyramid level appended are mirrored back: x1' = c - x2, x2' = c - x1.
//
// Neither launch needs a value on the host: the keep counts and the row range are read from device memory.
#include "common.h"

namespace {

constexpr int kVoteWaves = 4;
constexpr int kVoteTile = 512;                  // candidates per LDS tile: 6 x 4 KiB
struct VoteSegs { int off[TF_NMS_MAX_SEGMENTS + 1]; };       // by value, like nms.hip's table

__global__ void __launch_bounds__(kVoteWaves * 64) box_vote_kernel(const double* __restrict__ boxes, const double* __restrict__ scores,
                                                                   const VoteSegs sg, const int64_t* __restrict__ keep,
                                                                   const int32_t* __restrict__ num_keep, double thr, int weight_mode,
                                                                   double* __restrict__ out, int32_t* __restrict__ votes_out) {
  __shared__ double cx1[kVoteTile], cy1[kVoteTile], cx2[kVoteTile], cy2[kVoteTile], car[kVoteTile], csc[kVoteTile];
  const int s = blockIdx.y;
  const int base = sg.off[s], n = sg.off[s + 1] - base;
  const int nk = min(num_keep[s], n);                       // a count above the segment's length cannot come from the NMS; never index past it
  const int r0 = blockIdx.x * kVoteWaves;
  if (r0 >= nk) return;                                     // block-uniform, before the first barrier: the grid is sized for "every box kept"
  const int t = threadIdx.x, lane = t & 63, r = r0 + (t >> 6);
  int64_t k = r < nk ? keep[base + r] : -1;
  const bool live = k >= base && k < (int64_t)base + n;     // wave-uniform.  An index outside the segment (not the NMS's either) leaves its row unwritten
  double4 a = make_double4(0.0, 0.0, 0.0, 0.0);
  double ascore = 0.0;
  if (live) { a = *reinterpret_cast<const double4*>(boxes + 4 * (size_t)k); ascore = scores[k]; }
  const double iarea = (a.z - a.x) * (a.w - a.y);
  double sw = 0.0, sx1 = 0.0, sy1 = 0.0, sx2 = 0.0, sy2 = 0.0;
  int votes = 0;
  for (int j0 = 0; j0 < n; j0 += kVoteTile) {
    const int lim = min(kVoteTile, n - j0);
    __syncthreads();
    for (int c = t; c < lim; c += kVoteWaves * 64) {
      const double4 b = *reinterpret_cast<const double4*>(boxes + 4 * (size_t)(base + j0 + c));
      cx1[c] = b.x; cy1[c] = b.y; cx2[c] = b.z; cy2[c] = b.w;
      car[c] = (b.z - b.x) * (b.w - b.y);
      csc[c] = scores[base + j0 + c];
    }
    __syncthreads();
    if (!live) continue;
    for (int c = lane; c < lim; c += 64) {                  // kVoteTile % 64 == 0: a lane's candidates ascend across the tiles as well
      const double xx1 = fmax(a.x, cx1[c]), yy1 = fmax(a.y, cy1[c]);
      const double xx2 = fmin(a.z, cx2[c]), yy2 = fmin(a.w, cy2[c]);
      const double w = fmax(0.0, xx2 - xx1), h = fmax(0.0, yy2 - yy1);
      const double inter = w * h;
      if (inter == 0.0) continue;                           // IoU +0 or NaN (0 / 0): neither reaches a threshold > 0
      const double ovr = inter / (iarea + car[c] - inter);
      if (!(ovr >= thr)) continue;                          // a NaN is not a vote
      const double sc = csc[c];
      const double wt = weight_mode == TF_VOTE_WEIGHT_SIGMOID ? 1.0 / (1.0 + exp(-sc)) : sc;
      if (!(wt > 0.0)) continue;                            // non-positive and NaN weights are dropped
      sw += wt;
      sx1 += wt * cx1[c]; sy1 += wt * cy1[c]; sx2 += wt * cx2[c]; sy2 += wt * cy2[c];
      ++votes;
    }
  }
  if (!live) return;                                        // wave-uniform: the butterfly below runs with all 64 lanes
  sw = tf::wave_sum(sw);
  sx1 = tf::wave_sum(sx1); sy1 = tf::wave_sum(sy1); sx2 = tf::wave_sum(sx2); sy2 = tf::wave_sum(sy2);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) votes += __shfl_xor(votes, o, 64);
  if (lane == 0) {
    double* row = out + 5 * (size_t)(base + r);
    if (votes > 0 && sw > 0.0) { row[0] = sx1 / sw; row[1] = sy1 / sw; row[2] = sx2 / sw; row[3] = sy2 / sw; }
    else { row[0] = a.x; row[1] = a.y; row[2] = a.z; row[3] = a.w; }
    row[4] = ascore;
    if (votes_out) votes_out[base + r] = votes;
  }
}

__global__ void __launch_bounds__(256) boxes_unflip_kernel(double* __restrict__ dets, const int32_t* __restrict__ first,
                                                           const int32_t* __restrict__ last, int max_rows, double c) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  const int f = *first;
  if (f < 0 || t >= max_rows || t >= *last - f) return;
  double* row = dets + 5 * (size_t)(f + t);
  const double x1 = row[0], x2 = row[2];
  row[0] = c - x2;
  row[2] = c - x1;
}

}  // namespace

extern "C" int tf_box_vote_f64_batched(const double* boxes, const double* scores, const int32_t* host_seg_offsets, int num_segments,
                                       const int64_t* keep, const int32_t* num_keep, double vote_thresh, int weight_mode,
                                       double* out, int32_t* votes_out, void* stream_) {
  const int S = num_segments;
  if (!host_seg_offsets || S <= 0 || S > TF_NMS_MAX_SEGMENTS || !num_keep || host_seg_offsets[0] != 0) return TF_ERR_ARG;
  if (weight_mode != TF_VOTE_WEIGHT_SIGMOID && weight_mode != TF_VOTE_WEIGHT_SCORE) return TF_ERR_ARG;
  if (!(vote_thresh > 0.0 && vote_thresh <= 1.0)) return TF_ERR_ARG;           // (a NaN fails both)
  VoteSegs sg;
  int nmax = 0;
  for (int s = 0; s < S; ++s) {
    const int ns = host_seg_offsets[s + 1] - host_seg_offsets[s];
    if (ns < 0) return TF_ERR_ARG;
    if (ns > nmax) nmax = ns;
  }
  for (int s = 0; s <= TF_NMS_MAX_SEGMENTS; ++s) sg.off[s] = host_seg_offsets[s < S ? s : S];
  if (host_seg_offsets[S] == 0) return TF_OK;
  if (!boxes || !scores || !keep || !out) return TF_ERR_ARG;
  hipLaunchKernelGGL(box_vote_kernel, dim3((nmax + kVoteWaves - 1) / kVoteWaves, S), dim3(kVoteWaves * 64), 0, (hipStream_t)stream_,
                     boxes, scores, sg, keep, num_keep, vote_thresh, weight_mode, out, votes_out);
  TF_CHECK_LAUNCH();
  return TF_OK;
}

extern "C" int tf_box_vote_f64(const double* boxes, const double* scores, int n, const int64_t* keep, const int32_t* num_keep,
                               double vote_thresh, int weight_mode, double* out, int32_t* votes_out, void* stream_) {
  if (n < 0) return TF_ERR_ARG;
  const int32_t off[2] = {0, n};
  return tf_box_vote_f64_batched(boxes, scores, off, 1, keep, num_keep, vote_thresh, weight_mode, out, votes_out, stream_);
}

extern "C" int tf_boxes_unflip_f64(double* dets, const int32_t* first, const int32_t* last, int max_rows, double c, void* stream_) {
  if (!dets || !first || !last || max_rows < 0) return TF_ERR_ARG;
  if (max_rows == 0) return TF_OK;
  hipLaunchKernelGGL(boxes_unflip_kernel, dim3((max_rows + 255) / 256), dim3(256), 0, (hipStream_t)stream_, dets, first, last, max_rows, c);
  TF_CHECK_LAUNCH();
  return TF_OK;
}
