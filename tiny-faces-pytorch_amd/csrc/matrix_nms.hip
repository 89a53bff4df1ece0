// Matrix NMS (Wang et al., SOLOv2, NeurIPS 2020; PaddleDetection's matrix_nms) in float64, next to the hard NMS of csrc/nms.hip and the Soft-NMS
// of csrc/soft_nms.hip: the score of a candidate is decayed by the better-scored candidates that overlap it, each weighed against ITS largest
// overlap with something still better (its "compensation"), in closed form -- nothing is selected in turn, so nothing is serial (semantics:
// include/tinyfaces_hip.h; numpy restatement: tests/matrix_nms_ref.py).  Compiled with -ffp-contract=off: the IoU is nms_mask_kernel's bit for bit.
//
//   1 admit       pv[i] = p_i (the sigmoid of the logit, or the score itself) where p_i >= score_thresh, else -1 ("not there"; a NaN fails the
//                 test).  One thread per candidate of the concatenated list.
//   2 rank        rank[i] = #{j : pv_j > pv_i or (pv_j == pv_i and j < i)}: nms_rank_kernel's all-pairs count (score tiles of 2048 in LDS, one
//                 compare per pair away from the block's own tile).  -1 ranks every unadmitted candidate behind every admitted one, so the
//                 order is a permutation of 0..n-1 and every slot of order / sorted boxes / sorted p is written; no count of the admitted is
//                 needed: later passes see p < 0 and stop.
//   3 comp        comp[j] = max_{i<j} IoU(i, j) over the sorted list.  A block owns 64 rows j (registers) and walks the columns i < j in LDS
//                 tiles of 256; its four waves take every fourth column of a tile (the column is wave-uniform: an LDS broadcast) and meet in
//                 LDS at the end.  Disjoint pairs (nearly all) skip the division, as in nms_mask_kernel.
//   4 decay       the same walk with comp_i staged beside the column box: linear d_j = min (1 - IoU) / (1 - comp_i) over comp_i < 1, gaussian
//                 x_j = max (IoU^2 - comp_i^2) and ONE exp per candidate; then sv[j] = p_j * d_j where that is >= score_thresh, else -1.
//                 A disjoint pair contributes a term >= 1 (linear) / <= 0 (gaussian) and rank 0 one <= 1 / >= 0, so starting from 1 / 0 and
//                 skipping the disjoint pairs gives the defined minimum / maximum exactly.
//   5 emit        the rank kernel again, on (sv, rank): row er of the output is the candidate with er better (s, rank) pairs in front of it;
//                 rows below the cap are written, block 0 of a segment writes min(K, max_keep).
// Five launches whatever n and S (segments ride in blockIdx.y).  max and min are exact and order-independent, the only atomic is an integer count
// in LDS: the same bits on every run.  Workspace: 68 bytes per candidate.  No memset, no grid barrier, no host synchronisation.
#include "common.h"

namespace {

constexpr int kMaxSeg = TF_NMS_MAX_SEGMENTS;
constexpr int kRows = 64;                            // rows (candidates j) per block of the pair passes: one per lane
constexpr int kSlices = 4;                           // waves per block: wave p takes columns p, p + 4, ... of a tile
constexpr int kTile = 256;                           // columns (candidates i) per LDS tile: one staged by each thread
static_assert(kRows * kSlices == kTile, "every thread of a pair block stages one column of a tile");

struct MSegs {                                       // by value, like nms.hip's table
  int off[kMaxSeg + 1];                              // box offsets
};

__global__ void __launch_bounds__(256) mnms_admit_kernel(const double* __restrict__ scores, int n, int score_mode, double sthr,
                                                         double* __restrict__ pv) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double sc = scores[i];
  const double p = score_mode == TF_VOTE_WEIGHT_SIGMOID ? 1.0 / (1.0 + exp(-sc)) : sc;
  pv[i] = p >= sthr ? p : -1.0;                      // (a NaN fails the test)
}

// rank[i] = #{j : v_j > v_i or (v_j == v_i and j < i)} over the values of one segment: nms_rank_kernel's scheme (32 Q boxes x 8 column slices
// per block; a 2048-value tile entirely below / above the block's own boxes takes one compare per pair) without its NaN paths -- no value
// here is a NaN, "not there" is -1 and every live value is >= 0.
//   kEmit = false: v = pv in input order.    order[rank] = i, sboxes[rank] = box_i, sp[rank] = v_i, for every i.
//   kEmit = true:  v = sv in rank order.     For v_i >= 0 and a row below the cap: keep[rank] = base + order[i], score[rank] = v_i; block 0
//                                            writes the segment's count (the live values counted while the tiles are staged).
template <int Q, bool kEmit>
__global__ void __launch_bounds__(256) mnms_rank_kernel(const double* __restrict__ val_all, const double* __restrict__ boxes_all, const MSegs sg,
                                                        int max_keep, int* __restrict__ order_all, double* __restrict__ sboxes_all,
                                                        double* __restrict__ sp_all, int64_t* __restrict__ keep_all,
                                                        double* __restrict__ score_all, int32_t* __restrict__ num_keep) {
  __shared__ double tile[2048];
  constexpr int kRankBoxes = 32 * Q;
  __shared__ int part[8][kRankBoxes];
  __shared__ int live_total;
  const int base = sg.off[blockIdx.y], n = sg.off[blockIdx.y + 1] - base;
  const int i0 = blockIdx.x * kRankBoxes;
  if (kEmit && n == 0 && blockIdx.x == 0 && threadIdx.x == 0) num_keep[blockIdx.y] = 0;
  if (i0 >= n) return;                                    // block-uniform: the grid is sized for the largest segment
  const double* val = val_all + base;
  const int li = threadIdx.x & 31, p = threadIdx.x >> 5;
  double si[Q]; int rank[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) {
    const int i = i0 + li + 32 * q;
    si[q] = i < n ? val[i] : -1.0; rank[q] = 0;
  }
  const bool counts = kEmit && blockIdx.x == 0;           // block-uniform
  if (threadIdx.x == 0) live_total = 0;
  int live = 0;                                           // live values among those THIS thread stages: every j of the list exactly once
  for (int j0 = 0; j0 < n; j0 += 2048) {
    __syncthreads();                                      // (the first one also orders the reset of live_total)
    if (j0 + 2048 <= n) {                                 // a whole tile (all but the last): no bound to test per value
#pragma unroll
      for (int k = threadIdx.x; k < 2048; k += 256) {
        const double v = val[j0 + k];
        tile[k] = v; live += v >= 0.0;
      }
    } else {
      for (int k = threadIdx.x; k < 2048; k += 256) {
        const double v = (j0 + k < n) ? val[j0 + k] : -1.0e300;
        tile[k] = v; live += v >= 0.0;
      }
    }
    __syncthreads();
    const int lim = min(2048, n - j0);
    if (j0 + 2048 <= i0) {                                // every j of the tile is below every i of the block: ties count
#pragma unroll 4
      for (int k = p; k < lim; k += 8) {
        const double sj = tile[k];
#pragma unroll
        for (int q = 0; q < Q; ++q) rank[q] += sj >= si[q];
      }
    } else if (j0 >= i0 + kRankBoxes) {                   // every j above every i: ties do not count (nor does the -1e300 padding)
#pragma unroll 4
      for (int k = p; k < lim; k += 8) {
        const double sj = tile[k];
#pragma unroll
        for (int q = 0; q < Q; ++q) rank[q] += sj > si[q];
      }
    } else {                                              // the tile that holds the block's own boxes: the full predicate
#pragma unroll 2
      for (int k = p; k < lim; k += 8) {
        const double sj = tile[k];
#pragma unroll
        for (int q = 0; q < Q; ++q) rank[q] += (sj > si[q]) || (sj == si[q] && (j0 + k) < i0 + li + 32 * q);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) part[p][li + 32 * q] = rank[q];
  if (counts && live) atomicAdd(&live_total, live);       // an integer sum: the same whatever the arrival order
  __syncthreads();
  if (threadIdx.x < kRankBoxes) {
    const int i = i0 + threadIdx.x;
    if (i < n) {
      int r = 0;
#pragma unroll
      for (int q = 0; q < 8; ++q) r += part[q][threadIdx.x];
      const double v = val[i];
      if (!kEmit) {
        order_all[base + r] = i;
        const double4 bx = *reinterpret_cast<const double4*>(boxes_all + 4 * (size_t)(base + i));
        *reinterpret_cast<double4*>(sboxes_all + 4 * (size_t)(base + r)) = bx;
        sp_all[base + r] = v;
      } else if (v >= 0.0 && (max_keep == 0 || r < max_keep)) {     // every live value ranks in front of every -1: r < K here
        keep_all[base + r] = (int64_t)(base + order_all[base + i]);  // index into the concatenated input
        score_all[base + r] = v;
      }
    }
  }
  if (counts && threadIdx.x == 0) num_keep[blockIdx.y] = (max_keep > 0 && live_total > max_keep) ? max_keep : live_total;
}

// The two all-pairs passes over the score-sorted list of a segment: rows j in registers (one per lane, 64 per block), columns i < j staged in
// LDS tiles of kTile.  kDecay = false: comp[j].  kDecay = true: sv[j] from comp[].  Blocks are dealt longest first (the last rows have the
// most columns): blockIdx.x = 0 is the LAST row block.
template <bool kDecay>
__global__ void __launch_bounds__(kTile) mnms_pair_kernel(const double* __restrict__ sboxes_all, const double* __restrict__ sp_all, const MSegs sg,
                                                          int method, double sigma, double sthr, double* __restrict__ comp_all,
                                                          double* __restrict__ sv_all) {
  __shared__ double col[kTile][6];                        // x1 y1 x2 y2 area comp: 48-byte rows, read as a broadcast
  __shared__ double part[kSlices][kRows];
  const int base = sg.off[blockIdx.y], n = sg.off[blockIdx.y + 1] - base;
  const int nblocks = (n + kRows - 1) / kRows;
  if ((int)blockIdx.x >= nblocks) return;                 // block-uniform: the grid is sized for the largest segment
  const int j0 = (nblocks - 1 - (int)blockIdx.x) * kRows;
  const double* sboxes = sboxes_all + 4 * (size_t)base;
  const double* sp = sp_all + base;
  double* comp = comp_all + base;
  double* sv = sv_all + base;
  const int t = threadIdx.x, r = t & (kRows - 1), p = t / kRows;
  const int j = j0 + r;
  const bool row = j < n;
  if (sp[j0] < 0.0) {                                     // block-uniform: p descends and -1 comes last, so nobody in this block is admitted
    if (kDecay && p == 0 && row) sv[j] = -1.0;
    return;
  }
  double4 b = make_double4(0.0, 0.0, 0.0, 0.0);
  if (row) b = *reinterpret_cast<const double4*>(sboxes + 4 * (size_t)j);
  const double jarea = (b.z - b.x) * (b.w - b.y);
  const bool linear = method == TF_MATRIX_NMS_LINEAR;
  double acc = (kDecay && linear) ? 1.0 : 0.0;            // comp: max from 0; linear decay: min from 1; gaussian argument: max from 0
  const int cend = min(n, j0 + kRows) - 1;                // columns i < j <= the block's last row
  for (int i0 = 0; i0 < cend; i0 += kTile) {
    __syncthreads();
    if (i0 + t < cend) {
      const double4 c = *reinterpret_cast<const double4*>(sboxes + 4 * (size_t)(i0 + t));
      col[t][0] = c.x; col[t][1] = c.y; col[t][2] = c.z; col[t][3] = c.w;
      col[t][4] = (c.z - c.x) * (c.w - c.y);
      col[t][5] = kDecay ? comp[i0 + t] : 0.0;
    }
    __syncthreads();
    const int lim = min(kTile, cend - i0);
    const bool below = i0 + kTile <= j0;                  // block-uniform: every column of the tile is in front of every row of the block
#pragma unroll 2
    for (int k = p; k < lim; k += kSlices) {
      const double xx1 = fmax(b.x, col[k][0]), yy1 = fmax(b.y, col[k][1]);
      const double xx2 = fmin(b.z, col[k][2]), yy2 = fmin(b.w, col[k][3]);
      const double w = fmax(0.0, xx2 - xx1), h = fmax(0.0, yy2 - yy1);
      const double inter = w * h;
      // disjoint pairs (nearly all of them): IoU 0, which changes neither the maximum nor, as said above, the minimum
      if (!(inter > 0.0) || !(below || i0 + k < j)) continue;
      const double ovr = inter / (col[k][4] + jarea - inter);
      if (!kDecay) {
        if (ovr > acc) acc = ovr;                         // (a NaN quotient counts as 0: the compare is false)
      } else if (linear) {
        const double ci = col[k][5];
        if (ci < 1.0) {                                   // comp_i >= 1: an exact duplicate of a better box, which stands in for it
          const double term = (1.0 - ovr) / (1.0 - ci);
          if (term < acc) acc = term;
        }
      } else {
        const double ci = col[k][5];
        const double term = ovr * ovr - ci * ci;
        if (term > acc) acc = term;
      }
    }
  }
  part[p][r] = acc;
  __syncthreads();
  if (p != 0 || !row) return;
#pragma unroll
  for (int q = 1; q < kSlices; ++q) {
    const double o = part[q][r];
    if (kDecay && linear ? o < acc : o > acc) acc = o;
  }
  if (!kDecay) { comp[j] = acc; return; }
  const double pj = sp[j];
  const double d = linear ? acc : (j == 0 ? 1.0 : exp(-acc / sigma));
  const double s = pj * d;
  sv[j] = (pj >= 0.0 && s >= sthr) ? s : -1.0;            // (a NaN fails the test)
}

}  // namespace

static inline size_t mnms_align256(size_t x) { return (x + 255) & ~(size_t)255; }

// validates the table; returns false on a bad one
static bool mnms_table(const int32_t* off, int S, MSegs* sg, int* nmax) {
  if (!off || S <= 0 || S > kMaxSeg || off[0] != 0) return false;
  int mx = 0;
  for (int s = 0; s < S; ++s) {
    const int ns = off[s + 1] - off[s];
    if (ns < 0) return false;
    if (ns > mx) mx = ns;
  }
  if (sg) for (int s = 0; s <= kMaxSeg; ++s) sg->off[s] = off[s < S ? s : S];
  *nmax = mx;
  return true;
}

extern "C" size_t tf_matrix_nms_batched_workspace_bytes(const int32_t* host_seg_offsets, int num_segments) {
  int nmax = 0;
  if (!mnms_table(host_seg_offsets, num_segments, nullptr, &nmax) || host_seg_offsets[num_segments] == 0) return 0;
  const size_t n = (size_t)host_seg_offsets[num_segments];
  // pv, sorted p, comp, sv (8 bytes each), the sorted boxes (32), the order (4)
  return 4 * mnms_align256(n * 8) + mnms_align256(n * 32) + mnms_align256(n * 4);
}

extern "C" size_t tf_matrix_nms_workspace_bytes(int n) {
  if (n <= 0) return 0;
  const int32_t off[2] = {0, n};
  return tf_matrix_nms_batched_workspace_bytes(off, 1);
}

extern "C" int tf_matrix_nms_f64_batched(const double* boxes, const double* scores, const int32_t* host_seg_offsets, int num_segments, int method,
                                         double sigma, double score_thresh, int score_mode, int max_keep, int64_t* keep_out, double* score_out,
                                         int32_t* num_keep, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int S = num_segments;
  MSegs sg;
  int nmax = 0;
  if (!num_keep || max_keep < 0 || !mnms_table(host_seg_offsets, S, &sg, &nmax)) return TF_ERR_ARG;
  if (method != TF_MATRIX_NMS_LINEAR && method != TF_MATRIX_NMS_GAUSSIAN) return TF_ERR_ARG;
  if (score_mode != TF_VOTE_WEIGHT_SIGMOID && score_mode != TF_VOTE_WEIGHT_SCORE) return TF_ERR_ARG;
  if (!(sigma > 0.0) || !(score_thresh >= 0.0)) return TF_ERR_ARG;           // (a NaN fails each)
  const int n = host_seg_offsets[S];
  if (n == 0) return TF_OK;                                  // nothing to do: num_keep stays as the caller zeroed it
  if (!boxes || !scores || !keep_out || !score_out) return TF_ERR_ARG;
  if (nmax > TF_MATRIX_NMS_MAX_BOXES) return TF_ERR_UNSUPPORTED;
  if (!ws || ws_bytes < tf_matrix_nms_batched_workspace_bytes(host_seg_offsets, S)) return TF_ERR_WORKSPACE;
  char* w = (char*)ws;
  double* pv = (double*)w;       w += mnms_align256((size_t)n * 8);
  double* sp = (double*)w;       w += mnms_align256((size_t)n * 8);
  double* comp = (double*)w;     w += mnms_align256((size_t)n * 8);
  double* sv = (double*)w;       w += mnms_align256((size_t)n * 8);
  double* sboxes = (double*)w;   w += mnms_align256((size_t)n * 32);
  int* order = (int*)w;
  hipLaunchKernelGGL(mnms_admit_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, scores, n, score_mode, score_thresh, pv);
  // 128 boxes per rank block for long lists, 32 (four times the blocks) below 16 384, as the hard NMS
  const bool wide = nmax >= 16384;
  const dim3 rgrid(wide ? (nmax + 127) / 128 : (nmax + 31) / 32, S);
  if (wide) hipLaunchKernelGGL((mnms_rank_kernel<4, false>), rgrid, dim3(256), 0, stream, pv, boxes, sg, 0, order, sboxes, sp, nullptr, nullptr, nullptr);
  else hipLaunchKernelGGL((mnms_rank_kernel<1, false>), rgrid, dim3(256), 0, stream, pv, boxes, sg, 0, order, sboxes, sp, nullptr, nullptr, nullptr);
  const dim3 pgrid((nmax + kRows - 1) / kRows, S);
  hipLaunchKernelGGL(mnms_pair_kernel<false>, pgrid, dim3(kTile), 0, stream, sboxes, sp, sg, method, sigma, score_thresh, comp, sv);
  hipLaunchKernelGGL(mnms_pair_kernel<true>, pgrid, dim3(kTile), 0, stream, sboxes, sp, sg, method, sigma, score_thresh, comp, sv);
  if (wide) hipLaunchKernelGGL((mnms_rank_kernel<4, true>), rgrid, dim3(256), 0, stream, sv, nullptr, sg, max_keep, order, nullptr, nullptr, keep_out, score_out, num_keep);
  else hipLaunchKernelGGL((mnms_rank_kernel<1, true>), rgrid, dim3(256), 0, stream, sv, nullptr, sg, max_keep, order, nullptr, nullptr, keep_out, score_out, num_keep);
  TF_CHECK_LAUNCH();
  return TF_OK;
}

extern "C" int tf_matrix_nms_f64(const double* boxes, const double* scores, int n, int method, double sigma, double score_thresh, int score_mode,
                                 int max_keep, int64_t* keep_out, double* score_out, int32_t* num_keep, void* ws, size_t ws_bytes,
                                 void* stream_) {
  if (n < 0) return TF_ERR_ARG;
  const int32_t off[2] = {0, n};
  return tf_matrix_nms_f64_batched(boxes, scores, off, 1, method, sigma, score_thresh, score_mode, max_keep, keep_out, score_out, num_keep,
                                   ws, ws_bytes, stream_);
}
