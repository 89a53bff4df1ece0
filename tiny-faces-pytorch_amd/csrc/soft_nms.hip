// Soft-NMS (Bodla et al., ICCV 2017; Detectron's soft_nms) in float64, next to the hard greedy NMS of csrc/nms.hip: a candidate that overlaps a
// better one is not dropped, its score is decayed, the list is re-ranked, and it survives while its score stays >= score_thresh (semantics:
// include/tinyfaces_hip.h; numpy restatement: tests/soft_nms_ref.py).  Compiled with -ffp-contract=off: the IoU is nms_mask_kernel's bit for bit.
//
//   1 adjacency   adj[i][w] bit j = "selecting i can decay 64w+j": IoU > iou_thresh (linear) or inter > 0 (gaussian), in INPUT order and for every
//                 pair (the order of selection is not known in advance, so there is no triangle to leave out).  One wave per 64x64 block, the
//                 column boxes staged in LDS, as nms_mask_kernel.  Chip-wide; n^2 / 8 bytes.
//   2 selection   one workgroup per segment, one 64-candidate word per thread (hence kMaxBoxes = 64 x 1024).  A thread keeps the liveness bits of
//                 its word and its cached maximum (value, index) in registers; the running scores live in the workspace and are only ever touched
//                 by their owner.  A round: wave butterfly + one LDS step -> block arg-max (lowest index on a tie); every thread reads ITS word of
//                 the selected row; for the set bits that are still live the IoU is recomputed, the score decayed and tested.  A score only ever
//                 falls, so a cached maximum stands unless it was the candidate selected or decayed: only then the thread rescans its 64 scores
//                 (16 independent 32-byte loads; the owner of the selected box does it while the row word travels).  So a round costs one
//                 reduction, one row read and the few decays, not a pass over the candidates.  One barrier per round (the reduction slots alternate).  The loop is a `for` over at most n
//                 rounds inside one workgroup: no grid barrier, no cooperative launch, no spinning on another workgroup.  No atomics anywhere:
//                 the same bits on every run.  max_keep > 0 (the *_capped entries) ends the loop after that many selections: the rows written
//                 are the first max_keep rows of the uncapped run, whose later rounds cannot change them.
#include "common.h"

namespace {

constexpr int kMaxSeg = TF_NMS_MAX_SEGMENTS;
constexpr int kMaxBoxes = TF_SOFT_NMS_MAX_BOXES;
constexpr int kSelThreads = kMaxBoxes / 64;          // 1024: one 64-candidate word per thread
static_assert(kSelThreads == 1024, "the selection kernel owns one word per thread of a 1024-thread workgroup");

struct SoftSegs {                                    // by value, like nms.hip's table
  int off[kMaxSeg + 1];                              // box offsets
  unsigned long long moff[kMaxSeg];                  // offset (64-bit words) of the segment's adjacency matrix
  int woff[kMaxSeg];                                 // offset (64-candidate words) of the segment's running scores
};

__global__ void __launch_bounds__(64) soft_nms_adj_kernel(const double* __restrict__ boxes_all, const SoftSegs sg, int method, double thr,
                                                          unsigned long long* __restrict__ adj_all) {
  const int base = sg.off[blockIdx.z], n = sg.off[blockIdx.z + 1] - base, nwords = (n + 63) / 64;
  const int rb = blockIdx.y, cb = blockIdx.x;
  if (rb >= nwords || cb >= nwords) return;  // block-uniform: the grid is sized for the largest segment
  const double* boxes = boxes_all + 4 * (size_t)base;
  unsigned long long* adj = adj_all + sg.moff[blockIdx.z];
  __shared__ double cbox[64][4];
  __shared__ double carea[64];
  const int t = threadIdx.x;
  const int cj = cb * 64 + t;
  if (cj < n) {
    const double4 b = *reinterpret_cast<const double4*>(boxes + 4 * (size_t)cj);
    cbox[t][0] = b.x; cbox[t][1] = b.y; cbox[t][2] = b.z; cbox[t][3] = b.w;
    carea[t] = (b.z - b.x) * (b.w - b.y);
  }
  __syncthreads();
  const int i = rb * 64 + t;
  if (i >= n) return;
  const double4 a = *reinterpret_cast<const double4*>(boxes + 4 * (size_t)i);
  const double iarea = (a.z - a.x) * (a.w - a.y);
  unsigned long long bits = 0;
  const int lim = min(64, n - cb * 64);
  for (int j = 0; j < lim; ++j) {
    const double xx1 = fmax(a.x, cbox[j][0]), yy1 = fmax(a.y, cbox[j][1]);
    const double xx2 = fmin(a.z, cbox[j][2]), yy2 = fmin(a.w, cbox[j][3]);
    const double w = fmax(0.0, xx2 - xx1), h = fmax(0.0, yy2 - yy1);
    const double inter = w * h;
    if (!(inter > 0.0)) continue;            // inter == 0 (or NaN): never decayed, whatever the method
    if (method == TF_SOFT_NMS_LINEAR) {
      const double ovr = inter / (iarea + carea[j] - inter);
      if (!(ovr > thr)) continue;
    }
    bits |= 1ull << j;
  }
  adj[(size_t)i * nwords + cb] = bits;
}

// (value, index) arg-max: the larger value, the lower index on a bit-equal tie.  v = -1 / i = INT_MAX: "nothing live" (live scores are >= 0)
__device__ __forceinline__ void take_better(double& v, int& i, double ov, int oi) {
  if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
}

__global__ void __launch_bounds__(kSelThreads) soft_nms_select_kernel(const double* __restrict__ boxes_all, const double* __restrict__ scores_all,
                                                                      const SoftSegs sg, int method, double thr, double sigma, double sthr,
                                                                      int score_mode, int max_keep, const unsigned long long* __restrict__ adj_all,
                                                                      double* __restrict__ run_all, int64_t* __restrict__ keep_all,
                                                                      double* __restrict__ score_all, int32_t* __restrict__ num_keep) {
  __shared__ double red_v[2][kSelThreads / 64];
  __shared__ int red_i[2][kSelThreads / 64];
  const int s = blockIdx.x;
  const int base = sg.off[s], n = sg.off[s + 1] - base, nwords = (n + 63) / 64;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, nwaves = blockDim.x >> 6;
  if (n == 0) { if (t == 0) num_keep[s] = 0; return; }       // block-uniform
  const double* boxes = boxes_all + 4 * (size_t)base;
  const unsigned long long* adj = adj_all + sg.moff[s];
  double* run = run_all + 64 * (size_t)sg.woff[s];           // [nwords * 64] running scores; thread t owns run[64t .. 64t+63]
  const bool owner = t < nwords;                             // the host sizes the block so that every word has its thread

  // initial scores, coalesced; the tail of the last word is padding no liveness bit ever points at
  for (int j = t; j < nwords * 64; j += blockDim.x) {
    double v = -1.0;
    if (j < n) {
      const double sc = scores_all[base + j];
      v = score_mode == TF_VOTE_WEIGHT_SIGMOID ? 1.0 / (1.0 + exp(-sc)) : sc;
    }
    run[j] = v;
  }
  __syncthreads();                                           // the only hand-over of run[] between threads: from here on a word is its owner's alone

  unsigned long long live = 0;
  if (owner) { const int nv = min(64, n - 64 * t); live = nv >= 64 ? ~0ull : ((1ull << nv) - 1ull); }
  double best = -1.0;
  int besti = 0x7fffffff;
  bool dirty = owner;
  int r = 0;
  // rescan the word: liveness test (s >= score_thresh; a NaN fails it) and the cached maximum, lowest index first.  Eight independent 32-byte
  // loads in flight, twice (all sixteen at once spill: 128 VGPRs at 1024 threads)
  auto rescan = [&]() {
    best = -1.0; besti = 0x7fffffff;
    const double4* rw = reinterpret_cast<const double4*>(run + 64 * (size_t)t);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      double4 v[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) v[q] = rw[8 * half + q];
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const double e[4] = {v[q].x, v[q].y, v[q].z, v[q].w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int b = 32 * half + 4 * q + u;
          if (!((live >> b) & 1ull)) continue;
          if (!(e[u] >= sthr)) { live &= ~(1ull << b); continue; }
          if (e[u] > best) { best = e[u]; besti = 64 * t + b; }
        }
      }
    }
  };
  for (int round = 0; round <= n; ++round) {                 // at most n selections, then one round that finds nothing live
    if (dirty) { rescan(); dirty = false; }
    // block arg-max: xor butterfly inside the wave, then the <= 16 wave results through LDS (slots alternate: one barrier per round)
    double v = best;
    int vi = besti;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(vi, o, 64);
      take_better(v, vi, ov, oi);
    }
    const int slot = round & 1;
    if (lane == 0) { red_v[slot][wave] = v; red_i[slot][wave] = vi; }
    __syncthreads();
    v = red_v[slot][0]; vi = red_i[slot][0];
    for (int w = 1; w < nwaves; ++w) take_better(v, vi, red_v[slot][w], red_i[slot][w]);
    if (vi == 0x7fffffff) break;                             // block-uniform: nothing is live
    const int m = vi;
    if (t == 0) { keep_all[base + r] = (int64_t)(base + m); score_all[base + r] = v; }
    ++r;
    if (r == max_keep) break;                                // block-uniform: the cap (0 = none: r >= 1 here)
    if (owner) {
      // the row word and the selected box are asked for first; the owner of m rescans its word (its cached maximum is gone) while they travel
      const unsigned long long arow = adj[(size_t)m * nwords + t];
      const double4 a = *reinterpret_cast<const double4*>(boxes + 4 * (size_t)m);
      if ((m >> 6) == t) { live &= ~(1ull << (m & 63)); rescan(); }
      unsigned long long hit = arow & live;
      if (hit) {
        const double marea = (a.z - a.x) * (a.w - a.y);
        for (int k = 0; k < 64 && hit; ++k) {                // one step per set bit
          const int b = __builtin_ctzll(hit);
          hit &= hit - 1;
          const int j = 64 * t + b;
          const double4 c = *reinterpret_cast<const double4*>(boxes + 4 * (size_t)j);
          const double xx1 = fmax(a.x, c.x), yy1 = fmax(a.y, c.y);
          const double xx2 = fmin(a.z, c.z), yy2 = fmin(a.w, c.w);
          const double w = fmax(0.0, xx2 - xx1), h = fmax(0.0, yy2 - yy1);
          const double inter = w * h;
          if (inter == 0.0) continue;
          const double ovr = inter / (marea + (c.z - c.x) * (c.w - c.y) - inter);
          double sj = run[j];
          if (method == TF_SOFT_NMS_LINEAR) {
            if (!(ovr > thr)) continue;
            sj = sj * (1.0 - ovr);
          } else {
            if (!(ovr > 0.0)) continue;
            sj = sj * exp(-(ovr * ovr) / sigma);
          }
          run[j] = sj;
          if (!(sj >= sthr)) live &= ~(1ull << b);           // the liveness test (a NaN fails it)
          if (j == besti) dirty = true;                      // a score only ever falls: the cached maximum stands unless it was this one
        }
      }
    }
  }
  if (t == 0) num_keep[s] = r;
}

}  // namespace

static inline size_t soft_align256(size_t x) { return (x + 255) & ~(size_t)255; }

// validates the table; returns false on a bad one.  words: adjacency words of all segments, vwords: 64-candidate words of all segments
static bool soft_table(const int32_t* off, int S, SoftSegs* sg, size_t* words, size_t* vwords, int* nmax) {
  if (!off || S <= 0 || S > kMaxSeg || off[0] != 0) return false;
  size_t w = 0, vw = 0;
  int mx = 0;
  for (int s = 0; s < S; ++s) {
    const int ns = off[s + 1] - off[s];
    if (ns < 0) return false;
    if (ns > mx) mx = ns;
    const size_t nw = ((size_t)ns + 63) / 64;
    if (sg) { sg->moff[s] = w; sg->woff[s] = (int)vw; }
    w += (size_t)ns * nw;
    vw += nw;
  }
  if (sg) {
    for (int s = 0; s <= kMaxSeg; ++s) sg->off[s] = off[s < S ? s : S];
    for (int s = S; s < kMaxSeg; ++s) { sg->moff[s] = 0; sg->woff[s] = 0; }
  }
  *words = w; *vwords = vw; *nmax = mx;
  return true;
}

extern "C" size_t tf_soft_nms_batched_workspace_bytes(const int32_t* host_seg_offsets, int num_segments) {
  size_t words = 0, vwords = 0;
  int nmax = 0;
  if (!soft_table(host_seg_offsets, num_segments, nullptr, &words, &vwords, &nmax) || host_seg_offsets[num_segments] == 0) return 0;
  return soft_align256(vwords * 64 * 8) + soft_align256(words * 8);
}

extern "C" size_t tf_soft_nms_workspace_bytes(int n) {
  if (n <= 0) return 0;
  const int32_t off[2] = {0, n};
  return tf_soft_nms_batched_workspace_bytes(off, 1);
}

extern "C" int tf_soft_nms_f64_batched_capped(const double* boxes, const double* scores, const int32_t* host_seg_offsets, int num_segments,
                                              int method, double iou_thresh, double sigma, double score_thresh, int score_mode, int max_keep,
                                              int64_t* keep_out, double* score_out, int32_t* num_keep, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int S = num_segments;
  SoftSegs sg;
  size_t words = 0, vwords = 0;
  int nmax = 0;
  if (!num_keep || max_keep < 0 || !soft_table(host_seg_offsets, S, &sg, &words, &vwords, &nmax)) return TF_ERR_ARG;
  if (method != TF_SOFT_NMS_LINEAR && method != TF_SOFT_NMS_GAUSSIAN) return TF_ERR_ARG;
  if (score_mode != TF_VOTE_WEIGHT_SIGMOID && score_mode != TF_VOTE_WEIGHT_SCORE) return TF_ERR_ARG;
  if (!(sigma > 0.0) || !(iou_thresh >= 0.0 && iou_thresh <= 1.0) || !(score_thresh >= 0.0)) return TF_ERR_ARG;      // (a NaN fails each)
  if (host_seg_offsets[S] == 0) return TF_OK;                // nothing to do: num_keep stays as the caller zeroed it
  if (!boxes || !scores || !keep_out || !score_out) return TF_ERR_ARG;
  if (nmax > kMaxBoxes) return TF_ERR_UNSUPPORTED;           // one 64-candidate word per thread of the selection workgroup
  if (!ws || ws_bytes < tf_soft_nms_batched_workspace_bytes(host_seg_offsets, S)) return TF_ERR_WORKSPACE;
  double* run = (double*)ws;
  unsigned long long* adj = (unsigned long long*)((char*)ws + soft_align256(vwords * 64 * 8));
  const int nwmax = (nmax + 63) / 64;
  hipLaunchKernelGGL(soft_nms_adj_kernel, dim3(nwmax, nwmax, S), dim3(64), 0, stream, boxes, sg, method, iou_thresh, adj);
  const int threads = ((nwmax + 63) / 64) * 64;              // whole waves, one thread per word of the longest segment (<= 1024)
  hipLaunchKernelGGL(soft_nms_select_kernel, dim3(S), dim3(threads), 0, stream, boxes, scores, sg, method, iou_thresh, sigma, score_thresh,
                     score_mode, max_keep, adj, run, keep_out, score_out, num_keep);
  TF_CHECK_LAUNCH();
  return TF_OK;
}

extern "C" int tf_soft_nms_f64_batched(const double* boxes, const double* scores, const int32_t* host_seg_offsets, int num_segments,
                                       int method, double iou_thresh, double sigma, double score_thresh, int score_mode,
                                       int64_t* keep_out, double* score_out, int32_t* num_keep, void* ws, size_t ws_bytes, void* stream_) {
  return tf_soft_nms_f64_batched_capped(boxes, scores, host_seg_offsets, num_segments, method, iou_thresh, sigma, score_thresh, score_mode, 0,
                                        keep_out, score_out, num_keep, ws, ws_bytes, stream_);
}

extern "C" int tf_soft_nms_f64_capped(const double* boxes, const double* scores, int n, int method, double iou_thresh, double sigma,
                                      double score_thresh, int score_mode, int max_keep, int64_t* keep_out, double* score_out,
                                      int32_t* num_keep, void* ws, size_t ws_bytes, void* stream_) {
  if (n < 0) return TF_ERR_ARG;
  const int32_t off[2] = {0, n};
  return tf_soft_nms_f64_batched_capped(boxes, scores, off, 1, method, iou_thresh, sigma, score_thresh, score_mode, max_keep, keep_out, score_out,
                                        num_keep, ws, ws_bytes, stream_);
}

extern "C" int tf_soft_nms_f64(const double* boxes, const double* scores, int n, int method, double iou_thresh, double sigma,
                               double score_thresh, int score_mode, int64_t* keep_out, double* score_out, int32_t* num_keep,
                               void* ws, size_t ws_bytes, void* stream_) {
  if (n < 0) return TF_ERR_ARG;
  const int32_t off[2] = {0, n};
  return tf_soft_nms_f64_batched(boxes, scores, off, 1, method, iou_thresh, sigma, score_thresh, score_mode, keep_out, score_out, num_keep,
                                 ws, ws_bytes, stream_);
}
