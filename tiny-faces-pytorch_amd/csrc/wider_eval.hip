// WIDER FACE matching and precision / recall accumulation on the device (semantics: include/tinyfaces_hip.h; host reference:
// tinyfaces/wider_eval.py image_evaluation / image_pr_info; numpy restatement of the parallel form: tests/wider_ref.py).
//
// image_evaluation walks the detections of an image in score order and keeps a per-box state.  Only one part of it is sequential:
//   * the best ground-truth box of a detection (largest IoU, lowest index on a tie, a match iff IoU >= iou_thresh) depends on nothing else;
//   * proposal[h] = -1 iff h matched a box that the setting does not keep;
//   * a kept box changes state once, at the FIRST detection that matched it, so
//         pred_recall[h] = #{kept boxes g : first[g] <= h},  first[g] = min{h : best[h] == g}  (an integer min)
//     = the inclusive prefix sum of "h matched a kept box and h == first[best[h]]".
// The match and first[] do not depend on the setting: they are computed once, then every setting is two flags and two prefix sums.
//
//   match kernel   one 256-thread workgroup per image.  Pass 1: detections strided over the threads, the image's boxes staged through LDS in
//                  tiles of kGtTile (corners + area, so G is not bounded by LDS); best[h] to the workspace.  Pass 2: first[] by integer
//                  atomic min (workgroup scope: only this workgroup touches its image's slice).  Pass 3, per setting: chunks of 256
//                  detections in order, a wavefront scan (__shfl_up) of the two flags, the four wave totals through LDS, a running carry.
//   pr kernel      one thread per threshold t and group of kPrSegs segments: a binary search per (segment, t) for the last row whose
//                  normalised score is >= thresh[t] (segments are score-descending and (s - lo) / d is monotone in s), sums in registers,
//                  one 64-bit integer atomic per non-zero (setting, t, column).  Integer sums: the same bits in any arrival order.
// Segment tables ride in the kernel arguments (nms.hip's way), kSegChunk segments per launch: no copy, no memset, no host synchronisation.
// The float64 arithmetic must round like numpy's: the file is compiled with -ffp-contract=off (build.py EXACT).
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kGtTile = TF_WIDER_GT_TILE;         // boxes per LDS tile: 5 doubles each, 10 KiB
constexpr int kSegChunk = 256;                    // segments per launch: two tables of 257 ints by value
constexpr int kPrSegs = 8;                        // segments a thread of the pr kernel sums before its atomics

struct WiderSegs {
  int doff[kSegChunk + 1];                        // detection offsets of this chunk's segments (absolute rows)
  int goff[kSegChunk + 1];                        // ground-truth offsets
};
struct PrSegs {
  int doff[kSegChunk + 1];
};

// inclusive scan of (a, b) over the 256 threads of the block; tot = the block totals.  sh: 2 * kWaves ints.  Block-uniform call sites only.
__device__ __forceinline__ void block_scan2(int& a, int& b, int& tota, int& totb, int* sh) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int va = __shfl_up(a, o, 64), vb = __shfl_up(b, o, 64);
    if (lane >= o) { a += va; b += vb; }
  }
  __syncthreads();                                // the previous round's readers of sh are done
  if (lane == 63) { sh[wave] = a; sh[kWaves + wave] = b; }
  __syncthreads();
  tota = 0; totb = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    const int sa = sh[w], sb = sh[kWaves + w];
    if (w < wave) { a += sa; b += sb; }
    tota += sa; totb += sb;
  }
}

__global__ void __launch_bounds__(kThreads) wider_match_kernel(const double* __restrict__ rows, const double* __restrict__ gt,
                                                               const WiderSegs sg, const uint8_t* __restrict__ keep, int nset,
                                                               long long n_all, long long g_all, double iou_thresh,
                                                               int* __restrict__ counted, int* __restrict__ recalled,
                                                               int* __restrict__ best_ws, int* __restrict__ first_ws) {
  __shared__ double gx1[kGtTile], gy1[kGtTile], gx2[kGtTile], gy2[kGtTile], ga[kGtTile];
  __shared__ int sh[2 * kWaves];
  const int s = blockIdx.x, t = threadIdx.x;
  const int d0 = sg.doff[s], N = sg.doff[s + 1] - d0;
  const int g0 = sg.goff[s], G = sg.goff[s + 1] - g0;
  if (N <= 0) return;                                                  // block-uniform: nothing to write
  int* best = best_ws + d0;
  int* first = first_ws + g0;

  // pass 1: the best box of every detection
  for (int c0 = 0; c0 < N; c0 += kThreads) {                           // block-uniform trip count
    const int h = c0 + t;
    const bool live = h < N;
    double px1 = 0, py1 = 0, px2 = 0, py2 = 0, pb = 0;
    if (live) {
      const double* r = rows + (size_t)(d0 + h) * 5;
      px1 = r[0]; py1 = r[1];
      px2 = r[2] + px1; py2 = r[3] + py1;                              // image_evaluation: p[:, 2] += p[:, 0]
      pb = (px2 - px1 + 1) * (py2 - py1 + 1);
    }
    double bv = -__builtin_huge_val();
    int bi = -1;
    for (int j0 = 0; j0 < G; j0 += kGtTile) {
      const int m = min(kGtTile, G - j0);
      __syncthreads();                                                 // the previous tile's readers are done
      for (int j = t; j < m; j += kThreads) {
        const double* b = gt + (size_t)(g0 + j0 + j) * 4;
        const double x1 = b[0], y1 = b[1], x2 = b[2] + x1, y2 = b[3] + y1;
        gx1[j] = x1; gy1[j] = y1; gx2[j] = x2; gy2[j] = y2;
        ga[j] = (x2 - x1 + 1) * (y2 - y1 + 1);
      }
      __syncthreads();
      if (live) {
        for (int j = 0; j < m; ++j) {                                  // every lane reads the same LDS word: a broadcast
          const double w = fmin(gx2[j], px2) - fmax(gx1[j], px1) + 1;
          const double hh = fmin(gy2[j], py2) - fmax(gy1[j], py1) + 1;
          double o = 0.0;                                              // box_overlap: 0 when w <= 0 or h <= 0, decided before the division
          if (w > 0 && hh > 0) {
            const double inter = w * hh;
            o = inter / ((ga[j] + pb) - inter);
          }
          if (o > bv) { bv = o; bi = j0 + j; }                         // strict: the lowest index wins a tie (np.argmax)
        }
      }
    }
    if (live) best[h] = (bi >= 0 && bv >= iou_thresh) ? bi : -1;
  }

  // pass 2: the first detection that matched each box
  for (int j = t; j < G; j += kThreads) __hip_atomic_store(&first[j], 0x7fffffff, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __syncthreads();                                                     // best[] and the initial first[] are visible to the workgroup
  for (int h = t; h < N; h += kThreads) {
    const int b = best[h];
    if (b >= 0) __hip_atomic_fetch_min(&first[b], h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  __syncthreads();

  // pass 3: per setting, the two running counts
  for (int k = 0; k < nset; ++k) {
    const uint8_t* kp = keep + (size_t)k * g_all + g0;
    int* cnt = counted + (size_t)k * n_all + d0;
    int* rec = recalled + (size_t)k * n_all + d0;
    int carry_c = 0, carry_r = 0;
    for (int c0 = 0; c0 < N; c0 += kThreads) {                         // block-uniform trip count
      const int h = c0 + t;
      int fc = 0, fr = 0;
      if (h < N) {
        const int b = best[h];
        fc = 1;
        if (b >= 0) {
          if (kp[b]) fr = __hip_atomic_load(&first[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == h;
          else fc = 0;                                                 // matched an ignored box: proposal = -1
        }
      }
      int tc, tr;
      block_scan2(fc, fr, tc, tr, sh);
      if (h < N) { cnt[h] = carry_c + fc; rec[h] = carry_r + fr; }
      carry_c += tc; carry_r += tr;
    }
  }
}

__global__ void __launch_bounds__(kThreads) wider_pr_kernel(const double* __restrict__ scores, const PrSegs sg, int nseg,
                                                            const int* __restrict__ counted, const int* __restrict__ recalled, int nset,
                                                            long long n_all, const double* __restrict__ lo_d,
                                                            const double* __restrict__ thresh, int T, unsigned long long* __restrict__ pr) {
  const int t = blockIdx.x * kThreads + threadIdx.x;
  if (t >= T) return;
  const double lo = lo_d[0], d = lo_d[1], th = thresh[t];
  const int s0 = blockIdx.y * kPrSegs, s1 = min(nseg, s0 + kPrSegs);
  for (int k = 0; k < nset; ++k) {
    long long sc = 0, sr = 0;
    for (int s = s0; s < s1; ++s) {
      const int a = sg.doff[s], b = sg.doff[s + 1];
      int lo_i = a, hi_i = b;                                          // the first row of [a, b) that is NOT >= th
      while (lo_i < hi_i) {
        const int mid = lo_i + ((hi_i - lo_i) >> 1);
        if ((scores[mid] - lo) / d >= th) lo_i = mid + 1; else hi_i = mid;
      }
      if (lo_i > a) {
        sc += counted[(size_t)k * n_all + lo_i - 1];
        sr += recalled[(size_t)k * n_all + lo_i - 1];
      }
    }
    unsigned long long* p = pr + ((size_t)k * T + t) * 2;
    if (sc) atomicAdd(p, (unsigned long long)sc);
    if (sr) atomicAdd(p + 1, (unsigned long long)sr);
  }
}

}  // namespace

// tf_nms_f64_batched's refusals for a table of any length: starts at 0, never descends
static bool wider_table_ok(const int32_t* off, int S) {
  if (!off || S < 1 || off[0] != 0) return false;
  for (int s = 0; s < S; ++s)
    if (off[s + 1] < off[s]) return false;
  return true;
}

static inline size_t wider_align256(size_t x) { return (x + 255) & ~(size_t)255; }

extern "C" size_t tf_wider_match_workspace_bytes(int n, int g) {
  if (n <= 0) return 0;
  return wider_align256((size_t)n * sizeof(int)) + wider_align256((size_t)(g > 0 ? g : 0) * sizeof(int));
}

extern "C" int tf_wider_match_f64_batched(const double* rows, const int32_t* host_det_offsets, const double* gt,
                                          const int32_t* host_gt_offsets, int num_segments, const uint8_t* keep, int nset, double iou_thresh,
                                          int32_t* counted, int32_t* recalled, void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int S = num_segments;
  if (nset < 1 || !(iou_thresh == iou_thresh)) return TF_ERR_ARG;
  if (!wider_table_ok(host_det_offsets, S) || !wider_table_ok(host_gt_offsets, S)) return TF_ERR_ARG;
  const int n = host_det_offsets[S], g = host_gt_offsets[S];
  if (n == 0) return TF_OK;                                            // nothing is launched
  if (!rows || !counted || !recalled || (g > 0 && (!gt || !keep))) return TF_ERR_ARG;
  if (!ws || ws_bytes < tf_wider_match_workspace_bytes(n, g)) return TF_ERR_ARG;
  int* best = (int*)ws;
  int* first = (int*)((char*)ws + wider_align256((size_t)n * sizeof(int)));
  for (int c0 = 0; c0 < S; c0 += kSegChunk) {
    const int m = S - c0 < kSegChunk ? S - c0 : kSegChunk;
    if (host_det_offsets[c0 + m] == host_det_offsets[c0]) continue;   // no detection in the chunk
    WiderSegs sg;
    for (int i = 0; i <= kSegChunk; ++i) {
      sg.doff[i] = host_det_offsets[c0 + (i < m ? i : m)];
      sg.goff[i] = host_gt_offsets[c0 + (i < m ? i : m)];
    }
    hipLaunchKernelGGL(wider_match_kernel, dim3(m), dim3(kThreads), 0, stream, rows, gt, sg, keep, nset, (long long)n, (long long)g,
                       iou_thresh, counted, recalled, best, first);
  }
  TF_CHECK_LAUNCH();
  return TF_OK;
}

extern "C" int tf_wider_pr_accumulate(const double* scores, const int32_t* host_det_offsets, int num_segments, const int32_t* counted,
                                      const int32_t* recalled, int nset, const double* lo_d, const double* thresh, int num_thresh,
                                      int64_t* pr, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int S = num_segments, T = num_thresh;
  if (nset < 1 || T < 0) return TF_ERR_ARG;
  if (!wider_table_ok(host_det_offsets, S)) return TF_ERR_ARG;
  const int n = host_det_offsets[S];
  if (n == 0 || T == 0) return TF_OK;                                  // nothing to add
  if (!scores || !counted || !recalled || !lo_d || !thresh || !pr) return TF_ERR_ARG;
  for (int c0 = 0; c0 < S; c0 += kSegChunk) {
    const int m = S - c0 < kSegChunk ? S - c0 : kSegChunk;
    if (host_det_offsets[c0 + m] == host_det_offsets[c0]) continue;
    PrSegs sg;
    for (int i = 0; i <= kSegChunk; ++i) sg.doff[i] = host_det_offsets[c0 + (i < m ? i : m)];
    hipLaunchKernelGGL(wider_pr_kernel, dim3((T + kThreads - 1) / kThreads, (m + kPrSegs - 1) / kPrSegs), dim3(kThreads), 0, stream, scores, sg,
                       m, counted, recalled, nset, (long long)n, lo_d, thresh, T, (unsigned long long*)pr);
  }
  TF_CHECK_LAUNCH();
  return TF_OK;
}
