// Deterministic batched top-k SELECTION on float64 scores (semantics: include/tinyfaces_hip.h; numpy restatement: tests/topk_ref.py): per
// segment, the min(n_s, k) rows that come first in the hard NMS's own order (larger score, lower index on a tie, NaN last), written as
// indices into the concatenated input in ASCENDING index order.  It bounds what reaches the O(n^2) suppression kernels (nms.hip,
// soft_nms.hip) and takes lists too long for either.
//
//   key        an order-preserving uint64 of the score: sign bit flipped for non-negatives, all bits for negatives, -0 canonicalised to +0,
//              NaN -> 0 (below -inf's key).  "first in the NMS order" = larger key, then lower index.
//   histogram  MSB-first radix select, 8-bit digits, 8 passes.  Pass p counts, per segment, digit p of the keys whose digits 0..p-1 equal
//              the prefix found so far: per-wave counts in LDS (one add for a wave whose lanes agree, the common case in the exponent
//              digits), then ONE integer atomic per non-empty bin per block into hist[p][s][256].  Integer sums do not depend on arrival
//              order.  Every block begins a pass by locating the prefix itself from the finished histograms of the passes before it (p scans
//              of 256 counters, one per thread): no "pick" launch, no flag, no grid barrier.
//   compaction decode.hip's ordered compaction: per-block counts (keys above the threshold T, keys equal to it) -> one-workgroup exclusive
//              scan per segment (chunks of 1024 blocks with a carry) -> ordered write.  Row i is written iff key_i > T, or key_i == T and
//              fewer than `need` equal keys precede it; its slot is (#above before i) + min(#equal before i, need).
//   launches   1 memset + 8 histogram + count + scan + write = 12, whatever n and S.  Work per pass is linear in n.  A segment with
//              n_s <= k takes no part in the passes; the write launch copies it through.
//
// Digit width: 8 bits makes the locate step one counter per thread of a 256-thread block (two barriers per earlier pass) and the LDS
// histogram 4 KiB.  11-bit digits would save two of the eight passes and 16-bit digits four, at 8 / 256 times the counters to zero, scan
// redundantly in every block and flush; a pass over the 65 536-candidate list reads 512 KiB, so the passes are launch-bound, not
// bandwidth-bound, and the measured cost of the whole select is in profiles/topk.jsonl.
#include "common.h"

namespace {

constexpr int kMaxSeg = TF_NMS_MAX_SEGMENTS;
constexpr int kBins = 256;                        // 8-bit digits
constexpr int kPasses = 8;
constexpr int kThreads = 256;                     // == kBins: the locate step owns one counter per thread
constexpr int kItems = 16;                        // scores per thread
constexpr int kTile = kThreads * kItems;          // 4096 scores per block
static_assert(kThreads == kBins && (kThreads / 64) * kItems == 64, "one wave scans the (chunk, wave) counts of a tile");

struct TopkSegs {                                 // by value, like nms.hip's table
  int off[kMaxSeg + 1];                           // input offsets
  int ooff[kMaxSeg];                              // output offsets: sum of min(n_r, k) over r < s
};

__device__ __forceinline__ unsigned long long topk_key(double x) {
  if (x != x) return 0ull;                                             // NaN: behind every number
  unsigned long long b = (unsigned long long)__double_as_longlong(x);
  if (b == 0x8000000000000000ull) b = 0ull;                            // -0.0 == +0.0
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);                 // -inf -> 0x000f..f > 0
}

// The prefix (digits 0..passes-1 of the k-th key) and how many keys are still to be taken inside it, from the finished histograms.
// Called by all 256 threads; `sh` is 6 words of LDS.  Invariant: 1 <= krem <= #keys with the prefix, so exactly one thread matches.
__device__ __forceinline__ void topk_locate(const unsigned* __restrict__ hist_seg, size_t pass_stride, int passes, unsigned k,
                                            unsigned long long& prefix, unsigned& krem, unsigned* sh) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  prefix = 0ull; krem = k;
  for (int q = 0; q < passes; ++q) {
    const unsigned d = (unsigned)(kBins - 1 - t);                      // thread order = descending digit
    const unsigned c = hist_seg[(size_t)q * pass_stride + d];
    unsigned incl = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned v = __shfl_up(incl, o, 64); if (lane >= o) incl += v; }
    if (lane == 63) sh[wave] = incl;
    __syncthreads();
    for (int w = 0; w < wave; ++w) incl += sh[w];
    const unsigned excl = incl - c;
    if (excl < krem && krem <= incl) { sh[4] = d; sh[5] = krem - excl; }
    __syncthreads();
    prefix = (prefix << 8) | (unsigned long long)sh[4];
    krem = sh[5];
  }
}

__global__ void __launch_bounds__(kThreads) topk_hist_kernel(const double* __restrict__ scores, const TopkSegs sg, int k, int pass, int S,
                                                             unsigned* __restrict__ hist) {
  __shared__ unsigned wh[kThreads / 64][kBins];
  __shared__ unsigned sh[6];
  const int s = blockIdx.y;
  const int base = sg.off[s], n = sg.off[s + 1] - base;
  const long long t0 = (long long)blockIdx.x * kTile;
  if (n <= k || t0 >= n) return;                                       // block-uniform: passed through whole, or a tile beyond the segment
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t pass_stride = (size_t)S * kBins;
  unsigned long long prefix; unsigned krem;
  topk_locate(hist + (size_t)s * kBins, pass_stride, pass, (unsigned)k, prefix, krem, sh);
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) wh[w][t] = 0u;
  __syncthreads();
  const int shift = 56 - 8 * pass;
  const double* sc = scores + base;
#pragma unroll 4
  for (int j = 0; j < kItems; ++j) {
    const long long i = t0 + (long long)j * kThreads + t;
    bool in = i < n;
    unsigned d = 0;
    if (in) {
      const unsigned long long key = topk_key(sc[i]);
      in = pass == 0 || (key >> (shift + 8)) == prefix;
      d = (unsigned)(key >> shift) & 0xffu;
    }
    const unsigned long long act = __ballot(in);
    if (act == 0ull) continue;                                         // wave-uniform
    const unsigned d0 = (unsigned)__shfl((int)d, __builtin_ctzll(act), 64);
    if (__ballot(in && d == d0) == act) {                              // every active lane has the same digit: one add
      if (lane == 0) atomicAdd(&wh[wave][d0], (unsigned)__popcll(act));
    } else if (in) {
      atomicAdd(&wh[wave][d], 1u);
    }
  }
  __syncthreads();
  unsigned c = 0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) c += wh[w][t];
  if (c) atomicAdd(&hist[(size_t)pass * pass_stride + (size_t)s * kBins + t], c);
}

// PHASE 0: blk[s][b] = (#keys above T, #keys equal to T) of tile b.  PHASE 1: blk holds the exclusive sums; ordered write.
template <int PHASE>
__global__ void __launch_bounds__(kThreads) topk_compact_kernel(const double* __restrict__ scores, const TopkSegs sg, int k, int S, int nbmax,
                                                                const unsigned* __restrict__ hist, int2* __restrict__ blk,
                                                                int64_t* __restrict__ idx_out) {
  __shared__ unsigned sh[6];
  __shared__ int cg[64], ce[64];                                       // per (chunk j, wave w), entry 4j + w: counts, then exclusive sums
  __shared__ int tot[2];
  const int s = blockIdx.y;
  const int base = sg.off[s], n = sg.off[s + 1] - base;
  const long long t0 = (long long)blockIdx.x * kTile;
  if (t0 >= n) return;                                                 // block-uniform
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  if (n <= k) {                                                        // the segment is passed through whole
    if (PHASE == 1) {
      int64_t* out = idx_out + sg.ooff[s];
      for (int j = 0; j < kItems; ++j) {
        const long long i = t0 + (long long)j * kThreads + t;
        if (i < n) out[i] = (int64_t)base + i;
      }
    }
    return;
  }
  unsigned long long T; unsigned need;
  topk_locate(hist + (size_t)s * kBins, (size_t)S * kBins, kPasses, (unsigned)k, T, need, sh);
  const double* sc = scores + base;
  unsigned gbits = 0, ebits = 0;                                       // bit j: item j of this thread is above / equal to T
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const long long i = t0 + (long long)j * kThreads + t;
    bool g = false, e = false;
    if (i < n) { const unsigned long long key = topk_key(sc[i]); g = key > T; e = key == T; }
    const unsigned long long bg = __ballot(g), be = __ballot(e);
    if (lane == 0) { cg[4 * j + wave] = __popcll(bg); ce[4 * j + wave] = __popcll(be); }
    gbits |= (unsigned)g << j; ebits |= (unsigned)e << j;
  }
  __syncthreads();
  if (wave == 0) {                                                     // 64 entries: one wave scans them
    const int vg = cg[lane], ve = ce[lane];
    int ig = vg, ie = ve;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int a = __shfl_up(ig, o, 64), b = __shfl_up(ie, o, 64);
      if (lane >= o) { ig += a; ie += b; }
    }
    cg[lane] = ig - vg; ce[lane] = ie - ve;
    if (lane == 63) { tot[0] = ig; tot[1] = ie; }
  }
  __syncthreads();
  int2* myblk = blk + (size_t)s * nbmax + blockIdx.x;
  if (PHASE == 0) {
    if (t == 0) *myblk = make_int2(tot[0], tot[1]);
    return;
  }
  const int2 before = *myblk;
  const int m = k;                                                     // n > k here: the segment emits exactly k rows
  int64_t* out = idx_out + sg.ooff[s];
  const unsigned long long lt = (1ull << lane) - 1ull;
#pragma unroll
  for (int j = 0; j < kItems; ++j) {
    const bool g = (gbits >> j) & 1u, e = (ebits >> j) & 1u;
    const unsigned long long bg = __ballot(g), be = __ballot(e);
    if (!(g || e)) continue;
    const int gb = before.x + cg[4 * j + wave] + __popcll(bg & lt);
    const int eb = before.y + ce[4 * j + wave] + __popcll(be & lt);
    if (e && (unsigned)eb >= need) continue;                           // an equal key beyond the ties still needed
    const int pos = gb + (int)min((unsigned)eb, need);
    if (pos < m) out[pos] = (int64_t)base + (t0 + (long long)j * kThreads + t);      // (pos < k always: #above == k - need)
  }
}

// exclusive scan of a segment's per-tile (above, equal) counts: decode_scan_kernel's shape, one workgroup per segment
__global__ void __launch_bounds__(1024) topk_scan_kernel(const TopkSegs sg, int k, int nbmax, int2* __restrict__ blk_all) {
  __shared__ int pa[1024], pb[1024];
  __shared__ int carry[2];
  const int s = blockIdx.x;
  const int n = sg.off[s + 1] - sg.off[s];
  if (n <= k) return;                                                  // block-uniform
  const int nblk = (int)(((long long)n + kTile - 1) / kTile);
  int2* blk = blk_all + (size_t)s * nbmax;
  if (threadIdx.x == 0) { carry[0] = 0; carry[1] = 0; }
  __syncthreads();
  for (int b0 = 0; b0 < nblk; b0 += 1024) {
    const int i = b0 + threadIdx.x;
    const int2 v = i < nblk ? blk[i] : make_int2(0, 0);
    pa[threadIdx.x] = v.x; pb[threadIdx.x] = v.y;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
      const int aa = threadIdx.x >= o ? pa[threadIdx.x - o] : 0, ab = threadIdx.x >= o ? pb[threadIdx.x - o] : 0;
      __syncthreads();
      pa[threadIdx.x] += aa; pb[threadIdx.x] += ab;
      __syncthreads();
    }
    const int ia = pa[threadIdx.x], ib = pb[threadIdx.x];
    if (i < nblk) blk[i] = make_int2(carry[0] + ia - v.x, carry[1] + ib - v.y);
    __syncthreads();
    if (threadIdx.x == 1023) { carry[0] += ia; carry[1] += ib; }
    __syncthreads();
  }
}

}  // namespace

static inline size_t topk_align256(size_t x) { return (x + 255) & ~(size_t)255; }

// validates the table (tf_nms_f64_batched's refusals); total = sum of min(n_s, k), nmax = the longest segment that has to be cut (0: none)
static bool topk_table(const int32_t* off, int S, int k, TopkSegs* sg, long long* total, int* nmax) {
  if (!off || S <= 0 || S > kMaxSeg || off[0] != 0 || k < 1) return false;
  long long tot = 0;
  int mx = 0;
  for (int s = 0; s < S; ++s) {
    const int ns = off[s + 1] - off[s];
    if (ns < 0 || off[s + 1] < 0) return false;
    if (ns > k && ns > mx) mx = ns;
    if (sg) sg->ooff[s] = (int)tot;
    tot += ns < k ? ns : k;
  }
  if (sg) {
    for (int s = 0; s <= kMaxSeg; ++s) sg->off[s] = off[s < S ? s : S];
    for (int s = S; s < kMaxSeg; ++s) sg->ooff[s] = 0;
  }
  *total = tot; *nmax = mx;
  return true;
}

static inline size_t topk_hist_bytes(int S) { return topk_align256((size_t)kPasses * S * kBins * sizeof(unsigned)); }
static inline int topk_tiles(int n) { return (int)(((long long)n + kTile - 1) / kTile); }

extern "C" size_t tf_topk_batched_workspace_bytes(const int32_t* host_seg_offsets, int num_segments, int k) {
  long long total = 0;
  int nmax = 0;
  if (!topk_table(host_seg_offsets, num_segments, k, nullptr, &total, &nmax) || host_seg_offsets[num_segments] == 0) return 0;
  // (a table with nothing to cut still gets the histogram block: a non-zero size for every call that launches)
  return topk_hist_bytes(num_segments) + topk_align256((size_t)num_segments * topk_tiles(nmax) * sizeof(int2));
}

extern "C" size_t tf_topk_workspace_bytes(int n, int k) {
  if (n <= 0) return 0;
  const int32_t off[2] = {0, n};
  return tf_topk_batched_workspace_bytes(off, 1, k);
}

extern "C" int tf_topk_select_f64_batched(const double* scores, const int32_t* host_seg_offsets, int num_segments, int k, int64_t* idx_out,
                                          void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  const int S = num_segments;
  TopkSegs sg;
  long long total = 0;
  int nmax = 0;
  if (!topk_table(host_seg_offsets, S, k, &sg, &total, &nmax)) return TF_ERR_ARG;
  const int n = host_seg_offsets[S];
  if (n == 0) return TF_OK;                                            // nothing is launched
  if (!scores || !idx_out) return TF_ERR_ARG;
  if (!ws || ws_bytes < tf_topk_batched_workspace_bytes(host_seg_offsets, S, k)) return TF_ERR_ARG;
  int nlong = 0;                                                       // the write launch also copies the segments passed through whole
  for (int s = 0; s < S; ++s) nlong = host_seg_offsets[s + 1] - host_seg_offsets[s] > nlong ? host_seg_offsets[s + 1] - host_seg_offsets[s] : nlong;
  unsigned* hist = (unsigned*)ws;
  int2* blk = (int2*)((char*)ws + topk_hist_bytes(S));
  const int nbmax = topk_tiles(nmax);
  if (nmax > 0) {
    if (hipMemsetAsync(hist, 0, (size_t)kPasses * S * kBins * sizeof(unsigned), stream) != hipSuccess) return TF_ERR_LAUNCH;
    for (int pass = 0; pass < kPasses; ++pass)
      hipLaunchKernelGGL(topk_hist_kernel, dim3(nbmax, S), dim3(kThreads), 0, stream, scores, sg, k, pass, S, hist);
    hipLaunchKernelGGL(topk_compact_kernel<0>, dim3(nbmax, S), dim3(kThreads), 0, stream, scores, sg, k, S, nbmax, hist, blk, idx_out);
    hipLaunchKernelGGL(topk_scan_kernel, dim3(S), dim3(1024), 0, stream, sg, k, nbmax, blk);
  }
  hipLaunchKernelGGL(topk_compact_kernel<1>, dim3(topk_tiles(nlong), S), dim3(kThreads), 0, stream, scores, sg, k, S, nbmax, hist, blk, idx_out);
  TF_CHECK_LAUNCH();
  return TF_OK;
}

extern "C" int tf_topk_select_f64(const double* scores, int n, int k, int64_t* idx_out, void* ws, size_t ws_bytes, void* stream_) {
  if (n < 0) return TF_ERR_ARG;
  const int32_t off[2] = {0, n};
  return tf_topk_select_f64_batched(scores, off, 1, k, idx_out, ws, ws_bytes, stream_);
}
