// ATSS target assignment (the rule: include/tinyfaces_hip.h, "ATSS"; numpy restatement: tests/atss_ref.py).  Every face takes the k unpadded
// cells of every template nearest to its centre as candidates, thresholds their IoUs at mean + std, keeps the passing ones whose anchor centre
// lies strictly inside it (or, having none, its best candidate), and an anchor several faces claim goes to the larger IoU, then the lower face.
// The anchor whose IoU a candidate gets is anchor_at of csrc/targets_shared.h, the single definition csrc/targets.hip and
// csrc/targets_ignore.hip use too; image_of comes from there as well.  Everything else -- candidates, statistics, claims -- is this file's own.
// Compiled with -ffp-contract=off (build.py EXACT): every f64 op must round exactly like numpy's.
//
// Four stream-ordered launches, no memset:
//   init    grid-stride over the B * nt * vsy * vsx anchors: class_map = -1, reg_map = 0, the two claim words of the anchor cleared
//   claim   one workgroup per face: candidates, statistics, claims; a claim is an atomicMax of (IoU bit pattern + 1) on the anchor's word
//           (non-negative doubles order as unsigned integers; + 1 so that 0 means "unclaimed" and a fallback claim of IoU 0 still counts)
//   owner   one workgroup per face: atomicMin of the face index on every anchor where its claim equals the maximum
//   write   one workgroup per face: label, the four regression values and match_count for the anchors it won
// Integer atomics only, so the bits do not depend on arrival order; no grid barrier, no host synchronisation.
// The candidates of a face are KEPT in the workspace (16 * nt slots per box: anchor index + IoU, the IoU then replaced by the claim key or 0),
// not recomputed: owner and write only walk that list.
//
// Candidate selection.  The unpadded cells of a template form a rectangle [xlo, xhi] x [ylo, yhi]: the padding predicate is a disjunction of
// four one-sided tests, each monotone in the cell coordinate.  Its bounds are estimated by one division and then corrected with the predicate
// itself, so they are exact (unpadded_range, nearest_window, centre and sqdist live in csrc/targets_shared.h: the TAL assigner uses them too).  The squared distance is separable and each axis term is unimodal in the cell coordinate, so the k nearest cells
// lie inside the W nearest columns x the W nearest rows for any W >= k.  The window is chosen by the axis term alone while the rule ranks by
// the ROUNDED sum of both terms: two columns that mirror each other about a face centre a hair off a column centre can tie in the sum with
// unequal axis terms, and the rule then prefers the lower cell index.  The kernel therefore takes W = k + 1 at every k (up to 17 x 17 = 289
// cells), one column and one row more than needed, which holds both columns of such a pair (there is at most one pair per axis at the
// window's edge), and ranks the cells of that window by counting through LDS, at most two cells per thread, with the rule's own key
// (distance, then cell index).
#include "targets_shared.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxK = 16;                          // candidates per template and face
constexpr int kWindow = (kMaxK + 1) * (kMaxK + 1);  // cells of the largest window: 289, ranked by strided threads

struct AtssParams {
  const double* boxes; const int32_t* box_off; const double* tpl; int B, nt, tstride;
  int vsy, vsx, ofy, ofx, sty, stx;
  const int32_t* paste; const int32_t* flips;
  int k, nslots;
  int32_t* match_count; float* cls; float* reg;
  unsigned long long* amax;                        // [B * A]   per anchor: the largest claim key, 0 = unclaimed
  unsigned int* aown;                              // [B * A]   per anchor: the lowest face index among the claims that hold the maximum
  unsigned long long* cval;                        // [nslots * 16 * nt]   per candidate: the IoU (claim kernel, first half), then the claim key or 0
  int32_t* cidx;                                   // [nslots * 16 * nt]   per candidate: t * cells + cell
  int32_t* ncand;                                  // [nslots]
};

__global__ void __launch_bounds__(kThreads) atss_init_kernel(AtssParams p) {
  if (p.box_off[p.B] > p.nslots) return;                                       // more boxes than the workspace has slots for: touch nothing
  const size_t BA = (size_t)p.B * p.nt * p.vsy * p.vsx;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < BA; i += (size_t)gridDim.x * kThreads) {
    p.cls[i] = -1.f;
    p.reg[i] = 0.f; p.reg[BA + i] = 0.f; p.reg[2 * BA + i] = 0.f; p.reg[3 * BA + i] = 0.f;      // the map is 4 * BA contiguous floats
    p.amax[i] = 0ull;
    p.aown[i] = 0xffffffffu;
  }
}

__global__ void __launch_bounds__(kThreads) atss_claim_kernel(AtssParams p) {
  __shared__ double s_d[kWindow];                  // window: squared distance; statistics: one chunk of kThreads of the candidates' IoUs
  __shared__ int s_c[kWindow];                     // window: cell index
  __shared__ double s_mean, s_var;
  __shared__ int s_best;
  const int gi = blockIdx.x;
  const int total = p.box_off[p.B];
  if (total > p.nslots || gi >= total) return;
  const int b = image_of(p.box_off, gi);
  const double* bx = p.boxes + 4 * (size_t)gi;
  const double gx1 = bx[0], gy1 = bx[1], gx2 = bx[2], gy2 = bx[3];
  const double fcx = (gx1 + gx2) / 2.0, fcy = (gy1 + gy2) / 2.0;
  const double bw = gx2 - gx1 + 1.0, bh = gy2 - gy1 + 1.0, barea = bw * bh;
  const int cells = p.vsy * p.vsx;
  const size_t slot = (size_t)gi * kMaxK * p.nt;
  unsigned long long* cv = p.cval + slot;                                       // IoUs travel as their bit patterns
  int32_t* ci = p.cidx + slot;
  const bool flip = p.paste && p.flips && p.flips[b];
  const int W = p.k + 1;                                                       // <= kMaxK + 1: the spare column and row at every k
  const int tid = threadIdx.x;

  // 1. candidates, 2. their IoUs -> cv / ci in list order (t ascending, then rank)
  int n = 0;                                                                   // block-uniform
  for (int t = 0; t < p.nt; ++t) {
    const double* tp = p.tpl + (size_t)t * p.tstride;
    const double dx1 = tp[0], dy1 = tp[1], dx2 = tp[2], dy2 = tp[3];
    int xlo = 0, xhi = p.vsx - 1, ylo = 0, yhi = p.vsy - 1;
    if (p.paste) {
      const int32_t* pb = p.paste + 4 * b;
      unpadded_range(p.ofx, p.stx, p.vsx, dx1, dx2, pb[0], pb[2], xlo, xhi);
      unpadded_range(p.ofy, p.sty, p.vsy, dy1, dy2, pb[1], pb[3], ylo, yhi);
      if (flip) { const int l = p.vsx - 1 - xhi; xhi = p.vsx - 1 - xlo; xlo = l; }         // the mask is mirrored, the anchors are not
    }
    if (xlo > xhi || ylo > yhi) continue;                                      // no unpadded cell of this template
    const int wx = min(W, xhi - xlo + 1), wy = min(W, yhi - ylo + 1);
    const int x0 = nearest_window(p.ofx, p.stx, xlo, xhi, wx, dx1, dx2, fcx);
    const int y0 = nearest_window(p.ofy, p.sty, ylo, yhi, wy, dy1, dy2, fcy);
    const int m = wx * wy, nt_k = min(p.k, m);
    __syncthreads();                                                           // the previous template's readers are done
    for (int i = tid; i < m; i += kThreads) {                                  // at most two cells per thread (m <= 17 * 17)
      const int r = i / wx;
      const int y = y0 + r, x = x0 + (i - r * wx);
      const double ex = sqdist(p.ofx, p.stx, x, dx1, dx2, fcx), ey = sqdist(p.ofy, p.sty, y, dy1, dy2, fcy);
      s_d[i] = ex + ey; s_c[i] = y * p.vsx + x;
    }
    __syncthreads();
    for (int i = tid; i < m; i += kThreads) {
      const double d = s_d[i];
      const int cell = s_c[i];
      int rank = 0;
#pragma unroll 8
      for (int j = 0; j < m; ++j) {                                            // unrolled: the LDS reads of several keys are in flight together
        const double dj = s_d[j];
        rank += (dj < d || (!(dj > d) && s_c[j] < cell)) ? 1 : 0;                // !(>) is == for numbers; for a NaN box (every distance NaN) the cell index alone orders, so the ranks stay a permutation and every list slot is written
      }
      if (rank < nt_k) {
        const int y = cell / p.vsx, x = cell - y * p.vsx;
        const Anchor an = anchor_at(dx1, dy1, dx2, dy2, p.ofy, p.ofx, p.sty, p.stx, y, x);
        const double iw = fmin(an.x2, gx2) - fmax(an.x1, gx1) + 1.0, ih = fmin(an.y2, gy2) - fmax(an.y1, gy1) + 1.0;
        double v = 0.0;
        if (ih > 0.0 && iw > 0.0) {
          const double ia = iw * ih;
          v = ia / (an.farea + barea - ia);
        }
        cv[n + rank] = (unsigned long long)__double_as_longlong(v);
        ci[n + rank] = t * cells + cell;
      }
    }
    n += nt_k;
  }
  if (tid == 0) p.ncand[gi] = n;
  if (n == 0) return;                                                          // block-uniform: the face claims nothing

  // 3. mean and unbiased variance, summed serially in list order by one lane; the list passes through LDS in chunks of kThreads.  The same
  //    lane finds the fallback of step 5: the largest IoU, the earlier position on a tie.
  double sum = 0.0, bestv = -1.0;
  int besti = 0;
  for (int i0 = 0; i0 < n; i0 += kThreads) {
    const int m = min(kThreads, n - i0);
    __syncthreads();                                                           // cv is written; the previous chunk's reader is done
    if (tid < m) s_d[tid] = __longlong_as_double((long long)cv[i0 + tid]);
    __syncthreads();
    if (tid == 0)
      for (int j = 0; j < m; ++j) {
        const double v = s_d[j];
        sum = sum + v;
        if (v > bestv) { bestv = v; besti = i0 + j; }
      }
  }
  if (tid == 0) { s_mean = sum / (double)n; s_best = besti; }
  __syncthreads();
  const double mean = s_mean;
  double acc = 0.0;
  for (int i0 = 0; i0 < n; i0 += kThreads) {
    const int m = min(kThreads, n - i0);
    __syncthreads();
    if (tid < m) s_d[tid] = __longlong_as_double((long long)cv[i0 + tid]);
    __syncthreads();
    if (tid == 0)
      for (int j = 0; j < m; ++j) {
        const double dv = s_d[j] - mean;
        acc = acc + dv * dv;
      }
  }
  if (tid == 0) s_var = n > 1 ? acc / (double)(n - 1) : 0.0;
  __syncthreads();
  const double var = s_var;

  // 4. positive claims, 5. the fallback, 6. the claim itself.  Every thread owns the candidates i = tid, tid + kThreads, ...
  int any = 0;
  for (int i = tid; i < n; i += kThreads) {
    const double v = __longlong_as_double((long long)cv[i]);
    const double dv = v - mean;
    bool claim = dv >= 0.0 && dv * dv >= var;
    if (claim) {
      const int a = ci[i];
      const int t = a / cells, cell = a - t * cells;
      const int y = cell / p.vsx, x = cell - y * p.vsx;
      const double* tp = p.tpl + (size_t)t * p.tstride;
      const double acx = centre(p.ofx, p.stx, x, tp[0], tp[2]), acy = centre(p.ofy, p.sty, y, tp[1], tp[3]);
      claim = gx1 < acx && acx < gx2 && gy1 < acy && acy < gy2;
    }
    any |= claim ? 1 : 0;
    cv[i] = claim ? (unsigned long long)__double_as_longlong(v) + 1ull : 0ull;
  }
  any = __syncthreads_or(any);
  if (!any && tid == 0) cv[s_best] = (unsigned long long)__double_as_longlong(bestv) + 1ull;     // (thread 0 holds bestv)
  __syncthreads();                                                             // the keys are written
  const size_t img = (size_t)b * p.nt * cells;
  for (int i = tid; i < n; i += kThreads) {
    const unsigned long long key = cv[i];
    if (key) atomicMax(&p.amax[img + ci[i]], key);
  }
}

__global__ void __launch_bounds__(kThreads) atss_owner_kernel(AtssParams p) {
  const int gi = blockIdx.x;
  const int total = p.box_off[p.B];
  if (total > p.nslots || gi >= total) return;
  const int n = p.ncand[gi];
  if (n == 0) return;
  const size_t img = (size_t)image_of(p.box_off, gi) * p.nt * p.vsy * p.vsx;
  const size_t slot = (size_t)gi * kMaxK * p.nt;
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const unsigned long long key = p.cval[slot + i];
    const size_t a = img + p.cidx[slot + i];
    if (key && key == p.amax[a]) atomicMin(&p.aown[a], (unsigned int)gi);      // faces of one image: the lower gi is the lower g
  }
}

__global__ void __launch_bounds__(kThreads) atss_write_kernel(AtssParams p) {
  __shared__ int s_won;
  const int gi = blockIdx.x;
  const int total = p.box_off[p.B];
  if (total > p.nslots || gi >= total) return;
  const int n = p.ncand[gi];
  if (threadIdx.x == 0) s_won = 0;
  __syncthreads();
  const int b = image_of(p.box_off, gi);
  const int cells = p.vsy * p.vsx;
  const size_t img = (size_t)b * p.nt * cells;
  const size_t slot = (size_t)gi * kMaxK * p.nt;
  const double* bx = p.boxes + 4 * (size_t)gi;
  const double gx1 = bx[0], gy1 = bx[1], gx2 = bx[2], gy2 = bx[3];
  const double fcx = (gx1 + gx2) / 2.0, fcy = (gy1 + gy2) / 2.0;               // processor.py:181-182
  int won = 0;
  for (int i = threadIdx.x; i < n; i += kThreads) {
    const unsigned long long key = p.cval[slot + i];
    const int a = p.cidx[slot + i];
    if (!key || key != p.amax[img + a] || p.aown[img + a] != (unsigned int)gi) continue;
    const int t = a / cells, cell = a - t * cells;
    const int y = cell / p.vsx, x = cell - y * p.vsx;
    const double* tp = p.tpl + (size_t)t * p.tstride;
    const double fh = tp[3] - tp[1] + 1.0, fw = tp[2] - tp[0] + 1.0;
    const double coarse_x = (double)(p.ofx + x * p.stx), coarse_y = (double)(p.ofy + y * p.sty);
    const size_t plane = (size_t)cells;
    p.cls[img + a] = 1.f;
    float* r = p.reg + ((size_t)b * 4 * p.nt + t) * plane + cell;
    r[0] = (float)((fcx - coarse_x) / fw);                                     // :184-185
    r[(size_t)p.nt * plane] = (float)((fcy - coarse_y) / fh);
    r[(size_t)2 * p.nt * plane] = (float)log((gx2 - gx1 + 1.0) / fw);          // :187-191
    r[(size_t)3 * p.nt * plane] = (float)log((gy2 - gy1 + 1.0) / fh);
    ++won;
  }
  if (!p.match_count) return;                                                  // kernel-uniform
  if (won) atomicAdd(&s_won, won);                                             // LDS, integer: order-free
  __syncthreads();
  if (threadIdx.x == 0) p.match_count[gi] = s_won;
}

// per box slot: 16 * nt candidates of key (8) + anchor index (4), and the candidate count (4)
inline size_t slot_bytes(int nt) { return (size_t)kMaxK * (size_t)nt * 12 + 4; }

}  // namespace

// workspace: per anchor the claim key (8) + the owner (4), per box slot slot_bytes(nt)
extern "C" size_t tf_targets_atss_workspace_bytes(int total_boxes, int B, int nt, int vsy, int vsx) {
  const size_t n = (size_t)(total_boxes > 0 ? total_boxes : 1);
  const size_t anchors = (size_t)(B > 0 ? B : 0) * (size_t)(nt > 0 ? nt : 0) * (size_t)(vsy > 0 ? vsy : 0) * (size_t)(vsx > 0 ? vsx : 0);
  return n * slot_bytes(nt > 0 ? nt : 0) + anchors * 12 + 64;
}

extern "C" int tf_targets_atss(const double* boxes, const int32_t* box_offsets, int B,
                               const double* templates, int nt, int tstride,
                               int vsy, int vsx, int ofy, int ofx, int sty, int stx,
                               const int32_t* paste_boxes, const int32_t* flips,
                               int k, int32_t* match_count,
                               float* class_map, float* reg_map,
                               void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B <= 0 || nt <= 0 || vsy <= 0 || vsx <= 0 || !box_offsets || !templates || !class_map || !reg_map) return TF_ERR_ARG;
  if (tstride < 4 || sty <= 0 || stx <= 0) return TF_ERR_ARG;
  if (k < 1 || k > kMaxK) return TF_ERR_ARG;
  const size_t per_image = (size_t)nt * (size_t)vsy * (size_t)vsx;
  if (per_image > (size_t)0x7fffffff || (size_t)nt * kMaxK > (size_t)0x7fffffff) return TF_ERR_UNSUPPORTED;      // t * cells + cell and the list position are int32
  // the cell coordinate of * st + of is formed in int32, as in tf_dense_overlap_targets
  if ((double)(vsx - 1) * stx + fabs((double)ofx) > 2147483647.0 || (double)(vsy - 1) * sty + fabs((double)ofy) > 2147483647.0) return TF_ERR_UNSUPPORTED;
  // total boxes is only known on device; the caller sizes ws from its host copy, and every kernel leaves at once if the device's total
  // exceeds the slots the workspace holds
  if (!ws || ws_bytes < tf_targets_atss_workspace_bytes(1, B, nt, vsy, vsx)) return TF_ERR_WORKSPACE;
  const size_t anchors = (size_t)B * per_image;
  size_t nslots = (ws_bytes - 64 - anchors * 12) / slot_bytes(nt);
  if (nslots > ((size_t)1 << 30)) nslots = (size_t)1 << 30;
  AtssParams p;
  p.boxes = boxes; p.box_off = box_offsets; p.tpl = templates; p.B = B; p.nt = nt; p.tstride = tstride;
  p.vsy = vsy; p.vsx = vsx; p.ofy = ofy; p.ofx = ofx; p.sty = sty; p.stx = stx;
  p.paste = paste_boxes; p.flips = flips; p.k = k; p.nslots = (int)nslots;
  p.match_count = match_count; p.cls = class_map; p.reg = reg_map;
  char* w = (char*)ws;                                                         // the 8-byte arrays first
  p.amax = (unsigned long long*)w;                 w += anchors * 8;
  p.cval = (unsigned long long*)w;                 w += nslots * kMaxK * nt * 8;
  p.aown = (unsigned int*)w;                       w += anchors * 4;
  p.cidx = (int32_t*)w;                            w += nslots * kMaxK * nt * 4;
  p.ncand = (int32_t*)w;
  const size_t init_blocks = (anchors + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(atss_init_kernel, dim3((unsigned)(init_blocks < 4096 ? init_blocks : 4096)), dim3(kThreads), 0, stream, p);
  hipLaunchKernelGGL(atss_claim_kernel, dim3((unsigned)nslots), dim3(kThreads), 0, stream, p);
  hipLaunchKernelGGL(atss_owner_kernel, dim3((unsigned)nslots), dim3(kThreads), 0, stream, p);
  hipLaunchKernelGGL(atss_write_kernel, dim3((unsigned)nslots), dim3(kThreads), 0, stream, p);
  TF_CHECK_LAUNCH();
  return TF_OK;
}
