// Task-aligned target assignment (the rule: include/tinyfaces_hip.h, "TAL"; numpy restatement: tests/tal_ref.py).  The one assigner that reads
// the network's own output: for every face the candidates are the anchors whose centre lies strictly inside it, each is measured by
// m = sigmoid(z)^alpha * u^beta with u the IoU of the anchor's PREDICTED box with the face, the face claims its topk candidates of largest m,
// and an anchor several faces claim goes to the larger u, then the lower face.  The anchor geometry is anchor_at of csrc/targets_shared.h, the
// unpadded rectangle of a template is unpadded_range of the same header (ATSS's own predicate), image_of comes from there as well.
// Compiled with -ffp-contract=off (build.py EXACT): every f64 op must round exactly like numpy's (exp and pow are the library's: a selection
// they decide by less than their error is what tests/tal_ref.py calls ambiguous).
//
// Four stream-ordered launches, no memset, and the two maps are only written where a face wins:
//   init    grid-stride over the B * nt * vsy * vsx anchors: the two claim words of the anchor cleared (workspace only)
//   claim   one 256-thread workgroup per face: its window of cells, all templates, m and u of every candidate, its topk, and for each winner an
//           atomicMax of u's bit pattern on the anchor's word (positive doubles order as unsigned integers; u > 0 for every candidate, so 0
//           means "unclaimed")
//   owner   one wave per face: atomicMin of the face index on every winner whose claim equals the maximum
//   write   one wave per face: +1, the four regression values and match_count for the anchors it won
// Integer atomics only, so the bits do not depend on arrival order; no grid barrier, no host synchronisation.
//
// Selection: per-tile partial top-k merged through LDS, not the compensation stage's rounds behind the previous winner.  A round costs one walk
// over the face's whole window and every walk re-evaluates two exp and two pow in float64 per candidate; topk = 13 rounds would pay that 13
// times, the merge pays it once.  The window is walked in tiles of 256 candidates (one per thread).  LDS holds the running list of at most 32
// best (m, u, anchor) next to the tile; a candidate that cannot enter the list (it does not beat the list's last entry once the list is full)
// is dropped at once, a tile without a survivor is skipped, and otherwise the <= 288 entries are ranked by counting with the rule's own total
// order (m descending, then the lower anchor index) and the first topk become the new list.  The order is total and the anchors of one face are
// distinct, so the list after the last tile does not depend on how the window was cut into tiles.  Nothing is bounded by LDS: the templates pass
// in tiles of 64 (their windows' rectangles and a prefix sum of their sizes), the candidates of such a tile in tiles of 256.
// The winners of a face (<= 32 anchors and their keys) are kept in the workspace for owner and write; there is no candidate list anywhere.
//
// tf_targets_tal_aligned (step 7 of the rule) is the same four launches with the aligned instantiations of init, claim and write: init also
// stores 1.0f to every element of align_map, claim keeps the m it ranked by next to the winner's key (the bits themselves, not a value formed
// again), and write -- one wave per face -- takes the maxima of m and of u over the lanes that WON by wave shuffles and stores
// (float)((m / M_g) * U_g) beside the +1.  The kernels are templates over their parameter block: tf_targets_tal instantiates them with
// TalParams and is, kernel argument for kernel argument, what it was.
#include <type_traits>

#include "targets_shared.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxTop = 32;                        // topk <= 32: the running list
constexpr int kEntries = kMaxTop + kThreads;       // list + one tile
constexpr int kTplTile = 64;                       // templates whose rectangles are resident at a time
constexpr int kWave = 64;                          // owner / write: one wave per face (<= 32 winners)
constexpr double kBoxClip = 4.135166556742356;     // log(1000 / 16), the clamp of the overlap losses (csrc/criterion_shared.h), here as a double

struct TalParams {
  const float* out;                                // [B][5 nt][vsy][vsx]: nt class logits, then px, py, pw, ph of every template
  const double* boxes; const int32_t* box_off; const double* tpl; int B, nt, tstride;
  int vsy, vsx, ofy, ofx, sty, stx;
  const int32_t* paste; const int32_t* flips;
  int topk; double alpha, beta; int nslots;
  int32_t* match_count; float* cls; float* reg;
  unsigned long long* amax;                        // [B * A]   per anchor: the largest claim key, 0 = unclaimed
  unsigned int* aown;                              // [B * A]   per anchor: the lowest face index among the claims that hold the maximum
  unsigned long long* wkey;                        // [nslots * 32]   per winner: the bit pattern of u
  int32_t* widx;                                   // [nslots * 32]   per winner: t * cells + cell
  int32_t* nwin;                                   // [nslots]
};

struct TalAlignedParams : TalParams {              // tf_targets_tal_aligned: step 7
  float* align;                                    // [B * A]   1.0f everywhere, the normalised alignment at the anchors won
  double* wm;                                      // [nslots * 32]   per winner: the m the claim kernel ranked it by
};
template <class P> constexpr bool kAligned = std::is_same<P, TalAlignedParams>::value;

// [a, b] = the indices i of [lo, hi] whose anchor centre lies strictly between g1 and g2 (empty: a > b).  The centre is monotone in i: one
// division estimates each bound and the predicate itself corrects it, so the bounds are exact; a NaN face gives the empty range.
__device__ __forceinline__ void inside_range(int of, int st, int lo, int hi, double d1, double d2, double g1, double g2, int& a, int& b) {
  if (lo > hi) { a = 0; b = -1; return; }
  const double c0 = (d1 + d2) / 2.0 + (double)of;
  a = clamp_to_int(floor((g1 - c0) / (double)st) + 1.0, lo, hi + 1);
  while (a > lo && centre(of, st, a - 1, d1, d2) > g1) --a;
  while (a <= hi && !(centre(of, st, a, d1, d2) > g1)) ++a;
  b = clamp_to_int(ceil((g2 - c0) / (double)st) - 1.0, lo - 1, hi);
  while (b < hi && centre(of, st, b + 1, d1, d2) < g2) ++b;
  while (b >= lo && !(centre(of, st, b, d1, d2) < g2)) --b;
}

struct Face { double gx1, gy1, gx2, gy2, fcx, fcy, bw, bh; int b; bool flip; };
struct Rect { int x0, y0, wx, wy; };

// the unpadded rectangle of template tp in the face's image (ATSS's predicate, under paste box and flip)
__device__ __forceinline__ void unpadded_rect(const TalParams& p, const Face& f, const double* tp, int& xlo, int& xhi, int& ylo, int& yhi) {
  xlo = 0; xhi = p.vsx - 1; ylo = 0; yhi = p.vsy - 1;
  if (p.paste) {
    const int32_t* pb = p.paste + 4 * f.b;
    unpadded_range(p.ofx, p.stx, p.vsx, tp[0], tp[2], pb[0], pb[2], xlo, xhi);
    unpadded_range(p.ofy, p.sty, p.vsy, tp[1], tp[3], pb[1], pb[3], ylo, yhi);
    if (f.flip) { const int l = p.vsx - 1 - xhi; xhi = p.vsx - 1 - xlo; xlo = l; }           // the mask is mirrored, the anchors are not
  }
}

// the window of the face in template t: the unpadded cells whose anchor centre lies strictly inside it
__device__ __forceinline__ Rect inside_rect(const TalParams& p, const Face& f, int t) {
  const double* tp = p.tpl + (size_t)t * p.tstride;
  int xlo, xhi, ylo, yhi, xa, xb, ya, yb;
  unpadded_rect(p, f, tp, xlo, xhi, ylo, yhi);
  inside_range(p.ofx, p.stx, xlo, xhi, tp[0], tp[2], f.gx1, f.gx2, xa, xb);
  inside_range(p.ofy, p.sty, ylo, yhi, tp[1], tp[3], f.gy1, f.gy2, ya, yb);
  Rect r; r.x0 = xa; r.y0 = ya; r.wx = xb >= xa ? xb - xa + 1 : 0; r.wy = yb >= ya ? yb - ya + 1 : 0;
  if (r.wx == 0 || r.wy == 0) { r.wx = 0; r.wy = 0; }
  return r;
}

// the face without a window: per template the single unpadded cell nearest its centre, ATSS's candidate at k = 1 (squared distance of the
// anchor centre ascending, the lower cell index on a tie).  As there, the two nearest columns x the two nearest rows hold it whatever the
// rounded sum of the two axis terms ties on.
__device__ __forceinline__ Rect nearest_rect(const TalParams& p, const Face& f, int t) {
  const double* tp = p.tpl + (size_t)t * p.tstride;
  int xlo, xhi, ylo, yhi;
  unpadded_rect(p, f, tp, xlo, xhi, ylo, yhi);
  Rect r; r.x0 = 0; r.y0 = 0; r.wx = 0; r.wy = 0;
  if (xlo > xhi || ylo > yhi) return r;
  const int wx = min(2, xhi - xlo + 1), wy = min(2, yhi - ylo + 1);
  const int x0 = nearest_window(p.ofx, p.stx, xlo, xhi, wx, tp[0], tp[2], f.fcx);
  const int y0 = nearest_window(p.ofy, p.sty, ylo, yhi, wy, tp[1], tp[3], f.fcy);
  double bd = 0.0;
  int bc = -1;
  for (int j = 0; j < wy; ++j)
    for (int i = 0; i < wx; ++i) {
      const double ex = sqdist(p.ofx, p.stx, x0 + i, tp[0], tp[2], f.fcx), ey = sqdist(p.ofy, p.sty, y0 + j, tp[1], tp[3], f.fcy);
      const double d = ex + ey;
      const int cell = (y0 + j) * p.vsx + (x0 + i);
      if (bc < 0 || d < bd) { bd = d; bc = cell; }                              // ascending cell order: the first of the smallest stays
    }
  r.y0 = bc / p.vsx; r.x0 = bc - r.y0 * p.vsx; r.wx = 1; r.wy = 1;
  return r;
}

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN and Inf

template <class P>
__global__ void __launch_bounds__(kThreads) tal_init_kernel(P p) {
  if (p.box_off[p.B] > p.nslots) return;                                       // more boxes than the workspace has slots for: touch nothing
  const size_t BA = (size_t)p.B * p.nt * p.vsy * p.vsx;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < BA; i += (size_t)gridDim.x * kThreads) {
    p.amax[i] = 0ull;
    p.aown[i] = 0xffffffffu;
    if constexpr (kAligned<P>) p.align[i] = 1.f;                                // an anchor labelled +1 by something else keeps the hard target
  }
}

template <class P>
__global__ void __launch_bounds__(kThreads) tal_claim_kernel(P p) {
  __shared__ double e_m[kEntries], e_u[kEntries];  // [0, 32): the running list, best first; [32, 288): the tile.  m < 0: no entry
  __shared__ int e_i[kEntries];
  __shared__ double n_m[kMaxTop], n_u[kMaxTop];    // the list of the next tile, while the ranks are being formed
  __shared__ int n_i[kMaxTop];
  __shared__ int s_x0[kTplTile], s_y0[kTplTile], s_wx[kTplTile], s_pre[kTplTile + 1];
  const int gi = blockIdx.x;
  const int total = p.box_off[p.B];
  if (total > p.nslots || gi >= total) return;
  const int tid = threadIdx.x;
  Face f;
  f.b = image_of(p.box_off, gi);
  const double* bx = p.boxes + 4 * (size_t)gi;
  f.gx1 = bx[0]; f.gy1 = bx[1]; f.gx2 = bx[2]; f.gy2 = bx[3];
  f.fcx = (f.gx1 + f.gx2) / 2.0; f.fcy = (f.gy1 + f.gy2) / 2.0;
  f.bw = f.gx2 - f.gx1 + 1.0; f.bh = f.gy2 - f.gy1 + 1.0;
  f.flip = p.paste && p.flips && p.flips[f.b];
  const double barea = f.bw * f.bh;
  const double fx1 = f.fcx - f.bw / 2.0, fx2 = f.fcx + f.bw / 2.0, fy1 = f.fcy - f.bh / 2.0, fy2 = f.fcy + f.bh / 2.0;
  const int cells = p.vsy * p.vsx;
  const size_t E = (size_t)p.nt * cells;
  const float* out = p.out + (size_t)f.b * 5 * E;

  // does any template have a window?  (if none: the nearest-cell rule)
  int any = 0;
  for (int t = tid; t < p.nt; t += kThreads) any |= inside_rect(p, f, t).wx > 0 ? 1 : 0;
  any = __syncthreads_or(any);
  if (tid < kMaxTop) e_m[tid] = -1.0;
  int ntop = 0;                                                                // block-uniform

  for (int t0 = 0; t0 < p.nt; t0 += kTplTile) {
    __syncthreads();                                                           // the previous tile's readers are done
    if (tid < kTplTile) {
      Rect r; r.x0 = 0; r.y0 = 0; r.wx = 0; r.wy = 0;
      if (t0 + tid < p.nt) r = any ? inside_rect(p, f, t0 + tid) : nearest_rect(p, f, t0 + tid);
      s_x0[tid] = r.x0; s_y0[tid] = r.y0; s_wx[tid] = r.wx; s_pre[tid + 1] = r.wx * r.wy;      // <= cells; the sum over a tile <= nt * cells < 2^31
    }
    __syncthreads();
    if (tid == 0) {
      s_pre[0] = 0;
      for (int i = 0; i < kTplTile; ++i) s_pre[i + 1] += s_pre[i];
    }
    __syncthreads();
    const int ncand = s_pre[kTplTile];
    for (int c0 = 0; c0 < ncand; c0 += kThreads) {
      const int c = c0 + tid;
      double m = -1.0, u = 0.0;
      int flat = 0x7fffffff;
      if (c < ncand) {
        int ti = 0;
#pragma unroll
        for (int s = kTplTile / 2; s > 0; s >>= 1) ti += (s_pre[ti + s] <= c) ? s : 0;       // the last template whose prefix is <= c
        const int local = c - s_pre[ti], wx = s_wx[ti];
        const int ry = local / wx;
        const int y = s_y0[ti] + ry, x = s_x0[ti] + (local - ry * wx), t = t0 + ti;
        const int cell = y * p.vsx + x;
        const size_t oi = (size_t)t * cells + cell;
        const double z = (double)out[oi];
        const double px = (double)out[oi + E], py = (double)out[oi + 2 * E], pw = (double)out[oi + 3 * E], ph = (double)out[oi + 4 * E];
        if (finite_d(z) && finite_d(px) && finite_d(py) && finite_d(pw) && finite_d(ph)) {
          const double* tp = p.tpl + (size_t)t * p.tstride;
          const Anchor an = anchor_at(tp[0], tp[1], tp[2], tp[3], p.ofy, p.ofx, p.sty, p.stx, y, x);
          const double cx = (double)p.ofx + (double)x * ((double)p.stx / 1.0), cy = (double)p.ofy + (double)y * ((double)p.sty / 1.0);
          const double bcx = cx + px * an.fw, bcy = cy + py * an.fh;
          const double w = an.fw * exp(fmin(fmax(pw, -kBoxClip), kBoxClip)), h = an.fh * exp(fmin(fmax(ph, -kBoxClip), kBoxClip));
          const double hx = w / 2.0, hy = h / 2.0;
          const double iw = fmin(bcx + hx, fx2) - fmax(bcx - hx, fx1), ih = fmin(bcy + hy, fy2) - fmax(bcy - hy, fy1);
          if (iw > 0.0 && ih > 0.0) {
            const double ia = iw * ih;
            u = ia / (w * h + barea - ia);
          }
          if (u > 0.0) {
            const double s = 1.0 / (1.0 + exp(-z));
            const double mm = pow(s, p.alpha) * pow(u, p.beta);
            if (finite_d(mm)) { m = mm; flat = (int)oi; }
          }
        }
      }
      bool live = m >= 0.0;
      if (live && ntop == p.topk) {                                            // a full list: only what beats its last entry can enter
        const double lm = e_m[p.topk - 1];
        live = m > lm || (m == lm && flat < e_i[p.topk - 1]);
      }
      const int nlive = __syncthreads_count(live ? 1 : 0);
      if (nlive == 0) continue;                                                // block-uniform
      e_m[kMaxTop + tid] = live ? m : -1.0; e_u[kMaxTop + tid] = u; e_i[kMaxTop + tid] = flat;
      __syncthreads();
      for (int i = tid; i < kEntries; i += kThreads) {
        const double mi = e_m[i];
        if (!(mi >= 0.0)) continue;
        const int ii = e_i[i];
        int rank = 0;
#pragma unroll 8
        for (int j = 0; j < kEntries; ++j) {
          const double mj = e_m[j];
          rank += (mj > mi || (mj == mi && e_i[j] < ii)) ? 1 : 0;
        }
        if (rank < p.topk) { n_m[rank] = mi; n_u[rank] = e_u[i]; n_i[rank] = ii; }
      }
      __syncthreads();
      ntop = min(p.topk, ntop + nlive);
      if (tid < kMaxTop) {
        const bool in = tid < ntop;
        e_m[tid] = in ? n_m[tid] : -1.0; e_u[tid] = in ? n_u[tid] : 0.0; e_i[tid] = in ? n_i[tid] : 0x7fffffff;
      }
      __syncthreads();
    }
  }
  __syncthreads();
  if (tid == 0) p.nwin[gi] = ntop;
  if (tid < ntop) {
    const unsigned long long key = (unsigned long long)__double_as_longlong(e_u[tid]);
    const int a = e_i[tid];
    p.wkey[(size_t)gi * kMaxTop + tid] = key;
    p.widx[(size_t)gi * kMaxTop + tid] = a;
    if constexpr (kAligned<P>) p.wm[(size_t)gi * kMaxTop + tid] = e_m[tid];
    atomicMax(&p.amax[(size_t)f.b * E + a], key);
  }
}

__global__ void __launch_bounds__(kWave) tal_owner_kernel(TalParams p) {
  const int gi = blockIdx.x;
  const int total = p.box_off[p.B];
  if (total > p.nslots || gi >= total) return;
  if ((int)threadIdx.x >= p.nwin[gi]) return;
  const size_t img = (size_t)image_of(p.box_off, gi) * p.nt * p.vsy * p.vsx;
  const size_t a = img + p.widx[(size_t)gi * kMaxTop + threadIdx.x];
  if (p.wkey[(size_t)gi * kMaxTop + threadIdx.x] == p.amax[a]) atomicMin(&p.aown[a], (unsigned int)gi);     // faces of one image: the lower gi is the lower g
}

template <class P>
__global__ void __launch_bounds__(kWave) tal_write_kernel(P p) {
  const int gi = blockIdx.x;
  const int total = p.box_off[p.B];
  if (total > p.nslots || gi >= total) return;
  const int b = image_of(p.box_off, gi);
  const int cells = p.vsy * p.vsx;
  const size_t img = (size_t)b * p.nt * cells;
  bool won = false;
  int a = 0;
  unsigned long long key = 0ull;
  if ((int)threadIdx.x < p.nwin[gi]) {
    a = p.widx[(size_t)gi * kMaxTop + threadIdx.x];
    key = p.wkey[(size_t)gi * kMaxTop + threadIdx.x];
    won = key == p.amax[img + a] && p.aown[img + a] == (unsigned int)gi;
    if (won) {
      const double* bx = p.boxes + 4 * (size_t)gi;
      const double gx1 = bx[0], gy1 = bx[1], gx2 = bx[2], gy2 = bx[3];
      const double fcx = (gx1 + gx2) / 2.0, fcy = (gy1 + gy2) / 2.0;           // processor.py:181-182
      const int t = a / cells, cell = a - t * cells;
      const int y = cell / p.vsx, x = cell - y * p.vsx;
      const double* tp = p.tpl + (size_t)t * p.tstride;
      const double fh = tp[3] - tp[1] + 1.0, fw = tp[2] - tp[0] + 1.0;
      const double coarse_x = (double)(p.ofx + x * p.stx), coarse_y = (double)(p.ofy + y * p.sty);
      const size_t plane = (size_t)cells;
      p.cls[img + a] = 1.f;
      float* r = p.reg + ((size_t)b * 4 * p.nt + t) * plane + cell;
      r[0] = (float)((fcx - coarse_x) / fw);                                   // :184-185
      r[(size_t)p.nt * plane] = (float)((fcy - coarse_y) / fh);
      r[(size_t)2 * p.nt * plane] = (float)log((gx2 - gx1 + 1.0) / fw);        // :187-191
      r[(size_t)3 * p.nt * plane] = (float)log((gy2 - gy1 + 1.0) / fh);
    }
  }
  if constexpr (kAligned<P>) {                                                 // step 7: every lane of the wave takes part in the shuffles
    const double m = won ? p.wm[(size_t)gi * kMaxTop + threadIdx.x] : -1.0;    // m >= 0 and u > 0 for every winner
    const double u = won ? __longlong_as_double((long long)key) : 0.0;
    double M = m, U = u;
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
      const double vm = __shfl_xor(M, o, kWave), vu = __shfl_xor(U, o, kWave);
      M = vm > M ? vm : M;
      U = vu > U ? vu : U;
    }
    if (won) p.align[img + a] = M == 0.0 ? 0.f : (float)((m / M) * U);
  }
  if (!p.match_count) return;                                                  // kernel-uniform
  const int n = __popcll(__ballot(won));
  if (threadIdx.x == 0) p.match_count[gi] = n;
}

// per box slot: 32 winners of key (8) + anchor index (4) [+ m (8), aligned], and the winner count (4)
template <class P> inline size_t slot_bytes() { return (size_t)kMaxTop * (kAligned<P> ? 20 : 12) + 4; }

// workspace: per anchor the claim key (8) + the owner (4), per box slot slot_bytes()
template <class P> inline size_t workspace_bytes(int total_boxes, int B, int nt, int vsy, int vsx) {
  const size_t n = (size_t)(total_boxes > 0 ? total_boxes : 1);
  const size_t anchors = (size_t)(B > 0 ? B : 0) * (size_t)(nt > 0 ? nt : 0) * (size_t)(vsy > 0 ? vsy : 0) * (size_t)(vsx > 0 ? vsx : 0);
  return n * slot_bytes<P>() + anchors * 12 + 64;
}

}  // namespace

extern "C" size_t tf_targets_tal_workspace_bytes(int total_boxes, int B, int nt, int vsy, int vsx) {
  return workspace_bytes<TalParams>(total_boxes, B, nt, vsy, vsx);
}

extern "C" size_t tf_targets_tal_aligned_workspace_bytes(int total_boxes, int B, int nt, int vsy, int vsx) {
  return workspace_bytes<TalAlignedParams>(total_boxes, B, nt, vsy, vsx);
}

namespace {

// both entry points: the refusals, the workspace carved, the four launches
template <class P>
int tal_launch(const float* output, const double* boxes, const int32_t* box_offsets, int B, const double* templates, int nt, int tstride,
               int vsy, int vsx, int ofy, int ofx, int sty, int stx, const int32_t* paste_boxes, const int32_t* flips,
               int topk, double alpha, double beta, int32_t* match_count, float* class_map, float* reg_map, float* align_map,
               void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (B <= 0 || nt <= 0 || vsy <= 0 || vsx <= 0 || !output || !box_offsets || !templates || !class_map || !reg_map) return TF_ERR_ARG;
  if (tstride < 4 || sty <= 0 || stx <= 0) return TF_ERR_ARG;
  if (topk < 1 || topk > kMaxTop) return TF_ERR_ARG;
  if (!(alpha >= 0.0) || !(beta > 0.0) || std::isinf(alpha) || std::isinf(beta)) return TF_ERR_ARG;
  const size_t per_image = (size_t)nt * (size_t)vsy * (size_t)vsx;
  if (per_image > (size_t)0x7fffffff) return TF_ERR_UNSUPPORTED;               // t * cells + cell is int32
  // the cell coordinate of * st + of is formed in int32, as in tf_dense_overlap_targets
  if ((double)(vsx - 1) * stx + fabs((double)ofx) > 2147483647.0 || (double)(vsy - 1) * sty + fabs((double)ofy) > 2147483647.0) return TF_ERR_UNSUPPORTED;
  // total boxes is only known on device; the caller sizes ws from its host copy, and every kernel leaves at once if the device's total
  // exceeds the slots the workspace holds
  if (!ws || ws_bytes < workspace_bytes<P>(1, B, nt, vsy, vsx)) return TF_ERR_WORKSPACE;
  const size_t anchors = (size_t)B * per_image;
  size_t nslots = (ws_bytes - 64 - anchors * 12) / slot_bytes<P>();
  if (nslots > ((size_t)1 << 30)) nslots = (size_t)1 << 30;
  P p;
  p.out = output; p.boxes = boxes; p.box_off = box_offsets; p.tpl = templates; p.B = B; p.nt = nt; p.tstride = tstride;
  p.vsy = vsy; p.vsx = vsx; p.ofy = ofy; p.ofx = ofx; p.sty = sty; p.stx = stx;
  p.paste = paste_boxes; p.flips = flips; p.topk = topk; p.alpha = alpha; p.beta = beta; p.nslots = (int)nslots;
  p.match_count = match_count; p.cls = class_map; p.reg = reg_map;
  char* w = (char*)ws;                                                         // the 8-byte arrays first
  p.amax = (unsigned long long*)w;                 w += anchors * 8;
  p.wkey = (unsigned long long*)w;                 w += nslots * kMaxTop * 8;
  if constexpr (kAligned<P>) { p.align = align_map; p.wm = (double*)w; w += nslots * kMaxTop * 8; }
  p.aown = (unsigned int*)w;                       w += anchors * 4;
  p.widx = (int32_t*)w;                            w += nslots * kMaxTop * 4;
  p.nwin = (int32_t*)w;
  const size_t init_blocks = (anchors + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(tal_init_kernel<P>, dim3((unsigned)(init_blocks < 4096 ? init_blocks : 4096)), dim3(kThreads), 0, stream, p);
  hipLaunchKernelGGL(tal_claim_kernel<P>, dim3((unsigned)nslots), dim3(kThreads), 0, stream, p);
  hipLaunchKernelGGL(tal_owner_kernel, dim3((unsigned)nslots), dim3(kWave), 0, stream, p);
  hipLaunchKernelGGL(tal_write_kernel<P>, dim3((unsigned)nslots), dim3(kWave), 0, stream, p);
  TF_CHECK_LAUNCH();
  return TF_OK;
}

}  // namespace

extern "C" int tf_targets_tal(const float* output, const double* boxes, const int32_t* box_offsets, int B,
                              const double* templates, int nt, int tstride,
                              int vsy, int vsx, int ofy, int ofx, int sty, int stx,
                              const int32_t* paste_boxes, const int32_t* flips,
                              int topk, double alpha, double beta, int32_t* match_count,
                              float* class_map, float* reg_map,
                              void* ws, size_t ws_bytes, void* stream) {
  return tal_launch<TalParams>(output, boxes, box_offsets, B, templates, nt, tstride, vsy, vsx, ofy, ofx, sty, stx, paste_boxes, flips, topk, alpha, beta,
                               match_count, class_map, reg_map, nullptr, ws, ws_bytes, stream);
}

extern "C" int tf_targets_tal_aligned(const float* output, const double* boxes, const int32_t* box_offsets, int B,
                                      const double* templates, int nt, int tstride,
                                      int vsy, int vsx, int ofy, int ofx, int sty, int stx,
                                      const int32_t* paste_boxes, const int32_t* flips,
                                      int topk, double alpha, double beta, int32_t* match_count,
                                      float* class_map, float* reg_map, float* align_map,
                                      void* ws, size_t ws_bytes, void* stream) {
  if (!align_map) return TF_ERR_ARG;
  return tal_launch<TalAlignedParams>(output, boxes, box_offsets, B, templates, nt, tstride, vsy, vsx, ofy, ofx, sty, stx, paste_boxes, flips, topk, alpha,
                                      beta, match_count, class_map, reg_map, align_map, ws, ws_bytes, stream);
}
