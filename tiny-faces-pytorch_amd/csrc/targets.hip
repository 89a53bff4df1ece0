// dense_overlap anchor-IoU + heat-map target assignment, fused, float64-exact.
// Replaces tinyfaces/datasets/dense_overlap.py:4-75 + processor.py:114-277 (see tinyfaces_hip.h).
// Compiled with -ffp-contract=off: every f64 op must round exactly like numpy's.
//
// HBM-write bound by design: one thread per (template, y, x) anchor, x fastest so the
// [B][5nt][vsy][vsx] float maps are written fully coalesced; boxes are wave-uniform scalar
// loads; the (vsy,vsx,nt,G) IoU tensor only ever exists in registers.
// Three stream-ordered phases:
//   A  per anchor: best GT (first arg-max of perturbed IoU), labels, regression targets;
//      per GT: atomicMax of the perturbed-IoU bit pattern (only values > neg_thresh matter)
//   B  per anchor: recompute, atomicMin the C-order flat index of anchors that hit that max
//   C  per GT: label its best anchor +1 (processor.py:252-257) unless padded (:272-273)
// tf_dense_overlap_targets_comp adds the scale-compensation stage (contract in tinyfaces_hip.h): phase A also stores every anchor's owner
// and best perturbed IoU, then
//   D  per anchor: count the positives each GT owns (integer atomics, one per wave and owner)
//   E  per GT, one workgroup: promote its N - count best candidates, one block arg-max per promotion
// Shared with csrc/targets_ignore.hip and csrc/targets_atss.hip through csrc/targets_shared.h: the anchor geometry (anchor_at, its single
// definition), the image lookup (image_of) and the operand block of the two entry points (TgtParams, base_params).
#include "targets_shared.h"

namespace {

// IoU of anchor (template t at cell y,x) with box g, rounded to 14 decimals: dense_overlap.py:32-75
__device__ __forceinline__ double iou14(double x1, double y1, double x2, double y2, double farea,
                                        double gx1, double gy1, double gx2, double gy2) {
  double bw = gx2 - gx1 + 1.0, bh = gy2 - gy1 + 1.0;
  double barea = bw * bh;
  double xx1 = fmax(x1, gx1), yy1 = fmax(y1, gy1), xx2 = fmin(x2, gx2), yy2 = fmin(y2, gy2);
  double iw = xx2 - xx1 + 1.0, ih = yy2 - yy1 + 1.0;
  double ov = 0.0;
  if (ih > 0.0 && iw > 0.0) {
    double ia = iw * ih;
    double un = farea + barea - ia;
    ov = ia / un;
  }
  return rint(ov * 1e14) / 1e14;   // np.around(x, 14) == rint(x * 1e14) / 1e14
}

__device__ __forceinline__ double noise_at(const TgtParams& p, int b, int flat, int g, int G) {
  if (p.noise) return p.noise[p.noise_off[b] + (int64_t)flat * G + g];
  return tf::u01(tf::hash4(p.seed, (uint64_t)b, (uint64_t)flat, (uint64_t)g));
}

__device__ __forceinline__ bool pad_at(const TgtParams& p, int b, int y, int x, double dx1, double dy1,
                                       double dx2, double dy2) {
  if (!p.paste) return false;
  int xs = (p.flips && p.flips[b]) ? (p.vsx - 1 - x) : x;   // fliplr of the mask (wider_face.py:165)
  double cx = (double)(p.ofx + xs * p.stx), cy = (double)(p.ofy + y * p.sty);
  const int32_t* pb = p.paste + 4 * b;
  return (cx + dx1 < (double)(pb[0] + 1)) | (cy + dy1 < (double)(pb[1] + 1)) |
         (cx + dx2 > (double)pb[2]) | (cy + dy2 > (double)pb[3]);      // processor.py:143-148
}

// the operands of the compensation stage: everything the three phases take, plus the per-anchor owner / best value they leave behind
struct TgtCompParams : TgtParams {
  int32_t* own; double* best; int32_t* count; int32_t* match_count;
  int nslots, N; double T;
};
template <class P> struct is_comp { static constexpr bool value = false; };
template <> struct is_comp<TgtCompParams> { static constexpr bool value = true; };

template <int PHASE, class P = TgtParams>
__global__ void __launch_bounds__(256) targets_kernel(P p) {
  constexpr bool COMP = is_comp<P>::value;
  if constexpr (COMP) {
    if (p.box_off[gridDim.y] > p.nslots) return;         // more boxes than the workspace has slots for: touch nothing
  }
  const int b = blockIdx.y;
  const int cells = p.vsy * p.vsx;
  const int idx = blockIdx.x * 256 + threadIdx.x;        // (t, y, x), x fastest
  const bool active = idx < p.nt * cells;
  const int t = active ? idx / cells : 0;
  const int cell = active ? idx - t * cells : 0;
  const int y = cell / p.vsx, x = cell - y * p.vsx;
  const int flat = cell * p.nt + t;                      // C-order over (y, x, t): reference index
  const int g0 = p.box_off[b], G = p.box_off[b + 1] - g0;
  const double* tp = p.tpl + (size_t)t * p.tstride;
  const double dx1 = tp[0], dy1 = tp[1], dx2 = tp[2], dy2 = tp[3];
  const Anchor an = anchor_at(dx1, dy1, dx2, dy2, p.ofy, p.ofx, p.sty, p.stx, y, x);
  const double fw = an.fw, fh = an.fh;

  double best = -1.0; int bestg = 0;
  for (int g = 0; g < G; ++g) {
    const double* bx = p.boxes + 4 * (size_t)(g0 + g);
    const double gx1 = bx[0], gy1 = bx[1], gx2 = bx[2], gy2 = bx[3];
    double v = -1.0;
    if (active) {
      double r = iou14(an.x1, an.y1, an.x2, an.y2, an.farea, gx1, gy1, gx2, gy2);
      v = r + 1e-6 * noise_at(p, b, flat, g, G);                      // processor.py:195
      if (v > best) { best = v; bestg = g; }                          // first arg-max (:197)
    }
    const bool hot = v > p.neg_thresh;                                 // only these can win (:255)
    if (__ballot(hot)) {
      unsigned long long bits = hot ? (unsigned long long)__double_as_longlong(v) : 0ull;
      if (PHASE == 0) {
        unsigned long long m = bits;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          unsigned long long other = __shfl_xor(m, o, 64);
          m = other > m ? other : m;
        }
        if (tf::lane_id() == 0) atomicMax(&p.gmax[g0 + g], m);
      } else {
        if (hot && bits == p.gmax[g0 + g]) atomicMin(&p.gidx[g0 + g], (unsigned int)flat);
      }
    }
  }
  if (PHASE != 0 || !active) return;

  float cls = -1.f, tx = 0.f, ty = 0.f, tw = 0.f, th = 0.f;
  if (G > 0) {
    const double* bx = p.boxes + 4 * (size_t)(g0 + bestg);
    const double gx1 = bx[0], gy1 = bx[1], gx2 = bx[2], gy2 = bx[3];
    const double fcx = (gx1 + gx2) / 2.0, fcy = (gy1 + gy2) / 2.0;     // processor.py:181-182
    const double coarse_x = (double)(p.ofx + x * p.stx), coarse_y = (double)(p.ofy + y * p.sty);
    tx = (float)((fcx - coarse_x) / fw);                               // :184-185
    ty = (float)((fcy - coarse_y) / fh);
    tw = (float)log((gx2 - gx1 + 1.0) / fw);                           // :187-191
    th = (float)log((gy2 - gy1 + 1.0) / fh);
    if (best >= p.pos_thresh) cls = 1.f;                               // :260-261
    else if (p.neg_thresh <= best && best < p.pos_thresh) cls = 0.f;   // :264-269
  }
  if (cls != -1.f && pad_at(p, b, y, x, dx1, dy1, dx2, dy2)) { cls = 0.f; tx = 0.f; }   // :272-274 (tx only: D5)
  const size_t plane = (size_t)cells;
  p.cls[((size_t)b * p.nt + t) * plane + cell] = cls;
  float* r = p.reg + ((size_t)b * 4 * p.nt + t) * plane + cell;
  r[0] = tx; r[(size_t)p.nt * plane] = ty; r[(size_t)2 * p.nt * plane] = tw; r[(size_t)3 * p.nt * plane] = th;
  if constexpr (COMP) {
    const size_t a = (size_t)b * p.nt * plane + idx;     // the class map's own index: (b, t, y, x)
    p.own[a] = bestg; p.best[a] = best;
  }
}

__global__ void targets_best_anchor_kernel(TgtParams p, int total) {
  int gi = blockIdx.x * blockDim.x + threadIdx.x;
  if (gi >= total) return;
  if (__longlong_as_double((long long)p.gmax[gi]) > p.neg_thresh) {     // :255
    const int b = image_of(p.box_off, gi);
    unsigned int flat = p.gidx[gi];
    int t = flat % p.nt, cell = flat / p.nt;
    int y = cell / p.vsx, x = cell - y * p.vsx;
    const double* tp = p.tpl + (size_t)t * p.tstride;
    if (!pad_at(p, b, y, x, tp[0], tp[1], tp[2], tp[3]))
      p.cls[((size_t)b * p.nt + t) * (size_t)(p.vsy * p.vsx) + cell] = 1.f;   // :257 then :272-273
  }
}

// ---- scale compensation (tinyfaces_hip.h: "the rule").  Every anchor has ONE owner, so a face's workgroup is the only writer of the
// anchors it promotes: no race between faces, and an image's result does not depend on the rest of the batch.

// D: count(g) = anchors labelled +1 whose owner is g.  Neighbouring anchors mostly share their owner: the wave adds once per distinct owner.
__global__ void __launch_bounds__(256) targets_count_kernel(TgtCompParams p) {
  if (p.box_off[gridDim.y] > p.nslots) return;
  const int b = blockIdx.y;
  const int A = p.nt * p.vsy * p.vsx;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  int slot = -1;
  if (idx < A) {
    const size_t a = (size_t)b * A + idx;
    if (p.cls[a] == 1.f) slot = p.box_off[b] + p.own[a];
  }
  unsigned long long pending = __ballot(slot >= 0);
  while (pending) {                                        // wave-uniform
    const int leader = __ffsll((long long)pending) - 1;
    const int s = __shfl(slot, leader, 64);
    const unsigned long long same = __ballot(slot == s);
    if (tf::lane_id() == leader) atomicAdd(&p.count[s], (int)__popcll(same));
    pending &= ~same;
  }
}

// order of the candidates: larger best first, then the lower reference flat index.  best >= T > 0, so the bit pattern of the double orders
// like the value and 0 is free to mean "none".
__device__ __forceinline__ bool cand_before(unsigned long long ka, unsigned int fa, unsigned long long kb, unsigned int fb) {
  return ka > kb || (ka == kb && fa < fb);
}

// E: one workgroup per face.  Up to N - count rounds; each is a block arg-max over the candidates strictly behind the previous winner, so
// no candidate list is stored.  Only the cells at which a template can reach IoU T with the face are walked (a superset: eligibility is exact).
__global__ void __launch_bounds__(256) targets_select_kernel(TgtCompParams p, int B) {
  __shared__ unsigned long long s_k[4];
  __shared__ unsigned int s_f[4];
  const int gi = blockIdx.x;
  const int total = p.box_off[B];
  if (total > p.nslots || gi >= total) return;
  const int cnt = p.count[gi];
  const int need = p.N - cnt;
  if (need <= 0) {                                         // the common case of medium and large faces
    if (threadIdx.x == 0 && p.match_count) p.match_count[gi] = cnt;
    return;
  }
  const int b = image_of(p.box_off, gi);
  const int g = gi - p.box_off[b];
  const double* bx = p.boxes + 4 * (size_t)gi;
  const double gx1 = bx[0], gy1 = bx[1], gx2 = bx[2], gy2 = bx[3];
  const int cells = p.vsy * p.vsx;
  const size_t img = (size_t)b * p.nt * cells;
  const int wave = threadIdx.x >> 6;
  const double bw = gx2 - gx1 + 1.0, bh = gy2 - gy1 + 1.0, barea = bw * bh;
  const double Tm = p.T - 2e-6;                            // noise < 1e-6, rounding 5e-15

  unsigned long long prev_k = ~0ull;                       // before every candidate
  unsigned int prev_f = 0;
  int promoted = 0;
  while (promoted < need) {
    unsigned long long my_k = 0ull;
    unsigned int my_f = 0xffffffffu;
    for (int t = wave; t < p.nt; t += 4) {                  // a wave per template: the windows of the templates that matter are small
      const double* tp = p.tpl + (size_t)t * p.tstride;
      const double dx1 = tp[0], dy1 = tp[1], dx2 = tp[2], dy2 = tp[3];
      // A candidate has IoU >= Tm (best >= T, less the noise and the rounding).  The union is at least the larger of the two areas and the
      // intersection at most iw * min(heights), so: the smaller area is at least Tm times the larger (else the template has no candidate), and
      // iw >= Tm * larger / min(heights) = iwm, likewise ih >= ihm.  With c = of + i * st the template box [d1 + c, d2 + c] overlaps the
      // face by iw = min(d2 + c, g2) - max(d1 + c, g1) + 1 >= iwm only if d2 + c >= g1 - 1 + iwm and d1 + c <= g2 + 1 - iwm.
      const double fw = dx2 - dx1 + 1.0, fh = dy2 - dy1 + 1.0, farea = fw * fh;
      const double larger = fmax(farea, barea);
      if (!(fmin(farea, barea) >= Tm * larger)) continue;
      const double iwm = Tm * larger / fmin(fh, bh) * (1.0 - 1e-9), ihm = Tm * larger / fmin(fw, bw) * (1.0 - 1e-9);
      const double xl = fmax(floor((gx1 - 1.0 + iwm - dx2 - (double)p.ofx) / (double)p.stx), 0.0);
      const double xh = fmin(ceil((gx2 + 1.0 - iwm - dx1 - (double)p.ofx) / (double)p.stx), (double)(p.vsx - 1));
      const double yl = fmax(floor((gy1 - 1.0 + ihm - dy2 - (double)p.ofy) / (double)p.sty), 0.0);
      const double yh = fmin(ceil((gy2 + 1.0 - ihm - dy1 - (double)p.ofy) / (double)p.sty), (double)(p.vsy - 1));
      if (!(xl <= xh) || !(yl <= yh)) continue;            // (a NaN coordinate walks nothing)
      const int x0 = (int)xl, y0 = (int)yl, ww = (int)xh - x0 + 1, wh = (int)yh - y0 + 1;
      for (int i = tf::lane_id(); i < ww * wh; i += 64) {
        const int wy = i / ww;
        const int y = y0 + wy, x = x0 + (i - wy * ww);
        const int cell = y * p.vsx + x;
        const size_t a = img + (size_t)t * cells + cell;
        if (p.own[a] != g) continue;
        const double bv = p.best[a];
        if (!(bv >= p.T) || p.cls[a] == 1.f || pad_at(p, b, y, x, dx1, dy1, dx2, dy2)) continue;
        const unsigned long long k = (unsigned long long)__double_as_longlong(bv);
        const unsigned int f = (unsigned int)(cell * p.nt + t);
        if (cand_before(prev_k, prev_f, k, f) && cand_before(k, f, my_k, my_f)) { my_k = k; my_f = f; }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long ok = __shfl_xor(my_k, o, 64);
      const unsigned int of = __shfl_xor(my_f, o, 64);
      if (cand_before(ok, of, my_k, my_f)) { my_k = ok; my_f = of; }
    }
    if (tf::lane_id() == 0) { s_k[wave] = my_k; s_f[wave] = my_f; }
    __syncthreads();
    unsigned long long win_k = s_k[0];
    unsigned int win_f = s_f[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (cand_before(s_k[w], s_f[w], win_k, win_f)) { win_k = s_k[w]; win_f = s_f[w]; }
    __syncthreads();                                       // s_k / s_f are rewritten by the next round
    if (win_k == 0ull) break;                              // fewer candidates than needed: all of them are promoted
    if (threadIdx.x == 0) {
      const int t = win_f % p.nt, cell = win_f / p.nt;
      p.cls[img + (size_t)t * cells + cell] = 1.f;
    }
    prev_k = win_k; prev_f = win_f;
    ++promoted;
  }
  if (threadIdx.x == 0 && p.match_count) p.match_count[gi] = cnt + promoted;
}

__global__ void iou_dump_kernel(const double* boxes, int G, const double* tpl, int nt, int tstride, int vsy, int vsx,
                                int ofy, int ofx, int sty, int stx, double* out) {
  int flat = blockIdx.x * blockDim.x + threadIdx.x;
  if (flat >= vsy * vsx * nt) return;
  int t = flat % nt, cell = flat / nt, y = cell / vsx, x = cell % vsx;
  const double* tp = tpl + (size_t)t * tstride;
  // anchor_at's geometry written out by hand: `out` may alias `tpl`, so the compiler re-reads the template row behind every store; anchor_at
  // takes the row by value, which hoists those loads and changes the code of this test hook.  tests/test_gpu_targets.py pins it against numpy.
  double cx = (double)ofx + (double)x * ((double)stx / 1.0), cy = (double)ofy + (double)y * ((double)sty / 1.0);
  double fh = tp[3] - tp[1] + 1.0, fw = tp[2] - tp[0] + 1.0;
  for (int g = 0; g < G; ++g)
    out[(size_t)flat * G + g] = iou14(tp[0] + cx, tp[1] + cy, tp[2] + cx, tp[3] + cy, fw * fh,
                                      boxes[4 * g], boxes[4 * g + 1], boxes[4 * g + 2], boxes[4 * g + 3]);
}

}  // namespace

extern "C" size_t tf_targets_workspace_bytes(int total_boxes) {
  size_t n = (size_t)(total_boxes > 0 ? total_boxes : 1);
  return n * 8 + n * 4 + 64;
}

extern "C" int tf_dense_overlap_targets(const double* boxes, const int32_t* box_offsets, int B,
                                        const double* templates, int nt, int tstride,
                                        int vsy, int vsx, int ofy, int ofx, int sty, int stx,
                                        const int32_t* paste_boxes, const int32_t* flips,
                                        const double* noise, const int64_t* noise_offsets, uint64_t seed,
                                        double pos_thresh, double neg_thresh,
                                        float* class_map, float* reg_map,
                                        void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  TgtParams p;
  if (int rc = base_params(p, boxes, box_offsets, B, templates, nt, tstride, vsy, vsx, ofy, ofx, sty, stx, paste_boxes, flips, noise, noise_offsets,
                           seed, pos_thresh, neg_thresh, class_map, reg_map)) return rc;
  // total boxes is only known on device; the caller sizes ws from its host copy.
  size_t nslots = (ws_bytes - 64) / 12;
  if (!ws || ws_bytes < 76) return TF_ERR_WORKSPACE;
  p.gmax = (unsigned long long*)ws;
  p.gidx = (unsigned int*)((char*)ws + nslots * 8);
  if (hipMemsetAsync(p.gmax, 0, nslots * 8, stream) != hipSuccess) return TF_ERR_LAUNCH;
  if (hipMemsetAsync(p.gidx, 0xff, nslots * 4, stream) != hipSuccess) return TF_ERR_LAUNCH;
  dim3 grid((nt * vsy * vsx + 255) / 256, B);
  hipLaunchKernelGGL(targets_kernel<0>, grid, dim3(256), 0, stream, p);
  hipLaunchKernelGGL(targets_kernel<1>, grid, dim3(256), 0, stream, p);
  int total = (int)nslots;
  // total real boxes <= nslots; surplus slots keep gmax == 0 and are skipped by the threshold test
  hipLaunchKernelGGL(targets_best_anchor_kernel, dim3((total + 127) / 128), dim3(128), 0, stream, p, total);
  TF_CHECK_LAUNCH();
  return TF_OK;
}

// workspace of the compensated call: per box slot gmax (8) + gidx (4) + count (4), per anchor best (8) + own (4)
extern "C" size_t tf_targets_comp_workspace_bytes(int total_boxes, int B, int nt, int vsy, int vsx) {
  size_t n = (size_t)(total_boxes > 0 ? total_boxes : 1);
  size_t anchors = (size_t)(B > 0 ? B : 0) * (size_t)(nt > 0 ? nt : 0) * (size_t)(vsy > 0 ? vsy : 0) * (size_t)(vsx > 0 ? vsx : 0);
  return n * 16 + anchors * 12 + 64;
}

extern "C" int tf_dense_overlap_targets_comp(const double* boxes, const int32_t* box_offsets, int B,
                                             const double* templates, int nt, int tstride,
                                             int vsy, int vsx, int ofy, int ofx, int sty, int stx,
                                             const int32_t* paste_boxes, const int32_t* flips,
                                             const double* noise, const int64_t* noise_offsets, uint64_t seed,
                                             double pos_thresh, double neg_thresh,
                                             int N, double T, int32_t* match_count,
                                             float* class_map, float* reg_map,
                                             void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  TgtCompParams p;
  if (int rc = base_params(p, boxes, box_offsets, B, templates, nt, tstride, vsy, vsx, ofy, ofx, sty, stx, paste_boxes, flips, noise, noise_offsets,
                           seed, pos_thresh, neg_thresh, class_map, reg_map)) return rc;
  if (sty <= 0 || stx <= 0) return TF_ERR_ARG;                       // the window of phase E divides by the stride
  if (N < 1 || N > 64) return TF_ERR_ARG;
  if (!(T >= 0.01) || !(T < pos_thresh) || !(T - T == 0.0)) return TF_ERR_ARG;       // (T - T: NaN for an infinite T)
  const size_t anchors = (size_t)B * nt * vsy * vsx;
  if ((size_t)nt * vsy * vsx > (size_t)0x7fffffff) return TF_ERR_UNSUPPORTED;
  // total boxes is only known on device; the caller sizes ws from its host copy, and every kernel leaves at once if the device's total
  // exceeds the slots the workspace holds
  if (!ws || ws_bytes < tf_targets_comp_workspace_bytes(1, B, nt, vsy, vsx)) return TF_ERR_WORKSPACE;
  size_t nslots = (ws_bytes - 64 - anchors * 12) / 16;
  if (nslots > ((size_t)1 << 30)) nslots = (size_t)1 << 30;
  char* w = (char*)ws;
  p.gmax = (unsigned long long*)w;                 w += nslots * 8;
  p.best = (double*)w;                             w += anchors * 8;
  p.gidx = (unsigned int*)w;                       w += nslots * 4;
  p.count = (int32_t*)w;                           w += nslots * 4;
  p.own = (int32_t*)w;
  p.match_count = match_count; p.nslots = (int)nslots; p.N = N; p.T = T;
  if (hipMemsetAsync(p.gmax, 0, nslots * 8, stream) != hipSuccess) return TF_ERR_LAUNCH;
  if (hipMemsetAsync(p.gidx, 0xff, nslots * 4, stream) != hipSuccess) return TF_ERR_LAUNCH;
  if (hipMemsetAsync(p.count, 0, nslots * 4, stream) != hipSuccess) return TF_ERR_LAUNCH;
  dim3 grid((nt * vsy * vsx + 255) / 256, B);
  hipLaunchKernelGGL((targets_kernel<0, TgtCompParams>), grid, dim3(256), 0, stream, p);
  hipLaunchKernelGGL((targets_kernel<1, TgtCompParams>), grid, dim3(256), 0, stream, p);
  const TgtParams& base = p;
  hipLaunchKernelGGL(targets_best_anchor_kernel, dim3(((int)nslots + 127) / 128), dim3(128), 0, stream, base, (int)nslots);
  hipLaunchKernelGGL(targets_count_kernel, grid, dim3(256), 0, stream, p);
  hipLaunchKernelGGL(targets_select_kernel, dim3((unsigned)nslots), dim3(256), 0, stream, p, B);
  TF_CHECK_LAUNCH();
  return TF_OK;
}

extern "C" int tf_dense_overlap_iou(const double* boxes, int G, const double* templates, int nt, int tstride,
                                    int vsy, int vsx, int ofy, int ofx, int sty, int stx,
                                    double* iou_out, void* stream_) {
  if (G <= 0) return TF_OK;
  int n = vsy * vsx * nt;
  hipLaunchKernelGGL(iou_dump_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream_, boxes, G, templates, nt,
                     tstride, vsy, vsx, ofy, ofx, sty, stx, iou_out);
  TF_CHECK_LAUNCH();
  return TF_OK;
}

// ---- template clustering: the n x n distance matrix 1 - IoU of the centred ground-truth shapes
// (tinyfaces/clustering/cluster.py:28-37 over tinyfaces/metrics.py:8-40: plain areas, no +1, IoU = 0 when the union is not
// positive).  float64, every operation rounded like numpy's (this file is compiled with -ffp-contract=off): bit-exact with the
// reference's double loop, which is what makes the k-medoids that follows index-exact.
namespace {
__global__ void __launch_bounds__(256) pairwise_dist_kernel(const double* __restrict__ boxes, int n, double* __restrict__ out) {
  __shared__ double4 col[256];
  const int j0 = blockIdx.x * 256, i0 = blockIdx.y * 16;
  const int j = j0 + threadIdx.x;
  if (j < n) col[threadIdx.x] = *reinterpret_cast<const double4*>(boxes + 4 * (size_t)j);
  __syncthreads();
  if (j >= n) return;
  const double4 b = col[threadIdx.x];
  const double area_b = (b.z - b.x) * (b.w - b.y);
  for (int i = i0; i < min(n, i0 + 16); ++i) {
    const double4 a = *reinterpret_cast<const double4*>(boxes + 4 * (size_t)i);       // wave-uniform: one scalar-path load
    const double area_a = (a.z - a.x) * (a.w - a.y);
    const double xa = fmax(a.x, b.x), ya = fmax(a.y, b.y), xb = fmin(a.z, b.z), yb = fmin(a.w, b.w);
    const double inter = (xb - xa) * (yb - ya);
    const double uni = area_a + area_b - inter;
    out[(size_t)i * n + j] = 1.0 - (uni <= 0.0 ? 0.0 : inter / uni);
  }
}
}  // namespace

extern "C" int tf_pairwise_iou_distance(const double* boxes, int n, double* out, void* stream) {
  if (n < 0 || (n > 0 && (!boxes || !out))) return TF_ERR_ARG;
  if (n == 0) return TF_OK;
  hipLaunchKernelGGL(pairwise_dist_kernel, dim3((n + 255) / 256, (n + 15) / 16), dim3(256), 0, (hipStream_t)stream, boxes, n, out);
  TF_CHECK_LAUNCH();
  return TF_OK;
}

