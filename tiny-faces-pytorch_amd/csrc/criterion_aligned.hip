// Task-aligned form of the detection criterion (tf_criterion_aligned_fwd_bwd; Feng et al. 2021, TOOD): the quality focal form with the target
// of a positive READ from align_map -- the normalised alignment tf_targets_tal_aligned stored, q = min(1, max(0, a)), a NaN giving 0 -- instead
// of formed from the positive's own box, and the regression term of every positive weighted by the same q; the definition is in
// include/tinyfaces_hip.h.  The classification arithmetic is the quality pass's (qfl_weight of criterion_shared.h, the stable softplus and
// sigmoid), the regression term box_term and the SmoothL1 lines of csrc/criterion.hip.  Three launches, as there:
//   A1  per block the +1 labels (one int) and the sum of their q (one fp64): TF_FOCAL_NORM_ALIGN needs an image's sum of q before any of its
//       gradient can be written
//   A2  the block adds its image's counts and, for TF_FOCAL_NORM_ALIGN, its image's q partials in a fixed order; then labels, logits, q, loss
//       terms and the gradient: every element of grad_out is written exactly once; one fp64 partial triple (cls, reg, q) per block
//   A3  one block: per image the partials in a fixed order, times the normaliser (not the q sums), then the images in index order
// No floating-point atomics, no grid barrier: the same bits on every run.
#include <cmath>

#include "common.h"
#include "criterion_shared.h"

namespace {

constexpr int NORM_NONE = 0, NORM_POS = 1, NORM_ALIGN = 2;         // TF_FOCAL_NORM_*

// FocalParams carries the pass as in the quality form: `gamma` holds beta, `alpha` is unused, `partial` is [B][nblk][3], `loss` has four doubles.
struct AlignedParams {
  FocalParams f;
  const float* align;     // [B][E]
  double* qpart;          // [B][nblk]: the sum of q over the block's positives
};

// NaN -> 0: fmaxf returns its other operand
__device__ __forceinline__ float aligned_q(float a) { return fminf(1.f, fmaxf(0.f, a)); }

// the sum of q over image b's positives, from the per-block sums in a fixed order: every thread of the (256-thread) block returns the total
__device__ __forceinline__ double aligned_image_qsum(const AlignedParams& p, int b, double* wq /*[4], shared*/) {
  double s = 0.0;
  for (int i = threadIdx.x; i < p.f.nblk; i += 256) s += p.qpart[(size_t)b * p.f.nblk + i];
  s = tf::wave_sum(s);
  if ((threadIdx.x & 63) == 0) wq[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((wq[0] + wq[1]) + wq[2]) + wq[3];
}

// the factor of image b's sums and gradient
__device__ __forceinline__ double aligned_norm(int normalize, int npos, double qsum) {
  if (normalize == NORM_POS) return 1.0 / (double)(npos > 1 ? npos : 1);
  if (normalize == NORM_ALIGN) return 1.0 / (qsum > 1.0 ? qsum : 1.0);
  return 1.0;
}

__global__ void __launch_bounds__(256) aligned_count_kernel(AlignedParams p) {
  const int b = blockIdx.y, blk = blockIdx.x;
  __shared__ int wn[4];
  __shared__ double wq[4];
  int n = 0;
  double q = 0.0;
#pragma unroll
  for (int k = 0; k < EPB / 256; ++k) {
    const int e = blk * EPB + k * 256 + threadIdx.x;
    const bool isp = e < p.f.E && p.f.cls[(size_t)b * p.f.E + e] == 1.f;
    n += __popcll(__ballot(isp));
    if (isp) q += (double)aligned_q(p.align[(size_t)b * p.f.E + e]);
  }
  q = tf::wave_sum(q);
  if ((threadIdx.x & 63) == 0) { wn[threadIdx.x >> 6] = n; wq[threadIdx.x >> 6] = q; }
  __syncthreads();
  if (threadIdx.x == 0) {
    p.f.blkpos[(size_t)b * p.f.nblk + blk] = wn[0] + wn[1] + wn[2] + wn[3];
    p.qpart[(size_t)b * p.f.nblk + blk] = ((wq[0] + wq[1]) + wq[2]) + wq[3];
  }
}

template <int REG>
__global__ void __launch_bounds__(256) aligned_apply_kernel(AlignedParams pa) {
  const FocalParams& p = pa.f;
  const int b = blockIdx.y, blk = blockIdx.x;
  __shared__ int wn[4];
  __shared__ double wq[4];
  __shared__ double wloss[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int npos = focal_image_npos(p, b, wn);
  const double qsum = p.normalize == NORM_ALIGN ? aligned_image_qsum(pa, b, wq) : 0.0;      // kernel-uniform
  // the gradient's factor in fp32: for TF_FOCAL_NORM_POS the quality pass's own division, for TF_FOCAL_NORM_ALIGN the fp64 factor rounded once
  const float inv = p.normalize == NORM_POS ? 1.f / (float)(npos > 1 ? npos : 1) : (float)aligned_norm(p.normalize, npos, qsum);
  const float beta = p.gamma;
  double lcls = 0.0, lreg = 0.0, lq = 0.0;
#pragma unroll
  for (int k = 0; k < EPB / 256; ++k) {
    const int e = blk * EPB + k * 256 + threadIdx.x;
    if (e < p.E) {
      const float y = p.cls[(size_t)b * p.E + e];
      const bool isp = y == 1.f, isn = y == -1.f;
      const size_t oi = (size_t)b * 5 * p.E + e;
      float q = 0.f, gr[4] = {0.f, 0.f, 0.f, 0.f};
      if (isp) {
        q = aligned_q(pa.align[(size_t)b * p.E + e]);
        lq += (double)q;
        float v[4], t[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          v[c] = p.out[oi + (size_t)(c + 1) * p.E];
          t[c] = p.reg[(size_t)b * 4 * p.E + (size_t)c * p.E + e];
        }
        const float sc = q * (p.reg_weight * inv);
        float term = 0.f;
        if constexpr (REG == REG_SMOOTH_L1) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float d = v[c] - t[c];
            const float ad = fabsf(d);
            term += ad < 1.f ? 0.5f * d * d : ad - 0.5f;            // SmoothL1, beta = 1
            gr[c] = sc * (d < -1.f ? -1.f : (d > 1.f ? 1.f : d));
          }
        } else {                                                    // ONE overlap term per positive, its four derivatives in registers
          float a = 1.f;
          if (REG == REG_DIOU) { const float* wh = p.twh + 2 * (e / p.HW); a = wh[0] / wh[1]; }
          term = box_term<REG>(v[0], v[1], v[2], v[3], t[0], t[1], t[2], t[3], a, gr);
#pragma unroll
          for (int c = 0; c < 4; ++c) gr[c] *= sc;
        }
        lreg += (double)(q * term);
      }
      float g = 0.f;
      if (isp || isn) {
        const float s = p.out[oi];
        const float ez = expf(-fabsf(s)), r = 1.f / (1.f + ez);      // stable softplus: max(v, 0) + log1p(exp(-|v|))
        const float sp = fmaxf(s, 0.f) + log1pf(ez);
        const float sg = s >= 0.f ? r : ez * r;                     // sigmoid(s); sigma (1 - sigma) = ez r r on either side
        const float d = sg - q, bce = sp - q * s;
        float w, dw;
        qfl_weight(d, beta, w, dw);
        lcls += (double)(w * bce);
        g = inv * (w * d + dw * (ez * r * r) * bce);
      }
      p.grad[oi] = g;
#pragma unroll
      for (int c = 0; c < 4; ++c) p.grad[oi + (size_t)(c + 1) * p.E] = gr[c];
    }
  }
  lcls = tf::wave_sum(lcls); lreg = tf::wave_sum(lreg); lq = tf::wave_sum(lq);
  if (lane == 0) { wloss[wave][0] = lcls; wloss[wave][1] = lreg; wloss[wave][2] = lq; }
  __syncthreads();
  if (threadIdx.x < 3)
    p.partial[((size_t)b * p.nblk + blk) * 3 + threadIdx.x] = wloss[0][threadIdx.x] + wloss[1][threadIdx.x] + wloss[2][threadIdx.x] + wloss[3][threadIdx.x];
}

// one block of 256 threads
__global__ void __launch_bounds__(256) aligned_finish_kernel(AlignedParams pa) {
  const FocalParams& p = pa.f;
  __shared__ int wn[4];
  __shared__ double wq[4];
  __shared__ double wloss[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double total[3] = {0.0, 0.0, 0.0};                               // thread 0's
  long long all_pos = 0;
  for (int b = 0; b < p.B; ++b) {
    const int npos = focal_image_npos(p, b, wn);
    const double qsum = p.normalize == NORM_ALIGN ? aligned_image_qsum(pa, b, wq) : 0.0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int i = threadIdx.x; i < p.nblk; i += 256) {
      const double* q = p.partial + ((size_t)b * p.nblk + i) * 3;
      a0 += q[0]; a1 += q[1]; a2 += q[2];
    }
    a0 = tf::wave_sum(a0); a1 = tf::wave_sum(a1); a2 = tf::wave_sum(a2);
    if (lane == 0) { wloss[wave][0] = a0; wloss[wave][1] = a1; wloss[wave][2] = a2; }
    __syncthreads();
    if (threadIdx.x == 0) {
      const double norm = aligned_norm(p.normalize, npos, qsum);
      total[0] += (wloss[0][0] + wloss[1][0] + wloss[2][0] + wloss[3][0]) * norm;
      total[1] += (wloss[0][1] + wloss[1][1] + wloss[2][1] + wloss[3][1]) * norm;
      total[2] += wloss[0][2] + wloss[1][2] + wloss[2][2] + wloss[3][2];
      all_pos += npos;
      if (p.npos_out) p.npos_out[b] = npos;
    }
    __syncthreads();                                               // wn / wq / wloss are reused by the next image
  }
  if (threadIdx.x == 0) { p.loss[0] = total[0]; p.loss[1] = total[1]; p.loss[2] = total[2]; p.loss[3] = (double)all_pos; }
}

}  // namespace

// per block: the partial triple (3 doubles), the q sum (1 double), the count (1 int)
extern "C" size_t tf_criterion_aligned_workspace_bytes(int B, int nt, int H, int W) {
  if (B <= 0 || nt <= 0 || H <= 0 || W <= 0) return 0;
  const size_t E = (size_t)nt * H * W, nblk = (E + EPB - 1) / EPB;
  return a256((size_t)B * nblk * 3 * sizeof(double)) + a256((size_t)B * nblk * sizeof(double)) + a256((size_t)B * nblk * sizeof(int));
}

extern "C" int tf_criterion_aligned_fwd_bwd(const float* output, const float* class_map, const float* reg_map, const float* align_map,
                                            int B, int nt, int H, int W, float beta, int normalize, float reg_weight, int reg_form,
                                            const float* template_wh, float* grad_out, double* loss_out, int32_t* npos_out,
                                            void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!output || !class_map || !reg_map || !align_map || !grad_out || !loss_out || B <= 0 || nt <= 0 || H <= 0 || W <= 0) return TF_ERR_ARG;
  if (B > 65535 || (size_t)nt * H * W > ((size_t)1 << 30)) return TF_ERR_ARG;      // grid.y; element indices are ints
  if (!(beta >= 1.f) || !std::isfinite(beta) || !std::isfinite(reg_weight)) return TF_ERR_ARG;
  if (normalize != NORM_NONE && normalize != NORM_POS && normalize != NORM_ALIGN) return TF_ERR_ARG;
  if (reg_form < REG_SMOOTH_L1 || reg_form > REG_DIOU || (reg_form == REG_DIOU && !template_wh)) return TF_ERR_ARG;
  if (!ws || ws_bytes < tf_criterion_aligned_workspace_bytes(B, nt, H, W)) return TF_ERR_WORKSPACE;
  AlignedParams pa;
  FocalParams& p = pa.f;
  p.out = output; p.cls = class_map; p.reg = reg_map; p.B = B;
  p.E = nt * H * W; p.nblk = (p.E + EPB - 1) / EPB;
  p.gamma = beta; p.alpha = -1.f; p.normalize = normalize; p.reg_weight = reg_weight;
  p.grad = grad_out; p.loss = loss_out; p.npos_out = npos_out;
  p.twh = reg_form == REG_DIOU ? template_wh : nullptr; p.HW = H * W;
  pa.align = align_map;
  char* w = (char*)ws;
  p.partial = (double*)w;        w += a256((size_t)B * p.nblk * 3 * sizeof(double));
  pa.qpart = (double*)w;         w += a256((size_t)B * p.nblk * sizeof(double));
  p.blkpos = (int*)w;
  dim3 grid(p.nblk, B);
  hipLaunchKernelGGL(aligned_count_kernel, grid, dim3(256), 0, stream, pa);
  switch (reg_form) {
    case REG_IOU:  hipLaunchKernelGGL(aligned_apply_kernel<REG_IOU>, grid, dim3(256), 0, stream, pa); break;
    case REG_GIOU: hipLaunchKernelGGL(aligned_apply_kernel<REG_GIOU>, grid, dim3(256), 0, stream, pa); break;
    case REG_DIOU: hipLaunchKernelGGL(aligned_apply_kernel<REG_DIOU>, grid, dim3(256), 0, stream, pa); break;
    default:       hipLaunchKernelGGL(aligned_apply_kernel<REG_SMOOTH_L1>, grid, dim3(256), 0, stream, pa); break;
  }
  hipLaunchKernelGGL(aligned_finish_kernel, dim3(1), dim3(256), 0, stream, pa);
  TF_CHECK_LAUNCH();
  return TF_OK;
}
