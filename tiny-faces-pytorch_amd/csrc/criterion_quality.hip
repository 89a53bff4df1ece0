// Quality focal form of the detection criterion (tf_criterion_quality_fwd_bwd; Li et al. 2020, Generalized Focal Loss): the class logit of a
// positive is trained towards q = min(1, IoU) of its OWN predicted box with its target, that of a negative towards 0; the definition is in
// include/tinyfaces_hip.h.  With sigma = sigmoid(s), d = sigma - q, BCE = softplus(s) - q s:
//   QFL     = |d|^beta BCE
//   dQFL/ds = |d|^beta d + beta |d|^(beta - 1) sgn(d) sigma (1 - sigma) BCE
// q is a constant of the classification term: nothing flows from it into the four regression channels, whose term and gradient are those of
// the focal pass's regression form (box_term and the SmoothL1 lines of csrc/criterion.hip).  The same three launches as the focal pass:
//   Q1  focal_count_kernel (criterion_shared.h): +1 labels of every block, one int per block
//   Q2  the block adds its image's counts, then labels, logits, q, loss terms and the gradient: every element of grad_out is written exactly
//       once; a positive lane loads its four predictions and four targets ONCE, for q and for the regression term; one fp64 partial
//       triple (cls, reg, q) per block
//   Q3  one block: per image the partials in a fixed order, times the normaliser (not the q sums), then the images in index order
// No floating-point atomics, no grid barrier: the same bits on every run.
#include <cmath>

#include "common.h"
#include "criterion_shared.h"

namespace {

// FocalParams carries the pass: `gamma` holds beta, `alpha` is unused, `partial` is [B][nblk][3], `loss` has four doubles.

// IoU of the overlap-loss section of the header, the operations box_term takes to its `iou` (the compiler shares them where both are called).
__device__ __forceinline__ float box_iou(float px, float py, float pw, float ph, float tx, float ty, float tw, float th) {
  const float hwp = 0.5f * expf(fminf(fmaxf(pw, -BOX_CLIP), BOX_CLIP)), hhp = 0.5f * expf(fminf(fmaxf(ph, -BOX_CLIP), BOX_CLIP));
  const float hwt = 0.5f * expf(tw), hht = 0.5f * expf(th);
  const float dx = px - tx, dy = py - ty;
  const float iwr = fminf(2.f * fminf(hwp, hwt), hwp + hwt - fabsf(dx)), ihr = fminf(2.f * fminf(hhp, hht), hhp + hht - fabsf(dy));
  const float iw = fmaxf(iwr, 0.f), ih = fmaxf(ihr, 0.f);
  const float ap = 4.f * hwp * hhp, at = 4.f * hwt * hht;
  const float I = iw * ih, U = ap + at - I, rU = 1.f / U;
  return I * rU;
}

template <int REG>
__global__ void __launch_bounds__(256) quality_apply_kernel(FocalParams p) {
  const int b = blockIdx.y, blk = blockIdx.x;
  __shared__ int wn[4];
  __shared__ double wloss[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int npos = focal_image_npos(p, b, wn);
  const float inv = p.normalize ? 1.f / (float)(npos > 1 ? npos : 1) : 1.f;
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
      if (isp) {                                                    // the eight box operands, once: q and the regression term
        float v[4], t[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          v[c] = p.out[oi + (size_t)(c + 1) * p.E];
          t[c] = p.reg[(size_t)b * 4 * p.E + (size_t)c * p.E + e];
        }
        q = fminf(box_iou(v[0], v[1], v[2], v[3], t[0], t[1], t[2], t[3]), 1.f);
        lq += (double)q;
        const float sc = p.reg_weight * inv;
        if constexpr (REG == REG_SMOOTH_L1) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float d = v[c] - t[c];
            const float ad = fabsf(d);
            lreg += (double)(ad < 1.f ? 0.5f * d * d : ad - 0.5f);   // SmoothL1, beta = 1
            gr[c] = sc * (d < -1.f ? -1.f : (d > 1.f ? 1.f : d));
          }
        } else {                                                    // ONE overlap term per positive, its four derivatives in registers
          float a = 1.f;
          if (REG == REG_DIOU) { const float* wh = p.twh + 2 * (e / p.HW); a = wh[0] / wh[1]; }
          lreg += (double)box_term<REG>(v[0], v[1], v[2], v[3], t[0], t[1], t[2], t[3], a, gr);
#pragma unroll
          for (int c = 0; c < 4; ++c) gr[c] *= sc;
        }
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
__global__ void __launch_bounds__(256) quality_finish_kernel(FocalParams p) {
  __shared__ int wn[4];
  __shared__ double wloss[4][3];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double total[3] = {0.0, 0.0, 0.0};                               // thread 0's
  long long all_pos = 0;
  for (int b = 0; b < p.B; ++b) {
    const int npos = focal_image_npos(p, b, wn);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    for (int i = threadIdx.x; i < p.nblk; i += 256) {
      const double* q = p.partial + ((size_t)b * p.nblk + i) * 3;
      a0 += q[0]; a1 += q[1]; a2 += q[2];
    }
    a0 = tf::wave_sum(a0); a1 = tf::wave_sum(a1); a2 = tf::wave_sum(a2);
    if (lane == 0) { wloss[wave][0] = a0; wloss[wave][1] = a1; wloss[wave][2] = a2; }
    __syncthreads();
    if (threadIdx.x == 0) {
      const double norm = p.normalize ? 1.0 / (double)(npos > 1 ? npos : 1) : 1.0;
      total[0] += (wloss[0][0] + wloss[1][0] + wloss[2][0] + wloss[3][0]) * norm;
      total[1] += (wloss[0][1] + wloss[1][1] + wloss[2][1] + wloss[3][1]) * norm;
      total[2] += wloss[0][2] + wloss[1][2] + wloss[2][2] + wloss[3][2];
      all_pos += npos;
      if (p.npos_out) p.npos_out[b] = npos;
    }
    __syncthreads();                                               // wn / wloss are reused by the next image
  }
  if (threadIdx.x == 0) { p.loss[0] = total[0]; p.loss[1] = total[1]; p.loss[2] = total[2]; p.loss[3] = (double)all_pos; }
}

}  // namespace

extern "C" size_t tf_criterion_quality_workspace_bytes(int B, int nt, int H, int W) {
  if (B <= 0 || nt <= 0 || H <= 0 || W <= 0) return 0;
  const size_t E = (size_t)nt * H * W, nblk = (E + EPB - 1) / EPB;
  return a256((size_t)B * nblk * 3 * sizeof(double)) + a256((size_t)B * nblk * sizeof(int));
}

extern "C" int tf_criterion_quality_fwd_bwd(const float* output, const float* class_map, const float* reg_map, int B, int nt, int H, int W,
                                            float beta, int normalize, float reg_weight, int reg_form, const float* template_wh,
                                            float* grad_out, double* loss_out, int32_t* npos_out,
                                            void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!output || !class_map || !reg_map || !grad_out || !loss_out || B <= 0 || nt <= 0 || H <= 0 || W <= 0) return TF_ERR_ARG;
  if (B > 65535 || (size_t)nt * H * W > ((size_t)1 << 30)) return TF_ERR_ARG;      // grid.y; element indices are ints
  if (!(beta >= 1.f) || !std::isfinite(beta) || !std::isfinite(reg_weight)) return TF_ERR_ARG;
  if (normalize != 0 && normalize != 1) return TF_ERR_ARG;
  if (reg_form < REG_SMOOTH_L1 || reg_form > REG_DIOU || (reg_form == REG_DIOU && !template_wh)) return TF_ERR_ARG;
  if (!ws || ws_bytes < tf_criterion_quality_workspace_bytes(B, nt, H, W)) return TF_ERR_WORKSPACE;
  FocalParams p;
  p.out = output; p.cls = class_map; p.reg = reg_map; p.B = B;
  p.E = nt * H * W; p.nblk = (p.E + EPB - 1) / EPB;
  p.gamma = beta; p.alpha = -1.f; p.normalize = normalize; p.reg_weight = reg_weight;
  p.grad = grad_out; p.loss = loss_out; p.npos_out = npos_out;
  p.twh = reg_form == REG_DIOU ? template_wh : nullptr; p.HW = H * W;
  char* w = (char*)ws;
  p.partial = (double*)w;        w += a256((size_t)B * p.nblk * 3 * sizeof(double));
  p.blkpos = (int*)w;
  dim3 grid(p.nblk, B);
  hipLaunchKernelGGL(focal_count_kernel, grid, dim3(256), 0, stream, p);
  switch (reg_form) {
    case REG_IOU:  hipLaunchKernelGGL(quality_apply_kernel<REG_IOU>, grid, dim3(256), 0, stream, p); break;
    case REG_GIOU: hipLaunchKernelGGL(quality_apply_kernel<REG_GIOU>, grid, dim3(256), 0, stream, p); break;
    case REG_DIOU: hipLaunchKernelGGL(quality_apply_kernel<REG_DIOU>, grid, dim3(256), 0, stream, p); break;
    default:       hipLaunchKernelGGL(quality_apply_kernel<REG_SMOOTH_L1>, grid, dim3(256), 0, stream, p); break;
  }
  hipLaunchKernelGGL(quality_finish_kernel, dim3(1), dim3(256), 0, stream, p);
  TF_CHECK_LAUNCH();
  return TF_OK;
}
