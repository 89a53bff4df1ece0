// DetectionCriterion forward + backward on device: OHEM, balance sampling, masked
// SoftMargin / SmoothL1 sums and d(total)/d(output), no host round trip.
// Replaces tinyfaces/models/loss.py:47-93 and tinyfaces/models/utils.py:103-163.
//
// Elements of one image are walked in C-order over (template, y, x) -- the order np.where /
// ravel_multi_index give in balance_sampling (utils.py:115-117,127-129) -- so "rank of a
// positive/negative label" means the same thing here and in the reference.
//   K1  OHEM in place (loss.py:59-63) + per-block counts of +1 / -1 labels
//   K2  per image: exclusive scan of the block counts, totals, and (if no keep flags are
//       injected) a uniformly random keep-subset of size <= max via rejection sampling into
//       a bitmap (one wave, counter RNG)
//   K3  ordered rank of every label (ballot prefix), sampling decision, loss terms, gradient;
//       every element of grad_out is written exactly once (no memset needed)
// Below them: the focal-loss form of the same pass (tf_criterion_focal_fwd_bwd), kernels F1-F3, and its overlap regression forms
// (tf_criterion_focal_box_fwd_bwd: IoU / GIoU / DIoU instantiations of F2).
#include <cmath>

#include "common.h"
#include "criterion_shared.h"      // EPB, a256, FocalParams, box_term, focal_count_kernel: shared with criterion_quality.hip

namespace {

struct CritParams {
  const float* out; float* cls; const float* reg;
  int B, nt, H, W, E, nblk;
  float ohem; int max_pos, max_neg; float reg_weight;
  const uint8_t* pos_keep; const uint8_t* neg_keep; uint64_t seed;
  float* label_out; float* grad; double* loss; int* counts_out;
  int* blkcnt;            // [B][nblk][2] counts, then exclusive offsets in place
  int* totals;            // [B][2]
  unsigned int* bitmap;   // [B][2][words]
  int words;
};

__device__ __forceinline__ float soft_margin(float s, float y) { return log1pf(expf(-s * y)); }   // ATen soft_margin_loss

__global__ void __launch_bounds__(256) crit_ohem_count_kernel(CritParams p) {
  const int b = blockIdx.y, blk = blockIdx.x;
  __shared__ int wsum[4][2];
  int npos = 0, nneg = 0;
#pragma unroll
  for (int k = 0; k < EPB / 256; ++k) {
    const int e = blk * EPB + k * 256 + threadIdx.x;
    if (e < p.E) {
      const size_t ci = (size_t)b * p.E + e;
      float y = p.cls[ci];
      const float s = p.out[(size_t)b * 5 * p.E + e];     // channels [0, nt) are the class logits
      if (soft_margin(s, y) < p.ohem) { y = 0.f; p.cls[ci] = 0.f; }     // loss.py:60-62 (in place)
      npos += (y == 1.f); nneg += (y == -1.f);
    }
  }
  npos = (int)tf::wave_sum((float)npos); nneg = (int)tf::wave_sum((float)nneg);
  if ((threadIdx.x & 63) == 0) { wsum[threadIdx.x >> 6][0] = npos; wsum[threadIdx.x >> 6][1] = nneg; }
  __syncthreads();
  if (threadIdx.x < 2) {
    int* c = p.blkcnt + ((size_t)b * p.nblk + blk) * 2;
    c[threadIdx.x] = wsum[0][threadIdx.x] + wsum[1][threadIdx.x] + wsum[2][threadIdx.x] + wsum[3][threadIdx.x];
  }
}

// one block (64 threads = one wave) per image
__global__ void __launch_bounds__(64) crit_scan_sample_kernel(CritParams p) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int* c = p.blkcnt + (size_t)b * p.nblk * 2;
  int carry[2] = {0, 0};
  for (int i0 = 0; i0 < p.nblk; i0 += 64) {
    const int i = i0 + lane;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int v = i < p.nblk ? c[2 * i + k] : 0;
      int incl = v;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) { int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
      if (i < p.nblk) c[2 * i + k] = carry[k] + incl - v;
      carry[k] += __shfl(incl, 63, 64);
    }
  }
  if (lane == 0) {
    p.totals[2 * b] = carry[0]; p.totals[2 * b + 1] = carry[1];
    if (p.counts_out) { p.counts_out[2 * b] = carry[0]; p.counts_out[2 * b + 1] = carry[1]; }
  }
  // random keep-subsets (bitmaps are zeroed by the host-side memset before this kernel)
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint8_t* inj = k == 0 ? p.pos_keep : p.neg_keep;
    const int n = carry[k], want = k == 0 ? p.max_pos : p.max_neg;
    if (inj || n <= want) continue;
    unsigned int* bm = p.bitmap + ((size_t)b * 2 + k) * p.words;
    int have = 0;
    for (unsigned round = 0; have < want; ++round) {
      const int need = want - have;
      bool fresh = false;
      if (lane < need) {
        const uint64_t h = tf::hash4(p.seed, ((uint64_t)b << 1) | k, round, lane);
        const unsigned int r = (unsigned int)(((h >> 32) * (uint64_t)n) >> 32);     // uniform in [0, n)
        const unsigned int bit = 1u << (r & 31);
        fresh = !(atomicOr(&bm[r >> 5], bit) & bit);
      }
      have += __popcll(__ballot(fresh));
    }
  }
}

__global__ void __launch_bounds__(256) crit_apply_kernel(CritParams p) {
  const int b = blockIdx.y, blk = blockIdx.x;
  __shared__ int wcnt[4][2];
  __shared__ double wloss[4][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int* off = p.blkcnt + ((size_t)b * p.nblk + blk) * 2;
  int base_pos = off[0], base_neg = off[1];
  const int npos = p.totals[2 * b], nneg = p.totals[2 * b + 1];
  const bool all_pos = npos <= p.max_pos, all_neg = nneg <= p.max_neg;     // utils.py:119,131
  const unsigned int* bm_pos = p.bitmap + ((size_t)b * 2) * p.words;
  const unsigned int* bm_neg = bm_pos + p.words;
  double lcls = 0.0, lreg = 0.0;
  for (int k = 0; k < EPB / 256; ++k) {
    const int e = blk * EPB + k * 256 + threadIdx.x;
    const bool in = e < p.E;
    const size_t ci = (size_t)b * p.E + (in ? e : 0);
    float y = in ? p.cls[ci] : 0.f;
    const bool isp = y == 1.f, isn = y == -1.f;
    const unsigned long long bp = __ballot(isp), bn = __ballot(isn);
    if (lane == 0) { wcnt[wave][0] = __popcll(bp); wcnt[wave][1] = __popcll(bn); }
    __syncthreads();
    int before_p = 0, before_n = 0, all_p = 0, all_n = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      all_p += wcnt[w][0]; all_n += wcnt[w][1];
      if (w < wave) { before_p += wcnt[w][0]; before_n += wcnt[w][1]; }
    }
    const unsigned long long lower = (1ull << lane) - 1ull;
    if (isp && !all_pos) {
      const int r = base_pos + before_p + __popcll(bp & lower);
      const bool keep = p.pos_keep ? p.pos_keep[(size_t)b * p.E + r] != 0 : (bm_pos[r >> 5] >> (r & 31)) & 1u;
      if (!keep) y = 0.f;
    }
    if (isn && !all_neg) {
      const int r = base_neg + before_n + __popcll(bn & lower);
      const bool keep = p.neg_keep ? p.neg_keep[(size_t)b * p.E + r] != 0 : (bm_neg[r >> 5] >> (r & 31)) & 1u;
      if (!keep) y = 0.f;
    }
    base_pos += all_p; base_neg += all_n;
    if (in) {
      if (p.label_out) p.label_out[ci] = y;
      const size_t oi = (size_t)b * 5 * p.E + e;
      const float s = p.out[oi];
      float g = 0.f;
      if (y != 0.f) {                                           // loss.py:77-79
        const float z = expf(-s * y);
        lcls += (double)log1pf(z);
        g = -y * z / (1.f + z);                                 // ATen soft_margin_loss_backward
      }
      p.grad[oi] = g;
#pragma unroll
      for (int c = 1; c <= 4; ++c) {                            // tx | ty | tw | th blocks (loss.py:66-67,83)
        const size_t ri = oi + (size_t)c * p.E;
        float gr = 0.f;
        if (y > 0.f) {
          const float d = p.out[ri] - p.reg[(size_t)b * 4 * p.E + (size_t)(c - 1) * p.E + e];
          const float ad = fabsf(d);
          lreg += (double)(ad < 1.f ? 0.5f * d * d : ad - 0.5f);     // SmoothL1, beta = 1
          gr = p.reg_weight * (d < -1.f ? -1.f : (d > 1.f ? 1.f : d));
        }
        p.grad[ri] = gr;
      }
    }
    __syncthreads();
  }
  lcls = tf::wave_sum(lcls); lreg = tf::wave_sum(lreg);
  if (lane == 0) { wloss[wave][0] = lcls; wloss[wave][1] = lreg; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const double v = wloss[0][threadIdx.x] + wloss[1][threadIdx.x] + wloss[2][threadIdx.x] + wloss[3][threadIdx.x];
    if (v != 0.0) atomicAdd(&p.loss[threadIdx.x], v);
  }
}

}  // namespace

extern "C" size_t tf_criterion_workspace_bytes(int B, int nt, int H, int W) {
  const size_t E = (size_t)nt * H * W, nblk = (E + EPB - 1) / EPB, words = (E + 31) / 32;
  return a256(B * nblk * 2 * 4) + a256(B * 2 * 4) + a256(B * 2 * words * 4) + 256;
}

extern "C" int tf_criterion_fwd_bwd(const float* output, float* class_map, const float* reg_map,
                                    int B, int nt, int H, int W, float ohem_thresh, int max_pos, int max_neg,
                                    float reg_weight, const uint8_t* pos_keep, const uint8_t* neg_keep, uint64_t seed,
                                    float* label_out, float* grad_out, double* loss_out, int32_t* counts_out,
                                    void* ws, size_t ws_bytes, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!output || !class_map || !reg_map || !grad_out || !loss_out || B <= 0 || nt <= 0 || H <= 0 || W <= 0) return TF_ERR_ARG;
  if (!ws || ws_bytes < tf_criterion_workspace_bytes(B, nt, H, W)) return TF_ERR_WORKSPACE;
  CritParams p;
  p.out = output; p.cls = class_map; p.reg = reg_map; p.B = B; p.nt = nt; p.H = H; p.W = W;
  p.E = nt * H * W; p.nblk = (p.E + EPB - 1) / EPB;
  p.ohem = ohem_thresh; p.max_pos = max_pos; p.max_neg = max_neg; p.reg_weight = reg_weight;
  p.pos_keep = pos_keep; p.neg_keep = neg_keep; p.seed = seed;
  p.label_out = label_out; p.grad = grad_out; p.loss = loss_out; p.counts_out = counts_out;
  p.words = (p.E + 31) / 32;
  char* w = (char*)ws;
  p.blkcnt = (int*)w;            w += a256((size_t)B * p.nblk * 2 * 4);
  p.totals = (int*)w;            w += a256((size_t)B * 2 * 4);
  p.bitmap = (unsigned int*)w;
  if (hipMemsetAsync(p.bitmap, 0, (size_t)B * 2 * p.words * 4, stream) != hipSuccess) return TF_ERR_LAUNCH;
  if (hipMemsetAsync(loss_out, 0, 2 * sizeof(double), stream) != hipSuccess) return TF_ERR_LAUNCH;
  dim3 grid(p.nblk, B);
  hipLaunchKernelGGL(crit_ohem_count_kernel, grid, dim3(256), 0, stream, p);
  hipLaunchKernelGGL(crit_scan_sample_kernel, dim3(B), dim3(64), 0, stream, p);
  hipLaunchKernelGGL(crit_apply_kernel, grid, dim3(256), 0, stream, p);
  TF_CHECK_LAUNCH();
  return TF_OK;
}

// ---------------------------------------------------------------------------------------------------------------- focal loss
// Sigmoid focal loss (Lin et al. 2017; alpha as in torchvision's sigmoid_focal_loss) over EVERY labelled element + SmoothL1 over every
// positive: no mining, no sampling, class_map is only read.  With x = y s:
//   FL     = a_t exp(-gamma softplus(x)) softplus(-x)
//   dFL/ds = -y a_t exp(-gamma softplus(x)) (gamma sigmoid(x) softplus(-x) + sigmoid(-x))
// and, for normalize = 1, both sums and all five gradient channels of image b times 1 / max(1, npos_b); images are summed.
//   F1  +1 labels of every block (ballot + popcount), one int per block, no atomics
//   F2  the block adds its image's counts (the same order in every block), then labels, logits, loss terms and the gradient:
//       every element of grad_out is written exactly once; one fp64 partial pair per block
//   F3  one block: per image the partials in a fixed order, times the normaliser, then the images in index order
namespace {

template <int REG>
__global__ void __launch_bounds__(256) focal_apply_kernel(FocalParams p) {
  const int b = blockIdx.y, blk = blockIdx.x;
  __shared__ int wn[4];
  __shared__ double wloss[4][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int npos = focal_image_npos(p, b, wn);
  const float inv = p.normalize ? 1.f / (float)(npos > 1 ? npos : 1) : 1.f;
  double lcls = 0.0, lreg = 0.0;
#pragma unroll
  for (int k = 0; k < EPB / 256; ++k) {
    const int e = blk * EPB + k * 256 + threadIdx.x;
    if (e < p.E) {
      const float y = p.cls[(size_t)b * p.E + e];
      const bool isp = y == 1.f, isn = y == -1.f;
      const size_t oi = (size_t)b * 5 * p.E + e;
      float g = 0.f;
      if (isp || isn) {
        const float s = p.out[oi];
        const float x = isp ? s : -s;
        const float ez = expf(-fabsf(x)), t = log1pf(ez);          // stable softplus: max(v, 0) + log1p(exp(-|v|))
        const float sp_x = fmaxf(x, 0.f) + t, sp_mx = fmaxf(-x, 0.f) + t;
        const float r = 1.f / (1.f + ez);
        const float sg_x = x >= 0.f ? r : ez * r, sg_mx = x >= 0.f ? ez * r : r;
        const float at = p.alpha < 0.f ? 1.f : (isp ? p.alpha : 1.f - p.alpha);
        const float mod = at * expf(-p.gamma * sp_x);
        lcls += (double)(mod * sp_mx);
        g = (isp ? -inv : inv) * mod * (p.gamma * sg_x * sp_mx + sg_mx);
      }
      p.grad[oi] = g;
      if constexpr (REG == REG_SMOOTH_L1) {
#pragma unroll
        for (int c = 1; c <= 4; ++c) {                              // tx | ty | tw | th blocks
          const size_t ri = oi + (size_t)c * p.E;
          float gr = 0.f;
          if (isp) {
            const float d = p.out[ri] - p.reg[(size_t)b * 4 * p.E + (size_t)(c - 1) * p.E + e];
            const float ad = fabsf(d);
            lreg += (double)(ad < 1.f ? 0.5f * d * d : ad - 0.5f);   // SmoothL1, beta = 1
            gr = p.reg_weight * inv * (d < -1.f ? -1.f : (d > 1.f ? 1.f : d));
          }
          p.grad[ri] = gr;
        }
      } else {                                                      // ONE overlap term per positive, its four derivatives in registers
        float gr[4] = {0.f, 0.f, 0.f, 0.f};
        if (isp) {
          float q[4], t[4];
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            q[c] = p.out[oi + (size_t)(c + 1) * p.E];
            t[c] = p.reg[(size_t)b * 4 * p.E + (size_t)c * p.E + e];
          }
          float a = 1.f;
          if (REG == REG_DIOU) { const float* wh = p.twh + 2 * (e / p.HW); a = wh[0] / wh[1]; }
          lreg += (double)box_term<REG>(q[0], q[1], q[2], q[3], t[0], t[1], t[2], t[3], a, gr);
          const float sc = p.reg_weight * inv;
#pragma unroll
          for (int c = 0; c < 4; ++c) gr[c] *= sc;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) p.grad[oi + (size_t)(c + 1) * p.E] = gr[c];
      }
    }
  }
  lcls = tf::wave_sum(lcls); lreg = tf::wave_sum(lreg);
  if (lane == 0) { wloss[wave][0] = lcls; wloss[wave][1] = lreg; }
  __syncthreads();
  if (threadIdx.x < 2)
    p.partial[((size_t)b * p.nblk + blk) * 2 + threadIdx.x] = wloss[0][threadIdx.x] + wloss[1][threadIdx.x] + wloss[2][threadIdx.x] + wloss[3][threadIdx.x];
}

// one block of 256 threads
__global__ void __launch_bounds__(256) focal_finish_kernel(FocalParams p) {
  __shared__ int wn[4];
  __shared__ double wloss[4][2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double total[2] = {0.0, 0.0};                                    // thread 0's
  for (int b = 0; b < p.B; ++b) {
    const int npos = focal_image_npos(p, b, wn);
    double a0 = 0.0, a1 = 0.0;
    for (int i = threadIdx.x; i < p.nblk; i += 256) {
      const double* q = p.partial + ((size_t)b * p.nblk + i) * 2;
      a0 += q[0]; a1 += q[1];
    }
    a0 = tf::wave_sum(a0); a1 = tf::wave_sum(a1);
    if (lane == 0) { wloss[wave][0] = a0; wloss[wave][1] = a1; }
    __syncthreads();
    if (threadIdx.x == 0) {
      const double norm = p.normalize ? 1.0 / (double)(npos > 1 ? npos : 1) : 1.0;
      total[0] += (wloss[0][0] + wloss[1][0] + wloss[2][0] + wloss[3][0]) * norm;
      total[1] += (wloss[0][1] + wloss[1][1] + wloss[2][1] + wloss[3][1]) * norm;
      if (p.npos_out) p.npos_out[b] = npos;
    }
    __syncthreads();                                               // wn / wloss are reused by the next image
  }
  if (threadIdx.x == 0) { p.loss[0] = total[0]; p.loss[1] = total[1]; }
}

}  // namespace

extern "C" size_t tf_criterion_focal_workspace_bytes(int B, int nt, int H, int W) {
  if (B <= 0 || nt <= 0 || H <= 0 || W <= 0) return 0;
  const size_t E = (size_t)nt * H * W, nblk = (E + EPB - 1) / EPB;
  return a256((size_t)B * nblk * 2 * sizeof(double)) + a256((size_t)B * nblk * sizeof(int));
}

namespace {

// the three launches of the focal pass; the regression form selects the instantiation of the apply kernel
int focal_launch(const float* output, const float* class_map, const float* reg_map, int B, int nt, int H, int W,
                 float gamma, float alpha, int normalize, float reg_weight, int reg_form, const float* template_wh,
                 float* grad_out, double* loss_out, int32_t* npos_out, void* ws, size_t ws_bytes, hipStream_t stream) {
  if (!output || !class_map || !reg_map || !grad_out || !loss_out || B <= 0 || nt <= 0 || H <= 0 || W <= 0) return TF_ERR_ARG;
  if (B > 65535 || (size_t)nt * H * W > ((size_t)1 << 30)) return TF_ERR_ARG;      // grid.y; element indices are ints
  if (!(gamma >= 0.f) || !std::isfinite(gamma) || !std::isfinite(alpha) || alpha > 1.f) return TF_ERR_ARG;
  if (normalize != 0 && normalize != 1) return TF_ERR_ARG;
  if (reg_form < REG_SMOOTH_L1 || reg_form > REG_DIOU || (reg_form == REG_DIOU && !template_wh)) return TF_ERR_ARG;
  if (!ws || ws_bytes < tf_criterion_focal_workspace_bytes(B, nt, H, W)) return TF_ERR_WORKSPACE;
  FocalParams p;
  p.out = output; p.cls = class_map; p.reg = reg_map; p.B = B;
  p.E = nt * H * W; p.nblk = (p.E + EPB - 1) / EPB;
  p.gamma = gamma; p.alpha = alpha; p.normalize = normalize; p.reg_weight = reg_weight;
  p.grad = grad_out; p.loss = loss_out; p.npos_out = npos_out;
  p.twh = reg_form == REG_DIOU ? template_wh : nullptr; p.HW = H * W;
  char* w = (char*)ws;
  p.partial = (double*)w;        w += a256((size_t)B * p.nblk * 2 * sizeof(double));
  p.blkpos = (int*)w;
  dim3 grid(p.nblk, B);
  hipLaunchKernelGGL(focal_count_kernel, grid, dim3(256), 0, stream, p);
  switch (reg_form) {
    case REG_IOU:  hipLaunchKernelGGL(focal_apply_kernel<REG_IOU>, grid, dim3(256), 0, stream, p); break;
    case REG_GIOU: hipLaunchKernelGGL(focal_apply_kernel<REG_GIOU>, grid, dim3(256), 0, stream, p); break;
    case REG_DIOU: hipLaunchKernelGGL(focal_apply_kernel<REG_DIOU>, grid, dim3(256), 0, stream, p); break;
    default:       hipLaunchKernelGGL(focal_apply_kernel<REG_SMOOTH_L1>, grid, dim3(256), 0, stream, p); break;
  }
  hipLaunchKernelGGL(focal_finish_kernel, dim3(1), dim3(256), 0, stream, p);
  TF_CHECK_LAUNCH();
  return TF_OK;
}

}  // namespace

extern "C" int tf_criterion_focal_fwd_bwd(const float* output, const float* class_map, const float* reg_map, int B, int nt, int H, int W,
                                          float gamma, float alpha, int normalize, float reg_weight,
                                          float* grad_out, double* loss_out, int32_t* npos_out,
                                          void* ws, size_t ws_bytes, void* stream_) {
  return focal_launch(output, class_map, reg_map, B, nt, H, W, gamma, alpha, normalize, reg_weight, REG_SMOOTH_L1, nullptr,
                      grad_out, loss_out, npos_out, ws, ws_bytes, (hipStream_t)stream_);
}

extern "C" int tf_criterion_focal_box_fwd_bwd(const float* output, const float* class_map, const float* reg_map, int B, int nt, int H, int W,
                                              float gamma, float alpha, int normalize, float reg_weight,
                                              int reg_form, const float* template_wh,
                                              float* grad_out, double* loss_out, int32_t* npos_out,
                                              void* ws, size_t ws_bytes, void* stream_) {
  if (!std::isfinite(reg_weight)) return TF_ERR_ARG;
  return focal_launch(output, class_map, reg_map, B, nt, H, W, gamma, alpha, normalize, reg_weight, reg_form, template_wh,
                      grad_out, loss_out, npos_out, ws, ws_bytes, (hipStream_t)stream_);
}
