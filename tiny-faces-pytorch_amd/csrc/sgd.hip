// Fused SGD(momentum, weight decay) step over a flat fp32 segment.
// Replaces torch.optim.SGD.step as configured at main.py:67-70 (dampening 0, no nesterov):
//   d = grad*grad_scale + wd*p ;  buf = mu*buf + d  (buf starts at 0, so step 1 gives buf = d) ;  p -= lr*buf
// HBM bound: 3 reads + 2 writes of 4 B per element, float4-vectorised, grid-stride.
#include "common.h"

namespace {
__global__ void __launch_bounds__(256) sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                  int64_t n, float lr, float mu, float wd, float gs, int vec) {
  const int64_t n4 = vec ? (n >> 2) : 0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i];
    mv.x = mu * mv.x + (gv.x * gs + wd * pv.x); pv.x -= lr * mv.x;
    mv.y = mu * mv.y + (gv.y * gs + wd * pv.y); pv.y -= lr * mv.y;
    mv.z = mu * mv.z + (gv.z * gs + wd * pv.z); pv.z -= lr * mv.z;
    mv.w = mu * mv.w + (gv.w * gs + wd * pv.w); pv.w -= lr * mv.w;
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(p)[i] = pv;
  }
  for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float mv = mu * m[i] + (g[i] * gs + wd * p[i]);
    m[i] = mv;
    p[i] -= lr * mv;
  }
}

// The same update over a table of element ranges (frozen BatchNorm: the conv weights of the trunk group, whose BN vectors sit in between and
// must see neither weight decay nor momentum).  The ranges are laid end to end into one compact index space (cum[k] = elements in front of
// range k); a thread takes four consecutive compact elements, finds their range by bisection and moves them as one float4 when the table
// is 4-aligned (every conv weight of the trunk is), one by one otherwise.
struct SgdSegs { int64_t start[TF_SGD_MAX_SEGMENTS]; int64_t cum[TF_SGD_MAX_SEGMENTS + 1]; };
__device__ __forceinline__ int seg_of(const SgdSegs& t, int nseg, int64_t j) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (t.cum[mid] <= j) lo = mid; else hi = mid - 1; }
  return lo;
}
__global__ void __launch_bounds__(256) sgd_segments_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           const SgdSegs t, int nseg, float lr, float mu, float wd, float gs, int vec) {
  const int64_t total = t.cum[nseg];
  const int64_t stride = (int64_t)gridDim.x * 256 * 4;
  for (int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; j < total; j += stride) {
    const int k = seg_of(t, nseg, j);
    const int64_t i = t.start[k] + (j - t.cum[k]);
    if (vec) {                                   // 4-aligned table: the four elements lie in range k
      float4 pv = *reinterpret_cast<float4*>(p + i);
      const float4 gv = *reinterpret_cast<const float4*>(g + i);
      float4 mv = *reinterpret_cast<float4*>(m + i);
      mv.x = mu * mv.x + (gv.x * gs + wd * pv.x); pv.x -= lr * mv.x;
      mv.y = mu * mv.y + (gv.y * gs + wd * pv.y); pv.y -= lr * mv.y;
      mv.z = mu * mv.z + (gv.z * gs + wd * pv.z); pv.z -= lr * mv.z;
      mv.w = mu * mv.w + (gv.w * gs + wd * pv.w); pv.w -= lr * mv.w;
      *reinterpret_cast<float4*>(m + i) = mv;
      *reinterpret_cast<float4*>(p + i) = pv;
    } else {
      for (int e = 0; e < 4 && j + e < total; ++e) {
        const int ke = seg_of(t, nseg, j + e);
        const int64_t ie = t.start[ke] + (j + e - t.cum[ke]);
        const float mv = mu * m[ie] + (g[ie] * gs + wd * p[ie]);
        m[ie] = mv;
        p[ie] -= lr * mv;
      }
    }
  }
}
}  // namespace

extern "C" int tf_sgd_step_segments(float* param, const float* grad, float* momentum_buf, const int64_t* host_segments, int nseg,
                                    float lr, float momentum, float weight_decay, float grad_scale, void* stream) {
  if (nseg < 0 || (nseg > 0 && (!param || !grad || !momentum_buf || !host_segments))) return TF_ERR_ARG;
  if (nseg == 0) return TF_OK;
  int64_t prev = 0;
  for (int k = 0; k < nseg; ++k) {
    const int64_t s = host_segments[2 * k], e = host_segments[2 * k + 1];
    if (s < prev || e < s) return TF_ERR_ARG;                  // ascending, disjoint
    prev = e;
  }
  const bool aligned = (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)momentum_buf) & 15) == 0;
  for (int k0 = 0; k0 < nseg; k0 += TF_SGD_MAX_SEGMENTS) {
    const int n = nseg - k0 < TF_SGD_MAX_SEGMENTS ? nseg - k0 : TF_SGD_MAX_SEGMENTS;
    SgdSegs t;
    int vec = aligned ? 1 : 0;
    int64_t cum = 0;
    int used = 0;
    for (int k = 0; k < n; ++k) {
      const int64_t s = host_segments[2 * (k0 + k)], e = host_segments[2 * (k0 + k) + 1];
      if (e == s) continue;
      if ((s & 3) || (e & 3)) vec = 0;
      t.start[used] = s; t.cum[used] = cum; cum += e - s; ++used;
    }
    if (used == 0) continue;
    t.cum[used] = cum;
    for (int k = used; k < TF_SGD_MAX_SEGMENTS; ++k) { t.start[k] = 0; t.cum[k + 1] = cum; }
    int64_t blocks = ((cum + 3) / 4 + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(sgd_segments_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad, momentum_buf, t, used, lr,
                       momentum, weight_decay, grad_scale, vec);
  }
  TF_CHECK_LAUNCH();
  return TF_OK;
}

extern "C" int tf_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n,
                           float lr, float momentum, float weight_decay, float grad_scale, void* stream) {
  if (n < 0 || (n > 0 && (!param || !grad || !momentum_buf))) return TF_ERR_ARG;
  if (n == 0) return TF_OK;
  const int vec = (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)momentum_buf) & 15) == 0;   // float4 path needs 16-byte alignment
  int64_t blocks = ((vec ? (n >> 2) : n) + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad, momentum_buf, n, lr,
                     momentum, weight_decay, grad_scale, vec);
  TF_CHECK_LAUNCH();
  return TF_OK;
}
