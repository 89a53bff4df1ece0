// Fused AdamW step over a flat fp32 segment / a table of element ranges.
// Replaces torch.optim.AdamW.step (single-tensor path, amsgrad / maximize / capturable off) for one parameter group:
//   g = grad*gs ;  p *= 1 - lr*wd ;  m = lerp(m, g, 1 - b1) ;  v = b2*v + (1 - b2)*g*g ;  p -= (lr / bias1) * m / (sqrt(v) / sqrt(bias2) + eps)
// with bias1 = 1 - b1^step, bias2 = 1 - b2^step.  The step counter and the two corrections live in DEVICE memory (tf_adam_state):
//   adamw_advance_kernel                    one thread, once per optimizer step, behind tf_grad_clip_coef: a step the non-finite guard drops
//                                           does not advance the bias correction, and the host never has to know
//   adamw_kernel<CLIP, EMA> / adamw_segments_kernel<CLIP, EMA>   the update; CLIP and EMA as in sgd.hip (step_common.h)
// Every per-element line is one fp32 operation rounded to nearest, in the order of the header (include/tinyfaces_hip.h); this file is
// compiled with -ffp-contract=off (build.py: EXACT), so the only fused operations are the two written as __fmaf_rn.  sqrtf and `/` are the
// correctly rounded forms (no fast-math flags).
// HBM bound: 4 reads + 3 writes of 4 B per element (28 B; 36 B with the EMA), float4-vectorised, grid-stride.  No LDS, no atomics.
#include <math.h>

#include "common.h"
#include "step_common.h"

namespace {
// The per-element constants, each derived on the host in double and rounded once; ss and c2 are filled in by the kernel prologue from *st.
struct AdamK { float decay, w1, b2, w2, eps, gs, ss, c2; };

__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, const AdamK& k) {
  g = g * k.gs;
  p = p * k.decay;
  m = __fmaf_rn(k.w1, g - m, m);                 // torch.lerp(m, g, w1) for w1 < 0.5
  v = (k.b2 * v) + ((k.w2 * g) * g);
  const float d = (sqrtf(v) / k.c2) + k.eps;
  p = p - k.ss * (m / d);
}

// Uniform prologue: false when the step is skipped.  lr / bias1 and sqrt(bias2) in double from the device state, each rounded once.
template <bool CLIP>
__device__ __forceinline__ bool adam_prologue(AdamK& k, double lr, const tf_adam_state* __restrict__ st, const tf_clip_state* __restrict__ clip) {
  if constexpr (CLIP) {
    if (clip->skip) return false;
    k.gs = k.gs * clip->coef;
  }
  k.ss = (float)(lr / st->bias1);
  k.c2 = (float)sqrt(st->bias2);
  return true;
}

template <bool CLIP, bool EMA>
__global__ void __launch_bounds__(256) adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, int64_t n, double lr, AdamK k, int vec,
                                                    const tf_adam_state* __restrict__ st, const StepArgs<EMA> a) {
  if (!adam_prologue<CLIP>(k, lr, st, a.st)) return;
  const int64_t n4 = vec ? (n >> 2) : 0;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 pv = reinterpret_cast<float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<float4*>(m)[i];
    float4 vv = reinterpret_cast<float4*>(v)[i];
    adam_elem(pv.x, gv.x, mv.x, vv.x, k); adam_elem(pv.y, gv.y, mv.y, vv.y, k);
    adam_elem(pv.z, gv.z, mv.z, vv.z, k); adam_elem(pv.w, gv.w, mv.w, vv.w, k);
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
    reinterpret_cast<float4*>(p)[i] = pv;
    if constexpr (EMA) {
      float4 ev = reinterpret_cast<float4*>(a.e)[i];
      ev.x = ema_of(ev.x, pv.x, a.w); ev.y = ema_of(ev.y, pv.y, a.w); ev.z = ema_of(ev.z, pv.z, a.w); ev.w = ema_of(ev.w, pv.w, a.w);
      reinterpret_cast<float4*>(a.e)[i] = ev;
    }
  }
  for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    float pn = p[i], mn = m[i], vn = v[i];
    adam_elem(pn, g[i], mn, vn, k);
    m[i] = mn; v[i] = vn; p[i] = pn;
    if constexpr (EMA) a.e[i] = ema_of(a.e[i], pn, a.w);
  }
}

// The same update over a table of element ranges (SgdSegs, step_common.h): the index space of sgd_segments_kernel.
template <bool CLIP, bool EMA>
__global__ void __launch_bounds__(256) adamw_segments_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                             float* __restrict__ v, const SgdSegs t, int nseg, double lr, AdamK k, int vec,
                                                             const tf_adam_state* __restrict__ st, const StepArgs<EMA> a) {
  if (!adam_prologue<CLIP>(k, lr, st, a.st)) return;
  const int64_t total = t.cum[nseg];
  const int64_t stride = (int64_t)gridDim.x * 256 * 4;
  for (int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; j < total; j += stride) {
    const int kk = seg_of(t, nseg, j);
    const int64_t i = t.start[kk] + (j - t.cum[kk]);
    if (vec) {                                   // 4-aligned table: the four elements lie in range kk
      float4 pv = *reinterpret_cast<float4*>(p + i);
      const float4 gv = *reinterpret_cast<const float4*>(g + i);
      float4 mv = *reinterpret_cast<float4*>(m + i);
      float4 vv = *reinterpret_cast<float4*>(v + i);
      adam_elem(pv.x, gv.x, mv.x, vv.x, k); adam_elem(pv.y, gv.y, mv.y, vv.y, k);
      adam_elem(pv.z, gv.z, mv.z, vv.z, k); adam_elem(pv.w, gv.w, mv.w, vv.w, k);
      *reinterpret_cast<float4*>(m + i) = mv;
      *reinterpret_cast<float4*>(v + i) = vv;
      *reinterpret_cast<float4*>(p + i) = pv;
      if constexpr (EMA) {
        float4 ev = *reinterpret_cast<float4*>(a.e + i);
        ev.x = ema_of(ev.x, pv.x, a.w); ev.y = ema_of(ev.y, pv.y, a.w); ev.z = ema_of(ev.z, pv.z, a.w); ev.w = ema_of(ev.w, pv.w, a.w);
        *reinterpret_cast<float4*>(a.e + i) = ev;
      }
    } else {
      for (int c = 0; c < 4 && j + c < total; ++c) {
        const int kc = seg_of(t, nseg, j + c);
        const int64_t ic = t.start[kc] + (j + c - t.cum[kc]);
        float pn = p[ic], mn = m[ic], vn = v[ic];
        adam_elem(pn, g[ic], mn, vn, k);
        m[ic] = mn; v[ic] = vn; p[ic] = pn;
        if constexpr (EMA) a.e[ic] = ema_of(a.e[ic], pn, a.w);
      }
    }
  }
}

// beta^t by square-and-multiply, least significant bit first, every product a double-double product built from plain double operations
// (Dekker's exact product on Veltkamp's split; no fma, and this file is compiled without contraction): the rule of the header, which a
// host can repeat operation for operation.  Plain double products would carry up to (t - 1) * 2^-53 of relative error through the
// squarings; this is right to about one ulp for every t.
struct DD { double hi, lo; };
__device__ __forceinline__ DD two_prod(double a, double b) {          // hi = fl(a * b), hi + lo = a * b exactly
  const double split = 134217729.0;                                   // 2^27 + 1
  const double p = a * b;
  const double ca = split * a, ah = ca - (ca - a), al = a - ah;
  const double cb = split * b, bh = cb - (cb - b), bl = b - bh;
  const double e = ((ah * bh - p) + ah * bl + al * bh) + al * bl;
  return DD{p, e};
}
__device__ __forceinline__ DD dd_mul(DD x, DD y) {
  const DD p = two_prod(x.hi, y.hi);
  const double e = p.lo + (x.hi * y.lo + x.lo * y.hi);
  const double s = p.hi + e;
  return DD{s, e - (s - p.hi)};
}
__device__ __forceinline__ double pow_int(double beta, int64_t t) {
  DD r{1.0, 0.0}, x{beta, 0.0};
  while (t) {
    if (t & 1) r = dd_mul(r, x);
    x = dd_mul(x, x);
    t >>= 1;
  }
  return r.hi;
}
// One thread.  The only writer of *st while it runs.
__global__ void adamw_advance_kernel(tf_adam_state* __restrict__ st, double beta1, double beta2, const tf_clip_state* __restrict__ clip) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (clip != nullptr && clip->skip) return;
  const int64_t t = st->step + 1;
  st->step = t;
  st->bias1 = 1.0 - pow_int(beta1, t);
  st->bias2 = 1.0 - pow_int(beta2, t);
}

bool hyper_ok(double lr, double beta1, double beta2, double eps, double weight_decay) {
  return beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0 && eps > 0.0 && lr == lr && weight_decay == weight_decay;
}
// Every constant once, in double, rounded once to float.
AdamK constants(double lr, double beta1, double beta2, double eps, double weight_decay, float grad_scale) {
  AdamK k;
  k.decay = (float)(1.0 - lr * weight_decay);
  k.w1 = (float)(1.0 - beta1);
  k.b2 = (float)beta2;
  k.w2 = (float)(1.0 - beta2);
  k.eps = (float)eps;
  k.gs = grad_scale;
  k.ss = 0.f;
  k.c2 = 1.f;
  return k;
}

template <typename... Args>
void launch_flat(bool clip, bool ema, unsigned blocks, hipStream_t s, const StepArgs<true>& ea, const StepArgs<false>& sa, Args... args) {
  if (ema && clip) hipLaunchKernelGGL((adamw_kernel<true, true>), dim3(blocks), dim3(256), 0, s, args..., ea);
  else if (ema) hipLaunchKernelGGL((adamw_kernel<false, true>), dim3(blocks), dim3(256), 0, s, args..., ea);
  else if (clip) hipLaunchKernelGGL((adamw_kernel<true, false>), dim3(blocks), dim3(256), 0, s, args..., sa);
  else hipLaunchKernelGGL((adamw_kernel<false, false>), dim3(blocks), dim3(256), 0, s, args..., sa);
}
template <typename... Args>
void launch_segments(bool clip, bool ema, unsigned blocks, hipStream_t s, const StepArgs<true>& ea, const StepArgs<false>& sa, Args... args) {
  if (ema && clip) hipLaunchKernelGGL((adamw_segments_kernel<true, true>), dim3(blocks), dim3(256), 0, s, args..., ea);
  else if (ema) hipLaunchKernelGGL((adamw_segments_kernel<false, true>), dim3(blocks), dim3(256), 0, s, args..., ea);
  else if (clip) hipLaunchKernelGGL((adamw_segments_kernel<true, false>), dim3(blocks), dim3(256), 0, s, args..., sa);
  else hipLaunchKernelGGL((adamw_segments_kernel<false, false>), dim3(blocks), dim3(256), 0, s, args..., sa);
}
}  // namespace

extern "C" int tf_adamw_advance(tf_adam_state* st, double beta1, double beta2, const tf_clip_state* clip, void* stream) {
  if (!st || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return TF_ERR_ARG;
  hipLaunchKernelGGL(adamw_advance_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, st, beta1, beta2, clip);
  TF_CHECK_LAUNCH();
  return TF_OK;
}

extern "C" int tf_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, double lr,
                             double beta1, double beta2, double eps, double weight_decay, float grad_scale, float ema_weight,
                             const tf_adam_state* st, const tf_clip_state* clip, void* stream) {
  if (n < 0 || !hyper_ok(lr, beta1, beta2, eps, weight_decay)) return TF_ERR_ARG;
  if (n > 0 && (!param || !grad || !exp_avg || !exp_avg_sq || !st)) return TF_ERR_ARG;
  if (n == 0) return TF_OK;
  const int vec = (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)ema) & 15) == 0;
  int64_t blocks = ((vec ? (n >> 2) : n) + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  const StepArgs<true> ea{clip, ema, ema_weight};
  const StepArgs<false> sa{clip};
  launch_flat(clip != nullptr, ema != nullptr, (unsigned)blocks, (hipStream_t)stream, ea, sa, param, grad, exp_avg, exp_avg_sq, n, lr,
              constants(lr, beta1, beta2, eps, weight_decay, grad_scale), vec, st);
  TF_CHECK_LAUNCH();
  return TF_OK;
}

extern "C" int tf_adamw_step_segments(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema,
                                      const int64_t* host_segments, int nseg, double lr, double beta1, double beta2, double eps,
                                      double weight_decay, float grad_scale, float ema_weight, const tf_adam_state* st,
                                      const tf_clip_state* clip, void* stream) {
  if (nseg < 0 || !hyper_ok(lr, beta1, beta2, eps, weight_decay)) return TF_ERR_ARG;
  if (nseg > 0 && (!param || !grad || !exp_avg || !exp_avg_sq || !st || !host_segments)) return TF_ERR_ARG;
  if (nseg == 0) return TF_OK;
  if (!table_ok(host_segments, nseg)) return TF_ERR_ARG;
  const bool aligned = (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)ema) & 15) == 0;
  const StepArgs<true> ea{clip, ema, ema_weight};
  const StepArgs<false> sa{clip};
  const AdamK k = constants(lr, beta1, beta2, eps, weight_decay, grad_scale);
  for (int k0 = 0; k0 < nseg; k0 += TF_SGD_MAX_SEGMENTS) {
    SgdSegs t;
    int vec = aligned ? 1 : 0;
    int64_t blocks = 0;
    const int used = fill_table(host_segments, nseg, k0, &t, &vec, &blocks);
    if (used == 0) continue;
    launch_segments(clip != nullptr, ema != nullptr, (unsigned)blocks, (hipStream_t)stream, ea, sa, param, grad, exp_avg, exp_avg_sq, t, used,
                    lr, k, vec, st);
  }
  TF_CHECK_LAUNCH();
  return TF_OK;
}
