// Fused SGD(momentum, weight decay) step over a flat fp32 segment.
// Replaces torch.optim.SGD.step as configured at main.py:67-70 (dampening 0, no nesterov):
//   d = grad*grad_scale + wd*p ;  buf = mu*buf + d  (buf starts at 0, so step 1 gives buf = d) ;  p -= lr*buf
// HBM bound: 3 reads + 2 writes of 4 B per element, float4-vectorised, grid-stride.
//
// Gradient-norm clipping and the non-finite-step guard (the spot between loss.backward() and optimizer.step(), tinyfaces/trainer.py:86-87):
//   grad_sqnorm_kernel         sum of squares over a range table, fp64, one plain store per block (no atomics: bit-identical run to run)
//   grad_norm_finalize_kernel  one block: the partials in a fixed order -> tf_clip_state {sumsq, norm, coef, skip, skipped} in device memory
//   sgd_kernel<true> / sgd_segments_kernel<true>   the update with grad_scale * coef, nothing at all when skip is set
//   scale_segments_kernel      g *= coef for the autograd path (torch.optim.SGD applies the update)
// The norm pass reads 4 B per trained element and nothing else: HBM bound.
//
// Model EMA (torch.optim.swa_utils.AveragedModel.update_parameters behind optimizer.step(), tinyfaces/trainer.py:87):
//   sgd_kernel<CLIP, true> / sgd_segments_kernel<CLIP, true>   e = fmaf(w, p - e, e) on the parameter the update just left in registers:
//                              one more read and one more write of 4 B per element (28 B instead of 20 B)
//   ema_segments_kernel        the same average alone over a range table, for the autograd path (reads p and e, writes e)
//
// Gradient accumulation (several loss.backward() calls into one .grad before optimizer.step(), tinyfaces/trainer.py:85-87):
//   grad_accumulate_kernel<MODE>   over a range table: STORE acc = g (first micro-batch; acc is not read), ADD acc = acc + g, FINISH
//                              g = acc + g (last micro-batch: the sum lands in the buffer every later launch of the step reads).  Plain
//                              fp32 adds, left to right.  HBM bound: 8 B (STORE) / 12 B (ADD, FINISH) per trained element.
#include <math.h>

#include "common.h"
#include "step_common.h"      // StepArgs<EMA> (CLIP / EMA are explained there), ema_of, SgdSegs, seg_of, table_ok, fill_table

namespace {
template <bool CLIP, bool EMA>
__global__ void __launch_bounds__(256) sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                  int64_t n, float lr, float mu, float wd, float gs, int vec, const StepArgs<EMA> a) {
  if constexpr (CLIP) {
    if (a.st->skip) return;
    gs = gs * a.st->coef;
  }
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
    if constexpr (EMA) {
      float4 ev = reinterpret_cast<float4*>(a.e)[i];
      ev.x = ema_of(ev.x, pv.x, a.w); ev.y = ema_of(ev.y, pv.y, a.w); ev.z = ema_of(ev.z, pv.z, a.w); ev.w = ema_of(ev.w, pv.w, a.w);
      reinterpret_cast<float4*>(a.e)[i] = ev;
    }
  }
  for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const float mv = mu * m[i] + (g[i] * gs + wd * p[i]);
    m[i] = mv;
    if constexpr (EMA) {
      const float pn = p[i] - lr * mv;
      p[i] = pn;
      a.e[i] = ema_of(a.e[i], pn, a.w);
    } else {
      p[i] -= lr * mv;
    }
  }
}

// The same update over a table of element ranges (SgdSegs, step_common.h).
template <bool CLIP, bool EMA>
__global__ void __launch_bounds__(256) sgd_segments_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           const SgdSegs t, int nseg, float lr, float mu, float wd, float gs, int vec,
                                                           const StepArgs<EMA> a) {
  if constexpr (CLIP) {
    if (a.st->skip) return;
    gs = gs * a.st->coef;
  }
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
      if constexpr (EMA) {
        float4 ev = *reinterpret_cast<float4*>(a.e + i);
        ev.x = ema_of(ev.x, pv.x, a.w); ev.y = ema_of(ev.y, pv.y, a.w); ev.z = ema_of(ev.z, pv.z, a.w); ev.w = ema_of(ev.w, pv.w, a.w);
        *reinterpret_cast<float4*>(a.e + i) = ev;
      }
    } else {
      for (int e = 0; e < 4 && j + e < total; ++e) {
        const int ke = seg_of(t, nseg, j + e);
        const int64_t ie = t.start[ke] + (j + e - t.cum[ke]);
        const float mv = mu * m[ie] + (g[ie] * gs + wd * p[ie]);
        m[ie] = mv;
        if constexpr (EMA) {
          const float pn = p[ie] - lr * mv;
          p[ie] = pn;
          a.e[ie] = ema_of(a.e[ie], pn, a.w);
        } else {
          p[ie] -= lr * mv;
        }
      }
    }
  }
}
// e = fmaf(w, p - e, e) over a range table (the index space of scale_segments_kernel), behind an optimizer that is not ours: reads p and
// e, writes e, nothing outside the ranges.  st may be null; a state that says skip makes the launch a no-op.
__global__ void __launch_bounds__(256) ema_segments_kernel(float* __restrict__ e, const float* __restrict__ p, const SgdSegs t, int nseg,
                                                           float w, int vec, const tf_clip_state* __restrict__ st) {
  if (st != nullptr && st->skip) return;
  const int64_t total = t.cum[nseg];
  const int64_t stride = (int64_t)gridDim.x * 256 * 4;
  for (int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; j < total; j += stride) {
    const int k = seg_of(t, nseg, j);
    const int64_t i = t.start[k] + (j - t.cum[k]);
    if (vec) {
      const float4 pv = *reinterpret_cast<const float4*>(p + i);
      float4 ev = *reinterpret_cast<float4*>(e + i);
      ev.x = ema_of(ev.x, pv.x, w); ev.y = ema_of(ev.y, pv.y, w); ev.z = ema_of(ev.z, pv.z, w); ev.w = ema_of(ev.w, pv.w, w);
      *reinterpret_cast<float4*>(e + i) = ev;
    } else {
      for (int c = 0; c < 4 && j + c < total; ++c) {
        const int kc = seg_of(t, nseg, j + c);
        const int64_t ic = t.start[kc] + (j + c - t.cum[kc]);
        e[ic] = ema_of(e[ic], p[ic], w);
      }
    }
  }
}
// g *= coef over a range table (the index space of sgd_segments_kernel).  A skipped step stores zeros without reading: coef is 0 then, and
// NaN * 0 would stay NaN.
__global__ void __launch_bounds__(256) scale_segments_kernel(float* __restrict__ g, const SgdSegs t, int nseg, int vec,
                                                             const tf_clip_state* __restrict__ st) {
  const int skip = st->skip;
  const float coef = st->coef;
  const int64_t total = t.cum[nseg];
  const int64_t stride = (int64_t)gridDim.x * 256 * 4;
  for (int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; j < total; j += stride) {
    const int k = seg_of(t, nseg, j);
    const int64_t i = t.start[k] + (j - t.cum[k]);
    if (vec) {
      float4 gv = make_float4(0.f, 0.f, 0.f, 0.f);
      if (!skip) {
        gv = *reinterpret_cast<const float4*>(g + i);
        gv.x *= coef; gv.y *= coef; gv.z *= coef; gv.w *= coef;
      }
      *reinterpret_cast<float4*>(g + i) = gv;
    } else {
      for (int e = 0; e < 4 && j + e < total; ++e) {
        const int ke = seg_of(t, nseg, j + e);
        const int64_t ie = t.start[ke] + (j + e - t.cum[ke]);
        g[ie] = skip ? 0.f : g[ie] * coef;
      }
    }
  }
}
// Gradient accumulation over a range table (the index space of scale_segments_kernel).  MODE is one of TF_ACCUM_*: STORE writes acc without
// reading it (whatever an earlier window left there, a NaN included, is gone), ADD writes acc, FINISH writes g and leaves acc alone.  Every
// element is read and written by the same thread, so FINISH works in place; nothing outside the ranges is touched.
template <int MODE>
__global__ void __launch_bounds__(256) grad_accumulate_kernel(float* acc, float* g, const SgdSegs t, int nseg, int vec) {
  const int64_t total = t.cum[nseg];
  const int64_t stride = (int64_t)gridDim.x * 256 * 4;
  for (int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; j < total; j += stride) {
    const int k = seg_of(t, nseg, j);
    const int64_t i = t.start[k] + (j - t.cum[k]);
    if (vec) {
      float4 gv = *reinterpret_cast<const float4*>(g + i);
      if constexpr (MODE != TF_ACCUM_STORE) {
        const float4 av = *reinterpret_cast<const float4*>(acc + i);
        gv.x = av.x + gv.x; gv.y = av.y + gv.y; gv.z = av.z + gv.z; gv.w = av.w + gv.w;
      }
      *reinterpret_cast<float4*>((MODE == TF_ACCUM_FINISH ? g : acc) + i) = gv;
    } else {
      for (int e = 0; e < 4 && j + e < total; ++e) {
        const int ke = seg_of(t, nseg, j + e);
        const int64_t ie = t.start[ke] + (j + e - t.cum[ke]);
        if constexpr (MODE == TF_ACCUM_STORE) acc[ie] = g[ie];
        else if constexpr (MODE == TF_ACCUM_ADD) acc[ie] = acc[ie] + g[ie];
        else g[ie] = acc[ie] + g[ie];
      }
    }
  }
}

// Sum of squares over a range table: every element widened to fp64 (the square of an fp32 value is exact there), a private sum per
// thread over its grid-stride walk, then wave (xor butterfly) -> block (LDS, waves in order) -> ONE plain store per block.  Nothing
// outside the ranges is read; the order of every addition is a function of the launch geometry alone.
__global__ void __launch_bounds__(256) grad_sqnorm_kernel(const float* __restrict__ g, const SgdSegs t, int nseg, int vec,
                                                          double* __restrict__ partials) {
  __shared__ double wsum[4];
  const int64_t total = t.cum[nseg];
  const int64_t stride = (int64_t)gridDim.x * 256 * 4;
  double acc = 0.0;
  for (int64_t j = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4; j < total; j += stride) {
    const int k = seg_of(t, nseg, j);
    const int64_t i = t.start[k] + (j - t.cum[k]);
    if (vec) {
      const float4 gv = *reinterpret_cast<const float4*>(g + i);
      const double x = gv.x, y = gv.y, z = gv.z, w = gv.w;
      acc += (x * x + y * y) + (z * z + w * w);
    } else {
      for (int e = 0; e < 4 && j + e < total; ++e) {
        const int ke = seg_of(t, nseg, j + e);
        const double x = g[t.start[ke] + (j + e - t.cum[ke])];
        acc += x * x;
      }
    }
  }
  acc = tf::wave_sum(acc);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// One block: thread t adds partials t, t + 256, ... in index order, then the same wave -> LDS order as above; thread 0 writes the state.
// It is the only writer of *st while it runs, so `skipped` advances with a plain read-modify-write.
__global__ void __launch_bounds__(256) grad_norm_finalize_kernel(const double* __restrict__ partials, int count, float grad_scale,
                                                                 float max_norm, int flags, tf_clip_state* __restrict__ st) {
  __shared__ double wsum[4];
  double acc = 0.0;
  for (int i = threadIdx.x; i < count; i += 256) acc += partials[i];
  acc = tf::wave_sum(acc);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const double sumsq = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
  const double norm = fabs((double)grad_scale) * sqrt(sumsq);
  double coef = 1.0;
  if (max_norm > 0.f && !isinf(max_norm)) {
    const double c = (double)max_norm / (norm + 1e-6);
    coef = c > 1.0 ? 1.0 : c;                      // a NaN stays a NaN, as torch.clamp(max=1) leaves it
  }
  int skip = 0;
  if ((flags & TF_CLIP_SKIP_NONFINITE) && !isfinite(norm)) { skip = 1; coef = 0.0; }
  st->sumsq = sumsq;
  st->norm = norm;
  st->coef = (float)coef;
  st->skip = skip;
  if (skip) st->skipped = st->skipped + 1;
}

// `ema` null: the plain / clipped launches of before.  Otherwise the EMA instantiation, whose 16-byte path also needs `ema` aligned.
int sgd_segments(float* param, const float* grad, float* momentum_buf, float* ema, const int64_t* host_segments, int nseg, float lr,
                 float momentum, float weight_decay, float grad_scale, float ema_weight, const tf_clip_state* state, void* stream) {
  if (nseg < 0 || (nseg > 0 && (!param || !grad || !momentum_buf || !host_segments))) return TF_ERR_ARG;
  if (nseg == 0) return TF_OK;
  if (!table_ok(host_segments, nseg)) return TF_ERR_ARG;
  const bool aligned = (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)momentum_buf | (uintptr_t)ema) & 15) == 0;
  const StepArgs<true> ea{state, ema, ema_weight};
  const StepArgs<false> sa{state};
  for (int k0 = 0; k0 < nseg; k0 += TF_SGD_MAX_SEGMENTS) {
    SgdSegs t;
    int vec = aligned ? 1 : 0;
    int64_t blocks = 0;
    const int used = fill_table(host_segments, nseg, k0, &t, &vec, &blocks);
    if (used == 0) continue;
    if (ema && state)
      hipLaunchKernelGGL((sgd_segments_kernel<true, true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad,
                         momentum_buf, t, used, lr, momentum, weight_decay, grad_scale, vec, ea);
    else if (ema)
      hipLaunchKernelGGL((sgd_segments_kernel<false, true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad,
                         momentum_buf, t, used, lr, momentum, weight_decay, grad_scale, vec, ea);
    else if (state)
      hipLaunchKernelGGL((sgd_segments_kernel<true, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad,
                         momentum_buf, t, used, lr, momentum, weight_decay, grad_scale, vec, sa);
    else
      hipLaunchKernelGGL((sgd_segments_kernel<false, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad,
                         momentum_buf, t, used, lr, momentum, weight_decay, grad_scale, vec, sa);
  }
  TF_CHECK_LAUNCH();
  return TF_OK;
}

int sgd_flat(float* param, const float* grad, float* momentum_buf, float* ema, int64_t n, float lr, float momentum, float weight_decay,
             float grad_scale, float ema_weight, const tf_clip_state* state, void* stream) {
  if (n < 0 || (n > 0 && (!param || !grad || !momentum_buf))) return TF_ERR_ARG;
  if (n == 0) return TF_OK;
  const int vec = (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)momentum_buf | (uintptr_t)ema) & 15) == 0;   // float4 path needs 16-byte alignment
  int64_t blocks = ((vec ? (n >> 2) : n) + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 2048) blocks = 2048;
  const StepArgs<true> ea{state, ema, ema_weight};
  const StepArgs<false> sa{state};
  if (ema && state)
    hipLaunchKernelGGL((sgd_kernel<true, true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad, momentum_buf, n, lr,
                       momentum, weight_decay, grad_scale, vec, ea);
  else if (ema)
    hipLaunchKernelGGL((sgd_kernel<false, true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad, momentum_buf, n, lr,
                       momentum, weight_decay, grad_scale, vec, ea);
  else if (state)
    hipLaunchKernelGGL((sgd_kernel<true, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad, momentum_buf, n, lr,
                       momentum, weight_decay, grad_scale, vec, sa);
  else
    hipLaunchKernelGGL((sgd_kernel<false, false>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, param, grad, momentum_buf, n, lr,
                       momentum, weight_decay, grad_scale, vec, sa);
  TF_CHECK_LAUNCH();
  return TF_OK;
}
}  // namespace

extern "C" int tf_sgd_step_segments(float* param, const float* grad, float* momentum_buf, const int64_t* host_segments, int nseg,
                                    float lr, float momentum, float weight_decay, float grad_scale, void* stream) {
  return sgd_segments(param, grad, momentum_buf, nullptr, host_segments, nseg, lr, momentum, weight_decay, grad_scale, 0.f, nullptr, stream);
}

extern "C" int tf_sgd_step_segments_clipped(float* param, const float* grad, float* momentum_buf, const int64_t* host_segments, int nseg,
                                            float lr, float momentum, float weight_decay, float grad_scale, const tf_clip_state* state,
                                            void* stream) {
  if (!state) return TF_ERR_ARG;
  return sgd_segments(param, grad, momentum_buf, nullptr, host_segments, nseg, lr, momentum, weight_decay, grad_scale, 0.f, state, stream);
}

extern "C" int tf_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n,
                           float lr, float momentum, float weight_decay, float grad_scale, void* stream) {
  return sgd_flat(param, grad, momentum_buf, nullptr, n, lr, momentum, weight_decay, grad_scale, 0.f, nullptr, stream);
}

extern "C" int tf_sgd_step_clipped(float* param, const float* grad, float* momentum_buf, int64_t n,
                                   float lr, float momentum, float weight_decay, float grad_scale, const tf_clip_state* state, void* stream) {
  if (!state) return TF_ERR_ARG;
  return sgd_flat(param, grad, momentum_buf, nullptr, n, lr, momentum, weight_decay, grad_scale, 0.f, state, stream);
}

// The two updates with the model EMA fused in (state may be null: not clipped, not guarded).
extern "C" int tf_sgd_step_ema(float* param, const float* grad, float* momentum_buf, float* ema, int64_t n, float lr, float momentum,
                               float weight_decay, float grad_scale, float ema_weight, const tf_clip_state* state, void* stream) {
  if (n > 0 && !ema) return TF_ERR_ARG;
  return sgd_flat(param, grad, momentum_buf, ema, n, lr, momentum, weight_decay, grad_scale, ema_weight, state, stream);
}

extern "C" int tf_sgd_step_segments_ema(float* param, const float* grad, float* momentum_buf, float* ema, const int64_t* host_segments, int nseg,
                                        float lr, float momentum, float weight_decay, float grad_scale, float ema_weight,
                                        const tf_clip_state* state, void* stream) {
  if (nseg > 0 && !ema) return TF_ERR_ARG;
  return sgd_segments(param, grad, momentum_buf, ema, host_segments, nseg, lr, momentum, weight_decay, grad_scale, ema_weight, state, stream);
}

extern "C" int tf_ema_update_segments(float* ema, const float* param, const int64_t* host_segments, int nseg, float ema_weight,
                                      const tf_clip_state* state, void* stream) {
  if (nseg < 0 || (nseg > 0 && (!ema || !param || !host_segments))) return TF_ERR_ARG;
  if (nseg == 0) return TF_OK;
  if (!table_ok(host_segments, nseg)) return TF_ERR_ARG;
  const bool aligned = (((uintptr_t)ema | (uintptr_t)param) & 15) == 0;
  for (int k0 = 0; k0 < nseg; k0 += TF_SGD_MAX_SEGMENTS) {
    SgdSegs t;
    int vec = aligned ? 1 : 0;
    int64_t blocks = 0;
    const int used = fill_table(host_segments, nseg, k0, &t, &vec, &blocks);
    if (used == 0) continue;
    hipLaunchKernelGGL(ema_segments_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ema, param, t, used, ema_weight, vec,
                       state);
  }
  TF_CHECK_LAUNCH();
  return TF_OK;
}

// One double per block of every launch, at the capped grid: the caller sizes the workspace from the table length alone.
extern "C" size_t tf_grad_norm_workspace_bytes(int nseg) {
  if (nseg <= 0) return 0;
  const size_t launches = ((size_t)nseg + TF_SGD_MAX_SEGMENTS - 1) / TF_SGD_MAX_SEGMENTS;
  return launches * 2048 * sizeof(double);
}

extern "C" int tf_grad_clip_coef(const float* grad, const int64_t* host_segments, int nseg, float grad_scale, float max_norm, int flags,
                                 void* ws, size_t ws_bytes, tf_clip_state* state, void* stream) {
  if (!state || nseg < 0 || (nseg > 0 && (!grad || !host_segments || !ws))) return TF_ERR_ARG;
  if (nseg > 0 && (!table_ok(host_segments, nseg) || ws_bytes < tf_grad_norm_workspace_bytes(nseg) || ((uintptr_t)ws & 7))) return TF_ERR_ARG;
  double* partials = (double*)ws;
  const bool aligned = ((uintptr_t)grad & 15) == 0;
  int64_t base = 0;                                             // partials written so far: launch k stores [base, base + its blocks)
  for (int k0 = 0; k0 < nseg; k0 += TF_SGD_MAX_SEGMENTS) {
    SgdSegs t;
    int vec = aligned ? 1 : 0;
    int64_t blocks = 0;
    const int used = fill_table(host_segments, nseg, k0, &t, &vec, &blocks);
    if (used == 0) continue;
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, grad, t, used, vec, partials + base);
    base += blocks;
  }
  hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)partials, (int)base, grad_scale,
                     max_norm, flags, state);
  TF_CHECK_LAUNCH();
  return TF_OK;
}

extern "C" int tf_scale_segments(float* grad, const int64_t* host_segments, int nseg, const tf_clip_state* state, void* stream) {
  if (!state || nseg < 0 || (nseg > 0 && (!grad || !host_segments))) return TF_ERR_ARG;
  if (nseg == 0) return TF_OK;
  if (!table_ok(host_segments, nseg)) return TF_ERR_ARG;
  const bool aligned = ((uintptr_t)grad & 15) == 0;
  for (int k0 = 0; k0 < nseg; k0 += TF_SGD_MAX_SEGMENTS) {
    SgdSegs t;
    int vec = aligned ? 1 : 0;
    int64_t blocks = 0;
    const int used = fill_table(host_segments, nseg, k0, &t, &vec, &blocks);
    if (used == 0) continue;
    hipLaunchKernelGGL(scale_segments_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, grad, t, used, vec, state);
  }
  TF_CHECK_LAUNCH();
  return TF_OK;
}

extern "C" int tf_grad_accumulate_segments(float* acc, float* grad, const int64_t* host_segments, int nseg, int mode, void* stream) {
  if (mode != TF_ACCUM_STORE && mode != TF_ACCUM_ADD && mode != TF_ACCUM_FINISH) return TF_ERR_ARG;
  if (nseg < 0 || (nseg > 0 && (!acc || !grad || !host_segments))) return TF_ERR_ARG;
  if (nseg == 0) return TF_OK;
  if (!table_ok(host_segments, nseg)) return TF_ERR_ARG;
  const bool aligned = (((uintptr_t)acc | (uintptr_t)grad) & 15) == 0;
  for (int k0 = 0; k0 < nseg; k0 += TF_SGD_MAX_SEGMENTS) {
    SgdSegs t;
    int vec = aligned ? 1 : 0;
    int64_t blocks = 0;
    const int used = fill_table(host_segments, nseg, k0, &t, &vec, &blocks);
    if (used == 0) continue;
    if (mode == TF_ACCUM_STORE)
      hipLaunchKernelGGL((grad_accumulate_kernel<TF_ACCUM_STORE>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, acc, grad, t, used, vec);
    else if (mode == TF_ACCUM_ADD)
      hipLaunchKernelGGL((grad_accumulate_kernel<TF_ACCUM_ADD>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, acc, grad, t, used, vec);
    else
      hipLaunchKernelGGL((grad_accumulate_kernel<TF_ACCUM_FINISH>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, acc, grad, t, used, vec);
  }
  TF_CHECK_LAUNCH();
  return TF_OK;
}
