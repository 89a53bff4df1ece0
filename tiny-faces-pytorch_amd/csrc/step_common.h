// What the optimizer translation units (sgd.hip, adamw.hip) share: the tail arguments of a step kernel, the fused model-EMA operation and
// the range table of the *_segments entry points with its host-side helpers.  Everything sits in an anonymous namespace, as it did when
// sgd.hip held it alone: each translation unit gets its own copy, and the kernels keep their names and their code.
#pragma once
#include "common.h"

namespace {
// CLIP: `st` is the verdict of a tf_grad_clip_coef enqueued earlier on the stream -- a skipped step returns before it touches p or m, a
// clipped one uses gs * coef (one fp32 product).  CLIP = false never looks at `st`: the code of the plain entry points.
//
// EMA: `a.e` is the averaged copy of p, updated behind the update of the same element as e = fmaf(w, p_new - e, e), one explicitly
// fused fp32 operation (torch.lerp(e, p, w) for w < 0.5) that no contraction flag can change.  A skipped step returns before it touches e
// either.  The last kernel argument is the clip state alone for EMA = false -- the argument block and the code the kernel had before the
// average existed -- and the state, e and w for EMA = true.
template <bool EMA> struct StepArgs { const tf_clip_state* st; float* e; float w; };
template <> struct StepArgs<false> { const tf_clip_state* st; };
__device__ __forceinline__ float ema_of(float e, float p, float w) { return __fmaf_rn(w, p - e, e); }

// A table of element ranges (frozen BatchNorm: the conv weights of the trunk group, whose BN vectors sit in between and must see neither
// weight decay nor momentum).  The ranges are laid end to end into one compact index space (cum[k] = elements in front of range k); a
// thread takes four consecutive compact elements, finds their range by bisection and moves them as one float4 when the table is
// 4-aligned (every conv weight of the trunk is), one by one otherwise.
struct SgdSegs { int64_t start[TF_SGD_MAX_SEGMENTS]; int64_t cum[TF_SGD_MAX_SEGMENTS + 1]; };
__device__ __forceinline__ int seg_of(const SgdSegs& t, int nseg, int64_t j) {
  int lo = 0, hi = nseg - 1;
  while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (t.cum[mid] <= j) lo = mid; else hi = mid - 1; }
  return lo;
}

bool table_ok(const int64_t* host_segments, int nseg) {          // ascending, disjoint
  int64_t prev = 0;
  for (int k = 0; k < nseg; ++k) {
    const int64_t s = host_segments[2 * k], e = host_segments[2 * k + 1];
    if (s < prev || e < s) return false;
    prev = e;
  }
  return true;
}
// The table of the launch that starts at range k0 (empty ranges dropped).  Returns the ranges used; *vec is cleared by a range that is not
// 4-aligned, *blocks is the capped grid (<= 2048 blocks of 256 threads, four compact elements per thread and trip).
int fill_table(const int64_t* host_segments, int nseg, int k0, SgdSegs* t, int* vec, int64_t* blocks) {
  const int n = nseg - k0 < TF_SGD_MAX_SEGMENTS ? nseg - k0 : TF_SGD_MAX_SEGMENTS;
  int64_t cum = 0;
  int used = 0;
  for (int k = 0; k < n; ++k) {
    const int64_t s = host_segments[2 * (k0 + k)], e = host_segments[2 * (k0 + k) + 1];
    if (e == s) continue;
    if ((s & 3) || (e & 3)) *vec = 0;
    t->start[used] = s; t->cum[used] = cum; cum += e - s; ++used;
  }
  if (used == 0) return 0;
  t->cum[used] = cum;
  for (int k = used; k < TF_SGD_MAX_SEGMENTS; ++k) { t->start[k] = 0; t->cum[k + 1] = cum; }
  int64_t b = ((cum + 3) / 4 + 255) / 256;
  if (b < 1) b = 1;
  if (b > 2048) b = 2048;
  *blocks = b;
  return used;
}
}  // namespace
