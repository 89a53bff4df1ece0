// wgrad_det: the deterministic form of the split-K weight gradients (tf_conv2d_wgrad_det, tf_stem_wgrad_det share its summing kernel).
//
// The atomic epilogues of wgrad_dma_kernel, wgrad_kernel and stem_wgrad_kernel add every block's fp32 tile into dW in the order the blocks
// happen to finish: the last bits of a weight gradient differ from run to run.  In the slab form (template parameter DET of those kernels) a
// block stores its tile with plain 16-byte stores into its own place of a caller-owned slab -- never read by the kernel, never zeroed -- and
// the kernel of this file, generalised from wgrad3x3_reduce_kernel, sums the slices of every output element in an order that depends on the
// slice count alone (include/tinyfaces_hip.h at tf_conv2d_wgrad_det) and adds the total ONCE into dW: one writer per element, no atomics.
#include "wgrad_det.h"
#include "profile.h"

namespace {

// 256 threads = (256 / SG) float4 columns x SG slice groups.  Group g sums the slices g, g + SG, g + 2 SG ... in rising order from 0.0f; the
// group sums meet in LDS and are added in rising g onto group 0's.  (fp32 adds only: nothing here can be contracted into an FMA.)
template <int SG>
__global__ void __launch_bounds__(256) wgrad_det_reduce_kernel(const tf_wdet_reduce a) {
  constexpr int COLS = 256 / SG;
  __shared__ float4 part[SG][COLS + 1];
  const bool flat = a.flat_floats > 0;
  const int tile_floats = a.BC * a.BC;
  const size_t slice_floats = flat ? (size_t)a.flat_floats : (size_t)a.ntaps * a.nco * a.nci * tile_floats;
  const size_t total4 = slice_floats / 4;
  const int col = threadIdx.x % COLS, sg = threadIdx.x / COLS;
  const size_t e4 = (size_t)blockIdx.x * COLS + col;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (e4 < total4) {
    const float* src = a.slab + e4 * 4;
#pragma unroll 4
    for (int ks = sg; ks < a.slices; ks += SG) {
      const float4 v = *reinterpret_cast<const float4*>(src + (size_t)ks * slice_floats);
      s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
    }
  }
  if (SG > 1) {
    part[sg][col] = s;
    __syncthreads();
    if (sg != 0) return;
#pragma unroll
    for (int g = 1; g < SG; ++g) { const float4 v = part[g][col]; s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
  }
  if (e4 >= total4) return;
  const size_t e = e4 * 4;
  const float v[4] = {s.x, s.y, s.z, s.w};
  if (flat) {
#pragma unroll
    for (int j = 0; j < 4; ++j) a.dw[e + j] += v[j];
    return;
  }
  const int tile = (int)(e / tile_floats), rem = (int)(e - (size_t)tile * tile_floats);
  const int tci = tile % a.nci, t2 = tile / a.nci, tco = t2 % a.nco, tap = t2 / a.nco;
  const int co = tco * a.BC + rem / a.BC, ci = tci * a.BC + rem % a.BC;
  if (co >= a.Cout) return;
  const float sc = a.row_scale ? a.row_scale[co] : 1.f;
  float* d = a.dw + (size_t)co * a.dw_ld + (size_t)tap * a.tap_stride;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (ci + j < a.Cin) d[(size_t)(ci + j) * a.ci_stride] += a.row_scale ? __fmul_rn(v[j], sc) : v[j];      // (rounded product: no FMA with the add into dw)
}

}  // namespace

// slice groups of the summing kernel: a function of the slice count alone (part of the summation-order contract; the all-taps 3x3 kernel's
// own summing kernel takes the same)
extern "C" int tf_wgrad_det_groups(int slices) { return slices >= 128 ? 16 : slices >= 32 ? 4 : slices >= 16 ? 2 : 1; }

int tf_wgrad_det_reduce_launch(const tf_wdet_reduce& r, hipStream_t stream) {
  if (r.slices < 1 || !r.slab || !r.dw) return TF_ERR_ARG;
  const size_t slice_floats = r.flat_floats > 0 ? (size_t)r.flat_floats : (size_t)r.ntaps * r.nco * r.nci * r.BC * r.BC;
  if (slice_floats == 0 || slice_floats % 4) return TF_ERR_ARG;
  const size_t total4 = slice_floats / 4;
  const int sg = tf_wgrad_det_groups(r.slices);
  const size_t cols = 256 / sg, blocks = (total4 + cols - 1) / cols;
  if (blocks > 0x7fffffffull) return TF_ERR_ARG;
  const dim3 grid((unsigned)blocks);
  if (sg == 16)     hipLaunchKernelGGL(wgrad_det_reduce_kernel<16>, grid, dim3(256), 0, stream, r);
  else if (sg == 4) hipLaunchKernelGGL(wgrad_det_reduce_kernel<4>, grid, dim3(256), 0, stream, r);
  else if (sg == 2) hipLaunchKernelGGL(wgrad_det_reduce_kernel<2>, grid, dim3(256), 0, stream, r);
  else              hipLaunchKernelGGL(wgrad_det_reduce_kernel<1>, grid, dim3(256), 0, stream, r);
  return hipGetLastError() == hipSuccess ? TF_OK : TF_ERR_LAUNCH;
}

namespace {
// the operand checks and the kernel choice of tf_conv2d_wgrad (csrc/wgrad.hip), in its slab form
int det_dispatch(const tf_wgrad_args* a, hipStream_t stream, size_t* query) {
  if (!a || !a->x || !a->dy || !a->dw_oihw) return TF_ERR_ARG;
  if (a->dtype != TF_BF16 && a->dtype != TF_F32) return TF_ERR_UNSUPPORTED;
  const int eps = a->dtype == TF_BF16 ? 8 : 4;
  if (a->ldx % eps || a->lddy % eps || a->ldx < a->Cin || a->lddy < a->Cout) return TF_ERR_ARG;
  if (a->pro_scale && (!a->pro_shift || a->Cin % eps)) return TF_ERR_ARG;
  if (a->N < 1 || a->OH < 1 || a->OW < 1 || a->Cin < 1 || a->Cout < 1 || a->KH < 1 || a->KW < 1) return TF_ERR_ARG;
  if (!query && (!a->partial_ws || ((uintptr_t)a->partial_ws & 15))) return TF_ERR_ARG;      // 16-byte stores into the slab
  if ((a->tile == 0 || a->tile == 3) && a->dtype == TF_BF16 && !a->pro_scale) {
    const int rc = a->row_scale ? TF_ERR_UNSUPPORTED : tf_wgrad3x3_det_launch(a, stream, query);
    if (rc != TF_ERR_UNSUPPORTED || a->tile == 3) return rc;
  }
  if ((a->tile == 0 || a->tile == 1) && a->dtype == TF_BF16 && !a->pro_scale) return tf_wgrad_dma_det_launch(a, stream, query);
  if (a->tile == 1 || a->tile == 3) return TF_ERR_UNSUPPORTED;
  return tf_wgrad_reg_det_launch(a, stream, query);
}
}  // namespace

extern "C" size_t tf_wgrad_det_workspace_bytes(const tf_wgrad_args* a) {
  size_t bytes = 0;
  return det_dispatch(a, nullptr, &bytes) == TF_OK ? bytes : 0;
}

extern "C" int tf_conv2d_wgrad_det(const tf_wgrad_args* a, void* stream) { return det_dispatch(a, (hipStream_t)stream, nullptr); }
