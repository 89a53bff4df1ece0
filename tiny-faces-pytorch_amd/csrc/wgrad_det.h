// Deterministic (slab) form of the split-K weight gradients: what the kernel files share with csrc/wgrad_det.hip.
#pragma once
#include "common.h"

// one summing launch: dw += row_scale * (sum over the slices of a slab), single writer per element (contract: include/tinyfaces_hip.h)
struct tf_wdet_reduce {
  const float* slab; float* dw; const float* row_scale;
  int slices;                       // >= 1, every one written by the launch in front
  // tiled form: slab [slice][tap][co tile][ci tile][BC][BC]
  int BC, ntaps, nco, nci, Cout, Cin, dw_ld, ci_stride, tap_stride;
  // flat form (flat_floats > 0, a multiple of 4): slab [slice][flat_floats], dw [flat_floats] contiguous
  int flat_floats;
};
int tf_wgrad_det_reduce_launch(const tf_wdet_reduce& r, hipStream_t stream);

// the slab forms of the three kernel files.  query != NULL: nothing is launched, *query = the preferred slab bytes of the call
int tf_wgrad_dma_det_launch(const tf_wgrad_args* a, hipStream_t stream, size_t* query);        // wgrad_dma.hip
int tf_wgrad_reg_det_launch(const tf_wgrad_args* a, hipStream_t stream, size_t* query);        // wgrad.hip
int tf_wgrad3x3_det_launch(const tf_wgrad_args* a, hipStream_t stream, size_t* query);         // wgrad3x3.hip
