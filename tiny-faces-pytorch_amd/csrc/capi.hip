// Library identity + the list of symbols a binding must resolve (checked by the CPU test-suite).
#include "common.h"
#include "debug_api.h"

static const char* const kSymbols[] = {
    "tf_version", "tf_build_id", "tf_symbol_count", "tf_symbol_name",
    "tf_targets_workspace_bytes", "tf_dense_overlap_targets", "tf_dense_overlap_iou", "tf_pairwise_iou_distance",
    "tf_targets_comp_workspace_bytes", "tf_dense_overlap_targets_comp", "tf_targets_apply_ignore",
    "tf_targets_atss_workspace_bytes", "tf_targets_atss", "tf_targets_tal_workspace_bytes", "tf_targets_tal",
    "tf_targets_tal_aligned_workspace_bytes", "tf_targets_tal_aligned",
    "tf_nms_workspace_bytes", "tf_nms_f64", "tf_nms_batched_workspace_bytes", "tf_nms_f64_batched",
    "tf_decode_workspace_bytes", "tf_decode_compact",
    "tf_box_vote_f64", "tf_box_vote_f64_batched", "tf_boxes_unflip_f64",
    "tf_soft_nms_workspace_bytes", "tf_soft_nms_f64", "tf_soft_nms_batched_workspace_bytes", "tf_soft_nms_f64_batched",
    "tf_soft_nms_f64_capped", "tf_soft_nms_f64_batched_capped",
    "tf_matrix_nms_workspace_bytes", "tf_matrix_nms_f64", "tf_matrix_nms_batched_workspace_bytes", "tf_matrix_nms_f64_batched",
    "tf_topk_workspace_bytes", "tf_topk_select_f64", "tf_topk_batched_workspace_bytes", "tf_topk_select_f64_batched",
    "tf_wider_match_workspace_bytes", "tf_wider_match_f64_batched", "tf_wider_pr_accumulate",
    "tf_criterion_workspace_bytes", "tf_criterion_fwd_bwd", "tf_criterion_focal_workspace_bytes", "tf_criterion_focal_fwd_bwd",
    "tf_criterion_focal_box_fwd_bwd", "tf_criterion_quality_workspace_bytes", "tf_criterion_quality_fwd_bwd",
    "tf_criterion_aligned_workspace_bytes", "tf_criterion_aligned_fwd_bwd",
    "tf_sgd_step", "tf_sgd_step_segments", "tf_image_prepare", "tf_image_prepare_jitter_workspace_bytes", "tf_image_prepare_jitter",
    "tf_grad_norm_workspace_bytes", "tf_grad_clip_coef", "tf_sgd_step_clipped", "tf_sgd_step_segments_clipped", "tf_scale_segments",
    "tf_sgd_step_ema", "tf_sgd_step_segments_ema", "tf_ema_update_segments",
    "tf_grad_accumulate_segments",
    "tf_adamw_advance", "tf_adamw_step", "tf_adamw_step_segments",
    "tf_conv_mtiles", "tf_conv2d", "tf_pack_weight", "tf_pack_weights_batched", "tf_pack_weights_tiled", "tf_conv2d_wgrad", "tf_conv2d_wgrad_group", "tf_wgrad_workspace_bytes", "tf_unpack_dw",
    "tf_wgrad_det_workspace_bytes", "tf_conv2d_wgrad_det", "tf_wgrad_det_groups", "tf_stem_wgrad_det", "tf_stem_wgrad_det_workspace_bytes",
    "tf_set_deterministic", "tf_get_deterministic",
    "tf_stem_im2col", "tf_stem_conv", "tf_stem_wgrad", "tf_maxpool_fwd", "tf_maxpool_bwd", "tf_maxpool_bwd_stats", "tf_colstats_blocks", "tf_colstats",
    "tf_bn_finalize", "tf_bn_fold", "tf_bn_bwd_finalize", "tf_bn_bwd_apply", "tf_bn_relu", "tf_bn_add_relu",
    "tf_bn_relu_fused", "tf_bn_add_relu_fused", "tf_bn_bwd_apply_fused",
    "tf_upsample_add_crop", "tf_upsample_add_crop_bwd", "tf_reduce_partials",
    "tf_detnet_num_params", "tf_detnet_param_name", "tf_detnet_param_numel", "tf_detnet_workspace_bytes",
    "tf_detnet_out_shape", "tf_detnet_param_region_bytes", "tf_detnet_forward", "tf_detnet_backward", "tf_detnet_ctx_create", "tf_detnet_ctx_destroy", "tf_detnet_forward_ctx", "tf_detnet_backward_ctx", "tf_comm_available", "tf_comm_unique_id", "tf_comm_init", "tf_comm_destroy", "tf_comm_rank", "tf_comm_world", "tf_allreduce_bucket", "tf_comm_join", "tf_comm_allreduce_hook",
    "tf_detnet_set_dual_stream", "tf_detnet_set_grad_events", "tf_detnet_set_grad_callback",
    "tf_detnet_trunk_num_params", "tf_detnet_trunk_param_name", "tf_detnet_trunk_param_numel", "tf_detnet_trunk_workspace_bytes",
    "tf_detnet_trunk_param_region_bytes", "tf_detnet_trunk_forward_ctx", "tf_detnet_trunk_backward_ctx",
    "tf_detnet_trunk_backward_frozen_ctx", "tf_detnet_backward_frozen_ctx", "tf_detnet_trunk_backward_frozen_from_ctx",
    "tf_set_stat_rows", "tf_get_stat_rows", "tf_profile_enable", "tf_profile_collect", "tf_profile_shapes",
};

namespace tf {
static thread_local hipEvent_t g_next_stop_event = nullptr;
void set_next_stop_event(hipEvent_t e) { g_next_stop_event = e; }
hipEvent_t take_next_stop_event() { hipEvent_t e = g_next_stop_event; g_next_stop_event = nullptr; return e; }
}  // namespace tf

extern "C" int tf_version(void) { return 810; }   // 810: Matrix NMS (tf_matrix_nms_f64, tf_matrix_nms_f64_batched and their workspace queries); 800: task-aligned target assignment (tf_targets_tal, tf_targets_tal_workspace_bytes); 790: quality focal loss (tf_criterion_quality_fwd_bwd, tf_criterion_quality_workspace_bytes); 780: ATSS target assignment (tf_targets_atss, tf_targets_atss_workspace_bytes); 770: ignore regions of the training targets (tf_targets_apply_ignore); 760: scale-compensated anchor matching (tf_dense_overlap_targets_comp, tf_targets_comp_workspace_bytes); 750: deterministic training (tf_set_deterministic, tf_conv2d_wgrad_det, tf_stem_wgrad_det and their workspace queries); 740: WIDER evaluation on the device (tf_wider_match_f64_batched, tf_wider_pr_accumulate, tf_wider_match_workspace_bytes); 730: colour jitter (tf_image_prepare_jitter, tf_image_prepare_jitter_workspace_bytes); 720: top-k selection + the Soft-NMS cap (tf_topk_select_f64[_batched], tf_soft_nms_f64[_batched]_capped); 710: AdamW (tf_adamw_advance, tf_adamw_step, tf_adamw_step_segments); 700: IoU / GIoU / DIoU regression losses (tf_criterion_focal_box_fwd_bwd); 690: focal loss (tf_criterion_focal_fwd_bwd); 680: Soft-NMS (tf_soft_nms_f64, tf_soft_nms_f64_batched); 670: gradient accumulation (tf_grad_accumulate_segments); 660: test-time augmentation (tf_box_vote_f64, tf_box_vote_f64_batched, tf_boxes_unflip_f64); 650: model EMA (tf_sgd_step_ema, tf_sgd_step_segments_ema, tf_ema_update_segments); 640: gradient-norm clipping + the non-finite-step guard (tf_grad_clip_coef, tf_sgd_step*_clipped, tf_scale_segments); 630: partial freeze (tf_detnet_trunk_backward_frozen_from_ctx); 620: frozen BatchNorm (training = 2, tf_detnet_*backward_frozen_ctx, tf_sgd_step_segments); 610: tf_detnet_trunk_* (ResNet-50 / -152 trunks); r6: tf_build_id; r4: context + hooks + communicator entry points
#ifndef TF_BUILD_ID
#define TF_BUILD_ID "unstamped"
#endif
// digest of the sources this library was built from (build.py: sha256 over csrc/* + include/tinyfaces_hip.h + the compiler flags): what a
// committed profile is stamped with, so that a measurement taken with another binary is recognised as stale (bench.py `traffic_stale`)
extern "C" const char* tf_build_id(void) { return TF_BUILD_ID; }
static int g_stat_rows = 8;
// deterministic switch: while on, the statistic rows read as unfolded whatever was set (a tf_set_stat_rows call in between is kept for when
// the switch goes off) and the executor takes the slab forms of the weight gradients (csrc/detnet.hip)
static int g_deterministic = 0;
extern "C" int tf_set_stat_rows(int rows) { g_stat_rows = rows <= 0 ? (1 << 30) : (rows > TF_STAT_ROWS ? TF_STAT_ROWS : rows); return TF_OK; }
extern "C" int tf_get_stat_rows(void) { return g_deterministic ? (1 << 30) : g_stat_rows; }
extern "C" int tf_set_deterministic(int on) { g_deterministic = on ? 1 : 0; return TF_OK; }
extern "C" int tf_get_deterministic(void) { return g_deterministic; }
extern "C" int tf_symbol_count(void) { return (int)(sizeof(kSymbols) / sizeof(kSymbols[0])); }
extern "C" const char* tf_symbol_name(int i) { return (i >= 0 && i < tf_symbol_count()) ? kSymbols[i] : nullptr; }

// Hardware probe used by the GPU test-suite: records what ds_read_b64_tr_b16 returns when LDS
// holds the identity (element e = e) and lane l supplies the address of elements [4l, 4l+4).
namespace {
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
__global__ void probe_tr16_kernel(unsigned short* out) {
  __shared__ __attribute__((aligned(16))) unsigned short lds[256];
  for (int i = threadIdx.x; i < 256; i += 64) lds[i] = (unsigned short)i;
  __syncthreads();
  typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
  const bf16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)(lds + threadIdx.x * 4));
  const uint2 raw = __builtin_bit_cast(uint2, v);
  out[threadIdx.x * 4 + 0] = (unsigned short)(raw.x & 0xffff); out[threadIdx.x * 4 + 1] = (unsigned short)(raw.x >> 16);
  out[threadIdx.x * 4 + 2] = (unsigned short)(raw.y & 0xffff); out[threadIdx.x * 4 + 3] = (unsigned short)(raw.y >> 16);
}
}  // namespace
extern "C" int tf_probe_tr16(unsigned short* out256, void* stream) {
  hipLaunchKernelGGL(probe_tr16_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out256);
  TF_CHECK_LAUNCH();
  return TF_OK;
}
