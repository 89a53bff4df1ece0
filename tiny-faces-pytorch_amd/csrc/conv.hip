// tf_conv2d: argument checks, tile selection (pick_tile) and dispatch of the convolution kernels (gfx950).
// Replaces the nn.Conv2d / BatchNorm2d / ReLU / residual-add chain of tinyfaces/models/model.py:90-106 and the torchvision Bottleneck
// (see tinyfaces_hip.h).  GEMM view:  D[channel][pixel] = sum_k W[channel][k] * X[pixel][k],  k = (tap, cin).
// The kernels: conv_dma_impl.h (LDS-DMA implicit GEMM: every conv but ...), conv3x3h.hip (... the 3x3 / stride 1 convs with >= 256 input
// channels), conv_pws.hip (the wave-autonomous streaming kernel of the short-K / large-M pointwise launches).  r4: the register-staged kernel of round 1
// (conv_igemm, tile codes 1-3, the only one with a producer-BN prologue) was dead on the executor's path since round 1's LDS-DMA
// kernel and was removed: tf_conv2d returns TF_ERR_UNSUPPORTED for tile codes < 10 and for pro_scale (tf_conv2d_wgrad keeps its prologue).
#include <cstdlib>
#include "common.h"
#include "profile.h"

int tf_conv_dma_launch(const tf_conv_args* a, int tile, int depth, hipStream_t stream);   // conv_dma.hip
bool tf_conv3x3h_applicable(const tf_conv_args* a, bool forced);                              // conv3x3h.hip
int tf_conv3x3h_mtiles(const tf_conv_args* a);
int tf_conv3x3h_launch(const tf_conv_args* a, hipStream_t stream);
bool tf_conv_pws_applicable(const tf_conv_args* a);                                            // conv_pws.hip
int tf_conv_pws_launch(const tf_conv_args* a, hipStream_t stream);

namespace {

int pick_tile(const tf_conv_args* a) {
  if (a->tile) return a->tile;
  // 70 = conv_pws (r5): wave-autonomous streaming kernel for the short-K / large-M pointwise launches (layer 1, the large pyramid levels)
  if (tf_conv_pws_applicable(a)) return 70;
  // measured on the bs=12 500x500 layer shapes (scripts/microbench.py): 128 pixels x 64 channels wins on every
  // layer (more, smaller tiles -> more blocks in flight per CU); 64x64 only when even that leaves CUs idle.
  const long M = (long)a->N * a->OH * a->OW;
  // LDS-DMA pipeline.  bf16 convs of <= 4 K-stages (K <= 256 pointwise) are dispatch + epilogue bound: 128-pixel tiles without a
  // ring halve their block count at the same 4 blocks per CU (+0.6 % on the step, A/B on one box: 1036.6 -> 1043.3 img/s);
  // everything else 64x64 with the ring depth chosen by K.  The choice lives HERE so that tf_conv_mtiles agrees with the launch.
  const int nst = a->KH * a->KW * (a->Cin / 64);
  // r3: ... except where the launch is big enough to be throughput-bound: from M = 16 384 pixels on, 64 pixels x 128 channels on
  // 32x32x16 fragments with a 2-deep ring moves the same bytes faster (1920x2560 pyramid level: 256 -> 1024 at M = 19 200 35.6 -> 30.7 us,
  // 128 -> 512 at M = 76 800 49.1 -> 40.8 us, 64 -> 256 at M = 307 200 103 -> 95 us; profiles/r03_microbench_eval.txt).  The hand-over
  // data gradients (RES + MASK2 [+ STATS3]: four M x Cout tensors per launch) take it from the same M.
  // (r4: a 128 x 128 / eight-wave pointwise kernel, conv_pw8, was built for the K >= 512 GEMMs and measured no faster on any layer shape:
  //  profiles/r04_conv_pw8_negative.txt -- removed again)
  if (a->dtype != TF_F32 && nst <= 4 && M >= 16384 && a->Cout % 128 == 0 && a->Cout >= 256) return 46;
  if (a->dtype != TF_F32 && nst <= 4) return 32;
  // 32x32x16 fragments (64 pixels x 128 channels per block, 32 x 64 per wave, 2-deep ring) win where a launch still has several
  // blocks per CU AND a long K loop: 3x3 convs / K >= 576 with M >= 16 384 pixels -- layer 2 at bs = 12 (26.3 vs 32.9 us forward,
  // 25.0 vs 30.6 us data gradient) and layers 2-3 of the evaluation pyramid (41.0 vs 50.6, 40.2 vs 44.8, 21.3 vs 23.8 us);
  // at M = 12 288 (layer 3, bs = 12) they lose: one block per CU, nothing hides a wave's LDS latency
  // (profiles/r02a_microbench_mma32_tiles.txt, profiles/r02a_microbench_eval_tiles.txt)
  // 3x3 / stride 1 with >= 128 output channels and enough tiles to fill the chip: the halo-resident kernel (conv3x3h.hip), which
  // moves each input byte into LDS once per 64-channel chunk instead of once per tap
  if (tf_conv3x3h_applicable(a, false)) return 50;
  if (a->dtype != TF_F32 && nst >= 9 && M >= 16384 && a->Cout % 128 == 0) return 46;
  return 13;
}
int tile_bm(int t) { return ((t % 10) == 3 || (t % 10) == 6) ? 64 : 128; }
// every epilogue moves 16-byte chunks of a row of y / aux / aux2 / aux3 (4 fp32, 8 bf16 / fp16 channels) guarded by c0 < ldy alone, and reads the
// per-channel vectors [ldy] the same way: a row pitch that is no multiple of 16 bytes would let the last chunk of a row run into the next one
bool ldy_ok(const tf_conv_args* a) {
  const int eps = a->dtype == TF_F32 ? 4 : 8;
  return a->ldy >= a->Cout && a->ldy % eps == 0;
}

}  // namespace

extern "C" int tf_conv_mtiles(const tf_conv_args* a) {
  if (!a || !ldy_ok(a)) return TF_ERR_ARG;
  const long M = (long)a->N * a->OH * a->OW;
  const int t = pick_tile(a);
  if (t == 50) { const int mt = tf_conv3x3h_mtiles(a); return mt > tf_get_stat_rows() ? tf_get_stat_rows() : mt; }
  if (t == 60) return TF_ERR_UNSUPPORTED;         // a removed kernel, like codes 1-3: no buffer may be sized from it (the tile-70 rule below)
  // 70 = conv_pws: its blocks add into row blockIdx % rows of the FOLDED statistic rows.  An explicit tile = 70 on a launch the kernel does not
  // take (tf_conv2d then returns TF_ERR_UNSUPPORTED) must not size the caller's buffer from it -- with tf_set_stat_rows(0) that would be 1 << 30
  // rows: such a request is an argument error here too.
  if (t == 70) return tf_conv_pws_applicable(a) ? tf_get_stat_rows() : TF_ERR_UNSUPPORTED;
  const int bm = tile_bm(t);
  const int mt = (int)((M + bm - 1) / bm);
  return (t >= 10 && mt > tf_get_stat_rows()) ? tf_get_stat_rows() : mt;     // the DMA kernel folds its tiles into <= TF_STAT_ROWS rows
}

extern "C" int tf_conv2d(const tf_conv_args* a, void* stream_) {
  hipStream_t stream = (hipStream_t)stream_;
  if (!a || !a->x || !a->w || !a->y) return TF_ERR_ARG;
  const int kch = a->dtype == TF_F32 ? 32 : 64;
  if (a->dtype != TF_BF16 && a->dtype != TF_F32 && a->dtype != TF_F16) return TF_ERR_UNSUPPORTED;
  if (a->pro_scale) return TF_ERR_UNSUPPORTED;    // the producer-BN prologue went with the register-staged kernel (r4)
  if (a->bnf) return TF_ERR_UNSUPPORTED;          // the in-LDS BatchNorm prologue was measured, lost and removed: the bnf* fields are reserved
  if (a->Cin % kch != 0 || !ldy_ok(a)) return TF_ERR_ARG;
  if (a->stride != 1 && a->stride != 2) return TF_ERR_UNSUPPORTED;
  if ((a->epi & (TF_EPI_STATS | TF_EPI_STATS2 | TF_EPI_STATS3)) && !a->stat_out) return TF_ERR_ARG;
  {
    const int ns = !!(a->epi & TF_EPI_STATS) + !!(a->epi & TF_EPI_STATS2) + !!(a->epi & TF_EPI_STATS3);
    if (ns > 1) return TF_ERR_ARG;
  }
  if ((a->epi & TF_EPI_MASK2) && !a->aux2) return TF_ERR_ARG;
  if ((a->epi & TF_EPI_STATS3) && !a->aux3) return TF_ERR_ARG;
  if ((a->epi & TF_EPI_JOIN) && (a->epi & (TF_EPI_MASK2 | TF_EPI_STATS3))) return TF_ERR_ARG;     // aux2 / aux3 have one meaning per launch
  if ((a->epi & (TF_EPI_RES | TF_EPI_MASK | TF_EPI_STATS2)) && !a->aux) return TF_ERR_ARG;
  if ((a->epi & TF_EPI_JOIN) && (!a->aux2 || !a->aux3)) return TF_ERR_ARG;
  if ((a->epi & TF_EPI_AFFINE) && (!a->epi_scale || !a->epi_shift)) return TF_ERR_ARG;
  if ((a->epi & TF_EPI_MASK) && (!a->mask_scale || !a->mask_shift)) return TF_ERR_ARG;
  const int t = pick_tile(a);
  if (t == 50) return tf_conv3x3h_applicable(a, true) ? tf_conv3x3h_launch(a, stream) : TF_ERR_UNSUPPORTED;
  if (t == 60) return TF_ERR_UNSUPPORTED;         // the register-staged pointwise kernel with BatchNorm prologues: measured, lost, removed
  if (t == 70) return tf_conv_pws_launch(a, stream);
  if (t >= 10) {
    return tf_conv_dma_launch(a, t % 10, t >= 40 ? 2 : (t >= 30 ? 1 : (t >= 20 ? 4 : 3)), stream);
  }
  return TF_ERR_UNSUPPORTED;                      // tile codes 1-3: the register-staged kernel of round 1, removed in r4
}
