// The detector network as a native graph executor: every kernel launch of a forward or a
// backward pass is issued from here (one C-ABI call per pass, no Python in the loop), with all
// activations carved from one caller-provided arena.
// Replaces DetectionModel.forward (tinyfaces/models/model.py:89-128) over a torchvision
// Bottleneck trunk (stride on the 3x3): ResNet-101 [3,4,23] by default, ResNet-50 [3,4,6] and
// ResNet-152 [3,8,36] through the tf_detnet_trunk_* entry points; and the autograd backward that
// tinyfaces/trainer.py:86 triggers.
//
// Data layout in HBM: activations NHWC ("pixels x channels"), dtype bf16 (fast) or fp32
// (parity); BN vectors, statistics and all gradients fp32; weights re-packed once per training
// step (or once per constant_weights() session in eval) from the fp32 OIHW master copy into
// K-contiguous [Cout][tap][Cin] (forward / wgrad operand) and [Cin][tap][Cout] (data-gradient
// operand), both from one read of the master (tf_pack_weights_tiled).
//
// Fusion plan (what never makes an HBM round trip, and what never costs a launch):
//   eval : BN folded to a per-channel affine inside every conv epilogue, + residual + ReLU.
//   train: conv epilogues fold per-tile (sum, sumsq) into the BN's own statistic rows; the
//          elementwise consumer (bn_relu_fused -> a1/a2, bn_add_relu_fused -> y) finalizes them
//          in-kernel, so a bottleneck is 6 launches.  a1/a2 are materialised on purpose: every
//          conv and every weight gradient then runs on the LDS-DMA pipeline (no prologue).
//   backward: dgrad epilogues apply the ReLU mask and fold the BN-backward sums; the last data
//          gradient of a block hands the previous block g*(y>0) AND its BN3-backward sums
//          (RES|MASK2|STATS3); bn_bwd_apply_fused finalizes in-kernel; weight gradients run on
//          the context's second stream against per-block operand buffers (r4) -- per launch for
//          layers 1-2, deferred and grouped (tf_conv2d_wgrad_group: 8 + 7 + 7 blocks) for the
//          identity bottlenecks of layer 3.
//   stem (r4): conv1 and its weight gradient straight from the NCHW image (stem_conv.hip), the
//          BN-backward sums inside the max-pool backward, the apply inside the weight gradient.
//   tf_set_stat_rows(0) (unfolded, bit-reproducible statistics) falls back to the separate
//   finalize kernels and the unmasked gradient flow: the A/B and race-screen path.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "common.h"
#include "tuning.h"

extern "C" {
int tf_stem_im2col(const float*, int, int, int, int, void*, int, void*);
int tf_stem_conv(int, const float*, int, int, int, const void*, int, void*, int, const float*, const float*, float*, int*, void*);
int tf_stem_wgrad(int, const float*, int, int, int, const void*, const void*, const float*, const float*, const float*, float*, void*);
int tf_maxpool_fwd(int, const void*, int, int, int, int, const float*, const float*, void*, uint8_t*, void*);
int tf_maxpool_bwd(int, const void*, const uint8_t*, const void*, const float*, const float*, int, int, int, int, void*, void*);
int tf_maxpool_bwd_stats(int, const void*, const uint8_t*, const void*, const float*, const float*, int, int, int, int, void*, float*, int*, void*);
int tf_colstats_blocks(int, int, int);
int tf_colstats(int, const void*, const void*, const void*, const void*, int, int, int, float*, void*);
int tf_bn_finalize(const float*, int, int, int, float, const float*, const float*, float, float, float*, float*, float*, float*, float*,
                   float*, int, void*);
int tf_bn_fold(const float*, const float*, const float*, const float*, float, int, float*, float*, void*);
int tf_bn_bwd_finalize(const float*, int, int, int, int, int, float, const float*, const float*, const float*, float*, float*, float*, float*,
                       float*, int, void*);
int tf_bn_bwd_apply(int, const void*, const void*, const void*, const float*, const float*, const float*, int64_t, int, void*, void*);
int tf_bn_add_relu(int, const void*, const float*, const float*, const void*, const float*, const float*, int64_t, int, void*, void*);
int tf_bn_relu(int, const void*, const float*, const float*, int64_t, int, void*, void*);
int tf_upsample_add_crop(int, const void*, const void*, const float*, int, int, int, int, int, int, int, float*, void*);
int tf_upsample_add_crop_bwd(int, const float*, const float*, int, int, int, int, int, int, int, void*, void*, void*);
int tf_reduce_partials(const float*, int, int, int, int, int, float*, int, void*);
int tf_conv2d_wgrad_group(const tf_wgrad_args*, int, void*);
}

namespace {

constexpr int kStemK = 192;     // 147 taps*channels padded to 3 x 64
// r4: conv1 AND its weight gradient straight from the image (csrc/stem_conv.hip: tf_stem_conv, tf_stem_wgrad) for the 2-byte operand types:
// no 288 MB im2col matrix in a training step or an evaluation forward.  fp32 and the unfolded-statistics mode keep im2col + GEMM.
bool stem_direct_mode(int dtype, bool training, bool fused) { return dtype != TF_F32 && (!training || fused); }
constexpr int kHeadLd = 128;    // 125 outputs padded
constexpr int kConstC = 1024;   // widest channel count of the trunk (layer 3 output)
constexpr int kFrozen = TF_DETNET_FROZEN_BN;     // `training` = 2: the evaluation forward + a backward through the folded BN

struct ConvUnit {               // one conv + (optional) BN, with indices into the parameter table
  std::string name;             // e.g. "model.layer1.0.conv1"
  int cin, cout, k, stride, pad;
  int w, gamma, beta, rmean, rvar;   // param-table indices (-1 if absent)
  int bias;                          // heads only
};
struct Block { ConvUnit c1, c2, c3, ds; bool has_ds; int planes, stride, cin; };
struct Arch {
  ConvUnit stem;
  std::vector<Block> blocks;    // 16 / 30 / 47 bottlenecks (resnet50 / 101 / 152)
  int layer_end[3];             // index of the last block of layer1/2/3
  ConvUnit head3, head4;
  int upsample_w;
  std::vector<std::string> names;
};

int add_param(Arch& a, const std::string& n) { a.names.push_back(n); return (int)a.names.size() - 1; }

ConvUnit make_unit(Arch& a, const std::string& conv, const std::string& bn, int cin, int cout, int k, int stride, int pad) {
  ConvUnit u;
  u.name = conv; u.cin = cin; u.cout = cout; u.k = k; u.stride = stride; u.pad = pad; u.bias = -1;
  u.w = add_param(a, conv + ".weight");
  u.gamma = add_param(a, bn + ".weight"); u.beta = add_param(a, bn + ".bias");
  u.rmean = add_param(a, bn + ".running_mean"); u.rvar = add_param(a, bn + ".running_var");
  return u;
}

// The trunks the executor takes: torchvision's Bottleneck ResNets (groups 1, width 64) by their block counts in layers 1-3.  Every
// bottleneck of every trunk has the shape of the same bottleneck of ResNet-101; only the number of identity blocks per layer differs.
constexpr int kTrunks[3][3] = {{3, 4, 6}, {3, 4, 23}, {3, 8, 36}};     // resnet50, resnet101 (the default), resnet152
constexpr int kDefaultTrunk = 1;

Arch build_arch(const int* nblk) {
  Arch a;
  a.stem = make_unit(a, "model.conv1", "model.bn1", 3, 64, 7, 2, 3);
  const int planes[3] = {64, 128, 256};
  int inpl = 64;
  for (int L = 0; L < 3; ++L) {
    for (int b = 0; b < nblk[L]; ++b) {
      Block B;
      const std::string p = "model.layer" + std::to_string(L + 1) + "." + std::to_string(b);
      B.planes = planes[L]; B.stride = (b == 0 && L > 0) ? 2 : 1; B.cin = inpl;
      B.c1 = make_unit(a, p + ".conv1", p + ".bn1", inpl, planes[L], 1, 1, 0);
      B.c2 = make_unit(a, p + ".conv2", p + ".bn2", planes[L], planes[L], 3, B.stride, 1);
      B.c3 = make_unit(a, p + ".conv3", p + ".bn3", planes[L], planes[L] * 4, 1, 1, 0);
      B.has_ds = (b == 0);
      if (B.has_ds) B.ds = make_unit(a, p + ".downsample.0", p + ".downsample.1", inpl, planes[L] * 4, 1, B.stride, 0);
      inpl = planes[L] * 4;
      a.blocks.push_back(B);
    }
    a.layer_end[L] = (int)a.blocks.size() - 1;
  }
  auto head = [&](const std::string& n, int cin) {
    ConvUnit u; u.name = n; u.cin = cin; u.cout = -1; u.k = 1; u.stride = 1; u.pad = 0;
    u.w = add_param(a, n + ".weight"); u.bias = add_param(a, n + ".bias");
    u.gamma = u.beta = u.rmean = u.rvar = -1;
    return u;
  };
  a.head3 = head("score_res3", 512);
  a.head4 = head("score_res4", 1024);
  a.upsample_w = add_param(a, "score4_upsample.weight");
  return a;
}

// The Arch of a trunk (blocks = its block counts in layers 1-3; NULL = ResNet-101), or NULL when the executor does not take it.  All of them
// are built once, under the thread-safe initialisation of a function-local static, and never move: tf_detnet_trunk_param_name hands out
// pointers into them.
const Arch* find_arch(const int* blocks) {
  static const std::vector<Arch> cache = [] {
    std::vector<Arch> v;
    for (const auto& t : kTrunks) v.push_back(build_arch(t));
    return v;
  }();
  if (!blocks) return &cache[kDefaultTrunk];
  for (int k = 0; k < 3; ++k)
    if (blocks[0] == kTrunks[k][0] && blocks[1] == kTrunks[k][1] && blocks[2] == kTrunks[k][2]) return &cache[k];
  return nullptr;
}

// r4: the weight gradients of the identity bottlenecks of layer 3 (22 blocks of identical shape) are differentiated in GROUPS of up to
// kWgradGroup bottlenecks per launch (tf_conv2d_wgrad_group: full-K tiles, no split-K / atomics / partial tiles); their dY operands then
// live in per-block buffers instead of the two parity sets.
constexpr int kWgradGroup = 8;
inline bool wgrad_group_mode(int dtype, int training) { return training && dtype == TF_BF16; }

inline int down2(int n) { return (n - 1) / 2 + 1; }   // every stride-2 stage of the trunk: ceil(n/2)
inline size_t esize(int dtype) { return dtype == TF_F32 ? 4 : 2; }
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Arena {
  char* base; size_t cap, off; bool ok;
  Arena(void* b, size_t c) : base((char*)b), cap(c), off(0), ok(true) {}
  void* get(size_t bytes) {
    const size_t o = off; off += up256(bytes);
    if (off > cap && base) ok = false;
    return base ? base + o : nullptr;
  }
  float* f32(size_t n) { return (float*)get(n * 4); }
};

// per-BN scratch: scale/shift (forward affine), mean/invstd, backward coefficients
// fst / bst: this BN's own statistic rows ([TF_STAT_ROWS][2][C] forward sums, [TF_STAT_ROWS][3][C] backward sums) for the
// consumers that finalize in-kernel (bn_fused.hip); all of them are zeroed by ONE memset per pass
struct BnBuf { float *scale, *shift, *mean, *invstd, *cA, *cB, *cD, *fst, *bst; int C; };
BnBuf bn_alloc(Arena& ar, int C) {
  BnBuf b; float* p = ar.f32((size_t)7 * C);
  b.scale = p; b.shift = p + C; b.mean = p + 2 * C; b.invstd = p + 3 * C; b.cA = p + 4 * C; b.cB = p + 5 * C; b.cD = p + 6 * C;
  b.fst = b.bst = nullptr; b.C = C;
  return b;
}

struct Plan {                    // everything a forward carves; backward re-derives the same pointers
  int dtype, N, H, W, nout, training;
  int H1, W1, H2, W2;            // stem conv out, maxpool out
  void *col, *cstem, *pool, *a1tmp; uint8_t* pool_idx; BnBuf bn_stem;
  void *wstem;
  struct Blk {
    int Hin, Win, Hout, Wout;
    void *c1, *c2, *c3, *d, *y;
    void *a1, *a2;                   // relu(bn1(c1)), relu(bn2(c2)) materialised in training (operands of conv2/conv3 and of their weight gradients)
    void *w1, *w2, *w3, *wd;         // packed forward weights
    void *w1t, *w2t, *w3t, *wdt;     // packed data-gradient (transposed) weights, training only
    void *gT1, *gT2, *gU1, *gT3;     // r4: this block's own g_c3 / g_c2 / g_c1 / downsample-branch gradient (alive until its weight gradients ran)
    BnBuf b1, b2, b3, bd;
  };
  std::vector<Blk> blk;
  void *w_h3, *w_h4, *w_h3t, *w_h4t, *s3, *s4; float *hbias3, *hbias4, *ones, *wup_diag;
  float *c_one, *c_zero;         // frozen BN: kConstC ones / zeros (mask_scale / mask_shift and epi_shift of the AFFINE | MASK data gradients)
  float *partial, *partial_b; size_t partial_floats;      // per-tile partial rows of the forward / backward pass (each behind its statistic region)
  float *stat_fwd, *stat_bwd; size_t stat_fwd_floats, stat_bwd_floats;   // per-BN statistic regions (fused finalize)
  // backward-only
  void *g3, *g4, *G0, *G1, *T4, *R3, *wt; float* dwp; size_t dwp_floats;
  int H3, W3, H4, W4;
  size_t total, param_bytes;
};

size_t packed_bytes(int dtype, int rows, int taps, int cols) { return (size_t)((rows + 127) / 128 * 128) * taps * cols * esize(dtype); }

void build_plan(const Arch& A, Plan& P, Arena& ar, int dtype, int N, int H, int W, int nout, int training) {
  const size_t es = esize(dtype);
  P.dtype = dtype; P.N = N; P.H = H; P.W = W; P.nout = nout; P.training = training;
  P.H1 = down2(H); P.W1 = down2(W); P.H2 = down2(P.H1); P.W2 = down2(P.W1);
  const size_t M1 = (size_t)N * P.H1 * P.W1, M2 = (size_t)N * P.H2 * P.W2;
  // rows of per-tile partial sums the unfolded (tf_set_stat_rows(0)) flow and colstats need: known from the shapes alone
  size_t max_partial = 0;
  {
    auto part = [&](size_t M, int C) { size_t t = ((M + 63) / 64) * 2 * (size_t)C; if (t > max_partial) max_partial = t; };
    part(M1, 64);
    int h = P.H2, w = P.W2;
    for (size_t i = 0; i < A.blocks.size(); ++i) {
      const Block& B = A.blocks[i];
      const int ho = B.stride == 2 ? down2(h) : h, wo = B.stride == 2 ? down2(w) : w;
      part((size_t)N * h * w, B.planes); part((size_t)N * ho * wo, B.planes * 4);
      h = ho; w = wo;
      if ((int)i == A.layer_end[1]) part((size_t)N * h * w, kHeadLd);
    }
    if (max_partial < (size_t)1100 * 3 * 1024) max_partial = (size_t)1100 * 3 * 1024;   // colstats: up to ~1024 blocks x 3 sums x 1024 channels
  }
  P.partial_floats = max_partial + 4096;
  // ---- parameter-derived buffers first: their offsets depend on (dtype, nout, training) only, never on the image size, so an
  //      eval-mode caller may keep them across forwards of different sizes (TF_DETNET_WEIGHTS_READY)
  P.bn_stem = bn_alloc(ar, 64);
  P.wstem = ar.get(packed_bytes(dtype, 64, 1, kStemK));
  P.blk.resize(A.blocks.size());
  size_t max_wt = 0;
  for (size_t i = 0; i < A.blocks.size(); ++i) {
    const Block& B = A.blocks[i];
    Plan::Blk& b = P.blk[i];
    const int pl = B.planes, c4 = pl * 4;
    b.w1 = ar.get(packed_bytes(dtype, pl, 1, B.cin)); b.w2 = ar.get(packed_bytes(dtype, pl, 9, pl));
    b.w3 = ar.get(packed_bytes(dtype, c4, 1, pl));
    b.wd = B.has_ds ? ar.get(packed_bytes(dtype, c4, 1, B.cin)) : nullptr;
    b.w1t = training ? ar.get(packed_bytes(dtype, B.cin, 1, pl)) : nullptr;
    b.w2t = training ? ar.get(packed_bytes(dtype, pl, 9, pl)) : nullptr;
    b.w3t = training ? ar.get(packed_bytes(dtype, pl, 1, c4)) : nullptr;
    b.wdt = (training && B.has_ds) ? ar.get(packed_bytes(dtype, B.cin, 1, c4)) : nullptr;
    b.b1 = bn_alloc(ar, pl); b.b2 = bn_alloc(ar, pl); b.b3 = bn_alloc(ar, c4);
    if (B.has_ds) b.bd = bn_alloc(ar, c4);
    const size_t wtb = packed_bytes(dtype, pl, 9, pl);
    if (wtb > max_wt) max_wt = wtb;
    if (packed_bytes(dtype, B.cin, 1, c4) > max_wt) max_wt = packed_bytes(dtype, B.cin, 1, c4);
  }
  P.w_h3 = ar.get(packed_bytes(dtype, kHeadLd, 1, 512)); P.w_h4 = ar.get(packed_bytes(dtype, kHeadLd, 1, 1024));
  P.w_h3t = training ? ar.get(packed_bytes(dtype, 512, 1, kHeadLd)) : nullptr;
  P.w_h4t = training ? ar.get(packed_bytes(dtype, 1024, 1, kHeadLd)) : nullptr;
  P.hbias3 = ar.f32(kHeadLd); P.hbias4 = ar.f32(kHeadLd); P.ones = ar.f32(kHeadLd);
  P.wup_diag = ar.f32((size_t)nout * 16);
  P.c_one = P.c_zero = nullptr;
  if (training == kFrozen) { P.c_one = ar.f32(kConstC); P.c_zero = ar.f32(kConstC); }
  const bool stats = training != 0 && training != kFrozen;              // the batch-statistics graph: statistic regions, a1 / a2 / c3, the BN-backward operand of the downsample branch
  P.param_bytes = ar.off;
  // ---- per-BN statistic regions, contiguous so that one memset per pass clears them
  {
    std::vector<BnBuf*> bns;
    for (size_t i = 0; i < A.blocks.size(); ++i) {
      Plan::Blk& b = P.blk[i];
      bns.push_back(&b.b1); bns.push_back(&b.b2); bns.push_back(&b.b3);
      if (A.blocks[i].has_ds) bns.push_back(&b.bd);
    }
    size_t nf = 0, nb = 0;
    // forward region of a BN: TF_STAT_ROWS x (sum, sum of squares) + ONE row holding the shift the producer subtracted (r3)
    for (BnBuf* q : bns) { nf += (size_t)(TF_STAT_ROWS * 2 + 1) * q->C; nb += (size_t)TF_STAT_ROWS * 3 * q->C; }
    P.stat_fwd_floats = stats ? nf : 0; P.stat_bwd_floats = stats ? nb : 0;
    // r4: [forward statistic rows | forward partial rows] and [backward statistic rows | backward partial rows] are contiguous pairs, so that
    // ONE memset per pass clears the statistic region AND the head of the pass's partial buffer (two dispatches per pass in rounds 1-3)
    P.stat_fwd = ar.f32(P.stat_fwd_floats); P.partial = ar.f32(P.partial_floats);
    P.stat_bwd = ar.f32(P.stat_bwd_floats); P.partial_b = training ? ar.f32(P.partial_floats) : nullptr;
    size_t of = 0, ob = 0;
    for (BnBuf* q : bns) {
      q->fst = stats && P.stat_fwd ? P.stat_fwd + of : nullptr; q->bst = stats && P.stat_bwd ? P.stat_bwd + ob : nullptr;
      of += (size_t)(TF_STAT_ROWS * 2 + 1) * q->C; ob += (size_t)TF_STAT_ROWS * 3 * q->C;
    }
  }
  // ---- activations
  P.col = ar.get(M1 * kStemK * es);
  P.cstem = ar.get(M1 * 64 * es);
  P.pool = ar.get(M2 * 64 * es);
  P.pool_idx = (uint8_t*)ar.get(training ? M2 * 64 : 0);
  int h = P.H2, w = P.W2;
  size_t max_act = M1 * 64 * es;
  for (size_t i = 0; i < A.blocks.size(); ++i) {
    const Block& B = A.blocks[i];
    Plan::Blk& b = P.blk[i];
    b.Hin = h; b.Win = w; b.Hout = B.stride == 2 ? down2(h) : h; b.Wout = B.stride == 2 ? down2(w) : w;
    const size_t Min = (size_t)N * h * w, Mout = (size_t)N * b.Hout * b.Wout;
    const int pl = B.planes, c4 = pl * 4;
    b.c1 = ar.get(Min * pl * es); b.c2 = ar.get(Mout * pl * es);
    b.a1 = stats ? ar.get(Min * pl * es) : nullptr; b.a2 = stats ? ar.get(Mout * pl * es) : nullptr;
    b.c3 = stats ? ar.get(Mout * c4 * es) : nullptr;
    b.d = B.has_ds ? ar.get(Mout * c4 * es) : nullptr;
    b.y = ar.get(Mout * c4 * es);
    // r4: every block owns its backward operands (g_c3, g_c2, g_c1, downsample-branch gradient).  Rounds 1-3 shared two parity sets and
    // made the chain wait for the weight gradients of block i+2 before it reused their buffers: with the second stream behind by a group
    // launch the chain stalled there (79 us at the top of layer 2, profiles/r04_step_timeline.txt).  0.85 GB of 288 (bf16, bs = 12).
    b.gT1 = b.gT2 = b.gU1 = b.gT3 = nullptr;
    if (training) {
      b.gT1 = ar.get(Mout * c4 * es); b.gT2 = ar.get(Mout * pl * es); b.gU1 = ar.get(Min * pl * es);
      // (frozen BN: gT1 holds the block's OWN masked output gradient gm -- the weight gradients of conv3 and of the downsample conv read it
      //  on the second stream -- and the downsample branch has no BN-backward operand)
      if (B.has_ds && stats) b.gT3 = ar.get(Mout * c4 * es);
    }
    if (Min * (size_t)B.cin * es > max_act) max_act = Min * B.cin * es;
    if (Mout * c4 * es > max_act) max_act = Mout * c4 * es;
    h = b.Hout; w = b.Wout;
  }
  const Plan::Blk& l2 = P.blk[A.layer_end[1]];
  const Plan::Blk& l3 = P.blk[A.layer_end[2]];
  P.H3 = l2.Hout; P.W3 = l2.Wout; P.H4 = l3.Hout; P.W4 = l3.Wout;
  const size_t M3 = (size_t)N * P.H3 * P.W3, M4 = (size_t)N * P.H4 * P.W4;
  P.a1tmp = nullptr;
  P.s3 = ar.get(M3 * kHeadLd * es); P.s4 = ar.get(M4 * kHeadLd * es);
  if (training) {
    P.g3 = ar.get(M3 * kHeadLd * es); P.g4 = ar.get(M4 * kHeadLd * es);
    P.G0 = stats ? ar.get(max_act) : nullptr; P.G1 = stats ? ar.get(max_act) : nullptr;      // (frozen BN: the gradients ping-pong through the blocks' own gT1)
    P.T4 = ar.get(max_act); P.R3 = ar.get(max_act);
    if (packed_bytes(dtype, 1024, 1, kHeadLd) > max_wt) max_wt = packed_bytes(dtype, 1024, 1, kHeadLd);
    P.wt = ar.get(max_wt);
    // scratch of the 3x3 weight gradients: the partial [slice][tile][tap][64][64] tiles of the all-taps kernel (one block per CU:
    // at most 256 + 16 tiles of 144 KiB) or, for the stride-2 convs, the packed [Cout][tap][Cin] gradient of the per-tap kernel
    P.dwp_floats = (size_t)(256 + 16) * 9 * 64 * 64;
    P.dwp = ar.f32(P.dwp_floats);
  } else {
    P.g3 = P.g4 = P.G0 = P.G1 = P.T4 = P.R3 = P.wt = nullptr; P.dwp = nullptr; P.dwp_floats = 0;
  }
  P.total = ar.off;
}

__global__ void fill_const_kernel(float* one, float* zero, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) one[i] = 1.f; else if (i < 2 * n) zero[i - n] = 0.f;
}
// zero up to kZeroRanges ranges per launch (frozen BN: the BN segments inside the range of the flat gradient the split memset skips)
constexpr int kZeroRanges = 128;
struct ZeroRanges { float* p[kZeroRanges]; int n[kZeroRanges]; };
__global__ void zero_ranges_kernel(const ZeroRanges r) {
  float* p = r.p[blockIdx.y];
  const int n = r.n[blockIdx.y];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) p[i] = 0.f;
}

__global__ void head_vectors_kernel(const float* b3, const float* b4, const float* wup, int nout, float* hb3, float* hb4, float* ones,
                                    float* diag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < kHeadLd) { hb3[i] = i < nout ? b3[i] : 0.f; hb4[i] = i < nout ? b4[i] : 0.f; ones[i] = 1.f; }
  if (i < nout * 16) { const int c = i / 16, k = i % 16; diag[i] = wup[((size_t)c * nout + c) * 16 + k]; }
}

struct Ctx {
  int dtype; hipStream_t stream; void* const* params; void* const* grads; int rc;
  bool grads_zeroed = false;
  bool skip_fold = false;
  // tf_set_deterministic(1): every weight gradient takes its slab form (tf_conv2d_wgrad_det / tf_stem_wgrad_det), all on wstream(), so
  // consecutive gradients share the one slab (the arena's P.dwp)
  bool det = false; float* det_slab = nullptr; size_t det_slab_bytes = 0;
  std::vector<tf_pack_job> jobs;
  std::vector<tf_pack2_job> jobs2;
  hipStream_t side = nullptr;                 // weight gradients run here, concurrently with the data-gradient chain
  std::vector<hipEvent_t>* events = nullptr; size_t ev_next = 0;
  hipEvent_t next_event() {
    if (ev_next == events->size()) { hipEvent_t e; if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { chk(TF_ERR_LAUNCH); return nullptr; } events->push_back(e); }
    return (*events)[ev_next++];
  }
  // fork without a packet of its own on `stream`: the NEXT kernel launched through TF_LAUNCH_WITH_STOP_EVENT (the fused BN-backward
  // apply that produces a weight gradient's dY operand) carries the event as its completion signal; join_side() then makes the
  // weight-gradient stream wait for it.  hipEventRecord costs a barrier packet = an ~8 us bubble on the data-gradient chain
  // (profiles/r02_step_timeline.txt), three to four times per bottleneck.
  hipEvent_t pending = nullptr;
  void arm_fork() { if (!side) return; pending = next_event(); if (pending) tf::set_next_stop_event(pending); }
  void fork_armed() {
    if (!side) return;
    if (tf::take_next_stop_event()) pending = nullptr;     // armed but no kernel took it (the producer refused its arguments): plain fork
    if (pending) { (void)hipStreamWaitEvent(side, pending, 0); pending = nullptr; }
    else fork();
  }
  // everything enqueued on `stream` so far becomes a dependency of what is enqueued on `side` next
  void fork() { if (!side) return; hipEvent_t e = next_event(); if (e) { (void)hipEventRecord(e, stream); (void)hipStreamWaitEvent(side, e, 0); } }
  hipEvent_t mark_side() { if (!side) return nullptr; hipEvent_t e = next_event(); if (e) (void)hipEventRecord(e, side); return e; }
  void wait_on_main(hipEvent_t e) { if (e) (void)hipStreamWaitEvent(stream, e, 0); }
  hipStream_t wstream() const { return side ? side : stream; }
  void flush_packs(hipStream_t s = nullptr) {
    if (!s) s = stream;
    if (!jobs.empty()) { chk(tf_pack_weights_batched(dtype, jobs.data(), (int)jobs.size(), s)); jobs.clear(); }
    if (!jobs2.empty()) { chk(tf_pack_weights_tiled(dtype, jobs2.data(), (int)jobs2.size(), s)); jobs2.clear(); }
  }
  const float* P(int i) const { return (const float*)params[i]; }
  float* G(int i) const { return grads ? (float*)grads[i] : nullptr; }
  void chk(int r) { if (r != TF_OK && rc == TF_OK) rc = r; }
};

void conv_fill(tf_conv_args& a, int dtype, int mode, int N, int H, int W, int Cin, int OH, int OW, int Cout, int k, int stride, int pad,
               int ldy, const void* x, const void* w, void* y) {
  memset(&a, 0, sizeof(a));
  a.dtype = dtype; a.mode = mode; a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.OH = OH; a.OW = OW; a.Cout = Cout; a.KH = k; a.KW = k;
  a.stride = stride; a.pad = pad; a.ldy = ldy; a.x = x; a.w = w; a.y = y;
}

void pack(Ctx& c, const ConvUnit& u, int cout, void* out, bool transpose, int cin_override = 0, int cols_pad_override = 0,
          int k_override = 0) {
  const int cin = cin_override ? cin_override : u.cin;
  const int k = k_override ? k_override : u.k;
  tf_pack_job j;
  j.src = c.P(u.w); j.dst = out; j.cout = cout; j.cin = cin; j.taps = k * k; j.transpose = transpose ? 1 : 0;
  if (!transpose) { j.rows_pad = (cout + 127) / 128 * 128; j.cols_pad = cols_pad_override ? cols_pad_override : cin; }
  else            { j.rows_pad = (cin + 127) / 128 * 128;  j.cols_pad = cols_pad_override ? cols_pad_override : cout; }
  c.jobs.push_back(j);
}

// forward operand [cout pad 128][taps][cin] and (training) data-gradient operand [cin pad 128][taps][cout] in one job
void pack2(Ctx& c, const ConvUnit& u, int cout, void* out, void* out_t, int cin_override = 0, int cols_pad_override = 0, int k_override = 0,
           const float* scale_t = nullptr) {
  const int cin = cin_override ? cin_override : u.cin;
  const int k = k_override ? k_override : u.k;
  tf_pack2_job j;
  j.src = c.P(u.w); j.dst = out; j.dst_t = out_t; j.cout = cout; j.cin = cin; j.taps = k * k;
  j.rows_pad = (cout + 127) / 128 * 128; j.cols_pad = cols_pad_override ? cols_pad_override : cin;
  j.rows_pad_t = (cin + 127) / 128 * 128; j.cols_pad_t = cout; j.scale_t = scale_t;
  c.jobs2.push_back(j);
}

// BN as a constant affine (evaluation and frozen BN): fold the running statistics into scale / shift, unless the arena already holds them
void bn_fold(Ctx& c, const ConvUnit& u, int C, BnBuf& b, float eps) {
  if (!c.skip_fold) c.chk(tf_bn_fold(c.P(u.gamma), c.P(u.beta), c.P(u.rmean), c.P(u.rvar), eps, C, b.scale, b.shift, c.stream));
}
// BN over batch statistics where no consumer finalizes in-kernel (the stem; every BN of the unfolded flow): finalize the `rows` partial
// rows (leading dimension ld) its producer left (+ running update)
void bn_finalize(Ctx& c, const ConvUnit& u, int C, BnBuf& b, const float* partial, int rows, int ld, float count, float eps, float mom) {
  c.chk(tf_bn_finalize(partial, rows, ld, C, count, c.P(u.gamma), c.P(u.beta), eps, mom, b.scale, b.shift, b.mean, b.invstd,
                       (float*)c.params[u.rmean], (float*)c.params[u.rvar], 1, c.stream));
}

// r3: the conv that produces a BN's statistics subtracts the BN's running mean before summing (sum (x - s), sum (x - s)^2) and records
// s in the extra row of the BN's statistic region, where the consumer's table picks it up (fused flow only; bn_fused.hip fwd_table).
// E[x^2] - mean^2 from fp32 sums loses (mean / std)^2 of the significant bits; around the running mean it loses ((mean - s) / std)^2.
void stat_shift(tf_conv_args& a, const Ctx& c, const ConvUnit& u, const BnBuf& b, bool fused) {
  if (!fused || !b.fst || u.rmean < 0) return;
  a.stat_shift = (const float*)c.params[u.rmean];
  a.stat_shift_out = b.fst + (size_t)TF_STAT_ROWS * 2 * b.C;
}

tf_bn_fwd_desc fwd_desc(const Ctx& c, const ConvUnit& u, const BnBuf& b) {
  tf_bn_fwd_desc d;
  d.stat = b.fst; d.gamma = c.P(u.gamma); d.beta = c.P(u.beta);
  d.scale = b.scale; d.shift = b.shift; d.mean = b.mean; d.invstd = b.invstd;
  d.running_mean = (float*)c.params[u.rmean]; d.running_var = (float*)c.params[u.rvar];
  d.stat_shift = b.fst ? b.fst + (size_t)TF_STAT_ROWS * 2 * b.C : nullptr;      // zero (memset) unless the producer recorded a shift
  return d;
}
tf_bn_bwd_desc bwd_desc(const Ctx& c, const ConvUnit& u, const BnBuf& b, const float* stat, int nk, int kidx) {
  tf_bn_bwd_desc d;
  d.stat = stat; d.gamma = c.P(u.gamma); d.mean = b.mean; d.invstd = b.invstd; d.dgamma = c.G(u.gamma); d.dbeta = c.G(u.beta);
  d.nk = nk; d.kidx = kidx;
  return d;
}

}  // namespace

extern "C" int tf_detnet_trunk_num_params(const int* blocks) {
  const Arch* a = find_arch(blocks);
  return a ? (int)a->names.size() : TF_ERR_UNSUPPORTED;
}
extern "C" const char* tf_detnet_trunk_param_name(const int* blocks, int i) {
  const Arch* a = find_arch(blocks);
  return (a && i >= 0 && i < (int)a->names.size()) ? a->names[i].c_str() : nullptr;
}
extern "C" int64_t tf_detnet_trunk_param_numel(const int* blocks, int i, int nout) {
  const Arch* ap = find_arch(blocks);
  if (!ap) return TF_ERR_UNSUPPORTED;
  const Arch& a = *ap;
  auto unit = [&](const ConvUnit& u, int cout) -> int64_t {
    if (i == u.w) return (int64_t)cout * u.cin * u.k * u.k;
    if (i == u.gamma || i == u.beta || i == u.rmean || i == u.rvar || i == u.bias) return cout;
    return -1;
  };
  int64_t r;
  if ((r = unit(a.stem, 64)) >= 0) return r;
  for (const Block& B : a.blocks) {
    if ((r = unit(B.c1, B.planes)) >= 0) return r;
    if ((r = unit(B.c2, B.planes)) >= 0) return r;
    if ((r = unit(B.c3, B.planes * 4)) >= 0) return r;
    if (B.has_ds && (r = unit(B.ds, B.planes * 4)) >= 0) return r;
  }
  if ((r = unit(a.head3, nout)) >= 0) return r;
  if ((r = unit(a.head4, nout)) >= 0) return r;
  if (i == a.upsample_w) return (int64_t)nout * nout * 16;
  return -1;
}
extern "C" int tf_detnet_num_params(void) { return tf_detnet_trunk_num_params(nullptr); }
extern "C" const char* tf_detnet_param_name(int i) { return tf_detnet_trunk_param_name(nullptr, i); }
extern "C" int64_t tf_detnet_param_numel(int i, int nout) { return tf_detnet_trunk_param_numel(nullptr, i, nout); }

extern "C" int tf_detnet_out_shape(int H, int W, int* H3, int* W3) {
  if (H3) *H3 = down2(down2(down2(H)));
  if (W3) *W3 = down2(down2(down2(W)));
  return TF_OK;
}

extern "C" size_t tf_detnet_trunk_workspace_bytes(const int* blocks, int dtype, int N, int H, int W, int nout, int training) {
  const Arch* A = find_arch(blocks);
  if (!A) return 0;
  Plan P; Arena ar(nullptr, 0);
  build_plan(*A, P, ar, dtype, N, H, W, nout, training);
  return P.total + 4096;
}
extern "C" size_t tf_detnet_workspace_bytes(int dtype, int N, int H, int W, int nout, int training) {
  return tf_detnet_trunk_workspace_bytes(nullptr, dtype, N, H, W, nout, training);
}

extern "C" size_t tf_detnet_trunk_param_region_bytes(const int* blocks, int dtype, int nout, int training) {
  const Arch* A = find_arch(blocks);
  if (!A) return 0;
  Plan P; Arena ar(nullptr, 0);
  build_plan(*A, P, ar, dtype, 1, 32, 32, nout, training);
  return P.param_bytes;
}
extern "C" size_t tf_detnet_param_region_bytes(int dtype, int nout, int training) { return tf_detnet_trunk_param_region_bytes(nullptr, dtype, nout, training); }

// The executor's own state lives in an explicit CONTEXT (tf_detnet_ctx): the second stream of the device it was created on (weight
// gradients of the backward pass; the packing of the layer-3 weights beside the start of the forward pass), the pool of fork / join
// events, and -- per backward call -- the caller's gradient-ready hooks (tf_detnet_hooks).  The entry points without a context
// (tf_detnet_forward / tf_detnet_backward / tf_detnet_set_*) remain as wrappers over ONE default context per device and thread-unsafe
// process-wide hooks, for callers that drive one model from one thread.
// The second stream is created at the DEFAULT priority: at the lowest one the kernels of BOTH queues stretch ~1.6x as soon as the process
// has a few more busy queues -- RCCL with its collectives overlapping the backward pass, i.e. the data-parallel path
// (profiles/r03_stream_priority.txt).
struct tf_detnet_ctx {
  int device = -1;
  hipStream_t side = nullptr;
  hipEvent_t pack_fork = nullptr, pack_join = nullptr;
  std::vector<hipEvent_t> events;
};
namespace {
// the stream and the events are created lazily, on the device the context belongs to (the caller has made it current: the binding wraps
// every call in torch.cuda.device(x.device))
hipStream_t ctx_side(tf_detnet_ctx* x) {
  if (x && !x->side && hipStreamCreateWithFlags(&x->side, hipStreamNonBlocking) != hipSuccess) x->side = nullptr;
  return x ? x->side : nullptr;
}
tf_detnet_ctx* default_ctx() {            // one per device: what the context-free entry points use
  static tf_detnet_ctx* per_dev[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  if (!per_dev[dev]) { per_dev[dev] = new tf_detnet_ctx; per_dev[dev]->device = dev; }
  return per_dev[dev];
}
}  // namespace
extern "C" int tf_detnet_ctx_create(tf_detnet_ctx** out) {
  if (!out) return TF_ERR_ARG;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return TF_ERR_LAUNCH;
  tf_detnet_ctx* x = new tf_detnet_ctx; x->device = dev;
  *out = x;
  return TF_OK;
}
extern "C" int tf_detnet_ctx_destroy(tf_detnet_ctx* x) {
  if (!x) return TF_OK;
  if (x->side) (void)hipStreamSynchronize(x->side);
  for (hipEvent_t e : x->events) (void)hipEventDestroy(e);
  if (x->pack_fork) (void)hipEventDestroy(x->pack_fork);
  if (x->pack_join) (void)hipEventDestroy(x->pack_join);
  if (x->side) (void)hipStreamDestroy(x->side);
  delete x;
  return TF_OK;
}
// legacy process-wide switches (tf_detnet_set_dual_stream / _grad_events / _grad_callback): hooks of the context-free entry points
static bool g_force_single = false;      // tf_detnet_set_dual_stream(0): everything on the caller's stream

extern "C" int tf_detnet_trunk_forward_ctx(const int* blocks, tf_detnet_ctx* xctx, int single_stream, int dtype, int training, const float* x, int N,
                                           int H, int W, int nout, void* const* params, float eps, float mom, float* out, void* ws, size_t ws_bytes,
                                           int flags, void* stream_) {
  const Arch* Ap = find_arch(blocks);
  if (!Ap) return TF_ERR_UNSUPPORTED;
  if (!xctx) xctx = default_ctx();
  if (!x || !params || !out || !ws || nout <= 0 || nout > kHeadLd) return TF_ERR_ARG;
  if (dtype != TF_BF16 && dtype != TF_F32 && dtype != TF_F16) return TF_ERR_UNSUPPORTED;
  if (dtype == TF_F16 && training) return TF_ERR_UNSUPPORTED;       // fp16 operands: the inference graph only (BASELINE.json configs[4])
  const Arch& A = *Ap;
  Plan P; Arena ar(ws, ws_bytes);
  build_plan(A, P, ar, dtype, N, H, W, nout, training);
  if (!ar.ok) return TF_ERR_WORKSPACE;
  Ctx c{dtype, (hipStream_t)stream_, params, nullptr, TF_OK};
  tf_conv_args a;
  const bool tr = training != 0 && training != kFrozen;      // the batch-statistics graph
  const bool fz = training == kFrozen;     // frozen BN: the evaluation graph's launches + what the backward needs
  const bool step = tr || fz;              // a training step: the weights are re-packed, the transposed operands too
  // eval only: the packed weights, folded BN affines and head vectors at the front of `ws` are already those of `params`
  const bool ready = !step && (flags & TF_DETNET_WEIGHTS_READY);

  c.skip_fold = ready;
  // statistics folded into <= TF_STAT_ROWS rows: the elementwise consumers finalize them in-kernel (bn_fused.hip);
  // unfolded (tf_set_stat_rows(0), bit-reproducible sums): separate finalize kernels on the shared partial buffer
  const int srows = tf_get_stat_rows();
  const bool fused = tr && srows <= TF_STAT_ROWS;
  // statistic rows start at zero: the per-BN regions and, right behind them in the arena, the head of the shared partial buffer -- ONE memset
  if (tr && hipMemsetAsync(P.stat_fwd, 0, (size_t)((char*)P.partial - (char*)P.stat_fwd) + (size_t)TF_STAT_ROWS * 3 * 1024 * 4, c.stream) != hipSuccess) c.chk(TF_ERR_LAUNCH);
  // ---- stem: conv1 (direct, or im2col + GEMM) (+BN+ReLU) + maxpool
  const int M1 = N * P.H1 * P.W1;
  // r3: the weights of layer 3 and of the heads (62 % of the bytes) are packed on the context's second stream (idle during the forward pass:
  // no further hardware queue), forked at the top of the step and joined in front of the first layer-3 bottleneck: beside the stem and
  // layers 1-2, whose launches are latency-bound at bs = 12, instead of in front of them.  TINYFACES_SINGLE_STREAM=1 or `single_stream`:
  // everything inline.
  hipStream_t pack_stream = nullptr;
  if (step && !ready && !tf::tuning().single_stream && !single_stream && xctx) {
    pack_stream = ctx_side(xctx);
    if (pack_stream && !xctx->pack_fork && (hipEventCreateWithFlags(&xctx->pack_fork, hipEventDisableTiming) != hipSuccess ||
                                            hipEventCreateWithFlags(&xctx->pack_join, hipEventDisableTiming) != hipSuccess)) pack_stream = nullptr;
  }
  const bool pack_side = pack_stream != nullptr;
  bool pack_joined = false;
  const bool stem_direct = stem_direct_mode(dtype, tr, fused);
  if (fz) {
    // frozen BN: every fold first -- the scales of bn3 / the downsample BN ride in the transposed operands packed below (possibly on the
    // second stream), and the backward pass reads all of them.  Same kernel, same values as the evaluation graph's folds.
    bn_fold(c, A.stem, 64, P.bn_stem, eps);
    for (size_t i = 0; i < A.blocks.size(); ++i) {
      const Block& B = A.blocks[i];
      Plan::Blk& b = P.blk[i];
      bn_fold(c, B.c1, B.planes, b.b1, eps); bn_fold(c, B.c2, B.planes, b.b2, eps); bn_fold(c, B.c3, B.planes * 4, b.b3, eps);
      if (B.has_ds) bn_fold(c, B.ds, B.planes * 4, b.bd, eps);
    }
    c.skip_fold = true;
    hipLaunchKernelGGL(fill_const_kernel, dim3((2 * kConstC + 255) / 256), dim3(256), 0, c.stream, P.c_one, P.c_zero, kConstC);
  }
  if (pack_side) {                         // everything enqueued so far (the previous step's SGD: the masters) precedes the packing
    if (hipEventRecord(xctx->pack_fork, c.stream) != hipSuccess || hipStreamWaitEvent(pack_stream, xctx->pack_fork, 0) != hipSuccess) c.chk(TF_ERR_LAUNCH);
  }
  if (!stem_direct) c.chk(tf_stem_im2col(x, N, H, W, dtype, P.col, kStemK, c.stream));
  // ---- every weight of the pass re-packed from the fp32 master copy in two launches
  if (!ready) {
  // every operand of the pass (and, in training, of the backward pass) from ONE read of the fp32 masters
  pack2(c, A.stem, 64, P.wstem, nullptr, 147, kStemK, 1);     // conv1.weight flattened OIHW == im2col k order
  for (size_t i = 0; i < A.blocks.size(); ++i) {
    const Block& B = A.blocks[i];
    Plan::Blk& b = P.blk[i];
    if (pack_side && (int)i == A.layer_end[1] + 1) c.flush_packs();       // stem + layers 1-2 are needed first: inline, behind the im2col
    pack2(c, B.c1, B.planes, b.w1, b.w1t); pack2(c, B.c2, B.planes, b.w2, b.w2t);
    pack2(c, B.c3, B.planes * 4, b.w3, b.w3t, 0, 0, 0, fz ? b.b3.scale : nullptr);       // frozen BN: (W3 diag(s3))^T
    if (B.has_ds) pack2(c, B.ds, B.planes * 4, b.wd, b.wdt, 0, 0, 0, fz ? b.bd.scale : nullptr);
  }
  {
    tf_pack2_job j;
    j.src = c.P(A.head3.w); j.dst = P.w_h3; j.dst_t = P.w_h3t; j.cout = nout; j.cin = 512; j.taps = 1;
    j.rows_pad = kHeadLd; j.cols_pad = 512; j.rows_pad_t = 512; j.cols_pad_t = kHeadLd; j.scale_t = nullptr;
    c.jobs2.push_back(j);
    j.src = c.P(A.head4.w); j.dst = P.w_h4; j.dst_t = P.w_h4t; j.cin = 1024; j.cols_pad = 1024; j.rows_pad_t = 1024;
    c.jobs2.push_back(j);
  }
  c.flush_packs(pack_stream);
  if (pack_side && hipEventRecord(xctx->pack_join, pack_stream) != hipSuccess) c.chk(TF_ERR_LAUNCH);
  }
  if (stem_direct) {
    if (tr) {
      int rows = 0;
      c.chk(tf_stem_conv(dtype, x, N, H, W, P.wstem, kStemK, P.cstem, TF_EPI_STATS, nullptr, nullptr, P.partial, &rows, c.stream));
      bn_finalize(c, A.stem, 64, P.bn_stem, P.partial, rows, 64, (float)M1, eps, mom);
    } else {
      bn_fold(c, A.stem, 64, P.bn_stem, eps);
      c.chk(tf_stem_conv(dtype, x, N, H, W, P.wstem, kStemK, P.cstem, TF_EPI_AFFINE | TF_EPI_RELU, P.bn_stem.scale, P.bn_stem.shift, nullptr, nullptr,
                         c.stream));
    }
  } else {
    conv_fill(a, dtype, 0, 1, 1, M1, kStemK, 1, M1, 64, 1, 1, 0, 64, P.col, P.wstem, P.cstem);
    a.alg_k = 147;                                  // 7 x 7 x 3 taps*channels, zero-padded to kStemK for the 64-deep K stages
    if (tr) { a.epi = TF_EPI_STATS; a.stat_out = P.partial; }
    else {
      bn_fold(c, A.stem, 64, P.bn_stem, eps);
      a.epi = TF_EPI_AFFINE | TF_EPI_RELU; a.epi_scale = P.bn_stem.scale; a.epi_shift = P.bn_stem.shift;
    }
    c.chk(tf_conv2d(&a, c.stream));
    if (tr) bn_finalize(c, A.stem, 64, P.bn_stem, P.partial, tf_conv_mtiles(&a), a.ldy, (float)M1, eps, mom);
  }
  c.chk(tf_maxpool_fwd(dtype, P.cstem, N, P.H1, P.W1, 64, tr ? P.bn_stem.scale : nullptr, tr ? P.bn_stem.shift : nullptr, P.pool,
                       step ? P.pool_idx : nullptr, c.stream));

  // ---- bottlenecks
  const void* yin = P.pool;
  for (size_t i = 0; i < A.blocks.size(); ++i) {
    const Block& B = A.blocks[i];
    Plan::Blk& b = P.blk[i];
    const int pl = B.planes, c4 = pl * 4;
    const int Min = N * b.Hin * b.Win, Mout = N * b.Hout * b.Wout;
    if (pack_side && (int)i == A.layer_end[1] + 1) { pack_joined = true; if (hipStreamWaitEvent(c.stream, xctx->pack_join, 0) != hipSuccess) c.chk(TF_ERR_LAUNCH); }
    // conv1 1x1
    conv_fill(a, dtype, 0, N, b.Hin, b.Win, B.cin, b.Hin, b.Win, pl, 1, 1, 0, pl, yin, b.w1, b.c1);
    if (tr) { a.epi = TF_EPI_STATS; a.stat_out = fused ? b.b1.fst : P.partial; stat_shift(a, c, B.c1, b.b1, fused); }
    else { bn_fold(c, B.c1, pl, b.b1, eps); a.epi = TF_EPI_AFFINE | TF_EPI_RELU; a.epi_scale = b.b1.scale; a.epi_shift = b.b1.shift; }
    c.chk(tf_conv2d(&a, c.stream));
    // a1 = relu(bn1(c1)), materialised on purpose: every consumer (conv2, its weight gradient) uses the LDS-DMA pipeline
    if (fused) {
      const tf_bn_fwd_desc d = fwd_desc(c, B.c1, b.b1);
      c.chk(tf_bn_relu_fused(dtype, b.c1, &d, srows, Min, pl, (float)Min, eps, mom, b.a1, c.stream));
    } else if (tr) {
      bn_finalize(c, B.c1, pl, b.b1, P.partial, tf_conv_mtiles(&a), a.ldy, (float)Min, eps, mom);
      c.chk(tf_bn_relu(dtype, b.c1, b.b1.scale, b.b1.shift, Min, pl, b.a1, c.stream));
    }
    // conv2 3x3 (stride here)
    conv_fill(a, dtype, 0, N, b.Hin, b.Win, pl, b.Hout, b.Wout, pl, 3, B.stride, 1, pl, tr ? b.a1 : b.c1, b.w2, b.c2);
    if (tr) { a.epi = TF_EPI_STATS; a.stat_out = fused ? b.b2.fst : P.partial; stat_shift(a, c, B.c2, b.b2, fused); }
    else { bn_fold(c, B.c2, pl, b.b2, eps); a.epi = TF_EPI_AFFINE | TF_EPI_RELU; a.epi_scale = b.b2.scale; a.epi_shift = b.b2.shift; }
    c.chk(tf_conv2d(&a, c.stream));
    if (tr && !fused) bn_finalize(c, B.c2, pl, b.b2, P.partial, tf_conv_mtiles(&a), a.ldy, (float)Mout, eps, mom);
    // downsample 1x1 (stride)
    if (B.has_ds) {
      conv_fill(a, dtype, 0, N, b.Hin, b.Win, B.cin, b.Hout, b.Wout, c4, 1, B.stride, 0, c4, yin, b.wd, b.d);
      if (tr) { a.epi = TF_EPI_STATS; a.stat_out = fused ? b.bd.fst : P.partial; stat_shift(a, c, B.ds, b.bd, fused); }
      else { bn_fold(c, B.ds, c4, b.bd, eps); a.epi = TF_EPI_AFFINE; a.epi_scale = b.bd.scale; a.epi_shift = b.bd.shift; }
      c.chk(tf_conv2d(&a, c.stream));
      if (tr && !fused) bn_finalize(c, B.ds, c4, b.bd, P.partial, tf_conv_mtiles(&a), a.ldy, (float)Mout, eps, mom);
    }
    // a2 = relu(bn2(c2)): a launch of its own (folding it into conv3's LDS stage lost 1.3 % on the step: DESIGN_HISTORY.md)
    if (fused) {
      const tf_bn_fwd_desc d2 = fwd_desc(c, B.c2, b.b2);
      c.chk(tf_bn_relu_fused(dtype, b.c2, &d2, srows, Mout, pl, (float)Mout, eps, mom, b.a2, c.stream));
    } else if (tr) {
      c.chk(tf_bn_relu(dtype, b.c2, b.b2.scale, b.b2.shift, Mout, pl, b.a2, c.stream));
    }
    // conv3 1x1 (+ BN + residual + ReLU)
    conv_fill(a, dtype, 0, N, b.Hout, b.Wout, pl, b.Hout, b.Wout, c4, 1, 1, 0, c4, tr ? b.a2 : b.c2, b.w3, tr ? b.c3 : b.y);
    if (tr) { a.epi = TF_EPI_STATS; a.stat_out = fused ? b.b3.fst : P.partial; stat_shift(a, c, B.c3, b.b3, fused); }
    else {
      bn_fold(c, B.c3, c4, b.b3, eps);
      a.epi = TF_EPI_AFFINE | TF_EPI_RES | TF_EPI_RELU; a.epi_scale = b.b3.scale; a.epi_shift = b.b3.shift; a.aux = B.has_ds ? b.d : yin;
    }
    c.chk(tf_conv2d(&a, c.stream));
    if (fused) {
      const tf_bn_fwd_desc d3 = fwd_desc(c, B.c3, b.b3);
      tf_bn_fwd_desc dd; if (B.has_ds) dd = fwd_desc(c, B.ds, b.bd);
      c.chk(tf_bn_add_relu_fused(dtype, b.c3, &d3, B.has_ds ? b.d : yin, B.has_ds ? &dd : nullptr, srows, Mout, c4, (float)Mout, eps, mom, b.y,
                                 c.stream));
    } else if (tr) {
      bn_finalize(c, B.c3, c4, b.b3, P.partial, tf_conv_mtiles(&a), a.ldy, (float)Mout, eps, mom);
      c.chk(tf_bn_add_relu(dtype, b.c3, b.b3.scale, b.b3.shift, B.has_ds ? b.d : yin, B.has_ds ? b.bd.scale : nullptr,
                           B.has_ds ? b.bd.shift : nullptr, Mout, c4, b.y, c.stream));
    }
    yin = b.y;
  }

  // ---- heads + bilinear upsample + crop + add
  const void* res3 = P.blk[A.layer_end[1]].y;
  const void* res4 = P.blk[A.layer_end[2]].y;
  if (!ready)
    hipLaunchKernelGGL(head_vectors_kernel, dim3((nout * 16 + 255) / 256), dim3(256), 0, c.stream, c.P(A.head3.bias), c.P(A.head4.bias),
                       c.P(A.upsample_w), nout, P.hbias3, P.hbias4, P.ones, P.wup_diag);
  conv_fill(a, dtype, 0, N, P.H3, P.W3, 512, P.H3, P.W3, kHeadLd, 1, 1, 0, kHeadLd, res3, P.w_h3, P.s3);
  a.epi = TF_EPI_AFFINE; a.epi_scale = P.ones; a.epi_shift = P.hbias3; a.alg_n = nout;
  c.chk(tf_conv2d(&a, c.stream));
  conv_fill(a, dtype, 0, N, P.H4, P.W4, 1024, P.H4, P.W4, kHeadLd, 1, 1, 0, kHeadLd, res4, P.w_h4, P.s4);
  a.epi = TF_EPI_AFFINE; a.epi_scale = P.ones; a.epi_shift = P.hbias4; a.alg_n = nout;
  c.chk(tf_conv2d(&a, c.stream));
  c.chk(tf_upsample_add_crop(dtype, P.s3, P.s4, P.wup_diag, N, nout, kHeadLd, P.H3, P.W3, P.H4, P.W4, out, c.stream));
  if (pack_side && !pack_joined) (void)hipStreamWaitEvent(c.stream, xctx->pack_join, 0);      // (never leave the caller's stream un-joined)
  if (hipGetLastError() != hipSuccess && c.rc == TF_OK) c.rc = TF_ERR_LAUNCH;
  return c.rc;
}
extern "C" int tf_detnet_forward_ctx(tf_detnet_ctx* xctx, int single_stream, int dtype, int training, const float* x, int N, int H, int W, int nout,
                                     void* const* params, float eps, float mom, float* out, void* ws, size_t ws_bytes, int flags, void* stream_) {
  return tf_detnet_trunk_forward_ctx(nullptr, xctx, single_stream, dtype, training, x, N, H, W, nout, params, eps, mom, out, ws, ws_bytes, flags, stream_);
}
extern "C" int tf_detnet_forward(int dtype, int training, const float* x, int N, int H, int W, int nout, void* const* params, float eps,
                                 float mom, float* out, void* ws, size_t ws_bytes, int flags, void* stream_) {
  return tf_detnet_forward_ctx(nullptr, g_force_single ? 1 : 0, dtype, training, x, N, H, W, nout, params, eps, mom, out, ws, ws_bytes, flags, stream_);
}

// ------------------------------------------------------------------------------------------------
// backward
namespace {

// g_x for a BN whose output-gradient sums are in `partial`: finalize (dgamma, dbeta, coefficients)
void bn_backward_coefs(Ctx& c, const ConvUnit& u, int C, BnBuf& b, const float* partial, int nblk, int nk, int kidx, int ld, float count,
                       int clear = 1) {
  c.chk(tf_bn_bwd_finalize(partial, nblk, nk, kidx, ld, C, count, c.P(u.gamma), b.mean, b.invstd, c.G(u.gamma), c.G(u.beta), b.cA, b.cB,
                           b.cD, clear, c.stream));
}

tf_wgrad_args wgrad_args(const Ctx& c, const ConvUnit& u, int cout, int N, int H, int W, int OH, int OW, const void* x, int ldx, const void* dy,
                         int lddy, int cin_override = 0, int k_override = 0, int dw_ld = 0) {
  tf_wgrad_args w;
  memset(&w, 0, sizeof(w));
  const int cin = cin_override ? cin_override : u.cin, k = k_override ? k_override : u.k;
  w.dtype = c.dtype; w.N = N; w.H = H; w.W = W; w.Cin = cin; w.OH = OH; w.OW = OW; w.Cout = cout; w.KH = k; w.KW = k;
  w.stride = u.stride; w.pad = u.pad; w.ldx = ldx; w.lddy = lddy; w.x = x; w.dy = dy; w.dw_oihw = c.G(u.w);
  w.dw_ld = dw_ld ? dw_ld : cin * k * k;
  return w;
}

// one weight gradient on the weight-gradient stream.  row_scale (frozen BN, pointwise convs): dW[co] *= the folded scale of the BN behind the conv
void wgrad(Ctx& c, const ConvUnit& u, int cout, int N, int H, int W, int OH, int OW, const void* x, int ldx, const void* dy, int lddy,
           const float* row_scale = nullptr, int cin_override = 0, int k_override = 0, int dw_ld = 0, float* packed_scratch = nullptr,
           size_t scratch_floats = 0) {
  // timing-ablation knob (RESULTS INVALID): the step without any weight gradient = what the data-gradient chain costs when it owns the GPU
  const bool skip = tf::tuning().dbg_skip_wgrad;
  if (skip) return;
  const int cin = cin_override ? cin_override : u.cin, k = k_override ? k_override : u.k;
  tf_wgrad_args w = wgrad_args(c, u, cout, N, H, W, OH, OW, x, ldx, dy, lddy, cin_override, k_override, dw_ld);
  w.row_scale = row_scale;
  if (c.det) {
    // slab form: the slices of every split-K kernel go through the slab and are summed in a fixed order straight into the OIHW gradient
    // (the stride-2 3x3 convs too: no packed scratch, no transposing copy); a slab too small for the preferred plan means fewer slices
    if (!c.grads_zeroed && hipMemsetAsync(w.dw_oihw, 0, (size_t)cout * w.dw_ld * 4, c.wstream()) != hipSuccess) c.chk(TF_ERR_LAUNCH);
    w.partial_ws = c.det_slab; w.partial_ws_bytes = c.det_slab_bytes;
    c.chk(tf_conv2d_wgrad_det(&w, c.wstream()));
    return;
  }
  if (k > 1 && packed_scratch && c.grads_zeroed) {
    // 3x3 / stride 1: the all-taps kernel sums its split-K slices through the scratch straight into the (already zeroed) OIHW
    // gradient: no memset, no atomics, no transposing copy
    w.partial_ws = packed_scratch; w.partial_ws_bytes = scratch_floats * 4;
    if (tf_wgrad_workspace_bytes(&w) != 0 && tf_wgrad_workspace_bytes(&w) <= w.partial_ws_bytes) { c.chk(tf_conv2d_wgrad(&w, c.wstream())); return; }
    w.partial_ws = nullptr; w.partial_ws_bytes = 0;
  }
  if (k > 1 && packed_scratch) {          // 3x3 (stride 2): coalesced atomics into [Cout][tap][Cin], then one transposing copy to OIHW
    float* oihw = w.dw_oihw;
    w.dw_oihw = packed_scratch; w.packed = 1;
    if (hipMemsetAsync(packed_scratch, 0, (size_t)cout * w.dw_ld * 4, c.wstream()) != hipSuccess) c.chk(TF_ERR_LAUNCH);   // scratch: always
    c.chk(tf_conv2d_wgrad(&w, c.wstream()));
    c.chk(tf_unpack_dw(packed_scratch, cout, cin, k * k, oihw, c.wstream()));
    return;
  }
  if (!c.grads_zeroed && hipMemsetAsync(w.dw_oihw, 0, (size_t)cout * w.dw_ld * 4, c.wstream()) != hipSuccess) c.chk(TF_ERR_LAUNCH);
  c.chk(tf_conv2d_wgrad(&w, c.wstream()));
}

}  // namespace

// gradient-ready hooks (data-parallel overlap): after the weight gradients of bottleneck `block` (backward order: the LAST block of a
// bucket) are enqueued, the caller's event is recorded on the stream that carries them and / or the caller's function is called with that
// stream, so that the bucket's all-reduce starts while the rest of the backward pass runs.  block -1 = the very end (stem done).
// r4: the hooks are an ARGUMENT of the backward call (tf_detnet_hooks), not a process-wide registration.
static std::vector<std::pair<int, hipEvent_t>> g_grad_events;      // legacy registration (tf_detnet_set_grad_events), used by tf_detnet_backward only
extern "C" int tf_detnet_set_grad_events(const int* blocks, void* const* events, int n) {
  g_grad_events.clear();
  if (n < 0 || (n > 0 && (!blocks || !events))) return TF_ERR_ARG;       // (events[k] itself may be NULL)
  for (int k = 0; k < n; ++k) g_grad_events.emplace_back(blocks[k], (hipEvent_t)events[k]);      // a NULL event: the callback only
  return TF_OK;
}
static tf_grad_ready_fn g_grad_cb = nullptr;
static void* g_grad_cb_user = nullptr;
extern "C" int tf_detnet_set_grad_callback(tf_grad_ready_fn fn, void* user) { g_grad_cb = fn; g_grad_cb_user = user; return TF_OK; }
static void record_grad_events(const tf_detnet_hooks* h, int block, hipStream_t s, int& rc) {
  if (!h) return;
  bool registered = false;
  for (int k = 0; k < h->n; ++k)
    if (h->blocks[k] == block) {
      registered = true;
      hipEvent_t e = h->events ? (hipEvent_t)h->events[k] : nullptr;
      if (e && hipEventRecord(e, s) != hipSuccess && rc == TF_OK) rc = TF_ERR_LAUNCH;
    }
  if (registered && h->fn) h->fn(block, (void*)s, h->user);
}
// 1 = weight gradients on a second stream (default), 0 = everything on the caller's stream (A/B + race tests)
extern "C" int tf_detnet_set_dual_stream(int on) { g_force_single = !on; return TF_OK; }

// ---- the stages the two backward passes (batch statistics below, frozen BN behind it) share: everything that is not BN mathematics
namespace {

// entry: the trunk, the plan of the forward that ran (`training` = 1 or TF_DETNET_FROZEN_BN) and the launch context with its second stream
int open_backward(const int* blocks, tf_detnet_ctx* xctx, const tf_detnet_hooks* hooks, int dtype, const float* x, int N, int H, int W, int nout,
                  void* const* params, void* const* grads, const float* gout, void* ws, size_t ws_bytes, void* stream_, int training,
                  const Arch*& A, Plan& P, Ctx& c) {
  A = find_arch(blocks);
  if (!A) return TF_ERR_UNSUPPORTED;
  if (!x || !params || !grads || !gout || !ws) return TF_ERR_ARG;
  if (hooks && (hooks->n < 0 || (hooks->n > 0 && !hooks->blocks))) return TF_ERR_ARG;
  if (!xctx) xctx = default_ctx();
  if (dtype != TF_BF16 && dtype != TF_F32) return TF_ERR_UNSUPPORTED;
  Arena ar(ws, ws_bytes);
  build_plan(*A, P, ar, dtype, N, H, W, nout, training);
  if (!ar.ok) return TF_ERR_WORKSPACE;
  c = Ctx{dtype, (hipStream_t)stream_, params, grads, TF_OK};   // (grads_zeroed / jobs default-initialised)
  if (!tf::tuning().single_stream && !(hooks && hooks->single_stream) && xctx) { c.side = ctx_side(xctx); c.events = &xctx->events; }
  c.det = tf_get_deterministic() != 0; c.det_slab = P.dwp; c.det_slab_bytes = P.dwp_floats * sizeof(float);
  return TF_OK;
}

// exit: the caller's stream sees every weight gradient, then the hook of the very end.  first_block > 0 (a backward cut at a stage boundary,
// tf_detnet_trunk_backward_frozen_from_ctx): the hooks of the blocks below the cut, whose ranges hold nothing but the memset's zeros, fire here
// too, in the registered order, each block once, ahead of the -1 hook.
int close_backward(Ctx& c, const tf_detnet_hooks* hooks, int first_block = -1) {
  // (r5, measured and removed: returning WITHOUT joining the last kernel, conv1's weight gradient, and running the SGD update of every other
  //  parameter beside it -- 1282.2 / 1284.0 against 1282.1 / 1281.2 img/s joined: both are HBM-bound, side by side they take as long as back
  //  to back)
  c.wait_on_main(c.mark_side());
  for (int k = 0; hooks && first_block > 0 && k < hooks->n; ++k) {
    const int blk = hooks->blocks[k];
    bool seen = false;
    for (int j = 0; j < k && !seen; ++j) seen = hooks->blocks[j] == blk;
    if (blk >= 0 && blk < first_block && !seen) record_grad_events(hooks, blk, c.stream, c.rc);
  }
  record_grad_events(hooks, -1, c.stream, c.rc);
  if (hipGetLastError() != hipSuccess && c.rc == TF_OK) c.rc = TF_ERR_LAUNCH;
  return c.rc;
}

// is parameter q a trained tensor (conv weight, BN gamma / beta) of the identity bottleneck B?
bool block_owns(const Block& B, int q) {
  for (const ConvUnit* u : {&B.c1, &B.c2, &B.c3})
    if (q == u->w || q == u->gamma || q == u->beta) return true;
  return false;
}

// One memset for every weight gradient (atomics accumulate into them) ...
// r4: ... except where nothing accumulates: the grouped weight gradients OVERWRITE theirs, and the BatchNorm gradients in between are
// published with plain stores (bn_fused.hip) -- the 22 identity bottlenecks of layer 3 are 98 of the 111 MB of the flat gradient.
// With the table in executor order (DetectionModel.flatten_parameters) they are ONE range: [layer3.1.conv1.weight, score_res3.weight),
// skipped when every trained tensor of these blocks lies inside it and nothing else does (TINYFACES_GRAD_MEMSET_FULL=1: never).
// zero_bn_slices (frozen BN): the BN segments inside that range have NO writer: zero_ranges_kernel clears them, so that the optimizer, the
// all-reduce buckets and a checkpoint never see what an earlier (batch-statistics) step left there.
void zero_flat_gradient(Ctx& c, const Arch& A, void* grad_flat, size_t grad_flat_bytes, bool group_on, bool zero_bn_slices) {
  if (!grad_flat || !grad_flat_bytes) return;
  const int first_id = A.layer_end[1] + 2, last_id = A.layer_end[2];           // the identity bottlenecks of layer 3 (ResNet-101: blocks 8 .. 29)
  char* lo = group_on ? (char*)c.G(A.blocks[first_id].c1.w) : nullptr;
  char* hi = group_on ? (char*)c.G(A.head3.w) : nullptr;
  char* g0 = (char*)grad_flat; char* g1 = g0 + grad_flat_bytes;
  bool split = lo && hi && lo >= g0 && hi <= g1 && lo < hi;
  std::vector<std::pair<float*, int>> zr;           // the BN slices inside the range, adjacent ones (gamma | beta of one BN) merged
  for (int i = first_id; split && i <= last_id; ++i)                // every trained tensor of these blocks must lie inside the range
    for (const ConvUnit* u : {&A.blocks[i].c1, &A.blocks[i].c2, &A.blocks[i].c3}) {
      char* w = (char*)c.G(u->w);
      split = split && w >= lo && w < hi;
      for (int q : {u->gamma, u->beta}) {
        char* t = (char*)c.G(q);
        if (!t && zero_bn_slices) continue;                 // (a table without BN gradient slots: nothing to zero)
        split = split && t >= lo && t + (size_t)u->cout * 4 <= hi;
        if (!zero_bn_slices) continue;
        if (!zr.empty() && zr.back().first + zr.back().second == (float*)t) zr.back().second += u->cout;
        else zr.emplace_back((float*)t, u->cout);
      }
    }
  for (int q = 0; split && q < (int)A.names.size(); ++q) {          // ... and nothing else may
    char* t = (char*)c.G(q);
    if (!t || t < lo || t >= hi) continue;
    bool mine = false;
    for (int i = first_id; i <= last_id && !mine; ++i) mine = block_owns(A.blocks[i], q);
    split = split && mine;
  }
  const bool split_off = tf::tuning().grad_memset_full;     // A/B + safety knob
  if (split && !split_off) {
    if (lo > g0 && hipMemsetAsync(g0, 0, (size_t)(lo - g0), c.stream) != hipSuccess) c.chk(TF_ERR_LAUNCH);
    if (g1 > hi && hipMemsetAsync(hi, 0, (size_t)(g1 - hi), c.stream) != hipSuccess) c.chk(TF_ERR_LAUNCH);
    // one launch per kZeroRanges ranges (ResNet-101: 66 ranges, ResNet-152: 105 -- one launch; the table travels as kernel arguments)
    for (size_t at = 0; at < zr.size(); at += kZeroRanges) {
      ZeroRanges tab;
      const int nz = (int)(zr.size() - at < (size_t)kZeroRanges ? zr.size() - at : (size_t)kZeroRanges);
      for (int q = 0; q < kZeroRanges; ++q) { tab.p[q] = q < nz ? zr[at + q].first : nullptr; tab.n[q] = q < nz ? zr[at + q].second : 0; }
      hipLaunchKernelGGL(zero_ranges_kernel, dim3(1, nz), dim3(256), 0, c.stream, tab);
    }
  } else if (hipMemsetAsync(grad_flat, 0, grad_flat_bytes, c.stream) != hipSuccess) c.chk(TF_ERR_LAUNCH);
  c.grads_zeroed = true;
}

// The heads: the gradients of the two score maps, their bias and weight gradients, and the data gradients into the trunk -- res3's into
// P.R3, the last block's output gradient into `gtop` with the epilogue `top` gives it (the one thing the two graphs do differently here).
// (the transposed weight operands w*t were packed by the training forward, together with the forward operands)
// want_top / want_r3 = false (a frozen-BN backward cut above layer 3 / above layer 2): that data gradient has no reader and is not launched.
template <class F>
void heads_backward(Ctx& c, const Arch& A, const Plan& P, const float* gout, void* grad_flat, size_t grad_flat_bytes, void* gtop, F&& top,
                    bool want_top = true, bool want_r3 = true) {
  const int dtype = P.dtype, N = P.N, nout = P.nout;
  const int M3 = N * P.H3 * P.W3, M4 = N * P.H4 * P.W4;
  c.chk(tf_upsample_add_crop_bwd(dtype, gout, P.wup_diag, N, nout, kHeadLd, P.H3, P.W3, P.H4, P.W4, P.g3, P.g4, c.stream));
  const int nb3 = tf_colstats_blocks(M3, kHeadLd, dtype), nb4 = tf_colstats_blocks(M4, kHeadLd, dtype);
  c.chk(tf_colstats(dtype, P.g3, nullptr, nullptr, nullptr, M3, kHeadLd, kHeadLd, P.partial_b, c.stream));
  c.chk(tf_reduce_partials(P.partial_b, nb3, 1, 0, kHeadLd, nout, c.G(A.head3.bias), 1, c.stream));
  c.chk(tf_colstats(dtype, P.g4, nullptr, nullptr, nullptr, M4, kHeadLd, kHeadLd, P.partial_b, c.stream));
  c.chk(tf_reduce_partials(P.partial_b, nb4, 1, 0, kHeadLd, nout, c.G(A.head4.bias), 1, c.stream));
  c.fork();
  wgrad(c, A.head3, nout, N, P.H3, P.W3, P.H3, P.W3, P.blk[A.layer_end[1]].y, 512, P.g3, kHeadLd);
  wgrad(c, A.head4, nout, N, P.H4, P.W4, P.H4, P.W4, P.blk[A.layer_end[2]].y, 1024, P.g4, kHeadLd);
  // score4_upsample.weight has lr 0 (model.py:84): its gradient is defined as zero here
  {
    char* u = (char*)c.G(A.upsample_w);
    const bool covered = c.grads_zeroed && u >= (char*)grad_flat && u + (size_t)nout * nout * 16 * 4 <= (char*)grad_flat + grad_flat_bytes;     // (the flat buffer's memset)
    if (u && !covered && hipMemsetAsync(u, 0, (size_t)nout * nout * 16 * 4, c.stream) != hipSuccess) c.chk(TF_ERR_LAUNCH);
  }
  tf_conv_args a;
  if (want_top) {
    conv_fill(a, dtype, 1, N, P.H4, P.W4, kHeadLd, P.H4, P.W4, 1024, 1, 1, 0, 1024, P.g4, P.w_h4t, gtop);
    a.alg_k = nout;
    top(a);
    c.chk(tf_conv2d(&a, c.stream));
  }
  if (want_r3) {
    conv_fill(a, dtype, 1, N, P.H3, P.W3, kHeadLd, P.H3, P.W3, 512, 1, 1, 0, 512, P.g3, P.w_h3t, P.R3);
    a.alg_k = nout;
    c.chk(tf_conv2d(&a, c.stream));
  }
}

// r4: GROUPED weight gradients of the identity bottlenecks of layer 3.  Their three gradients are not launched
// per block any more: the block's dY operands go to buffers of its own (Plan::Blk::gT1 / gT2 / gU1), the problems are queued, and when
// a group is complete -- behind the kernel that produces the last operand of its LAST (lowest) block -- ONE fork hands the second stream
// two launches (tf_conv2d_wgrad_group): the 2 x n pointwise problems (128 x 128 tiles, each reduced over all 12 288 pixels in-block) and
// the n 3x3 problems (all-taps kernel, splitk = 1).  No split-K, no atomics, no partial tiles, no reduce kernel, 3 forks instead of 22
// for these blocks; the gradient-ready events of the group's blocks fire behind the group.
struct WgradGroups {
  int first_id = 0, last_id = -1;                     // the identity bottlenecks of layer 3 (ResNet-101: blocks 8 .. 29); empty when grouping is off
  std::vector<int> group_close;                       // block index that closes each group (descending)
  std::vector<tf_wgrad_args> pend_pw, pend_c3;
  std::vector<int> pend_blocks;
  WgradGroups(const Arch& A, bool on) {
    if (!on) return;
    first_id = A.layer_end[1] + 2; last_id = A.layer_end[2];
    const int nid = last_id - first_id + 1, gs = kWgradGroup, ng = (nid + gs - 1) / gs;
    for (int g = 1; g <= ng; ++g) group_close.push_back(last_id + 1 - (int)(((long long)nid * g + ng - 1) / ng));      // balanced: 8 + 7 + 7 (ResNet-101)
  }
  bool grouped(int i) const { return i >= first_id && i <= last_id; }
  bool closes(int i) const { for (int gc : group_close) if (gc == i) return true; return false; }
  void push(int block, const tf_wgrad_args& w3, const tf_wgrad_args& w2, const tf_wgrad_args& w1) {
    pend_pw.push_back(w3); pend_pw.push_back(w1); pend_c3.push_back(w2); pend_blocks.push_back(block);
  }
  void flush(Ctx& c, const tf_detnet_hooks* hooks) {
    if (pend_blocks.empty()) return;
    const bool skip = tf::tuning().dbg_skip_wgrad;
    if (!skip) {
      // the 3x3 group first: 16 tiles per problem = half a machine for a group of eight; the pointwise launch behind it fills the CUs its
      // tail leaves (both are enqueued behind the same fork)
      // A refused group (e.g. a layer-3 width the all-taps plan does not take: inputs wider than ~2000 px) falls back to the per-problem
      // split-K kernels, which ACCUMULATE with fp32 atomics -- and the split memset skipped exactly these tensors, so on a persistent
      // flat gradient they would be added onto the previous step's (all-reduced) values: zero each one here, on the stream the
      // fallback launches run on (tests/test_gpu_model.py::test_refused_wgrad_group_falls_back_into_zeroed_gradients)
      auto fallback = [&](const std::vector<tf_wgrad_args>& v) {
        for (const tf_wgrad_args& w : v) {
          if (hipMemsetAsync(w.dw_oihw, 0, (size_t)w.Cout * w.dw_ld * 4, c.wstream()) != hipSuccess) c.chk(TF_ERR_LAUNCH);
          if (c.det) {
            tf_wgrad_args d = w;
            d.partial_ws = c.det_slab; d.partial_ws_bytes = c.det_slab_bytes;
            c.chk(tf_conv2d_wgrad_det(&d, c.wstream()));
          } else c.chk(tf_conv2d_wgrad(&w, c.wstream()));
        }
      };
      const bool force_refuse = tf::tuning().dbg_group_refuse;      // test knob: exercise the fallback at any size
      int rc = force_refuse ? TF_ERR_UNSUPPORTED : tf_conv2d_wgrad_group(pend_c3.data(), (int)pend_c3.size(), c.wstream());
      if (rc == TF_ERR_UNSUPPORTED) fallback(pend_c3);
      else c.chk(rc);
      // The pointwise group is ONE launch.  A group of eight bottlenecks is 256 tiles = one block on EVERY CU for ~150 us, and beside it the
      // chain's kernels crawl (profiles/r05_step_timeline.txt: the data gradient that normally takes 22 us takes 118-130 us while the group
      // runs); split into several launches that leave CUs to the chain, the step measured no faster (DESIGN_HISTORY.md section 7, row 46).
      rc = force_refuse ? TF_ERR_UNSUPPORTED : tf_conv2d_wgrad_group(pend_pw.data(), (int)pend_pw.size(), c.wstream());
      if (rc == TF_ERR_UNSUPPORTED) fallback(pend_pw);
      else c.chk(rc);
    }
    // a gradient-ready event of a grouped block promises "every gradient of the blocks >= it, and of the heads": all of them are on this stream
    for (int blk : pend_blocks) record_grad_events(hooks, blk, c.wstream(), c.rc);
    pend_pw.clear(); pend_c3.clear(); pend_blocks.clear();
  }
};

// The gradient w.r.t. a block's input -> dst:  W1^T g1 + the skip branch (+ `extra`: the head's gradient w.r.t. res3, where the input is
// res3).  gskip is the skip branch's operand: the identity residual, or dY of the downsample conv where the block has one.  hand_over
// decorates the launch(es) that complete dst -- the one place the two graphs differ (ReLU mask of the previous block, its BN3 sums, tile).
// r6: the stride-2 downsample gradient is nonzero on the even-even pixels of the block's input raster only.  Rounds 3-5 zeroed (or, with
// the res3 head gradient, copied) a raster of that size, scattered into it, and the hand-over conv read it back as its residual: a
// 96 MB fill + 49 MB copy by blit kernels at 2.6 TB/s and two more passes over those rasters.  Now the hand-over writes the raster first
// (residual = the head gradient where there is one) and the scattered gradient ACCUMULATES IN PLACE (tf_conv2d: aux == y), applying the
// same ReLU mask and adding its own share to the same BN-backward sums.  A caller whose hand-over does not mask (!inplace_ok):
// the old order, through P.T4.
template <class F>
void input_gradient(Ctx& c, const Plan& P, const Block& B, const Plan::Blk& b, const void* g1, const void* gskip, const void* extra, void* dst,
                    bool inplace_ok, F&& hand_over) {
  const int dtype = P.dtype, N = P.N, pl = B.planes, c4 = pl * 4;
  tf_conv_args a;
  if (!B.has_ds) {
    conv_fill(a, dtype, 1, N, b.Hin, b.Win, pl, b.Hin, b.Win, B.cin, 1, 1, 0, B.cin, g1, b.w1t, dst);
    a.epi = TF_EPI_RES; a.aux = gskip;
    hand_over(a);
    c.chk(tf_conv2d(&a, c.stream));
  } else if (inplace_ok && B.stride == 2) {
    conv_fill(a, dtype, 1, N, b.Hin, b.Win, pl, b.Hin, b.Win, B.cin, 1, 1, 0, B.cin, g1, b.w1t, dst);
    if (extra) { a.epi = TF_EPI_RES; a.aux = extra; }
    hand_over(a);
    c.chk(tf_conv2d(&a, c.stream));
    conv_fill(a, dtype, 1, N, b.Hout, b.Wout, c4, b.Hin, b.Win, B.cin, 1, B.stride, 0, B.cin, gskip, b.wdt, dst);
    a.epi = TF_EPI_RES; a.aux = dst;
    hand_over(a);
    c.chk(tf_conv2d(&a, c.stream));
  } else {
    conv_fill(a, dtype, 1, N, b.Hout, b.Wout, c4, b.Hin, b.Win, B.cin, 1, B.stride, 0, B.cin, gskip, b.wdt, P.T4);
    if (extra) { a.epi = TF_EPI_RES; a.aux = extra; }
    c.chk(tf_conv2d(&a, c.stream));
    conv_fill(a, dtype, 1, N, b.Hin, b.Win, pl, b.Hin, b.Win, B.cin, 1, 1, 0, B.cin, g1, b.w1t, dst);
    a.epi = TF_EPI_RES; a.aux = P.T4;
    hand_over(a);
    c.chk(tf_conv2d(&a, c.stream));
  }
}

}  // namespace

// backward through the BATCH-STATISTICS graph (forward with training = 1)
extern "C" int tf_detnet_trunk_backward_ctx(const int* blocks, tf_detnet_ctx* xctx, const tf_detnet_hooks* hooks, int dtype, const float* x, int N,
                                            int H, int W, int nout, void* const* params, void* const* grads, const float* gout, void* grad_flat,
                                            size_t grad_flat_bytes, void* ws, size_t ws_bytes, void* stream_) {
  const Arch* Ap; Plan P; Ctx c{};
  const int rc0 = open_backward(blocks, xctx, hooks, dtype, x, N, H, W, nout, params, grads, gout, ws, ws_bytes, stream_, 1, Ap, P, c);
  if (rc0 != TF_OK) return rc0;
  const Arch& A = *Ap;
  tf_conv_args a;

  const int srows = tf_get_stat_rows();
  const bool fused = srows <= TF_STAT_ROWS;   // see tf_detnet_forward
  // statistic rows start at zero: the per-BN backward regions + the head of this pass's partial buffer right behind them, ONE memset
  if (hipMemsetAsync(P.stat_bwd, 0, (size_t)((char*)P.partial_b - (char*)P.stat_bwd) + (size_t)TF_STAT_ROWS * 3 * 1024 * 4, c.stream) != hipSuccess) c.chk(TF_ERR_LAUNCH);
  // the forward pass took conv1 straight from the image; its weight gradient does too (tf_stem_wgrad)
  const bool stem_direct = stem_direct_mode(dtype, true, fused);
  const bool group_on = wgrad_group_mode(dtype, 1) && fused;
  zero_flat_gradient(c, A, grad_flat, grad_flat_bytes, group_on, false);

  // Buffer roles: Gcur/Gnext ping-pong the gradient w.r.t. a block output / input; T1 = g_c3 then g_c1;
  // T2 = gz2 -> g_c2; T3 = g_d; T4 = downsample-branch input gradient; R3 = gradient w.r.t. res3 from the head.
  void *Gcur = P.G0, *Gnext = P.G1;
  heads_backward(c, A, P, gout, grad_flat, grad_flat_bytes, Gcur, [&](tf_conv_args& q) {
    if (!fused) return;
    // fused flow: Gcur always carries gz = g_y * (y > 0) of the block about to be processed, and (unless that block has a
    // downsample branch) its BN3-backward sums are accumulated by the conv that produces it (MASK2 | STATS3)
    const size_t last = A.blocks.size() - 1;
    q.epi = TF_EPI_MASK2; q.aux2 = P.blk[last].y;
    if (!A.blocks[last].has_ds) { q.epi |= TF_EPI_STATS3; q.aux3 = P.blk[last].c3; q.stat_out = P.blk[last].b3.bst; }
  });

  // Every fork makes its producer kernel carry a completion signal, which costs ~6 us of main-queue bubble behind that kernel
  // (profiles/r02b_step_timeline.txt: 90 x 5.9 us).  The ungrouped identity bottlenecks of layer 3 therefore fork ONCE, behind the
  // BN1-backward apply, when the dY operands of all three weight gradients exist: conv3's and conv2's gradients start ~100 us
  // later and overlap the next bottleneck instead, far from the end of the pass (layer 1 / 2 and the stem keep one fork per
  // gradient so that the tail of the weight-gradient stream stays short).
  WgradGroups groups(A, group_on);        // a group closes behind the BN1-backward apply of its lowest block
  // ---- bottlenecks in reverse
  for (int i = (int)A.blocks.size() - 1; i >= 0; --i) {
    const Block& B = A.blocks[i];
    Plan::Blk& b = P.blk[i];
    const int pl = B.planes, c4 = pl * 4;
    const int Min = N * b.Hin * b.Win, Mout = N * b.Hout * b.Wout;
    const void* yin = i == 0 ? P.pool : P.blk[i - 1].y;
    const void* extra = (i == A.layer_end[1] + 1) ? P.R3 : nullptr;     // the block whose INPUT is res3
    const bool grouped = groups.grouped(i), closes_group = groups.closes(i);
    const bool late = !grouped && fused && i > A.layer_end[1] && !B.has_ds;    // the three gradients behind ONE fork
    void *T1 = b.gT1, *T2 = b.gT2, *U1 = b.gU1, *T3 = b.gT3;      // the block's own buffers: nothing on this stream ever waits for a weight gradient
    // (1) per-channel sums for bn3 (and the downsample BN) with gz = g_y * (y > 0)
    const int nb = tf_colstats_blocks(Mout, c4, dtype);
    const int nk = B.has_ds ? 3 : 2;
    if (!fused) c.chk(tf_colstats(dtype, Gcur, b.y, b.c3, b.d, Mout, c4, c4, P.partial_b, c.stream));
    else if (B.has_ds) c.chk(tf_colstats(dtype, Gcur, nullptr, b.c3, b.d, Mout, c4, c4, b.b3.bst, c.stream));   // Gcur is already masked
    // (2) g_c3 -> T1
    if (fused) {
      const tf_bn_bwd_desc d = bwd_desc(c, B.c3, b.b3, b.b3.bst, nk, 1);
      if (!late && !grouped) c.arm_fork();
      c.chk(tf_bn_bwd_apply_fused(dtype, Gcur, nullptr, b.c3, &d, srows, Mout, c4, (float)Mout, T1, c.stream));
    } else {
      bn_backward_coefs(c, B.c3, c4, b.b3, P.partial_b, nb, nk, 1, c4, (float)Mout, B.has_ds ? 0 : 1);   // the last reader clears the partial rows
      if (B.has_ds) bn_backward_coefs(c, B.ds, c4, b.bd, P.partial_b, nb, nk, 2, c4, (float)Mout, 1);
      c.chk(tf_bn_bwd_apply(dtype, Gcur, b.y, b.c3, b.b3.cA, b.b3.cB, b.b3.cD, Mout, c4, T1, c.stream));
    }
    // (3) wgrad conv3 (its input is relu(bn2(c2)), materialised in the forward)
    auto wg3 = [&]() { wgrad(c, B.c3, c4, N, b.Hout, b.Wout, b.Hout, b.Wout, b.a2, pl, T1, c4); };
    if (!grouped && !late) { c.fork_armed(); wg3(); }
    // (4) dgrad conv3 -> gz2 in T2 (masked by relu(bn2(c2))) + BN-backward sums
    conv_fill(a, dtype, 1, N, b.Hout, b.Wout, c4, b.Hout, b.Wout, pl, 1, 1, 0, pl, T1, b.w3t, T2);
    a.epi = TF_EPI_MASK | TF_EPI_STATS2; a.aux = b.c2; a.mask_scale = b.b2.scale; a.mask_shift = b.b2.shift;
    a.stat_out = fused ? b.b2.bst : P.partial_b;
    c.chk(tf_conv2d(&a, c.stream));
    // (5) g_c2 in place
    if (fused) {
      const tf_bn_bwd_desc d = bwd_desc(c, B.c2, b.b2, b.b2.bst, 2, 1);
      if (!late && !grouped) c.arm_fork();
      c.chk(tf_bn_bwd_apply_fused(dtype, T2, nullptr, b.c2, &d, srows, Mout, pl, (float)Mout, T2, c.stream));
    } else {
      bn_backward_coefs(c, B.c2, pl, b.b2, P.partial_b, tf_conv_mtiles(&a), 2, 1, pl, (float)Mout);
      c.chk(tf_bn_bwd_apply(dtype, T2, nullptr, b.c2, b.b2.cA, b.b2.cB, b.b2.cD, Mout, pl, T2, c.stream));
    }
    // (6) wgrad conv2 (input relu(bn1(c1)))
    auto wg2 = [&]() { wgrad(c, B.c2, pl, N, b.Hin, b.Win, b.Hout, b.Wout, b.a1, pl, T2, pl, nullptr, 0, 0, 0, P.dwp, P.dwp_floats); };
    if (!grouped && !late) { c.fork_armed(); wg2(); }
    // (7) dgrad conv2 -> gz1 in U1 (+ sums); output spatial = conv2's input
    conv_fill(a, dtype, 1, N, b.Hout, b.Wout, pl, b.Hin, b.Win, pl, 3, B.stride, 1, pl, T2, b.w2t, U1);
    a.epi = TF_EPI_MASK | TF_EPI_STATS2; a.aux = b.c1; a.mask_scale = b.b1.scale; a.mask_shift = b.b1.shift;
    a.stat_out = fused ? b.b1.bst : P.partial_b;
    c.chk(tf_conv2d(&a, c.stream));
    // (8) g_c1 in place
    if (fused) {
      const tf_bn_bwd_desc d = bwd_desc(c, B.c1, b.b1, b.b1.bst, 2, 1);
      if (!grouped || closes_group) c.arm_fork();                 // grouped: only the kernel that completes a GROUP's operands carries a fork
      c.chk(tf_bn_bwd_apply_fused(dtype, U1, nullptr, b.c1, &d, srows, Min, pl, (float)Min, U1, c.stream));
    } else {
      bn_backward_coefs(c, B.c1, pl, b.b1, P.partial_b, tf_conv_mtiles(&a), 2, 1, pl, (float)Min);
      c.chk(tf_bn_bwd_apply(dtype, U1, nullptr, b.c1, b.b1.cA, b.b1.cB, b.b1.cD, Min, pl, U1, c.stream));
    }
    // (9) wgrad conv1 (input = block input, already activated); a grouped block queues its three problems instead
    if (grouped) {
      groups.push(i, wgrad_args(c, B.c3, c4, N, b.Hout, b.Wout, b.Hout, b.Wout, b.a2, pl, T1, c4),
                  wgrad_args(c, B.c2, pl, N, b.Hin, b.Win, b.Hout, b.Wout, b.a1, pl, T2, pl),
                  wgrad_args(c, B.c1, pl, N, b.Hin, b.Win, b.Hin, b.Win, yin, B.cin, U1, pl));
      if (closes_group) { c.fork_armed(); groups.flush(c, hooks); }
    } else {
      c.fork_armed();
      if (late) { wg3(); wg2(); }
      wgrad(c, B.c1, pl, N, b.Hin, b.Win, b.Hin, b.Win, yin, B.cin, U1, pl);
    }
    // (10) gradient w.r.t. the block input -> Gnext.  Fused flow: the conv that completes it also applies the ReLU mask of
    //      the previous block's output (MASK2 with aux2 = yin) and, unless that block has a downsample branch, accumulates
    //      its BN3-backward sums (STATS3 with aux3 = its c3), so the next iteration starts at step (2).
    auto hand_over = [&](tf_conv_args& q) {
      if (!fused || i == 0) return;                        // block 0's input is the max-pool output: no ReLU in between
      q.epi |= TF_EPI_MASK2; q.aux2 = yin;
      if (!A.blocks[i - 1].has_ds) { q.epi |= TF_EPI_STATS3; q.aux3 = P.blk[i - 1].c3; q.stat_out = P.blk[i - 1].b3.bst; }
    };
    if (B.has_ds) {                                        // the downsample BN's backward -> T3, and the weight gradient of its conv
      if (fused) {
        const tf_bn_bwd_desc d = bwd_desc(c, B.ds, b.bd, b.b3.bst, 3, 2);      // the downsample BN's sums are row 2 of bn3's region
        c.arm_fork();
        c.chk(tf_bn_bwd_apply_fused(dtype, Gcur, nullptr, b.d, &d, srows, Mout, c4, (float)Mout, T3, c.stream));
      } else {
        c.chk(tf_bn_bwd_apply(dtype, Gcur, b.y, b.d, b.bd.cA, b.bd.cB, b.bd.cD, Mout, c4, T3, c.stream));
      }
      c.fork_armed();
      wgrad(c, B.ds, c4, N, b.Hin, b.Win, b.Hout, b.Wout, yin, B.cin, T3, c4);
    }
    if (fused || B.has_ds) input_gradient(c, P, B, b, U1, B.has_ds ? T3 : Gcur, extra, Gnext, fused && i > 0, hand_over);   // identity branch: Gcur is already g_y * (y > 0)
    else {                                                 // unfolded flow, identity branch: + g_y * (y > 0)
      conv_fill(a, dtype, 1, N, b.Hin, b.Win, pl, b.Hin, b.Win, B.cin, 1, 1, 0, B.cin, U1, b.w1t, Gnext);
      a.epi = TF_EPI_JOIN; a.aux2 = b.y; a.aux3 = Gcur;
      c.chk(tf_conv2d(&a, c.stream));
    }
    // everything up to here: the weight / BN gradients of blocks >= i and of the heads (grouped blocks: their events fire behind the group)
    if (!grouped) record_grad_events(hooks, i, c.wstream(), c.rc);
    void* t = Gcur; Gcur = Gnext; Gnext = t;
  }

  // ---- stem
  const int M1 = N * P.H1 * P.W1;
  void* gz = P.T4;                          // main-stream scratch (its last reader, block 0's conv1 dgrad, is ahead on this stream)
  // r4: the statistic sums of the stem's BN backward ride in the max-pool backward (gz and x are in its registers): one pass over two 96 MB
  // tensors and one launch fewer at the very end of the chain (the unfolded flow keeps the two-pass form)
  int nb = 0;
  if (fused) {
    c.chk(tf_maxpool_bwd_stats(dtype, Gcur, P.pool_idx, P.cstem, P.bn_stem.scale, P.bn_stem.shift, N, P.H1, P.W1, 64, gz, P.partial_b, &nb, c.stream));
  } else {
    c.chk(tf_maxpool_bwd(dtype, Gcur, P.pool_idx, P.cstem, P.bn_stem.scale, P.bn_stem.shift, N, P.H1, P.W1, 64, gz, c.stream));
    nb = tf_colstats_blocks(M1, 64, dtype);
    c.chk(tf_colstats(dtype, gz, nullptr, P.cstem, nullptr, M1, 64, 64, P.partial_b, c.stream));
  }
  bn_backward_coefs(c, A.stem, 64, P.bn_stem, P.partial_b, nb, 2, 1, 64, (float)M1);
  // (r4: with the direct weight gradient the apply rides in that kernel's staging -- its output has no other reader)
  if (!stem_direct) c.chk(tf_bn_bwd_apply(dtype, gz, nullptr, P.cstem, P.bn_stem.cA, P.bn_stem.cB, P.bn_stem.cD, M1, 64, gz, c.stream));
  // P.col still holds the im2col matrix of this forward (nothing else is carved from that range)
  {
    ConvUnit s = A.stem; s.stride = 1; s.pad = 0;
    c.fork();
    if (stem_direct) {
      if (!c.grads_zeroed && hipMemsetAsync(c.G(A.stem.w), 0, (size_t)64 * 147 * 4, c.wstream()) != hipSuccess) c.chk(TF_ERR_LAUNCH);
      if (c.det) c.chk(tf_stem_wgrad_det(dtype, x, N, H, W, gz, P.cstem, P.bn_stem.cA, P.bn_stem.cB, P.bn_stem.cD, c.G(A.stem.w), c.det_slab, c.det_slab_bytes, c.wstream()));
      else c.chk(tf_stem_wgrad(dtype, x, N, H, W, gz, P.cstem, P.bn_stem.cA, P.bn_stem.cB, P.bn_stem.cD, c.G(A.stem.w), c.wstream()));
    } else wgrad(c, s, 64, 1, 1, M1, 1, M1, P.col, kStemK, gz, 64, nullptr, 147, 1, 147);
  }
  return close_backward(c, hooks);
}
extern "C" int tf_detnet_backward_ctx(tf_detnet_ctx* xctx, const tf_detnet_hooks* hooks, int dtype, const float* x, int N, int H, int W, int nout,
                                      void* const* params, void* const* grads, const float* gout, void* grad_flat, size_t grad_flat_bytes,
                                      void* ws, size_t ws_bytes, void* stream_) {
  return tf_detnet_trunk_backward_ctx(nullptr, xctx, hooks, dtype, x, N, H, W, nout, params, grads, gout, grad_flat, grad_flat_bytes, ws, ws_bytes,
                                      stream_);
}

// ------------------------------------------------------------------------------------------------
// backward through the FROZEN-BN graph (forward with training = TF_DETNET_FROZEN_BN).  Every BN is the constant map v -> v * s + h, so with
// gm = g_y * (y > 0) arriving from the block above, a1 / a2 the stored post-ReLU activations (c1 / c2 of the evaluation plan; a post-ReLU
// tensor is its own mask) and s1, s2, s3, sd the folded scales:
//   dW3 = diag(s3) (gm^T a2)            g2 = (W3 diag(s3))^T gm * (a2 > 0) * s2         [row scale | scaled transposed operand, AFFINE | MASK]
//   dW2 = g2^T (*) a1                   g1 = W2^T (*) g2 * (a1 > 0) * s1                [AFFINE | MASK]
//   dW1 = g1^T x                        gm_prev = (W1^T g1 + skip) * (x > 0)            [RES | MASK2]
//   skip = gm (identity) | (Wd diag(sd))^T gm, dWd = diag(sd) (gm^T x)                  [in place for stride 2]
// Three data-gradient launches per identity bottleneck and nothing else on the caller's stream.  gm lives in the block's own gT1 (the weight
// gradients of conv3 / the downsample conv read it on the second stream), g2 in gT2, g1 in gU1: the chain never waits for a weight gradient.
// Forks: ONE per block, carried by the conv2 data gradient (the kernel that produces the block's last weight-gradient operand); the grouped
// identity bottlenecks of layer 3 fork once per group, as in the batch-statistics graph.
//
// first_block (partial freeze: the stem and the lowest stages keep their weights) = the lowest bottleneck that receives weight gradients; -1 =
// the stem too, the whole graph.  Only stage boundaries are taken: a cut inside layer 3 would have to flush a half-filled weight-gradient group.
// The chain stops where the trained part begins: block first_block runs its two data gradients and its weight gradients (dW1 / dWd read the
// frozen prefix's output) but no input gradient, nothing below it is launched, and a head data gradient that has lost its reader is skipped.
extern "C" int tf_detnet_trunk_backward_frozen_from_ctx(const int* blocks, tf_detnet_ctx* xctx, const tf_detnet_hooks* hooks, int dtype,
                                                        const float* x, int N, int H, int W, int nout, void* const* params, void* const* grads,
                                                        const float* gout, void* grad_flat, size_t grad_flat_bytes, void* ws, size_t ws_bytes,
                                                        void* stream_, int first_block) {
  if (const Arch* a0 = find_arch(blocks)) {
    const int nb = (int)a0->blocks.size();
    if (first_block != -1 && first_block != 0 && first_block != a0->layer_end[0] + 1 && first_block != a0->layer_end[1] + 1 && first_block != nb)
      return TF_ERR_ARG;
  }
  const Arch* Ap; Plan P; Ctx c{};
  const int rc0 = open_backward(blocks, xctx, hooks, dtype, x, N, H, W, nout, params, grads, gout, ws, ws_bytes, stream_, kFrozen, Ap, P, c);
  if (rc0 != TF_OK) return rc0;
  const Arch& A = *Ap;
  tf_conv_args a;
  const int nblocks = (int)A.blocks.size();
  // the head-bias column sums fold into the head of this pass's partial buffer: zero on entry
  if (hipMemsetAsync(P.partial_b, 0, (size_t)TF_STAT_ROWS * 3 * 1024 * 4, c.stream) != hipSuccess) c.chk(TF_ERR_LAUNCH);
  const bool stem_direct = stem_direct_mode(dtype, false, false);      // (what the frozen forward took)
  const bool group_on = wgrad_group_mode(dtype, 1);
  // (the tensors of the frozen stages have no writer: the memset covers them; the split memset only where layer 3 is trained)
  zero_flat_gradient(c, A, grad_flat, grad_flat_bytes, group_on && first_block < nblocks, true);
  // gm of the last block: the head's data gradient, masked by the block's own output
  heads_backward(c, A, P, gout, grad_flat, grad_flat_bytes, P.blk[nblocks - 1].gT1,
                 [&](tf_conv_args& q) { q.epi = TF_EPI_MASK2; q.aux2 = P.blk[nblocks - 1].y; },
                 first_block < nblocks, first_block <= A.layer_end[1]);      // (R3's only reader is the input gradient of layer 3's first block)
  WgradGroups groups(A, group_on);        // a group closes behind the conv2 data gradient of its lowest block

  // ---- bottlenecks in reverse, down to the lowest trained one
  for (int i = nblocks - 1; i >= (first_block > 0 ? first_block : 0); --i) {
    const Block& B = A.blocks[i];
    Plan::Blk& b = P.blk[i];
    const int pl = B.planes, c4 = pl * 4;
    const void* yin = i == 0 ? P.pool : P.blk[i - 1].y;
    const void* extra = (i == A.layer_end[1] + 1) ? P.R3 : nullptr;     // the block whose INPUT is res3
    const bool grouped = groups.grouped(i), closes_group = groups.closes(i);
    void *gm = b.gT1, *T2 = b.gT2, *U1 = b.gU1;
    void* gprev = i > 0 ? P.blk[i - 1].gT1 : P.R3;      // (block 0: the gradient of the max-pool output; R3's last reader is far ahead on this stream)
    // (1) g2 = (W3 diag(s3))^T gm * (a2 > 0) * s2
    conv_fill(a, dtype, 1, N, b.Hout, b.Wout, c4, b.Hout, b.Wout, pl, 1, 1, 0, pl, gm, b.w3t, T2);
    a.epi = TF_EPI_AFFINE | TF_EPI_MASK; a.epi_scale = b.b2.scale; a.epi_shift = P.c_zero; a.aux = b.c2; a.mask_scale = P.c_one; a.mask_shift = P.c_zero;
    c.chk(tf_conv2d(&a, c.stream));
    // (2) g1 = W2^T (*) g2 * (a1 > 0) * s1; it completes the block's weight-gradient operands: the launch carries the fork
    conv_fill(a, dtype, 1, N, b.Hout, b.Wout, pl, b.Hin, b.Win, pl, 3, B.stride, 1, pl, T2, b.w2t, U1);
    a.epi = TF_EPI_AFFINE | TF_EPI_MASK; a.epi_scale = b.b1.scale; a.epi_shift = P.c_zero; a.aux = b.c1; a.mask_scale = P.c_one; a.mask_shift = P.c_zero;
    // (a stride-2 3x3 data gradient is four parity-class launches: the first would carry the event away -- a plain fork behind all four)
    if ((!grouped || closes_group) && B.stride == 1) c.arm_fork();
    c.chk(tf_conv2d(&a, c.stream));
    // (3) weight gradients, on the second stream; a grouped block queues its three problems instead
    if (grouped) {
      tf_wgrad_args w3 = wgrad_args(c, B.c3, c4, N, b.Hout, b.Wout, b.Hout, b.Wout, b.c2, pl, gm, c4);
      w3.row_scale = b.b3.scale;
      groups.push(i, w3, wgrad_args(c, B.c2, pl, N, b.Hin, b.Win, b.Hout, b.Wout, b.c1, pl, T2, pl),
                  wgrad_args(c, B.c1, pl, N, b.Hin, b.Win, b.Hin, b.Win, yin, B.cin, U1, pl));
      if (closes_group) { c.fork_armed(); groups.flush(c, hooks); }
    } else {
      c.fork_armed();
      wgrad(c, B.c3, c4, N, b.Hout, b.Wout, b.Hout, b.Wout, b.c2, pl, gm, c4, b.b3.scale);
      wgrad(c, B.c2, pl, N, b.Hin, b.Win, b.Hout, b.Wout, b.c1, pl, T2, pl, nullptr, 0, 0, 0, P.dwp, P.dwp_floats);
      wgrad(c, B.c1, pl, N, b.Hin, b.Win, b.Hin, b.Win, yin, B.cin, U1, pl);
      if (B.has_ds) wgrad(c, B.ds, c4, N, b.Hin, b.Win, b.Hout, b.Wout, yin, B.cin, gm, c4, b.bd.scale);
      record_grad_events(hooks, i, c.wstream(), c.rc);
    }
    // (4) gm_prev = (W1^T g1 + skip) * (x > 0) -> the previous block's gT1 (block 0: no ReLU between the max-pool and its input); gm is the
    //     skip branch's operand either way: the identity residual (already g_y * (y > 0)), or dY of the scaled downsample conv
    if (i == first_block) break;          // what lies below is frozen: nobody reads the gradient of this block's input
    input_gradient(c, P, B, b, U1, gm, extra, gprev, i > 0, [&](tf_conv_args& q) { if (i > 0) { q.epi |= TF_EPI_MASK2; q.aux2 = yin; } });
  }
  if (first_block >= 0) return close_backward(c, hooks, first_block);      // the stem is frozen too: no max-pool backward, no fork, no weight gradient

  // ---- stem: max-pool backward masks through relu (the stored cstem is post-ReLU: scale 1, shift 0), the BN scale rides in the weight gradient
  const int M1 = N * P.H1 * P.W1;
  void* gz = P.T4;
  c.chk(tf_maxpool_bwd(dtype, P.R3, P.pool_idx, P.cstem, P.c_one, P.c_zero, N, P.H1, P.W1, 64, gz, c.stream));
  {
    ConvUnit s = A.stem; s.stride = 1; s.pad = 0;
    c.fork();
    if (stem_direct) {
      if (!c.grads_zeroed && hipMemsetAsync(c.G(A.stem.w), 0, (size_t)64 * 147 * 4, c.wstream()) != hipSuccess) c.chk(TF_ERR_LAUNCH);
      // operand = cA * g + cB * x_conv + cD with cA = the folded scale, cB = cD = 0
      if (c.det) c.chk(tf_stem_wgrad_det(dtype, x, N, H, W, gz, P.cstem, P.bn_stem.scale, P.c_zero, P.c_zero, c.G(A.stem.w), c.det_slab, c.det_slab_bytes, c.wstream()));
      else c.chk(tf_stem_wgrad(dtype, x, N, H, W, gz, P.cstem, P.bn_stem.scale, P.c_zero, P.c_zero, c.G(A.stem.w), c.wstream()));
    } else wgrad(c, s, 64, 1, 1, M1, 1, M1, P.col, kStemK, gz, 64, P.bn_stem.scale, 147, 1, 147);      // (P.col still holds the im2col matrix of this forward)
  }
  return close_backward(c, hooks);
}
extern "C" int tf_detnet_trunk_backward_frozen_ctx(const int* blocks, tf_detnet_ctx* xctx, const tf_detnet_hooks* hooks, int dtype, const float* x,
                                                   int N, int H, int W, int nout, void* const* params, void* const* grads, const float* gout,
                                                   void* grad_flat, size_t grad_flat_bytes, void* ws, size_t ws_bytes, void* stream_) {
  return tf_detnet_trunk_backward_frozen_from_ctx(blocks, xctx, hooks, dtype, x, N, H, W, nout, params, grads, gout, grad_flat, grad_flat_bytes, ws,
                                                  ws_bytes, stream_, -1);
}
extern "C" int tf_detnet_backward_frozen_ctx(tf_detnet_ctx* xctx, const tf_detnet_hooks* hooks, int dtype, const float* x, int N, int H, int W, int nout,
                                             void* const* params, void* const* grads, const float* gout, void* grad_flat, size_t grad_flat_bytes,
                                             void* ws, size_t ws_bytes, void* stream_) {
  return tf_detnet_trunk_backward_frozen_from_ctx(nullptr, xctx, hooks, dtype, x, N, H, W, nout, params, grads, gout, grad_flat, grad_flat_bytes,
                                                  ws, ws_bytes, stream_, -1);
}

// context-free form (rounds 1-3): the default context of the current device + the process-wide hooks registered with tf_detnet_set_*
extern "C" int tf_detnet_backward(int dtype, const float* x, int N, int H, int W, int nout, void* const* params, void* const* grads,
                                  const float* gout, void* grad_flat, size_t grad_flat_bytes, void* ws, size_t ws_bytes, void* stream_) {
  std::vector<int> blocks; std::vector<void*> events;
  for (const auto& e : g_grad_events) { blocks.push_back(e.first); events.push_back((void*)e.second); }
  tf_detnet_hooks h;
  h.blocks = blocks.data(); h.events = events.data(); h.n = (int)blocks.size(); h.fn = g_grad_cb; h.user = g_grad_cb_user; h.single_stream = g_force_single ? 1 : 0;
  return tf_detnet_backward_ctx(nullptr, &h, dtype, x, N, H, W, nout, params, grads, gout, grad_flat, grad_flat_bytes, ws, ws_bytes, stream_);
}
