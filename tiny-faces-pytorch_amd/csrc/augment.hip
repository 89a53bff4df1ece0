// Image preparation in front of the detector: everything between the decoded uint8 image and
// the normalised fp32 NCHW tensor, in one pass per image:
//   PIL BILINEAR resize (x0.5 / x2 in training, any ratio for the evaluation pyramid)   tinyfaces/datasets/wider_face.py:136-146,
//                                                                                        tinyfaces/evaluation.py:46 (through
//                                                                                        torchvision.transforms.functional.resize)
//   500x500 crop pasted at a random place on the mean colour                            tinyfaces/datasets/processor.py:41-76
//   horizontal flip                                                                     tinyfaces/datasets/wider_face.py:155-157
//   ToTensor + Normalize                                                                main.py:44-46
// Only the pixels of the crop window are ever resampled (the reference resizes the whole image on the CPU, then crops).
//
// Bit-exactness: the resize is Pillow's two-pass 8-bit resample (src/libImaging/Resample.c: precompute_coeffs with the bilinear
// filter, normalize_coeffs_8bpc, horizontal pass then vertical pass with a uint8 intermediate).  Every output pixel re-derives
// its own coefficients in double precision exactly as Pillow does (this file is compiled with -ffp-contract=off: the
// `0.5 + w * 2^22` rounding must not become an FMA) and evaluates the horizontal pass for each of its vertical taps, so no
// intermediate image exists.  The float stage divides (x / 255, (x - mean) / std) like torch does.
#include "common.h"

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;

struct Taps { int lo, n; double center, ss, ww; };

__device__ __forceinline__ double bilinear_w(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}

// precompute_coeffs for output index xx of an axis resampled from in_size to out_size (in0 = 0)
__device__ __forceinline__ Taps taps_for(int in_size, int out_size, int xx) {
  Taps t;
  const double scale = (double)in_size / (double)out_size;
  double filterscale = scale;
  if (filterscale < 1.0) filterscale = 1.0;
  const double support = 1.0 * filterscale;
  t.center = (xx + 0.5) * scale;
  t.ss = 1.0 / filterscale;
  int lo = (int)(t.center - support + 0.5);
  if (lo < 0) lo = 0;
  int hi = (int)(t.center + support + 0.5);
  if (hi > in_size) hi = in_size;
  t.lo = lo; t.n = hi - lo;
  double ww = 0.0;
  for (int x = 0; x < t.n; ++x) ww += bilinear_w((x + lo - t.center + 0.5) * t.ss);
  t.ww = ww;
  return t;
}
__device__ __forceinline__ int fixed_coef(const Taps& t, int x) {
  double w = bilinear_w((x + t.lo - t.center + 0.5) * t.ss);
  if (t.ww != 0.0) w /= t.ww;
  return w < 0 ? (int)(-0.5 + w * (double)(1 << kPrecisionBits)) : (int)(0.5 + w * (double)(1 << kPrecisionBits));
}
__device__ __forceinline__ int clip8(int v) {
  v >>= kPrecisionBits;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// The uint8 pixel of the augmented OH x OW image at (ox, oy): the mean colour outside the pasted window, Pillow's resample inside.
// Shared by the plain pass and the colour-jitter passes (integers only: the same bits wherever it is inlined).
__device__ __forceinline__ void augmented_pixel(const tf_image_prepare_args& a, int ox, int oy, int (&px)[3]) {
  const int bx = a.flip ? a.OW - 1 - ox : ox, by = oy;           // position in the un-flipped buffer
  px[0] = a.bg[0]; px[1] = a.bg[1]; px[2] = a.bg[2];
  const int wy = by - a.paste_y, wx = bx - a.paste_x;
  if (wy >= 0 && wy < a.crop_h && wx >= 0 && wx < a.crop_w) {
    const int ry = a.crop_y + wy, rx = a.crop_x + wx;            // pixel of the resized image
    const bool hres = a.RW != a.W, vres = a.RH != a.H;
    Taps th, tv;
    if (hres) th = taps_for(a.W, a.RW, rx);
    if (vres) tv = taps_for(a.H, a.RH, ry);
    auto hpass = [&](int y, int (&o)[3]) {                        // value of the horizontally resampled image at (y, rx)
      const unsigned char* row = a.img + (size_t)y * a.W * 3;
      if (!hres) { o[0] = row[rx * 3]; o[1] = row[rx * 3 + 1]; o[2] = row[rx * 3 + 2]; return; }
      int acc[3] = {1 << (kPrecisionBits - 1), 1 << (kPrecisionBits - 1), 1 << (kPrecisionBits - 1)};
      for (int x = 0; x < th.n; ++x) {
        const int k = fixed_coef(th, x);
        const unsigned char* p = row + (size_t)(th.lo + x) * 3;
        acc[0] += p[0] * k; acc[1] += p[1] * k; acc[2] += p[2] * k;
      }
      o[0] = clip8(acc[0]); o[1] = clip8(acc[1]); o[2] = clip8(acc[2]);
    };
    if (!vres) {
      hpass(ry, px);
    } else {
      int acc[3] = {1 << (kPrecisionBits - 1), 1 << (kPrecisionBits - 1), 1 << (kPrecisionBits - 1)};
      for (int y = 0; y < tv.n; ++y) {
        int h[3];
        hpass(tv.lo + y, h);
        const int k = fixed_coef(tv, y);
        acc[0] += h[0] * k; acc[1] += h[1] * k; acc[2] += h[2] * k;
      }
      px[0] = clip8(acc[0]); px[1] = clip8(acc[1]); px[2] = clip8(acc[2]);
    }
  }
}

// ToTensor + Normalize of one pixel
__device__ __forceinline__ void store_normalized(const tf_image_prepare_args& a, int ox, int oy, const int (&px)[3]) {
  const size_t plane = (size_t)a.OH * a.OW, o = (size_t)oy * a.OW + ox;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float x = (float)px[c] / 255.0f;
    a.out[c * plane + o] = (x - a.mean[c]) / a.std[c];
  }
}

__global__ void __launch_bounds__(256) image_prepare_kernel(const tf_image_prepare_args a) {
  const int ox = blockIdx.x * 64 + (threadIdx.x & 63), oy = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (ox >= a.OW || oy >= a.OH) return;
  int px[3];
  augmented_pixel(a, ox, oy, px);
  store_normalized(a, ox, oy, px);
}

// ---- f1: colour jitter (include/tinyfaces_hip.h has the definition; tests/color_jitter_ref.py the same arithmetic in numpy) ----
struct JitterChain { int n; int op[4]; float f[4]; };

__device__ __forceinline__ int sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Pillow's ImagingBlend on one channel (ImageEnhance: Image.blend(degenerate, image, factor))
__device__ __forceinline__ int blend8(int d, int x, float f) {
  const float t = (float)d + f * ((float)x - (float)d);
  if (f >= 0.f && f <= 1.f) return (int)t;
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}
__device__ __forceinline__ int luma8(const int (&px)[3]) { return (px[0] * 19595 + px[1] * 38470 + px[2] * 7471 + 0x8000) >> 16; }

// Pillow's rgb2hsv, the hue byte shifted, Pillow's hsv2rgb (the latter in double)
__device__ __forceinline__ void hue_shift(int (&px)[3], int shift) {
  const int r = px[0], g = px[1], b = px[2];
  const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
  int uh = 0, us = 0;
  const int uv = mx;
  if (mx != mn) {
    const float cr = (float)(mx - mn);
    const float s = cr / (float)mx;
    const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
    float h;
    if (r == mx) h = (float)((double)bc - (double)gc);
    else if (g == mx) h = (float)(2.0 + (double)rc - (double)bc);
    else h = (float)(4.0 + (double)gc - (double)rc);
    const double x = (double)h / 6.0 + 1.0;                      // in [5/6, 11/6]: fmod(x, 1.0) = x - floor(x), exactly
    h = (float)(x - floor(x));
    uh = sat8((int)((double)h * 255.0));
    us = sat8((int)(s * 255.0f));
  }
  uh = (uh + shift) & 255;
  if (us == 0) { px[0] = px[1] = px[2] = uv; return; }
  const double fh = (double)uh * 6.0 / 255.0;
  const double fi = floor(fh);
  const double f = fh - fi, fs = (double)us / 255.0, v = (double)uv;
  const int p = sat8((int)floor(v * (1.0 - fs) + 0.5));
  const int q = sat8((int)floor(v * (1.0 - fs * f) + 0.5));
  const int t = sat8((int)floor(v * (1.0 - fs * (1.0 - f)) + 0.5));
  switch ((int)fi % 6) {
    case 0: px[0] = uv; px[1] = t; px[2] = p; break;
    case 1: px[0] = q; px[1] = uv; px[2] = p; break;
    case 2: px[0] = p; px[1] = uv; px[2] = t; break;
    case 3: px[0] = p; px[1] = q; px[2] = uv; break;
    case 4: px[0] = t; px[1] = p; px[2] = uv; break;
    default: px[0] = uv; px[1] = p; px[2] = q; break;
  }
}

// ops [first, last) of the chain on one pixel; m = the contrast mean (read only when contrast is in the range)
__device__ __forceinline__ void apply_chain(const JitterChain& ch, int first, int last, int m, int (&px)[3]) {
  for (int i = first; i < last; ++i) {
    const float f = ch.f[i];
    switch (ch.op[i]) {
      case TF_JITTER_BRIGHTNESS: px[0] = blend8(0, px[0], f); px[1] = blend8(0, px[1], f); px[2] = blend8(0, px[2], f); break;
      case TF_JITTER_CONTRAST: px[0] = blend8(m, px[0], f); px[1] = blend8(m, px[1], f); px[2] = blend8(m, px[2], f); break;
      case TF_JITTER_SATURATION: {
        const int l = luma8(px);
        px[0] = blend8(l, px[0], f); px[1] = blend8(l, px[1], f); px[2] = blend8(l, px[2], f);
      } break;
      default: hue_shift(px, (int)f); break;
    }
  }
}

// sum of v over the 256 threads of the block, returned to every thread (wave64: 6 shuffle steps, then 4 words of LDS)
__device__ __forceinline__ unsigned block_sum_u32(unsigned v, unsigned (&lds)[4]) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  return lds[0] + lds[1] + lds[2] + lds[3];
}

// PHASE 0: a chain without contrast, one launch.  PHASE 1: the ops in front of contrast (chain positions [0, split)), the uint8 image to
// ws_img and the block's sum of L to ws_part[block].  PHASE 2: the mean from the partial sums, contrast and the rest (positions [split, n)).
// Every partial sum, and their total (<= 2^24 * 255), fits 32 bits.
template <int PHASE>
__global__ void __launch_bounds__(256) image_prepare_jitter_kernel(const tf_image_prepare_args a, const JitterChain ch, int split,
                                                                   unsigned* ws_part, unsigned char* ws_img) {
  __shared__ unsigned lds[4];
  const int ox = blockIdx.x * 64 + (threadIdx.x & 63), oy = blockIdx.y * 4 + (threadIdx.x >> 6);
  const bool inside = ox < a.OW && oy < a.OH;
  const size_t o = (size_t)oy * a.OW + ox;
  int px[3] = {0, 0, 0};
  if (PHASE == 0) {
    if (!inside) return;
    augmented_pixel(a, ox, oy, px);
    apply_chain(ch, 0, ch.n, 0, px);
    store_normalized(a, ox, oy, px);
  } else if (PHASE == 1) {
    unsigned l = 0;                                              // threads outside the image add nothing, but take part in the sum
    if (inside) {
      augmented_pixel(a, ox, oy, px);
      apply_chain(ch, 0, split, 0, px);
      ws_img[o * 3] = (unsigned char)px[0]; ws_img[o * 3 + 1] = (unsigned char)px[1]; ws_img[o * 3 + 2] = (unsigned char)px[2];
      l = (unsigned)luma8(px);
    }
    const unsigned s = block_sum_u32(l, lds);
    if (threadIdx.x == 0) ws_part[blockIdx.y * gridDim.x + blockIdx.x] = s;
  } else {
    const unsigned nblocks = gridDim.x * gridDim.y;
    unsigned part = 0;
    for (unsigned i = threadIdx.x; i < nblocks; i += 256) part += ws_part[i];
    const unsigned long long S = block_sum_u32(part, lds), n = (unsigned long long)a.OH * a.OW;
    if (!inside) return;
    const int m = (int)((2 * S + n) / (2 * n));
    px[0] = ws_img[o * 3]; px[1] = ws_img[o * 3 + 1]; px[2] = ws_img[o * 3 + 2];
    apply_chain(ch, split, ch.n, m, px);
    store_normalized(a, ox, oy, px);
  }
}

int check_prepare_args(const tf_image_prepare_args* a) {
  if (!a || !a->img || !a->out) return TF_ERR_ARG;
  if (a->H <= 0 || a->W <= 0 || a->RH <= 0 || a->RW <= 0 || a->OH <= 0 || a->OW <= 0) return TF_ERR_ARG;
  if (a->crop_h < 0 || a->crop_w < 0 || a->crop_y < 0 || a->crop_x < 0 || a->crop_y + a->crop_h > a->RH || a->crop_x + a->crop_w > a->RW)
    return TF_ERR_ARG;
  if (a->paste_y < 0 || a->paste_x < 0 || a->paste_y + a->crop_h > a->OH || a->paste_x + a->crop_w > a->OW) return TF_ERR_ARG;
  for (int c = 0; c < 3; ++c) if (!(a->std[c] != 0.f)) return TF_ERR_ARG;
  return TF_OK;
}

constexpr long long kJitterMaxPixels = 1ll << 24;

// position of contrast in the chain (-1: none), or -2 for a chain the entry refuses
int contrast_position(int n_ops, const int* op) {
  if (n_ops < 0 || n_ops > 4 || (n_ops > 0 && !op)) return -2;
  int seen = 0, at = -1;
  for (int i = 0; i < n_ops; ++i) {
    if (op[i] < 0 || op[i] > TF_JITTER_HUE || (seen >> op[i] & 1)) return -2;
    seen |= 1 << op[i];
    if (op[i] == TF_JITTER_CONTRAST) at = i;
  }
  return at;
}
size_t partials_bytes(int OH, int OW) { return (((size_t)((OW + 63) / 64) * (size_t)((OH + 3) / 4) * 4) + 255) / 256 * 256; }

}  // namespace

extern "C" int tf_image_prepare(const tf_image_prepare_args* a, void* stream) {
  if (const int rc = check_prepare_args(a)) return rc;
  hipLaunchKernelGGL(image_prepare_kernel, dim3((a->OW + 63) / 64, (a->OH + 3) / 4), dim3(256), 0, (hipStream_t)stream, *a);
  TF_CHECK_LAUNCH();
  return TF_OK;
}

extern "C" size_t tf_image_prepare_jitter_workspace_bytes(int OH, int OW, int n_ops, const int* op) {
  if (OH <= 0 || OW <= 0 || (long long)OH * OW > kJitterMaxPixels || contrast_position(n_ops, op) < 0) return 0;
  return partials_bytes(OH, OW) + (size_t)3 * OH * OW;
}

extern "C" int tf_image_prepare_jitter(const tf_image_prepare_args* a, int n_ops, const int* op, const float* factor, void* ws,
                                       size_t ws_bytes, void* stream) {
  if (const int rc = check_prepare_args(a)) return rc;
  if ((long long)a->OH * a->OW > kJitterMaxPixels) return TF_ERR_ARG;
  const int at = contrast_position(n_ops, op);
  if (at == -2 || (n_ops > 0 && !factor)) return TF_ERR_ARG;
  JitterChain ch = {};
  ch.n = n_ops;
  for (int i = 0; i < n_ops; ++i) {
    const float f = factor[i];
    if (!(f >= 0.f) || !(f <= 3.0e38f)) return TF_ERR_ARG;        // negative, NaN, Inf
    if (op[i] == TF_JITTER_HUE && (f > 255.f || f != (float)(int)f)) return TF_ERR_ARG;
    ch.op[i] = op[i]; ch.f[i] = f;
  }
  const dim3 grid((a->OW + 63) / 64, (a->OH + 3) / 4), block(256);
  if (at < 0) {
    hipLaunchKernelGGL(image_prepare_jitter_kernel<0>, grid, block, 0, (hipStream_t)stream, *a, ch, 0, (unsigned*)nullptr, (unsigned char*)nullptr);
    TF_CHECK_LAUNCH();
    return TF_OK;
  }
  const size_t pb = partials_bytes(a->OH, a->OW);
  if (!ws || ws_bytes < pb + (size_t)3 * a->OH * a->OW) return TF_ERR_WORKSPACE;
  unsigned* part = (unsigned*)ws;
  unsigned char* img = (unsigned char*)ws + pb;
  hipLaunchKernelGGL(image_prepare_jitter_kernel<1>, grid, block, 0, (hipStream_t)stream, *a, ch, at, part, img);
  TF_CHECK_LAUNCH();
  hipLaunchKernelGGL(image_prepare_jitter_kernel<2>, grid, block, 0, (hipStream_t)stream, *a, ch, at, part, img);
  TF_CHECK_LAUNCH();
  return TF_OK;
}
