// On-device pre/post-processing around the denoise loop (reference app.ipynb:370-383 mask,
// :332-344 + :722-745 resize / normalise pipelines, :776-779 mask to latent resolution, :825-846 paste-back).
// The reference does all of this on the host with PIL / numpy / cv2 / albumentations and crosses PCIe twice; here the
// uint8 source image stays in HBM and the three 512x512 network inputs (image, masked image, mask) come out of ONE kernel,
// the result is pasted back by another.  Pure HBM-bound byte work: one thread per destination pixel, coalesced writes.
//
// The resize arithmetic (OpenCV INTER_LINEAR as published) lives in prepost_resize.h, shared with the batched kernels of prepost_batch.hip.
#include "common.h"
#include "kernels.h"
#include "prepost_resize.h"
#include "glyph_resample.h"
#include <math.h>

namespace {
using namespace dmx_resize;

struct PreArgs {
  const unsigned char* img; const unsigned char* mask; int H, W;       // HWC uint8 image, [H][W] mask of {0,1}
  Geom g;                                                              // crop origin, (clipped) extent, scales
  int S;                                                               // network resolution (512)
  float* out_img; float* out_masked; unsigned char* out_mask; float* out_mask_lat;   // [3][S][S], [3][S][S], [S][S], [S/8][S/8]
};

__global__ __launch_bounds__(256) void dmx_preprocess_kernel(const PreArgs p) {
  const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y;
  if (dx >= p.S) return;
  int vi[3], vm[3], vk;
  pre_pixel(p.img, p.W, p.g, [&](int y, int x) -> int { return p.mask[(size_t)(p.g.ys + y) * p.W + p.g.xs + x]; }, dx, dy, vi, vm, vk);
  pre_store(vi, vm, vk, p.S, dx, dy, p.out_img, p.out_masked, p.out_mask, p.out_mask_lat);
}

__global__ __launch_bounds__(256) void dmx_mask_rasterize_kernel(unsigned char* mask, int H, int W, int x0, int y0, int x1, int y1) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x < W) mask[(size_t)y * W + x] = (x >= x0 && x <= x1 && y >= y0 && y <= y1) ? 1 : 0;   // PIL rectangles include both corners
}

struct PostArgs {
  const float* vae; int S;                     // decoder output [3][S][S] in [-1, 1]
  const unsigned char* ori; unsigned char* out; int H, W;
  Geom g;                                      // paste origin, the extent the S x S image is resized to, scales
  int x1, y1, x2, y2;                          // text box: only these pixels are replaced
};
__global__ __launch_bounds__(256) void dmx_postprocess_kernel(const PostArgs p) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= p.W) return;
  const size_t o = ((size_t)y * p.W + x) * 3;
  const bool in_box = x >= p.x1 && x < p.x2 && y >= p.y1 && y < p.y2;
  const int dx = x - p.g.xs, dy = y - p.g.ys;
  const bool in_crop = dx >= 0 && dx < p.g.cw && dy >= 0 && dy < p.g.ch;
  if (!(in_box && in_crop)) { p.out[o] = p.ori[o]; p.out[o + 1] = p.ori[o + 1]; p.out[o + 2] = p.ori[o + 2]; return; }
#pragma unroll
  for (int c = 0; c < 3; ++c) p.out[o + c] = post_pixel(p.vae, p.S, p.g, c, dx, dy);
}
}  // namespace

extern "C" int dmx_mask_rasterize(unsigned char* mask, int H, int W, int x0, int y0, int x1, int y1, dmx_stream_t stream) {
  DMX_REQUIRE(mask && H > 0 && W > 0 && H <= 65535, "mask_rasterize: bad arguments");
  hipLaunchKernelGGL(dmx_mask_rasterize_kernel, dim3(cdiv(W, 256), H), dim3(256), 0, (hipStream_t)stream, mask, H, W, x0, y0, x1, y1);
  return dmx_check_launch("dmx_mask_rasterize_kernel");
}

extern "C" int dmx_preprocess_crop(const unsigned char* image_hwc, const unsigned char* mask, int H, int W, int x_s, int y_s, int crop_scale,
                                   int S, float* out_image, float* out_masked_image, unsigned char* out_mask, float* out_mask_latent,
                                   dmx_stream_t stream) {
  DMX_REQUIRE(image_hwc && mask && out_image && out_masked_image && out_mask, "preprocess_crop: null argument");
  DMX_REQUIRE(H > 0 && W > 0 && S > 0 && S % 8 == 0 && S <= 65535 && crop_scale > 0, "preprocess_crop: bad sizes");
  DMX_REQUIRE(x_s >= 0 && y_s >= 0 && x_s < W && y_s < H, "preprocess_crop: crop origin (%d, %d) outside the %dx%d image", x_s, y_s, W, H);
  PreArgs p{};
  p.img = image_hwc; p.mask = mask; p.H = H; p.W = W;
  p.g = pre_geom(H, W, x_s, y_s, crop_scale, S);                       // numpy slicing clips the crop at the border
  p.S = S; p.out_img = out_image; p.out_masked = out_masked_image; p.out_mask = out_mask; p.out_mask_lat = out_mask_latent;
  hipLaunchKernelGGL(dmx_preprocess_kernel, dim3(cdiv(S, 256), S), dim3(256), 0, (hipStream_t)stream, p);
  return dmx_check_launch("dmx_preprocess_kernel");
}

extern "C" int dmx_postprocess_paste(const float* image_vae, int S, const unsigned char* original_hwc, unsigned char* out_hwc, int H, int W,
                                     int x_s, int y_s, int crop_scale, int x1, int y1, int x2, int y2, dmx_stream_t stream) {
  DMX_REQUIRE(image_vae && original_hwc && out_hwc, "postprocess_paste: null argument");
  DMX_REQUIRE(H > 0 && W > 0 && H <= 65535 && S > 0 && crop_scale > 0 && x_s >= 0 && y_s >= 0 && x_s < W && y_s < H, "postprocess_paste: bad sizes");
  PostArgs p{};
  p.vae = image_vae; p.S = S; p.ori = original_hwc; p.out = out_hwc; p.H = H; p.W = W;
  p.g = post_geom(H, W, x_s, y_s, crop_scale, S);                      // app.ipynb:831-839
  p.x1 = x1; p.y1 = y1; p.x2 = x2; p.y2 = y2;
  hipLaunchKernelGGL(dmx_postprocess_kernel, dim3(cdiv(W, 256), H), dim3(256), 0, (hipStream_t)stream, p);
  return dmx_check_launch("dmx_postprocess_kernel");
}

// ---- TrOCRProcessor's image half (reference: `processor(images=ttf_imgs, return_tensors="pt").pixel_values`, app.ipynb:773,
// train_diffute_v1.py:868): Pillow's 8-bit two-pass resample (Resample.c as published) + the processor's rescale / normalise, for a
// ragged batch in ONE launch.  Everything that involves floating point is done on the host and shipped as tables: per (in, out, filter) the
// bounds [out][2] = (first source index, tap count) followed by the 2^22 fixed-point coefficients [out][ksize]; the uint8 -> fp32
// normalisation as norm[3][256].  The kernel is integer MACs and table look-ups only, so its result does not depend on build flags.
//   horizontal pass first: h = clip8((2^21 + sum pixel * k) >> 22) stored as a BYTE, the vertical pass runs on those bytes; a pass whose
//   input and output size are equal is skipped (table offset < 0).
// One thread per destination pixel, all three channels; the per-pixel arithmetic is glyph_resample.h.
namespace {
struct GlyphArgs {
  const dmx_glyph_image* desc; const int* tab; const float* norm;
  int S_h, S_w; float* out; unsigned char* out_u8;
};
__global__ __launch_bounds__(128) void dmx_glyph_resize_normalize_kernel(const GlyphArgs p) {
  const int ox = blockIdx.x * blockDim.x + threadIdx.x, oy = blockIdx.y, b = blockIdx.z;
  if (ox >= p.S_w) return;
  const dmx_glyph_image d = p.desc[b];
  const unsigned char* src = (const unsigned char*)d.src;
  const dmx_glyph::Passes ps{d.h_off, d.h_taps, d.v_off, d.v_taps};
  int v[3];
  // the two-pass arithmetic and its clamps: glyph_resample.h, shared with the read-back kernel (readback.hip)
  dmx_glyph::glyph_resample_pixel(
      [&](int y, int x, int c) -> int { return src[(long long)y * d.stride_y + (long long)x * d.stride_x + (long long)c * d.stride_c]; }, d.H, d.W,
      p.tab, ps, p.S_h, p.S_w, ox, oy, v);
  const size_t plane = (size_t)p.S_h * p.S_w, o = (size_t)b * 3 * plane + (size_t)oy * p.S_w + ox;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    p.out[o + c * plane] = p.norm[c * 256 + v[c]];
    if (p.out_u8) p.out_u8[o + c * plane] = (unsigned char)v[c];
  }
}
}  // namespace

extern "C" int dmx_glyph_max_taps(void) { return DMX_GLYPH_MAX_TAPS; }

extern "C" int dmx_glyph_resize_normalize(const dmx_glyph_image* images, int B, const int* tables, const float* norm, int max_taps, int S_h, int S_w,
                                          float* out_pixel_values, unsigned char* out_resized, dmx_stream_t stream) {
  DMX_REQUIRE(images && tables && norm && out_pixel_values, "glyph_resize_normalize: null argument");
  DMX_REQUIRE(B > 0 && B <= 65535 && S_h > 0 && S_h <= 65535 && S_w > 0, "glyph_resize_normalize: bad sizes (B %d, output %dx%d)", B, S_h, S_w);
  DMX_REQUIRE(max_taps >= 0 && max_taps <= DMX_GLYPH_MAX_TAPS,
              "glyph_resize_normalize: %d taps per output pixel exceed the cap of %d (downscale ratio at most 31 for bilinear, 15 for bicubic)",
              max_taps, DMX_GLYPH_MAX_TAPS);
  GlyphArgs p{images, tables, norm, S_h, S_w, out_pixel_values, out_resized};
  hipLaunchKernelGGL(dmx_glyph_resize_normalize_kernel, dim3(cdiv(S_w, 128), S_h, B), dim3(128), 0, (hipStream_t)stream, p);
  return dmx_check_launch("dmx_glyph_resize_normalize_kernel");
}
