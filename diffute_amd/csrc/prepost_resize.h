// The resize arithmetic of the pre/post-processing kernels, stated once: prepost.hip (one box per launch, geometry as kernel
// arguments, mask read from memory) and prepost_batch.hip (B boxes of one image per launch, geometry from a device table, mask
// as a predicate) both compute a pixel through pre_pixel / post_pixel below, so their results agree bit for bit.
//
// Resize semantics follow OpenCV's cv::resize(INTER_LINEAR) as published (imgproc/resize.cpp), which is what
// albumentations.Resize and the notebook's cv2.resize call:
//   source coordinate fx = (dx + 0.5) * scale - 0.5, sx = floor(fx), a horizontal tap off the border is moved onto it with its weight reset, vertical taps only clamp the row;
//   uint8 images: fixed point - weights cvRound(w * 2048) as int16, horizontal sums kept as int32, vertical
//     dst = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2;
//   float images: horizontal r = s0*a0 + s1*a1, vertical dst = r0*b0 + r1*b1 in fp32;
//   an exact 2x downscale is taken by the INTER_AREA fast path instead (2x2 mean; uint8 (a+b+c+d+2)>>2).
// cv2 / albumentations are not installed in the build image, so these rules are restated, not pinned against the library
// ("parity unpinned" in oracle/prepost.py, which the tests compare against bit for bit).
#pragma once
#include <math.h>
#include <stddef.h>
#include "kernels.h"

namespace dmx_resize {
// What a resize needs besides the pixels: where the crop sits in the image, its extent clipped at the border (numpy slicing
// clips; app.ipynb:831-839 does the same by hand for the paste) and the two scale factors as doubles, like cv::resize.
//   preprocess:  crop (cw x ch) -> S x S, scale = extent / S, area2 when the extent is exactly 2S x 2S
//   postprocess: S x S -> crop (cw x ch), scale = S / extent, area2 when S is exactly twice the extent
struct Geom {
  int xs, ys, cw, ch;
  double sx, sy;
  int area2;
};
inline int clipped_extent(int crop_scale, int origin, int size) { return crop_scale < size - origin ? crop_scale : size - origin; }
inline Geom pre_geom(int H, int W, int x_s, int y_s, int crop_scale, int S) {
  Geom g{};
  g.xs = x_s; g.ys = y_s; g.cw = clipped_extent(crop_scale, x_s, W); g.ch = clipped_extent(crop_scale, y_s, H);
  g.sx = (double)g.cw / S; g.sy = (double)g.ch / S;
  g.area2 = (g.cw == 2 * S && g.ch == 2 * S) ? 1 : 0;
  return g;
}
inline Geom post_geom(int H, int W, int x_s, int y_s, int crop_scale, int S) {
  Geom g{};
  g.xs = x_s; g.ys = y_s; g.cw = clipped_extent(crop_scale, x_s, W); g.ch = clipped_extent(crop_scale, y_s, H);
  g.sx = (double)S / g.cw; g.sy = (double)S / g.ch;
  g.area2 = (S == 2 * g.cw && S == 2 * g.ch) ? 1 : 0;
  return g;
}

#ifdef __HIPCC__
struct Tap { int s0, s1; short a0, a1; float f0, f1; };

// OpenCV's tap for destination index d: `n` source samples, `scale` = n / dst_size (double, like cv::resize).
//   fx = (float)((d + 0.5) * scale - 0.5); s = cvFloor(fx); fx -= s;
// Horizontally a tap that falls off the border is moved onto it and its weight reset (s < 0 -> s = 0, fx = 0;
// s >= n-1 -> s = n-1, fx = 0); vertically only the row indices are clamped and the weights are kept.
__device__ __forceinline__ Tap tap_for(int d, int n, double scale, bool horizontal) {
  float f = (float)(((double)d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  float w = f - (float)s;
  Tap t;
  if (horizontal) {
    if (s < 0) { s = 0; w = 0.f; }
    if (s >= n - 1) { s = n - 1; w = 0.f; }
    t.s0 = s; t.s1 = min(s + 1, n - 1);
  } else {
    t.s0 = min(max(s, 0), n - 1); t.s1 = min(max(s + 1, 0), n - 1);
  }
  t.f0 = 1.f - w; t.f1 = w;
  t.a0 = (short)__float2int_rn(t.f0 * 2048.f);       // saturate_cast<short>(cvRound(.)); |value| <= 2048
  t.a1 = (short)__float2int_rn(t.f1 * 2048.f);
  return t;
}
__device__ __forceinline__ int vert_u8(int r0, int r1, short b0, short b1) {
  return ((((int)b0 * (r0 >> 4)) >> 16) + (((int)b1 * (r1 >> 4)) >> 16) + 2) >> 2;
}
// albumentations.Normalize(mean 0.5, std 0.5, max_pixel_value 255): (x - 127.5) * (1 / 127.5) in fp32
__device__ __forceinline__ float normalize_u8(int v) {
  const float mean = 0.5f * 255.f, inv = 1.0f / (0.5f * 255.f);
  return ((float)v - mean) * inv;
}

// Destination pixel (dx, dy) of the S x S network inputs: the resized crop of the image (vi), of the image with the text box
// blacked out BEFORE the resize (vm; prepare_mask_and_masked_image, app.ipynb:380-383) and of the mask itself (vk), all as
// bytes.  img: uint8 HWC with row length W; mk(y, x) -> {0, 1} is the mask at crop coordinates.
template <class Mask>
__device__ __forceinline__ void pre_pixel(const unsigned char* img, int W, const Geom& g, Mask mk, int dx, int dy, int vi[3], int vm[3], int& vk) {
  auto px = [&](int y, int x, int c) -> int { return img[((size_t)(g.ys + y) * W + g.xs + x) * 3 + c]; };
  if (g.area2) {
    const int x0 = 2 * dx, y0 = 2 * dy;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int a = 0, b = 0;
      for (int j = 0; j < 2; ++j)
        for (int i = 0; i < 2; ++i) { const int v = px(y0 + j, x0 + i, c); a += v; b += mk(y0 + j, x0 + i) ? 0 : v; }
      vi[c] = (a + 2) >> 2; vm[c] = (b + 2) >> 2;
    }
    vk = (mk(y0, x0) + mk(y0, x0 + 1) + mk(y0 + 1, x0) + mk(y0 + 1, x0 + 1) + 2) >> 2;
  } else {
    const Tap tx = tap_for(dx, g.cw, g.sx, true), ty = tap_for(dy, g.ch, g.sy, false);
    const int m00 = mk(ty.s0, tx.s0), m01 = mk(ty.s0, tx.s1), m10 = mk(ty.s1, tx.s0), m11 = mk(ty.s1, tx.s1);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int s00 = px(ty.s0, tx.s0, c), s01 = px(ty.s0, tx.s1, c), s10 = px(ty.s1, tx.s0, c), s11 = px(ty.s1, tx.s1, c);
      vi[c] = vert_u8(s00 * tx.a0 + s01 * tx.a1, s10 * tx.a0 + s11 * tx.a1, ty.a0, ty.a1);
      vm[c] = vert_u8((m00 ? 0 : s00) * tx.a0 + (m01 ? 0 : s01) * tx.a1, (m10 ? 0 : s10) * tx.a0 + (m11 ? 0 : s11) * tx.a1, ty.a0, ty.a1);
    }
    vk = vert_u8(m00 * tx.a0 + m01 * tx.a1, m10 * tx.a0 + m11 * tx.a1, ty.a0, ty.a1);
  }
}

// One thread's stores of the four preprocess outputs (planes of S x S; the latent mask is the nearest downsample,
// F.interpolate(mask, size = S/8): source index = floor(dst * 8)).
__device__ __forceinline__ void pre_store(const int vi[3], const int vm[3], int vk, int S, int dx, int dy,
                                          float* out_img, float* out_masked, unsigned char* out_mask, float* out_mask_lat) {
  const size_t plane = (size_t)S * S, o = (size_t)dy * S + dx;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    out_img[c * plane + o] = normalize_u8(vi[c]);
    out_masked[c * plane + o] = normalize_u8(vm[c]);
  }
  out_mask[o] = (unsigned char)vk;
  if (out_mask_lat && (dx & 7) == 0 && (dy & 7) == 0) out_mask_lat[(size_t)(dy >> 3) * (S >> 3) + (dx >> 3)] = (float)vk;
}

__device__ __forceinline__ float post_src(const float* vae, int S, int c, int y, int x) {
  return (vae[((size_t)c * S + y) * S + x] / 2.f + 0.5f) * 255.0f;      // (image_vae / 2 + 0.5) * 255.0
}
// Channel c of pixel (dx, dy) of the decoder output vae [3][S][S] resized to the crop extent, as the byte that is pasted.
// inf_res.round().astype("uint8"): round half to even; values outside [0, 255] are clamped here (numpy's cast of an
// out-of-range float is undefined behaviour - the one deliberate deviation)
__device__ __forceinline__ unsigned char post_pixel(const float* vae, int S, const Geom& g, int c, int dx, int dy) {
  float v;
  if (g.area2) {
    v = (post_src(vae, S, c, 2 * dy, 2 * dx) + post_src(vae, S, c, 2 * dy, 2 * dx + 1) + post_src(vae, S, c, 2 * dy + 1, 2 * dx) +
         post_src(vae, S, c, 2 * dy + 1, 2 * dx + 1)) * 0.25f;
  } else {
    const Tap tx = tap_for(dx, S, g.sx, true), ty = tap_for(dy, S, g.sy, false);
    const float r0 = post_src(vae, S, c, ty.s0, tx.s0) * tx.f0 + post_src(vae, S, c, ty.s0, tx.s1) * tx.f1;
    const float r1 = post_src(vae, S, c, ty.s1, tx.s0) * tx.f0 + post_src(vae, S, c, ty.s1, tx.s1) * tx.f1;
    v = r0 * ty.f0 + r1 * ty.f1;
  }
  v = rintf(v);
  v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
  return (unsigned char)v;
}

// A table the entry could not inspect (the device copy) must never send a read outside the image: origin and extent are clamped to
// it, and the exact-2x path is taken only when the clamped extent really is twice / half of S.
__device__ __forceinline__ Geom item_geom(const dmx_edit_item& it, int H, int W, int S, bool pre) {
  Geom g;
  g.xs = min(max(it.x_s, 0), W - 1); g.ys = min(max(it.y_s, 0), H - 1);
  g.cw = min(max(it.cw, 1), W - g.xs); g.ch = min(max(it.ch, 1), H - g.ys);
  if (pre) { g.sx = it.pre_sx; g.sy = it.pre_sy; g.area2 = (it.pre_area2 && g.cw == 2 * S && g.ch == 2 * S) ? 1 : 0; }
  else { g.sx = it.post_sx; g.sy = it.post_sy; g.area2 = (it.post_area2 && S == 2 * g.cw && S == 2 * g.ch) ? 1 : 0; }
  return g;
}

// The page of an item of a paged launch (include/diffute_hip.h dmx_edit_page): dmx_edit_pages_prepare writes its index into the item,
// and like everything that comes from the device table it is clamped.
__device__ __forceinline__ int page_of(const dmx_edit_item& it, int P) { return min(max(it.reserved, 0), P - 1); }
#endif  // __HIPCC__
}  // namespace dmx_resize
