// The geometry of quadrilateral text regions with oriented crops, stated once: the host half (what dmx_edit_quads_prepare fills into a
// dmx_edit_quad) and the per-pixel arithmetic of the three kernels of prepost_quad.hip in their similarity frame (the projective frame's
// coordinates are prepost_persp.h).  tests/quad_restatement.py restates this comment in numpy and the GPU tests compare bit for bit.
// Everything a kernel reads from the table is an integer.
//
// Quad.  Corners k = 0..3 with integer page coordinates (x_k, y_k) in the OCR record's order - top-left, top-right, bottom-right,
//   bottom-left of the text as read -, clockwise with y down.  Pixel (X, Y) is inside iff all four edge functions
//     E_k = (x_{k+1} - x_k) * (Y - y_k) - (y_{k+1} - y_k) * (X - x_k)        (k + 1 taken mod 4; 64-bit integers)
//   are >= 0: edges included.  For the axis-aligned quad (x1,y1) (x2,y1) (x2,y2) (x1,y2) that is generate_mask's inclusive rectangle.
//   The SAME predicate decides the mask and the paste - a deliberate deviation from the reference, which masks the inclusive box but
//   pastes the half-open slice [y1:y2, x1:x2]: a quad has no "slice", and pasting what was masked leaves no blacked-out rim unpainted.
//   A quad is accepted when every turn e_k x e_{k+1} = ex_k * ey_{k+1} - ey_k * ex_{k+1} is >= 0 and twice its area (their shoelace sum)
//   is > 0: convex, clockwise, not flat.
//
// Frame (the oriented crop).  Integers: centre (cx2, cy2) in half-pixels of pixel-index space (pixel X has its centre at 2X), side
//   crop_scale in page pixels, baseline direction (ux, uy).  With n = sqrt((double)(ux*ux + uy*uy)) and rn = round-half-even (rint),
//   all in double and in exactly this order of operations (the integer products are exact in a double),
//     a  = rn((crop_scale * ux * 32768.0) / (n * S))      c  = rn((crop_scale * uy * 32768.0) / (n * S))      b  = -c    d  = a
//     ia = rn((S * ux * 32768.0) / (n * crop_scale))      ib = rn((S * uy * 32768.0) / (n * crop_scale))      ic = -ib   id = ia
//   (Q15).  Crop pixel (dx, dy), 0 <= dx, dy < S, samples the page at the Q16 coordinates
//     X16 = (cx2 << 15) + a * (2dx + 1 - S) + b * (2dy + 1 - S)
//     Y16 = (cy2 << 15) + c * (2dx + 1 - S) + d * (2dy + 1 - S)                                                (64-bit)
//   Taps: i0 = X16 >> 16 (floor) and i0 + 1, EACH clamped to the page (border replicated); f = X16 & 65535, weights 65536 - f and f.
//   A channel's byte is (sum over the four taps of w_x * w_y * v + 2^31) >> 32 in 64-bit: four products, ONE rounding.  (Rounding the
//   horizontal pass before the vertical one, or keeping fewer fraction bits, makes the result depend on which axis came first: a page
//   turned by 90 degrees, quad and frame turned along, would no longer give the same crop.  With one rounding of the full-precision sum
//   it does, bit for bit.)  image: v = the page byte; masked image: v = 0 at a tap (after the clamp) inside the quad - blacked out
//   BEFORE resampling, as pre_pixel does -; mask: v = the predicate at the tap, so the byte is 0 or 1.  Stores: pre_store
//   (prepost_resize.h): normalised fp32 planes, the mask byte, the latent mask = every 8th mask pixel.
//
// Paste.  Page pixel (X, Y) has the crop coordinates (Q16, pixel-index space of the S x S decoder output)
//     U16 = ((S - 1) << 15) + ia * (2X - cx2) + ib * (2Y - cy2)
//     V16 = ((S - 1) << 15) + ic * (2X - cx2) + id * (2Y - cy2)                                                (64-bit)
//   Among the items of the pixel's page, the LAST one whose quad covers the pixel decides: the pixel is pasted iff
//   -2^15 <= U16, V16 < (S << 16) - 2^15 for that item (it lies on the crop), and is the original byte otherwise, as is every pixel no
//   quad covers.  The union mask is 1 where any quad covers the pixel.  Value: taps as above on the S x S image; post_src (prepost_resize.h)
//   at each tap; fp32, horizontal first - r = s0 * w0 + s1 * w1 with w1 = f / 65536, w0 = (65536 - f) / 65536 (exact in fp32) -, then
//   vertical alike; rintf; clamp to [0, 255].  The build's -ffp-contract=off keeps every product and sum rounded on its own.
//
// Rectify.  u = (TR - TL) + (BR - BL), v = (BL - TL) + (BR - TR); the strip is rw x rh with rw = rn(sqrt(u.u) / 2) + 1,
//   rh = rn(sqrt(v.v) / 2) + 1.  ra = rn((ux * 32768.0) / n), rc = rn((uy * 32768.0) / n), rb = -rc, rd = ra with n = sqrt(u.u): scale 1
//   along u.  The centre is the corner mean held in quarter-pixels, sx4 = sum of x_k, sy4 = sum of y_k.  Strip pixel (i, j) samples
//     X16 = (sx4 << 14) + ra * (2i + 1 - rw) + rb * (2j + 1 - rh),    Y16 = (sy4 << 14) + rc * (2i + 1 - rw) + rd * (2j + 1 - rh)
//   with the tap rule and the single rounding of the frame.  An axis-aligned quad yields exactly page[y1:y2+1, x1:x2+1].
#pragma once
#include <math.h>
#include <stddef.h>
#include <string.h>
#include "kernels.h"
#include "prepost_resize.h"

namespace dmx_quad {
inline int rn_ratio(double num, double den) { return (int)rint(num / den); }

// The derived fields of one quad, from its caller-filled ones; rect_off / rect_block_lo are the running sums over the items before it.
// The caller has validated the quad (prepost_quad.hip check_quads): nothing here divides by zero or leaves an int.
inline void fill_derived(dmx_edit_quad& q, int S, long long rect_off, int rect_block_lo) {
  const double n = sqrt((double)((long long)q.ux * q.ux + (long long)q.uy * q.uy));
  const int a = rn_ratio((double)q.crop_scale * q.ux * 32768.0, n * S), c = rn_ratio((double)q.crop_scale * q.uy * 32768.0, n * S);
  const int ia = rn_ratio((double)S * q.ux * 32768.0, n * q.crop_scale), ib = rn_ratio((double)S * q.uy * 32768.0, n * q.crop_scale);
  q.fwd[0] = a; q.fwd[1] = -c; q.fwd[2] = c; q.fwd[3] = a;
  q.inv[0] = ia; q.inv[1] = ib; q.inv[2] = -ib; q.inv[3] = ia;
  q.bx1 = q.bx2 = q.x[0]; q.by1 = q.by2 = q.y[0];
  for (int k = 0; k < 4; ++k) {
    q.ex[k] = q.x[(k + 1) & 3] - q.x[k]; q.ey[k] = q.y[(k + 1) & 3] - q.y[k];
    q.bx1 = q.x[k] < q.bx1 ? q.x[k] : q.bx1; q.bx2 = q.x[k] > q.bx2 ? q.x[k] : q.bx2;
    q.by1 = q.y[k] < q.by1 ? q.y[k] : q.by1; q.by2 = q.y[k] > q.by2 ? q.y[k] : q.by2;
  }
  const long long rux = (long long)(q.x[1] - q.x[0]) + (q.x[2] - q.x[3]), ruy = (long long)(q.y[1] - q.y[0]) + (q.y[2] - q.y[3]);
  const long long rvx = (long long)(q.x[3] - q.x[0]) + (q.x[2] - q.x[1]), rvy = (long long)(q.y[3] - q.y[0]) + (q.y[2] - q.y[1]);
  const double nu = sqrt((double)(rux * rux + ruy * ruy)), nv = sqrt((double)(rvx * rvx + rvy * rvy));
  q.rw = (int)rint(nu / 2.0) + 1; q.rh = (int)rint(nv / 2.0) + 1;
  const int ra = rn_ratio((double)rux * 32768.0, nu), rc = rn_ratio((double)ruy * 32768.0, nu);
  q.rect[0] = ra; q.rect[1] = -rc; q.rect[2] = rc; q.rect[3] = ra;
  q.sx4 = q.x[0] + q.x[1] + q.x[2] + q.x[3]; q.sy4 = q.y[0] + q.y[1] + q.y[2] + q.y[3];
  q.rect_block_lo = rect_block_lo; q.rect_blocks = q.rh * ((q.rw + 255) / 256);
  q.rect_off = rect_off;
}

#ifdef __HIPCC__
// what the paste scans per item, staged in LDS
struct QuadEdges { int x[4], y[4], ex[4], ey[4]; int bx1, by1, bx2, by2; };

template <class Q>
__device__ __forceinline__ int inside(const Q& q, int X, int Y) {
  int in = 1;
#pragma unroll
  for (int k = 0; k < 4; ++k) in &= ((long long)q.ex[k] * ((long long)Y - q.y[k]) - (long long)q.ey[k] * ((long long)X - q.x[k])) >= 0 ? 1 : 0;
  return in;
}

struct Tap16 { int i0, i1; long long w0, w1; };
// floor and floor + 1 of a Q16 coordinate, each clamped to [0, n - 1]; whatever the coordinate, the indices lie inside
__device__ __forceinline__ Tap16 tap16(long long c16, int n) {
  const long long fl = c16 >> 16, hi = (long long)n - 1;
  Tap16 t;
  t.i0 = (int)(fl < 0 ? 0 : (fl > hi ? hi : fl));
  t.i1 = (int)(fl + 1 < 0 ? 0 : (fl + 1 > hi ? hi : fl + 1));
  t.w1 = c16 & 65535; t.w0 = 65536 - t.w1;
  return t;
}
__device__ __forceinline__ int round32(long long acc) { return (int)((acc + (1ll << 31)) >> 32); }

// The three bytes-to-be of one destination pixel that samples the H x W page at (X16, Y16): image (vi), image with the quad blacked out
// before resampling (vm), mask (vk).  in(X, Y) -> {0, 1}.
template <class In>
__device__ __forceinline__ void pre_pixel(const unsigned char* img, int H, int W, long long X16, long long Y16, In in, int vi[3], int vm[3], int& vk) {
  const Tap16 tx = tap16(X16, W), ty = tap16(Y16, H);
  const long long w00 = ty.w0 * tx.w0, w01 = ty.w0 * tx.w1, w10 = ty.w1 * tx.w0, w11 = ty.w1 * tx.w1;
  const int m00 = in(tx.i0, ty.i0), m01 = in(tx.i1, ty.i0), m10 = in(tx.i0, ty.i1), m11 = in(tx.i1, ty.i1);
  const unsigned char *r0 = img + (size_t)ty.i0 * W * 3, *r1 = img + (size_t)ty.i1 * W * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const long long s00 = r0[tx.i0 * 3 + c], s01 = r0[tx.i1 * 3 + c], s10 = r1[tx.i0 * 3 + c], s11 = r1[tx.i1 * 3 + c];
    vi[c] = round32(w00 * s00 + w01 * s01 + w10 * s10 + w11 * s11);
    vm[c] = round32(w00 * (m00 ? 0 : s00) + w01 * (m01 ? 0 : s01) + w10 * (m10 ? 0 : s10) + w11 * (m11 ? 0 : s11));
  }
  vk = round32(w00 * m00 + w01 * m01 + w10 * m10 + w11 * m11);
}
// The single-rounding bilinear of four taps: at(kx, ky) -> the byte at tap (kx ? tx.i1 : tx.i0, ky ? ty.i1 : ty.i0).  Integers: exact
// whatever the order of the sum.
template <class At>
__device__ __forceinline__ int sample4(const Tap16& tx, const Tap16& ty, At at) {
  return round32(ty.w0 * tx.w0 * at(0, 0) + ty.w0 * tx.w1 * at(1, 0) + ty.w1 * tx.w0 * at(0, 1) + ty.w1 * tx.w1 * at(1, 1));
}
// one channel of the page itself at (X16, Y16): the rectified strip
__device__ __forceinline__ int page_sample(const unsigned char* img, int W, const Tap16& tx, const Tap16& ty, int c) {
  const unsigned char *r0 = img + (size_t)ty.i0 * W * 3, *r1 = img + (size_t)ty.i1 * W * 3;
  return sample4(tx, ty, [&](int kx, int ky) -> long long { return (ky ? r1 : r0)[(kx ? tx.i1 : tx.i0) * 3 + c]; });
}

// Channel c of the decoder output vae [3][S][S] at the crop coordinates (U16, V16), as the byte that is pasted
__device__ __forceinline__ unsigned char post_pixel(const float* vae, int S, int c, long long U16, long long V16) {
  using dmx_resize::post_src;
  const Tap16 tx = tap16(U16, S), ty = tap16(V16, S);
  const float fx0 = (float)tx.w0 / 65536.f, fx1 = (float)tx.w1 / 65536.f, fy0 = (float)ty.w0 / 65536.f, fy1 = (float)ty.w1 / 65536.f;
  const float r0 = post_src(vae, S, c, ty.i0, tx.i0) * fx0 + post_src(vae, S, c, ty.i0, tx.i1) * fx1;
  const float r1 = post_src(vae, S, c, ty.i1, tx.i0) * fx0 + post_src(vae, S, c, ty.i1, tx.i1) * fx1;
  float v = rintf(r0 * fy0 + r1 * fy1);
  v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
  return (unsigned char)v;
}
#endif  // __HIPCC__
}  // namespace dmx_quad
