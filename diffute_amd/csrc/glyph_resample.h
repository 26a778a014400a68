// Pillow's 8-bit two-pass resample for ONE destination pixel, stated once: the glyph kernel of prepost.hip (source = an image in memory,
// read through its strides) and the read-back kernel of readback.hip (source = a text box of the page a paste WOULD write, computed on
// the fly) both call glyph_resample_pixel below, so their bytes agree bit for bit.  Integer MACs and table look-ups only:
//   horizontal pass first: h = clip8((2^21 + sum pixel * k) >> 22) kept as a BYTE, the vertical pass runs on those bytes; a pass whose
//   input and output size are equal is skipped (table offset < 0).
// The thread recomputes the horizontally-resampled bytes its vertical taps need.
#pragma once
#include "kernels.h"

namespace dmx_glyph {
#ifdef __HIPCC__
__device__ __forceinline__ int clip8(int v) { v >>= 22; return v < 0 ? 0 : (v > 255 ? 255 : v); }

// One pass table set of one source image: offsets (in ints) into `tab`, < 0 = pass skipped; taps = coefficient row length.
struct Passes { int h_off, h_taps, v_off, v_taps; };

// The source span [lo, lo + n) that output index o of one pass (table at `off`, not skipped) reads, clamped to the `src` source pixels.
// glyph_resample_pixel reads its bounds through this; a kernel that stages source pixels first (glyph_text.hip) asks it what to stage.
__device__ __forceinline__ void pass_span(const int* tab, int off, int taps, int o, int src, int& lo, int& n) {
  const int* t = tab + off;
  lo = min(max(t[2 * o], 0), src - 1); n = min(min(t[2 * o + 1], taps), min(src - lo, DMX_GLYPH_MAX_TAPS));
}

// Destination pixel (ox, oy) of an S_h x S_w output from a src_h x src_w source; px(y, x, c) -> the source byte.  The tables come
// from device memory the entry cannot inspect: every bound is clamped to the source, so a bad table reads wrong pixels, never outside.
template <class Px>
__device__ __forceinline__ void glyph_resample_pixel(Px px, int src_h, int src_w, const int* tab, const Passes& d, int S_h, int S_w,
                                                     int ox, int oy, int v[3]) {
  int xmin = ox, xn = 1, ymin = oy, yn = 1;
  const int *kh = nullptr, *kv = nullptr;
  if (d.h_off >= 0) {
    pass_span(tab, d.h_off, d.h_taps, ox, src_w, xmin, xn);
    kh = tab + d.h_off + 2 * S_w + (size_t)ox * d.h_taps;
  } else xmin = min(xmin, src_w - 1);
  if (d.v_off >= 0) {
    pass_span(tab, d.v_off, d.v_taps, oy, src_h, ymin, yn);
    kv = tab + d.v_off + 2 * S_h + (size_t)oy * d.v_taps;
  } else ymin = min(ymin, src_h - 1);
  int acc[3] = {1 << 21, 1 << 21, 1 << 21}, h[3] = {0, 0, 0};
  for (int j = 0; j < yn; ++j) {
    if (kh) {
      int s[3] = {1 << 21, 1 << 21, 1 << 21};
      for (int i = 0; i < xn; ++i) {
        const int k = kh[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += px(ymin + j, xmin + i, c) * k;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) h[c] = clip8(s[c]);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) h[c] = px(ymin + j, xmin, c);
    }
    if (kv) {
      const int k = kv[j];
#pragma unroll
      for (int c = 0; c < 3; ++c) acc[c] += h[c] * k;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = kv ? clip8(acc[c]) : h[c];
}
#endif  // __HIPCC__
}  // namespace dmx_glyph
