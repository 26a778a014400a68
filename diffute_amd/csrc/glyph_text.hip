// Glyph images from text on the device (reference: draw_text, app.ipynb:347-363, train_diffute_v1.py:352-368 - PIL on the host: a white
// canvas, ImageDraw.text in black).  The font is rasterised once on the host into an atlas of coverage bitmaps, text is laid out on the
// host into placements (glyph, x, y) - include/diffute_hip.h dmx_glyph_render - and composed here:
//   coverage m over the item's placements IN ORDER: m = s + round(m * (255 - s) / 255), canvas byte = 255 - m, three equal channels.
// That is Pillow's BASIC-layout ImageDraw.text bit for bit (taking the maximum, or adding, is wrong where neighbours overlap).  The
// coverage of a pixel and the checks of atlas and placements live in glyph_coverage.h, shared with the page composer (page_compose.hip).
//   dmx_glyph_render             the uint8 canvases of a ragged batch, one thread per canvas pixel.
//   dmx_glyph_text_pixel_values  placements -> the processor's fp32 batch in one launch: a block of 128 output pixels of one output row
//                                renders the few source rows x columns its taps touch as grey bytes into LDS, then every thread runs
//                                glyph_resample.h's two-pass resample on that strip - the arithmetic dmx_glyph_resize_normalize runs on
//                                the canvas in memory, so the bytes agree - and writes the three normalised channels of its one grey value.
// Integer arithmetic only: the bf16 and the fp16 build agree bit for bit.  Byte-sized and latency-bound: no MFMA, a few KB of LDS, a few
// dozen VGPRs, plain coalesced vector stores.  Everything read from a device table is clamped (placement range, glyph index, pool
// offset, table offsets, strip indices): a bad table gives wrong pixels, never an access outside the tables, the pool or the strip.
#include "common.h"
#include "kernels.h"
#include "glyph_resample.h"
#include "glyph_coverage.h"
#include <limits.h>

namespace {
constexpr int kBlock = DMX_GLYPH_TEXT_BLOCK;

using dmx_glyph::Tables;
using dmx_glyph::text_coverage;                 // glyph_coverage.h: shared with the page composer

struct TextArgs {
  Tables g;
  const dmx_glyph_text_item* items;
};

// the item's placement range, clamped to the table
__device__ __forceinline__ void text_range(const TextArgs& a, const dmx_glyph_text_item& it, int& first, int& count) {
  dmx_glyph::text_range(a.g, it.first, it.count, first, count);
}

__global__ __launch_bounds__(kBlock) void dmx_glyph_render_kernel(const TextArgs a) {
  const int bx0 = blockIdx.x * kBlock, x = bx0 + threadIdx.x, y = blockIdx.y;
  const dmx_glyph_text_item it = a.items[blockIdx.z];
  if (x >= it.W || y >= it.H) return;
  int first, count;
  text_range(a, it, first, count);
  const unsigned char v = (unsigned char)(255 - text_coverage(a.g, first, count, bx0, bx0 + kBlock, y, y + 1, x, y));
  unsigned char* dst = (unsigned char*)it.dst + (long long)y * it.stride_y + (long long)x * it.stride_x;
  dst[0] = v; dst[it.stride_c] = v; dst[2 * it.stride_c] = v;
}

struct FusedArgs {
  TextArgs t;
  const int* tab; long long table_ints; const float* norm;
  int S_h, S_w, lds_bytes; float* out; unsigned char* out_u8;
};

// offset of a pass table, or -1 (pass skipped) if it is none or the table would end past `tables`
__device__ __forceinline__ int pass_off(int off, int& taps, int n_out, long long table_ints) {
  taps = min(max(taps, 1), DMX_GLYPH_MAX_TAPS);
  return (off >= 0 && (long long)off + 2ll * n_out + (long long)n_out * taps <= table_ints) ? off : -1;
}

// columns of the strip one block may need (include/diffute_hip.h states the bound); host and device compute it alike
__host__ __device__ inline long long strip_cols_cap(int W, int S_w, int h_off, int h_taps) {
  const long long c = h_off < 0 ? kBlock : (long long)(kBlock - 1) * W / S_w + h_taps + 2;
  return c < W ? c : W;
}

__global__ __launch_bounds__(kBlock) void dmx_glyph_text_pixel_values_kernel(const FusedArgs p) {
  extern __shared__ unsigned char strip[];
  __shared__ int s_lo, s_hi;
  const int tid = threadIdx.x, ox = blockIdx.x * kBlock + tid, oy = blockIdx.y, b = blockIdx.z;
  const dmx_glyph_text_item it = p.t.items[b];
  const int H = max(it.H, 1), W = max(it.W, 1);
  dmx_glyph::Passes ps{it.h_off, it.h_taps, it.v_off, it.v_taps};
  ps.h_off = pass_off(ps.h_off, ps.h_taps, p.S_w, p.table_ints);
  ps.v_off = pass_off(ps.v_off, ps.v_taps, p.S_h, p.table_ints);
  // the source columns this block's outputs read, by the bounds glyph_resample_pixel will use
  if (tid == 0) { s_lo = INT_MAX; s_hi = 0; }
  __syncthreads();
  if (ox < p.S_w) {
    int lo = min(ox, W - 1), n = 1;
    if (ps.h_off >= 0) dmx_glyph::pass_span(p.tab, ps.h_off, ps.h_taps, ox, W, lo, n);
    atomicMin(&s_lo, lo);
    atomicMax(&s_hi, lo + max(n, 1));
  }
  __syncthreads();
  int y_lo = min(oy, H - 1), rows = 1;                                    // one output row per block: every thread reads the same rows
  if (ps.v_off >= 0) dmx_glyph::pass_span(p.tab, ps.v_off, ps.v_taps, oy, H, y_lo, rows);
  rows = min(max(rows, 1), p.lds_bytes);
  const int x_lo = min(s_lo, W - 1);
  int cols = (int)min((long long)max(s_hi - x_lo, 1), strip_cols_cap(W, p.S_w, ps.h_off, ps.h_taps));
  cols = max(min(cols, p.lds_bytes / rows), 1);                           // (the entry sized the LDS for rows * cols; a bad table cannot exceed it)
  int first, count;
  text_range(p.t, it, first, count);
  for (int i = tid; i < rows * cols; i += kBlock) {
    const int r = i / cols, c = i - r * cols;
    strip[i] = (unsigned char)(255 - text_coverage(p.t.g, first, count, x_lo, x_lo + cols, y_lo, y_lo + rows, x_lo + c, y_lo + r));
  }
  __syncthreads();
  if (ox >= p.S_w) return;
  int v[3];
  dmx_glyph::glyph_resample_pixel(
      [&](int y, int x, int) -> int { return strip[min(max(y - y_lo, 0), rows - 1) * cols + min(max(x - x_lo, 0), cols - 1)]; }, H, W, p.tab, ps,
      p.S_h, p.S_w, ox, oy, v);
  const size_t plane = (size_t)p.S_h * p.S_w, o = (size_t)b * 3 * plane + (size_t)oy * p.S_w + ox;
#pragma unroll
  for (int c = 0; c < 3; ++c) {                                           // a grey canvas: one resampled byte, the three channels' norm rows
    p.out[o + c * plane] = p.norm[c * 256 + v[0]];
    if (p.out_u8) p.out_u8[o + c * plane] = (unsigned char)v[0];
  }
}

// what both entries ask of the atlas, the items and the placements; fills `a`
int check_text(const char* what, const dmx_glyph_atlas* atlas, const dmx_glyph_text_item* items_host, const dmx_glyph_text_item* items_device,
               const dmx_glyph_placement* places_host, const dmx_glyph_placement* places_device, int n_places, int B, TextArgs& a) {
  DMX_REQUIRE(atlas && items_host && items_device, "%s: null argument", what);
  DMX_REQUIRE(B >= 1 && B <= 65535, "%s: B = %d, expected 1 .. 65535", what, B);
  const int rc = dmx_glyph::check_tables(what, atlas, places_host, places_device, n_places, a.g);
  if (rc != DMX_OK) return rc;
  for (int b = 0; b < B; ++b) {
    const dmx_glyph_text_item& it = items_host[b];
    DMX_REQUIRE(it.H >= 1 && it.H <= 65535 && it.W >= 1 && it.W <= DMX_GLYPH_TEXT_MAX_COORD, "%s: item %d: bad canvas %dx%d", what, b, it.W, it.H);
    DMX_REQUIRE(it.first >= 0 && it.count >= 0 && (long long)it.first + it.count <= n_places,
                "%s: item %d: placements [%d, %d + %d) end past the table of %d", what, b, it.first, it.first, it.count, n_places);
  }
  a.items = items_device;
  return DMX_OK;
}
}  // namespace

extern "C" int dmx_glyph_render(const dmx_glyph_atlas* atlas, const dmx_glyph_text_item* items_host, const dmx_glyph_text_item* items_device,
                                const dmx_glyph_placement* placements_host, const dmx_glyph_placement* placements_device, int n_placements, int B,
                                dmx_stream_t stream) {
  const char* what = "glyph_render";
  TextArgs a;
  const int rc = check_text(what, atlas, items_host, items_device, placements_host, placements_device, n_placements, B, a);
  if (rc != DMX_OK) return rc;
  int H = 0, W = 0;
  for (int b = 0; b < B; ++b) {
    DMX_REQUIRE(items_host[b].dst, "%s: item %d: null destination", what, b);
    H = items_host[b].H > H ? items_host[b].H : H;
    W = items_host[b].W > W ? items_host[b].W : W;
  }
  hipLaunchKernelGGL(dmx_glyph_render_kernel, dim3(cdiv(W, kBlock), H, B), dim3(kBlock), 0, (hipStream_t)stream, a);
  return dmx_check_launch("dmx_glyph_render_kernel");
}

extern "C" int dmx_glyph_text_pixel_values(const dmx_glyph_atlas* atlas, const dmx_glyph_text_item* items_host,
                                           const dmx_glyph_text_item* items_device, const dmx_glyph_placement* placements_host,
                                           const dmx_glyph_placement* placements_device, int n_placements, int B, const int* tables,
                                           long long table_ints, const float* norm, int max_taps, int S_h, int S_w, float* out_pixel_values,
                                           unsigned char* out_resized, dmx_stream_t stream) {
  const char* what = "glyph_text_pixel_values";
  DMX_REQUIRE(tables && norm && out_pixel_values, "%s: null argument", what);
  DMX_REQUIRE(S_h > 0 && S_h <= 65535 && S_w > 0 && S_w <= 65535, "%s: bad output size %dx%d", what, S_w, S_h);
  DMX_REQUIRE(max_taps >= 0 && max_taps <= DMX_GLYPH_MAX_TAPS,
              "%s: %d taps per output pixel exceed the cap of %d (downscale ratio at most 31 for bilinear, 15 for bicubic)", what, max_taps,
              DMX_GLYPH_MAX_TAPS);
  DMX_REQUIRE(table_ints >= 0 && table_ints < (1ll << 31), "%s: bad table size %lld", what, table_ints);
  FusedArgs p{};
  const int rc = check_text(what, atlas, items_host, items_device, placements_host, placements_device, n_placements, B, p.t);
  if (rc != DMX_OK) return rc;
  long long lds = 1;
  for (int b = 0; b < B; ++b) {
    const dmx_glyph_text_item& it = items_host[b];
    const struct { const char* name; int off, taps, n_in, n_out; } pass[2] = {{"horizontal", it.h_off, it.h_taps, it.W, S_w},
                                                                             {"vertical", it.v_off, it.v_taps, it.H, S_h}};
    for (const auto& q : pass) {
      if (q.n_in == q.n_out) {                                                                 // equal sizes: Pillow skips the pass
        DMX_REQUIRE(q.off < 0, "%s: item %d: the %s pass resizes %d -> %d and must be skipped (offset < 0)", what, b, q.name, q.n_in, q.n_out);
        continue;
      }
      DMX_REQUIRE(q.off >= 0 && q.taps >= 1 && q.taps <= max_taps, "%s: item %d: %s pass: offset %d, %d taps (max_taps %d)", what, b, q.name, q.off,
                  q.taps, max_taps);
      DMX_REQUIRE((long long)q.off + 2ll * q.n_out + (long long)q.n_out * q.taps <= table_ints,
                  "%s: item %d: the %s table (offset %d, %d x %d taps) ends past the %lld ints of `tables`", what, b, q.name, q.off, q.n_out, q.taps,
                  table_ints);
    }
    const long long rows = it.v_off < 0 ? 1 : (it.v_taps < it.H ? it.v_taps : it.H);
    const long long need = rows * strip_cols_cap(it.W, S_w, it.h_off, it.h_taps);
    if (need > DMX_GLYPH_TEXT_LDS_BYTES) {
      dmx_set_error("%s: item %d: a block's strip of the %dx%d canvas takes %lld bytes of LDS, the budget is %d", what, b, it.W, it.H, need,
                    DMX_GLYPH_TEXT_LDS_BYTES);
      return DMX_ERR_UNSUPPORTED;
    }
    lds = need > lds ? need : lds;
  }
  p.tab = tables; p.table_ints = table_ints; p.norm = norm; p.S_h = S_h; p.S_w = S_w; p.lds_bytes = (int)lds;
  p.out = out_pixel_values; p.out_u8 = out_resized;
  hipLaunchKernelGGL(dmx_glyph_text_pixel_values_kernel, dim3(cdiv(S_w, kBlock), S_h, B), dim3(kBlock), (size_t)lds, (hipStream_t)stream, p);
  return dmx_check_launch("dmx_glyph_text_pixel_values_kernel");
}
