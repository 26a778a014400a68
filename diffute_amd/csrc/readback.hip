// OCR read-back of edited text boxes (reference: app.ipynb:842-846 - crop inf_res[y1:y2, x1:x2], run the processor, call generate):
// from the decoder outputs of K candidates per box straight to the `pixel_values` the OCR encoder reads, in ONE launch.  Row (b, k) is,
// bit for bit, what dmx_glyph_resize_normalize makes of the slice [y1:y2, x1:x2] of the page dmx_postprocess_paste writes for
// image_vae[b][k] ALONE over the original image - but neither the page nor the slice exists: a source byte at page position (X, Y) is
//   post_pixel(...) of that candidate   where (X, Y) lies inside item b's clipped crop extent (inside its box it does by construction),
//   the original byte                   elsewhere (a box wider than its crop keeps original pixels there, as the slice would).
// The per-pixel arithmetic is shared, not restated: prepost_resize.h (post_pixel, item_geom's clamps) for the paste and glyph_resample.h
// (Pillow's integer two-pass resample) for the processor; the library is built with -ffp-contract=off, so the shared fp32 expressions
// round alike in every kernel.  Pure byte work on a few thousand pixels per box: launch- and HBM-latency-bound, one thread per
// destination pixel, coalesced plain vector stores, no uint8 intermediate in HBM.
// ONE kernel body over a page source (prepost_paste.h), instantiated for the boxes of one image (OnePage) and for boxes on several pages
// (PageTable: the item's page - its index travels in the item, clamped - supplies the image pointer, H and W).
#include "common.h"
#include "kernels.h"
#include "prepost_paste.h"
#include "prepost_resize.h"
#include "glyph_resample.h"

namespace {
using namespace dmx_resize;
using dmx_paste::OnePage;
using dmx_paste::PageTable;

struct ReadbackArgs {
  const float* vae; int S;                                 // decoder outputs [B][K][3][S][S] in [-1, 1]
  const dmx_edit_item* items; const dmx_readback_pass* passes; int B, K;
  const int* tab; const float* norm;
  int S_h, S_w; float* out; unsigned char* out_u8;         // [B*K][3][S_h][S_w]
};

// Output pixel (ox, oy) of row r = b * K + k: item `it` = p.items[b] on its page pg (the original, HWC uint8).
__device__ __forceinline__ void readback_row(const ReadbackArgs& p, const dmx_edit_page& pg, const dmx_edit_item& it, int r, int ox, int oy) {
  const int b = r / p.K, H = pg.H, W = pg.W;
  const unsigned char* ori = (const unsigned char*)pg.original;
  const dmx_readback_pass ps = p.passes[b];
  // everything that comes from the device table is clamped: the box to the image (at least one pixel), the crop by item_geom
  const int x1 = min(max(it.x1, 0), W - 1), y1 = min(max(it.y1, 0), H - 1);
  const int bw = min(max(it.x2 - x1, 1), W - x1), bh = min(max(it.y2 - y1, 1), H - y1);
  const Geom g = item_geom(it, H, W, p.S, false);
  const float* vae = p.vae + (size_t)r * 3 * p.S * p.S;
  auto px = [&](int y, int x, int c) -> int {                                                  // byte (x, y) of the box slice of the pasted page
    const int X = x1 + x, Y = y1 + y, dx = X - g.xs, dy = Y - g.ys;
    if (dx >= 0 && dx < g.cw && dy >= 0 && dy < g.ch) return post_pixel(vae, p.S, g, c, dx, dy);
    return ori[((size_t)Y * W + X) * 3 + c];
  };
  const dmx_glyph::Passes tp{ps.h_off, ps.h_taps, ps.v_off, ps.v_taps};
  int v[3];
  dmx_glyph::glyph_resample_pixel(px, bh, bw, p.tab, tp, p.S_h, p.S_w, ox, oy, v);
  const size_t plane = (size_t)p.S_h * p.S_w, o = (size_t)r * 3 * plane + (size_t)oy * p.S_w + ox;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    p.out[o + c * plane] = p.norm[c * 256 + v[c]];
    if (p.out_u8) p.out_u8[o + c * plane] = (unsigned char)v[c];
  }
}

// grid (ceil(S_w / 128), S_h, B * K)
template <class Pages>
__global__ __launch_bounds__(128) void dmx_readback_boxes_kernel(const ReadbackArgs p, const Pages pages) {
  const int ox = blockIdx.x * blockDim.x + threadIdx.x, oy = blockIdx.y, r = blockIdx.z;       // r = b * K + k
  if (ox >= p.S_w) return;
  const dmx_edit_item it = p.items[r / p.K];
  readback_row(p, pages.of(it), it, r, ox, oy);
}

// The launch; the tables are checked.  `kernel` names it in the last-error string.
template <class Pages>
int launch_readback(const char* kernel, const Pages& pages, const float* image_vae, int S, const dmx_edit_item* items_device, int B, int K,
                    const int* tables, const float* norm, const dmx_readback_pass* passes_device, int S_h, int S_w, float* out_pixel_values,
                    unsigned char* out_resized, dmx_stream_t stream) {
  ReadbackArgs p{image_vae, S, items_device, passes_device, B, K, tables, norm, S_h, S_w, out_pixel_values, out_resized};
  hipLaunchKernelGGL(dmx_readback_boxes_kernel<Pages>, dim3(cdiv(S_w, 128), S_h, B * K), dim3(128), 0, (hipStream_t)stream, p, pages);
  return dmx_check_launch(kernel);
}

// what the read-back asks of the boxes [lo, hi) beyond dmx_check_edit_items: a non-empty box inside the H x W page, and of each one's passes
// what dmx_check_readback_item asks at the box's size
int check_readback_boxes(const char* what, const dmx_edit_item* items_host, const dmx_readback_pass* passes_host, int lo, int hi, int H, int W,
                         int max_taps, long long table_ints, int S_h, int S_w) {
  for (int b = lo; b < hi; ++b) {
    const dmx_edit_item& it = items_host[b];
    DMX_REQUIRE(it.x2 > it.x1 && it.y2 > it.y1, "%s: item %d: empty box (%d, %d, %d, %d)", what, b, it.x1, it.y1, it.x2, it.y2);
    DMX_REQUIRE(it.x1 >= 0 && it.y1 >= 0 && it.x2 <= W && it.y2 <= H, "%s: item %d: box (%d, %d, %d, %d) outside the %dx%d image", what, b, it.x1,
                it.y1, it.x2, it.y2, W, H);
    const int rc = dmx_check_readback_item(what, b, passes_host[b], it.x2 - it.x1, it.y2 - it.y1, max_taps, table_ints, S_h, S_w);
    if (rc != DMX_OK) return rc;
  }
  return DMX_OK;
}
}  // namespace

// The pass tables of item b, whose source - a box's slice, a quad's strip - is src_w x src_h: inside `tables`, and skipped where the sizes
// are equal
int dmx_check_readback_item(const char* what, int b, const dmx_readback_pass& ps, int src_w, int src_h, int max_taps, long long table_ints, int S_h,
                            int S_w) {
  const struct { const char* name; int off, taps, n_in, n_out; } pass[2] = {{"horizontal", ps.h_off, ps.h_taps, src_w, S_w},
                                                                           {"vertical", ps.v_off, ps.v_taps, src_h, S_h}};
  for (const auto& q : pass) {
    if (q.n_in == q.n_out) {                                                                   // equal sizes: Pillow skips the pass
      DMX_REQUIRE(q.off < 0, "%s: item %d: the %s pass resizes %d -> %d and must be skipped (offset < 0)", what, b, q.name, q.n_in, q.n_out);
      continue;
    }
    DMX_REQUIRE(q.off >= 0 && q.taps >= 1 && q.taps <= max_taps, "%s: item %d: %s pass: offset %d, %d taps (max_taps %d)", what, b, q.name, q.off,
                q.taps, max_taps);
    DMX_REQUIRE((long long)q.off + 2ll * q.n_out + (long long)q.n_out * q.taps <= table_ints,
                "%s: item %d: the %s table (offset %d, %d x %d taps) ends past the %lld ints of `tables`", what, b, q.name, q.off, q.n_out, q.taps,
                table_ints);
  }
  return DMX_OK;
}

// the scalar arguments every read-back entry shares (boxes here, quads in prepost_quad.hip)
int dmx_check_readback_scalars(const char* what, int K, int max_taps, long long table_ints, int S_h, int S_w) {
  DMX_REQUIRE(K >= 1 && K <= DMX_SELECT_MAX_CANDIDATES, "%s: %d candidates per box, expected 1 .. %d", what, K, DMX_SELECT_MAX_CANDIDATES);
  DMX_REQUIRE(S_h > 0 && S_h <= 65535 && S_w > 0 && S_w <= 65535, "%s: bad output size %dx%d", what, S_w, S_h);
  DMX_REQUIRE(max_taps >= 0 && max_taps <= DMX_GLYPH_MAX_TAPS,
              "%s: %d taps per output pixel exceed the cap of %d (downscale ratio at most 31 for bilinear, 15 for bicubic)", what, max_taps,
              DMX_GLYPH_MAX_TAPS);
  DMX_REQUIRE(table_ints >= 0 && table_ints < (1ll << 31), "%s: bad table size %lld", what, table_ints);
  return DMX_OK;
}

extern "C" int dmx_readback_pixel_values(const float* image_vae, int S, const unsigned char* original_hwc, int H, int W,
                                         const dmx_edit_item* items_host, const dmx_edit_item* items_device, int B, int K, const int* tables,
                                         long long table_ints, const float* norm, const dmx_readback_pass* passes_host,
                                         const dmx_readback_pass* passes_device, int max_taps, int S_h, int S_w, float* out_pixel_values,
                                         unsigned char* out_resized, dmx_stream_t stream) {
  const char* what = "readback_pixel_values";
  DMX_REQUIRE(image_vae && original_hwc && items_device && tables && norm && passes_host && passes_device && out_pixel_values, "%s: null argument", what);
  int rc = dmx_check_readback_scalars(what, K, max_taps, table_ints, S_h, S_w);
  if (rc == DMX_OK) rc = dmx_check_edit_items(what, items_host, B, H, W, S, true);
  if (rc == DMX_OK) rc = check_readback_boxes(what, items_host, passes_host, 0, B, H, W, max_taps, table_ints, S_h, S_w);
  if (rc != DMX_OK) return rc;
  return launch_readback("dmx_readback_pixel_values_kernel", OnePage{original_hwc, nullptr, nullptr, H, W}, image_vae, S, items_device, B, K, tables, norm,
                         passes_device, S_h, S_w, out_pixel_values, out_resized, stream);
}

extern "C" int dmx_readback_pixel_values_pages(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                               const dmx_edit_item* items_host, const dmx_edit_item* items_device, int B, int K, const int* tables,
                                               long long table_ints, const float* norm, const dmx_readback_pass* passes_host,
                                               const dmx_readback_pass* passes_device, int max_taps, int S_h, int S_w, float* out_pixel_values,
                                               unsigned char* out_resized, dmx_stream_t stream) {
  const char* what = "readback_pixel_values_pages";
  DMX_REQUIRE(image_vae && pages_device && items_device && tables && norm && passes_host && passes_device && out_pixel_values, "%s: null argument", what);
  DMX_REQUIRE(S > 0 && S <= 65535, "%s: bad S = %d", what, S);
  int rc = dmx_check_readback_scalars(what, K, max_taps, table_ints, S_h, S_w);
  if (rc == DMX_OK) rc = dmx_check_edit_pages(what, pages_host, P, items_host, B, S, true);
  if (rc != DMX_OK) return rc;
  for (int q = 0; q < P; ++q) {
    const dmx_edit_page& pg = pages_host[q];
    DMX_REQUIRE(pg.original, "%s: page %d: null original image", what, q);
    rc = check_readback_boxes(what, items_host, passes_host, pg.item_lo, pg.item_hi, pg.H, pg.W, max_taps, table_ints, S_h, S_w);
    if (rc != DMX_OK) return rc;
  }
  return launch_readback("dmx_readback_pages_kernel", PageTable{pages_device, P}, image_vae, S, items_device, B, K, tables, norm, passes_device, S_h, S_w,
                         out_pixel_values, out_resized, stream);
}
