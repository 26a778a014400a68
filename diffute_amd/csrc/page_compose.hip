// Synthetic document pages on the device: P ragged pages of coloured text lines over a textured background in one launch
// (include/diffute_hip.h dmx_page_compose).  The reference trains on a private set of scanned pages with OCR records
// (train_diffute_v1.py:444-489 OursDataset); here pages whose strings and boxes are known are composed from the glyph atlas.
// Per page pixel (y, x), channel c - integer arithmetic only, so the bf16 and the fp16 build agree bit for bit:
//   background  v = clip8(bg[c] + off), off = (int)(h % (2 * tex_amp + 1)) - tex_amp, with the 32-bit counter hash (mod 2^32)
//                 h = tex_seed + 0x9E3779B1 * y + 0x85EBCA77 * x + 0xC2B2AE3D * c
//                 h ^= h >> 16;  h *= 0x7FEB352D;  h ^= h >> 15;  h *= 0x846CA68B;  h ^= h >> 16
//   lines       in table order: m = the line's coverage (glyph_coverage.h: in-order composite of its placements), then
//                 v = DIV255(v * (255 - m) + rgb[c] * m),  DIV255(t) = ((u >> 8) + u) >> 8 with u = t + 128
//               - Pillow's masked fill (Paste.c fill_mask_L / BLEND8): ONE rounding of the sum, not two rounded products.
//   store       three plain byte stores through the page's strides.
// One thread per page pixel, grid (column block, row, page), the block of the text renderer.  A line whose box misses the block's
// pixels is skipped on a block-uniform branch, then a glyph whose bitmap misses them: a pixel looks into the few bitmaps near it.
// Byte-sized and latency-bound: no LDS, no MFMA.  Everything read from a device table is clamped (line range, placement range, glyph
// index, pool offset, colours, tex_amp): a bad device table gives wrong pixels, never an access outside the tables and the pool.
#include "common.h"
#include "kernels.h"
#include "glyph_coverage.h"

namespace {
constexpr int kBlock = DMX_GLYPH_TEXT_BLOCK;

struct PageArgs {
  dmx_glyph::Tables g;
  const dmx_page_rec* pages;
  const dmx_page_line* lines; int n_lines;
};

__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }

__device__ __forceinline__ unsigned tex_hash(unsigned seed, unsigned y, unsigned x, unsigned c) {
  unsigned h = seed + 0x9E3779B1u * y + 0x85EBCA77u * x + 0xC2B2AE3Du * c;
  h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
  return h;
}

__global__ __launch_bounds__(kBlock) void dmx_page_compose_kernel(const PageArgs a) {
  const int bx0 = blockIdx.x * kBlock, x = bx0 + threadIdx.x, y = blockIdx.y;
  const dmx_page_rec pg = a.pages[blockIdx.z];
  if (x >= pg.W || y >= pg.H) return;
  const int amp = clip8(pg.tex_amp);
  int v[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int off = amp ? (int)(tex_hash(pg.tex_seed, (unsigned)y, (unsigned)x, (unsigned)c) % (unsigned)(2 * amp + 1)) - amp : 0;
    v[c] = clip8(clip8(pg.bg[c]) + off);
  }
  const int l0 = min(max(pg.first_line, 0), a.n_lines), nl = min(max(pg.n_lines, 0), a.n_lines - l0);
  for (int l = 0; l < nl; ++l) {
    const dmx_page_line ln = a.lines[l0 + l];
    if (ln.x1 <= bx0 || ln.x0 >= bx0 + kBlock || ln.y1 <= y || ln.y0 > y) continue;      // block-uniform: the whole block sits on row y
    int first, count;
    dmx_glyph::text_range(a.g, ln.first, ln.count, first, count);
    const int m = dmx_glyph::text_coverage(a.g, first, count, bx0, bx0 + kBlock, y, y + 1, x, y);
    if (m == 0) continue;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int u = v[c] * (255 - m) + clip8(ln.rgb[c]) * m + 128;
      v[c] = ((u >> 8) + u) >> 8;
    }
  }
  unsigned char* dst = (unsigned char*)pg.dst + (long long)y * pg.stride_y + (long long)x * pg.stride_x;
  dst[0] = (unsigned char)v[0]; dst[pg.stride_c] = (unsigned char)v[1]; dst[2 * pg.stride_c] = (unsigned char)v[2];
}
}  // namespace

extern "C" int dmx_page_compose(const dmx_glyph_atlas* atlas, const dmx_page_rec* pages_host, const dmx_page_rec* pages_device, int P,
                                const dmx_page_line* lines_host, const dmx_page_line* lines_device, int n_lines_total,
                                const dmx_glyph_placement* placements_host, const dmx_glyph_placement* placements_device, int n_placements,
                                dmx_stream_t stream) {
  const char* what = "page_compose";
  DMX_REQUIRE(atlas && pages_host && pages_device, "%s: null argument", what);
  DMX_REQUIRE(P >= 1 && P <= 65535, "%s: P = %d, expected 1 .. 65535", what, P);
  DMX_REQUIRE(n_lines_total >= 0 && (n_lines_total == 0 || (lines_host && lines_device)), "%s: %d lines but no line table", what, n_lines_total);
  PageArgs a{};
  const int rc = dmx_glyph::check_tables(what, atlas, placements_host, placements_device, n_placements, a.g);
  if (rc != DMX_OK) return rc;
  for (int l = 0; l < n_lines_total; ++l) {
    const dmx_page_line& ln = lines_host[l];
    DMX_REQUIRE(ln.first >= 0 && ln.count >= 0 && (long long)ln.first + ln.count <= n_placements,
                "%s: line %d: placements [%d, %d + %d) end past the table of %d", what, l, ln.first, ln.first, ln.count, n_placements);
    for (int c = 0; c < 3; ++c) DMX_REQUIRE(ln.rgb[c] >= 0 && ln.rgb[c] <= 255, "%s: line %d: ink %d of channel %d is no byte", what, l, ln.rgb[c], c);
    for (int i = ln.first; i < ln.first + ln.count; ++i) {                                  // the box is used for rejection: it must hold the bitmaps
      const dmx_glyph_placement& p = placements_host[i];
      const dmx_glyph_rec& g = atlas->glyphs_host[p.glyph];
      DMX_REQUIRE(g.w == 0 || g.h == 0 || (p.x >= ln.x0 && p.y >= ln.y0 && (long long)p.x + g.w <= ln.x1 && (long long)p.y + g.h <= ln.y1),
                  "%s: line %d: the bitmap of placement %d (%dx%d at %d, %d) leaves the line's box [%d, %d) x [%d, %d)", what, l, i, g.w, g.h, p.x,
                  p.y, ln.x0, ln.x1, ln.y0, ln.y1);
    }
  }
  int H = 0, W = 0;
  for (int p = 0; p < P; ++p) {
    const dmx_page_rec& pg = pages_host[p];
    DMX_REQUIRE(pg.dst, "%s: page %d: null destination", what, p);
    DMX_REQUIRE(pg.H >= 1 && pg.H <= 65535 && pg.W >= 1 && pg.W <= DMX_GLYPH_TEXT_MAX_COORD, "%s: page %d: bad size %dx%d", what, p, pg.W, pg.H);
    DMX_REQUIRE(pg.first_line >= 0 && pg.n_lines >= 0 && (long long)pg.first_line + pg.n_lines <= n_lines_total,
                "%s: page %d: lines [%d, %d + %d) end past the table of %d", what, p, pg.first_line, pg.first_line, pg.n_lines, n_lines_total);
    DMX_REQUIRE(pg.tex_amp >= 0 && pg.tex_amp <= 255, "%s: page %d: tex_amp %d, expected 0 .. 255", what, p, pg.tex_amp);
    for (int c = 0; c < 3; ++c) DMX_REQUIRE(pg.bg[c] >= 0 && pg.bg[c] <= 255, "%s: page %d: background %d of channel %d is no byte", what, p, pg.bg[c], c);
    H = pg.H > H ? pg.H : H;
    W = pg.W > W ? pg.W : W;
  }
  a.pages = pages_device; a.lines = lines_device; a.n_lines = n_lines_total;
  hipLaunchKernelGGL(dmx_page_compose_kernel, dim3(cdiv(W, kBlock), H, P), dim3(kBlock), 0, (hipStream_t)stream, a);
  return dmx_check_launch("dmx_page_compose_kernel");
}
