// The coverage of one pixel under a run of glyph placements, shared by the text renderer (glyph_text.hip) and the page composer
// (page_compose.hip): m over the placements IN ORDER, m = s + round(m * (255 - s) / 255) - Pillow's BASIC-layout text mask bit for bit.
// Integer arithmetic only.  Everything read from a device table is clamped (placement range, glyph index, pool offset).
#pragma once
#include "common.h"
#include "kernels.h"

namespace dmx_glyph {
// the atlas and the placement table as a kernel reads them
struct Tables {
  const unsigned char* pool; long long pool_bytes;
  const dmx_glyph_rec* glyphs; int n_glyphs;
  const dmx_glyph_placement* places; int n_places;
};

// Pillow's MULDIV255: round(a * b / 255) for bytes a, b
__device__ __forceinline__ int muldiv255(int a, int b) { const int t = a * b + 128; return ((t >> 8) + t) >> 8; }

// a placement range, clamped to the table
__device__ __forceinline__ void text_range(const Tables& a, int it_first, int it_count, int& first, int& count) {
  first = min(max(it_first, 0), a.n_places);
  count = min(max(it_count, 0), a.n_places - first);
}

// Coverage of canvas pixel (x, y) under placements [first, first + count).  [bx0, bx1) x [by0, by1) holds every pixel the BLOCK asks for:
// a glyph that misses it is skipped on a block-uniform branch, so a pixel only looks into the few bitmaps near it.
__device__ __forceinline__ int text_coverage(const Tables& a, int first, int count, int bx0, int bx1, int by0, int by1, int x, int y) {
  int m = 0;
  for (int i = 0; i < count; ++i) {
    const dmx_glyph_placement p = a.places[first + i];
    const dmx_glyph_rec g = a.glyphs[min(max(p.glyph, 0), a.n_glyphs - 1)];
    if ((long long)p.x + g.w <= bx0 || p.x >= bx1 || (long long)p.y + g.h <= by0 || p.y >= by1) continue;
    const long long lx = (long long)x - p.x, ly = (long long)y - p.y;
    if (lx < 0 || lx >= g.w || ly < 0 || ly >= g.h) continue;
    const long long o = min(max((long long)g.off + ly * g.w + lx, 0ll), a.pool_bytes - 1);
    const int s = a.pool[o];
    m = s + muldiv255(m, 255 - s);
  }
  return m;
}

// what every entry asks of the atlas and the placements (host copies); fills `a` with the device side
inline int check_tables(const char* what, const dmx_glyph_atlas* atlas, const dmx_glyph_placement* places_host,
                        const dmx_glyph_placement* places_device, int n_places, Tables& a) {
  DMX_REQUIRE(atlas, "%s: null argument", what);
  DMX_REQUIRE(atlas->pool && atlas->glyphs_host && atlas->glyphs_device, "%s: null atlas table", what);
  DMX_REQUIRE(atlas->n_glyphs >= 1 && atlas->pool_bytes >= 1 && atlas->pool_bytes < (1ll << 31), "%s: bad atlas (%d glyphs, %lld pool bytes)", what,
              atlas->n_glyphs, atlas->pool_bytes);
  DMX_REQUIRE(n_places >= 0 && (n_places == 0 || (places_host && places_device)), "%s: %d placements but no placement table", what, n_places);
  for (int g = 0; g < atlas->n_glyphs; ++g) {
    const dmx_glyph_rec& r = atlas->glyphs_host[g];
    DMX_REQUIRE(r.off >= 0 && r.w >= 0 && r.h >= 0 && r.w <= 65535 && r.h <= 65535 && (long long)r.off + (long long)r.w * r.h <= atlas->pool_bytes,
                "%s: glyph %d: bitmap %dx%d at %d lies outside the pool of %lld bytes", what, g, r.w, r.h, r.off, atlas->pool_bytes);
  }
  for (int i = 0; i < n_places; ++i) {
    const dmx_glyph_placement& p = places_host[i];
    DMX_REQUIRE(p.glyph >= 0 && p.glyph < atlas->n_glyphs, "%s: placement %d: glyph %d outside the atlas of %d", what, i, p.glyph, atlas->n_glyphs);
    DMX_REQUIRE(p.x >= -DMX_GLYPH_TEXT_MAX_COORD && p.x <= DMX_GLYPH_TEXT_MAX_COORD && p.y >= -DMX_GLYPH_TEXT_MAX_COORD && p.y <= DMX_GLYPH_TEXT_MAX_COORD,
                "%s: placement %d: position (%d, %d) beyond +-%d", what, i, p.x, p.y, DMX_GLYPH_TEXT_MAX_COORD);
  }
  a = Tables{atlas->pool, atlas->pool_bytes, atlas->glyphs_device, atlas->n_glyphs, places_device, n_places};
  return DMX_OK;
}
}  // namespace dmx_glyph
