// Quadrilateral text regions with oriented crops: the two ends of the editing path for skewed and rotated lines (pipeline.edit_quads),
// beside prepost_batch.hip's axis-aligned boxes.  Items are dmx_edit_quad, pages the dmx_edit_page table of the *_pages entries.  Three
// kernels, one launch each: the crop (mask = the quad itself, frame turned to the baseline), the paste (every page pixel mapped back
// through the inverse frame; the last quad that covers a pixel decides) and the rectify (a quad as an upright strip, for the OCR model).
// The per-pixel arithmetic is prepost_quad.h.  Pure HBM-bound byte work: one thread per destination pixel, coalesced plain vector
// stores, the integer tables staged in LDS once per block, no atomics.
#include "common.h"
#include "kernels.h"
#include "prepost_quad.h"

namespace {
using namespace dmx_quad;

constexpr int kQuadInts = (int)(sizeof(dmx_edit_quad) / sizeof(int));
static_assert(sizeof(dmx_edit_quad) % sizeof(int) == 0 && kQuadInts <= 256, "a block stages one quad with one int per thread");

// one table entry into LDS, one int per thread; ends with a barrier
__device__ __forceinline__ void stage_quad(dmx_edit_quad* s_q, const dmx_edit_quad* src) {
  if ((int)threadIdx.x < kQuadInts) ((int*)s_q)[threadIdx.x] = ((const int*)src)[threadIdx.x];
  __syncthreads();
}

struct PreQuadArgs {
  const dmx_edit_page* pages; int P;
  const dmx_edit_quad* quads; int S;
  float* out_img; float* out_masked; unsigned char* out_mask; float* out_mask_lat;
};

// grid (ceil(S / 256), S, B): block z handles row y of quad z's crop
__global__ __launch_bounds__(256) void dmx_preprocess_quads_kernel(const PreQuadArgs p) {
  __shared__ dmx_edit_quad s_q;
  const int b = blockIdx.z;
  stage_quad(&s_q, p.quads + b);
  const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y;
  if (dx >= p.S) return;
  const dmx_edit_page pg = p.pages[min(max(s_q.page, 0), p.P - 1)];
  if (pg.H <= 0 || pg.W <= 0) return;
  const long long px = 2 * dx + 1 - p.S, py = 2 * dy + 1 - p.S;
  const long long X16 = ((long long)s_q.cx2 << 15) + s_q.fwd[0] * px + s_q.fwd[1] * py;
  const long long Y16 = ((long long)s_q.cy2 << 15) + s_q.fwd[2] * px + s_q.fwd[3] * py;
  int vi[3], vm[3], vk;
  pre_pixel((const unsigned char*)pg.original, pg.H, pg.W, X16, Y16, [&](int X, int Y) -> int { return inside(s_q, X, Y); }, vi, vm, vk);
  const size_t plane = (size_t)p.S * p.S, lat = (size_t)(p.S >> 3) * (p.S >> 3);
  dmx_resize::pre_store(vi, vm, vk, p.S, dx, dy, p.out_img + (size_t)b * 3 * plane, p.out_masked + (size_t)b * 3 * plane,
                        p.out_mask + (size_t)b * plane, p.out_mask_lat ? p.out_mask_lat + (size_t)b * lat : nullptr);
}

struct PostQuadArgs {
  const float* vae; int S;
  const dmx_edit_page* pages; int P;
  const dmx_edit_quad* quads; int B;
};

// The paste over P pages: blocks enumerate (page, row, 256-column tile) along grid.x as in dmx_postprocess_pages_kernel; a block finds
// its page by a uniform scan of the block_lo values and stages the page's quads - corners, edges, bounding box - in LDS.  A pixel scans
// them last to first and stops at the first quad that covers it.
__global__ __launch_bounds__(256) void dmx_postprocess_quads_kernel(const PostQuadArgs p) {
  __shared__ QuadEdges s_e[DMX_EDIT_MAX_ITEMS];
  int pi = 0;
  for (int i = 1; i < p.P; ++i) pi = (int)blockIdx.x >= p.pages[i].block_lo ? i : pi;
  const dmx_edit_page pg = p.pages[pi];
  if (pg.H <= 0 || pg.W <= 0 || pg.W > 65535) return;                          // (uniform per block: a stale table)
  const int tiles = (pg.W + 255) / 256, local = (int)blockIdx.x - pg.block_lo;
  if (local < 0 || local / tiles >= pg.H) return;
  const int lo = min(max(pg.item_lo, 0), p.B - 1), n = min(max(pg.item_hi - lo, 1), p.B - lo);
  if ((int)threadIdx.x < n) {
    const dmx_edit_quad& q = p.quads[lo + threadIdx.x];
    QuadEdges e;
#pragma unroll
    for (int k = 0; k < 4; ++k) { e.x[k] = q.x[k]; e.y[k] = q.y[k]; e.ex[k] = q.ex[k]; e.ey[k] = q.ey[k]; }
    e.bx1 = q.bx1; e.by1 = q.by1; e.bx2 = q.bx2; e.by2 = q.by2;
    s_e[threadIdx.x] = e;
  }
  __syncthreads();
  const int y = local / tiles, x = (local % tiles) * 256 + (int)threadIdx.x;
  if (x >= pg.W) return;
  int hit = -1;
  for (int b = n - 1; b >= 0; --b) {
    const QuadEdges& e = s_e[b];
    if (x >= e.bx1 && x <= e.bx2 && y >= e.by1 && y <= e.by2 && inside(e, x, y)) { hit = b; break; }
  }
  const unsigned char* ori = (const unsigned char*)pg.original;
  unsigned char *out = (unsigned char*)pg.out, *umask = (unsigned char*)pg.union_mask;
  const size_t o = ((size_t)y * pg.W + x) * 3;
  if (umask) umask[(size_t)y * pg.W + x] = (unsigned char)(hit >= 0 ? 1 : 0);
  bool paste = false;
  long long U16 = 0, V16 = 0;
  if (hit >= 0) {
    const dmx_edit_quad& q = p.quads[lo + hit];
    const long long qx = 2ll * x - q.cx2, qy = 2ll * y - q.cy2, base = (long long)(p.S - 1) << 15, top = ((long long)p.S << 16) - 32768;
    U16 = base + q.inv[0] * qx + q.inv[1] * qy;
    V16 = base + q.inv[2] * qx + q.inv[3] * qy;
    paste = U16 >= -32768 && U16 < top && V16 >= -32768 && V16 < top;
  }
  if (!paste) { out[o] = ori[o]; out[o + 1] = ori[o + 1]; out[o + 2] = ori[o + 2]; return; }
  const float* vae = p.vae + (size_t)(lo + hit) * 3 * p.S * p.S;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[o + c] = post_pixel(vae, p.S, c, U16, V16);
}

struct RectQuadArgs {
  const dmx_edit_page* pages; int P;
  const dmx_edit_quad* quads; int B;
  unsigned char* out; long long out_bytes;
};

// The strips of all quads: blocks enumerate (quad, row, 256-column tile) along grid.x; a block finds its quad by a uniform scan of the
// rect_block_lo values (staged in LDS), stages that quad and writes one tile of one strip row.  No byte is written at or past out_bytes.
__global__ __launch_bounds__(256) void dmx_rectify_quads_kernel(const RectQuadArgs p) {
  __shared__ int s_lo[DMX_EDIT_MAX_ITEMS];
  __shared__ dmx_edit_quad s_q;
  if ((int)threadIdx.x < p.B) s_lo[threadIdx.x] = p.quads[threadIdx.x].rect_block_lo;
  __syncthreads();
  int b = 0;
  for (int i = 1; i < p.B; ++i) b = (int)blockIdx.x >= s_lo[i] ? i : b;
  stage_quad(&s_q, p.quads + b);
  const dmx_edit_page pg = p.pages[min(max(s_q.page, 0), p.P - 1)];
  const int rw = s_q.rw, rh = s_q.rh;
  if (pg.H <= 0 || pg.W <= 0 || rw <= 0 || rh <= 0 || rw > (1 << 20) || s_q.rect_off < 0) return;
  const int tiles = (rw + 255) / 256, local = (int)blockIdx.x - s_q.rect_block_lo;
  if (local < 0 || local / tiles >= rh) return;
  const int j = local / tiles, i = (local % tiles) * 256 + (int)threadIdx.x;
  if (i >= rw) return;
  const long long o = s_q.rect_off + ((long long)j * rw + i) * 3;
  if (o + 3 > p.out_bytes) return;
  const long long px = 2 * i + 1 - rw, py = 2 * j + 1 - rh;
  const long long X16 = ((long long)s_q.sx4 << 14) + s_q.rect[0] * px + s_q.rect[1] * py;
  const long long Y16 = ((long long)s_q.sy4 << 14) + s_q.rect[2] * px + s_q.rect[3] * py;
  const Tap16 tx = tap16(X16, pg.W), ty = tap16(Y16, pg.H);
#pragma unroll
  for (int c = 0; c < 3; ++c) p.out[o + c] = (unsigned char)page_sample((const unsigned char*)pg.original, pg.W, tx, ty, c);
}

}  // namespace

namespace dmx_quad {
// The host-side checks of a page table and a quad table.  frames: the frame fields are looked at (the rectify entry reads none of
// them).  prepared: the derived fields of both tables are compared with what dmx_edit_quads_prepare fills.  A bad page is named by page
// index, a bad quad by its index in the whole table.
int check_quads(const char* what, const dmx_edit_page* pages, int P, const dmx_edit_quad* quads, int B, int S, bool frames, bool prepared) {
  DMX_REQUIRE(pages && quads, "%s: null page or quad table", what);
  DMX_REQUIRE(P >= 1 && P <= DMX_EDIT_MAX_ITEMS, "%s: %d pages, expected 1 .. %d", what, P, DMX_EDIT_MAX_ITEMS);
  DMX_REQUIRE(B >= 1 && B <= DMX_EDIT_MAX_ITEMS, "%s: %d items, expected 1 .. %d", what, B, DMX_EDIT_MAX_ITEMS);
  DMX_REQUIRE(!frames || (S >= 1 && S <= 65535), "%s: bad S = %d (1 .. 65535)", what, S);
  long long blocks = 0, rect_off = 0, rect_blocks = 0;
  for (int q = 0, next = 0; q < P; ++q) {
    const dmx_edit_page& pg = pages[q];
    DMX_REQUIRE(pg.H > 0 && pg.W > 0 && pg.H <= 65535 && pg.W <= 65535, "%s: page %d: bad size %dx%d (1 <= H, W <= 65535)", what, q, pg.W, pg.H);
    DMX_REQUIRE(pg.item_hi > pg.item_lo, "%s: page %d: no items (range [%d, %d))", what, q, pg.item_lo, pg.item_hi);
    DMX_REQUIRE(pg.item_lo == next && pg.item_hi <= B,
                "%s: page %d: its items [%d, %d) must start at %d and end at or before %d (the ranges tile [0, B) in page order)", what, q, pg.item_lo,
                pg.item_hi, next, B);
    DMX_REQUIRE(q + 1 < P || pg.item_hi == B, "%s: page %d: the last page's items end at %d, the table holds %d", what, q, pg.item_hi, B);
    next = pg.item_hi;
    const long long mine = (long long)pg.H * cdiv(pg.W, 256);
    if (prepared)
      DMX_REQUIRE(pg.block_lo == (int)blocks && pg.blocks == (int)mine,
                  "%s: page %d: derived fields do not belong to this page table (dmx_edit_quads_prepare fills them)", what, q);
    blocks += mine;                                                    // (at most 64 * 65535 * 256 < 2^31)
  }
  for (int q = 0; q < P; ++q) {                                        // the ranges tile [0, B): every item has its page
    const dmx_edit_page& pg = pages[q];
    for (int b = pg.item_lo; b < pg.item_hi; ++b) {
      const dmx_edit_quad& it = quads[b];
      for (int k = 0; k < 4; ++k)
        DMX_REQUIRE(it.x[k] >= 0 && it.x[k] < pg.W && it.y[k] >= 0 && it.y[k] < pg.H, "%s: item %d: corner %d (%d, %d) lies outside the %dx%d page", what,
                    b, k, it.x[k], it.y[k], pg.W, pg.H);
      long long area2 = 0;
      for (int k = 0; k < 4; ++k) {
        const int k1 = (k + 1) & 3, k2 = (k + 2) & 3;
        const long long ex = it.x[k1] - it.x[k], ey = it.y[k1] - it.y[k], fx = it.x[k2] - it.x[k1], fy = it.y[k2] - it.y[k1];
        DMX_REQUIRE(ex * fy - ey * fx >= 0,
                    "%s: item %d: the quad turns the wrong way at corner %d: not convex, or counter-clockwise (corners run TL, TR, BR, BL)", what, b, k1);
        area2 += (long long)it.x[k] * it.y[k1] - (long long)it.x[k1] * it.y[k];
      }
      DMX_REQUIRE(area2 > 0, "%s: item %d: the quad has no area", what, b);
      // (a convex quad with area has u, v != 0; the strip's matrix divides by |u|)
      DMX_REQUIRE(((it.x[1] - it.x[0]) + (it.x[2] - it.x[3]) != 0 || (it.y[1] - it.y[0]) + (it.y[2] - it.y[3]) != 0) &&
                      ((it.x[3] - it.x[0]) + (it.x[2] - it.x[1]) != 0 || (it.y[3] - it.y[0]) + (it.y[2] - it.y[1]) != 0),
                  "%s: item %d: the quad's summed opposite edges vanish", what, b);
      DMX_REQUIRE(it.page == q, "%s: item %d: page index %d, the item lies in the range of page %d", what, b, it.page, q);
      if (frames) {
        DMX_REQUIRE(it.ux != 0 || it.uy != 0, "%s: item %d: the baseline direction (ux, uy) is (0, 0)", what, b);
        DMX_REQUIRE(it.ux >= -131070 && it.ux <= 131070 && it.uy >= -131070 && it.uy <= 131070, "%s: item %d: baseline direction (%d, %d) beyond +-131070",
                    what, b, it.ux, it.uy);
        DMX_REQUIRE(it.crop_scale >= 1 && it.crop_scale <= 65535, "%s: item %d: crop_scale %d, expected 1 .. 65535", what, b, it.crop_scale);
        DMX_REQUIRE(it.cx2 >= 0 && it.cx2 <= 2 * (pg.W - 1) && it.cy2 >= 0 && it.cy2 <= 2 * (pg.H - 1),
                    "%s: item %d: the frame's centre (%d, %d) half-pixels lies outside the %dx%d page", what, b, it.cx2, it.cy2, pg.W, pg.H);
      }
      dmx_edit_quad t = it;
      if (!frames) { t.crop_scale = 1; t.ux = 1; t.uy = 0; }
      fill_derived(t, frames ? S : 1, rect_off, (int)rect_blocks);
      DMX_REQUIRE(rect_blocks + t.rect_blocks < (1ll << 31), "%s: item %d: the strips need more than 2^31 - 1 blocks of 256 pixels", what, b);
      if (prepared) {
        if (!frames) { t.crop_scale = it.crop_scale; t.ux = it.ux; t.uy = it.uy; memcpy(t.fwd, it.fwd, sizeof t.fwd); memcpy(t.inv, it.inv, sizeof t.inv); }
        DMX_REQUIRE(memcmp(&t, &it, sizeof t) == 0, "%s: item %d: derived fields do not belong to this quad, page table and S (dmx_edit_quads_prepare fills them)",
                    what, b);
      }
      rect_off += (long long)t.rw * t.rh * 3;
      rect_blocks += t.rect_blocks;
    }
  }
  return DMX_OK;
}

int check_quad_pages(const char* what, const dmx_edit_page* pages, int P, bool need_out) {
  for (int q = 0; q < P; ++q) {
    DMX_REQUIRE(pages[q].original, "%s: page %d: null original image", what, q);
    DMX_REQUIRE(!need_out || (pages[q].out && pages[q].out != pages[q].original), "%s: page %d: the output image is null or the original itself", what, q);
  }
  return DMX_OK;
}
}  // namespace dmx_quad

extern "C" int dmx_edit_quads_prepare(dmx_edit_page* pages, int P, dmx_edit_quad* quads, int B, int S) {
  const int rc = check_quads("edit_quads_prepare", pages, P, quads, B, S, true, false);
  if (rc != DMX_OK) return rc;
  int blocks = 0, rect_blocks = 0;
  long long rect_off = 0;
  for (int q = 0; q < P; ++q) {
    dmx_edit_page& pg = pages[q];
    pg.block_lo = blocks; pg.blocks = pg.H * cdiv(pg.W, 256);
    blocks += pg.blocks;
  }
  for (int b = 0; b < B; ++b) {
    fill_derived(quads[b], S, rect_off, rect_blocks);
    rect_off += (long long)quads[b].rw * quads[b].rh * 3;
    rect_blocks += quads[b].rect_blocks;
  }
  return DMX_OK;
}

extern "C" int dmx_preprocess_quads(const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P, const dmx_edit_quad* quads_host,
                                    const dmx_edit_quad* quads_device, int B, int S, float* out_image, float* out_masked_image,
                                    unsigned char* out_mask, float* out_mask_latent, dmx_stream_t stream) {
  DMX_REQUIRE(pages_device && quads_device && out_image && out_masked_image && out_mask, "preprocess_quads: null argument");
  DMX_REQUIRE(S > 0 && S <= 65535 && S % 8 == 0, "preprocess_quads: S = %d is no positive multiple of 8 (up to 65535)", S);
  int rc = check_quads("preprocess_quads", pages_host, P, quads_host, B, S, true, true);
  if (rc == DMX_OK) rc = check_quad_pages("preprocess_quads", pages_host, P, false);
  if (rc != DMX_OK) return rc;
  PreQuadArgs p{pages_device, P, quads_device, S, out_image, out_masked_image, out_mask, out_mask_latent};
  hipLaunchKernelGGL(dmx_preprocess_quads_kernel, dim3(cdiv(S, 256), S, B), dim3(256), 0, (hipStream_t)stream, p);
  return dmx_check_launch("dmx_preprocess_quads_kernel");
}

extern "C" int dmx_postprocess_paste_quads(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                           const dmx_edit_quad* quads_host, const dmx_edit_quad* quads_device, int B, dmx_stream_t stream) {
  DMX_REQUIRE(image_vae && pages_device && quads_device, "postprocess_paste_quads: null argument");
  int rc = check_quads("postprocess_paste_quads", pages_host, P, quads_host, B, S, true, true);
  if (rc == DMX_OK) rc = check_quad_pages("postprocess_paste_quads", pages_host, P, true);
  if (rc != DMX_OK) return rc;
  PostQuadArgs p{image_vae, S, pages_device, P, quads_device, B};
  hipLaunchKernelGGL(dmx_postprocess_quads_kernel, dim3(pages_host[P - 1].block_lo + pages_host[P - 1].blocks), dim3(256), 0, (hipStream_t)stream, p);
  return dmx_check_launch("dmx_postprocess_quads_kernel");
}

extern "C" int dmx_rectify_quads(const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P, const dmx_edit_quad* quads_host,
                                 const dmx_edit_quad* quads_device, int B, unsigned char* out, long long out_bytes, dmx_stream_t stream) {
  DMX_REQUIRE(pages_device && quads_device && out, "rectify_quads: null argument");
  int rc = check_quads("rectify_quads", pages_host, P, quads_host, B, 0, false, true);
  if (rc == DMX_OK) rc = check_quad_pages("rectify_quads", pages_host, P, false);
  if (rc != DMX_OK) return rc;
  const dmx_edit_quad& last = quads_host[B - 1];
  DMX_REQUIRE(out_bytes >= last.rect_off + (long long)last.rw * last.rh * 3, "rectify_quads: the strips take %lld bytes, the output holds %lld",
              last.rect_off + (long long)last.rw * last.rh * 3, out_bytes);
  RectQuadArgs p{pages_device, P, quads_device, B, out, out_bytes};
  hipLaunchKernelGGL(dmx_rectify_quads_kernel, dim3(last.rect_block_lo + last.rect_blocks), dim3(256), 0, (hipStream_t)stream, p);
  return dmx_check_launch("dmx_rectify_quads_kernel");
}
