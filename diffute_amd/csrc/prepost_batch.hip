// Several text boxes per launch: the batched ends of the editing path (pipeline.edit_boxes, pipeline.edit_pages).  prepost.hip turns
// one box into the [1,3,S,S] network inputs and pastes one decoder output back, with the geometry as kernel arguments and a full-size
// [H][W] mask rasterised by a launch of its own; here B boxes share the uint8 pages in HBM, item b's geometry comes from a device table
// of dmx_edit_item, and the mask is the predicate "inside item b's inclusive box" (PIL's rectangle rule, what dmx_mask_rasterize_kernel
// writes), so there is neither a mask buffer nor a rasterise launch.  The per-pixel arithmetic is prepost_resize.h, the same
// functions the single-box kernels call: row b is bit for bit what the single-box entry gives for item b.
// Pure HBM-bound byte work: one thread per destination pixel, coalesced plain vector stores.
// Three kernel bodies - crop, paste, select-paste -, each written ONCE over a page source (prepost_paste.h) and instantiated twice:
//   OnePage     the boxes of ONE image, given by kernel arguments: the dmx_*_batch entries and dmx_postprocess_paste_select;
//   PageTable   boxes on SEVERAL pages: a second device table, of dmx_edit_page, says where each page lives and which contiguous range
//               of the item table belongs to it: the dmx_*_pages entries.  A page is bit for bit what the one-page kernel gives for its
//               items alone.  Whatever comes from the device tables is clamped (page_of, item_geom: prepost_resize.h; page_block):
//               a stale table reads wrong pixels, never outside a page (the pages' own addresses and sizes are trusted, as the
//               one-page kernels trust their arguments).
#include "common.h"
#include "kernels.h"
#include "prepost_paste.h"
#include "prepost_resize.h"

namespace {
using namespace dmx_resize;
using namespace dmx_paste;      // PasteArgs, OnePage, PageTable, PageBlock, select_choices: shared with prepost_blend.hip

struct PreArgs {
  const dmx_edit_item* items; int S;
  float* out_img; float* out_masked; unsigned char* out_mask; float* out_mask_lat;   // [B][3][S][S], [B][3][S][S], [B][S][S], [B][S/8][S/8]
};

// Destination pixel (dx, dy) of row b: item `it` cropped from its page pg (HWC uint8).
__device__ __forceinline__ void pre_item(const PreArgs& p, const dmx_edit_page& pg, const dmx_edit_item& it, int b, int dx, int dy) {
  const Geom g = item_geom(it, pg.H, pg.W, p.S, true);
  int vi[3], vm[3], vk;
  // generate_mask (app.ipynb:370-378) as a predicate on image coordinates: item b's box alone, both corners included
  auto mk = [&](int y, int x) -> int {
    const int X = g.xs + x, Y = g.ys + y;
    return (X >= it.x1 && X <= it.x2 && Y >= it.y1 && Y <= it.y2) ? 1 : 0;
  };
  pre_pixel((const unsigned char*)pg.original, pg.W, g, mk, dx, dy, vi, vm, vk);
  const size_t plane = (size_t)p.S * p.S, lat = (size_t)(p.S >> 3) * (p.S >> 3);
  pre_store(vi, vm, vk, p.S, dx, dy, p.out_img + (size_t)b * 3 * plane, p.out_masked + (size_t)b * 3 * plane, p.out_mask + (size_t)b * plane,
            p.out_mask_lat ? p.out_mask_lat + (size_t)b * lat : nullptr);
}

// grid (ceil(S / 256), S, B): the grid runs over items; the item's page supplies the image pointer, H and W
template <class Pages>
__global__ __launch_bounds__(256) void dmx_preprocess_boxes_kernel(const PreArgs p, const Pages pages) {
  const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y, b = blockIdx.z;
  if (dx >= p.S) return;
  const dmx_edit_item it = p.items[b];
  pre_item(p, pages.of(it), it, b, dx, dy);
}

// B chained single pastes in index order leave, at every pixel, the value of the LAST item whose (half-open box) AND (resized crop
// extent) covers it, computed from that item's decoder output alone, or the original where no item does: scan from the last item down
// and stop at the first hit.  The integer half of the page's items (t: its page and its slice of the table) is staged in LDS once per
// block (every pixel of the row scans all of it).
__device__ __forceinline__ void stage_items(const PasteArgs& p, const PageBlock& t, int4* s_box, int4* s_crop) {
  if ((int)threadIdx.x < t.n) {
    const dmx_edit_item& it = p.items[t.lo + threadIdx.x];
    s_box[threadIdx.x] = make_int4(it.x1, it.y1, it.x2, it.y2);
    const int xs = min(max(it.x_s, 0), t.pg.W - 1), ys = min(max(it.y_s, 0), t.pg.H - 1);       // item_geom's clamps
    s_crop[threadIdx.x] = make_int4(xs, ys, min(max(it.cw, 1), t.pg.W - xs), min(max(it.ch, 1), t.pg.H - ys));
  }
}
// Pixel (t.x, t.y) of the page.  row(b) -> which [3][S][S] image of p.vae the page's item b pastes, < 0 = the item is skipped (it still
// counts for the union mask: the mask says where the boxes are, not what was pasted).
template <class Row>
__device__ __forceinline__ void paste_pixel(const PasteArgs& p, const PageBlock& t, const int4* s_box, const int4* s_crop, Row row) {
  const int x = t.x, y = t.y, W = t.pg.W;
  int hit = -1, any = 0;
  for (int b = t.n - 1; b >= 0; --b) {
    const int4 bx = s_box[b];
    any |= (x >= bx.x && x <= bx.z && y >= bx.y && y <= bx.w) ? 1 : 0;                    // union mask: PIL's inclusive rectangle
    if (hit < 0 && row(b) >= 0 && x >= bx.x && x < bx.z && y >= bx.y && y < bx.w) {        // the paste: inf_res[y1:y2, x1:x2]
      const int4 cr = s_crop[b];
      const int dx = x - cr.x, dy = y - cr.y;
      if (dx >= 0 && dx < cr.z && dy >= 0 && dy < cr.w) hit = b;
    }
    if (hit >= 0) break;                                                     // (a hit lies inside that item's inclusive box: `any` is set)
  }
  const unsigned char* ori = (const unsigned char*)t.pg.original;
  unsigned char *out = (unsigned char*)t.pg.out, *umask = (unsigned char*)t.pg.union_mask;
  const size_t o = ((size_t)y * W + x) * 3;
  if (umask) umask[(size_t)y * W + x] = (unsigned char)any;
  if (hit < 0) { out[o] = ori[o]; out[o + 1] = ori[o + 1]; out[o + 2] = ori[o + 2]; return; }
  const Geom g = item_geom(p.items[t.lo + hit], t.pg.H, W, p.S, false);
  const float* vae = p.vae + (size_t)row(hit) * 3 * p.S * p.S;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[o + c] = post_pixel(vae, p.S, g, c, x - g.xs, y - g.ys);
}

// One 256-pixel tile of one page row per block: grid (ceil(W / 256), H) for one page; for a page table the blocks enumerate (page, row,
// column tile) along grid.x (dmx_paste::page_block), and a pixel scans only its own page's items, last to first.
template <class Pages>
__global__ __launch_bounds__(256) void dmx_postprocess_boxes_kernel(const PasteArgs p, const Pages pages) {
  __shared__ int4 s_box[DMX_EDIT_MAX_ITEMS], s_crop[DMX_EDIT_MAX_ITEMS];
  PageBlock t;
  if (!pages.tile(p.B, t)) return;                                             // (uniform per block: a stale table)
  stage_items(p, t, s_box, s_crop);
  __syncthreads();
  if (t.x >= t.pg.W) return;
  const int lo = t.lo;
  paste_pixel(p, t, s_box, s_crop, [lo](int b) -> int { return lo + b; });
}

// Best of K candidates per item, chosen and pasted in ONE launch: p.vae is [B][K][3][S][S], scores [B][K] lives on the device, so the
// host never waits for it.  choice is [B] over all items; every live block stages the score table in LDS and derives all of it (one
// rule, one table: select_choices, which contains barriers - a block enters it with all its threads or not at all):
//   choice[b] = arg-max over k of scores[b][k], the lowest k on a tie; a NaN never wins; 0 when every score is NaN;
//   -1 (the item is skipped, its box keeps the original pixels) when the best score is below `threshold`.
// The source's one `chooser` block stores `choice`, with plain vector stores - also where a stale page table leaves it no pixel; any
// other block without a pixel returns at once.  The paste is paste_pixel, the rule of the kernel above.
template <class Pages>
__global__ __launch_bounds__(256) void dmx_postprocess_select_boxes_kernel(const PasteArgs p, const Pages pages, const float* scores, int K,
                                                                           float threshold, int* choice) {
  __shared__ int4 s_box[DMX_EDIT_MAX_ITEMS], s_crop[DMX_EDIT_MAX_ITEMS];
  __shared__ float s_score[DMX_EDIT_MAX_ITEMS * DMX_SELECT_MAX_CANDIDATES];
  __shared__ int s_choice[DMX_EDIT_MAX_ITEMS];
  PageBlock t;
  const bool live = pages.tile(p.B, t), chooser = pages.chooser();
  if (!live && !chooser) return;
  if (live) stage_items(p, t, s_box, s_crop);
  select_choices(scores, p.B, K, threshold, s_score, s_choice, choice, chooser);
  if (!live || t.x >= t.pg.W) return;
  const int lo = t.lo;
  paste_pixel(p, t, s_box, s_crop, [&](int b) -> int { const int k = s_choice[lo + b]; return k < 0 ? -1 : (lo + b) * K + k; });
}

// The launches, one per stage; the tables are checked.  `kernel` names the launch in the last-error string.
template <class Pages>
int launch_pre(const char* kernel, const Pages& pages, const dmx_edit_item* items_device, int B, int S, float* out_image, float* out_masked_image,
               unsigned char* out_mask, float* out_mask_latent, dmx_stream_t stream) {
  PreArgs p{items_device, S, out_image, out_masked_image, out_mask, out_mask_latent};
  hipLaunchKernelGGL(dmx_preprocess_boxes_kernel<Pages>, dim3(cdiv(S, 256), S, B), dim3(256), 0, (hipStream_t)stream, p, pages);
  return dmx_check_launch(kernel);
}

template <class Pages>
int launch_post(const char* kernel, const Pages& pages, dim3 grid, const float* image_vae, int S, const dmx_edit_item* items_device, int B,
                dmx_stream_t stream) {
  PasteArgs p{image_vae, S, items_device, B};
  hipLaunchKernelGGL(dmx_postprocess_boxes_kernel<Pages>, grid, dim3(256), 0, (hipStream_t)stream, p, pages);
  return dmx_check_launch(kernel);
}

template <class Pages>
int launch_select(const char* kernel, const Pages& pages, dim3 grid, const float* image_vae, int S, const float* scores, float threshold, int* choice,
                  const dmx_edit_item* items_device, int B, int K, dmx_stream_t stream) {
  PasteArgs p{image_vae, S, items_device, B};
  hipLaunchKernelGGL(dmx_postprocess_select_boxes_kernel<Pages>, grid, dim3(256), 0, (hipStream_t)stream, p, pages, scores, K, threshold, choice);
  return dmx_check_launch(kernel);
}

}  // namespace

// the checks of the single-box entries, per item; `prepared` also compares the derived fields with what edit_items_prepare fills
// (index0: the table index of items[0], for the messages - the pages entries check one page's slice at a time)
int dmx_check_edit_items(const char* what, const dmx_edit_item* items, int B, int H, int W, int S, bool prepared, int index0) {
  DMX_REQUIRE(items, "%s: null item table", what);
  DMX_REQUIRE(B >= 1 && B <= DMX_EDIT_MAX_ITEMS, "%s: %d items, expected 1 .. %d", what, B, DMX_EDIT_MAX_ITEMS);
  DMX_REQUIRE(H > 0 && W > 0 && H <= 65535 && S > 0 && S <= 65535, "%s: bad sizes (image %dx%d, S %d)", what, W, H, S);
  for (int b = 0; b < B; ++b) {
    const dmx_edit_item& it = items[b];
    DMX_REQUIRE(it.crop_scale > 0, "%s: item %d: crop_scale %d", what, index0 + b, it.crop_scale);
    DMX_REQUIRE(it.x_s >= 0 && it.y_s >= 0 && it.x_s < W && it.y_s < H, "%s: item %d: crop origin (%d, %d) outside the %dx%d image", what, index0 + b,
                it.x_s, it.y_s, W, H);
    if (!prepared) continue;
    const Geom a = pre_geom(H, W, it.x_s, it.y_s, it.crop_scale, S), z = post_geom(H, W, it.x_s, it.y_s, it.crop_scale, S);
    DMX_REQUIRE(it.cw == a.cw && it.ch == a.ch && it.pre_area2 == a.area2 && it.post_area2 == z.area2 && it.pre_sx == a.sx && it.pre_sy == a.sy &&
                    it.post_sx == z.sx && it.post_sy == z.sy,
                "%s: item %d: derived fields do not belong to a %dx%d image at S = %d (dmx_edit_items_prepare fills them)", what, index0 + b, W, H, S);
  }
  return DMX_OK;
}

extern "C" int dmx_edit_items_prepare(dmx_edit_item* items, int B, int H, int W, int S) {
  const int rc = dmx_check_edit_items("edit_items_prepare", items, B, H, W, S, false);
  if (rc != DMX_OK) return rc;
  for (int b = 0; b < B; ++b) {
    dmx_edit_item& it = items[b];
    const Geom a = pre_geom(H, W, it.x_s, it.y_s, it.crop_scale, S), z = post_geom(H, W, it.x_s, it.y_s, it.crop_scale, S);
    it.cw = a.cw; it.ch = a.ch; it.pre_area2 = a.area2; it.post_area2 = z.area2; it.reserved = 0;
    it.pre_sx = a.sx; it.pre_sy = a.sy; it.post_sx = z.sx; it.post_sy = z.sy;
  }
  return DMX_OK;
}

extern "C" int dmx_preprocess_crop_batch(const unsigned char* image_hwc, int H, int W, const dmx_edit_item* items_host, const dmx_edit_item* items_device,
                                         int B, int S, float* out_image, float* out_masked_image, unsigned char* out_mask, float* out_mask_latent,
                                         dmx_stream_t stream) {
  DMX_REQUIRE(image_hwc && items_device && out_image && out_masked_image && out_mask, "preprocess_crop_batch: null argument");
  DMX_REQUIRE(S > 0 && S % 8 == 0, "preprocess_crop_batch: S = %d is no positive multiple of 8", S);
  const int rc = dmx_check_edit_items("preprocess_crop_batch", items_host, B, H, W, S, true);
  if (rc != DMX_OK) return rc;
  return launch_pre("dmx_preprocess_batch_kernel", OnePage{image_hwc, nullptr, nullptr, H, W}, items_device, B, S, out_image, out_masked_image, out_mask,
                    out_mask_latent, stream);
}

extern "C" int dmx_postprocess_paste_batch(const float* image_vae, int S, const unsigned char* original_hwc, unsigned char* out_hwc,
                                           unsigned char* union_mask, int H, int W, const dmx_edit_item* items_host,
                                           const dmx_edit_item* items_device, int B, dmx_stream_t stream) {
  DMX_REQUIRE(image_vae && original_hwc && out_hwc && items_device, "postprocess_paste_batch: null argument");
  const int rc = dmx_check_edit_items("postprocess_paste_batch", items_host, B, H, W, S, true);
  if (rc != DMX_OK) return rc;
  return launch_post("dmx_postprocess_batch_kernel", OnePage{original_hwc, out_hwc, union_mask, H, W}, dim3(cdiv(W, 256), H), image_vae, S, items_device,
                     B, stream);
}

// what the two select entries ask of their scalars
int dmx_check_select_scalars(const char* what, int K, float threshold) {
  DMX_REQUIRE(K >= 1 && K <= DMX_SELECT_MAX_CANDIDATES, "%s: %d candidates per box, expected 1 .. %d", what, K, DMX_SELECT_MAX_CANDIDATES);
  DMX_REQUIRE(!(threshold != threshold), "%s: the threshold is NaN (pass -inf for none)", what);
  return DMX_OK;
}

extern "C" int dmx_postprocess_paste_select(const float* image_vae, int S, const float* scores, float threshold, const unsigned char* original_hwc,
                                            unsigned char* out_hwc, unsigned char* union_mask, int* choice, int H, int W,
                                            const dmx_edit_item* items_host, const dmx_edit_item* items_device, int B, int K, dmx_stream_t stream) {
  DMX_REQUIRE(image_vae && scores && original_hwc && out_hwc && choice && items_device, "postprocess_paste_select: null argument");
  int rc = dmx_check_select_scalars("postprocess_paste_select", K, threshold);
  if (rc == DMX_OK) rc = dmx_check_edit_items("postprocess_paste_select", items_host, B, H, W, S, true);
  if (rc != DMX_OK) return rc;
  return launch_select("dmx_postprocess_select_kernel", OnePage{original_hwc, out_hwc, union_mask, H, W}, dim3(cdiv(W, 256), H), image_vae, S, scores,
                       threshold, choice, items_device, B, K, stream);
}

// ---- pages
// the page table of 1 .. DMX_EDIT_MAX_ITEMS pages and B items of any kind (kernels.h); a bad page is named by page index
int dmx_check_page_table(const char* what, const dmx_edit_page* pages, int P, int B, int max_w, const char* prepare, bool prepared) {
  long long blocks = 0;
  for (int q = 0, next = 0; q < P; ++q) {
    const dmx_edit_page& pg = pages[q];
    // (W + 255 must not overflow an int, here or in the kernels' tile count)
    DMX_REQUIRE(pg.H > 0 && pg.W > 0 && pg.H <= 65535 && pg.W <= max_w, "%s: page %d: bad size %dx%d (1 <= H <= 65535, 1 <= W <= %d)", what, q, pg.W,
                pg.H, max_w);
    DMX_REQUIRE(pg.item_hi > pg.item_lo, "%s: page %d: no items (range [%d, %d))", what, q, pg.item_lo, pg.item_hi);
    DMX_REQUIRE(pg.item_lo == next && pg.item_hi <= B,
                "%s: page %d: its items [%d, %d) must start at %d and end at or before %d (the ranges tile [0, B) in page order)", what, q, pg.item_lo,
                pg.item_hi, next, B);
    DMX_REQUIRE(q + 1 < P || pg.item_hi == B, "%s: page %d: the last page's items end at %d, the table holds %d", what, q, pg.item_hi, B);
    next = pg.item_hi;
    const long long mine = (long long)pg.H * cdiv(pg.W, 256);
    DMX_REQUIRE(blocks + mine < (1ll << 31), "%s: page %d: the pages need more than 2^31 - 1 blocks of 256 pixels", what, q);
    if (prepared)
      DMX_REQUIRE(pg.block_lo == (int)blocks && pg.blocks == (int)mine, "%s: page %d: derived fields do not belong to this page table (%s fills them)",
                  what, q, prepare);
    blocks += mine;
  }
  return DMX_OK;
}

// the page table, then every page's slice of the item table against that page; `prepared` also compares the derived fields of both
// tables with what edit_pages_prepare fills.  A bad page is named by page index, a bad item by its index in the whole table.
int dmx_check_edit_pages(const char* what, const dmx_edit_page* pages, int P, const dmx_edit_item* items, int B, int S, bool prepared) {
  DMX_REQUIRE(pages && items, "%s: null page or item table", what);
  DMX_REQUIRE(P >= 1 && P <= DMX_EDIT_MAX_ITEMS, "%s: %d pages, expected 1 .. %d", what, P, DMX_EDIT_MAX_ITEMS);
  DMX_REQUIRE(B >= 1 && B <= DMX_EDIT_MAX_ITEMS, "%s: %d items, expected 1 .. %d", what, B, DMX_EDIT_MAX_ITEMS);
  int rc = dmx_check_page_table(what, pages, P, B, DMX_EDIT_PAGE_MAX_W, "dmx_edit_pages_prepare", prepared);
  for (int q = 0; q < P && rc == DMX_OK; ++q) {                        // the ranges tile [0, B): every item has its page
    const dmx_edit_page& pg = pages[q];
    rc = dmx_check_edit_items(what, items + pg.item_lo, pg.item_hi - pg.item_lo, pg.H, pg.W, S, prepared, pg.item_lo);
    if (rc != DMX_OK || !prepared) continue;
    for (int b = pg.item_lo; b < pg.item_hi; ++b)
      DMX_REQUIRE(items[b].reserved == q, "%s: item %d: page index %d, the item lies in the range of page %d (dmx_edit_pages_prepare fills it)", what, b,
                  items[b].reserved, q);
  }
  return rc;
}

int dmx_check_page_addresses(const char* what, const dmx_edit_page* pages, int P, bool need_out) {
  for (int q = 0; q < P; ++q) {
    DMX_REQUIRE(pages[q].original, "%s: page %d: null original image", what, q);
    DMX_REQUIRE(!need_out || (pages[q].out && pages[q].out != pages[q].original), "%s: page %d: the output image is null or the original itself", what, q);
  }
  return DMX_OK;
}

extern "C" int dmx_edit_pages_prepare(dmx_edit_page* pages, int P, dmx_edit_item* items, int B, int S) {
  int rc = dmx_check_edit_pages("edit_pages_prepare", pages, P, items, B, S, false);
  if (rc != DMX_OK) return rc;
  int blocks = 0;
  for (int q = 0; q < P; ++q) {
    dmx_edit_page& pg = pages[q];
    rc = dmx_edit_items_prepare(items + pg.item_lo, pg.item_hi - pg.item_lo, pg.H, pg.W, S);      // each item with its own page's size
    if (rc != DMX_OK) return rc;
    for (int b = pg.item_lo; b < pg.item_hi; ++b) items[b].reserved = q;
    pg.block_lo = blocks; pg.blocks = pg.H * cdiv(pg.W, 256);
    blocks += pg.blocks;
  }
  return DMX_OK;
}

extern "C" int dmx_preprocess_crop_pages(const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P, const dmx_edit_item* items_host,
                                         const dmx_edit_item* items_device, int B, int S, float* out_image, float* out_masked_image,
                                         unsigned char* out_mask, float* out_mask_latent, dmx_stream_t stream) {
  DMX_REQUIRE(pages_device && items_device && out_image && out_masked_image && out_mask, "preprocess_crop_pages: null argument");
  DMX_REQUIRE(S > 0 && S <= 65535 && S % 8 == 0, "preprocess_crop_pages: S = %d is no positive multiple of 8 (up to 65535)", S);
  int rc = dmx_check_edit_pages("preprocess_crop_pages", pages_host, P, items_host, B, S, true);
  if (rc == DMX_OK) rc = dmx_check_page_addresses("preprocess_crop_pages", pages_host, P, false);
  if (rc != DMX_OK) return rc;
  return launch_pre("dmx_preprocess_pages_kernel", PageTable{pages_device, P}, items_device, B, S, out_image, out_masked_image, out_mask,
                    out_mask_latent, stream);
}

extern "C" int dmx_postprocess_paste_pages(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                           const dmx_edit_item* items_host, const dmx_edit_item* items_device, int B, dmx_stream_t stream) {
  DMX_REQUIRE(image_vae && pages_device && items_device, "postprocess_paste_pages: null argument");
  DMX_REQUIRE(S > 0 && S <= 65535, "postprocess_paste_pages: bad S = %d", S);
  int rc = dmx_check_edit_pages("postprocess_paste_pages", pages_host, P, items_host, B, S, true);
  if (rc == DMX_OK) rc = dmx_check_page_addresses("postprocess_paste_pages", pages_host, P, true);
  if (rc != DMX_OK) return rc;
  return launch_post("dmx_postprocess_pages_kernel", PageTable{pages_device, P}, paged_grid(pages_host, P), image_vae, S, items_device, B, stream);
}

extern "C" int dmx_postprocess_paste_select_pages(const float* image_vae, int S, const float* scores, float threshold, int* choice,
                                                  const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                                  const dmx_edit_item* items_host, const dmx_edit_item* items_device, int B, int K,
                                                  dmx_stream_t stream) {
  DMX_REQUIRE(image_vae && scores && choice && pages_device && items_device, "postprocess_paste_select_pages: null argument");
  DMX_REQUIRE(S > 0 && S <= 65535, "postprocess_paste_select_pages: bad S = %d", S);
  int rc = dmx_check_select_scalars("postprocess_paste_select_pages", K, threshold);
  if (rc == DMX_OK) rc = dmx_check_edit_pages("postprocess_paste_select_pages", pages_host, P, items_host, B, S, true);
  if (rc == DMX_OK) rc = dmx_check_page_addresses("postprocess_paste_select_pages", pages_host, P, true);
  if (rc != DMX_OK) return rc;
  return launch_select("dmx_postprocess_select_pages_kernel", PageTable{pages_device, P}, paged_grid(pages_host, P), image_vae, S, scores, threshold,
                       choice, items_device, B, K, stream);
}
