// Curved text regions: the two ends of the editing path for lines on an arc - signs, seals, stamps, labels (pipeline.edit_curved) -, beside
// prepost_quad.hip's quads.  Items are dmx_edit_curved - polygons of 2n points, cut into n - 1 quad cells and 2 (n - 1) affine pieces -,
// their maps a table of dmx_curved_piece, pages the dmx_edit_page table of the quad entries.  Three kernels, one launch each: the crop
// (the network sees the line straight; mask = the union of the cells seen through the pieces), the paste (a page pixel finds its item, its
// cell and its piece and maps itself back through that piece) and the rectify (the line as an upright strip, for the OCR model).  The
// arithmetic is stated in prepost_curved.h; the maps are dmx_persp_map evaluated by dmx_persp::coords, and everything after the
// coordinates is prepost_quad.h's.  They do not fit prepost_quad.hip's frames: a frame maps an ITEM, here the map changes from pixel to
// pixel and the predicate is a union.  Pure HBM-bound byte work: one thread per destination pixel, coalesced plain vector stores, the
// integer tables staged in LDS once per block, no atomics.
#include <stddef.h>
#include "common.h"
#include "kernels.h"
#include "prepost_paste.h"
#include "prepost_quad_frame.h"
#include "prepost_curved.h"

namespace {
using namespace dmx_quad;
using namespace dmx_curved;

constexpr int kItemInts = (int)(sizeof(dmx_edit_curved) / sizeof(int));
constexpr int kMapWords = (int)(sizeof(dmx_persp_map) / sizeof(long long));
static_assert(sizeof(dmx_edit_curved) % sizeof(int) == 0 && kItemInts <= 256, "a block stages one item with one int per thread");
static_assert(sizeof(dmx_curved_piece) % sizeof(long long) == 0 && sizeof(dmx_persp_map) % sizeof(long long) == 0, "maps are staged word by word");

// What a block of the crop and of the rectify stages of item b in LDS: the record, its cells as the predicate takes them, and ONE map
// (at byte offset map_off of dmx_curved_piece) of each of its pieces.  Called on a block of 256 threads; ends with a barrier.
struct Item { dmx_edit_curved it; QuadEdges cell[kMaxCells]; dmx_persp_map map[2 * kMaxCells]; int n, M; };

__device__ __forceinline__ void stage(Item& s, const dmx_edit_curved* items, const dmx_curved_piece* pieces, int NP, int b, size_t map_off) {
  const int t = threadIdx.x;
  if (t < kItemInts) ((int*)&s.it)[t] = ((const int*)(items + b))[t];
  __syncthreads();
  const int n = pairs(s.it), M = n - 1;
  if (t == 0) { s.n = n; s.M = M; }
  if (t < M) s.cell[t] = cell_edges(s.it, n, t);
  for (int i = t; i < 2 * M * kMapWords; i += blockDim.x) {
    const int piece = i / kMapWords, w = i - piece * kMapWords, g = min(max(s.it.piece_lo + piece, 0), NP - 1);
    ((long long*)&s.map[piece])[w] = ((const long long*)((const char*)(pieces + g) + map_off))[w];
  }
  __syncthreads();
}

struct PreCurvedArgs {
  const dmx_edit_page* pages; int P;
  const dmx_edit_curved* items; const dmx_curved_piece* pieces; int NP; int S;
  float* out_img; float* out_masked; unsigned char* out_mask; float* out_mask_lat;
};

// grid (ceil(S / 256), S, B): block z handles row y of item z's crop
__global__ __launch_bounds__(256) void dmx_preprocess_curved_kernel(const PreCurvedArgs p) {
  __shared__ Item s;
  const int b = blockIdx.z;
  stage(s, p.items, p.pieces, p.NP, b, offsetof(dmx_curved_piece, crop));
  const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y;
  if (dx >= p.S) return;
  const dmx_edit_page pg = p.pages[min(max(s.it.page, 0), p.P - 1)];
  if (pg.H <= 0 || pg.W <= 0) return;
  const long long gp = 2 * dx + 1 - p.S, gq = 2 * dy + 1 - p.S;
  const int piece = piece_of(s.it.c, s.M, s.it.rh, (long long)p.S * s.it.ci2 + (long long)s.it.crop_scale * gp,
                             (long long)p.S * s.it.cj2 + (long long)s.it.crop_scale * gq, 2ll * p.S);
  long long X16 = 0, Y16 = 0;                                                   // (a stale table: the sample is the page's corner)
  dmx_persp::coords(s.map[piece], gp, gq, X16, Y16);
  int vi[3], vm[3], vk;
  const int M = s.M;
  pre_pixel((const unsigned char*)pg.original, pg.H, pg.W, X16, Y16,
            [&](int X, int Y) -> int {
              int in = 0;
              for (int k = 0; k < M; ++k) in |= covers(s.cell[k], X, Y);
              return in;
            },
            vi, vm, vk);
  const size_t plane = (size_t)p.S * p.S, lat = (size_t)(p.S >> 3) * (p.S >> 3);
  dmx_resize::pre_store(vi, vm, vk, p.S, dx, dy, p.out_img + (size_t)b * 3 * plane, p.out_masked + (size_t)b * 3 * plane,
                        p.out_mask + (size_t)b * plane, p.out_mask_lat ? p.out_mask_lat + (size_t)b * lat : nullptr);
}

struct RectCurvedArgs {
  const dmx_edit_page* pages; int P;
  const dmx_edit_curved* items; const dmx_curved_piece* pieces; int NP; int B;
  unsigned char* out; long long out_bytes;
};

// The strips of all items: blocks enumerate (item, row, 256-column tile) along grid.x, as the quads' rectify does.  No byte is written at
// or past out_bytes.
__global__ __launch_bounds__(256) void dmx_rectify_curved_kernel(const RectCurvedArgs p) {
  __shared__ int s_lo[DMX_EDIT_MAX_ITEMS];
  __shared__ Item s;
  if ((int)threadIdx.x < p.B) s_lo[threadIdx.x] = p.items[threadIdx.x].rect_block_lo;
  __syncthreads();
  int b = 0;
  for (int i = 1; i < p.B; ++i) b = (int)blockIdx.x >= s_lo[i] ? i : b;
  stage(s, p.items, p.pieces, p.NP, b, offsetof(dmx_curved_piece, strip));
  const dmx_edit_page pg = p.pages[min(max(s.it.page, 0), p.P - 1)];
  const int rw = s.it.rw, rh = s.it.rh;
  if (pg.H <= 0 || pg.W <= 0 || rw <= 0 || rh <= 0 || rw > kSizeMax || s.it.rect_off < 0) return;
  const int tiles = (rw + 255) / 256, local = (int)blockIdx.x - s.it.rect_block_lo;
  if (local < 0 || local / tiles >= rh) return;
  const int j = local / tiles, i = (local % tiles) * 256 + (int)threadIdx.x;
  if (i >= rw) return;
  const long long o = s.it.rect_off + ((long long)j * rw + i) * 3;
  if (o + 3 > p.out_bytes) return;
  const int piece = piece_of(s.it.c, s.M, rh, i, j, 1);
  long long X16 = 0, Y16 = 0;
  dmx_persp::coords(s.map[piece], 2 * i + 1 - rw, 2 * j + 1 - rh, X16, Y16);
  const Tap16 tx = tap16(X16, pg.W), ty = tap16(Y16, pg.H);
#pragma unroll
  for (int c = 0; c < 3; ++c) p.out[o + c] = (unsigned char)page_sample((const unsigned char*)pg.original, pg.W, tx, ty, c);
}

struct PostCurvedArgs {
  const float* vae; int S;
  const dmx_edit_page* pages; int P;
  const dmx_edit_curved* items; const dmx_curved_piece* pieces; int NP; int B;
  int cap;                                   // the cells the block's LDS holds: at least kMaxCells, at least the cells of any page
};

// the paste map of a piece, in the shape dmx_quad::on_crop asks of a frame: `b` is the piece's index in the table
struct PieceFrame {
  const dmx_curved_piece* pieces;
  __device__ __forceinline__ bool paste(const dmx_edit_quad*, int b, int, int x, int y, long long& U16, long long& V16) const {
    const dmx_curved_piece& f = pieces[b];
    return dmx_persp::coords(f.paste, 2ll * x - f.cx2, 2ll * y - f.cy2, U16, V16);
  }
};

// what the paste's scan reads per item: the polygon's bounding box, its cells [cl, cl + M) of the staged cells, its first piece
struct ItemScan { int bx1, by1, bx2, by2, cl, M, piece_lo; };

// The paste over P pages: blocks enumerate (page, row, 256-column tile) along grid.x (dmx_paste::page_block).  A block stages, per item
// of its page, the bounding box and, per cell, corners, edges and bounding box - the maps stay in global memory: a pixel reads one.
__global__ __launch_bounds__(256) void dmx_postprocess_curved_kernel(const PostCurvedArgs p) {
  extern __shared__ QuadEdges s_cell[];
  __shared__ ItemScan s_item[DMX_EDIT_MAX_ITEMS];
  dmx_paste::PageBlock t;
  if (!dmx_paste::page_block(p.pages, p.P, p.B, 65535, t)) return;             // (uniform per block: a stale table)
  if ((int)threadIdx.x < t.n) {
    const dmx_edit_curved& it = p.items[t.lo + threadIdx.x];
    const int n = pairs(it), M = n - 1;
    ItemScan si{it.bx1, it.by1, it.bx2, it.by2, 0, M, it.piece_lo};
    si.cl = min(max((it.piece_lo - p.items[t.lo].piece_lo) / 2, 0), p.cap - M);
    for (int k = 0; k < M; ++k) s_cell[si.cl + k] = cell_edges(it, n, k);
    s_item[threadIdx.x] = si;
  }
  __syncthreads();
  if (t.x >= t.pg.W) return;
  const dmx_edit_page& pg = t.pg;
  const int x = t.x, y = t.y;
  int hit = -1, piece = 0;
  for (int b = t.n - 1; b >= 0 && hit < 0; --b) {
    const ItemScan& si = s_item[b];
    if (x < si.bx1 || x > si.bx2 || y < si.by1 || y > si.by2) continue;
    for (int k = 0; k < si.M; ++k) {
      const QuadEdges& e = s_cell[si.cl + k];
      if (!covers(e, x, y)) continue;
      const long long E = (long long)(e.x[3] - e.x[1]) * ((long long)y - e.y[1]) - (long long)(e.y[3] - e.y[1]) * ((long long)x - e.x[1]);
      hit = b; piece = min(max(si.piece_lo + 2 * k + (E >= 0 ? 0 : 1), 0), p.NP - 1);
      break;
    }
  }
  const unsigned char* ori = (const unsigned char*)pg.original;
  unsigned char *out = (unsigned char*)pg.out, *umask = (unsigned char*)pg.union_mask;
  const size_t o = ((size_t)y * pg.W + x) * 3;
  if (umask) umask[(size_t)y * pg.W + x] = (unsigned char)(hit >= 0);
  long long U16 = 0, V16 = 0;
  const bool paste = hit >= 0 && on_crop(PieceFrame{p.pieces}, nullptr, piece, p.S, x, y, U16, V16);
  if (!paste) { out[o] = ori[o]; out[o + 1] = ori[o + 1]; out[o + 2] = ori[o + 2]; return; }
  const float* vae = p.vae + (size_t)(t.lo + hit) * 3 * p.S * p.S;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[o + c] = post_pixel(vae, p.S, c, U16, V16);
}

// The host-side check of the three tables.  S >= 1: frames and all three maps; S == 0: the strips alone (the frames are not looked at).
// fill == false: the derived fields of all three tables are compared with what the prepare entry fills; true: they are written (the
// page table's by the caller).  A bad page is named by page index, a bad item by its index in the whole table, a bad cell by its number.
// *max_cells: the most cells on one page.
int check_curved(const char* what, const dmx_edit_page* pages, int P, dmx_edit_curved* items, dmx_curved_piece* pieces, int B, int S, bool fill,
                 int* max_cells) {
  DMX_REQUIRE(pages && items && pieces, "%s: null page, item or piece table", what);
  DMX_REQUIRE(P >= 1 && P <= DMX_EDIT_MAX_ITEMS, "%s: %d pages, expected 1 .. %d", what, P, DMX_EDIT_MAX_ITEMS);
  DMX_REQUIRE(B >= 1 && B <= DMX_EDIT_MAX_ITEMS, "%s: %d items, expected 1 .. %d", what, B, DMX_EDIT_MAX_ITEMS);
  DMX_REQUIRE(S >= 0 && S <= 65535, "%s: bad S = %d (0 = strips only, 1 .. 65535)", what, S);
  const int rc = dmx_check_page_table(what, pages, P, B, 65535, "dmx_edit_curved_prepare", !fill);
  if (rc != DMX_OK) return rc;
  long long rect_off = 0, rect_blocks = 0;
  int cells = 0;
  *max_cells = 0;
  for (int q = 0; q < P; ++q) {                                        // the ranges tile [0, B): every item has its page
    const dmx_edit_page& pg = pages[q];
    const int cells_before = cells;
    for (int b = pg.item_lo; b < pg.item_hi; ++b) {
      const dmx_edit_curved& it = items[b];
      DMX_REQUIRE(it.count >= 0 && (it.count & 1) == 0, "%s: item %d: %d points: a curved region has as many points on top as on the bottom", what, b,
                  it.count);
      const int n = it.count / 2, M = n - 1;
      DMX_REQUIRE(n >= 2 && n <= kMaxPairs, "%s: item %d: %d point pairs, expected 2 .. %d", what, b, n, kMaxPairs);
      DMX_REQUIRE(cells + M <= DMX_CURVED_MAX_CELLS, "%s: item %d: more than %d cells in one launch", what, b, DMX_CURVED_MAX_CELLS);
      DMX_REQUIRE(it.page == q, "%s: item %d: page index %d, the item lies in the range of page %d", what, b, it.page, q);
      for (int k = 0; k < 2 * n; ++k) {
        const int pair = k < n ? k : 2 * n - 1 - k;                    // (the last pair closes cell M - 1)
        DMX_REQUIRE(it.x[k] >= 0 && it.x[k] < pg.W && it.y[k] >= 0 && it.y[k] < pg.H, "%s: item %d: cell %d: point %d (%d, %d) lies outside the %dx%d page",
                    what, b, pair < M ? pair : M - 1, k, it.x[k], it.y[k], pg.W, pg.H);
      }
      for (int c = 0; c < M; ++c) {
        const int idx[4] = {c, c + 1, 2 * n - 2 - c, 2 * n - 1 - c};
        long long area2 = 0;
        for (int k = 0; k < 4; ++k) {
          const int a0 = idx[k], a1 = idx[(k + 1) & 3], a2 = idx[(k + 2) & 3];
          const long long ex = it.x[a1] - it.x[a0], ey = it.y[a1] - it.y[a0], fx = it.x[a2] - it.x[a1], fy = it.y[a2] - it.y[a1];
          DMX_REQUIRE(ex * fy - ey * fx >= 0,
                      "%s: item %d: cell %d turns the wrong way at point %d: not convex, or counter-clockwise (top points as read, then bottom points backwards)",
                      what, b, c, a1);
          area2 += (long long)it.x[a0] * it.y[a1] - (long long)it.x[a1] * it.y[a0];
        }
        DMX_REQUIRE(area2 > 0, "%s: item %d: cell %d has no area", what, b, c);
      }
      dmx_edit_curved t = it;
      fill_strip_size(t, n);
      DMX_REQUIRE(t.rh >= 2, "%s: item %d: the strip is thinner than 2 pixels (rh >= 2)", what, b);
      DMX_REQUIRE(t.rw <= kSizeMax && t.rh <= kSizeMax, "%s: item %d: a %dx%d strip, at most %d either way", what, b, t.rw, t.rh, kSizeMax);
      if (S >= 1) {
        const char* wrong = check_frame(t);
        DMX_REQUIRE(!wrong, "%s: item %d: the frame: %s", what, b, wrong);
      }
      t.piece_lo = 2 * cells; t.pieces = 2 * M;
      t.rect_block_lo = (int)rect_blocks; t.rect_blocks = t.rh * cdiv(t.rw, 256);
      t.rect_off = rect_off;
      DMX_REQUIRE(rect_blocks + t.rect_blocks < (1ll << 31), "%s: item %d: the strips need more than 2^31 - 1 blocks of 256 pixels", what, b);
      for (int piece = 0; piece < 2 * M; ++piece) {
        dmx_curved_piece x;
        memset(&x, 0, sizeof x);
        const char* where = "";
        const char* wrong = fill_piece(t, n, piece, S, x, &where);
        DMX_REQUIRE(!wrong, "%s: item %d: cell %d: piece %d: %s: %s", what, b, piece >> 1, piece, where, wrong);
        dmx_curved_piece& have = pieces[t.piece_lo + piece];
        if (fill) { have = x; continue; }
        const bool same = S >= 1 ? memcmp(&x, &have, sizeof x) == 0 : memcmp(&x.strip, &have.strip, sizeof x.strip) == 0;
        DMX_REQUIRE(same, "%s: item %d: cell %d: piece %d: derived fields do not belong to this polygon, frame and S (dmx_edit_curved_prepare fills them)", what,
                    b, piece >> 1, piece);
      }
      if (fill) items[b] = t;
      else
        DMX_REQUIRE(memcmp(&t, &it, sizeof t) == 0, "%s: item %d: derived fields do not belong to this polygon and page table (dmx_edit_curved_prepare fills them)",
                    what, b);
      rect_off += (long long)t.rw * t.rh * 3;
      rect_blocks += t.rect_blocks;
      cells += M;
    }
    *max_cells = cells - cells_before > *max_cells ? cells - cells_before : *max_cells;
  }
  return DMX_OK;
}

// what every launch entry asks of its host tables: prepared tables and the pages' addresses
int check_tables(const char* what, const dmx_edit_page* pages, int P, const dmx_edit_curved* items, const dmx_curved_piece* pieces, int B, int S,
                 bool need_out, int* max_cells) {
  const int rc = check_curved(what, pages, P, const_cast<dmx_edit_curved*>(items), const_cast<dmx_curved_piece*>(pieces), B, S, false, max_cells);
  return rc != DMX_OK ? rc : dmx_check_page_addresses(what, pages, P, need_out);
}

inline int piece_count(const dmx_edit_curved* items_host, int B) { return items_host[B - 1].piece_lo + items_host[B - 1].pieces; }

}  // namespace

extern "C" int dmx_edit_curved_prepare(dmx_edit_page* pages, int P, dmx_edit_curved* items, dmx_curved_piece* pieces, int B, int S) {
  int max_cells = 0;
  const int rc = check_curved("edit_curved_prepare", pages, P, items, pieces, B, S, true, &max_cells);
  if (rc != DMX_OK) return rc;
  int blocks = 0;
  for (int q = 0; q < P; ++q) {
    dmx_edit_page& pg = pages[q];
    pg.block_lo = blocks; pg.blocks = pg.H * cdiv(pg.W, 256);
    blocks += pg.blocks;
  }
  return DMX_OK;
}

extern "C" int dmx_preprocess_curved(const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P, const dmx_edit_curved* items_host,
                                     const dmx_edit_curved* items_device, const dmx_curved_piece* pieces_host, const dmx_curved_piece* pieces_device,
                                     int B, int S, float* out_image, float* out_masked_image, unsigned char* out_mask, float* out_mask_latent,
                                     dmx_stream_t stream) {
  DMX_REQUIRE(pages_device && items_device && pieces_device && out_image && out_masked_image && out_mask, "preprocess_curved: null argument");
  DMX_REQUIRE(S > 0 && S <= 65535 && S % 8 == 0, "preprocess_curved: S = %d is no positive multiple of 8 (up to 65535)", S);
  int max_cells = 0;
  const int rc = check_tables("preprocess_curved", pages_host, P, items_host, pieces_host, B, S, false, &max_cells);
  if (rc != DMX_OK) return rc;
  PreCurvedArgs p{pages_device, P, items_device, pieces_device, piece_count(items_host, B), S, out_image, out_masked_image, out_mask, out_mask_latent};
  hipLaunchKernelGGL(dmx_preprocess_curved_kernel, dim3(cdiv(S, 256), S, B), dim3(256), 0, (hipStream_t)stream, p);
  return dmx_check_launch("dmx_preprocess_curved_kernel");
}

extern "C" int dmx_postprocess_paste_curved(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                            const dmx_edit_curved* items_host, const dmx_edit_curved* items_device,
                                            const dmx_curved_piece* pieces_host, const dmx_curved_piece* pieces_device, int B, dmx_stream_t stream) {
  DMX_REQUIRE(image_vae && pages_device && items_device && pieces_device, "postprocess_paste_curved: null argument");
  DMX_REQUIRE(S > 0 && S <= 65535, "postprocess_paste_curved: bad S = %d (1 .. 65535)", S);
  int max_cells = 0;
  const int rc = check_tables("postprocess_paste_curved", pages_host, P, items_host, pieces_host, B, S, true, &max_cells);
  if (rc != DMX_OK) return rc;
  const int cap = max_cells > kMaxCells ? max_cells : kMaxCells;
  PostCurvedArgs p{image_vae, S, pages_device, P, items_device, pieces_device, piece_count(items_host, B), B, cap};
  hipLaunchKernelGGL(dmx_postprocess_curved_kernel, dmx_paste::paged_grid(pages_host, P), dim3(256), (size_t)cap * sizeof(QuadEdges), (hipStream_t)stream,
                     p);
  return dmx_check_launch("dmx_postprocess_curved_kernel");
}

extern "C" int dmx_rectify_curved(const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P, const dmx_edit_curved* items_host,
                                  const dmx_edit_curved* items_device, const dmx_curved_piece* pieces_host, const dmx_curved_piece* pieces_device,
                                  int B, unsigned char* out, long long out_bytes, dmx_stream_t stream) {
  DMX_REQUIRE(pages_device && items_device && pieces_device && out, "rectify_curved: null argument");
  int max_cells = 0;
  const int rc = check_tables("rectify_curved", pages_host, P, items_host, pieces_host, B, 0, false, &max_cells);
  if (rc != DMX_OK) return rc;
  const dmx_edit_curved& last = items_host[B - 1];
  DMX_REQUIRE(out_bytes >= last.rect_off + (long long)last.rw * last.rh * 3, "rectify_curved: the strips take %lld bytes, the output holds %lld",
              last.rect_off + (long long)last.rw * last.rh * 3, out_bytes);
  RectCurvedArgs p{pages_device, P, items_device, pieces_device, piece_count(items_host, B), B, out, out_bytes};
  hipLaunchKernelGGL(dmx_rectify_curved_kernel, dim3(last.rect_block_lo + last.rect_blocks), dim3(256), 0, (hipStream_t)stream, p);
  return dmx_check_launch("dmx_rectify_curved_kernel");
}
