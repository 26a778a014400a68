// Quadrilateral text regions: the two ends of the editing path for skewed, rotated and keystoned lines (pipeline.edit_quads), beside
// prepost_batch.hip's axis-aligned boxes.  Items are dmx_edit_quad, pages the dmx_edit_page table of the *_pages entries.  Three
// kernels, one launch each: the crop (mask = the quad itself, seen through the frame), the paste (every page pixel mapped back through
// the inverse frame; the last quad that covers a pixel decides) and the rectify (a quad as an upright strip, for the OCR model).  Two
// more for verified edits, beside readback.hip's for boxes: the read-back (K candidates per quad -> the OCR model's pixel_values: paste,
// rectify and Pillow resample of one candidate in one pass, no page and no strip in memory) and the select-paste (the paste of the
// best-scoring candidate per quad, chosen on the device).
// Each kernel is written ONCE, over a frame that says where the sample coordinates come from:
//   SimilarityFrame   one rotation and one scale, the Q15 matrices of dmx_edit_quad (prepost_quad.h): the dmx_*_quads entries;
//   ProjectiveFrame   the homography that takes the quad to its upright strip, from a parallel, index-aligned table of dmx_quad_persp
//                     (prepost_persp.h) - phone photos, signs and scene text, where a line is a trapezoid and the similarity frame leaves
//                     the text keystoned: the dmx_*_quads_persp entries.  Per pixel two 64-bit numerators, one denominator and four
//                     64-bit divisions more.
// The frames themselves live in prepost_quad_frame.h (the blended pastes of prepost_quad_blend.hip are written over them too).
// Everything after the coordinates (taps, rounding, predicate, paste rule, stores) is prepost_quad.h's.  Pure HBM-bound byte work: one
// thread per destination pixel, coalesced plain vector stores, the integer tables staged in LDS once per block, no atomics.
#include "common.h"
#include "kernels.h"
#include "prepost_paste.h"
#include "prepost_quad_frame.h"
#include "glyph_resample.h"

namespace {
using namespace dmx_quad;

struct PreQuadArgs {
  const dmx_edit_page* pages; int P;
  const dmx_edit_quad* quads; int S;
  float* out_img; float* out_masked; unsigned char* out_mask; float* out_mask_lat;
};

// grid (ceil(S / 256), S, B): block z handles row y of quad z's crop
template <class Frame>
__global__ __launch_bounds__(256) void dmx_preprocess_quads_kernel(const PreQuadArgs p, const Frame frame) {
  __shared__ typename Frame::Item s;
  const int b = blockIdx.z;
  frame.stage(s, p.quads, b);
  const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y;
  if (dx >= p.S) return;
  const dmx_edit_page pg = p.pages[min(max(s.q.page, 0), p.P - 1)];
  if (pg.H <= 0 || pg.W <= 0) return;
  long long X16 = 0, Y16 = 0;
  frame.crop(s, 2 * dx + 1 - p.S, 2 * dy + 1 - p.S, X16, Y16);
  int vi[3], vm[3], vk;
  pre_pixel((const unsigned char*)pg.original, pg.H, pg.W, X16, Y16, [&](int X, int Y) -> int { return inside(s.q, X, Y); }, vi, vm, vk);
  const size_t plane = (size_t)p.S * p.S, lat = (size_t)(p.S >> 3) * (p.S >> 3);
  dmx_resize::pre_store(vi, vm, vk, p.S, dx, dy, p.out_img + (size_t)b * 3 * plane, p.out_masked + (size_t)b * 3 * plane,
                        p.out_mask + (size_t)b * plane, p.out_mask_lat ? p.out_mask_lat + (size_t)b * lat : nullptr);
}

struct PostQuadArgs {
  const float* vae; int S;
  const dmx_edit_page* pages; int P;
  const dmx_edit_quad* quads; int B;
};

// The paste over P pages: blocks enumerate (page, row, 256-column tile) along grid.x as in the paged box pastes
// (dmx_paste::page_block); a block stages its page's quads - corners, edges, bounding box - in LDS (stage_edges; the caller's barrier
// follows).  A pixel scans them last to first, stops at the first quad that covers it and is not skipped, and maps itself through THAT
// item's frame (paste_quads_pixel).  row(b) -> item lo + b's row of p.vae, or < 0: the item is skipped - transparent, an earlier quad
// under it still shows -, as paste_pixel of prepost_batch.hip has it; the union mask counts skipped items too.
__device__ __forceinline__ void stage_edges(const PostQuadArgs& p, const dmx_paste::PageBlock& t, QuadEdges* s_e) {
  if ((int)threadIdx.x < t.n) {
    const dmx_edit_quad& q = p.quads[t.lo + threadIdx.x];
    QuadEdges e;
#pragma unroll
    for (int k = 0; k < 4; ++k) { e.x[k] = q.x[k]; e.y[k] = q.y[k]; e.ex[k] = q.ex[k]; e.ey[k] = q.ey[k]; }
    e.bx1 = q.bx1; e.by1 = q.by1; e.bx2 = q.bx2; e.by2 = q.by2;
    s_e[threadIdx.x] = e;
  }
}

template <class Frame, class Row>
__device__ __forceinline__ void paste_quads_pixel(const PostQuadArgs& p, const Frame& frame, const dmx_paste::PageBlock& t, const QuadEdges* s_e,
                                                  Row row) {
  const dmx_edit_page& pg = t.pg;
  const int lo = t.lo, x = t.x, y = t.y;
  int hit = -1, any = 0;
  for (int b = t.n - 1; b >= 0; --b) {
    const QuadEdges& e = s_e[b];
    if (x >= e.bx1 && x <= e.bx2 && y >= e.by1 && y <= e.by2 && inside(e, x, y)) {
      any = 1;
      if (row(b) >= 0) { hit = b; break; }
    }
  }
  const unsigned char* ori = (const unsigned char*)pg.original;
  unsigned char *out = (unsigned char*)pg.out, *umask = (unsigned char*)pg.union_mask;
  const size_t o = ((size_t)y * pg.W + x) * 3;
  if (umask) umask[(size_t)y * pg.W + x] = (unsigned char)any;
  long long U16 = 0, V16 = 0;
  const bool paste = hit >= 0 && on_crop(frame, p.quads, lo + hit, p.S, x, y, U16, V16);
  if (!paste) { out[o] = ori[o]; out[o + 1] = ori[o + 1]; out[o + 2] = ori[o + 2]; return; }
  const float* vae = p.vae + (size_t)row(hit) * 3 * p.S * p.S;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[o + c] = post_pixel(vae, p.S, c, U16, V16);
}

template <class Frame>
__global__ __launch_bounds__(256) void dmx_postprocess_quads_kernel(const PostQuadArgs p, const Frame frame) {
  __shared__ QuadEdges s_e[DMX_EDIT_MAX_ITEMS];
  dmx_paste::PageBlock t;
  if (!dmx_paste::page_block(p.pages, p.P, p.B, 65535, t)) return;             // (uniform per block: a stale table)
  stage_edges(p, t, s_e);
  __syncthreads();
  if (t.x >= t.pg.W) return;
  const int lo = t.lo;
  paste_quads_pixel(p, frame, t, s_e, [lo](int b) -> int { return lo + b; });
}

// Best of K candidates per quad, chosen and pasted in ONE launch: p.vae is [B][K][3][S][S], scores [B][K] lives on the device.  choice is
// [B] over all items and every block derives all of it by the rule of the box pastes (dmx_paste::select_choices, which ends with a
// barrier); block 0 alone stores it, with plain vector stores.  The block then stages ONE int per item of its page beside the edges -
// the item's row of p.vae, or -1 for a skipped item - so that a pixel's scan reads s_row[b] as it reads s_e[b].
template <class Frame>
__global__ __launch_bounds__(256) void dmx_postprocess_select_quads_kernel(const PostQuadArgs p, const Frame frame, const float* scores, int K,
                                                                           float threshold, int* choice) {
  __shared__ QuadEdges s_e[DMX_EDIT_MAX_ITEMS];
  __shared__ float s_score[DMX_EDIT_MAX_ITEMS * DMX_SELECT_MAX_CANDIDATES];
  __shared__ int s_choice[DMX_EDIT_MAX_ITEMS], s_row[DMX_EDIT_MAX_ITEMS];
  dmx_paste::PageBlock t;
  const bool live = dmx_paste::page_block(p.pages, p.P, p.B, 65535, t);
  if (!live && blockIdx.x != 0) return;
  if (live) stage_edges(p, t, s_e);
  dmx_paste::select_choices(scores, p.B, K, threshold, s_score, s_choice, choice, blockIdx.x == 0);
  if (!live) return;                                                           // (uniform per block)
  if ((int)threadIdx.x < t.n) {
    const int b = t.lo + (int)threadIdx.x, k = min(s_choice[b], K - 1);
    s_row[threadIdx.x] = k < 0 ? -1 : b * K + k;
  }
  __syncthreads();
  if (t.x >= t.pg.W) return;
  paste_quads_pixel(p, frame, t, s_e, [&](int b) -> int { return s_row[b]; });
}

struct ReadQuadArgs {
  const float* vae; int S;                                 // decoder outputs [B][K][3][S][S] in [-1, 1]
  const dmx_edit_page* pages; int P;
  const dmx_edit_quad* quads; const dmx_readback_pass* passes; int K;
  const int* tab; const float* norm;
  int S_h, S_w; float* out; unsigned char* out_u8;         // [B*K][3][S_h][S_w]
};

// OCR read-back of K candidates per quad: from the decoder outputs straight to the OCR model's pixel_values, grid (ceil(S_w / 256), S_h,
// B * K), block z = row r = b * K + k.  The row is the Pillow resample (glyph_resample.h) of quad b's upright strip of the page that the
// paste above would write for candidate r ALONE over the original page - a one-quad table -, but neither that page nor the strip exists:
// strip byte (i, j) is the rectify kernel's sample4 of four page taps, and a tap (after its clamp to the page) is the candidate's
// post_pixel where the paste would have pasted it - inside quad b and on its crop (on_crop) -, the original byte elsewhere.  A thread
// keeps the three channels of the strip pixel it computed last: the resample asks for them one after the other.
template <class Frame>
__global__ __launch_bounds__(256) void dmx_readback_quads_kernel(const ReadQuadArgs p, const Frame frame) {
  __shared__ typename Frame::Item s;
  const int r = blockIdx.z, b = r / p.K;                                       // (the grid is B * K rows deep: b lies inside the tables)
  frame.stage(s, p.quads, b);
  const int ox = blockIdx.x * blockDim.x + threadIdx.x, oy = blockIdx.y;
  if (ox >= p.S_w) return;
  const dmx_edit_page pg = p.pages[min(max(s.q.page, 0), p.P - 1)];
  if (pg.H <= 0 || pg.W <= 0) return;
  const dmx_readback_pass ps = p.passes[b];
  const int rw = max(s.q.rw, 1), rh = max(s.q.rh, 1);
  const unsigned char* ori = (const unsigned char*)pg.original;
  const float* vae = p.vae + (size_t)r * 3 * p.S * p.S;
  int ly = -1, lx = -1, lv[3] = {0, 0, 0};
  auto px = [&](int y, int x, int c) -> int {                                  // byte (x, y) of the strip of the pasted page
    if (y != ly || x != lx) {
      ly = y; lx = x;
      long long X16 = 0, Y16 = 0;
      frame.strip(s, 2ll * x + 1 - rw, 2ll * y + 1 - rh, X16, Y16);
      const Tap16 tx = tap16(X16, pg.W), ty = tap16(Y16, pg.H);
      bool gen[2][2];
      long long U16[2][2], V16[2][2];
#pragma unroll
      for (int ky = 0; ky < 2; ++ky)
#pragma unroll
        for (int kx = 0; kx < 2; ++kx) {
          const int X = kx ? tx.i1 : tx.i0, Y = ky ? ty.i1 : ty.i0;
          U16[ky][kx] = V16[ky][kx] = 0;
          gen[ky][kx] = inside(s.q, X, Y) && on_crop(frame, p.quads, b, p.S, X, Y, U16[ky][kx], V16[ky][kx]);
        }
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        lv[ch] = sample4(tx, ty, [&](int kx, int ky) -> long long {
          if (gen[ky][kx]) return post_pixel(vae, p.S, ch, U16[ky][kx], V16[ky][kx]);
          return ori[((size_t)(ky ? ty.i1 : ty.i0) * pg.W + (kx ? tx.i1 : tx.i0)) * 3 + ch];
        });
    }
    return lv[c];
  };
  const dmx_glyph::Passes tp{ps.h_off, ps.h_taps, ps.v_off, ps.v_taps};
  int v[3];
  dmx_glyph::glyph_resample_pixel(px, rh, rw, p.tab, tp, p.S_h, p.S_w, ox, oy, v);
  const size_t plane = (size_t)p.S_h * p.S_w, o = (size_t)r * 3 * plane + (size_t)oy * p.S_w + ox;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    p.out[o + c * plane] = p.norm[c * 256 + v[c]];
    if (p.out_u8) p.out_u8[o + c * plane] = (unsigned char)v[c];
  }
}

struct RectQuadArgs {
  const dmx_edit_page* pages; int P;
  const dmx_edit_quad* quads; int B;
  unsigned char* out; long long out_bytes;
};

// The strips of all quads: blocks enumerate (quad, row, 256-column tile) along grid.x; a block finds its quad by a uniform scan of the
// rect_block_lo values (staged in LDS), stages that item and writes one tile of one strip row.  No byte is written at or past out_bytes.
template <class Frame>
__global__ __launch_bounds__(256) void dmx_rectify_quads_kernel(const RectQuadArgs p, const Frame frame) {
  __shared__ int s_lo[DMX_EDIT_MAX_ITEMS];
  __shared__ typename Frame::Item s;
  if ((int)threadIdx.x < p.B) s_lo[threadIdx.x] = p.quads[threadIdx.x].rect_block_lo;
  __syncthreads();
  int b = 0;
  for (int i = 1; i < p.B; ++i) b = (int)blockIdx.x >= s_lo[i] ? i : b;
  frame.stage(s, p.quads, b);
  const dmx_edit_page pg = p.pages[min(max(s.q.page, 0), p.P - 1)];
  const int rw = s.q.rw, rh = s.q.rh;
  if (pg.H <= 0 || pg.W <= 0 || rw <= 0 || rh <= 0 || rw > (1 << 20) || s.q.rect_off < 0) return;
  const int tiles = (rw + 255) / 256, local = (int)blockIdx.x - s.q.rect_block_lo;
  if (local < 0 || local / tiles >= rh) return;
  const int j = local / tiles, i = (local % tiles) * 256 + (int)threadIdx.x;
  if (i >= rw) return;
  const long long o = s.q.rect_off + ((long long)j * rw + i) * 3;
  if (o + 3 > p.out_bytes) return;
  long long X16 = 0, Y16 = 0;
  frame.strip(s, 2 * i + 1 - rw, 2 * j + 1 - rh, X16, Y16);
  const Tap16 tx = tap16(X16, pg.W), ty = tap16(Y16, pg.H);
#pragma unroll
  for (int c = 0; c < 3; ++c) p.out[o + c] = (unsigned char)page_sample((const unsigned char*)pg.original, pg.W, tx, ty, c);
}

// The host-side checks of a page table and a quad table.  frames: the frame fields are looked at (the rectify entry and the projective
// entries read none of them).  prepared: the derived fields of both tables are compared with what dmx_edit_quads_prepare fills.  A bad
// page is named by page index, a bad quad by its index in the whole table.
int check_quads(const char* what, const dmx_edit_page* pages, int P, const dmx_edit_quad* quads, int B, int S, bool frames, bool prepared) {
  DMX_REQUIRE(pages && quads, "%s: null page or quad table", what);
  DMX_REQUIRE(P >= 1 && P <= DMX_EDIT_MAX_ITEMS, "%s: %d pages, expected 1 .. %d", what, P, DMX_EDIT_MAX_ITEMS);
  DMX_REQUIRE(B >= 1 && B <= DMX_EDIT_MAX_ITEMS, "%s: %d items, expected 1 .. %d", what, B, DMX_EDIT_MAX_ITEMS);
  DMX_REQUIRE(!frames || (S >= 1 && S <= 65535), "%s: bad S = %d (1 .. 65535)", what, S);
  const int rc = dmx_check_page_table(what, pages, P, B, 65535, "dmx_edit_quads_prepare", prepared);
  if (rc != DMX_OK) return rc;
  long long rect_off = 0, rect_blocks = 0;
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

// The host-side check of the projective table beside checked, PREPARED page and quad tables.  S >= 1: frames and all three maps; S == 0:
// the strip maps alone (the rectify entry reads nothing else).  fill == null: the derived fields are compared with what the prepare
// entry fills; otherwise they are written there.  A bad item is named by its index in the whole table.
int check_persp(const char* what, const dmx_edit_quad* quads, const dmx_quad_persp* persp, dmx_quad_persp* fill, int B, int S) {
  const bool prepared = fill == nullptr;
  DMX_REQUIRE(persp, "%s: null projective table", what);
  for (int b = 0; b < B; ++b) {
    dmx_quad_persp t = persp[b];
    const char *where = "", *wrong = nullptr;
    if (S >= 1) {
      wrong = dmx_persp::fill_derived(quads[b], t, S, &where);
    } else {
      where = "the strip";
      wrong = dmx_persp::fill_strip(quads[b], t);
    }
    DMX_REQUIRE(!wrong, "%s: item %d: %s: %s", what, b, where, wrong);
    if (!prepared) { fill[b] = t; continue; }
    const bool same = S >= 1 ? memcmp(&t, &persp[b], sizeof t) == 0 : memcmp(&t.strip, &persp[b].strip, sizeof t.strip) == 0;
    DMX_REQUIRE(same, "%s: item %d: derived fields do not belong to this quad, projective frame and S (dmx_edit_quads_persp_prepare fills them)", what, b);
  }
  return DMX_OK;
}

// what every launch entry asks of its host tables: prepared page and quad tables (check_quads) and the pages' addresses
int check_tables(const char* what, const dmx_edit_page* pages, int P, const dmx_edit_quad* quads, int B, int S, bool frames, bool need_out) {
  const int rc = check_quads(what, pages, P, quads, B, S, frames, true);
  return rc != DMX_OK ? rc : dmx_check_page_addresses(what, pages, P, need_out);
}

// The launches, one per stage; the tables are checked.  `kernel` names the launch in the last-error string.
template <class Frame>
int launch_pre(const char* kernel, const Frame& frame, const dmx_edit_page* pages_device, int P, const dmx_edit_quad* quads_device, int B, int S,
               float* out_image, float* out_masked_image, unsigned char* out_mask, float* out_mask_latent, dmx_stream_t stream) {
  PreQuadArgs p{pages_device, P, quads_device, S, out_image, out_masked_image, out_mask, out_mask_latent};
  hipLaunchKernelGGL(dmx_preprocess_quads_kernel<Frame>, dim3(cdiv(S, 256), S, B), dim3(256), 0, (hipStream_t)stream, p, frame);
  return dmx_check_launch(kernel);
}

template <class Frame>
int launch_post(const char* kernel, const Frame& frame, const float* image_vae, int S, const dmx_edit_page* pages_host,
                const dmx_edit_page* pages_device, int P, const dmx_edit_quad* quads_device, int B, dmx_stream_t stream) {
  PostQuadArgs p{image_vae, S, pages_device, P, quads_device, B};
  hipLaunchKernelGGL(dmx_postprocess_quads_kernel<Frame>, dim3(pages_host[P - 1].block_lo + pages_host[P - 1].blocks), dim3(256), 0,
                     (hipStream_t)stream, p, frame);
  return dmx_check_launch(kernel);
}

template <class Frame>
int launch_select(const char* kernel, const Frame& frame, const float* image_vae, int S, const float* scores, float threshold, int* choice,
                  const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P, const dmx_edit_quad* quads_device, int B, int K,
                  dmx_stream_t stream) {
  PostQuadArgs p{image_vae, S, pages_device, P, quads_device, B};
  hipLaunchKernelGGL(dmx_postprocess_select_quads_kernel<Frame>, dim3(pages_host[P - 1].block_lo + pages_host[P - 1].blocks), dim3(256), 0,
                     (hipStream_t)stream, p, frame, scores, K, threshold, choice);
  return dmx_check_launch(kernel);
}

// what the read-back asks of checked, prepared quads beyond their tables: the pass tables of every strip (source size rw x rh)
int check_readback_quads(const char* what, const dmx_edit_quad* quads_host, const dmx_readback_pass* passes_host, int B, int max_taps,
                         long long table_ints, int S_h, int S_w) {
  for (int b = 0; b < B; ++b) {
    const int rc = dmx_check_readback_item(what, b, passes_host[b], quads_host[b].rw, quads_host[b].rh, max_taps, table_ints, S_h, S_w);
    if (rc != DMX_OK) return rc;
  }
  return DMX_OK;
}

template <class Frame>
int launch_readback(const char* kernel, const Frame& frame, const float* image_vae, int S, const dmx_edit_page* pages_device, int P,
                    const dmx_edit_quad* quads_device, int B, int K, const int* tables, const float* norm, const dmx_readback_pass* passes_device,
                    int S_h, int S_w, float* out_pixel_values, unsigned char* out_resized, dmx_stream_t stream) {
  ReadQuadArgs p{image_vae, S, pages_device, P, quads_device, passes_device, K, tables, norm, S_h, S_w, out_pixel_values, out_resized};
  hipLaunchKernelGGL(dmx_readback_quads_kernel<Frame>, dim3(cdiv(S_w, 256), S_h, B * K), dim3(256), 0, (hipStream_t)stream, p, frame);
  return dmx_check_launch(kernel);
}

template <class Frame>
int launch_rectify(const char* what, const char* kernel, const Frame& frame, const dmx_edit_page* pages_device, int P,
                   const dmx_edit_quad* quads_host, const dmx_edit_quad* quads_device, int B, unsigned char* out, long long out_bytes,
                   dmx_stream_t stream) {
  const dmx_edit_quad& last = quads_host[B - 1];
  DMX_REQUIRE(out_bytes >= last.rect_off + (long long)last.rw * last.rh * 3, "%s: the strips take %lld bytes, the output holds %lld", what,
              last.rect_off + (long long)last.rw * last.rh * 3, out_bytes);
  RectQuadArgs p{pages_device, P, quads_device, B, out, out_bytes};
  hipLaunchKernelGGL(dmx_rectify_quads_kernel<Frame>, dim3(last.rect_block_lo + last.rect_blocks), dim3(256), 0, (hipStream_t)stream, p, frame);
  return dmx_check_launch(kernel);
}

}  // namespace

int dmx_check_quad_tables(const char* what, const dmx_edit_page* pages, int P, const dmx_edit_quad* quads, int B, int S, bool frames, bool need_out) {
  return check_tables(what, pages, P, quads, B, S, frames, need_out);
}
int dmx_check_quad_persp(const char* what, const dmx_edit_quad* quads, const dmx_quad_persp* persp, int B, int S) {
  return check_persp(what, quads, persp, nullptr, B, S);
}

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

extern "C" int dmx_edit_quads_persp_prepare(const dmx_edit_page* pages, int P, const dmx_edit_quad* quads, dmx_quad_persp* persp, int B, int S) {
  DMX_REQUIRE(S >= 0 && S <= 65535, "edit_quads_persp_prepare: bad S = %d (0 = strips only, 1 .. 65535)", S);
  const int rc = check_quads("edit_quads_persp_prepare", pages, P, quads, B, 0, false, true);
  return rc != DMX_OK ? rc : check_persp("edit_quads_persp_prepare", quads, persp, persp, B, S);
}

// ---- the similarity frame
extern "C" int dmx_preprocess_quads(const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P, const dmx_edit_quad* quads_host,
                                    const dmx_edit_quad* quads_device, int B, int S, float* out_image, float* out_masked_image,
                                    unsigned char* out_mask, float* out_mask_latent, dmx_stream_t stream) {
  DMX_REQUIRE(pages_device && quads_device && out_image && out_masked_image && out_mask, "preprocess_quads: null argument");
  DMX_REQUIRE(S > 0 && S <= 65535 && S % 8 == 0, "preprocess_quads: S = %d is no positive multiple of 8 (up to 65535)", S);
  const int rc = check_tables("preprocess_quads", pages_host, P, quads_host, B, S, true, false);
  if (rc != DMX_OK) return rc;
  return launch_pre("dmx_preprocess_quads_kernel", SimilarityFrame{}, pages_device, P, quads_device, B, S, out_image, out_masked_image, out_mask,
                    out_mask_latent, stream);
}

extern "C" int dmx_postprocess_paste_quads(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                           const dmx_edit_quad* quads_host, const dmx_edit_quad* quads_device, int B, dmx_stream_t stream) {
  DMX_REQUIRE(image_vae && pages_device && quads_device, "postprocess_paste_quads: null argument");
  const int rc = check_tables("postprocess_paste_quads", pages_host, P, quads_host, B, S, true, true);
  if (rc != DMX_OK) return rc;
  return launch_post("dmx_postprocess_quads_kernel", SimilarityFrame{}, image_vae, S, pages_host, pages_device, P, quads_device, B, stream);
}

extern "C" int dmx_rectify_quads(const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P, const dmx_edit_quad* quads_host,
                                 const dmx_edit_quad* quads_device, int B, unsigned char* out, long long out_bytes, dmx_stream_t stream) {
  DMX_REQUIRE(pages_device && quads_device && out, "rectify_quads: null argument");
  const int rc = check_tables("rectify_quads", pages_host, P, quads_host, B, 0, false, false);
  if (rc != DMX_OK) return rc;
  return launch_rectify("rectify_quads", "dmx_rectify_quads_kernel", SimilarityFrame{}, pages_device, P, quads_host, quads_device, B, out, out_bytes,
                        stream);
}

extern "C" int dmx_readback_pixel_values_quads(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                               const dmx_edit_quad* quads_host, const dmx_edit_quad* quads_device, int B, int K, const int* tables,
                                               long long table_ints, const float* norm, const dmx_readback_pass* passes_host,
                                               const dmx_readback_pass* passes_device, int max_taps, int S_h, int S_w, float* out_pixel_values,
                                               unsigned char* out_resized, dmx_stream_t stream) {
  const char* what = "readback_pixel_values_quads";
  DMX_REQUIRE(image_vae && pages_device && quads_device && tables && norm && passes_host && passes_device && out_pixel_values, "%s: null argument", what);
  int rc = dmx_check_readback_scalars(what, K, max_taps, table_ints, S_h, S_w);
  if (rc == DMX_OK) rc = check_tables(what, pages_host, P, quads_host, B, S, true, false);
  if (rc == DMX_OK) rc = check_readback_quads(what, quads_host, passes_host, B, max_taps, table_ints, S_h, S_w);
  if (rc != DMX_OK) return rc;
  return launch_readback("dmx_readback_quads_kernel", SimilarityFrame{}, image_vae, S, pages_device, P, quads_device, B, K, tables, norm,
                         passes_device, S_h, S_w, out_pixel_values, out_resized, stream);
}

extern "C" int dmx_postprocess_paste_select_quads(const float* image_vae, int S, const float* scores, float threshold, int* choice,
                                                  const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                                  const dmx_edit_quad* quads_host, const dmx_edit_quad* quads_device, int B, int K,
                                                  dmx_stream_t stream) {
  const char* what = "postprocess_paste_select_quads";
  DMX_REQUIRE(image_vae && scores && choice && pages_device && quads_device, "%s: null argument", what);
  int rc = dmx_check_select_scalars(what, K, threshold);
  if (rc == DMX_OK) rc = check_tables(what, pages_host, P, quads_host, B, S, true, true);
  if (rc != DMX_OK) return rc;
  return launch_select("dmx_postprocess_select_quads_kernel", SimilarityFrame{}, image_vae, S, scores, threshold, choice, pages_host, pages_device, P,
                       quads_device, B, K, stream);
}

// ---- the projective frame: the quad table's own frames are placeholders, not looked at
extern "C" int dmx_preprocess_quads_persp(const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P, const dmx_edit_quad* quads_host,
                                          const dmx_edit_quad* quads_device, const dmx_quad_persp* persp_host, const dmx_quad_persp* persp_device,
                                          int B, int S, float* out_image, float* out_masked_image, unsigned char* out_mask,
                                          float* out_mask_latent, dmx_stream_t stream) {
  DMX_REQUIRE(pages_device && quads_device && persp_device && out_image && out_masked_image && out_mask, "preprocess_quads_persp: null argument");
  DMX_REQUIRE(S > 0 && S <= 65535 && S % 8 == 0, "preprocess_quads_persp: S = %d is no positive multiple of 8 (up to 65535)", S);
  int rc = check_tables("preprocess_quads_persp", pages_host, P, quads_host, B, 0, false, false);
  if (rc == DMX_OK) rc = check_persp("preprocess_quads_persp", quads_host, persp_host, nullptr, B, S);
  if (rc != DMX_OK) return rc;
  return launch_pre("dmx_preprocess_quads_persp_kernel", ProjectiveFrame{persp_device}, pages_device, P, quads_device, B, S, out_image,
                    out_masked_image, out_mask, out_mask_latent, stream);
}

extern "C" int dmx_postprocess_paste_quads_persp(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device,
                                                 int P, const dmx_edit_quad* quads_host, const dmx_edit_quad* quads_device,
                                                 const dmx_quad_persp* persp_host, const dmx_quad_persp* persp_device, int B, dmx_stream_t stream) {
  DMX_REQUIRE(image_vae && pages_device && quads_device && persp_device, "postprocess_paste_quads_persp: null argument");
  DMX_REQUIRE(S > 0 && S <= 65535, "postprocess_paste_quads_persp: bad S = %d (1 .. 65535)", S);
  int rc = check_tables("postprocess_paste_quads_persp", pages_host, P, quads_host, B, 0, false, true);
  if (rc == DMX_OK) rc = check_persp("postprocess_paste_quads_persp", quads_host, persp_host, nullptr, B, S);
  if (rc != DMX_OK) return rc;
  return launch_post("dmx_postprocess_quads_persp_kernel", ProjectiveFrame{persp_device}, image_vae, S, pages_host, pages_device, P, quads_device, B,
                     stream);
}

extern "C" int dmx_rectify_quads_persp(const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P, const dmx_edit_quad* quads_host,
                                       const dmx_edit_quad* quads_device, const dmx_quad_persp* persp_host, const dmx_quad_persp* persp_device, int B,
                                       unsigned char* out, long long out_bytes, dmx_stream_t stream) {
  DMX_REQUIRE(pages_device && quads_device && persp_device && out, "rectify_quads_persp: null argument");
  int rc = check_tables("rectify_quads_persp", pages_host, P, quads_host, B, 0, false, false);
  if (rc == DMX_OK) rc = check_persp("rectify_quads_persp", quads_host, persp_host, nullptr, B, 0);
  if (rc != DMX_OK) return rc;
  return launch_rectify("rectify_quads_persp", "dmx_rectify_quads_persp_kernel", ProjectiveFrame{persp_device}, pages_device, P, quads_host,
                        quads_device, B, out, out_bytes, stream);
}

extern "C" int dmx_readback_pixel_values_quads_persp(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device,
                                                     int P, const dmx_edit_quad* quads_host, const dmx_edit_quad* quads_device,
                                                     const dmx_quad_persp* persp_host, const dmx_quad_persp* persp_device, int B, int K,
                                                     const int* tables, long long table_ints, const float* norm,
                                                     const dmx_readback_pass* passes_host, const dmx_readback_pass* passes_device, int max_taps,
                                                     int S_h, int S_w, float* out_pixel_values, unsigned char* out_resized, dmx_stream_t stream) {
  const char* what = "readback_pixel_values_quads_persp";
  DMX_REQUIRE(image_vae && pages_device && quads_device && persp_device && tables && norm && passes_host && passes_device && out_pixel_values,
              "%s: null argument", what);
  DMX_REQUIRE(S > 0 && S <= 65535, "%s: bad S = %d (1 .. 65535)", what, S);
  int rc = dmx_check_readback_scalars(what, K, max_taps, table_ints, S_h, S_w);
  if (rc == DMX_OK) rc = check_tables(what, pages_host, P, quads_host, B, 0, false, false);
  if (rc == DMX_OK) rc = check_persp(what, quads_host, persp_host, nullptr, B, S);
  if (rc == DMX_OK) rc = check_readback_quads(what, quads_host, passes_host, B, max_taps, table_ints, S_h, S_w);
  if (rc != DMX_OK) return rc;
  return launch_readback("dmx_readback_quads_persp_kernel", ProjectiveFrame{persp_device}, image_vae, S, pages_device, P, quads_device, B, K, tables,
                         norm, passes_device, S_h, S_w, out_pixel_values, out_resized, stream);
}

extern "C" int dmx_postprocess_paste_select_quads_persp(const float* image_vae, int S, const float* scores, float threshold, int* choice,
                                                        const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                                        const dmx_edit_quad* quads_host, const dmx_edit_quad* quads_device,
                                                        const dmx_quad_persp* persp_host, const dmx_quad_persp* persp_device, int B, int K,
                                                        dmx_stream_t stream) {
  const char* what = "postprocess_paste_select_quads_persp";
  DMX_REQUIRE(image_vae && scores && choice && pages_device && quads_device && persp_device, "%s: null argument", what);
  DMX_REQUIRE(S > 0 && S <= 65535, "%s: bad S = %d (1 .. 65535)", what, S);
  int rc = dmx_check_select_scalars(what, K, threshold);
  if (rc == DMX_OK) rc = check_tables(what, pages_host, P, quads_host, B, 0, false, true);
  if (rc == DMX_OK) rc = check_persp(what, quads_host, persp_host, nullptr, B, S);
  if (rc != DMX_OK) return rc;
  return launch_select("dmx_postprocess_select_quads_persp_kernel", ProjectiveFrame{persp_device}, image_vae, S, scores, threshold, choice, pages_host,
                       pages_device, P, quads_device, B, K, stream);
}
