// Quadrilateral text regions in PERSPECTIVE: prepost_quad.hip's three kernels with the coordinates of a projective frame - the
// homography that takes the quad to its upright strip - for phone photos, signs and scene text, where a line is a trapezoid and one
// rotation and one scale (the similarity frame) leave the text keystoned.  Items are dmx_edit_quad with a parallel, index-aligned table of
// dmx_quad_persp; pages the dmx_edit_page table.  One launch each, the launch shapes of prepost_quad.hip; the arithmetic is
// prepost_persp.h, everything after the coordinates (taps, rounding, predicate, paste rule, stores) is prepost_quad.h's, called.
// Per pixel two 64-bit numerators, one denominator and four 64-bit divisions are new; the stores stay plain, coalesced vector stores.
#include "common.h"
#include "kernels.h"
#include "prepost_persp.h"

namespace {
using namespace dmx_quad;
using dmx_persp::coords;

constexpr int kQuadInts = (int)(sizeof(dmx_edit_quad) / sizeof(int));
constexpr int kPerspInts = (int)(sizeof(dmx_quad_persp) / sizeof(int));
static_assert(sizeof(dmx_edit_quad) % sizeof(int) == 0 && sizeof(dmx_quad_persp) % sizeof(int) == 0 && kQuadInts + kPerspInts <= 256,
              "a block stages one quad and its projective frame with one int per thread");

// one entry of each table into LDS, one int per thread; ends with a barrier
__device__ __forceinline__ void stage_item(dmx_edit_quad* s_q, dmx_quad_persp* s_x, const dmx_edit_quad* q, const dmx_quad_persp* x) {
  const int t = threadIdx.x;
  if (t < kQuadInts) ((int*)s_q)[t] = ((const int*)q)[t];
  else if (t < kQuadInts + kPerspInts) ((int*)s_x)[t - kQuadInts] = ((const int*)x)[t - kQuadInts];
  __syncthreads();
}

struct PrePerspArgs {
  const dmx_edit_page* pages; int P;
  const dmx_edit_quad* quads; const dmx_quad_persp* persp; int S;
  float* out_img; float* out_masked; unsigned char* out_mask; float* out_mask_lat;
};

// grid (ceil(S / 256), S, B): block z handles row y of quad z's crop
__global__ __launch_bounds__(256) void dmx_preprocess_quads_persp_kernel(const PrePerspArgs p) {
  __shared__ dmx_edit_quad s_q;
  __shared__ dmx_quad_persp s_x;
  const int b = blockIdx.z;
  stage_item(&s_q, &s_x, p.quads + b, p.persp + b);
  const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y;
  if (dx >= p.S) return;
  const dmx_edit_page pg = p.pages[min(max(s_q.page, 0), p.P - 1)];
  if (pg.H <= 0 || pg.W <= 0) return;
  long long X16 = 0, Y16 = 0;
  coords(s_x.crop, 2 * dx + 1 - p.S, 2 * dy + 1 - p.S, X16, Y16);                // (a stale table: the page's corner; tap16 clamps anyway)
  int vi[3], vm[3], vk;
  pre_pixel((const unsigned char*)pg.original, pg.H, pg.W, X16, Y16, [&](int X, int Y) -> int { return inside(s_q, X, Y); }, vi, vm, vk);
  const size_t plane = (size_t)p.S * p.S, lat = (size_t)(p.S >> 3) * (p.S >> 3);
  dmx_resize::pre_store(vi, vm, vk, p.S, dx, dy, p.out_img + (size_t)b * 3 * plane, p.out_masked + (size_t)b * 3 * plane,
                        p.out_mask + (size_t)b * plane, p.out_mask_lat ? p.out_mask_lat + (size_t)b * lat : nullptr);
}

struct PostPerspArgs {
  const float* vae; int S;
  const dmx_edit_page* pages; int P;
  const dmx_edit_quad* quads; const dmx_quad_persp* persp; int B;
};

// The paste over P pages: blocks enumerate (page, row, 256-column tile) along grid.x; a block finds its page by a uniform scan of the
// block_lo values and stages the page's quads - corners, edges, bounding box - in LDS.  A pixel scans them last to first, stops at the
// first quad that covers it and maps itself through THAT item's page -> crop homography.
__global__ __launch_bounds__(256) void dmx_postprocess_quads_persp_kernel(const PostPerspArgs p) {
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
    const dmx_quad_persp& f = p.persp[lo + hit];
    const long long top = ((long long)p.S << 16) - 32768;
    paste = coords(f.paste, 2ll * x - f.cx2, 2ll * y - f.cy2, U16, V16) && U16 >= -32768 && U16 < top && V16 >= -32768 && V16 < top;
  }
  if (!paste) { out[o] = ori[o]; out[o + 1] = ori[o + 1]; out[o + 2] = ori[o + 2]; return; }
  const float* vae = p.vae + (size_t)(lo + hit) * 3 * p.S * p.S;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[o + c] = post_pixel(vae, p.S, c, U16, V16);
}

struct RectPerspArgs {
  const dmx_edit_page* pages; int P;
  const dmx_edit_quad* quads; const dmx_quad_persp* persp; int B;
  unsigned char* out; long long out_bytes;
};

// The strips of all quads: blocks enumerate (quad, row, 256-column tile) along grid.x; a block finds its quad by a uniform scan of the
// rect_block_lo values (staged in LDS), stages that item and writes one tile of one strip row.  No byte is written at or past out_bytes.
__global__ __launch_bounds__(256) void dmx_rectify_quads_persp_kernel(const RectPerspArgs p) {
  __shared__ int s_lo[DMX_EDIT_MAX_ITEMS];
  __shared__ dmx_edit_quad s_q;
  __shared__ dmx_quad_persp s_x;
  if ((int)threadIdx.x < p.B) s_lo[threadIdx.x] = p.quads[threadIdx.x].rect_block_lo;
  __syncthreads();
  int b = 0;
  for (int i = 1; i < p.B; ++i) b = (int)blockIdx.x >= s_lo[i] ? i : b;
  stage_item(&s_q, &s_x, p.quads + b, p.persp + b);
  const dmx_edit_page pg = p.pages[min(max(s_q.page, 0), p.P - 1)];
  const int rw = s_q.rw, rh = s_q.rh;
  if (pg.H <= 0 || pg.W <= 0 || rw <= 0 || rh <= 0 || rw > (1 << 20) || s_q.rect_off < 0) return;
  const int tiles = (rw + 255) / 256, local = (int)blockIdx.x - s_q.rect_block_lo;
  if (local < 0 || local / tiles >= rh) return;
  const int j = local / tiles, i = (local % tiles) * 256 + (int)threadIdx.x;
  if (i >= rw) return;
  const long long o = s_q.rect_off + ((long long)j * rw + i) * 3;
  if (o + 3 > p.out_bytes) return;
  long long X16 = 0, Y16 = 0;
  coords(s_x.strip, 2 * i + 1 - rw, 2 * j + 1 - rh, X16, Y16);
  const Tap16 tx = tap16(X16, pg.W), ty = tap16(Y16, pg.H);
#pragma unroll
  for (int c = 0; c < 3; ++c) p.out[o + c] = (unsigned char)page_sample((const unsigned char*)pg.original, pg.W, tx, ty, c);
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
}  // namespace

extern "C" int dmx_edit_quads_persp_prepare(const dmx_edit_page* pages, int P, const dmx_edit_quad* quads, dmx_quad_persp* persp, int B, int S) {
  DMX_REQUIRE(S >= 0 && S <= 65535, "edit_quads_persp_prepare: bad S = %d (0 = strips only, 1 .. 65535)", S);
  const int rc = check_quads("edit_quads_persp_prepare", pages, P, quads, B, 0, false, true);
  return rc != DMX_OK ? rc : check_persp("edit_quads_persp_prepare", quads, persp, persp, B, S);
}

extern "C" int dmx_preprocess_quads_persp(const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P, const dmx_edit_quad* quads_host,
                                          const dmx_edit_quad* quads_device, const dmx_quad_persp* persp_host, const dmx_quad_persp* persp_device,
                                          int B, int S, float* out_image, float* out_masked_image, unsigned char* out_mask,
                                          float* out_mask_latent, dmx_stream_t stream) {
  DMX_REQUIRE(pages_device && quads_device && persp_device && out_image && out_masked_image && out_mask, "preprocess_quads_persp: null argument");
  DMX_REQUIRE(S > 0 && S <= 65535 && S % 8 == 0, "preprocess_quads_persp: S = %d is no positive multiple of 8 (up to 65535)", S);
  int rc = check_quads("preprocess_quads_persp", pages_host, P, quads_host, B, 0, false, true);
  if (rc == DMX_OK) rc = check_quad_pages("preprocess_quads_persp", pages_host, P, false);
  if (rc == DMX_OK) rc = check_persp("preprocess_quads_persp", quads_host, persp_host, nullptr, B, S);
  if (rc != DMX_OK) return rc;
  PrePerspArgs p{pages_device, P, quads_device, persp_device, S, out_image, out_masked_image, out_mask, out_mask_latent};
  hipLaunchKernelGGL(dmx_preprocess_quads_persp_kernel, dim3(cdiv(S, 256), S, B), dim3(256), 0, (hipStream_t)stream, p);
  return dmx_check_launch("dmx_preprocess_quads_persp_kernel");
}

extern "C" int dmx_postprocess_paste_quads_persp(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device,
                                                 int P, const dmx_edit_quad* quads_host, const dmx_edit_quad* quads_device,
                                                 const dmx_quad_persp* persp_host, const dmx_quad_persp* persp_device, int B, dmx_stream_t stream) {
  DMX_REQUIRE(image_vae && pages_device && quads_device && persp_device, "postprocess_paste_quads_persp: null argument");
  DMX_REQUIRE(S > 0 && S <= 65535, "postprocess_paste_quads_persp: bad S = %d (1 .. 65535)", S);
  int rc = check_quads("postprocess_paste_quads_persp", pages_host, P, quads_host, B, 0, false, true);
  if (rc == DMX_OK) rc = check_quad_pages("postprocess_paste_quads_persp", pages_host, P, true);
  if (rc == DMX_OK) rc = check_persp("postprocess_paste_quads_persp", quads_host, persp_host, nullptr, B, S);
  if (rc != DMX_OK) return rc;
  PostPerspArgs p{image_vae, S, pages_device, P, quads_device, persp_device, B};
  hipLaunchKernelGGL(dmx_postprocess_quads_persp_kernel, dim3(pages_host[P - 1].block_lo + pages_host[P - 1].blocks), dim3(256), 0,
                     (hipStream_t)stream, p);
  return dmx_check_launch("dmx_postprocess_quads_persp_kernel");
}

extern "C" int dmx_rectify_quads_persp(const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P, const dmx_edit_quad* quads_host,
                                       const dmx_edit_quad* quads_device, const dmx_quad_persp* persp_host, const dmx_quad_persp* persp_device, int B,
                                       unsigned char* out, long long out_bytes, dmx_stream_t stream) {
  DMX_REQUIRE(pages_device && quads_device && persp_device && out, "rectify_quads_persp: null argument");
  int rc = check_quads("rectify_quads_persp", pages_host, P, quads_host, B, 0, false, true);
  if (rc == DMX_OK) rc = check_quad_pages("rectify_quads_persp", pages_host, P, false);
  if (rc == DMX_OK) rc = check_persp("rectify_quads_persp", quads_host, persp_host, nullptr, B, 0);
  if (rc != DMX_OK) return rc;
  const dmx_edit_quad& last = quads_host[B - 1];
  DMX_REQUIRE(out_bytes >= last.rect_off + (long long)last.rw * last.rh * 3, "rectify_quads_persp: the strips take %lld bytes, the output holds %lld",
              last.rect_off + (long long)last.rw * last.rh * 3, out_bytes);
  RectPerspArgs p{pages_device, P, quads_device, persp_device, B, out, out_bytes};
  hipLaunchKernelGGL(dmx_rectify_quads_persp_kernel, dim3(last.rect_block_lo + last.rect_blocks), dim3(256), 0, (hipStream_t)stream, p);
  return dmx_check_launch("dmx_rectify_quads_persp_kernel");
}
