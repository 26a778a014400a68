// Several text boxes of ONE image per launch: the batched ends of the editing path (pipeline.edit_boxes).  prepost.hip turns one box
// into the [1,3,S,S] network inputs and pastes one decoder output back, with the geometry as kernel arguments and a full-size [H][W]
// mask rasterised by a launch of its own; here B boxes share the uint8 image in HBM, item b's geometry comes from a device table of
// dmx_edit_item, and the mask is the predicate "inside item b's inclusive box" (PIL's rectangle rule, what dmx_mask_rasterize_kernel
// writes), so there is neither a mask buffer nor a rasterise launch.  The per-pixel arithmetic is prepost_resize.h, the same
// functions the single-box kernels call: row b is bit for bit what the single-box entry gives for item b.
// Pure HBM-bound byte work: one thread per destination pixel, coalesced plain vector stores.
#include "common.h"
#include "kernels.h"
#include "prepost_resize.h"
#include "../../include/diffute_hip.h"

namespace {
using namespace dmx_resize;

struct PreBatchArgs {
  const unsigned char* img; int H, W;                                  // HWC uint8 image shared by all items
  const dmx_edit_item* items; int S;
  float* out_img; float* out_masked; unsigned char* out_mask; float* out_mask_lat;   // [B][3][S][S], [B][3][S][S], [B][S][S], [B][S/8][S/8]
};

__global__ __launch_bounds__(256) void dmx_preprocess_batch_kernel(const PreBatchArgs p) {
  const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y, b = blockIdx.z;
  if (dx >= p.S) return;
  const dmx_edit_item it = p.items[b];
  const Geom g = item_geom(it, p.H, p.W, p.S, true);
  int vi[3], vm[3], vk;
  // generate_mask (app.ipynb:370-378) as a predicate on image coordinates: item b's box alone, both corners included
  auto mk = [&](int y, int x) -> int {
    const int X = g.xs + x, Y = g.ys + y;
    return (X >= it.x1 && X <= it.x2 && Y >= it.y1 && Y <= it.y2) ? 1 : 0;
  };
  pre_pixel(p.img, p.W, g, mk, dx, dy, vi, vm, vk);
  const size_t plane = (size_t)p.S * p.S, lat = (size_t)(p.S >> 3) * (p.S >> 3);
  pre_store(vi, vm, vk, p.S, dx, dy, p.out_img + (size_t)b * 3 * plane, p.out_masked + (size_t)b * 3 * plane, p.out_mask + (size_t)b * plane,
            p.out_mask_lat ? p.out_mask_lat + (size_t)b * lat : nullptr);
}

struct PostBatchArgs {
  const float* vae; int S;                     // decoder outputs [B][3][S][S] in [-1, 1]
  const unsigned char* ori; unsigned char* out; unsigned char* umask; int H, W;
  const dmx_edit_item* items; int B;
};

// B chained single pastes in index order leave, at every pixel, the value of the LAST item whose (half-open box) AND (resized crop
// extent) covers it, computed from that item's decoder output alone, or the original where no item does: scan from the last item down
// and stop at the first hit.  The integer half of the table is staged in LDS once per block (every pixel of the row scans all of it).
__device__ __forceinline__ void stage_items(const PostBatchArgs& p, int4* s_box, int4* s_crop) {
  if ((int)threadIdx.x < p.B) {
    const dmx_edit_item& it = p.items[threadIdx.x];
    s_box[threadIdx.x] = make_int4(it.x1, it.y1, it.x2, it.y2);
    const int xs = min(max(it.x_s, 0), p.W - 1), ys = min(max(it.y_s, 0), p.H - 1);       // item_geom's clamps
    s_crop[threadIdx.x] = make_int4(xs, ys, min(max(it.cw, 1), p.W - xs), min(max(it.ch, 1), p.H - ys));
  }
}
// One pixel of the page.  row(b) -> which [3][S][S] image of p.vae item b pastes, < 0 = the item is skipped (it still counts for the
// union mask: the mask says where the boxes are, not what was pasted).
template <class Row>
__device__ __forceinline__ void paste_pixel(const PostBatchArgs& p, const int4* s_box, const int4* s_crop, Row row, int x, int y) {
  int hit = -1, any = 0;
  for (int b = p.B - 1; b >= 0; --b) {
    const int4 bx = s_box[b];
    any |= (x >= bx.x && x <= bx.z && y >= bx.y && y <= bx.w) ? 1 : 0;                    // union mask: PIL's inclusive rectangle
    if (hit < 0 && row(b) >= 0 && x >= bx.x && x < bx.z && y >= bx.y && y < bx.w) {        // the paste: inf_res[y1:y2, x1:x2]
      const int4 cr = s_crop[b];
      const int dx = x - cr.x, dy = y - cr.y;
      if (dx >= 0 && dx < cr.z && dy >= 0 && dy < cr.w) hit = b;
    }
    if (hit >= 0) break;                                                     // (a hit lies inside that item's inclusive box: `any` is set)
  }
  const size_t o = ((size_t)y * p.W + x) * 3;
  if (p.umask) p.umask[(size_t)y * p.W + x] = (unsigned char)any;
  if (hit < 0) { p.out[o] = p.ori[o]; p.out[o + 1] = p.ori[o + 1]; p.out[o + 2] = p.ori[o + 2]; return; }
  const Geom g = item_geom(p.items[hit], p.H, p.W, p.S, false);
  const float* vae = p.vae + (size_t)row(hit) * 3 * p.S * p.S;
#pragma unroll
  for (int c = 0; c < 3; ++c) p.out[o + c] = post_pixel(vae, p.S, g, c, x - g.xs, y - g.ys);
}

__global__ __launch_bounds__(256) void dmx_postprocess_batch_kernel(const PostBatchArgs p) {
  __shared__ int4 s_box[DMX_EDIT_MAX_ITEMS], s_crop[DMX_EDIT_MAX_ITEMS];
  stage_items(p, s_box, s_crop);
  __syncthreads();
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= p.W) return;
  paste_pixel(p, s_box, s_crop, [](int b) -> int { return b; }, x, y);
}

// Best of K candidates per item, chosen and pasted in ONE launch: p.vae is [B][K][3][S][S], scores [B][K] lives on the device, so the
// host never waits for it.  Every block stages the score table in LDS and derives the same choices from it:
//   choice[b] = arg-max over k of scores[b][k], the lowest k on a tie; a NaN never wins; 0 when every score is NaN;
//   -1 (the item is skipped, its box keeps the original pixels) when the best score is below `threshold`.
// Block (0, 0) alone writes `choice`, with plain vector stores.  The paste is paste_pixel, the rule of the kernel above.
__global__ __launch_bounds__(256) void dmx_postprocess_select_kernel(const PostBatchArgs p, const float* scores, int K, float threshold, int* choice) {
  __shared__ int4 s_box[DMX_EDIT_MAX_ITEMS], s_crop[DMX_EDIT_MAX_ITEMS];
  __shared__ float s_score[DMX_EDIT_MAX_ITEMS * DMX_SELECT_MAX_CANDIDATES];
  __shared__ int s_choice[DMX_EDIT_MAX_ITEMS];
  stage_items(p, s_box, s_crop);
  for (int i = threadIdx.x; i < p.B * K; i += blockDim.x) s_score[i] = scores[i];
  __syncthreads();
  if ((int)threadIdx.x < p.B) {
    const float* sc = s_score + threadIdx.x * K;
    int best = -1;
    float bv = 0.f;
    for (int k = 0; k < K; ++k) {
      const float v = sc[k];
      if (v != v) continue;                                                                // NaN
      if (best < 0 || v > bv) { best = k; bv = v; }
    }
    const int ch = best < 0 ? 0 : (bv < threshold ? -1 : best);
    s_choice[threadIdx.x] = ch;
    if (blockIdx.x == 0 && blockIdx.y == 0) choice[threadIdx.x] = ch;
  }
  __syncthreads();
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= p.W) return;
  paste_pixel(p, s_box, s_crop, [&](int b) -> int { const int k = s_choice[b]; return k < 0 ? -1 : b * K + k; }, x, y);
}

}  // namespace

// the checks of the single-box entries, per item; `prepared` also compares the derived fields with what edit_items_prepare fills
int dmx_check_edit_items(const char* what, const dmx_edit_item* items, int B, int H, int W, int S, bool prepared) {
  DMX_REQUIRE(items, "%s: null item table", what);
  DMX_REQUIRE(B >= 1 && B <= DMX_EDIT_MAX_ITEMS, "%s: %d items, expected 1 .. %d", what, B, DMX_EDIT_MAX_ITEMS);
  DMX_REQUIRE(H > 0 && W > 0 && H <= 65535 && S > 0 && S <= 65535, "%s: bad sizes (image %dx%d, S %d)", what, W, H, S);
  for (int b = 0; b < B; ++b) {
    const dmx_edit_item& it = items[b];
    DMX_REQUIRE(it.crop_scale > 0, "%s: item %d: crop_scale %d", what, b, it.crop_scale);
    DMX_REQUIRE(it.x_s >= 0 && it.y_s >= 0 && it.x_s < W && it.y_s < H, "%s: item %d: crop origin (%d, %d) outside the %dx%d image", what, b,
                it.x_s, it.y_s, W, H);
    if (!prepared) continue;
    const Geom a = pre_geom(H, W, it.x_s, it.y_s, it.crop_scale, S), z = post_geom(H, W, it.x_s, it.y_s, it.crop_scale, S);
    DMX_REQUIRE(it.cw == a.cw && it.ch == a.ch && it.pre_area2 == a.area2 && it.post_area2 == z.area2 && it.pre_sx == a.sx && it.pre_sy == a.sy &&
                    it.post_sx == z.sx && it.post_sy == z.sy,
                "%s: item %d: derived fields do not belong to a %dx%d image at S = %d (dmx_edit_items_prepare fills them)", what, b, W, H, S);
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
  PreBatchArgs p{image_hwc, H, W, items_device, S, out_image, out_masked_image, out_mask, out_mask_latent};
  hipLaunchKernelGGL(dmx_preprocess_batch_kernel, dim3(cdiv(S, 256), S, B), dim3(256), 0, (hipStream_t)stream, p);
  return dmx_check_launch("dmx_preprocess_batch_kernel");
}

extern "C" int dmx_postprocess_paste_batch(const float* image_vae, int S, const unsigned char* original_hwc, unsigned char* out_hwc,
                                           unsigned char* union_mask, int H, int W, const dmx_edit_item* items_host,
                                           const dmx_edit_item* items_device, int B, dmx_stream_t stream) {
  DMX_REQUIRE(image_vae && original_hwc && out_hwc && items_device, "postprocess_paste_batch: null argument");
  const int rc = dmx_check_edit_items("postprocess_paste_batch", items_host, B, H, W, S, true);
  if (rc != DMX_OK) return rc;
  PostBatchArgs p{image_vae, S, original_hwc, out_hwc, union_mask, H, W, items_device, B};
  hipLaunchKernelGGL(dmx_postprocess_batch_kernel, dim3(cdiv(W, 256), H), dim3(256), 0, (hipStream_t)stream, p);
  return dmx_check_launch("dmx_postprocess_batch_kernel");
}

extern "C" int dmx_postprocess_paste_select(const float* image_vae, int S, const float* scores, float threshold, const unsigned char* original_hwc,
                                            unsigned char* out_hwc, unsigned char* union_mask, int* choice, int H, int W,
                                            const dmx_edit_item* items_host, const dmx_edit_item* items_device, int B, int K, dmx_stream_t stream) {
  DMX_REQUIRE(image_vae && scores && original_hwc && out_hwc && choice && items_device, "postprocess_paste_select: null argument");
  DMX_REQUIRE(K >= 1 && K <= DMX_SELECT_MAX_CANDIDATES, "postprocess_paste_select: %d candidates per box, expected 1 .. %d", K, DMX_SELECT_MAX_CANDIDATES);
  DMX_REQUIRE(!(threshold != threshold), "postprocess_paste_select: the threshold is NaN (pass -inf for none)");
  const int rc = dmx_check_edit_items("postprocess_paste_select", items_host, B, H, W, S, true);
  if (rc != DMX_OK) return rc;
  PostBatchArgs p{image_vae, S, original_hwc, out_hwc, union_mask, H, W, items_device, B};
  hipLaunchKernelGGL(dmx_postprocess_select_kernel, dim3(cdiv(W, 256), H), dim3(256), 0, (hipStream_t)stream, p, scores, K, threshold, choice);
  return dmx_check_launch("dmx_postprocess_select_kernel");
}
