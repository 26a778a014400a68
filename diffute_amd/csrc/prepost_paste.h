// What the box kernels of prepost_batch.hip (crop, paste, select-paste), prepost_blend.hip (colour statistics, feathered paste) and
// readback.hip share: the page SOURCE each of them is written over - one page given by kernel arguments, or a device table of pages -,
// the block -> (page, row, column tile) map of the paged grid - which the quad pastes of prepost_quad.hip use too -, and the choice rule
// of the verified edits.  Device code only; the pastes are called on a block of 256 threads.
#pragma once
#include "common.h"
#include "kernels.h"
#include "prepost_resize.h"

namespace dmx_paste {

struct PasteArgs {
  const float* vae; int S;                     // decoder outputs [B][3][S][S] in [-1, 1]
  const dmx_edit_item* items; int B;
};

// choice[b] for all B items from the score table [B][K]: staged in LDS, one thread per item; `writer` blocks also store it to HBM.
// Ends with a barrier: s_choice is complete on return.
__device__ __forceinline__ void select_choices(const float* scores, int B, int K, float threshold, float* s_score, int* s_choice, int* choice,
                                               bool writer) {
  for (int i = threadIdx.x; i < B * K; i += blockDim.x) s_score[i] = scores[i];
  __syncthreads();
  if ((int)threadIdx.x < B) {
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
    if (writer) choice[threadIdx.x] = ch;
  }
  __syncthreads();
}

// The paste over P pages in ONE launch.  The rows of all pages do not fit in grid.y, so blocks enumerate (page, row, column tile) along
// grid.x: page p owns the blocks [block_lo, block_lo + H * ceil(W / 256)).  A block finds its page by a uniform scan of the (at most
// 64) block_lo values, then pastes one 256-pixel tile of one row with the page's view: a pixel scans only its own page's items.
// The quad pastes (prepost_quad.hip) enumerate their blocks the same way: page_block is the map, whatever the items are.
struct PageBlock { dmx_edit_page pg; int lo, n, x, y; };         // the page, its items [lo, lo + n) of the table, this thread's pixel

// false: the block has no pixel to write (a stale table - with a good one every block lies inside its page, no wider than max_w, and
// its items inside the table of B).  Uniform per block.
__device__ __forceinline__ bool page_block(const dmx_edit_page* pages, int P, int B, int max_w, PageBlock& t) {
  int pi = 0;
  for (int i = 1; i < P; ++i) pi = (int)blockIdx.x >= pages[i].block_lo ? i : pi;
  t.pg = pages[pi];
  if (t.pg.H <= 0 || t.pg.W <= 0 || t.pg.W > max_w) return false;
  const int tiles = (t.pg.W + 255) / 256, local = (int)blockIdx.x - t.pg.block_lo;
  if (local < 0 || local / tiles >= t.pg.H) return false;
  t.lo = min(max(t.pg.item_lo, 0), B - 1);
  t.n = min(max(t.pg.item_hi - t.lo, 1), B - t.lo);
  t.y = local / tiles;
  t.x = (local % tiles) * 256 + (int)threadIdx.x;
  return true;
}

// A page source travels to the kernels by value, beside their arguments, and answers, uniformly per block:
//   tile     (the paste-shaped grids) this thread's pixel, the page and the page's slice of the item table, as a PageBlock; false: the
//            block has no pixel to write;
//   of       (the item-shaped grids: crop, statistics, read-back) the page of an item - `original`, H and W of it are read;
//   chooser  (the select-paste) whether this block stores `choice`.
// A page is a dmx_edit_page to every kernel body; OnePage's holds its arguments and no item range or block numbers.
struct OnePage {                               // the dmx_*_batch and unsuffixed entries: grid (ceil(W / 256), H), every block has pixels
  const unsigned char* ori; unsigned char* out; unsigned char* umask; int H, W;
  __device__ __forceinline__ dmx_edit_page page() const {
    return dmx_edit_page{(unsigned long long)ori, (unsigned long long)out, (unsigned long long)umask, H, W, 0, 0, 0, 0};
  }
  __device__ __forceinline__ bool tile(int B, PageBlock& t) const {
    t.pg = page(); t.lo = 0; t.n = B;
    t.x = blockIdx.x * 256 + threadIdx.x; t.y = blockIdx.y;
    return true;
  }
  __device__ __forceinline__ dmx_edit_page of(const dmx_edit_item&) const { return page(); }
  __device__ __forceinline__ bool chooser() const { return blockIdx.x == 0 && blockIdx.y == 0; }
};

struct PageTable {                             // the dmx_*_pages entries: the 1-D grid of page_block, clamps included
  const dmx_edit_page* pages; int P;
  __device__ __forceinline__ bool tile(int B, PageBlock& t) const { return page_block(pages, P, B, DMX_EDIT_PAGE_MAX_W, t); }
  __device__ __forceinline__ dmx_edit_page of(const dmx_edit_item& it) const { return pages[dmx_resize::page_of(it, P)]; }
  __device__ __forceinline__ bool chooser() const { return blockIdx.x == 0; }
};

// the 1-D grid of a checked, prepared host page table
inline dim3 paged_grid(const dmx_edit_page* pages_host, int P) { return dim3(pages_host[P - 1].block_lo + pages_host[P - 1].blocks); }

// What the blended pastes share (prepost_blend.hip for boxes, prepost_quad_blend.hip for quads).
// the decoder row of item b (its index in the whole table): b itself, or with a choice table row b * K + choice[b]; < 0 = skipped
__device__ __forceinline__ int row_of(const int* choice, int K, int b) {
  if (!choice) return b;
  const int k = choice[b];
  return k < 0 ? -1 : b * K + min(k, K - 1);
}

__device__ __forceinline__ long long floor_div(long long a, long long b) {           // b > 0
  const long long q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// dmx_paste_blend as the kernels take it: F = feather + 1
struct Blend { int F, grow, ring, max_shift, match; };

// the colour shift of one channel from an item's statistics (n > 0): floor((2 D + n) / (2 n)); |D| <= 255 n, the clamp is for stale tables
__device__ __forceinline__ int color_shift(long long D, long long n) { return (int)min(max(floor_div(2 * D + n, 2 * n), -255ll), 255ll); }

}  // namespace dmx_paste

// the blend parameters and the choice table, as every blended entry checks them (prepost_blend.hip); cap: DMX_PASTE_BLEND_MAX for boxes,
// DMX_QUAD_BLEND_MAX for quads
int dmx_check_paste_blend(const char* what, const dmx_paste_blend* blend, int cap, const int* choice, int K, dmx_paste::Blend& bl);
