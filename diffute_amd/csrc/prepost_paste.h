// What the paste kernels of prepost_batch.hip (the plain paste) and prepost_blend.hip (the feathered, colour-matched paste) share: the
// arguments of a one-page paste and of a paged one, the block -> (page, row, column tile) map of the paged grid, and the choice rule of
// the verified edits.  Device code only; everything here is called on a block of 256 threads.
#pragma once
#include "common.h"
#include "kernels.h"
#include "prepost_resize.h"

namespace dmx_paste {

struct PostBatchArgs {
  const float* vae; int S;                     // decoder outputs [B][3][S][S] in [-1, 1]
  const unsigned char* ori; unsigned char* out; unsigned char* umask; int H, W;
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
struct PostPagesArgs {
  const float* vae; int S;
  const dmx_edit_page* pages; int P;
  const dmx_edit_item* items; int B;
};
struct PageTile { PostBatchArgs view; int lo, x, y; };

// false: the block has no pixel to write (a stale table - with a good one every block lies inside its page).  Uniform per block.
__device__ __forceinline__ bool page_tile(const PostPagesArgs& p, PageTile& t) {
  int pi = 0;
  for (int i = 1; i < p.P; ++i) pi = (int)blockIdx.x >= p.pages[i].block_lo ? i : pi;
  const dmx_edit_page pg = p.pages[pi];
  if (pg.H <= 0 || pg.W <= 0 || pg.W > DMX_EDIT_PAGE_MAX_W) return false;
  const int tiles = (pg.W + 255) / 256, local = (int)blockIdx.x - pg.block_lo;
  if (local < 0 || local / tiles >= pg.H) return false;
  t.lo = min(max(pg.item_lo, 0), p.B - 1);
  const int n = min(max(pg.item_hi - t.lo, 1), p.B - t.lo);
  t.view = PostBatchArgs{p.vae, p.S, (const unsigned char*)pg.original, (unsigned char*)pg.out, (unsigned char*)pg.union_mask, pg.H, pg.W,
                         p.items + t.lo, n};
  t.y = local / tiles;
  t.x = (local % tiles) * 256 + (int)threadIdx.x;
  return true;
}

}  // namespace dmx_paste
