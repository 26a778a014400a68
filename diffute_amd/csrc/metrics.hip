// Comparing two versions of a set of pages: per-box SSE / SSIM (dmx_box_metrics_pages) and what changed outside all boxes
// (dmx_page_outside_diff).  Ragged in both directions - pages of different sizes, any number of boxes per page - so the geometry travels
// in two device tables, dmx_metric_page and dmx_metric_box, as in prepost_batch.hip's page kernels, and blocks enumerate (box, tile) /
// (page, row, 256-pixel run) along grid.x and find their box / page by a binary search of the tables' first-block fields.
//
// SSIM.  A tile is TILE x TILE window centres counted from the box's own corner, so its block reads the (TILE + 10)^2 pixels of both pages
// into LDS once, runs the 11-tap Gaussian as a horizontal and a vertical pass over x, y, x^2, y^2, xy, and evaluates one window per thread.
// The moments are taken about an integer pivot, the rounded mean of `a` over the tile's pixels: variance and covariance do not depend on it, the means get
// it added back, and on a flat bright page G*(x^2) - (G*x)^2 no longer cancels at 65025 against a C2 of 58.5.  The pivoted pixels and their
// products are integers below 2^17, exact in fp32; everything per window is fp32 in one written-down order (no contraction: the Makefile
// passes -ffp-contract=off), the sums over a tile's windows and over a box's tiles are fp64 in a fixed order.  A box's results depend on
// nothing but its own pixels: bit-equal from run to run and wherever the box stands in the table.
// SSE and the outside-diff sums are integers: exact, order-free.
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace {
constexpr int TILE = DMX_METRIC_TILE, WIN = DMX_METRIC_WINDOW, REG = TILE + WIN - 1;      // a tile reads REG x REG pixels
static_assert(TILE * TILE == 256, "one thread per window centre of a tile");

struct Weights { float w[WIN]; };
struct TileRec { double ssim[3]; unsigned long long sse[3]; };      // what one (box, tile) block leaves in the workspace

struct BoxArgs {
  const dmx_metric_page* pages; int P;
  const dmx_metric_box* boxes; int B;
  TileRec* ws; int total_tiles;
  Weights g; float C1, C2;
};

// the last entry of a table of ascending first-block fields that starts at or before `key` (n >= 1; any table gives an index in [0, n))
template <class Rec, class Lo>
__device__ __forceinline__ int find_range(const Rec* table, int n, int key, Lo lo_of) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (lo_of(table[mid]) <= key) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// a box as the kernels use it: everything read from the device tables clamped to the tables and the page, the tile counts derived again
struct BoxView { const unsigned char* a; const unsigned char* b; int W, x1, y1, w, h, tiles_x, tiles_y; };
__device__ __forceinline__ bool box_view(const dmx_metric_page* pages, int P, const dmx_metric_box& bx, BoxView& v) {
  const dmx_metric_page pg = pages[min(max(bx.page, 0), P - 1)];
  if (pg.H <= 0 || pg.W <= 0) return false;
  v.a = (const unsigned char*)pg.a; v.b = (const unsigned char*)pg.b; v.W = pg.W;
  v.x1 = min(max(bx.x1, 0), pg.W - 1); v.y1 = min(max(bx.y1, 0), pg.H - 1);
  v.w = min(max(bx.x2, v.x1 + 1), pg.W) - v.x1; v.h = min(max(bx.y2, v.y1 + 1), pg.H) - v.y1;
  v.tiles_x = max(1, (v.w - (WIN - 1) + TILE - 1) / TILE); v.tiles_y = max(1, (v.h - (WIN - 1) + TILE - 1) / TILE);
  return true;
}

// lane 0 of each wave gets the wave's sum, in the same order whatever the values; block_sum then adds the four waves in wave order
template <class V> __device__ __forceinline__ V wave_sum(V v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  return v;
}
template <class V> __device__ __forceinline__ V block_sum(V v, V* s4) {      // 256 threads, all of them get the sum
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  return s4[0] + s4[1] + s4[2] + s4[3];
}

__global__ __launch_bounds__(256) void dmx_box_metrics_kernel(const BoxArgs p) {
  __shared__ float s_a[3][REG][REG + 1], s_b[3][REG][REG + 1];     // the tile's pixels, per channel
  __shared__ float s_h[5][REG][TILE];                              // the horizontal pass of x, y, xx, yy, xy
  __shared__ double s_d[4];
  __shared__ unsigned s_u[4];
  const int tid = threadIdx.x;
  const int bi = find_range(p.boxes, p.B, (int)blockIdx.x, [](const dmx_metric_box& b) { return b.tile_lo; });
  const dmx_metric_box bx = p.boxes[bi];
  BoxView v;
  if (!box_view(p.pages, p.P, bx, v)) return;
  const int local = (int)blockIdx.x - bx.tile_lo;
  if (local < 0 || local / v.tiles_x >= v.tiles_y) return;         // a stale table: with a good one every block lies inside its box
  const int tx = local % v.tiles_x, ty = local / v.tiles_x;
  const int rw = min(REG, v.w - tx * TILE), rh = min(REG, v.h - ty * TILE);                       // pixels the tile reads (>= 1 each)
  const int ow = min(TILE, v.w - (WIN - 1) - tx * TILE), oh = min(TILE, v.h - (WIN - 1) - ty * TILE);   // window centres (<= 0: none)
  const bool last_x = tx == v.tiles_x - 1, last_y = ty == v.tiles_y - 1;
  const size_t origin = ((size_t)(v.y1 + ty * TILE) * v.W + (v.x1 + tx * TILE)) * 3;
  // stage; every pixel of the box belongs to exactly one tile for the SSE: the tile whose first TILE rows / columns hold it, the rest of
  // the region to the last tile of the row / column
  unsigned sse[3] = {0u, 0u, 0u}, sum[3] = {0u, 0u, 0u};
  for (int i = tid; i < rh * rw; i += 256) {
    const int ly = i / rw, lx = i - ly * rw;
    const size_t o = origin + ((size_t)ly * v.W + lx) * 3;
    const bool own = (ly < TILE || last_y) && (lx < TILE || last_x);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int a = v.a[o + c], b = v.b[o + c], d = a - b;
      if (own) sse[c] += (unsigned)(d * d);
      sum[c] += (unsigned)a;
      s_a[c][ly][lx] = (float)a;
      s_b[c][ly][lx] = (float)b;
    }
  }
  // the pivot of the tile's moments: the rounded mean of `a` over the pixels the tile reads (block_sum's barriers also publish s_a / s_b)
  float piv[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) piv[c] = (float)((block_sum(sum[c], s_u) + (unsigned)(rh * rw) / 2u) / (unsigned)(rh * rw));
  double ssim[3] = {0.0, 0.0, 0.0};
  if (ow > 0 && oh > 0) {                                          // uniform per block
    const int oy = tid / TILE, ox = tid % TILE;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      for (int i = tid; i < rh * ow; i += 256) {
        const int ly = i / ow, lx = i - ly * ow;
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
          const float x = s_a[c][ly][lx + k] - piv[c], y = s_b[c][ly][lx + k] - piv[c], g = p.g.w[k];
          m[0] += g * x; m[1] += g * y; m[2] += g * (x * x); m[3] += g * (y * y); m[4] += g * (x * y);
        }
#pragma unroll
        for (int j = 0; j < 5; ++j) s_h[j][ly][lx] = m[j];
      }
      __syncthreads();
      if (oy < oh && ox < ow) {
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < WIN; ++k) {
          const float g = p.g.w[k];
#pragma unroll
          for (int j = 0; j < 5; ++j) m[j] += g * s_h[j][oy + k][ox];
        }
        const float vx = m[2] - m[0] * m[0], vy = m[3] - m[1] * m[1], vxy = m[4] - m[0] * m[1];
        const float ux = m[0] + piv[c], uy = m[1] + piv[c];
        const float a1 = 2.f * ux * uy + p.C1, a2 = 2.f * vxy + p.C2;
        const float b1 = ux * ux + uy * uy + p.C1, b2 = vx + vy + p.C2;
        ssim[c] = (double)((a1 * a2) / (b1 * b2));
      }
      __syncthreads();
    }
  }
  TileRec rec;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    rec.ssim[c] = block_sum(ssim[c], s_d);
    rec.sse[c] = block_sum(sse[c], s_u);                            // <= REG^2 * 255^2: fits 32 bits
  }
  if (tid == 0) p.ws[blockIdx.x] = rec;
}

// one block per box: thread t adds the tile records t, t + 256, ... of the box in that order, then the block in block_sum's order
__global__ __launch_bounds__(256) void dmx_box_metrics_combine_kernel(const BoxArgs p, unsigned long long* sse, float* ssim) {
  __shared__ double s_d[4];
  __shared__ unsigned long long s_u[4];
  const int b = blockIdx.x;
  const dmx_metric_box bx = p.boxes[b];
  BoxView v;
  long long n = 0;
  int lo = 0;
  if (box_view(p.pages, p.P, bx, v)) {
    lo = min(max(bx.tile_lo, 0), p.total_tiles);
    n = min((long long)v.tiles_x * v.tiles_y, (long long)(p.total_tiles - lo));
  } else {
    v.w = v.h = 0;
  }
  double s[3] = {0.0, 0.0, 0.0};
  unsigned long long e[3] = {0ull, 0ull, 0ull};
  for (long long i = threadIdx.x; i < n; i += 256) {
    const TileRec& r = p.ws[lo + i];
#pragma unroll
    for (int c = 0; c < 3; ++c) { s[c] += r.ssim[c]; e[c] += r.sse[c]; }
  }
  const bool windows = v.w >= WIN && v.h >= WIN;
  const double count = windows ? (double)(v.w - (WIN - 1)) * (double)(v.h - (WIN - 1)) : 1.0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double sc = block_sum(s[c], s_d);
    const unsigned long long ec = block_sum(e[c], s_u);
    if (threadIdx.x == 0) {
      sse[(size_t)b * 3 + c] = ec;
      ssim[(size_t)b * 3 + c] = windows ? (float)(sc / count) : __builtin_nanf("");
    }
  }
}

struct OutsideArgs {
  const dmx_metric_page* pages; int P;
  const dmx_metric_box* boxes; int B;
  unsigned long long* out;                                          // [P][2]: changed, sse; zero before the launch
};

// blocks enumerate (page, row, run of 256 pixels) as the paste kernels of prepost_batch.hip do; a pixel scans the boxes of its own page,
// staged 256 at a time in LDS
__global__ __launch_bounds__(256) void dmx_page_outside_diff_kernel(const OutsideArgs p) {
  __shared__ int4 s_box[256];
  __shared__ unsigned s_u[4];
  const int tid = threadIdx.x;
  const int q = find_range(p.pages, p.P, (int)blockIdx.x, [](const dmx_metric_page& g) { return g.block_lo; });
  const dmx_metric_page pg = p.pages[q];
  if (pg.H <= 0 || pg.W <= 0 || pg.W > DMX_EDIT_PAGE_MAX_W) return;
  const int runs = (pg.W + 255) / 256, local = (int)blockIdx.x - pg.block_lo;
  if (local < 0 || local / runs >= pg.H) return;                    // a stale table
  const int y = local / runs, x = (local % runs) * 256 + tid;
  const int lo = min(max(pg.box_lo, 0), p.B), hi = min(max(pg.box_hi, lo), p.B);
  bool covered = false;
  for (int base = lo; base < hi; base += 256) {
    __syncthreads();
    if (base + tid < hi) {
      const dmx_metric_box& bx = p.boxes[base + tid];
      s_box[tid] = make_int4(bx.x1, bx.y1, bx.x2, bx.y2);
    }
    __syncthreads();
    const int n = min(256, hi - base);
    for (int j = 0; j < n; ++j) {
      const int4 r = s_box[j];
      covered |= x >= r.x && x < r.z && y >= r.y && y < r.w;
    }
  }
  unsigned changed = 0u, sse = 0u;
  if (x < pg.W && !covered) {
    const size_t o = ((size_t)y * pg.W + x) * 3;
    const unsigned char* a = (const unsigned char*)pg.a;
    const unsigned char* b = (const unsigned char*)pg.b;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int d = (int)a[o + c] - (int)b[o + c];
      sse += (unsigned)(d * d);
    }
    changed = sse != 0u;
  }
  const unsigned cs = block_sum(changed, s_u), es = block_sum(sse, s_u);     // <= 256 * 3 * 255^2: fits 32 bits
  if (tid == 0) {
    if (cs) atomicAdd(p.out + (size_t)q * 2, (unsigned long long)cs);
    if (es) atomicAdd(p.out + (size_t)q * 2 + 1, (unsigned long long)es);
  }
}

long long tiles_along(int n) { return n - (WIN - 1) > 0 ? (n - (WIN - 1) + TILE - 1) / TILE : 1; }

// both tables; `prepared` also compares the derived fields with what dmx_metric_tables_prepare fills.  *total_tiles (optional): the
// blocks of the box-metrics grid
int check_tables(const char* what, const dmx_metric_page* pages, int P, const dmx_metric_box* boxes, int B, bool prepared, long long* total_tiles) {
  DMX_REQUIRE(pages, "%s: null page table", what);
  DMX_REQUIRE(P >= 1, "%s: %d pages, expected at least 1", what, P);
  DMX_REQUIRE(B >= 0 && (B == 0 || boxes), "%s: %d boxes and %s box table", what, B, boxes ? "a" : "no");
  long long blocks = 0, tiles = 0;
  for (int q = 0, next = 0; q < P; ++q) {
    const dmx_metric_page& pg = pages[q];
    DMX_REQUIRE(pg.H > 0 && pg.W > 0 && pg.W <= DMX_EDIT_PAGE_MAX_W, "%s: page %d: bad size %dx%d (1 <= H, 1 <= W <= %d)", what, q, pg.W, pg.H,
                DMX_EDIT_PAGE_MAX_W);
    DMX_REQUIRE(pg.a && pg.b, "%s: page %d: null image", what, q);
    DMX_REQUIRE(pg.box_lo == next && pg.box_hi >= pg.box_lo && pg.box_hi <= B,
                "%s: page %d: its boxes [%d, %d) must start at %d and end at or before %d (the ranges tile [0, B) in page order)", what, q, pg.box_lo,
                pg.box_hi, next, B);
    DMX_REQUIRE(q + 1 < P || pg.box_hi == B, "%s: page %d: the last page's boxes end at %d, the table holds %d", what, q, pg.box_hi, B);
    next = pg.box_hi;
    const long long mine = (long long)pg.H * cdiv(pg.W, 256);
    DMX_REQUIRE(blocks + mine < (1ll << 31), "%s: page %d: the pages need more than 2^31 - 1 blocks of 256 pixels", what, q);
    if (prepared)
      DMX_REQUIRE(pg.block_lo == (int)blocks && pg.blocks == (int)mine,
                  "%s: page %d: derived fields do not belong to this page table (dmx_metric_tables_prepare fills them)", what, q);
    blocks += mine;
    for (int b = pg.box_lo; b < pg.box_hi; ++b) {
      const dmx_metric_box& bx = boxes[b];
      DMX_REQUIRE(bx.page == q, "%s: box %d: page index %d, the box lies in the range of page %d", what, b, bx.page, q);
      DMX_REQUIRE(bx.x2 > bx.x1 && bx.y2 > bx.y1, "%s: box %d: (%d, %d, %d, %d) is empty", what, b, bx.x1, bx.y1, bx.x2, bx.y2);
      DMX_REQUIRE(bx.x1 >= 0 && bx.y1 >= 0 && bx.x2 <= pg.W && bx.y2 <= pg.H, "%s: box %d: (%d, %d, %d, %d) lies outside the %dx%d page %d", what, b,
                  bx.x1, bx.y1, bx.x2, bx.y2, pg.W, pg.H, q);
      const long long nx = tiles_along(bx.x2 - bx.x1), ny = tiles_along(bx.y2 - bx.y1);
      DMX_REQUIRE(tiles + nx * ny < (1ll << 31), "%s: box %d: the boxes need more than 2^31 - 1 tiles", what, b);
      if (prepared)
        DMX_REQUIRE(bx.tiles_x == (int)nx && bx.tiles_y == (int)ny && bx.tile_lo == (int)tiles,
                    "%s: box %d: derived fields do not belong to this box table (dmx_metric_tables_prepare fills them)", what, b);
      tiles += nx * ny;
    }
  }
  if (total_tiles) *total_tiles = tiles;
  return DMX_OK;
}

void ssim_weights(float* w) {
  double g[WIN], s = 0.0;
  for (int i = 0; i < WIN; ++i) {
    const double x = (double)(i - WIN / 2);
    g[i] = exp(-(x * x) / 4.5);                                     // sigma 1.5
    s += g[i];
  }
  for (int i = 0; i < WIN; ++i) w[i] = (float)(g[i] / s);
}

}  // namespace

extern "C" int dmx_metric_tables_prepare(dmx_metric_page* pages, int P, dmx_metric_box* boxes, int B) {
  const int rc = check_tables("metric_tables_prepare", pages, P, boxes, B, false, nullptr);
  if (rc != DMX_OK) return rc;
  int blocks = 0, tiles = 0;
  for (int q = 0; q < P; ++q) {
    dmx_metric_page& pg = pages[q];
    pg.block_lo = blocks; pg.blocks = pg.H * cdiv(pg.W, 256);
    blocks += pg.blocks;
    for (int b = pg.box_lo; b < pg.box_hi; ++b) {
      dmx_metric_box& bx = boxes[b];
      bx.tiles_x = (int)tiles_along(bx.x2 - bx.x1); bx.tiles_y = (int)tiles_along(bx.y2 - bx.y1);
      bx.tile_lo = tiles;
      tiles += bx.tiles_x * bx.tiles_y;
    }
  }
  return DMX_OK;
}

extern "C" int dmx_box_metrics_weights(float* h_weights) {
  DMX_REQUIRE(h_weights, "box_metrics_weights: null argument");
  ssim_weights(h_weights);
  return DMX_OK;
}

extern "C" size_t dmx_box_metrics_workspace_bytes(const dmx_metric_box* boxes_host, int B) {
  if (!boxes_host || B < 1) return 0;
  const dmx_metric_box& z = boxes_host[B - 1];
  if (z.tile_lo < 0 || z.tiles_x < 1 || z.tiles_y < 1) return 0;
  return (size_t)((long long)z.tile_lo + (long long)z.tiles_x * z.tiles_y) * sizeof(TileRec);
}

extern "C" int dmx_box_metrics_pages(const dmx_metric_page* pages_host, const dmx_metric_page* pages_device, int P, const dmx_metric_box* boxes_host,
                                     const dmx_metric_box* boxes_device, int B, unsigned long long* sse, float* ssim, void* workspace,
                                     size_t workspace_bytes, dmx_stream_t stream) {
  DMX_REQUIRE(pages_device && boxes_device && sse && ssim, "box_metrics_pages: null argument");
  DMX_REQUIRE(B >= 1, "box_metrics_pages: %d boxes, expected at least 1", B);
  long long tiles = 0;
  const int rc = check_tables("box_metrics_pages", pages_host, P, boxes_host, B, true, &tiles);
  if (rc != DMX_OK) return rc;
  const size_t need = (size_t)tiles * sizeof(TileRec);
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 7)) {
    dmx_set_error("box_metrics_pages: the workspace holds %zu bytes, %zu are needed (8-byte aligned; dmx_box_metrics_workspace_bytes)", workspace_bytes,
                  need);
    return DMX_ERR_WORKSPACE;
  }
  BoxArgs p{pages_device, P, boxes_device, B, (TileRec*)workspace, (int)tiles, {}, 0.f, 0.f};
  ssim_weights(p.g.w);
  p.C1 = (float)((0.01 * 255.0) * (0.01 * 255.0)); p.C2 = (float)((0.03 * 255.0) * (0.03 * 255.0));
  hipLaunchKernelGGL(dmx_box_metrics_kernel, dim3((unsigned)tiles), dim3(256), 0, (hipStream_t)stream, p);
  int lc = dmx_check_launch("dmx_box_metrics_kernel");
  if (lc != DMX_OK) return lc;
  hipLaunchKernelGGL(dmx_box_metrics_combine_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, p, sse, ssim);
  return dmx_check_launch("dmx_box_metrics_combine_kernel");
}

extern "C" int dmx_page_outside_diff(const dmx_metric_page* pages_host, const dmx_metric_page* pages_device, int P, const dmx_metric_box* boxes_host,
                                     const dmx_metric_box* boxes_device, int B, unsigned long long* out, dmx_stream_t stream) {
  DMX_REQUIRE(pages_device && out && (B == 0 || boxes_device), "page_outside_diff: null argument");
  const int rc = check_tables("page_outside_diff", pages_host, P, boxes_host, B, true, nullptr);
  if (rc != DMX_OK) return rc;
  DMX_HIP(hipMemsetAsync(out, 0, (size_t)P * 2 * sizeof(unsigned long long), (hipStream_t)stream));
  OutsideArgs p{pages_device, P, boxes_device, B, out};
  hipLaunchKernelGGL(dmx_page_outside_diff_kernel, dim3(pages_host[P - 1].block_lo + pages_host[P - 1].blocks), dim3(256), 0, (hipStream_t)stream, p);
  return dmx_check_launch("dmx_page_outside_diff_kernel");
}
