// CURVED text regions, stated once: polygons of 2n points straightened by piecewise-affine maps.  The host half is what
// dmx_edit_curved_prepare fills into a dmx_edit_curved and its dmx_curved_piece entries, the device half how the three kernels of
// prepost_curved.hip choose a piece.  tests/curved_restatement.py restates this comment in Python ints and numpy int64 and the GPU tests
// compare bit for bit.  Only THE REGION AND WHICH MAP A PIXEL TAKES are new: a map is a dmx_persp_map derived by dmx_persp::relative from an
// exact integer matrix and evaluated by dmx_persp::coords (prepost_persp.h); taps, the single rounding, the quad predicate, blacking out
// before resampling and the paste rule are dmx_quad::tap16, pre_pixel, page_sample, sample4, post_pixel, post_src and inside of
// prepost_quad.h, called, not restated.
//
// Region.  2n points p[0 .. 2n - 1], 2 <= n <= 17, integer page coordinates: the top points left to right as read, then the bottom points
//   right to left; clockwise with y down.  Pair k: T_k = p[k], B_k = p[2n - 1 - k].  Cell k = 0 .. M - 1, M = n - 1: the quad
//   T_k, T_k+1, B_k+1, B_k, accepted as prepost_quad.h accepts a quad (every turn >= 0, twice the area > 0, corners on the page).  A pixel
//   is inside the region iff dmx_quad::inside holds for some cell (edges included).
//
// Strip, on the host, in double and in exactly this order of operations (integer products and sums are exact in a double):
//     u_k = (T_k+1 - T_k) + (B_k+1 - B_k),   w_k = max(1, rn(sqrt(u_k . u_k) / 2.0)),   c_0 = 0,  c_k+1 = c_k + w_k,   rw = c_M + 1
//     rh = rn((sqrt(d_0 . d_0) + sqrt(d_1 . d_1) + ... + sqrt(d_M . d_M)) / (double)(M + 1)) + 1,  d_k = B_k - T_k, summed from k = 0 upwards
//   rn = round-half-even (rint).  rh < 2 is refused, and rw or rh beyond 2^20.  In the strip's pixel-index space T_k <-> (c_k, 0),
//   B_k <-> (c_k, rh - 1).  For n = 2 on a parallelogram (rw, rh) is the quad's strip size.
//
// Pieces.  Cell k is cut by the diagonal T_k+1 - B_k: piece 2k = (T_k, T_k+1, B_k), piece 2k + 1 = (T_k+1, B_k+1, B_k).  A piece is the affine
//   map strip -> page that takes its strip triangle to its page triangle; with w = w_k, h = rh - 1, multiplied through by w h:
//     piece 2k      rows ((T_k+1 - T_k) h,  (B_k - T_k) w,      T_k w h - (T_k+1 - T_k) h c_k),                          (0, 0, w h)
//     piece 2k + 1  rows ((B_k+1 - B_k) h,  (B_k+1 - T_k+1) w,  B_k+1 w h - (B_k+1 - B_k) h (c_k + w) - (B_k+1 - T_k+1) w h),  (0, 0, w h)
//   (x and y alike): exact integers, the G of prepost_persp.h.  Two pieces that share an edge or a diagonal agree on that whole line,
//   extended: the map is continuous over the whole strip plane, which is where the window's context outside the strip comes from.  (One
//   homography per cell would agree with its neighbour at the two ends of the shared edge only, and the paste would tear.)
//
// Which piece.  A strip position (i, j) = (I / den, J / den), exact integers I, J, den > 0: the crop pixel (dx, dy) of frame
//   (ci2, cj2, crop_scale) has I = S ci2 + crop_scale (2dx + 1 - S), J = S cj2 + crop_scale (2dy + 1 - S), den = 2S; strip pixel (i, j) has
//   I = i, J = j, den = 1.  Its cell is the column band: k = the number of m in 1 .. M - 1 with I >= den c_m - so left of c_0 it is
//   cell 0, at and right of c_M-1 cell M - 1, and a shared column goes to the right-hand cell.  Its piece is 2k iff
//     (I - den c_k) (rh - 1) + J w_k <= den w_k (rh - 1)                                       (64-bit integers; below 2^59)
//   and 2k + 1 otherwise; the diagonal itself goes to 2k.  Rows above and below the strip take the same test.
//
// Three maps per piece, as prepost_persp.h states them for a quad, with the piece's matrix for G and the ITEM's rw, rh and frame: crop
//   = G * [[crop_scale, 0, S ci2], [0, crop_scale, S cj2], [0, 0, 2S]] on the grid (2dx + 1 - S, 2dy + 1 - S); strip =
//   G * [[1, 0, rw - 1], [0, 1, rh - 1], [0, 0, 2]] on the grid (2i + 1 - rw, 2j + 1 - rh); paste = page -> crop about the piece's own
//   (cx2, cy2) = (rdiv(c16[0], 2^15), rdiv(c16[1], 2^15)) of its crop map.  An affine map has t6 = t7 = 0 and D = 2^43 everywhere, so the
//   budget of prepost_persp.h is checked unchanged (check_window: over the crop window, over the strip, and for the paste at the four
//   corners of the piece's cell) and its accuracy bound, 0.6251 units of 2^-16, and the ties-away-from-zero quarter-turn property carry
//   over.  For n = 2 on a parallelogram both pieces hold the maps dmx_edit_quads_persp_prepare fills for that quad and frame; a
//   parallelogram cut at whole-number cell lengths holds them in every piece (relative is scale-invariant).
//
// Crop.  Piece as above; each of the four page taps is blacked out, and counts in the mask, iff some cell of the item covers it; then
//   pre_pixel's order.  Paste.  The items of the pixel's page last to first; within an item the FIRST cell that covers the pixel; the
//   piece by the diagonal's edge function E = (B_k - T_k+1) x ((X, Y) - T_k+1) = (x3 - x1)(Y - y1) - (y3 - y1)(X - x1) over the cell's
//   corners 0..3: 2k iff E >= 0.  The pixel is pasted iff on_crop holds under that piece's paste map, and is the original byte otherwise.
//   Rectify.  Piece as above from (i, j); the tap rule and the single rounding of the quads.
//   Limits: no read-back / select-paste and no blend; no fan cells (a repeated point gives a piece without area: refused); the
//   same number of points on top and bottom; the window's centre is not moved to keep the window on the page.
#pragma once
#include "prepost_persp.h"

namespace dmx_curved {
using dmx_persp::Exact;
using dmx_persp::Mat3;

constexpr int kMaxPairs = DMX_CURVED_MAX_PAIRS;
constexpr int kMaxCells = kMaxPairs - 1;
constexpr int kSizeMax = 1 << 20;              // rw, rh

// rw, rh, c[] and the bounding box of one item with n pairs whose cells have been accepted
inline void fill_strip_size(dmx_edit_curved& it, int n) {
  const int M = n - 1;
  for (int k = 0; k < kMaxPairs; ++k) it.c[k] = 0;
  double sum = 0.0;
  for (int k = 0; k <= M; ++k) {
    const long long dx = (long long)it.x[2 * n - 1 - k] - it.x[k], dy = (long long)it.y[2 * n - 1 - k] - it.y[k];
    sum += sqrt((double)(dx * dx + dy * dy));
    if (k == M) break;
    const long long ux = ((long long)it.x[k + 1] - it.x[k]) + ((long long)it.x[2 * n - 2 - k] - it.x[2 * n - 1 - k]);
    const long long uy = ((long long)it.y[k + 1] - it.y[k]) + ((long long)it.y[2 * n - 2 - k] - it.y[2 * n - 1 - k]);
    const int w = (int)rint(sqrt((double)(ux * ux + uy * uy)) / 2.0);
    it.c[k + 1] = it.c[k] + (w < 1 ? 1 : w);
  }
  it.rw = it.c[M] + 1;
  it.rh = (int)rint(sum / (double)(M + 1)) + 1;
  it.bx1 = it.bx2 = it.x[0]; it.by1 = it.by2 = it.y[0];
  for (int k = 0; k < 2 * n; ++k) {
    it.bx1 = it.x[k] < it.bx1 ? it.x[k] : it.bx1; it.bx2 = it.x[k] > it.bx2 ? it.x[k] : it.bx2;
    it.by1 = it.y[k] < it.by1 ? it.y[k] : it.by1; it.by2 = it.y[k] > it.by2 ? it.y[k] : it.by2;
  }
}

// strip pixel-index space -> page for one piece of a PREPARED item: exact, times w h (corners below 2^16, w, h, c_k at most 2^20)
inline Mat3 piece_to_page(const dmx_edit_curved& it, int n, int piece) {
  const int k = piece >> 1;
  const long long w = it.c[k + 1] - it.c[k], h = it.rh - 1, ck = it.c[k];
  const long long t0[2] = {it.x[k], it.y[k]}, t1[2] = {it.x[k + 1], it.y[k + 1]};
  const long long b1[2] = {it.x[2 * n - 2 - k], it.y[2 * n - 2 - k]}, b0[2] = {it.x[2 * n - 1 - k], it.y[2 * n - 1 - k]};
  long long r[2][3];
  for (int a = 0; a < 2; ++a) {
    if ((piece & 1) == 0) {
      r[a][0] = (t1[a] - t0[a]) * h; r[a][1] = (b0[a] - t0[a]) * w; r[a][2] = t0[a] * w * h - r[a][0] * ck;
    } else {
      r[a][0] = (b1[a] - b0[a]) * h; r[a][1] = (b1[a] - t1[a]) * w; r[a][2] = b1[a] * w * h - r[a][0] * (ck + w) - r[a][1] * h;
    }
  }
  return dmx_persp::ints3(r[0][0], r[0][1], r[0][2], r[1][0], r[1][1], r[1][2], 0, 0, w * h);
}

// what is wrong with an item's frame, or null: fill_derived's checks of prepost_persp.h
inline const char* check_frame(const dmx_edit_curved& it) {
  if (it.crop_scale == 0) return "no frame (crop_scale 0)";
  if (it.crop_scale < 1 || it.crop_scale > 65535) return "crop_scale outside 1 .. 65535";
  if (it.ci2 < -dmx_persp::kCentreMax || it.ci2 > dmx_persp::kCentreMax || it.cj2 < -dmx_persp::kCentreMax || it.cj2 > dmx_persp::kCentreMax)
    return "the centre lies beyond +-2^20 half-pixels";
  return nullptr;
}

// The maps of one piece of a PREPARED item (rw, rh, c filled; the frame checked).  S = 0: the strip map alone.  Returns what is wrong,
// or null; `where` names the map.  The order of the checks is dmx_persp::fill_derived's.
inline const char* fill_piece(const dmx_edit_curved& it, int n, int piece, int S, dmx_curved_piece& x, const char** where) {
  using namespace dmx_persp;
  Exact e;
  const Mat3 G = piece_to_page(it, n, piece);
  if (S >= 1) {
    const Mat3 M = mul3(e, G, ints3(it.crop_scale, 0, (long long)S * it.ci2, 0, it.crop_scale, (long long)S * it.cj2, 0, 0, 2ll * S));
    *where = "the crop window";
    if (!relative(e, M, x.crop)) return "the denominator vanishes at its centre";
    if (!e.ok) return kTooBig;
    const long long g = S - 1, win[4][2] = {{-g, -g}, {g, -g}, {g, g}, {-g, g}};
    if (const char* w = check_window(x.crop, win, true)) return w;
    *where = "the page -> crop map";
    const long long cx2 = e.rdiv_shl(x.crop.c16[0], 0, 32768), cy2 = e.rdiv_shl(x.crop.c16[1], 0, 32768);
    if (cx2 < -(1ll << 30) || cx2 > (1ll << 30) || cy2 < -(1ll << 30) || cy2 > (1ll << 30)) return "the window's centre lies beyond 2^29 page pixels";
    x.cx2 = (int)cx2; x.cy2 = (int)cy2;
    const Mat3 K = mul3(e, ints3(1, 0, S - 1, 0, 1, S - 1, 0, 0, 2), adj3(e, mul3(e, ints3(2, 0, -cx2, 0, 2, -cy2, 0, 0, 1), M)));
    if (!relative(e, K, x.paste)) return "the denominator vanishes at its centre";
    if (!e.ok) return kTooBig;
    const int k = piece >> 1, idx[4] = {k, k + 1, 2 * n - 2 - k, 2 * n - 1 - k};
    long long pts[4][2];
    for (int a = 0; a < 4; ++a) { pts[a][0] = 2ll * it.x[idx[a]] - cx2; pts[a][1] = 2ll * it.y[idx[a]] - cy2; }
    if (const char* w = check_window(x.paste, pts, false)) return w;
  }
  *where = "the strip";
  if (!relative(e, mul3(e, G, ints3(1, 0, it.rw - 1, 0, 1, it.rh - 1, 0, 0, 2)), x.strip)) return "the denominator vanishes at its centre";
  if (!e.ok) return kTooBig;
  const long long gi = it.rw - 1, gj = it.rh - 1, win[4][2] = {{-gi, -gj}, {gi, -gj}, {gi, gj}, {-gi, gj}};
  return check_window(x.strip, win, true);
}

#ifdef __HIPCC__
// the pairs of an item read from the device copy: inside the arrays whatever the table says
__device__ __forceinline__ int pairs(const dmx_edit_curved& it) { return min(max(it.count >> 1, 2), kMaxPairs); }

// cell k of an item with n pairs as the quad predicate takes it
__device__ __forceinline__ dmx_quad::QuadEdges cell_edges(const dmx_edit_curved& it, int n, int k) {
  dmx_quad::QuadEdges e;
  const int idx[4] = {k, k + 1, 2 * n - 2 - k, 2 * n - 1 - k};
#pragma unroll
  for (int a = 0; a < 4; ++a) { e.x[a] = it.x[idx[a]]; e.y[a] = it.y[idx[a]]; }
  e.bx1 = e.bx2 = e.x[0]; e.by1 = e.by2 = e.y[0];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    e.ex[a] = e.x[(a + 1) & 3] - e.x[a]; e.ey[a] = e.y[(a + 1) & 3] - e.y[a];
    e.bx1 = min(e.bx1, e.x[a]); e.bx2 = max(e.bx2, e.x[a]); e.by1 = min(e.by1, e.y[a]); e.by2 = max(e.by2, e.y[a]);
  }
  return e;
}
__device__ __forceinline__ int covers(const dmx_quad::QuadEdges& e, int X, int Y) {
  return X >= e.bx1 && X <= e.bx2 && Y >= e.by1 && Y <= e.by2 && dmx_quad::inside(e, X, Y);
}

// the piece, 0 .. 2M - 1, of the strip position (I / den, J / den): the column band, then the side of the diagonal
__device__ __forceinline__ int piece_of(const int* c, int M, int rh, long long I, long long J, long long den) {
  int k = 0;
  for (int m = 1; m < M; ++m) k += I >= den * c[m] ? 1 : 0;
  const long long w = c[k + 1] - c[k], h = rh - 1;
  return 2 * k + ((I - den * c[k]) * h + J * w <= den * w * h ? 0 : 1);
}
#endif  // __HIPCC__
}  // namespace dmx_curved
