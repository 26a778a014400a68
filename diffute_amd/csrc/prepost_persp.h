// Quadrilateral text regions seen in PERSPECTIVE, stated once: the projective frame beside prepost_quad.h's similarity frame.  The host
// half is what dmx_edit_quads_persp_prepare fills into a dmx_quad_persp, the device half the coordinates of the three kernels of
// prepost_quad.hip in their projective frame.  tests/persp_restatement.py restates this comment in Python ints and numpy int64 and
// the GPU tests compare bit for bit.  Only WHERE THE COORDINATES COME FROM is new: taps, the single rounding, the predicate, blacking out before resampling and the
// paste rule are dmx_quad::tap16, pre_pixel, page_sample, post_pixel and inside of prepost_quad.h, called, not restated.
//
// Strip space.  rw x rh of prepost_quad.h's rectify section; in the strip's pixel-index space TL <-> (0, 0), TR <-> (rw - 1, 0),
//   BR <-> (rw - 1, rh - 1), BL <-> (0, rh - 1).  rw < 2 or rh < 2 is refused.
//
// Homography G (strip -> page).  The unit square -> quad homography in closed form, multiplied through by its denominator: with
//     dx1 = x1 - x2, dx2 = x3 - x2, sx = x0 - x1 + x2 - x3 (dy1, dy2, sy alike), den = dx1 * dy2 - dy1 * dx2,
//     g = sx * dy2 - sy * dx2, h = dx1 * sy - dy1 * sx
//   the rows are ((x1 - x0) den + g x1, (x3 - x0) den + h x3, x0 den), the same in y, (g, h, den): exact integers.  It is evaluated at
//   u = i / (rw - 1), v = j / (rh - 1):  G = that matrix * diag(rh - 1, rw - 1, (rw - 1)(rh - 1)).
//
// Frame.  (ci2, cj2, crop_scale): the window's centre in half-pixels of the strip's pixel-index space, its side in strip pixels.  Crop
//   pixel (dx, dy) has the grid coordinates (p, q) = (2dx + 1 - S, 2dy + 1 - S) and the strip position i = ci2 / 2 + crop_scale * p / (2S),
//   j alike: grid -> page is the integer homography  M = G * [[crop_scale, 0, S ci2], [0, crop_scale, S cj2], [0, 0, 2S]].
//
// A map as the table holds it (dmx_persp_map), from an integer homography m0..m8 whose sign makes m8 > 0.  rdiv(a, b) is a / b rounded to
//   nearest, TIES AWAY FROM ZERO - it commutes with negation, so a page turned by a quarter, quad turned along, gives the same crop bit
//   for bit; a floor does not.
//     c16[0] = rdiv(m2 * 2^16, m8), c16[1] = rdiv(m5 * 2^16, m8)                        the Q16 image of the grid's centre
//     t0..t2 = rdiv((m_k * 2^16 - c16[0] * m_{6+k}) * 2^(Q-16), m8), k = 0, 1, 2         about that ROUNDED centre: t2 carries its residual
//     t3..t5 alike from m3..m5 and c16[1];   t6 = rdiv(m6 * 2^Q, m8), t7 alike, t8 = 2^Q.      Q = 43
//   Host arithmetic is exact: __int128 products whose operands' bit lengths are checked, no double anywhere, so a table does not depend
//   on a compiler's floating point; matrices are divided by their entries' gcd where they grow (the t are scale-invariant), and a
//   geometry whose intermediates still leave 126 bits is refused.
//
// Device half, 64-bit integers only.  At grid point (p, q):
//     n_x = t0 p + t1 q + t2,   n_y = t3 p + t4 q + t5,   D = t6 p + t7 q + t8
//     X16 = c16[0] + rdiv(n_x * 2^16, D),   Y16 alike,   rdiv in two steps so that nothing leaves an int64:
//     q1 = |n| / D,  r1 = |n| - q1 D,  q2 = ((r1 << 17) + D) / (2D),  result = sign(n) * ((q1 << 16) + q2).
//
// Three maps per item.  crop: M, for the crop.  strip: G * [[1, 0, rw - 1], [0, 1, rh - 1], [0, 0, 2]] on the grid (2i + 1 - rw, 2j + 1 - rh),
//   for the rectified strip.  paste: page -> crop.  (cx2, cy2) = (rdiv(c16[0], 2^15), rdiv(c16[1], 2^15)) of the crop map is the page-side
//   centre in half-pixels; page pixel (X, Y) has the grid coordinates (2X - cx2, 2Y - cy2), and the homography is
//     [[1, 0, S - 1], [0, 1, S - 1], [0, 0, 2]] * adj([[2, 0, -cx2], [0, 2, -cy2], [0, 0, 1]] * M)
//   (the adjugate, not its transpose), giving U16, V16 in the pixel-index space of the S x S decoder output as prepost_quad.h's paste has
//   them.  The paste evaluates it only at pixels some quad covers.
//
// Budget, checked by the host for every map over its window - the crop grid's corners (+-(S - 1), +-(S - 1)), the strip grid's corners,
//   for the paste the quad's four corners - with gx, gy the largest |p|, |q| there.  D is linear, so the corners bound it:
//     min D > 0                                             the horizon does not cross the window
//     max D <= kCap * min D   (crop and strip)              kCap = 4: a stated limit, not a measurement.  Past it the far side of the
//                                                           window is sampled at under a quarter of the near side's linear scale and
//                                                           carries no usable context.
//     max D < 2^45 = 4 * 2^Q                                (r1 << 17) + D < 2^63.  The cap gives max D <= 1.6 * 2^Q on a window, and
//                                                           <= 2.5 * 2^Q at the corners of a quad that lies inside its window.
//     A = |t0| gx + |t1| gy + |t2| < 2^58  (and in y)       bounds |n| and every partial sum of it; q1 << 16 stays far inside
//     ((gx + gy + 1) * (min D + A)) << 18 <= (min D)^2      accuracy: every t is off by at most 1/2, so n by at most (gx + gy + 1) / 2
//                                                           and D by less; 2^16 n / D then moves by less than
//                                                           2^15 (gx + gy + 1)(min D + A) / (min D)^2 * (1 + 2^-18) < 0.1251, and with the
//                                                           final rdiv X16 is within 0.6251 of the exact coordinate * 2^16.
//   For a 700-pixel line on a 1100 x 1300 page at S = 512: A < 2^53, min D > 2^41.
//   Limits: the window's centre is NOT moved to keep the window on the page (clamped taps replicate the border); a window beyond the
//   cap is refused; a line on an arc is no quad: curved text is prepost_curved.h's, whose affine pieces are maps of this kind.
#pragma once
#include "prepost_quad.h"

namespace dmx_persp {
constexpr int kQ = 43;                      // t8 = 2^kQ
constexpr int kCap = 4;                     // max D <= kCap * min D over a crop window and over a strip
constexpr long long kDMax = 1ll << 45;
constexpr long long kNMax = 1ll << 58;
constexpr int kErrShift = 18;
constexpr int kCentreMax = 1 << 20;         // |ci2|, |cj2|

typedef __int128 i128;

// exact integers with a sticky overflow flag: every product and sum is formed only if it provably fits
struct Exact {
  bool ok = true;
  static int bits(i128 a) {
    unsigned __int128 u = a < 0 ? -(unsigned __int128)a : (unsigned __int128)a;
    const unsigned long long hi = (unsigned long long)(u >> 64), lo = (unsigned long long)u;
    return hi ? 128 - __builtin_clzll(hi) : (lo ? 64 - __builtin_clzll(lo) : 0);
  }
  i128 mul(i128 a, i128 b) {
    if (bits(a) + bits(b) > 125) { ok = false; return 0; }
    return a * b;
  }
  i128 add(i128 a, i128 b) {
    if (bits(a) > 125 || bits(b) > 125) { ok = false; return 0; }
    return a + b;
  }
  i128 shl(i128 a, int s) {
    if (bits(a) + s > 125) { ok = false; return 0; }
    return a * ((i128)1 << s);
  }
  // rdiv(a * 2^s, d), d > 0, as a long division: quotient of a first, then the shifted remainder
  long long rdiv_shl(i128 a, int s, i128 d) {
    if (d <= 0 || bits(d) + s + 2 > 125) { ok = false; return 0; }
    const bool neg = a < 0;
    const i128 m = neg ? -a : a;
    if (bits(m) + s + 2 <= 125) {                              // the shifted numerator fits: one division
      const i128 r = (2 * (m * ((i128)1 << s)) + d) / (2 * d);
      if (bits(r) > 61) { ok = false; return 0; }
      return (long long)(neg ? -r : r);
    }
    const i128 q1 = m / d, r1 = m - q1 * d;
    if (bits(q1) + s > 61) { ok = false; return 0; }
    const i128 r = q1 * ((i128)1 << s) + (2 * (r1 * ((i128)1 << s)) + d) / (2 * d);
    return (long long)(neg ? -r : r);
  }
};

struct Mat3 { i128 m[9]; };

inline i128 gcd128(i128 a, i128 b) {
  a = a < 0 ? -a : a; b = b < 0 ? -b : b;
  while (b) { const i128 t = a % b; a = b; b = t; }
  return a;
}
// a homography is its own multiple: where an entry has grown past 62 bits, divide by the entries' gcd
inline void reduce(Mat3& a) {
  int top = 0;
  for (int k = 0; k < 9; ++k) top = Exact::bits(a.m[k]) > top ? Exact::bits(a.m[k]) : top;
  if (top <= 62) return;
  i128 g = 0;
  for (int k = 0; k < 9; ++k) g = gcd128(g, a.m[k]);
  if (g > 1) for (int k = 0; k < 9; ++k) a.m[k] /= g;
}
inline Mat3 mul3(Exact& e, const Mat3& a, const Mat3& b) {
  Mat3 r;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      r.m[i * 3 + j] = e.add(e.add(e.mul(a.m[i * 3], b.m[j]), e.mul(a.m[i * 3 + 1], b.m[3 + j])), e.mul(a.m[i * 3 + 2], b.m[6 + j]));
  reduce(r);
  return r;
}
inline Mat3 adj3(Exact& e, const Mat3& s) {
  const i128* m = s.m;
  auto det2 = [&](int a, int b, int c, int d) { return e.add(e.mul(m[a], m[b]), -e.mul(m[c], m[d])); };
  Mat3 r = {{det2(4, 8, 5, 7), det2(2, 7, 1, 8), det2(1, 5, 2, 4), det2(5, 6, 3, 8), det2(0, 8, 2, 6), det2(2, 3, 0, 5), det2(3, 7, 4, 6),
             det2(1, 6, 0, 7), det2(0, 4, 1, 3)}};
  reduce(r);
  return r;
}
inline Mat3 ints3(long long a, long long b, long long c, long long d, long long f, long long g, long long h, long long i, long long j) {
  return Mat3{{a, b, c, d, f, g, h, i, j}};
}

// strip pixel-index space -> page
inline Mat3 strip_to_page(Exact& e, const dmx_edit_quad& q) {
  const long long x0 = q.x[0], x1 = q.x[1], x2 = q.x[2], x3 = q.x[3], y0 = q.y[0], y1 = q.y[1], y2 = q.y[2], y3 = q.y[3];
  const long long dx1 = x1 - x2, dx2 = x3 - x2, sx = x0 - x1 + x2 - x3, dy1 = y1 - y2, dy2 = y3 - y2, sy = y0 - y1 + y2 - y3;
  const long long den = dx1 * dy2 - dy1 * dx2, g = sx * dy2 - sy * dx2, h = dx1 * sy - dy1 * sx;       // (corners below 2^16: below 2^35)
  const Mat3 unit = ints3((x1 - x0) * den + g * x1, (x3 - x0) * den + h * x3, x0 * den, (y1 - y0) * den + g * y1, (y3 - y0) * den + h * y3, y0 * den, g,
                          h, den);
  const long long a1 = q.rw - 1, b1 = q.rh - 1;
  return mul3(e, unit, ints3(b1, 0, 0, 0, a1, 0, 0, 0, a1 * b1));
}

// an integer homography as the table holds it; false where the denominator vanishes at the centre
inline bool relative(Exact& e, Mat3 a, dmx_persp_map& out) {
  if (a.m[8] < 0) for (int k = 0; k < 9; ++k) a.m[k] = -a.m[k];
  const i128 m8 = a.m[8];
  if (m8 == 0) return false;
  for (int r = 0; r < 2; ++r) {
    out.c16[r] = e.rdiv_shl(a.m[r * 3 + 2], 16, m8);
    for (int k = 0; k < 3; ++k)
      out.t[r * 3 + k] = e.rdiv_shl(e.add(e.shl(a.m[r * 3 + k], 16), -e.mul(out.c16[r], a.m[6 + k])), kQ - 16, m8);
  }
  out.t[6] = e.rdiv_shl(a.m[6], kQ, m8); out.t[7] = e.rdiv_shl(a.m[7], kQ, m8); out.t[8] = 1ll << kQ;
  return true;
}

// one map over its window: pts are the window's four corners in grid coordinates.  Returns what is wrong, or null.
inline const char* check_window(const dmx_persp_map& m, const long long pts[4][2], bool cap) {
  i128 dmin = 0, dmax = 0;
  long long gx = 0, gy = 0;
  for (int k = 0; k < 4; ++k) {
    const i128 d = (i128)m.t[6] * pts[k][0] + (i128)m.t[7] * pts[k][1] + m.t[8];
    dmin = (k == 0 || d < dmin) ? d : dmin; dmax = (k == 0 || d > dmax) ? d : dmax;
    const long long ax = pts[k][0] < 0 ? -pts[k][0] : pts[k][0], ay = pts[k][1] < 0 ? -pts[k][1] : pts[k][1];
    gx = ax > gx ? ax : gx; gy = ay > gy ? ay : gy;
  }
  if (dmin <= 0) return "the denominator is not positive at all four corners (the horizon crosses it)";
  if (cap && dmax > kCap * dmin) return "the denominators' ratio over it lies beyond the cap of 4";
  if (dmax >= kDMax) return "the denominator leaves the budget";
  for (int r = 0; r < 6; r += 3) {
    auto mag = [](long long v) { return (i128)(v < 0 ? -(i128)v : (i128)v); };
    const i128 A = mag(m.t[r]) * gx + mag(m.t[r + 1]) * gy + mag(m.t[r + 2]);                 // (each t below 2^62, gx below 2^21)
    if (A >= kNMax || (((i128)(gx + gy + 1) * (dmin + A)) << kErrShift) > dmin * dmin) return "the numerator leaves the budget";
  }
  return nullptr;
}

inline const char* kTooBig = "the geometry leaves the host's 126-bit integers";
inline const char* kThin = "the strip is thinner than 2 pixels (rw, rh >= 2)";

// The strip map of one PREPARED quad (it depends on no frame and no S).  Returns what is wrong, or null.
inline const char* fill_strip(const dmx_edit_quad& q, dmx_quad_persp& x) {
  if (q.rw < 2 || q.rh < 2) return kThin;
  Exact e;
  if (!relative(e, mul3(e, strip_to_page(e, q), ints3(1, 0, q.rw - 1, 0, 1, q.rh - 1, 0, 0, 2)), x.strip)) return "the denominator vanishes at its centre";
  if (!e.ok) return kTooBig;
  const long long gi = q.rw - 1, gj = q.rh - 1, win[4][2] = {{-gi, -gj}, {gi, -gj}, {gi, gj}, {-gi, gj}};
  return check_window(x.strip, win, true);
}

// The derived fields of one item's projective frame, from the PREPARED quad and the caller-filled ci2, cj2, crop_scale.  Returns what
// is wrong with the item, or null; `where` names the map.
inline const char* fill_derived(const dmx_edit_quad& q, dmx_quad_persp& x, int S, const char** where) {
  *where = "the frame";
  if (q.rw < 2 || q.rh < 2) return kThin;
  if (x.crop_scale == 0) return "no projective frame (crop_scale 0)";
  if (x.crop_scale < 1 || x.crop_scale > 65535) return "crop_scale outside 1 .. 65535";
  if (x.ci2 < -kCentreMax || x.ci2 > kCentreMax || x.cj2 < -kCentreMax || x.cj2 > kCentreMax) return "the centre lies beyond +-2^20 half-pixels";
  Exact e;
  const Mat3 M = mul3(e, strip_to_page(e, q), ints3(x.crop_scale, 0, (long long)S * x.ci2, 0, x.crop_scale, (long long)S * x.cj2, 0, 0, 2ll * S));
  *where = "the crop window";
  if (!relative(e, M, x.crop)) return "the denominator vanishes at its centre";
  if (!e.ok) return kTooBig;
  const long long g = S - 1, win[4][2] = {{-g, -g}, {g, -g}, {g, g}, {-g, g}};
  if (const char* w = check_window(x.crop, win, true)) return w;
  *where = "the strip";
  if (const char* w = fill_strip(q, x)) return w;
  *where = "the page -> crop map";
  const long long cx2 = e.rdiv_shl(x.crop.c16[0], 0, 32768), cy2 = e.rdiv_shl(x.crop.c16[1], 0, 32768);
  if (cx2 < -(1ll << 30) || cx2 > (1ll << 30) || cy2 < -(1ll << 30) || cy2 > (1ll << 30)) return "the window's centre lies beyond 2^29 page pixels";
  x.cx2 = (int)cx2; x.cy2 = (int)cy2; x.reserved = 0;
  const Mat3 K = mul3(e, ints3(1, 0, S - 1, 0, 1, S - 1, 0, 0, 2), adj3(e, mul3(e, ints3(2, 0, -cx2, 0, 2, -cy2, 0, 0, 1), M)));
  if (!relative(e, K, x.paste)) return "the denominator vanishes at its centre";
  if (!e.ok) return kTooBig;
  long long pts[4][2];
  for (int k = 0; k < 4; ++k) { pts[k][0] = 2ll * q.x[k] - cx2; pts[k][1] = 2ll * q.y[k] - cy2; }
  return check_window(x.paste, pts, false);
}

#ifdef __HIPCC__
// rdiv(n * 2^16, D) for D > 0, in two steps
__device__ __forceinline__ long long div16(long long n, long long D) {
  const long long a = n < 0 ? -n : n, q1 = a / D, r1 = a - q1 * D;
  const long long r = (q1 << 16) + ((r1 << 17) + D) / (2 * D);
  return n < 0 ? -r : r;
}
// the Q16 coordinates of grid point (p, q) under one map; false (and nothing written) where D is not positive or beyond the budget -
// a table the host accepted never gives that
__device__ __forceinline__ bool coords(const dmx_persp_map& m, long long p, long long q, long long& X16, long long& Y16) {
  const long long D = m.t[6] * p + m.t[7] * q + m.t[8];
  if (D <= 0 || D >= kDMax) return false;
  X16 = m.c16[0] + div16(m.t[0] * p + m.t[1] * q + m.t[2], D);
  Y16 = m.c16[1] + div16(m.t[3] * p + m.t[4] * q + m.t[5], D);
  return true;
}
#endif  // __HIPCC__
}  // namespace dmx_persp
