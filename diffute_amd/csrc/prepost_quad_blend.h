// The exact integer arithmetic of the quad blend (prepost_quad_blend.hip; stated in include/diffute_hip.h above
// dmx_paste_color_stats_quads), compiled for host and device: the host-only entries dmx_test_quad_edge_steps / _threshold evaluate the same
// functions the kernels call, and tests/test_quad_blend_host.py compares them with Python ints at magnitudes no small page reaches.
// A float only ESTIMATES; every value returned is fixed by 64-bit integer comparisons, so host and device agree whatever the estimate.
//
// Budget.  |ex|, |ey| <= 65535, so L2 = ex^2 + ey^2 < 2^33; page coordinates <= 65535, so |E| < 2^33.  M = 2 DMX_QUAD_BLEND_MAX + 2 = 2050,
// M^2 < 2^23, M^2 L2 < 2^56.  |E| >= 2^31 lies beyond M sqrt(L2) < 2^28 and saturates by its sign alone; below that E^2 < 2^62 and
// every j^2 L2 compared with it has j <= M + 1: nothing leaves 64 bits.
#pragma once

#ifdef __HIPCC__
#define DMX_QB_HD __host__ __device__ __forceinline__
#else
#define DMX_QB_HD inline
#endif

namespace dmx_quad_blend {

constexpr int kMaxSteps = 2 * DMX_QUAD_BLEND_MAX + 2;                                  // M

// s = floor(E / sqrt(L2)) saturated to [-M, M]: for E >= 0 the largest j >= 0 with j^2 L2 <= E^2, for E < 0 minus the smallest j with
// j^2 L2 >= E^2.  L2 == 0 (an edge of length 0 takes part in nothing): M, the neutral element of the minimum over the edges.
DMX_QB_HD int edge_steps(long long L2, long long E, int M) {
  if (L2 == 0) return M;
  const long long aE = E < 0 ? -E : E;
  if (aE >= (1ll << 31)) return E < 0 ? -M : M;
  const long long E2 = aE * aE;
  const float est = (float)aE / sqrtf((float)L2);                                      // an estimate: the loops below decide
  long long j = est >= (float)(M + 1) ? M + 1 : (long long)est;
  while (j > 0 && j * j * L2 > E2) --j;
  while (j <= M && (j + 1) * (j + 1) * L2 <= E2) ++j;                                  // j = min(floor(|E| / sqrt(L2)), M + 1), exactly
  if (E >= 0) return (int)(j < M ? j : M);
  if (j * j * L2 != E2) ++j;                                                           // the ceiling for a negative E
  return -(int)(j < M ? j : M);
}

// floor(sqrt(v)), 0 <= v < 2^62
DMX_QB_HD long long isqrt_floor(long long v) {
  long long r = (long long)sqrt((double)v);
  while (r > 0 && r * r > v) --r;
  while ((r + 1) * (r + 1) <= v) ++r;
  return r;
}

// The least E with edge_steps(L2, E, .) >= j, for L2 > 0 and |j| <= M: s >= j > 0 iff E >= ceil(j sqrt(L2)); s >= j, j <= 0, iff
// E >= -floor(|j| sqrt(L2)).  j^2 L2 < 2^56.
DMX_QB_HD long long edge_threshold(long long L2, int j) {
  const long long v = (long long)j * j * L2, r = isqrt_floor(v);
  if (j > 0) return r * r == v ? r : r + 1;
  return -r;
}

}  // namespace dmx_quad_blend
