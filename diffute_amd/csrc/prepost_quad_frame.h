// The two frames the quad kernels are written over (prepost_quad.hip: crop, paste, rectify, read-back, select-paste; prepost_quad_blend.hip:
// colour statistics, feathered paste), and the predicate that decides between the decoder's byte and the original one.  Device code only;
// stage() is called on a block of 256 threads.
#pragma once
#include "common.h"
#include "kernels.h"
#include "prepost_quad.h"
#include "prepost_persp.h"

namespace dmx_quad {

constexpr int kQuadInts = (int)(sizeof(dmx_edit_quad) / sizeof(int));
constexpr int kPerspInts = (int)(sizeof(dmx_quad_persp) / sizeof(int));
static_assert(sizeof(dmx_edit_quad) % sizeof(int) == 0 && sizeof(dmx_quad_persp) % sizeof(int) == 0 && kQuadInts + kPerspInts <= 256,
              "a block stages one quad and its projective frame with one int per thread");

// A frame travels to the kernels by value, beside their arguments.  Item: what a block of the crop and of the rectify stages of item b
// in LDS - stage() fills it with one int per thread and ends with ONE barrier.  crop / strip: the page coordinates (Q16) of the grid
// point (p, q) of the staged item's crop / strip.  paste: the crop coordinates of page pixel (x, y) for item b, read from global memory
// (the paste stages edges, not frames); false where the map is not defined.
struct SimilarityFrame {
  struct Item { dmx_edit_quad q; };
  __device__ __forceinline__ void stage(Item& s, const dmx_edit_quad* quads, int b) const {
    if ((int)threadIdx.x < kQuadInts) ((int*)&s.q)[threadIdx.x] = ((const int*)(quads + b))[threadIdx.x];
    __syncthreads();
  }
  __device__ __forceinline__ void crop(const Item& s, long long p, long long q, long long& X16, long long& Y16) const {
    X16 = ((long long)s.q.cx2 << 15) + s.q.fwd[0] * p + s.q.fwd[1] * q;
    Y16 = ((long long)s.q.cy2 << 15) + s.q.fwd[2] * p + s.q.fwd[3] * q;
  }
  __device__ __forceinline__ void strip(const Item& s, long long p, long long q, long long& X16, long long& Y16) const {
    X16 = ((long long)s.q.sx4 << 14) + s.q.rect[0] * p + s.q.rect[1] * q;
    Y16 = ((long long)s.q.sy4 << 14) + s.q.rect[2] * p + s.q.rect[3] * q;
  }
  __device__ __forceinline__ bool paste(const dmx_edit_quad* quads, int b, int S, int x, int y, long long& U16, long long& V16) const {
    const dmx_edit_quad& q = quads[b];
    const long long qx = 2ll * x - q.cx2, qy = 2ll * y - q.cy2, base = (long long)(S - 1) << 15;
    U16 = base + q.inv[0] * qx + q.inv[1] * qy;
    V16 = base + q.inv[2] * qx + q.inv[3] * qy;
    return true;
  }
};

struct ProjectiveFrame {
  const dmx_quad_persp* table;
  struct Item { dmx_edit_quad q; dmx_quad_persp x; };
  __device__ __forceinline__ void stage(Item& s, const dmx_edit_quad* quads, int b) const {
    const int t = threadIdx.x;
    if (t < kQuadInts) ((int*)&s.q)[t] = ((const int*)(quads + b))[t];
    else if (t < kQuadInts + kPerspInts) ((int*)&s.x)[t - kQuadInts] = ((const int*)(table + b))[t - kQuadInts];
    __syncthreads();
  }
  // (a stale table: coords writes nothing, the sample is the page's corner; tap16 clamps anyway)
  __device__ __forceinline__ void crop(const Item& s, long long p, long long q, long long& X16, long long& Y16) const {
    dmx_persp::coords(s.x.crop, p, q, X16, Y16);
  }
  __device__ __forceinline__ void strip(const Item& s, long long p, long long q, long long& X16, long long& Y16) const {
    dmx_persp::coords(s.x.strip, p, q, X16, Y16);
  }
  __device__ __forceinline__ bool paste(const dmx_edit_quad*, int b, int, int x, int y, long long& U16, long long& V16) const {
    const dmx_quad_persp& f = table[b];
    return dmx_persp::coords(f.paste, 2ll * x - f.cx2, 2ll * y - f.cy2, U16, V16);
  }
};

// Item b's crop coordinates of page pixel (x, y), and whether the pixel lies on that crop with the frame's map defined there: what decides
// between the decoder's byte and the original one, in the paste and in the read-back alike.
template <class Frame>
__device__ __forceinline__ bool on_crop(const Frame& frame, const dmx_edit_quad* quads, int b, int S, int x, int y, long long& U16, long long& V16) {
  const long long top = ((long long)S << 16) - 32768;
  return frame.paste(quads, b, S, x, y, U16, V16) && U16 >= -32768 && U16 < top && V16 >= -32768 && V16 < top;
}

}  // namespace dmx_quad
