// Multi-tensor EMA update and cast-copy (diffusers EMAModel; reference: `ema_unet.step(unet.parameters())`,
// train_diffute_v1.py:934-935, and copy_to / store / restore).  One launch per call whatever the number of tensors: the
// host builds a table of <= 64 Ki-element chunks (dmx_multi_chunk, include/diffute_hip.h), one block per chunk.
//
// Per element of an EMA entry, diffusers' `s.sub_(one_minus_decay * (s - p))` with torch's type promotion: the two
// intermediates are rounded to T = promote(shadow dtype, param dtype) (the shared dtype when they agree, fp32 otherwise),
// the in-place subtraction to the shadow's dtype; every op is computed in fp32 (torch's opmath) with explicit _rn ops
// (the library builds with -ffp-contract=off).  16-bit roundings are RNE (torch's casts).
// The 16-bit types are named explicitly (__bf16 / _Float16), not through common.h's build-dependent element type: the
// bf16 and the fp16 builds of the library run the same arithmetic here.
#include "common.h"
#include "kernels.h"

namespace {

template <int DT> struct Elem;
template <> struct Elem<DMX_DT_F32> {
  static __device__ __forceinline__ float load(const void* p, size_t i) { return ((const float*)p)[i]; }
  static __device__ __forceinline__ void store(void* p, size_t i, float v) { ((float*)p)[i] = v; }
  static __device__ __forceinline__ float round(float v) { return v; }
};
template <> struct Elem<DMX_DT_BF16> {
  static __device__ __forceinline__ float load(const void* p, size_t i) {
    return __uint_as_float(((unsigned int)((const unsigned short*)p)[i]) << 16);
  }
  static __device__ __forceinline__ unsigned short bits(float v) { return __builtin_bit_cast(unsigned short, (__bf16)v); }
  static __device__ __forceinline__ void store(void* p, size_t i, float v) { ((unsigned short*)p)[i] = bits(v); }
  static __device__ __forceinline__ float round(float v) { return __uint_as_float(((unsigned int)bits(v)) << 16); }
};
template <> struct Elem<DMX_DT_F16> {
  static __device__ __forceinline__ float load(const void* p, size_t i) {
    return (float)__builtin_bit_cast(_Float16, ((const unsigned short*)p)[i]);
  }
  static __device__ __forceinline__ unsigned short bits(float v) { return __builtin_bit_cast(unsigned short, (_Float16)v); }
  static __device__ __forceinline__ void store(void* p, size_t i, float v) { ((unsigned short*)p)[i] = bits(v); }
  static __device__ __forceinline__ float round(float v) { return (float)(_Float16)v; }
};

// new shadow value (dtype SD) from shadow s and parameter p, both widened to fp32
template <int SD, int PD> __device__ __forceinline__ float ema_elem(float s, float p, float omd) {
  typedef Elem<SD == PD ? SD : DMX_DT_F32> T;
  const float d = T::round(__fsub_rn(s, p));
  const float m = T::round(__fmul_rn(omd, d));
  return Elem<SD>::round(__fsub_rn(s, m));
}

// 4-element groups; fp32 groups are one 16-byte access, 16-bit groups one 8-byte access
template <int DT> struct Vec4;
template <> struct Vec4<DMX_DT_F32> {
  static __device__ __forceinline__ void load(const void* p, size_t g, float* v) {
    const float4 x = ((const float4*)p)[g]; v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
  }
  static __device__ __forceinline__ void store(void* p, size_t g, const float* v) { ((float4*)p)[g] = make_float4(v[0], v[1], v[2], v[3]); }
};
template <int DT> struct Vec4 {          // bf16 / fp16
  static __device__ __forceinline__ void load(const void* p, size_t g, float* v) {
    const uint2 x = ((const uint2*)p)[g];
    const unsigned short h[4] = {(unsigned short)(x.x & 0xffffu), (unsigned short)(x.x >> 16), (unsigned short)(x.y & 0xffffu), (unsigned short)(x.y >> 16)};
    for (int k = 0; k < 4; ++k) v[k] = Elem<DT>::load(h, k);
  }
  static __device__ __forceinline__ void store(void* p, size_t g, const float* v) {
    unsigned short h[4];
    for (int k = 0; k < 4; ++k) h[k] = Elem<DT>::bits(v[k]);
    ((uint2*)p)[g] = make_uint2((unsigned)h[0] | ((unsigned)h[1] << 16), (unsigned)h[2] | ((unsigned)h[3] << 16));
  }
};

// one chunk: dst (dtype SD) <- EMA(dst, src) or cast(src); src has dtype PD
template <int SD, int PD> __device__ __forceinline__ void run_chunk(const dmx_multi_chunk& c, float omd, int all_copy) {
  const bool copy = all_copy || c.mode == DMX_MULTI_COPY;
  const size_t n = c.count;
  size_t done = 0;
  if ((((uintptr_t)c.dst | (uintptr_t)c.src) & 15) == 0) {
    const size_t ng = n / 4;
    for (size_t g = threadIdx.x; g < ng; g += blockDim.x) {
      float s[4], p[4];
      Vec4<PD>::load(c.src, g, p);
      if (copy) {
        for (int k = 0; k < 4; ++k) s[k] = Elem<SD>::round(p[k]);
      } else {
        Vec4<SD>::load(c.dst, g, s);
        for (int k = 0; k < 4; ++k) s[k] = ema_elem<SD, PD>(s[k], p[k], omd);
      }
      Vec4<SD>::store(c.dst, g, s);
    }
    done = ng * 4;
  }
  for (size_t i = done + threadIdx.x; i < n; i += blockDim.x) {
    const float p = Elem<PD>::load(c.src, i);
    Elem<SD>::store(c.dst, i, copy ? p : ema_elem<SD, PD>(Elem<SD>::load(c.dst, i), p, omd));
  }
}

template <int SD> __device__ __forceinline__ void run_chunk_sd(const dmx_multi_chunk& c, float omd, int all_copy) {
  switch (c.src_dtype) {
    case DMX_DT_F32: run_chunk<SD, DMX_DT_F32>(c, omd, all_copy); break;
    case DMX_DT_BF16: run_chunk<SD, DMX_DT_BF16>(c, omd, all_copy); break;
    case DMX_DT_F16: run_chunk<SD, DMX_DT_F16>(c, omd, all_copy); break;
  }
}

// one block per chunk; the dtype switch is uniform over the block.  all_copy: every entry is a cast-copy (dmx_copy_multi)
__global__ __launch_bounds__(256) void dmx_multi_kernel(const dmx_multi_chunk* table, float omd, int all_copy) {
  const dmx_multi_chunk c = table[blockIdx.x];
  switch (c.dst_dtype) {
    case DMX_DT_F32: run_chunk_sd<DMX_DT_F32>(c, omd, all_copy); break;
    case DMX_DT_BF16: run_chunk_sd<DMX_DT_BF16>(c, omd, all_copy); break;
    case DMX_DT_F16: run_chunk_sd<DMX_DT_F16>(c, omd, all_copy); break;
  }
}

int multi_launch(const void* table, int nchunks, float omd, int all_copy, hipStream_t stream) {
  if (nchunks == 0) return DMX_OK;
  hipLaunchKernelGGL(dmx_multi_kernel, dim3(nchunks), dim3(256), 0, stream, (const dmx_multi_chunk*)table, omd, all_copy);
  return dmx_check_launch("dmx_multi_kernel");
}

}  // namespace

extern "C" int dmx_ema_step_multi(const void* table, int nchunks, float one_minus_decay, dmx_stream_t stream) {
  DMX_REQUIRE(nchunks >= 0, "ema_step_multi: nchunks %d < 0", nchunks);
  DMX_REQUIRE(table || nchunks == 0, "ema_step_multi: null table");
  return multi_launch(table, nchunks, one_minus_decay, 0, (hipStream_t)stream);
}
extern "C" int dmx_copy_multi(const void* table, int nchunks, dmx_stream_t stream) {
  DMX_REQUIRE(nchunks >= 0, "copy_multi: nchunks %d < 0", nchunks);
  DMX_REQUIRE(table || nchunks == 0, "copy_multi: null table");
  return multi_launch(table, nchunks, 0.0f, 1, (hipStream_t)stream);
}
