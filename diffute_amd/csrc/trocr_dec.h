// The TrOCR text decoder's model handle and the device code shared by the step path (trocr_dec.hip) and the teacher-forced
// prefill (trocr_prefill.hip): the wave reductions, the greedy order and the embedding row
#pragma once
#include <vector>
#include "exec.h"

// byte offsets of one layer's parameters in the weights arena
struct DecLayer { size_t wqkv, bqkv, wo, bo, l1g, l1b, wcq, bcq, wco, bco, l2g, l2b, w1, b1, w2, b2, l3g, l3b; };

struct dmx_trocr_dec : ModelBase {
  dmx_trocr_dec_config cfg;
  size_t emb, posw, leg = 0, leb = 0, wckv, bckv, lm;
  int npos = 0, kdim = 0, cnt_slice = 0;
  std::vector<DecLayer> layers;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
  return v;
}
// greedy order: larger value first, equal values -> lower index (torch.argmax); NaN never wins
__device__ __forceinline__ bool pick_better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }
__device__ __forceinline__ void pick_merge(float& bv, int& bi, float v, int i) { if (pick_better(v, i, bv, bi)) { bv = v; bi = i; } }

// row m of x = LN(embed[tok] * scale + pos_table[prow]) (LN skipped without gamma) by one wave, D = 64 nper values: the fp32
// stream and its 16-bit copy.  tok and prow arrive clamped to their tables
__device__ __forceinline__ void dec_embed_row(int tok, int prow, int lane, int m, const bf16* emb, const float* posw, float scale,
                                              const float* gamma, const float* beta, int D, float* yf, bf16* yb) {
  const int nper = D >> 6;
  float v[16];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) {                                // (clamped, unconditional loads: all in flight together)
    const int n = min(j, nper - 1) * 64 + lane;
    v[j] = (float)emb[(size_t)tok * D + n] * scale + posw[(size_t)prow * D + n];
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) if (j < nper) s += v[j];
  if (gamma) {
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) if (j < nper) { const float d = v[j] - mean; q += d * d; }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + 1e-5f);
#pragma unroll
    for (int j = 0; j < 16; ++j) if (j < nper) { const int n = j * 64 + lane; v[j] = (v[j] - mean) * rstd * gamma[n] + beta[n]; }
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) if (j < nper) {
    const int n = j * 64 + lane;
    yf[(size_t)m * D + n] = v[j];
    yb[(size_t)m * D + n] = (bf16)v[j];
  }
}
