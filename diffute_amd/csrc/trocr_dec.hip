// OCR read-back: the text decoder of TrOCR (reference: `full_trocr_model = VisionEncoderDecoderModel.from_pretrained(
// 'microsoft/trocr-large-printed')`, app.ipynb:548; `full_trocr_model_te.generate(pixel_values)`, :845).  Module structure =
// transformers' TrOCRForCausalLM (BART-style post-LN decoder):
//   x = LN_emb(embed_tokens[tok] * scale + embed_positions[pos + 2])
//   L x { x = LN(x + o(self_attn(qkv(x))));  x = LN(x + o(cross_attn(q(x), K/V(enc))));  x = LN(x + fc2(act(fc1(x)))) }
//   logits = x output_projection^T  (tied to embed_tokens unless the checkpoint says otherwise)
// Greedy decode is batch-small (M = number of crops <= 64) and weight-streaming: every kernel of a step reads its weights once.
//   dec_linear  - y[M][N] = x[M][K] W[N][K]^T on v_mfma_f32_16x16x32 with the M rows padded to 16 in registers (zero lanes), 64
//                 output features per block, K split over blockIdx.y.  The split partials are combined by the LAST block of each
//                 feature tile to arrive (integer counter, fixed summation order s = 0..splits-1: deterministic, no float atomics),
//                 which also applies the epilogue: bias [+ act] | q-scale + K/V-cache write | + residual and, through a second
//                 counter over the tiles, the row LayerNorm | logits + per-block (max, lowest index) and the greedy pick.
//   dec_attn    - one query row per (b, head), d = 64, split over 64-key chunks; the last chunk block combines in chunk order.
//   dec_embed   - token + position (+ scale) + layernorm_embedding, token and position read from device memory (the row's
//                 arithmetic, the wave reductions and the greedy order are in trocr_dec.h, shared with the prefill).
// Per step: 1 + 8 per layer + 1 launches; the counters reset themselves, so one captured graph replays every step.
// Beam search (rows = items x beams) runs the same step with an LM head that writes fp32 logits + log-sum-exp partials, one
//   beam_select launch (top 2 x beams candidates per item, running / finished bookkeeping, loop condition) and an ancestry table through which
//   the self-attention reads the never-reordered K/V cache: 1 + 8 per layer + 2 launches.
#include <math.h>
#include <memory>
#include <string>
#include <vector>
#include "trocr_dec.h"

namespace {
enum { EPI_STORE = 0, EPI_QKV = 1, EPI_LN = 2, EPI_PICK = 3, EPI_BEAM = 4 };
enum { ACT_NONE = 0, ACT_GELU = 1, ACT_RELU = 2 };
// state words at the start of the cache: the public header's names, and the words reserved for them in front of the counters
enum { ST_POS = DMX_TROCR_STATE_POS, ST_DONE = DMX_TROCR_STATE_DONE, ST_STOP = DMX_TROCR_STATE_STOP_LEN, ST_TOK = DMX_TROCR_STATE_TOKENS,
       ST_FIN = DMX_TROCR_STATE_FINISHED, ST_INTS = 256 };
// beam state block (DMX_TROCR_BEAM_* in the header): int32 / fp32 words, then the token history int32 [max_len][64], the
// finished ids int32 [64][max_len] and the two ancestry tables uint8 [2][64][max_len]
enum { BS_RUN = 0, BS_FSC = 64, BS_FFLAG = 128, BS_FLEN = 192, BS_IMPR = 256, BS_PARENT = 320, BS_FULL = 384, BS_HIT = 448,
       BS_CNT = 512, BS_STEPS = 580, BS_WORDS = 640 };
constexpr int kBeamMaxK = 32, kBeamLds = 8192, kBeamEntries = kBeamLds / 2;

struct DecLin {
  const bf16* x; int ldx;            // [M][K]
  const bf16* w; int ldw;            // [N][K]
  const float* bias;                 // [N] or null
  int M, N, K, kchunk, splits;
  float* part;                       // [splits][M][N] fp32 (splits > 1)
  int* cnt;                          // [gridDim.x + 1] self-resetting counters (zero on entry)
  int epi, act;
  float oscale;                      // EPI_STORE: y = act(acc + bias) * oscale
  float* yf; int ldyf;               // fp32 out (EPI_STORE / EPI_QKV: q / EPI_LN: hidden / EPI_PICK: logits, optional)
  bf16* yb; int ldyb;                // bf16 out (EPI_STORE / EPI_LN)
  // EPI_QKV: columns [0, D) are q (-> yf, times oscale), [D, 3D) k|v -> kv + m * kv_bstride + pos * 2D
  bf16* kv; long long kv_bstride; const int* state; int D;
  // EPI_LN: pre = acc + bias + res; then LN over the row (gamma, beta, eps) -> yf, yb
  const float* res; float* pre; const float* gamma; const float* beta; float eps;
  // EPI_PICK: per-block partials [M][gridDim.x], then the greedy pick into state / ids
  float* pv; int* pi; long long* ids; int max_len, eos, pad;
  // EPI_BEAM: logits -> yf; per-block (max, sum exp(x - max)) -> pv, psum [M][gridDim.x]
  float* psum;
};

// Cross-block hand-offs: the data another block of the same launch reads are stored WRITE-THROUGH (sc1 buffer stores) and read
// with sc1 loads, so publishing needs no agent-scope release / acquire fence (buffer_wbl2 walks the whole L2, buffer_inv drops it:
// microseconds per block - the recipe of gemm.hip's stream-K fix-up)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wt_rsrc(const void* base, size_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, 0x00020000);
}
__device__ __forceinline__ void wt_store(__amdgpu_buffer_rsrc_t rs, size_t idx, float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rs, (int)(idx * 4), 0, 16);
}
__device__ __forceinline__ void wt_store_i(__amdgpu_buffer_rsrc_t rs, size_t idx, int v) {
  __builtin_amdgcn_raw_buffer_store_b32((unsigned)v, rs, (int)(idx * 4), 0, 16);
}
__device__ __forceinline__ float wt_load(__amdgpu_buffer_rsrc_t rs, size_t idx) {
  return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (int)(idx * 4), 0, 16));
}
__device__ __forceinline__ int wt_load_i(__amdgpu_buffer_rsrc_t rs, size_t idx) {
  return (int)__builtin_amdgcn_raw_buffer_load_b32(rs, (int)(idx * 4), 0, 16);
}
// four consecutive floats (idx % 4 == 0)
__device__ __forceinline__ void wt_store4(__amdgpu_buffer_rsrc_t rs, size_t idx, f32x4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rs, (int)(idx * 4), 0, 16);
}
__device__ __forceinline__ f32x4 wt_load4(__amdgpu_buffer_rsrc_t rs, size_t idx) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(idx * 4), 0, 16));
}

// the block that increments `c` last (of `total` arrivals) returns true; every arrival's write-through stores have drained
// before its increment.  The last one resets the counter for the next launch.
__device__ __forceinline__ bool last_arrival(int* c, int total) {
  __shared__ int s_last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const int old = __hip_atomic_fetch_add(c, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = (old == total - 1);
    if (s_last) __hip_atomic_store(c, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  return s_last != 0;
}

// one row of the LayerNorm tail: v = this lane's nper = N / 64 consecutive values (columns lane * nper + e, nper % 4 == 0), held
// in one vector register tuple; gamma / beta come in the same layout, loaded once per tail; the row leaves with 16-byte stores
__device__ __forceinline__ void ln_row(f32x16 v, int nper, int N, int m, f32x16 g, f32x16 b, float eps, float* yf, bf16* yb) {
  const int c0 = (threadIdx.x & 63) * nper;
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) if (e < nper) s += v[e];
  const float mean = wave_sum(s) / (float)N;
  float sq = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) if (e < nper) { const float d = v[e] - mean; sq += d * d; }
  const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)N + eps);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (4 * q >= nper) break;
    float y[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = (v[4 * q + e] - mean) * rstd * g[4 * q + e] + b[4 * q + e];
    *(f32x4*)(yf + (size_t)m * N + c0 + 4 * q) = (f32x4){y[0], y[1], y[2], y[3]};
    *(u32x2*)(yb + (size_t)m * N + c0 + 4 * q) = (u32x2){pack_bf2(y[0], y[1]), pack_bf2(y[2], y[3])};
  }
}
__device__ __forceinline__ f32x16 ln_load(__amdgpu_buffer_rsrc_t rs, size_t row0, int nper) {
  const int c0 = (threadIdx.x & 63) * nper;
  f32x16 v;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 u = wt_load4(rs, row0 + c0 + min(q, nper / 4 - 1) * 4);
    v[4 * q] = u[0]; v[4 * q + 1] = u[1]; v[4 * q + 2] = u[2]; v[4 * q + 3] = u[3];
  }
  return v;
}
__device__ __forceinline__ f32x16 ln_vec(const float* p, int nper) {
  const int c0 = (threadIdx.x & 63) * nper;
  f32x16 v;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const f32x4 u = *(const f32x4*)(p + c0 + min(q, nper / 4 - 1) * 4);
    v[4 * q] = u[0]; v[4 * q + 1] = u[1]; v[4 * q + 2] = u[2]; v[4 * q + 3] = u[3];
  }
  return v;
}
// row LayerNorm of pre[M][N] (N % 256 == 0, N <= 1024) by one block: wave w takes rows w, w + 4, ..., four rows at a time with
// all of their loads in flight together (the tail is a chain of round trips, not of bandwidth)
__device__ void rows_layernorm(const float* pre, int M, int N, const float* gamma, const float* beta, float eps, float* yf, bf16* yb) {
  const int wv = threadIdx.x >> 6, nper = N >> 6;
  const __amdgpu_buffer_rsrc_t rs = wt_rsrc(pre, (size_t)M * N * 4);
  const f32x16 g = ln_vec(gamma, nper), b = ln_vec(beta, nper);
  for (int m0 = wv; m0 < M; m0 += 16) {
    const f32x16 v0 = ln_load(rs, (size_t)m0 * N, nper);
    const f32x16 v1 = ln_load(rs, (size_t)min(m0 + 4, M - 1) * N, nper);
    const f32x16 v2 = ln_load(rs, (size_t)min(m0 + 8, M - 1) * N, nper);
    const f32x16 v3 = ln_load(rs, (size_t)min(m0 + 12, M - 1) * N, nper);
    ln_row(v0, nper, N, m0, g, b, eps, yf, yb);
    if (m0 + 4 < M) ln_row(v1, nper, N, m0 + 4, g, b, eps, yf, yb);
    if (m0 + 8 < M) ln_row(v2, nper, N, m0 + 8, g, b, eps, yf, yb);
    if (m0 + 12 < M) ln_row(v3, nper, N, m0 + 12, g, b, eps, yf, yb);
  }
}

template <int MT>
__global__ __launch_bounds__(256) void dmx_dec_linear_kernel(DecLin a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int g = lane >> 4, r = lane & 15;
  const int nb = blockIdx.x, s = blockIdx.y;
  const int n0 = nb * 64 + wv * 16;
  const int k_beg = s * a.kchunk, k_end = min(a.K, k_beg + a.kchunk);
  // lane (g, r): weight row n0 + r and activation rows t*16 + r, k = kb + 32 g + 8 j + e for MFMA j - the same k set in A and B,
  // so each lane reads one contiguous 64-byte run per operand and 128-k step
  const bool wok = n0 + r < a.N;
  const bf16* wp = a.w + (size_t)(wok ? n0 + r : 0) * a.ldw + g * 32;
  const bf16* xp[MT];
  bool xok[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    xok[t] = t * 16 + r < a.M;
    xp[t] = a.x + (size_t)(xok[t] ? t * 16 + r : 0) * a.ldx + g * 32;
  }
  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int k = k_beg; k < k_end; k += 128) {
    u32x4 wa[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wa[j] = wok ? *(const u32x4*)(wp + k + j * 8) : zero;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      u32x4 xb[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) xb[j] = xok[t] ? *(const u32x4*)(xp[t] + k + j * 8) : zero;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[t] = DMX_MFMA_16x16x32(__builtin_bit_cast(bf16x8, wa[j]), __builtin_bit_cast(bf16x8, xb[j]), acc[t]);
    }
  }
  // acc[t][i]: feature n0 + 4 g + i, row t * 16 + r
  if (a.splits > 1) {
    const size_t plane = (size_t)a.M * a.N;
    const __amdgpu_buffer_rsrc_t rs = wt_rsrc(a.part, plane * a.splits * 4);
    // split planes hold 16-byte runs: the four features n0 + 4g .. + 3 of a lane are consecutive (split plans have N % 64 == 0)
    const int n4 = n0 + 4 * g;
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int m = t * 16 + r;
      if (m < a.M && n4 < a.N) wt_store4(rs, s * plane + (size_t)m * a.N + n4, acc[t]);
    }
    if (!last_arrival(a.cnt + nb, a.splits)) return;
    // fixed order s = 0, 1, ...; the loads of SB splits of every row tile are issued before their adds (round trips, not
    // bandwidth, bound this)
    constexpr int SB = MT == 1 ? 16 : 8;
    f32x4 sum[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) sum[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int s0 = 0; s0 < a.splits; s0 += SB) {
      f32x4 u[MT][SB];
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        const int m = min(t * 16 + r, a.M - 1);
#pragma unroll
        for (int e = 0; e < SB; ++e) u[t][e] = wt_load4(rs, min(s0 + e, a.splits - 1) * plane + (size_t)m * a.N + min(n4, a.N - 4));
      }
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int e = 0; e < SB; ++e) if (s0 + e < a.splits) sum[t] += u[t][e];
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = sum[t];
  }
  if (a.epi == EPI_PICK) {
    __shared__ float sv[4][64];
    __shared__ int si[4][64];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int m = t * 16 + r;
      float bv = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int n = n0 + 4 * g + i;
        if (m < a.M && n < a.N) {
          if (a.yf) a.yf[(size_t)m * a.ldyf + n] = acc[t][i];
          pick_merge(bv, bi, acc[t][i], n);
        }
      }
#pragma unroll
      for (int d = 16; d <= 32; d <<= 1) {
        const float ov = __shfl_xor(bv, d); const int oi = __shfl_xor(bi, d);
        pick_merge(bv, bi, ov, oi);
      }
      if (g == 0) { sv[wv][t * 16 + r] = bv; si[wv][t * 16 + r] = bi; }
    }
    __syncthreads();
    if ((int)threadIdx.x < a.M) {
      const int m = threadIdx.x;
      float bv = sv[0][m]; int bi = si[0][m];
      for (int w = 1; w < 4; ++w) pick_merge(bv, bi, sv[w][m], si[w][m]);
      wt_store(wt_rsrc(a.pv, (size_t)a.M * gridDim.x * 4), (size_t)m * gridDim.x + nb, bv);
      wt_store_i(wt_rsrc(a.pi, (size_t)a.M * gridDim.x * 4), (size_t)m * gridDim.x + nb, bi);
    }
    if (!last_arrival(a.cnt + gridDim.x, gridDim.x)) return;
    int* st = const_cast<int*>(a.state);
    const int pos = st[ST_POS];
    const __amdgpu_buffer_rsrc_t rv = wt_rsrc(a.pv, (size_t)a.M * gridDim.x * 4), ri = wt_rsrc(a.pi, (size_t)a.M * gridDim.x * 4);
    const int nbk = gridDim.x;
    __shared__ int s_best[64];
    // two rows per wave at a time, every load of both in flight together; the order of the merges does not matter (the
    // greedy order is total)
    for (int m0 = wv; m0 < a.M; m0 += 8) {
      const int m1 = min(m0 + 4, a.M - 1);
      float bv0 = -INFINITY, bv1 = -INFINITY; int bi0 = 0x7fffffff, bi1 = 0x7fffffff;
      for (int c0 = 0; c0 < nbk; c0 += 16 * 64) {
        float pv0[16], pv1[16]; int pi0[16], pi1[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int c = min(c0 + e * 64 + lane, nbk - 1);
          pv0[e] = wt_load(rv, (size_t)m0 * nbk + c); pi0[e] = wt_load_i(ri, (size_t)m0 * nbk + c);
          pv1[e] = wt_load(rv, (size_t)m1 * nbk + c); pi1[e] = wt_load_i(ri, (size_t)m1 * nbk + c);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) { pick_merge(bv0, bi0, pv0[e], pi0[e]); pick_merge(bv1, bi1, pv1[e], pi1[e]); }
      }
#pragma unroll
      for (int d = 1; d <= 32; d <<= 1) {
        const float ov0 = __shfl_xor(bv0, d); const int oi0 = __shfl_xor(bi0, d);
        const float ov1 = __shfl_xor(bv1, d); const int oi1 = __shfl_xor(bi1, d);
        pick_merge(bv0, bi0, ov0, oi0); pick_merge(bv1, bi1, ov1, oi1);
      }
      if (lane == 0) { s_best[m0] = bi0; if (m0 + 4 < a.M) s_best[m0 + 4] = bi1; }
    }
    __syncthreads();
    if ((int)threadIdx.x < a.M) {
      const int m = threadIdx.x;
      int bi = s_best[m];
      if (bi < 0 || bi >= a.N) bi = 0;                           // (all logits NaN: keep the id in range)
      const int fin = st[ST_FIN + m];
      const int tok = fin ? a.pad : bi;                          // a finished row emits pad_token_id
      if (pos + 1 < a.max_len) a.ids[(size_t)m * a.max_len + pos + 1] = tok;
      st[ST_TOK + m] = tok;
      if (a.eos >= 0 && tok == a.eos) st[ST_FIN + m] = 1;
    }
    __syncthreads();
    __threadfence_block();
    if (threadIdx.x == 0) {
      int all = 1;
      for (int m = 0; m < a.M; ++m) all &= (st[ST_FIN + m] != 0);
      if (all && st[ST_DONE] == 0) { st[ST_DONE] = 1; st[ST_STOP] = pos + 2; }
      st[ST_POS] = pos + 1;
    }
    return;
  }
  if (a.epi == EPI_BEAM) {
    // fp32 logits, and per (row, 64-feature block) the block maximum and sum exp(x - max): the row's log-sum-exp follows from
    // the partials in block order (beam_row_lse), without a second pass over the weights
    __shared__ float bm_s[4][64], bs_s[4][64];
    float bmx[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int m = t * 16 + r;
      float mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int n = n0 + 4 * g + i;
        if (m < a.M && n < a.N) { a.yf[(size_t)m * a.ldyf + n] = acc[t][i]; mx = fmaxf(mx, acc[t][i]); }
      }
      mx = fmaxf(mx, __shfl_xor(mx, 16)); mx = fmaxf(mx, __shfl_xor(mx, 32));
      if (g == 0) bm_s[wv][t * 16 + r] = mx;
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int m = t * 16 + r;
      bmx[t] = fmaxf(fmaxf(bm_s[0][m], bm_s[1][m]), fmaxf(bm_s[2][m], bm_s[3][m]));
      float sm = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int n = n0 + 4 * g + i;
        if (m < a.M && n < a.N && bmx[t] != -INFINITY) sm += expf(acc[t][i] - bmx[t]);
      }
      sm += __shfl_xor(sm, 16); sm += __shfl_xor(sm, 32);
      if (g == 0) bs_s[wv][m] = sm;
    }
    __syncthreads();
    if ((int)threadIdx.x < a.M) {
      const int m = threadIdx.x;
      const float mx = fmaxf(fmaxf(bm_s[0][m], bm_s[1][m]), fmaxf(bm_s[2][m], bm_s[3][m]));
      const float sm = ((bs_s[0][m] + bs_s[1][m]) + bs_s[2][m]) + bs_s[3][m];
      wt_store(wt_rsrc(a.pv, (size_t)a.M * gridDim.x * 4), (size_t)m * gridDim.x + nb, mx);
      wt_store(wt_rsrc(a.psum, (size_t)a.M * gridDim.x * 4), (size_t)m * gridDim.x + nb, sm);
    }
    return;
  }
  const int pos = a.epi == EPI_QKV ? a.state[ST_POS] : 0;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = t * 16 + r;
    if (m >= a.M) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = n0 + 4 * g + i;
      if (n >= a.N) continue;
      float v = acc[t][i] + (a.bias ? a.bias[n] : 0.f);
      if (a.epi == EPI_STORE) {
        if (a.act == ACT_GELU) v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
        else if (a.act == ACT_RELU) v = fmaxf(v, 0.f);
        v *= a.oscale;
        if (a.yf) a.yf[(size_t)m * a.ldyf + n] = v;
        if (a.yb) a.yb[(size_t)m * a.ldyb + n] = (bf16)v;
      } else if (a.epi == EPI_QKV) {
        if (n < a.D) a.yf[(size_t)m * a.ldyf + n] = v * a.oscale;
        else if (pos < a.max_len) a.kv[(size_t)m * a.kv_bstride + (size_t)pos * 2 * a.D + (n - a.D)] = (bf16)v;
      } else {                                                   // EPI_LN
        wt_store(wt_rsrc(a.pre, (size_t)a.M * a.N * 4), (size_t)m * a.N + n, v + a.res[(size_t)m * a.N + n]);
      }
    }
  }
  if (a.epi == EPI_LN && last_arrival(a.cnt + gridDim.x, gridDim.x))
    rows_layernorm(a.pre, a.M, a.N, a.gamma, a.beta, a.eps, a.yf, a.yb);
}

struct DecAttn {
  const float* q; int ldq;           // [M][ldq], already scaled by head_dim^-0.5
  const bf16* kv; long long bstride; int rstride;   // key j of batch b, head h: kv + b*bstride + j*rstride + h*64; value: + D
  const int* state; int L;           // self-attention: L = min(state[ST_POS] + 1, L); cross-attention (state null): L
  int M, H, D, nch;
  float* part; int* cnt;             // [M][H][nch][66]; [M*H]
  bf16* o; int ldo;
  // beam search: key j < pos of row b lies in physical row src[b * src_ld + j] of the table half (pos & 1) (pos = state[ST_POS];
  // without state pos = L - 1 and the table is the first half), key pos in row b itself; rpi > 0: row b reads the K/V of item
  // b / rpi (cross-attention)
  const unsigned char* src; int src_ld, rpi;
};

__global__ __launch_bounds__(64) void dmx_dec_attn_kernel(DecAttn a) {
  const int lane = threadIdx.x, c = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int L = a.state ? min(a.state[ST_POS] + 1, a.L) : a.L;
  const int j0 = c * 64, nvalid = max(0, min(64, L - j0));
  // physical row of this lane's key
  int prow = a.rpi > 0 ? b / a.rpi : b;
  if (a.src && lane < nvalid) {
    const int pos = a.state ? a.state[ST_POS] : a.L - 1;
    const size_t half = a.state ? (size_t)(pos & 1) * 64 * a.src_ld : 0;
    if (j0 + lane < pos) prow = a.src[half + (size_t)b * a.src_ld + j0 + lane];
  }
  const bf16* kb = a.kv + (size_t)prow * a.bstride + h * 64;
  float s = -INFINITY;
  if (lane < nvalid) {
    const float* q = a.q + (size_t)b * a.ldq + h * 64;
    const bf16* kr = kb + (size_t)(j0 + lane) * a.rstride;
    float dot = 0.f;
#pragma unroll
    for (int d = 0; d < 64; d += 8) {
      float kf[8]; unpack_bf8(*(const u32x4*)(kr + d), kf);
      const f32x4 q0 = *(const f32x4*)(q + d), q1 = *(const f32x4*)(q + d + 4);
      dot += q0[0] * kf[0] + q0[1] * kf[1] + q0[2] * kf[2] + q0[3] * kf[3] + q1[0] * kf[4] + q1[1] * kf[5] + q1[2] * kf[6] + q1[3] * kf[7];
    }
    s = dot;
  }
  const float mx = wave_max(s);
  const float p = lane < nvalid ? expf(s - mx) : 0.f;
  const float l = wave_sum(p);
  // o[d] = sum_j p_j v_j[d]: lane (kg = lane / 8, dg = lane % 8) takes keys kg, kg + 8, ... and dims 8 dg ... 8 dg + 7 with 16-byte
  // loads (all eight issued before the first FMA), then the eight key groups are summed across lanes
  const int kg = lane >> 3, dg = lane & 7;
  float o8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  u32x4 vv[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int jj = u * 8 + kg;
    const int pr = __shfl(prow, jj);
    vv[u] = jj < nvalid ? *(const u32x4*)(a.kv + (size_t)pr * a.bstride + h * 64 + a.D + (size_t)(j0 + jj) * a.rstride + dg * 8)
                        : (u32x4){0u, 0u, 0u, 0u};
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const float pj = __shfl(p, u * 8 + kg);
    float vf[8]; unpack_bf8(vv[u], vf);
#pragma unroll
    for (int e = 0; e < 8; ++e) o8[e] += pj * vf[e];
  }
#pragma unroll
  for (int d = 8; d <= 32; d <<= 1)
#pragma unroll
    for (int e = 0; e < 8; ++e) o8[e] += __shfl_xor(o8[e], d);
  const int bh = b * a.H + h;
  const size_t rec = (size_t)a.M * a.H * a.nch * 66;
  const __amdgpu_buffer_rsrc_t rs = wt_rsrc(a.part, rec * 4);
  const size_t P = ((size_t)bh * a.nch + c) * 66;
  if (lane == 0) { wt_store(rs, P, nvalid ? mx : -INFINITY); wt_store(rs, P + 1, l); }
  if (kg == 0) {
#pragma unroll
    for (int e = 0; e < 8; ++e) wt_store(rs, P + 2 + dg * 8 + e, o8[e]);
  }
  if (!last_arrival(a.cnt + bh, a.nch)) return;
  // chunk order 0, 1, ...; the (m, l, o) of 16 chunks are loaded together
  const size_t Pb = (size_t)bh * a.nch * 66;
  float M = -INFINITY;
  for (int c0 = 0; c0 < a.nch; c0 += 16) {
    float mc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) mc[e] = wt_load(rs, Pb + (size_t)min(c0 + e, a.nch - 1) * 66);
#pragma unroll
    for (int e = 0; e < 16; ++e) M = fmaxf(M, mc[e]);
  }
  float acc = 0.f, den = 0.f;
  for (int c0 = 0; c0 < a.nch; c0 += 16) {
    float mc[16], lc[16], oc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const size_t q = Pb + (size_t)min(c0 + e, a.nch - 1) * 66;
      mc[e] = wt_load(rs, q); lc[e] = wt_load(rs, q + 1); oc[e] = wt_load(rs, q + 2 + lane);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      if (c0 + e >= a.nch) break;
      const float w = mc[e] == -INFINITY ? 0.f : expf(mc[e] - M);
      den += w * lc[e];
      acc += w * oc[e];
    }
  }
  a.o[(size_t)b * a.ldo + h * 64 + lane] = (bf16)(acc / den);
}

// x = LN(embed[tok] * scale + pos_table[pos + 2]) (LN skipped without gamma): one wave per row (dec_embed_row), token and
// position read from the state words
__global__ __launch_bounds__(64) void dmx_dec_embed_kernel(const int* state, const bf16* emb, int V, const float* posw, int npos, float scale,
                                                           const float* gamma, const float* beta, int D, float* yf, bf16* yb) {
  const int lane = threadIdx.x, m = blockIdx.x;
  int tok = state[ST_TOK + m]; tok = min(max(tok, 0), V - 1);
  const int prow = min(state[ST_POS] + 2, npos - 1);
  dec_embed_row(tok, prow, lane, m, emb, posw, scale, gamma, beta, D, yf, yb);
}

// zero the counters / state, every row starts from `start`
__global__ __launch_bounds__(256) void dmx_dec_reset_kernel(int* words, size_t nwords, int B, int start, long long* ids, int max_len) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += (size_t)gridDim.x * blockDim.x)
    words[i] = (i >= ST_TOK && i < (size_t)ST_TOK + B) ? start : 0;
  if (blockIdx.x == 0 && (int)threadIdx.x < B && ids) ids[(size_t)threadIdx.x * max_len] = start;
}
__global__ __launch_bounds__(256) void dmx_i64_to_i32_kernel(const long long* in, int* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = (int)in[i];
}

// ---- beam search: selection + bookkeeping of one step in one launch (transformers' GenerationMixin._beam_search, do_sample=False,
// no logits processors, one eos id, decoder prompt length 1)
struct BeamSel {
  const float* logits; int ldl;      // [M][V] fp32, M = B * nb rows (row = item * nb + beam)
  const float* pmax; const float* psum; int nblk;   // per (row, 64-feature block): max, sum exp(x - max)
  int B, nb, V, K, chunk, C, max_len, eos, early;   // K = 2 nb; early: 0 False, 1 True, 2 "never"
  float lp;                          // length_penalty
  int* state; int* bs;               // the state words; the beam state block
  float* cv; int* ci;                // chunk candidates [M][C][K]: accumulated score, token
  float* logp;                       // nullable [M][V]: the log-probs the selection used
};
__device__ __forceinline__ int* beam_hist(int* bs) { return bs + BS_WORDS; }
__device__ __forceinline__ int* beam_fin_ids(int* bs, int max_len) { return bs + BS_WORDS + (size_t)max_len * 64; }
__device__ __forceinline__ unsigned char* beam_src(int* bs, int max_len) { return (unsigned char*)(bs + BS_WORDS + (size_t)max_len * 128); }

// the K best of s_val[0, n) in the order rule (larger first, equal values -> lower index, NaN never wins), best first, into
// ov / oi (LDS); the index of entry i is s_idx[i], or i.  Winners leave s_val as NaN; a slot nothing could fill holds (NaN, INT_MAX)
__device__ void block_topk(float* s_val, const int* s_idx, int n, int K, float* ov, int* oi) {
  __shared__ float r_v[4];
  __shared__ int r_i[4], r_p[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int it = 0; it < K; ++it) {
    float bv = -INFINITY; int bi = 0x7fffffff, bp = -1;
    for (int i = threadIdx.x; i < n; i += 256) {
      const float v = s_val[i]; const int id = s_idx ? s_idx[i] : i;
      if (pick_better(v, id, bv, bi)) { bv = v; bi = id; bp = i; }
    }
#pragma unroll
    for (int d = 1; d <= 32; d <<= 1) {
      const float xv = __shfl_xor(bv, d); const int xi = __shfl_xor(bi, d), xp = __shfl_xor(bp, d);
      if (pick_better(xv, xi, bv, bi)) { bv = xv; bi = xi; bp = xp; }
    }
    if (lane == 0) { r_v[wv] = bv; r_i[wv] = bi; r_p[wv] = bp; }
    __syncthreads();
    bv = r_v[0]; bi = r_i[0]; bp = r_p[0];
    for (int w = 1; w < 4; ++w) if (pick_better(r_v[w], r_i[w], bv, bi)) { bv = r_v[w]; bi = r_i[w]; bp = r_p[w]; }
    if (threadIdx.x == 0) { ov[it] = bp >= 0 ? bv : NAN; oi[it] = bp >= 0 ? bi : 0x7fffffff; }
    if (bp >= 0 && (bp & 255) == (int)threadIdx.x) s_val[bp] = NAN;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void dmx_dec_beam_select_kernel(BeamSel a) {
  __shared__ float s_buf[kBeamLds];
  __shared__ float s_tv[kBeamMaxK], s_cand[kBeamMaxK], s_pen[kBeamMaxK], s_mv[kBeamMaxK + 16], s_nsc[16], s_red[4];
  __shared__ int s_ti[kBeamMaxK], s_par[kBeamMaxK], s_tok[kBeamMaxK], s_hit[kBeamMaxK], s_mf[kBeamMaxK + 16];
  __shared__ int s_newpar[16], s_fsrc[16], s_nfl[16], s_nln[16], s_oln[16];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = blockIdx.x, m = blockIdx.y, nb = a.nb, b = m / nb, V = a.V, K = a.K;
  int* st = a.state; int* bs = a.bs;
  if (st[ST_DONE]) {                                             // the search has ended: later replays change nothing
    if (c == 0 && m == 0 && tid == 0) bs[BS_STEPS] += 1;
    return;
  }
  const int pos = st[ST_POS], cur = pos + 1;                     // cur: tokens so far
  // the row's log-sum-exp from the LM head's block partials, in block order
  const float* pm = a.pmax + (size_t)m * a.nblk; const float* ps = a.psum + (size_t)m * a.nblk;
  float mx = -INFINITY;
  for (int i = tid; i < a.nblk; i += 256) mx = fmaxf(mx, pm[i]);
  mx = wave_max(mx);
  if (lane == 0) s_red[wv] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
  __syncthreads();
  float sm = 0.f;
  for (int i = tid; i < a.nblk; i += 256) { const float v = pm[i]; sm += v == -INFINITY ? 0.f : ps[i] * expf(v - mx); }
  sm = wave_sum(sm);
  if (lane == 0) s_red[wv] = sm;
  __syncthreads();
  const float lse = mx + logf(((s_red[0] + s_red[1]) + s_red[2]) + s_red[3]);
  // this chunk's accumulated scores: running score + (logit - lse), one fp32 add
  const float rs = ((const float*)bs)[BS_RUN + m];
  const int n0 = c * a.chunk, n = max(0, min(a.chunk, V - n0));
  for (int i = tid; i < n; i += 256) {
    const float lpv = a.logits[(size_t)m * a.ldl + n0 + i] - lse;
    if (a.logp) a.logp[(size_t)m * V + n0 + i] = lpv;
    s_buf[i] = lpv + rs;
  }
  __syncthreads();
  block_topk(s_buf, nullptr, n, K, s_tv, s_ti);
  const size_t ncand = (size_t)a.B * nb * a.C * K;
  const __amdgpu_buffer_rsrc_t rcv = wt_rsrc(a.cv, ncand * 4), rci = wt_rsrc(a.ci, ncand * 4);
  if (tid < K) {
    const size_t q = ((size_t)m * a.C + c) * K + tid;
    wt_store(rcv, q, s_tv[tid]);
    wt_store_i(rci, q, s_ti[tid] == 0x7fffffff ? 0x7fffffff : n0 + s_ti[tid]);
  }
  if (!last_arrival(bs + BS_CNT + b, nb * a.C)) return;

  // ---- the item's last block: merge nb x C sorted lists, then the step's bookkeeping
  const int ne = nb * a.C * K;
  float* e_v = s_buf; int* e_i = (int*)(s_buf + kBeamEntries);
  for (int i = tid; i < ne; i += 256) {
    const size_t q = (size_t)b * ne + i;
    const float v = wt_load(rcv, q); const int id = wt_load_i(rci, q);
    const bool ok = id != 0x7fffffff;
    e_v[i] = ok ? v : NAN; e_i[i] = ok ? (i / (a.C * K)) * V + id : 0x7fffffff;
  }
  __syncthreads();
  block_topk(e_v, e_i, ne, K, s_tv, s_ti);
  float* rsv = (float*)bs + BS_RUN + b * nb; float* fsc = (float*)bs + BS_FSC + b * nb;
  int* ffl = bs + BS_FFLAG + b * nb; int* fln = bs + BS_FLEN + b * nb;
  int* hist = beam_hist(bs); int* fin = beam_fin_ids(bs, a.max_len);
  const unsigned char* told = beam_src(bs, a.max_len) + (size_t)(pos & 1) * 64 * a.max_len;
  unsigned char* tnew = beam_src(bs, a.max_len) + (size_t)((pos + 1) & 1) * 64 * a.max_len;
  if (tid == 0) {
    int allhit = 1;
    for (int i = 0; i < K; ++i) {
      float v = s_tv[i]; int fl = s_ti[i];
      if (fl == 0x7fffffff || fl < 0) { v = -INFINITY; fl = 0; }   // (only with NaN logits: keep the ids in range)
      const int tk = fl % V;
      const int hit = (tk == a.eos) || (cur + 1 >= a.max_len);
      s_cand[i] = v; s_par[i] = fl / V; s_tok[i] = tk; s_hit[i] = hit; allhit &= hit;
      s_pen[i] = hit ? v + -1.0e9f : v;
    }
    // the next running beams: top nb of the penalised candidates
    unsigned taken = 0;
    for (int r = 0; r < nb; ++r) {
      float bv = -INFINITY; int bi = 0x7fffffff;
      for (int i = 0; i < K; ++i) if (!((taken >> i) & 1)) pick_merge(bv, bi, s_pen[i], i);
      if (bi == 0x7fffffff) for (int i = K - 1; i >= 0; --i) if (!((taken >> i) & 1)) bi = i;
      taken |= 1u << bi;
      const int row = b * nb + r, prow = b * nb + s_par[bi];
      rsv[r] = s_pen[bi]; bs[BS_PARENT + row] = prow; s_newpar[r] = prow; st[ST_TOK + row] = s_tok[bi];
      if (cur < a.max_len) hist[(size_t)cur * 64 + row] = s_tok[bi];
    }
    // the finished set: [nb finished | K candidates] -> top nb
    const float div = (float)pow((double)cur, (double)a.lp);
    int full = 1;
    for (int j = 0; j < nb; ++j) { full &= (ffl[j] != 0); s_mv[j] = fsc[j]; s_mf[j] = ffl[j]; s_oln[j] = fln[j]; }
    const int impr = bs[BS_IMPR + b];
    for (int i = 0; i < K; ++i) {
      float sc = s_cand[i] / div;
      if (full && a.early == 1) sc += -1.0e9f;
      if (!impr) sc += -1.0e9f;
      const int fini = s_hit[i] && i < nb;
      if (!fini) sc += -1.0e9f;
      s_mv[nb + i] = sc; s_mf[nb + i] = fini;
    }
    unsigned long long tk2 = 0;
    for (int j = 0; j < nb; ++j) {
      float bv = -INFINITY; int bi = 0x7fffffff;
      for (int i = 0; i < nb + K; ++i) if (!((tk2 >> i) & 1)) pick_merge(bv, bi, s_mv[i], i);
      if (bi == 0x7fffffff) for (int i = nb + K - 1; i >= 0; --i) if (!((tk2 >> i) & 1)) bi = i;
      tk2 |= 1ull << bi;
      s_fsrc[j] = bi; s_nsc[j] = s_mv[bi]; s_nfl[j] = s_mf[bi]; s_nln[j] = bi < nb ? s_oln[bi] : cur;
    }
    float mn = INFINITY; int full2 = 1;
    for (int j = 0; j < nb; ++j) { fsc[j] = s_nsc[j]; ffl[j] = s_nfl[j]; mn = fminf(mn, s_nsc[j]); full2 &= (s_nfl[j] != 0); }
    // can the running beams still improve on the finished ones?
    const int hl = (a.early == 2 && a.lp > 0.f) ? a.max_len - 1 : cur;
    const float best = rsv[0] / (float)pow((double)hl, (double)a.lp);
    int any = 0;
    for (int j = 0; j < nb; ++j) any |= best > (s_nfl[j] ? mn : -1.0e9f);
    const __amdgpu_buffer_rsrc_t rb = wt_rsrc(bs, (size_t)BS_WORDS * 4);
    wt_store_i(rb, BS_IMPR + b, impr && any); wt_store_i(rb, BS_FULL + b, full2); wt_store_i(rb, BS_HIT + b, allhit);
  }
  __syncthreads();
  // ancestry of the new rows: the parent's row of every earlier position, then the parent itself (the other half of the table)
  for (int i = tid; i < nb * cur; i += 256) {
    const int r = i / cur, j = i % cur, p = s_newpar[r];
    tnew[(size_t)(b * nb + r) * a.max_len + j] = j < pos ? told[(size_t)p * a.max_len + j] : (unsigned char)p;
  }
  // finished ids, in place: an old slot only moves down, so the slots are filled from the last one up
  for (int j = nb - 1; j >= 0; --j) {
    const int mi = s_fsrc[j];
    int* dst = fin + (size_t)(b * nb + j) * a.max_len;
    if (mi < nb) {
      if (mi != j) {
        const int* src = fin + (size_t)(b * nb + mi) * a.max_len;
        for (int i = tid; i <= min(s_oln[mi], a.max_len - 1); i += 256) dst[i] = src[i];
      }
    } else {
      const int p = b * nb + s_par[mi - nb];
      for (int i = tid; i <= pos; i += 256) dst[i] = hist[(size_t)i * 64 + (i < pos ? told[(size_t)p * a.max_len + i] : p)];
      if (tid == 0 && cur < a.max_len) dst[cur] = s_tok[mi - nb];
    }
    __syncthreads();
  }
  if (tid < nb) fln[tid] = s_nln[tid];
  if (!last_arrival(bs + BS_CNT + 64, a.B)) return;
  if (tid == 0) {                                               // the whole batch's loop condition
    const __amdgpu_buffer_rsrc_t rb = wt_rsrc(bs, (size_t)BS_WORDS * 4);
    int any_impr = 0, all_full = 1, all_hit = 1;
    for (int i = 0; i < a.B; ++i) {
      any_impr |= wt_load_i(rb, BS_IMPR + i); all_full &= wt_load_i(rb, BS_FULL + i); all_hit &= wt_load_i(rb, BS_HIT + i);
    }
    const int go = any_impr && !(all_full && a.early == 1) && !all_hit;
    if (!go) { st[ST_DONE] = 1; st[ST_STOP] = cur + 1; }
    st[ST_POS] = pos + 1;
    bs[BS_STEPS] += 1;
  }
}

// per (row, 64-feature block) maximum and sum exp(x - max) of supplied logits (the op entry; the decoder's LM head writes them itself)
__global__ __launch_bounds__(64) void dmx_dec_beam_partials_kernel(const float* logits, int ldl, int V, int nblk, float* pmax, float* psum) {
  const int lane = threadIdx.x, blk = blockIdx.x, m = blockIdx.y, n = blk * 64 + lane;
  const float x = n < V ? logits[(size_t)m * ldl + n] : -INFINITY;
  const float mx = wave_max(x);
  const float e = (n < V && mx != -INFINITY) ? expf(x - mx) : 0.f;
  const float sm = wave_sum(e);
  if (lane == 0) { pmax[(size_t)m * nblk + blk] = mx; psum[(size_t)m * nblk + blk] = sm; }
}

// cache words zeroed with every row's input = start; beam state: running scores [0, -1e9, ...], finished scores -1e9, every
// item improvable, position 0 of the history and of every finished slot = start
__global__ __launch_bounds__(256) void dmx_dec_beam_reset_kernel(int* words, size_t nwords, int M, int nb, int start, int* bs, size_t bwords, int max_len) {
  const size_t stride = (size_t)gridDim.x * blockDim.x, i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = i0; i < nwords; i += stride) words[i] = (i >= ST_TOK && i < (size_t)ST_TOK + M) ? start : 0;
  const size_t fin0 = (size_t)BS_WORDS + (size_t)max_len * 64, fin1 = fin0 + (size_t)max_len * 64;
  for (size_t i = i0; i < bwords; i += stride) {
    int v = 0;
    if (i < (size_t)BS_RUN + 64) v = (int)__float_as_uint((i - BS_RUN) % nb == 0 ? 0.f : -1.0e9f);
    else if (i < (size_t)BS_FSC + 64) v = (int)__float_as_uint(-1.0e9f);
    else if (i >= BS_IMPR && i < (size_t)BS_IMPR + 64) v = 1;
    else if (i >= BS_WORDS && i < (size_t)BS_WORDS + 64) v = start;
    else if (i >= fin0 && i < fin1 && (i - fin0) % max_len == 0) v = start;
    bs[i] = v;
  }
}
// the first nret finished slots of every item: ids (pad beyond the hypothesis), score, generated length
__global__ __launch_bounds__(64) void dmx_dec_beam_gather_kernel(int* bs, int nb, int nret, int max_len, int pad, long long* seq, float* scores, int* lens) {
  const int o = blockIdx.x, b = o / nret, slot = b * nb + o % nret;
  const int len = min(bs[BS_FLEN + slot], max_len - 1);
  const int* fin = beam_fin_ids(bs, max_len) + (size_t)slot * max_len;
  for (int i = threadIdx.x; i < max_len; i += 64) seq[(size_t)o * max_len + i] = i <= len ? fin[i] : pad;
  if (threadIdx.x == 0) { scores[o] = ((const float*)bs)[BS_FSC + slot]; lens[o] = len; }
}

int dec_linear_launch(const DecLin& a, hipStream_t stream) {
  const int nblk = cdiv(a.N, 64);
  DMX_REQUIRE(a.M >= 1 && a.M <= 64 && a.K % 128 == 0 && a.kchunk % 128 == 0 && a.ldw % 8 == 0 && a.ldx % 8 == 0,
              "dec_linear: M=%d K=%d kchunk=%d", a.M, a.K, a.kchunk);
  DMX_REQUIRE(a.splits == cdiv(a.K, a.kchunk), "dec_linear: splits %d != K / kchunk", a.splits);
  DMX_REQUIRE((a.epi != EPI_PICK && a.epi != EPI_BEAM) || a.splits == 1, "dec_linear: the pick / beam epilogues run unsplit");
  DMX_REQUIRE(a.splits == 1 || a.N % 4 == 0, "dec_linear: a split plan needs N %% 4 == 0 (16-byte partial runs)");
  DMX_REQUIRE(a.epi != EPI_LN || (a.N % 256 == 0 && a.N <= 1024), "dec_linear: LayerNorm epilogue needs N %% 256 == 0, N <= 1024");
  const dim3 grid(nblk, a.splits);
  switch ((a.M + 15) / 16) {
    case 1: hipLaunchKernelGGL(dmx_dec_linear_kernel<1>, grid, dim3(256), 0, stream, a); break;
    case 2: hipLaunchKernelGGL(dmx_dec_linear_kernel<2>, grid, dim3(256), 0, stream, a); break;
    case 3: hipLaunchKernelGGL(dmx_dec_linear_kernel<3>, grid, dim3(256), 0, stream, a); break;
    default: hipLaunchKernelGGL(dmx_dec_linear_kernel<4>, grid, dim3(256), 0, stream, a); break;
  }
  return dmx_check_launch("dmx_dec_linear_kernel");
}
}  // namespace

namespace {
constexpr int kLaunchesPerLayer = 8;

// split-K plan of one weight-streaming linear: enough blocks to cover the CUs several times over, partials bounded at large M
int plan_kchunk(int N, int K, int M, int epi) {
  if (epi == EPI_PICK || epi == EPI_BEAM) return K;
  const int nblk = cdiv(N, 64);
  int sp = std::min(K / 128, std::max(1, 1024 / nblk));
  sp = std::max(1, std::min(sp, std::max(2, 256 / M)));
  return (int)align_up((size_t)cdiv(K, sp), 128);
}
size_t lin_part_floats(int N, int K, int M, int epi) {
  const int kc = plan_kchunk(N, K, M, epi), sp = cdiv(K, kc);
  return sp > 1 ? (size_t)sp * M * N : 0;
}
}  // namespace

namespace {
struct DecLayout {                   // byte offsets in the cache / workspace
  size_t words, kv, ckv, cache_total;
  size_t xf, xb, qf, ab, hb, pre, part, apart, pv, pi, encb, gemm_ws, step_total, ws_total;
  int nch_self, nch_cross, lm_blocks;
};
DecLayout dec_layout(const dmx_trocr_dec* d, int B, int S, int max_len) {
  const dmx_trocr_dec_config& c = d->cfg;
  const int D = c.d_model, F = c.ffn_dim, L = c.num_layers, H = D / 64, V = c.vocab_size;
  DecLayout y{};
  const int nslices = kLaunchesPerLayer * L + 1;
  y.words = 0;
  y.kv = align_up(((size_t)ST_INTS + (size_t)nslices * d->cnt_slice) * 4, 256);
  y.ckv = y.kv + align_up((size_t)L * B * max_len * 2 * D * 2, 256);
  y.cache_total = y.ckv + align_up((size_t)B * S * L * 2 * D * 2, 256);
  y.nch_self = cdiv(max_len, 64); y.nch_cross = cdiv(S, 64); y.lm_blocks = cdiv(V, 64);
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t r = o; o += align_up(bytes, 256); return r; };
  y.xf = take((size_t)B * D * 4); y.xb = take((size_t)B * D * 2); y.qf = take((size_t)B * D * 4); y.ab = take((size_t)B * D * 2);
  y.hb = take((size_t)B * F * 2); y.pre = take((size_t)B * D * 4);
  size_t pf = 0;
  pf = std::max(pf, lin_part_floats(3 * D, D, B, EPI_QKV));
  pf = std::max(pf, lin_part_floats(D, D, B, EPI_LN));
  pf = std::max(pf, lin_part_floats(D, D, B, EPI_STORE));
  pf = std::max(pf, lin_part_floats(F, D, B, EPI_STORE));
  pf = std::max(pf, lin_part_floats(D, F, B, EPI_LN));
  y.part = take(pf * 4 + 4);
  y.apart = take((size_t)B * H * std::max(y.nch_self, y.nch_cross) * 66 * 4);
  y.pv = take((size_t)B * y.lm_blocks * 4); y.pi = take((size_t)B * y.lm_blocks * 4);
  y.step_total = o;
  // cross K/V (dmx_trocr_dec_cross_kv, before the steps): the bf16 encoder states and the GEMM's own workspace, from offset 0
  o = 0;
  y.encb = take((size_t)B * S * d->kdim * 2);
  y.gemm_ws = o;
  Exec ex = Exec::dry_run();
  ex.gemm_raw(nullptr, d->kdim, B * S, nullptr, d->kdim, 2 * L * D, d->kdim, nullptr, nullptr, 2 * L * D, 0);
  y.ws_total = std::max(y.step_total, y.gemm_ws + ex.ws.peak() + 4096);
  return y;
}

// cross K/V of every layer, once per image: the encoder states as bf16 (encb), then one GEMM at B * S rows
int cross_kv_launch(const dmx_trocr_dec* d, const float* enc, int B, int S, bf16* encb, char* gemm_ws, size_t gemm_ws_bytes, void* ckv_out,
                    hipStream_t stream) {
  const int rc = dmx_cast_f32_to_bf16_launch(enc, encb, (size_t)B * S * d->kdim, stream);
  if (rc) return rc;
  Exec ex = Exec::on(stream, gemm_ws, gemm_ws_bytes);
  const int N = 2 * d->cfg.num_layers * d->cfg.d_model;
  ex.gemm_raw(encb, d->kdim, B * S, d->at<bf16>(d->wckv), d->kdim, N, d->kdim, d->at<float>(d->bckv), ckv_out, N, 0);
  return ex.rc;
}

int dec_attn_launch(const DecAttn& a0, int M, hipStream_t stream) {
  DecAttn a = a0; a.M = M;
  hipLaunchKernelGGL(dmx_dec_attn_kernel, dim3(a.nch, a.H, M), dim3(64), 0, stream, a);
  return dmx_check_launch("dmx_dec_attn_kernel");
}

DecLin lin_base(const bf16* x, int M, int K, const bf16* w, int N, const float* bias, int epi, int* cnt, float* part) {
  DecLin a{};
  a.x = x; a.ldx = K; a.w = w; a.ldw = K; a.bias = bias; a.M = M; a.N = N; a.K = K; a.epi = epi; a.cnt = cnt; a.part = part;
  a.kchunk = plan_kchunk(N, K, M, epi); a.splits = cdiv(K, a.kchunk); a.oscale = 1.f; a.eps = 1e-5f; a.eos = -1;
  return a;
}

const unsigned char* beam_src_host(const int* bs, int max_len) { return (const unsigned char*)(bs + BS_WORDS + (size_t)max_len * 128); }
// beam search (null: greedy): the B rows of the step are nb beams of B / nb items
struct BeamStep { int nb, early; float lp; float* logp; };
struct BeamLayout { DecLayout y; size_t bstate, cache_total, logits, cv, ci, ws_total; int K, chunk, C; };
size_t beam_state_bytes(int max_len) { return ((size_t)BS_WORDS + (size_t)max_len * 160) * 4; }
// selection plan: 2048-value chunks, grown until the nb x C x K candidates of an item fit the merge's LDS
int beam_chunk(int V, int nb) {
  for (int ch = 2048; ch <= kBeamLds; ch += 2048) if ((size_t)nb * cdiv(V, ch) * 2 * nb <= (size_t)kBeamEntries) return ch;
  return 0;
}
BeamLayout beam_layout(const dmx_trocr_dec* d, int B, int nb, int S, int max_len) {
  const dmx_trocr_dec_config& c = d->cfg;
  const int M = B * nb;
  BeamLayout z{};
  z.y = dec_layout(d, M, S, max_len);                            // M rows everywhere but the cross K/V, which is per item
  z.bstate = z.y.ckv + align_up((size_t)B * S * c.num_layers * 2 * c.d_model * 2, 256);
  z.cache_total = z.bstate + align_up(beam_state_bytes(max_len), 256);
  z.K = 2 * nb; z.chunk = beam_chunk(c.vocab_size, nb); z.C = z.chunk ? cdiv(c.vocab_size, z.chunk) : 0;
  size_t o = align_up(z.y.ws_total, 256);
  auto take = [&](size_t bytes) { const size_t r = o; o += align_up(bytes, 256); return r; };
  z.logits = take((size_t)M * c.vocab_size * 4);
  z.cv = take((size_t)M * z.C * z.K * 4); z.ci = take((size_t)M * z.C * z.K * 4);
  z.ws_total = o;
  return z;
}
int beam_select_launch(const BeamSel& a, hipStream_t st) {
  DMX_REQUIRE(a.nb >= 2 && a.nb <= 16 && a.B >= 1 && a.B * a.nb <= 64 && a.K == 2 * a.nb && a.V >= a.K, "beam_select: B=%d beams=%d V=%d", a.B, a.nb, a.V);
  DMX_REQUIRE(a.chunk > 0 && a.chunk <= kBeamLds && a.C == cdiv(a.V, a.chunk) && (size_t)a.nb * a.C * a.K <= (size_t)kBeamEntries,
              "beam_select: vocabulary %d too large for %d beams", a.V, a.nb);
  DMX_REQUIRE(a.max_len >= 2, "beam_select: max_len %d", a.max_len);
  hipLaunchKernelGGL(dmx_dec_beam_select_kernel, dim3(a.C, a.B * a.nb), dim3(256), 0, st, a);
  return dmx_check_launch("dmx_dec_beam_select_kernel");
}

int dec_step(dmx_trocr_dec* d, char* cache, int B, int S, int max_len, int eos, int pad, long long* ids, float* logits, int ldl,
             char* ws, size_t ws_bytes, hipStream_t st, const BeamStep* bm = nullptr) {
  const dmx_trocr_dec_config& c = d->cfg;
  const int D = c.d_model, F = c.ffn_dim, L = c.num_layers, H = D / 64, V = c.vocab_size;
  BeamLayout z{};
  if (bm) z = beam_layout(d, B / bm->nb, bm->nb, S, max_len);
  const DecLayout y = bm ? z.y : dec_layout(d, B, S, max_len);
  DMX_REQUIRE(ws_bytes >= (bm ? z.ws_total : y.ws_total), "trocr_dec_step: workspace %zu < %zu bytes", ws_bytes, bm ? z.ws_total : y.ws_total);
  int* bstate = bm ? (int*)(cache + z.bstate) : nullptr;
  int* state = (int*)(cache + y.words);
  int* cnt = state + ST_INTS;
  int slice = 0;
  auto next_cnt = [&]() { return cnt + (size_t)(slice++) * d->cnt_slice; };
  float* xf = (float*)(ws + y.xf); bf16* xb = (bf16*)(ws + y.xb); float* qf = (float*)(ws + y.qf); bf16* ab = (bf16*)(ws + y.ab);
  bf16* hb = (bf16*)(ws + y.hb); float* pre = (float*)(ws + y.pre); float* part = (float*)(ws + y.part); float* apart = (float*)(ws + y.apart);
  bf16* kv = (bf16*)(cache + y.kv); const bf16* ckv = (const bf16*)(cache + y.ckv);
  const float qscale = 0.125f;                                   // head_dim ** -0.5, head_dim = 64
  const float escale = c.scale_embedding ? sqrtf((float)D) : 1.0f;
  hipLaunchKernelGGL(dmx_dec_embed_kernel, dim3(B), dim3(64), 0, st, state, d->at<bf16>(d->emb), V, d->at<float>(d->posw), d->npos, escale,
                     c.layernorm_embedding ? d->at<float>(d->leg) : nullptr, c.layernorm_embedding ? d->at<float>(d->leb) : nullptr, D, xf, xb);
  int rc = dmx_check_launch("dmx_dec_embed_kernel");
  const int act = c.activation == 1 ? ACT_RELU : ACT_GELU;
  // x = LN(x + in w^T + bias): the residual stream xf / xb rewritten in place by the linear's LayerNorm epilogue
  auto ln_linear = [&](const bf16* in, int K, size_t w, size_t bias, size_t gamma, size_t beta) {
    DecLin a = lin_base(in, B, K, d->at<bf16>(w), D, d->at<float>(bias), EPI_LN, next_cnt(), part);
    a.res = xf; a.pre = pre; a.gamma = d->at<float>(gamma); a.beta = d->at<float>(beta); a.yf = xf; a.yb = xb;
    return dec_linear_launch(a, st);
  };
  for (int l = 0; l < L && !rc; ++l) {
    const DecLayer& W = d->layers[l];
    bf16* kvl = kv + (size_t)l * B * max_len * 2 * D;
    DecLin a = lin_base(xb, B, D, d->at<bf16>(W.wqkv), 3 * D, d->at<float>(W.bqkv), EPI_QKV, next_cnt(), part);
    a.oscale = qscale; a.yf = qf; a.ldyf = D; a.kv = kvl; a.kv_bstride = (long long)max_len * 2 * D; a.state = state; a.D = D; a.max_len = max_len;
    if ((rc = dec_linear_launch(a, st))) break;
    DecAttn t{};
    t.q = qf; t.ldq = D; t.kv = kvl; t.bstride = (long long)max_len * 2 * D; t.rstride = 2 * D; t.state = state; t.L = max_len; t.H = H; t.D = D;
    t.nch = y.nch_self; t.part = apart; t.cnt = next_cnt(); t.o = ab; t.ldo = D;
    if (bm) { t.src = beam_src_host(bstate, max_len); t.src_ld = max_len; }
    if ((rc = dec_attn_launch(t, B, st))) break;
    if ((rc = ln_linear(ab, D, W.wo, W.bo, W.l1g, W.l1b))) break;
    a = lin_base(xb, B, D, d->at<bf16>(W.wcq), D, d->at<float>(W.bcq), EPI_STORE, next_cnt(), part);
    a.oscale = qscale; a.yf = qf; a.ldyf = D;
    if ((rc = dec_linear_launch(a, st))) break;
    t.kv = ckv + (size_t)l * 2 * D; t.bstride = (long long)S * L * 2 * D; t.rstride = L * 2 * D; t.state = nullptr; t.L = S;
    t.nch = y.nch_cross; t.cnt = next_cnt(); t.src = nullptr; t.rpi = bm ? bm->nb : 0;
    if ((rc = dec_attn_launch(t, B, st))) break;
    if ((rc = ln_linear(ab, D, W.wco, W.bco, W.l2g, W.l2b))) break;
    a = lin_base(xb, B, D, d->at<bf16>(W.w1), F, d->at<float>(W.b1), EPI_STORE, next_cnt(), part);
    a.act = act; a.yb = hb; a.ldyb = F;
    if ((rc = dec_linear_launch(a, st))) break;
    if ((rc = ln_linear(hb, F, W.w2, W.b2, W.l3g, W.l3b))) break;
  }
  if (rc) return rc;
  if (bm) {
    // LM head: fp32 logits + block partials of the log-sum-exp, then selection and bookkeeping in one launch
    DecLin a = lin_base(xb, B, D, d->at<bf16>(d->lm), V, nullptr, EPI_BEAM, next_cnt(), part);
    a.yf = (float*)(ws + z.logits); a.ldyf = V; a.pv = (float*)(ws + y.pv); a.psum = (float*)(ws + y.pi);
    if ((rc = dec_linear_launch(a, st))) return rc;
    BeamSel q{};
    q.logits = a.yf; q.ldl = V; q.pmax = a.pv; q.psum = a.psum; q.nblk = y.lm_blocks; q.B = B / bm->nb; q.nb = bm->nb; q.V = V; q.K = z.K;
    q.chunk = z.chunk; q.C = z.C; q.max_len = max_len; q.eos = eos; q.early = bm->early; q.lp = bm->lp; q.state = state; q.bs = bstate;
    q.cv = (float*)(ws + z.cv); q.ci = (int*)(ws + z.ci); q.logp = bm->logp;
    return beam_select_launch(q, st);
  }
  DecLin a = lin_base(xb, B, D, d->at<bf16>(d->lm), V, nullptr, EPI_PICK, next_cnt(), part);
  a.yf = logits; a.ldyf = ldl; a.pv = (float*)(ws + y.pv); a.pi = (int*)(ws + y.pi); a.ids = ids; a.max_len = max_len;
  a.eos = eos; a.pad = pad; a.state = state;
  return dec_linear_launch(a, st);
}
}  // namespace

extern "C" dmx_trocr_dec* dmx_trocr_dec_create(const dmx_trocr_dec_config* cfg) {
  if (!cfg) { dmx_set_error("trocr_dec_create: null config"); return nullptr; }
  const int D = cfg->d_model, F = cfg->ffn_dim, L = cfg->num_layers, V = cfg->vocab_size;
  const int kdim = cfg->cross_hidden_size > 0 ? cfg->cross_hidden_size : D;
  if (D % 256 != 0 || D > 1024 || cfg->num_heads != D / 64) { dmx_set_error("trocr_dec_create: d_model=%d heads=%d: head dim must be 64, d_model a multiple of 256 and <= 1024", D, cfg->num_heads); return nullptr; }
  if (F % 128 != 0 || kdim % 64 != 0 || L <= 0 || V <= 0 || cfg->max_position_embeddings <= 0) { dmx_set_error("trocr_dec_create: bad ffn_dim / cross size / layers / vocab"); return nullptr; }
  if (cfg->activation != 0 && cfg->activation != 1) { dmx_set_error("trocr_dec_create: activation %d (0 gelu, 1 relu)", cfg->activation); return nullptr; }
  auto d = std::make_unique<dmx_trocr_dec>();
  d->cfg = *cfg; d->kdim = kdim; d->npos = cfg->max_position_embeddings + 2;
  d->cnt_slice = (int)align_up((size_t)std::max(cdiv(std::max(V, std::max(3 * D, F)), 64) + 1, 64 * (D / 64)), 64);
  ParamTable& pt = d->pt;
  const std::string p0 = "model.decoder.";
  d->emb = pt.linear(p0 + "embed_tokens.weight", V, D);
  { PackRule r; r.kind = PackRule::COPY_F32; r.dst = pt.reserve((size_t)d->npos * D * 4); r.rows = d->npos * D; pt.add(p0 + "embed_positions.weight", {d->npos, D}, r); d->posw = r.dst; }
  if (cfg->layernorm_embedding) { d->leg = pt.f32(p0 + "layernorm_embedding.weight", D); d->leb = pt.f32(p0 + "layernorm_embedding.bias", D); }
  d->wckv = pt.reserve((size_t)L * 2 * D * kdim * 2);
  d->bckv = pt.reserve((size_t)L * 2 * D * 4);
  d->layers.resize(L);
  for (int i = 0; i < L; ++i) {
    DecLayer& W = d->layers[i];
    const std::string p = p0 + "layers." + std::to_string(i) + ".";
    W.wqkv = pt.reserve((size_t)3 * D * D * 2); W.bqkv = pt.reserve((size_t)3 * D * 4);
    // transformers' state-dict order: k, v, q; packed q | k | v
    pt.linear_at(p + "self_attn.k_proj.weight", D, D, W.wqkv + (size_t)D * D * 2, D); pt.f32_at(p + "self_attn.k_proj.bias", D, W.bqkv + (size_t)D * 4);
    pt.linear_at(p + "self_attn.v_proj.weight", D, D, W.wqkv + (size_t)2 * D * D * 2, D); pt.f32_at(p + "self_attn.v_proj.bias", D, W.bqkv + (size_t)2 * D * 4);
    pt.linear_at(p + "self_attn.q_proj.weight", D, D, W.wqkv, D); pt.f32_at(p + "self_attn.q_proj.bias", D, W.bqkv);
    W.wo = pt.linear(p + "self_attn.out_proj.weight", D, D); W.bo = pt.f32(p + "self_attn.out_proj.bias", D);
    W.l1g = pt.f32(p + "self_attn_layer_norm.weight", D); W.l1b = pt.f32(p + "self_attn_layer_norm.bias", D);
    // cross k / v of every layer: rows [l][k | v] of one [L * 2D][kdim] matrix (one GEMM per image, dmx_trocr_dec_cross_kv)
    const size_t kr = (size_t)i * 2 * D;
    pt.linear_at(p + "encoder_attn.k_proj.weight", D, kdim, d->wckv + kr * kdim * 2, kdim); pt.f32_at(p + "encoder_attn.k_proj.bias", D, d->bckv + kr * 4);
    pt.linear_at(p + "encoder_attn.v_proj.weight", D, kdim, d->wckv + (kr + D) * kdim * 2, kdim); pt.f32_at(p + "encoder_attn.v_proj.bias", D, d->bckv + (kr + D) * 4);
    W.wcq = pt.linear(p + "encoder_attn.q_proj.weight", D, D); W.bcq = pt.f32(p + "encoder_attn.q_proj.bias", D);
    W.wco = pt.linear(p + "encoder_attn.out_proj.weight", D, D); W.bco = pt.f32(p + "encoder_attn.out_proj.bias", D);
    W.l2g = pt.f32(p + "encoder_attn_layer_norm.weight", D); W.l2b = pt.f32(p + "encoder_attn_layer_norm.bias", D);
    W.w1 = pt.linear(p + "fc1.weight", F, D); W.b1 = pt.f32(p + "fc1.bias", F);
    W.w2 = pt.linear(p + "fc2.weight", D, F); W.b2 = pt.f32(p + "fc2.bias", D);
    W.l3g = pt.f32(p + "final_layer_norm.weight", D); W.l3b = pt.f32(p + "final_layer_norm.bias", D);
  }
  d->lm = cfg->tie_word_embeddings ? d->emb : pt.linear("output_projection.weight", V, D);
  return d.release();
}
DMX_MODEL_ABI(dmx_trocr_dec, trocr_dec)
extern "C" int dmx_trocr_dec_finalize(dmx_trocr_dec* d, dmx_stream_t stream) { return model_finalize(d, "trocr_dec", (hipStream_t)stream); }
extern "C" size_t dmx_trocr_dec_cache_bytes(const dmx_trocr_dec* d, int B, int S, int max_len) {
  return d ? dec_layout(d, B, S, max_len).cache_total : 0;
}
extern "C" size_t dmx_trocr_dec_workspace_bytes(const dmx_trocr_dec* d, int B, int S, int max_len) {
  return d ? dec_layout(d, B, S, max_len).ws_total : 0;
}
extern "C" int dmx_trocr_dec_launches_per_step(const dmx_trocr_dec* d) { return d ? 2 + kLaunchesPerLayer * d->cfg.num_layers : 0; }

extern "C" int dmx_trocr_dec_cross_kv(dmx_trocr_dec* d, const float* enc, int B, int S, int max_len, void* cache, void* ws, size_t ws_bytes,
                                      dmx_stream_t stream) {
  DMX_REQUIRE(d && d->finalized, "trocr_dec_cross_kv: weights not finalized (bind_arena, load_param*, finalize)");
  DMX_REQUIRE(enc && cache && ws && B >= 1 && B <= 64 && S >= 1 && max_len >= 1 && max_len <= d->cfg.max_position_embeddings,
              "trocr_dec_cross_kv: bad argument (B=%d S=%d max_len=%d)", B, S, max_len);
  const DecLayout y = dec_layout(d, B, S, max_len);
  DMX_REQUIRE(ws_bytes >= y.ws_total, "trocr_dec_cross_kv: workspace %zu < %zu bytes", ws_bytes, y.ws_total);
  return cross_kv_launch(d, enc, B, S, (bf16*)((char*)ws + y.encb), (char*)ws + y.gemm_ws, ws_bytes - y.gemm_ws, (char*)cache + y.ckv,
                         (hipStream_t)stream);
}
extern "C" int dmx_trocr_dec_reset(dmx_trocr_dec* d, void* cache, int B, int S, int max_len, int start_token, long long* ids, dmx_stream_t stream) {
  DMX_REQUIRE(d && cache && B >= 1 && B <= 64, "trocr_dec_reset: bad argument");
  const DecLayout y = dec_layout(d, B, S, max_len);
  const size_t nwords = (y.kv - y.words) / 4;
  hipLaunchKernelGGL(dmx_dec_reset_kernel, dim3((unsigned)std::min<size_t>(1024, (nwords + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (int*)((char*)cache + y.words), nwords, B, start_token, ids, max_len);
  return dmx_check_launch("dmx_dec_reset_kernel");
}
extern "C" int dmx_trocr_dec_set_tokens(dmx_trocr_dec* d, void* cache, const long long* tokens, int B, dmx_stream_t stream) {
  DMX_REQUIRE(d && cache && tokens && B >= 1 && B <= 64, "trocr_dec_set_tokens: bad argument");
  hipLaunchKernelGGL(dmx_i64_to_i32_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, tokens, (int*)cache + ST_TOK, B);
  return dmx_check_launch("dmx_i64_to_i32_kernel");
}
extern "C" int dmx_trocr_dec_step(dmx_trocr_dec* d, void* cache, int B, int S, int max_len, int eos_token_id, int pad_token_id,
                                  long long* ids, float* logits, int ld_logits, void* ws, size_t ws_bytes, dmx_stream_t stream) {
  DMX_REQUIRE(d && d->finalized, "trocr_dec_step: weights not finalized (bind_arena, load_param*, finalize)");
  DMX_REQUIRE(cache && ids && ws && B >= 1 && B <= 64 && S >= 1 && max_len >= 1 && max_len <= d->cfg.max_position_embeddings,
              "trocr_dec_step: bad argument (B=%d S=%d max_len=%d)", B, S, max_len);
  DMX_REQUIRE(!logits || ld_logits >= d->cfg.vocab_size, "trocr_dec_step: ld_logits %d < vocab %d", ld_logits, d->cfg.vocab_size);
  return dec_step(d, (char*)cache, B, S, max_len, eos_token_id, pad_token_id, ids, logits, ld_logits, (char*)ws, ws_bytes, (hipStream_t)stream);
}

// ---- beam search: cache = state words | self K/V of B * nb rows | cross K/V of B items | beam state block
static int beam_args_ok(const dmx_trocr_dec* d, int B, int nb, int S, int max_len) {
  return d && B >= 1 && nb >= 2 && nb <= 16 && B * nb <= 64 && S >= 1 && max_len >= 2 && max_len <= d->cfg.max_position_embeddings &&
         d->cfg.vocab_size >= 2 * nb && beam_chunk(d->cfg.vocab_size, nb) > 0;
}
extern "C" size_t dmx_trocr_dec_beam_cache_bytes(const dmx_trocr_dec* d, int B, int nb, int S, int max_len) {
  return beam_args_ok(d, B, nb, S, max_len) ? beam_layout(d, B, nb, S, max_len).cache_total : 0;
}
extern "C" size_t dmx_trocr_dec_beam_workspace_bytes(const dmx_trocr_dec* d, int B, int nb, int S, int max_len) {
  return beam_args_ok(d, B, nb, S, max_len) ? beam_layout(d, B, nb, S, max_len).ws_total : 0;
}
extern "C" size_t dmx_trocr_dec_beam_state_offset(const dmx_trocr_dec* d, int B, int nb, int S, int max_len) {
  return beam_args_ok(d, B, nb, S, max_len) ? beam_layout(d, B, nb, S, max_len).bstate : 0;
}
extern "C" size_t dmx_trocr_dec_beam_state_bytes(int max_len) { return max_len >= 1 ? beam_state_bytes(max_len) : 0; }
extern "C" int dmx_trocr_dec_beam_launches_per_step(const dmx_trocr_dec* d) { return d ? 3 + kLaunchesPerLayer * d->cfg.num_layers : 0; }
extern "C" int dmx_trocr_dec_beam_begin(dmx_trocr_dec* d, const float* enc, int B, int nb, int S, int max_len, int start_token, void* cache,
                                        void* ws, size_t ws_bytes, dmx_stream_t stream) {
  DMX_REQUIRE(d && d->finalized, "trocr_dec_beam_begin: weights not finalized (bind_arena, load_param*, finalize)");
  DMX_REQUIRE(enc && cache && ws && beam_args_ok(d, B, nb, S, max_len), "trocr_dec_beam_begin: bad argument (B=%d beams=%d S=%d max_len=%d)", B, nb, S, max_len);
  const BeamLayout z = beam_layout(d, B, nb, S, max_len);
  DMX_REQUIRE(ws_bytes >= z.ws_total, "trocr_dec_beam_begin: workspace %zu < %zu bytes", ws_bytes, z.ws_total);
  hipStream_t st = (hipStream_t)stream;
  // cross K/V once per item: the GEMM runs at B * S rows
  const int rc = cross_kv_launch(d, enc, B, S, (bf16*)((char*)ws + z.y.encb), (char*)ws + z.y.gemm_ws, ws_bytes - z.y.gemm_ws,
                                 (char*)cache + z.y.ckv, st);
  if (rc) return rc;
  const size_t nwords = (z.y.kv - z.y.words) / 4, bwords = beam_state_bytes(max_len) / 4;
  hipLaunchKernelGGL(dmx_dec_beam_reset_kernel, dim3((unsigned)std::min<size_t>(1024, (std::max(nwords, bwords) + 255) / 256)), dim3(256), 0, st,
                     (int*)((char*)cache + z.y.words), nwords, B * nb, nb, start_token, (int*)((char*)cache + z.bstate), bwords, max_len);
  return dmx_check_launch("dmx_dec_beam_reset_kernel");
}
extern "C" int dmx_trocr_dec_beam_step(dmx_trocr_dec* d, void* cache, int B, int nb, int S, int max_len, int eos_token_id, float length_penalty,
                                       int early_stopping, float* logp, void* ws, size_t ws_bytes, dmx_stream_t stream) {
  DMX_REQUIRE(d && d->finalized, "trocr_dec_beam_step: weights not finalized (bind_arena, load_param*, finalize)");
  DMX_REQUIRE(cache && ws && beam_args_ok(d, B, nb, S, max_len) && early_stopping >= 0 && early_stopping <= 2,
              "trocr_dec_beam_step: bad argument (B=%d beams=%d S=%d max_len=%d early_stopping=%d)", B, nb, S, max_len, early_stopping);
  BeamStep bm{nb, early_stopping, length_penalty, logp};
  return dec_step(d, (char*)cache, B * nb, S, max_len, eos_token_id, 0, nullptr, nullptr, 0, (char*)ws, ws_bytes, (hipStream_t)stream, &bm);
}
extern "C" int dmx_trocr_dec_beam_finalize(dmx_trocr_dec* d, void* cache, int B, int nb, int S, int max_len, int num_return, int pad_token_id,
                                           long long* sequences, float* scores, int* lengths, dmx_stream_t stream) {
  DMX_REQUIRE(cache && sequences && scores && lengths && beam_args_ok(d, B, nb, S, max_len) && num_return >= 1 && num_return <= nb,
              "trocr_dec_beam_finalize: bad argument");
  const BeamLayout z = beam_layout(d, B, nb, S, max_len);
  hipLaunchKernelGGL(dmx_dec_beam_gather_kernel, dim3(B * num_return), dim3(64), 0, (hipStream_t)stream, (int*)((char*)cache + z.bstate), nb,
                     num_return, max_len, pad_token_id, sequences, scores, lengths);
  return dmx_check_launch("dmx_dec_beam_gather_kernel");
}
// op entry (tests): one selection step on supplied fp32 logits [B * nb][V], through the launch function the step calls.  state:
// the 256 state words; beam_state: dmx_trocr_dec_beam_state_bytes(max_len) bytes (set up by reset != 0: position 0)
extern "C" size_t dmx_trocr_dec_beam_select_workspace_bytes(int B, int nb, int V) {
  if (B < 1 || nb < 2 || nb > 16 || B * nb > 64 || V < 2 * nb || !beam_chunk(V, nb)) return 0;
  const size_t M = (size_t)B * nb, C = cdiv(V, beam_chunk(V, nb));
  return 2 * align_up(M * cdiv(V, 64) * 4, 256) + 2 * align_up(M * C * 2 * nb * 4, 256);
}
extern "C" int dmx_trocr_dec_beam_select(const float* logits, int B, int nb, int V, int max_len, int eos_token_id, float length_penalty,
                                         int early_stopping, int reset, int start_token, int* state, void* beam_state, float* logp,
                                         void* ws, size_t ws_bytes, dmx_stream_t stream) {
  const size_t need = dmx_trocr_dec_beam_select_workspace_bytes(B, nb, V);
  DMX_REQUIRE(logits && state && beam_state && ws && need && ws_bytes >= need && max_len >= 2 && early_stopping >= 0 && early_stopping <= 2,
              "trocr_dec_beam_select: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const int M = B * nb, nblk = cdiv(V, 64);
  BeamSel q{};
  q.chunk = beam_chunk(V, nb); q.C = cdiv(V, q.chunk); q.K = 2 * nb;
  char* p = (char*)ws;
  float* pmax = (float*)p; p += align_up((size_t)M * nblk * 4, 256);
  float* psum = (float*)p; p += align_up((size_t)M * nblk * 4, 256);
  q.cv = (float*)p; p += align_up((size_t)M * q.C * q.K * 4, 256);
  q.ci = (int*)p;
  int rc;
  if (reset) {
    const size_t bwords = beam_state_bytes(max_len) / 4;
    hipLaunchKernelGGL(dmx_dec_beam_reset_kernel, dim3((unsigned)std::min<size_t>(1024, (bwords + 255) / 256)), dim3(256), 0, st, state, (size_t)ST_INTS,
                       M, nb, start_token, (int*)beam_state, bwords, max_len);
    if ((rc = dmx_check_launch("dmx_dec_beam_reset_kernel"))) return rc;
  }
  hipLaunchKernelGGL(dmx_dec_beam_partials_kernel, dim3(nblk, M), dim3(64), 0, st, logits, V, V, nblk, pmax, psum);
  if ((rc = dmx_check_launch("dmx_dec_beam_partials_kernel"))) return rc;
  q.logits = logits; q.ldl = V; q.pmax = pmax; q.psum = psum; q.nblk = nblk; q.B = B; q.nb = nb; q.V = V; q.max_len = max_len;
  q.eos = eos_token_id; q.early = early_stopping; q.lp = length_penalty; q.state = state; q.bs = (int*)beam_state; q.logp = logp;
  return beam_select_launch(q, st);
}
// the body of both decode-attention op entries (arguments checked by the entry): counters zeroed, then one launch
static int attn_op(const float* q, int M, int H, const void* kv, long long bstride, int rstride, int L, const void* table, int ld_table,
                   int rows_per_item, void* out, void* ws, hipStream_t st) {
  int* cnt = (int*)ws;
  hipLaunchKernelGGL(dmx_dec_reset_kernel, dim3(1), dim3(256), 0, st, cnt, (size_t)M * H, 0, 0, (long long*)nullptr, 1);
  int rc = dmx_check_launch("dmx_dec_reset_kernel");
  if (rc) return rc;
  DecAttn t{};
  t.q = q; t.ldq = H * 64; t.kv = (const bf16*)kv; t.bstride = bstride; t.rstride = rstride; t.state = nullptr; t.L = L; t.H = H; t.D = H * 64;
  t.nch = cdiv(L, 64); t.part = (float*)((char*)ws + align_up((size_t)M * H * 4, 256)); t.cnt = cnt; t.o = (bf16*)out; t.ldo = H * 64;
  t.src = (const unsigned char*)table; t.src_ld = ld_table; t.rpi = rows_per_item;
  return dec_attn_launch(t, M, st);
}
// decode attention with the beam indirections: table (nullable) uint8 [M][ld_table] - key j < L - 1 of row b from physical row
// table[b][j], key L - 1 from row b -, rows_per_item > 0: row b reads the K/V of item b / rows_per_item
extern "C" int dmx_trocr_dec_beam_attn(const float* q, int M, int H, const void* kv, long long bstride, int rstride, int L, const void* table,
                                       int ld_table, int rows_per_item, void* out, void* ws, size_t ws_bytes, dmx_stream_t stream) {
  DMX_REQUIRE(q && kv && out && ws && M >= 1 && M <= 64 && H >= 1 && L >= 1 && rstride >= 2 * H * 64 && rows_per_item >= 0, "trocr_dec_beam_attn: bad argument");
  DMX_REQUIRE(!table || ld_table >= L - 1, "trocr_dec_beam_attn: ld_table %d < L - 1", ld_table);
  DMX_REQUIRE(ws_bytes >= dmx_trocr_dec_attn_workspace_bytes(M, H, L), "trocr_dec_beam_attn: workspace too small");
  return attn_op(q, M, H, kv, bstride, rstride, L, table, ld_table, rows_per_item, out, ws, (hipStream_t)stream);
}

// ---- op entry points (tests / benchmarks): one weight-streaming linear with a chosen epilogue, one decode attention
extern "C" size_t dmx_trocr_dec_linear_workspace_bytes(int M, int N, int K) {
  const size_t nblk = (size_t)cdiv(N, 64);
  return align_up((nblk + 1) * 4, 256) + align_up((size_t)(K / 128) * M * N * 4, 256) + align_up((size_t)M * N * 4, 256) + 2 * align_up((size_t)M * nblk * 4, 256);
}
extern "C" int dmx_trocr_dec_linear(int epi, int act, const void* x, int M, int K, const void* w, int N, const float* bias, float oscale,
                                    float* yf, int ldyf, void* yb, const float* res, const float* gamma, const float* beta,
                                    void* kv, int max_len, int* state, long long* ids, int eos, int pad, int kchunk,
                                    void* ws, size_t ws_bytes, dmx_stream_t stream) {
  DMX_REQUIRE(x && w && ws && epi >= 0 && epi <= 3 && M >= 1 && M <= 64 && N >= 1 && K >= 128, "trocr_dec_linear: bad argument");
  DMX_REQUIRE(ws_bytes >= dmx_trocr_dec_linear_workspace_bytes(M, N, K), "trocr_dec_linear: workspace too small");
  DMX_REQUIRE(epi != EPI_QKV || (N % 3 == 0 && yf && kv && state), "trocr_dec_linear: q|k|v epilogue needs N = 3D, yf, kv, state");
  DMX_REQUIRE(epi != EPI_LN || (res && gamma && beta && yf && yb), "trocr_dec_linear: LayerNorm epilogue needs res, gamma, beta, yf, yb");
  DMX_REQUIRE(epi != EPI_PICK || (state && ids && max_len >= 1), "trocr_dec_linear: pick epilogue needs state, ids");
  hipStream_t st = (hipStream_t)stream;
  const size_t nblk = (size_t)cdiv(N, 64);
  char* p = (char*)ws;
  int* cnt = (int*)p; p += align_up((nblk + 1) * 4, 256);
  float* part = (float*)p; p += align_up((size_t)(K / 128) * M * N * 4, 256);
  float* pre = (float*)p; p += align_up((size_t)M * N * 4, 256);
  float* pv = (float*)p; p += align_up((size_t)M * nblk * 4, 256);
  int* pi = (int*)p;
  hipLaunchKernelGGL(dmx_dec_reset_kernel, dim3(1), dim3(256), 0, st, cnt, nblk + 1, 0, 0, (long long*)nullptr, 1);
  int rc = dmx_check_launch("dmx_dec_reset_kernel");
  if (rc) return rc;
  DecLin a = lin_base((const bf16*)x, M, K, (const bf16*)w, N, bias, epi, cnt, part);
  if (kchunk > 0) { a.kchunk = kchunk; a.splits = cdiv(K, kchunk); }
  a.act = act; a.oscale = oscale; a.yf = yf; a.ldyf = ldyf; a.yb = (bf16*)yb; a.ldyb = N;
  if (epi == EPI_QKV) { a.D = N / 3; a.ldyf = a.D; a.kv = (bf16*)kv; a.kv_bstride = (long long)max_len * 2 * a.D; a.state = state; a.max_len = max_len; }
  if (epi == EPI_LN) { a.res = res; a.pre = pre; a.gamma = gamma; a.beta = beta; a.ldyb = N; }
  if (epi == EPI_PICK) { a.pv = pv; a.pi = pi; a.ids = ids; a.max_len = max_len; a.eos = eos; a.pad = pad; a.state = state; }
  return dec_linear_launch(a, st);
}
extern "C" size_t dmx_trocr_dec_attn_workspace_bytes(int M, int H, int L) {
  return align_up((size_t)M * H * 4, 256) + (size_t)M * H * cdiv(L, 64) * 66 * 4;
}
extern "C" int dmx_trocr_dec_attn(const float* q, int M, int H, const void* kv, long long bstride, int rstride, int L, void* out,
                                  void* ws, size_t ws_bytes, dmx_stream_t stream) {
  DMX_REQUIRE(q && kv && out && ws && M >= 1 && H >= 1 && L >= 1 && rstride >= 2 * H * 64, "trocr_dec_attn: bad argument");
  DMX_REQUIRE(ws_bytes >= dmx_trocr_dec_attn_workspace_bytes(M, H, L), "trocr_dec_attn: workspace too small");
  return attn_op(q, M, H, kv, bstride, rstride, L, nullptr, 0, 0, out, ws, (hipStream_t)stream);
}
