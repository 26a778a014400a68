// OCR read-back, teacher-forced: how well does an edited box read as the text that was asked for?  transformers'
// `VisionEncoderDecoderModel(pixel_values=..., labels=...)` over the decoder of trocr_dec.hip (app.ipynb:548).  With the ids known all
// M = B * T rows go through every layer at once - GEMMs at M rows with the weights read once instead of T decode steps at B rows:
//   prefill_embed - token + position (+ scale) + layernorm_embedding of a [B][T] block, the label shift (shift_tokens_right) applied
//                   on the device: position 0 reads start_token, position t labels[t - 1] (ignore_index -> pad_token)
//   prefill_attn  - causal self-attention, d = 64, on MFMA: one wave per (item, head, 16-query tile) walks 32-key tiles up to its
//                   diagonal (tiles behind it are never read), masks the diagonal tile in registers, keeps (max, sum) in fp32 and
//                   feeds P to the PV MFMAs as a bf16 pair hi + lo, so the probabilities lose nothing to the 16-bit operand
//   lm_tile       - x[M][K] W[V][K]^T on MFMA, 64 rows x 64 vocabulary entries per block; per (row, tile): (max, sum exp(x - max)),
//                   (best value, lowest index), the label's logit where the label falls in the tile; fp32 logits only on request
//   lm_combine    - one wave per row merges the tile partials in tile order: log-sum-exp, arg-max (ties -> lowest index, pick_better
//                   of trocr_dec.h), token_logprob = logit[label] - lse.  No counters, no float atomics: two plain launches.
// The layers (post-LN, tests/trocr_restatement._layers) are the GEMM / attention / cast kernels of the other models at fixed plans
// (one tile instance, no K split: a row's arithmetic does not depend on how many rows run with it), with the residual stream in
// fp32 as on the step path: x = LN(x + y) reads the GEMM's fp32 output and writes the fp32 stream and its 16-bit copy.
#include <math.h>
#include <algorithm>
#include "trocr_dec.h"

namespace {
constexpr int kMaxRows = 4096, kMaxItems = 64, kMaxT = 512;

// ---- embedding of a [B][T] block: one wave per row (dec_embed_row), the token from the shifted labels, the position from the row
__global__ __launch_bounds__(64) void dmx_prefill_embed_kernel(const long long* labels, const long long* dec_ids, int T, int start, int pad, int ignore,
                                                               const bf16* emb, int V, const float* posw, int npos, float scale,
                                                               const float* gamma, const float* beta, int D, float* yf, bf16* yb) {
  const int lane = threadIdx.x, m = blockIdx.x, t = m % T;
  long long id;
  if (dec_ids) id = dec_ids[m];
  else if (t == 0) id = start;
  else { id = labels[m - 1]; if (id == (long long)ignore) id = pad; }
  const int tok = id < 0 ? 0 : id >= V ? V - 1 : (int)id;
  const int prow = min(t + 2, npos - 1);
  dec_embed_row(tok, prow, lane, m, emb, posw, scale, gamma, beta, D, yf, yb);
}

// ---- x = LN(x + y) over rows of D = 64 nper values (D % 256 == 0, D <= 1024): one wave per row, lane -> columns lane * nper + e.
// y is the fp32 output (bias included) of the GEMM in front; x is the fp32 residual stream, rewritten in place with its 16-bit copy
__global__ __launch_bounds__(64) void dmx_prefill_add_ln_kernel(const float* y, float* xf, bf16* xb, const float* gamma, const float* beta, float eps, int D) {
  const int lane = threadIdx.x, nper = D >> 6, c0 = lane * nper;
  const size_t row = (size_t)blockIdx.x * D;
  float v[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = c0 + min(q, nper / 4 - 1) * 4;
    const f32x4 a = *(const f32x4*)(y + row + c), b = *(const f32x4*)(xf + row + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[4 * q + e] = a[e] + b[e];
  }
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) if (e < nper) s += v[e];
  const float mean = wave_sum(s) / (float)D;
  float sq = 0.f;
#pragma unroll
  for (int e = 0; e < 16; ++e) if (e < nper) { const float d = v[e] - mean; sq += d * d; }
  const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)D + eps);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (4 * q >= nper) break;
    const int c = c0 + 4 * q;
    const f32x4 g = *(const f32x4*)(gamma + c), b = *(const f32x4*)(beta + c);
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (v[4 * q + e] - mean) * rstd * g[e] + b[e];
    *(f32x4*)(xf + row + c) = (f32x4){o[0], o[1], o[2], o[3]};
    *(u32x2*)(xb + row + c) = (u32x2){pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3])};
  }
}

// ReLU in place on 16-bit elements (configs with activation_function = "relu": the GEMM epilogue knows GELU only); exact on the
// rounded values: relu(round(v)) = round(relu(v))
__global__ __launch_bounds__(256) void dmx_prefill_relu_kernel(bf16* x, size_t n8) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
    float f[8];
    unpack_bf8(*(const u32x4*)(x + i * 8), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = fmaxf(f[e], 0.f);
    *(u32x4*)(x + i * 8) = pack_bf8(f);
  }
}

// ---- causal self-attention, d = 64
struct PfAttn {
  const bf16* q; int ldq; const bf16* k; int ldk; const bf16* v; int ldv;   // row b * T + t, head h at column h * 64
  bf16* o; int ldo;
  int B, H, T; float scale;
};
// lane (g, r) = (lane / 16, lane % 16).  S^T = K Q^T per 16-key tile: A = key rows, B = query rows, both read as d = 32 j + 8 g + e;
// the result holds, for query q0 + r, the keys 4 g + i.  O^T = V^T P: the MFMA's 32 k-slots of lane group g are the keys
// {4 g + e, 16 + 4 g + e} of the 32-key tile - exactly the scores the lane holds - in A (V^T, gathered) and B (P) alike.
__global__ __launch_bounds__(64) void dmx_prefill_attn_kernel(PfAttn a) {
  const int lane = threadIdx.x, g = lane >> 4, r = lane & 15;
  const int q0 = blockIdx.x * 16, h = blockIdx.y, b = blockIdx.z, T = a.T;
  const size_t row0 = (size_t)b * T;
  const int qi = q0 + r;                                         // this lane's query (rows >= T of a ragged tile compute on row T - 1, unstored)
  const bf16* qp = a.q + (row0 + min(qi, T - 1)) * a.ldq + h * 64 + 8 * g;
  const bf16x8 qf0 = *(const bf16x8*)qp, qf1 = *(const bf16x8*)(qp + 32);
  const int kend = min(q0 + 16, T);                              // keys [0, kend): tiles behind the diagonal are skipped
  float m = -INFINITY, l = 0.f;
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < kend; k0 += 32) {
    float s[8];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const bf16* kp = a.k + (row0 + min(k0 + 16 * u + r, T - 1)) * a.ldk + h * 64 + 8 * g;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      acc = DMX_MFMA_16x16x32(*(const bf16x8*)kp, qf0, acc);
      acc = DMX_MFMA_16x16x32(*(const bf16x8*)(kp + 32), qf1, acc);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = k0 + 16 * u + 4 * g + i;
        s[4 * u + i] = (key <= qi && key < T) ? acc[i] * a.scale : -INFINITY;      // the diagonal tile, masked in registers
      }
    }
    float mx = s[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) mx = fmaxf(mx, s[e]);
    mx = fmaxf(mx, __shfl_xor(mx, 16)); mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx);                               // finite from the first tile on: key 0 is visible to every query
    const float corr = expf(m - mn);
    float p[8], ps = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { p[e] = s[e] == -INFINITY ? 0.f : expf(s[e] - mn); ps += p[e]; }
    ps += __shfl_xor(ps, 16); ps += __shfl_xor(ps, 32);
    l = l * corr + ps; m = mn;
    bf16x8 ph, pl;
#pragma unroll
    for (int e = 0; e < 8; ++e) { ph[e] = (bf16)p[e]; pl[e] = (bf16)(p[e] - (float)ph[e]); }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      bf16x8 vf;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int key = k0 + (e < 4 ? 4 * g + e : 16 + 4 * g + (e - 4));
        vf[e] = key < kend ? a.v[(row0 + key) * a.ldv + h * 64 + 16 * dt + r] : (bf16)0.f;
      }
      o[dt] *= corr;
      o[dt] = DMX_MFMA_16x16x32(vf, ph, o[dt]);
      o[dt] = DMX_MFMA_16x16x32(vf, pl, o[dt]);
    }
  }
  if (qi >= T) return;
  const float inv = 1.0f / l;
  bf16* op = a.o + (row0 + qi) * a.ldo + h * 64 + 4 * g;         // o[dt][i]: d = 16 dt + 4 g + i
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
    *(u32x2*)(op + 16 * dt) = (u32x2){pack_bf2(o[dt][0] * inv, o[dt][1] * inv), pack_bf2(o[dt][2] * inv, o[dt][3] * inv)};
}

// ---- fused LM head + loss
struct PfLm {
  const bf16* x; int ldx;            // [M][K]
  const bf16* w; int ldw;            // [V][K]
  int M, V, K, NT;                   // NT = cdiv(V, 64) vocabulary tiles
  const long long* labels; int ignore;
  float* pmax; float* psum; int* pidx;   // [M][NT]
  float* labv;                       // [M]: the label's logit (written by the one lane that owns the column)
  float* logits; int ldl;            // optional [M][ldl]
  float* logp; int* amax;            // combine: token_logprob [M] (with labels), argmax [M] (optional)
};
// block (mt, nt): rows mt * 64 ..., vocabulary entries nt * 64 ...; wave w takes 16 entries against all 64 rows.  Operands as in
// dmx_dec_linear_kernel: lane (g, r) reads weight row n + r and activation rows 16 t + r at k = kb + 32 g + 8 j + e for MFMA j
__global__ __launch_bounds__(256) void dmx_prefill_lm_tile_kernel(PfLm a) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, g = lane >> 4, r = lane & 15;
  const int m0 = blockIdx.x * 64, nt = blockIdx.y, n0 = nt * 64 + wv * 16;
  const bool wok = n0 + r < a.V;
  const bf16* wp = a.w + (size_t)(wok ? n0 + r : 0) * a.ldw + g * 32;
  const bf16* xp[4]; bool xok[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    xok[t] = m0 + t * 16 + r < a.M;
    xp[t] = a.x + (size_t)(xok[t] ? m0 + t * 16 + r : 0) * a.ldx + g * 32;
  }
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const u32x4 zero = {0u, 0u, 0u, 0u};
  for (int k = 0; k < a.K; k += 128) {
    u32x4 wa[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wa[j] = wok ? *(const u32x4*)(wp + k + j * 8) : zero;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      u32x4 xb[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) xb[j] = xok[t] ? *(const u32x4*)(xp[t] + k + j * 8) : zero;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[t] = DMX_MFMA_16x16x32(__builtin_bit_cast(bf16x8, wa[j]), __builtin_bit_cast(bf16x8, xb[j]), acc[t]);
    }
  }
  // acc[t][i]: entry n0 + 4 g + i, row m0 + 16 t + r
  __shared__ float sv[4][64], ss[4][64];
  __shared__ int si[4][64];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int m = m0 + t * 16 + r;
    const bool mok = m < a.M;
    const long long lab = (a.labels && mok) ? a.labels[m] : -1;
    float bv = -INFINITY; int bi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = n0 + 4 * g + i;
      if (n < a.V) {
        if (mok && a.logits) a.logits[(size_t)m * a.ldl + n] = acc[t][i];
        if (mok && lab == (long long)n) a.labv[m] = acc[t][i];
        pick_merge(bv, bi, acc[t][i], n);
      }
    }
#pragma unroll
    for (int d = 16; d <= 32; d <<= 1) {
      const float ov = __shfl_xor(bv, d); const int oi = __shfl_xor(bi, d);
      pick_merge(bv, bi, ov, oi);
    }
    float sm = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) if (n0 + 4 * g + i < a.V && bv != -INFINITY) sm += expf(acc[t][i] - bv);
    sm += __shfl_xor(sm, 16); sm += __shfl_xor(sm, 32);
    if (g == 0) { sv[wv][t * 16 + r] = bv; si[wv][t * 16 + r] = bi; ss[wv][t * 16 + r] = sm; }
  }
  __syncthreads();
  const int tid = threadIdx.x;
  if (tid < 64 && m0 + tid < a.M) {                              // the four waves of a row in wave order
    float bv = sv[0][tid]; int bi = si[0][tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) pick_merge(bv, bi, sv[w][tid], si[w][tid]);
    float sm = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) if (sv[w][tid] != -INFINITY) sm += ss[w][tid] * expf(sv[w][tid] - bv);
    const size_t q = (size_t)(m0 + tid) * a.NT + nt;
    a.pmax[q] = bv; a.pidx[q] = bi; a.psum[q] = sm;
  }
}
// one wave per row: the tile partials in tile order (lane c takes tiles c, c + 64, ...; the cross-lane merges are order-free for
// (value, index) and a fixed butterfly for the sum)
__global__ __launch_bounds__(64) void dmx_prefill_lm_combine_kernel(PfLm a) {
  const int lane = threadIdx.x, m = blockIdx.x;
  const float* pm = a.pmax + (size_t)m * a.NT; const float* ps = a.psum + (size_t)m * a.NT; const int* pi = a.pidx + (size_t)m * a.NT;
  float bv = -INFINITY; int bi = 0x7fffffff;
  for (int c = lane; c < a.NT; c += 64) pick_merge(bv, bi, pm[c], pi[c]);
#pragma unroll
  for (int d = 1; d <= 32; d <<= 1) {
    const float ov = __shfl_xor(bv, d); const int oi = __shfl_xor(bi, d);
    pick_merge(bv, bi, ov, oi);
  }
  float sm = 0.f;
  for (int c = lane; c < a.NT; c += 64) { const float v = pm[c]; if (v != -INFINITY) sm += ps[c] * expf(v - bv); }
  sm = wave_sum(sm);
  if (lane != 0) return;
  if (a.amax) a.amax[m] = (bi < 0 || bi >= a.V) ? 0 : bi;        // (all logits NaN: keep the id in range)
  if (a.labels) {
    const long long lab = a.labels[m];
    const float lse = bv + logf(sm);
    a.logp[m] = lab == (long long)a.ignore ? 0.f : (lab >= 0 && lab < a.V) ? a.labv[m] - lse : NAN;
  }
}

int embed_launch(const long long* labels, const long long* dec_ids, int B, int T, int start, int pad, int ignore, const bf16* emb, int V,
                 const float* posw, int npos, float scale, const float* gamma, const float* beta, int D, float* xf, bf16* xb, hipStream_t st) {
  hipLaunchKernelGGL(dmx_prefill_embed_kernel, dim3(B * T), dim3(64), 0, st, labels, dec_ids, T, start, pad, ignore, emb, V, posw, npos, scale,
                     gamma, beta, D, xf, xb);
  return dmx_check_launch("dmx_prefill_embed_kernel");
}
int attn_launch(const PfAttn& a, hipStream_t st) {
  DMX_REQUIRE(a.B >= 1 && a.H >= 1 && a.T >= 1 && a.T <= kMaxT && (long long)a.B * a.T <= kMaxRows, "trocr_dec_prefill_attn: B=%d H=%d T=%d", a.B, a.H, a.T);
  DMX_REQUIRE(a.ldq % 8 == 0 && a.ldk % 8 == 0 && a.ldv % 8 == 0 && a.ldo % 8 == 0 && a.ldq >= a.H * 64 && a.ldk >= a.H * 64 && a.ldv >= a.H * 64 && a.ldo >= a.H * 64,
              "trocr_dec_prefill_attn: row strides must be multiples of 8 and hold H * 64 columns");
  DMX_REQUIRE(((size_t)a.q | (size_t)a.k | (size_t)a.v | (size_t)a.o) % 16 == 0, "trocr_dec_prefill_attn: operands must be 16-byte aligned");
  hipLaunchKernelGGL(dmx_prefill_attn_kernel, dim3(cdiv(a.T, 16), a.H, a.B), dim3(64), 0, st, a);
  return dmx_check_launch("dmx_prefill_attn_kernel");
}
size_t lm_ws_bytes(int M, int V) { return 3 * align_up((size_t)M * cdiv(V, 64) * 4, 256) + align_up((size_t)M * 4, 256); }
int lm_launch(PfLm a, void* ws, hipStream_t st) {
  DMX_REQUIRE(a.M >= 1 && a.M <= kMaxRows && a.V >= 1 && a.K >= 128 && a.K % 128 == 0 && a.ldx % 8 == 0 && a.ldw % 8 == 0,
              "trocr_dec_prefill_lm_loss: M=%d V=%d K=%d", a.M, a.V, a.K);
  DMX_REQUIRE(!a.logits || a.ldl >= a.V, "trocr_dec_prefill_lm_loss: ld_logits %d < vocab %d", a.ldl, a.V);
  DMX_REQUIRE(!a.labels || a.logp, "trocr_dec_prefill_lm_loss: labels need token_logprob");
  a.NT = cdiv(a.V, 64);
  char* p = (char*)ws;
  const size_t plane = align_up((size_t)a.M * a.NT * 4, 256);
  a.pmax = (float*)p; a.psum = (float*)(p + plane); a.pidx = (int*)(p + 2 * plane); a.labv = (float*)(p + 3 * plane);
  hipLaunchKernelGGL(dmx_prefill_lm_tile_kernel, dim3(cdiv(a.M, 64), a.NT), dim3(256), 0, st, a);
  int rc = dmx_check_launch("dmx_prefill_lm_tile_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(dmx_prefill_lm_combine_kernel, dim3(a.M), dim3(64), 0, st, a);
  return dmx_check_launch("dmx_prefill_lm_combine_kernel");
}

// y[M][N] = x[M][K] W[N][K]^T + bias on the 128 x 64 tile instance without a K split, whatever M is: a row's sum runs in the same
// order alone and inside a batch.  act = 1: exact GELU in the epilogue (16-bit output only)
int gemm_fixed(const bf16* x, int M, int K, const bf16* w, int N, const float* bias, void* out, int out_f32, int act, hipStream_t st) {
  GemmArgs a{};
  a.x0 = x; a.x1 = x; a.ldx0 = K; a.ldx1 = K; a.cx0 = K; a.Cin = K;
  a.direct = 1; a.ksize = 1; a.stride = 1; a.IH = a.OH = 1; a.IW = a.OW = M;
  a.Ktaps = K; a.K = K; a.w = w; a.ldw = K; a.M = M; a.N = N;
  a.bias = bias; a.rows_per_group = 1; a.out = out; a.ldo = N; a.out_f32 = out_f32; a.act = act;
  a.force_tn = 1; a.force_splitk = 1;
  return dmx_gemm_launch(a, nullptr, 0, st);
}

struct PfLayout { size_t encb, ckv, xf, xb, y, qkv, ab, qc, hb, lm, total; };
PfLayout pf_layout(const dmx_trocr_dec* d, int B, int S, int T) {
  const dmx_trocr_dec_config& c = d->cfg;
  const size_t M = (size_t)B * T, D = c.d_model, F = c.ffn_dim, L = c.num_layers;
  PfLayout y{};
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t r = o; o += align_up(bytes, 256); return r; };
  y.encb = take((size_t)B * S * d->kdim * 2); y.ckv = take((size_t)B * S * L * 2 * D * 2);
  y.xf = take(M * D * 4); y.xb = take(M * D * 2); y.y = take(M * D * 4); y.qkv = take(M * 3 * D * 2); y.ab = take(M * D * 2);
  y.qc = take(M * D * 2); y.hb = take(M * F * 2); y.lm = take(lm_ws_bytes((int)M, c.vocab_size));
  y.total = o;
  return y;
}
bool pf_args_ok(const dmx_trocr_dec* d, int B, int S, int T) {
  return d && B >= 1 && B <= kMaxItems && S >= 1 && T >= 1 && T <= d->cfg.max_position_embeddings && T <= kMaxT && (long long)B * T <= kMaxRows;
}
}  // namespace

extern "C" size_t dmx_trocr_dec_prefill_workspace_bytes(const dmx_trocr_dec* d, int B, int S, int T) {
  return pf_args_ok(d, B, S, T) ? pf_layout(d, B, S, T).total : 0;
}

extern "C" int dmx_trocr_dec_score(dmx_trocr_dec* d, const float* enc, int B, int S, const long long* labels, const long long* dec_ids, int T,
                                   int start_token, int pad_token, int ignore_index, float* token_logprob, int* argmax, float* logits,
                                   int ld_logits, void* ws, size_t ws_bytes, dmx_stream_t stream) {
  DMX_REQUIRE(d && d->finalized, "trocr_dec_score: weights not finalized (bind_arena, load_param*, finalize)");
  DMX_REQUIRE(pf_args_ok(d, B, S, T), "trocr_dec_score: bad argument (B=%d S=%d T=%d): 1 <= B <= 64, 1 <= T <= %d, B * T <= %d", B, S, T,
              std::min(d->cfg.max_position_embeddings, kMaxT), kMaxRows);
  DMX_REQUIRE(enc && ws && (labels || dec_ids), "trocr_dec_score: null argument (encoder states, workspace, labels or decoder_input_ids)");
  DMX_REQUIRE(!labels || token_logprob, "trocr_dec_score: labels need token_logprob");
  DMX_REQUIRE(labels || argmax || logits, "trocr_dec_score: nothing to write (no labels, argmax or logits)");
  const dmx_trocr_dec_config& c = d->cfg;
  const int D = c.d_model, F = c.ffn_dim, L = c.num_layers, H = D / 64, V = c.vocab_size, M = B * T;
  DMX_REQUIRE(!logits || ld_logits >= V, "trocr_dec_score: ld_logits %d < vocab %d", ld_logits, V);
  const PfLayout y = pf_layout(d, B, S, T);
  DMX_REQUIRE(ws_bytes >= y.total, "trocr_dec_score: workspace %zu < %zu bytes", ws_bytes, y.total);
  hipStream_t st = (hipStream_t)stream;
  char* w = (char*)ws;
  bf16* encb = (bf16*)(w + y.encb); bf16* ckv = (bf16*)(w + y.ckv); float* xf = (float*)(w + y.xf); bf16* xb = (bf16*)(w + y.xb);
  float* yf = (float*)(w + y.y); bf16* qkv = (bf16*)(w + y.qkv); bf16* ab = (bf16*)(w + y.ab); bf16* qc = (bf16*)(w + y.qc); bf16* hb = (bf16*)(w + y.hb);
  // cross K/V of every layer: one GEMM at B * S rows, as the step path's cross_kv_launch but on the fixed plan
  int rc = dmx_cast_f32_to_bf16_launch(enc, encb, (size_t)B * S * d->kdim, st);
  if (rc) return rc;
  const int Nkv = 2 * L * D;
  if ((rc = gemm_fixed(encb, B * S, d->kdim, d->at<bf16>(d->wckv), Nkv, d->at<float>(d->bckv), ckv, 0, 0, st))) return rc;
  const float escale = c.scale_embedding ? sqrtf((float)D) : 1.0f;
  if ((rc = embed_launch(dec_ids ? nullptr : labels, dec_ids, B, T, start_token, pad_token, ignore_index, d->at<bf16>(d->emb), V, d->at<float>(d->posw),
                         d->npos, escale, c.layernorm_embedding ? d->at<float>(d->leg) : nullptr, c.layernorm_embedding ? d->at<float>(d->leb) : nullptr,
                         D, xf, xb, st))) return rc;
  const float qscale = 0.125f;                                   // head_dim ** -0.5: a power of two, so scaling the scores of the rounded q
                                                                 // equals rounding the scaled q (q is scaled after its bias either way)
  auto add_ln = [&](const float* g, const float* b) {
    hipLaunchKernelGGL(dmx_prefill_add_ln_kernel, dim3(M), dim3(64), 0, st, (const float*)yf, xf, xb, g, b, 1e-5f, D);
    return dmx_check_launch("dmx_prefill_add_ln_kernel");
  };
  for (int l = 0; l < L; ++l) {
    const DecLayer& W = d->layers[l];
    if ((rc = gemm_fixed(xb, M, D, d->at<bf16>(W.wqkv), 3 * D, d->at<float>(W.bqkv), qkv, 0, 0, st))) return rc;
    PfAttn t{};
    t.q = qkv; t.k = qkv + D; t.v = qkv + 2 * D; t.ldq = t.ldk = t.ldv = 3 * D; t.o = ab; t.ldo = D; t.B = B; t.H = H; t.T = T; t.scale = qscale;
    if ((rc = attn_launch(t, st))) return rc;
    if ((rc = gemm_fixed(ab, M, D, d->at<bf16>(W.wo), D, d->at<float>(W.bo), yf, 1, 0, st))) return rc;
    if ((rc = add_ln(d->at<float>(W.l1g), d->at<float>(W.l1b)))) return rc;
    if ((rc = gemm_fixed(xb, M, D, d->at<bf16>(W.wcq), D, d->at<float>(W.bcq), qc, 0, 0, st))) return rc;
    AttnArgs ca{};                                               // queries [B * T] against each item's S encoder rows: the plain grid (one
    ca.q = qc; ca.ldq = D; ca.k = ckv + (size_t)l * 2 * D; ca.ldk = Nkv; ca.kv_rows = S; ca.v = ca.k + D; ca.ldv = Nkv;     // block walks all keys)
    ca.o = ab; ca.ldo = D; ca.B = B; ca.H = H; ca.Sq = T; ca.Skv = S; ca.scale = qscale;
    if ((rc = dmx_attention_launch(ca, st))) return rc;
    if ((rc = gemm_fixed(ab, M, D, d->at<bf16>(W.wco), D, d->at<float>(W.bco), yf, 1, 0, st))) return rc;
    if ((rc = add_ln(d->at<float>(W.l2g), d->at<float>(W.l2b)))) return rc;
    if ((rc = gemm_fixed(xb, M, D, d->at<bf16>(W.w1), F, d->at<float>(W.b1), hb, 0, c.activation == 1 ? 0 : 1, st))) return rc;
    if (c.activation == 1) {
      const size_t n8 = (size_t)M * F / 8;
      hipLaunchKernelGGL(dmx_prefill_relu_kernel, dim3((unsigned)std::min<size_t>(4096, (n8 + 255) / 256)), dim3(256), 0, st, hb, n8);
      if ((rc = dmx_check_launch("dmx_prefill_relu_kernel"))) return rc;
    }
    if ((rc = gemm_fixed(hb, M, F, d->at<bf16>(W.w2), D, d->at<float>(W.b2), yf, 1, 0, st))) return rc;
    if ((rc = add_ln(d->at<float>(W.l3g), d->at<float>(W.l3b)))) return rc;
  }
  PfLm q{};
  q.x = xb; q.ldx = D; q.w = d->at<bf16>(d->lm); q.ldw = D; q.M = M; q.V = V; q.K = D; q.labels = labels; q.ignore = ignore_index;
  q.logits = logits; q.ldl = ld_logits; q.logp = token_logprob; q.amax = argmax;
  return lm_launch(q, w + y.lm, st);
}

// ---- op entry points (tests)
extern "C" int dmx_trocr_dec_prefill_embed(const long long* labels, const long long* dec_ids, int B, int T, int start_token, int pad_token,
                                           int ignore_index, const void* emb, int V, const float* posw, int npos, float scale,
                                           const float* gamma, const float* beta, int D, float* xf, void* xb, dmx_stream_t stream) {
  DMX_REQUIRE((labels || dec_ids) && emb && posw && xf && xb && (!gamma || beta), "trocr_dec_prefill_embed: null argument");
  DMX_REQUIRE(B >= 1 && B <= kMaxItems && T >= 1 && T <= kMaxT && (long long)B * T <= kMaxRows && V >= 1 && npos >= 1 && D % 256 == 0 && D >= 256 && D <= 1024,
              "trocr_dec_prefill_embed: B=%d T=%d V=%d D=%d", B, T, V, D);
  return embed_launch(dec_ids ? nullptr : labels, dec_ids, B, T, start_token, pad_token, ignore_index, (const bf16*)emb, V, posw, npos, scale, gamma, beta,
                      D, xf, (bf16*)xb, (hipStream_t)stream);
}
extern "C" int dmx_trocr_dec_prefill_attn(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out, int ldo,
                                          int B, int H, int T, float scale, dmx_stream_t stream) {
  DMX_REQUIRE(q && k && v && out, "trocr_dec_prefill_attn: null argument");
  PfAttn t{};
  t.q = (const bf16*)q; t.ldq = ldq; t.k = (const bf16*)k; t.ldk = ldk; t.v = (const bf16*)v; t.ldv = ldv; t.o = (bf16*)out; t.ldo = ldo;
  t.B = B; t.H = H; t.T = T; t.scale = scale;
  return attn_launch(t, (hipStream_t)stream);
}
extern "C" size_t dmx_trocr_dec_prefill_lm_loss_workspace_bytes(int M, int V) {
  return (M >= 1 && M <= kMaxRows && V >= 1) ? lm_ws_bytes(M, V) : 0;
}
extern "C" int dmx_trocr_dec_prefill_lm_loss(const void* x, int M, int K, const void* w, int V, const long long* labels, int ignore_index,
                                             float* token_logprob, int* argmax, float* logits, int ld_logits,
                                             void* ws, size_t ws_bytes, dmx_stream_t stream) {
  DMX_REQUIRE(x && w && ws && (labels || argmax || logits), "trocr_dec_prefill_lm_loss: null argument");
  DMX_REQUIRE(M >= 1 && M <= kMaxRows && V >= 1, "trocr_dec_prefill_lm_loss: M=%d V=%d", M, V);
  DMX_REQUIRE(ws_bytes >= lm_ws_bytes(M, V), "trocr_dec_prefill_lm_loss: workspace %zu < %zu bytes", ws_bytes, lm_ws_bytes(M, V));
  PfLm q{};
  q.x = (const bf16*)x; q.ldx = K; q.w = (const bf16*)w; q.ldw = K; q.M = M; q.V = V; q.K = K; q.labels = labels; q.ignore = ignore_index;
  q.logits = logits; q.ldl = ld_logits; q.logp = token_logprob; q.amax = argmax;
  return lm_launch(q, ws, (hipStream_t)stream);
}
