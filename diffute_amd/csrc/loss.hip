// The weighted training objective of the denoiser (dmx_diffusion_loss, include/diffute_hip.h): Min-SNR-gamma sample weights, an emphasis on
// the text box, the epsilon / v target, the gradient with respect to the prediction and the per-sample sums, from the tensors the training
// step already holds.  Neither a target nor a weight tensor is materialised.  Two launches: per-block partial sums, then one block that
// folds them.  Compiled with -ffp-contract=off and written with explicit _rn ops: every number is one rounded fp32 operation in the order
// the header gives, so a sample's gradient row and record are the same bits alone or as row b of any batch, and from run to run.
//
// Reduction shape (DMX_LOSS_CHUNK = 2048 elements of one sample per block, 256 threads):
//   thread t of chunk j adds elements j*2048 + {0,1024} + 4 t + {0,1,2,3} in that order           8 serial adds
//   the 256 thread sums are folded by a binary tree in LDS                                          8 adds
//   the ceil(C*hw / 2048) chunk sums of a sample are added serially by one thread of the fold       ceil(C*hw / 2048) adds
// so a term passes through at most k = 16 + ceil(C*hw / 2048) additions (24 at 4 x 64 x 64).  Which elements a thread owns never depends on
// whether it reads them as one 16-byte access or as scalars: the vector path is taken per sample where the sample's first element is
// 16-byte aligned in every tensor, the quad that crosses the end of the span is always scalar.
#include "common.h"
#include "kernels.h"
#include <cmath>

namespace {
constexpr int LOSS_THREADS = 256;
constexpr int LOSS_PART_FLOATS = 4;             // sq_all, sq_mask, sq_weighted, mask_sum of one chunk

struct LossArgs {
  const float* pred; const float* x0; const float* noise; const float* mask; const int64_t* timesteps;
  const float* sa; const float* sb; const float* wt;
  float* dpred; float* part;
  int C, hw, T, vpred, chunks;
  float lambda, gs;
  unsigned align_or;                            // the OR of the addresses of pred, x0, noise and dpred (a NULL dpred adds nothing)
};

// the table index of a sample and whether its timestep was inside the tables
__device__ __forceinline__ int loss_timestep(const int64_t* timesteps, int b, int T, bool& in_range) {
  const int64_t t = timesteps[b];
  in_range = t >= 0 && t < (int64_t)T;
  return t < 0 ? 0 : (t >= (int64_t)T ? T - 1 : (int)t);
}

__global__ __launch_bounds__(LOSS_THREADS) void dmx_diffusion_loss_part_kernel(const LossArgs a) {
  __shared__ float red[LOSS_PART_FLOATS][LOSS_THREADS];
  const int b = blockIdx.y, j = blockIdx.x, tid = threadIdx.x;
  const int S = a.C * a.hw;
  bool in_range;
  const int t = loss_timestep(a.timesteps, b, a.T, in_range);
  const float sa = a.sa[t], sb = a.sb[t];
  const float w = in_range ? a.wt[t] : __builtin_nanf("");
  const size_t base = (size_t)b * S;
  const float* mrow = a.mask ? a.mask + (size_t)b * a.hw : nullptr;
  const bool vec = ((a.align_or & 15u) == 0) && ((base & 3) == 0);
  const bool mvec = mrow && (a.hw % 4 == 0) && (((size_t)mrow & 15) == 0);
  float s_all = 0.f, s_mask = 0.f, s_w = 0.f, s_m = 0.f;
#pragma unroll
  for (int it = 0; it < DMX_LOSS_CHUNK / (4 * LOSS_THREADS); ++it) {
    const int i = j * DMX_LOSS_CHUNK + it * 4 * LOSS_THREADS + 4 * tid;          // first element of this thread's quad inside the sample
    if (i >= S) break;
    const int cnt = S - i < 4 ? S - i : 4;
    const bool v4 = vec && cnt == 4;
    float p[4], x[4], nz[4], M[4], g[4];
    if (v4) {
      const float4 pv = *(const float4*)(a.pred + base + i), nv = *(const float4*)(a.noise + base + i);
      p[0] = pv.x; p[1] = pv.y; p[2] = pv.z; p[3] = pv.w; nz[0] = nv.x; nz[1] = nv.y; nz[2] = nv.z; nz[3] = nv.w;
      if (a.vpred) { const float4 xv = *(const float4*)(a.x0 + base + i); x[0] = xv.x; x[1] = xv.y; x[2] = xv.z; x[3] = xv.w; }
    } else {
      for (int e = 0; e < 4; ++e) {
        const bool in = e < cnt;
        p[e] = in ? a.pred[base + i + e] : 0.f; nz[e] = in ? a.noise[base + i + e] : 0.f;
        if (a.vpred) x[e] = in ? a.x0[base + i + e] : 0.f;
      }
    }
    const int pix = i % a.hw;                                                      // pixel of the quad's first element; the mask is broadcast over C
    if (mvec && cnt == 4) {                                                        // hw % 4 == 0: a quad never crosses a channel
      const float4 mv = *(const float4*)(mrow + pix);
      M[0] = mv.x; M[1] = mv.y; M[2] = mv.z; M[3] = mv.w;
    } else {
      for (int e = 0; e < 4; ++e) M[e] = (mrow && e < cnt) ? mrow[(pix + e) % a.hw] : 0.f;
    }
    const int first_channel_end = a.hw - i;                                        // elements of the quad below this offset lie in channel 0
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      if (e < cnt) {
        const float tau = a.vpred ? __fsub_rn(__fmul_rn(sa, nz[e]), __fmul_rn(sb, x[e])) : nz[e];
        const float d = __fsub_rn(p[e], tau);
        const float q = __fmul_rn(d, d);
        const float m = __fadd_rn(1.0f, __fmul_rn(a.lambda, M[e]));
        g[e] = __fmul_rn(__fmul_rn(d, __fmul_rn(w, m)), a.gs);
        s_all = __fadd_rn(s_all, q);
        s_mask = __fadd_rn(s_mask, __fmul_rn(M[e], q));
        s_w = __fadd_rn(s_w, __fmul_rn(m, q));
        if (e < first_channel_end) s_m = __fadd_rn(s_m, M[e]);
      }
    }
    if (a.dpred) {
      if (v4) *(float4*)(a.dpred + base + i) = make_float4(g[0], g[1], g[2], g[3]);
      else for (int e = 0; e < cnt; ++e) a.dpred[base + i + e] = g[e];
    }
  }
  red[0][tid] = s_all; red[1][tid] = s_mask; red[2][tid] = s_w; red[3][tid] = s_m;
  __syncthreads();
  for (int k = LOSS_THREADS / 2; k >= 1; k >>= 1) {
    if (tid < k) {
#pragma unroll
      for (int f = 0; f < LOSS_PART_FLOATS; ++f) red[f][tid] = __fadd_rn(red[f][tid], red[f][tid + k]);
    }
    __syncthreads();
  }
  if (tid < LOSS_PART_FLOATS) a.part[((size_t)b * a.chunks + j) * LOSS_PART_FLOATS + tid] = red[tid][0];
}

// one block: thread b % 256 adds the chunk sums of sample b in chunk order and writes its record; thread 0 then folds the records in row order
__global__ __launch_bounds__(LOSS_THREADS) void dmx_diffusion_loss_fold_kernel(const float* part, const int64_t* timesteps, const float* wt, int B, int T,
                                                                               int chunks, float* records, float* loss, float inv_n) {
  for (int b = threadIdx.x; b < B; b += LOSS_THREADS) {
    float s[LOSS_PART_FLOATS] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < chunks; ++j) {
#pragma unroll
      for (int f = 0; f < LOSS_PART_FLOATS; ++f) s[f] = __fadd_rn(s[f], part[((size_t)b * chunks + j) * LOSS_PART_FLOATS + f]);
    }
    bool in_range;
    const int t = loss_timestep(timesteps, b, T, in_range);
    float* r = records + (size_t)b * DMX_LOSS_ROW_FLOATS;
    r[DMX_LOSS_SQ_ALL] = s[0]; r[DMX_LOSS_SQ_MASK] = s[1]; r[DMX_LOSS_SQ_WEIGHTED] = s[2]; r[DMX_LOSS_MASK_SUM] = s[3];
    r[DMX_LOSS_WEIGHT] = in_range ? wt[t] : __builtin_nanf("");
  }
  __threadfence_block();
  __syncthreads();
  if (threadIdx.x == 0) {
    float acc = 0.f;
    for (int b = 0; b < B; ++b) {
      const float* r = records + (size_t)b * DMX_LOSS_ROW_FLOATS;
      acc = __fadd_rn(acc, __fmul_rn(r[DMX_LOSS_WEIGHT], r[DMX_LOSS_SQ_WEIGHTED]));
    }
    *loss = __fmul_rn(acc, inv_n);
  }
}
}  // namespace

static int loss_chunks(int C, int hw) { return (int)(((size_t)C * hw + DMX_LOSS_CHUNK - 1) / DMX_LOSS_CHUNK); }

size_t dmx_diffusion_loss_ws_bytes(int B, int C, int hw) {
  if (B <= 0 || C <= 0 || hw <= 0) return 0;
  return (size_t)B * loss_chunks(C, hw) * LOSS_PART_FLOATS * sizeof(float);
}

int dmx_diffusion_loss_launch(const float* pred, const float* latents, const float* noise, const float* mask, const int64_t* timesteps,
                              const float* sa, const float* sb, const float* wt, int B, int C, int hw, int T, int v_prediction,
                              float mask_weight, float grad_scale, float* loss, float* records, float* dpred,
                              void* workspace, size_t workspace_bytes, hipStream_t stream) {
  DMX_REQUIRE(pred && latents && noise && timesteps && sa && sb && wt && loss && records, "diffusion_loss: null argument");
  DMX_REQUIRE(B > 0 && C > 0 && hw > 0 && T > 0, "diffusion_loss: B=%d C=%d hw=%d T=%d must be positive", B, C, hw, T);
  DMX_REQUIRE((size_t)C * hw <= ((size_t)1 << 30) && B <= 65535, "diffusion_loss: C*hw=%zu (at most 2^30) or B=%d (at most 65535) too large", (size_t)C * hw, B);
  DMX_REQUIRE(v_prediction == 0 || v_prediction == 1, "diffusion_loss: v_prediction=%d must be 0 or 1", v_prediction);
  DMX_REQUIRE(std::isfinite(mask_weight) && mask_weight >= 0.f, "diffusion_loss: mask_weight=%g must be finite and >= 0", (double)mask_weight);
  DMX_REQUIRE(workspace && workspace_bytes >= dmx_diffusion_loss_ws_bytes(B, C, hw), "diffusion_loss: workspace too small");
  const double N = (double)B * C * hw;
  LossArgs a;
  a.pred = pred; a.x0 = latents; a.noise = noise; a.mask = mask; a.timesteps = timesteps; a.sa = sa; a.sb = sb; a.wt = wt;
  a.dpred = dpred; a.part = (float*)workspace;
  a.C = C; a.hw = hw; a.T = T; a.vpred = v_prediction; a.chunks = loss_chunks(C, hw);
  a.lambda = mask_weight; a.gs = (float)(2.0 * (double)grad_scale / N);
  a.align_or = (unsigned)((size_t)pred | (size_t)latents | (size_t)noise | (size_t)dpred);
  hipLaunchKernelGGL(dmx_diffusion_loss_part_kernel, dim3(a.chunks, B), dim3(LOSS_THREADS), 0, stream, a);
  int rc = dmx_check_launch("dmx_diffusion_loss_part_kernel");
  if (rc) return rc;
  hipLaunchKernelGGL(dmx_diffusion_loss_fold_kernel, dim3(1), dim3(LOSS_THREADS), 0, stream, (const float*)workspace, timesteps, wt, B, T,
                     a.chunks, records, loss, (float)(1.0 / N));
  return dmx_check_launch("dmx_diffusion_loss_fold_kernel");
}

extern "C" size_t dmx_diffusion_loss_workspace_bytes(int B, int C, int hw) { return dmx_diffusion_loss_ws_bytes(B, C, hw); }
extern "C" int dmx_diffusion_loss(const float* pred, const float* latents, const float* noise, const float* mask, const int64_t* timesteps,
                                  const float* sa, const float* sb, const float* wt, int B, int C, int hw, int T, int v_prediction,
                                  float mask_weight, float grad_scale, float* loss, float* records, float* dpred,
                                  void* workspace, size_t workspace_bytes, dmx_stream_t stream) {
  return dmx_diffusion_loss_launch(pred, latents, noise, mask, timesteps, sa, sb, wt, B, C, hw, T, v_prediction, mask_weight, grad_scale, loss, records,
                                   dpred, workspace, workspace_bytes, (hipStream_t)stream);
}
