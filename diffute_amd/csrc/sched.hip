// Scheduler-step and latent glue kernels, fp32 elementwise.
// Compiled with -ffp-contract=off and written with explicit _rn ops in the op order of
// diffusers' DDIMScheduler.step / DDPMScheduler.step so results are bit-identical to the
// fp32 CPU evaluation of the same formulas (scalar coefficients are computed on the host).
// DPMSolverMultistepScheduler.step likewise.  One step is one dmx_sched_row_rec (diffute_amd/schedulers.py plan()): the scalar entries receive it
// by value, the per-row entry of the in-flight engine reads it from the plan array; ddim_elem / ddpm_elem / dpm_elem are the arithmetic and
// sched_span is the one loop around them, so a row is the same bits through either entry.  The guided entry (dmx_sched_step_guided: classifier-free
// guidance, the optional guidance rescale and the update in one launch) runs the same loop on the combined model output (sched_span_g).
#include "common.h"
#include "kernels.h"

// DDIM: x0 = (x - sqrt(1-abar_t)*eps)/sqrt(abar_t); prev = sqrt(abar_p)*x0 + dir*eps (+ std*noise)
__device__ __forceinline__ float ddim_elem(float xv, float ev, bool has_noise, float nz, float sqrt_bt, float sqrt_at, float sqrt_ap, float dir_coef,
                                           float std, int vpred) {
  float x0, pe;
  if (!vpred) {
    x0 = __fdiv_rn(__fsub_rn(xv, __fmul_rn(sqrt_bt, ev)), sqrt_at);
    pe = ev;
  } else {
    x0 = __fsub_rn(__fmul_rn(sqrt_at, xv), __fmul_rn(sqrt_bt, ev));
    pe = __fadd_rn(__fmul_rn(sqrt_at, ev), __fmul_rn(sqrt_bt, xv));
  }
  float prev = __fadd_rn(__fmul_rn(sqrt_ap, x0), __fmul_rn(dir_coef, pe));
  if (has_noise) prev = __fadd_rn(prev, __fmul_rn(std, nz));
  return prev;
}

// DDPM: prev = c0*x0 + c1*x (+ sigma*noise when t>0)
__device__ __forceinline__ float ddpm_elem(float xv, float ev, bool has_noise, float nz, float sqrt_bt, float sqrt_at, float c0, float c1, float sigma,
                                           int vpred) {
  float x0;
  if (!vpred) x0 = __fdiv_rn(__fsub_rn(xv, __fmul_rn(sqrt_bt, ev)), sqrt_at);
  else x0 = __fsub_rn(__fmul_rn(sqrt_at, xv), __fmul_rn(sqrt_bt, ev));
  float prev = __fadd_rn(__fmul_rn(c0, x0), __fmul_rn(c1, xv));
  if (has_noise) prev = __fadd_rn(prev, __fmul_rn(sigma, nz));
  return prev;
}

// add_noise: sa[b]*x0 + sb[b]*noise ; velocity: sa[b]*noise - sb[b]*x0   (per-sample coefficients)
__global__ __launch_bounds__(256) void dmx_add_noise_kernel(const float* x0, const float* noise, const float* sa, const float* sb,
                                                            float* out, int B, size_t per, int velocity) {
  const size_t n = (size_t)B * per;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / per);
    const float a = sa[b], s = sb[b];
    out[i] = velocity ? __fsub_rn(__fmul_rn(a, noise[i]), __fmul_rn(s, x0[i]))
                      : __fadd_rn(__fmul_rn(a, x0[i]), __fmul_rn(s, noise[i]));
  }
}
int dmx_add_noise_launch(const float* x0, const float* noise, const float* sa, const float* sb, float* out,
                         int B, size_t per, int velocity, hipStream_t stream) {
  const size_t n = (size_t)B * per;
  int blocks = (int)((n + 255) / 256); if (blocks > 2048) blocks = 2048; if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(dmx_add_noise_kernel, dim3(blocks), dim3(256), 0, stream, x0, noise, sa, sb, out, B, per, velocity);
  return dmx_check_launch("dmx_add_noise_kernel");
}

// DiagonalGaussianDistribution.sample()/mode() on NCHW fp32 moments [B][2C][HW], then * scale
__global__ __launch_bounds__(256) void dmx_gaussian_sample_kernel(const float* moments, const float* noise, float* out, int B, int C, int HW, float scale) {
  const size_t n = (size_t)B * C * HW;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t b = i / ((size_t)C * HW);
    const size_t r = i - b * (size_t)C * HW;
    const float mean = moments[b * 2 * C * HW + r];
    float v = mean;
    if (noise) {
      float lv = moments[b * 2 * C * HW + (size_t)C * HW + r];
      lv = fminf(fmaxf(lv, -30.0f), 20.0f);
      const float sd = expf(__fmul_rn(0.5f, lv));
      v = __fadd_rn(mean, __fmul_rn(sd, noise[i]));
    }
    out[i] = __fmul_rn(v, scale);
  }
}
int dmx_gaussian_sample_launch(const float* moments, const float* noise, float* out, int B, int C, int HW, float scale, hipStream_t stream) {
  const size_t n = (size_t)B * C * HW;
  int blocks = (int)((n + 255) / 256); if (blocks > 2048) blocks = 2048; if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(dmx_gaussian_sample_kernel, dim3(blocks), dim3(256), 0, stream, moments, noise, out, B, C, HW, scale);
  return dmx_check_launch("dmx_gaussian_sample_kernel");
}

// DPM-Solver++ multistep (Lu et al. 2022, Alg. 2; DPMSolverMultistepScheduler.step of diffusers >=0.15), orders 1-3.  Per element:
//   m0 = (x - sigma_s0*eps)/alpha_s0  (eps)  |  alpha_s0*x - sigma_s0*v  (v_prediction)      -> x0_out (the caller's history)
//   order 1: prev = c_x*x - c_m0*m0
//   order 2: D1 = inv_r0*(m0 - m1);                                              prev = c_x*x - c_m0*m0 + c_d1*D1
//   order 3: D1_0 = inv_r0*(m0 - m1), D1_1 = inv_r1*(m1 - m2), D1 = D1_0 + w*(D1_0 - D1_1), D2 = inv_r01*(D1_0 - D1_1);
//            prev = c_x*x - c_m0*m0 + c_d1*D1 - c_d2*D2
// c_d1 carries the sign of its term (midpoint: -(0.5*c_m0); fsub(a, b*c) == fadd(a, (-b)*c) exactly in round-to-nearest).
__device__ __forceinline__ float dpm_elem(float x, float e, float m1, float m2, float& m0, int order, const dmx_dpm_coefs& c, int vpred) {
  m0 = !vpred ? __fdiv_rn(__fsub_rn(x, __fmul_rn(c.sigma_s0, e)), c.alpha_s0)
              : __fsub_rn(__fmul_rn(c.alpha_s0, x), __fmul_rn(c.sigma_s0, e));
  float prev = __fsub_rn(__fmul_rn(c.c_x, x), __fmul_rn(c.c_m0, m0));
  if (order == 2) {
    const float d1 = __fmul_rn(c.inv_r0, __fsub_rn(m0, m1));
    prev = __fadd_rn(prev, __fmul_rn(c.c_d1, d1));
  } else if (order == 3) {
    const float d10 = __fmul_rn(c.inv_r0, __fsub_rn(m0, m1));
    const float d11 = __fmul_rn(c.inv_r1, __fsub_rn(m1, m2));
    const float dd = __fsub_rn(d10, d11);
    const float d1 = __fadd_rn(d10, __fmul_rn(c.r0_over_r01, dd));
    const float d2 = __fmul_rn(c.inv_r01, dd);
    prev = __fsub_rn(__fadd_rn(prev, __fmul_rn(c.c_d1, d1)), __fmul_rn(c.c_d2, d2));
  }
  return prev;
}

// ---- the one loop around the three per-element updates.  One SPAN is n elements under one record: the whole tensor of a scalar entry, or one row
// of the in-flight engine (diffute_amd/inflight.py).  float4 where every slab pointer of THIS span is 16-byte aligned (a row's length need not be
// a multiple of 4, so the rows of one launch differ), the n % 4 tail - or the whole span otherwise - by scalar accesses of the grid's first
// threads.  nz == nullptr: no noise term (always for DPM-Solver++).  m0 / m1 / m2: this step's data prediction (written) and the previous two
// (read where the order asks for them), DPM-Solver++ only.  out may be x: every element is read before it is written, by the same thread.
static_assert(sizeof(dmx_sched_row_rec) == 88, "dmx_sched_row_rec: the host packs 88-byte records (diffute_amd/_cabi.py SchedRowRec)");
// whether a span takes the float4 path: every slab it touches is 16-byte aligned.  Which slabs those are is decided HERE, for the kernel and for
// the host launcher that sizes the grid: x, eps, out; DDIM / DDPM the noise where given; DPM-Solver++ m0 and the previous predictions its order reads.
__host__ __device__ __forceinline__ bool sched_span_aligned(bool dpm, int order, const float* x, const float* eps, const float* nz, const float* m1,
                                                            const float* m2, const float* m0, const float* out) {
  const uintptr_t bits = (uintptr_t)x | (uintptr_t)eps | (uintptr_t)out | (dpm ? (uintptr_t)m0 : (uintptr_t)nz) |
                         (dpm && order >= 2 ? (uintptr_t)m1 : 0) | (dpm && order >= 3 ? (uintptr_t)m2 : 0);
  return (bits & 15) == 0;
}
// GUIDED (dmx_sched_step_guided): `eps` is the conditional model output and G.eu the unconditional one; the update runs on their
// classifier-free combination (guided_eps) and the result is stored twice, to out and to G.out2.  Not GUIDED: G is never read.
struct sched_guide {
  const float* eu; float* out2;                // the unconditional model output of the span; the second copy of prev_sample
  float scale, rescale, one_minus_rescale, k;  // k: the span's std(ec) / std(g) (guided_ratio), read only when rescale != 0
};
// g = eu + scale * (ec - eu); rescale != 0 (Lin et al. 2023, diffusers' rescale_noise_cfg): rescale * (g * k) + (1 - rescale) * g
__device__ __forceinline__ float guided_mix(float ec, float eu, float scale) { return __fadd_rn(eu, __fmul_rn(scale, __fsub_rn(ec, eu))); }
__device__ __forceinline__ float guided_eps(float ec, float eu, const sched_guide& G) {
  const float g = guided_mix(ec, eu, G.scale);
  if (G.rescale == 0.f) return g;
  return __fadd_rn(__fmul_rn(G.rescale, __fmul_rn(g, G.k)), __fmul_rn(G.one_minus_rescale, g));
}
template <int KIND, bool GUIDED>
__device__ __forceinline__ void sched_span_g(const dmx_sched_row_rec& r, const float* x, const float* eps, const float* nz, const float* m1,
                                             const float* m2, float* m0, float* out, size_t n, int vpred, const sched_guide& G) {
  constexpr bool DPM = KIND == DMX_SCHED_DPMPP;
  const int order = DPM ? r.order : 0;
  const bool has_noise = !DPM && nz != nullptr;
  auto elem = [&](float xv, float ev, float nv, float a1, float a2, float& d0) -> float {
    if (KIND == DMX_SCHED_DDIM) return ddim_elem(xv, ev, has_noise, nv, r.c[0], r.c[1], r.c[2], r.c[3], r.c[4], vpred);
    if (KIND == DMX_SCHED_DDPM) return ddpm_elem(xv, ev, has_noise, nv, r.c[0], r.c[1], r.c[2], r.c[3], r.c[4], vpred);
    return dpm_elem(xv, ev, a1, a2, d0, order, r.dpm, vpred);
  };
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  size_t done = 0;
  if (sched_span_aligned(DPM, order, x, eps, nz, m1, m2, m0, out) && (!GUIDED || (((uintptr_t)G.eu | (uintptr_t)G.out2) & 15) == 0)) {
    const size_t n4 = n / 4;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (size_t i = tid; i < n4; i += stride) {
      const float4 xv = reinterpret_cast<const float4*>(x)[i];
      float4 ev = reinterpret_cast<const float4*>(eps)[i];
      if (GUIDED) {
        const float4 uv = reinterpret_cast<const float4*>(G.eu)[i];
        ev.x = guided_eps(ev.x, uv.x, G); ev.y = guided_eps(ev.y, uv.y, G); ev.z = guided_eps(ev.z, uv.z, G); ev.w = guided_eps(ev.w, uv.w, G);
      }
      const float4 nv = has_noise ? reinterpret_cast<const float4*>(nz)[i] : z4;
      const float4 a = order >= 2 ? reinterpret_cast<const float4*>(m1)[i] : z4;
      const float4 c = order >= 3 ? reinterpret_cast<const float4*>(m2)[i] : z4;
      float4 d0 = z4, p;
      p.x = elem(xv.x, ev.x, nv.x, a.x, c.x, d0.x);
      p.y = elem(xv.y, ev.y, nv.y, a.y, c.y, d0.y);
      p.z = elem(xv.z, ev.z, nv.z, a.z, c.z, d0.z);
      p.w = elem(xv.w, ev.w, nv.w, a.w, c.w, d0.w);
      if (DPM) reinterpret_cast<float4*>(m0)[i] = d0;
      reinterpret_cast<float4*>(out)[i] = p;
      if (GUIDED) reinterpret_cast<float4*>(G.out2)[i] = p;
    }
    done = n4 * 4;
  }
  for (size_t i = done + tid; i < n; i += stride) {
    float d0 = 0.f;
    const float xv = x[i], ec = eps[i];
    const float ev = GUIDED ? guided_eps(ec, G.eu[i], G) : ec;
    const float p = elem(xv, ev, has_noise ? nz[i] : 0.f, order >= 2 ? m1[i] : 0.f, order >= 3 ? m2[i] : 0.f, d0);
    if (DPM) m0[i] = d0;
    out[i] = p;
    if (GUIDED) G.out2[i] = p;
  }
}
template <int KIND>
__device__ __forceinline__ void sched_span(const dmx_sched_row_rec& r, const float* x, const float* eps, const float* nz, const float* m1,
                                           const float* m2, float* m0, float* out, size_t n, int vpred) {
  sched_span_g<KIND, false>(r, x, eps, nz, m1, m2, m0, out, n, vpred, sched_guide{});
}
// one of three instantiations by the runtime kind
#define DMX_SCHED_LAUNCH(kind, kernel, grid, ...)                                                                                   \
  do {                                                                                                                              \
    if ((kind) == DMX_SCHED_DDIM) hipLaunchKernelGGL(kernel<DMX_SCHED_DDIM>, grid, dim3(256), 0, stream, __VA_ARGS__);               \
    else if ((kind) == DMX_SCHED_DDPM) hipLaunchKernelGGL(kernel<DMX_SCHED_DDPM>, grid, dim3(256), 0, stream, __VA_ARGS__);          \
    else hipLaunchKernelGGL(kernel<DMX_SCHED_DPMPP>, grid, dim3(256), 0, stream, __VA_ARGS__);                                       \
  } while (0)

// the scalar entries (dmx_sched_step_ddim / _ddpm / _dpmpp): one span, the record travels by value as a kernel argument.  The noise term is
// added when `noise` is given (the record's use_noise is the per-row form's); out may differ from x; x0_out is DPM-Solver++'s m0.
template <int KIND>
__global__ __launch_bounds__(256) void dmx_sched_step_kernel(dmx_sched_row_rec r, const float* x, const float* eps, const float* noise,
                                                             const float* m1, const float* m2, float* x0_out, float* out, size_t n, int vpred) {
  sched_span<KIND>(r, x, eps, noise, m1, m2, x0_out, out, n, vpred);
}
int dmx_sched_step_launch(int kind, const dmx_sched_row_rec& r, const float* x, const float* eps, const float* noise, const float* m1,
                          const float* m2, float* x0_out, float* out, size_t n, int vpred, hipStream_t stream) {
  // the grid is sized for the path the kernel will take
  const bool dpm = kind == DMX_SCHED_DPMPP;
  const size_t work = sched_span_aligned(dpm, dpm ? r.order : 0, x, eps, noise, m1, m2, x0_out, out) ? (n + 3) / 4 : n;
  int blocks = (int)((work + 255) / 256); if (blocks > 2048) blocks = 2048; if (blocks < 1) blocks = 1;
  DMX_SCHED_LAUNCH(kind, dmx_sched_step_kernel, dim3(blocks), r, x, eps, noise, m1, m2, x0_out, out, n, vpred);
  return dmx_check_launch("dmx_sched_step_kernel");
}

// the per-row form (dmx_sched_step_rows): grid (chunks of a row, row), one record per block.  Row b runs plan[row_index[b]] in place
// (row_index[b] < 0: idle - the block returns before it reads or writes anything of the row), with the noise term only where the record asks
// for it.  hist [n_hist][B][per]: the DPM-Solver++ ring; the record names the slot it writes (ring_w) and the two it reads (ring_m1, ring_m2).
// The span is the scalar entries', so an active row equals the scalar entry run on that row alone, bit for bit.
// the history slices of row b under record r -> false: a record the ring cannot serve (the row is left alone).  Not DPM-Solver++: no slices.
template <int KIND>
__device__ __forceinline__ bool sched_row_ring(const dmx_sched_row_rec& r, float* hist, int n_hist, int B, int b, size_t per, float*& m0,
                                               const float*& m1, const float*& m2) {
  m0 = nullptr; m1 = nullptr; m2 = nullptr;
  if (KIND != DMX_SCHED_DPMPP) return true;
  const int order = r.order;
  if (order < 1 || order > n_hist || order > 3 || r.ring_w < 0 || r.ring_w >= n_hist) return false;
  m0 = hist + ((size_t)r.ring_w * B + b) * per;
  if (order >= 2) { if (r.ring_m1 < 0 || r.ring_m1 >= n_hist || r.ring_m1 == r.ring_w) return false; m1 = hist + ((size_t)r.ring_m1 * B + b) * per; }
  if (order >= 3) { if (r.ring_m2 < 0 || r.ring_m2 >= n_hist || r.ring_m2 == r.ring_w) return false; m2 = hist + ((size_t)r.ring_m2 * B + b) * per; }
  return true;
}
template <int KIND>
__global__ __launch_bounds__(256) void dmx_sched_rows_kernel(float* x, const float* eps, const float* noise, float* hist, int n_hist,
                                                             const dmx_sched_row_rec* plan, const int* row_index, int B, size_t per, int vpred) {
  const int b = blockIdx.y;
  const int idx = row_index[b];
  if (idx < 0) return;
  const dmx_sched_row_rec r = plan[idx];
  float* m0; const float* m1; const float* m2;
  if (!sched_row_ring<KIND>(r, hist, n_hist, B, b, per, m0, m1, m2)) return;
  float* xr = x + (size_t)b * per;
  sched_span<KIND>(r, xr, eps + (size_t)b * per, noise != nullptr && r.use_noise != 0 ? noise + (size_t)b * per : nullptr, m1, m2, m0, xr, per, vpred);
}
int dmx_sched_rows_launch(float* x, const float* eps, const float* noise, float* hist, int n_hist, const dmx_sched_row_rec* plan,
                          const int* row_index, int B, size_t per, int kind, int vpred, hipStream_t stream) {
  const size_t work = (per + 3) / 4;
  int chunks = (int)((work + 255) / 256); if (chunks > 512) chunks = 512; if (chunks < 1) chunks = 1;
  DMX_SCHED_LAUNCH(kind, dmx_sched_rows_kernel, dim3(chunks, B), x, eps, noise, hist, n_hist, plan, row_index, B, per, vpred);
  return dmx_check_launch("dmx_sched_rows_kernel");
}
#undef DMX_SCHED_LAUNCH

// ---- the guided step (dmx_sched_step_guided): classifier-free guidance, the optional guidance rescale and the scheduler update of B samples
// in one launch.  eps [2B][per]: rows [0,B) conditional, [B,2B) unconditional; x [2B][per]: sample b is read from row b only and prev_sample
// is stored to row b AND row B + b (the next 2B-row forward needs no copy; an element is read before it is written, by the same thread);
// noise / hist [.][B][per].  The record travels by value; the host entry has refused a ring it cannot be served from.
// One block row per sample (blockIdx.y).  rescale == 0: grid (chunks, B) of 256 threads, the span of the per-row kernel.  rescale != 0: grid
// (1, B) of 1024 threads; the block first reduces the sample's two standard deviations (guided_ratio), then runs the same span.
//
// guided_ratio: k = std(ec) / std(g), both UNBIASED over the sample's n elements, g = guided_mix recomputed from (ec, eu) exactly as the span
// recomputes it.  Two passes - the means, then the centred squares (never E[x^2] - E[x]^2) - each in fp32 and in a FIXED order, so the result
// is the same bits on every run: a thread sums its elements in index order (float4 i = tid, tid + T, ..: lanes x, y, z, w in turn; then the
// n % 4 tail - or everything, unaligned - as scalars i = tid, tid + T, ..), a wave combines its 64 partials by an xor butterfly (32, 16, .. 1:
// fp32 addition is commutative, so every lane holds the same bits), and every thread adds the waves' partials from LDS in wave order.  No
// atomics.  std(g) == 0 gives k = inf (or NaN for 0 / 0) and propagates, as in diffusers.
__device__ __forceinline__ float2 guided_block_sum2(float a, float b, float2* sh) {
  for (int o = 32; o > 0; o >>= 1) { a = __fadd_rn(a, __shfl_xor(a, o)); b = __fadd_rn(b, __shfl_xor(b, o)); }
  __syncthreads();                                        // (the previous round's reads of sh are done)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = make_float2(a, b);
  __syncthreads();
  float2 s = make_float2(0.f, 0.f);
  for (int w = 0; w < (int)(blockDim.x >> 6); w++) { s.x = __fadd_rn(s.x, sh[w].x); s.y = __fadd_rn(s.y, sh[w].y); }
  return s;
}
// sum over the row of f(ec, g) -> (x, y) contributions, the calling block's threads in the order above
template <class F>
__device__ __forceinline__ float2 guided_row_sum2(const float* ec, const float* eu, size_t n, float scale, float2* sh, F f) {
  float a = 0.f, b = 0.f;
  auto add = [&](float c, float u) { const float2 v = f(c, guided_mix(c, u, scale)); a = __fadd_rn(a, v.x); b = __fadd_rn(b, v.y); };
  size_t done = 0;
  if ((((uintptr_t)ec | (uintptr_t)eu) & 15) == 0) {
    const size_t n4 = n / 4;
    for (size_t i = threadIdx.x; i < n4; i += blockDim.x) {
      const float4 c = reinterpret_cast<const float4*>(ec)[i], u = reinterpret_cast<const float4*>(eu)[i];
      add(c.x, u.x); add(c.y, u.y); add(c.z, u.z); add(c.w, u.w);
    }
    done = n4 * 4;
  }
  for (size_t i = done + threadIdx.x; i < n; i += blockDim.x) add(ec[i], eu[i]);
  return guided_block_sum2(a, b, sh);
}
__device__ __forceinline__ float guided_ratio(const float* ec, const float* eu, size_t n, float scale, float2* sh) {
  const float2 s = guided_row_sum2(ec, eu, n, scale, sh, [](float c, float g) { return make_float2(c, g); });
  const float mc = __fdiv_rn(s.x, (float)n), mg = __fdiv_rn(s.y, (float)n);
  const float2 q = guided_row_sum2(ec, eu, n, scale, sh, [=](float c, float g) {
    const float dc = __fsub_rn(c, mc), dg = __fsub_rn(g, mg);
    return make_float2(__fmul_rn(dc, dc), __fmul_rn(dg, dg));
  });
  const float nm1 = (float)(n - 1);
  return __fdiv_rn(__fsqrt_rn(__fdiv_rn(q.x, nm1)), __fsqrt_rn(__fdiv_rn(q.y, nm1)));
}
template <int KIND>
__global__ __launch_bounds__(1024) void dmx_sched_guided_kernel(dmx_sched_row_rec r, float* x, const float* eps, const float* noise, float* hist,
                                                                float scale, float rescale, float one_minus_rescale, float* ratio_out, int B,
                                                                size_t per, int vpred) {
  __shared__ float2 sh[16];
  const int b = blockIdx.y;
  float* m0 = nullptr; const float* m1 = nullptr; const float* m2 = nullptr;
  if (KIND == DMX_SCHED_DPMPP) {
    m0 = hist + ((size_t)r.ring_w * B + b) * per;
    if (r.order >= 2) m1 = hist + ((size_t)r.ring_m1 * B + b) * per;
    if (r.order >= 3) m2 = hist + ((size_t)r.ring_m2 * B + b) * per;
  }
  const float* ec = eps + (size_t)b * per;
  sched_guide G{eps + ((size_t)B + b) * per, x + ((size_t)B + b) * per, scale, rescale, one_minus_rescale, 1.f};
  if (rescale != 0.f) {                                   // (uniform over the launch: the grid is (1, B) then)
    G.k = guided_ratio(ec, G.eu, per, scale, sh);
    if (ratio_out != nullptr && threadIdx.x == 0) ratio_out[b] = G.k;
  }
  float* xr = x + (size_t)b * per;
  sched_span_g<KIND, true>(r, xr, ec, noise != nullptr ? noise + (size_t)b * per : nullptr, m1, m2, m0, xr, per, vpred, G);
}
int dmx_sched_guided_launch(int kind, const dmx_sched_row_rec& r, float* x, const float* eps, const float* noise, float* hist, float scale,
                            float rescale, float one_minus_rescale, float* ratio_out, int B, size_t per, int vpred, hipStream_t stream) {
  const size_t work = (per + 3) / 4;
  int chunks = (int)((work + 255) / 256); if (chunks > 512) chunks = 512; if (chunks < 1) chunks = 1;
  const dim3 grid(rescale != 0.f ? 1 : chunks, B), block(rescale != 0.f ? 1024 : 256);
  if (kind == DMX_SCHED_DDIM)
    hipLaunchKernelGGL(dmx_sched_guided_kernel<DMX_SCHED_DDIM>, grid, block, 0, stream, r, x, eps, noise, hist, scale, rescale, one_minus_rescale, ratio_out, B, per, vpred);
  else if (kind == DMX_SCHED_DDPM)
    hipLaunchKernelGGL(dmx_sched_guided_kernel<DMX_SCHED_DDPM>, grid, block, 0, stream, r, x, eps, noise, hist, scale, rescale, one_minus_rescale, ratio_out, B, per, vpred);
  else
    hipLaunchKernelGGL(dmx_sched_guided_kernel<DMX_SCHED_DPMPP>, grid, block, 0, stream, r, x, eps, noise, hist, scale, rescale, one_minus_rescale, ratio_out, B, per, vpred);
  return dmx_check_launch("dmx_sched_guided_kernel");
}

// ---- the per-row guided step (dmx_sched_step_rows_guided): the per-row form for an engine whose rows are plain or halves of a guided pair.
// guide [B]: row b's role.  One block row per engine row; every early return below depends on b alone, so a block leaves whole (before any
// barrier):
//   idle (row_index[b] < 0)  returns first, whatever guide[b] says: nothing of the row is read or written;
//   PLAIN                    sched_span on plan[row_index[b]], the body of dmx_sched_rows_kernel: the same bits;
//   UNCOND                   returns: its sample slab is written by its partner's block and never read, its noise / history slices are nobody's;
//   COND, partner p          the body of dmx_sched_guided_kernel on (ec = eps[b], eu = eps[p]) with the row's OWN record, scale and rescale,
//                            noise[b] where the record asks for it, the history slices hist[.][b]; prev_sample goes to x[b] and x[p];
//   anything else            (a role outside the enum; a partner outside [0, B), equal to b, on another plan row, not UNCOND, or not pointing
//                            back at b; a record the ring cannot serve) the row is left alone, the per-row kernel's rule for a bad ring.
// Whether a row reduces (its rescale != 0) is per row here, and guided_ratio's summation order depends on the block size: so EVERY launch of
// this entry is grid (1, B) of 1024 threads, the shape dmx_sched_guided_kernel reduces with - k is that entry's bits.  One block per row is
// enough: a row is 16384 floats at 512 px, 4 float4 trips per thread, and the launch is bounded by its latency, not by one block's bandwidth
// (the rescale path); the per-element results do not depend on the grid, so PLAIN and rescale-free rows lose no bit by it.
template <int KIND>
__global__ __launch_bounds__(1024) void dmx_sched_rows_guided_kernel(float* x, const float* eps, const float* noise, float* hist, int n_hist,
                                                                     const dmx_sched_row_rec* plan, const int* row_index, const dmx_guide_row* guide,
                                                                     float* ratio_out, int B, size_t per, int vpred) {
  __shared__ float2 sh[16];
  const int b = blockIdx.y;
  const int idx = row_index[b];
  if (idx < 0) return;
  const dmx_guide_row g = guide[b];
  if (g.role != DMX_GUIDE_PLAIN && g.role != DMX_GUIDE_COND) return;
  const int p = g.partner;
  if (g.role == DMX_GUIDE_COND) {
    if (p < 0 || p >= B || p == b || row_index[p] != idx) return;
    const dmx_guide_row gp = guide[p];
    if (gp.role != DMX_GUIDE_UNCOND || gp.partner != b) return;
  }
  const dmx_sched_row_rec r = plan[idx];
  float* m0; const float* m1; const float* m2;
  if (!sched_row_ring<KIND>(r, hist, n_hist, B, b, per, m0, m1, m2)) return;
  float* xr = x + (size_t)b * per;
  const float* ec = eps + (size_t)b * per;
  const float* nz = noise != nullptr && r.use_noise != 0 ? noise + (size_t)b * per : nullptr;
  if (g.role == DMX_GUIDE_PLAIN) {
    sched_span<KIND>(r, xr, ec, nz, m1, m2, m0, xr, per, vpred);
    return;
  }
  sched_guide G{eps + (size_t)p * per, x + (size_t)p * per, g.scale, g.rescale, g.one_minus_rescale, 1.f};
  if (g.rescale != 0.f) {                                 // (uniform over the block)
    G.k = guided_ratio(ec, G.eu, per, g.scale, sh);
    if (ratio_out != nullptr && threadIdx.x == 0) ratio_out[b] = G.k;
  }
  sched_span_g<KIND, true>(r, xr, ec, nz, m1, m2, m0, xr, per, vpred, G);
}
int dmx_sched_rows_guided_launch(float* x, const float* eps, const float* noise, float* hist, int n_hist, const dmx_sched_row_rec* plan,
                                 const int* row_index, const dmx_guide_row* guide, float* ratio_out, int B, size_t per, int kind, int vpred,
                                 hipStream_t stream) {
  const dim3 grid(1, B), block(1024);
  if (kind == DMX_SCHED_DDIM)
    hipLaunchKernelGGL(dmx_sched_rows_guided_kernel<DMX_SCHED_DDIM>, grid, block, 0, stream, x, eps, noise, hist, n_hist, plan, row_index, guide, ratio_out, B, per, vpred);
  else if (kind == DMX_SCHED_DDPM)
    hipLaunchKernelGGL(dmx_sched_rows_guided_kernel<DMX_SCHED_DDPM>, grid, block, 0, stream, x, eps, noise, hist, n_hist, plan, row_index, guide, ratio_out, B, per, vpred);
  else
    hipLaunchKernelGGL(dmx_sched_rows_guided_kernel<DMX_SCHED_DPMPP>, grid, block, 0, stream, x, eps, noise, hist, n_hist, plan, row_index, guide, ratio_out, B, per, vpred);
  return dmx_check_launch("dmx_sched_rows_guided_kernel");
}
// the guide entries of one request, from kernel arguments (no staging buffer).  guided: rows [b0, b0 + n) COND with partner b + n, rows
// [b0 + n, b0 + 2n) UNCOND with partner b - n, all with the request's scalars; not guided: rows [b0, b0 + n) PLAIN (all-zero entries).
__global__ void dmx_rows_guide_kernel(dmx_guide_row* guide, int b0, int n, int guided, float scale, float rescale, float one_minus_rescale) {
  for (int i = threadIdx.x; i < (guided ? 2 * n : n); i += blockDim.x) {
    dmx_guide_row g{};                                    // PLAIN is the all-zero entry: a zeroed table is a table of PLAIN rows
    if (guided) {
      g.role = i < n ? DMX_GUIDE_COND : DMX_GUIDE_UNCOND;
      g.partner = i < n ? b0 + i + n : b0 + i - n;
      g.scale = scale; g.rescale = rescale; g.one_minus_rescale = one_minus_rescale;
    }
    guide[b0 + i] = g;
  }
}
int dmx_rows_guide_launch(dmx_guide_row* guide, int b0, int n, int guided, float scale, float rescale, float one_minus_rescale, hipStream_t stream) {
  hipLaunchKernelGGL(dmx_rows_guide_kernel, dim3(1), dim3(64), 0, stream, guide, b0, n, guided, scale, rescale, one_minus_rescale);
  return dmx_check_launch("dmx_rows_guide_kernel");
}

// the two device ints of a row: row_index[b] (a plan row, -1 = idle) and row_left[b] (steps still to run).  One block each; the values of an
// admission travel as kernel arguments.
__global__ void dmx_rows_admit_kernel(int* row_index, int* row_left, int b, int plan_base, int n_steps) {
  if (threadIdx.x == 0) { row_index[b] = n_steps > 0 ? plan_base : -1; row_left[b] = n_steps > 0 ? n_steps : 0; }
}
__global__ void dmx_rows_advance_kernel(int* row_index, int* row_left, int B) {
  for (int b = threadIdx.x; b < B; b += blockDim.x) {
    const int idx = row_index[b];
    if (idx < 0) continue;
    const int left = row_left[b] - 1;
    row_left[b] = left;
    row_index[b] = left > 0 ? idx + 1 : -1;
  }
}
int dmx_rows_admit_launch(int* row_index, int* row_left, int b, int plan_base, int n_steps, hipStream_t stream) {
  hipLaunchKernelGGL(dmx_rows_admit_kernel, dim3(1), dim3(64), 0, stream, row_index, row_left, b, plan_base, n_steps);
  return dmx_check_launch("dmx_rows_admit_kernel");
}
int dmx_rows_advance_launch(int* row_index, int* row_left, int B, hipStream_t stream) {
  hipLaunchKernelGGL(dmx_rows_advance_kernel, dim3(1), dim3(64), 0, stream, row_index, row_left, B);
  return dmx_check_launch("dmx_rows_advance_kernel");
}
