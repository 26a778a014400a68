// Scheduler-step and latent glue kernels, fp32 elementwise.
// Compiled with -ffp-contract=off and written with explicit _rn ops in the op order of
// diffusers' DDIMScheduler.step / DDPMScheduler.step so results are bit-identical to the
// fp32 CPU evaluation of the same formulas (scalar coefficients are computed on the host).
// DPMSolverMultistepScheduler.step likewise (diffute_amd/schedulers.py step_plan: one coefficient struct per step).
#include "common.h"
#include "kernels.h"
#include "../../include/diffute_hip.h"

// DDIM: x0 = (x - sqrt(1-abar_t)*eps)/sqrt(abar_t); prev = sqrt(abar_p)*x0 + dir*eps (+ std*noise)
// One element of the update; the scalar-timestep kernel and the per-row kernel (dmx_sched_rows_kernel) both call it, so a row is the same bits in either.
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
__global__ __launch_bounds__(256) void dmx_sched_ddim_kernel(const float* x, const float* eps, const float* noise, float* out, size_t n,
                                                             float sqrt_bt, float sqrt_at, float sqrt_ap, float dir_coef, float std, int vpred) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = ddim_elem(x[i], eps[i], noise != nullptr, noise ? noise[i] : 0.f, sqrt_bt, sqrt_at, sqrt_ap, dir_coef, std, vpred);
}
int dmx_sched_ddim_launch(const float* x, const float* eps, const float* noise, float* out, size_t n,
                          float sqrt_bt, float sqrt_at, float sqrt_ap, float dir_coef, float std, int vpred, hipStream_t stream) {
  int blocks = (int)((n + 255) / 256); if (blocks > 2048) blocks = 2048; if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(dmx_sched_ddim_kernel, dim3(blocks), dim3(256), 0, stream, x, eps, noise, out, n, sqrt_bt, sqrt_at, sqrt_ap, dir_coef, std, vpred);
  return dmx_check_launch("dmx_sched_ddim_kernel");
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
__global__ __launch_bounds__(256) void dmx_sched_ddpm_kernel(const float* x, const float* eps, const float* noise, float* out, size_t n,
                                                             float sqrt_bt, float sqrt_at, float c0, float c1, float sigma, int vpred) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = ddpm_elem(x[i], eps[i], noise != nullptr, noise ? noise[i] : 0.f, sqrt_bt, sqrt_at, c0, c1, sigma, vpred);
}
int dmx_sched_ddpm_launch(const float* x, const float* eps, const float* noise, float* out, size_t n,
                          float sqrt_bt, float sqrt_at, float c0, float c1, float sigma, int vpred, hipStream_t stream) {
  int blocks = (int)((n + 255) / 256); if (blocks > 2048) blocks = 2048; if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(dmx_sched_ddpm_kernel, dim3(blocks), dim3(256), 0, stream, x, eps, noise, out, n, sqrt_bt, sqrt_at, c0, c1, sigma, vpred);
  return dmx_check_launch("dmx_sched_ddpm_kernel");
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
// prev may alias x: every element is read before it is written, by the same thread.
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

// VEC: every pointer is 16-byte aligned; float4 over the first n/4*4 elements, the n % 4 tail by the first threads of block 0
template <bool VEC>
__global__ __launch_bounds__(256) void dmx_sched_dpmpp_kernel(const float* x, const float* eps, const float* m1, const float* m2, float* x0_out,
                                                              float* out, size_t n, int order, dmx_dpm_coefs c, int vpred) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  size_t done = 0;
  if (VEC) {
    const size_t n4 = n / 4;
    for (size_t i = tid; i < n4; i += stride) {
      const float4 xv = reinterpret_cast<const float4*>(x)[i], ev = reinterpret_cast<const float4*>(eps)[i];
      const float4 a = order >= 2 ? reinterpret_cast<const float4*>(m1)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 b = order >= 3 ? reinterpret_cast<const float4*>(m2)[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      float4 m0, p;
      p.x = dpm_elem(xv.x, ev.x, a.x, b.x, m0.x, order, c, vpred);
      p.y = dpm_elem(xv.y, ev.y, a.y, b.y, m0.y, order, c, vpred);
      p.z = dpm_elem(xv.z, ev.z, a.z, b.z, m0.z, order, c, vpred);
      p.w = dpm_elem(xv.w, ev.w, a.w, b.w, m0.w, order, c, vpred);
      reinterpret_cast<float4*>(x0_out)[i] = m0;
      reinterpret_cast<float4*>(out)[i] = p;
    }
    done = n4 * 4;
  }
  for (size_t i = done + tid; i < n; i += stride) {
    float m0;
    const float p = dpm_elem(x[i], eps[i], order >= 2 ? m1[i] : 0.f, order >= 3 ? m2[i] : 0.f, m0, order, c, vpred);
    x0_out[i] = m0;
    out[i] = p;
  }
}
int dmx_sched_dpmpp_launch(const float* x, const float* eps, const float* m1, const float* m2, float* x0_out, float* out, size_t n,
                           int order, const dmx_dpm_coefs& c, int vpred, hipStream_t stream) {
  auto a16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  const bool vec = a16(x) && a16(eps) && a16(x0_out) && a16(out) && (order < 2 || a16(m1)) && (order < 3 || a16(m2));
  const size_t work = vec ? (n + 3) / 4 : n;
  int blocks = (int)((work + 255) / 256); if (blocks > 2048) blocks = 2048; if (blocks < 1) blocks = 1;
  if (vec) hipLaunchKernelGGL(dmx_sched_dpmpp_kernel<true>, dim3(blocks), dim3(256), 0, stream, x, eps, m1, m2, x0_out, out, n, order, c, vpred);
  else hipLaunchKernelGGL(dmx_sched_dpmpp_kernel<false>, dim3(blocks), dim3(256), 0, stream, x, eps, m1, m2, x0_out, out, n, order, c, vpred);
  return dmx_check_launch("dmx_sched_dpmpp_kernel");
}

// ---- in-flight batching (diffute_amd/inflight.py): every row of the batch on its own schedule.  Row b runs plan record plan[row_index[b]]
// (row_index[b] < 0: idle - the block returns before it reads or writes anything of the row).  Grid (chunks of a row, row): one record per block.
// Per element the update is ddim_elem / ddpm_elem / dpm_elem above, so an active row equals the scalar entry run on that row alone, bit for bit.
// hist [n_hist][B][per]: the DPM-Solver++ ring; the record names the slot it writes (ring_w) and the two it reads (ring_m1, ring_m2).
// float4 where every slab of THIS row is 16-byte aligned (per need not be a multiple of 4, so rows differ), the per % 4 tail by scalar accesses.
static_assert(sizeof(dmx_sched_row_rec) == 88, "dmx_sched_row_rec: the host packs 88-byte records (diffute_amd/_cabi.py SchedRowRec)");
template <int KIND>
__global__ __launch_bounds__(256) void dmx_sched_rows_kernel(float* x, const float* eps, const float* noise, float* hist, int n_hist,
                                                             const dmx_sched_row_rec* plan, const int* row_index, int B, size_t per, int vpred) {
  const int b = blockIdx.y;
  const int idx = row_index[b];
  if (idx < 0) return;
  const dmx_sched_row_rec r = plan[idx];
  float* xr = x + (size_t)b * per;
  const float* er = eps + (size_t)b * per;
  const bool has_noise = KIND != DMX_SCHED_DPMPP && noise != nullptr && r.use_noise != 0;
  const float* nr = has_noise ? noise + (size_t)b * per : nullptr;
  const int order = KIND == DMX_SCHED_DPMPP ? r.order : 0;
  float* m0r = nullptr; const float* m1r = nullptr; const float* m2r = nullptr;
  if (KIND == DMX_SCHED_DPMPP) {
    if (order < 1 || order > n_hist || order > 3 || r.ring_w < 0 || r.ring_w >= n_hist) return;      // (a record the ring cannot serve: the row is left alone)
    m0r = hist + ((size_t)r.ring_w * B + b) * per;
    if (order >= 2) { if (r.ring_m1 < 0 || r.ring_m1 >= n_hist || r.ring_m1 == r.ring_w) return; m1r = hist + ((size_t)r.ring_m1 * B + b) * per; }
    if (order >= 3) { if (r.ring_m2 < 0 || r.ring_m2 >= n_hist || r.ring_m2 == r.ring_w) return; m2r = hist + ((size_t)r.ring_m2 * B + b) * per; }
  }
  auto elem = [&](float xv, float ev, float nz, float a1, float a2, float& m0) -> float {
    if (KIND == DMX_SCHED_DDIM) return ddim_elem(xv, ev, has_noise, nz, r.c[0], r.c[1], r.c[2], r.c[3], r.c[4], vpred);
    if (KIND == DMX_SCHED_DDPM) return ddpm_elem(xv, ev, has_noise, nz, r.c[0], r.c[1], r.c[2], r.c[3], r.c[4], vpred);
    return dpm_elem(xv, ev, a1, a2, m0, order, r.dpm, vpred);
  };
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  const uintptr_t bits = (uintptr_t)xr | (uintptr_t)er | (uintptr_t)nr | (uintptr_t)m0r | (uintptr_t)m1r | (uintptr_t)m2r;
  size_t done = 0;
  if ((bits & 15) == 0) {
    const size_t n4 = per / 4;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (size_t i = tid; i < n4; i += stride) {
      const float4 xv = reinterpret_cast<const float4*>(xr)[i], ev = reinterpret_cast<const float4*>(er)[i];
      const float4 nz = has_noise ? reinterpret_cast<const float4*>(nr)[i] : z4;
      const float4 a = order >= 2 ? reinterpret_cast<const float4*>(m1r)[i] : z4;
      const float4 c = order >= 3 ? reinterpret_cast<const float4*>(m2r)[i] : z4;
      float4 m0 = z4, p;
      p.x = elem(xv.x, ev.x, nz.x, a.x, c.x, m0.x);
      p.y = elem(xv.y, ev.y, nz.y, a.y, c.y, m0.y);
      p.z = elem(xv.z, ev.z, nz.z, a.z, c.z, m0.z);
      p.w = elem(xv.w, ev.w, nz.w, a.w, c.w, m0.w);
      if (KIND == DMX_SCHED_DPMPP) reinterpret_cast<float4*>(m0r)[i] = m0;
      reinterpret_cast<float4*>(xr)[i] = p;
    }
    done = n4 * 4;
  }
  for (size_t i = done + tid; i < per; i += stride) {
    float m0 = 0.f;
    const float p = elem(xr[i], er[i], has_noise ? nr[i] : 0.f, order >= 2 ? m1r[i] : 0.f, order >= 3 ? m2r[i] : 0.f, m0);
    if (KIND == DMX_SCHED_DPMPP) m0r[i] = m0;
    xr[i] = p;
  }
}
int dmx_sched_rows_launch(float* x, const float* eps, const float* noise, float* hist, int n_hist, const dmx_sched_row_rec* plan,
                          const int* row_index, int B, size_t per, int kind, int vpred, hipStream_t stream) {
  const size_t work = (per + 3) / 4;
  int chunks = (int)((work + 255) / 256); if (chunks > 512) chunks = 512; if (chunks < 1) chunks = 1;
  const dim3 grid(chunks, B);
  if (kind == DMX_SCHED_DDIM) hipLaunchKernelGGL(dmx_sched_rows_kernel<DMX_SCHED_DDIM>, grid, dim3(256), 0, stream, x, eps, noise, hist, n_hist, plan, row_index, B, per, vpred);
  else if (kind == DMX_SCHED_DDPM) hipLaunchKernelGGL(dmx_sched_rows_kernel<DMX_SCHED_DDPM>, grid, dim3(256), 0, stream, x, eps, noise, hist, n_hist, plan, row_index, B, per, vpred);
  else hipLaunchKernelGGL(dmx_sched_rows_kernel<DMX_SCHED_DPMPP>, grid, dim3(256), 0, stream, x, eps, noise, hist, n_hist, plan, row_index, B, per, vpred);
  return dmx_check_launch("dmx_sched_rows_kernel");
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
