// Composition of two back-to-back linears into one weight matrix (the UNet's ff.net.2 -> proj_out fold, unet.hip Fwd::xformer):
//   h4 = g Wf2^T + bf2 + h3 ;  y = h4 Wpo^T + bpo + x   ==>   y = [g | h3] [Wpo Wf2 | Wpo]^T + (Wpo bf2 + bpo) + x
// out [C][K + C] (ld = K + C): row n = [ (Wpo Wf2)[n][0..K) | Wpo[n][0..C) ], b_out[n] = bpo[n] + sum_j Wpo[n][j] bf2[j].
// Inputs are the arena's 16-bit weights; every sum is fp32 in a fixed order (j ascending; the bias: 64 strided partial sums and a
// butterfly), each product element is rounded ONCE to the 16-bit element.  Two plain launches, no allocation, no synchronisation:
// legal inside a stream capture.  Weight preparation, not a hot path: it runs once per weights change.
#include "kernels.h"

namespace {

constexpr int FT = 64;        // output tile: FT x FT, 256 threads of 4 x 4
constexpr int FJ = 16;        // j (inner dimension) per staged slab

// out[n][k] = round16(sum_j a[n][j] * b[j][k]), n < N, k < K, j < J; any sizes (every access is bounds-checked)
__global__ __launch_bounds__(256) void dmx_compose_linear_kernel(const bf16* a, int lda, const bf16* b, int ldb, bf16* out, int ldo, int N, int J, int K) {
  __shared__ __attribute__((aligned(16))) float As[FJ][FT + 4];      // As[j][n]
  __shared__ __attribute__((aligned(16))) float Bs[FJ][FT];          // Bs[j][k]
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  const int n0 = blockIdx.y * FT, k0 = blockIdx.x * FT;
  float acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[r][c] = 0.f;
  for (int j0 = 0; j0 < J; j0 += FJ) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int n = n0 + ty + 16 * i, j = j0 + tx;
      As[tx][ty + 16 * i] = (n < N && j < J) ? (float)a[(size_t)n * lda + j] : 0.f;
      const int k = k0 + (t & 63), jb = j0 + (t >> 6) + 4 * i;
      Bs[(t >> 6) + 4 * i][t & 63] = (jb < J && k < K) ? (float)b[(size_t)jb * ldb + k] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int jj = 0; jj < FJ; ++jj) {
      const f32x4 av = *(const f32x4*)&As[jj][ty * 4];
      const f32x4 bv = *(const f32x4*)&Bs[jj][tx * 4];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] += av[r] * bv[c];
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int n = n0 + ty * 4 + r;
    if (n >= N) continue;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = k0 + tx * 4 + c;
      if (k < K) out[(size_t)n * ldo + k] = (bf16)acc[r][c];
    }
  }
}

// one wave per row n: out[n][K + j] = a[n][j] (the second K segment) and b_out[n] = b1[n] + sum_j a[n][j] * b0[j]
__global__ __launch_bounds__(64) void dmx_compose_tail_kernel(const bf16* a, int lda, const float* b0, const float* b1, bf16* out, int ldo, float* b_out, int N, int J, int K) {
  const int n = blockIdx.x, lane = threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
  for (int j = lane; j < J; j += 64) {
    const bf16 w = a[(size_t)n * lda + j];
    out[(size_t)n * ldo + K + j] = w;
    s += (float)w * b0[j];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  if (lane == 0) b_out[n] = b1[n] + s;
}

}  // namespace

int dmx_compose_linear_launch(const bf16* wpo, const bf16* wf2, const float* bf2, const float* bpo, bf16* w_out, float* b_out, int C, int K, hipStream_t stream) {
  DMX_REQUIRE(wpo && wf2 && bf2 && bpo && w_out && b_out && C > 0 && K > 0, "compose_linear: bad argument (C=%d K=%d)", C, K);
  {                                                    // reads Wpo and Wf2, writes the K product columns (16-bit elements)
    ProfScope ps(PROF_OTHER, stream, 2.0 * C * (double)C * K, 2.0 * ((double)C * C + 2.0 * (double)C * K), "compose linear");
    dmx_profile_note_symbol("dmx_compose_linear_kernel");
    hipLaunchKernelGGL(dmx_compose_linear_kernel, dim3(cdiv(K, FT), cdiv(C, FT)), dim3(256), 0, stream, wpo, C, wf2, K, w_out, K + C, C, C, K);
    if (const int rc = dmx_check_launch("dmx_compose_linear_kernel")) return rc;
  }
  ProfScope ps(PROF_OTHER, stream, 2.0 * C * (double)C, 4.0 * (double)C * C + 12.0 * C, "compose linear tail");      // Wpo read and copied; three fp32 vectors
  dmx_profile_note_symbol("dmx_compose_tail_kernel");
  hipLaunchKernelGGL(dmx_compose_tail_kernel, dim3(C), dim3(64), 0, stream, wpo, C, bf2, bpo, w_out, K + C, b_out, C, C, K);
  return dmx_check_launch("dmx_compose_tail_kernel");
}
