// Low-rank adapters (LoRA) on the UNet's linear weights, merged: the arena holds W' = W0 + sum_j s_j B_j A_j and every forward / backward
// graph runs unchanged (include/diffute_hip.h "LoRA").  Two multi-tensor kernels over a table of dmx_lora_rec, one record per
// (target linear, active adapter), and the entry that packs the merged targets into the weights arena:
//
//   dmx_lora_merge       W'[n][k] = W0[n][k] + sum_j s_j sum_p B_j[n][p] A_j[p][k], fp32, torch layout, into the records' staging destination
//   dmx_lora_grads       dA_j[p][k] = s_j sum_n B_j[n][p] dW[n][k],  dB_j[n][p] = s_j sum_k dW[n][k] A_j[p][k]  from a torch-layout dW
//   dmx_unet_lora_apply  merge, then ParamTable::load of every target (the pack path of dmx_unet_load_param), then dmx_unet_refresh_derived
//
// Every output element is computed by ONE thread (merge), one thread column plus a fixed four-way combine (dA) or one wave with a fixed
// butterfly (dB), in an order that depends only on the record's own N, K, r: results are bit-equal from run to run and do not depend on
// which other records share the launch.  All arithmetic is IEEE fp32 fma / add / mul: an inf or NaN in dW reaches every dA column and dB row
// it takes part in.
#include "unet_model.h"

namespace {

constexpr int LM_ROWS = 16, LM_COLS = 256;      // merge: a block owns 16 rows x 256 columns of one target, a thread one column of it
constexpr int LG_COLS = 64, LG_ROWS = 16;       // grads: a dA block owns 64 columns (4 row slices), a dB block 16 rows (4 per wave)
constexpr int LR_CHUNK = 16;                    // ranks handled per pass

__global__ __launch_bounds__(256) void dmx_lora_merge_kernel(const dmx_lora_rec* __restrict__ recs) {
  const dmx_lora_rec head = recs[blockIdx.y];
  if (head.count <= 0) return;                                        // (only a target's first record owns blocks)
  const int N = head.N, K = head.K;
  const int kt = (K + LM_COLS - 1) / LM_COLS, nt = (N + LM_ROWS - 1) / LM_ROWS;
  if ((int)blockIdx.x >= kt * nt) return;
  const int n0 = ((int)blockIdx.x / kt) * LM_ROWS, k = ((int)blockIdx.x % kt) * LM_COLS + (int)threadIdx.x;
  const bool kin = k < K;
  __shared__ float sB[LM_ROWS][LR_CHUNK];
  float acc[LM_ROWS];
#pragma unroll
  for (int i = 0; i < LM_ROWS; ++i) acc[i] = (kin && n0 + i < N) ? head.W[(size_t)(n0 + i) * K + k] : 0.f;
  for (int j = 0; j < head.count; ++j) {                             // the adapters of this target, in table order
    const dmx_lora_rec rc = recs[blockIdx.y + j];
    float dot[LM_ROWS];
#pragma unroll
    for (int i = 0; i < LM_ROWS; ++i) dot[i] = 0.f;
    for (int p0 = 0; p0 < rc.r; p0 += LR_CHUNK) {
      const int pc = rc.r - p0 < LR_CHUNK ? rc.r - p0 : LR_CHUNK;
      __syncthreads();
      { const int i = (int)threadIdx.x / LR_CHUNK, p = (int)threadIdx.x % LR_CHUNK;
        sB[i][p] = (n0 + i < N && p < pc) ? rc.B[(size_t)(n0 + i) * rc.r + p0 + p] : 0.f; }
      __syncthreads();
      for (int p = 0; p < pc; ++p) {                                   // ascending rank: the element's summation order
        const float a = kin ? rc.A[(size_t)(p0 + p) * K + k] : 0.f;
#pragma unroll
        for (int i = 0; i < LM_ROWS; ++i) dot[i] = fmaf(sB[i][p], a, dot[i]);
      }
    }
#pragma unroll
    for (int i = 0; i < LM_ROWS; ++i) acc[i] = fmaf(rc.s, dot[i], acc[i]);
  }
  if (kin)
#pragma unroll
    for (int i = 0; i < LM_ROWS; ++i)
      if (n0 + i < N) head.dst[(size_t)(n0 + i) * K + k] = acc[i];
}

__global__ __launch_bounds__(256) void dmx_lora_grads_kernel(const dmx_lora_rec* __restrict__ recs) {
  const dmx_lora_rec rc = recs[blockIdx.y];
  const int N = rc.N, K = rc.K, r = rc.r;
  const int ta = (K + LG_COLS - 1) / LG_COLS, tb = (N + LG_ROWS - 1) / LG_ROWS;
  const int t = (int)blockIdx.x;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const float* __restrict__ dW = rc.W;
  if (t < ta) {
    // dA: column k = t*64 + lane; wave w sums the rows of its quarter of [0, N) in ascending order, the four partial sums are combined ((0+1)+2)+3
    __shared__ float red[4][LR_CHUNK][LG_COLS];
    const int k = t * LG_COLS + lane;
    const int per = (N + 3) / 4, n_lo = wave * per, n_hi = n_lo + per < N ? n_lo + per : N;
    for (int p0 = 0; p0 < r; p0 += LR_CHUNK) {
      const int pc = r - p0 < LR_CHUNK ? r - p0 : LR_CHUNK;
      float acc[LR_CHUNK];
#pragma unroll
      for (int p = 0; p < LR_CHUNK; ++p) acc[p] = 0.f;
      if (k < K)
        for (int n = n_lo; n < n_hi; ++n) {
          const float d = dW[(size_t)n * K + k];
          const float* b = rc.B + (size_t)n * r + p0;
#pragma unroll
          for (int p = 0; p < LR_CHUNK; ++p)
            if (p < pc) acc[p] = fmaf(b[p], d, acc[p]);
        }
#pragma unroll
      for (int p = 0; p < LR_CHUNK; ++p) red[wave][p][lane] = acc[p];
      __syncthreads();
      if (wave == 0 && k < K)
        for (int p = 0; p < pc; ++p)
          rc.dst[(size_t)(p0 + p) * K + k] = rc.s * (((red[0][p][lane] + red[1][p][lane]) + red[2][p][lane]) + red[3][p][lane]);
      __syncthreads();
    }
  } else if (t - ta < tb) {
    // dB: wave w owns rows nb .. nb+3; lane l sums columns l, l+64, ... in ascending order, then a fixed shuffle tree over the 64 lanes
    const int nb = (t - ta) * LG_ROWS + wave * 4;
    if (nb >= N) return;
    for (int p0 = 0; p0 < r; p0 += LR_CHUNK) {
      const int pc = r - p0 < LR_CHUNK ? r - p0 : LR_CHUNK;
      float acc[4][LR_CHUNK];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int p = 0; p < LR_CHUNK; ++p) acc[i][p] = 0.f;
      for (int k = lane; k < K; k += 64) {
        float d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) d[i] = nb + i < N ? dW[(size_t)(nb + i) * K + k] : 0.f;
#pragma unroll
        for (int p = 0; p < LR_CHUNK; ++p)
          if (p < pc) {
            const float a = rc.A[(size_t)(p0 + p) * K + k];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i][p] = fmaf(d[i], a, acc[i][p]);
          }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int p = 0; p < LR_CHUNK; ++p) {
          float v = acc[i][p];
          for (int off = 32; off >= 1; off >>= 1) v += __shfl_down(v, off, 64);
          if (lane == 0 && p < pc && nb + i < N) rc.dst2[(size_t)(nb + i) * r + p0 + p] = rc.s * v;
        }
    }
  }
}

// the records a launch reads: every pointer it dereferences is there, and a target's records agree on the target
int check_records(const char* who, const dmx_lora_rec* h, int n, bool grads) {
  for (int i = 0; i < n; ++i) {
    const dmx_lora_rec& q = h[i];
    DMX_REQUIRE(q.A && q.B && q.W && q.dst && (!grads || q.dst2), "%s: record %d: null pointer", who, i);
    DMX_REQUIRE(q.N >= 1 && q.K >= 1 && q.r >= 1, "%s: record %d: N=%d K=%d r=%d", who, i, q.N, q.K, q.r);
    DMX_REQUIRE((const void*)q.W != (const void*)q.dst, "%s: record %d: the destination is the source", who, i);
  }
  if (grads) return DMX_OK;
  for (int i = 0; i < n;) {
    const int c = h[i].count;
    DMX_REQUIRE(c >= 1 && c <= n - i, "%s: record %d opens a target of %d records (%d left)", who, i, c, n - i);
    for (int j = 1; j < c; ++j)
      DMX_REQUIRE(h[i + j].count == 0 && h[i + j].N == h[i].N && h[i + j].K == h[i].K && h[i + j].W == h[i].W && h[i + j].dst == h[i].dst,
                  "%s: record %d does not continue the target opened by record %d", who, i + j, i);
    i += c;
  }
  return DMX_OK;
}

int upload(const char* who, const dmx_lora_rec* h, int n, void* table, size_t table_bytes, hipStream_t s) {
  DMX_REQUIRE(table && table_bytes >= (size_t)n * sizeof(dmx_lora_rec), "%s: the table needs %zu bytes", who, (size_t)n * sizeof(dmx_lora_rec));
  DMX_REQUIRE(n <= 65535, "%s: %d records (at most 65535 per launch)", who, n);
  DMX_HIP(hipMemcpyAsync(table, h, (size_t)n * sizeof(dmx_lora_rec), hipMemcpyHostToDevice, s));
  return DMX_OK;
}

}  // namespace

extern "C" int dmx_lora_merge(const dmx_lora_rec* h_recs, int n_records, void* table, size_t table_bytes, dmx_stream_t stream) {
  if (n_records == 0) return DMX_OK;
  DMX_REQUIRE(h_recs && n_records > 0, "lora_merge: null records");
  if (const int rc = check_records("lora_merge", h_recs, n_records, false)) return rc;
  if (const int rc = upload("lora_merge", h_recs, n_records, table, table_bytes, (hipStream_t)stream)) return rc;
  long long tiles = 1;
  for (int i = 0; i < n_records; ++i)
    if (h_recs[i].count > 0)
      tiles = std::max(tiles, (long long)((h_recs[i].K + LM_COLS - 1) / LM_COLS) * ((h_recs[i].N + LM_ROWS - 1) / LM_ROWS));
  DMX_REQUIRE(tiles <= 0x7fffffffLL, "lora_merge: target too large");
  hipLaunchKernelGGL(dmx_lora_merge_kernel, dim3((unsigned)tiles, (unsigned)n_records), dim3(256), 0, (hipStream_t)stream, (const dmx_lora_rec*)table);
  return dmx_check_launch("dmx_lora_merge_kernel");
}

extern "C" int dmx_lora_grads(const dmx_lora_rec* h_recs, int n_records, void* table, size_t table_bytes, dmx_stream_t stream) {
  if (n_records == 0) return DMX_OK;
  DMX_REQUIRE(h_recs && n_records > 0, "lora_grads: null records");
  if (const int rc = check_records("lora_grads", h_recs, n_records, true)) return rc;
  if (const int rc = upload("lora_grads", h_recs, n_records, table, table_bytes, (hipStream_t)stream)) return rc;
  long long tiles = 1;
  for (int i = 0; i < n_records; ++i)
    tiles = std::max(tiles, (long long)((h_recs[i].K + LG_COLS - 1) / LG_COLS) + (h_recs[i].N + LG_ROWS - 1) / LG_ROWS);
  hipLaunchKernelGGL(dmx_lora_grads_kernel, dim3((unsigned)tiles, (unsigned)n_records), dim3(256), 0, (hipStream_t)stream, (const dmx_lora_rec*)table);
  return dmx_check_launch("dmx_lora_grads_kernel");
}

extern "C" int dmx_unet_lora_apply(dmx_unet* u, const dmx_lora_target* h_targets, int n_targets, const dmx_lora_rec* h_recs, int n_records,
                                   void* table, size_t table_bytes, dmx_stream_t stream) {
  DMX_REQUIRE(u && u->arena && u->finalized, "unet_lora_apply: weights not finalized");
  DMX_REQUIRE(n_targets >= 0 && n_records >= 0 && (n_targets == 0 || h_targets) && (n_records == 0 || h_recs), "unet_lora_apply: null argument");
  std::vector<const float*> src(n_targets);
  int next = 0;
  for (int t = 0; t < n_targets; ++t) {
    const dmx_lora_target& g = h_targets[t];
    DMX_REQUIRE(g.name && g.w0, "unet_lora_apply: target %d: null name or base weight", t);
    const ParamEntry* e = u->pt.find(g.name);
    DMX_REQUIRE(e != nullptr, "unet_lora_apply: unknown parameter '%s'", g.name);
    const PackRule& r = e->rule;
    DMX_REQUIRE(r.kind == PackRule::LINEAR || r.kind == PackRule::GEGLU_W, "unet_lora_apply: '%s' is not a linear weight", g.name);
    src[t] = g.w0;                                                    // no record: the base weight is packed (the adapter is removed)
    if (g.nrec == 0) continue;
    DMX_REQUIRE(g.rec0 == next && g.nrec > 0 && g.nrec <= n_records - g.rec0, "unet_lora_apply: '%s': records [%d, %d) of %d, expected to start at %d",
                g.name, g.rec0, g.rec0 + g.nrec, n_records, next);
    const dmx_lora_rec& h = h_recs[g.rec0];
    DMX_REQUIRE(h.count == g.nrec && h.N == r.rows && h.K == r.cols && h.W == g.w0,
                "unet_lora_apply: '%s' is [%d][%d]: its first record says count %d, [%d][%d]", g.name, r.rows, r.cols, h.count, h.N, h.K);
    src[t] = h.dst;
    next = g.rec0 + g.nrec;
  }
  DMX_REQUIRE(next == n_records, "unet_lora_apply: %d records belong to no target", n_records - next);
  if (const int rc = dmx_lora_merge(h_recs, n_records, table, table_bytes, stream)) return rc;
  for (int t = 0; t < n_targets; ++t)
    if (const int rc = u->pt.load(u->arena, h_targets[t].name, src[t], (hipStream_t)stream)) return rc;
  return dmx_unet_refresh_derived(u, stream);
}
