/*
 * diffute_hip.h - C-ABI of the MI355X-native (gfx950) DiffUTE hot path.
 *
 * The reference (chenhaoxing/DiffUTE) has no FFI of its own: its hot path is reached
 * through three Python classes of the un-vendored `diffusers` library.  Each entry point
 * below names the reference call site (file:line under /root/reference) whose arithmetic
 * it replaces; INTEGRATION.md shows the Python-side binding (ctypes) a maintainer adds.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless it is named
 *     `h_...` or is a `const char*` / descriptor struct (host memory);
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *   - activations between kernels are NHWC ("pixel-major") bf16 (fp16 in the -DDMX_F16 build, see dmx_element_type);
 *     model inputs / outputs at
 *     the Python boundary stay NCHW fp32 exactly as the reference passes them
 *     (app.ipynb:762, train_diffute_v1.py:731), converted inside the library;
 *   - functions return 0 on success, a negative DMX_ERR_* code otherwise; the message of
 *     the last failure on the calling thread is `dmx_last_error()`;
 *   - the library never allocates model memory: weights arena, context cache and workspace
 *     are caller-provided (sizes from the *_bytes queries).  The only internal allocation
 *     is one 4 KiB zero page used for convolution padding.
 */
#ifndef DIFFUTE_HIP_H
#define DIFFUTE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMX_OK 0
#define DMX_ERR_ARG (-1)
#define DMX_ERR_HIP (-2)
#define DMX_ERR_UNSUPPORTED (-3)
#define DMX_ERR_WORKSPACE (-4)

typedef void* dmx_stream_t;
typedef struct dmx_unet dmx_unet;
typedef struct dmx_vae dmx_vae;

int dmx_version(void);
const char* dmx_last_error(void);
/* Device-side failures.  Kernels that wait for other blocks of their launch (the K-split slab exchange of dmx_conv3x3_gn, the
 * stream-K fix-up of the persistent GEMMs) bound the wait (~40 ms); a block that gives up writes a record into pinned host memory
 * and goes on (the GPU never hangs, the launch's result is invalid).  Every later launch of the library, every graph replay and this
 * poll read the record WITHOUT synchronising and return DMX_ERR_DEVICE (-5) once, with the detail in dmx_last_error().  Call it
 * after your own stream / device synchronisation to cover the last launches. */
int dmx_device_error(void);
/* test support for that channel: one thread raises `code`; `blocks` single-wave blocks that each fill a CU's LDS spin for ticks x 10 ns */
int dmx_test_raise_device_error(int code, dmx_stream_t stream);
int dmx_test_occupy_cus(int blocks, long long ticks, dmx_stream_t stream);
/* The 16-bit storage / MFMA operand type this build of the library computes in: "bf16" (libdiffute_hip.so) or "fp16"
 * (libdiffute_hip_f16.so, the same sources compiled with -DDMX_F16).  Wherever this header says "bf16" for an activation,
 * weight or context buffer it means this element type.  The host mirror loads the fp16 build for a model moved with
 * `.to(dtype=torch.float16)` (vae.to(device, dtype=weight_dtype), train_diffute_v1.py:789-797; BASELINE configs[4]). */
const char* dmx_element_type(void);

/* ------------------------------------------------------------------------------------
 * Test support: the small kernels of the training graphs that have no operator-level entry (the W^T transposes, the
 * gradient add, the row softmax and its backward of the VAE's single-head attention, the 1x1 convolutions between <= 8
 * channels, the backward of the fp32 time-embedding linears, the casts around the posterior mode).  Each entry checks its
 * arguments and forwards to the launch function the training graphs call; tests/test_train_small_gpu.py compares them with
 * fp64.  "16" below is the build's 16-bit element; row strides (ld*) are in elements.
 * ---------------------------------------------------------------------------------- */
/* out[c][r] = in[r][c], 16-bit, R x C -> C x R */
int dmx_test_transpose_bf16(const void* in, int ldin, void* out, int ldout, int R, int C, dmx_stream_t stream);
/* the same for a list of jobs in ONE launch, as *_train_prepare runs its transposes.  `table`: device buffer of table_bytes
 * (>= 40 * njobs, <= 81920) that receives the job table; the entry remembers the table it uploaded last and skips the upload
 * when the next call's jobs are identical.  njobs = 0 (or another `table`) forgets it. */
typedef struct dmx_test_tr_job { const void* in; int ldin; void* out; int ldout; int R, C; } dmx_test_tr_job;
int dmx_test_transpose_batch(const dmx_test_tr_job* h_jobs, int njobs, void* table, size_t table_bytes, dmx_stream_t stream);
/* out = a + b (16-bit, one fp32 add per element); C and the strides multiples of 8 */
int dmx_test_add_bf16(const void* a, int lda, const void* b, int ldb, void* out, int ldo, int rows, int C, dmx_stream_t stream);
/* p (16) = softmax(scale * s) along each row of the fp32 scores; ds (16) = scale * p o (dp - rowsum(dp o p)) */
int dmx_test_softmax_rows(const float* s, int lds, void* p, int ldp, int rows, int n, float scale, dmx_stream_t stream);
int dmx_test_softmax_bwd_rows(const void* p, int ldp, const float* dp, int lddp, void* ds, int ldds, int rows, int n, float scale, dmx_stream_t stream);
/* y[m][o] = bias[o] + sum_i w[o][i] x[m][i], Cin, Cout <= 8; x, w 16-bit, bias fp32 or NULL, y fp32 (out_f32) or 16-bit.
 * Backward: dx (16, or NULL) = dy w, dw[o][i] = sum_m dy[m][o] x[m][i], db[o] = sum_m dy[m][o]; dy, dw, db fp32 */
int dmx_test_pointwise_small_fwd(const void* x, int ldx, const void* w, int ldw, const float* bias, void* y, int ldy, int M, int Cin, int Cout,
                                 int out_f32, dmx_stream_t stream);
size_t dmx_test_pointwise_small_bwd_workspace_bytes(int M, int Cin, int Cout);
int dmx_test_pointwise_small_bwd(const void* x, int ldx, const float* dy, int lddy, const void* w, int ldw, void* dx, int lddx,
                                 float* dw, int lddw, float* db, int M, int Cin, int Cout, void* workspace, size_t workspace_bytes, dmx_stream_t stream);
/* backward of y = w act(x) + b, act = SiLU when silu_in (dmx_linear_small): x [B][K], dy [B][N], dw [N][K], dx [B][K] fp32, w [N][K] 16-bit;
 * dw (+)= dy^T act(x), db[n * db_stride] (+)= sum_b dy[b][n] (with dw only), dx = act'(x) o (dy w).  dw or dx may be NULL. */
int dmx_test_linear_small_bwd(const float* x, int ldx, const float* dy, int lddy, const void* w, int ldw, float* dw, int lddw, float* db, int db_stride,
                              float* dx, int lddx, int B, int N, int K, int silu_in, int accumulate, dmx_stream_t stream);
/* out (16) [M][C] = in (fp32) [M][0:C]; dmom (fp32, dense [M][2C]) = (dz (16) | 0); out (fp32, dense [M][C]) = in (16) */
int dmx_test_slice_cast(const float* in, int ldin, void* out, int ldo, int M, int C, dmx_stream_t stream);
int dmx_test_mode_bwd(const void* dz, int lddz, float* dmom, int M, int C, dmx_stream_t stream);
int dmx_test_bf16_to_f32_rows(const void* in, int ldin, float* out, int M, int C, dmx_stream_t stream);
/* the weight-preparation kernels only the model executors launch (tests/test_weight_pack_gpu.py).  Folded LayerNorm: w_out (16) [N][K] =
 * round16(w_raw (16) [N][K] * gamma[k]), c1[n] = sum_k w_out[n][k], c2[n] = sum_k beta[k] * w_raw[n][k] (+ bias[n], bias may be NULL); K a
 * multiple of 8.  Context cast: out (16) [B][Spad][C] = in [B][S][C] (fp32, or 16-bit when in_is_16), rows >= S zero. */
int dmx_test_ln_fold(const void* w_raw, void* w_out, const float* gamma, const float* beta, const float* bias, float* c1, float* c2,
                     int N, int K, dmx_stream_t stream);
int dmx_test_cast_pad_rows(const void* in, int in_is_16, void* out, int B, int S, int Spad, int C, dmx_stream_t stream);
/* the composition behind dmx_set_ff_fold (tests/test_ff_fold_gpu.py): w_out (16) [C][K + C], row n = [ round16(sum_j wpo[n][j] * wf2[j][k]), k < K |
 * wpo[n][0..C) ], from wpo (16) [C][C] and wf2 (16) [C][K]; b_out[n] = bpo[n] + sum_j wpo[n][j] * bf2[j].  fp32 sums in a fixed order; any C, K. */
int dmx_test_compose_linear(const void* wpo, const void* wf2, const float* bf2, const float* bpo, void* w_out, float* b_out, int C, int K, dmx_stream_t stream);
/* the folded block tail as the UNet walk runs it, on the executor: y (16) [B*HW][C] = [g (16) [B*HW][4C] | h3 (16) [B*HW][C]] wfpo^T + bfpo + x, then
 * t (16) = GroupNorm(y; groups, eps 1e-5, no activation).  mode 0: the GEMM completes y itself; 1: a split-K plan leaves its reduce pass (with bfpo and x)
 * to the GroupNorm; 2: as 1, but x is released before the GroupNorm, which completes y first.  The three give the same bits.  C a multiple of 64. */
/* the exact integer arithmetic of the quad blend (csrc/prepost_quad_blend.h, stated above dmx_paste_color_stats_quads), host-only, no GPU:
 * the edge steps s = floor(E / sqrt(ex^2 + ey^2)) of an edge (ex, ey) at edge function E, saturated to [-M, M] - M for an edge of
 * length 0, which takes part in nothing -, and the threshold of s >= j: the least E with s(E) >= j, by which the kernels know a pixel to
 * be outside or at full weight.  |ex|, |ey| <= 65535, |E| <= 2^33, 1 <= M <= 2 DMX_QUAD_BLEND_MAX + 2, |j| <= 2 DMX_QUAD_BLEND_MAX + 2, an
 * edge with length for the threshold; anything else returns LLONG_MIN.  tests/test_quad_blend_host.py compares both with Python ints at
 * magnitudes no small page reaches. */
long long dmx_test_quad_edge_steps(int ex, int ey, long long E, int M);
long long dmx_test_quad_edge_threshold(int ex, int ey, int j);
size_t dmx_test_folded_tail_gn_workspace_bytes(int B, int HW, int C, int groups, int mode);
int dmx_test_folded_tail_gn(const void* g, const void* h3, const void* x, const void* wfpo, const float* bfpo, const float* gamma, const float* beta,
                            int B, int HW, int C, int groups, int mode, void* y_out, void* t_out, void* workspace, size_t workspace_bytes, dmx_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Operator level.  Used by the parity tests and by the executors.
 * ---------------------------------------------------------------------------------- */

/* K1/K1s/K2/K7/K8/K10: fused implicit-GEMM convolution / linear layer.
 * Replaces torch conv2d / linear / F.interpolate(nearest x2) / torch.cat(dim=1) inside
 * diffusers ResnetBlock2D, Downsample2D, Upsample2D, Attention and FeedForward, reached from
 * unet(...) app.ipynb:814, train_diffute_v1.py:913 and vae.encode/decode app.ipynb:793,819. */
typedef struct dmx_gemm_desc {
  const void* x0; const void* x1;   /* bf16 activations; x1 = second channel range or NULL   */
  int ldx0, ldx1, cx0;              /* row strides (elements); channels taken from x0        */
  int direct;                       /* 1: X row m = activation row m (linear / 1x1 stride 1) */
  int IH, IW, OH, OW;               /* source grid (before x2 upsample) and output grid      */
  int stride, pad, ups, ksize;      /* ksize 1 or 3; pad = top/left pad; ups = nearest x2    */
  int Cin;                          /* channels per tap (cx0 + channels of x1)               */
  int Ktaps;                        /* ksize*ksize*Cin                                       */
  const void* s0; const void* s1;   /* optional fused 1x1 shortcut sources (K - Ktaps chans) */
  int lds0, lds1, cs0;
  const void* w; int ldw;           /* bf16 weights [N][K], K = (tap, channel) contiguous    */
  int M, N, K;
  const float* bias;                /* [N] or NULL                                           */
  const float* rowbias;             /* [M/rows_per_group][ldrb] or NULL (time embedding)     */
  int rows_per_group, ldrb;
  const void* res; int ldres;       /* bf16 residual or NULL                                 */
  void* out; int ldo; int out_f32;  /* bf16 (default) or fp32 output                         */
  int geglu;                        /* 1: weights/bias GEGLU-packed, out[m][j] = a*gelu(b)   */
  int force_tn, force_splitk;       /* 0 = automatic plan; tuning / tests may pin the tile instance (1..16) and split */
  int group_m;                      /* m-tiles per L2 super-tile of the block rasterisation (0 = default) */
  long long* timing;                /* optional device buffer [blocks][4]: per-block start / prologue / loop / end
                                       timestamps in 10 ns ticks (measurement aid), normally NULL */
  int dbg;                          /* measurement aid, must be 0: bit0 skips the MFMA phase, bit1 the DMA refills */
  int act;                          /* 1: exact (erf) GELU after the bias (ViT MLP fc1), bf16 output only             */
  /* Folded LayerNorm (diffusers BasicTransformerBlock norm1/2/3 in front of attn1.to_q|k|v, attn2.to_q, ff.net.0.proj,
   * reached from unet(...) app.ipynb:814): the GEMM that PRODUCES the residual stream also emits, per output row, partial
   * (sum, sum of squares) of its rounded output - rowstats_out [dmx_conv_gemm_rowstats_tiles(d)][M][2] fp32 - and the GEMM
   * that CONSUMES LayerNorm(x) runs on the raw rows with w = W*diag(gamma) and finishes
   * y = rstd*(acc - mean*ln_c1[n]) + ln_c2[n]   (ln_c1[n] = sum_k w[n][k], ln_c2[n] = sum_k beta[k] W[n][k] + bias[n]). */
  float* rowstats_out;              /* producer side, or NULL                                                          */
  const float* ln_stats; int ln_tiles;   /* consumer side: the producer's partials and how many it wrote per row       */
  const float* ln_c1; const float* ln_c2; int ln_C; float ln_eps;   /* ln_C = normalised feature count (= K)           */
  /* GroupNorm statistics from the producer (ResnetBlock2D norm1 / norm2, Transformer2DModel.norm and conv_norm_out behind
   * unet(...), app.ipynb:814, and the same norms of AutoencoderKL): the conv / linear that WRITES a tensor also adds, per
   * (sample, channel), a statistics record of its rounded outputs - four int64 words {sum * 2^20, floor(sumsq * 2^8),
   * (sumsq - that) * 2^40, 0}, exact integer accumulation, no wrap below sumsq = 3.6e16 - into
   * colstats[(sample*N + n)*4 ..] (zero before the call; cs_rows = rows per sample, a multiple of the plan's tile
   * rows - dmx_conv_gemm_colstats_ok(d) says whether the plan this problem gets can do it).  The GroupNorm that READS the
   * tensor is then dmx_groupnorm_from_stats: one apply-only pass, no statistics pass over the tensor. */
  long long* colstats; int cs_rows;
} dmx_gemm_desc;
size_t dmx_conv_gemm_workspace_bytes(const dmx_gemm_desc* d);
int dmx_set_gn_producer_stats(int on);                      /* tuning aid: 0 makes the model executors compute GroupNorm statistics in the
                                                               consumer again (A/B runs inside one process); returns the old setting */
int dmx_conv_gemm_colstats_ok(const dmx_gemm_desc* d);      /* 1 when dmx_conv_gemm(d) can fill d->colstats (d->cs_rows set)      */
int dmx_conv_gemm_rowstats_tiles(const dmx_gemm_desc* d);   /* partials per row that dmx_conv_gemm(d) will write to rowstats_out */
int dmx_conv_gemm(const dmx_gemm_desc* d, void* workspace, size_t workspace_bytes, dmx_stream_t stream);
/* Test support (tests/test_gemm_plan_host.py; declared here because it takes the descriptor): what dmx_conv_gemm(d) would do on a device of
 * n_cus compute units, without a device call and without reading through any pointer of d.  Returns what dmx_conv_gemm returns for the
 * arguments (DMX_ERR_ARG for a problem it refuses, out zeroed) and writes out[12] = {plan id, split-K factor, K-tiles per split, n-tiles,
 * blocks of a persistent plan (0: classic), workspace bytes, grid x, grid y, block threads, dynamic LDS bytes without and with weight-prefetch
 * ranges, dmx_conv_gemm_colstats_ok(d)}.  d->ups = 2 stands for the problem dmx_conv_ups2x builds (ksize 2, K = 4 Cin, M = 4 rows per source pixel). */
int dmx_test_gemm_plan(const dmx_gemm_desc* d, int n_cus, long long* out);

/* K10 (Upsample2D: F.interpolate(scale 2, nearest) + conv3x3, the diffusers call inside pipeline_diffute.py's unet(...),
 * SURVEY.md 8a) as four 2x2 convolutions on the SOURCE grid, one per output pixel parity, with the 3x3 taps that land on
 * the same source pixel summed beforehand: 4/9 of the multiply-adds of the direct form, same result up to one bf16
 * rounding of the summed taps.  phase_weights = [4][N][4*Cin] bf16 from dmx_pack_ups_phase_weights (w3 = taps-major
 * packed 3x3 weights [N][ldw3] as dmx_pack_conv_weight writes them).  x: NHWC bf16 [B*IH*IW][ldx]; out: NHWC bf16
 * [B*2IH*2IW][ldo]; bias fp32 [N] or NULL. */
int dmx_pack_ups_phase_weights(const void* w3, int ldw3, void* phase_weights, int N, int Cin, dmx_stream_t stream);
size_t dmx_conv_ups2x_workspace_bytes(int B, int IH, int IW, int Cin, int N, int force_tn, int force_splitk);
int dmx_conv_ups2x(const void* x, int ldx, int B, int IH, int IW, int Cin, const void* phase_weights, int N, const float* bias,
                   void* out, int ldo, int force_tn, int force_splitk, void* workspace, size_t workspace_bytes, dmx_stream_t stream);

/* Tuning aid (scripts/tune_in_situ.py): override the tile plan of every GEMM with this (M, N, K, stride, ups) signature
 * (ups: 0, 1, or 2 for the phase-decomposed upsample conv) by tile instance `cfg`
 * (plan id 0..15, the rows of csrc/gemm_tile.h: 0..11 classic tiles, 12..15 persistent stream-K; force_tn = 1 for id 1, 2 for id 0, id + 1 otherwise) and split-K factor; cfg < 0
 * clears all overrides.  Not thread-safe; captured hipGraphs keep the plan they were captured with. */
int dmx_gemm_plan_override(int M, int N, int K, int stride, int ups, int cfg, int splitk);

/* Training: weight gradient of the conv / linear that `d` describes (the forward call's gather
 * fields x0/x1/cx0/direct/IH.../ksize/Cin and M, N; K taken as Ktaps - the fused shortcut is a separate direct call):
 *   dw[n][k] (+)= sum_m dy[m][n] * X[m][k]   fp32, k in the packed (tap, channel) order of the forward weights.
 * Replaces the conv/linear weight-gradient kernels autograd runs under `accelerator.backward(loss)`
 * (train_diffute_v1.py:925).  dmx_colsum gives the bias gradient (groups = 1) and the per-image gradient of the
 * time-embedding row bias (groups = B, rows_per_group = OH*OW). */
size_t dmx_conv_wgrad_workspace_bytes(const dmx_gemm_desc* d, int accumulate);
int dmx_conv_wgrad(const dmx_gemm_desc* d, const void* dy, int lddy, float* dw, int accumulate,
                   void* workspace, size_t workspace_bytes, dmx_stream_t stream);
size_t dmx_colsum_workspace_bytes(int groups, int rows_per_group, int N);
int dmx_colsum(const void* dy, int lddy, int groups, int rows_per_group, int N, float* out, int ldo, int accumulate,
               void* workspace, size_t workspace_bytes, dmx_stream_t stream);

/* K3: GroupNorm (+SiLU) over NHWC bf16; optional virtual channel concat of (x0 | x1).
 * Replaces torch.nn.GroupNorm + SiLU in ResnetBlock2D / Transformer2DModel / VAE blocks. */
size_t dmx_groupnorm_workspace_bytes(int B, int HW, int groups);
int dmx_groupnorm(const void* x0, int ldx0, const void* x1, int ldx1, int c0, int C, int groups,
                  int B, int HW, const float* gamma, const float* beta, float eps, int silu,
                  void* y, int ldy, void* workspace, size_t workspace_bytes, dmx_stream_t stream);
/* GroupNorm (+SiLU) with the statistics taken from the producers of x0 / x1: st0 = colstats of the GEMM that wrote x0
 * ([B][c0][4] int64 records), st1 likewise for x1 ([B][C - c0][4]) or NULL without a second source.  One launch. */
int dmx_groupnorm_from_stats(const void* x0, int ldx0, const void* x1, int ldx1, int c0, int C, int groups,
                             int B, int HW, const float* gamma, const float* beta, float eps, int silu,
                             const long long* st0, const long long* st1, void* y, int ldy, dmx_stream_t stream);

/* K1 + K3 as ONE launch (north_star: "NHWC conv2d with LDS-staged input tiles ... GroupNorm/SiLU fused per-channel in LDS"):
 * conv3x3 (stride 1, pad 1) over a halo tile that is staged ONCE per 64-channel chunk in LDS - the nine taps are shifted LDS
 * fragment reads - with the GroupNorm(32 groups)[+SiLU] in front of it applied to the staged tile in place, from the statistics
 * records of the tensor's producer(s).  Replaces `conv1(nonlinearity(norm1(x)))` / `conv2(nonlinearity(norm2(h)))` (+ conv_shortcut,
 * + the time-embedding add, + the residual add) of every diffusers ResnetBlock2D behind unet(...) /root/reference/app.ipynb:814,
 * train_diffute_v1.py:913 and vae.encode / vae.decode app.ipynb:793,819.
 *   x0 | x1: NHWC input (virtual channel concat; x1 NULL without one), cx0 / Cin multiples of 64; H x W a multiple of 8 x 32 or 16 x 16
 *   gn = 1: y = GroupNorm(x)[SiLU] feeds the conv (padding pixels are zeros of y); st0 / st1 = records [B][channels][4] of x0 / x1
 *   s0 | s1: optional 1x1 shortcut K segment on RAW tensors of the output grid (Csc channels, multiples of 64; 0 = none)
 *   w: [N][ldw] with k = tap*Cin + c, then the shortcut channels (dmx_pack_conv_weight); N a multiple of 160 or of 128
 *   out = conv + bias[n] + rowbias[b*ldrb + n] + res, NHWC; colstats: records of the OUTPUT [B][N][4], added to, or NULL
 * dmx_conv3x3_gn_supported: 1 when the kernel takes the problem (otherwise use dmx_groupnorm + dmx_conv_gemm).
 * dmx_colstats: the statistics records of a tensor whose producer emitted none (one streaming pass; st zero before the call). */
typedef struct dmx_halo_conv_desc {
  const void* x0; const void* x1; int ldx0, ldx1, cx0, Cin;
  int B, H, W;
  int gn, silu, groups; float eps;
  const long long* st0; const long long* st1;
  const float* gamma; const float* beta;
  const void* s0; const void* s1; int lds0, lds1, cs0, Csc;
  const void* w; int ldw; int N;
  const float* bias; const float* rowbias; int ldrb;
  const void* res; int ldres;
  void* out; int ldo;
  long long* colstats;
  int force_split;                  /* 0 = automatic; 1 / 2 / 4 / 8 blocks share the K range of a tile (tests, tuning) */
  int force_bn;                     /* 0 = automatic; 160 / 128 / 80 / 64 output columns per block (tests, tuning) */
  int force_waves;                  /* 0 = automatic; 8 = two-group ping-pong; 4 / 12 = warp-specialised, 4 compute + 4 / 8 loader waves (160 / 128-column tiles, bf16 build) */
  int dbg; long long* timing;       /* measurement aids, 0 / NULL */
} dmx_halo_conv_desc;
int dmx_conv3x3_gn_supported(const dmx_halo_conv_desc* d);
size_t dmx_conv3x3_gn_workspace_bytes(const dmx_halo_conv_desc* d);
int dmx_conv3x3_gn(const dmx_halo_conv_desc* d, void* workspace, size_t workspace_bytes, dmx_stream_t stream);
/* Test support (tests/test_halo_plan_host.py; declared here because it takes the descriptor): what dmx_conv3x3_gn(d) would do on a device of n_cus
 * compute units with dmx_set_exclusive_device(exclusive), dmx_set_halo_peers(peers) and dmx_set_halo_ws(ws), without a device call and without reading
 * through any pointer of d.  Returns what dmx_conv3x3_gn returns for the arguments (DMX_ERR_ARG for a problem it refuses, out zeroed) and writes
 * out[23] = {tile rows, tile columns, output columns per block, the instance's force_waves value, K split, blocks, block threads, dynamic LDS bytes,
 * zeroed flag words, workspace bytes, pixel-tile-major dealing, peers on one XCD, the five counts of the kernel's block decode (tiles per row, per
 * image, pixel tiles, (column tile, slice) combos, channels per group) and its six division constants}. */
int dmx_test_halo_plan(const dmx_halo_conv_desc* d, int n_cus, int exclusive, int peers, int ws, long long* out);
int dmx_colstats(const void* x, int ldx, int B, int HW, int C, long long* st, dmx_stream_t stream);
int dmx_set_halo_conv(int on);      /* tuning aid: 0 makes the model executors use GroupNorm + dmx_conv_gemm everywhere; returns the old setting */
int dmx_set_exclusive_device(int on); /* 1 (default): the library's launches have the GPU to themselves, one stream at a time.  0: other streams or other kernels (micro-batches on
                                       * several streams, a collective on a side stream) may hold CUs while a launch runs: dmx_conv3x3_gn then takes no in-kernel K split (its peers
                                       * must be co-resident; a starved launch raises DMX_ERR_DEVICE) and the executors use GroupNorm + dmx_conv_gemm where a split would be needed.
                                       * Returns the old setting; captured UNet steps are keyed on dmx_plan_epoch(), which it bumps.  The host mirror switches it
                                       * to 0 by itself wherever IT creates the concurrency (denoise(micro_batches > 1), set_gradient_sync with world > 1);
                                       * diffute_amd.set_exclusive_device() is the public setter for everything else (a second model / thread / stream). */
int dmx_get_exclusive_device(void); /* the current setting */
int dmx_plan_epoch(void);           /* counter bumped by every switch that changes which kernels / plans a graph walk uses (every dmx_set_* below and above,
                                     * dmx_gemm_plan_override): part of the key of the captured UNet steps, and what a caller that caches workspace sizes keys on */
int dmx_set_defer_reduce(int on);   /* tuning aid: 0 = a split-K convolution whose output is read first by a GroupNorm runs its own reduce pass (default 1: the GroupNorm's slab
                                     * kernel sums the partial planes in its load stage - bit-identical, one launch less; 2: only inside a resnet, conv1 -> norm2, not conv2 -> the next block's first GroupNorm); returns the old setting */
int dmx_set_halo_peers(int on);     /* 1 (default): the K-split blocks of a dmx_conv3x3_gn tile are dealt to ONE XCD and, once every peer has confirmed its XCC id, exchange their
                                       fp32 slabs through that XCD's L2 (plain stores); 0: the round-5 dealing with write-through slabs everywhere.  Same bits either way; returns the old setting */
int dmx_set_halo_ws(int on);        /* tuning aid: 0 keeps dmx_conv3x3_gn's planner off the warp-specialised instances (4 compute + 4 loader waves); returns the old setting */

/* Weight-streaming conv3x3 / conv1x1 / linear for the SKINNY levels (M = B H W in {64, 128, 256} output rows: ResnetBlock2D conv1 / conv2 at the 8x8 level at
 * batch 4 and at the 16x16 / 8x8 levels at batch 1, behind unet(...), /root/reference/app.ipynb:814).  K is a list of up to four SEGMENTS - a source tensor
 * [B H W][C] seen through 9 taps (3x3, stride 1, pad 1) or 1 tap (the fused 1x1 shortcut of a resnet; a linear) - and the weights come in FRAGMENT ORDER
 * (dmx_skinny_pack): every compute wave streams its 1-KB MFMA operands straight from memory into registers, the activations of a K slice are staged once in
 * LDS, the GroupNorm (+ SiLU) in front of the conv is applied to the staged chunk from the statistics records of its input(s) (seg.st; NULL = plain input),
 * N / 32 x S blocks ~ one per CU reduce their K slices inside the kernel in slice order (bit-reproducible).  Epilogue: + bias + rowbias[b] + residual, one
 * rounding, optional statistics records of the output.  Needs dmx_set_exclusive_device(1) (the S blocks of a tile wait for each other, bounded: a starved
 * launch raises DMX_ERR_DEVICE).  Round 6: the kernel is correct and exported, but it measures slower than the tiled split-K GEMM + GroupNorm launch it would
 * replace (EXPERIMENTS.md round 6), so the model executors do NOT take it; dmx_set_skinny is reserved for the day they do (returns the old setting). */
typedef struct {
  const void* x; int ld;            /* NHWC 16-bit rows = output pixels */
  int C;                            /* channels, multiple of 16 */
  int taps;                         /* 9 or 1 */
  const long long* st;              /* statistics records [B][C][4] of x, or NULL (no normalisation) */
  const float* gamma; const float* beta;   /* GroupNorm affine of THIS tensor's channels */
  int gn_c0;                        /* first channel of x inside the normalised (concatenated) tensor */
} dmx_skinny_seg;
typedef struct {
  dmx_skinny_seg seg[4]; int nseg;
  int B, H, W;
  int gn_groups, gn_Ctot; float gn_eps; int silu;    /* GroupNorm over the concatenation of the segments with st != NULL (gn_groups = 0: none) */
  const void* wp;                   /* dmx_skinny_pack output */
  int N;                            /* multiple of 32 */
  const float* bias; const float* rowbias; int ldrb;
  const void* res; int ldres;
  void* out; int ldo;
  long long* colstats;
  int force_S;                      /* 0 = automatic number of K slices (1 .. 8; tests) */
  long long* timing;                /* measurement aid: [blocks][6] phase stamps in 10 ns ticks, or NULL */
  int dbg;                          /* measurement aid, 0 */
} dmx_skinny_desc;
int dmx_skinny_conv_supported(const dmx_skinny_desc* d);
size_t dmx_skinny_conv_workspace_bytes(const dmx_skinny_desc* d);
int dmx_skinny_conv(const dmx_skinny_desc* d, void* workspace, size_t workspace_bytes, dmx_stream_t stream);
/* w [N][ldw] 16-bit, column of (segment s, tap t, channel c) = t * tap_stride[s] + koff[s] + c  ->  wp: N x sum_s(C[s] * taps[s]) elements in fragment order */
int dmx_skinny_pack(const void* w, int ldw, void* wp, int N, int nseg, const int* C, const int* taps, const int* tap_stride, const int* koff, dmx_stream_t stream);
int dmx_set_skinny(int on);

/* The row-local chains of diffusers' BasicTransformerBlock + Transformer2DModel.proj_out (the unet(...) call at
 * /root/reference/app.ipynb:814) at the C = 320 levels, ONE launch each (xf_chain.hip); rows M % 64 == 0:
 *   mode 0:  h_out = x w0^T + b0 + res ;  y = LayerNorm(h_out) folded into w1:  rstd * (h_out w1^T - mean * c1) + c2
 *            (attn1.to_out.0 + residual, then attn2.to_q behind norm2; w1 / c1 / c2 as dmx_pack_ln_fold writes them)
 *   mode 2:  h_out = x w0^T + b0 (res unused) ;  y[M][3C] = LayerNorm(h_out) folded into w1 [3C][C] with c1 / c2 [3C]
 *            (proj_in on the GroupNorm output, then attn1's stacked to_q | to_k | to_v behind norm1; ldy >= 3C)
 *   mode 1:  h_out = x w0^T + b0 + res ;  h3 = h_out + wf2 GEGLU(LayerNorm(h_out) folded into wf1) + bf2 ;
 *            y = h3 wpo^T + bpo + xres     (attn2.to_out.0 + residual, ff.net, proj_out + the block residual; wf1 [8C][C] in
 *            the packed GEGLU order of dmx_pack_geglu_weight with c1 / c2 [8C] in the same order; wf2 [C][4C])
 * All 16-bit operands in the build's element type, biases / c1 / c2 fp32.  dmx_xf_chain_supported: 1 for (M, C) it takes.
 * The UNet executor takes the chains when the M / 64 row blocks fill their last round of CUs at least half; dmx_set_xf_chain(0) makes it use the separate
 * GEMMs always, 2 the chains at every supported size (A/B runs in one process); returns the old setting. */
typedef struct {
  int M, C;
  const void* x; int ldx;
  const void* res; int ldres;
  const void* w0; const float* b0;
  void* h_out; int ldh;
  const void* w1;
  const float* c1; const float* c2;
  void* y; int ldy;
  const void* wf1;
  const void* wf2; const float* bf2;
  const void* wpo; const float* bpo;
  const void* xres; int ldxres;
  float eps;
  int dbg; long long* timing;   /* measurement aids, 0 / NULL: ablation bits (results invalid), [M/64][8] phase timestamps in 10 ns ticks */
  /* mode 1, optional: statistics records of y for the GroupNorm that reads it next, [M / cs_rows][C][4] int64, ADDED to (zero them first);
   * cs_rows = rows per sample, a multiple of 64 */
  long long* colstats; int cs_rows;
  /* mode 2, optional: x is the RAW tensor and GroupNorm(gn_groups, gn_eps, gn_gamma, gn_beta; no activation) is applied in the operand
   * load from the statistics records gn_st of x ([M / gn_rows][C][4], as dmx_colstats / a producer's colstats writes them; gn_rows = rows
   * per sample, a multiple of 64) - bit-identical to dmx_groupnorm_from_stats followed by the plain mode 2 */
  const long long* gn_st; const float* gn_gamma; const float* gn_beta; int gn_groups; int gn_rows; float gn_eps;
} dmx_xf_chain_desc;
int dmx_xf_chain_ok(int M, int C);
int dmx_xf_chain(const dmx_xf_chain_desc* d, int mode, dmx_stream_t stream);
int dmx_set_xf_chain(int on);
/* ff.net.2 + proj_out of the transformer blocks that run as separate GEMMs (the levels the chains do not take) as ONE GEMM over
 * [g | h3] with the composed weights [Wpo Wf2 | Wpo] and bias Wpo bf2 + bpo: 1 (default) on, 0 the two launches; returns the old setting.
 * The composed weights are derived data: the first dmx_unet_forward* call after the weights changed (finalize, dmx_unet_refresh_derived)
 * composes them on its stream, before its own launches and outside its own graph capture; dmx_unet_refresh_derived itself only marks them stale.
 * What the caller orders: (a) that composition is enqueued on the stream of the call that finds the weights stale - an inference call on ANOTHER
 * stream must be ordered behind that call (event / synchronise), as behind dmx_unet_refresh_derived; (b) a graph the caller itself captured around
 * dmx_unet_forward* while the composed weights were fresh contains no composition: after a weights change, make one dmx_unet_forward* call outside
 * that graph (it recomposes in place, same addresses) before replaying it - every other derived weight is rebuilt by dmx_unet_refresh_derived
 * itself, the composed ones are not.  A graph captured while they were stale contains the composition and recomposes at every replay. */
int dmx_set_ff_fold(int on);
int dmx_set_weight_prefetch(int on); /* tuning aid: 0 = the launches of dmx_unet_forward* do not touch the weights of the launches that follow them
                                      * (default 1: every GEMM / attention / halo-conv / chain launch prefetches up to 4 MB of them into the memory-side
                                      * cache - the plan comes from a dry walk of the same graph); returns the old setting */

/* Training (P5 over K3/K4/K8): forward GroupNorm that also keeps (mean, rstd) per (image, group), and the backward
 * kernels of GroupNorm(+SiLU), LayerNorm and the unfused GEGLU.  All deterministic.  `res*` is an optional gradient
 * added into dx (the tensor's other consumer, e.g. the residual branch); dgamma/dbeta fp32, `accumulate` adds.
 * Replace autograd's native_group_norm_backward / native_layer_norm_backward / gelu_backward under
 * accelerator.backward (train_diffute_v1.py:925). */
int dmx_groupnorm_train(const void* x0, int ldx0, const void* x1, int ldx1, int c0, int C, int groups,
                        int B, int HW, const float* gamma, const float* beta, float eps, int silu,
                        void* y, int ldy, float* stats, void* workspace, size_t workspace_bytes, dmx_stream_t stream);
size_t dmx_groupnorm_bwd_workspace_bytes(int B, int HW, int C);
int dmx_groupnorm_bwd(const void* x0, int ldx0, const void* x1, int ldx1, int c0, int C, int groups, int B, int HW,
                      const float* gamma, const float* beta, int silu, const float* stats,
                      const void* dy, int lddy, void* dx0, int lddx0, void* dx1, int lddx1,
                      const void* res0, int ldres0, const void* res1, int ldres1,
                      float* dgamma, float* dbeta, int accumulate,
                      void* workspace, size_t workspace_bytes, dmx_stream_t stream);
size_t dmx_layernorm_bwd_workspace_bytes(int rows, int C);
int dmx_layernorm_bwd(const void* x, int ldx, const void* dy, int lddy, const float* gamma, void* dx, int lddx,
                      const void* res, int ldres, float* dgamma, float* dbeta, int accumulate,
                      int rows, int C, float eps, void* workspace, size_t workspace_bytes, dmx_stream_t stream);
int dmx_geglu_fwd(const void* h, int ldh, void* y, int ldy, int rows, int C2, dmx_stream_t stream);
int dmx_geglu_bwd(const void* h, int ldh, const void* dy, int lddy, void* dh, int lddh, int rows, int C2, dmx_stream_t stream);

/* K4: LayerNorm over the channel axis of [rows][C] bf16 (BasicTransformerBlock norm1/2/3). */
int dmx_layernorm(const void* x, int ldx, void* y, int ldy, const float* gamma, const float* beta,
                  int rows, int C, float eps, dmx_stream_t stream);

/* K5/K6: fused attention core softmax(Q K^T * scale) V, head dim 64, no mask.
 * q: row (b*Sq+s), head h at column 64h.  k: row (b*kv_rows+s).  vt: V transposed,
 * row (64h+d), column (b*skv_stride+s); columns [Skv, round_up(Skv,8)) must be finite.
 * Replaces diffusers Attention (optionally xformers, train_diffute_v1.py:648-659). */
int dmx_attention_fwd(const void* q, int ldq, const void* k, int ldk, int kv_rows,
                      const void* vt, int ldvt, int skv_stride, void* o, int ldo,
                      int B, int H, int Sq, int Skv, float scale, dmx_stream_t stream);

/* Same attention with V given row-major (row b*kv_rows+s, head h at column 64h - e.g. a slice of a fused
 * q|k|v projection): the P.V operand is fetched with gfx950 LDS transpose reads, no V^T tensor is needed. */
/* K6b: single-head attention with a wide head, d = 128 / 256 / 512 (AutoencoderKL mid block: diffusers `Attention` inside
 * the VAE's UNetMidBlock2D, reached from vae.encode / vae.decode, app.ipynb:793,819; train_diffute_v1.py:875,886).
 * q / k / v / o: bf16 row-major, row (b*Sq + s) resp. (b*kv_rows + s), d contiguous (column slices of one fused q|k|v buffer
 * are fine: pass the row stride).  Fused flash-style: no S x S buffer, no workspace. */
int dmx_attention_wide(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int kv_rows,
                       void* o, int ldo, int B, int Sq, int Skv, int D, float scale, dmx_stream_t stream);
int dmx_attention_fwd_v(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int kv_rows,
                        void* o, int ldo, int B, int H, int Sq, int Skv, float scale, dmx_stream_t stream);
/* The same op on the BALANCED schedule (stream-K over (128-query block, 64-key tile) items on 3 x CUs block slots; a split row's (O, m, l) halves are
 * folded in a fixed order: bit-repeatable, equal to dmx_attention_fwd_v within the fp32 rounding of the fold).  The executors take it where the plain
 * grid leaves at most two blocks per CU (the 4096 x 4096 self-attention of the 64x64 level at batch 1 - 3; at the headline batch 4 the plain grid
 * stays).  workspace_bytes = 0: the plan keeps the plain grid. */
size_t dmx_attention_fwd_v_balanced_workspace_bytes(int B, int H, int Sq, int Skv);
int dmx_attention_fwd_v_balanced(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int kv_rows,
                                 void* o, int ldo, int B, int H, int Sq, int Skv, float scale,
                                 void* workspace, size_t workspace_bytes, dmx_stream_t stream);
int dmx_set_attn_balanced(int mode);   /* 0: never; 1 (default): where the plan says it pays; 2: wherever the kernel takes the problem (tests, A/B); returns the old setting */

/* Training (P5 over K5/K6): forward that also keeps each row's log2-sum-exp, and the flash-style backward (dQ, dK, dV;
 * deterministic, nothing of size Sq x Skv is stored).  workspace: [B][H][Sq] floats.  Replace autograd's scaled-dot-
 * product-attention backward under accelerator.backward (train_diffute_v1.py:925). */
int dmx_attention_fwd_train(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int kv_rows,
                            void* o, int ldo, float* lse, int B, int H, int Sq, int Skv, float scale, dmx_stream_t stream);
size_t dmx_attention_bwd_workspace_bytes(int B, int H, int Sq);
int dmx_attention_bwd(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, int kv_rows,
                      const void* o, const void* d_o, int ldo, const float* lse,
                      void* dq, int lddq, void* dk, int lddk, void* dv, int lddv,
                      int B, int H, int Sq, int Skv, float scale,
                      void* workspace, size_t workspace_bytes, dmx_stream_t stream);

/* K9: sinusoidal timestep embedding (flip_sin_to_cos) and the small-M fp32 linear used by the
 * time-embedding MLP.  t: int64 [t_count] (t_count 1 or B); freq: fp32 [dim/2] table. */
int dmx_timestep_embedding(const int64_t* t, int t_count, const float* freq, int B, int dim, float* out, dmx_stream_t stream);
int dmx_linear_small(const float* x, int ldx, const void* w_bf16, int ldw, const float* bias, float* y, int ldy,
                     int B, int N, int K, int silu_in, dmx_stream_t stream);

/* small-channel im2col (conv_in 9->320, VAE 3->128 / 4->512, quant convs): NCHW fp32 sources
 * (f0|f1|f2 concatenated on channels = torch.cat([latents, mask, masked_latents], 1),
 * app.ipynb:811) or one NHWC bf16 source -> bf16 [B*OH*OW][Kpad]. */
int dmx_im2col_small(const float* f0, int c0, const float* f1, int c1, const float* f2, int c2,
                     const void* h_nhwc, int ldh, int C, int B, int IH, int IW, int OH, int OW,
                     int ksize, int stride, int pad, void* out, int Kpad, dmx_stream_t stream);

/* weight packing: fp32 torch layouts -> bf16 GEMM rows */
int dmx_pack_conv_weight(const float* w, void* out, int Cout, int Cin, int ksize, int ldk, int koff, dmx_stream_t stream);
int dmx_pack_linear_weight(const float* w, void* out, int rows, int cols, int ldo, int geglu, dmx_stream_t stream);
int dmx_pack_geglu_bias(const float* b, float* out, int n, dmx_stream_t stream);
/* training: the data gradient dX = dY * W runs through dmx_conv_gemm with a transposed pack of W
 * (conv: out[ci][flip(tap)*Cout + n], linear: out[k][n]); a stride-2 conv first zero-inserts dY to the input grid,
 * a conv behind a nearest x2 upsample sum-pools its data gradient 2x2.  (autograd conv/linear backward,
 * train_diffute_v1.py:925) */
int dmx_pack_conv_weight_t(const float* w, void* out, int Cout, int Cin, int ksize, int ldk, int koff, dmx_stream_t stream);
int dmx_pack_linear_weight_t(const float* w, void* out, int rows, int cols, int ldo, dmx_stream_t stream);
int dmx_zero_insert2(const void* dy, int lddy, void* z, int B, int OH, int OW, int C, dmx_stream_t stream);
int dmx_sumpool2(const void* du, int lddu, int du_f32, void* dx, int lddx, int B, int H, int W, int C, int accumulate, dmx_stream_t stream);

/* layout helpers */
int dmx_cast_f32_to_bf16(const float* in, void* out, size_t n, dmx_stream_t stream);
int dmx_nhwc_bf16_to_nchw_f32(const void* in, int ldin, float* out, int B, int C, int HW, dmx_stream_t stream);
int dmx_nhwc_f32_to_nchw_f32(const float* in, int ldin, float* out, int B, int C, int HW, dmx_stream_t stream);
int dmx_nchw_f32_to_nhwc_bf16(const float* in, void* out, int ldo, int B, int C, int HW, dmx_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Scheduler.  Scalar coefficients are computed by the host-side
 * scheduler classes; these are the elementwise updates over [B,4,h,w] fp32 latents.
 * ---------------------------------------------------------------------------------- */
/* DDIMScheduler.step(...).prev_sample  (north_star; same call shape as app.ipynb:816) */
int dmx_sched_step_ddim(const float* sample, const float* model_output, const float* noise, float* prev_sample, size_t n,
                        float sqrt_beta_prod_t, float sqrt_alpha_prod_t, float sqrt_alpha_prod_prev,
                        float dir_coef, float std_dev, int v_prediction, dmx_stream_t stream);
/* DDPMScheduler.step(...).prev_sample  (app.ipynb:816); noise = NULL when t == 0 */
int dmx_sched_step_ddpm(const float* sample, const float* model_output, const float* noise, float* prev_sample, size_t n,
                        float sqrt_beta_prod_t, float sqrt_alpha_prod_t, float coef_x0, float coef_xt,
                        float sigma, int v_prediction, dmx_stream_t stream);
/* DPMSolverMultistepScheduler.step(...).prev_sample (DPM-Solver++, orders 1-3): the per-step scalars, computed on the
 * host (diffute_amd/schedulers.py step_plan).  alpha_s0 / sigma_s0 convert the model output to the data prediction m0;
 * c_x = sigma_t/sigma_s0, c_m0 = alpha_t*(exp(-h)-1); order >= 2: inv_r0 = 1/r0 and c_d1, the SIGNED coefficient of D1
 * (midpoint -(0.5*c_m0), heun / order 3 alpha_t*((exp(-h)-1)/h+1)); order 3: inv_r1 = 1/r1, r0_over_r01 = r0/(r0+r1),
 * inv_r01 = 1/(r0+r1), c_d2 = alpha_t*((exp(-h)-1+h)/h^2-0.5) (subtracted).  Fields an order does not read are ignored. */
typedef struct dmx_dpm_coefs {
  float alpha_s0, sigma_s0;
  float c_x, c_m0, c_d1, c_d2;
  float inv_r0, inv_r1, r0_over_r01, inv_r01;
} dmx_dpm_coefs;
/* m1 / m2: the data predictions of the previous two steps (NULL when `order` does not read them: m1 for order >= 2, m2 for
 * order 3); x0_out receives this step's m0 (the next step's m1) and must not overlap m1, m2 or prev_sample; prev_sample may
 * be `sample` (in-place update).  Bit-identical to the fp32 CPU evaluation of diffusers' expressions in their op order. */
int dmx_sched_step_dpmpp(const float* sample, const float* model_output, const float* m1, const float* m2, float* x0_out,
                         float* prev_sample, size_t n, int order, dmx_dpm_coefs coefs, int v_prediction, dmx_stream_t stream);
/* ---- in-flight batching (diffute_amd/inflight.py DenoiseEngine): every row of a denoise batch on its own schedule.
 * A PLAN is built once per (scheduler kind, num_inference_steps): a device array of per-step records and a time-embedding table
 * (dmx_unet_temb_table) with the same row numbering, so plan row p names the timestep, the table row and the scheduler scalars of
 * one step at once.  Plans of several step counts are stored back to back in one array / one table.  Row b of the batch is two
 * device ints at fixed addresses: row_index[b] (a plan row, -1 = idle) and row_left[b] (steps still to run).
 * c[5]: DDIM (sqrt_beta_prod_t, sqrt_alpha_prod_t, sqrt_alpha_prod_prev, dir_coef, std_dev) or DDPM (sqrt_beta_prod_t,
 * sqrt_alpha_prod_t, coef_x0, coef_xt, sigma) - the scalar arguments of the entries above in their order; dpm / order: the
 * arguments of the DPM-Solver++ entry; ring_w / ring_m1 / ring_m2: the history slots step i of its request writes (i % k) and reads
 * ((i-1) % k, (i-2) % k; k = solver_order); use_noise: add c[4] * noise (the entries above: noise != NULL). */
typedef struct dmx_sched_row_rec {
  float c[5];
  dmx_dpm_coefs dpm;
  int order, use_noise;
  int ring_w, ring_m1, ring_m2;
  int64_t timestep;
} dmx_sched_row_rec;
enum { DMX_SCHED_DDIM = 0, DMX_SCHED_DDPM = 1, DMX_SCHED_DPMPP = 2 };
/* One launch for all B rows: row b with row_index[b] >= 0 is updated IN PLACE (sample [B][per_sample]) with record
 * plan[row_index[b]]; per element bit-identical to the matching entry above run on that row alone.  A row with row_index[b] < 0
 * is neither read nor written, nor is its slice of any history buffer.  model_output / noise [B][per_sample] (noise may be NULL:
 * no row adds noise); hist [n_hist][B][per_sample] (DPM-Solver++ only, n_hist = solver_order; NULL, 0 otherwise).  per_sample
 * need not be a multiple of 4. */
int dmx_sched_step_rows(float* sample, const float* model_output, const float* noise, float* hist, int n_hist,
                        const dmx_sched_row_rec* plan, const int* row_index, int B, size_t per_sample, int kind, int v_prediction,
                        dmx_stream_t stream);
/* Classifier-free guidance (Ho & Salimans 2022), the optional guidance rescale (Lin et al. 2023, diffusers' rescale_noise_cfg) and the
 * scheduler step of B samples in ONE launch.  model_output [2B][per_sample]: rows [0,B) from the conditional context, rows [B,2B) from
 * the unconditional one.  sample [2B][per_sample]: sample b is READ from row b only; prev_sample is written to row b AND row B + b, so
 * the next 2B-row forward reads it with no copy (rows [B,2B) are write-only).  noise [B][per_sample] or NULL (added when given; must be
 * NULL for DPM-Solver++); hist [n_hist][B][per_sample], the DPM-Solver++ ring (NULL, 0 otherwise): rec names the slot it writes
 * (ring_w, this step's m0) and the two it reads, as for the per-row entry.  rec: the step's record, by value.  Per element, ec / eu the
 * conditional / unconditional model output, every op fp32 round-to-nearest in this order:
 *   g = eu + guidance_scale * (ec - eu);   rescale == 0: e = g;   else e = rescale * (g * k_b) + one_minus_rescale * g
 * with k_b = std_b(ec) / std_b(g), the UNBIASED standard deviations over the per_sample elements of sample b (fp32, mean first, then
 * the centred squares, in a fixed order: the same bits on every run).  std_b(g) == 0 gives k_b = inf or NaN, which propagates into the
 * sample as it does in diffusers.  Then the update of `kind` on (sample, e): bit-identical to the matching scalar entry above run on e.
 * ratio_out [B] or NULL receives k_b (written only when rescale != 0).  per_sample need not be a multiple of 4.
 * DMX_ERR_ARG, nothing written: B < 1, per_sample == 0, NULL sample / model_output, kind outside the enum, DPM-Solver++ with noise or
 * with a record its ring cannot serve (order 1..n_hist, slots inside the ring, a read slot equal to the written one), rescale outside
 * [0, 1], rescale != 0 with per_sample < 2, a non-finite guidance_scale / rescale / one_minus_rescale. */
int dmx_sched_step_guided(float* sample, const float* model_output, const float* noise, float* hist, int n_hist, dmx_sched_row_rec rec,
                          int kind, int v_prediction, float guidance_scale, float rescale, float one_minus_rescale, float* ratio_out,
                          int B, size_t per_sample, dmx_stream_t stream);
/* ---- the per-row guided step: in-flight batching WITH classifier-free guidance.  A guided request of n samples holds 2n consecutive
 * engine rows, [s0, s0+n) on the glyph context and [s0+n, s0+2n) on the unconditional one - the layout dmx_sched_step_guided gives its 2B
 * rows; both halves are admitted with the same (plan_base, n_steps), so they advance and retire together.  The GUIDE TABLE, one entry per
 * engine row at a fixed address, says which half a row is: role (PLAIN: a row of a request without guidance; COND / UNCOND: the two halves
 * of a pair), partner (the other row of the pair; unused for PLAIN) and the pair's own scale, rescale and one_minus_rescale (read from
 * the COND entry). */
typedef struct dmx_guide_row { int role, partner; float scale, rescale, one_minus_rescale; } dmx_guide_row;
enum { DMX_GUIDE_PLAIN = 0, DMX_GUIDE_COND = 1, DMX_GUIDE_UNCOND = 2 };
/* One launch for all B rows, dmx_sched_step_rows with the guide table.  Per row b:
 *   row_index[b] < 0           idle: nothing of the row is read or written, whatever guide[b] says;
 *   PLAIN                      dmx_sched_step_rows' update of the row, bit for bit;
 *   UNCOND                     nothing is done for the row itself: its sample slab is written by its partner's update and never read, its
 *                              noise and history slices are neither read nor written;
 *   COND with partner p        dmx_sched_step_guided run on the pair alone (B = 1), bit for bit: ec = model_output[b], eu = model_output[p],
 *                              the record plan[row_index[b]], guide[b]'s scale / rescale / one_minus_rescale, noise[b] where the record
 *                              asks for it (use_noise), the history slices hist[.][b]; prev_sample is written to sample[b] AND sample[p],
 *                              and with rescale != 0 the ratio k to ratio_out[b] (ratio_out [B] or NULL).
 * A row that cannot be served is left alone (sample, noise and history slices unchanged), the rest of the launch is not affected: a role
 * outside the enum; a COND row whose partner is outside [0, B), is b itself, has another row_index, is not UNCOND or does not name b as ITS
 * partner; for DPM-Solver++ a record its ring cannot serve (as for dmx_sched_step_rows).  The launch is always B blocks of 1024 threads, the
 * shape dmx_sched_step_guided reduces the ratio with: the sums of k are taken in that entry's order.
 * DMX_ERR_ARG, nothing written: B < 1, per_sample < 2 (a rescaled row divides by per_sample - 1), NULL sample / model_output / plan /
 * row_index / guide, kind outside the enum, DPM-Solver++ with noise, with hist == NULL or n_hist outside 1..3. */
int dmx_sched_step_rows_guided(float* sample, const float* model_output, const float* noise, float* hist, int n_hist,
                               const dmx_sched_row_rec* plan, const int* row_index, const dmx_guide_row* guide, float* ratio_out, int B,
                               size_t per_sample, int kind, int v_prediction, dmx_stream_t stream);
/* the guide entries of one request, one tiny launch (the values travel as kernel arguments: no staging buffer).  guided = 1: rows
 * [b0, b0+n) become COND with partner b + n and rows [b0+n, b0+2n) UNCOND with partner b - n, all carrying the three scalars;
 * guided = 0: rows [b0, b0+n) become PLAIN, the all-zero entry (a zeroed table is a table of PLAIN rows; the scalars are checked but not
 * stored).  The caller keeps [b0, b0+2n) / [b0, b0+n) inside its table.
 * DMX_ERR_ARG, nothing written: NULL guide, b0 < 0, n < 1, guided outside {0, 1}, a non-finite scalar, rescale outside [0, 1]. */
int dmx_rows_guide(dmx_guide_row* guide, int b0, int n, int guided, float scale, float rescale, float one_minus_rescale, dmx_stream_t stream);
/* row b starts at plan row plan_base with n_steps steps to run (the values travel as kernel arguments: no staging buffer) */
int dmx_rows_admit(int* row_index, int* row_left, int b, int plan_base, int n_steps, dmx_stream_t stream);
/* after the scheduler launch of a tick: every active row index++, left--, index = -1 at left == 0 */
int dmx_rows_advance(int* row_index, int* row_left, int B, dmx_stream_t stream);
/* scheduler.add_noise / get_velocity (train_diffute_v1.py:897,907): per-sample coefficients */
int dmx_sched_add_noise(const float* x0, const float* noise, const float* sqrt_alpha_prod, const float* sqrt_one_minus,
                        float* out, int B, size_t per_sample, dmx_stream_t stream);
int dmx_sched_get_velocity(const float* x0, const float* noise, const float* sqrt_alpha_prod, const float* sqrt_one_minus,
                           float* out, int B, size_t per_sample, dmx_stream_t stream);
/* latent_dist.sample() * scaling_factor (app.ipynb:793-794; train_diffute_v1.py:875-876);
 * noise = NULL gives latent_dist.mode() (train_vae.py:721). moments NCHW fp32 [B][2C][HW]. */
int dmx_gaussian_sample(const float* moments, const float* noise, float* out, int B, int C, int HW, float scale, dmx_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Whole-model executors.
 * ---------------------------------------------------------------------------------- */
typedef struct dmx_unet_config {
  int in_channels, out_channels;
  int block_out_channels[4];
  int layers_per_block;
  int heads[4];                 /* diffusers `attention_head_dim` (= head counts)            */
  int cross_attention_dim;
  int norm_num_groups;
  int down_has_attn[4], up_has_attn[4];
} dmx_unet_config;

/* UNet2DConditionModel  (from_pretrained: train_diffute_v1.py:633-635, app.ipynb:551-553) */
dmx_unet* dmx_unet_create(const dmx_unet_config* cfg);
void dmx_unet_destroy(dmx_unet* u);
int dmx_unet_param_count(const dmx_unet* u);
/* name = diffusers state-dict key; shape up to 4 dims (unused = 0) */
int dmx_unet_param_info(const dmx_unet* u, int index, const char** name, int shape[4]);
size_t dmx_unet_arena_bytes(const dmx_unet* u);
int dmx_unet_bind_arena(dmx_unet* u, void* arena, size_t bytes);
int dmx_unet_load_param(dmx_unet* u, const char* name, const float* src_f32, dmx_stream_t stream);
int dmx_unet_finalize(dmx_unet* u, const float* h_freq_table, dmx_stream_t stream);
size_t dmx_unet_context_bytes(const dmx_unet* u, int B, int ctx_len);
size_t dmx_unet_workspace_bytes(dmx_unet* u, int B, int H, int W, int ctx_len);
/* cross-attention K / V^T of the glyph context, constant across denoise steps (app.ipynb:776,814) */
int dmx_unet_set_context(dmx_unet* u, const void* ctx, int ctx_is_bf16, int B, int ctx_len,
                         void* context_cache, size_t context_bytes, void* workspace, size_t workspace_bytes,
                         dmx_stream_t stream);
/* The same projection for `n` context rows (ctx [n][ctx_len][cross_attention_dim]) into rows [row0, row0 + n) of a cache laid out
 * for B rows (dmx_unet_context_bytes(u, B, ctx_len)): one row of a running batch gets a new glyph context while the others are mid-loop.
 * No byte of another row is written.  row0 = 0, n = B issues the GEMMs of dmx_unet_set_context (same M, ld, pointers): the same bytes. */
int dmx_unet_set_context_rows(dmx_unet* u, const void* ctx, int ctx_is_bf16, int row0, int n, int B, int ctx_len,
                              void* context_cache, size_t context_bytes, void* workspace, size_t workspace_bytes,
                              dmx_stream_t stream);
/* unet(sample, timestep, encoder_hidden_states).sample  (app.ipynb:814, train_diffute_v1.py:913).
 * The 9-channel sample is given as up to three NCHW fp32 tensors (c0+c1+c2 = in_channels):
 * pass the concatenated tensor as f0 with c0 = 9, or latents/mask/masked latents separately
 * (fuses torch.cat of app.ipynb:811).  timesteps: device int64 [t_count], t_count 1 or B.
 * out: NCHW fp32 [B][out_channels][H][W]. */
int dmx_unet_forward(dmx_unet* u, const float* f0, int c0, const float* f1, int c1, const float* f2, int c2,
                     const int64_t* timesteps, int t_count, const void* context_cache, int ctx_len,
                     float* out, int B, int H, int W, void* workspace, size_t workspace_bytes, dmx_stream_t stream);

/* The time-embedding MLP and the stacked time_emb_proj of every resnet depend on the timestep only: a denoise loop
 * (/root/reference/app.ipynb:806-816) can compute them for ALL its timesteps in one batched pass and let each step fetch its row
 * - one tiny launch instead of four per step, and the 49 MB of projection weights are streamed once per loop instead of once
 * per step.  Rows are bit-identical to what the per-step path computes.  dmx_unet_temb_table fills table[T][tproj] (fp32;
 * dmx_unet_temb_table_floats(T) elements); dmx_unet_use_temb_table(u, table, step_index) makes the following scalar-timestep
 * forwards read row *step_index (an int on the device, updated by the caller between steps); (NULL, NULL) switches back. */
size_t dmx_unet_temb_table_floats(dmx_unet* u, int T);
size_t dmx_unet_temb_table_workspace_bytes(dmx_unet* u, int T);
int dmx_unet_temb_table(dmx_unet* u, const int64_t* timesteps, int T, float* table, void* workspace, size_t workspace_bytes, dmx_stream_t stream);
int dmx_unet_use_temb_table(dmx_unet* u, const float* table, const int* step_index);
/* Per-row form (in-flight batching): with (table, plan, row_index) set, a forward with t_count == B fetches
 * tproj[b] = table[max(row_index[b], 0)] with one launch, which also WRITES timesteps[b] = plan[max(row_index[b], 0)].timestep into the
 * forward's `timesteps` argument (it stays truthful; the buffer must be writable).  `table` and `plan` share their row numbering;
 * row_index is int [B] on the device.  All three NULL switches back.  A handle holds ONE table source: setting either form replaces
 * the other, and the all-NULL call of a form clears the source only while it holds that form. */
int dmx_unet_use_temb_table_rows(dmx_unet* u, const float* table, const dmx_sched_row_rec* plan, const int* row_index);
/* Same as dmx_unet_forward; the launch sequence is captured into a hipGraph the second time an identical argument
 * tuple is seen and replayed afterwards.  Requires a non-NULL stream (falls back to eager launches otherwise). */
int dmx_unet_forward_graph(dmx_unet* u, const float* f0, int c0, const float* f1, int c1, const float* f2, int c2,
                           const int64_t* timesteps, int t_count, const void* context_cache, int ctx_len,
                           float* out, int B, int H, int W, void* workspace, size_t workspace_bytes, dmx_stream_t stream);

/* Step cache (DeepCache-style reuse of the deep features across denoise steps; Ma et al., CVPR 2024).  The output of the deep part of
 * the UNet - levels 1..3, the mid block, up-blocks 0..2 - changes slowly from step to step, so a loop may run it on some steps only.
 * A FILL forward is dmx_unet_forward (bit-equal `out`) that also leaves the tensor entering the last up-block
 * ([B*H*W][block_out_channels[1]] in the compute element type) and its GroupNorm statistics records in `cache`, a caller-owned device
 * buffer of dmx_unet_step_cache_bytes(u, B, H, W) bytes, 16-byte aligned.  A USE forward runs only conv_in, down-block 0, up-block 3 (fed
 * the kept tensor), conv_norm_out and conv_out: with the inputs of the FILL that wrote the cache it returns that forward's bits, with
 * other inputs the shallow step of the cached algorithm.  Both need dmx_unet_workspace_bytes_cached (the larger of the two walks); the
 * _graph form captures one hipGraph per (call, cache, mode).  The time-embedding sources of dmx_unet_use_temb_table* apply as usual.
 * A cache serves USE forwards of the shape (B, H, W) and under the dmx_set_* switches it was filled with; refill it after changing either. */
#define DMX_STEP_CACHE_FILL 1
#define DMX_STEP_CACHE_USE 2
size_t dmx_unet_step_cache_bytes(dmx_unet* u, int B, int H, int W);
size_t dmx_unet_workspace_bytes_cached(dmx_unet* u, int B, int H, int W, int ctx_len);
int dmx_unet_forward_cached(dmx_unet* u, const float* f0, int c0, const float* f1, int c1, const float* f2, int c2,
                            const int64_t* timesteps, int t_count, const void* context_cache, int ctx_len,
                            float* out, int B, int H, int W, void* cache, size_t cache_bytes, int mode,
                            void* workspace, size_t workspace_bytes, dmx_stream_t stream);
int dmx_unet_forward_cached_graph(dmx_unet* u, const float* f0, int c0, const float* f1, int c1, const float* f2, int c2,
                                  const int64_t* timesteps, int t_count, const void* context_cache, int ctx_len,
                                  float* out, int B, int H, int W, void* cache, size_t cache_bytes, int mode,
                                  void* workspace, size_t workspace_bytes, dmx_stream_t stream);

/* Validation / debugging entry points (tests only; the product path never calls them).
 *   dmx_unet_forward_taps   dmx_unet_forward that also copies out the block outputs conv_in, down0..3, mid, up0..3 (the points the
 *                           oracle taps, oracle/unet.py) as NCHW fp32, back to back, into `taps`; tap_shapes[4*i..] = (B, C, H, W).
 *   dmx_unet_forward_f32    the same graph walker on fp32 activations, the fp32 master copy of the parameters (`masters`:
 *                           dmx_unet_grad_bytes(u) bytes filled by dmx_unet_master_import for every parameter) and plain fp32
 *                           kernels: north_star's "within 1e-3 rel fp32" against the fp32 reference path (app.ipynb:560 runs
 *                           inference in fp32).  `context` = raw glyph context [B][ctx_len][cross_attention_dim] fp32; taps optional. */
int dmx_unet_forward_taps(dmx_unet* u, const float* f0, int c0, const float* f1, int c1, const float* f2, int c2,
                          const int64_t* timesteps, int t_count, const void* context_cache, int ctx_len, float* out, int B, int H, int W,
                          void* workspace, size_t workspace_bytes, float* taps, size_t tap_floats, int* tap_shapes, int* n_taps, dmx_stream_t stream);
size_t dmx_unet_workspace_bytes_f32(dmx_unet* u, int B, int H, int W, int ctx_len);
int dmx_unet_forward_f32(dmx_unet* u, const void* masters, const float* f0, int c0, const float* f1, int c1, const float* f2, int c2,
                         const int64_t* timesteps, int t_count, const float* context, int ctx_len, float* out, int B, int H, int W,
                         void* workspace, size_t workspace_bytes, float* taps, size_t tap_floats, int* tap_shapes, int* n_taps, dmx_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Training of the denoiser: train_diffute_v1.py:913-925.
 *   dmx_unet_train_prepare   W^T copies of every GEMM weight (data-gradient operands) into `wt`; after each weight update
 *   dmx_unet_train_forward   pred = unet(cat(f0,f1,f2), t, ctx), keeping what the backward needs inside `workspace`
 *   dmx_unet_train_backward  all parameter gradients (fp32, packed like the weights arena: the gradient of the element
 *                            at arena byte offset o sits at byte offset 2*o of `grads`); records event i when gradient
 *                            bucket i is final, so the gradient exchange (RCCL) can overlap the rest of the backward
 *   dmx_unet_grad_export     one parameter's gradient in its torch layout
 *   dmx_mse_loss             loss = mean((pred - target)^2) and dpred = 2 (pred - target) / n * grad_scale
 *   dmx_diffusion_loss       the Min-SNR / text-box weighted objective with its target, gradient and per-sample sums (declared below)
 * ---------------------------------------------------------------------------------- */
size_t dmx_unet_train_workspace_bytes(dmx_unet* u, int B, int H, int W, int ctx_len);
size_t dmx_unet_train_wt_bytes(const dmx_unet* u);
int dmx_unet_train_prepare(dmx_unet* u, void* wt_arena, size_t wt_bytes, dmx_stream_t stream);
size_t dmx_unet_grad_bytes(const dmx_unet* u);
int dmx_unet_train_forward(dmx_unet* u, const void* wt_arena,
                           const float* f0, int c0, const float* f1, int c1, const float* f2, int c2,
                           const int64_t* timesteps, int t_count, const void* ctx, int ctx_is_bf16, int ctx_len,
                           float* pred, int B, int H, int W, void* workspace, size_t workspace_bytes, dmx_stream_t stream);
int dmx_unet_train_bucket_count(const dmx_unet* u);
int dmx_unet_train_bucket_range(const dmx_unet* u, int i, size_t* begin, size_t* end);
int dmx_unet_train_tail_range(const dmx_unet* u, size_t* begin, size_t* end);
int dmx_unet_train_backward(dmx_unet* u, void* grads, const float* dpred, void* const* events, int n_events, dmx_stream_t stream);
int dmx_unet_grad_export(const dmx_unet* u, const void* grads, const char* name, float* dst, dmx_stream_t stream);
int dmx_unet_grad_range(const dmx_unet* u, const char* name, size_t* begin, size_t* end);
/* Training of the autoencoder (train_vae.py:716-736): recon = decode(encode(x).latent_dist.mode()),
 * backward for dLoss/drecon.  Same protocol and gradient-arena convention as the UNet. */
size_t dmx_vae_train_workspace_bytes(dmx_vae* v, int B, int H, int W);
size_t dmx_vae_train_wt_bytes(const dmx_vae* v);
int dmx_vae_train_prepare(dmx_vae* v, void* wt_arena, size_t wt_bytes, dmx_stream_t stream);
size_t dmx_vae_grad_bytes(const dmx_vae* v);
int dmx_vae_train_forward(dmx_vae* v, const void* wt_arena, const float* x, float* recon, int B, int H, int W,
                          void* workspace, size_t workspace_bytes, dmx_stream_t stream);
int dmx_vae_train_backward(dmx_vae* v, void* grads, const float* drecon, dmx_stream_t stream);
int dmx_vae_grad_export(const dmx_vae* v, const void* grads, const char* name, float* dst, dmx_stream_t stream);

/* On-device pre/post-processing either side of the denoise loop.  Reference (host, PIL / numpy / cv2 /
 * albumentations): generate_mask app.ipynb:370-378; prepare_mask_and_masked_image :380-383; the crop + alb.Resize(512,512)
 * + alb.Normalize(0.5, 0.5) + ToTensorV2 pipelines :332-344,:722-745; F.interpolate(mask, latent size) :776-779;
 * (image_vae / 2 + 0.5) * 255, cv2.resize to the crop, paste inside the text box, round to uint8 :825-846.
 * Resize semantics: OpenCV INTER_LINEAR as published (uint8 fixed point / fp32; exact 2x downscale = 2x2 area mean).
 *   mask_rasterize:   mask[y][x] = 1 inside the inclusive rectangle (x0,y0)-(x1,y1), else 0 (PIL draw.rectangle, fill=1).
 *   preprocess_crop:  image_hwc uint8 [H][W][3], mask uint8 [H][W]; crop [y_s:y_s+crop_scale, x_s:x_s+crop_scale] (clipped at
 *                     the border like a numpy slice) -> S x S: out_image / out_masked_image fp32 [3][S][S] normalised to
 *                     [-1,1] (masked = image * (mask < 0.5) before the resize), out_mask uint8 [S][S],
 *                     out_mask_latent fp32 [S/8][S/8] (nearest; may be NULL).
 *   postprocess_paste: image_vae fp32 [3][S][S] in [-1,1] -> resized to the crop extent, written over original_hwc inside
 *                     the box [y1:y2, x1:x2] only; out_hwc uint8 [H][W][3] (everything else copied).  Values outside
 *                     [0,255] are clamped (numpy's cast is undefined there). */
int dmx_mask_rasterize(unsigned char* mask, int H, int W, int x0, int y0, int x1, int y1, dmx_stream_t stream);
int dmx_preprocess_crop(const unsigned char* image_hwc, const unsigned char* mask, int H, int W, int x_s, int y_s, int crop_scale,
                        int S, float* out_image, float* out_masked_image, unsigned char* out_mask, float* out_mask_latent,
                        dmx_stream_t stream);
int dmx_postprocess_paste(const float* image_vae, int S, const unsigned char* original_hwc, unsigned char* out_hwc, int H, int W,
                          int x_s, int y_s, int crop_scale, int x1, int y1, int x2, int y2, dmx_stream_t stream);

/* Several text boxes of ONE image in one launch each way (1 <= B <= DMX_EDIT_MAX_ITEMS, H <= 65535).  The geometry of the
 * boxes travels as a table of dmx_edit_item, not as kernel arguments.  The caller fills box, origin and crop_scale of every
 * item, lets edit_items_prepare validate them and fill the derived fields (the host arithmetic of the single-box entries:
 * extent clipped at the border, scales as doubles, the exact-2x flags), and copies the table to the device in stream order
 * (one asynchronous copy from pinned memory) before the launch.  Both entries take the host table and its device copy: the
 * host table is checked again, item by item, exactly like the arguments of the single-box entries - a bad item is reported
 * by index through the last-error string and nothing is launched -, the kernels read the device copy (trusted to hold the same
 * bytes; they clamp every origin / extent to the image, so a stale table reads wrong pixels, never outside).
 *   preprocess_crop_batch:  row b of out_image / out_masked_image fp32 [B][3][S][S], out_mask uint8 [B][1][S][S] and
 *                     out_mask_latent fp32 [B][1][S/8][S/8] (may be NULL) is what preprocess_crop writes for item b with the
 *                     mask mask_rasterize draws for item b's box alone (both corners included).  The mask is a predicate
 *                     inside the kernel: no [H][W] buffer, no rasterise launch.
 *   postprocess_paste_batch: image_vae fp32 [B][3][S][S]; out_hwc is what B chained postprocess_paste calls in index order
 *                     leave (where boxes overlap the later item wins; a pixel no item covers is copied).  union_mask
 *                     (may be NULL) uint8 [H][W]: 1 where the inclusive box of any item covers the pixel. */
#define DMX_EDIT_MAX_ITEMS 64
typedef struct dmx_edit_item {
  int x1, y1, x2, y2;               /* text box */
  int x_s, y_s, crop_scale;         /* crop origin and side */
  int cw, ch;                       /* derived: crop extent clipped at the image border */
  int pre_area2, post_area2;        /* derived: the crop is exactly 2S x 2S / exactly S/2 x S/2 */
  int reserved;
  double pre_sx, pre_sy;            /* derived: cw / S, ch / S */
  double post_sx, post_sy;          /* derived: S / cw, S / ch */
} dmx_edit_item;
int dmx_edit_items_prepare(dmx_edit_item* items, int B, int H, int W, int S);
int dmx_preprocess_crop_batch(const unsigned char* image_hwc, int H, int W, const dmx_edit_item* items_host, const dmx_edit_item* items_device,
                              int B, int S, float* out_image, float* out_masked_image, unsigned char* out_mask, float* out_mask_latent,
                              dmx_stream_t stream);
int dmx_postprocess_paste_batch(const float* image_vae, int S, const unsigned char* original_hwc, unsigned char* out_hwc,
                                unsigned char* union_mask, int H, int W, const dmx_edit_item* items_host,
                                const dmx_edit_item* items_device, int B, dmx_stream_t stream);

/* The image half of TrOCRProcessor (`processor(images=ttf_imgs, return_tensors="pt").pixel_values`, app.ipynb:773,
 * train_diffute_v1.py:868; a ViT image processor: PIL resize, rescale, normalise): ONE launch turns a ragged batch of uint8
 * 3-channel images into out_pixel_values fp32 [B][3][S_h][S_w], bit for bit what Pillow's 8-bit Image.resize (Resample.c as
 * published: horizontal pass, result stored as bytes, then the vertical pass; a pass whose sizes are equal is skipped)
 * followed by the processor's float arithmetic gives.  All floating point is done by the CALLER and passed as device tables:
 *   images  B descriptors.  src = device address of pixel (0,0) channel 0; strides in bytes, so HWC, CHW and strided views
 *           are read in place.  h_off / v_off = offset (in ints) of that pass's table inside `tables`, < 0 = pass skipped;
 *           h_taps / v_taps = its coefficient row length (Pillow's ksize).
 *   tables  per pass: bounds int[out][2] = (first source index, tap count), then coefficients int[out][taps] in 2^22
 *           fixed point.  Each output byte is clip8((2^21 + sum pixel * k) >> 22).
 *   norm    float[3][256]: the value written for channel c and resized byte v.
 *   max_taps the largest h_taps / v_taps of the batch; more than DMX_GLYPH_MAX_TAPS is refused (DMX_ERR_ARG): a thread does
 *           h_taps * v_taps MACs per channel, which caps the downscale ratio at 31 (bilinear) / 15 (bicubic).
 *   out_resized (optional, may be NULL) uint8 [B][3][S_h][S_w]: the resized bytes before normalisation.
 * Table bounds are clamped to the image inside the kernel; the descriptors' addresses and strides are trusted. */
#define DMX_GLYPH_MAX_TAPS 64
typedef struct dmx_glyph_image {
  unsigned long long src;
  long long stride_y, stride_x, stride_c;
  int H, W;
  int h_off, h_taps, v_off, v_taps;
} dmx_glyph_image;
int dmx_glyph_max_taps(void);
int dmx_glyph_resize_normalize(const dmx_glyph_image* images, int B, const int* tables, const float* norm, int max_taps, int S_h, int S_w,
                               float* out_pixel_values, unsigned char* out_resized, dmx_stream_t stream);

/* Glyph images from text (the reference's draw_text, app.ipynb:347-363, train_diffute_v1.py:352-368: a white canvas, black text) on the
 * device.  The caller rasterises a font ONCE into an atlas - per glyph a coverage bitmap (uint8, row-major, w x h bytes at `off` of
 * the pool) with its offset (left, top) - and lays text out on the host into placements: (glyph, x, y) = where the bitmap's top-left
 * pixel lands on the canvas.  A canvas byte is 255 - m in all three channels, m the coverage composed over the item's placements IN
 * ORDER, m = s + round(m * (255 - s) / 255) with s the glyph's byte at that pixel (0 outside its bitmap); what leaves the canvas on
 * any side is clipped.  This is, bit for bit, Pillow's ImageDraw.text under the BASIC layout.  Integer arithmetic only.
 *   atlas   pool / glyphs_device on the device, glyphs_host the same records on the host.  Refused: a record whose bitmap is not
 *           inside the pool.
 *   items   B of them, a host copy the entry checks and a device copy the kernel reads: the item's placements are
 *           [first, first + count) of the placement table (count may be 0: a white canvas), its canvas is H x W.
 *           glyph_render writes byte (y, x, c) to dst + y * stride_y + x * stride_x + c * stride_c (bytes; trusted, like
 *           dmx_glyph_image); the h_* / v_* fields are the canvas's pass tables for glyph_text_pixel_values, as in dmx_glyph_image.
 *   placements  n_placements of them, host and device copies (both may be NULL when n_placements is 0).  Refused: a range that
 *           ends past the table, a glyph index outside the atlas, a coordinate beyond +-2^24.
 *   glyph_render: one launch, one thread per canvas pixel of the ragged batch.
 *   glyph_text_pixel_values: from the placements straight to out_pixel_values fp32 [B][3][S_h][S_w] (and out_resized, optional), bit
 *           for bit glyph_resize_normalize over the canvases glyph_render writes - without a canvas in memory: a block of
 *           DMX_GLYPH_TEXT_BLOCK output pixels of one row renders the source rows and columns its taps touch as grey bytes into LDS
 *           and resamples from there.  tables / table_ints / norm / max_taps as for readback_pixel_values.  The strip of a block is
 *           at most min(v_taps, H) rows (1 if the vertical pass is skipped) of min(W, (BLOCK - 1) * W / S_w + h_taps + 2) columns
 *           (min(W, BLOCK) if the horizontal pass is skipped); if that exceeds DMX_GLYPH_TEXT_LDS_BYTES for any item the entry
 *           returns DMX_ERR_UNSUPPORTED and launches nothing (glyph_render + glyph_resize_normalize serve every shape).
 * The kernels clamp what they read from the device copies - placement range, glyph index, bitmap offset - to the tables and the
 * pool, and the strip reads to the strip: a device table that differs from its host copy gives wrong pixels, no access outside. */
#define DMX_GLYPH_TEXT_BLOCK 128
#define DMX_GLYPH_TEXT_LDS_BYTES 32768
#define DMX_GLYPH_TEXT_MAX_COORD 16777216
typedef struct dmx_glyph_rec {
  int off, w, h;                    /* bitmap: w * h bytes at pool + off */
  int left, top;                    /* offset of the bitmap from the pen position (host layout only) */
  int advance;                      /* in 1/64 px (host layout only) */
} dmx_glyph_rec;
typedef struct dmx_glyph_atlas {
  const unsigned char* pool;
  long long pool_bytes;
  const dmx_glyph_rec* glyphs_host;
  const dmx_glyph_rec* glyphs_device;
  int n_glyphs;
} dmx_glyph_atlas;
typedef struct dmx_glyph_placement {
  int glyph, x, y;
} dmx_glyph_placement;
typedef struct dmx_glyph_text_item {
  unsigned long long dst;
  long long stride_y, stride_x, stride_c;
  int first, count;
  int H, W;
  int h_off, h_taps, v_off, v_taps;
} dmx_glyph_text_item;
int dmx_glyph_render(const dmx_glyph_atlas* atlas, const dmx_glyph_text_item* items_host, const dmx_glyph_text_item* items_device,
                     const dmx_glyph_placement* placements_host, const dmx_glyph_placement* placements_device, int n_placements, int B,
                     dmx_stream_t stream);
int dmx_glyph_text_pixel_values(const dmx_glyph_atlas* atlas, const dmx_glyph_text_item* items_host,
                                const dmx_glyph_text_item* items_device, const dmx_glyph_placement* placements_host,
                                const dmx_glyph_placement* placements_device, int n_placements, int B, const int* tables,
                                long long table_ints, const float* norm, int max_taps, int S_h, int S_w, float* out_pixel_values,
                                unsigned char* out_resized, dmx_stream_t stream);

/* Synthetic document pages (page_compose.hip): P ragged pages of coloured text lines on a textured background in ONE launch - training
 * pages whose strings and boxes are known.  Atlas and placements as for glyph_render, placements in PAGE coordinates.  Per page pixel
 * (y, x) and channel c, integer arithmetic only:
 *   background  v = clip8(bg[c] + off), off = (int)(h % (2 * tex_amp + 1)) - tex_amp (0 when tex_amp is 0) with the 32-bit hash, all
 *           arithmetic modulo 2^32,
 *               h = tex_seed + 0x9E3779B1 * y + 0x85EBCA77 * x + 0xC2B2AE3D * c
 *               h ^= h >> 16;  h *= 0x7FEB352D;  h ^= h >> 15;  h *= 0x846CA68B;  h ^= h >> 16
 *   lines   for the page's lines [first_line, first_line + n_lines) of the line table IN TABLE ORDER: m = the coverage of the line's
 *           placements [first, first + count) composed in order as in glyph_render, m = s + round(m * (255 - s) / 255); then
 *               v = round((v * (255 - m) + rgb[c] * m) / 255),   round(t / 255) = ((u >> 8) + u) >> 8 with u = t + 128
 *           - one rounding of the sum: Pillow's masked fill (ImageDraw.text(xy, text, font=font, fill=rgb) on an RGB image, BASIC
 *           layout), bit for bit.  A later line is drawn over an earlier one; the maximum over lines, or one coverage for all of
 *           them, differs where lines overlap.
 *   store   byte (y, x, c) of page p goes to dst + y * stride_y + x * stride_x + c * stride_c (bytes; trusted, as in glyph_render):
 *           HWC and planar destinations both work.
 *   pages   P of them, 1 <= P <= 65535, host copy and device copy; 1 <= H <= 65535, 1 <= W <= DMX_GLYPH_TEXT_MAX_COORD, bg in 0 .. 255,
 *           0 <= tex_amp <= 255.  n_lines may be 0.
 *   lines   n_lines_total of them, host and device copies (both may be NULL when there is none).  [x0, x1) x [y0, y1) is a box that
 *           holds every bitmap of the line; it is used for rejection only: a block of DMX_GLYPH_TEXT_BLOCK pixels of one row skips a
 *           line whose box misses it, then a glyph whose bitmap misses it.  rgb in 0 .. 255.
 * Refused (DMX_ERR_ARG, nothing launched): a null table or destination, P out of range, a line range past the line table, a placement
 * range past the placement table, a bitmap of a line outside the line's box, a value out of the ranges above, and what glyph_render
 * refuses of the atlas and the placements.  The kernel clamps what it reads from the device copies (line range, placement range, glyph
 * index, bitmap offset, colours, tex_amp): a device table that differs from its host copy gives wrong pixels, no access outside the
 * tables and the pool. */
typedef struct dmx_page_rec {
  unsigned long long dst;
  long long stride_y, stride_x, stride_c;
  int H, W;
  int first_line, n_lines;
  unsigned int tex_seed;
  int tex_amp;
  int bg[3];
  int reserved;
} dmx_page_rec;
typedef struct dmx_page_line {
  int first, count;                 /* the line's placements */
  int x0, y0, x1, y1;               /* box of the line's bitmaps, upper corner exclusive */
  int rgb[3];
  int reserved;
} dmx_page_line;
int dmx_page_compose(const dmx_glyph_atlas* atlas, const dmx_page_rec* pages_host, const dmx_page_rec* pages_device, int P,
                     const dmx_page_line* lines_host, const dmx_page_line* lines_device, int n_lines_total,
                     const dmx_glyph_placement* placements_host, const dmx_glyph_placement* placements_device, int n_placements,
                     dmx_stream_t stream);

/* Verified edits: K candidates per text box, read back by the OCR model, the best one pasted (reference sketch of the read-back:
 * app.ipynb:842-846 - crop inf_res[y1:y2, x1:x2], run the processor, call generate).  Two launches, no page copy, no host sync.
 *   readback_pixel_values: image_vae fp32 [B][K][3][S][S]; row (b, k) uses item b.  out_pixel_values fp32 [B*K][3][S_h][S_w]: row
 *           (b, k) is, bit for bit, glyph_resize_normalize applied to the slice [y1:y2, x1:x2] of the page postprocess_paste writes
 *           for image_vae[b][k] ALONE over original_hwc (one paste onto the ORIGINAL image, not chained with other boxes): a source
 *           byte inside the item's clipped crop extent is the pasted byte of that candidate, any other the original byte (a box
 *           wider than its crop keeps original pixels there).  Neither the page nor the slice is materialised.
 *           tables / norm / max_taps / out_resized as for glyph_resize_normalize; table_ints = the length of `tables`.  passes: per
 *           item the offsets and tap counts of its two pass tables (source size = the box, x2 - x1 by y2 - y1); a pass whose sizes
 *           are equal must carry an offset < 0.  Host and device copies of items and passes, as for the batch entries above.
 *           Refused (DMX_ERR_ARG, nothing launched): an empty box (x2 <= x1 or y2 <= y1), a box outside the image, K < 1 or
 *           K > DMX_SELECT_MAX_CANDIDATES, max_taps > DMX_GLYPH_MAX_TAPS, a table that ends past table_ints.  The kernel clamps
 *           whatever it reads from the device tables to the image.
 *   postprocess_paste_select: image_vae as above, scores fp32 [B][K] ON THE DEVICE.  choice int32 [B] (device, out):
 *           choice[b] = arg-max over k of scores[b][k], the lowest k on a tie; a NaN never wins; 0 if every score of the box is NaN;
 *           -1 if the best score is below `threshold` (pass -INFINITY for none; NaN is refused) - that item is skipped and its box
 *           keeps the original pixels.  out_hwc = postprocess_paste_batch of the chosen rows over the items that were not skipped
 *           (a later item wins where boxes overlap); union_mask (may be NULL) covers the inclusive boxes of ALL items. */
#define DMX_SELECT_MAX_CANDIDATES 16
typedef struct dmx_readback_pass {
  int h_off, h_taps, v_off, v_taps;
} dmx_readback_pass;
int dmx_readback_pixel_values(const float* image_vae, int S, const unsigned char* original_hwc, int H, int W,
                              const dmx_edit_item* items_host, const dmx_edit_item* items_device, int B, int K, const int* tables,
                              long long table_ints, const float* norm, const dmx_readback_pass* passes_host,
                              const dmx_readback_pass* passes_device, int max_taps, int S_h, int S_w, float* out_pixel_values,
                              unsigned char* out_resized, dmx_stream_t stream);
int dmx_postprocess_paste_select(const float* image_vae, int S, const float* scores, float threshold, const unsigned char* original_hwc,
                                 unsigned char* out_hwc, unsigned char* union_mask, int* choice, int H, int W,
                                 const dmx_edit_item* items_host, const dmx_edit_item* items_device, int B, int K, dmx_stream_t stream);

/* The four entries above for boxes on SEVERAL pages (images of different sizes) in one launch each: B items on P pages,
 * 1 <= P <= DMX_EDIT_MAX_ITEMS, 1 <= B <= DMX_EDIT_MAX_ITEMS in all, every page with at least one item.  A table of dmx_edit_page
 * travels like the item table, as a host copy the entry checks and a device copy the kernel reads.  The caller fills the addresses,
 * H, W and the item range of every page - the ranges tile [0, B) in page order - and box, origin and crop_scale of every item, lets
 * edit_pages_prepare validate both tables and fill the derived fields (every item with the arithmetic of edit_items_prepare at ITS
 * page's size, the item's page index in `reserved`, every page's first block in the paste grid), and copies both to the device in
 * stream order.  A bad page is reported by page index, a bad item by its index in the whole table; nothing is launched then.
 *   preprocess_crop_pages / readback_pixel_values_pages: row b (rows (b, k)) is what the one-page entry writes for item b on its own
 *           page.  They read `original` only.
 *   postprocess_paste_pages / postprocess_paste_select_pages: page p's `out` (and `union_mask`, 0 = none) is what the one-page entry
 *           writes for the items of page p alone; `out` must not be `original`.  choice is [B], scores [B][K], over all items.  One
 *           launch covers the pixels of all pages, so H <= 65535 holds per page, not for the sum; W <= DMX_EDIT_PAGE_MAX_W, and the
 *           pages together may take up to 2^31 - 1 blocks of 256 pixels.
 * The kernels clamp what they read from the device tables (page index, item range, origins, extents, boxes) to the page; the
 * pages' addresses and sizes are trusted. */
#define DMX_EDIT_PAGE_MAX_W 0x7fffff00            /* 2^31 - 256: ceil(W / 256) is computed in int */
typedef struct dmx_edit_page {
  unsigned long long original;      /* device address of the page, uint8 [H][W][3] */
  unsigned long long out;           /* device address of the pasted page (the paste entries) */
  unsigned long long union_mask;    /* device address of uint8 [H][W], or 0 (the paste entries) */
  int H, W;
  int item_lo, item_hi;             /* the page's items: [item_lo, item_hi) of the item table */
  int block_lo, blocks;             /* derived: the page's blocks in the paste grid, H * ceil(W / 256) of them */
} dmx_edit_page;
int dmx_edit_pages_prepare(dmx_edit_page* pages, int P, dmx_edit_item* items, int B, int S);
int dmx_preprocess_crop_pages(const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P, const dmx_edit_item* items_host,
                              const dmx_edit_item* items_device, int B, int S, float* out_image, float* out_masked_image,
                              unsigned char* out_mask, float* out_mask_latent, dmx_stream_t stream);
int dmx_postprocess_paste_pages(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                const dmx_edit_item* items_host, const dmx_edit_item* items_device, int B, dmx_stream_t stream);
int dmx_readback_pixel_values_pages(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                    const dmx_edit_item* items_host, const dmx_edit_item* items_device, int B, int K, const int* tables,
                                    long long table_ints, const float* norm, const dmx_readback_pass* passes_host,
                                    const dmx_readback_pass* passes_device, int max_taps, int S_h, int S_w, float* out_pixel_values,
                                    unsigned char* out_resized, dmx_stream_t stream);
int dmx_postprocess_paste_select_pages(const float* image_vae, int S, const float* scores, float threshold, int* choice,
                                       const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                       const dmx_edit_item* items_host, const dmx_edit_item* items_device, int B, int K, dmx_stream_t stream);

/* Seam-free paste (prepost_blend.hip): the pastes above with a feathered edge and a colour match of the generated patch against its
 * surroundings, in integers throughout.  For item b with box (x1, y1, x2, y2) and clipped crop extent E = [xs, xs+cw) x [ys, ys+ch),
 * G(x, y, c) is the byte the plain paste would write at page pixel (x, y) - defined on all of E, not only inside the box.
 *   paste rectangle  R = [x1-grow, x2+grow) x [y1-grow, y2+grow) intersected with E; an empty R pastes nothing.
 *   colour statistics (match_color): over the ring Q = ([x1-grow-ring, x2+grow+ring) x [y1-grow-ring, y2+grow+ring) in E) \ R of the
 *           ORIGINAL page and the item's own decoder row, never of another item's paste: n = |Q| and per channel
 *           D_c = sum over Q of (original - G), clamped to [-max_shift * n, max_shift * n].  Integer sums: any order is exact.
 *   corrected byte   g1 = clamp(floor((2 (G n + D_c) + n) / (2 n)), 0, 255) when match_color and n > 0, else G (floor division; this is
 *           G + floor((2 D_c + n) / (2 n)), one constant per item and channel: a mean shift, no gain).
 *   weight           F = feather + 1, d = the pixel's distance to the nearest edge of R (0 on the edge), a = min(d + 1, F).
 *   blend            cur' = floor((2 (a g1 + (F - a) cur) + F) / (2 F)).
 * A page pixel starts as the original byte and is updated by every item whose R covers it, in ascending index order; an item with
 * choice[b] < 0 updates nothing.  feather = grow = 0 without match_color is the plain paste, bit for bit.  With grow >= feather the whole
 * box is fully generated and the ramp lies in the ring around it; with grow = 0 the ramp lies inside the box.
 *   paste_color_stats[_pages]: image_vae fp32 [B*K][3][S][S]; choice int32 [B] on the device or NULL (then K must be 1): item b reads
 *           row b * K + choice[b], choice[b] < 0 = skipped.  stats (device, out) [B][4] = n, D_r, D_g, D_b, clamped; a skipped item
 *           writes zeros.  One block per item: an item's numbers do not depend on the rest of the table.
 *   postprocess_paste_blend[_pages]: the arguments of postprocess_paste_batch / _pages, then blend, stats (what paste_color_stats wrote;
 *           NULL without match_color), choice and K as above.  union_mask: 1 where the R of any item (skipped ones included) covers
 *           the pixel, and out == original wherever it is 0.
 *   select_choices: choice[b] by the rule of postprocess_paste_select from scores fp32 [B][K] on the device, as a launch of its own
 *           (one block), so choose -> stats -> paste runs without the host reading a score.
 * Refused (DMX_ERR_ARG, nothing launched): feather, grow < 0 or > DMX_PASTE_BLEND_MAX, ring < 1 or > DMX_PASTE_BLEND_MAX, max_shift
 * outside 0 .. 255, match_color without stats, K outside 1 .. DMX_SELECT_MAX_CANDIDATES, K > 1 without choice, and whatever the plain
 * entries refuse.  The kernels clamp what they read from the device tables exactly as the plain pastes do; a stale choice or stats
 * table changes bytes inside the paste rectangles, never an address. */
#define DMX_PASTE_BLEND_MAX 1048576
typedef struct dmx_paste_blend {
  int feather, grow, ring, max_shift, match_color;
} dmx_paste_blend;
int dmx_paste_color_stats(const float* image_vae, int S, const unsigned char* original_hwc, int H, int W, const dmx_edit_item* items_host,
                          const dmx_edit_item* items_device, int B, const dmx_paste_blend* blend, const int* choice, int K, long long* stats,
                          dmx_stream_t stream);
int dmx_paste_color_stats_pages(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                const dmx_edit_item* items_host, const dmx_edit_item* items_device, int B, const dmx_paste_blend* blend,
                                const int* choice, int K, long long* stats, dmx_stream_t stream);
int dmx_postprocess_paste_blend(const float* image_vae, int S, const unsigned char* original_hwc, unsigned char* out_hwc,
                                unsigned char* union_mask, int H, int W, const dmx_edit_item* items_host, const dmx_edit_item* items_device,
                                int B, const dmx_paste_blend* blend, const long long* stats, const int* choice, int K, dmx_stream_t stream);
int dmx_postprocess_paste_blend_pages(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                      const dmx_edit_item* items_host, const dmx_edit_item* items_device, int B, const dmx_paste_blend* blend,
                                      const long long* stats, const int* choice, int K, dmx_stream_t stream);
int dmx_select_choices(const float* scores, int B, int K, float threshold, int* choice, dmx_stream_t stream);

/* Skewed and rotated text: QUADRILATERAL regions with ORIENTED crops (prepost_quad.hip; the arithmetic is stated in csrc/prepost_quad.h).
 * An item is a dmx_edit_quad: the four corners of a text line as an OCR record gives them (top-left, top-right, bottom-right,
 * bottom-left as read; clockwise with y down) and a frame - a square crop of side crop_scale, centred at (cx2 / 2, cy2 / 2) in
 * pixel-index space, whose x axis runs along (ux, uy).  The mask is the quad itself (edges included), the network sees the crop with
 * the baseline horizontal, and the paste maps every page pixel inside the quad back through the inverse of the frame.  The same
 * predicate decides mask and paste (the reference pastes the half-open slice of the box; a quad has none).  Paged form only: the pages
 * travel as a dmx_edit_page table exactly as for the *_pages entries (one page is P = 1), here with W <= 65535 as well.  The caller
 * fills the pages' addresses, sizes and item ranges and every quad's corners, frame and page index, lets edit_quads_prepare validate
 * both tables and fill the derived fields (host-only: callable without a GPU), and copies both to the device in stream order.
 *   edit_quads_prepare refuses, by page or item index: a quad that is not convex, not clockwise or has no area; a corner outside
 *           its page; (ux, uy) = (0, 0) or a component beyond +-131070; a centre outside the page; crop_scale outside 1 .. 65535; a page
 *           index that is not the page whose range holds the item; B or P outside 1 .. DMX_EDIT_MAX_ITEMS; item ranges that do not tile
 *           [0, B); S outside 1 .. 65535.
 *   preprocess_quads: the four outputs of preprocess_crop_pages, row b from quad b's frame (S a multiple of 8).
 *   postprocess_paste_quads: page p's `out` (and `union_mask`, 0 = none; 1 where any quad of the page covers the pixel) from image_vae
 *           fp32 [B][3][S][S]; where quads overlap the later item decides; every other pixel is copied; `out` must not be `original`.
 *   rectify_quads: quad b as an upright strip uint8 [rh][rw][3] at out + rect_off of its table entry (the strips are packed in item
 *           order; out_bytes >= the last strip's end).  It reads neither the frames nor S.
 * Each entry is one launch; each checks the host tables again (a bad page or item is named by index and nothing is launched), the kernels
 * read the device copies and clamp what comes from them: taps to the page, page index and item range to the tables, strip writes to
 * out_bytes. */
typedef struct dmx_edit_quad {
  int x[4], y[4];                   /* corners: TL, TR, BR, BL */
  int cx2, cy2;                     /* frame centre in half-pixels of pixel-index space */
  int crop_scale;                   /* frame side in page pixels */
  int ux, uy;                       /* baseline direction */
  int page;                         /* index of the quad's page */
  int fwd[4], inv[4];               /* derived: a b c d (crop -> page) and ia ib ic id (page -> crop), Q15 */
  int ex[4], ey[4];                 /* derived: edge k runs from corner k to corner k + 1 */
  int bx1, by1, bx2, by2;           /* derived: bounding box, both corners included */
  int rect[4];                      /* derived: ra rb rc rd, Q15, scale 1 along u */
  int sx4, sy4;                     /* derived: corner sums = the centre in quarter-pixels */
  int rw, rh;                       /* derived: size of the rectified strip */
  int rect_block_lo, rect_blocks;   /* derived: the strip's blocks in the rectify grid, rh * ceil(rw / 256) of them */
  long long rect_off;               /* derived: byte offset of the strip in the rectify output */
} dmx_edit_quad;
int dmx_edit_quads_prepare(dmx_edit_page* pages, int P, dmx_edit_quad* quads, int B, int S);
int dmx_preprocess_quads(const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P, const dmx_edit_quad* quads_host,
                         const dmx_edit_quad* quads_device, int B, int S, float* out_image, float* out_masked_image, unsigned char* out_mask,
                         float* out_mask_latent, dmx_stream_t stream);
int dmx_postprocess_paste_quads(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                const dmx_edit_quad* quads_host, const dmx_edit_quad* quads_device, int B, dmx_stream_t stream);
int dmx_rectify_quads(const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P, const dmx_edit_quad* quads_host,
                      const dmx_edit_quad* quads_device, int B, unsigned char* out, long long out_bytes, dmx_stream_t stream);

/* Text in PERSPECTIVE: a projective frame beside the similarity frame of the quad entries (prepost_quad.hip; the arithmetic is stated in
 * csrc/prepost_persp.h).  A trapezoid - a line on a phone photo, a sign - is no rotated rectangle: through one rotation and one scale the
 * network sees keystoned text.  Here the homography that takes the quad to its upright rw x rh strip drives the crop (a square window
 * of side crop_scale STRIP pixels, centred at (ci2 / 2, cj2 / 2) in the strip's pixel-index space, extrapolated by the homography), the
 * paste (through its inverse) and the rectified strip.  A table of dmx_quad_persp runs parallel to the dmx_edit_quad table, index for
 * index; dmx_edit_quad keeps its layout, and its similarity frame is not read (any frame edit_quads_prepare accepts will do).  The
 * caller prepares pages and quads with edit_quads_prepare, fills ci2, cj2, crop_scale of every item and lets edit_quads_persp_prepare
 * (host-only) fill the three integer maps; S = 0 fills the strip maps alone, which is all rectify_quads_persp reads.
 *   edit_quads_persp_prepare refuses, by item index, on top of what edit_quads_prepare refuses about pages and quads (tables it did not
 *           prepare included): rw or rh below 2; an item without a frame (crop_scale 0) or with crop_scale beyond 65535 or a centre beyond
 *           +-2^20; a crop window or a strip on which the homography's denominator D is not positive at all four corners (the horizon
 *           crosses it) or on which max D > 4 * min D (the stated cap); a page -> crop denominator that is not positive at the quad's
 *           corners; any map whose numerators or denominators leave the 64-bit budget of csrc/prepost_persp.h, or whose exact host
 *           arithmetic leaves 126 bits.
 *   preprocess_quads_persp / postprocess_paste_quads_persp / rectify_quads_persp: what the quad entries of the same name write, with
 *           the projective coordinates; mask, blacking-out, taps, rounding and the paste rule are theirs.  The window's centre is not
 *           moved to keep the window on the page: clamped taps replicate the border.
 * Each entry is one launch; each checks the host tables again (a bad page or item is named by index and nothing is launched); the
 * kernels clamp what they read from the device tables exactly as the quad entries do, and paste nothing where a denominator read
 * from the device table is not positive. */
typedef struct dmx_persp_map {
  long long c16[2];                 /* the Q16 image of the grid's centre */
  long long t[9];                   /* numerators' (t0..t5) and denominator's (t6..t8, t8 = 2^43) coefficients about that centre */
} dmx_persp_map;
typedef struct dmx_quad_persp {
  int ci2, cj2;                     /* the window's centre in half-pixels of the strip's pixel-index space */
  int crop_scale;                   /* the window's side in strip pixels */
  int cx2, cy2;                     /* derived: the page-side centre in half-pixels, the origin of the paste map's grid */
  int reserved;
  dmx_persp_map crop, paste, strip; /* derived: crop grid -> page, page -> crop, strip grid -> page */
} dmx_quad_persp;
int dmx_edit_quads_persp_prepare(const dmx_edit_page* pages, int P, const dmx_edit_quad* quads, dmx_quad_persp* persp, int B, int S);
int dmx_preprocess_quads_persp(const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P, const dmx_edit_quad* quads_host,
                               const dmx_edit_quad* quads_device, const dmx_quad_persp* persp_host, const dmx_quad_persp* persp_device, int B,
                               int S, float* out_image, float* out_masked_image, unsigned char* out_mask, float* out_mask_latent,
                               dmx_stream_t stream);
int dmx_postprocess_paste_quads_persp(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                      const dmx_edit_quad* quads_host, const dmx_edit_quad* quads_device, const dmx_quad_persp* persp_host,
                                      const dmx_quad_persp* persp_device, int B, dmx_stream_t stream);
int dmx_rectify_quads_persp(const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P, const dmx_edit_quad* quads_host,
                            const dmx_edit_quad* quads_device, const dmx_quad_persp* persp_host, const dmx_quad_persp* persp_device, int B,
                            unsigned char* out, long long out_bytes, dmx_stream_t stream);

/* Verified edits for quads (prepost_quad.hip): the read-back and the select-paste of the box entries above, through a quad's frame; each
 * is written once and instantiated for the similarity and the projective frame (the _persp entries take the projective table as the
 * quad entries of that name do).  Two launches, no page copy, no strip in memory, no host sync.
 *   readback_pixel_values_quads[_persp]: image_vae fp32 [B][K][3][S][S]; out_pixel_values fp32 [B*K][3][S_h][S_w] (and out_resized uint8,
 *           optional).  Row (b, k) is, bit for bit, the end of this chain: postprocess_paste_quads[_persp] pastes image_vae[b][k] ALONE over
 *           the original page - a one-quad table that holds quad b and its frame, so other quads of the page play no part -,
 *           rectify_quads[_persp] takes quad b's strip from that page, glyph_resize_normalize resamples the strip.  Per pixel: source byte
 *           (i, j, c) of the rw x rh strip is the rectify's single-rounding bilinear of four page taps at the frame's strip coordinates of
 *           (2i + 1 - rw, 2j + 1 - rh); a tap at page pixel (X, Y), taken after the clamp to the page, is the paste's byte of the
 *           candidate's row at the crop coordinates (U16, V16) of (X, Y) when (X, Y) is inside quad b (edges included), the frame's paste
 *           map is defined there and -2^15 <= U16, V16 < (S << 16) - 2^15; otherwise it is the original page byte.  tables / table_ints /
 *           norm / passes / max_taps as for readback_pixel_values_pages, the source size of item b being (rw, rh) of the prepared quad.
 *   postprocess_paste_select_quads[_persp]: scores fp32 [B][K] ON THE DEVICE, choice int32 [B] (device, out) by the rule of
 *           postprocess_paste_select.  The paste is postprocess_paste_quads[_persp] with item b reading row b * K + choice[b]; an item with
 *           choice[b] < 0 is TRANSPARENT: the last-to-first scan of the page's quads passes over it, so an earlier chosen quad under it
 *           still shows, and where no chosen quad covers the pixel the original byte stays.  The union mask is 1 where any quad covers
 *           the pixel, skipped ones included.  With K = 1 and threshold = -INFINITY pages and union masks equal
 *           postprocess_paste_quads[_persp] bit for bit.
 * Refused (DMX_ERR_ARG, nothing launched, a bad page or item named by index): what the quad entries refuse of their tables (the _persp
 * entries re-check the prepared projective table), K outside 1 .. DMX_SELECT_MAX_CANDIDATES, a NaN threshold, null arguments, and for the
 * read-back what readback_pixel_values_pages refuses of its scalars and pass tables.  The kernels trust the pages' addresses and sizes
 * and clamp everything else they read from the device tables (page index, rw / rh to at least 1, pass spans, taps): a stale table reads
 * wrong pixels, never outside a buffer; output addresses depend on the grid alone. */
int dmx_readback_pixel_values_quads(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                    const dmx_edit_quad* quads_host, const dmx_edit_quad* quads_device, int B, int K, const int* tables,
                                    long long table_ints, const float* norm, const dmx_readback_pass* passes_host,
                                    const dmx_readback_pass* passes_device, int max_taps, int S_h, int S_w, float* out_pixel_values,
                                    unsigned char* out_resized, dmx_stream_t stream);
int dmx_readback_pixel_values_quads_persp(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                          const dmx_edit_quad* quads_host, const dmx_edit_quad* quads_device, const dmx_quad_persp* persp_host,
                                          const dmx_quad_persp* persp_device, int B, int K, const int* tables, long long table_ints,
                                          const float* norm, const dmx_readback_pass* passes_host, const dmx_readback_pass* passes_device,
                                          int max_taps, int S_h, int S_w, float* out_pixel_values, unsigned char* out_resized,
                                          dmx_stream_t stream);
int dmx_postprocess_paste_select_quads(const float* image_vae, int S, const float* scores, float threshold, int* choice,
                                       const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                       const dmx_edit_quad* quads_host, const dmx_edit_quad* quads_device, int B, int K, dmx_stream_t stream);
int dmx_postprocess_paste_select_quads_persp(const float* image_vae, int S, const float* scores, float threshold, int* choice,
                                             const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                             const dmx_edit_quad* quads_host, const dmx_edit_quad* quads_device,
                                             const dmx_quad_persp* persp_host, const dmx_quad_persp* persp_device, int B, int K,
                                             dmx_stream_t stream);

/* Seam-free paste for quads (prepost_quad_blend.hip): the feathered, colour-matched paste of the box entries above, through a quad's
 * frame.  The ramp is measured PERPENDICULAR to the quad's edges, in whole steps of one pixel, in integers throughout: no floating-point
 * value decides a weight, a membership or a sum (a float estimate is corrected by exact integer comparisons).  dmx_paste_blend is
 * reused; dmx_edit_quad keeps its layout.  Item b is a quad with corners (x_k, y_k), edges (ex_k, ey_k), inclusive bounding box
 * (bx1, by1, bx2, by2) and L2_k = ex_k^2 + ey_k^2 (64 bits, computed by the kernels).  Per page pixel (X, Y):
 *   edge function    E_k of csrc/prepost_quad.h, 64 bits.
 *   edge steps       s_k = floor(E_k / sqrt(L2_k)), exactly: for E_k >= 0 the largest j >= 0 with j^2 L2_k <= E_k^2, for E_k < 0 minus the
 *           smallest j with j^2 L2_k >= E_k^2; saturated to [-M, M], M = 2 DMX_QUAD_BLEND_MAX + 2.  An edge of length 0 (a degenerate
 *           corner is accepted, its E is 0) takes part in nothing.
 *   box steps        t = min(X - bx1, bx2 - X, Y - by1, by2 - Y): negative outside the bounding box.
 *   depth            m = min(min_k s_k, t).  The plain coverage of the quad pastes is m >= 0; for an axis-aligned quad m is the box
 *           blend's distance d on the rectangle (x1, y1, x2 + 1, y2 + 1).
 *   grown coverage   C_b(g) = the page pixels with m >= -g: the quad with every edge moved out by g pixels, its mitres cut by the
 *           bounding box grown by g - a bounded region, which a block can walk.
 *   paste region     R_b = C_b(grow) intersected with on_crop_b, the predicate of the plain quad paste (the frame's paste map defined,
 *           -2^15 <= U16, V16 < (S << 16) - 2^15).  G(X, Y, c) is the byte the plain paste forms at the item's (U16, V16): defined on
 *           all of on_crop_b.
 *   colour statistics (match_color): over the ring Q_b = (C_b(grow + ring) \ C_b(grow)) intersected with on_crop_b, of the ORIGINAL
 *           page and the item's own decoder row: n = |Q_b|, D_c = sum over Q_b of (original - G) in 64-bit integers, clamped to
 *           [-max_shift n, max_shift n].
 *   corrected byte   g1 = clamp(G + floor((2 D_c + n) / (2 n)), 0, 255) when match_color and n > 0, else G (floor division).
 *   weight           F = feather + 1, d = m + grow, a = min(d + 1, F).
 *   blend            cur' = floor((2 (a g1 + (F - a) cur) + F) / (2 F)).
 * A page pixel starts as the original byte; the items of its page are scanned in ASCENDING order and every item that is not skipped
 * (choice[b] >= 0, or no choice table) and has the pixel in its R_b updates cur.  The union mask is 1 where any C_b(grow) covers the
 * pixel - skipped items and off-crop pixels count -, and out == original wherever it is 0.
 * A DEVIATION from the plain quad paste: there the LAST covering quad decides, and a pixel off THAT quad's crop is the original byte;
 * here an item whose pixel is off its crop updates nothing and an earlier item shows through.  So feather = grow = 0 without
 * match_color equals postprocess_paste_quads[_persp] bit for bit exactly when every pixel of every quad lies on that quad's crop.
 * Quarter turn: E_k, L2_k, t, U16 and V16 are unchanged when page, quads and frames are turned by 90 degrees, so statistics, pages and
 * masks of the turned input are the turned outputs, bit for bit.
 * Integer budget: H, W <= 65535, so |E_k| < 2^33 and L2_k < 2^33; M^2 < 2^23 and M^2 L2_k < 2^56; |E_k| >= 2^31 lies beyond
 * M sqrt(L2_k) < 2^28 and saturates by its sign alone; below that E_k^2 < 2^62.  Nothing needs 128 bits, and no pixel a 64-bit division:
 * a float estimate of s_k is corrected by exact comparisons, and only where the pixel is neither known to be outside (E_k below the
 * exact threshold of s_k >= -grow) nor known to be at full weight (E_k at or above that of s_k >= feather - grow); the thresholds are
 * exact integer square roots, taken once per staged item and edge.
 *   paste_color_stats_quads[_persp]: the arguments of postprocess_paste_quads[_persp], then blend, choice, K, stats as for
 *           paste_color_stats_pages: stats (device, out) [B][4] = n, D_r, D_g, D_b; a skipped item writes four zeros.  One block per
 *           item: an item's numbers are the same alone or in any batch.
 *   postprocess_paste_blend_quads[_persp]: the arguments of postprocess_paste_quads[_persp], then blend, stats (NULL without
 *           match_color), choice and K as for postprocess_paste_blend_pages.  select_choices serves unchanged.
 * Refused (DMX_ERR_ARG, nothing launched): feather or grow outside 0 .. DMX_QUAD_BLEND_MAX, ring outside 1 .. DMX_QUAD_BLEND_MAX,
 * max_shift outside 0 .. 255, match_color without stats, K outside 1 .. DMX_SELECT_MAX_CANDIDATES, K > 1 without choice, and whatever
 * the plain quad entries refuse (a bad page or item named by index).  The kernels clamp what they read from the device tables as the
 * plain pastes do; a stale table changes bytes inside grown bounding boxes, never an address. */
#define DMX_QUAD_BLEND_MAX 1024
int dmx_paste_color_stats_quads(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                const dmx_edit_quad* quads_host, const dmx_edit_quad* quads_device, int B, const dmx_paste_blend* blend,
                                const int* choice, int K, long long* stats, dmx_stream_t stream);
int dmx_paste_color_stats_quads_persp(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                      const dmx_edit_quad* quads_host, const dmx_edit_quad* quads_device, const dmx_quad_persp* persp_host,
                                      const dmx_quad_persp* persp_device, int B, const dmx_paste_blend* blend, const int* choice, int K,
                                      long long* stats, dmx_stream_t stream);
int dmx_postprocess_paste_blend_quads(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                      const dmx_edit_quad* quads_host, const dmx_edit_quad* quads_device, int B, const dmx_paste_blend* blend,
                                      const long long* stats, const int* choice, int K, dmx_stream_t stream);
int dmx_postprocess_paste_blend_quads_persp(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device,
                                            int P, const dmx_edit_quad* quads_host, const dmx_edit_quad* quads_device,
                                            const dmx_quad_persp* persp_host, const dmx_quad_persp* persp_device, int B,
                                            const dmx_paste_blend* blend, const long long* stats, const int* choice, int K,
                                            dmx_stream_t stream);

/* CURVED text: polygon regions straightened by piecewise-affine maps (prepost_curved.hip; the arithmetic is stated in
 * csrc/prepost_curved.h).  An item is a dmx_edit_curved: a polygon of 2n points, 2 <= n <= DMX_CURVED_MAX_PAIRS, in the order scene-text
 * OCR gives a curved line - the n top points left to right as read, then the n bottom points right to left; clockwise with y down.
 * Point pair k is T_k = p[k], B_k = p[2n - 1 - k]; CELL k = 0 .. M - 1, M = n - 1, is the quad T_k, T_k+1, B_k+1, B_k, and the region is the
 * union of its cells: a pixel is inside iff the quad predicate (csrc/prepost_quad.h, edges included) holds for some cell.  The same
 * predicate decides mask and paste.  The straightened strip is rw x rh with pair k at column c_k (T_k at (c_k, 0), B_k at (c_k, rh - 1));
 * every cell is cut by the diagonal T_k+1 - B_k into PIECES 2k = (T_k, T_k+1, B_k) and 2k + 1 = (T_k+1, B_k+1, B_k), and a piece is the
 * affine map that takes its strip triangle to its page triangle - continuous across every shared line, so the paste does not tear.  The
 * frame is the projective entries': a square window of side crop_scale STRIP pixels centred at (ci2 / 2, cj2 / 2) in the strip's
 * pixel-index space.  A piece holds the three maps of a dmx_quad_persp as dmx_persp_map, with t6 = t7 = 0; the table of dmx_curved_piece is
 * ordered by item, then piece: item b owns [piece_lo, piece_lo + pieces), pieces = 2M.  For n = 2 on a parallelogram every piece holds
 * the maps dmx_edit_quads_persp_prepare fills for the same quad and frame.
 *   edit_curved_prepare (host-only): validates pages, items and frames, fills the derived fields of all three tables.  S = 0 fills the
 *           strip maps alone (the frames are not looked at), which is all rectify_curved reads.  Refuses, by page or item index, naming
 *           the cell: an odd point count, or n outside 2 .. DMX_CURVED_MAX_PAIRS; a cell that
 *           is not convex, not clockwise or has no area; a point outside the page; rh < 2, rw or rh beyond 2^20; a frame without
 *           crop_scale (0) or with crop_scale beyond 65535 or a centre beyond +-2^20; a piece whose maps leave the budget of
 *           csrc/prepost_persp.h over the crop window, the strip or its cell; B or P outside 1 .. DMX_EDIT_MAX_ITEMS; more than
 *           DMX_CURVED_MAX_CELLS cells in the launch; what edit_quads_prepare refuses about the page table.
 *   preprocess_curved: the four outputs of preprocess_quads, row b from item b's window: a crop pixel takes the piece of its column band
 *           and its side of the diagonal; a page tap is blacked out (and counts in the mask) iff some cell of the item covers it.
 *   postprocess_paste_curved: the outputs of postprocess_paste_quads.  The items of a page are scanned last to first - the later item
 *           decides -, within an item the first covering cell is taken, then the piece by the sign of the diagonal's edge function
 *           (>= 0: piece 2k); the pixel is pasted iff it lies on the crop under that piece's paste map; every other pixel is copied.
 *   rectify_curved: item b's strip uint8 [rh][rw][3] at out + rect_off, packed in item order; out_bytes >= the last strip's end.
 * Each entry is one launch; each checks the host tables again (stale derived fields are refused, a bad page or item is named by index,
 * nothing is launched); the kernels clamp what they read from the device tables: taps to the page, n, page index, item, cell and piece
 * ranges to the tables, strip writes to out_bytes, and paste nothing where a map is not defined.
 * Limits: no fused read-back / select-paste and no blend for curved regions; no fan cells (a repeated point gives a piece without area: refused);
 * top and bottom carry the same number of points. */
#define DMX_CURVED_MAX_PAIRS 17
#define DMX_CURVED_MAX_CELLS 512
typedef struct dmx_edit_curved {
  int x[34], y[34];                 /* the polygon: n top points as read, then n bottom points backwards; the rest is 0 */
  int count;                        /* the number of points, 2n */
  int page;                         /* index of the item's page */
  int ci2, cj2;                     /* the window's centre in half-pixels of the strip's pixel-index space */
  int crop_scale;                   /* the window's side in strip pixels */
  int rw, rh;                       /* derived: size of the straightened strip */
  int c[17];                        /* derived: column of pair k in the strip, c[0] = 0, c[n - 1] = rw - 1; the rest is 0 */
  int bx1, by1, bx2, by2;           /* derived: bounding box of the polygon, both corners included */
  int piece_lo, pieces;             /* derived: the item's pieces in the piece table, 2 (n - 1) of them; its cells are piece_lo / 2 .. */
  int rect_block_lo, rect_blocks;   /* derived: the strip's blocks in the rectify grid, rh * ceil(rw / 256) of them */
  long long rect_off;               /* derived: byte offset of the strip in the rectify output */
} dmx_edit_curved;
typedef struct dmx_curved_piece {
  int cx2, cy2;                     /* derived: the page-side centre in half-pixels, the origin of the paste map's grid */
  dmx_persp_map crop, paste, strip; /* derived: crop grid -> page, page -> crop, strip grid -> page */
} dmx_curved_piece;
int dmx_edit_curved_prepare(dmx_edit_page* pages, int P, dmx_edit_curved* items, dmx_curved_piece* pieces, int B, int S);
int dmx_preprocess_curved(const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P, const dmx_edit_curved* items_host,
                          const dmx_edit_curved* items_device, const dmx_curved_piece* pieces_host, const dmx_curved_piece* pieces_device, int B,
                          int S, float* out_image, float* out_masked_image, unsigned char* out_mask, float* out_mask_latent,
                          dmx_stream_t stream);
int dmx_postprocess_paste_curved(const float* image_vae, int S, const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P,
                                 const dmx_edit_curved* items_host, const dmx_edit_curved* items_device, const dmx_curved_piece* pieces_host,
                                 const dmx_curved_piece* pieces_device, int B, dmx_stream_t stream);
int dmx_rectify_curved(const dmx_edit_page* pages_host, const dmx_edit_page* pages_device, int P, const dmx_edit_curved* items_host,
                       const dmx_edit_curved* items_device, const dmx_curved_piece* pieces_host, const dmx_curved_piece* pieces_device, int B,
                       unsigned char* out, long long out_bytes, dmx_stream_t stream);

/* Comparing two versions of a set of pages (metrics.hip): what the scene-text-editing literature reports on the edited box - MSE,
 * PSNR, SSIM - and what changed OUTSIDE all boxes.  P pairs of pages a / b, uint8 [H][W][3] contiguous, both of a pair H x W; B boxes
 * (page, x1, y1, x2, y2), each the slice [y1:y2, x1:x2] of its page: exclusive upper corner, non-empty, inside the page (the read-back's
 * convention).  B is not capped at DMX_EDIT_MAX_ITEMS; P >= 1; a page may have no box.  The boxes of page q are [box_lo, box_hi) of the
 * box table and the ranges tile [0, B) in page order.  The caller fills addresses, sizes and ranges of the pages and page and corners of
 * the boxes, lets metric_tables_prepare validate both tables and fill the derived fields, and copies both to the device in stream order.
 * The entries take the host tables and their device copies, as the page entries above: a bad page is reported by page index, a bad box
 * by its index in the whole table, and nothing is launched.  The kernels clamp what they read from the device tables (page index, box
 * corners, ranges) to the tables and the page; the pages' addresses and sizes are trusted.
 *   box_metrics_pages: per box and channel, sse [B][3] = the exact integer sum of (a - b)^2 over the box, and ssim [B][3] = the mean SSIM
 *           of Wang et al. 2004 with an 11-tap Gaussian window (sigma 1.5, radius 5, weights computed in double and rounded to fp32:
 *           box_metrics_weights returns them), population covariance, data range 255, K1 = 0.01, K2 = 0.03, over the (h - 10) (w - 10)
 *           window centres whose whole window lies inside the box (scikit-image's structural_similarity with gaussian_weights=True,
 *           use_sample_covariance=False on the slice).  Pixels outside the box never enter.  A box with min(h, w) < 11 gets NaN in all
 *           three channels; its sse is still written.  Blocks enumerate (box, tile): a tile is DMX_METRIC_TILE x DMX_METRIC_TILE window
 *           centres counted from the BOX's corner; the moments of a tile are taken about an integer pivot, the rounded mean of `a` over its pixels
 *           (a variance is a small difference of large numbers on a flat bright page otherwise), per window in fp32; a tile's sums and
 *           the sums over a box's tiles are fp64 in a fixed order, a second small launch combines them.  So a box's outputs are
 *           bit-equal from run to run, alone or anywhere in a batch, and in both builds of the library; overlapping boxes are independent.
 *           workspace: box_metrics_workspace_bytes of the PREPARED box table; too small is DMX_ERR_WORKSPACE.
 *   page_outside_diff: out [P][2] = per page (changed_outside, sse_outside): the number of pixels covered by NO box of that page
 *           whose three bytes are not all equal in a and b, and the exact sum of (a - b)^2 over those pixels and the three channels.
 *           A page without boxes counts all its pixels.  One launch over blocks of 256 pixels, a page's blocks taken from the table
 *           (up to 2^31 - 1 blocks in all); integer sums, so the result does not depend on any order. */
#define DMX_METRIC_TILE 16
#define DMX_METRIC_WINDOW 11
typedef struct dmx_metric_page {
  unsigned long long a, b;          /* device addresses of the two versions of the page, uint8 [H][W][3] */
  int H, W;
  int box_lo, box_hi;               /* the page's boxes: [box_lo, box_hi) of the box table; may be empty */
  int block_lo, blocks;             /* derived: the page's blocks in the outside-diff grid, H * ceil(W / 256) of them */
} dmx_metric_page;
typedef struct dmx_metric_box {
  int page, x1, y1, x2, y2;
  int tiles_x, tiles_y;             /* derived: max(1, ceil((w - 10) / TILE)), likewise in y */
  int tile_lo;                      /* derived: the box's first block in the box-metrics grid (and first record in the workspace) */
} dmx_metric_box;
int dmx_metric_tables_prepare(dmx_metric_page* pages, int P, dmx_metric_box* boxes, int B);
int dmx_box_metrics_weights(float* h_weights);
size_t dmx_box_metrics_workspace_bytes(const dmx_metric_box* boxes_host, int B);
int dmx_box_metrics_pages(const dmx_metric_page* pages_host, const dmx_metric_page* pages_device, int P, const dmx_metric_box* boxes_host,
                          const dmx_metric_box* boxes_device, int B, unsigned long long* sse, float* ssim, void* workspace,
                          size_t workspace_bytes, dmx_stream_t stream);
int dmx_page_outside_diff(const dmx_metric_page* pages_host, const dmx_metric_page* pages_device, int P, const dmx_metric_box* boxes_host,
                          const dmx_metric_box* boxes_device, int B, unsigned long long* out, dmx_stream_t stream);

/* Fused AdamW + global-norm clipping over packed fp32 arenas (torch.optim.AdamW + clip_grad_norm_,
 * train_diffute_v1.py:721-727,927-930).  masters / exp_avg / exp_avg_sq / grads: dmx_unet_grad_bytes each.  The step also
 * rewrites the weights arena (bf16 weights, fp32 vectors) in place; afterwards call dmx_unet_refresh_derived (folded
 * LayerNorm / bias copies of the inference graph) and dmx_unet_train_prepare (transposed weights).
 * scalars: device float[2] = (gradient norm before clipping, clip coefficient).
 * ema (optional, may be NULL): fp32 shadow arena of the same layout, updated in the same pass with
 * ema -= (1 - ema_decay) * (ema - p_new)  (diffusers EMAModel.step; `ema_unet.step(unet.parameters())`, :934-935). */
int dmx_unet_optim_chunks(const dmx_unet* u);
size_t dmx_unet_optim_table_bytes(const dmx_unet* u);
size_t dmx_unet_optim_elements(const dmx_unet* u);
int dmx_unet_optim_table(const dmx_unet* u, void* table_dev, size_t bytes, dmx_stream_t stream);
int dmx_unet_master_import(const dmx_unet* u, void* masters, const char* name, const float* src, dmx_stream_t stream);
int dmx_unet_adamw_step(dmx_unet* u, const void* table_dev, int nchunks, void* masters, void* exp_avg, void* exp_avg_sq, const void* grads,
                        float lr, float beta1, float beta2, float eps, float weight_decay, int step, float max_grad_norm,
                        float* scalars, void* workspace, size_t workspace_bytes, void* ema, float ema_decay, dmx_stream_t stream);
/* The same step on a LOSS-SCALED gradient (accelerate's `--mixed_precision fp16`, train_diffute_v1.py:267,583,925: GradScaler.scale(loss)
 * .backward(), then unscale_ -> clip_grad_norm_ -> step inside accelerator.clip_grad_norm_ / optimizer.step()): grads holds g * S and
 * grad_inv_scale = 1 / S.  Norm, clipping and the update use the unscaled gradient; scalars is device float[3] = (norm of the unscaled
 * gradient, factor applied to the arena's values, found_inf): when the gradient holds an inf or NaN, found_inf = 1 and the step changes
 * NOTHING (masters, moments, EMA shadow, weights arena) - the caller then must not count it (GradScaler.step / update). */
int dmx_unet_adamw_step_scaled(dmx_unet* u, const void* table_dev, int nchunks, void* masters, void* exp_avg, void* exp_avg_sq, const void* grads,
                               float lr, float beta1, float beta2, float eps, float weight_decay, int step, float max_grad_norm,
                               float* scalars, void* workspace, size_t workspace_bytes, void* ema, float ema_decay, float grad_inv_scale,
                               dmx_stream_t stream);
int dmx_unet_refresh_derived(dmx_unet* u, dmx_stream_t stream);

/* LoRA: low-rank adapters on the UNet's linear weights, MERGED into the weights arena (diffute_amd/lora.py; peft / diffusers
 * `unet.add_adapter`).  The arena holds W' = W0 + sum_j s_j B_j A_j, so every forward and backward graph runs unchanged, and the adapter
 * gradients are linear images of the dW the backward leaves in the gradient arena: dA_j = s_j B_j^T dW, dB_j = s_j dW A_j^T.
 * One dmx_lora_rec per (target linear, active adapter); all matrices fp32, row-major, dense: A [r][K] and B [N][r] (peft's lora_A.weight /
 * lora_B.weight), s = weight * alpha / r.  The calls take the records on the HOST and upload them into `table`, the caller's device buffer
 * of at least n_records * sizeof(dmx_lora_rec) bytes, on `stream`; at most 65535 records per call.
 *   dmx_lora_merge  W = the target's base weight W0 [N][K] (torch layout), dst = where W' [N][K] goes.  The records of one target are
 *                   contiguous and are summed in table order; the first carries count = their number, the others count = 0, and all repeat
 *                   N, K, W and dst.  W'[n][k] = fma(s_J, dot_J, ... fma(s_1, dot_1, W0[n][k])), dot_j = the fma chain over p = 0 .. r-1 from 0:
 *                   one thread per element, so the bits depend on nothing but the target's own records.  One launch.
 *   dmx_lora_grads  W = dW [N][K] (torch layout, e.g. from dmx_unet_grad_export), dst = dA [r][K], dst2 = dB [N][r]; count is ignored.
 *                   dA[p][k] = s * (((q0 + q1) + q2) + q3), q_i the fma chain over the i-th quarter (ceil(N / 4) rows) of n ascending;
 *                   dB[n][p] = s * the sum over k: per lane l of 64 the fma chain over k = l, l + 64, ..., then a fixed halving tree.  Plain
 *                   IEEE arithmetic: an inf / NaN in dW comes through in every dA column and dB row it takes part in.  One launch.
 *   dmx_unet_lora_apply  merges, packs every target's merged weight into the weights arena by the pack path of dmx_unet_load_param (a
 *                   target with nrec = 0 is packed from its base weight w0: the adapter is removed) and calls dmx_unet_refresh_derived.
 *                   Targets are linear weights (parameter names as in dmx_unet_param_info), in the order of their records. */
typedef struct dmx_lora_rec {
  const float* A; const float* B;
  const float* W;
  float* dst; float* dst2;
  int N, K, r;
  float s;
  int count;
  int reserved;
} dmx_lora_rec;
typedef struct dmx_lora_target {
  const char* name;
  const float* w0;
  int rec0, nrec;
} dmx_lora_target;
int dmx_lora_merge(const dmx_lora_rec* h_recs, int n_records, void* table, size_t table_bytes, dmx_stream_t stream);
int dmx_lora_grads(const dmx_lora_rec* h_recs, int n_records, void* table, size_t table_bytes, dmx_stream_t stream);
int dmx_unet_lora_apply(dmx_unet* u, const dmx_lora_target* h_targets, int n_targets, const dmx_lora_rec* h_recs, int n_records,
                        void* table, size_t table_bytes, dmx_stream_t stream);

/* Multi-tensor EMA update / cast-copy (diffusers EMAModel as the reference drives it: `ema_unet.step(unet.parameters())`,
 * train_diffute_v1.py:934-935; copy_to / store / restore; diffute_amd.EMAModel).  One launch per call whatever the number of
 * tensors: `table` is a DEVICE array of `nchunks` entries, each a contiguous run of `count` elements; the host splits large
 * tensors into several entries so the grid fills the GPU.  dst and src runs must not overlap each other or any other entry's dst.
 * Entries whose two pointers are both 16-byte aligned use 4-element vector accesses (16 bytes for fp32), others a scalar path.
 *   dmx_ema_step_multi  mode DMX_MULTI_EMA:  dst -= one_minus_decay * (dst - src), i.e. diffusers' `s.sub_(omd * (s - p))` with
 *                       torch's type promotion: d = s - p and m = omd * d are each rounded to T (the dtype of dst when src has
 *                       the same dtype, else fp32), then s - m is rounded to dst's dtype; every op is one fp32 _rn op,
 *                       16-bit roundings are RNE.  one_minus_decay is the fp32 rounding of the host's double `1 - decay` (what
 *                       torch does with a Python scalar), so the result is bit-identical to torch's.
 *                       mode DMX_MULTI_COPY: dst = cast(src) (`s.copy_(p)`, parameters with requires_grad=False).
 *   dmx_copy_multi      every entry: dst = cast(src) (the mode field is ignored).
 * dtypes: DMX_DT_F32, DMX_DT_BF16, DMX_DT_F16 for either side, in both builds of the library. */
#define DMX_DT_F32 0
#define DMX_DT_BF16 1
#define DMX_DT_F16 2
#define DMX_MULTI_EMA 0
#define DMX_MULTI_COPY 1
typedef struct dmx_multi_chunk {
  void* dst;                   /* first element of the run (shadow / destination) */
  const void* src;             /* first element of the run (parameter / source) */
  unsigned int count;          /* elements */
  unsigned char dst_dtype, src_dtype, mode, reserved;
} dmx_multi_chunk;             /* 24 bytes */
int dmx_ema_step_multi(const void* table, int nchunks, float one_minus_decay, dmx_stream_t stream);
int dmx_copy_multi(const void* table, int nchunks, dmx_stream_t stream);
size_t dmx_mse_loss_workspace_bytes(void);
int dmx_mse_loss(const float* pred, const float* target, size_t n, float* loss, float* dpred, float grad_scale,
                 void* workspace, size_t workspace_bytes, dmx_stream_t stream);
/* The weighted objective of the denoiser in one entry (csrc/loss.hip): Min-SNR-gamma sample weights (Hang et al., ICCV 2023; diffusers'
 * --snr_gamma), an emphasis on the text box, the epsilon / v target, dLoss/dpred and per-sample sums, from what the training step holds.
 * No target and no weight tensor is materialised.  pred, latents (x0), noise, dpred: fp32 [B][C][hw]; mask: fp32 [B][1][hw] at latent
 * resolution (1 inside the box) or NULL; timesteps: int64 [B]; sa = sqrt(abar), sb = sqrt(1 - abar), wt = the per-timestep sample weight:
 * T floats each.  For sample b with t = timesteps[b], every line one rounded fp32 operation, in this order:
 *     tau   = noise                                     (v_prediction 0)
 *     tau   = fsub(fmul(sa[t], noise), fmul(sb[t], x0)) (v_prediction 1: the bits dmx_sched_get_velocity writes)
 *     d     = fsub(pred, tau)          q = fmul(d, d)
 *     m     = fadd(1, fmul(mask_weight, M))             (M = mask[b][0][pixel], the same for every channel; M = 0 when mask is NULL)
 *     e     = fmul(wt[t], m)
 *     dpred = fmul(fmul(d, e), gs)                      gs = (float)(2 * grad_scale / N) in double on the host, N = B*C*hw
 * records: fp32 [B][DMX_LOSS_ROW_FLOATS], the sums of sample b over its C*hw elements (mask_sum: over its hw pixels) and its weight:
 *     SQ_ALL = sum q     SQ_MASK = sum fmul(M, q)     SQ_WEIGHTED = sum fmul(m, q)     MASK_SUM = sum M     WEIGHT = wt[t]
 * loss (fp32 [1]): acc = 0; for b = 0 .. B-1: acc = fadd(acc, fmul(WEIGHT[b], SQ_WEIGHTED[b])); loss = fmul(acc, (float)(1.0 / N)).
 * That is (1/N) sum_b w_b sum m (pred - tau)^2: diffusers' Min-SNR loss at mask_weight 0, the plain MSE when wt is all ones as well.  The
 * emphasis is NOT renormalised by sum m: mask_weight changes the scale of the loss.
 * Two launches (per-block partial sums; one block that folds them), no float atomics, no block waits for another.  A sample is cut into
 * chunks of DMX_LOSS_CHUNK elements, one block each, so which block and which thread adds an element depends on C*hw alone, never on B or
 * on b: a sample's record and dpred row are the same bits alone or as any row of any batch, and from run to run.  16-byte accesses where a
 * sample's first element is 16-byte aligned in every tensor (scalar otherwise and for the last, partial quad; the order of the additions
 * is the same either way).  Reduction shape: 8 serial adds per thread, an 8-level tree over the 256 threads of a block, then the
 * ceil(C*hw / DMX_LOSS_CHUNK) chunk sums serially: a term passes through at most k = 16 + ceil(C*hw / DMX_LOSS_CHUNK) additions.
 * A timestep outside [0, T) reads the tables at the clamped index and gives that sample WEIGHT = NaN, hence NaN dpred rows and a NaN
 * loss; the other samples' records and dpred rows are what they are in a clean batch.  dpred == NULL: loss and records only.
 * mask_weight must be finite and >= 0.  Everything is fp32: both builds of the library compute the same bits. */
#define DMX_LOSS_ROW_FLOATS 5
#define DMX_LOSS_SQ_ALL 0
#define DMX_LOSS_SQ_MASK 1
#define DMX_LOSS_SQ_WEIGHTED 2
#define DMX_LOSS_MASK_SUM 3
#define DMX_LOSS_WEIGHT 4
#define DMX_LOSS_CHUNK 2048
size_t dmx_diffusion_loss_workspace_bytes(int B, int C, int hw);
int dmx_diffusion_loss(const float* pred, const float* latents, const float* noise, const float* mask, const int64_t* timesteps,
                       const float* sa, const float* sb, const float* wt, int B, int C, int hw, int T, int v_prediction,
                       float mask_weight, float grad_scale, float* loss, float* records, float* dpred,
                       void* workspace, size_t workspace_bytes, dmx_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Glyph encoder: the ViT encoder of TrOCR, `trocr_model(pixel_values).last_hidden_state`
 * (app.ipynb:773-776, train_diffute_v1.py:868-871).  Same handle protocol as the UNet / VAE: create, enumerate the
 * parameters (transformers ViTModel state-dict keys), bind an arena, load fp32 tensors, finalize, forward.
 * ---------------------------------------------------------------------------------- */
typedef struct dmx_vit dmx_vit;
typedef struct dmx_vit_config {
  int image_size, patch_size, num_channels;     /* 384, 16, 3 */
  int hidden_size, num_layers, num_heads;       /* 1024, 24, 16 (head dim must be 64) */
  int intermediate_size;                        /* 4096 */
  int qkv_bias;                                 /* 0 for TrOCR (BEiT-style), 1 for plain ViT checkpoints */
  float layer_norm_eps;                         /* 1e-12 */
} dmx_vit_config;
dmx_vit* dmx_vit_create(const dmx_vit_config* cfg);
void dmx_vit_destroy(dmx_vit* v);
int dmx_vit_param_count(const dmx_vit* v);
int dmx_vit_param_info(const dmx_vit* v, int index, const char** name, int shape[4]);
size_t dmx_vit_arena_bytes(const dmx_vit* v);
int dmx_vit_bind_arena(dmx_vit* v, void* arena, size_t bytes);
int dmx_vit_load_param(dmx_vit* v, const char* name, const float* src_f32, dmx_stream_t stream);
int dmx_vit_finalize(dmx_vit* v, dmx_stream_t stream);
size_t dmx_vit_workspace_bytes(dmx_vit* v, int B);
int dmx_vit_forward(dmx_vit* v, const float* pixel_values, float* last_hidden_state, int B,
                    void* workspace, size_t workspace_bytes, dmx_stream_t stream);
/* fp32 VALIDATION instantiation (tests only): the same walker on fp32 activations, the fp32 master copy of the parameters
 * (`masters`: dmx_vit_master_bytes(v) bytes, zero-filled, then dmx_vit_master_import for every parameter) and the plain fp32
 * kernels - compared with transformers' ViTModel output (tests/golden/vit_transformers.npz) at north_star's 1e-3. */
size_t dmx_vit_master_bytes(const dmx_vit* v);
int dmx_vit_master_import(const dmx_vit* v, void* masters, const char* name, const float* src, dmx_stream_t stream);
size_t dmx_vit_workspace_bytes_f32(dmx_vit* v, int B);
int dmx_vit_forward_f32(dmx_vit* v, const void* masters, const float* pixel_values, float* last_hidden_state, int B,
                        void* workspace, size_t workspace_bytes, dmx_stream_t stream);

/* ------------------------------------------------------------------------------------
 * OCR read-back (app.ipynb:548/845): the text decoder of TrOCR - transformers' TrOCRForCausalLM, the `.decoder` of
 * `full_trocr_model = VisionEncoderDecoderModel.from_pretrained(...)` (app.ipynb:548) that `full_trocr_model_te.generate(
 * pixel_values)` (app.ipynb:845) runs greedily.  Same handle protocol as the ViT: create, enumerate the parameters (transformers
 * state-dict keys), bind an arena, load fp32 tensors, finalize.  The caller owns the arena, the cache and the workspace.
 * Generation: dmx_trocr_dec_cross_kv (once per image batch), dmx_trocr_dec_reset, then dmx_trocr_dec_step per token.  A step
 * reads the input token and the position from the cache's state words and advances them on the device, so one captured graph
 * of dmx_trocr_dec_step replays every step.
 * ---------------------------------------------------------------------------------- */
typedef struct dmx_trocr_dec dmx_trocr_dec;
typedef struct dmx_trocr_dec_config {           /* app.ipynb:548 (trocr-large: TrOCRConfig defaults) */
  int vocab_size, d_model, num_layers, num_heads; /* 50265, 1024, 12, 16 (head dim 64; d_model a multiple of 256, <= 1024) */
  int ffn_dim, max_position_embeddings;          /* 4096, 512 (learned positions: table of max + 2 rows) */
  int cross_hidden_size;                         /* k/v input width of the cross-attention (0: d_model) */
  int activation;                                /* 0 exact-erf gelu, 1 relu */
  int scale_embedding, layernorm_embedding, tie_word_embeddings;
} dmx_trocr_dec_config;
/* state words (int32) at the start of the cache: position of the current input token, all-rows-finished flag, the sequence
 * length at which every row had finished, the next input token of each row (B <= 64), the finished flag of each row */
#define DMX_TROCR_STATE_POS 0
#define DMX_TROCR_STATE_DONE 1
#define DMX_TROCR_STATE_STOP_LEN 2
#define DMX_TROCR_STATE_TOKENS 16
#define DMX_TROCR_STATE_FINISHED 80
dmx_trocr_dec* dmx_trocr_dec_create(const dmx_trocr_dec_config* cfg);                       /* app.ipynb:548 */
void dmx_trocr_dec_destroy(dmx_trocr_dec* d);                                               /* app.ipynb:548 */
int dmx_trocr_dec_param_count(const dmx_trocr_dec* d);                                      /* app.ipynb:548 */
int dmx_trocr_dec_param_info(const dmx_trocr_dec* d, int index, const char** name, int shape[4]);   /* app.ipynb:548 */
size_t dmx_trocr_dec_arena_bytes(const dmx_trocr_dec* d);                                   /* app.ipynb:548 */
int dmx_trocr_dec_bind_arena(dmx_trocr_dec* d, void* arena, size_t bytes);                  /* app.ipynb:548 */
int dmx_trocr_dec_load_param(dmx_trocr_dec* d, const char* name, const float* src_f32, dmx_stream_t stream);   /* app.ipynb:548 */
int dmx_trocr_dec_finalize(dmx_trocr_dec* d, dmx_stream_t stream);                          /* app.ipynb:548 */
/* cache: state words + self-attention K/V [layers][B][max_len][2 d_model] + cross K/V [B][S][layers][2 d_model] (bf16);
 * workspace: the activations of one step, or of the cross K/V GEMM (app.ipynb:845) */
size_t dmx_trocr_dec_cache_bytes(const dmx_trocr_dec* d, int B, int S, int max_len);        /* app.ipynb:845 */
size_t dmx_trocr_dec_workspace_bytes(const dmx_trocr_dec* d, int B, int S, int max_len);    /* app.ipynb:845 */
/* the k_proj | v_proj of every layer over the encoder states [B][S][cross_hidden_size] fp32: one GEMM (app.ipynb:845) */
int dmx_trocr_dec_cross_kv(dmx_trocr_dec* d, const float* encoder_hidden_states, int B, int S, int max_len, void* cache,
                           void* workspace, size_t workspace_bytes, dmx_stream_t stream);
/* position 0, no row finished, every row's input = start_token, ids[b][0] = start_token (ids: [B][max_len] int64) (app.ipynb:845) */
int dmx_trocr_dec_reset(dmx_trocr_dec* d, void* cache, int B, int S, int max_len, int start_token, long long* ids, dmx_stream_t stream);
/* teacher forcing: the next step's input tokens from tokens[B] (int64) (app.ipynb:845 restated as a forward) */
int dmx_trocr_dec_set_tokens(dmx_trocr_dec* d, void* cache, const long long* tokens, int B, dmx_stream_t stream);
/* one greedy step (app.ipynb:845): logits of the input tokens at the current position, argmax (lowest index on ties), a finished
 * row emits pad_token_id, a row that emits eos_token_id (< 0: none) finishes; the token goes to ids[b][pos + 1] and becomes the
 * next input; the position advances.  logits (nullable): fp32 [B][ld_logits] */
int dmx_trocr_dec_step(dmx_trocr_dec* d, void* cache, int B, int S, int max_len, int eos_token_id, int pad_token_id,
                       long long* ids, float* logits, int ld_logits, void* workspace, size_t workspace_bytes, dmx_stream_t stream);
int dmx_trocr_dec_launches_per_step(const dmx_trocr_dec* d);                                /* app.ipynb:845 */
/* op entry points of the decoder kernels (tests, benchmarks; app.ipynb:845): y = x W^T on M <= 64 rows with one epilogue
 * (0: y = act(xW^T + bias) * oscale -> yf fp32 and / or yb; 1: q|k|v - q * oscale -> yf, k|v -> kv row state[0];
 * 2: LayerNorm(xW^T + bias + res) -> yf, yb; 3: logits -> yf (nullable) + the greedy pick into state / ids);
 * kchunk > 0 forces the K split.  x, w, yb, kv: 16-bit elements. */
size_t dmx_trocr_dec_linear_workspace_bytes(int M, int N, int K);
int dmx_trocr_dec_linear(int epi, int act, const void* x, int M, int K, const void* w, int N, const float* bias, float oscale,
                         float* yf, int ld_yf, void* yb, const float* res, const float* gamma, const float* beta,
                         void* kv, int max_len, int* state, long long* ids, int eos, int pad, int kchunk,
                         void* workspace, size_t workspace_bytes, dmx_stream_t stream);
/* decode attention, one query row per (b, head), d = 64: q [M][H*64] fp32 (pre-scaled), key j of row b at kv + b*bstride + j*rstride
 * + h*64, its value d_model = H*64 elements further; out [M][H*64] (app.ipynb:845) */
size_t dmx_trocr_dec_attn_workspace_bytes(int M, int H, int L);
int dmx_trocr_dec_attn(const float* q, int M, int H, const void* kv, long long bstride, int rstride, int L, void* out,
                       void* workspace, size_t workspace_bytes, dmx_stream_t stream);

/* Beam search over the same decoder (transformers' GenerationMixin._beam_search with do_sample=False, no logits processors, one
 * eos id; app.ipynb:845 with a checkpoint's own num_beams / length_penalty / early_stopping).  Rows = B items x num_beams (<= 64,
 * 2 <= num_beams <= 16).  cache: state words | self K/V of every row | cross K/V of every ITEM | beam state block.  The self
 * K/V is never reordered: row r writes the K/V of its input token at the current position, and an ancestry table uint8
 * [2][64][max_len] (two halves, used by the parity of the position) names the physical row that holds position j of each beam.
 * A step = the greedy step's launches with an LM head that writes fp32 logits and log-sum-exp partials, plus ONE selection
 * launch (top 2 num_beams per item, running / finished bookkeeping, the loop condition into DMX_TROCR_STATE_DONE / _STOP_LEN).
 * Beam state block, int32 / fp32 words from dmx_trocr_dec_beam_state_offset: */
#define DMX_TROCR_BEAM_RUN_SCORE 0     /* fp32 [64] running score of each row */
#define DMX_TROCR_BEAM_FIN_SCORE 64    /* fp32 [64] finished slots: score, */
#define DMX_TROCR_BEAM_FIN_FLAG 128    /* finished flag, */
#define DMX_TROCR_BEAM_FIN_LEN 192     /* generated length */
#define DMX_TROCR_BEAM_IMPROVABLE 256  /* per item: the running beams can still improve on the finished ones */
#define DMX_TROCR_BEAM_PARENT 320      /* per row: the row it continued in the last step */
#define DMX_TROCR_BEAM_STEPS 580       /* selection launches since the reset */
#define DMX_TROCR_BEAM_WORDS 640       /* then: token history int32 [max_len][64], finished ids int32 [64][max_len], the table */
size_t dmx_trocr_dec_beam_cache_bytes(const dmx_trocr_dec* d, int B, int num_beams, int S, int max_len);       /* app.ipynb:845 */
size_t dmx_trocr_dec_beam_workspace_bytes(const dmx_trocr_dec* d, int B, int num_beams, int S, int max_len);   /* app.ipynb:845 */
size_t dmx_trocr_dec_beam_state_offset(const dmx_trocr_dec* d, int B, int num_beams, int S, int max_len);      /* app.ipynb:845 */
size_t dmx_trocr_dec_beam_state_bytes(int max_len);
int dmx_trocr_dec_beam_launches_per_step(const dmx_trocr_dec* d);                              /* app.ipynb:845 */
/* cross K/V of the B items (one GEMM at B * S rows) and the reset: position 0, running scores [0, -1e9, ...] (app.ipynb:845) */
int dmx_trocr_dec_beam_begin(dmx_trocr_dec* d, const float* encoder_hidden_states, int B, int num_beams, int S, int max_len, int start_token,
                             void* cache, void* workspace, size_t workspace_bytes, dmx_stream_t stream);
/* one beam step (app.ipynb:845); eos_token_id < 0: none; early_stopping 0 False, 1 True, 2 "never"; logp (nullable): fp32
 * [B * num_beams][vocab], the log-probs the selection used.  After DMX_TROCR_STATE_DONE is set a step changes nothing */
int dmx_trocr_dec_beam_step(dmx_trocr_dec* d, void* cache, int B, int num_beams, int S, int max_len, int eos_token_id, float length_penalty,
                            int early_stopping, float* logp, void* workspace, size_t workspace_bytes, dmx_stream_t stream);
/* the first num_return finished slots of every item: sequences int64 [B * num_return][max_len] (pad beyond the hypothesis),
 * scores fp32 and generated lengths int32 [B * num_return] (app.ipynb:845) */
int dmx_trocr_dec_beam_finalize(dmx_trocr_dec* d, void* cache, int B, int num_beams, int S, int max_len, int num_return, int pad_token_id,
                                long long* sequences, float* scores, int* lengths, dmx_stream_t stream);
/* op entry points (tests): one selection step on supplied fp32 logits [B * num_beams][V] through the step's launch function
 * (state: 256 state words, beam_state: dmx_trocr_dec_beam_state_bytes(max_len) bytes, both set up when reset != 0); the
 * decode attention with the ancestry table (nullable, uint8 [M][ld_table]: key j < L - 1 of row b from row table[b][j], key
 * L - 1 from row b) and rows_per_item > 0 rows sharing one item's K/V */
size_t dmx_trocr_dec_beam_select_workspace_bytes(int B, int num_beams, int V);
int dmx_trocr_dec_beam_select(const float* logits, int B, int num_beams, int V, int max_len, int eos_token_id, float length_penalty,
                              int early_stopping, int reset, int start_token, int* state, void* beam_state, float* logp,
                              void* workspace, size_t workspace_bytes, dmx_stream_t stream);
int dmx_trocr_dec_beam_attn(const float* q, int M, int H, const void* kv, long long bstride, int rstride, int L, const void* table,
                            int ld_table, int rows_per_item, void* out, void* workspace, size_t workspace_bytes, dmx_stream_t stream);

/* Teacher-forced scoring of known target ids (transformers' `VisionEncoderDecoderModel(pixel_values=..., labels=...)` over the
 * model of app.ipynb:548): all B * T rows go through every layer at once (prefill), and the LM head keeps per (row, vocabulary
 * tile) only the running (max, sum exp), the best (value, lowest index) and the label's logit, so the [B*T][V] logits exist in
 * memory only when the caller asks for them.  1 <= B <= 64, 1 <= T <= max_position_embeddings, B * T <= 4096.
 *   labels            int64 [B][T]; the decoder input at position 0 is start_token, at position t labels[t - 1] with
 *                     ignore_index replaced by pad_token (transformers' shift_tokens_right).  Nullable with decoder_input_ids.
 *   decoder_input_ids int64 [B][T] or null: the decoder inputs as they are (no shift)
 *   token_logprob     fp32 [B][T]: logit[label] - log-sum-exp, 0 where the label is ignore_index (required with labels)
 *   argmax            int32 [B][T], nullable: the teacher-forced arg-max (lowest index among equal maxima)
 *   logits            fp32 [B*T][ld_logits], nullable */
size_t dmx_trocr_dec_prefill_workspace_bytes(const dmx_trocr_dec* d, int B, int S, int T);     /* app.ipynb:845 */
int dmx_trocr_dec_score(dmx_trocr_dec* d, const float* encoder_hidden_states, int B, int S, const long long* labels,
                        const long long* decoder_input_ids, int T, int start_token, int pad_token, int ignore_index,
                        float* token_logprob, int* argmax, float* logits, int ld_logits,
                        void* workspace, size_t workspace_bytes, dmx_stream_t stream);          /* app.ipynb:845 */
/* op entry points of the prefill kernels (tests; app.ipynb:845).  Embedding of a [B][T] block with the label shift:
 * LN(embed_tokens[id] * scale + embed_positions[t + 2]) (no LayerNorm without gamma) -> xf fp32 and xb 16-bit, both [B*T][D] */
int dmx_trocr_dec_prefill_embed(const long long* labels, const long long* decoder_input_ids, int B, int T, int start_token, int pad_token,
                                int ignore_index, const void* embed_tokens, int V, const float* embed_positions, int num_positions,
                                float scale, const float* gamma, const float* beta, int D, float* xf, void* xb, dmx_stream_t stream);
/* causal self-attention, d = 64, Sq = Sk = T <= 512: row (b * T + t), head h at column h * 64 of q / k / v / out (16-bit
 * elements, any column slices of one fused buffer); out = softmax(scale * q k^T, keys <= t) v */
int dmx_trocr_dec_prefill_attn(const void* q, int ldq, const void* k, int ldk, const void* v, int ldv, void* out, int ldo,
                               int B, int H, int T, float scale, dmx_stream_t stream);
/* fused LM head + loss: x [M][K] and w [V][K] 16-bit (K % 128 == 0), labels int64 [M] or null -> token_logprob, argmax, logits
 * as in dmx_trocr_dec_score */
size_t dmx_trocr_dec_prefill_lm_loss_workspace_bytes(int M, int V);
int dmx_trocr_dec_prefill_lm_loss(const void* x, int M, int K, const void* w, int V, const long long* labels, int ignore_index,
                                  float* token_logprob, int* argmax, float* logits, int ld_logits,
                                  void* workspace, size_t workspace_bytes, dmx_stream_t stream);

typedef struct dmx_vae_config {
  int in_channels, out_channels, latent_channels;
  int block_out_channels[4];
  int layers_per_block;
  int norm_num_groups;
} dmx_vae_config;

/* AutoencoderKL (from_pretrained: train_diffute_v1.py:632, app.ipynb:550, train_vae.py:516) */
dmx_vae* dmx_vae_create(const dmx_vae_config* cfg);
void dmx_vae_destroy(dmx_vae* v);
int dmx_vae_param_count(const dmx_vae* v);
int dmx_vae_param_info(const dmx_vae* v, int index, const char** name, int shape[4]);
size_t dmx_vae_arena_bytes(const dmx_vae* v);
int dmx_vae_bind_arena(dmx_vae* v, void* arena, size_t bytes);
int dmx_vae_load_param(dmx_vae* v, const char* name, const float* src_f32, dmx_stream_t stream);
int dmx_vae_finalize(dmx_vae* v, dmx_stream_t stream);
size_t dmx_vae_workspace_bytes(dmx_vae* v, int B, int H, int W, int decode);
/* vae.encode(x) -> moments NCHW fp32 [B][2*latent][H/8][W/8]  (app.ipynb:781,793) */
int dmx_vae_encode(dmx_vae* v, const float* x, float* moments, int B, int H, int W,
                   void* workspace, size_t workspace_bytes, dmx_stream_t stream);
/* vae.decode(z).sample: z NCHW fp32 [B][latent][h][w] -> image [B][3][8h][8w]  (app.ipynb:819) */
/* fp32 VALIDATION instantiation of the two graphs above (tests only; north_star's "within 1e-3 rel fp32" at model level for
 * app.ipynb:793,819): fp32 activations, the fp32 master copy of the parameters (`masters`: dmx_vae_grad_bytes(v) bytes,
 * filled by dmx_vae_master_import for every parameter) and the plain fp32 kernels.  The mid-block attention keeps the
 * scores of 16 queries in LDS: images up to ~384 px. */
int dmx_vae_master_import(const dmx_vae* v, void* masters, const char* name, const float* src, dmx_stream_t stream);
size_t dmx_vae_workspace_bytes_f32(dmx_vae* v, int B, int H, int W, int decode);
int dmx_vae_encode_f32(dmx_vae* v, const void* masters, const float* x, float* moments, int B, int H, int W,
                       void* workspace, size_t workspace_bytes, dmx_stream_t stream);
int dmx_vae_decode_f32(dmx_vae* v, const void* masters, const float* z, float* image, int B, int h, int w,
                       void* workspace, size_t workspace_bytes, dmx_stream_t stream);
int dmx_vae_decode(dmx_vae* v, const float* z, float* image, int B, int h, int w,
                   void* workspace, size_t workspace_bytes, dmx_stream_t stream);

/* ------------------------------------------------------------------------------------
 * Measurement aid (bench.py roofline leg): while enabled, every executor launch is bracketed
 * by hipEvents on its own stream.  dmx_profile_end synchronises and fills, per kernel class
 * (0 conv/linear GEMM, 1 attention, 2 GroupNorm, 3 LayerNorm, 4 other), four doubles:
 * launches, total milliseconds, algorithmic FLOPs, algorithmic bytes.
 * ---------------------------------------------------------------------------------- */
int dmx_profile_begin(void);
int dmx_profile_end(double* h_out, int n_out);
/* optional: write one CSV row per launch (class, ms, flops, bytes, shape tag) at the next dmx_profile_end */
int dmx_profile_dump_path(const char* h_path);
size_t dmx_profile_symbols(char* buf, size_t cap);   /* per kernel SYMBOL of the region dmx_profile_end closed last: lines "class\tlaunches\tms\tflops\tbytes\tsymbol" (rocprofv3's spelling of the name); returns bytes written, 0 = buffer too small */

#ifdef __cplusplus
}
#endif
#endif /* DIFFUTE_HIP_H */
